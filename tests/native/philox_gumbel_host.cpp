// Host driver for ops/csrc/philox_gumbel.h (tests/test_lm_gumbel_native.py): one request per line
// of the file it is given, one line of output each.
//   G seed step id     -> the Philox word of the Gumbel contract (hex) and g (seed: signed 64-bit
//                         decimal)
//   W w         (hex)  -> g of one word
#include <inttypes.h>
#include <stdio.h>

#include "philox_gumbel.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (f == nullptr) return 2;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'G') {
      int64_t seed;
      uint32_t step, id;
      if (fscanf(f, "%" SCNd64 " %" SCNu32 " %" SCNu32, &seed, &step, &id) != 3) return 3;
      const uint64_t s = (uint64_t)seed;
      const uint32_t w = philox_gumbel_bits((uint32_t)s, (uint32_t)(s >> 32), id, step);
      printf("%08" PRIx32 " %.9g %.9g\n", w, philox_gumbel_word(w),
             philox_gumbel((uint32_t)s, (uint32_t)(s >> 32), id, step));
    } else if (kind == 'W') {
      uint32_t w;
      if (fscanf(f, "%" SCNx32, &w) != 1) return 3;
      printf("%.9g\n", philox_gumbel_word(w));
    } else {
      return 4;
    }
  }
  fclose(f);
  return 0;
}
