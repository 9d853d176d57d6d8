// Host driver for ops/csrc/philox_normal.h (tests/test_sampler_noise_native.py): one request per
// line of the file it is given, one line of output each.
//   N seed step pixel            -> the four Philox words (hex) and the four normals of the noise
//                                   contract (seed: signed 64-bit decimal)
//   K c0 c1 c2 c3 k0 k1  (hex)   -> the raw Philox4x32-10 words of a counter and key
//   B w0 w1              (hex)   -> the Box-Muller pair of two words
#include <inttypes.h>
#include <stdio.h>

#include "philox_normal.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (f == nullptr) return 2;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'K') {
      uint32_t c[4], k[2];
      if (fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &c[0], &c[1], &c[2], &c[3],
                 &k[0], &k[1]) != 6)
        return 3;
      philox4x32_10(c, k[0], k[1]);
      printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", c[0], c[1], c[2], c[3]);
    } else if (kind == 'N') {
      int64_t seed;
      uint32_t step, pixel;
      if (fscanf(f, "%" SCNd64 " %" SCNu32 " %" SCNu32, &seed, &step, &pixel) != 3) return 3;
      const uint64_t s = (uint64_t)seed;
      uint32_t w[4];
      float z[4];
      philox_normal4((uint32_t)s, (uint32_t)(s >> 32), pixel, step, w, z);
      printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %.9g %.9g %.9g %.9g\n", w[0], w[1], w[2], w[3],
             z[0], z[1], z[2], z[3]);
    } else if (kind == 'B') {
      uint32_t w0, w1;
      if (fscanf(f, "%" SCNx32 " %" SCNx32, &w0, &w1) != 2) return 3;
      float z0, z1;
      philox_box_muller(w0, w1, &z0, &z1);
      printf("%.9g %.9g\n", z0, z1);
    } else {
      return 4;
    }
  }
  fclose(f);
  return 0;
}
