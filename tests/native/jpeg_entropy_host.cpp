// Host driver of ops/csrc/jpeg_entropy_dec.h, the routine jpeg_entropy_decode_kernel runs per lane
// (tests/test_jpeg_entropy_native.py builds it plain and with ASan + UBSan on the host).
//
//   jpeg_entropy_host <cases.bin> <out.bin>
//
// cases.bin: "JED1", uint32 count, then per case uint32 nb, mcus, per (MCUs per interval), nint,
// nbytes, mutate; uint32 tables[JPEG_DEC_WORDS]; uint32 intervals[nint][2] (offset, length);
// nbytes bytes.  out.bin: per case uint32 status (0, or the code of the lowest failing interval),
// uint32 that interval, int16 coef[mcus * nb * 64].
//
// Every interval is decoded from a heap copy of exactly its length and into a coefficient buffer
// of exactly the case's size, so a read or a store one element outside either is a sanitizer
// report.  Then the mutation pass: for every case marked `mutate`, single-bit flips and
// truncations chosen by a fixed-seed generator (at most 2000 runs in all); each run has to end
// with some status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy_dec.h"

namespace {

struct Case {
  uint32_t nb, mcus, per, nint, nbytes, mutate;
  std::vector<uint32_t> tables, intervals;
  std::vector<uint8_t> bytes;
};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// decodes every interval; returns the status of the lowest failing one (and which)
int decode_case(const Case& c, const std::vector<uint8_t>& bytes, const std::vector<uint32_t>& ivals, int16_t* coef,
                uint32_t* where) {
  int first = JPEG_DEC_OK;
  *where = 0;
  for (uint32_t it = 0; it < c.nint; ++it) {
    const uint32_t off = ivals[2 * it], len = ivals[2 * it + 1];
    int st;
    const uint32_t m0 = it * c.per;
    if (m0 >= c.mcus) {
      st = JPEG_DEC_OVERRUN;
    } else if (off > bytes.size() || len > bytes.size() - off) {
      st = JPEG_DEC_TRUNCATED;
    } else {
      uint8_t* own = static_cast<uint8_t*>(malloc(len ? len : 1));      // exactly the interval
      if (len) memcpy(own, bytes.data() + off, len);
      const uint32_t left = c.mcus - m0;
      st = jpeg_decode_interval(own, len, c.tables.data(), (int)c.nb, (int)(left < c.per ? left : c.per),
                                coef + (size_t)m0 * c.nb * 64);
      free(own);
    }
    if (st != JPEG_DEC_OK && first == JPEG_DEC_OK) {
      first = st;
      *where = it;
    }
  }
  return first;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  char magic[4];
  uint32_t count = 0;
  if (!rd(f, magic, 4) || memcmp(magic, "JED1", 4) != 0 || !rd(f, &count, 4)) return 2;
  std::vector<Case> cases(count);
  for (Case& c : cases) {
    uint32_t h[6];
    if (!rd(f, h, sizeof h)) return 2;
    c.nb = h[0]; c.mcus = h[1]; c.per = h[2]; c.nint = h[3]; c.nbytes = h[4]; c.mutate = h[5];
    if ((c.nb != 3 && c.nb != 6) || c.per == 0 || c.mcus == 0 || c.mcus > (1u << 20) || c.nint > (1u << 20)) return 2;
    c.tables.resize(JPEG_DEC_WORDS);
    c.intervals.resize(2 * (size_t)c.nint);
    c.bytes.resize(c.nbytes);
    if (!rd(f, c.tables.data(), 4 * c.tables.size()) || !rd(f, c.intervals.data(), 4 * c.intervals.size()) ||
        !rd(f, c.bytes.data(), c.nbytes))
      return 2;
  }
  fclose(f);

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (const Case& c : cases) {
    const size_t n = (size_t)c.mcus * c.nb * 64;
    int16_t* coef = static_cast<int16_t*>(calloc(n, sizeof(int16_t)));
    uint32_t where = 0;
    const uint32_t st = (uint32_t)decode_case(c, c.bytes, c.intervals, coef, &where);
    fwrite(&st, 4, 1, o);
    fwrite(&where, 4, 1, o);
    fwrite(coef, sizeof(int16_t), n, o);
    free(coef);
  }
  fclose(o);

  // mutation pass
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  auto next = [&seed]() {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(seed >> 33);
  };
  size_t targets = 0;
  for (const Case& c : cases) targets += c.mutate && c.nbytes > 0;
  const int per_case = targets ? (int)(2000 / targets) : 0;
  long runs = 0, hist[5] = {0, 0, 0, 0, 0};
  for (const Case& c : cases) {
    if (!c.mutate || c.nbytes == 0) continue;
    const size_t n = (size_t)c.mcus * c.nb * 64;
    for (int k = 0; k < per_case; ++k) {
      std::vector<uint8_t> bytes = c.bytes;
      std::vector<uint32_t> ivals = c.intervals;
      if (k % 4 == 3) {                        // truncation of one interval
        const uint32_t it = next() % c.nint;
        if (ivals[2 * it + 1] > 0) ivals[2 * it + 1] = next() % ivals[2 * it + 1];
      } else {                                 // one flipped bit
        bytes[next() % c.nbytes] ^= (uint8_t)(1u << (next() & 7));
      }
      int16_t* coef = static_cast<int16_t*>(calloc(n, sizeof(int16_t)));
      uint32_t where = 0;
      const int st = decode_case(c, bytes, ivals, coef, &where);
      free(coef);
      if (st < 0 || st > 4) {
        printf("mutation %ld: status %d out of range\n", runs, st);
        return 1;
      }
      ++hist[st];
      ++runs;
    }
  }
  printf("cases %u mutations %ld ok %ld truncated %ld bad_code %ld overrun %ld wide %ld\n", count, runs, hist[0],
         hist[1], hist[2], hist[3], hist[4]);
  return 0;
}
