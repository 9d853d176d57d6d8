// Host driver of ops/csrc/jpeg_huff_opt.h (the table builder of the optimised Huffman tables) and
// of the counting sink of ops/csrc/jpeg_entropy_blk.h, the text jpeg_huff_count_kernel and
// jpeg_huff_build_kernel compile (tests/test_jpeg_huffman_native.py builds it plain and with
// ASan + UBSan on the host).
//
//   jpeg_huff_opt_host <cases.bin> <out.bin>
//
// cases.bin: "JHO1", uint32 count, then per case uint32 kind.
//   kind 0 (frequencies): uint32 freq[256].
//     out: uint32 bad, uint32 nvals, uint8 bits[16], uint8 vals[nvals], uint32 words[256].
//   kind 1 (coefficients): uint32 nb, mcus, per (MCUs per interval); int16 coef[mcus * nb * 64].
//     out: uint32 freq[544] (the histogram of the counting sink), uint32 bad, uint32 length, the
//     DHT segment of the four tables built from it, uint32 words[544].
// Every buffer is a heap block of exactly the size the routine is told, so a store outside is a
// sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy_blk.h"
#include "jpeg_huff_opt.h"

namespace {

constexpr int HUFF_WORDS = 2 * 16 + 2 * 256;
constexpr int BASE[4] = {0, 16, 32, 32 + 256};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
void wr(FILE* f, const void* p, size_t n) { fwrite(p, 1, n, f); }

void table(const uint32_t* freq, int nslots, JpegHuffWork* w, uint32_t* words) {
  for (int i = 0; i < JPEG_HUFF_SYMS; ++i) w->freq[i] = i < nslots ? freq[i] : 0u;
  jpeg_huff_build(*w, 0);
  jpeg_huff_assign(*w, words, nslots, 0);
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
  if (!rd(f, magic, 4) || memcmp(magic, "JHO1", 4) != 0 || !rd(f, &count, 4)) return 2;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  uint32_t refused = 0;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t kind = 0;
    if (!rd(f, &kind, 4)) return 2;
    if (kind == 0) {
      std::vector<uint32_t> freq(256);
      if (!rd(f, freq.data(), 4 * freq.size())) return 2;
      JpegHuffWork* w = static_cast<JpegHuffWork*>(malloc(sizeof(JpegHuffWork)));
      uint32_t* words = static_cast<uint32_t*>(malloc(256 * sizeof(uint32_t)));
      table(freq.data(), 256, w, words);
      refused += w->bad;
      uint8_t bits[16];
      for (int l = 1; l <= 16; ++l) bits[l - 1] = (uint8_t)w->bits[l];
      wr(o, &w->bad, 4);
      wr(o, &w->nvals, 4);
      wr(o, bits, 16);
      wr(o, w->vals, w->nvals);
      wr(o, words, 256 * sizeof(uint32_t));
      free(words);
      free(w);
    } else if (kind == 1) {
      uint32_t h[3];
      if (!rd(f, h, sizeof h)) return 2;
      const uint32_t nb = h[0], mcus = h[1], per = h[2];
      if ((nb != 3 && nb != 6) || per == 0 || mcus == 0 || mcus > (1u << 20)) return 2;
      const size_t n = (size_t)mcus * nb * 64;
      int16_t* coef = static_cast<int16_t*>(aligned_alloc(16, n * sizeof(int16_t)));
      if (!coef || !rd(f, coef, n * sizeof(int16_t))) return 2;
      uint32_t* hist = static_cast<uint32_t*>(calloc(HUFF_WORDS, sizeof(uint32_t)));
      for (size_t g = 0; g < (size_t)mcus * nb; ++g) {
        const long long m = (long long)(g / nb);
        const int k = (int)(g % nb);
        const bool luma = k < (int)nb - 2;
        jpeg_blk_count(coef + g * 64, jpeg_blk_pred(coef, m, k, (int)nb, (int)per), hist + (luma ? 0 : 16),
                       hist + 32 + (luma ? 0 : 256));
      }
      JpegHuffWork* w = static_cast<JpegHuffWork*>(malloc(4 * sizeof(JpegHuffWork)));
      uint32_t* words = static_cast<uint32_t*>(malloc(HUFF_WORDS * sizeof(uint32_t)));
      uint32_t bad = 0;
      for (int t = 0; t < 4; ++t) {
        table(hist + BASE[t], t < 2 ? 16 : 256, w + t, words + BASE[t]);
        bad |= w[t].bad;
      }
      refused += bad;
      uint32_t len = 4;
      for (int t = 0; t < 4; ++t) len += 17u + w[t].nvals;
      uint8_t* dht = static_cast<uint8_t*>(malloc(len));
      const uint32_t got = jpeg_huff_dht(w, dht, len, 0, 1);
      if (got != len) return 3;
      wr(o, hist, HUFF_WORDS * sizeof(uint32_t));
      wr(o, &bad, 4);
      wr(o, &len, 4);
      wr(o, dht, len);
      wr(o, words, HUFF_WORDS * sizeof(uint32_t));
      free(dht);
      free(words);
      free(w);
      free(hist);
      free(coef);
    } else {
      return 2;
    }
  }
  fclose(f);
  fclose(o);
  printf("cases %u refused %u max_bits %u\n", count, refused, JPEG_BLK_MAX_BITS_OPT);
  return 0;
}
