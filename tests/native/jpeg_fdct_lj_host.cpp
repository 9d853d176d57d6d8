// Host driver of ops/csrc/jpeg_fdct_lj.h (the arithmetic of the libjpeg forward contract), the
// text jpeg_transform_lj_kernel compiles, and of the per-table DHT layout of
// ops/csrc/jpeg_huff_opt.h (tests/test_jpeg_libjpeg_native.py builds it plain and with ASan +
// UBSan on the host).
//
//   jpeg_fdct_lj_host <cases.bin> <out.bin>
//
// cases.bin: "JLJ1", uint32 count, then per case uint32 H, W, s420; int32 qtab[128] (luma, chroma,
// natural order); uint8 pixels[H * W * 3].
//   out: uint32 n, int16 coef[n] (quantised zig-zag coefficients [mcus][nb][64]), uint32 length,
//   the four DHT segments (one per table) of the optimised tables of those coefficients.
// The pixels are a heap block of exactly H * W * 3 bytes, so a read outside the image is a
// sanitizer report; UBSan watches the 32-bit arithmetic.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "jpeg_entropy_blk.h"
#include "jpeg_fdct_lj.h"
#include "jpeg_huff_opt.h"

namespace {

constexpr int HUFF_WORDS = 2 * 16 + 2 * 256;
constexpr int BASE[4] = {0, 16, 32, 32 + 256};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
void wr(FILE* f, const void* p, size_t n) { fwrite(p, 1, n, f); }

// zig-zag position of every natural index: the walk along the anti-diagonals
void zigzag_positions(int* zpos) {
  int z = 0;
  for (int d = 0; d < 15; ++d)
    for (int i = 0; i <= d; ++i) {
      const int r = (d & 1) ? i : d - i, c = d - r;
      if (r < 8 && c < 8) zpos[r * 8 + c] = z++;
    }
}

// rows, columns, quantisation of one block of level-shifted samples -> zig-zag coefficients
void transform_block(int* s, const int32_t* q, const int* zpos, int16_t* out) {
  for (int r = 0; r < 8; ++r) jpeg_lj_fdct8<true>(s + r * 8);
  for (int c = 0; c < 8; ++c) {
    int v[8];
    for (int n = 0; n < 8; ++n) v[n] = s[n * 8 + c];
    jpeg_lj_fdct8<false>(v);
    for (int k = 0; k < 8; ++k) out[zpos[k * 8 + c]] = (int16_t)jpeg_lj_quant(v[k], q[k * 8 + c], k * 8 + c != 0);
  }
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
  if (!rd(f, magic, 4) || memcmp(magic, "JLJ1", 4) != 0 || !rd(f, &count, 4)) return 2;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  int zpos[64];
  zigzag_positions(zpos);
  uint32_t dummies = 0;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t h[3];
    int32_t qtab[128];
    if (!rd(f, h, sizeof h) || !rd(f, qtab, sizeof qtab)) return 2;
    const int H = (int)h[0], W = (int)h[1];
    const bool s420 = h[2] != 0;
    if (H < 1 || W < 1 || H > 4096 || W > 4096) return 2;
    uint8_t* img = static_cast<uint8_t*>(malloc((size_t)H * W * 3));
    if (!img || !rd(f, img, (size_t)H * W * 3)) return 2;
    const int mcu = s420 ? 16 : 8, nb = s420 ? 6 : 3;
    const int mx = (W + mcu - 1) / mcu, my = (H + mcu - 1) / mcu;
    const uint32_t n = (uint32_t)mx * my * nb * 64;
    int16_t* coef = static_cast<int16_t*>(aligned_alloc(16, (n * sizeof(int16_t) + 15) / 16 * 16));
    if (!coef) return 2;
    for (int mby = 0; mby < my; ++mby)
      for (int mbx = 0; mbx < mx; ++mbx) {
        int16_t* dst = coef + ((size_t)mby * mx + mbx) * nb * 64;
        int s[64];
        if (s420) {
          for (int k = 0; k < 4; ++k) {
            for (int r = 0; r < 8; ++r)
              for (int c = 0; c < 8; ++c) {
                const int y = jpeg_lj_src(mby * 16 + (k >> 1) * 8 + r, H), x = jpeg_lj_src(mbx * 16 + (k & 1) * 8 + c, W);
                s[r * 8 + c] = jpeg_lj_ycc(img + ((size_t)y * W + x) * 3).y - 128;
              }
            transform_block(s, qtab, zpos, dst + k * 64);
          }
          for (int comp = 0; comp < 2; ++comp) {
            for (int r = 0; r < 8; ++r)
              for (int c = 0; c < 8; ++c) {
                const int cx = mbx * 8 + c;
                int ys[2];
                jpeg_lj_chroma_rows(mby * 8 + r, H, ys[0], ys[1]);
                const int xs[2] = {jpeg_lj_src(2 * cx, W), jpeg_lj_src(2 * cx + 1, W)};
                int sum = 0;
                for (int d = 0; d < 4; ++d) {
                  const JpegLjYcc p = jpeg_lj_ycc(img + ((size_t)ys[d >> 1] * W + xs[d & 1]) * 3);
                  sum += comp == 0 ? p.cb : p.cr;
                }
                s[r * 8 + c] = jpeg_lj_chroma_mean(sum, cx) - 128;
              }
            transform_block(s, qtab + 64, zpos, dst + (4 + comp) * 64);
          }
          for (int k = 1; k < 4; ++k)
            if (jpeg_lj_dummy(k, mby, mbx, H, W)) {
              memset(dst + k * 64, 0, 64 * sizeof(int16_t));
              dst[k * 64] = dst[(k - 1) * 64];
              ++dummies;
            }
        } else {
          for (int comp = 0; comp < 3; ++comp) {
            for (int r = 0; r < 8; ++r)
              for (int c = 0; c < 8; ++c) {
                const int y = jpeg_lj_src(mby * 8 + r, H), x = jpeg_lj_src(mbx * 8 + c, W);
                const JpegLjYcc p = jpeg_lj_ycc(img + ((size_t)y * W + x) * 3);
                s[r * 8 + c] = (comp == 0 ? p.y : (comp == 1 ? p.cb : p.cr)) - 128;
              }
            transform_block(s, qtab + (comp == 0 ? 0 : 64), zpos, dst + comp * 64);
          }
        }
      }
    wr(o, &n, 4);
    wr(o, coef, n * sizeof(int16_t));
    // the image's optimised tables (no restart interval) as the four DHT segments of the PIL layout
    const int mcus = mx * my;
    uint32_t* hist = static_cast<uint32_t*>(calloc(HUFF_WORDS, sizeof(uint32_t)));
    for (size_t g = 0; g < (size_t)mcus * nb; ++g) {
      const int k = (int)(g % nb);
      const bool luma = k < nb - 2;
      jpeg_blk_count(coef + g * 64, jpeg_blk_pred(coef, (long long)(g / nb), k, nb, mcus), hist + (luma ? 0 : 16),
                     hist + 32 + (luma ? 0 : 256));
    }
    JpegHuffWork* w = static_cast<JpegHuffWork*>(malloc(4 * sizeof(JpegHuffWork)));
    uint32_t* words = static_cast<uint32_t*>(malloc(HUFF_WORDS * sizeof(uint32_t)));
    uint32_t len = 0;
    for (int t = 0; t < 4; ++t) {
      const int nslots = t < 2 ? 16 : 256;
      for (int j = 0; j < JPEG_HUFF_SYMS; ++j) w[t].freq[j] = j < nslots ? hist[BASE[t] + j] : 0u;
      jpeg_huff_build(w[t], 0);
      jpeg_huff_assign(w[t], words + BASE[t], nslots, 0);
      if (w[t].bad) return 3;
      len += 4u + 17u + w[t].nvals;
    }
    uint8_t* dht = static_cast<uint8_t*>(malloc(len));
    if (jpeg_huff_dht(w, dht, len, 0, 1, true) != len) return 3;
    wr(o, &len, 4);
    wr(o, dht, len);
    free(dht);
    free(words);
    free(w);
    free(hist);
    free(coef);
    free(img);
  }
  fclose(f);
  fclose(o);
  printf("cases %u dummies %u\n", count, dummies);
  return 0;
}
