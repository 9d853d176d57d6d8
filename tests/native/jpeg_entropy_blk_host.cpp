// Host driver of ops/csrc/jpeg_entropy_blk.h, the per-block coder and the stuffing piece the
// jpeg_blk_* kernels run per lane (tests/test_jpeg_block_native.py builds it plain and with ASan +
// UBSan on the host).
//
//   jpeg_entropy_blk_host <cases.bin> <out.bin>
//
// cases.bin: "JEB1", uint32 count, then per case uint32 nb, mcus, per (MCUs per interval), nint;
// uint32 huff[544]; int16 coef[mcus * nb * 64].  out.bin: per case uint32 length, then the scan
// bytes (RSTn markers and the EOI included).
//
// The passes of the block-parallel entropy coder run serially over the lanes: bits per block, scan
// per interval, pack, stuffed length per piece, scan, write.  Every interval's unstuffed string
// is a heap block of exactly ceil(bits / 32) words, filled with a pattern and zeroed only where
// the scan pass zeroes (the word every block starts in, the word the interval ends in), and the
// payload is a heap block of exactly the summed interval lengths; so a store one element outside
// either is a sanitizer report, and a word the pack pass merges into without its being zeroed
// shows in the bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy_blk.h"

namespace {

constexpr int HUFF_WORDS = 2 * 16 + 2 * 256;

struct Case {
  uint32_t nb, mcus, per, nint;
  std::vector<uint32_t> huff;
  int16_t* coef = nullptr;             // 16-byte aligned, exactly mcus * nb * 64 values
};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// returns false when a pass refused an index
bool encode_case(const Case& c, std::vector<uint8_t>& result) {
  const uint32_t nb = c.nb;
  const size_t nblk = (size_t)c.mcus * nb;
  uint32_t* bits = static_cast<uint32_t*>(malloc(nblk * sizeof(uint32_t)));
  const uint32_t* dcl = c.huff.data(), *dcc = dcl + 16, *acl = dcl + 32, *acc = dcl + 32 + 256;
  bool bad = false;
  // bits
  for (size_t g = 0; g < nblk; ++g) {
    const long long m = (long long)(g / nb);
    const int k = (int)(g % nb);
    const bool luma = k < (int)nb - 2;
    JpegBlkSink<false> w;
    jpeg_blk_code<false>(c.coef + g * 64, jpeg_blk_pred(c.coef, m, k, (int)nb, (int)c.per), luma ? dcl : dcc,
                         luma ? acl : acc, w);
    bits[g] = w.pos;
  }
  // scan, pack and stuffed lengths per interval
  std::vector<uint32_t*> slots(c.nint, nullptr);
  std::vector<uint32_t> nwords(c.nint, 0), ubytes(c.nint, 0), lens(c.nint, 0);
  for (uint32_t it = 0; it < c.nint; ++it) {
    const size_t m0 = (size_t)it * c.per, m1 = m0 + c.per < c.mcus ? m0 + c.per : c.mcus;
    uint32_t running = 0;
    for (size_t g = m0 * nb; g < m1 * nb; ++g) {
      const uint32_t v = bits[g];
      bits[g] = running;
      running += v;
    }
    nwords[it] = (running + 31u) / 32u;
    ubytes[it] = (running + 7u) / 8u;
    uint32_t* words = slots[it] = static_cast<uint32_t*>(malloc(nwords[it] ? nwords[it] * sizeof(uint32_t) : 1));
    memset(words, 0xAA, nwords[it] * sizeof(uint32_t));
    for (size_t g = m0 * nb; g < m1 * nb; ++g) {
      if ((bits[g] >> 5) < nwords[it]) words[bits[g] >> 5] = 0u;
      else bad = true;
    }
    if ((running >> 5) < nwords[it]) words[running >> 5] = 0u;
    for (size_t g = m0 * nb; g < m1 * nb; ++g) {
      const long long m = (long long)(g / nb);
      const int k = (int)(g % nb);
      const bool luma = k < (int)nb - 2;
      JpegBlkSink<true> w;
      w.start(words, nwords[it], bits[g]);
      jpeg_blk_code<true>(c.coef + g * 64, jpeg_blk_pred(c.coef, m, k, (int)nb, (int)c.per), luma ? dcl : dcc,
                          luma ? acl : acc, w);
      w.finish(bits[g], g + 1 == m1 * nb);
      bad |= w.bad;
    }
    uint32_t total = 0;
    for (uint32_t b0 = 0; b0 < ubytes[it]; b0 += JPEG_BLK_PIECE) {
      const uint32_t b1 = b0 + JPEG_BLK_PIECE < ubytes[it] ? b0 + JPEG_BLK_PIECE : ubytes[it];
      total += jpeg_blk_stuff<false>(words, nwords[it], b0, b1, nullptr, 0u, 0u, bad);
    }
    lens[it] = total + 2u;
  }
  // write
  uint32_t size = 0;
  for (uint32_t it = 0; it < c.nint; ++it) size += lens[it];
  uint8_t* out = static_cast<uint8_t*>(malloc(size ? size : 1));
  memset(out, 0x55, size);
  uint32_t at = 0;
  for (uint32_t it = 0; it < c.nint; ++it) {
    uint32_t running = 0;
    for (uint32_t b0 = 0; b0 < ubytes[it]; b0 += JPEG_BLK_PIECE) {
      const uint32_t b1 = b0 + JPEG_BLK_PIECE < ubytes[it] ? b0 + JPEG_BLK_PIECE : ubytes[it];
      running += jpeg_blk_stuff<true>(slots[it], nwords[it], b0, b1, out, at + running, size, bad);
    }
    if (running + 2u != lens[it] || at + running + 2u > size) {
      bad = true;
    } else {
      out[at + running] = 0xff;
      out[at + running + 1] = (uint8_t)(it + 1 < c.nint ? 0xD0u + (it & 7u) : 0xD9u);
    }
    at += lens[it];
    free(slots[it]);
  }
  result.assign(out, out + size);
  free(out);
  free(bits);
  return !bad;
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
  if (!rd(f, magic, 4) || memcmp(magic, "JEB1", 4) != 0 || !rd(f, &count, 4)) return 2;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  uint32_t refused = 0;
  for (uint32_t i = 0; i < count; ++i) {
    Case c;
    uint32_t h[4];
    if (!rd(f, h, sizeof h)) return 2;
    c.nb = h[0]; c.mcus = h[1]; c.per = h[2]; c.nint = h[3];
    if ((c.nb != 3 && c.nb != 6) || c.per == 0 || c.mcus == 0 || c.mcus > (1u << 20) ||
        c.nint != (c.mcus + c.per - 1) / c.per)
      return 2;
    c.huff.resize(HUFF_WORDS);
    const size_t n = (size_t)c.mcus * c.nb * 64;
    c.coef = static_cast<int16_t*>(aligned_alloc(16, n * sizeof(int16_t)));
    if (!c.coef || !rd(f, c.huff.data(), 4 * c.huff.size()) || !rd(f, c.coef, n * sizeof(int16_t))) return 2;
    std::vector<uint8_t> bytes;
    if (!encode_case(c, bytes)) ++refused;
    const uint32_t len = (uint32_t)bytes.size();
    fwrite(&len, 4, 1, o);
    fwrite(bytes.data(), 1, bytes.size(), o);
    free(c.coef);
  }
  fclose(f);
  fclose(o);
  printf("cases %u refused %u piece %u max_bits %u\n", count, refused, JPEG_BLK_PIECE, JPEG_BLK_MAX_BITS);
  return 0;
}
