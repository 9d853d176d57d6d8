// The per-interval entropy decoder of the ENTROPY DECODE CONTRACT (jpeg.hip's header comment):
// one restart interval of a baseline JPEG scan -> its quantised zig-zag coefficients.  A plain
// function over pointers and lengths, compiled as it stands by jpeg_entropy_decode_kernel (one
// lane per interval) and by a host program (tests/native/jpeg_entropy_host.cpp, which runs it
// under host sanitizers on arbitrary bytes).  ops/jpeg_format.py builds the tables
// (decode_tables) and is the numpy reference (entropy_decode).
//
// Memory safety for any input bytes: no byte at or past bytes[len] is read, every table index is
// masked or checked against the table's size, and a coefficient is stored only at
// coef[(m * nb + blk) * 64 + k] with m < nmcu, blk < nb, k <= 63 checked before the store.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define JPEG_DEC_FN __host__ __device__ inline
#else
#define JPEG_DEC_FN inline
#endif

enum JpegDecStatus { JPEG_DEC_OK = 0, JPEG_DEC_TRUNCATED = 1, JPEG_DEC_BAD_CODE = 2, JPEG_DEC_OVERRUN = 3, JPEG_DEC_WIDE = 4 };

// per Huffman table, 32-bit words: 128 of look-ahead (256 uint16 entries (length << 8) | symbol by
// the next 8 bits, 0 = longer code), 16 limits, 16 value offsets, 64 of values (256 bytes)
constexpr int JPEG_DEC_TABLE_WORDS = 128 + 16 + 16 + 64;
// tables as the decoder receives them: quantisation tables in zig-zag order (luma, chroma), then
// the four decode tables DC luma, DC chroma, AC luma, AC chroma
constexpr int JPEG_DEC_QZ_WORDS = 128;
constexpr int JPEG_DEC_WORDS = JPEG_DEC_QZ_WORDS + 4 * JPEG_DEC_TABLE_WORDS;
constexpr int JPEG_DEC_WIDE_T = 2047;         // jpeg_format.WIDE_T

struct JpegBits {
  const uint8_t* p;
  uint32_t len, pos;     // pos <= len: the next byte to read
  uint64_t acc;          // only the low n bits are pending
  int n;
};

// up to 64 pending bits; a 0xFF not followed by 0x00 ends the data
JPEG_DEC_FN void jpeg_bits_fill(JpegBits& r) {
  // One 8-byte load instead of six dependent byte loads (a lane's time is load latency): taken
  // when 8 bytes are left inside the interval and the next 6 hold no 0xFF, i.e. nothing to unstuff.
  if (r.n <= 16 && r.len - r.pos >= 8) {
    uint64_t w;
    __builtin_memcpy(&w, r.p + r.pos, 8);                      // little-endian: byte i at bits 8 i
    const uint64_t v = ~w | 0xffff000000000000ull;             // a zero byte of v = a 0xFF among the first 6
    if (((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) == 0) {
      r.acc = (r.acc << 48) | (__builtin_bswap64(w) >> 16);
      r.n += 48;
      r.pos += 6;
      return;
    }
  }
  while (r.n <= 56 && r.pos < r.len) {
    const uint32_t b = r.p[r.pos];
    if (b == 0xffu) {
      if (r.pos + 1 < r.len && r.p[r.pos + 1] == 0) {
        r.pos += 2;
      } else {
        r.len = r.pos;
        break;
      }
    } else {
      ++r.pos;
    }
    r.acc = (r.acc << 8) | b;
    r.n += 8;
  }
}

// the next Huffman symbol of table t, or -(status)
JPEG_DEC_FN int jpeg_dec_symbol(JpegBits& r, const uint32_t* t) {
  if (r.n < 16) jpeg_bits_fill(r);
  // the next 16 bits, zero-padded past the end of the data (then n < 16 is what is left)
  const uint32_t w = (r.n >= 16 ? (uint32_t)(r.acc >> (r.n - 16)) : (uint32_t)(r.acc << (16 - r.n))) & 0xffffu;
  const uint32_t i = w >> 8;
  const uint32_t e = (t[i >> 1] >> (16 * (i & 1))) & 0xffffu;
  int l;
  uint32_t sym;
  if (e != 0) {
    l = (int)(e >> 8);
    sym = e & 0xffu;
  } else {
    l = 9;
    while (l <= 16 && w >= t[128 + l - 1]) ++l;
    if (l > 16) return r.n < 16 ? -JPEG_DEC_TRUNCATED : -JPEG_DEC_BAD_CODE;
    const uint32_t idx = t[144 + l - 1] + (w >> (16 - l));      // mod 2^32: the offset may be negative
    if (idx > 255u) return -JPEG_DEC_BAD_CODE;
    sym = (t[160 + (idx >> 2)] >> (8 * (idx & 3))) & 0xffu;
  }
  if (l > r.n) return -JPEG_DEC_TRUNCATED;
  r.n -= l;
  return (int)sym;
}

// RECEIVE + EXTEND of s bits, 1 <= s <= 16; false when the data ends first
JPEG_DEC_FN bool jpeg_dec_receive(JpegBits& r, int s, int& v) {
  if (r.n < s) {
    jpeg_bits_fill(r);
    if (r.n < s) return false;
  }
  r.n -= s;
  const uint32_t u = (uint32_t)(r.acc >> r.n) & ((1u << s) - 1u);
  v = u >= (1u << (s - 1)) ? (int)u : (int)u - (1 << s) + 1;
  return true;
}

// One restart interval: bytes[0 .. len) -> coef [nmcu][nb][64], which the caller zeroed (only
// non-zero coefficients are stored).  tabs = JPEG_DEC_WORDS words.  Returns the status; after an
// error the coefficients stored so far stay.
JPEG_DEC_FN int jpeg_decode_interval(const uint8_t* bytes, uint32_t len, const uint32_t* tabs, int nb, int nmcu,
                                     int16_t* coef) {
  JpegBits r;
  r.p = bytes; r.len = len; r.pos = 0; r.acc = 0; r.n = 0;
  constexpr uint32_t T2 = (uint32_t)JPEG_DEC_WIDE_T * JPEG_DEC_WIDE_T;
  int p0 = 0, p1 = 0, p2 = 0;
  for (int m = 0; m < nmcu; ++m) {
    for (int blk = 0; blk < nb; ++blk) {
      const int comp = blk < nb - 2 ? 0 : blk - (nb - 2) + 1;
      const uint32_t* q = tabs + (comp == 0 ? 0 : 64);
      const uint32_t* dc = tabs + JPEG_DEC_QZ_WORDS + (comp == 0 ? 0 : JPEG_DEC_TABLE_WORDS);
      const uint32_t* ac = dc + 2 * JPEG_DEC_TABLE_WORDS;
      int16_t* out = coef + ((long long)m * nb + blk) * 64;
      int s = jpeg_dec_symbol(r, dc);
      if (s < 0) return -s;
      if (s > 11) return JPEG_DEC_BAD_CODE;
      int v = 0;
      if (s != 0 && !jpeg_dec_receive(r, s, v)) return JPEG_DEC_TRUNCATED;
      // |predictor| * Q <= WIDE_T after every block that passed, |v| < 2^11: no overflow
      const int pred = (comp == 0 ? p0 : (comp == 1 ? p1 : p2)) + v;
      if (comp == 0) p0 = pred; else if (comp == 1) p1 = pred; else p2 = pred;
      int d = pred * (int)q[0];
      if (d < -JPEG_DEC_WIDE_T || d > JPEG_DEC_WIDE_T) return JPEG_DEC_WIDE;
      uint32_t energy = (uint32_t)(d * d);
      if (pred != 0) out[0] = (int16_t)pred;
      int k = 1;
      while (k < 64) {
        const int rs = jpeg_dec_symbol(r, ac);
        if (rs < 0) return -rs;
        const int run = rs >> 4;
        s = rs & 15;
        if (s == 0) {
          if (rs == 0) break;                       // EOB
          if (run != 15) return JPEG_DEC_BAD_CODE;
          k += 16;                                  // ZRL: a non-zero coefficient has to follow
          if (k > 63) return JPEG_DEC_OVERRUN;
          continue;
        }
        if (s > 10) return JPEG_DEC_BAD_CODE;
        k += run;
        if (k > 63) return JPEG_DEC_OVERRUN;
        if (!jpeg_dec_receive(r, s, v)) return JPEG_DEC_TRUNCATED;
        d = v * (int)q[k];                          // |v| < 2^10, Q <= 255
        if (d < -JPEG_DEC_WIDE_T || d > JPEG_DEC_WIDE_T) return JPEG_DEC_WIDE;
        energy += (uint32_t)(d * d);                // at most 2 T^2
        if (energy > T2) return JPEG_DEC_WIDE;
        out[k] = (int16_t)v;
        ++k;
      }
      if (energy > T2) return JPEG_DEC_WIDE;
    }
  }
  return JPEG_DEC_OK;
}
