// The lane run of the CHUNKED ENTROPY DECODE CONTRACT (jpeg.hip's header comment): from a start
// state (p, blk, k) a lane decodes whole symbols of one restart interval while p is before the
// end of its chunk, and either only counts (the sync rounds) or stores (the write pass).  A plain
// function over pointers and lengths, compiled as it stands by jpeg_entropy_sync_kernel (one lane
// per chunk) and by a host program (tests/native/jpeg_entropy_sync_host.cpp, which runs the whole
// chunked decode serially under host sanitizers on arbitrary bytes).  The symbol decode itself is
// jpeg_entropy_dec.h's (jpeg_dec_symbol, jpeg_dec_receive) on a bit window this file fills;
// ops/jpeg_format.py is the numpy model (entropy_decode_chunked).
//
// Raw positions.  p is a raw bit position in the interval (stuffed zeros counted), so the window
// is refilled from p for every symbol instead of being carried: either from a cached 8-byte load
// that holds no 0xFF (raw bits = data bits inside it), or byte by byte with unstuffing, after
// which p is advanced by walking the same bytes again.  p never rests inside a stuffed 0x00.
//
// Memory safety for any input bytes and any start state: no byte at or past bytes[len] is read
// (len < 2^28, so 8 * len fits 32 bits), table indices are masked or checked by the routines of
// jpeg_entropy_dec.h, nothing is stored unless STORE, and then only at coef[g * 64 + k] with
// 0 <= g < nblk and k <= 63 checked before the store.
#pragma once
#include "jpeg_entropy_dec.h"

constexpr uint32_t JPEG_SYNC_MAX_LEN = 1u << 28;      // bytes per interval: bit positions fit 32 bits
constexpr int JPEG_SYNC_MAX_CHUNKS = 1024;            // chunks per interval (and lanes per group)
constexpr uint32_t JPEG_SYNC_ERR = 0xffffffffu;       // a packed exit that is no state

struct JpegSyncRun {
  uint32_t p;            // in: start; out: the first symbol boundary at or past the chunk end
  int blk, k;            // block of the MCU; 0 = a DC symbol is next, else the AC zig-zag index
  uint32_t blocks;       // out: DC symbols decoded
  uint32_t done;         // out: blocks completed (EOB or k = 63) with an index in 0 .. nblk-1
  int err;               // out: JPEG_DEC_OK or the first structural error
  int err_block;         // out: index of the block that error is in
};

// a state relative to the chunk end `base` (bytes): its bit offset is below 128
JPEG_DEC_FN uint32_t jpeg_sync_pack(uint32_t p, int blk, int k, uint32_t base) {
  return ((p - 8u * base) << 9) | ((uint32_t)blk << 6) | (uint32_t)k;
}
JPEG_DEC_FN void jpeg_sync_unpack(uint32_t w, uint32_t base, JpegSyncRun& s) {
  s.p = 8u * base + (w >> 9);
  s.blk = (int)((w >> 6) & 7u);
  s.k = (int)(w & 63u);
}

struct JpegSyncWindow {
  const uint8_t* b;
  uint32_t len;
  uint64_t win;          // bytes wbase .. wbase + 7, big-endian, none of them 0xFF
  uint32_t wbase;        // 0xffffffff: nothing cached
};

// The up to 32 data bits from raw bit p on, as a JpegBits nothing more can be read into.
// Returns true when they came from the cached window (then raw bits = data bits).
JPEG_DEC_FN bool jpeg_sync_peek(JpegSyncWindow& c, uint32_t p, JpegBits& r) {
  r.p = c.b; r.len = 0; r.pos = 0;                    // jpeg_bits_fill finds nothing to add
  const uint32_t B = p >> 3;
  uint32_t off = p - 8u * c.wbase;                    // wraps to something large when p < 8 wbase
  if (c.wbase == 0xffffffffu || p < 8u * c.wbase || off > 32u) {
    off = 64u;
    if (c.len >= 8u && B <= c.len - 8u) {
      uint64_t w;
      __builtin_memcpy(&w, c.b + B, 8);
      const uint64_t v = ~w;                                   // a zero byte of v = a 0xFF
      if (((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) == 0) {
        c.win = __builtin_bswap64(w);
        c.wbase = B;
        off = p & 7u;
      }
    }
  }
  if (off <= 32u) {
    r.acc = (c.win << off) >> 32;
    r.n = 32;
    return true;
  }
  uint64_t acc = 0;
  int nbytes = 0;
  uint32_t q = B;
  while (nbytes < 5 && q < c.len) {
    const uint32_t x = c.b[q];
    if (x == 0xffu) {
      if (q + 1 < c.len && c.b[q + 1] == 0) q += 2;
      else break;                                              // the data ends here
    } else {
      ++q;
    }
    acc = (acc << 8) | x;
    ++nbytes;
  }
  int n = 8 * nbytes - (int)(p & 7u);
  if (n < 0) n = 0;
  if (n > 32) {
    acc >>= n - 32;
    n = 32;
  }
  r.acc = acc;                                                 // only the low n bits are pending
  r.n = n;
  return false;
}

// p after `used` data bits that jpeg_sync_peek gathered byte by byte
JPEG_DEC_FN uint32_t jpeg_sync_walk(const JpegSyncWindow& c, uint32_t p, int used) {
  const uint32_t t = (p & 7u) + (uint32_t)used;
  uint32_t q = p >> 3;
  for (uint32_t i = 0; i < (t >> 3) && q < c.len; ++i) q += c.b[q] == 0xffu ? 2u : 1u;
  return 8u * q + (t & 7u);
}

// One lane run over bytes[0 .. len) of an interval: symbols while s.p < 8 * end (end <= len).
// tabs = JPEG_DEC_WORDS words.  first = index in the interval of the block s is in (k != 0) or
// about to start (k == 0); coef = the interval's first coefficient, nblk its block count.
template <bool STORE>
JPEG_DEC_FN void jpeg_sync_lane_run(const uint8_t* bytes, uint32_t len, uint32_t end, const uint32_t* tabs, int nb,
                                    JpegSyncRun& s, int first, int nblk, int16_t* coef) {
  JpegSyncWindow c;
  c.b = bytes; c.len = len; c.win = 0; c.wbase = 0xffffffffu;
  uint32_t p = s.p;
  int blk = s.blk, k = s.k, g = first;
  s.blocks = 0; s.done = 0; s.err = JPEG_DEC_OK; s.err_block = 0;
  const uint32_t stop = 8u * (end < len ? end : len);
  while (p < stop) {
    const uint32_t* dc = tabs + JPEG_DEC_QZ_WORDS + (blk < nb - 2 ? 0 : JPEG_DEC_TABLE_WORDS);
    JpegBits r;
    const bool fast = jpeg_sync_peek(c, p, r);
    const int n0 = r.n;
    int err = JPEG_DEC_OK, v = 0;
    bool complete = false;
    if (k == 0) {
      const int sz = jpeg_dec_symbol(r, dc);
      if (sz < 0) err = -sz;
      else if (sz > 11) err = JPEG_DEC_BAD_CODE;
      else if (sz != 0 && !jpeg_dec_receive(r, sz, v)) err = JPEG_DEC_TRUNCATED;
      if (err == JPEG_DEC_OK) {
        ++s.blocks;
        if (STORE && v != 0 && (uint32_t)g < (uint32_t)nblk) coef[(long long)g * 64] = (int16_t)v;
        k = 1;
      }
    } else {
      const int rs = jpeg_dec_symbol(r, dc + 2 * JPEG_DEC_TABLE_WORDS);
      const int run = rs >> 4, sz = rs & 15;
      if (rs < 0) {
        err = -rs;
      } else if (sz == 0) {
        if (rs == 0) complete = true;                          // EOB
        else if (run != 15) err = JPEG_DEC_BAD_CODE;
        else if (k + 16 > 63) err = JPEG_DEC_OVERRUN;          // ZRL: a coefficient has to follow
        else k += 16;
      } else if (sz > 10) {
        err = JPEG_DEC_BAD_CODE;
      } else if (k + run > 63) {
        err = JPEG_DEC_OVERRUN;
      } else if (!jpeg_dec_receive(r, sz, v)) {
        err = JPEG_DEC_TRUNCATED;
      } else {
        k += run;
        if (STORE && (uint32_t)g < (uint32_t)nblk && k <= 63) coef[(long long)g * 64 + k] = (int16_t)v;
        ++k;
        complete = k > 63;
      }
    }
    if (err != JPEG_DEC_OK) {
      s.err = err;
      s.err_block = g;
      break;
    }
    if (complete) {
      if ((uint32_t)g < (uint32_t)nblk) ++s.done;
      ++g;
      k = 0;
      blk = blk + 1 == nb ? 0 : blk + 1;
    }
    p = fast ? p + (uint32_t)(n0 - r.n) : jpeg_sync_walk(c, p, n0 - r.n);
  }
  s.p = p; s.blk = blk; s.k = k;
}

// The start of lane c > 0 in round 0: the first bit of its chunk, one byte later when that byte
// is a stuffed zero
JPEG_DEC_FN uint32_t jpeg_sync_guess(const uint8_t* bytes, uint32_t len, uint32_t begin) {
  const bool stuffed = begin > 0 && begin < len && bytes[begin] == 0 && bytes[begin - 1] == 0xffu;
  return 8u * (begin + (stuffed ? 1u : 0u));
}

// The refusal rule on one stored block (64 zig-zag coefficients, q = its zig-zag table)
JPEG_DEC_FN bool jpeg_sync_block_ok(const int16_t* coef, const uint32_t* q) {
  uint32_t energy = 0;
  bool ok = true;
  for (int k = 0; k < 64; ++k) {
    const int d = (int)coef[k] * (int)q[k];                    // |coef| < 2^15, Q <= 255
    if (d < -JPEG_DEC_WIDE_T || d > JPEG_DEC_WIDE_T) ok = false;
    else energy += (uint32_t)(d * d);                          // at most 64 T^2 < 2^32
  }
  return ok && energy <= (uint32_t)JPEG_DEC_WIDE_T * JPEG_DEC_WIDE_T;
}

// whether a DC predictor (32-bit prefix sum, taken as signed) may be stored: |pred * Q| <= T
JPEG_DEC_FN bool jpeg_sync_dc_ok(uint32_t pred, uint32_t q0) {
  const int32_t v = (int32_t)pred;
  const int32_t lim = (int32_t)((uint32_t)JPEG_DEC_WIDE_T / (q0 ? q0 : 1u));
  return v >= -lim && v <= lim;
}
