// The table builder of the OPTIMISED HUFFMAN TABLES section (jpeg.hip's header comment): from the
// 257 symbol frequencies of one table to its code lengths (T.81 K.2 as libjpeg's
// jpeg_gen_optimal_table runs it, tie rules included), the canonical (length << 16) | code words
// the coders read, the table's DHT values, and the DHT segment of an image's four tables.  Plain
// functions over pointers, compiled as they stand by jpeg_huff_build_kernel (jpeg.hip: one wave
// per table, `lane` = 0..63) and by a host program (tests/native/jpeg_huff_opt_host.cpp: one
// "lane", lane = 0, under host sanitizers).  ops/jpeg_format.py is the numpy model (optimal_table).
//
// A wave shares one JpegHuffWork in LDS.  The two searches for the smallest frequency are spread
// over the lanes and reduced; the merge and the walks along the `others` chains are lane 0's, and
// jpeg_huff_sync() orders its LDS stores before the other lanes' next loads.  Every loop is
// bounded by JPEG_HUFF_SYMS or JPEG_HUFF_MAX_LEN, whatever the frequencies are.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define JPEG_HUFF_FN __host__ __device__ inline
#else
#define JPEG_HUFF_FN inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
constexpr int JPEG_HUFF_LANES = 64;
#else
constexpr int JPEG_HUFF_LANES = 1;
#endif

constexpr int JPEG_HUFF_SYMS = 257;                   // 256 symbols + the reserved one
constexpr int JPEG_HUFF_MAX_LEN = 32;                 // code lengths before they are limited to 16
// bits per block with tables of the image's own: any code can be 16 bits long, a DC one included
// (jpeg_format.block_bits_bound_optimized())
constexpr uint32_t JPEG_BLK_MAX_BITS_OPT = 16 + 11 + 63 * (16 + 10);

struct JpegHuffWork {
  uint32_t freq[JPEG_HUFF_SYMS];
  int32_t codesize[JPEG_HUFF_SYMS];
  int32_t others[JPEG_HUFF_SYMS];
  int32_t bits[JPEG_HUFF_MAX_LEN + 1];
  uint32_t nvals;                                     // symbols of the finished table
  uint32_t bad;                                       // a code longer than JPEG_HUFF_MAX_LEN (256 symbols cannot reach it)
  uint8_t vals[256];                                  // the DHT's HUFFVAL
};

// lane 0's LDS stores before this point are what every lane of the wave loads after it
JPEG_HUFF_FN void jpeg_huff_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
#endif
}

// The index with the smallest non-zero frequency, the largest index among equal ones, `exclude`
// left out; -1 if there is none.  The key orders by frequency, then by reversed index.
JPEG_HUFF_FN int jpeg_huff_argmin(const uint32_t* freq, int exclude, int lane) {
  uint64_t best = ~0ull;
  for (int i = lane; i < JPEG_HUFF_SYMS; i += JPEG_HUFF_LANES) {
    const uint32_t f = freq[i];
    const uint64_t key = ((uint64_t)f << 32) | (uint32_t)(JPEG_HUFF_SYMS - 1 - i);
    if (f != 0u && i != exclude && key < best) best = key;
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o, 64);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, o, 64);
    const uint64_t other = ((uint64_t)hi << 32) | lo;
    if (other < best) best = other;
  }
#endif
  return best == ~0ull ? -1 : JPEG_HUFF_SYMS - 1 - (int)(uint32_t)best;
}

// freq[0 .. 255] filled by the caller (the sum below 2^32 - 1): code lengths into w.bits[1 .. 16].
JPEG_HUFF_FN void jpeg_huff_build(JpegHuffWork& w, int lane) {
  for (int i = lane; i < JPEG_HUFF_SYMS; i += JPEG_HUFF_LANES) {
    w.codesize[i] = 0;
    w.others[i] = -1;
  }
  for (int i = lane; i <= JPEG_HUFF_MAX_LEN; i += JPEG_HUFF_LANES) w.bits[i] = 0;
  if (lane == 0) {
    w.freq[JPEG_HUFF_SYMS - 1] = 1u;                  // the reserved symbol: no code is all ones
    w.nvals = 0u;
    w.bad = 0u;
  }
  jpeg_huff_sync();
  for (int round = 0; round < JPEG_HUFF_SYMS; ++round) {          // every merge empties one entry
    const int c1 = jpeg_huff_argmin(w.freq, -1, lane);
    const int c2 = c1 < 0 ? -1 : jpeg_huff_argmin(w.freq, c1, lane);
    if (c2 < 0) break;                                             // the same in every lane
    if (lane == 0) {
      w.freq[c1] += w.freq[c2];
      w.freq[c2] = 0u;
      int c = c1;
      for (int n = 0; n < JPEG_HUFF_SYMS; ++n) {                   // c1 and its chain
        ++w.codesize[c];
        if (w.others[c] < 0) break;
        c = w.others[c];
      }
      w.others[c] = c2;
      c = c2;
      for (int n = 0; n < JPEG_HUFF_SYMS; ++n) {                   // c2 and its chain
        ++w.codesize[c];
        if (w.others[c] < 0) break;
        c = w.others[c];
      }
    }
    jpeg_huff_sync();
  }
  if (lane == 0) {
    for (int i = 0; i < JPEG_HUFF_SYMS; ++i) {
      const int cs = w.codesize[i];
      if (cs > JPEG_HUFF_MAX_LEN) w.bad = 1u;
      else if (cs > 0) ++w.bits[cs];
    }
    for (int i = JPEG_HUFF_MAX_LEN; i > 16; --i) {
      for (int n = 0; n < JPEG_HUFF_SYMS && w.bits[i] > 0; ++n) {
        int j = i - 2;
        while (j > 0 && w.bits[j] == 0) --j;
        if (j == 0) {                                              // not a prefix code's counts: refuse
          w.bad = 1u;
          break;
        }
        w.bits[i] -= 2;
        w.bits[i - 1] += 1;
        w.bits[j + 1] += 2;
        w.bits[j] -= 1;
      }
    }
    int i = 16;
    while (i > 0 && w.bits[i] == 0) --i;
    if (i > 0) --w.bits[i];                                        // the reserved symbol leaves
    uint32_t n = 0;
    for (int l = 1; l <= 16; ++l) n += (uint32_t)w.bits[l];
    w.nvals = n > 256u ? 256u : n;
    if (n > 256u) w.bad = 1u;
  }
  jpeg_huff_sync();
}

// Canonical codes (T.81 Annex C) in the order of the DHT: symbols by code length before the
// limiting, then by value.  Symbol j < nslots gets words[j] = (length << 16) | code, 0 without a
// code; w.vals[rank] = j.  A lane owns the symbols lane, lane + LANES, ...
JPEG_HUFF_FN void jpeg_huff_assign(JpegHuffWork& w, uint32_t* words, int nslots, int lane) {
  for (int j = lane; j < 256; j += JPEG_HUFF_LANES) {
    const int cs = w.codesize[j];
    uint32_t word = 0u;
    if (cs > 0 && w.bad == 0u) {
      uint32_t rank = 0;
      for (int k = 0; k < 256; ++k) {
        const int ck = w.codesize[k];
        if (ck > 0 && (ck < cs || (ck == cs && k < j))) ++rank;
      }
      uint32_t first = 0, cum = 0;
      for (int l = 1; l <= 16; ++l) {
        const uint32_t n = (uint32_t)w.bits[l];
        if (rank < cum + n) {
          word = ((uint32_t)l << 16) | ((first + rank - cum) & 0xffffu);
          break;
        }
        first = (first + n) << 1;
        cum += n;
      }
      if (rank < 256u) w.vals[rank] = (uint8_t)j;
    }
    if (j < nslots) words[j] = word;
  }
  jpeg_huff_sync();
}

// The DHT segment of an image's four tables t[0 .. 3] = DC luma, DC chroma, AC luma, AC chroma,
// written in the order DC luma, AC luma, DC chroma, AC chroma at dst[0 .. cap): thread tid of
// nthreads stores the bytes tid, tid + nthreads, ...  Returns the segment's length, the same in
// every thread; a byte at or past cap is not stored.  per_table: a segment per table, each with
// its own marker and length (the layout libjpeg writes), in the same order.
JPEG_HUFF_FN uint32_t jpeg_huff_dht(const JpegHuffWork* t, uint8_t* dst, uint32_t cap, int tid, int nthreads,
                                    bool per_table = false) {
  // segment slot s = 0..3 holds table ((s & 1) << 1) | (s >> 1) under the id Tc = s & 1, Th = s >> 1
  if (per_table) {
    uint32_t at = 0;
    for (int s = 0; s < 4; ++s) {
      const JpegHuffWork& w = t[((s & 1) << 1) | (s >> 1)];
      const uint32_t n = 4u + 17u + w.nvals;
      for (uint32_t i = (uint32_t)tid; i < n; i += (uint32_t)nthreads) {
        uint32_t v;
        if (i < 4u) v = i == 0u ? 0xffu : (i == 1u ? 0xc4u : (i == 2u ? ((n - 2u) >> 8) : ((n - 2u) & 0xffu)));
        else if (i == 4u) v = (uint32_t)(((s & 1) << 4) | (s >> 1));
        else v = i < 21u ? (uint32_t)w.bits[i - 4u] : w.vals[i - 21u];
        if (at + i < cap) dst[at + i] = (uint8_t)v;
      }
      at += n;
    }
    return at;
  }
  uint32_t len = 4;
  for (int s = 0; s < 4; ++s) len += 17u + t[s].nvals;
  for (uint32_t i = (uint32_t)tid; i < len; i += (uint32_t)nthreads) {
    uint32_t v;
    if (i < 4u) {
      v = i == 0u ? 0xffu : (i == 1u ? 0xc4u : (i == 2u ? ((len - 2u) >> 8) : ((len - 2u) & 0xffu)));
    } else {
      uint32_t o = i - 4u;
      v = 0u;
      for (int s = 0; s < 4; ++s) {
        const JpegHuffWork& w = t[((s & 1) << 1) | (s >> 1)];
        const uint32_t n = 17u + w.nvals;
        if (o < n) {
          v = o == 0u ? (uint32_t)(((s & 1) << 4) | (s >> 1)) : (o < 17u ? (uint32_t)w.bits[o] : w.vals[o - 17u]);
          break;
        }
        o -= n;
      }
    }
    if (i < cap) dst[i] = (uint8_t)v;
  }
  return len;
}
