// The per-block coder and the stuffing piece of the BLOCK-PARALLEL ENTROPY CODER (jpeg.hip's header
// comment): the code bits of one 8x8 block depend on its 64 coefficients and on the DC value of
// the previous block of its component only, so every block is coded on its own, first without
// storing (its bit length) and then at its bit offset into the interval's unstuffed string; the
// byte stuffing is done afterwards on fixed-size pieces of that string.  Plain functions over
// pointers and sizes, compiled as they stand by the jpeg_blk_* kernels (jpeg.hip) and by a host
// program (tests/native/jpeg_entropy_blk_host.cpp, which runs the passes serially under host
// sanitizers on buffers of exactly the computed sizes).  ops/jpeg_format.py is the numpy model
// (entropy_blocks).
//
// The unstuffed string of an interval lives in 32-bit words, MSB first: bit p of the string is bit
// 31 - (p & 31) of word p >> 5, byte i is bits 31 - 8 (i & 3) .. 24 - 8 (i & 3) of word i >> 2.
//
// Both forms of a routine are one template (count / write), so the two passes cannot disagree; the
// symbol walk has a third form that only counts its symbols (the histogram of the optimised tables).
// Memory safety: a word is stored or merged only at an index below `nwords`, a payload byte only
// at an index below `out_size`, a scratch word is read only below `nwords`; a refused index sets
// `bad` and nothing is written.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define JPEG_BLK_FN __host__ __device__ inline
#else
#define JPEG_BLK_FN inline
#endif

// bits per block <= longest DC code (11) + 11 value bits + 63 * (longest AC code (16) + 10 value
// bits): jpeg_format.block_bits_bound() derives the same number from the tables (asserted)
constexpr uint32_t JPEG_BLK_MAX_BITS = 11 + 11 + 63 * (16 + 10);
constexpr uint32_t JPEG_BLK_PIECE = 32;                // unstuffed bytes per stuffing piece (a multiple of 4)

// merge into a zeroed word that other blocks merge into as well
JPEG_BLK_FN void jpeg_blk_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}

// The DC value the difference of block k of MCU m is taken against (coef: the image's [mcus][nb][64],
// per: MCUs per interval): the block before it of the same component in coding order, 0 at the
// start of an interval.  Luma blocks of an MCU follow each other, the first follows the last luma
// block of the MCU before; Cb / Cr follow the MCU before.
JPEG_BLK_FN int jpeg_blk_pred(const int16_t* coef, long long m, int k, int nb, int per) {
  const int nl = nb - 2;
  if (k > 0 && k < nl) return coef[(m * nb + k - 1) * 64];
  if (m % per == 0) return 0;
  return coef[((m - 1) * nb + (k == 0 ? nl - 1 : k)) * 64];
}

template <bool WRITE>
struct JpegBlkSink {
  uint32_t pos = 0;            // bits of this block so far
  // WRITE only
  uint64_t acc = 0;            // only the low `n` bits are pending
  int n = 0;                   // 0 .. 31 between puts; starts at the block's bit offset in its first word
  uint32_t w = 0;              // index of the word the pending bits belong to
  uint32_t* words = nullptr;
  uint32_t nwords = 0;
  bool shared = true;          // the next word out holds other blocks' bits too: merged, not stored
  bool bad = false;

  JPEG_BLK_FN void start(uint32_t* words_, uint32_t nwords_, uint32_t bit_offset) {
    words = words_;
    nwords = nwords_;
    w = bit_offset >> 5;
    n = (int)(bit_offset & 31u);
  }
  JPEG_BLK_FN void word(uint32_t v) {
    if (w < nwords) {
      if (shared) jpeg_blk_or(words + w, v);
      else words[w] = v;
    } else {
      bad = true;
    }
    ++w;
    shared = false;
  }
  JPEG_BLK_FN void put(uint32_t bits, int len) {     // len <= 27, bits < 2^len
    pos += (uint32_t)len;
    if (WRITE) {
      acc = (acc << len) | bits;
      n += len;
      if (n >= 32) {                                   // n < 32 + 27: one word at most
        word((uint32_t)(acc >> (n - 32)));
        n -= 32;
      }
    }
  }
  // a symbol of table `tab` followed by its `nbits` value bits
  JPEG_BLK_FN void sym(const uint32_t* tab, int index, uint32_t bits, int nbits) {
    const uint32_t h = tab[index];
    put(((h & 0xffffu) << nbits) | bits, (int)(h >> 16) + nbits);
  }
  // after the block's last symbol; `last`: the block ends its interval, whose last byte is padded
  // with 1-bits (bit_offset + pos is the interval's bit count)
  JPEG_BLK_FN void finish(uint32_t bit_offset, bool last) {
    if (!WRITE) return;
    if (last) {
      const int pad = (int)((8u - ((bit_offset + pos) & 7u)) & 7u);
      const uint32_t keep = pos;
      if (pad) put((1u << pad) - 1u, pad);
      pos = keep;
    }
    if (n > 0) {
      shared = true;                                   // the next block starts in this word (or nothing does)
      word((uint32_t)(acc << (32 - n)));
    }
  }
};

// The counting sink: the third form of the coder (OPTIMISED HUFFMAN TABLES, jpeg.hip's header
// comment).  Its "tables" are histograms in the same layout, and a symbol adds one to its word.
struct JpegBlkCount {
  JPEG_BLK_FN void sym(uint32_t* tab, int index, uint32_t, int) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(tab + index, 1u);
#else
    ++tab[index];
#endif
  }
};

template <class Sink, class Tab>
JPEG_BLK_FN void jpeg_blk_ac(Sink& w, Tab ac, int& run, int val) {
  if (val == 0) {
    ++run;
    return;
  }
  while (run >= 16) {
    w.sym(ac, 0xF0, 0u, 0);
    run -= 16;
  }
  const int a = val < 0 ? -val : val;
  const int cat = 32 - __builtin_clz((unsigned)a);
  const uint32_t bits = (uint32_t)(val < 0 ? val - 1 : val) & ((1u << cat) - 1u);
  w.sym(ac, ((run << 4) | cat) & 255, bits, cat);
  run = 0;
}

// One block (64 zig-zag coefficients, 16-byte aligned) through the symbol walk of the byte
// contract: the DC category of the difference, then (run << 4) | size, ZRL and EOB, each handed
// to the sink with its table, its value bits and their count.  Counting, measuring and storing
// are this one walk with three sinks, so they cannot disagree.
template <class Sink, class Tab>
JPEG_BLK_FN void jpeg_blk_walk(const int16_t* blk, int pred, Tab dc, Tab ac, Sink& w) {
  const uint8_t* src = static_cast<const uint8_t*>(__builtin_assume_aligned(blk, 16));
  int run = 0;
#pragma unroll 1
  for (int c = 0; c < 8; ++c) {
    uint32_t wd[4];
    __builtin_memcpy(wd, src + 16 * c, 16);
    if (c == 0) {
      const int v0 = (int16_t)(wd[0] & 0xffffu);
      const int d = v0 - pred;
      const int a = d < 0 ? -d : d;
      const int cat = a ? 32 - __builtin_clz((unsigned)a) : 0;
      const uint32_t bits = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << cat) - 1u);
      w.sym(dc, cat & 15, bits, cat);
      jpeg_blk_ac(w, ac, run, (int)(int16_t)(wd[0] >> 16));
#pragma unroll
      for (int j = 2; j < 8; ++j) jpeg_blk_ac(w, ac, run, (int)(int16_t)((wd[j >> 1] >> (16 * (j & 1))) & 0xffffu));
    } else if ((wd[0] | wd[1] | wd[2] | wd[3]) == 0u) {
      run += 8;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) jpeg_blk_ac(w, ac, run, (int)(int16_t)((wd[j >> 1] >> (16 * (j & 1))) & 0xffffu));
    }
  }
  if (run > 0) w.sym(ac, 0, 0u, 0);   // EOB
}

// The coder: dc / ac are the (length << 16) | code tables of the block's component; the bit count
// is w.pos.
template <bool WRITE>
JPEG_BLK_FN void jpeg_blk_code(const int16_t* blk, int pred, const uint32_t* dc, const uint32_t* ac,
                               JpegBlkSink<WRITE>& w) {
  jpeg_blk_walk(blk, pred, dc, ac, w);
}

// The histogram: dc / ac are the block's component's rows of a HUFF_WORDS histogram.
JPEG_BLK_FN void jpeg_blk_count(const int16_t* blk, int pred, uint32_t* dc, uint32_t* ac) {
  JpegBlkCount w;
  jpeg_blk_walk(blk, pred, dc, ac, w);
}

// One stuffing piece: the unstuffed bytes b0 .. b1 - 1 (b0 a multiple of 4) of the string in
// words[0 .. nwords).  Returns the piece's stuffed length = b1 - b0 + its 0xFF bytes; WRITE stores
// them at out[at ..], a 0x00 behind every 0xFF.
template <bool WRITE>
JPEG_BLK_FN uint32_t jpeg_blk_stuff(const uint32_t* words, uint32_t nwords, uint32_t b0, uint32_t b1, uint8_t* out,
                                    uint32_t at, uint32_t out_size, bool& bad) {
  uint32_t len = 0;
  for (uint32_t wi = b0 >> 2; 4u * wi < b1; ++wi) {
    if (wi >= nwords) {
      bad = true;
      break;
    }
    const uint32_t v = words[wi];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4u * wi + (uint32_t)j >= b1) break;
      const uint32_t b = (v >> (24 - 8 * j)) & 0xffu;
      const uint32_t k = b == 0xffu ? 2u : 1u;
      if (WRITE) {
        if ((uint64_t)at + len + k <= (uint64_t)out_size) {
          out[at + len] = (uint8_t)b;
          if (k == 2u) out[at + len + 1] = 0;
        } else {
          bad = true;
        }
      }
      len += k;
    }
  }
  return len;
}
