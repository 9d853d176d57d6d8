// The sizes of the JPEG codec's buffers, in one place: the MCU geometry of an image, the element
// counts and the word indices of every buffer an encode call takes (the bindings check against
// them, ops.jpeg_encode and tools/bench_jpeg.py allocate from them), the decode-side sizes, and
// every limit that keeps the kernels' 32-bit offsets, counts and launch grids in range.  Plain
// C++17 with no torch and no HIP: the bindings include it, and so does a host program
// (tests/native/jpeg_layout_host.cpp, under host sanitizers).  All arithmetic is in 64 bits, and a
// product that an absurd batch could push past them is bounded by a division first.  A refusal is
// a message (the text a caller raises), null when the call is accepted.
#pragma once
#include <stdint.h>

#include "jpeg_entropy_blk.h"   // JPEG_BLK_MAX_BITS
#include "jpeg_huff_opt.h"      // JPEG_BLK_MAX_BITS_OPT

struct JpegGeometry {
  int nb = 0, mx = 0, my = 0;   // blocks per MCU, MCUs per row, MCU rows
  long long mcus = 0;           // per image
  long long restart = 0;        // MCUs between restart markers as the kernels take it: all of them without DRI
  long long per = 0;            // MCUs per interval = min(restart, mcus)
  long long nint = 0;           // intervals per image
};

// H, W in 1..65535, restart in 0..65535 (0: the whole image is one interval): the callers' checks.
inline JpegGeometry jpeg_geometry(long long H, long long W, bool s420, long long restart) {
  const long long mcu = s420 ? 16 : 8;
  JpegGeometry g;
  g.nb = s420 ? 6 : 3;
  g.mx = (int)((W + mcu - 1) / mcu);
  g.my = (int)((H + mcu - 1) / mcu);
  g.mcus = (long long)g.mx * g.my;
  g.restart = restart ? restart : g.mcus;
  g.per = g.restart < g.mcus ? g.restart : g.mcus;
  g.nint = (g.mcus + g.restart - 1) / g.restart;
  return g;
}

// Encode.  work int32 = base [B + 1] (image offsets, payload size) | the block coder's error word |
// with optimised tables every image's header length [B]: the prefix the host reads; then lens and
// offs [B * nint] each.  blk int32 = bits [B * mcus * nb] | ubits [B * nint]; scratch int32
// [B * nint][stride]: an interval's unstuffed string with a slot for the worst case of every block;
// hopt int32 = symbol counts | code words [B * 544] each; hdrs uint8 [B][hdr_cap] every image's
// header: the shared bytes and room for its DHT, one segment header (lj: the four of libjpeg's
// layout) and four tables.  Counts of buffers a call does not take are 0, their indices -1.
struct JpegEncodeLayout {
  JpegGeometry g;
  long long coef = 0, work = 0, blk = 0, scratch = 0, hopt = 0, hdrs = 0;
  long long stride = 0, hdr_cap = 0;
  long long prefix = 0, err = -1, hdr_lens = -1, lens = 0, offs = 0;   // words of work
  long long slack = 0;          // out uint8 [base[B] + slack]: the block coder's error byte
  const char* refusal = nullptr;
};

constexpr long long JPEG_HUFF_WORDS = 544;                  // one set of Huffman tables as the coders read it
constexpr long long JPEG_DHT_BYTES = 4 * (17 + 256);        // the four tables of a DHT, without segment headers

inline JpegEncodeLayout jpeg_encode_layout(long long B, long long H, long long W, bool s420, long long restart,
                                           bool blocks, bool optimized, bool lj, long long header_bytes) {
  JpegEncodeLayout l;
  auto refuse = [&l](const char* why) { l.refusal = why; return l; };
  if (blocks ? restart < 0 || restart >= 65536 : restart < 1 || restart >= 65536)
    return refuse(blocks ? "jpeg: restart_mcus 0..65535" : "jpeg: the HIP encoder needs 1 <= restart_mcus <= 65535");
  if (B < 1 || H < 1 || W < 1) return refuse("jpeg: images uint8 [B, H, W, 3]");
  if (header_bytes < 1) return refuse("jpeg: header uint8");
  if (H >= 65536 || W >= 65536) return refuse("jpeg: image sides must be below 65536");
  const JpegGeometry g = l.g = jpeg_geometry(H, W, s420, restart);
  const long long per_img = g.mcus * g.nb;                  // blocks of one image, below 2^29
  // 32-bit payload offsets: bound by the coder's worst case (20 + 63 * 26 bits per block, 27 + 63 * 26
  // with optimised tables, every byte stuffed, one padding byte and one marker per interval)
  const char* const too_large = "jpeg: batch too large for 32-bit payload offsets";
  if (header_bytes >= 2147483648LL) return refuse(too_large);
  l.hdr_cap = header_bytes + (optimized ? (lj ? 4 * 4 : 4) + JPEG_DHT_BYTES : 0);
  if (B > 2147483647LL / (l.hdr_cap + per_img * (optimized ? 417 : 416) + g.nint * 3)) return refuse(too_large);
  // from here on every product is small: B * per_img * 416 is below 2^31
  const long long nblk = B * per_img, nivals = B * g.nint;
  l.coef = nblk * 64;
  l.err = blocks ? B + 1 : -1;
  l.hdr_lens = optimized ? B + 1 + (blocks ? 1 : 0) : -1;
  l.prefix = l.lens = B + 1 + (blocks ? 1 : 0) + (optimized ? B : 0);
  l.offs = l.lens + nivals;
  l.work = l.offs + nivals;
  if (optimized) {
    if (B > 65535) return refuse("jpeg: at most 65535 images per call with optimised Huffman tables");
    if (per_img * 64 >= 2147483648LL) return refuse("jpeg: optimised Huffman tables count symbols in 32-bit words");
    l.hopt = 2 * B * JPEG_HUFF_WORDS;
    l.hdrs = B * l.hdr_cap;
  }
  if (blocks) {
    const long long bits = g.per * g.nb * (long long)(optimized ? JPEG_BLK_MAX_BITS_OPT : JPEG_BLK_MAX_BITS);
    // bit offsets within an interval are 32-bit words; the slot holds the worst case of every block
    if (bits >= 4294967296LL) return refuse("jpeg: restart interval too long for 32-bit bit offsets");
    l.stride = (bits + 31) / 32;
    if (l.stride >= (1LL << 30)) return refuse("jpeg: stride = ceil(blocks per interval * max bits per block / 32)");
    if (nblk >= 256LL * 2147483647LL || nivals >= 2147483647LL) return refuse("jpeg: batch too large for one launch");
    l.blk = nblk + nivals;
    l.scratch = nivals * l.stride;
    l.slack = 1;
  }
  return l;
}

// Decode.  buf int16 = the coefficients [B * mcus * nb * 64], the 64-bit status word and 8 bytes of
// padding (interval mode), or the status word and uint32 flag, rounds, blocks completed, 0
// (chunked mode); planes one byte per padded sample.  staged uint8 = the interval table
// [B * nint][2] uint32, the nbytes entropy-coded bytes, and in chunked mode, from a later multiple
// of 4 on, uint32 lane0 [B * nint] and groups [ngroups][2].
struct JpegDecodeLayout {
  JpegGeometry g;
  long long nivals = 0, ncoef = 0, buf = 0, planes = 0;
  const char* refusal = nullptr;
  long long staged_min(long long nbytes) const { return 8 * nivals + nbytes; }
  long long sync_bytes(long long ngroups) const { return 4 * nivals + 8 * ngroups; }
};

inline JpegDecodeLayout jpeg_decode_layout(long long B, long long H, long long W, bool s420, long long restart,
                                           bool chunked) {
  JpegDecodeLayout l;
  auto refuse = [&l](const char* why) { l.refusal = why; return l; };
  if (B < 1 || H < 1 || W < 1 || H >= 65536 || W >= 65536) return refuse("jpeg: image sides must be in 1..65535");
  if (restart < 0 || restart >= 65536) return refuse("jpeg: restart interval 0..65535");
  const JpegGeometry g = l.g = jpeg_geometry(H, W, s420, restart);
  // one lane or workgroup per interval, one lane per block (256 to a workgroup); the block bound
  // also keeps the coefficient count in 64 bits
  if (B > 2147483646LL / g.nint || B > (256LL * 2147483647LL - 1) / (g.mcus * g.nb))
    return refuse(chunked ? "jpeg: too many restart intervals or blocks for one launch"
                          : "jpeg: too many restart intervals for one launch");
  l.nivals = B * g.nint;
  l.ncoef = B * g.mcus * g.nb * 64;
  l.buf = l.ncoef + (chunked ? 16 : 8);
  l.planes = l.ncoef;
  return l;
}
