// The arithmetic of the LIBJPEG FORWARD CONTRACT (jpeg.hip's header comment): colour conversion,
// the source coordinates of the edge rules, the h2v2 chroma mean with its alternating bias, the
// 8-point jfdctint pass, quantisation and the dummy-block rule.  Plain functions over values and
// pointers, compiled as they stand by jpeg_transform_lj_kernel (jpeg.hip) and by a host program
// (tests/native/jpeg_fdct_lj_host.cpp, under host sanitizers).  ops/jpeg_format.py is the numpy
// model (coefficients_libjpeg).  Every intermediate fits a 32-bit word for 8-bit samples (the
// model asserts it); `>>` is an arithmetic shift, and no negative value is shifted left.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define JPEG_LJ_FN __host__ __device__ inline
#else
#define JPEG_LJ_FN inline
#endif

struct JpegLjYcc { int y, cb, cr; };

// Colour (16-bit fixed point, JFIF / BT.601 full range): libjpeg's rgb_ycc_convert.
JPEG_LJ_FN JpegLjYcc jpeg_lj_ycc(const uint8_t* p) {
  const int r = p[0], g = p[1], b = p[2];
  JpegLjYcc o;
  o.y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  o.cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  o.cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
  return o;
}

// Edge replication of a full-resolution plane: sample v of n real ones.
JPEG_LJ_FN int jpeg_lj_src(int v, int n) { return v < n - 1 ? v : n - 1; }

// 4:2:0: the two image rows chroma row r averages.  Rows at or past ch = ceil(H / 2) are replicas
// of the downsampled row ch - 1, not means of replicated image rows.
JPEG_LJ_FN void jpeg_lj_chroma_rows(int r, int H, int& y0, int& y1) {
  const int ch = (H + 1) >> 1;
  y0 = 2 * (r < ch - 1 ? r : ch - 1);
  y1 = y0 + 1 < H - 1 ? y0 + 1 : H - 1;
}

// h2v2 mean of chroma column x: the bias alternates 1, 2, 1, 2 along a row.
JPEG_LJ_FN int jpeg_lj_chroma_mean(int sum4, int x) { return (sum4 + 1 + (x & 1)) >> 2; }

// (x + 2^(n-1)) >> n
JPEG_LJ_FN int jpeg_lj_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 8-point pass of jfdctint (CONST_BITS 13, PASS1_BITS 2) in place.  FIRST: the row pass, whose
// outputs carry 2 more fraction bits; otherwise the column pass, which removes them again (the
// result is 8 x the DCT coefficient).  12 multiplies.
template <bool FIRST>
JPEG_LJ_FN void jpeg_lj_fdct8(int* d) {
  constexpr int SH = FIRST ? 13 - 2 : 13 + 2;
  const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
  int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) * 4;
    d[4] = (t10 - t11) * 4;
  } else {
    d[0] = jpeg_lj_descale(t10 + t11, 2);
    d[4] = jpeg_lj_descale(t10 - t11, 2);
  }
  int z1 = (t12 + t13) * 4433;
  d[2] = jpeg_lj_descale(z1 + t13 * 6270, SH);
  d[6] = jpeg_lj_descale(z1 - t12 * 15137, SH);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446;
  t5 *= 16819;
  t6 *= 25172;
  t7 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = jpeg_lj_descale(t4 + z1 + z3, SH);
  d[5] = jpeg_lj_descale(t5 + z2 + z4, SH);
  d[3] = jpeg_lj_descale(t6 + z2 + z3, SH);
  d[1] = jpeg_lj_descale(t7 + z1 + z4, SH);
}

// f = 8 x the coefficient, q the table's value: round half away from zero; an AC value is held
// to +-1023 (a guard: libjpeg's transform of 8-bit samples stays below it).
JPEG_LJ_FN int jpeg_lj_quant(int f, int q, bool ac) {
  const int q8 = q * 8;
  int mag = ((f < 0 ? -f : f) + (q8 >> 1)) / q8;
  if (ac && mag > 1023) mag = 1023;
  return f < 0 ? -mag : mag;
}

// 4:2:0: is luma block k (Y00 Y01 Y10 Y11) of the MCU at MCU row mby, MCU column mbx a dummy
// block, one that lies outside the ceil(H / 8) x ceil(W / 8) real luma blocks?  A dummy block has
// no AC values and the quantised DC of block k - 1 of its MCU (a dummy itself or not).
JPEG_LJ_FN bool jpeg_lj_dummy(int k, int mby, int mbx, int H, int W) {
  return 2 * mby + (k >> 1) >= ((H + 7) >> 3) || 2 * mbx + (k & 1) >= ((W + 7) >> 3);
}
