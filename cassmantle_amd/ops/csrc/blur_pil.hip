// PIL's ImageFilter.GaussianBlur for gfx950, bit for bit, batched over radii: one uint8
// [H][W][3] image in HBM -> slices of a uint8 [N][H][W][3] buffer, one slice per radius.
// ops/blur_format.py is the numpy reference of the same contract and owns the host side (radius
// -> box parameters), which arrives here as a small int32 device table.
//
// THE BLUR CONTRACT (integer arithmetic end to end; the oracle is the installed Pillow)
//
//   Pillow's "Gaussian" is a box blur applied three times along the rows, then three times along
//   the columns (BoxBlur.c).  Host side, per radius; f32 = the step is rounded to float32, as
//   Pillow's C code computes in `float`:
//     radius <= 0: the input, unchanged
//     s2 = f32(f32(radius * radius) / f32(3))
//     L  = f32(sqrt(12.0 * double(s2) + 1.0));   l = f32(floor((double(L) - 1.0) / 2.0))
//     a  = f32(f32((2l + 1) * (l (l + 1) - 3 s2)) / f32(6 * (s2 - (l + 1)(l + 1))))   all float32
//     fr = f32(l + a);   r = int(fr)
//     ww = uint32(f32(2^24) / f32(2 fr + 1))          float32 division, truncated
//     fw = (2^24 - (2r + 1) * ww) / 2                  integer division
//   (radius 0 as a table row is r = 0, ww = 2^24, fw = 0: the identity.)
//
//   One pass along a line of n samples, each channel on its own:
//     out[x] = ( ww * sum_{k = -r .. r} in[clamp(x + k, 0, n - 1)]
//              + fw * (in[clamp(x - r - 1, 0, n - 1)] + in[clamp(x + r + 1, 0, n - 1)])
//              + 2^23 ) >> 24
//   The whole blur: three passes along W, then three along H; every pass reads the uint8 output
//   of the pass before it.
//
//   * (2r + 1) ww + 2 fw <= 2^24, so the sum fits in 32 unsigned bits.
//   * Every operation is an integer operation: any order of summation gives the same bits.
//     The tiled kernel keeps running window sums, the general kernel adds the taps directly.
//   * The clamp applies per pass, to that pass's input: a virtual pixel outside the image is the
//     edge pixel of the previous pass's output, not a value computed further out.
//
// Kernels.  Tiled (box radius r <= 15, i.e. Gaussian radius up to ~16.5): grid z is the row of
// the parameter table (r, ww, fw, slot); a block stages its T x T output tile plus a halo of
// 3 (r + 1) pixels per side, cut at the image border, as uint8 in LDS and runs the six passes
// between two LDS buffers; the last pass stores into slice `slot`.  Indices are clamped to the
// staged extent at every pass: where that extent ends at an image border this is the contract's
// clamp; where it ends inside the image the values near it go stale by r + 1 pixels per pass,
// which after three passes is exactly the halo, so the tile itself is exact.  Pass p of 3 only
// computes what the later passes read: the tile widened by (3 - p)(r + 1).
// The LDS of a launch is sized for the largest r of its table.  T = 64 with 512 threads (two
// 160 x 484 B buffers, 151 KiB, at r = 15): a 61-bucket prewarm's blur stage took 0.78 ms at 512^2
// and 2.97 ms at 1024^2 against 2.50 / 10.1 ms with T = 32 and 256 threads, whose halo is 14x the
// tile's area at r = 14 (profiles/blur_pil_tile_ab.jsonl), so only T = 64 is built.
// General (any r): six one-pass launches through two scratch images, one thread per byte.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PIL_RMAX = 15;           // largest box radius of the tiled kernel
constexpr uint32_t PIL_HALF = 1u << 23;

CM_DEVICE int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// LDS row pitch in bytes of a staged image `e` pixels wide: a multiple of 4 whose dword count is
// odd, so that lanes on consecutive rows (the row passes) fall on different banks
__host__ __device__ inline int pil_pitch(int e) {
  int s = (e * 3 + 3) & ~3;
  if (((s >> 2) & 1) == 0) s += 4;
  return s;
}

// One box pass over `nlines` lines of the staged image.  Line l starts at byte src + base(l) and
// its samples are `es` bytes apart; outputs o0 .. o1 - 1 of every line are computed, indices are
// clamped to 0 .. n - 1.  A work item is one segment of one line: a running window sum, two LDS
// reads and one store per output.  ROWS: line = (row, channel); else line = (column, channel)
// of the tile's columns, which are contiguous bytes.  FINAL: the store goes to global memory at
// gdst + l + x * gpitch instead of the other LDS buffer.
template <int NT, bool ROWS, bool FINAL>
CM_DEVICE void box_pass(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int nlines, int pitch, int col0,
                        int n, int o0, int o1, int r, uint32_t ww, uint32_t fw, uint8_t* __restrict__ gdst,
                        long long gpitch) {
  const int range = o1 - o0;
  if (range <= 0 || nlines <= 0) return;
  int nseg = (2 * NT + nlines - 1) / nlines;               // about two items per thread
  const int most = (range + 7) >> 3;                       // no segment shorter than 8 outputs
  nseg = nseg > most ? most : nseg;
  const int seg = (range + nseg - 1) / nseg;
  nseg = (range + seg - 1) / seg;
  const int es = ROWS ? 3 : pitch;
  for (int item = threadIdx.x; item < nlines * nseg; item += NT) {
    const int sg = item / nlines, l = item - sg * nlines;
    const int base = ROWS ? (l / 3) * pitch + (l % 3) : col0 * 3 + l;
    const int s0 = o0 + sg * seg;
    const int s1 = s0 + seg < o1 ? s0 + seg : o1;
    const uint8_t* p = src + base;
    uint32_t sum = 0;
    for (int k = -r; k <= r; ++k) sum += p[clampi(s0 + k, 0, n - 1) * es];
    uint32_t left = p[clampi(s0 - r - 1, 0, n - 1) * es];
    for (int x = s0; x < s1; ++x) {
      const uint32_t a = p[clampi(x + r + 1, 0, n - 1) * es];
      const uint32_t b = p[clampi(x - r, 0, n - 1) * es];
      const uint8_t v = (uint8_t)((ww * sum + fw * (left + a) + PIL_HALF) >> 24);
      if (FINAL) gdst[l + (long long)x * gpitch] = v;
      else dst[base + x * es] = v;
      sum += a - b;
      left = b;
    }
  }
}

template <int T, int NT>
__global__ void __launch_bounds__(NT) blur_pil_tile_kernel(const uint8_t* __restrict__ img, int H, int W,
                                                           const int* __restrict__ table, int rmax, int nslots,
                                                           uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pil_sm[];
  const int* prm = table + 4 * blockIdx.z;
  const int r = prm[0], slot = prm[3];
  const uint32_t ww = (uint32_t)prm[1], fw = (uint32_t)prm[2];
  // block-uniform: a table row outside what the launch was sized for touches nothing
  if (r < 0 || r > rmax || slot < 0 || slot >= nslots) return;
  const int emax = T + 6 * (rmax + 1);
  const int pitch = pil_pitch(emax);
  uint8_t* A = pil_sm;
  uint8_t* B = pil_sm + emax * pitch;
  const int step = r + 1, halo = 3 * step;
  const int tx0 = blockIdx.x * T, ty0 = blockIdx.y * T;
  const int tx1 = tx0 + T < W ? tx0 + T : W, ty1 = ty0 + T < H ? ty0 + T : H;
  const int lx0 = tx0 - halo > 0 ? tx0 - halo : 0, ly0 = ty0 - halo > 0 ? ty0 - halo : 0;
  const int lx1 = tx1 + halo < W ? tx1 + halo : W, ly1 = ty1 + halo < H ? ty1 + halo : H;
  const int ew = lx1 - lx0, eh = ly1 - ly0;                 // staged extent: <= emax each way
  const int cx0 = tx0 - lx0, cx1 = tx1 - lx0, cy0 = ty0 - ly0, cy1 = ty1 - ly0;   // the tile inside it
  const int tid = threadIdx.x;
  for (int row = tid >> 6; row < eh; row += NT >> 6) {      // one wave per staged row
    const uint8_t* g = img + ((long long)(ly0 + row) * W + lx0) * 3;
    for (int b = tid & 63; b < ew * 3; b += 64) A[row * pitch + b] = g[b];
  }
  __syncthreads();
  // along W, every staged row
  box_pass<NT, true, false>(A, B, eh * 3, pitch, 0, ew, clampi(cx0 - 2 * step, 0, ew), clampi(cx1 + 2 * step, 0, ew),
                            r, ww, fw, nullptr, 0);
  __syncthreads();
  box_pass<NT, true, false>(B, A, eh * 3, pitch, 0, ew, clampi(cx0 - step, 0, ew), clampi(cx1 + step, 0, ew),
                            r, ww, fw, nullptr, 0);
  __syncthreads();
  box_pass<NT, true, false>(A, B, eh * 3, pitch, 0, ew, cx0, cx1, r, ww, fw, nullptr, 0);
  __syncthreads();
  // along H, the tile's columns
  const int tw3 = (cx1 - cx0) * 3;
  box_pass<NT, false, false>(B, A, tw3, pitch, cx0, eh, clampi(cy0 - 2 * step, 0, eh), clampi(cy1 + 2 * step, 0, eh),
                             r, ww, fw, nullptr, 0);
  __syncthreads();
  box_pass<NT, false, false>(A, B, tw3, pitch, cx0, eh, clampi(cy0 - step, 0, eh), clampi(cy1 + step, 0, eh),
                             r, ww, fw, nullptr, 0);
  __syncthreads();
  // local row x of the tile's columns is image row ly0 + x
  uint8_t* g = out + ((long long)slot * H + ly0) * W * 3 + (long long)tx0 * 3;
  box_pass<NT, false, true>(B, nullptr, tw3, pitch, cx0, eh, cy0, cy1, r, ww, fw, g, (long long)W * 3);
}

// general path: one pass along W (axis 0) or H (axis 1) of a whole image, one thread per byte
__global__ void __launch_bounds__(256) blur_pil_line_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            int H, int W, int axis, int r, uint32_t ww, uint32_t fw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)H * W * 3) return;
  const long long px = i / 3;
  const int x = (int)(px % W), y = (int)(px / W);
  const int n = axis ? H : W, pos = axis ? y : x;
  const long long es = axis ? (long long)W * 3 : 3;
  const uint8_t* p = src + (i - pos * es);
  uint32_t sum = 0;
  for (int k = -r; k <= r; ++k) sum += p[clampi(pos + k, 0, n - 1) * es];
  const uint32_t edges = (uint32_t)p[clampi(pos - r - 1, 0, n - 1) * es] + p[clampi(pos + r + 1, 0, n - 1) * es];
  dst[i] = (uint8_t)((ww * sum + fw * edges + PIL_HALF) >> 24);
}

template <int T, int NT>
void launch_tile(const uint8_t* img, int H, int W, const int* table, int n, int rmax, int nslots, uint8_t* out,
                 hipStream_t s) {
  const int emax = T + 6 * (rmax + 1);
  const size_t lds = 2 * (size_t)emax * pil_pitch(emax);
  // more than 64 KiB of dynamic LDS needs the attribute (first call happens outside any graph
  // capture; thread-safe once)
  static const bool once = [] {
    const int e = T + 6 * (PIL_RMAX + 1);
    (void)hipFuncSetAttribute((const void*)&blur_pil_tile_kernel<T, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              2 * e * pil_pitch(e));
    return true;
  }();
  (void)once;
  dim3 grid((W + T - 1) / T, (H + T - 1) / T, n);
  hipLaunchKernelGGL((blur_pil_tile_kernel<T, NT>), grid, dim3(NT), lds, s, img, H, W, table, rmax, nslots, out);
}

}  // namespace

int blur_pil_max_tiled_radius() { return PIL_RMAX; }

void launch_blur_pil_tiled(const uint8_t* img, int H, int W, const int* table, int n, int rmax, int nslots,
                           uint8_t* out, hipStream_t s) {
  launch_tile<64, 512>(img, H, W, table, n, rmax, nslots, out, s);
}

void launch_blur_pil_general(const uint8_t* img, int H, int W, int r, uint32_t ww, uint32_t fw, uint8_t* s1,
                             uint8_t* s2, uint8_t* out, hipStream_t s) {
  const long long n = (long long)H * W * 3;
  const dim3 grid((unsigned)((n + 255) / 256));
  const uint8_t* src[6] = {img, s1, s2, s1, s2, s1};
  uint8_t* dst[6] = {s1, s2, s1, s2, s1, out};
  for (int p = 0; p < 6; ++p)
    hipLaunchKernelGGL(blur_pil_line_kernel, grid, dim3(256), 0, s, src[p], dst[p], H, W, p >= 3, r, ww, fw);
}
