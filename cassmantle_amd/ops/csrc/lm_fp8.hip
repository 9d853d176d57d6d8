// Weight-only fp8 for the prompt LM's decode path (gfx950): skinny-M GEMV over e4m3 weight rows on
// the bf16 MFMA, the row quantiser and the row dequantiser.
//
// lm.hip's gemv_kernel streams bf16 weights (7B = 14.5 GB per token) and spends M FMAs per weight, so
// it turns VALU-bound as the batch grows.  Here a weight is one byte and costs about half a
// conversion instruction whatever M: the products run on v_mfma_f32_16x16x32_bf16.
//
// WEIGHT CONTRACT (ops.reference.quantize_rows_fp8 / dequantize_rows_fp8 / linear_fp8 are its model)
//
// Format.  A projection W [Nw, K] is stored as q (uint8 [Nw, K], row-major, OCP e4m3fn codes) and
// scale (fp32 [Nw]).  K % 16 == 0, rows 16-byte aligned, every scale finite and > 0.  The
// dequantised weight is W'[n,k] = e4m3(q[n,k]) * scale[n].
//
// RMSNorm gain.  The gain is folded into the weight BEFORE quantisation, as ln_fold does for
// LayerNorm: v[n,k] = fp32(w[n,k]) * fp32(gamma[k]) (a product of two bf16 values, exact in fp32).
// The GEMV therefore multiplies RAW bf16 activations: an A operand rounded to bf16 after a scaling
// by gamma leaves the per-block error bound on outputs that nearly cancel against the residual;
// with raw x the output store is the only rounding.
//
// Quantiser.  a[n] = max_k |v[n,k]|; scale[n] = a[n] / 448 (correctly rounded fp32 division), 1.0
// for an all-zero row; q[n,k] = RNE_e4m3(v[n,k] / scale[n]) (the same division), subnormals kept,
// saturating at +-448: the NaN codes 0x7F / 0xFF are never produced.  A row that holds a
// non-finite value gets a non-finite scale (the op checks the scales once and raises).
//
// Product.  y[m,n] = act(r[m] * scale[n] * sum_k x[m,k] * e4m3(q[n,k]) + bias[n]) + residual[m,n],
// r[m] = rsqrt(mean_k x[m,k]^2 + eps) with the fused RMS scale (taken from the same activation
// loads), else 1.  fp32 accumulation; the bf16 (or fp32) store is the one rounding.  Gated
// activations (swiglu, geglu): value row n and gate row N + n, each with its own scale, combined
// as gemv_kernel combines them.  The order in which a row's products are summed depends on K
// alone, not on M or on the other rows: one template serves every M (rows >= M are zero A rows of
// the MFMA), so a sequence's logits are the same bits alone and in any batch bucket.
//
// gemv_fp8_kernel: a block owns 16 output columns (32 weight rows when gated); its 8 waves take the
// 128-wide k-steps round-robin.  In a step lane l = 16 g + c (c = l & 15, g = l >> 4) loads the 16
// codes of weight row c at k0 + 16 g and k0 + 64 + 16 g (two 16-byte loads: a wave covers 128
// contiguous bytes of each of its 16 rows) and converts them in registers to bf16 (exact) as the B
// fragments of four MFMAs; the A fragments are activation row c (zero for c >= M) at the same k.
// MFMA's k is a summation index, so a lane taking 16 consecutive k for two MFMAs is sound as long
// as A and B use the same permutation.  The row sums of squares come from the same A fragments
// (x . x^T on the MFMA, the diagonal), so the fused RMS scale costs no VALU per element.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int FP8_THREADS = 512;
constexpr int FP8_NW = FP8_THREADS / 64;   // waves of a block: they split K
constexpr int FP8_COLS = 16;               // output columns of a block (the MFMA's N)
constexpr int FP8_STEP = 128;              // k elements of one wave step (two 16-byte loads per lane)
constexpr int FP8_UNROLL = 4;              // steps of the unrolled body: all their loads issue first
constexpr int FP8_ROWS = 8;                // activation rows served
#define FP8_ZERO make_uint4(0u, 0u, 0u, 0u)

// four e4m3 codes (one dword, little-endian) -> four bf16, exact
CM_DEVICE void e4m3x4_to_bf16(uint32_t w, uint32_t& lo, uint32_t& hi) {
  lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
  hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
}

// 16 codes -> the bf16 fragments of k 0..7 and 8..15
CM_DEVICE void e4m3x16_to_frags(const uint4& q, bf16x8_t& f0, bf16x8_t& f1) {
  uint4 a, b;
  e4m3x4_to_bf16(q.x, a.x, a.y);
  e4m3x4_to_bf16(q.y, a.z, a.w);
  e4m3x4_to_bf16(q.z, b.x, b.y);
  e4m3x4_to_bf16(q.w, b.z, b.w);
  f0 = as_bf16x8(a);
  f1 = as_bf16x8(b);
}

template <int NB, bool RMS>
CM_DEVICE void fp8_chunk(const uint4 (&q)[NB], uint4 a0, uint4 a1, f32x4_t (&acc)[NB], f32x4_t& ss) {
  const bf16x8_t x0 = as_bf16x8(a0), x1 = as_bf16x8(a1);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    bf16x8_t w0, w1;
    e4m3x16_to_frags(q[b], w0, w1);
    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0, w0, acc[b], 0, 0, 0);
    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1, w1, acc[b], 0, 0, 0);
  }
  if constexpr (RMS) {
    ss = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0, x0, ss, 0, 0, 0);
    ss = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1, x1, ss, 0, 0, 0);
  }
}

template <bool GATED, bool RMS>
__global__ __launch_bounds__(FP8_THREADS) void gemv_fp8_kernel(GemvFp8Args p) {
  constexpr int NB = GATED ? 2 : 1;         // B fragments per step half: value rows, gate rows
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * FP8_COLS;
  const int nrow = n0 + c < p.N ? n0 + c : p.N - 1;   // clamp (result discarded)
  const uint8_t* wr[NB];
  wr[0] = p.Q + (long long)nrow * p.K + 16 * g;
  if constexpr (GATED) wr[1] = p.Q + (long long)(p.N + nrow) * p.K + 16 * g;
  const bool arow = c < p.M;                          // this lane holds activation row c
  const uint16_t* ar = p.A + (long long)(arow ? c : 0) * p.lda + 16 * g;

  f32x4_t acc[NB], ss = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // unrolled body: FP8_UNROLL whole steps of this wave, every weight load in flight before the
  // first conversion (the kernel is an HBM stream, no LDS staging)
  const int nfull = p.K / FP8_STEP;
  int s = wave;
  for (; s + (FP8_UNROLL - 1) * FP8_NW < nfull; s += FP8_UNROLL * FP8_NW) {
    uint4 q0[FP8_UNROLL][NB], q1[FP8_UNROLL][NB];
#pragma unroll
    for (int u = 0; u < FP8_UNROLL; ++u) {
      const long long k0 = (long long)(s + u * FP8_NW) * FP8_STEP;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        q0[u][b] = *reinterpret_cast<const uint4*>(wr[b] + k0);
        q1[u][b] = *reinterpret_cast<const uint4*>(wr[b] + k0 + 64);
      }
    }
#pragma unroll
    for (int u = 0; u < FP8_UNROLL; ++u) {
      const long long k0 = (long long)(s + u * FP8_NW) * FP8_STEP;
      uint4 a0 = FP8_ZERO, a1 = FP8_ZERO, a2 = FP8_ZERO, a3 = FP8_ZERO;
      if (arow) {
        a0 = *reinterpret_cast<const uint4*>(ar + k0);
        a1 = *reinterpret_cast<const uint4*>(ar + k0 + 8);
        a2 = *reinterpret_cast<const uint4*>(ar + k0 + 64);
        a3 = *reinterpret_cast<const uint4*>(ar + k0 + 72);
      }
      fp8_chunk<NB, RMS>(q0[u], a0, a1, acc, ss);
      fp8_chunk<NB, RMS>(q1[u], a2, a3, acc, ss);
    }
  }
  // remaining steps one at a time, each 16-wide chunk checked against K (K % 16 == 0)
  for (; (long long)s * FP8_STEP < p.K; s += FP8_NW) {
    const long long k0 = (long long)s * FP8_STEP;
    const bool in0 = k0 + 16 * g + 16 <= p.K, in1 = k0 + 64 + 16 * g + 16 <= p.K;
    uint4 q0[NB], q1[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      q0[b] = in0 ? *reinterpret_cast<const uint4*>(wr[b] + k0) : FP8_ZERO;
      q1[b] = in1 ? *reinterpret_cast<const uint4*>(wr[b] + k0 + 64) : FP8_ZERO;
    }
    uint4 a0 = FP8_ZERO, a1 = FP8_ZERO, a2 = FP8_ZERO, a3 = FP8_ZERO;
    if (arow && in0) {
      a0 = *reinterpret_cast<const uint4*>(ar + k0);
      a1 = *reinterpret_cast<const uint4*>(ar + k0 + 8);
    }
    if (arow && in1) {
      a2 = *reinterpret_cast<const uint4*>(ar + k0 + 64);
      a3 = *reinterpret_cast<const uint4*>(ar + k0 + 72);
    }
    fp8_chunk<NB, RMS>(q0, a0, a1, acc, ss);
    fp8_chunk<NB, RMS>(q1, a2, a3, acc, ss);
  }

  // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register: lane groups 0 and 1 hold the 8 rows
  __shared__ float red[FP8_NW][NB][FP8_ROWS][FP8_COLS];
  __shared__ float red_ss[FP8_NW][FP8_ROWS];
  if (g < 2) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][b][4 * g + r][c] = acc[b][r];
    }
    if constexpr (RMS) {
      // the diagonal of x . x^T: row c sits in lane group c >> 2, register c & 3
      if (c < FP8_ROWS && g == (c >> 2)) {
        const int r = c & 3;
        red_ss[wave][c] = r == 0 ? ss[0] : r == 1 ? ss[1] : r == 2 ? ss[2] : ss[3];
      }
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= FP8_ROWS * FP8_COLS) return;
  const int m = t >> 4, n = n0 + (t & 15);
  if (n >= p.N || m >= p.M) return;
  float rm = 1.f;
  if constexpr (RMS) {
    float s2 = 0.f;
#pragma unroll
    for (int w = 0; w < FP8_NW; ++w) s2 += red_ss[w][m];
    rm = rsqrtf(s2 / p.K + p.rms_eps);
  }
  float o = 0.f;
#pragma unroll
  for (int w = 0; w < FP8_NW; ++w) o += red[w][0][m][t & 15];
  o *= rm * p.scale[n];
  if constexpr (GATED) {
    float gt = 0.f;
#pragma unroll
    for (int w = 0; w < FP8_NW; ++w) gt += red[w][NB - 1][m][t & 15];
    gt *= rm * p.scale[p.N + n];
    if (p.bias) { o += bf2f(p.bias[n]); gt += bf2f(p.bias[p.N + n]); }
    o = gate_f(o, gt, p.act);
  } else {
    if (p.bias) o += bf2f(p.bias[n]);
    o = apply_act(o, p.act);
  }
  const long long off = (long long)m * p.ldc + n;
  if (p.residual) o += bf2f(p.residual[(long long)m * p.ldr + n]);
  if (p.out_f32) reinterpret_cast<float*>(p.C)[off] = o;
  else reinterpret_cast<uint16_t*>(p.C)[off] = f2bf(o);
}

// ------------------------------------------------------------------------------- quantiser
constexpr int QUANT_THREADS = 256;

// fp32 -> e4m3fn code, round to nearest even, subnormals kept, saturating (never 0x7F / 0xFF)
CM_DEVICE uint32_t e4m3_rne(float f) {
  const uint32_t sign = (__float_as_uint(f) >> 24) & 0x80u;
  const float a = fabsf(f);
  uint32_t code;
  if (!(a < 464.f)) {
    code = 0x7E;                                   // at or beyond the midpoint above 448 (NaN too)
  } else if (a >= 0.015625f) {                     // normal: 2^-6 and up, 20 mantissa bits dropped
    uint32_t u = __float_as_uint(a);
    u += 0x7FFFFu + ((u >> 20) & 1u);
    code = (u >> 20) - ((127u - 7u) << 3);
    if (code > 0x7Eu) code = 0x7E;
  } else {
    code = (uint32_t)rintf(a * 512.f);             // subnormal: multiples of 2^-9 (8 = the first normal)
  }
  return sign | code;
}

// one block per row: amax of w * gamma, the scale, then the codes
__global__ __launch_bounds__(QUANT_THREADS) void quant_rows_fp8_kernel(const uint16_t* w, const uint16_t* gamma,
                                                                       uint8_t* q, float* scale, int K) {
  const long long row = blockIdx.x;
  const uint16_t* wr = w + row * K;
  float amax = 0.f;
  bool bad = false;
  for (int k = threadIdx.x * 8; k < K; k += QUANT_THREADS * 8) {
    float v[8], gf[8];
    unpack8(*reinterpret_cast<const uint4*>(wr + k), v);
    if (gamma) unpack8(*reinterpret_cast<const uint4*>(gamma + k), gf);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = fabsf(gamma ? v[e] * gf[e] : v[e]);
      bad |= !(x < INFINITY);                      // Inf or NaN
      amax = fmaxf(amax, x);
    }
  }
  amax = wave_max(bad ? INFINITY : amax);
  __shared__ float red[QUANT_THREADS / 64];
  __shared__ float sc_sh;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = red[0];
#pragma unroll
    for (int i = 1; i < QUANT_THREADS / 64; ++i) a = fmaxf(a, red[i]);
    const float sc = a == 0.f ? 1.f : __fdiv_rn(a, 448.f);
    sc_sh = sc;
    scale[row] = sc;
  }
  __syncthreads();
  const float sc = sc_sh;
  for (int k = threadIdx.x * 8; k < K; k += QUANT_THREADS * 8) {
    float v[8], gf[8];
    unpack8(*reinterpret_cast<const uint4*>(wr + k), v);
    if (gamma) unpack8(*reinterpret_cast<const uint4*>(gamma + k), gf);
    uint32_t c[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = e4m3_rne(__fdiv_rn(gamma ? v[e] * gf[e] : v[e], sc));
    uint2 o;
    o.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    o.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
    *reinterpret_cast<uint2*>(q + row * K + k) = o;
  }
}

// ------------------------------------------------------------------------------ dequantiser
// out[n][k] = bf16_rne(fp32(e4m3(q[n][k])) * scale[n]); one lane per 16 codes
__global__ void dequant_rows_fp8_kernel(const uint8_t* q, const float* scale, uint16_t* out, long long chunks,
                                        int chunks_per_row) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= chunks) return;
  const float sc = scale[i / chunks_per_row];
  const uint4 v = *reinterpret_cast<const uint4*>(q + i * 16);
  uint4 b[2];
  e4m3x4_to_bf16(v.x, b[0].x, b[0].y);
  e4m3x4_to_bf16(v.y, b[0].z, b[0].w);
  e4m3x4_to_bf16(v.z, b[1].x, b[1].y);
  e4m3x4_to_bf16(v.w, b[1].z, b[1].w);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float f[8];
    unpack8(b[h], f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] *= sc;
    *reinterpret_cast<uint4*>(out + i * 16 + 8 * h) = pack8(f);
  }
}

template <bool GATED>
void gemv_fp8_launch(const GemvFp8Args& p, hipStream_t s) {
  const dim3 grid((p.N + FP8_COLS - 1) / FP8_COLS);
  if (p.rms) hipLaunchKernelGGL((gemv_fp8_kernel<GATED, true>), grid, dim3(FP8_THREADS), 0, s, p);
  else hipLaunchKernelGGL((gemv_fp8_kernel<GATED, false>), grid, dim3(FP8_THREADS), 0, s, p);
}

}  // namespace

bool launch_gemv_fp8(const GemvFp8Args& p, hipStream_t s) {
  if (p.M < 1 || p.M > FP8_ROWS || p.N < 1 || p.K < 16 || p.K % 16 != 0 || p.lda % 8 != 0) return false;
  if (is_gated(p.act)) gemv_fp8_launch<true>(p, s);
  else gemv_fp8_launch<false>(p, s);
  return true;
}

void launch_quant_rows_fp8(const uint16_t* w, const uint16_t* gamma, uint8_t* q, float* scale, long long rows, int K,
                           hipStream_t s) {
  if (rows == 0) return;
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)rows), dim3(QUANT_THREADS), 0, s, w, gamma, q, scale, K);
}

void launch_dequant_rows_fp8(const uint8_t* q, const float* scale, uint16_t* out, long long rows, int K,
                             hipStream_t s) {
  const long long chunks = rows * (K / 16);
  if (chunks == 0) return;
  hipLaunchKernelGGL(dequant_rows_fp8_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, q, scale, out,
                     chunks, K / 16);
}
