// Scorer, image and diffusion-glue kernels.
//
// * gather_cosine (K14): one wave per (guess, answer) pair: gather both table rows (bf16 or
//   f32), dot and both norms in one pass, wave reduction; OOV (-1) -> NaN.  A whole
//   micro-batch of players' guesses is one launch.
// * pair_cosine: row-wise cosine of two embedding matrices (MiniLM scorer).
// * cosine_gemv (K15): table . v / (|row| |v|) for most_similar, one wave per row.
// * mean_pool_l2 (K16 tail): masked mean over tokens + L2 normalisation, one block per row; a row
//   with lens == 0 is the zero vector.
// * gaussian_blur (K17): uint8 images (the served JPEG content), radius <= 48: ONE LDS-tiled
//   kernel per 32x32 output tile — the clamped input tile + halo is staged in LDS once, the
//   horizontal pass writes an f32 LDS intermediate, the vertical pass reads it (no global
//   scratch, one launch).  Other inputs: separable two-pass with a global f32 scratch.
// * to_uint8 (K18): VAE output [-1, 1] -> uint8 (x/2 + 0.5 clamp, *255, round).
// * timestep_embedding (K10), latent_step (K11: CFG combine + scheduler update + next UNet
//   input, reading its coefficient row through a device step counter so a hipGraph replays
//   it unchanged; latent_step_noise_kernel for plans with stochastic rows: one lane per latent
//   pixel, Gaussian noise from philox_normal.h keyed by the image's seed, the eval and the pixel),
//   advance_step, softmax_rows (VAE d=512 attention path).
#include "common.h"
#include "kernels.h"
#include "philox_normal.h"

namespace {

template <bool F32>
CM_DEVICE float ld(const void* p, long long i) {
  if constexpr (F32) return reinterpret_cast<const float*>(p)[i];
  else return bf2f(reinterpret_cast<const uint16_t*>(p)[i]);
}

template <bool F32>
__global__ void gather_cosine_kernel(const void* __restrict__ table, int D, const int* __restrict__ ia,
                                     const int* __restrict__ ib, float* __restrict__ out, int n) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (pair >= n) return;
  const int a = ia[pair], b = ib[pair];
  if (a < 0 || b < 0) {
    if (lane == 0) out[pair] = __builtin_nanf("");
    return;
  }
  float dot = 0.f, na = 0.f, nb = 0.f;
  for (int k = lane; k < D; k += 64) {
    float x = ld<F32>(table, (long long)a * D + k), y = ld<F32>(table, (long long)b * D + k);
    dot = fmaf(x, y, dot); na = fmaf(x, x, na); nb = fmaf(y, y, nb);
  }
  dot = wave_sum(dot); na = wave_sum(na); nb = wave_sum(nb);
  if (lane == 0) out[pair] = dot / fmaxf(sqrtf(na) * sqrtf(nb), 1e-12f);
}

__global__ void pair_cosine_kernel(const float* __restrict__ A, const float* __restrict__ Bm, int D,
                                   float* __restrict__ out, int n) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  float dot = 0.f, na = 0.f, nb = 0.f;
  for (int k = lane; k < D; k += 64) {
    float x = A[(long long)row * D + k], y = Bm[(long long)row * D + k];
    dot = fmaf(x, y, dot); na = fmaf(x, x, na); nb = fmaf(y, y, nb);
  }
  dot = wave_sum(dot); na = wave_sum(na); nb = wave_sum(nb);
  if (lane == 0) out[row] = dot / fmaxf(sqrtf(na) * sqrtf(nb), 1e-12f);
}

template <bool TF32, bool VF32>
__global__ void cosine_gemv_kernel(const void* __restrict__ table, int V, int D, const void* __restrict__ vec,
                                   float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= V) return;
  float dot = 0.f, nt = 0.f, nv = 0.f;
  for (int k = lane; k < D; k += 64) {
    float x = ld<TF32>(table, (long long)row * D + k), y = ld<VF32>(vec, k);
    dot = fmaf(x, y, dot); nt = fmaf(x, x, nt); nv = fmaf(y, y, nv);
  }
  dot = wave_sum(dot); nt = wave_sum(nt); nv = wave_sum(nv);
  if (lane == 0) out[row] = dot / fmaxf(sqrtf(nt) * sqrtf(nv), 1e-12f);
}

// ---------------------------------------------------------------- K15: cosine GEMV + top-k
// most_similar (reference src/backend.py:297-301: wv.most_similar(word, topn=50)) over a V x D
// word-vector table (V up to 3 M, D = 300).  No score vector goes to HBM and no library sort:
//  pass 1 (topk_partial_kernel): a block scores TK_CHUNK consecutive rows (one wave per row,
//         fp32 accumulation), keeps the scores in LDS as 64-bit keys {orderable(score), ~row},
//         bitonic-sorts them descending and writes its best k keys;
//  pass 2.. (topk_merge_kernel): the same sort over TK_CHUNK candidates per block until one
//         block is left, which decodes the k best into (score, row) -- torch.topk's outputs.
// The key order is total: equal scores rank the LOWER row first (deterministic ties).
constexpr int TK_CHUNK = 2048;
constexpr int TK_THREADS = 1024;

CM_DEVICE uint32_t f_orderable(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
CM_DEVICE float f_from_orderable(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
CM_DEVICE unsigned long long tk_key(float score, int row) {
  // score + 0.0f: -0.0 (an underflowing negative dot) is the same score as +0.0, the lower row first
  return ((unsigned long long)f_orderable(score + 0.0f) << 32) | (unsigned long long)(~(uint32_t)row);
}

// descending bitonic sort of TK_CHUNK keys in LDS by TK_THREADS threads (one pair each per step)
CM_DEVICE void tk_sort_desc(unsigned long long* s) {
  const int t = threadIdx.x;
  for (int size = 2; size <= TK_CHUNK; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int i = 2 * t - (t & (stride - 1));
      const int j = i + stride;
      const bool down = (i & size) == 0;          // this pair's run is sorted descending
      const unsigned long long a = s[i], b = s[j];
      if ((a < b) == down) { s[i] = b; s[j] = a; }
    }
  }
  __syncthreads();
}

template <bool TF32, bool VF32>
__global__ void __launch_bounds__(TK_THREADS) topk_partial_kernel(const void* __restrict__ table, int V, int D,
                                                                 const void* __restrict__ vec, int k,
                                                                 unsigned long long* __restrict__ cand) {
  __shared__ unsigned long long s[TK_CHUNK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int WAVES = TK_THREADS / 64, ROWS = TK_CHUNK / WAVES;
  float nv = 0.f;
  for (int c = lane; c < D; c += 64) { const float y = ld<VF32>(vec, c); nv = fmaf(y, y, nv); }
  nv = sqrtf(wave_sum(nv));
  const long long base = (long long)blockIdx.x * TK_CHUNK;
  for (int i = 0; i < ROWS; ++i) {
    const int slot = w * ROWS + i;
    const long long row = base + slot;
    unsigned long long key = 0ull;                 // below every real score: padding sorts last
    if (row < V) {
      float dot = 0.f, nt = 0.f;
      for (int c = lane; c < D; c += 64) {
        const float x = ld<TF32>(table, row * D + c), y = ld<VF32>(vec, c);
        dot = fmaf(x, y, dot); nt = fmaf(x, x, nt);
      }
      dot = wave_sum(dot); nt = wave_sum(nt);
      key = tk_key(dot / fmaxf(sqrtf(nt) * nv, 1e-12f), (int)row);
    }
    if (lane == 0) s[slot] = key;
  }
  tk_sort_desc(s);
  for (int j = threadIdx.x; j < k; j += TK_THREADS) cand[(long long)blockIdx.x * k + j] = s[j];
}

__global__ void __launch_bounds__(TK_THREADS) topk_merge_kernel(const unsigned long long* __restrict__ in, int n, int k,
                                                               unsigned long long* __restrict__ out,
                                                               float* __restrict__ vals, long long* __restrict__ idx) {
  __shared__ unsigned long long s[TK_CHUNK];
  const long long base = (long long)blockIdx.x * TK_CHUNK;
  for (int j = threadIdx.x; j < TK_CHUNK; j += TK_THREADS) s[j] = base + j < n ? in[base + j] : 0ull;
  tk_sort_desc(s);
  for (int j = threadIdx.x; j < k; j += TK_THREADS) {
    const unsigned long long key = s[j];
    if (vals != nullptr) {                         // last pass: decode (score, row)
      vals[j] = f_from_orderable((uint32_t)(key >> 32));
      idx[j] = (long long)(~(uint32_t)(key & 0xffffffffull));
    } else {
      out[(long long)blockIdx.x * k + j] = key;
    }
  }
}

__global__ void mean_pool_l2_kernel(const uint16_t* __restrict__ h, const int* __restrict__ lens,
                                    float* __restrict__ out, int T, int D) {
  extern __shared__ float buf[];   // [D] + [64]
  const int b = blockIdx.x;
  // lens > T clamps to T.  An empty row (lens <= 0) reads no token: its mean is 0 and the 1e-12
  // clamp below makes the output the zero vector, as ops/reference.py mean_pool_l2 (it used to
  // return the normalised first token, which is padding there)
  const int L = max(0, min(T, lens[b]));
  float* red = buf + D;
  float ss = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f;
    for (int t = 0; t < L; ++t) s += bf2f(h[((long long)b * T + t) * D + d]);
    s /= (float)max(L, 1);
    buf[d] = s;
    ss = fmaf(s, s, ss);
  }
  ss = wave_sum(ss);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) red[w] = ss;
  __syncthreads();
  float tot = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) tot += red[i];
  const float inv = 1.f / fmaxf(sqrtf(tot), 1e-12f);
  for (int d = threadIdx.x; d < D; d += blockDim.x) out[(long long)b * D + d] = buf[d] * inv;
}

template <bool U8>
__global__ void blur_h_kernel(const void* __restrict__ img, int H, int W, int C, const float* __restrict__ w,
                              int R, float* __restrict__ tmp) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long n = (long long)H * W * C;
  if (i >= n) return;
  int c = (int)(i % C);
  long long px = i / C;
  int x = (int)(px % W), y = (int)(px / W);
  float s = 0.f;
  for (int k = -R; k <= R; ++k) {
    int xx = min(max(x + k, 0), W - 1);
    long long j = ((long long)y * W + xx) * C + c;
    float v = U8 ? (float)reinterpret_cast<const uint8_t*>(img)[j] : reinterpret_cast<const float*>(img)[j];
    s = fmaf(w[k + R], v, s);
  }
  tmp[i] = s;
}

template <bool U8>
__global__ void blur_v_kernel(const float* __restrict__ tmp, int H, int W, int C, const float* __restrict__ w,
                              int R, void* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long n = (long long)H * W * C;
  if (i >= n) return;
  int c = (int)(i % C);
  long long px = i / C;
  int x = (int)(px % W), y = (int)(px / W);
  float s = 0.f;
  for (int k = -R; k <= R; ++k) {
    int yy = min(max(y + k, 0), H - 1);
    s = fmaf(w[k + R], tmp[((long long)yy * W + x) * C + c], s);
  }
  if (U8) reinterpret_cast<uint8_t*>(out)[i] = (uint8_t)fminf(fmaxf(rintf(s), 0.f), 255.f);
  else reinterpret_cast<float*>(out)[i] = s;
}

__global__ void to_uint8_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ out, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = bf2f(x[i]) * 0.5f + 0.5f;
  v = fminf(fmaxf(v, 0.f), 1.f) * 255.f;
  out[i] = (uint8_t)rintf(v);
}

__global__ void timestep_embedding_kernel(const float* __restrict__ t, void* __restrict__ out_, int B, int dim,
                                          int flip, float shift, int out_bf16) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int half = dim / 2;
  if (i >= B * half) return;
  int b = i / half, k = i % half;
  float ex = -logf(10000.f) * (float)k / ((float)half - shift);
  float arg = t[b] * expf(ex);
  float sv = sinf(arg), cv = cosf(arg);
  const float lo = flip ? cv : sv, hi = flip ? sv : cv;
  if (out_bf16) {     // the time MLP's input dtype directly (no separate cast launch)
    uint16_t* out = reinterpret_cast<uint16_t*>(out_);
    out[b * dim + k] = f2bf(lo);
    out[b * dim + half + k] = f2bf(hi);
  } else {
    float* out = reinterpret_cast<float*>(out_);
    out[b * dim + k] = lo;
    out[b * dim + half + k] = hi;
  }
}

// coefficient row layout: see models/schedulers.py
// Per-step time-conditioning rows: the next step's rows of up to two per-plan tables are copied
// into the fixed buffers the captured UNet reads (replaces an int->long cast + 2 index_select
// launches per step); these are extra blocks of the latent-step launch.
struct StepRows {
  const uint4* tab[2] = {nullptr, nullptr};
  uint4* buf[2] = {nullptr, nullptr};
  int row_units[2] = {0, 0};     // 16-byte units per row
  int rows = 0;                  // table rows (plan evals)
};

__global__ void latent_step_kernel(const uint16_t* __restrict__ eps, float* __restrict__ x,
                                   float* __restrict__ hist, float* __restrict__ xs,
                                   const float* __restrict__ coef, const int* __restrict__ step,
                                   uint16_t* __restrict__ unet_in, long long n, int cfg, int cin, int cstride,
                                   int latent_blocks, StepRows rows) {
  if ((int)blockIdx.x >= latent_blocks) {                   // next step's conditioning rows
    const int s = min(step[0] + 1, rows.rows - 1);
    const long long b = (long long)(blockIdx.x - latent_blocks) * blockDim.x + threadIdx.x;
    const long long tot0 = rows.row_units[0];
    if (b < tot0) {
      rows.buf[0][b] = rows.tab[0][(long long)s * tot0 + b];
    } else if (b - tot0 < rows.row_units[1]) {
      rows.buf[1][b - tot0] = rows.tab[1][(long long)s * rows.row_units[1] + (b - tot0)];
    }
    return;
  }
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = coef + 16 * step[0];
  float e;
  if (cfg) {
    float u = bf2f(eps[i]), c = bf2f(eps[n + i]);
    e = u + r[13] * (c - u);
  } else {
    e = bf2f(eps[i]);
  }
  float ep = r[0] * e;
  int s1 = (int)r[8], s2 = (int)r[9], s3 = (int)r[10], sv = (int)r[11];
  if (s1 >= 0) ep = fmaf(r[1], hist[(long long)s1 * n + i], ep);
  if (s2 >= 0) ep = fmaf(r[2], hist[(long long)s2 * n + i], ep);
  if (s3 >= 0) ep = fmaf(r[3], hist[(long long)s3 * n + i], ep);
  float xo = x[i];
  float xn = r[4] * xo + r[5] * xs[i] + r[6] * ep;
  if (sv >= 0) hist[(long long)sv * n + i] = e;
  if (r[12] > 0.f) xs[i] = xo;
  x[i] = xn;
  uint16_t o = f2bf(r[7] * xn);
  // the UNet input may be channel-padded (cstride 8 > cin 4: conv_in's K in whole 16-byte
  // chunks without a per-step pad copy); padding channels stay zero
  const long long ui = (i / cin) * cstride + (i % cin);
  const long long un = (n / cin) * cstride;
  unet_in[ui] = o;
  if (cfg) unet_in[un + ui] = o;
}

// latent_step for plans with stochastic rows (row column 15, ``noise``):
//     x = ax x + axs XS + b e' + r[15] z,   z ~ N(0, 1) by the NOISE CONTRACT of philox_normal.h
// One lane per latent pixel (cin == 4): its four channels are one 16-byte access of every fp32
// buffer and ONE Philox call.  r[15] != 0 is uniform over the launch (the row comes from the step
// counter), so a deterministic row of such a plan (its last) runs no Philox and reads no seed.
// ``seeds``: one 64-bit seed per image as (low, high) words; ``ppi``: pixels per image.
__global__ void latent_step_noise_kernel(const uint16_t* __restrict__ eps, float* __restrict__ x,
                                         float* __restrict__ hist, float* __restrict__ xs,
                                         const float* __restrict__ coef, const int* __restrict__ step,
                                         uint16_t* __restrict__ unet_in, long long npix, long long ppi, int cfg,
                                         int cstride, const uint2* __restrict__ seeds, int latent_blocks,
                                         StepRows rows) {
  if ((int)blockIdx.x >= latent_blocks) {                   // next step's conditioning rows, as above
    const int s = min(step[0] + 1, rows.rows - 1);
    const long long b = (long long)(blockIdx.x - latent_blocks) * blockDim.x + threadIdx.x;
    const long long tot0 = rows.row_units[0];
    if (b < tot0) {
      rows.buf[0][b] = rows.tab[0][(long long)s * tot0 + b];
    } else if (b - tot0 < rows.row_units[1]) {
      rows.buf[1][b - tot0] = rows.tab[1][(long long)s * rows.row_units[1] + (b - tot0)];
    }
    return;
  }
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  const int st = step[0];
  const float* r = coef + 16 * st;
  const uint2 pu = reinterpret_cast<const uint2*>(eps)[i];
  float e[4] = {__uint_as_float(pu.x << 16), __uint_as_float(pu.x & 0xffff0000u), __uint_as_float(pu.y << 16),
                __uint_as_float(pu.y & 0xffff0000u)};
  if (cfg) {
    const uint2 pc = reinterpret_cast<const uint2*>(eps)[npix + i];
    const float c[4] = {__uint_as_float(pc.x << 16), __uint_as_float(pc.x & 0xffff0000u),
                        __uint_as_float(pc.y << 16), __uint_as_float(pc.y & 0xffff0000u)};
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = e[k] + r[13] * (c[k] - e[k]);
  }
  float ep[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ep[k] = r[0] * e[k];
  float4* h4 = reinterpret_cast<float4*>(hist);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int sj = (int)r[8 + j];
    if (sj >= 0) {
      const float4 h = h4[(long long)sj * npix + i];
      ep[0] = fmaf(r[1 + j], h.x, ep[0]); ep[1] = fmaf(r[1 + j], h.y, ep[1]);
      ep[2] = fmaf(r[1 + j], h.z, ep[2]); ep[3] = fmaf(r[1 + j], h.w, ep[3]);
    }
  }
  const float4 xo = reinterpret_cast<float4*>(x)[i];
  const float4 xv = reinterpret_cast<float4*>(xs)[i];
  float xn[4] = {r[4] * xo.x + r[5] * xv.x + r[6] * ep[0], r[4] * xo.y + r[5] * xv.y + r[6] * ep[1],
                 r[4] * xo.z + r[5] * xv.z + r[6] * ep[2], r[4] * xo.w + r[5] * xv.w + r[6] * ep[3]};
  if (r[15] != 0.f) {
    const long long b = i / ppi;
    const uint2 seed = seeds[b];
    uint32_t w[4];
    float z[4];
    philox_normal4(seed.x, seed.y, (uint32_t)(i - b * ppi), (uint32_t)st, w, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) xn[k] = fmaf(r[15], z[k], xn[k]);
  }
  const int sv = (int)r[11];
  if (sv >= 0) h4[(long long)sv * npix + i] = make_float4(e[0], e[1], e[2], e[3]);
  if (r[12] > 0.f) reinterpret_cast<float4*>(xs)[i] = xo;
  reinterpret_cast<float4*>(x)[i] = make_float4(xn[0], xn[1], xn[2], xn[3]);
  // (channel-padded UNet input as in latent_step_kernel: channels 0..3 of a pixel of cstride)
  const uint2 o = make_uint2(pack2(r[7] * xn[0], r[7] * xn[1]), pack2(r[7] * xn[2], r[7] * xn[3]));
  *reinterpret_cast<uint2*>(unet_in + i * cstride) = o;
  if (cfg) *reinterpret_cast<uint2*>(unet_in + (npix + i) * cstride) = o;
}

__global__ void advance_step_kernel(int* step) { step[0] += 1; }

// ---- generation glue (one in-tree kernel each instead of ATen index / cat / cast / reduce
// launches around the captured denoise loop; verdict r2 "vendor/ATen kernels in the trace")

// out[r] = table[ids[r]] (+ pos[r % seq]), bf16 rows of D (D % 8 == 0), bf16-rounded add as the
// eager model does it (CLIP token + position embedding; row gathers: pooled EOS rows, the
// per-timestep repeat of SDXL's text embeddings)
__global__ void gather_add_kernel(const uint16_t* __restrict__ table, const int* __restrict__ ids,
                                  const uint16_t* __restrict__ pos, int seq, int D, long long rows,
                                  uint16_t* __restrict__ out) {
  const int V = D / 8;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * V) return;
  const long long r = i / V;
  const int v = (int)(i - r * V);
  uint4 a = reinterpret_cast<const uint4*>(table + (long long)ids[r] * D)[v];
  if (pos != nullptr) {
    float x[8], y[8];
    unpack8(a, x);
    unpack8(reinterpret_cast<const uint4*>(pos + (long long)(r % seq) * D)[v], y);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] += y[k];
    a = pack8(x);
  }
  reinterpret_cast<uint4*>(out + r * D)[v] = a;
}

// out[r] = [a[r] | b[r]] (bf16; b bf16 or fp32 -> bf16): SDXL's two text-encoder contexts and
// its add-embedding input, no torch.cat
__global__ void concat2_kernel(const uint16_t* __restrict__ a, int Da, const void* __restrict__ b, int Db, int b_f32,
                               long long rows, uint16_t* __restrict__ out) {
  const int Va = Da / 8, Vb = Db / 8, V = Va + Vb;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * V) return;
  const long long r = i / V;
  const int v = (int)(i - r * V);
  uint4 o;
  if (v < Va) {
    o = reinterpret_cast<const uint4*>(a + r * Da)[v];
  } else if (b_f32) {
    const float4* src = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(b) + r * Db + (v - Va) * 8);
    const float4 p0 = src[0], p1 = src[1];
    const float f[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
    o = pack8(f);
  } else {
    o = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(b) + r * Db)[v - Va];
  }
  reinterpret_cast<uint4*>(out + r * (Da + Db))[v] = o;
}

// in-place SiLU of bf16 (computed in fp32): the UNet time embedding after its add-embedding
__global__ void silu_bf16_kernel(uint16_t* __restrict__ x, long long n8) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  float f[8];
  unpack8(reinterpret_cast<uint4*>(x)[i], f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // below -80 exp(-x) leaves fp32's range (x / inf = -0.0 from -88.8 down) while x e^x is still a
    // bf16 value down to -97: there 1 + e^x == 1 in fp32, and expf keeps the denormal e^x
    f[k] = f[k] < -80.f ? f[k] * expf(f[k]) : f[k] / (1.f + __expf(-f[k]));
  }
  reinterpret_cast<uint4*>(x)[i] = pack8(f);
}

// start of a generation: fp32 master latents x = x0, xs = hist = 0, and the first UNet input
// (both CFG halves) = bf16(c_in0 * x0) in the channel-padded layout of latent_step (padding
// channels untouched: they are zero from allocation)
__global__ void latent_init_kernel(const float* __restrict__ x0, float c_in0, float* __restrict__ x,
                                   float* __restrict__ xs, float* __restrict__ hist, int nhist,
                                   uint16_t* __restrict__ unet_in, long long n, int cfg, int cin, int cstride) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x0[i];
  x[i] = v;
  xs[i] = 0.f;
  for (int k = 0; k < nhist; ++k) hist[(long long)k * n + i] = 0.f;
  const uint16_t o = f2bf(c_in0 * v);
  const long long ui = (i / cin) * cstride + (i % cin);
  unet_in[ui] = o;
  if (cfg) unet_in[(n / cin) * cstride + ui] = o;
}

// end of the denoise loop: bf16 copy of the fp32 latents for the VAE, and a device flag that
// is 1 iff every latent is finite.  ONE block (the latents are 64-256K floats: a few us on one
// CU) so the flag is written once, from the block-wide vote -- no memset node before it
__global__ void __launch_bounds__(1024) finalize_latents_kernel(const float* __restrict__ x, uint16_t* __restrict__ z,
                                                                long long n, uint8_t* __restrict__ finite) {
  int bad = 0;
  const long long n4 = n / 4;
  for (long long i = threadIdx.x; i < n4; i += blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<uint2*>(z)[i] = make_uint2(pack2(v.x, v.y), pack2(v.z, v.w));
    bad |= !isfinite(v.x) | !isfinite(v.y) | !isfinite(v.z) | !isfinite(v.w);
  }
  for (long long i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
    z[i] = f2bf(x[i]);
    bad |= !isfinite(x[i]);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) finite[0] = bad ? 0 : 1;
}

// zero-fill with 16-byte vector stores (the GroupNorm statistics slab cleared at the start of
// every captured UNet step; was an ATen fill kernel inside the graph)
__global__ void zero_kernel(uint4* __restrict__ p, long long n16, uint8_t* __restrict__ tail, int ntail) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16) p[i] = make_uint4(0, 0, 0, 0);
  if (i < ntail) tail[i] = 0;
}

// cache warm-up: read one dword per 64-B segment of [p, p + bytes) so the lines sit in the
// memory-side cache (MALL) and the issuing XCD's L2 when a later kernel reads them (the next
// layer's weights, read while the current layer runs on another stream).  The loads feed an
// XOR whose result is stored only if it equals a value it never takes in practice (keeps the
// loads alive without a store per line).
__global__ void __launch_bounds__(256) prefetch_kernel(const uint32_t* __restrict__ p, long long nseg, int stride,
                                                       uint32_t* __restrict__ sink) {
  uint32_t acc = 0;
  const long long n = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll 4
  for (; i < nseg; i += n) acc ^= p[i * stride] + (uint32_t)i;
  if (acc == 0x9E3779B9u) sink[0] = acc;
}

// device-to-device copy with 16-byte vector accesses (the per-generation refills of a captured
// step's input buffers: text context, time-table rows, add-embeds; was a runtime blit kernel)
__global__ void copy16_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, long long n16,
                              const uint8_t* __restrict__ stail, uint8_t* __restrict__ dtail, int ntail) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16) dst[i] = src[i];
  if (i < ntail) dtail[i] = stail[i];
}

// row softmax with optional causal / key-length mask (S fp32 [rows][cols] -> P bf16)
__global__ void softmax_rows_kernel(const float* __restrict__ S, uint16_t* __restrict__ P, int cols, int Nq,
                                    int causal, const int* __restrict__ kv_lens) {
  __shared__ float red[16];
  const long long row = blockIdx.x;
  const int qi = (int)(row % Nq);
  const int b = (int)(row / Nq);
  int lim = cols;
  if (kv_lens) lim = min(lim, kv_lens[b]);
  if (causal) lim = min(lim, qi + 1);
  const float* s = S + row * cols;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < lim; j += blockDim.x) mx = fmaxf(mx, s[j]);
  mx = wave_max(mx);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = -INFINITY;
  for (int i = 0; i < nw; ++i) mx = fmaxf(mx, red[i]);
  __syncthreads();
  float sum = 0.f;
  for (int j = threadIdx.x; j < lim; j += blockDim.x) sum += __expf(s[j] - mx);
  sum = wave_sum(sum);
  if (lane == 0) red[w] = sum;
  __syncthreads();
  sum = 0.f;
  for (int i = 0; i < nw; ++i) sum += red[i];
  const float inv = 1.f / sum;
  for (int j = threadIdx.x; j < cols; j += blockDim.x)
    P[row * cols + j] = f2bf(j < lim ? __expf(s[j] - mx) * inv : 0.f);
}

inline unsigned nblk(long long n, int t) { return (unsigned)((n + t - 1) / t); }

}  // namespace

void launch_gather_cosine(const void* table, int table_f32, int D, const int* ia, const int* ib, float* out,
                          int n, hipStream_t s) {
  if (n <= 0) return;
  if (table_f32) hipLaunchKernelGGL(gather_cosine_kernel<true>, dim3(nblk(n, 4)), dim3(256), 0, s, table, D, ia, ib, out, n);
  else hipLaunchKernelGGL(gather_cosine_kernel<false>, dim3(nblk(n, 4)), dim3(256), 0, s, table, D, ia, ib, out, n);
}

void launch_pair_cosine(const float* a, const float* b, int D, float* out, int n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(pair_cosine_kernel, dim3(nblk(n, 4)), dim3(256), 0, s, a, b, D, out, n);
}

void launch_cosine_gemv(const void* table, int table_f32, int V, int D, const void* vec, int vec_f32, float* out,
                        hipStream_t s) {
  dim3 g(nblk(V, 4));
  if (table_f32 && vec_f32) hipLaunchKernelGGL((cosine_gemv_kernel<true, true>), g, dim3(256), 0, s, table, V, D, vec, out);
  else if (table_f32) hipLaunchKernelGGL((cosine_gemv_kernel<true, false>), g, dim3(256), 0, s, table, V, D, vec, out);
  else if (vec_f32) hipLaunchKernelGGL((cosine_gemv_kernel<false, true>), g, dim3(256), 0, s, table, V, D, vec, out);
  else hipLaunchKernelGGL((cosine_gemv_kernel<false, false>), g, dim3(256), 0, s, table, V, D, vec, out);
}

int cosine_topk_workspace(int V, int k) {
  // keys held at once: pass-1 output plus the largest merge output (ping-pong halves)
  const long long n1 = (long long)((V + TK_CHUNK - 1) / TK_CHUNK) * k;
  const long long n2 = (long long)((n1 + TK_CHUNK - 1) / TK_CHUNK) * k;
  return (int)(n1 + n2);
}

void launch_cosine_topk(const void* table, int table_f32, int V, int D, const void* vec, int vec_f32, int k,
                        unsigned long long* ws, float* vals, long long* idx, hipStream_t s) {
  const int g1 = (V + TK_CHUNK - 1) / TK_CHUNK;
  if (table_f32 && vec_f32) hipLaunchKernelGGL((topk_partial_kernel<true, true>), dim3(g1), dim3(TK_THREADS), 0, s, table, V, D, vec, k, ws);
  else if (table_f32) hipLaunchKernelGGL((topk_partial_kernel<true, false>), dim3(g1), dim3(TK_THREADS), 0, s, table, V, D, vec, k, ws);
  else if (vec_f32) hipLaunchKernelGGL((topk_partial_kernel<false, true>), dim3(g1), dim3(TK_THREADS), 0, s, table, V, D, vec, k, ws);
  else hipLaunchKernelGGL((topk_partial_kernel<false, false>), dim3(g1), dim3(TK_THREADS), 0, s, table, V, D, vec, k, ws);
  long long n = (long long)g1 * k;
  unsigned long long* cur = ws;
  unsigned long long* nxt = ws + n;               // second half: every later pass fits (k < TK_CHUNK / 2)
  while (true) {
    const int g = (int)((n + TK_CHUNK - 1) / TK_CHUNK);
    if (g == 1) {
      hipLaunchKernelGGL(topk_merge_kernel, dim3(1), dim3(TK_THREADS), 0, s, cur, (int)n, k, nullptr, vals, idx);
      return;
    }
    hipLaunchKernelGGL(topk_merge_kernel, dim3(g), dim3(TK_THREADS), 0, s, cur, (int)n, k, nxt, nullptr, nullptr);
    n = (long long)g * k;
    unsigned long long* t = cur; cur = nxt; nxt = t;
  }
}

void launch_mean_pool_l2(const uint16_t* h, const int* lens, float* out, int B, int T, int D, hipStream_t s) {
  hipLaunchKernelGGL(mean_pool_l2_kernel, dim3(B), dim3(256), (D + 64) * sizeof(float), s, h, lens, out, T, D);
}

constexpr int BLUR_TS = 32;
constexpr int BLUR_MAXR = 48;

CM_DEVICE int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int C>
__global__ void __launch_bounds__(256) blur_tile_kernel(const uint8_t* __restrict__ img, int H, int W,
                                                        const float* __restrict__ w, int R, uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char blur_sm[];
  const int E = BLUR_TS + 2 * R;                               // staged tile edge (with halo)
  uint8_t* tin = blur_sm;                                      // [E][E][C] u8
  float* mid = reinterpret_cast<float*>(blur_sm + ((E * E * C + 15) & ~15));   // [E][TS][C]
  float* ws = mid + E * BLUR_TS * C;                           // [2R+1]
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * BLUR_TS - R, y0 = blockIdx.y * BLUR_TS - R;
  for (int i = tid; i < 2 * R + 1; i += 256) ws[i] = w[i];
  for (int i = tid; i < E * E; i += 256) {
    const int r = i / E, c = i - r * E;
    const int gy = clampi(y0 + r, 0, H - 1), gx = clampi(x0 + c, 0, W - 1);   // edge clamp
    const uint8_t* src = img + ((long long)gy * W + gx) * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) tin[i * C + ch] = src[ch];
  }
  __syncthreads();
  for (int i = tid; i < E * BLUR_TS; i += 256) {              // horizontal pass -> LDS f32
    const int r = i / BLUR_TS, j = i - r * BLUR_TS;
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.f;
    const uint8_t* row = tin + (r * E + j) * C;
    for (int k = 0; k <= 2 * R; ++k) {
      const float wk = ws[k];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) acc[ch] = fmaf(wk, (float)row[k * C + ch], acc[ch]);
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) mid[i * C + ch] = acc[ch];
  }
  __syncthreads();
  for (int i = tid; i < BLUR_TS * BLUR_TS; i += 256) {        // vertical pass -> uint8
    const int r = i / BLUR_TS, j = i - r * BLUR_TS;
    const int gy = blockIdx.y * BLUR_TS + r, gx = blockIdx.x * BLUR_TS + j;
    if (gy >= H || gx >= W) continue;
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.f;
    for (int k = 0; k <= 2 * R; ++k) {
      const float wk = ws[k];
      const float* m = mid + ((r + k) * BLUR_TS + j) * C;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) acc[ch] = fmaf(wk, m[ch], acc[ch]);
    }
    uint8_t* dst = out + ((long long)gy * W + gx) * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) dst[ch] = (uint8_t)fminf(fmaxf(rintf(acc[ch]), 0.f), 255.f);
  }
}

template <int C>
void launch_blur_tile(const uint8_t* img, int H, int W, const float* w, int R, uint8_t* out, hipStream_t s) {
  const int E = BLUR_TS + 2 * R;
  const size_t lds = ((size_t)(E * E * C + 15) & ~(size_t)15) + sizeof(float) * ((size_t)E * BLUR_TS * C + 2 * R + 1);
  // up to ~99 KiB at R = 48 (first call happens outside any graph capture; thread-safe once)
  static const bool once = [] {
    (void)hipFuncSetAttribute((const void*)&blur_tile_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(((size_t)(BLUR_TS + 2 * BLUR_MAXR) * (BLUR_TS + 2 * BLUR_MAXR) * C + 15 & ~(size_t)15) +
                                    sizeof(float) * ((size_t)(BLUR_TS + 2 * BLUR_MAXR) * BLUR_TS * C + 2 * BLUR_MAXR + 1)));
    return true;
  }();
  (void)once;
  dim3 grid((W + BLUR_TS - 1) / BLUR_TS, (H + BLUR_TS - 1) / BLUR_TS);
  hipLaunchKernelGGL(blur_tile_kernel<C>, grid, dim3(256), lds, s, img, H, W, w, R, out);
}

void launch_gaussian_blur(const void* img, int u8, int H, int W, int C, const float* w, int R, float* tmp,
                          void* out, hipStream_t s) {
  long long n = (long long)H * W * C;
  if (u8 && R <= BLUR_MAXR && (C == 1 || C == 3 || C == 4)) {
    const uint8_t* im = reinterpret_cast<const uint8_t*>(img);
    uint8_t* o = reinterpret_cast<uint8_t*>(out);
    if (C == 3) launch_blur_tile<3>(im, H, W, w, R, o, s);
    else if (C == 4) launch_blur_tile<4>(im, H, W, w, R, o, s);
    else launch_blur_tile<1>(im, H, W, w, R, o, s);
    return;
  }
  if (u8) {
    hipLaunchKernelGGL(blur_h_kernel<true>, dim3(nblk(n, 256)), dim3(256), 0, s, img, H, W, C, w, R, tmp);
    hipLaunchKernelGGL(blur_v_kernel<true>, dim3(nblk(n, 256)), dim3(256), 0, s, tmp, H, W, C, w, R, out);
  } else {
    hipLaunchKernelGGL(blur_h_kernel<false>, dim3(nblk(n, 256)), dim3(256), 0, s, img, H, W, C, w, R, tmp);
    hipLaunchKernelGGL(blur_v_kernel<false>, dim3(nblk(n, 256)), dim3(256), 0, s, tmp, H, W, C, w, R, out);
  }
}

void launch_to_uint8(const uint16_t* x, uint8_t* out, long long n, hipStream_t s) {
  hipLaunchKernelGGL(to_uint8_kernel, dim3(nblk(n, 256)), dim3(256), 0, s, x, out, n);
}

void launch_timestep_embedding(const float* t, void* out, int B, int dim, int flip, float shift, int out_bf16,
                               hipStream_t s) {
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(nblk((long long)B * dim / 2, 256)), dim3(256), 0, s, t, out, B,
                     dim, flip, shift, out_bf16);
}

void launch_gather_add(const uint16_t* table, const int* ids, const uint16_t* pos, int seq, int D, long long rows,
                       uint16_t* out, hipStream_t s) {
  hipLaunchKernelGGL(gather_add_kernel, dim3(nblk(rows * (D / 8), 256)), dim3(256), 0, s, table, ids, pos, seq, D,
                     rows, out);
}

void launch_concat2(const uint16_t* a, int Da, const void* b, int Db, int b_f32, long long rows, uint16_t* out,
                    hipStream_t s) {
  hipLaunchKernelGGL(concat2_kernel, dim3(nblk(rows * ((Da + Db) / 8), 256)), dim3(256), 0, s, a, Da, b, Db, b_f32,
                     rows, out);
}

void launch_silu_bf16(uint16_t* x, long long n, hipStream_t s) {
  hipLaunchKernelGGL(silu_bf16_kernel, dim3(nblk(n / 8, 256)), dim3(256), 0, s, x, n / 8);
}

void launch_latent_init(const float* x0, float c_in0, float* x, float* xs, float* hist, int nhist, uint16_t* unet_in,
                        long long n, int cfg, int cin, int cstride, hipStream_t s) {
  hipLaunchKernelGGL(latent_init_kernel, dim3(nblk(n, 256)), dim3(256), 0, s, x0, c_in0, x, xs, hist, nhist, unet_in,
                     n, cfg, cin, cstride);
}

void launch_finalize_latents(const float* x, uint16_t* z, long long n, uint8_t* finite, hipStream_t s) {
  hipLaunchKernelGGL(finalize_latents_kernel, dim3(1), dim3(1024), 0, s, x, z, n, finite);
}

void launch_latent_step(const uint16_t* eps, float* x, float* hist, float* xs, const float* coef, const int* step,
                        uint16_t* unet_in, long long n, int cfg, int cin, int cstride, const void* tab0, void* buf0,
                        long long row_bytes0, const void* tab1, void* buf1, long long row_bytes1, int rows,
                        const void* seeds, int images, hipStream_t s) {
  StepRows r;
  r.tab[0] = reinterpret_cast<const uint4*>(tab0); r.buf[0] = reinterpret_cast<uint4*>(buf0);
  r.tab[1] = reinterpret_cast<const uint4*>(tab1); r.buf[1] = reinterpret_cast<uint4*>(buf1);
  r.row_units[0] = tab0 ? (int)(row_bytes0 / 16) : 0;
  r.row_units[1] = tab1 ? (int)(row_bytes1 / 16) : 0;
  r.rows = rows;
  const int cb = (int)nblk((long long)r.row_units[0] + r.row_units[1], 256);
  if (seeds != nullptr) {           // a plan with stochastic rows: one lane per pixel (cin == 4)
    const long long npix = n / 4;
    const int lb = (int)nblk(npix, 256);
    hipLaunchKernelGGL(latent_step_noise_kernel, dim3(lb + cb), dim3(256), 0, s, eps, x, hist, xs, coef, step,
                       unet_in, npix, npix / images, cfg, cstride, reinterpret_cast<const uint2*>(seeds), lb, r);
    return;
  }
  const int lb = (int)nblk(n, 256);
  hipLaunchKernelGGL(latent_step_kernel, dim3(lb + cb), dim3(256), 0, s, eps, x, hist, xs, coef, step, unet_in, n,
                     cfg, cin, cstride, lb, r);
}

void launch_zero(void* p, long long bytes, hipStream_t s) {
  const long long n16 = bytes / 16;
  const int ntail = (int)(bytes - n16 * 16);
  const long long n = n16 > ntail ? n16 : ntail;
  if (n == 0) return;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<uint4*>(p), n16,
                     reinterpret_cast<uint8_t*>(p) + n16 * 16, ntail);
}

void launch_prefetch(const void* p, long long bytes, int blocks, void* sink, hipStream_t s) {
  const long long nseg = bytes / 64;
  if (nseg == 0) return;
  const long long want = (nseg + 255) / 256;
  const unsigned nb = (unsigned)(want < blocks ? want : blocks);
  hipLaunchKernelGGL(prefetch_kernel, dim3(nb), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(p), nseg, 16,
                     reinterpret_cast<uint32_t*>(sink));
}

void launch_copy(const void* src, void* dst, long long bytes, hipStream_t s) {
  const long long n16 = bytes / 16;
  const int ntail = (int)(bytes - n16 * 16);
  const long long n = n16 > ntail ? n16 : ntail;
  if (n == 0) return;
  hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), n16,
                     reinterpret_cast<const uint8_t*>(src) + n16 * 16, reinterpret_cast<uint8_t*>(dst) + n16 * 16, ntail);
}

void launch_advance_step(int* step, hipStream_t s) {
  hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(1), 0, s, step);
}

void launch_softmax_rows(const float* S, uint16_t* P, int rows, int cols, int Nq, int causal, const int* kv_lens,
                         hipStream_t s) {
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, s, S, P, cols, Nq, causal, kv_lens);
}
