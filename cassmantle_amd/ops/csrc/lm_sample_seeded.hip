// Batched decode-step sampler whose Gumbel noise is drawn in the kernel (gfx950).
//
// lm_sample_kernel (lm.hip) serves one sequence and reads its noise from a [steps, 1, V] table the
// host draws and uploads before every call.  Here one workgroup serves one row of a batch of up to
// 8 sequences and draws the noise itself, by the GUMBEL CONTRACT of philox_gumbel.h: keyed by the
// row's own 64-bit seed and its own step counter, so a sequence samples the same tokens alone, in
// any row of any batch and next to any other sequences, and nothing is uploaded.
//
// * lm_sample_seeded_kernel: per row b (blockIdx.x): v = logit / T (+ eos_bias[step_b] at eos, -0.0
//   turned into +0.0), the top-k set by the 4-pass 8-bit radix select of lm_sample_kernel on
//   order-preserving float keys (ties at the k-th value: the lower ids), Gumbel-max over the set
//   with g(S_b, step_b, id) (ties: larger v, then lower id), then the row's state update:
//   out[step_b, b] = tok[b] = id; pos[b], lens[b], step[b] += 1.  Philox runs for the members of
//   the set only (k calls per row, not V).  Every row owns its step counter: with one shared
//   counter some workgroups would read it after another had advanced it.
// * lm_gumbel_kernel: the noise alone, out[b, j] = g(S_b, step, ids[j]), for tests.
//
// lm.hip is not touched: its kernels compile to the instructions they had.
#include "common.h"
#include "kernels.h"
#include "philox_gumbel.h"

namespace {

constexpr int SEEDED_THREADS = 1024;
constexpr int SEEDED_WAVES = SEEDED_THREADS / 64;

CM_DEVICE unsigned seeded_fkey(float f) {           // order-preserving float -> uint32
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (score, value, id) order of the Gumbel-max: larger score, then larger value, then lower id
CM_DEVICE bool seeded_better(float s, float v, int i, float bs, float bv, int bi) {
  return s > bs || (s == bs && (v > bv || (v == bv && i < bi)));
}

template <bool F32>
__global__ void __launch_bounds__(SEEDED_THREADS) lm_sample_seeded_kernel(LmSampleSeededArgs a) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_rem, s_eq, s_cut;
  __shared__ unsigned wcnt[SEEDED_WAVES];
  __shared__ float r_sc[SEEDED_WAVES], r_v[SEEDED_WAVES];
  __shared__ int r_id[SEEDED_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int V = a.V;
  const long long step = a.step[b];
  // a row past its table (the host sizes out / eos_bias for the call) neither reads nor writes
  if (step < 0 || step >= a.steps || V <= 0) return;
  const float eb = a.eos_bias[step];
  const long long row = (long long)b * a.ld;
  const float temp = a.temp;
  const int eos = a.eos;
  auto value = [&](int i) -> float {
    const float l = F32 ? reinterpret_cast<const float*>(a.logits)[row + i]
                        : bf2f(reinterpret_cast<const uint16_t*>(a.logits)[row + i]);
    float v = l / temp;
    if (i == eos) v += eb;
    return v + 0.0f;                                // -0.0 -> +0.0, every other v unchanged
  };
  // ---- radix select of the k-th largest key, 8 bits per pass from the top
  unsigned prefix = 0, mask = 0, rem = (unsigned)min(a.k, V);
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += SEEDED_THREADS) {
      const unsigned key = seeded_fkey(value(i));
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned above = 0;
      int d = 255;
      for (; d > 0; --d) {                         // digits from the top until rem is reached
        if (above + hist[d] >= rem) break;
        above += hist[d];
      }
      s_prefix = prefix | ((unsigned)d << shift);
      s_rem = rem - above;
      s_eq = hist[d];                              // after the last pass: keys equal to the k-th
      if (shift == 0) s_cut = 0x7fffffffu;
    }
    __syncthreads();
    prefix = s_prefix;
    rem = s_rem;
    mask |= 255u << shift;
  }
  // ---- ties at the k-th key: keep the `rem` lowest ids (only when more keys equal it)
  if (s_eq > rem) {                                // block-uniform: s_eq is read after the barrier
    unsigned need = rem;
    for (int base = 0; base < V; base += SEEDED_THREADS) {
      const int i = base + tid;
      const bool eq = i < V && seeded_fkey(value(i)) == prefix;
      const unsigned long long bal = __ballot(eq);
      if (lane == 0) wcnt[wave] = (unsigned)__popcll(bal);
      __syncthreads();
      unsigned before = 0, total = 0;
#pragma unroll
      for (int j = 0; j < SEEDED_WAVES; ++j) {
        const unsigned c = wcnt[j];
        if (j < wave) before += c;
        total += c;
      }
      const unsigned rank = before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
      if (eq && rank == need - 1) s_cut = (unsigned)i;   // the last tied id that is kept
      __syncthreads();
      if (total >= need) break;
      need -= total;
    }
  }
  const unsigned cut = s_cut;
  // ---- Gumbel-max over the top-k set: Philox for its members only
  const unsigned long long seed = (unsigned long long)a.seeds[b];
  const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32), st = (uint32_t)step;
  float best = -INFINITY, bv = -INFINITY;
  int bid = 0x7fffffff;
  for (int i = tid; i < V; i += SEEDED_THREADS) {
    const float v = value(i);
    const unsigned key = seeded_fkey(v);
    if (key > prefix || (key == prefix && (unsigned)i <= cut)) {
      const float sc = v + philox_gumbel(seed_lo, seed_hi, (uint32_t)i, st);
      if (seeded_better(sc, v, i, best, bv, bid)) { best = sc; bv = v; bid = i; }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64), ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bid, o, 64);
    if (seeded_better(ob, ov, oi, best, bv, bid)) { best = ob; bv = ov; bid = oi; }
  }
  if (lane == 0) { r_sc[wave] = best; r_v[wave] = bv; r_id[wave] = bid; }
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < SEEDED_WAVES; ++j)
      if (seeded_better(r_sc[j], r_v[j], r_id[j], best, bv, bid)) { best = r_sc[j]; bv = r_v[j]; bid = r_id[j]; }
    a.out[step * a.B + b] = bid;
    a.tok[b] = bid;
    a.pos[b] += 1;
    a.lens[b] += 1;
    a.step[b] = step + 1;
  }
}

__global__ void lm_gumbel_kernel(const long long* __restrict__ seeds, uint32_t step, const long long* __restrict__ ids,
                                 int n, int B, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * n) return;
  const int b = (int)(t / n), j = (int)(t - (long long)b * n);
  const unsigned long long seed = (unsigned long long)seeds[b];
  out[t] = philox_gumbel((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)ids[j], step);
}

}  // namespace

void launch_lm_sample_seeded(const LmSampleSeededArgs& a, int logits_f32, hipStream_t s) {
  if (a.B <= 0) return;
  if (logits_f32) hipLaunchKernelGGL(lm_sample_seeded_kernel<true>, dim3(a.B), dim3(SEEDED_THREADS), 0, s, a);
  else hipLaunchKernelGGL(lm_sample_seeded_kernel<false>, dim3(a.B), dim3(SEEDED_THREADS), 0, s, a);
}

void launch_lm_gumbel(const long long* seeds, unsigned step, const long long* ids, int n, int B, float* out,
                      hipStream_t s) {
  const long long total = (long long)B * n;
  if (total <= 0) return;
  hipLaunchKernelGGL(lm_gumbel_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, seeds, step, ids, n, B,
                     out);
}
