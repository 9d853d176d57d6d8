// The LM decode step's sampler (gfx950): ONE launch, one workgroup per row, instead of ATen topk +
// gather + argmax + index_copy inside the captured decode graph.
//
// Contract (ops/reference.py lm_sample / lm_sample_seeded), per row b with its own step counter:
// v = logit / T (+ eos_bias[step_b] at eos); the k largest v by a 4-pass 8-bit radix select on
// order-preserving float keys (ties at the k-th value: the LOWER ids); among them the id maximising
// v + noise(id) (ties: larger v, then lower id); then out[step_b, b] = tok[b] = id and pos[b],
// lens[b], step[b] += 1.  -0.0 and +0.0 are one value, as in the reference's stable sort: value()
// turns -0.0 into +0.0, so the radix keys, the tie cut and the Gumbel comparison see one zero (fkey
// alone would rank -0.0 strictly below +0.0).
//
// One core (sample_row), two noise models, two kernel names:
// * lm_sample_kernel: batch 1, the noise is row `step` of a [steps, 1, V] table the host draws and
//   uploads before every call.
// * lm_sample_seeded_kernel: up to 8 rows, the noise is drawn here by the GUMBEL CONTRACT of
//   philox_gumbel.h, keyed by the row's own 64-bit seed and its own step counter, so a sequence
//   samples the same tokens alone, in any row of any batch and next to any other sequences, and
//   nothing is uploaded.  Philox runs for the members of the top-k set only (k calls per row, not
//   V).  Every row owns its step counter: with one shared counter some workgroups would read it
//   after another had advanced it.
// * lm_gumbel_kernel: the noise alone, out[b, j] = g(S_b, step, ids[j]), for tests.
#include "common.h"
#include "kernels.h"
#include "philox_gumbel.h"

namespace {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;

CM_DEVICE unsigned fkey(float f) {                  // order-preserving float -> uint32
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (score, value, id) order of the Gumbel-max: larger score, then larger value, then lower id
CM_DEVICE bool better(float s, float v, int i, float bs, float bv, int bi) {
  return s > bs || (s == bs && (v > bv || (v == bv && i < bi)));
}

// the noise of vocabulary id i at one row's step: a row of the host's table, or Philox
struct TableNoise {
  const float* g;
  CM_DEVICE float operator()(int i) const { return g[i]; }
};
struct PhiloxNoise {
  uint32_t seed_lo, seed_hi, step;
  CM_DEVICE float operator()(int i) const { return philox_gumbel(seed_lo, seed_hi, (uint32_t)i, step); }
};

// a row past its table (the host sizes out / eos_bias / the noise table for the call) neither
// reads nor writes
CM_DEVICE bool row_finished(const LmSampleArgs& a, long long step) { return step < 0 || step >= a.steps || a.V <= 0; }

template <bool F32, class Noise>
CM_DEVICE void sample_row(const LmSampleArgs& a, int b, long long step, Noise noise) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_rem, s_eq, s_cut;
  __shared__ unsigned wcnt[SAMPLE_WAVES];
  __shared__ float r_sc[SAMPLE_WAVES], r_v[SAMPLE_WAVES];
  __shared__ int r_id[SAMPLE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
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
    for (int i = tid; i < V; i += SAMPLE_THREADS) {
      const unsigned key = fkey(value(i));
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
      if (shift == 0) s_cut = 0x7fffffffu;          // ordered before every later read by the barrier below
    }
    __syncthreads();
    prefix = s_prefix;
    rem = s_rem;
    mask |= 255u << shift;
  }
  // ---- ties at the k-th key: keep the `rem` lowest ids (only when more keys equal it)
  if (s_eq > rem) {                                // block-uniform: s_eq is read after the barrier
    unsigned need = rem;                           // >= 1 throughout: the loop ends once it is covered
    for (int base = 0; base < V; base += SAMPLE_THREADS) {
      const int i = base + tid;
      const bool eq = i < V && fkey(value(i)) == prefix;
      const unsigned long long bal = __ballot(eq);
      if (lane == 0) wcnt[wave] = (unsigned)__popcll(bal);
      __syncthreads();
      unsigned before = 0, total = 0;
#pragma unroll
      for (int j = 0; j < SAMPLE_WAVES; ++j) {
        const unsigned c = wcnt[j];
        if (j < wave) before += c;
        total += c;
      }
      const unsigned rank = before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
      if (eq && rank == need - 1) s_cut = (unsigned)i;   // the last tied id that is kept
      __syncthreads();                             // orders s_cut before its read and wcnt's reuse
      if (total >= need) break;
      need -= total;
    }
  }
  const unsigned cut = s_cut;
  // ---- Gumbel-max over the top-k set: the noise is asked for its members only
  float best = -INFINITY, bv = -INFINITY;
  int bid = 0x7fffffff;
  for (int i = tid; i < V; i += SAMPLE_THREADS) {
    const float v = value(i);
    const unsigned key = fkey(v);
    if (key > prefix || (key == prefix && (unsigned)i <= cut)) {
      const float sc = v + noise(i);
      if (better(sc, v, i, best, bv, bid)) { best = sc; bv = v; bid = i; }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64), ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bid, o, 64);
    if (better(ob, ov, oi, best, bv, bid)) { best = ob; bv = ov; bid = oi; }
  }
  if (lane == 0) { r_sc[wave] = best; r_v[wave] = bv; r_id[wave] = bid; }
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < SAMPLE_WAVES; ++j)
      if (better(r_sc[j], r_v[j], r_id[j], best, bv, bid)) { best = r_sc[j]; bv = r_v[j]; bid = r_id[j]; }
    a.out[step * a.B + b] = bid;
    a.tok[b] = bid;
    a.pos[b] += 1;
    a.lens[b] += 1;
    a.step[b] = step + 1;
  }
}

template <bool F32>
__global__ void __launch_bounds__(SAMPLE_THREADS) lm_sample_kernel(LmSampleArgs a) {
  const long long step = a.step[0];
  if (row_finished(a, step)) return;
  sample_row<F32>(a, 0, step, TableNoise{a.noise + step * (long long)a.V});
}

template <bool F32>
__global__ void __launch_bounds__(SAMPLE_THREADS) lm_sample_seeded_kernel(LmSampleArgs a) {
  const int b = blockIdx.x;
  const long long step = a.step[b];
  if (row_finished(a, step)) return;
  const unsigned long long seed = (unsigned long long)a.seeds[b];
  sample_row<F32>(a, b, step, PhiloxNoise{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step});
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

void launch_lm_sample(const LmSampleArgs& a, int logits_f32, hipStream_t s) {
  if (a.B <= 0) return;
  const auto kernel = a.noise ? (logits_f32 ? lm_sample_kernel<true> : lm_sample_kernel<false>)
                              : (logits_f32 ? lm_sample_seeded_kernel<true> : lm_sample_seeded_kernel<false>);
  hipLaunchKernelGGL(kernel, dim3(a.noise ? 1 : a.B), dim3(SAMPLE_THREADS), 0, s, a);
}

void launch_lm_gumbel(const long long* seeds, unsigned step, const long long* ids, int n, int B, float* out,
                      hipStream_t s) {
  const long long total = (long long)B * n;
  if (total <= 0) return;
  hipLaunchKernelGGL(lm_gumbel_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, seeds, step, ids, n, B,
                     out);
}
