// MFMA GEMM / implicit-GEMM conv: tile planner and dispatch (kernels: gemm_impl.h, instantiated
// per A-operand mode in gemm_c*.hip).
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>

#include "common.h"
#include "gemm_tiles.h"
#include "kernels.h"

void gemm_c0_buf_launch(const GemmArgs& p, float* ws, hipStream_t s);
void gemm_c0_launch(const GemmArgs& p, float* ws, hipStream_t s);
void gemm_c1_launch(const GemmArgs& p, float* ws, hipStream_t s);
void gemm_c2_buf_launch(const GemmArgs& p, float* ws, hipStream_t s);
void gemm_c2_launch(const GemmArgs& p, float* ws, hipStream_t s);
void gemm_c3_launch(const GemmArgs& p, float* ws, hipStream_t s);
void gemm_pp_c0_launch(const GemmArgs& p, float* ws, hipStream_t s);
void gemm_pp_c2_launch(const GemmArgs& p, float* ws, hipStream_t s);

namespace {

constexpr int BK = 64;

// buffer-resource LDS-DMA path: K in whole k-tiles and every byte range addressable by a
// 31-bit buffer offset (num_records), plain GEMMs and Cin % 64 convolutions without upsample
bool buf_ok(const GemmArgs& p) {
  static const int force = [] {
    const char* e = getenv("CASSMANTLE_GEMM_BUF");
    return e ? atoi(e) : 1;
  }();
  if (p.A2 != nullptr) return true;   // two-source A exists only on this path (host-checked sizes)
  if (!force || p.K % BK != 0) return false;
  const long long ldw = p.ldw ? p.ldw : p.K;
  const long long lim = (1LL << 31) - 1;
  if (((long long)(p.Nw - 1) * ldw + p.K) * 2 > lim) return false;
  if (!p.conv) return ((long long)(p.M - 1) * p.lda + p.K) * 2 <= lim;
  if (p.upsample || p.Cin % 64 != 0) return false;
  const long long bias = ((long long)p.pad * p.IW + p.pad) * p.Cin * 2;
  return (long long)p.M / (p.Ho * p.Wo) * p.IH * p.IW * p.Cin * 2 + bias <= lim;
}

// SIMT fallback for shapes the MFMA path does not take (K % 8 != 0 linear layers: the
// 4 -> 4 post_quant_conv).  One thread per output element.
template <int CONV>
__global__ void gemm_simt_kernel(GemmArgs p) {
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)p.M * p.N;
  if (idx >= total) return;
  int m = (int)(idx / p.N), n = (int)(idx - (long long)m * p.N);
  const int batch = blockIdx.z;
  const uint16_t* A = p.A + (long long)batch * p.sA;
  const uint16_t* W = p.W + (long long)batch * p.sW + (long long)n * (p.ldw ? p.ldw : p.K);
  float s = 0.f;
  if constexpr (CONV == 0) {
    const uint16_t* a = A + (long long)m * p.lda;
    for (int k = 0; k < p.K; ++k) s += bf2f(a[k]) * bf2f(W[k]);
  } else {
    int hw = p.Ho * p.Wo;
    int b = m / hw, r = m - b * hw, oy = r / p.Wo, ox = r - oy * p.Wo;
    int Hv = p.upsample ? 2 * p.IH : p.IH, Wv = p.upsample ? 2 * p.IW : p.IW;
    for (int ky = 0; ky < p.ksize; ++ky) {
      int iy = oy * p.stride - p.pad + ky;
      if (iy < 0 || iy >= Hv) continue;
      for (int kx = 0; kx < p.ksize; ++kx) {
        int ix = ox * p.stride - p.pad + kx;
        if (ix < 0 || ix >= Wv) continue;
        int sy = p.upsample ? iy >> 1 : iy, sx = p.upsample ? ix >> 1 : ix;
        const uint16_t* a = A + (((long long)b * p.IH + sy) * p.IW + sx) * p.Cin;
        const uint16_t* w = W + (ky * p.ksize + kx) * p.Cin;
        for (int c = 0; c < p.Cin; ++c) s += bf2f(a[c]) * bf2f(w[c]);
      }
    }
  }
  float o = s * p.alpha;
  if (p.bias) o += bf2f(p.bias[n]);
  if (p.chan_bias) o += bf2f(p.chan_bias[(long long)(m / (p.Ho * p.Wo)) * (p.ldcb ? p.ldcb : p.N) + n]);
  o = apply_act(o, p.act);
  if (p.residual) o += bf2f(p.residual[(long long)m * p.ldc + n]);
  if (p.out_f32)
    reinterpret_cast<float*>(p.C)[(long long)batch * p.sC + (long long)m * p.ldc + n] = o;
  else
    reinterpret_cast<uint16_t*>(p.C)[(long long)batch * p.sC + (long long)m * p.ldc + n] = f2bf(o);
}

// can a kernel family run this call?  The ping-pong and deep-ring kernels take the buffer-resource
// modes (plain / two-source A, Cin % 64 convs without the fused upsample) with bf16 output; ping-pong
// only the bf16 outputs the LDS-staged epilogue takes (its direct path only stores split-K slabs)
bool family_runs(GemmTileFamily f, const GemmArgs& p) {
  if (f == kTileStatic) return true;
  if (f == kTileAreg) return gemm_areg_ok(p);
  if (f == kTilePingPong && (p.N % 8 != 0 || p.ldc % 8 != 0 || (p.ldcb ? p.ldcb : p.N) % 4 != 0)) return false;
  return !p.out_f32 && buf_ok(p) && p.K % BK == 0 && (!p.conv || (!p.upsample && p.Cin % 64 == 0)) && p.N > 16;
}

// a config is only taken -- from the tuning table or forced -- if it is live and its family can run
// the call, so a stale table never selects an unsupported path
bool cfg_runs(int cfg, const GemmArgs& p) {
  const GemmTile* t = gemm_tile(cfg);
  return t != nullptr && family_runs(t->family, p);
}

// ---- measured per-shape tuning table (tools/autotune_gemm.py -> ops/gemm_tuning.json, loaded by
// ops/__init__.py): shape key -> (tile config, split-K).  Consulted before the cost model.
std::mutex g_tune_mu;
std::unordered_map<std::string, GemmPlan> g_tune;
// per calling thread: the generation thread and the scorer thread both launch GEMMs, and these
// are written on every plan (tests/test_native_sanitizers.py runs the planner under TSan)
thread_local std::string g_last_key;
thread_local GemmPlan g_last_plan{0, 1};
std::atomic<bool> g_record_key{false};

}  // namespace

std::string gemm_key(const GemmArgs& p) {
  char buf[192];
  snprintf(buf, sizeof(buf), "m%d n%d k%d w%d b%d c%d:%d:%d:%d:%d:%d:%d:%d p%d a%d g%d s%d r%d cb%d ln%d f%d",
           p.M, p.N, p.K, p.Nw, p.batch, p.conv, p.IH, p.IW, p.Cin, p.stride, p.ksize, p.pad, p.upsample, p.parity,
           p.A2 != nullptr, is_gated(p.act) ? 1 : 0, p.stats != nullptr, p.residual != nullptr, p.chan_bias != nullptr,
           (p.ln_rows != nullptr || p.ln_rows_fx != nullptr) ? 1 : (p.ln_wsum != nullptr ? 2 : (p.gn_stats ? 3 : 0)),
           p.out_f32);
  return std::string(buf);
}

void gemm_tune_set(const std::string& key, int cfg, int split) {
  std::lock_guard<std::mutex> g(g_tune_mu);
  g_tune[key] = GemmPlan{cfg, split};
}
void gemm_tune_clear() {
  std::lock_guard<std::mutex> g(g_tune_mu);
  g_tune.clear();
}
int gemm_tune_size() {
  std::lock_guard<std::mutex> g(g_tune_mu);
  return (int)g_tune.size();
}
void gemm_record_keys(bool on) { g_record_key = on; }
std::string gemm_last_key() { return g_last_key; }
void gemm_last_plan(int* cfg, int* split) { *cfg = g_last_plan.cfg; *split = g_last_plan.split; }

// Choose tile config + split-K by an occupancy-round cost model: the kernel is latency-bound
// per k-tile, so time ~ rounds(blocks / 512) x k-tiles-per-block x tile-cost; split-K adds a
// reduction pass over split x M x N fp32.  Wave quantisation (e.g. 640 blocks = 1.25 rounds)
// was the single largest loss on the SD shapes (M = 32768 / 8192 / 2048 / 512).
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// A/B knobs for the microbenchmark / tile sweeps: CASSMANTLE_GEMM_CFG=<tile index>,
// CASSMANTLE_GEMM_SPLIT=<k slices>, or at run time gemm_set_override (tools/sweep_gemm.py)
static std::atomic<int> g_force_cfg{-2}, g_force_split{0};   // -2: not yet read from the environment
void gemm_set_override(int cfg, int split) {
  g_force_cfg = cfg;
  g_force_split = split;
}

// the folds only the A-in-registers kernel computes: LayerNorm with in-kernel row statistics, and
// GroupNorm of the A rows (gemm_route turns the calls that kernel does not take into a pre-pass first)
static bool areg_only(const GemmArgs& p) {
  return (p.ln_wsum != nullptr && p.ln_rows == nullptr && p.ln_rows_fx == nullptr) || p.gn_stats != nullptr;
}

// the planner: the menu's answer (tuning table, forced config, cost model) under what the call's
// epilogue admits
static GemmPlan gemm_plan_menu(const GemmArgs& p);
GemmPlan gemm_plan(const GemmArgs& p) {
  if (g_record_key) g_last_key = gemm_key(p);
  // neither the table nor a forced config may pick anything else
  GemmPlan r = areg_only(p) ? GemmPlan{kGemmAregTile, 1} : gemm_plan_menu(p);
  if (p.row_stats != nullptr) {
    // output row statistics exist only in the shared LDS-staged epilogue (tile_epilogue):
    // no split-K, not the A-in-registers kernel
    if (r.cfg == kGemmAregTile) r.cfg = 3;
    r.split = 1;
  }
  g_last_plan = r;
  return r;
}

static GemmPlan gemm_plan_menu(const GemmArgs& p) {
  GemmPlan best{0, 1};
  if (g_force_cfg.load(std::memory_order_acquire) == -2) {
    static const bool from_env = [] {
      g_force_split.store(env_int("CASSMANTLE_GEMM_SPLIT", 0));
      int expect = -2;
      g_force_cfg.compare_exchange_strong(expect, env_int("CASSMANTLE_GEMM_CFG", -1));
      return true;
    }();
    (void)from_env;
  }
  const int force_cfg = g_force_cfg.load(), force_split = g_force_split.load();
  if (force_cfg < 0) {
    bool have = false;
    GemmPlan tp{0, 1};
    {
      std::lock_guard<std::mutex> g(g_tune_mu);
      if (!g_tune.empty()) {
        auto it = g_tune.find(gemm_key(p));
        if (it != g_tune.end()) { tp = it->second; have = true; }
      }
    }
    if (have && cfg_runs(tp.cfg, p)) return tp;
  }
  static const int use_big = env_int("CASSMANTLE_GEMM_8WAVE", 0);
  const bool gated = p.act == ACT_GEGLU || p.act == ACT_SWIGLU;
  int only = -1;                         // forced tile (cost model still picks the split)
  // CASSMANTLE_GEMM_PP=0 keeps the planner on the 4-wave kernel (A/B knob); forced configs
  // (CASSMANTLE_GEMM_CFG / gemm_set_override) only need eligibility
  static const int pp_auto = env_int("CASSMANTLE_GEMM_PP", 0);
  const bool pp = pp_auto && family_runs(kTilePingPong, p);
  if (force_cfg >= 0 && cfg_runs(force_cfg, p)) {
    const GemmTile& ft = *gemm_tile(force_cfg);
    if (ft.family == kTileAreg) return GemmPlan{ft.id, 1};
    if ((ft.BN <= 16) == (p.N <= 16)) {   // the N <= 16 tile takes those shapes and no others
      if (gated) {
        // a tile without a gated instantiation maps to a gated default: its family's, or for the
        // table-only tiles (ping-pong 20-22 too, whose eligibility implies it) the deep ring's
        best.cfg = ft.gated() ? ft.id : gemm_default_tile(ft.model ? ft.family : kTileDeep, true);
        return best;
      }
      only = ft.id;
    }
  }
  if (gated) {
    if (pp && (p.N % 64 == 0) && (long long)(p.N / 64) * ((p.M + 255) / 256) >= 256)
      best.cfg = gemm_default_tile(kTilePingPong, true);
    return best;
  }
  const int nk = (p.K + BK - 1) / BK;
  // M <= 8 goes to the GEMV path; short prompts (M = tens of rows) need split-K to fill the chip
  // (batched calls -- the upsampling conv's 4 parity classes -- split per batch: slabs [z][split])
  const bool can_split = p.N % 4 == 0 && p.K % 8 == 0 && p.M > 8;
  double best_t = 1e30;
  for (const GemmTile& tc : kGemmTiles) {   // ascending ids: the first of equal times wins
    if (only >= 0 ? tc.id != only
                  : !tc.model || (tc.family == kTileStatic && tc.WM * tc.WN == 8 && !use_big) ||
                        (tc.family == kTilePingPong && !pp))
      continue;
    if ((tc.BN <= 16) != (p.N <= 16)) continue;
    const long long tiles = (long long)((p.N + tc.BN - 1) / tc.BN) * ((p.M + tc.BM - 1) / tc.BM) * p.batch;
    const double waste = (double)tc.BN * ((p.N + tc.BN - 1) / tc.BN) / p.N;   // padded columns
    for (int split = 1; split <= GEMM_MAX_SPLIT; ++split) {
      if (split > 1 && (!can_split || nk / split < 4)) break;
      const long long blocks = tiles * split;
      const long long rounds = (blocks + tc.slots - 1) / tc.slots;
      const int kper = (nk + split - 1) / split;
      // per-k-tile cost: fixed latency part + size part (normalised to a 128x128 tile)
      const double tile_cost = (0.55 + 0.45 * (tc.BM * tc.BN) / 16384.0) / tc.eff;
      // calibrated on MI355X: ~1.8 us per 128x128x64 k-tile per occupancy round (2 blocks/CU)
      double t = 1.8 * rounds * (kper + 2) * tile_cost * (waste > 1.3 ? waste : 1.0);
      // split-K: slab write + read at ~3 TB/s plus the extra reduce launch (~6 us in a graph)
      if (split > 1) t += 6.0 + 2.0 * (double)split * p.batch * p.M * p.N * 4 / 3.0e6;
      if (only >= 0 && force_split > 0 && split != force_split) continue;
      if (t < best_t - 1e-9) { best_t = t; best = GemmPlan{tc.id, split}; }
    }
  }
  return best;
}

// skinny M (decode tokens, time-embedding / pooled projections): the weight-streaming GEMV of lm.hip
bool gemv_ok(const GemmArgs& p) {
  if (p.conv || !gemv_rows(p.M) || p.M < 1 || p.chan_bias != nullptr) return false;
  return p.K % 8 == 0 && p.lda % 8 == 0 && (p.ldw ? p.ldw : p.K) % 8 == 0;
}

void gemm_apply_pre(GemmArgs& p, GemmPre pre, const void* tmp) {
  if (pre == kPreRowStats) { p.ln_rows = static_cast<const float*>(tmp); p.ln_eps = 0.f; }
  if (pre == kPreGnApply) { p.A = static_cast<const uint16_t*>(tmp); p.gn_stats = nullptr; p.gn_gamma = p.gn_beta = nullptr; }
}

static thread_local GemmRoute g_last_route{kGemmTiled, kA_c0, 0, 1, kPreNone, false, 0, nullptr};
GemmRoute gemm_last_route() { return g_last_route; }
static_assert(GN_MAX_C == 4096, "gemm_route's refusal text names the bound");

GemmRoute gemm_route(const GemmArgs& call) {
  GemmArgs p = call;
  GemmRoute r{kGemmTiled, kA_c0, -1, 1, kPreNone, false, 0, nullptr};
  auto refuse = [&r](bool cond, const char* why) { if (cond && r.refuse == nullptr) r.refuse = why; };
  const bool gated = is_gated(p.act), contig = p.lda == p.K || p.M == 1;
  // the pass a fold needs first where the A-in-registers kernel does not take the call as it stands
  // (CASSMANTLE_LN_INKERNEL=0 forces the row-statistics pass: A/B and debugging knob)
  static const bool ln_inkernel = [] { const char* e = getenv("CASSMANTLE_LN_INKERNEL"); return !(e && e[0] == '0'); }();
  if (p.gn_stats != nullptr) {
    if (!gemm_areg_ok(p)) r.pre = kPreGnApply;
    refuse(r.pre && !(contig && p.K % 8 == 0 && p.gn_groups > 0 && p.K % p.gn_groups == 0), "gemm gn fallback: contiguous rows");
  } else if (areg_only(p) && p.ln_eps > 0.f) {
    if (!ln_inkernel || !gemm_areg_ok(p)) r.pre = kPreRowStats;
    refuse(r.pre && !(contig && p.K <= 4096), "gemm: folded LayerNorm row statistics need contiguous rows");
  }
  alignas(64) static const char fresh[64] = {};   // stands for the pass's output, a fresh allocation
  gemm_apply_pre(p, r.pre, fresh);
  const GemmPlan plan = gemm_plan(p);
  p.cfg = plan.cfg;
  // fp8 K/V emission runs in the LDS-staged epilogue (V transposed through the tile in LDS);
  // the split-K reduce would scatter V byte by byte
  p.split = p.kv8 != nullptr ? 1 : plan.split;
  // the kernel, in the order of preference
  const bool mfma_ok = (p.K % 8 == 0) && (!p.conv || p.Cin % 8 == 0) && (p.conv || p.lda % 8 == 0) && (p.ldw % 8 == 0);
  const GemmTile* t = gemm_tile(p.cfg);
  const GemmTileFamily fam = t != nullptr ? t->family : kTileStatic;
  if (gemv_ok(p)) {
    r.kernel = kGemmGemv;
  } else if (!mfma_ok) {
    // one thread per output element and the plain epilogue: nothing else of the call is computed
    r.kernel = kGemmSimt;
    if (p.conv) r.mode = kA_c1;
    refuse(gated, "gemm: a gated call takes <= 8 rows (GEMV) or K, the row strides and Cin in multiples of 8 (MFMA)");
    refuse(p.row_stats || p.kv8 || p.ln_rows || p.ln_rows_fx || p.ln_wsum || p.gn_stats || p.A2,
           "gemm: K, the row strides and Cin must be multiples of 8 for row_stats, kv8, folded norms and two-source A");
  } else if (fam == kTileAreg && gemm_areg_ok(p)) {
    r.kernel = kGemmAreg;
    r.cfg = kGemmAregTile;
  } else if (fam == kTilePingPong && family_runs(fam, p)) {
    r.kernel = kGemmPingPong;
    r.mode = p.conv ? kA_c2_buf : kA_c0_buf;
    r.cfg = gemm_tile_that_runs(p.cfg, true, gated, false, true);
  } else {
    const bool buf = buf_ok(p);
    if (!p.conv) r.mode = buf ? kA_c0_buf : kA_c0;
    else if (p.Cin % 64 != 0) r.mode = kA_c1;
    else r.mode = p.upsample ? kA_c3 : buf ? kA_c2_buf : kA_c2;
    // (a gated call runs the gated instantiations, which store bf16)
    r.cfg = gemm_tile_that_runs(p.cfg, false, gated, !gated && p.out_f32, r.mode == kA_c0_buf || r.mode == kA_c2_buf);
  }
  // split-K is the tile kernels' (slabs [z][split], summed by their reduce pass)
  if (r.kernel == kGemmTiled || r.kernel == kGemmPingPong) r.split = p.split;
  if (r.split > 1) r.ws_floats = (long long)r.split * p.batch * p.M * p.N;
  // output statistics are fused into the LDS-staged bf16 epilogue of the MFMA kernels (split-K:
  // into the reduce pass), for one batch or the parity classes of one image set, above the GEMV's
  // row counts; every other call gets a per-channel statistics pass over the output
  const bool fuses_stats = r.kernel != kGemmGemv && r.kernel != kGemmSimt && !p.out_f32 && !gated &&
                           (p.batch == 1 || p.parity) && !gemv_rows(p.M);
  r.post_stats = p.stats != nullptr && !fuses_stats;
  refuse(r.post_stats && p.N > GN_MAX_C, "gemm stats: the separate statistics pass takes N <= 4096");
  g_last_route = r;
  return r;
}

void launch_gemm(const GemmArgs& call, const GemmRoute& r, float* ws, hipStream_t s) {
  GemmArgs p = call;
  p.cfg = r.cfg;
  p.split = r.split;
  switch (r.kernel) {
    case kGemmGemv: (void)launch_gemv(p, s); return;
    case kGemmSimt: {
      // shapes the MFMA path does not take (K % 8 != 0 linear layers: the 4 -> 4 post_quant_conv)
      const long long total = (long long)p.M * p.N;
      dim3 grid((unsigned)((total + 255) / 256), 1, p.batch);
      if (p.conv) hipLaunchKernelGGL(gemm_simt_kernel<1>, grid, dim3(256), 0, s, p);
      else hipLaunchKernelGGL(gemm_simt_kernel<0>, grid, dim3(256), 0, s, p);
      return;
    }
    case kGemmAreg: launch_gemm_areg(p, s); return;
    case kGemmPingPong: (r.mode == kA_c0_buf ? gemm_pp_c0_launch : gemm_pp_c2_launch)(p, ws, s); return;
    case kGemmTiled:
      switch (r.mode) {
        case kA_c0: gemm_c0_launch(p, ws, s); return;
        case kA_c0_buf: gemm_c0_buf_launch(p, ws, s); return;
        case kA_c1: gemm_c1_launch(p, ws, s); return;
        case kA_c2: gemm_c2_launch(p, ws, s); return;
        case kA_c2_buf: gemm_c2_buf_launch(p, ws, s); return;
        case kA_c3: gemm_c3_launch(p, ws, s); return;
      }
  }
}
