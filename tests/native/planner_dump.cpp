// Planner dump for the golden in tests/golden/planner_plans.txt (tests/test_gemm_menu.py).
// Linked like planner_sanitize.cpp: ops/csrc/gemm.hip + gemm_areg.hip with the tile launchers
// stubbed out, public API of kernels.h only, nothing touches a GPU.  One line per call class:
//   name | cost model | forced cfg -1..36, split 0 | forced cfg -1..36, split 3 | table cfg 0..36, split 2
// each plan as cfg:split.  Unknown and retired indices are included on purpose.  argv[1] labels
// the run (the environment knobs are read once per process, so the test runs this twice).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"

void gemm_c0_buf_launch(const GemmArgs&, float*, hipStream_t) { std::abort(); }
void gemm_c0_launch(const GemmArgs&, float*, hipStream_t) { std::abort(); }
void gemm_c1_launch(const GemmArgs&, float*, hipStream_t) { std::abort(); }
void gemm_c2_buf_launch(const GemmArgs&, float*, hipStream_t) { std::abort(); }
void gemm_c2_launch(const GemmArgs&, float*, hipStream_t) { std::abort(); }
void gemm_c3_launch(const GemmArgs&, float*, hipStream_t) { std::abort(); }
void gemm_pp_c0_launch(const GemmArgs&, float*, hipStream_t) { std::abort(); }
void gemm_pp_c2_launch(const GemmArgs&, float*, hipStream_t) { std::abort(); }
bool launch_gemv(const GemmArgs&, hipStream_t) { std::abort(); }

namespace {

constexpr int kMaxCfg = 36;   // past the last index on purpose
uint16_t dummy[64] __attribute__((aligned(64)));

GemmArgs plain(int M, int N, int K) {
  GemmArgs p;
  p.A = dummy; p.W = dummy; p.C = dummy;
  p.M = M; p.N = N; p.K = K; p.Nw = N;
  p.lda = K; p.ldc = N;
  return p;
}

GemmArgs conv(int B, int H, int W, int Cin, int Cout, int stride, int upsample) {
  GemmArgs p;
  p.A = dummy; p.W = dummy; p.C = dummy;
  p.conv = 1;
  p.IH = H; p.IW = W; p.Cin = Cin; p.ksize = 3; p.stride = stride; p.pad = 1; p.upsample = upsample;
  const int Hv = upsample ? 2 * H : H, Wv = upsample ? 2 * W : W;
  p.Ho = (Hv - 1) / stride + 1; p.Wo = (Wv - 1) / stride + 1;
  p.N = Cout; p.Nw = Cout;
  p.M = B * p.Ho * p.Wo; p.K = 9 * Cin;
  p.lda = Cin; p.ldc = Cout;
  p.stats_hw = p.Ho * p.Wo;
  return p;
}

std::vector<std::pair<std::string, GemmArgs>> classes() {
  std::vector<std::pair<std::string, GemmArgs>> v;
  auto name = [](const char* tag, const GemmArgs& p) {
    char b[96];
    snprintf(b, sizeof(b), "%s m%d n%d k%d", tag, p.M, p.N, p.K);
    return std::string(b);
  };
  const int mnk[][3] = {{32768, 320, 320}, {32768, 960, 320}, {32768, 1280, 320}, {8192, 640, 640},
                        {8192, 1920, 640}, {2048, 1280, 1280}, {512, 1280, 11520}, {77, 768, 768},
                        {4096, 4096, 4096}, {33, 5, 8}, {1, 320, 1280},
                        {4096, 16, 512},      // N <= 16
                        {2048, 320, 72}};     // K % 64 != 0: fails buf_ok
  for (auto& s : mnk) {
    GemmArgs p = plain(s[0], s[1], s[2]);
    v.emplace_back(name("plain", p), p);
  }
  const int base[][3] = {{2048, 1280, 1280}, {32768, 320, 320}};
  for (auto& s : base) {
    const int M = s[0], N = s[1], K = s[2];
    const int hw = M == 2048 ? 256 : 4096;
    GemmArgs p = plain(M, N, K);
    p.act = 4; p.Nw = 2 * N;                                   // ACT_GEGLU
    v.emplace_back(name("geglu", p), p);
    p = plain(M, N, K);
    p.stats = reinterpret_cast<long long*>(dummy); p.stats_hw = hw;
    v.emplace_back(name("stats", p), p);
    p = plain(M, N, K);
    p.row_stats = reinterpret_cast<long long*>(dummy);
    v.emplace_back(name("row_stats", p), p);
    p = plain(M, N, K);
    p.ln_wsum = reinterpret_cast<const float*>(dummy); p.ln_eps = 1e-5f;
    v.emplace_back(name("ln_kernel", p), p);
    p = plain(M, N, K);
    p.ln_wsum = reinterpret_cast<const float*>(dummy); p.ln_eps = 1e-5f;
    p.ln_rows_fx = reinterpret_cast<const long long*>(dummy);
    v.emplace_back(name("ln_rows_fx", p), p);
    p = plain(M, N, K);
    p.gn_stats = reinterpret_cast<const long long*>(dummy); p.gn_gamma = dummy; p.gn_beta = dummy;
    p.gn_groups = 32; p.gn_hw = hw; p.gn_eps = 1e-5f;
    v.emplace_back(name("gn_fold", p), p);
    p = plain(M, N, K);
    p.out_f32 = 1;
    v.emplace_back(name("out_f32", p), p);
    p = plain(M, N, K);
    p.A2 = dummy; p.ka = 320; p.lda = 320; p.lda2 = K - 320;
    v.emplace_back(name("a2", p), p);
    p = plain(M, N, K);
    p.batch = 4; p.sA = (long long)M * K; p.sW = (long long)N * K; p.sC = (long long)M * N;
    v.emplace_back(name("batch4", p), p);
  }
  GemmArgs c = conv(2, 32, 32, 320, 320, 1, 0);
  v.emplace_back(name("conv3x3", c), c);
  c = conv(2, 32, 32, 320, 320, 2, 0);
  v.emplace_back(name("conv3x3_s2", c), c);
  c = conv(2, 32, 32, 320, 320, 1, 1);
  v.emplace_back(name("conv3x3_up", c), c);
  c = conv(2, 32, 32, 8, 320, 1, 0);
  v.emplace_back(name("conv3x3_cin8", c), c);
  c = conv(2, 32, 32, 320, 320, 1, 0);
  c.parity = 1; c.ksize = 2; c.K = 4 * c.Cin; c.batch = 4; c.sW = (long long)c.N * 4 * c.Cin;
  v.emplace_back(name("conv_parity", c), c);
  return v;
}

void put(const GemmPlan& g) { std::printf(" %d:%d", g.cfg, g.split); }

}  // namespace

int main(int argc, char** argv) {
  std::printf("# %s\n", argc > 1 ? argv[1] : "env");
  for (auto& [name, p] : classes()) {
    std::printf("%s |", name.c_str());
    gemm_tune_clear();
    gemm_set_override(-1, 0);
    put(gemm_plan(p));
    for (int split : {0, 3}) {
      std::printf(" |");
      for (int c = -1; c <= kMaxCfg; ++c) {
        gemm_set_override(c, split);
        put(gemm_plan(p));
      }
    }
    std::printf(" |");
    gemm_set_override(-1, 0);
    const std::string key = gemm_key(p);
    for (int c = 0; c <= kMaxCfg; ++c) {
      gemm_tune_set(key, c, 2);
      put(gemm_plan(p));
    }
    gemm_tune_clear();
    std::printf("\n");
  }
  return 0;
}
