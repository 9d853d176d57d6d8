// The GEMM / conv call classes of the planner and route goldens (planner_dump.cpp, route_dump.cpp):
// GemmArgs as the bindings fill them, on dummy pointers -- nothing is launched.
#pragma once
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"

namespace {

constexpr int kMaxCfg = 36;   // past the last index on purpose
uint16_t dummy[64] __attribute__((aligned(64)));
using GemmClasses = std::vector<std::pair<std::string, GemmArgs>>;

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

std::string class_name(const char* tag, const GemmArgs& p) {
  char b[96];
  snprintf(b, sizeof(b), "%s m%d n%d k%d", tag, p.M, p.N, p.K);
  return std::string(b);
}

void with_geglu(GemmArgs& p) { p.act = 4; p.Nw = 2 * p.N; }   // ACT_GEGLU
void with_stats(GemmArgs& p, int hw) { p.stats = reinterpret_cast<long long*>(dummy); p.stats_hw = hw; }
void with_ln_kernel(GemmArgs& p) { p.ln_wsum = reinterpret_cast<const float*>(dummy); p.ln_eps = 1e-5f; }
void with_gn_fold(GemmArgs& p, int hw) {
  p.gn_stats = reinterpret_cast<const long long*>(dummy); p.gn_gamma = dummy; p.gn_beta = dummy;
  p.gn_groups = 32; p.gn_hw = hw; p.gn_eps = 1e-5f;
}
void with_batch4(GemmArgs& p) {
  p.batch = 4; p.sA = (long long)p.M * p.K; p.sW = (long long)p.N * p.K; p.sC = (long long)p.M * p.N;
}
GemmArgs conv_parity() {
  GemmArgs c = conv(2, 32, 32, 320, 320, 1, 0);
  c.parity = 1; c.ksize = 2; c.K = 4 * c.Cin; c.batch = 4; c.sW = (long long)c.N * 4 * c.Cin;
  return c;
}

// the classes of tests/golden/planner_plans.txt
GemmClasses planner_classes() {
  GemmClasses v;
  const int mnk[][3] = {{32768, 320, 320}, {32768, 960, 320}, {32768, 1280, 320}, {8192, 640, 640},
                        {8192, 1920, 640}, {2048, 1280, 1280}, {512, 1280, 11520}, {77, 768, 768},
                        {4096, 4096, 4096}, {33, 5, 8}, {1, 320, 1280},
                        {4096, 16, 512},      // N <= 16
                        {2048, 320, 72}};     // K % 64 != 0: fails buf_ok
  for (auto& s : mnk) {
    GemmArgs p = plain(s[0], s[1], s[2]);
    v.emplace_back(class_name("plain", p), p);
  }
  const int base[][3] = {{2048, 1280, 1280}, {32768, 320, 320}};
  for (auto& s : base) {
    const int M = s[0], N = s[1], K = s[2];
    const int hw = M == 2048 ? 256 : 4096;
    GemmArgs p = plain(M, N, K);
    with_geglu(p);
    v.emplace_back(class_name("geglu", p), p);
    p = plain(M, N, K);
    with_stats(p, hw);
    v.emplace_back(class_name("stats", p), p);
    p = plain(M, N, K);
    p.row_stats = reinterpret_cast<long long*>(dummy);
    v.emplace_back(class_name("row_stats", p), p);
    p = plain(M, N, K);
    with_ln_kernel(p);
    v.emplace_back(class_name("ln_kernel", p), p);
    p = plain(M, N, K);
    with_ln_kernel(p);
    p.ln_rows_fx = reinterpret_cast<const long long*>(dummy);
    v.emplace_back(class_name("ln_rows_fx", p), p);
    p = plain(M, N, K);
    with_gn_fold(p, hw);
    v.emplace_back(class_name("gn_fold", p), p);
    p = plain(M, N, K);
    p.out_f32 = 1;
    v.emplace_back(class_name("out_f32", p), p);
    p = plain(M, N, K);
    p.A2 = dummy; p.ka = 320; p.lda = 320; p.lda2 = K - 320;
    v.emplace_back(class_name("a2", p), p);
    p = plain(M, N, K);
    with_batch4(p);
    v.emplace_back(class_name("batch4", p), p);
  }
  GemmArgs c = conv(2, 32, 32, 320, 320, 1, 0);
  v.emplace_back(class_name("conv3x3", c), c);
  c = conv(2, 32, 32, 320, 320, 2, 0);
  v.emplace_back(class_name("conv3x3_s2", c), c);
  c = conv(2, 32, 32, 320, 320, 1, 1);
  v.emplace_back(class_name("conv3x3_up", c), c);
  c = conv(2, 32, 32, 8, 320, 1, 0);      // K = 72: the MFMA path in the generic conv mode (c1), not SIMT
  v.emplace_back(class_name("conv3x3_cin8", c), c);
  c = conv_parity();
  v.emplace_back(class_name("conv_parity", c), c);
  return v;
}

// what tests/golden/gemm_routes.txt adds: the edges between the kernels, the pre- and post-passes
GemmClasses route_classes() {
  GemmClasses v = planner_classes();
  for (int M : {1, 2, 4, 8}) {
    GemmArgs p = plain(M, 320, 1280);
    v.emplace_back(class_name("skinny", p), p);
    with_geglu(p);
    v.emplace_back(class_name("skinny_geglu", p), p);
  }
  GemmArgs p = plain(8, 320, 1280);
  p.chan_bias = dummy;
  v.emplace_back(class_name("skinny_chan_bias", p), p);
  p = plain(4, 320, 1280);
  p.lda = 1284;
  v.emplace_back(class_name("skinny_lda1284", p), p);
  p = conv(1, 2, 2, 320, 320, 1, 0);
  v.emplace_back(class_name("skinny_conv", p), p);
  p = plain(33, 8, 4);
  v.emplace_back(class_name("k4", p), p);
  with_stats(p, 33);
  v.emplace_back(class_name("k4_stats", p), p);
  p = plain(33, 8, 4);
  p.out_f32 = 1;
  v.emplace_back(class_name("k4_out_f32", p), p);
  p = plain(128, 384, 1280);
  p.kv8 = reinterpret_cast<uint8_t*>(dummy); p.kv8_ntok = 64; p.kv8_hk = 1; p.kv8_col0 = 256;
  v.emplace_back(class_name("kv8", p), p);
  p = plain(2048, 1280, 1280);
  p.ln_rows = reinterpret_cast<const float*>(dummy); p.ln_wsum = reinterpret_cast<const float*>(dummy);
  v.emplace_back(class_name("ln_rows", p), p);
  p = plain(32768, 320, 320);
  with_gn_fold(p, 64);
  v.emplace_back(class_name("gn_fold_hw64", p), p);
  p = plain(2048, 1280, 1280);
  with_stats(p, 256);
  p.out_f32 = 1;
  v.emplace_back(class_name("stats_out_f32", p), p);
  p = plain(2048, 1280, 1280);
  with_stats(p, 256);
  with_batch4(p);
  v.emplace_back(class_name("stats_batch4", p), p);
  p = plain(2048, 1280, 1280);
  with_stats(p, 256);
  with_geglu(p);
  v.emplace_back(class_name("stats_geglu", p), p);
  p = conv_parity();
  with_stats(p, p.Ho * p.Wo);
  v.emplace_back(class_name("stats_conv_parity", p), p);
  p = plain(33, 320, 1280);
  with_geglu(p);
  p.lda = 1284;
  v.emplace_back(class_name("geglu_lda1284", p), p);
  return v;
}

}  // namespace
