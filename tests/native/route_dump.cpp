// Route dump for the golden in tests/golden/gemm_routes.txt (tests/test_gemm_menu.py).  Linked like
// planner_dump.cpp: ops/csrc/gemm.hip + gemm_areg.hip with the launchers stubbed out, nothing touches
// a GPU.  One line per call class (gemm_call_classes.h):
//   name | cost model | forced cfg -1..36, split 0 | forced cfg -1..36, split 3
// each route as kernel:mode:cfg:split:pre:post_stats, or refuse.  argv[1] labels the run (the
// environment knobs are read once per process); argv[2], if given, keeps the classes whose name
// starts with it.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gemm_call_classes.h"

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

void put(const GemmArgs& p) {
  const GemmRoute r = gemm_route(p);
  if (r.refuse != nullptr) {
    std::printf(" refuse");
    return;
  }
  std::printf(" %s:%s:%d:%d:%s:%d", gemm_kernel_name(r.kernel), gemm_amode_name(r.mode), r.cfg, r.split,
              gemm_pre_name(r.pre), (int)r.post_stats);
}

}  // namespace

int main(int argc, char** argv) {
  std::printf("# %s\n", argc > 1 ? argv[1] : "env");
  const char* only = argc > 2 ? argv[2] : "";
  gemm_tune_clear();
  for (auto& [name, p] : route_classes()) {
    if (std::strncmp(name.c_str(), only, std::strlen(only)) != 0) continue;
    std::printf("%s |", name.c_str());
    gemm_set_override(-1, 0);
    put(p);
    for (int split : {0, 3}) {
      std::printf(" |");
      for (int c = -1; c <= kMaxCfg; ++c) {
        gemm_set_override(c, split);
        put(p);
      }
    }
    std::printf("\n");
  }
  return 0;
}
