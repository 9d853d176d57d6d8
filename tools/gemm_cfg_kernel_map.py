"""Which kernel does each GEMM tile config launch?  Forces every live config (ops/csrc/gemm_tiles.h)
once on a small call its family can run and pairs the launches with a rocprofv3 kernel trace:

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- \
        python tools/gemm_cfg_kernel_map.py run --order DIR/order.json
    python tools/gemm_cfg_kernel_map.py map --order DIR/order.json --trace DIR/.../run_kernel_trace.csv \
        [--tag NAME] >> profiles/gemm_menu_cfg_kernel_map.jsonl

Calls: plain M 512 x N 320 x K 640 for every config (N = 16 for the N <= 16 tile), and a GEGLU of
the same shape for the configs with a gated instantiation.  Split-K is forced to 1, so each call
is exactly one gemm*_kernel dispatch, in order."""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(a):
    import torch
    from cassmantle_amd import ops
    from cassmantle_amd.ops._ext import ext
    os.environ["CASSMANTLE_GEMM_TUNE"] = "0"
    ops.set_mode("hip")
    ext().gemm_tune_clear()
    if a.cfgs:
        menu = [(int(c), None, None, 0, None, None, None, c in a.gated.split(",")) for c in a.cfgs.split(",")]
    else:
        menu = [tuple(r) for r in ext().gemm_tile_menu()]
    M, K = 512, 640
    x = torch.randn(M, K, device="cuda").bfloat16()
    order = []
    for cfg, _, _, bn, _, _, _, gated in menu:
        small = bn == 16 or (a.cfgs and str(cfg) in a.small.split(","))
        calls = [("n16" if small else "plain", 16 if small else 320, None)] + ([("geglu", 320, "geglu")] if gated else [])
        for label, N, act in calls:
            w = torch.randn(N * (2 if act else 1), K, device="cuda").bfloat16()
            ext().gemm_set_override(cfg, 1)
            ops.linear(x, w, None, act=act)
            ext().gemm_set_override(-1, 0)
            order.append({"cfg": cfg, "call": label, "plan": list(ext().gemm_last_plan()),
                          "route": list(ext().gemm_last_route())})
    torch.cuda.synchronize()
    json.dump(order, open(a.order, "w"))


def map_(a):
    order = json.load(open(a.order))
    rows = [r for r in csv.DictReader(open(a.trace)) if re.search(r"gemm_(pp_|areg_)?kernel", r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(order), (len(rows), len(order))
    for o, r in zip(order, rows):
        name = r["Kernel_Name"].replace("void (anonymous namespace)::", "").replace("(anonymous namespace)::", "")
        print(json.dumps({"tag": a.tag, **o, "kernel": name, "grid": [int(r.get(f"Grid_Size_{d}", 0)) for d in "XYZ"],
                          "block": int(r.get("Workgroup_Size_X", 0))}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "map"])
    ap.add_argument("--order", required=True)
    ap.add_argument("--trace")
    ap.add_argument("--tag", default="")
    ap.add_argument("--cfgs", default=None, help="comma list of configs (default: gemm_tile_menu())")
    ap.add_argument("--gated", default="0,6,8,9,12", help="with --cfgs: the configs that also get a GEGLU call")
    ap.add_argument("--small", default="4", help="with --cfgs: the configs that get N = 16")
    a = ap.parse_args()
    {"run": run, "map": map_}[a.mode](a)
