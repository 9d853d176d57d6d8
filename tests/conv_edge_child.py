"""One conv case of kernel_oracle.conv_tile_cases on the GPU (:func:`launch_case`, shared with
test_kernel_edges_conv_gpu.py), and, run as a program, the Cin % 64 plain-conv cases of the static
tiles in a process of its own: ``CASSMANTLE_GEMM_BUF`` is read once per process, and with
``CASSMANTLE_GEMM_BUF=0`` those convs take gemm_c2, the global-load path with the zero page that a
conv input past the 31-bit buffer range takes.  Prints one JSON object on stdout: whether the
variable took effect and, per case, its id, plan, worst block, guard state and the statistics'
error.  It asserts nothing about the figures: the parent test does."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kernel_oracle as ko  # noqa: E402
from cassmantle_amd import ops  # noqa: E402
from cassmantle_amd.ops._ext import ext, ext_available, ext_error  # noqa: E402
from test_kernel_edges_gpu import DEV, MENU, G, P, last_plan, zeroed_stats  # noqa: E402


def launch_case(c: ko.ConvCase):
    """-> (guarded output, guarded statistics or None, fp64 reference, the plan that ran).  Inputs
    sit in NaN, chan_bias is a column slice of a wider NaN buffer, the tile and split are forced
    for this launch alone."""
    (x, w, b, cb, res), y64 = ko.conv_case_data(c)
    B, stride = x.shape[0], ko.CONV_GEOM[c.geom][3]
    g = G(y64.shape)
    st = zeroed_stats(B, c.Cout, 2) if c.stats else None
    stv = None if st is None else st.view
    xp, bp, rp, cbp = P(x), P(b), P(res), ko.chan_bias_slice(cb, DEV)
    assert cbp.stride(0) != c.Cout
    wp = P(ops.fold_upsample_weights(w) if c.op == "up2" else w)
    ext().gemm_set_override(c.cfg, c.split)
    try:
        if c.op == "up2":
            ops._launch(ext().conv2d_up2, xp, wp, bp, rp, cbp, g.view, stv)
        else:
            ops.conv2d(xp, wp, bp, stride=stride, padding=c.ksize // 2, residual=rp, upsample=c.op == "fused_up",
                       chan_bias=cbp, stats=stv, out=g.view)
        plan = last_plan()
    finally:
        ext().gemm_set_override(-1, 0)
    return g, st, y64, plan


def stats_rel_err(st_view, out_view, B) -> float:
    """check_stats' figure: epilogue statistics against those of the stored output"""
    exp = ops.new_stats(B, out_view.shape[-1], DEV)
    ops.channel_stats_ref(out_view.reshape(B, -1, out_view.shape[-1]), exp)
    a, b = ops.stats_to_float(st_view), ops.stats_to_float(exp)
    return ((a - b).norm() / b.norm()).item()


def child_cases(menu=MENU) -> list:
    """the 3x3 Cin % 64 cases of the static tiles: stride 1 and 2, the short-slice and the
    empty-slice split with either reduce kernel, and at Cin = 64 itself the one split the planner
    admits there (nk = 9 in two: slices of 5 and 4, the second starting inside the taps' second row)"""
    static = {r[0] for r in menu if r[1] == "static"}
    cases = [c for c in ko.conv_tile_cases(menu) if c.cfg in static and c.op == "conv" and c.Cin % 64 == 0 and c.Cout % 8 == 0]
    s1 = [c for c in cases if c.geom == "s1" and c.Cin == 64]
    return cases + [c._replace(split=2, stats=st) for c in s1 for st in (True, False)]


def main() -> int:
    assert os.environ.get("CASSMANTLE_GEMM_BUF") == "0", "run with CASSMANTLE_GEMM_BUF=0"
    assert ext_available(), ext_error()
    ops.set_mode("hip")
    rows = []
    cases = child_cases()
    # the variable took effect: without buffer resources no deep-ring tile runs (family_runs), so
    # a forced one falls back to the planner's choice
    deep = next(r[0] for r in MENU if r[1] == "deep")
    buf_off = launch_case(cases[0]._replace(cfg=deep, Cout=72))[3][0] != deep
    for c in cases:
        g, st, y64, plan = launch_case(c)
        torch.cuda.synchronize()
        rows.append({"id": c.id, "plan": list(plan), "guards": ko.guards_intact(g) and (st is None or ko.guards_intact(st)),
                     "err": ko.block_rel_err(g.view.reshape(-1, c.Cout), y64.flatten(0, 2)),
                     "stats_err": None if st is None else stats_rel_err(st.view, g.view, y64.shape[0])})
    json.dump({"buf_off": buf_off, "cases": rows}, sys.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
