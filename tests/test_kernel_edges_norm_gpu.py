"""norm.hip across its launch geometry, with the instruments of kernel_oracle.py.  The GroupNorm
launchers choose vectors per thread, lanes, chunks, rows per block and rows in flight from
(B, S, C); ``ext().group_norm_geometry`` reports that choice, every case of
kernel_oracle.GN_GEOM_CASES names the branches it exists for, and the tests assert from the
binding that the case reaches them (a retuned constant fails a case by name) and that the CPU
transcript gn_geometry_model still equals the binding.  The data gives every (image, group) a
mean and a deviation of its own, so statistics of the wrong group or image are orders of
magnitude over the bound (test_kernel_oracle.py plants them).  The statistics-fed kernels get
the statistics of channel_stats_ref, computed on the CPU; channel_stats_kernel is held per
(image, channel) to the error bound of its own fp32 chain, and row_stats per row to four times
the fp32 formula's error.  Inputs sit in NaN (int64 statistics between canaries), outputs
between canaries."""
import pytest
import torch

import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.ops import reference as ref
from cassmantle_amd.ops._ext import ext, ext_available, ext_error
from kernel_oracle import BOUND, F64
from test_kernel_edges_gpu import DEV, G, P, check, zeroed_stats

pytestmark = pytest.mark.gpu
GN_IDS = [c.id for c in ko.GN_GEOM_CASES]
GN_SHAPES = list({(c.B, c.S, c.C): c for c in ko.GN_GEOM_CASES}.values())     # channel_stats does not know G or Ca


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    assert ext_available(), ext_error()
    ops.set_mode("hip")


def geometry(c):
    return ext().group_norm_geometry(c.B, c.S, c.C)


def stats_in(st):
    """int64 statistics as a kernel input: inside a buffer of the canary pattern (7fa5a5a5a5a5a5a5,
    2^38 as a fixed-point sum), so a read before or past them wrecks the group it lands in"""
    g = G(st.shape, torch.int64)
    g.view.copy_(st)
    return g.view


# ------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("c", ko.GN_GEOM_CASES, ids=GN_IDS)
def test_group_norm_case_reaches_its_branches(c):
    geom = geometry(c)
    assert geom == ko.gn_geometry_model(c.B, c.S, c.C), "gn_geometry_model is no longer group_norm_geometry's transcript"
    got = ko.gn_branches(c.B, c.S, c.C, c.G, c.Ca, geom)
    assert set(c.reaches) <= got, f"{c.id} no longer reaches {sorted(set(c.reaches) - got)} under {geom}"


def test_every_launch_branch_has_a_case():
    seen = set()
    for c in ko.GN_GEOM_CASES:
        seen |= set(c.reaches) & ko.gn_branches(c.B, c.S, c.C, c.G, c.Ca, geometry(c))
    assert seen == set(ko.GN_BRANCHES), sorted(set(ko.GN_BRANCHES) - seen)


@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("c", ko.GN_GEOM_CASES, ids=GN_IDS)
def test_group_norm_geometry_edges(c, silu):
    x, gam, be = ko.gn_case_inputs(c)
    y64 = ref.group_norm(x, c.G, gam, be, 1e-5, silu, dtype=F64)
    block = (1, 16, c.C // c.G)
    st = torch.zeros(c.B, c.C, 2, dtype=torch.int64)
    ops.channel_stats_ref(x, st)
    xp, gp, bp = P(x), P(gam), P(be)
    errs = []
    g = G(x.shape)
    ext().group_norm(xp, gp, bp, g.view, c.G, 1e-5, int(silu))
    check(g, y64, "group_norm", f"group_norm {c.id}", block, errs)
    g = G(x.shape)
    ext().group_norm_stats(xp, stats_in(st), None, gp, bp, g.view, c.G, 1e-5, int(silu))
    check(g, y64, "group_norm", f"group_norm_stats {c.id}", block, errs)
    if c.Ca:
        g = G(x.shape)
        ext().group_norm_cat(P(x[..., :c.Ca].contiguous()), P(x[..., c.Ca:].contiguous()), stats_in(st[:, :c.Ca].contiguous()),
                             stats_in(st[:, c.Ca:].contiguous()), gp, bp, g.view, c.G, 1e-5, int(silu))
        check(g, y64, "group_norm", f"group_norm_cat {c.id}", block, errs)
        g = G(x.shape)          # the same split through group_norm_stats: one tensor, two statistics buffers
        ext().group_norm_stats(xp, stats_in(st[:, :c.Ca].contiguous()), stats_in(st[:, c.Ca:].contiguous()), gp, bp, g.view,
                               c.G, 1e-5, int(silu))
        check(g, y64, "group_norm", f"group_norm_stats, split {c.id}", block, errs)
    assert not errs, errs


@pytest.mark.parametrize("c", GN_SHAPES, ids=[f"{c.B}x{c.S}x{c.C}" for c in GN_SHAPES])
def test_channel_stats_geometry_edges(c):
    """per (image, channel) against the exact sums, under the bound of the kernel's own chain;
    the int64 output zeroed between canaries"""
    x = ko.gn_case_inputs(c)[0]
    st = zeroed_stats(c.B, c.C, 2)
    ext().channel_stats(P(x), st.view)
    torch.cuda.synchronize()
    ko.check_guards(st)
    e = ko.channel_stats_excess(ops.stats_to_float(st.view), x, geometry(c)["two_pass"])
    print(f"channel_stats {c.B}x{c.S}x{c.C}: worst statistic at {e:.3f} of its bound")
    assert e <= 1.0, e


@pytest.mark.parametrize("op", ["group_norm", "channel_stats", "gemm"])
def test_more_than_4096_channels_are_refused_before_any_launch(op):
    """C = 4104 would need a third vector per thread and more than 64 KiB of LDS: the binding
    raises and nothing is written.  ``gemm``: the separate statistics pass a GEMV-sized linear
    (M <= 8) runs over its output, refused before the GEMM itself is launched"""
    C = ko.GN_MAX_C + 8
    x = torch.ones(1, 2, C, dtype=ko.BF16, device=DEV)
    if op == "group_norm":
        g = G(x.shape)
        with pytest.raises(RuntimeError, match="C <= 4096"):
            ext().group_norm(x, x[0, 0], x[0, 0], g.view, 8, 1e-5, 0)
    elif op == "gemm":
        g, st = G((1, 2, C)), zeroed_stats(1, C, 2)
        with pytest.raises(RuntimeError, match="N <= 4096"):
            ops.linear(torch.ones(1, 2, 8, dtype=ko.BF16, device=DEV), torch.ones(C, 8, dtype=ko.BF16, device=DEV),
                       stats=st.view, out=g.view)
        torch.cuda.synchronize()
        ko.check_guards(st)
        assert not st.view.any()
    else:
        g = zeroed_stats(1, C, 2)
        with pytest.raises(RuntimeError, match="C <= 4096"):
            ext().channel_stats(x, g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    want = 0 if op == "channel_stats" else g.pattern
    assert bool((ko.int_view(g.view) == want).all())


# ------------------------------------------------------------------------------ row norms
@pytest.mark.parametrize("rows,D", ko.ROW_NORM_CASES)
def test_layer_norm_without_beta_and_row_stats_edges(rows, D):
    """(with beta, rms_norm and embed_layer_norm: test_kernel_edges_gpu.py::test_row_norm_edges,
    on the same cases and data)"""
    x, gam, _ = ko.norm_inputs(rows, D)
    xp = P(x)
    g = G((rows, D))
    ext().layer_norm(xp, P(gam), None, g.view, 1e-5)
    check(g, ref.layer_norm(x, gam, None, 1e-5, dtype=F64), "norm", f"layer_norm, no beta {rows}x{D}", (1, None))
    rs = G((rows, 2), torch.float32)
    ext().row_stats(xp, rs.view, 1e-5)
    torch.cuda.synchronize()
    ko.check_guards(rs)
    e = ko.row_stats_err(rs.view[:, 0], rs.view[:, 1], x)
    print(f"row_stats {rows}x{D}: mean {e[0]:.2e} of a deviation, rstd {e[1]:.2e} relative (bounds {ko.ROW_STATS_BOUND})")
    assert e[0] <= BOUND["row_stats mean"] and e[1] <= BOUND["row_stats rstd"], e
