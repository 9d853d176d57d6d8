"""The route of a GEMM call (``gemm_route``, ops/csrc/gemm.hip) as the extension reports it after the
launch: which kernel ran, in which A-operand mode and tile, and the passes before and after it.
The CPU golden (tests/golden/gemm_routes.txt, tests/test_gemm_menu.py) pins the whole decision; here
one call per edge runs on the GPU, with the numerics checks and tolerances of tests/test_kernels_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cassmantle_amd import ops  # noqa: E402
from cassmantle_amd.ops import reference as ref  # noqa: E402
from cassmantle_amd.ops._ext import ext  # noqa: E402
from test_kernels_gpu import DEV, force_cfg, rel_err, rnd  # noqa: E402,F401


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    from cassmantle_amd.ops._ext import ext_available, ext_error
    assert ext_available(), ext_error()
    ops.set_mode("hip")


def route():
    """(kernel, mode, cfg, split, pre, post_stats) of this thread's last GEMM"""
    return tuple(ext().gemm_last_route())


def test_simt_linear_and_its_statistics_pass():
    """K = 4: the SIMT kernel; it fuses no statistics, so ``stats=`` is a pass over the output (the
    same kernel on the same input as ops.channel_stats: equal to the bit)"""
    x = rnd(2, 8, 4, seed=301)
    w = rnd(8, 4, scale=0.5, seed=302)
    b = rnd(8, scale=0.1, seed=303)
    out = ops.linear(x, w, b)
    assert route()[0] == "simt" and route()[4:] == ("none", False)
    assert rel_err(out, ref.linear(x, w, b)) < 1e-2
    st = ops.new_stats(2, 8, DEV)
    out2 = ops.linear(x, w, b, stats=st)
    assert route()[0] == "simt" and route()[4:] == ("none", True)
    assert torch.equal(out2, out)
    exp = ops.new_stats(2, 8, DEV)
    ops.channel_stats(out2, exp)
    assert int(st.abs().sum()) > 0 and torch.equal(st, exp)


def test_skinny_linear_is_the_gemv():
    x = rnd(4, 64, seed=304)
    w = rnd(64, 64, scale=64 ** -0.5, seed=305)
    out = ops.linear(x, w)
    assert route()[0] == "gemv" and route()[3:] == (1, "none", False)
    assert rel_err(out, ref.linear(x, w)) < 1e-2


@pytest.mark.parametrize("K,areg,pre", [(320, True, "none"), (1280, False, "row_stats")])
def test_ln_linear_statistics_in_kernel_or_in_a_pass(K, areg, pre):
    rows, N = 64, 64
    x = rnd(rows, K, seed=306) * 1.5 + 0.3
    g = rnd(K, seed=307) * 0.3 + 1
    be = rnd(K, seed=308) * 0.2
    w = rnd(N, K, scale=K ** -0.5, seed=309)
    b = rnd(N, scale=0.1, seed=310)
    out = ops.ln_linear(x, g, be, 1e-5, w, b, fold=ops.ln_fold(g, be, w, b))
    assert (route()[0] == "areg", route()[4], route()[5]) == (areg, pre, False)
    assert rel_err(out, ref.linear(ref.layer_norm(x, g, be, 1e-5), w, b)) < 1.5e-2


@pytest.mark.parametrize("S,areg,pre", [(256, True, "none"), (64, False, "gn_apply")])
def test_gn_linear_fold_in_kernel_or_applied_first(S, areg, pre):
    C, N = 320, 64
    x = rnd(1, S, C, seed=311) * 1.5 + 0.3
    st = ops.new_stats(1, C, DEV)
    ops.channel_stats_ref(x, st)
    g = rnd(C, seed=312) * 0.5 + 1
    be = rnd(C, seed=313) * 0.2
    w = rnd(N, C, scale=C ** -0.5, seed=314)
    b = rnd(N, scale=0.1, seed=315)
    out = ops.gn_linear(x, st, g, be, 32, 1e-6, w, b)
    assert (route()[0] == "areg", route()[4], route()[5]) == (areg, pre, False)
    exp = ref.linear(ref.group_norm(x.float(), 32, g.float(), be.float(), 1e-6, False).to(torch.bfloat16), w, b)
    assert rel_err(out, exp) < 1e-2


def test_fp32_output_takes_the_statistics_pass():
    M, N, K = 128, 64, 128
    x = rnd(M, K, seed=316)
    w = rnd(N, K, scale=K ** -0.5, seed=317)
    out = torch.empty(M, N, device=DEV, dtype=torch.float32)
    ext().gemm(x, w, None, None, out, 0, ops.new_stats(1, N, DEV), M)
    assert route()[0] == "tiles" and route()[4:] == ("none", True)
    assert rel_err(out, ref.linear(x, w)) < 1e-2


@pytest.mark.parametrize("cfg,runs,kernel", [(7, 9, "pingpong"), (13, 12, "tiles")])
def test_forced_tile_without_gated_instantiation(cfg, runs, kernel, force_cfg):  # noqa: F811
    """a gated call forced onto a ping-pong / deep-ring tile that has no gated wave layout runs its
    family's gated default: the planner says so, and the route names the tile that ran"""
    M, N, K = 256, 64, 128
    x = rnd(M, K, seed=318)
    w = rnd(2 * N, K, scale=K ** -0.5, seed=319)
    b = rnd(2 * N, scale=0.1, seed=320)
    force_cfg(cfg, 1)
    out = ops.linear(x, w, b, act="geglu")
    force_cfg(-1)
    assert tuple(ext().gemm_last_plan()) == (runs, 1)
    assert route()[:4] == (kernel, "c0_buf", runs, 1)
    assert rel_err(out, ref.linear(x, w, b, act="geglu")) < 1e-2


def test_gated_call_no_kernel_takes_is_refused():
    """GEGLU on 33 rows with a row stride that is no multiple of 8: not the GEMV (> 8 rows), not the
    MFMA tiles (16-byte row loads), and the SIMT kernel has no gate.  A host check: nothing is
    launched and the output is not written"""
    M, N, K = 33, 64, 64
    x = rnd(M, K + 4, seed=321)[:, :K]
    assert x.stride(0) == K + 4
    w = rnd(2 * N, K, scale=K ** -0.5, seed=322)
    out = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="gated"):
        ext().gemm(x, w, None, None, out, 4, None, 0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
