"""The decode path (lm.hip) at its edges with the instruments of kernel_oracle.py: the skinny-M
GEMV at every column tail, k-loop edge and operand form, the dispatch boundary between it and the
MFMA GEMM (M = 8 | 9), decode attention at d = 128, every group size's ends and above 4096 keys,
and the sampler held to exact equality with ``ops.reference.lm_sample`` under rank probes.
Inputs sit in NaN, outputs between canaries, errors are per block against fp64 of the same
inputs; test_kernel_oracle.py proves these checks on planted bugs without a GPU."""
import pytest
import torch

import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.ops import reference as ref
from cassmantle_amd.ops._ext import ext, ext_available, ext_error
from kernel_oracle import BF16, BOUND, F64, block_rel_err
from test_kernel_edges_gpu import DEV, G, P, check, check_stats, gemm_raw, zeroed_stats

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    assert ext_available(), ext_error()
    ops.set_mode("hip")


# ------------------------------------------------------------------------------ GEMV
@pytest.mark.parametrize("c", ko.GEMV_CASES, ids=lambda c: c.id)
def test_gemv_edges(c):
    """contiguous and row-strided x; the block is the kernel's own: one row x the 4 (2) columns
    of a thread block"""
    x, w, b, r = ko.gemv_inputs(c)
    y64 = ko.linear64(x, w, b, r, c.act)
    wp, bp, rp = P(w), P(b), P(r)
    for xs in (P(x), P(x, strided=True)):
        g = G((c.M, c.N))
        assert xs.is_contiguous() or xs.stride(0) > c.K
        gemm_raw(xs, wp, bp, rp, g.view, c.act)
        check(g, y64, "gemm", f"gemv {c.id} lda={xs.stride(0)}", c.block)


def test_gemv_through_linear_with_strided_x_and_the_simt_fallback():
    """ops.linear makes a strided x contiguous first; K % 8 != 0 is not the GEMV's: the SIMT
    kernel takes it and must match as well"""
    for c in (ko.GemvCase(3, 7, 72, "silu"), ko.GEMV_SIMT_CASE):
        x, w, b, r = ko.gemv_inputs(c)
        g = G((c.M, c.N))
        ops.linear(P(x, strided=True), P(w), P(b), residual=P(r), act=c.act, out=g.view)
        check(g, ko.linear64(x, w, b, r, c.act), "gemm", f"linear {c.id}", c.block)


@pytest.mark.parametrize("c", ko.RMS_CASES, ids=lambda c: c.id)
def test_gemv_rms_prologue_edges(c):
    """every row has its own scale, so a 1/rms taken from another row shows"""
    x, gam, w, b, r = ko.rms_inputs(c)
    y64 = ko.rms_linear64(x, gam, w, b, r, c.act)
    y = ops.rms_linear(P(x), P(gam), 1e-5, P(w), P(b), residual=P(r), act=c.act)
    torch.cuda.synchronize()
    e = block_rel_err(y, y64, c.block)
    print(f"rms_linear {c.id}: worst block {e:.3e}")
    assert e < BOUND["gemm"], (c.id, e)
    g = G((c.M, c.N))                                         # the binding itself: strided x, guarded out
    ext().gemm_rms(P(x, strided=True), P(gam), 1e-5, P(w), P(b), P(r), g.view, ops._ACT[c.act])
    check(g, y64, "gemm", f"gemm_rms {c.id}", c.block)


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("Bt,M,N,K", ko.BMM_GEMV_CASES)
def test_gemv_bmm_nt_edges(Bt, M, N, K, dtype):
    """<= 8 rows per batch: blockIdx.z, the batch strides, alpha and the fp32 store of the GEMV"""
    a, b = ko.rnd(Bt, M, K, seed=M), ko.rnd(Bt, N, K, seed=M + 1)
    g = G((Bt, M, N), dtype)
    ap, bp = P(a, strided=True), P(b, strided=True)
    assert ap.stride(0) > M * ap.stride(1) and bp.stride(1) > K
    ext().bmm_nt(ap, bp, g.view, ko.BMM_ALPHA)
    check(g, ko.BMM_ALPHA * a.to(F64) @ b.to(F64).transpose(1, 2), "gemm", f"bmm_nt M={M} {dtype}", (1, 1, 4))


# ------------------------------------------------------------------------------ the GEMV | MFMA boundary
@pytest.mark.parametrize("M", ko.DISPATCH_M)
def test_dispatch_boundary_linear_stats_and_linear_cat(M):
    """the GEMV has no statistics epilogue and no second A: at M = 8 the binding's separate
    statistics pass and the wrapper's concatenation stand in, at M = 9 the MFMA epilogue"""
    N, K = ko.DISPATCH_NK
    c = ko.GemvCase(M, N, K, "none")
    x, w, b, r = ko.gemv_inputs(c)
    y64 = ko.linear64(x, w, b, r)
    g, st = G((1, M, N)), zeroed_stats(1, N, 2)
    ops.linear(P(x)[None], P(w), P(b), residual=P(r)[None], stats=st.view, out=g.view)
    check(g, y64[None], "gemm", f"linear stats M={M}", (1, 1, 4))
    ko.check_guards(st)
    check_stats(st.view, g.view, 1)
    st = zeroed_stats(1, N, 2)
    Ca = K // 2
    y = ops.linear_cat(P(x[:, :Ca].contiguous())[None], P(x[:, Ca:].contiguous())[None], P(w), P(b), residual=P(r)[None],
                       stats=st.view)
    torch.cuda.synchronize()
    ko.check_guards(st)
    e = block_rel_err(y, y64[None], (1, 1, 4))
    print(f"linear_cat M={M}: worst block {e:.3e}")
    assert e < BOUND["gemm"], e
    check_stats(st.view, y, 1)


@pytest.mark.parametrize("M", ko.DISPATCH_M)
def test_dispatch_boundary_ln_linear(M):
    """rows <= 8: LayerNorm kernel + GEMV; 9 rows: the fold with its row-statistics pass"""
    N, K = ko.DISPATCH_NK
    x, gam, be, w, b = ko.ln_fold_inputs(M, N, K, seed=M)
    y = ops.ln_linear(P(x), P(gam), P(be), 1e-5, P(w), P(b), fold=tuple(P(t) for t in ops.ln_fold(gam, be, w, b)))
    torch.cuda.synchronize()
    e = block_rel_err(y, ko.ln_linear64(x, gam, be, w, b), (1, None))
    print(f"ln_linear M={M}: worst block {e:.3e}")
    assert e < BOUND["ln_fold"], e


def test_dispatch_boundary_row_stats_producer():
    """9 rows is the first shape with a row-statistics epilogue; 8 rows must be refused, not
    handed to the GEMV, which would leave the statistics at zero"""
    N, K = ko.DISPATCH_NK
    x, w, b, r = ko.gemv_inputs(ko.GemvCase(9, N, K, "none"))
    g, rs = G((9, N)), zeroed_stats(9, 2)
    ops.linear(P(x), P(w), P(b), residual=P(r), row_stats=rs.view, out=g.view)
    check(g, ko.linear64(x, w, b, r), "gemm", "row_stats producer M=9", (1, 4))
    ko.check_guards(rs)
    yd = g.view.cpu().to(F64)
    got = ops.stats_to_float(rs.view.cpu().view(1, 9, 2))[0]
    for m in range(9):          # the tolerances of test_gemm_row_stats_feed_folded_layernorm, per row
        s, s2 = yd[m].sum().item(), (yd[m] * yd[m]).sum().item()
        assert abs(got[m, 0].item() - s) <= 1e-2 + 1e-4 * abs(s), (m, got[m, 0].item(), s)
        assert abs(got[m, 1].item() - s2) <= 1e-1 + 1e-4 * abs(s2), (m, got[m, 1].item(), s2)


@pytest.mark.parametrize("what", ["ln_wsum", "ln_rows_fx", "row_stats", "A2"])
def test_gemv_rows_with_an_argument_the_gemv_ignores_are_refused(what):
    N, K = ko.DISPATCH_NK
    x, gam, be, w, b = (t.to(DEV) for t in ko.ln_fold_inputs(8, N, K, seed=8))
    wf, wsum, bf = ops.ln_fold(gam, be, w, b)
    out = G((8, N))
    rs = zeroed_stats(8, 2)
    with pytest.raises(RuntimeError):
        if what == "ln_wsum":
            ext().gemm(x, wf, bf, None, out.view, 0, None, 0, ln_wsum=wsum, ln_eps=1e-5)
        elif what == "ln_rows_fx":
            ext().gemm(x, wf, bf, None, out.view, 0, None, 0, ln_wsum=wsum, ln_eps=1e-5, ln_rows_fx=rs.view)
        elif what == "row_stats":
            ext().gemm(x, w, b, None, out.view, 0, None, 0, row_stats=rs.view)
        else:
            ext().gemm_cat(x[:, :64].contiguous(), x[:, 64:].contiguous(), w, b, None, out.view, None, 0)
    torch.cuda.synchronize()
    ko.check_guards(out, rs)
    assert bool((ko.int_view(out.view) == out.pattern).all()) and not rs.view.any(), "a refused call wrote something"


# ------------------------------------------------------------------------------ decode attention
@pytest.mark.parametrize("L,group,d,lens", ko.DECODE_EDGE_CASES)
def test_decode_attention_head_dim_group_and_long_context_edges(L, group, d, lens):
    q, kc, vc, ln = ko.decode_edge_data(L, group, d, lens)
    g = G(q.shape)
    ext().decode_attention(P(q, strided=True, row_dims=2), P(kc), P(vc), torch.tensor(ln, dtype=torch.int32, device=DEV),
                           g.view, d ** -0.5)
    check(g, ko.decode64(q, kc, vc, ln), "decode", f"L={L} group={group} d={d} lens={ln}", (1, 1, None))


# ------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("T", [1.0, 0.8])
@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("c", ko.SAMPLER_CASES, ids=lambda c: c.name)
def test_lm_sample_rank_probes(c, dtype, T):
    """+1e4 of noise on the id ranked k - 1, k and k + 1 of the reference's order, one chained
    step each, then a step of Gumbel noise: out, tok, pos, lens and step equal the reference's,
    and a probed id wins exactly when it is inside the top k (and its value is finite)"""
    lg = c.logits.to(dtype)
    noise, ids, inside = ko.rank_probes(lg, T, c.k, c.eos, c.eos_bias)
    want = ko.run_sampler(ref.lm_sample, lg, noise, T, c.k, c.eos, c.eos_bias)
    V, n = lg.numel(), noise.shape[0]
    lgp, nzp = P(lg.reshape(1, V)), P(noise)
    out = ko.guarded((n, 1), torch.int64, device=DEV)
    state = ko.guarded((4,), torch.int64, device=DEV)           # step, tok and (as int32) pos, lens
    state.view.zero_()
    step, tok = state.view[0:1], state.view[1:2]
    pos, lens = state.view[2:3].view(torch.int32)[:1], state.view[3:4].view(torch.int32)[:1]
    lens.fill_(1)
    eb = P(torch.full((n,), c.eos_bias))
    for _ in range(n):
        ops.lm_sample(lgp, nzp, eb, c.eos, T, c.k, step, out.view, tok, pos, lens)
    torch.cuda.synchronize()
    ko.check_guards(out, state)
    got = (out.view.flatten().tolist(), int(tok), int(pos), int(lens), int(step))
    print(f"lm_sample {c.name} {dtype} T={T}: probed ids {ids} inside {inside} -> {got[0]} (reference {want[0]})")
    assert got == want, (c.name, got, want)
    v = ko.sample_values(lg, T, c.eos, c.eos_bias)
    for t, tid, ins in zip(got[0], ids, inside):
        if bool(torch.isfinite(v[tid])):
            assert (t == tid) == ins, (c.name, t, tid, ins)
