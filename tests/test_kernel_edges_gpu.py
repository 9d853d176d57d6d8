"""Every HIP kernel at its edges, with the three instruments of kernel_oracle.py at once: inputs
that sit in NaN (:func:`kernel_oracle.poisoned`), an output between two canary regions
(:func:`kernel_oracle.guarded`) and the worst per-block error against an fp64 reference of the
same bf16 inputs (:func:`kernel_oracle.block_rel_err`) under the family's existing whole-tensor
tolerance.  Shapes: one full tile, one partial tile and a tail.  The attention data makes the edge
keys matter (kernel_oracle.attn_data).  test_kernel_oracle.py shows, without a GPU, that these
checks reject the bugs the whole-tensor error lets through and accept the ideal kernel."""
import os

import pytest
import torch

import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.ops import reference as ref
from cassmantle_amd.ops._ext import ext, ext_available, ext_error
from kernel_oracle import BF16, BOUND, F64, block_rel_err
from test_gemm_menu import header_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"
MENU = [tuple(r) for r in ext().gemm_tile_menu()] if ext_available() else header_rows()
TILE = {r[0]: r for r in MENU}
QBLOCK = (1, 16, 1, None)          # 16 queries x d per (batch, head)


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    assert ext_available(), ext_error()
    ops.set_mode("hip")


@pytest.fixture
def force_cfg():
    yield lambda c, s=0: ext().gemm_set_override(c, s)
    ext().gemm_set_override(-1, 0)


def P(t, strided=False, row_dims=1):
    return None if t is None else ko.poisoned(t, strided, row_dims, device=DEV)


def G(shape, dtype=BF16):
    return ko.guarded(shape, dtype, device=DEV)


def zeroed_stats(*shape):
    g = G(shape, torch.int64)
    g.view.zero_()
    return g


def last_plan():
    return tuple(ext().gemm_last_plan())


def check(g, y64, family, what, block=ko.BLOCK_MN, errs=None):
    """guards intact, then the worst block under the family's bound (collected in ``errs`` when
    a test runs several cases, so one failure shows every figure)"""
    torch.cuda.synchronize()
    ko.check_guards(g)
    e = block_rel_err(g.view.reshape(y64.shape), y64, block)
    print(f"{family} {what}: worst block {e:.3e} (bound {BOUND[family]:g})")
    if errs is None:
        assert e < BOUND[family], (family, what, e)
    elif not e < BOUND[family]:
        errs.append((what, e))
    return e


def check_stats(st_view, out_view, B):
    """epilogue GroupNorm statistics against those of the stored output, as test_kernels_gpu.py does"""
    exp = ops.new_stats(B, out_view.shape[-1], DEV)
    ops.channel_stats_ref(out_view.reshape(B, -1, out_view.shape[-1]), exp)
    a, b = ops.stats_to_float(st_view), ops.stats_to_float(exp)
    assert ((a - b).norm() / b.norm()).item() < 1e-4


def gemm_raw(x2, w, bias, r2, out, act, **kw):
    """ops.linear's launch without its contiguity copy: the binding takes row-strided x"""
    ops._launch(ext().gemm, x2, w, bias, r2, out, ops._ACT[act], None, 0, **kw)


# ------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("c", ko.gemm_cases(MENU), ids=lambda c: c.id)
def test_gemm_tile_edges(c, force_cfg):
    x, w, b, r = ko.gemm_inputs(c)
    y64 = ko.linear64(x, w, b, r, c.act)
    wp, bp, rp = P(w), P(b), P(r)
    for xs in (P(x), P(x, strided=True)):
        g = G((c.M, c.N))
        if c.cfg >= 0:
            force_cfg(c.cfg, c.split)
        if xs.is_contiguous():
            ops.linear(xs, wp, bp, residual=rp, act=c.act, out=g.view)
        else:
            assert xs.stride(0) > c.K
            gemm_raw(xs, wp, bp, rp, g.view, c.act)
        if c.cfg >= 0 and c.act == "geglu":
            assert last_plan()[0] == c.cfg                     # a gated row runs its own gated tile
        elif c.cfg >= 0:
            assert last_plan() == (c.cfg, c.split)
        check(g, y64, "gemm", f"{c.id} lda={xs.stride(0)}")


@pytest.mark.parametrize("M,N,K", ko.AREG_CASES)
def test_gemm_areg_edges(M, N, K, force_cfg):
    """the A-in-registers kernel: plain, with the in-kernel LayerNorm, and (N = 72) the
    row-statistics path ln_linear falls back to where that kernel does not take the shape"""
    c = ko.GemmCase(15, 1, M, N, K, "silu")
    x, w, b, r = ko.gemm_inputs(c)
    g = G((M, N))
    force_cfg(15)
    gemm_raw(P(x, strided=True), P(w), P(b), P(r), g.view, "silu")
    assert last_plan()[0] == 15
    force_cfg(-1)
    check(g, ko.linear64(x, w, b, r, "silu"), "gemm", f"areg {M}x{N}x{K}")
    for n in (N, ko.AREG_FALLBACK_N):
        x, gam, be, w, b = ko.ln_fold_inputs(M, n, K, seed=M + K)
        wf, wsum, bf = ops.ln_fold(gam, be, w, b)
        g = G((M, n))
        # (the row-statistics pass of the fallback needs contiguous rows)
        gemm_raw(P(x, strided=n == N), P(wf), P(bf), None, g.view, None, ln_wsum=wsum.to(DEV), ln_eps=1e-5)
        assert (last_plan()[0] == 15) == (n == N)
        check(g, ko.ln_linear64(x, gam, be, w, b), "ln_fold", f"ln_linear {M}x{n}x{K}")


@pytest.mark.parametrize("N,K", [(128, 320), (96, 640), (ko.AREG_FALLBACK_N, 320), (ko.AREG_FALLBACK_N, 640)])
def test_gn_linear_edges(N, K):
    """GroupNorm folded into the A rows of the A-in-registers kernel (B = 1, S = 256); N = 72:
    the GroupNorm-apply kernel + GEMM the binding falls back to"""
    x, gam, be, w, b = ko.ln_fold_inputs(256, N, K, seed=K)
    st = torch.zeros(1, K, 2, dtype=torch.int64)
    ops.channel_stats_ref(x[None], st)
    g = G((256, N))
    areg = N != ko.AREG_FALLBACK_N
    gemm_raw(P(x, strided=areg), P(w), P(b), None, g.view, None, gn_stats=st.to(DEV), gn_gamma=P(gam), gn_beta=P(be),
             gn_groups=32, gn_hw=256, gn_eps=1e-6)
    assert (last_plan()[0] == 15) == areg
    check(g, ko.gn_linear64(x[None], gam, be, 32, 1e-6, w, b)[0], "gn_fold", f"gn_linear 256x{N}x{K}")


@pytest.mark.parametrize("Ca,Cb", ko.CAT_CASES)
def test_linear_cat_edges(Ca, Cb):
    """two-source A with epilogue statistics, M = BM + 1 of the tile the planner picks"""
    M = 129
    for _ in range(2):
        x, w, b, _r = ko.gemm_inputs(ko.GemmCase(-1, 0, M, ko.CAT_N, Ca + Cb, "none"))
        g, st = G((M, ko.CAT_N)), zeroed_stats(1, ko.CAT_N, 2)
        ops._launch(ext().gemm_cat, P(x[:, :Ca].contiguous()), P(x[:, Ca:].contiguous()), P(w), P(b), None, g.view, st.view, M)
        BM = TILE[last_plan()[0]][2]
        if M == BM + 1:
            break
        M = BM + 1
    assert M == BM + 1, (M, last_plan())
    check(g, ko.linear64(x, w, b), "gemm", f"linear_cat {Ca}|{Cb} M={M} plan={last_plan()}")
    ko.check_guards(st)
    check_stats(st.view, g.view[None], 1)


def test_row_stats_producer_and_consumer_edges():
    """linear(row_stats=) -> ln_linear(row_stats=): the fixed-point row sums row by row, then the
    folded consumer that reads them"""
    M, N, K = ko.ROW_STATS_CASE
    x, w, b, r = ko.gemm_inputs(ko.GemmCase(-1, 0, M, N, K, "none"))
    g, rs = G((M, N)), zeroed_stats(M, 2)
    ops.linear(P(x), P(w), P(b), residual=P(r), row_stats=rs.view, out=g.view)
    assert last_plan()[1] == 1
    check(g, ko.linear64(x, w, b, r), "gemm", "row_stats producer")
    ko.check_guards(rs)
    y = g.view.cpu()
    got = ops.stats_to_float(rs.view.cpu().view(1, M, 2))[0]
    yd = y.to(F64)
    for m in range(M):          # the tolerances of test_gemm_row_stats_feed_folded_layernorm, per row
        s, s2 = yd[m].sum().item(), (yd[m] * yd[m]).sum().item()
        assert abs(got[m, 0].item() - s) <= 1e-2 + 1e-4 * abs(s), (m, got[m, 0].item(), s)
        assert abs(got[m, 1].item() - s2) <= 1e-1 + 1e-4 * abs(s2), (m, got[m, 1].item(), s2)
    _, gam, be, w2, b2 = ko.ln_fold_inputs(M, 72, N, seed=77)
    wf, wsum, bf = ops.ln_fold(gam, be, w2, b2)
    g2 = G((M, 72))
    gemm_raw(P(y), P(wf), P(bf), None, g2.view, None, ln_wsum=wsum.to(DEV), ln_eps=1e-5, ln_rows_fx=rs.view)
    check(g2, ko.ln_linear64(y, gam, be, w2, b2), "ln_fold", "row_stats consumer")
    ko.check_guards(rs)


# ------------------------------------------------------------------------------ the tile raster
@pytest.fixture
def raster(force_cfg):
    """gemm_set_raster for plain and gated calls alike; the compiled default and no override afterwards"""
    assert "CASSMANTLE_GEMM_RASTER" not in os.environ, "CASSMANTLE_GEMM_RASTER must be unset: the G = 0 case is the compiled default"
    yield lambda G: ext().gemm_set_raster(G, G)
    ext().gemm_set_raster(0, 0)


@pytest.mark.parametrize("c", ko.raster_gemm_cases(MENU), ids=lambda c: c.id)
def test_gemm_raster_edges(c, force_cfg, raster):
    """6 x 3 tiles under every raster group: a tile the mapping misses stays NaN in the guarded
    output, one it maps outside the grid writes nothing or the guards"""
    assert ko.raster_tiles(c, MENU) == ko.RASTER_TILES
    x, w, b, r = ko.gemm_inputs(c)
    y64 = ko.linear64(x, w, b, r, c.act)
    xp, wp, bp, rp = P(x), P(w), P(b), P(r)
    errs = []
    for G_ in ko.RASTER_GROUPS:
        g = G((c.M, c.N))
        raster(G_)
        force_cfg(c.cfg, c.split)
        ops.linear(xp, wp, bp, residual=rp, act=c.act, out=g.view)
        assert last_plan() == (c.cfg, c.split)
        check(g, y64, "gemm", f"raster G={G_} {c.id}", errs=errs)
    assert errs == []


def test_conv_raster_edges(force_cfg, raster):
    B, H, W, Cin, Cout, stride = ko.RASTER_CONV
    assert (-(-B * H * W // TILE[0][2]), -(-Cout // TILE[0][3])) == ko.RASTER_TILES
    x, w, b, cb, res = ko.conv_inputs(B, H, W, Cin, Cout, stride)
    y64 = ko.conv64(x, w, b, cb, res, stride).flatten(0, 2)
    xp, wp, bp, rp, cbp = P(x), P(w), P(b), P(res), P(cb)
    errs = []
    for G_ in ko.RASTER_GROUPS:
        g, st = G((B, H, W, Cout)), zeroed_stats(B, Cout, 2)
        raster(G_)
        force_cfg(0, 1)
        ops.conv2d(xp, wp, bp, stride=stride, padding=1, residual=rp, chan_bias=cbp, stats=st.view, out=g.view)
        assert last_plan() == (0, 1)
        check(g, y64, "conv", f"raster G={G_} {B}x{H}x{W} {Cin}->{Cout}", errs=errs)
        ko.check_guards(st)
        check_stats(st.view, g.view, B)
    assert errs == []


# ------------------------------------------------------------------------------ conv
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", ko.CONV_CASES)
def test_conv_edges(B, H, W, Cin, Cout, stride):
    x, w, b, cb, res = ko.conv_inputs(B, H, W, Cin, Cout, stride)
    y64 = ko.conv64(x, w, b, cb, res, stride)
    g = G(y64.shape)
    st = zeroed_stats(B, Cout, 2) if Cout % 8 == 0 else None
    ops.conv2d(P(x), P(w), P(b), stride=stride, padding=1, residual=P(res), chan_bias=P(cb),
               stats=None if st is None else st.view, out=g.view)
    check(g, y64.flatten(0, 2), "conv", f"{B}x{H}x{W} {Cin}->{Cout} s{stride} plan={last_plan()}")
    if st is not None:
        ko.check_guards(st)
        check_stats(st.view, g.view, B)


@pytest.mark.parametrize("Cin,forced", [(ko.UP2_CASE[3], None), (ko.UP2_SPLIT_CIN, (1, 2))])
def test_conv_up2_edges(Cin, forced, force_cfg):
    """the four parity-class 2x2 convs; the block error is taken on the interleaved output, so one
    wrong class stands out.  The forced split-K plan needs eight k-tiles (4 Cin = 512): the
    planner gives every slice at least four."""
    B, H, W, _, Cout = ko.UP2_CASE
    x, w, b, cb, res = ko.conv_inputs(B, H, W, Cin, Cout, up=True)
    y64 = ko.conv64(x, w, b, cb, res, up=True)
    g, st = G(y64.shape), zeroed_stats(B, Cout, 2)
    if forced:
        force_cfg(*forced)
    ops._launch(ext().conv2d_up2, P(x), P(ops.fold_upsample_weights(w)), P(b), P(res), P(cb), g.view, st.view)
    if forced:
        assert last_plan() == forced
    check(g, y64.flatten(0, 2), "conv", f"up2 Cin={Cin} plan={last_plan()}")
    ko.check_guards(st)
    check_stats(st.view, g.view, B)


# ------------------------------------------------------------------------------ attention
def attn_reference(c):
    """q, k, v and the fp64 reference of a case (for a case that runs under more than one kernel)"""
    q, k, v = ko.attn_data(c)
    return q, k, v, ko.attention64(q, k, v, c.lens, c.causal)


def run_attention(c, errs, family="attention", fp8=False, prepack=False, what="", data=None):
    q, k, v, o64 = attn_reference(c) if data is None else data
    qp, kp, vp = (P(t, strided=True, row_dims=2) for t in (q, k, v))
    assert (c.Nq == 1 or qp.stride(1) > c.H * c.d) and (c.Nk == 1 or kp.stride(1) > c.Hk * c.d)
    lens = None if c.lens is None else torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    g = G(q.shape)
    kv8 = None
    if prepack:
        kv8 = G((int(ext().attention_fp8_bytes(c.B, c.Nk, c.Hk)),), torch.uint8)
        assert ops.pack_kv_fp8(kp, vp, lens, out=kv8.view).data_ptr() == kv8.view.data_ptr()
    ext().attention(qp, kp, vp, g.view, c.d ** -0.5, int(c.causal), lens, int(fp8), None if kv8 is None else kv8.view)
    check(g, o64, family, f"{what}{c.id}", QBLOCK, errs)
    if kv8 is not None:
        ko.check_guards(kv8)
    if c.lens is not None and c.lens[-1] == 0:
        assert not g.view[-1].any(), "a batch without a valid key must come out as zeros"


@pytest.mark.parametrize("d", [32, 64, 80, 160])
def test_attention_generic_edges(d):
    errs = []
    for c in ko.attn_cases(d):
        run_attention(c, errs)
    assert errs == []


@pytest.mark.parametrize("variant", ["16x16", "32x32"])
def test_attention_d40_edges(variant):
    errs = []
    ops.set_attention_d40_variant(variant)
    try:
        for c in ko.attn_cases(40):
            run_attention(c, errs, what=variant + " ")
    finally:
        ops.set_attention_d40_variant(None)
    assert errs == []


def test_attention_d512_edges():
    errs = []
    for c in ko.attn_cases(512) + [ko.D512_SPLIT_CASE]:
        run_attention(c, errs)
    assert errs == []


def test_attention_gqa_causal_edges():
    errs = []
    run_attention(ko.GQA_CASE, errs)
    assert errs == []


def last_kernel():
    return tuple(ext().attention_last_kernel())


@pytest.fixture
def default_attention_dispatch():
    """the kernels the cases below name are the ones launch_attention picks with its A/B knobs unset"""
    for var in ko.ATTN_KNOBS:
        assert var not in os.environ, f"{var} must be unset: it changes which attention kernel a shape launches"


def test_attention_last_kernel_follows_every_launcher(default_attention_dispatch):
    """the record is overwritten by the fp8 and d = 512 launchers too, so it is never another call's"""
    errs = []
    c = ko.attn_cases(64)[6]
    run_attention(c, errs)
    assert last_kernel()[:3] == ("fwd", 64, 64)
    run_attention(c, errs, "fp8", fp8=True)
    assert last_kernel()[:3] == ("fp8", 64, 64) and last_kernel()[3] in (4, 8)
    run_attention(ko.attn_cases(512)[6], errs)
    assert last_kernel() == ("d512", 512, 512, 8)
    run_attention(ko.attn_cases(40)[6], errs)
    assert last_kernel()[0] == "a16"
    assert errs == []


@pytest.mark.parametrize("d", ko.ATTN_ROUNDUP_D)
def test_attention_roundup_edges(d, default_attention_dispatch):
    """a head dim below each template width (zero-filled columns in LDS, stores cut at d), and
    the 96- and 128-wide templates at their own width"""
    w = ko.attn_template_width(d)
    errs = []
    for c in ko.attn_cases(d):
        run_attention(c, errs)
        assert last_kernel()[:3] == ("fwd", w, w), (c.id, last_kernel())
    assert errs == []


def test_attention_lm_prefill_edges(default_attention_dispatch):
    """models/lm.py's prefill call: d = 128, four query heads per K/V head, lens or causal, Q/K/V
    strided views as the KV cache's; then causal over five key tiles in 4-wave blocks"""
    errs, waves = [], set()
    for c in ko.attn_cases(128, *ko.LM_HEADS):
        run_attention(c, errs)
        assert last_kernel()[:3] == ("fwd", 128, 128), (c.id, last_kernel())
        waves.add(last_kernel()[3])
    assert waves == {2, 4}
    run_attention(ko.PREFILL_CASE, errs, what="prefill ")
    assert last_kernel() == ko.PREFILL_KERNEL
    assert errs == []


@pytest.mark.parametrize("c,kernel,kernel_32x32", ko.ATTN_WIDE_CASES, ids=[c.id for c, _, _ in ko.ATTN_WIDE_CASES])
def test_attention_wide_grid_edges(c, kernel, kernel_32x32, default_attention_dispatch):
    """the grids that reach the 8-wave blocks, the 8-wave 16x16 d = 40 kernel and the 512-block
    rule; the d = 40 row also under the 32x32 variant, on the same data"""
    errs, data = [], attn_reference(c)
    run_attention(c, errs, what=f"B={c.B} ", data=data)
    assert last_kernel() == kernel, (c.id, last_kernel())
    if kernel_32x32 is not None:
        try:
            for variant, want in (("16x16", kernel), ("32x32", kernel_32x32)):
                ops.set_attention_d40_variant(variant)
                run_attention(c, errs, what=f"{variant} B={c.B} ", data=data)
                assert last_kernel() == want, (c.id, variant, last_kernel())
        finally:
            ops.set_attention_d40_variant(None)
    assert errs == []


@pytest.mark.parametrize("prepack", [False, True], ids=["per_call_pack", "pack_kv_fp8"])
@pytest.mark.parametrize("variant", ops.FP8_ATTN_VARIANTS)
def test_attention_fp8_edges(variant, prepack):
    errs = []
    ops.set_fp8_attention_variant(variant)
    try:
        for c in ko.attn_cases(64):
            run_attention(c, errs, "fp8", fp8=True, prepack=prepack, what=variant + " ")
    finally:
        ops.set_fp8_attention_variant(None)
    assert errs == []


def test_attention_d256_gemm_fallback_edges():
    """bmm_nt -> softmax_rows -> bmm_nt; ops.attention allocates the pieces, so the inputs are
    poisoned here and bmm_nt gets its guarded output in test_bmm_nt_edges"""
    errs = []
    for c in ko.attn_cases(256):
        q, k, v = ko.attn_data(c)
        lens = None if c.lens is None else torch.tensor(c.lens, dtype=torch.int32, device=DEV)
        out = ops.attention(*(P(t, strided=True, row_dims=2) for t in (q, k, v)), causal=c.causal, kv_lens=lens)
        torch.cuda.synchronize()
        e = block_rel_err(out, ko.attention64(q, k, v, c.lens, c.causal), QBLOCK)
        print(f"attention d256 {c.id}: worst block {e:.3e}")
        if not e < BOUND["attention"]:
            errs.append((c.id, e))
    assert errs == []


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_bmm_nt_edges(dtype):
    a, b = ko.rnd(2, 33, 72, seed=1), ko.rnd(2, 65, 72, seed=2)
    g = G((2, 33, 65), dtype)
    ext().bmm_nt(P(a, strided=True), P(b, strided=True), g.view, 0.5)
    y64 = 0.5 * a.to(F64) @ b.to(F64).transpose(1, 2)
    check(g, y64, "gemm", f"bmm_nt {dtype}", (1, 16, 16))


@pytest.mark.parametrize("group", ko.DECODE_GROUPS)
@pytest.mark.parametrize("L", ko.DECODE_L)
def test_decode_attention_edges(L, group):
    q, kc, vc, lens = ko.decode_data(L, group)
    g = G(q.shape)
    ext().decode_attention(P(q, strided=True, row_dims=2), P(kc), P(vc), torch.tensor(lens, dtype=torch.int32, device=DEV),
                           g.view, 64 ** -0.5)
    check(g, ko.decode64(q, kc, vc, lens), "decode", f"L={L} group={group}", (1, 1, None))


def test_decode_attention_empty_sequence_is_zero():
    q, kc, vc, _ = ko.decode_data(129, 2)
    g = G(q.shape)
    ext().decode_attention(P(q), P(kc), P(vc), torch.tensor([129, 0, 5], dtype=torch.int32, device=DEV), g.view, 64 ** -0.5)
    torch.cuda.synchronize()
    ko.check_guards(g)
    assert not g.view[1].any() and torch.isfinite(g.view.float()).all()


# ------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("rows,D", ko.ROW_NORM_CASES)
def test_row_norm_edges(rows, D):
    x, gam, be = ko.norm_inputs(rows, D)
    g = G((rows, D))
    ext().layer_norm(P(x), P(gam), P(be), g.view, 1e-5)
    check(g, ref.layer_norm(x, gam, be, 1e-5, dtype=F64), "norm", f"layer_norm {rows}x{D}", (1, None))
    g = G((rows, D))
    ext().rms_norm(P(x), P(gam), g.view, 1e-5)
    check(g, ref.rms_norm(x, gam, 1e-5, dtype=F64), "norm", f"rms_norm {rows}x{D}", (1, None))
    word, ids, pos, add = ko.embed_inputs(rows, D)
    g = G((1, rows, D))
    ext().embed_layer_norm(P(word), ids.to(DEV).view(-1), P(pos), rows, P(add), P(gam), P(be), g.view, 1e-5)
    check(g, ko.embed_ln64(word, ids, pos, add, gam, be), "norm", f"embed_layer_norm {rows}x{D}", (1, 1, None))


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("B,S,C,G_", ko.GN_CASES)
def test_group_norm_edges(B, S, C, G_, silu):
    x, gam, be = ko.gn_inputs(B, S, C)
    y64 = ref.group_norm(x, G_, gam, be, 1e-5, silu, dtype=F64)
    block = (1, 16, C // G_)
    st = torch.zeros(B, C, 2, dtype=torch.int64)
    ops.channel_stats_ref(x, st)
    st, Ca = st.to(DEV), C // 2
    g = G(x.shape)
    ext().group_norm(P(x), P(gam), P(be), g.view, G_, 1e-5, int(silu))
    check(g, y64, "group_norm", f"group_norm {B}x{S}x{C}/{G_}", block)
    g = G(x.shape)
    ext().group_norm_stats(P(x), st, None, P(gam), P(be), g.view, G_, 1e-5, int(silu))
    check(g, y64, "group_norm", f"group_norm_stats {B}x{S}x{C}/{G_}", block)
    g = G(x.shape)
    ext().group_norm_cat(P(x[..., :Ca].contiguous()), P(x[..., Ca:].contiguous()), st[:, :Ca].contiguous(),
                         st[:, Ca:].contiguous(), P(gam), P(be), g.view, G_, 1e-5, int(silu))
    check(g, y64, "group_norm", f"group_norm_cat {B}x{S}x{C}/{G_}", block)


# ------------------------------------------------------------------------------ rope_kv
@pytest.mark.parametrize("B,T,H,Hk,d,L,pos0", ko.ROPE_CASES)
def test_rope_kv_edges(B, T, H, Hk, d, L, pos0):
    """guarded caches pre-filled with the pattern: every position outside [pos0, pos0 + T) stays
    bit-identical, pos0 + T reaching L exactly included"""
    assert max(pos0) + T == L
    qkv = ko.rnd(B, T, (H + 2 * Hk) * d, seed=T + d)
    q64, k64, v64 = ko.rope64(qkv, pos0, H, Hk, d)
    qg, kg, vg = G((B, T, H, d)), G((B, L, Hk, d)), G((B, L, Hk, d))
    flat = P(qkv.flatten(0, 1), strided=True)                  # token stride = row + 16, tokens packed per batch
    ld = qkv.shape[-1] + 16
    qkv_p = torch.as_strided(flat, qkv.shape, (T * ld, ld, 1), flat.storage_offset())
    assert torch.equal(qkv_p.cpu(), qkv)
    ext().rope_kv(qkv_p, torch.tensor(pos0, dtype=torch.int32, device=DEV), qg.view, kg.view, vg.view, H, Hk, 10000.0)
    check(qg, q64, "rope", f"q {B}x{T}x{H}x{d}", (1, 1, 1, None))
    torch.cuda.synchronize()
    ko.check_guards(kg, vg)
    written = torch.zeros(B, L, dtype=torch.bool)
    for b in range(B):
        written[b, pos0[b]:pos0[b] + T] = True
    for name, cg, y64 in (("k", kg, k64), ("v", vg, v64)):
        cache = cg.view.cpu()
        assert bool((ko.int_view(cache)[~written] == cg.pattern).all()), f"{name} cache written outside [pos0, pos0 + T)"
        got = torch.stack([cache[b, pos0[b]:pos0[b] + T] for b in range(B)])
        e = block_rel_err(got, y64, (1, 1, 1, None))
        print(f"rope {name} cache: worst block {e:.3e}")
        assert e < BOUND["rope"], (name, e)
    assert torch.equal(torch.stack([vg.view.cpu()[b, pos0[b]:pos0[b] + T] for b in range(B)]).to(F64), v64)
