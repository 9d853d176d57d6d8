"""The scorer and the glue kernels (misc.hip) at their edges with the instruments of
kernel_oracle.py: the cosine kernels against fp64 of the same inputs at one absolute tolerance
for fp32 and bf16 tables, mean_pool_l2 per row with NaN in every padding token, cosine_topk
against the fp64 scores around one 2048-row chunk and across merge passes, and the byte-moving
kernels bit for bit at their 8- and 16-byte vector tails.  Inputs sit in NaN, outputs between
canaries; test_kernel_oracle.py proves the checks on planted bugs without a GPU."""
import math

import pytest
import torch

import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.ops._ext import ext, ext_available, ext_error
from kernel_oracle import BF16, BOUND, F64, block_rel_err
from test_kernel_edges_gpu import DEV, G, P

pytestmark = pytest.mark.gpu
TABLE_DTYPES = pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["fp32", "bf16"])


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    assert ext_available(), ext_error()
    ops.set_mode("hip")


def close_to(got, s64, what):
    """|got - fp64| <= COS_ATOL, NaN exactly where the reference is NaN"""
    got = got.detach().to("cpu", F64)
    assert torch.equal(torch.isnan(got), torch.isnan(s64)), (what, got, s64)
    m = ~torch.isnan(s64)
    e = float((got[m] - s64[m]).abs().max()) if m.any() else 0.0
    print(f"{what}: worst |error| {e:.2e} (tolerance {ko.COS_ATOL:g})")
    assert e <= ko.COS_ATOL, (what, e)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((ko.int_view(a.cpu().contiguous()) == ko.int_view(b.cpu().contiguous())).all())


# ------------------------------------------------------------------------------ cosines
@TABLE_DTYPES
@pytest.mark.parametrize("n", ko.COS_N)
@pytest.mark.parametrize("D", ko.COS_D)
def test_gather_cosine_edges(D, n, dtype):
    t = ko.cos_table(D, dtype)
    ia, ib = (torch.tensor(p[:n], dtype=torch.int32) for p in zip(*ko.COS_PAIRS))
    assert int(ia[0]) == ko.COS_ROWS - 1                       # the last valid row of the poisoned table
    tp = P(t)
    for oov in (False, True):
        if oov:                                                # both -1, then either one
            ia[0], ib[0] = -1, -1
            if n > 1:
                ib[1], ia[2] = -1, -1
        s64 = ko.cosine64(t[ia.clamp(min=0).long()], t[ib.clamp(min=0).long()])
        s64[(ia < 0) | (ib < 0)] = math.nan
        g = G((n,), torch.float32)
        ext().gather_cosine(tp, ia.to(DEV), ib.to(DEV), g.view)
        torch.cuda.synchronize()
        ko.check_guards(g)
        close_to(g.view, s64, f"gather_cosine D={D} n={n} {dtype} oov={oov}")
        if not oov and n > 1:
            assert abs(float(g.view[1]) - 1.0) <= ko.COS_ATOL              # a == b
            assert float(g.view[2]) == 0.0                                 # an all-zero row: 0, not NaN


@pytest.mark.parametrize("n", ko.COS_N)
@pytest.mark.parametrize("D", ko.COS_D)
def test_pair_cosine_edges(D, n):
    t = ko.cos_table(D, torch.float32)
    ia, ib = (torch.tensor(p[:n]) for p in zip(*ko.COS_PAIRS))
    a, b = t[ia], t[ib]
    g = G((n,), torch.float32)
    ext().pair_cosine(P(a), P(b), g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    close_to(g.view, ko.cosine64(a, b), f"pair_cosine D={D} n={n}")
    if n > 1:
        assert abs(float(g.view[1]) - 1.0) <= ko.COS_ATOL and float(g.view[2]) == 0.0


@TABLE_DTYPES
@pytest.mark.parametrize("V", ko.COS_N)
@pytest.mark.parametrize("D", ko.COS_D)
def test_cosine_gemv_edges(D, V, dtype):
    t = ko.cos_table(D, dtype)[ko.COS_ROWS - V:]               # V = 5 keeps the zero row
    vec = ko.cos_table(D, dtype, rows=1, seed=1)[0]
    g = G((V,), torch.float32)
    ext().cosine_gemv(P(t), P(vec), g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    close_to(g.view, ko.cosine64(t, vec[None]), f"cosine_gemv D={D} V={V} {dtype}")
    if V == 5:
        assert not t[0].any() and float(g.view[0]) == 0.0
    g = G((V,), torch.float32)                                 # a row against itself
    ext().cosine_gemv(P(t), P(t[V - 1].clone()), g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    assert abs(float(g.view[V - 1]) - 1.0) <= ko.COS_ATOL


# ------------------------------------------------------------------------------ mean_pool_l2
@pytest.mark.parametrize("D", ko.POOL_D)
def test_mean_pool_l2_edges(D):
    """lens = [9, 1, 4, 0, 12] of T = 9: a full row, one token, a partial row, an empty row (the
    zero vector: no token is read, not even the finite token 0) and a length past T"""
    h, lens = ko.pool_inputs(D)
    y64 = ko.mean_pool64(h, lens)
    g = G((len(ko.POOL_LENS), D), torch.float32)
    ext().mean_pool_l2(P(h), lens.to(DEV), g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    e = block_rel_err(g.view, y64, (1, None))
    print(f"mean_pool_l2 D={D}: worst row {e:.3e} (bound {BOUND['pool']:g}); empty row |max| "
          f"{float(g.view[ko.POOL_LENS.index(0)].abs().max()):.3e}")
    assert e < BOUND["pool"], (D, e)
    assert not g.view[ko.POOL_LENS.index(0)].any()


# ------------------------------------------------------------------------------ cosine_topk
@TABLE_DTYPES
@pytest.mark.parametrize("V,k", ko.TOPK_CASES)
def test_cosine_topk_edges(V, k, dtype):
    """(the binding allocates vals and idx itself: no guards here, the table and the query are poisoned)"""
    t, vec, planted = ko.topk_inputs(V, dtype)
    s64 = ko.cosine64(t, vec[None])
    vals, idx = ext().cosine_topk(P(t), P(vec), k)
    torch.cuda.synchronize()
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.shape == idx.shape == (k,)
    assert bool(torch.isfinite(vals).all())
    ko.check_topk(vals, idx, s64, k, planted)
    if k == V:                                                 # every row comes back: negatives and the zero row too
        assert sorted(idx.tolist()) == list(range(V)) and (V == 1 or float(vals.min()) < 0)
        assert V <= ko.COS_ZERO_ROW or float(vals[idx.tolist().index(ko.COS_ZERO_ROW)]) == 0.0


# ------------------------------------------------------------------------------ glue
def test_to_uint8_every_bf16_value():
    """both sides do the same fp32 operations and round half to even: equality, not +-1"""
    x = ko.all_bf16()
    want = ((x.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)
    g = G(x.shape, torch.uint8)
    ext().to_uint8(P(x), g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    bad = (g.view.cpu() != want).nonzero().flatten()
    assert bad.numel() == 0, [(float(x[i]), int(g.view[i]), int(want[i])) for i in bad[:16]]
    assert torch.equal(ops.vae_postprocess(P(x)).cpu(), want)


def test_silu_every_bf16_value():
    """in place on every finite bf16 value: within one bf16 ulp of the rounded fp64 SiLU, the
    underflow range included; both zeros give a zero"""
    x = ko.all_bf16(with_inf=False)
    assert x.numel() % 8 == 0
    want = ko.silu64(x).to(BF16)
    g = G(x.shape)
    g.view.copy_(x)
    ext().silu_(g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    got = g.view.cpu()
    assert bool(torch.isfinite(got.float()).all())
    d = (ko.bf16_ordinal(got) - ko.bf16_ordinal(want)).abs()
    bad = (d > 1).nonzero().flatten()
    print(f"silu_: {int((d == 1).sum())} of {x.numel()} values one ulp off, {bad.numel()} further")
    assert bad.numel() == 0, [(float(x[i]), float(got[i]), float(want[i])) for i in bad[:16]]
    assert not got[x == 0].any()


@pytest.mark.parametrize("bdtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows", ko.GLUE_ROWS)
@pytest.mark.parametrize("Da,Db", [(8, 8), (8, 24), (24, 8)])
def test_concat_last_edges(Da, Db, rows, bdtype):
    a, b = ko.rnd(rows, Da, seed=Da), ko.rnd(rows, Db, seed=Db + 1, dtype=bdtype)
    g = G((rows, Da + Db))
    ext().concat2(P(a), P(b), g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    assert bits_equal(g.view, torch.cat([a, b.to(BF16)], dim=-1))


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("rows,seq", [(1, 1), (3, 2), (4, 3)])
@pytest.mark.parametrize("D", ko.GLUE_D)
def test_gather_add_edges(D, rows, seq, with_pos):
    """rows % seq != 0 where there is more than one row; the last table row is gathered"""
    table, pos = ko.rnd(6, D, seed=D), ko.rnd(seq, D, scale=0.1, seed=D + 1)
    ids = torch.tensor([5, 0, 3, 5][:rows], dtype=torch.int32)
    want = table[ids.long()]
    if with_pos:
        want = want + pos[torch.arange(rows) % seq]                       # the bf16 add of the eager model
    g = G((rows, D))
    ext().gather_add(P(table), ids.to(DEV), P(pos) if with_pos else None, seq if with_pos else 0, g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    assert bits_equal(g.view, want)


@pytest.mark.parametrize("n", ko.COPY_BYTES)
def test_copy_and_zero_edges(n):
    src = torch.randint(1, 255, (n,), dtype=torch.uint8, generator=torch.Generator().manual_seed(n))
    around = torch.full((256 + n + 256,), 0xEE, dtype=torch.uint8, device=DEV)      # the source inside other bytes
    around[256:256 + n] = src.to(DEV)
    g = G((n,), torch.uint8)
    ext().dcopy(around[256:256 + n], g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    assert torch.equal(g.view.cpu(), src)
    ext().zero_(g.view)
    torch.cuda.synchronize()
    ko.check_guards(g)
    assert not g.view.any()


@pytest.mark.parametrize("n", ko.FINALIZE_N)
def test_finalize_latents_edges(n):
    """the float4 body and the scalar tail; a NaN at the last element, at element 0, nowhere"""
    x = ko.rnd(n, seed=n, dtype=torch.float32)
    for where, flag in ((n - 1, 0), (0, 0), (None, 1)):
        xi = x.clone()
        if where is not None:
            xi[where] = math.nan
        z, f = G((n,)), G((1,), torch.uint8)
        ext().finalize_latents(P(xi), z.view, f.view)
        torch.cuda.synchronize()
        ko.check_guards(z, f)
        assert int(f.view[0]) == flag, (n, where)
        fin = torch.isfinite(xi)
        assert bits_equal(z.view.cpu()[fin], xi.to(BF16)[fin]) and bool(torch.isnan(z.view.cpu()[~fin].float()).all())


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("pixels", [1, 64, 65])
def test_latent_init_edges(pixels, cfg):
    """one pixel, one 256-lane block of elements, one more; the padding channels of the UNet
    input keep their bits"""
    cin, cstride, nhist = 4, 8, 3
    x0 = ko.rnd(1, pixels, 1, cin, seed=pixels, dtype=torch.float32)
    x, xs = G(x0.shape, torch.float32), G(x0.shape, torch.float32)
    hist = G((nhist, *x0.shape), torch.float32)
    u = G((2 if cfg else 1, pixels, 1, cstride))
    ext().latent_init(P(x0), 0.5, x.view, xs.view, hist.view, u.view, int(cfg))
    torch.cuda.synchronize()
    ko.check_guards(x, xs, hist, u)
    assert bits_equal(x.view, x0) and not xs.view.any() and not hist.view.any()
    want = ko.guarded(u.view.shape).view
    want[..., :cin] = (x0 * 0.5).to(BF16)
    assert bits_equal(u.view, want)
