"""Instruments for localised kernel errors, shared by test_kernel_oracle.py (CPU: the instruments
themselves, proven on planted bugs) and test_kernel_edges_gpu.py (the HIP kernels).

A whole-tensor ``|out - ref| / |ref|`` under 1e-2 passes a kernel that drops the bias of one row,
leaves one padding key unmasked or normalises one row group with another's statistics.  Three
instruments close that:

* :func:`block_rel_err`: the worst relative error over output blocks (a ratio of block norms, the
  partial edge blocks included) against a reference computed in fp64 from the same bf16 inputs
  (``ops.reference`` with ``dtype=torch.float64``).  The bound of a family is the whole-tensor
  tolerance tests/test_kernels_gpu.py already uses for it (:data:`BOUND`).
* :func:`guarded` / :func:`check_guards`: an output buffer in the middle of one allocation whose
  two guard regions (at least 256 rows or 1 MiB each) hold a fixed bit pattern; a store past a
  partial tile changes them.  The view itself starts as that pattern too, a NaN in every float
  type, so an element the kernel never wrote shows in the block error.
* :func:`poisoned`: an input equal to ``t`` inside a larger NaN buffer, row-strided where the
  binding takes strides, else a row slice of a taller buffer.  A kernel that reads past a row, a
  key or a tensor and multiplies by zero gets NaN here, as it would next to another tensor.

Everything a wrong kernel could plausibly touch lies inside those single allocations: the tests
never hand a kernel a pointer whose tile-sized neighbourhood is unallocated.

The ideal kernel (fp64 math, rounded only where the kernels' own headers say they round: the bf16
output, the bf16 scaled Q and P of attention, the bf16 folded W*gamma of the LayerNorm fold, the
bf16 normalised A rows of the GroupNorm fold, e4m3 Q/K/V/P of the fp8 attention) must stay under
HALF the bound in every block of every case of :mod:`test_kernel_edges_gpu`; test_kernel_oracle.py
asserts that.  Its worst block, measured on the CPU over those cases (the table
test_kernel_oracle.py::test_floor_table prints with ``-s``):

    family                block                      bound    ideal kernel's worst block
    gemm / linear_cat     16 rows x 16 columns       1e-2     2.81e-3
    conv2d / conv2d_up2   16 pixels x 16 channels    1e-2     2.96e-3
    LayerNorm fold        16 rows x 16 columns       1.5e-2   3.98e-3
    GroupNorm fold        16 rows x 16 columns       1e-2     2.73e-3
    attention (bf16)      16 queries x d             2e-2     3.36e-3
    attention (fp8)       16 queries x d             0.12     5.28e-2
    decode attention      one query x d              2e-2     8.22e-3   (with a bf16 P, as the flash kernels)
    layer / rms / embed   one row                    1e-2     2.25e-3
    group_norm            16 pixels x one group      1e-2     3.05e-3
    rope_kv               one token x one head       1e-2     1.91e-3

Nothing here is calibrated against what the HIP kernels return.

Two things the kernels' own rules set.  Causal attention has no key that every query must
ignore (key q + 1 is masked for query q and valid for the queries after it), so the causal
future key carries a large finite V (FUTURE_V) instead of 3e38, which would overflow the rows
that may see it.  And the GEMM planner runs a forced tile only at shapes its family takes:
:func:`gemm_cases` and the A-in-registers cases say where that moves a K or an N.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from cassmantle_amd import ops
from cassmantle_amd.ops import reference as ref

F64 = torch.float64
BF16 = torch.bfloat16

# per-block bounds: the existing whole-tensor tolerances of tests/test_kernels_gpu.py
BOUND = {"gemm": 1e-2, "conv": 1e-2, "ln_fold": 1.5e-2, "gn_fold": 1e-2, "attention": 2e-2, "fp8": 0.12,
         "decode": 2e-2, "norm": 1e-2, "group_norm": 1e-2, "rope": 1e-2}
BLOCK_MN = (16, 16)


# ------------------------------------------------------------------------------ block error
def _block_sums(t: torch.Tensor, block) -> torch.Tensor:
    """sum of ``t`` over blocks of ``block[i]`` along every dim (None: the whole dim); a dim that
    its block does not divide ends in a partial block"""
    assert len(block) == t.dim(), (block, t.shape)
    for i, b in enumerate(block):
        n = t.shape[i]
        b = n if b is None else min(int(b), max(n, 1))
        nb = max(1, -(-n // b))
        if nb * b != n:
            pad = list(t.shape)
            pad[i] = nb * b - n
            t = torch.cat([t, t.new_zeros(pad)], dim=i)
        t = t.unflatten(i, (nb, b)).sum(i + 1)
    return t


def block_rel_err(out: torch.Tensor, ref64: torch.Tensor, block=BLOCK_MN) -> float:
    """max over blocks of ``|out - ref|_block / |ref|_block``.  inf where ``out`` is not finite
    (an unwritten guarded element, a poisoned read).  A block whose reference is all zero must
    be zero exactly."""
    assert tuple(out.shape) == tuple(ref64.shape), (out.shape, ref64.shape)
    o = out.detach().to("cpu", F64)
    r = ref64.detach().to("cpu", F64)
    if not bool(torch.isfinite(o).all()):
        return math.inf
    e2 = _block_sums((o - r) ** 2, block)
    r2 = _block_sums(r * r, block)
    ratio = torch.where(r2 > 0, e2 / r2.clamp_min(1e-300), torch.where(e2 > 0, torch.full_like(e2, math.inf), e2))
    return math.sqrt(ratio.max().item()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------ guards
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
PATTERN = {1: 0xA5, 2: 0x7FA5, 4: 0x7FA5A5A5, 8: 0x7FA5A5A5A5A5A5A5}     # a NaN in bf16 / fp16 / fp32 / fp64


def guard_elems(shape, dtype) -> int:
    """elements of one guard region: 256 rows of the last dim or 1 MiB, whichever is smaller,
    rounded up to 256 bytes (the view keeps the allocation's alignment)"""
    size = torch.empty((), dtype=dtype).element_size()
    row = int(shape[-1]) if len(shape) else 1
    nbytes = min(256 * row * size, 1 << 20)
    return (nbytes + 255) // 256 * 256 // size


class Guarded(NamedTuple):
    view: torch.Tensor      # contiguous, in the middle of ``buf``
    buf: torch.Tensor       # the flat allocation
    guard: int              # elements of each guard region
    pattern: int


def int_view(t: torch.Tensor) -> torch.Tensor:
    return t.view(_INT[t.element_size()])


def guarded(shape, dtype=BF16, guard: Optional[int] = None, fill: Optional[int] = None, device="cpu") -> Guarded:
    """one flat buffer filled with a fixed bit pattern and a contiguous ``shape`` view in its middle"""
    shape = tuple(int(s) for s in shape)
    n = math.prod(shape)
    g = guard_elems(shape, dtype) if guard is None else int(guard)
    size = torch.empty((), dtype=dtype).element_size()
    pat = PATTERN[size] if fill is None else int(fill)
    buf = torch.full((g + n + g,), pat, dtype=_INT[size], device=device).view(dtype)
    view = buf[g:g + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return Guarded(view, buf, g, pat)


def guards_intact(g: Guarded) -> bool:
    iv = int_view(g.buf)
    n = g.view.numel()
    return bool((iv[:g.guard] == g.pattern).all()) and bool((iv[g.guard + n:] == g.pattern).all())


def check_guards(*gs: Guarded) -> None:
    """both guard regions of every buffer are bit-identical to the pattern (integer compare)"""
    for g in gs:
        iv = int_view(g.buf)
        n = g.view.numel()
        for name, region, base in (("before", iv[:g.guard], -g.guard), ("after", iv[g.guard + n:], n)):
            bad = (region != g.pattern).nonzero().flatten()
            assert bad.numel() == 0, (f"{bad.numel()} elements written {name} a {tuple(g.view.shape)} output, "
                                      f"first at flat offset {base + int(bad[0])}")


# ------------------------------------------------------------------------------ poison
def poisoned(t: torch.Tensor, strided: bool = False, row_dims: int = 1, device=None) -> torch.Tensor:
    """a view equal to ``t`` inside a larger NaN buffer on ``device``.  ``strided``: the last
    ``row_dims`` dims form a row; rows sit 8 elements into wider NaN rows (row stride = row + 16)
    and up to 256 NaN rows precede and follow those of every outer index.  Otherwise the view
    is contiguous, a slice of a flat NaN buffer with a guard-sized margin on either side."""
    device = t.device if device is None else device
    assert t.is_floating_point()
    if not strided:
        g = guard_elems(t.shape, t.dtype)
        buf = torch.full((g + t.numel() + g,), math.nan, dtype=t.dtype, device=device)
        view = buf[g:g + t.numel()].view(t.shape)
    else:
        lead, rows, rshape = t.shape[:-(row_dims + 1)], t.shape[-(row_dims + 1)], t.shape[-row_dims:]
        W = math.prod(rshape)
        pad = max(1, min(256, (1 << 20) // ((W + 16) * t.element_size())))
        buf = torch.full((*lead, rows + 2 * pad, W + 16), math.nan, dtype=t.dtype, device=device)
        view = buf[..., pad:pad + rows, 8:8 + W].unflatten(-1, tuple(rshape))
        assert not view.is_contiguous() or view.numel() <= W
    view.copy_(t)
    assert view.shape == t.shape and view.stride(-1) == 1
    return view


# ------------------------------------------------------------------------------ data
def rnd(*shape, scale=1.0, seed=0, shift=0.0, dtype=BF16) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(BF16)


def e4m3(t: torch.Tensor) -> torch.Tensor:
    """fp64 -> OCP e4m3 (saturating at 448) -> fp64"""
    return t.clamp(-448.0, 448.0).to(torch.float32).to(torch.float8_e4m3fn).to(F64)


# ------------------------------------------------------------------------------ GEMM cases
class GemmCase(NamedTuple):
    cfg: int          # forced tile (-1: the planner's choice)
    split: int        # forced split-K (0: the planner's choice)
    M: int
    N: int            # outputs (W has 2N rows for geglu)
    K: int
    act: str

    @property
    def id(self):
        return f"cfg{self.cfg}-s{self.split}-{self.M}x{self.N}x{self.K}-{self.act}"


def gemm_cases(menu) -> list:
    """every live row of the tile menu ((id, family, BM, BN, waves, stages, producers, gated)):
    one full tile, one partial tile (M = BM + 1, N = BN + 8) and K = one k-tile plus an 8-wide
    tail (fewer k-tiles than any ring has stages) / five plus a tail / eight plus a tail split in
    two.  The planner (gemm.hip) gives the ping-pong and deep-ring tiles only whole 64-wide
    k-tiles and splits only where every slice keeps four k-tiles, so those families get K = 64 /
    320 / 512 and the split-K case of every family its eight k-tiles: at any other K a forced
    config would not run and the case would test the planner's fallback instead."""
    cases = []
    for cid, fam, BM, BN, _, _, _, gated in menu:
        if fam == "areg":
            continue
        k1, k5, k8 = (72, 328, 520) if fam == "static" else (64, 320, 512)
        for N in ((16, 12) if cid == 4 else (BN + 8,)):
            cases += [GemmCase(cid, 1, BM + 1, N, k1, "silu"), GemmCase(cid, 1, BM + 1, N, k5, "silu"),
                      GemmCase(cid, 2, BM + 1, N, k8, "silu")]
        if gated:
            cases += [GemmCase(cid, 1, BM + 1, BN // 2 + 8, K, "geglu") for K in (k1, k5)]
    cases.append(GemmCase(-1, 0, 129, 20, 72, "silu"))                    # N % 8 != 0, planner-chosen
    cases += [GemmCase(-1, 0, M, 264, 72, "silu") for M in (8, 9)]       # the GEMV boundary
    return cases


def gemm_inputs(c: GemmCase):
    """x, w, bias, residual (bf16, CPU)"""
    Nw = 2 * c.N if c.act == "geglu" else c.N
    s = 1000 + 7 * c.M + 3 * c.N + c.K
    return (rnd(c.M, c.K, seed=s), rnd(Nw, c.K, scale=c.K ** -0.5, seed=s + 1), rnd(Nw, scale=0.1, seed=s + 2),
            rnd(c.M, c.N, seed=s + 3))


def linear64(x, w, b=None, r=None, act=None):
    return ref.linear(x, w, b, residual=r, act=act, dtype=F64)


# (M, N, K) of the A-in-registers kernel (cfg 15).  It streams W in whole chunks of 64 rows
# (K = 320) / 32 rows (K = 640) (gemm_areg_ok), so N is two / three chunks; N = 72 takes the paths
# ln_linear / gn_linear fall back to there (row-statistics pass or GroupNorm kernel, then a GEMM)
AREG_CASES = [(M, 128 if K == 320 else 96, K) for M in (33, 257) for K in (320, 640)]
AREG_FALLBACK_N = 72
CAT_CASES = [(64, 64), (64, 128)]                                         # (Ca, Cb)
CAT_N = 72
ROW_STATS_CASE = (129, 136, 72)                                           # (M, N, K) producer; consumer N -> 72


def ln_fold_inputs(M, N, K, seed):
    """x, ln gamma, ln beta, w, bias"""
    return (rnd(M, K, scale=1.5, shift=0.3, seed=seed), rnd(K, scale=0.3, shift=1.0, seed=seed + 1),
            rnd(K, scale=0.2, seed=seed + 2), rnd(N, K, scale=K ** -0.5, seed=seed + 3), rnd(N, scale=0.1, seed=seed + 4))


def ln_linear64(x, g, be, w, b, eps=1e-5):
    return ref.linear(ref.layer_norm(x, g, be, eps, dtype=F64), w, b, dtype=F64)


def ideal_ln_fold(x, g, be, w, b, eps=1e-5):
    """the folded form in fp64 with the fold's own roundings (bf16 W*gamma and b + W.beta)"""
    wf, wsum, bf = ops.ln_fold(g, be, w, b)
    xd = x.to(F64)
    mean = xd.mean(-1, keepdim=True)
    rstd = (xd.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    y = rstd * (xd @ wf.to(F64).t() - mean * wf.to(F64).sum(1)) + bf.to(F64)
    return bf16_round(y)


def gn_linear64(x, g, be, groups, eps, w, b):
    return ref.linear(ref.group_norm(x, groups, g, be, eps, False, dtype=F64), w, b, dtype=F64)


# ------------------------------------------------------------------------------ conv cases
CONV_CASES = [(B, H, W, Cin, Cout, stride) for (B, H, W) in ((2, 5, 7), (1, 1, 1))
              for (Cin, Cout) in ((64, 72), (32, 64), (8, 3)) for stride in (1, 2)]
UP2_CASE = (2, 3, 5, 64, 72)
UP2_SPLIT_CIN = 128          # a forced split-K plan needs eight k-tiles (K = 4 Cin): four per slice


def conv_inputs(B, H, W, Cin, Cout, stride=1, up=False):
    """x, w, bias, chan_bias, residual"""
    s = 2000 + 31 * H + 5 * Cin + Cout + stride
    Ho, Wo = ((2 * H, 2 * W) if up else ((H - 1) // stride + 1, (W - 1) // stride + 1))
    return (rnd(B, H, W, Cin, seed=s), rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=s + 1),
            rnd(Cout, scale=0.1, seed=s + 2), rnd(B, Cout, scale=0.1, seed=s + 3), rnd(B, Ho, Wo, Cout, seed=s + 4))


def conv64(x, w, b, cb, res, stride=1, up=False):
    return ref.conv2d(x, w, b, stride, 1, res, up, cb, dtype=F64)


# ------------------------------------------------------------------------------ attention
ATTN_NQ = (1, 33, 257)
ATTN_NK = (1, 63, 64, 65, 129)
SENTINEL_V = 3e38            # V of a key no query may see
FUTURE_V = 64.0              # V of the causal future key (later queries do see it, so it stays finite)
LAST_V = 8.0                 # V of the dominant last valid key


class AttnCase(NamedTuple):
    B: int
    Nq: int
    Nk: int
    H: int
    Hk: int
    d: int
    lens: Optional[tuple]
    causal: bool

    @property
    def id(self):
        return f"q{self.Nq}-k{self.Nk}-h{self.H}/{self.Hk}-d{self.d}-{'causal' if self.causal else 'lens'}"


def attn_cases(d, H=2, Hk=None):
    Hk = H if Hk is None else Hk
    cs = [AttnCase(3, Nq, Nk, H, Hk, d, (Nk, 1, 0), False) for Nq in ATTN_NQ for Nk in ATTN_NK]
    return cs + [AttnCase(3, 65, 65, H, Hk, d, None, True)]


GQA_CASE = AttnCase(3, 65, 65, 4, 2, 64, None, True)
D512_SPLIT_CASE = AttnCase(3, 33, 300, 2, 2, 512, (300, 1, 0), False)     # 6 blocks, 300 keys: two key splits (d512_splits)


def attn_data(c: AttnCase):
    """q, k, v (bf16, CPU) in which the edges matter.  Per (batch, kv head) a direction u: a
    quarter of the queries are u plus noise, the last valid key is 4u with V = LAST_V (dominant
    for them: score 4 sqrt(d) against N(0, 1)), and the first key past ``lens[b]`` is 4u too with
    V = SENTINEL_V.  Causal (Nq == Nk): for q = 0, 4, 8, ... key q is 4 q and key q + 1 as well,
    with V = FUTURE_V, which queries > q legitimately see."""
    s = 3000 + 13 * c.Nq + 7 * c.Nk + c.d + c.H
    q, k, v = rnd(c.B, c.Nq, c.H, c.d, seed=s), rnd(c.B, c.Nk, c.Hk, c.d, seed=s + 1), rnd(c.B, c.Nk, c.Hk, c.d, seed=s + 2)
    g = c.H // c.Hk
    if c.causal:
        assert c.Nq == c.Nk
        for qi in range(0, c.Nq, 4):
            k[:, qi] = (4 * q[:, qi, ::g].float()).to(BF16)
            v[:, qi] = LAST_V
            if qi + 1 < c.Nk:
                k[:, qi + 1] = k[:, qi]
                v[:, qi + 1] = FUTURE_V
        return q, k, v
    u = rnd(c.B, c.Hk, c.d, seed=s + 3)
    noise = rnd(c.B, c.Nq, c.H, c.d, scale=0.25, seed=s + 4)
    hot = torch.arange(c.Nq) % 4 == 0
    q[:, hot] = (u.repeat_interleave(g, 1)[:, None].float() + noise[:, hot].float()).to(BF16)
    for b in range(c.B):
        n = c.lens[b] if c.lens else c.Nk
        if n > 0:
            k[b, n - 1] = (4 * u[b].float()).to(BF16)
            v[b, n - 1] = LAST_V
        if n < c.Nk:
            k[b, n] = (4 * u[b].float()).to(BF16)
            v[b, n:] = SENTINEL_V
    return q, k, v


def attention64(q, k, v, lens=None, causal=False, scale=None) -> torch.Tensor:
    """fp64 reference on K/V truncated per batch: masked values never enter a product"""
    out = torch.zeros(q.shape, dtype=F64)
    for b in range(q.shape[0]):
        n = k.shape[1] if lens is None else int(lens[b])
        if n > 0:
            out[b] = ref.attention(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], scale, causal, dtype=F64)[0]
    return out


def ideal_attention(q, k, v, lens=None, causal=False, scale=None, fp8=False, drop_last=False, extra_key=False):
    """flash attention in fp64 with the kernels' roundings: Q * scale * log2(e) and the
    unnormalised P = 2^(S - max) in bf16 (e4m3 for fp8, as K and V).  The planted bugs:
    ``drop_last`` masks the last valid key, ``extra_key`` lets the first masked one in."""
    B, Nq, H, d = q.shape
    g = H // k.shape[2]
    scale = d ** -0.5 if scale is None else scale
    rq = e4m3 if fp8 else (lambda t: bf16_round(t).to(F64))
    out = torch.zeros(q.shape, dtype=F64)
    for b in range(B):
        n = k.shape[1] if lens is None else int(lens[b])
        n = n - 1 if drop_last else min(n + 1, k.shape[1]) if extra_key else n
        if n <= 0:
            continue
        qs = rq(q[b].to(F64) * (scale * math.log2(math.e))).permute(1, 0, 2)            # [H, Nq, d]
        kb = k[b, :n].to(F64).repeat_interleave(g, 1).permute(1, 0, 2)
        vb = v[b, :n].to(F64).repeat_interleave(g, 1).permute(1, 0, 2)
        if fp8:
            kb, vb = e4m3(kb), e4m3(vb)
        s = qs @ kb.transpose(1, 2)
        if causal:
            lim = torch.arange(Nq)[:, None] + (1 if extra_key else 0) - (1 if drop_last else 0)
            s = s.masked_fill(torch.arange(n)[None, :] > lim, -math.inf)
        m = s.max(-1, keepdim=True).values
        p = rq(torch.exp2(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))))
        l = p.sum(-1, keepdim=True)
        o = torch.where(l > 0, (p @ vb) / l.clamp_min(1e-300), torch.zeros_like(l))
        out[b] = o.permute(1, 0, 2)
    return bf16_round(out)


DECODE_L = (1, 127, 128, 129)
DECODE_GROUPS = (1, 2, 4)


def decode_data(L, group, d=64, Hk=2):
    """q [3, H, d], caches [3, L, Hk, d], lens = [L, 1, mid]: the last valid key dominant, the
    first one past ``lens`` dominant with V = SENTINEL_V"""
    B, H = 3, Hk * group
    s = 4000 + 3 * L + group
    lens = [L, 1, max(1, L // 2)]
    q, kc, vc = rnd(B, H, d, seed=s), rnd(B, L, Hk, d, seed=s + 1), rnd(B, L, Hk, d, seed=s + 2)
    u = rnd(B, Hk, d, seed=s + 3)
    q[:, ::2] = (u.repeat_interleave(group, 1)[:, ::2].float() + 0.25 * q[:, ::2].float()).to(BF16)
    for b, n in enumerate(lens):
        kc[b, n - 1] = (4 * u[b].float()).to(BF16)
        vc[b, n - 1] = LAST_V
        if n < L:
            kc[b, n] = kc[b, n - 1]
            vc[b, n:] = SENTINEL_V
    return q, kc, vc, lens


def decode64(q, kc, vc, lens):
    return attention64(q[:, None], kc, vc, lens)[:, 0]


# ------------------------------------------------------------------------------ norms, rope
GN_CASES = [(2, 17, 64, 8), (1, 1, 320, 32)]                               # (B, S, C, G)
ROW_NORM_CASES = [(rows, D) for rows in (1, 5) for D in (8, 136, 4096)]


def norm_inputs(rows, D):
    s = 5000 + rows + D
    return rnd(rows, D, scale=2.0, shift=1.0, seed=s), rnd(D, scale=0.5, shift=1.0, seed=s + 1), rnd(D, scale=0.1, seed=s + 2)


def gn_inputs(B, S, C):
    s = 6000 + S + C
    return rnd(B, S, C, shift=0.5, seed=s), rnd(C, scale=0.5, shift=1.0, seed=s + 1), rnd(C, scale=0.1, seed=s + 2)


def embed_inputs(rows, D, vocab=50):
    s = 7000 + rows + D
    ids = torch.randint(0, vocab, (1, rows), generator=torch.Generator().manual_seed(s))
    return rnd(vocab, D, seed=s + 1), ids, rnd(rows + 3, D, scale=0.1, seed=s + 2), rnd(D, scale=0.1, seed=s + 3)


def embed_ln64(word, ids, pos, add, g, b, eps=1e-5):
    x = word.to(F64)[ids] + pos.to(F64)[: ids.shape[1]][None] + add.to(F64)
    return ref.layer_norm(x, g, b, eps, dtype=F64)


ROPE_CASES = [(2, 5, 4, 2, 64, 16, (3, 11)), (1, 1, 4, 4, 128, 8, (7,)), (3, 4, 2, 1, 64, 12, (0, 8, 5))]   # B, T, H, Hk, d, L, pos0


def rope64(qkv, pos0, H, Hk, d, theta=10000.0):
    """rotated q [B, T, H, d], rotated k and plain v [B, T, Hk, d] in fp64"""
    B, T, _ = qkv.shape
    x = qkv.view(B, T, H + 2 * Hk, d)
    pos = torch.tensor(pos0)[:, None] + torch.arange(T)[None, :]
    return (ref.rope(x[:, :, :H], pos, theta, dtype=F64), ref.rope(x[:, :, H:H + Hk], pos, theta, dtype=F64),
            x[:, :, H + Hk:].to(F64))
