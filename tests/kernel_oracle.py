"""Instruments for localised kernel errors, shared by test_kernel_oracle.py (CPU: the instruments
themselves, proven on planted bugs; test_kv8_oracle.py: the fp8 K/V image model) and
test_kernel_edges_gpu.py, test_kernel_edges_conv_gpu.py, test_kernel_edges_decode_gpu.py,
test_kernel_edges_scorer_gpu.py, test_kernel_edges_kv8_gpu.py and test_kernel_edges_norm_gpu.py
(the HIP kernels).

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
HALF the bound in every block of every case of the four GPU files; test_kernel_oracle.py
asserts that.  Its worst block, measured on the CPU over those cases (the table
test_kernel_oracle.py::test_floor_table prints with ``-s``):

    family                block                      bound    ideal kernel's worst block
    gemm / linear_cat     16 rows x 16 columns       1e-2     2.81e-3
    conv2d / conv2d_up2   16 pixels x 16 channels    1e-2     2.96e-3   (the tile-by-tile cases: 2.13e-3)
    LayerNorm fold        16 rows x 16 columns       1.5e-2   3.98e-3
    GroupNorm fold        16 rows x 16 columns       1e-2     2.73e-3
    attention (bf16)      16 queries x d             2e-2     3.36e-3
    attention, dispatch   16 queries x d             2e-2     5.99e-3   (every instantiation, below; the worst: d = 128, GQA)
    attention (fp8)       16 queries x d             0.12     5.28e-2
    decode attention      one query x d              2e-2     8.22e-3   (with a bf16 P, as the flash kernels)
    layer / rms / embed   one row                    1e-2     3.31e-3   (every VPL and T, each row its own mean and scale)
    group_norm            16 pixels x one group      1e-2     3.05e-3   (the two iid cases)
    group_norm, geometry  16 pixels x one group      1e-2     2.96e-3   (GN_GEOM_CASES, each (image, group) its own moments)
    row_stats             one row: mean / rstd       8e-7     1.26e-7 / 1.65e-7   (the fp32 formula; the bound is 4 x 2e-7)
    channel_stats         one (image, channel)       derived  0.944 of it   (the kernel's own fp32 chain; channel_stats_bound)
    rope_kv               one token x one head       1e-2     1.91e-3
    GEMV (lm.hip)         one row x 4 columns (2)    1e-2     3.83e-3   (2: the gated 8-row template)
    GEMV + RMSNorm        one row x 4 columns (2)    1e-2     3.27e-3
    GEMV, batched         one row x 4 columns        1e-2     3.81e-3
    M = 8 | 9 linear      one row x 4 columns        1e-2     3.06e-3
    M = 8 | 9 ln_linear   one row                    1.5e-2   2.80e-3   (4 columns: 8.1e-3 at M = 8, so the row)
    decode, d = 128 / L > 4096   one query x d       2e-2     8.93e-3   (with a bf16 P)
    mean_pool_l2          one row                    1e-5     1.39e-7   (the fp32 evaluation; fp32 output)
    fp8 K/V image (kv8)   16 keys x d of one head    6e-2     2.88e-2   (the one-rounding writer only, see below)

The e4m3 K/V image of the fp8 attention kernel has a byte-exact CPU model (:func:`kv8_image_model`):
the pack and the LDS-staged GEMM epilogue convert bf16 values and must equal it byte for byte
(test_kernel_edges_kv8_gpu.py).  Only the A-in-registers epilogue, which rounds its fp32
accumulators to e4m3 once, is held to a bound, the ``kv8`` row: twice the worst block of e4m3(y64).

The GEMV keeps the kernel's own block, one row x the columns of one thread block: the bf16 store
alone stays under half of 1e-2 there.  The four cosine kernels are held to an absolute 1e-5
against fp64 (COS_ATOL) for fp32 and bf16 tables alike; the same formula in fp32 is within 2.4e-7
on every case.  The sampler, cosine_topk's order and the byte-moving glue kernels are exact.

Nothing here is calibrated against what the HIP kernels return.

norm.hip is held by its launch geometry.  The GroupNorm launchers pick vectors per thread, lanes,
chunks, rows per block and rows in flight from (B, S, C); ``ext().group_norm_geometry`` reports
the choice, :func:`gn_geometry_model` is its transcript, and every row of GN_GEOM_CASES names the
branches (GN_BRANCHES) it exists for; the GPU file asserts both from the binding, so a retuned
constant fails a case by name.  Their data (:func:`gn_moments`) gives every (image, group) a mean
and a deviation of its own and every LayerNorm row its own mean and scale (:func:`own_rows`): with
iid data the neighbouring group's statistics, or image 0's for every image, stay under the
whole-tensor 1e-2 (7.9e-3 and 5.6e-3 at 2 x 4096 x 320 / 32), with these they are 27 and 16 in the
worst block.  channel_stats_kernel is checked per (image, channel) against exact sums under the
worst-case error of its own summation chain, row_stats per row under four times the error of the
same formula in fp32.

Which kernel a case runs is asserted, not assumed: the GEMM cases force a tile and read
``gemm_last_plan()``, the attention cases name the instantiation launch_attention must pick
under default knobs and read ``attention_last_kernel()`` (ATTN_ROUNDUP_D, PREFILL_CASE,
ATTN_WIDE_CASES).  The raster cases (RASTER_GROUPS) walk an 18-tile grid under every group size:
a tile the mapping misses stays NaN in the guarded output.

Two things the kernels' own rules set.  Causal attention has no key that every query must
ignore (key q + 1 is masked for query q and valid for the queries after it), so the causal
future key carries a large finite V (FUTURE_V) instead of 3e38, which would overflow the rows
that may see it.  And the GEMM planner runs a forced tile only at shapes its family takes:
:func:`gemm_cases`, :func:`conv_tile_cases` and the A-in-registers cases say where that moves a
K or an N.
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


# ---- the tile raster (gemm_impl.h tile_of after common.h xcd_remap; gemm_set_raster).  G: M tiles
# per raster group; 0 is the compiled default (4), 1 the plain row-major walk, 8 more than nM.
# nM = 6 gives G = 4 and 5 a partial last group (nM > G, nM % G != 0), G = 3 two whole groups
RASTER_GROUPS = (0, 1, 3, 4, 5, 8)
RASTER_TILES = (6, 3)        # nM x nN = 18 tiles: no multiple of the 8 XCDs (xcd_remap's tail) nor of any G > 1
RASTER_CONV = (1, 23, 28, 64, 264, 1)      # B, H, W, Cin, Cout, stride at tile 0: M = 644 = 5 * 128 + 4, N = 2 * 128 + 8


def raster_gemm_cases(menu) -> list:
    """one live row of each family, one with producer waves, and the gated instantiation of one
    static and one ping-pong row (the first of each in the menu), at M = 5 BM + 1 and N = 2 BN + 8
    (a gated block covers BN / 2 outputs: N = BN + 8) with K = one k-tile (gemm_cases' rule)"""
    def first(pred):
        return next(r for r in menu if pred(r))
    rows = [(first(lambda r, f=f: r[1] == f), False) for f in ("static", "pingpong", "deep")]
    rows.append((first(lambda r: r[1] != "areg" and r[6] > 0), False))
    rows += [(first(lambda r, f=f: r[1] == f and r[7]), True) for f in ("static", "pingpong")]
    cases = []
    for (cid, fam, BM, BN, *_), gated in rows:
        assert BN > 16
        cases.append(GemmCase(cid, 1, 5 * BM + 1, BN + 8 if gated else 2 * BN + 8, 72 if fam == "static" else 64,
                              "geglu" if gated else "silu"))
    return cases


def raster_tiles(c: GemmCase, menu) -> tuple:
    """(nM, nN) of a forced case"""
    _, _, BM, BN, *_ = next(r for r in menu if r[0] == c.cfg)
    return -(-c.M // BM), -(-c.N // (BN // 2 if c.act == "geglu" else BN))


def tile_of_model(lin, nM, nN, G):
    """gemm_impl.h tile_of for G >= 1 on the CPU: (tm, tn) of linear index ``lin``"""
    G = min(G, nM)
    if G <= 1:
        return lin // nN, lin % nN
    grp = lin // (G * nN)
    gs = min(G, nM - grp * G)
    r = lin - grp * G * nN
    return grp * G + r % gs, r // gs


def xcd_remap_model(bid, n):
    """common.h xcd_remap: block ``bid`` of ``n`` round-robin over 8 XCDs -> a contiguous range per XCD"""
    q, r = divmod(n, 8)
    xcd, idx = bid % 8, bid // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


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


def conv_inputs(B, H, W, Cin, Cout, stride=1, up=False, ksize=3):
    """x, w, bias, chan_bias, residual (``ksize`` 3: padding 1; 1: padding 0)"""
    s = 2000 + 31 * H + 5 * Cin + Cout + stride + (0 if ksize == 3 else 977 * ksize)
    Ho, Wo = ((2 * H, 2 * W) if up else ((H - 1) // stride + 1, (W - 1) // stride + 1))
    return (rnd(B, H, W, Cin, seed=s), rnd(Cout, ksize, ksize, Cin, scale=(ksize * ksize * Cin) ** -0.5, seed=s + 1),
            rnd(Cout, scale=0.1, seed=s + 2), rnd(B, Cout, scale=0.1, seed=s + 3), rnd(B, Ho, Wo, Cout, seed=s + 4))


def conv64(x, w, b, cb, res, stride=1, up=False, padding=1):
    return ref.conv2d(x, w, b, stride, padding, res, up, cb, dtype=F64)


# ---- the implicit-GEMM conv tile by tile (test_kernel_edges_conv_gpu.py)
BK = 64                      # k-tile of every MFMA GEMM / conv kernel
# (B, H, W, stride) of the input: the smallest that give a BM = 256 tile one full M tile and a
# partial one, an image boundary inside a tile (135 / 150 output pixels per image) and a W that is
# no multiple of 16.  s2: Ho x Wo = 10 x 15, the bottom edge padded (odd H), the right one not
# (even W).  up: the low-res input of an 18 x 30 output.
CONV_GEOM = {"s1": (2, 9, 15, 1), "s2": (2, 19, 30, 2), "up": (2, 9, 15, 1)}
CONV_KINDS = ("s1", "s2", "up2")      # what a tuning-table entry can be: stride 1, stride 2, parity classes


class ConvCase(NamedTuple):
    group: str        # "plain" (ops.conv2d, 3x3) | "up2" (the parity classes) | "modes" (static tiles only)
    cfg: int          # forced tile
    split: int        # forced split-K
    geom: str         # key of CONV_GEOM
    Cin: int
    Cout: int
    stats: bool       # epilogue statistics (a split case: splitk_reduce_stats_kernel, else splitk_reduce_kernel)
    op: str = "conv"  # "conv" | "up2" (conv2d_up2) | "fused_up" (conv2d(upsample=True)) | "1x1" (pad 0)

    @property
    def kind(self):
        return "up2" if self.op == "up2" else self.geom

    @property
    def ksize(self):
        return 1 if self.op == "1x1" else 3

    @property
    def K(self):
        """the GEMM's K: taps x Cin (four taps per parity class)"""
        return (4 if self.op == "up2" else self.ksize ** 2) * self.Cin

    @property
    def nk(self):
        return -(-self.K // BK)

    @property
    def id(self):
        return f"cfg{self.cfg}-s{self.split}-{self.op}-{self.geom}-{self.Cin}to{self.Cout}-{'stats' if self.stats else 'nostats'}"


def split_slices(nk, split) -> list:
    """k-tiles of every split-K slice as the kernels cut them: ``per = ceil(nk / split)`` each,
    the last ones shorter or empty"""
    per = -(-nk // split)
    return [max(0, min(nk, (s + 1) * per) - s * per) for s in range(split)]


def conv_tile_cases(menu) -> list:
    """every live non-areg row of the tile menu on the conv A loader.  Cout = BN + 8 (one full, one
    partial N tile; the N <= 16 tile: 16).  Per tile, Cin % 64 == 0: stride 1 and 2 at nk = 9; a
    split in four of nk = 18 (slices of 5, 5, 5, 3: the last shorter than the 4- and 5-stage
    rings, each starting in the middle of the taps); a split in seven of nk = 36 (six slices of
    six, the seventh empty: its slab must be zeros); conv2d_up2 at nk = 4 and nk = 20 split in
    three (7, 7, 6).  Split cases run with and without statistics: the two reduce kernels.  All
    satisfy the planner's rules for a forced plan (family_runs: Cin % 64, N > 16, N % 8, ldcb % 4;
    nk / split >= 4), so none tests its fallback.  The static tiles have the other A modes as
    well: Cin = 32 / 24 (gemm_c1: tap boundaries inside a k-tile), the fused 2x upsample at
    Cin = 64 (gemm_c3) / 32 (gemm_c1), a 1x1 pad-0 conv, and N % 8 != 0 through the plain reduce."""
    cases = []
    for cid, fam, BM, BN, *_ in menu:
        if fam == "areg":
            continue
        N = 16 if BN <= 16 else BN + 8
        cases += [ConvCase("plain", cid, 1, g, 64, N, True) for g in ("s1", "s2")]
        cases += [ConvCase("plain", cid, s, "s1", cin, N, st) for s, cin in ((4, 128), (7, 256)) for st in (True, False)]
        cases.append(ConvCase("up2", cid, 1, "up", 64, N, True, "up2"))
        cases += [ConvCase("up2", cid, 3, "up", 320, N, st, "up2") for st in (True, False)]
        if fam == "static":
            cases += [ConvCase("modes", cid, 1, g, cin, N, True) for cin in (32, 24) for g in ("s1", "s2")]
            cases += [ConvCase("modes", cid, 1, "up", cin, N, True, "fused_up") for cin in (64, 32)]
            cases.append(ConvCase("modes", cid, 1, "s1", 64, N, True, "1x1"))
            if cid == 3:
                cases.append(ConvCase("modes", cid, 4, "s1", 128, BN + 4, False))
    return cases


_CONV_REF = {}


def conv_case_data(c: ConvCase):
    """(x, w, bias, chan_bias, residual), fp64 reference [B, Ho, Wo, Cout]; computed once per
    geometry and channel counts and shared by every tile (do not modify)"""
    B, H, W, stride = CONV_GEOM[c.geom]
    up = c.op in ("up2", "fused_up")
    key = (c.geom, c.Cin, c.Cout, up, c.ksize)
    if key not in _CONV_REF:
        args = conv_inputs(B, H, W, c.Cin, c.Cout, stride, up, c.ksize)
        _CONV_REF[key] = (args, conv64(*args, stride=stride, up=up, padding=c.ksize // 2))
    return _CONV_REF[key]


def chan_bias_slice(cb: torch.Tensor, device=None) -> torch.Tensor:
    """``cb`` [B, N] as a column slice of a wider NaN buffer whose row stride is a multiple of 8
    and greater than N (ldcb != N: the batched time-embedding projection hands every ResNet its
    columns of one wide output)"""
    B, N = cb.shape
    ld = (N + 7) // 8 * 8 + 16
    buf = torch.full((B + 2, ld), math.nan, dtype=cb.dtype, device=cb.device if device is None else device)
    view = buf[1:B + 1, 8:8 + N]
    view.copy_(cb)
    assert view.stride(0) > N and view.stride(0) % 8 == 0 and view.stride(1) == 1
    return view


def conv_im2col(x, ksize=3, stride=1, wrap_left=False, one_image=False) -> torch.Tensor:
    """A [B * Ho * Wo, ksize^2 * Cin] of the implicit GEMM in fp64 (k = tap * Cin + channel,
    padding ksize // 2).  The planted bugs of a linear tap offset without its mask:
    ``wrap_left`` reads the left padding tap one pixel below the row's first, the previous row's
    last pixel; ``one_image`` bounds the rows by the whole batch, so a tap above an image's first
    row (below its last) reads the neighbouring image."""
    B, H, W, Cin = x.shape
    pad = ksize // 2
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    xf = torch.cat([x.to(F64).reshape(B * H * W, Cin), torch.zeros(1, Cin, dtype=F64)])      # last row: the zero page
    b, oy, ox = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    cols = []
    for ky in range(ksize):
        for kx in range(ksize):
            iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
            flat = (b * H + iy) * W + ix
            ok_y = ((b * H + iy >= 0) & (b * H + iy < B * H)) if one_image else ((iy >= 0) & (iy < H))
            ok_x = (ix >= 0) & (ix < W)
            if wrap_left:
                ok_x = ok_x | ((ix == -1) & (flat >= 0))
            cols.append(xf[torch.where(ok_y & ok_x, flat, torch.full_like(flat, B * H * W)).reshape(-1)])
    return torch.cat(cols, dim=1)


def conv_model(x, w, b, cb, res, stride=1, split=1, drop_slice=None, **bugs) -> torch.Tensor:
    """the implicit GEMM in fp64, k-tile slices summed as the split-K reduce does, epilogue, bf16
    store; [B, Ho, Wo, Cout].  ``drop_slice``: the planted reduce that leaves that slice out."""
    Cout, ksize = w.shape[0], w.shape[1]
    A = conv_im2col(x, ksize, stride, **bugs)
    Wm = w.to(F64).reshape(Cout, -1)
    y, kt = torch.zeros(A.shape[0], Cout, dtype=F64), 0
    for s, n in enumerate(split_slices(-(-A.shape[1] // BK), split)):
        if s != drop_slice:
            y += A[:, kt * BK:(kt + n) * BK] @ Wm[:, kt * BK:(kt + n) * BK].t()
        kt += n
    y = y.view(res.shape) + b.to(F64) + cb.to(F64)[:, None, None, :] + res.to(F64)
    return bf16_round(y)


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

# ---- every instantiation launch_attention can pick (attention.hip), by what attention_last_kernel()
# reports: (family, DQK, DO, waves per block).  A head dim below each template width (the round-up
# branch, d < DQK) and the two exact widths without an edge test of their own
ATTN_ROUNDUP_D = (24, 48, 88, 96, 112, 128, 136)
ATTN_TEMPLATE_WIDTHS = (32, 64, 96, 128, 160)
LM_HEADS = (8, 2)            # (H, Hk) of the GQA cases at the LM's head dim 128
# LM prefill: causal over five key tiles in 4-wave blocks, GQA, K/V a strided (KV-cache) view
PREFILL_CASE = AttnCase(3, 257, 257, 8, 2, 128, None, True)
PREFILL_KERNEL = ("fwd", 128, 128, 4)


def attn_template_width(d) -> int:
    """the template a head dim that has no kernel of its own rounds up to"""
    return next(w for w in ATTN_TEMPLATE_WIDTHS if d <= w)


def cyc(B, Nk) -> tuple:
    """kv_lens (Nk, 1, 0) taking turns; B = 3n keeps the last batch without a key"""
    return tuple((Nk, 1, 0)[b % 3] for b in range(B))


# The smallest grids that cross the wave-count thresholds under default knobs: 1024 blocks of 256
# queries (8 waves, DO <= 96), 256 such blocks for the 16x16 d = 40 kernel, 512 blocks of 128 queries
# (4 waves at Nq < 256).  Nq = 257: the second 8-wave block has seven idle waves that still take
# every barrier and staging load.  (case, the kernel it must launch, the kernel under the d = 40
# variant "32x32" where that differs)
ATTN_WIDE_CASES = [
    (AttnCase(33, 257, 129, 16, 16, 32, cyc(33, 129), False), ("fwd", 32, 32, 8), None),
    (AttnCase(33, 257, 257, 16, 4, 64, None, True), ("fwd", 64, 64, 8), None),              # GQA, causal
    (AttnCase(33, 257, 129, 16, 16, 80, cyc(33, 129), False), ("fwd", 80, 96, 8), None),    # the ones column
    (AttnCase(33, 257, 257, 16, 16, 96, None, True), ("fwd", 96, 96, 8), None),
    (AttnCase(33, 257, 257, 16, 16, 40, None, True), ("fwd", 48, 64, 8), None),             # the MF path
    (AttnCase(3, 257, 257, 2, 2, 40, None, True), ("fwd", 48, 64, 4), None),
    (AttnCase(33, 257, 129, 4, 4, 40, cyc(33, 129), False), ("a16", 48, 48, 8), ("fwd", 48, 64, 4)),
    (AttnCase(66, 33, 65, 8, 8, 64, cyc(66, 65), False), ("fwd", 64, 64, 4), None),         # blocks4 >= 512: three idle waves
]
ATTN_KNOBS = ("CASSMANTLE_ATTN_NW", "CASSMANTLE_ATTN_NW4_MIN", "CASSMANTLE_ATTN16", "CASSMANTLE_ATTN16_NW8_MIN")

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


def ideal_attention(q, k, v, lens=None, causal=False, scale=None, fp8=False, drop_last=False, extra_key=False,
                    kv8=None):
    """flash attention in fp64 with the kernels' roundings: Q * scale * log2(e) and the
    unnormalised P = 2^(S - max) in bf16 (e4m3 for fp8, as K and V).  The planted bugs:
    ``drop_last`` masks the last valid key, ``extra_key`` lets the first masked one in.
    ``kv8`` (with fp8): a K/V image (:func:`kv8_image_model`) whose decoded bytes stand in for
    e4m3(k) and e4m3(v), as the fp8 kernel reads them; k and v then give the shapes only."""
    B, Nq, H, d = q.shape
    if kv8 is not None:
        assert fp8
        k, v = (t[:, :k.shape[1]] for t in kv8_unpack(kv8, B, k.shape[1], k.shape[2]))
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


# ------------------------------------------------------------------------------ the fp8 K/V image
# K8 [B][Hk][Nkp][64] then V8t [B][Hk][64][Nkp] (Nkp: keys rounded up to 64), OCP e4m3 bytes, every
# key at or past min(Nk, lens[b]) zero, every 64-key block of a V8t row in slot order (attention.hip's
# header comment).  Two writers: attn_fp8_pack_kernel and the GEMM epilogues (GemmArgs::kv8).
BOUND["kv8"] = 6e-2          # decoded image against fp64 K/V per 16 keys x 64 d of one head: twice the worst block of
#                              e4m3(y64) on the KV8_AREG_C cases (2.88e-2, test_kernel_oracle.py::test_ideal_kv8_writer)
KV8_BLOCK = (1, 16, 1, None)
CANARY = PATTERN[1]          # the byte of a guarded uint8 buffer: -0.203 in e4m3, small and finite
KV8_PACK_CASES = ([(3, Nk, 2, lens) for Nk in ATTN_NK for lens in ((Nk, 1, 0), None)] +      # (B, Nk, Hk, lens)
                  [(3, 65, Hk, (65, 1, 0)) for Hk in (1, 3)])
# (images, tokens per image) of the QKV GEMM at C = 192: Hk = 3, N = 576, K = 192, K columns from
# 192, V columns from 384.  M = 192: one full BM = 128 tile and a partial one of exactly one key
# block, three images in a BM = 256 tile; M = 384: an image boundary inside a tile of either BM.
# BN = 256, 160 and 80 straddle Q|K and K|V and end in a partial tile, 128 straddles Q|K, 64 is aligned
KV8_EPI_GEOMS = ((3, 64), (2, 192))
KV8_EPI_C = 192
KV8_SPLIT_K = 512            # a forced (cfg, 2) needs eight k-tiles to be a plan (gemm_cases); kv8 then runs it unsplit
KV8_AREG_C = (320, 640)      # the A-in-registers writer, geometry KV8_EPI_GEOMS[0]


def kv8_key(slot):
    """key offset (0..63) that slot 32h + j of a 64-key block holds:
    kappa(h, j) = 32(j>>4) + (j&3) + 8((j&15)>>2) + 4h"""
    h, j = slot >> 5, slot & 31
    return 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * h


def kv8_slot(kk):
    """slot of key offset kk (0..63), kappa inverted bit by bit: kk>>5 is j>>4, kk&3 is j&3,
    (kk>>3)&3 is (j&15)>>2 and (kk>>2)&1 is h"""
    return 32 * ((kk >> 2) & 1) + 16 * (kk >> 5) + 4 * ((kk >> 3) & 3) + (kk & 3)


def kv8_key_halves_swapped(slot):
    """planted: kappa with the lane-half bit h and the key-half bit j>>4 exchanged"""
    h, j = slot >> 5, slot & 31
    return 32 * h + (j & 3) + 8 * ((j & 15) >> 2) + 4 * (j >> 4)


def kv8_image_model(k, v, lens=None, key_of_slot=kv8_key, zero_past_lens=True) -> torch.Tensor:
    """the flat uint8 image of bf16 k, v [B, Nk, Hk, 64] on the CPU: ref.e4m3_encode of every
    valid key (fp32, saturating at +-448, round to nearest even, subnormals included), 0x00 for
    every key from min(Nk, lens[b]) to Nkp.  test_kernel_edges_kv8_gpu.py holds the emitters to
    that rule over all of bf16.  On an MI355X v_cvt_pk_fp8_f32 agrees with the CPU cast on every
    finite bf16 value up to 464 in magnitude (subnormals, ties, both zeros; 450 .. 464 round down
    to 448), and returns the NaN code 0x7F / 0xFF from 466 on: it does not saturate, so the
    emitters clamp to +-448 first (f8x4_sat in common.h).  The planted bugs: ``key_of_slot``
    (another order of a block's keys), ``zero_past_lens=False`` (keys past lens converted like
    the others)."""
    B, Nk, Hk, d = k.shape
    assert d == 64 and v.shape == k.shape
    Nkp = (Nk + 63) // 64 * 64
    kz, vz = torch.zeros(2, B, Nkp, Hk, 64, dtype=torch.uint8)
    for b in range(B):
        n = Nk if lens is None or not zero_past_lens else min(Nk, int(lens[b]))
        kz[b, :n], vz[b, :n] = ref.e4m3_encode(k[b, :n].cpu()), ref.e4m3_encode(v[b, :n].cpu())
    idx = torch.arange(Nkp)
    src = (idx & ~63) + key_of_slot(idx & 63)
    return torch.cat([kz.permute(0, 2, 1, 3).flatten(), vz[:, src].permute(0, 2, 3, 1).flatten()])


def kv8_views(image, B, Nk, Hk):
    """K8 [B, Hk, Nkp, 64] and V8t [B, Hk, 64, Nkp] of a flat image (views)"""
    Nkp = (Nk + 63) // 64 * 64
    half = B * Hk * Nkp * 64
    assert image.numel() == 2 * half
    return image[:half].view(B, Hk, Nkp, 64), image[half:].view(B, Hk, 64, Nkp)


def kv8_unpack(image, B, Nk, Hk):
    """fp64 K and V [B, Nkp, Hk, 64] of an image, the keys back in their natural order"""
    K8, V8t = kv8_views(image.cpu(), B, Nk, Hk)
    idx = torch.arange(K8.shape[2])
    dst = (idx & ~63) + kv8_slot(idx & 63)
    return (ref.e4m3_decode(K8, F64).permute(0, 2, 1, 3).contiguous(),
            ref.e4m3_decode(V8t, F64)[..., dst].permute(0, 3, 1, 2).contiguous())


def kv8_stale_run(image, B, Nk, Hk, b=0, h=0, d=5, run=1) -> torch.Tensor:
    """planted: a copy of the image in which one 16-slot run of one V8t row was never written"""
    bug = image.clone()
    kv8_views(bug, B, Nk, Hk)[1][b, h, d, 16 * run:16 * run + 16] = CANARY
    return bug


def kv8_neighbour_head(image, B, Nk, Hk, h=1) -> torch.Tensor:
    """planted: the V bytes of head h (the last 64 columns of a column tile) taken from head h - 1"""
    bug = image.clone()
    V8t = kv8_views(bug, B, Nk, Hk)[1]
    V8t[:, h] = V8t[:, h - 1].clone()
    return bug


def kv8_codes_apart(a, b) -> int:
    """the largest distance of two images' bytes in e4m3 codes: sign-magnitude order, both zeros equal"""
    def ordinal(t):
        i = t.cpu().to(torch.int64)
        return torch.where(i >= 128, -(i & 127), i)
    return int((ordinal(a) - ordinal(b)).abs().max())


def kv8_epi_inputs(geom, C=KV8_EPI_C, K=None):
    """x [B * ntok, K], ln gamma, ln beta, w [3C, K], bias of the QKV projection"""
    B, ntok = geom
    K = C if K is None else K
    return ln_fold_inputs(B * ntok, 3 * C, K, seed=500 + B * ntok + C + K)


def qkv_split(y, geom, C):
    """[M, 3C] -> Q [M, C], K and V [B, ntok, C // 64, 64]"""
    B, ntok = geom
    return y[:, :C], y[:, C:2 * C].reshape(B, ntok, C // 64, 64), y[:, 2 * C:].reshape(B, ntok, C // 64, 64)


DECODE_L = (1, 127, 128, 129)
DECODE_GROUPS = (1, 2, 4)


def decode_key_gain(d) -> float:
    """the dominant key is this times its query's direction: 4 at d = 64 and the same score
    (gain * sqrt(d)) at d = 128, where a gain of 4 would put the bf16-P model of a head that does
    not follow the direction at 1.3e-2, over half the bound (the key's norm scales its rounding)"""
    return 4.0 * (64.0 / d) ** 0.5


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
        kc[b, n - 1] = (decode_key_gain(d) * u[b].float()).to(BF16)
        vc[b, n - 1] = LAST_V
        if n < L:
            kc[b, n] = kc[b, n - 1]
            vc[b, n:] = SENTINEL_V
    return q, kc, vc, lens


def decode64(q, kc, vc, lens):
    return attention64(q[:, None], kc, vc, lens)[:, 0]


# ------------------------------------------------------------------------------ norms, rope
GN_CASES = [(2, 17, 64, 8), (1, 1, 320, 32)]                               # (B, S, C, G), iid data (gn_inputs)


def _cdiv(a, b):
    return -(-a // b)


# ---- the row norms (norm.hip launch_ln): T lanes per row, VPL 8-element vectors per lane
LN_MAX_D = 4096


def ln_geometry_model(D) -> dict:
    """launch_ln / launch_ln_t on the CPU: lanes per row, vectors per lane, rows per 256-thread block"""
    V, T = D // 8, 1
    while T < 64 and T * 8 < V:
        T *= 2
    return {"T": T, "VPL": _cdiv(V, T), "rows_per_block": 4 * (64 // T)}


# D = 8 .. 64: VPL 1 .. 8 at T = 1; 72 and 104: T = 2 (104: V = 13, the last lane one vector short);
# 136 .. 2056: T = 4 .. 64 with a partial last vector round; the widths of the models; 4096: the cap
ROW_NORM_D = (8, 16, 24, 32, 40, 48, 56, 64, 72, 104, 136, 320, 384, 768, 1024, 1280, 2048, 2056, 4096)
# rows: one, five (a partial wave or block), and one more than a block holds (a second block of one row)
ROW_NORM_CASES = [(rows, D) for D in ROW_NORM_D for rows in sorted({1, 5, ln_geometry_model(D)["rows_per_block"] + 1})]
ROW_SCALE = (1.0, 2.0, 0.5)          # row r is ROW_SCALE[r % 3] * ((-1)^r + N(0, 1)): a mean and a scale of its own


def own_rows(rows, D, seed) -> torch.Tensor:
    """[rows, D] bf16 in which adjacent rows have means of opposite sign and scales a factor of 2
    or 4 apart, so a lane segment reduced into its neighbour's row (a shuffle offset >= T) shows
    in LayerNorm (the pooled mean) and in RMSNorm (the pooled mean square) alike"""
    r = torch.arange(rows)
    a = torch.tensor(ROW_SCALE)[r % 3]
    sgn = 1.0 - 2.0 * (r % 2)
    z = rnd(rows, D, seed=seed, dtype=torch.float32)
    return (a[:, None] * (sgn[:, None] + z)).to(BF16)


def norm_inputs(rows, D):
    s = 5000 + rows + D
    return own_rows(rows, D, s), rnd(D, scale=0.5, shift=1.0, seed=s + 1), rnd(D, scale=0.1, seed=s + 2)


def gn_inputs(B, S, C):
    s = 6000 + S + C
    return rnd(B, S, C, shift=0.5, seed=s), rnd(C, scale=0.5, shift=1.0, seed=s + 1), rnd(C, scale=0.1, seed=s + 2)


def embed_inputs(rows, D, vocab=50):
    s = 7000 + rows + D
    ids = torch.randint(0, vocab, (1, rows), generator=torch.Generator().manual_seed(s))
    return own_rows(vocab, D, s + 1), ids, rnd(rows + 3, D, scale=0.1, seed=s + 2), rnd(D, scale=0.1, seed=s + 3)


def layer_norm_model(x, g, b, eps=1e-5, rms=False, pair_rows=False) -> torch.Tensor:
    """LayerNorm / RMSNorm in fp64 with the bf16 store.  The planted bug ``pair_rows``: the
    reductions of rows 2k and 2k + 1 run together (xor offsets up to T instead of T / 2), so both
    rows get the mean and the variance of their 2 D elements; an unpaired last row is reduced
    with zeros."""
    xd = x.to(F64)
    rows, D = xd.shape
    if pair_rows:
        xp = torch.cat([xd, xd.new_zeros(rows % 2, D)]).view(-1, 2 * D)
        mean = (torch.zeros(xp.shape[0], 1, dtype=F64) if rms else xp.sum(-1, keepdim=True) / D)
        ms = ((xp - mean) ** 2).sum(-1, keepdim=True) / D
        mean, ms = (t.repeat_interleave(2, 0)[:rows] for t in (mean, ms))
    else:
        mean = torch.zeros(rows, 1, dtype=F64) if rms else xd.mean(-1, keepdim=True)
        ms = ((xd - mean) ** 2).mean(-1, keepdim=True)
    y = (xd - mean) * (ms + eps).rsqrt() * g.to(F64)
    return bf16_round(y if b is None else y + b.to(F64))


# ---- row_stats (the STATS instantiation of ln_kernel): float2 (mean, rstd) per row
def row_stats64(x, eps=1e-5):
    xd = x.to(F64)
    mean = xd.mean(-1)
    return mean, (((xd - mean[:, None]) ** 2).mean(-1) + eps).rsqrt()


def row_stats32(x, eps=1e-5):
    """the kernel's two-pass formula in fp32 (torch's summation order)"""
    xf = x.float()
    mean = xf.sum(-1) / xf.shape[-1]
    d = xf - mean[:, None]
    return mean, torch.rsqrt((d * d).sum(-1) / xf.shape[-1] + eps)


def row_stats_err(mean, rstd, x, eps=1e-5) -> tuple:
    """worst row of (|mean - mean64| * rstd64, |rstd / rstd64 - 1|): the mean's error in units of
    the row's deviation, which is what a consumer's (x - mean) * rstd sees, and the relative
    error of rstd"""
    m64, r64 = row_stats64(x, eps)
    m, r = mean.detach().to("cpu", F64), rstd.detach().to("cpu", F64)
    if not bool(torch.isfinite(m).all() and torch.isfinite(r).all()):
        return math.inf, math.inf
    return float(((m - m64).abs() * r64).max()), float((r / r64 - 1).abs().max())


# the fp32 formula's worst row over ROW_NORM_CASES, each figure rounded up to one digit
# (test_kernel_oracle.py::test_row_stats_floor measures them); the kernel, whose lane-tree order
# differs from torch's, gets four times as much
ROW_STATS_FLOOR = (2e-7, 2e-7)       # (mean, rstd)
ROW_STATS_BOUND = tuple(4 * f for f in ROW_STATS_FLOOR)
BOUND["row_stats mean"], BOUND["row_stats rstd"] = ROW_STATS_BOUND


# ---- GroupNorm by launch geometry (norm.hip group_norm_geometry; ext().group_norm_geometry)
GN_THREADS, GN_UNROLL, GN_APPLY_U, GN_APPLY_BLOCKS = 256, 4, 4, 1024
GN_MAX_C = 4096                      # group_norm / channel_stats instantiate VPT 1 and 2 only


def gn_geometry_model(B, S, C) -> dict:
    """group_norm_geometry on the CPU, under the default build and no environment knobs.
    ``two_pass`` (group_norm, channel_stats): gn_geom, gn_chunks, rows per chunk, and the apply's
    rows per block and blocks.  ``stats_fed`` (group_norm_stats, group_norm_cat): gn_apply_geom,
    the rows U a thread keeps in flight, and launch_apply's rows per block and blocks."""
    V = C // 8
    VPT = _cdiv(V, GN_THREADS)
    T = _cdiv(V, VPT)
    R = max(1, GN_THREADS // T)
    chunks = max(1, min(_cdiv(512, B), _cdiv(S, 4 * R)))
    rpb = 2 * GN_UNROLL * R
    if _cdiv(S, rpb) * B < 2048:
        rpb = GN_UNROLL * R
    two = {"VPT": VPT, "T": T, "R": R, "chunks": chunks, "rows_per_chunk": _cdiv(S, chunks),
           "rows_per_block": rpb, "blocks": _cdiv(S, rpb)}
    a, best = {"VPT": VPT, "T": T, "R": R}, -1
    for vpt in (1, 2):
        t = _cdiv(V, vpt)
        if t > GN_THREADS:
            continue
        r = GN_THREADS // t
        if r * t * 10 > best * 11:           # more than 10 % more active threads
            best, a = r * t, {"VPT": vpt, "T": t, "R": r}
    U = 8 if 512 <= C <= 1024 and S >= 4096 else GN_APPLY_U      # (VPT x U <= 16 holds for U = 4 at every VPT)
    step = U * a["R"]
    want = _cdiv(S, _cdiv(GN_APPLY_BLOCKS, B))
    rpb = step * _cdiv(want, step)
    return {"two_pass": two, "stats_fed": dict(a, U=U, rows_per_block=rpb, blocks=_cdiv(S, rpb))}


def _unrolled_and_tail(n, R) -> tuple:
    """over the row lanes of a chunk or block of n rows: does any lane run a whole GN_UNROLL-row
    iteration, does any run a single-row tail iteration (gn_stats_kernel, gn_apply_kernel)"""
    main = tail = False
    for rl in range(min(R, n)):
        r = rl
        while r + (GN_UNROLL - 1) * R < n:
            r, main = r + GN_UNROLL * R, True
        tail |= r < n
    return main, tail


def gn_fold_tpg(G) -> int:
    """threads per group of the statistics fold in gn_apply_cs_kernel"""
    return 1 if G >= GN_THREADS else next(t for t in (8, 4, 2, 1) if GN_THREADS // G >= t)


GN_BRANCHES = (
    "stats VPT=2",                   # C > 2048 in gn_stats_kernel / gn_apply_kernel / channel_stats_kernel
    "apply VPT=2 by the 10% rule",   # gn_apply_geom prefers two vectors per thread although one would cover the row
    "odd V, two-pass",               # the last lane's second vector is off (v >= V), VPT = 2
    "odd V, stats-fed",
    "idle row lanes",                # T * R < 256
    "R=1",
    "unrolled loop and tail",        # some row lanes of a chunk take the GN_UNROLL loop, some the single-row tail
    "ragged last chunk",
    "empty last chunk",
    "partial last apply block",      # load_group clamps rows to rend - 1
    "last block of one row",
    "pipelined loop twice",          # rows_per_block > U * R
    "U=8",
    "fold past 16 loads",            # Cg > 16 tpg: the fold's leftover loop
    "Cg straddles vectors",          # Cg % 8 != 0: one 8-channel vector, two groups
    "group straddles Ca",            # group_norm_cat: one group's channels come from both tensors
    "one thread, two tensors",       # group_norm_cat at VPT = 2: vector tv from x, vector tv + T from x2
)


def gn_branches(B, S, C, G, Ca, geom) -> set:
    """the branches of GN_BRANCHES a shape reaches under ``geom`` (the binding's or the model's)"""
    two, fed = geom["two_pass"], geom["stats_fed"]
    V, Cg = C // 8, C // G
    out = set()
    if two["VPT"] == 2:
        out.add("stats VPT=2")
        if V % 2:
            assert (two["T"] - 1) + two["T"] >= V
            out.add("odd V, two-pass")
    if fed["VPT"] == 2:
        if V <= GN_THREADS:
            out.add("apply VPT=2 by the 10% rule")
        if V % 2:
            out.add("odd V, stats-fed")
    if two["T"] * two["R"] < GN_THREADS or fed["T"] * fed["R"] < GN_THREADS:
        out.add("idle row lanes")
    if two["R"] == 1 and fed["R"] == 1:
        out.add("R=1")
    rpc, chunks = two["rows_per_chunk"], two["chunks"]
    sizes = {max(0, min(S, (k + 1) * rpc) - k * rpc) for k in range(chunks)}
    flags = [_unrolled_and_tail(n, two["R"]) for n in sizes]
    if any(m for m, _ in flags) and any(t for _, t in flags):
        out.add("unrolled loop and tail")
    if any(0 < n < rpc for n in sizes):
        out.add("ragged last chunk")
    if 0 in sizes:
        out.add("empty last chunk")
    last = S - (fed["blocks"] - 1) * fed["rows_per_block"]
    if last % (fed["U"] * fed["R"]):
        out.add("partial last apply block")
    if last == 1:
        out.add("last block of one row")
    if fed["rows_per_block"] > fed["U"] * fed["R"]:
        out.add("pipelined loop twice")
    if fed["U"] == 8:
        out.add("U=8")
    if Cg > 16 * gn_fold_tpg(G):
        out.add("fold past 16 loads")
    if Cg % 8:
        out.add("Cg straddles vectors")
    if Ca and Ca % Cg:
        out.add("group straddles Ca")
    if Ca and fed["VPT"] == 2 and any(8 * tv < Ca <= 8 * (tv + fed["T"]) and tv + fed["T"] < V for tv in range(fed["T"])):
        out.add("one thread, two tensors")
    return out


class GnCase(NamedTuple):
    B: int
    S: int
    C: int
    G: int
    Ca: int           # channels of the first tensor of group_norm_cat (0: no split, the case skips it)
    reaches: tuple    # the branches of GN_BRANCHES the case exists for

    @property
    def id(self):
        return f"{self.B}x{self.S}x{self.C}/{self.G}" + (f"-cat{self.Ca}" if self.Ca else "")


GN_GEOM_CASES = [
    GnCase(2, 300, 64, 8, 0, ("unrolled loop and tail", "partial last apply block")),          # R = 32, 3 chunks of 100, 3 blocks (44)
    GnCase(2, 37, 320, 32, 0, ("Cg straddles vectors", "idle row lanes", "ragged last chunk", "partial last apply block")),
    GnCase(2, 37, 320, 2, 0, ("fold past 16 loads",)),                                        # Cg = 160 > 16 * 8
    GnCase(2, 9, 2560, 32, 0, ("stats VPT=2", "R=1", "idle row lanes", "last block of one row")),
    GnCase(1, 7, 2056, 8, 0, ("stats VPT=2", "odd V, two-pass", "odd V, stats-fed", "R=1")),  # V = 257, T = 129
    GnCase(2, 21, 1032, 24, 0, ("apply VPT=2 by the 10% rule", "odd V, stats-fed", "ragged last chunk")),   # T = 65, R = 3; Cg = 43
    GnCase(1, 4100, 512, 32, 0, ("U=8", "ragged last chunk", "partial last apply block")),   # 129 blocks (4 rows), 257 chunks
    GnCase(256, 600, 64, 8, 0, ("pipelined loop twice",)),                                   # 19.7 MB, the largest
    GnCase(64, 33, 1032, 24, 0, ("empty last chunk",)),                                      # 8 chunks of 5 rows over 33
    GnCase(2, 29, 960, 32, 640, ("group straddles Ca",)),                                    # group 21: channels 630 .. 659
    GnCase(2, 29, 960, 32, 320, ("group straddles Ca",)),
    GnCase(3, 23, 1280, 32, 640, ("apply VPT=2 by the 10% rule", "one thread, two tensors")),
    GnCase(1, 5, GN_MAX_C, 32, 0, ("stats VPT=2", "R=1")),       # the cap: T = 256, the statistics kernel's LDS at 64 KiB exactly
]
GN_SIGMA = (0.5, 1.0, 2.0)


def gn_moments(B, G) -> tuple:
    """nominal (mu, sigma) [B, G] of the geometry cases' data: sigma of one group a factor of 2 or
    4 apart between consecutive images, adjacent groups' means of opposite sign, |mu| / sigma in
    1 .. 8 (all eight ratios within any eight adjacent groups).  The cap is derived: the one-pass
    variance of the two-pass path loses (mu^2 / sigma^2 + 1) * depth * 2^-24 relative to sigma^2,
    under 4e-4 at a depth of 100 fp32 additions."""
    b, g = torch.arange(B)[:, None], torch.arange(G)[None, :]
    sigma = torch.tensor(GN_SIGMA, dtype=F64)[(b + g) % 3]
    ratio = (1 + (3 * g + 5 * b) % 8).to(F64)
    return (1.0 - 2.0 * (g % 2)) * ratio * sigma, sigma


_GN_DATA = {}


def gn_case_inputs(c: GnCase):
    """x [B, S, C], gamma, beta (bf16, CPU), once per shape (do not modify)"""
    key = (c.B, c.S, c.C, c.G)
    if key not in _GN_DATA:
        s = 6500 + c.S + c.C + c.G
        mu, sigma = gn_moments(c.B, c.G)
        z = rnd(c.B, c.S, c.G, c.C // c.G, seed=s, dtype=torch.float32)
        x = (mu[:, None, :, None].float() + sigma[:, None, :, None].float() * z).reshape(c.B, c.S, c.C).to(BF16)
        _GN_DATA[key] = (x, rnd(c.C, scale=0.5, shift=1.0, seed=s + 1), rnd(c.C, scale=0.1, seed=s + 2))
    return _GN_DATA[key]


def gn_sums64(x, rows=None) -> torch.Tensor:
    """fp64 (sum, sum of squares, sum of magnitudes) [B, C, 3] over the rows [0, rows) of every image"""
    xd = x[:, :rows].to(F64)
    return torch.stack([xd.sum(1), (xd * xd).sum(1), xd.abs().sum(1)], dim=-1)


def group_norm_model(x, G, gam, be, eps, silu, geom=None, neighbour_stats=False, image0_stats=False,
                     drop_last_chunk=False, stats_a_past_ca=0, clamped_row=False, last_vector=None) -> torch.Tensor:
    """GroupNorm as the kernels compute it (mean = sum / n, var = sumsq / n - mean^2 from
    per-channel sums, then one multiply-add per element) in fp64, with the bf16 store.  The
    planted bugs: ``neighbour_stats`` (group g normalised with group g - 1's statistics),
    ``image0_stats`` (every image with image 0's), ``drop_last_chunk`` (the last non-empty
    statistics chunk of ``geom`` never summed, n unchanged), ``stats_a_past_ca`` = Ca (channels
    >= Ca index stats_a instead of stats_b: the next image's first channels, NaN past the last
    image), ``clamped_row`` (the first row of the last partial stats-fed block normalised from
    the values of the row its load was clamped to, the image's last), ``last_vector`` =
    "unwritten" | "raw" (the last 8-channel vector of every row never stored / stored as read)."""
    B, S, C = x.shape
    Cg = C // G
    rows = None
    if drop_last_chunk:
        rpc = geom["two_pass"]["rows_per_chunk"]
        rows = (_cdiv(S, rpc) - 1) * rpc
    sums = gn_sums64(x, rows)[..., :2]                                         # [B, C, 2]
    if stats_a_past_ca:
        Ca = stats_a_past_ca
        flat = torch.cat([sums[:, :Ca].reshape(B * Ca, 2), torch.full((C, 2), math.nan, dtype=F64)])
        idx = torch.arange(B)[:, None] * Ca + torch.arange(C)[None, :]
        sums = torch.where((torch.arange(C) < Ca)[None, :, None], sums, flat[idx])
    gs = sums.view(B, G, Cg, 2).sum(2)
    n = float(S * Cg)
    mean = gs[..., 0] / n
    rstd = ((gs[..., 1] / n - mean * mean).clamp_min(0) + eps).rsqrt()
    if neighbour_stats:
        mean, rstd = mean.roll(1, 1), rstd.roll(1, 1)
    if image0_stats:
        mean, rstd = mean[:1].expand(B, G), rstd[:1].expand(B, G)
    xd = x.to(F64)
    if clamped_row:
        fed = geom["stats_fed"]
        first = (fed["blocks"] - 1) * fed["rows_per_block"]
        assert first < S - 1
        xd = xd.clone()
        xd[:, first] = xd[:, S - 1]
    sc = gam.to(F64).view(G, Cg) * rstd[:, :, None]                            # [B, G, Cg]
    sf = be.to(F64).view(G, Cg) - mean[:, :, None] * sc
    y = xd.view(B, S, G, Cg) * sc[:, None] + sf[:, None]
    if silu:
        y = y / (1 + torch.exp(-y))
    y = bf16_round(y.reshape(B, S, C))
    if last_vector == "unwritten":
        y[..., -8:] = math.nan
    elif last_vector == "raw":
        y[..., -8:] = x[..., -8:]
    return y


def channel_stats_bound(x, two) -> tuple:
    """exact (fp64) per-(image, channel) sums [B, C, 2] of a bf16 x and channel_stats_kernel's
    error bound for them: gamma * sum|x| + chunks * 2^-25 and gamma * sum x^2 + chunks * 2^-17,
    gamma = (ceil(rows_per_chunk / R) + R + 1) * 2^-24: the worst case of the kernel's own fp32
    chain (a row lane's serial sum, then the R lanes of a channel) under ``two``, the binding's
    two-pass geometry, plus one fixed-point rounding (scales 2^24 and 2^16) per chunk's atomic"""
    s = gn_sums64(x)
    gamma = (_cdiv(two["rows_per_chunk"], two["R"]) + two["R"] + 1) * 2.0 ** -24
    bound = torch.stack([gamma * s[..., 2] + two["chunks"] * 2.0 ** -25, gamma * s[..., 1] + two["chunks"] * 2.0 ** -17], dim=-1)
    return s[..., :2], bound


def channel_stats_model(x, two, drop_row=None) -> torch.Tensor:
    """channel_stats_kernel's arithmetic on the CPU -> int64 [B, C, 2]: per chunk, row lane rl sums
    rows rl, rl + R, ... serially in fp32 (the squares by fused multiply-add), the R lanes of a
    channel are added in order, and the result is rounded once to fixed point.  The planted bug
    ``drop_row``: that row of every image is never read."""
    B, S, C = x.shape
    R, rpc, chunks = two["R"], two["rows_per_chunk"], two["chunks"]
    xf = x.float()
    if drop_row is not None:
        xf = xf.clone()
        xf[:, drop_row] = 0
    tot = torch.zeros(B, C, 2, dtype=torch.int64)
    for ck in range(chunks):
        rows = xf[:, ck * rpc:min(S, (ck + 1) * rpc)]
        s, q = torch.zeros(2, B, R, C)
        for i in range(_cdiv(rows.shape[1], R)):
            blk = rows[:, i * R:(i + 1) * R]
            n = blk.shape[1]
            s[:, :n] += blk
            q[:, :n] = (q[:, :n].double() + blk.double() ** 2).float()
        acc = torch.zeros(2, B, C)
        for k in range(R):
            acc[0] += s[:, k]
            acc[1] += q[:, k]
        tot[..., 0] += torch.round(acc[0].double() * 2.0 ** 24).to(torch.int64)
        tot[..., 1] += torch.round(acc[1].double() * 2.0 ** 16).to(torch.int64)
    return tot


def channel_stats_excess(got64, x, two) -> float:
    """worst (image, channel, statistic) of |got - exact| / bound; inf where ``got`` is not finite"""
    exact, bound = channel_stats_bound(x, two)
    got64 = got64.detach().to("cpu", F64)
    if not bool(torch.isfinite(got64).all()):
        return math.inf
    return float(((got64 - exact).abs() / bound).max())


def embed_ln64(word, ids, pos, add, g, b, eps=1e-5):
    """LayerNorm in fp64 of the embedding sum the encoder defines: word + pos and then + add are
    bf16 additions (an exact sum rounded to bf16 once each), as the eager model and ln_kernel<EMB>
    round them.  Against fp64 sums those two roundings alone put the ideal kernel at 7.8e-3 in the
    worst 8-element row of the cases (5.6e-3 with zero-mean rows), over half the bound; they are
    part of the operation, so the reference has them and a kernel that rounds otherwise shows."""
    x = (word.to(F64)[ids] + pos.to(F64)[: ids.shape[1]][None]).to(BF16)
    x = (x.to(F64) + add.to(F64)).to(BF16)
    return ref.layer_norm(x, g, b, eps, dtype=F64)


ROPE_CASES = [(2, 5, 4, 2, 64, 16, (3, 11)), (1, 1, 4, 4, 128, 8, (7,)), (3, 4, 2, 1, 64, 12, (0, 8, 5))]   # B, T, H, Hk, d, L, pos0


def rope64(qkv, pos0, H, Hk, d, theta=10000.0):
    """rotated q [B, T, H, d], rotated k and plain v [B, T, Hk, d] in fp64"""
    B, T, _ = qkv.shape
    x = qkv.view(B, T, H + 2 * Hk, d)
    pos = torch.tensor(pos0)[:, None] + torch.arange(T)[None, :]
    return (ref.rope(x[:, :, :H], pos, theta, dtype=F64), ref.rope(x[:, :, H:H + Hk], pos, theta, dtype=F64),
            x[:, :, H + Hk:].to(F64))


# ------------------------------------------------------------------------------ GEMV (lm.hip)
GEMV_STEP = 2048             # k elements one pass of the 256 lanes covers (8 each)
GATED = ("geglu", "swiglu")


class GemvCase(NamedTuple):
    M: int
    N: int            # outputs (W has 2N rows for the gated activations)
    K: int
    act: str

    @property
    def gated(self):
        return self.act in GATED

    @property
    def cols(self):
        """output columns one block of gemv_kernel owns: 4, or 2 for the gated M = 8 template"""
        return 2 if self.gated and self.M > 4 else 4

    @property
    def block(self):
        return (1, self.cols)

    @property
    def id(self):
        return f"{self.M}x{self.N}x{self.K}-{self.act}"


GEMV_N = (1, 5, 7, 70)
GEMV_K = (8, 72, 2048, 2056, 4096, 4104, 6152)      # one lane / one pass / the two-chunk loop once, twice, +- a lane


def gemv_cases() -> list:
    """per (M template, gated or not): every N at K = 72 and every K at N = 7 (gated: 3), the rows
    M of that template and its two activations taking turns.  M = 3 and 5 run the 4- and 8-row
    templates with idle rows.  N: a block's column tail (4 wide, 2 for the gated 8-row template);
    K: see GEMV_K."""
    cases = []
    for Ms in ((1,), (2,), (3, 4), (5, 8)):
        for acts in (("none", "silu"), GATED):
            gated = acts == GATED
            shapes = [(N, 72) for N in GEMV_N + ((3, 9) if gated and Ms == (5, 8) else ())]
            shapes += [(3 if gated else 7, K) for K in GEMV_K]
            shapes = list(dict.fromkeys(shapes))
            cases += [GemvCase(Ms[i % len(Ms)], N, K, acts[(i // len(Ms)) % 2]) for i, (N, K) in enumerate(shapes)]
    return cases


GEMV_CASES = gemv_cases()
GEMV_SIMT_CASE = GemvCase(3, 7, 12, "silu")                                # K % 8 != 0: not the GEMV's
RMS_CASES = [GemvCase(M, 7, K, act) for M in (1, 5, 8) for K in (8, 2056, 4104) for act in ("none", "swiglu")]
RMS_ROW_SCALE = (1.0, 2.0, 0.5)      # row m of x is scaled by 3 * RMS_ROW_SCALE[m % 3]: every row its own 1/rms
BMM_GEMV_CASES = [(3, M, 5, 72) for M in (1, 8)]                           # (batch, M, N, K)
BMM_ALPHA = 0.37
DISPATCH_M = (8, 9)                  # the last GEMV row count and the first MFMA one
DISPATCH_NK = (72, 128)              # N % 8 == 0 (statistics), K = Ca + Cb of linear_cat


def gemv_inputs(c: GemvCase):
    """x, w, bias, residual (bf16, CPU)"""
    Nw = 2 * c.N if c.gated else c.N
    s = 8000 + 7 * c.M + 3 * c.N + c.K + len(c.act)
    return (rnd(c.M, c.K, seed=s), rnd(Nw, c.K, scale=c.K ** -0.5, seed=s + 1), rnd(Nw, scale=0.1, seed=s + 2),
            rnd(c.M, c.N, seed=s + 3))


def rms_inputs(c: GemvCase):
    """x (rows scaled by 3 * RMS_ROW_SCALE), gamma, w, bias, residual"""
    x, w, b, r = gemv_inputs(c)
    sc = torch.tensor([3 * RMS_ROW_SCALE[m % 3] for m in range(c.M)])
    x = (x.float() * sc[:, None]).to(BF16)
    return x, rnd(c.K, scale=0.3, shift=1.0, seed=c.K + c.M), w, b, r


def rms_linear64(x, g, w, b, r, act, eps=1e-5):
    return ref.linear(ref.rms_norm(x, g, eps, dtype=F64), w, b, residual=r, act=act, dtype=F64)


def gemv_model(c: GemvCase, x, w, b, r, gamma=None, eps=1e-5, skip_tail_column=False, drop_last_chunk=False,
               rms_of_row0=False) -> Guarded:
    """gemv_kernel in fp64 with its one rounding (the bf16 store), written into a guarded output
    as the kernel writes it.  The planted bugs: ``skip_tail_column`` never stores the last column
    of a partial block, ``drop_last_chunk`` leaves the 8 k-elements at K - 8 out of every dot
    product, ``rms_of_row0`` scales every row by row 0's 1/rms."""
    xd, wd = x.to(F64), w.to(F64)
    scale = torch.ones(c.M, 1, dtype=F64)
    if gamma is not None:
        ss = (xd * xd).mean(-1, keepdim=True)
        scale = (ss[:1].expand_as(ss) if rms_of_row0 else ss).add(eps).rsqrt()
        xd = xd * gamma.to(F64)
    if drop_last_chunk:
        xd = xd.clone()
        xd[:, c.K - 8:] = 0
    y = (xd @ wd.t()) * scale + b.to(F64)
    if c.gated:
        h, g = y.chunk(2, dim=-1)
        y = h * (torch.nn.functional.gelu(g) if c.act == "geglu" else torch.nn.functional.silu(g))
    elif c.act == "silu":
        y = torch.nn.functional.silu(y)
    y = y + r.to(F64)
    out = guarded((c.M, c.N))
    n = c.N - 1 if skip_tail_column and c.N % c.cols else c.N
    out.view[:, :n] = y[:, :n].to(BF16)
    return out


# ------------------------------------------------------------------------------ decode attention, the edges
# (L, group, d, lens or None): every head dim and the odd / largest group at a span's edge; above
# L = 4096 decode_splits stays at 32 splits and a split's span grows to 256 keys
DECODE_EDGE_CASES = ([(L, g, 128, None) for L in (127, 129) for g in (3, 8)] +
                     [(L, 2, 64, (L, 1, 257)) for L in (4097, 4224)])


def decode_edge_data(L, group, d, lens):
    """decode_data with the dominant last key / sentinel V construction at ``lens``"""
    q, kc, vc, ln = decode_data(L, group, d)
    if lens is None:
        return q, kc, vc, ln
    s = 4500 + 3 * L + group
    kc, vc = rnd(3, L, 2, d, seed=s + 1), rnd(3, L, 2, d, seed=s + 2)
    u = rnd(3, 2, d, seed=4000 + 3 * L + group + 3)           # decode_data's directions (its q follows them)
    for b, n in enumerate(lens):
        kc[b, n - 1] = (decode_key_gain(d) * u[b].float()).to(BF16)
        vc[b, n - 1] = LAST_V
        if n < L:
            kc[b, n] = kc[b, n - 1]
            vc[b, n:] = SENTINEL_V
    return q, kc, vc, list(lens)


# ------------------------------------------------------------------------------ sampler (lm_sample_kernel)
SAMPLE_CHUNK = 1024          # ids one pass of the tie cut covers
PROBE_NOISE = 1e4
NEG_INF = -math.inf


class SampleCase(NamedTuple):
    name: str
    logits: torch.Tensor      # fp32 [V]
    k: int
    eos: int
    eos_bias: float
    signed_zero: bool = False


def _neg(V, seed):
    """distinct negative logits, none of them a zero"""
    return -(0.5 + torch.rand(V, generator=torch.Generator().manual_seed(seed)) * 6)


def sampler_cases() -> list:
    cs = []
    for V in (1, 255, 1024, 1025, 2049):
        for k in dict.fromkeys((1, 40, V, V + 5)):
            cs.append(SampleCase(f"rand-V{V}-k{k}", rnd(V, scale=3.0, seed=V + k, dtype=torch.float32), k, 7 % V, 0.0))
    for k in (40, 1500):                                     # all equal: the cut keeps ids 0 .. k - 1
        cs.append(SampleCase(f"equal-k{k}", torch.full((2049,), 1.5), k, 7, 0.0))
    lg = _neg(2049, 1)                                       # 20 above, 1500 tied at the k-th place: `need` = 1200
    lg[100:1600] = 1.0                                       # crosses the chunk of ids < 1024 (924 tied there)
    lg[2000:2020] = 5.0 + torch.arange(20) / 8
    cs.append(SampleCase("tie-across-chunks", lg, 1220, 7, 0.0))
    # -0.0 and +0.0 at the k-th place (k = 3: the contract keeps {2, 5, 9}, a key order that puts
    # -0.0 below +0.0 keeps {2, 9, 11} / {2, 5, 11})
    for name, z in (("minus-zero-at-lower-id", (-0.0, 0.0, 0.0)), ("minus-zero-at-higher-id", (0.0, -0.0, 0.0))):
        lg = _neg(300, 2)
        lg[2] = 4.0
        lg[5], lg[9], lg[11] = z
        cs.append(SampleCase(name, lg, 3, 7, 0.0, signed_zero=True))
    lg = rnd(255, scale=3.0, seed=3, dtype=torch.float32)    # members that never win
    lg[3] = lg[200] = NEG_INF
    cs.append(SampleCase("neg-inf-members", lg, 255, 7, NEG_INF))
    for eos in (0, 1024):
        cs.append(SampleCase(f"eos-at-{eos}", rnd(1025, scale=3.0, seed=4, dtype=torch.float32), 40, eos, 5.0))
    return cs


SAMPLER_CASES = sampler_cases()


def sample_values(logits, T, eos, eos_bias) -> torch.Tensor:
    """v of the contract: logits.float() / T with the EOS bias (fp32, as ops.reference.lm_sample)"""
    v = logits.float().reshape(-1) / T
    if 0 <= eos < v.numel():
        v[eos] += eos_bias
    return v


def rank_probes(logits, T, k, eos, eos_bias):
    """noise rows [n, 1, V] that put PROBE_NOISE on the id ranked k - 1, k and k + 1 (1-based, in
    the reference's stable descending order) and 0 elsewhere, then one row of Gumbel noise; with
    them the probed ids and whether each is inside the top-k set"""
    v = sample_values(logits, T, eos, eos_bias)
    V = v.numel()
    order = torch.sort(v, descending=True, stable=True).indices
    kk = min(k, V)
    ranks = [r for r in (kk - 1, kk, kk + 1) if 1 <= r <= V]
    noise = torch.zeros(len(ranks) + 1, 1, V)
    ids = [int(order[r - 1]) for r in ranks]
    for i, t in enumerate(ids):
        noise[i, 0, t] = PROBE_NOISE
    u = torch.rand(V, generator=torch.Generator().manual_seed(V + k)).clamp_(1e-10, 1 - 1e-7)
    noise[-1, 0] = -torch.log(-torch.log(u))
    return noise, ids, [r <= kk for r in ranks]


def fkey(v: torch.Tensor) -> torch.Tensor:
    """lm.hip's order-preserving float -> uint32 key (as int64)"""
    u = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(u >= 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def sampler_model(logits, noise_row, T, k, eos, eos_bias, canonical_zero=True, admit=0) -> int:
    """lm_sample_kernel's selection on the CPU: top-k by (key descending, id ascending), then the
    id maximising v + noise (ties: larger v, then lower id).  The planted bugs: ``admit`` lets
    that many more ranks into the set, ``canonical_zero=False`` keys -0.0 below +0.0."""
    v = sample_values(logits, T, eos, eos_bias)
    if canonical_zero:
        v = v + 0.0
    V = v.numel()
    key = fkey(v)
    order = sorted(range(V), key=lambda i: (-int(key[i]), i))[:min(k + admit, V)]
    sc = v + noise_row.reshape(-1)
    return min(order, key=lambda i: (-float(sc[i]), -float(v[i]), i) if not math.isnan(float(sc[i])) else (math.inf, 0, i))


def run_sampler(fn, logits, noise, T, k, eos, eos_bias, device="cpu"):
    """``fn`` (ops.lm_sample's signature) over every noise row, chained on the device counters:
    (out, tok, pos, lens, step)"""
    n = noise.shape[0]
    step = torch.zeros(1, device=device, dtype=torch.long)
    out = torch.full((n, 1), -1, device=device, dtype=torch.long)
    tok = torch.zeros(1, device=device, dtype=torch.long)
    pos = torch.zeros(1, device=device, dtype=torch.int32)
    lens = torch.ones(1, device=device, dtype=torch.int32)
    eb = torch.full((n,), eos_bias, device=device)
    lg, nz = logits.to(device).reshape(1, -1), noise.to(device)
    for _ in range(n):
        fn(lg, nz, eb, eos, T, k, step, out, tok, pos, lens)
    return out.flatten().tolist(), int(tok), int(pos), int(lens), int(step)


# ------------------------------------------------------------------------------ scorer (misc.hip)
COS_ATOL = 1e-5              # the fp32 test's absolute tolerance, for bf16 tables too: both sides share the inputs
COS_FLOOR = 5e-6             # the same formula in fp32 stays under this (test_kernel_oracle.py)
COS_D = (1, 8, 63, 64, 65, 300)
COS_N = (1, 4, 5)
COS_ROWS = 8                 # table rows; row COS_ZERO_ROW is all zero, the last one is used as an index
COS_ZERO_ROW = 3
COS_PAIRS = ((COS_ROWS - 1, 0), (2, 2), (COS_ZERO_ROW, 1), (0, 1), (4, 5))


def cos_table(D, dtype, rows=COS_ROWS, seed=0):
    t = rnd(rows, D, seed=9000 + D + seed, dtype=torch.float32)
    if rows > COS_ZERO_ROW:
        t[COS_ZERO_ROW] = 0
    return t.to(dtype)


def cosine64(a, b):
    """fp64 cosine of rows, 0 where a norm is 0 (the kernels' clamp)"""
    a, b = a.to(F64), b.to(F64)
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1)).clamp_min(1e-12)


def cosine32(a, b):
    """the kernels' formula in fp32: fp32 products and sums, sqrt(na) * sqrt(nb), clamp 1e-12"""
    a, b = a.float(), b.float()
    return (a * b).sum(-1) / ((a * a).sum(-1).sqrt() * (b * b).sum(-1).sqrt()).clamp_min(1e-12)


POOL_D = (8, 384, 1000)
POOL_LENS = (9, 1, 4, 0, 12)
POOL_T = 9
BOUND["pool"] = 1e-5         # per row, fp32 out: 9 + ~12 fp32 roundings per element (test_kernel_oracle.py measures the floor)


def pool_inputs(D):
    """hidden [5, 9, D] bf16 with NaN in every token at or past lens[b] (the empty row keeps token
    0 finite: the kernel may not use it either), and the lengths"""
    h = rnd(len(POOL_LENS), POOL_T, D, seed=9500 + D)
    for b, n in enumerate(POOL_LENS):
        h[b, max(n, 1):] = math.nan
    return h, torch.tensor(POOL_LENS, dtype=torch.int32)


def mean_pool64(h, lens, min_len=0):
    """fp64 masked mean and normalisation; an empty row is the zero vector.  ``min_len=1``: the
    planted L = max(1, .) rule"""
    out = torch.zeros(h.shape[0], h.shape[2], dtype=F64)
    for b, n in enumerate(lens.tolist()):
        n = max(min_len, min(n, h.shape[1]))
        if n > 0:
            s = h[b, :n].to(F64).mean(0)
            out[b] = s / s.norm().clamp_min(1e-12)
    return out


def mean_pool32(h, lens):
    out = torch.zeros(h.shape[0], h.shape[2])
    for b, n in enumerate(lens.tolist()):
        n = min(n, h.shape[1])
        if n > 0:
            s = torch.zeros(h.shape[2])
            for t in range(n):
                s = s + h[b, t].float()
            s = s / float(n)
            out[b] = s * (1.0 / (s * s).sum().sqrt().clamp_min(1e-12))
    return out


TOPK_CHUNK = 2048
TOPK_D = 8
TOPK_CASES = ((1, 1), (2047, 5), (2048, 5), (2049, 1024), (2049, 5), (1024, 1024), (6145, 1024), (6145, 51))   # (V, k)
TOPK_TOL = 2e-5              # two scores COS_ATOL from their fp64 values may swap


def topk_inputs(V, dtype):
    """table [V, 8], query, the rows that are bit-identical copies of the query (ascending)"""
    t = rnd(V, TOPK_D, seed=9700 + V, dtype=torch.float32).to(dtype)
    vec = rnd(TOPK_D, seed=9701, dtype=torch.float32).to(dtype)
    if V > COS_ZERO_ROW:
        t[COS_ZERO_ROW] = 0
    planted = sorted({r for r in (2047, 2048, 4096, V - 1) if 0 <= r < V and r != COS_ZERO_ROW})
    for r in planted:
        t[r] = vec
    return t, vec, planted


def topk_model(s: torch.Tensor, k: int, padding_surfaces=False):
    """topk_partial_kernel / topk_merge_kernel on scores ``s``: 2048-row chunks padded with the
    key 0, each sorted and cut to k, merged until one is left.  A key is (orderable score, ~row);
    the planted bug gives padding the key of a score of +0.0 at row 0xffffffff - slot instead"""
    V = s.numel()
    keys = [(int(fkey(s[i:i + 1] + 0.0)), 0xFFFFFFFF - i) for i in range(V)]
    chunks = []
    for c0 in range(0, V, TOPK_CHUNK):
        ch = keys[c0:c0 + TOPK_CHUNK]
        pad = TOPK_CHUNK - len(ch)
        ch = ch + [((0x80000000, j) if padding_surfaces else (0, 0)) for j in range(pad)]
        chunks.append(sorted(ch, reverse=True)[:k])
    flat = [x for ch in chunks for x in ch]
    best = sorted(flat, reverse=True)[:k]
    return [0xFFFFFFFF - r for _, r in best]


def check_topk(vals, idx, s64, k, planted):
    """the assertions of a cosine_topk result against the fp64 scores"""
    V = s64.numel()
    vals, idx = vals.to("cpu", F64), idx.cpu().long()
    assert idx.numel() == k and len(set(idx.tolist())) == k, "rows repeat"
    assert int(idx.min()) >= 0 and int(idx.max()) < V, "a row outside the table (a padding key surfaced)"
    assert bool((vals[1:] <= vals[:-1]).all()), "vals must be non-increasing"
    top = torch.sort(s64, descending=True).values
    assert float((vals - s64[idx]).abs().max()) <= COS_ATOL
    assert float((s64[idx] - top[:k]).abs().max()) <= TOPK_TOL
    must = (s64 > top[k - 1] + TOPK_TOL).nonzero().flatten().tolist()
    assert set(must) <= set(idx.tolist()), "a row clearly inside the top k is missing"
    n = min(len(planted), k)
    assert idx[:n].tolist() == planted[:n], "copies of the query come first, the lower row first"
    assert n == 0 or bool((vals[:n] == vals[0]).all())


# ------------------------------------------------------------------------------ glue (misc.hip)
def all_bf16(with_inf=True) -> torch.Tensor:
    """every finite bf16 bit pattern (65280 of them, a multiple of 8), then -inf and +inf"""
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    fin = x[torch.isfinite(x.float())]
    assert fin.numel() == 65280
    return torch.cat([fin, torch.tensor([-math.inf, math.inf], dtype=BF16)]) if with_inf else fin


def bf16_ordinal(t: torch.Tensor) -> torch.Tensor:
    """bf16 -> integers in which neighbouring values differ by one (both zeros are 0)"""
    i = t.contiguous().view(torch.int16).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def silu64(x):
    xd = x.to(F64)
    return xd / (1 + torch.exp(-xd))


GLUE_ROWS = (1, 3)
GLUE_D = (8, 24)
COPY_BYTES = (1, 15, 16, 17, 4096 + 7)
FINALIZE_N = (1, 3, 4, 5, 4099)
