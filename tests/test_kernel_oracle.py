"""The instruments of kernel_oracle.py, proven on the CPU with ``ops.reference`` as the kernel:
the ideal kernel (fp64 math, one rounding where the HIP kernels round) stays under half the bound
in every block of every case test_kernel_edges_gpu.py, test_kernel_edges_conv_gpu.py,
test_kernel_edges_decode_gpu.py and test_kernel_edges_scorer_gpu.py run, and each planted bug -- those of the first file all get past
the whole-tensor error of tests/test_kernels_gpu.py -- fails its check.  The sampler, the top-k
and mean_pool_l2 have models of the kernels' own selection rules here; their planted bugs are the
ones those kernels had or could have (a tie cut one rank too wide, -0.0 keyed below +0.0, a
padding key that surfaces, the first token of an empty row).  For norm.hip
(test_kernel_edges_norm_gpu.py) the launch geometry has a transcript here: every case reaches the
branches it names, and the planted bugs are those of that geometry (the neighbouring group's or
image 0's statistics, the last statistics chunk missing, the last vector of an odd row, channels
past Ca read from the first statistics buffer, a row normalised from the row its load was clamped
to, two LayerNorm rows reduced together, a row missing from channel_stats)."""
import math

import pytest
import torch

import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.ops import reference as ref
from kernel_oracle import BF16, BOUND, F64, bf16_round, block_rel_err
from test_gemm_menu import header_rows

FLOOR = {}      # table row -> (family, the ideal kernel's worst block over the cases run so far)
CONV_TILE_CASES = ko.conv_tile_cases(header_rows())


def _conv_case(**kw):
    """a case of the table by its fields (the first that matches; tile 3 unless ``cfg`` is given)"""
    kw.setdefault("cfg", 3)
    return next(c for c in CONV_TILE_CASES if all(getattr(c, k) == v for k, v in kw.items()))


def floor(family, err, what, row=None):
    """``row``: a line of its own in the table for cases that share a family's bound"""
    FLOOR[row or family] = (family, max(FLOOR.get(row or family, (family, 0.0))[1], err))
    assert err < 0.5 * BOUND[family], (family, what, err)


def global_rel_err(out, ref64):
    return ((out.to(F64) - ref64).norm() / ref64.norm()).item()


# ------------------------------------------------------------------------------ the ideal kernel passes
def test_ideal_gemm():
    for c in ko.gemm_cases(header_rows()) + ko.raster_gemm_cases(header_rows()):
        x, w, b, r = ko.gemm_inputs(c)
        y64 = ko.linear64(x, w, b, r, c.act)
        floor("gemm", block_rel_err(bf16_round(y64), y64), c.id)
    for M, N, K in ko.AREG_CASES:
        x, w, b, r = ko.gemm_inputs(ko.GemmCase(15, 1, M, N, K, "silu"))
        y64 = ko.linear64(x, w, b, r, "silu")
        floor("gemm", block_rel_err(bf16_round(y64), y64), ("areg", M, N, K))
        for n in (N, ko.AREG_FALLBACK_N):
            x, g, be, w, b = ko.ln_fold_inputs(M, n, K, seed=M + K)
            floor("ln_fold", block_rel_err(ko.ideal_ln_fold(x, g, be, w, b), ko.ln_linear64(x, g, be, w, b)), (M, n, K))
    for _, N, K in ko.AREG_CASES[:2] + [(0, ko.AREG_FALLBACK_N, 320), (0, ko.AREG_FALLBACK_N, 640)]:   # gn_linear: B = 1, S = 256
        x, g, be, w, b = ko.ln_fold_inputs(256, N, K, seed=K)
        x = x[None]
        y64 = ko.gn_linear64(x, g, be, 32, 1e-6, w, b)
        xn = ref.group_norm(x, 32, g, be, 1e-6, False, dtype=F64).to(BF16)      # the A rows the MFMA sees
        floor("gn_fold", block_rel_err(bf16_round(ko.linear64(xn, w, b))[0], y64[0]), ("gn", K))
    for Ca, Cb in ko.CAT_CASES:
        x, w, b, _ = ko.gemm_inputs(ko.GemmCase(-1, 0, 129, ko.CAT_N, Ca + Cb, "none"))
        y64 = ko.linear64(x, w, b)
        floor("gemm", block_rel_err(bf16_round(y64), y64), ("cat", Ca, Cb))
    M, N, K = ko.ROW_STATS_CASE
    x, g, be, w, b = ko.ln_fold_inputs(M, 72, N, seed=77)
    floor("ln_fold", block_rel_err(ko.ideal_ln_fold(x, g, be, w, b), ko.ln_linear64(x, g, be, w, b)), "row_stats")


def test_ideal_conv():
    for B, H, W, Cin, Cout, stride in ko.CONV_CASES + [ko.RASTER_CONV]:
        args = ko.conv_inputs(B, H, W, Cin, Cout, stride)
        y64 = ko.conv64(*args, stride=stride).flatten(0, 2)
        floor("conv", block_rel_err(bf16_round(y64), y64), (B, H, W, Cin, Cout, stride))
    B, H, W, Cin, Cout = ko.UP2_CASE
    for cin in (Cin, ko.UP2_SPLIT_CIN):
        y64 = ko.conv64(*ko.conv_inputs(B, H, W, cin, Cout, up=True), up=True).flatten(0, 2)
        floor("conv", block_rel_err(bf16_round(y64), y64), ("up2", cin))
    seen = set()
    for c in CONV_TILE_CASES:                                  # the tiles share their data: once per reference
        (x, w, b, cb, res), y64 = ko.conv_case_data(c)
        if id(y64) not in seen:
            seen.add(id(y64))
            floor("conv", block_rel_err(bf16_round(y64).flatten(0, 2), y64.flatten(0, 2)), c.id, "conv, tile by tile")


def test_conv_model_is_the_reference():
    """the im2col model the planted conv bugs are cut from, sliced as split-K cuts it, is the
    reference itself: within the bf16 store of it at every stride, kernel size and split"""
    for c in (_conv_case(split=1, geom="s1"), _conv_case(split=1, geom="s2"), _conv_case(split=4, Cin=128),
              _conv_case(split=7, Cin=256), _conv_case(group="modes", split=1, Cin=24, geom="s2"),
              _conv_case(group="modes", split=1, op="1x1")):
        args, y64 = ko.conv_case_data(c)
        y = ko.conv_model(*args, stride=ko.CONV_GEOM[c.geom][3], split=c.split)
        assert block_rel_err(y.flatten(0, 2), y64.flatten(0, 2)) < 0.5 * BOUND["conv"], c.id
        assert (y != bf16_round(y64)).float().mean().item() < 1e-3, c.id       # (a summation order apart)


IDEAL_ATTN = ([(str(d), d) for d in (32, 40, 64, 80, 160, 256, 512) + ko.ATTN_ROUNDUP_D] +
              [("lm", "lm")] + [("wide-" + c.id, c) for c, _, _ in ko.ATTN_WIDE_CASES])


@pytest.mark.parametrize("d", [d for _, d in IDEAL_ATTN], ids=[i for i, _ in IDEAL_ATTN])
def test_ideal_attention(d):
    """``d``: a head dim (attn_cases and the single cases at that dim), "lm" (the GQA and prefill
    cases at d = 128) or one wide-grid case"""
    if isinstance(d, ko.AttnCase):
        cases = [d]
    elif d == "lm":
        cases = ko.attn_cases(128, *ko.LM_HEADS) + [ko.PREFILL_CASE]
    else:
        cases = ko.attn_cases(d) + ([ko.GQA_CASE] if d == 64 else []) + ([ko.D512_SPLIT_CASE] if d == 512 else [])
    row = None if d in (32, 40, 64, 80, 160, 256, 512) else "attention, dispatch"     # a table line for the instantiation cases
    for c in cases:
        q, k, v = ko.attn_data(c)
        o64 = ko.attention64(q, k, v, c.lens, c.causal)
        floor("attention", block_rel_err(ko.ideal_attention(q, k, v, c.lens, c.causal), o64, (1, 16, 1, None)), c.id, row)
        if d == 64:                                           # the cases the fp8 kernel runs
            floor("fp8", block_rel_err(ko.ideal_attention(q, k, v, c.lens, c.causal, fp8=True), o64, (1, 16, 1, None)), c.id)


def test_ideal_decode_attention():
    for L in ko.DECODE_L:
        for g in ko.DECODE_GROUPS:
            q, kc, vc, lens = ko.decode_data(L, g)
            o64 = ko.decode64(q, kc, vc, lens)
            o = ko.ideal_attention(q[:, None], kc, vc, lens)[:, 0]
            floor("decode", block_rel_err(o, o64, (1, 1, None)), (L, g))
            # ops.reference.decode_attention is the same function up to its fp32 math
            assert block_rel_err(ref.decode_attention(q, kc, vc, torch.tensor(lens), 64 ** -0.5), o64, (1, 1, None)) < BOUND["decode"]


def test_ideal_norms_and_rope():
    for rows, D in ko.ROW_NORM_CASES:
        x, g, b = ko.norm_inputs(rows, D)
        for y64 in (ref.layer_norm(x, g, b, 1e-5, dtype=F64), ref.layer_norm(x, g, None, 1e-5, dtype=F64),
                    ref.rms_norm(x, g, 1e-5, dtype=F64)):
            floor("norm", block_rel_err(bf16_round(y64), y64, (1, None)), (rows, D))
        word, ids, pos, add = ko.embed_inputs(rows, D)
        y64 = ko.embed_ln64(word, ids, pos, add, g, b)
        floor("norm", block_rel_err(bf16_round(y64), y64, (1, 1, None)), ("embed", rows, D))
    for B, S, C, G in ko.GN_CASES:
        x, g, b = ko.gn_inputs(B, S, C)
        for silu in (False, True):
            y64 = ref.group_norm(x, G, g, b, 1e-5, silu, dtype=F64)
            floor("group_norm", block_rel_err(bf16_round(y64), y64, (1, 16, C // G)), (B, S, C, G, silu))
    for c in ko.GN_GEOM_CASES:
        x, g, b = ko.gn_case_inputs(c)
        for silu in (False, True):
            y64 = ref.group_norm(x, c.G, g, b, 1e-5, silu, dtype=F64)
            floor("group_norm", block_rel_err(bf16_round(y64), y64, (1, 16, c.C // c.G)), (c.id, silu), "group_norm, geometry")
    for B, T, H, Hk, d, L, pos0 in ko.ROPE_CASES:
        qkv = ko.rnd(B, T, (H + 2 * Hk) * d, seed=T + d)
        for y64 in ko.rope64(qkv, pos0, H, Hk, d):
            floor("rope", block_rel_err(bf16_round(y64), y64, (1, 1, 1, None)), (B, T, H, Hk, d))


# ------------------------------------------------------------------------------ planted bugs
def _linear_257():
    """the smallest shape of test_kernels_gpu.py::test_gemm, with its bias and residual"""
    x, w, b, r = ko.rnd(257, 320, seed=1), ko.rnd(320, 320, scale=320 ** -0.5, seed=2), ko.rnd(320, scale=0.1, seed=3), ko.rnd(257, 320, seed=4)
    return x, w, b, r, ko.linear64(x, w, b, r)


def test_bias_dropped_in_the_last_row_fails():
    x, w, b, r, y64 = _linear_257()
    bad = y64.clone()
    bad[-1] = ko.linear64(x[-1:], w, None, r[-1:])[0]
    bad = bf16_round(bad)
    assert global_rel_err(bad, y64) < 1e-2                    # the whole-tensor check lets it through
    assert block_rel_err(bad, y64) > 2 * BOUND["gemm"]
    assert block_rel_err(bf16_round(y64), y64) < 0.5 * BOUND["gemm"]


def test_bias_dropped_in_the_last_8_columns_fails():
    x, w, b, r, y64 = _linear_257()
    bad = y64.clone()
    bad[:, -8:] = ko.linear64(x, w[-8:], None, r[:, -8:])
    bad = bf16_round(bad)
    assert global_rel_err(bad, y64) < 1e-2
    assert block_rel_err(bad, y64) > 2 * BOUND["gemm"]


def test_row_group_with_another_rows_layernorm_statistics_fails():
    M, N, K = 129, 72, 320
    x, g, be, w, b = ko.ln_fold_inputs(M, N, K, seed=9)
    y64 = ko.ln_linear64(x, g, be, w, b)
    wf, _, bf = ops.ln_fold(g, be, w, b)
    xd = x.to(F64)
    mean, rstd = xd.mean(-1, keepdim=True), (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    mean[16:32], rstd[16:32] = mean[0], rstd[0]               # one 16-row group: row 0's statistics
    bad = bf16_round(rstd * (xd @ wf.to(F64).t() - mean * wf.to(F64).sum(1)) + bf.to(F64))
    assert block_rel_err(bad, y64) > BOUND["ln_fold"]
    assert block_rel_err(ko.ideal_ln_fold(x, g, be, w, b), y64) < 0.5 * BOUND["ln_fold"]


@pytest.mark.parametrize("Nk", [63, 64, 65, 129])
def test_key_past_kv_lens_included_fails(Nk):
    c = ko.AttnCase(3, 33, Nk, 2, 2, 64, (Nk, 1, 0), False)
    q, k, v = ko.attn_data(c)
    o64 = ko.attention64(q, k, v, c.lens)
    assert block_rel_err(ko.ideal_attention(q, k, v, c.lens, extra_key=True), o64, (1, 16, 1, None)) > BOUND["attention"]
    assert block_rel_err(ko.ideal_attention(q, k, v, c.lens), o64, (1, 16, 1, None)) < 0.5 * BOUND["attention"]


@pytest.mark.parametrize("causal", [False, True])
def test_last_valid_key_dropped_fails(causal):
    c = ko.AttnCase(3, 65, 65, 2, 2, 64, None if causal else (65, 1, 0), causal)
    q, k, v = ko.attn_data(c)
    o64 = ko.attention64(q, k, v, c.lens, causal)
    assert block_rel_err(ko.ideal_attention(q, k, v, c.lens, causal, drop_last=True), o64, (1, 16, 1, None)) > BOUND["attention"]


def test_causal_future_key_included_fails():
    c = ko.attn_cases(64)[-1]
    q, k, v = ko.attn_data(c)
    o64 = ko.attention64(q, k, v, None, True)
    assert block_rel_err(ko.ideal_attention(q, k, v, None, True, extra_key=True), o64, (1, 16, 1, None)) > BOUND["attention"]


def test_planted_key_bugs_fail_on_a_wide_grid():
    """B = 33, H = 16 (the 8-wave d = 32 case): one block in 2112 still decides"""
    c = ko.ATTN_WIDE_CASES[0][0]
    assert c.B == 33 and c.lens is not None
    q, k, v = ko.attn_data(c)
    o64 = ko.attention64(q, k, v, c.lens)
    for bug in ({"drop_last": True}, {"extra_key": True}):
        e = block_rel_err(ko.ideal_attention(q, k, v, c.lens, **bug), o64, (1, 16, 1, None))
        print(f"wide grid {bug}: worst block {e:.3e}")
        assert e > BOUND["attention"], bug


def test_wide_cases_cross_the_launch_thresholds():
    """the grid arithmetic of launch_nw / launch_attention (attention.hip) on the wide cases: each
    sits at or just above the block count that selects the kernel it names, at the smallest B"""
    for c, want, alt in ko.ATTN_WIDE_CASES:
        blocks4, blocks8 = -(-c.Nq // 128) * c.H * c.B, -(-c.Nq // 256) * c.H * c.B
        for fam, dqk, do, nw in (want,) + ((alt,) if alt else ()):
            if fam == "a16":
                assert nw == 8 and not c.causal and c.d == 40 and blocks8 >= 256 > -(-c.Nq // 256) * c.H * (c.B - 3)
            elif nw == 8:
                assert do <= 96 and blocks8 >= 1024 > -(-c.Nq // 256) * c.H * (c.B - 3), c.id
            else:
                assert nw == 4 and (do > 96 or blocks8 < 1024) and (blocks4 >= 512 or (c.Nq >= 256 and blocks4 >= 16)), c.id
        assert c.lens is None or (len(c.lens) == c.B and c.lens[-1] == 0)
    c = ko.PREFILL_CASE
    assert ko.PREFILL_KERNEL[2] > 96 and c.Nq >= 256 and -(-c.Nq // 128) * c.H * c.B >= 16 and -(-c.Nk // 64) == 5
    assert {ko.attn_template_width(d) for d in ko.ATTN_ROUNDUP_D} == set(ko.ATTN_TEMPLATE_WIDTHS)
    assert {d for d in ko.ATTN_ROUNDUP_D if d in ko.ATTN_TEMPLATE_WIDTHS} == {96, 128}


def _raster_walk(nM, nN, G, partial_group=True):
    """tiles in launch order: every block id through xcd_remap, then tile_of.  ``partial_group=False``:
    the planted raster whose last group is as tall as the others"""
    tiles = []
    for bid in range(nM * nN):
        lin = ko.xcd_remap_model(bid, nM * nN)
        if partial_group or G <= 1:
            tiles.append(ko.tile_of_model(lin, nM, nN, G))
        else:
            g = min(G, nM)
            grp, r = divmod(lin, g * nN)
            tiles.append((grp * g + r % g, r // g))
    return tiles


def test_raster_is_a_bijection_and_a_planted_one_fails():
    """the CPU transcript of xcd_remap and tile_of visits each of the 18 tiles once for every G;
    without the partial last group, a tile is never written and another is outside the grid: the
    NaN-prefilled guarded output shows it as an infinite block"""
    nM, nN = ko.RASTER_TILES
    for c in ko.raster_gemm_cases(header_rows()):
        assert ko.raster_tiles(c, header_rows()) == (nM, nN), c.id
    all_tiles = sorted((m, n) for m in range(nM) for n in range(nN))
    partial = []
    for G in ko.RASTER_GROUPS:
        g = G or 4
        assert sorted(_raster_walk(nM, nN, g)) == all_tiles, G
        if nM > g > 1 and nM % g:
            partial.append(G)
            bad = _raster_walk(nM, nN, g, partial_group=False)
            assert sorted(bad) != all_tiles
            c = ko.GemmCase(3, 1, 5 * 128 + 1, 2 * 64 + 8, 72, "silu")
            y64 = ko.linear64(*ko.gemm_inputs(c), c.act)
            out = ko.guarded((c.M, c.N))
            for tm, tn in bad:
                if tm < nM:
                    out.view[tm * 128:(tm + 1) * 128, tn * 64:(tn + 1) * 64] = bf16_round(y64)[tm * 128:(tm + 1) * 128, tn * 64:(tn + 1) * 64]
            assert block_rel_err(out.view, y64) == math.inf
    assert partial == [0, 4, 5]


def test_decode_key_past_lens_or_dropped_fails():
    q, kc, vc, lens = ko.decode_data(129, 2)
    o64 = ko.decode64(q, kc, vc, lens)
    for bug in ({"extra_key": True}, {"drop_last": True}):
        assert block_rel_err(ko.ideal_attention(q[:, None], kc, vc, lens, **bug)[:, 0], o64, (1, 1, None)) > BOUND["decode"]


def test_element_written_past_the_output_fails():
    for shape, dtype in (((257, 72), BF16), ((3, 33, 2, 64), BF16), ((2, 8, 2), torch.int64), ((5,), torch.float32)):
        g = ko.guarded(shape, dtype)
        assert g.view.is_contiguous() and tuple(g.view.shape) == shape
        assert g.guard * g.view.element_size() >= min(256 * shape[-1] * g.view.element_size(), 1 << 20)
        g.view.zero_()
        ko.check_guards(g)
        for off in (g.guard + g.view.numel(), g.guard - 1, 0, g.buf.numel() - 1):
            h = ko.guarded(shape, dtype)
            h.view.zero_()
            ko.int_view(h.buf)[off] = 0
            assert not ko.guards_intact(h)
            with pytest.raises(AssertionError):
                ko.check_guards(h)
    # an unwritten output element is a NaN of the pattern: the block error sees it
    g = ko.guarded((17, 24))
    y64 = torch.ones(17, 24, dtype=F64)
    g.view.fill_(1.0)
    assert block_rel_err(g.view, y64) == 0.0
    ko.int_view(g.view)[16, 23] = g.pattern
    assert block_rel_err(g.view, y64) == math.inf


def test_nan_read_past_the_k_columns_of_a_strided_x_fails():
    x, w, b, r, y64 = _linear_257()
    xs = ko.poisoned(x, strided=True)
    assert torch.equal(xs, x) and xs.stride(0) > x.shape[1] and not xs.is_contiguous()
    assert block_rel_err(bf16_round(ko.linear64(xs, w, b, r)), y64) < 0.5 * BOUND["gemm"]
    # a kernel that loads one more 8-wide chunk of every row and multiplies it by zero weights
    wide = torch.as_strided(xs, (257, 328), xs.stride(), xs.storage_offset())
    wz = torch.cat([w, torch.zeros(320, 8, dtype=BF16)], dim=1)
    assert block_rel_err(bf16_round(ko.linear64(wide, wz, b, r)), y64) == math.inf
    # contiguous operands: the rows before and after are NaN
    xc = ko.poisoned(x)
    assert xc.is_contiguous() and torch.equal(xc, x)
    flat = torch.as_strided(xc, (x.numel() + 2,), (1,), xc.storage_offset() - 1)
    assert math.isnan(flat[0].item()) and math.isnan(flat[-1].item())
    q = ko.poisoned(ko.rnd(3, 5, 2, 16), strided=True, row_dims=2)
    assert q.stride(1) == 2 * 16 + 16 and q.stride(2) == 16 and all(s % 8 == 0 for s in q.stride()[:3])


# ------------------------------------------------------------------------------ planted conv bugs
def _conv_bug(c, **kw):
    """(block error of the planted bug, of the unharmed model) on case ``c``"""
    args, y64 = ko.conv_case_data(c)
    stride, y64 = ko.CONV_GEOM[c.geom][3], y64.flatten(0, 2)
    good = block_rel_err(ko.conv_model(*args, stride=stride, split=c.split).flatten(0, 2), y64)
    return block_rel_err(ko.conv_model(*args, stride=stride, split=c.split, **kw).flatten(0, 2), y64), good


@pytest.mark.parametrize("geom", ["s1", "s2"])
def test_conv_left_padding_tap_from_the_previous_row_fails(geom):
    """the linear tap offset of the buffer modes without the per-lane tap mask: ix = -1 is the
    previous row's last pixel"""
    bad, good = _conv_bug(_conv_case(split=1, geom=geom, Cin=64), wrap_left=True)
    assert bad > 2 * BOUND["conv"] and good < 0.5 * BOUND["conv"], (bad, good)


@pytest.mark.parametrize("geom", ["s1", "s2"])
def test_conv_two_images_as_one_tall_image_fails(geom):
    """rows bounded by the batch, not the image: only the pixel rows next to the image boundary
    differ (2 of 18 at stride 1, 1 of 20 at stride 2: the second image's top; the first one's
    bottom row 18 is real padding of an odd H)"""
    bad, good = _conv_bug(_conv_case(split=1, geom=geom, Cin=64), one_image=True)
    assert bad > 2 * BOUND["conv"] and good < 0.5 * BOUND["conv"], (bad, good)


@pytest.mark.parametrize("split,Cin", [(4, 128), (7, 256)])
def test_split_k_sum_without_the_last_non_empty_slice_fails(split, Cin):
    c = _conv_case(split=split, Cin=Cin)
    last = max(s for s, n in enumerate(ko.split_slices(c.nk, c.split)) if n > 0)
    bad, good = _conv_bug(c, drop_slice=last)
    assert bad > 2 * BOUND["conv"] and good < 0.5 * BOUND["conv"], (bad, good)
    if split == 7:                                             # the empty slice adds nothing
        args, _ = ko.conv_case_data(c)
        assert torch.equal(ko.conv_model(*args, split=7, drop_slice=6), ko.conv_model(*args, split=7))


# ------------------------------------------------------------------------------ the conv case table
def test_conv_case_table_structure():
    """every live non-areg tile has a stride-1, a stride-2, a short-slice, an empty-slice and
    an up2 case (plain and split), the split cases with either reduce kernel; the slices are
    what ceil(nk / split) gives; the shapes are what the tiles need"""
    assert ko.split_slices(18, 4) == [5, 5, 5, 3] and ko.split_slices(36, 7) == [6] * 6 + [0]
    assert ko.split_slices(20, 3) == [7, 7, 6] and ko.split_slices(9, 1) == [9]
    menu = [r for r in header_rows() if r[1] != "areg"]
    assert {c.cfg for c in CONV_TILE_CASES} == {r[0] for r in menu}
    assert len({c.id for c in CONV_TILE_CASES}) == len(CONV_TILE_CASES)
    deepest = max(r[5] for r in menu)
    for cid, fam, BM, BN, _, stages, *_ in menu:
        mine = [c for c in CONV_TILE_CASES if c.cfg == cid]
        have = lambda **kw: [c for c in mine if all(getattr(c, k) == v for k, v in kw.items())]   # noqa: E731
        assert have(op="conv", geom="s1", split=1, Cin=64) and have(op="conv", geom="s2", split=1, Cin=64)
        for split, nk, slices in ((4, 18, [5, 5, 5, 3]), (7, 36, [6] * 6 + [0])):
            cs = have(op="conv", geom="s1", split=split, nk=nk)
            assert {c.stats for c in cs if c.Cout % 8 == 0} == {True, False}, (cid, split)
            assert ko.split_slices(nk, split) == slices and nk // split >= 4       # the planner's nk / split >= 4
        assert min(ko.split_slices(18, 4)) < min(4, deepest) and ko.split_slices(36, 7)[-1] == 0
        assert have(op="up2", split=1, nk=4) and {c.stats for c in have(op="up2", split=3, nk=20)} == {True, False}
        for c in mine:
            B, H, W, stride = ko.CONV_GEOM[c.geom]
            up = 2 if c.op in ("up2", "fused_up") else 1
            hw = ((H - 1) // stride + 1) * ((W - 1) // stride + 1) * (1 if c.op == "up2" else up * up)   # GEMM rows per image
            M = B * hw
            assert M > BM and M % BM != 0, (c.id, M)                             # a full M tile and a partial one
            assert B == 2 and hw % BM != 0, c.id                                 # the image boundary inside a tile
            assert W % 16 != 0 and (c.Cout == BN + 8 or (BN == 16 and c.Cout == 16) or c.Cout == BN + 4), c.id
            assert (BN <= 16) == (c.Cout <= 16) and c.Cout % 4 == 0              # the BN <= 16 rule, can_split
            assert c.split == 1 or c.nk // c.split >= 4, c.id
            assert not c.stats or c.Cout % 8 == 0, c.id
            if fam != "static":                                                    # family_runs
                assert c.Cin % 64 == 0 and c.op in ("conv", "up2") and c.Cout > 16 and c.Cout % 8 == 0, c.id
        if fam == "static":
            assert {(c.Cin, c.geom) for c in have(group="modes", op="conv", split=1)} == {(ci, g) for ci in (32, 24) for g in ("s1", "s2")}
            assert {c.Cin for c in have(op="fused_up")} == {64, 32} and have(op="1x1")
    assert [c for c in CONV_TILE_CASES if c.Cout % 8 != 0 and c.split > 1 and not c.stats], "N % 8 != 0 through the plain reduce"


def test_conv_cases_cover_the_tuning_table():
    """every conv / conv2d_up2 entry of the committed tuning table: its (tile, kind) is in the
    case table, and a tile the table splits has a split case of that kind's family (plain / up2)"""
    import json
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "gemm_tuning.json")
    key = re.compile(r"^m\d+ n\d+ k\d+ w\d+ b\d+ c(\d+):\d+:\d+:\d+:(\d+):\d+:\d+:\d+ p(\d+) ")      # gemm_key (gemm.hip)
    have = {(c.cfg, c.kind) for c in CONV_TILE_CASES}
    have_split = {(c.cfg, c.op == "up2") for c in CONV_TILE_CASES if c.split > 1}
    n = 0
    for e in json.load(open(path))["entries"]:
        m = key.match(e["key"])
        assert m, e["key"]
        conv, stride, parity = (int(v) for v in m.groups())
        if not conv:
            continue
        n += 1
        kind = "up2" if parity else {1: "s1", 2: "s2"}[stride]
        assert kind in ko.CONV_KINDS and (int(e["cfg"]), kind) in have, e
        assert int(e["split"]) == 1 or (int(e["cfg"]), bool(parity)) in have_split, e
    assert n > 0


def test_block_rel_err_blocks():
    r = torch.ones(33, 20, dtype=F64)
    o = r.clone()
    o[32, 19] = 2.0                                            # the 1 x 4 corner block
    assert block_rel_err(o, r) == pytest.approx(0.5)
    assert block_rel_err(o, r, (None, None)) == pytest.approx(1 / math.sqrt(660))
    z = torch.zeros(4, 8, dtype=F64)
    assert block_rel_err(z, z, (1, None)) == 0.0
    o = z.clone()
    o[3, 0] = 1e-3                                             # a zero reference row must be zero exactly
    assert block_rel_err(o, z, (1, None)) == math.inf


# ------------------------------------------------------------------------------ the empty-row contract
def test_attention_without_a_valid_key_is_zero():
    q, k, v = ko.rnd(3, 5, 2, 16, seed=1), ko.rnd(3, 7, 2, 16, seed=2), ko.rnd(3, 7, 2, 16, seed=3)
    lens = torch.tensor([7, 1, 0], dtype=torch.int32)
    o = ref.attention(q, k, v, kv_lens=lens)
    assert o.dtype == BF16 and torch.isfinite(o.float()).all()
    assert not o[2].any() and o[0].any() and o[1].any()
    assert torch.equal(o[:2], ref.attention(q[:2], k[:2], v[:2], kv_lens=lens[:2]))
    assert torch.equal(o[0], ref.attention(q[:1], k[:1], v[:1])[0])                # full rows: as before
    assert torch.equal(o[1], ref.attention(q[1:2], k[1:2, :1], v[1:2, :1])[0])
    assert torch.equal(ops.attention(q, k, v, kv_lens=lens), o)                    # CPU dispatch
    # masked K/V never reach the result, whatever they hold
    k2, v2 = k.clone(), v.clone()
    k2[1, 1:], v2[1, 1:], v2[2] = math.nan, math.inf, math.nan
    assert torch.equal(ref.attention(q, k2, v2, kv_lens=lens), o)
    kc, vc = ko.rnd(3, 9, 2, 16, seed=4), ko.rnd(3, 9, 2, 16, seed=5)
    qd = ko.rnd(3, 4, 16, seed=6)
    od = ref.decode_attention(qd, kc, vc, torch.tensor([9, 0, 4]), 0.25)
    assert torch.isfinite(od.float()).all() and not od[1].any() and od[0].any() and od[2].any()
    assert torch.equal(ops.decode_attention(qd, kc, vc, torch.tensor([9, 0, 4]), 0.25), od)


# ------------------------------------------------------------------------------ decode, sampler, scorer: the ideal kernel passes
def test_ideal_gemv():
    """gemv_kernel's blocks are one row x 4 columns (2 for the gated 8-row template); the bf16 store
    alone stays under half the bound there, so the family keeps its narrow block"""
    assert 80 <= len(ko.GEMV_CASES) <= 100 and len({c.id for c in ko.GEMV_CASES}) == len(ko.GEMV_CASES)
    for c in ko.GEMV_CASES:
        x, w, b, r = ko.gemv_inputs(c)
        g = ko.gemv_model(c, x, w, b, r)
        ko.check_guards(g)
        floor("gemm", block_rel_err(g.view, ko.linear64(x, w, b, r, c.act), c.block), c.id, "gemv")
    for c in ko.RMS_CASES:
        x, gam, w, b, r = ko.rms_inputs(c)
        g = ko.gemv_model(c, x, w, b, r, gamma=gam)
        floor("gemm", block_rel_err(g.view, ko.rms_linear64(x, gam, w, b, r, c.act), c.block), c.id, "gemv + rms")
    for Bt, M, N, K in ko.BMM_GEMV_CASES:
        a, b = ko.rnd(Bt, M, K, seed=M), ko.rnd(Bt, N, K, seed=M + 1)
        y64 = ko.BMM_ALPHA * a.to(F64) @ b.to(F64).transpose(1, 2)
        floor("gemm", block_rel_err(bf16_round(y64), y64, (1, 1, 4)), ("bmm", M), "gemv bmm_nt")
    N, K = ko.DISPATCH_NK
    for M in ko.DISPATCH_M + (9,):                             # (9: the row_stats producer's inputs)
        x, w, b, r = ko.gemv_inputs(ko.GemvCase(M, N, K, "none"))
        y64 = ko.linear64(x, w, b, r)
        floor("gemm", block_rel_err(bf16_round(y64), y64, (1, 4)), ("dispatch", M), "gemv | mfma")
        x, g, be, w, b = ko.ln_fold_inputs(M, N, K, seed=M)
        y64 = ko.ln_linear64(x, g, be, w, b)
        floor("ln_fold", block_rel_err(ko.ideal_ln_fold(x, g, be, w, b), y64, (1, None)), ("dispatch ln", M), "gemv | mfma ln")
        xn = ref.layer_norm(x, g, be, 1e-5, dtype=F64).to(BF16)                  # <= 8 rows: LayerNorm kernel, then the GEMV
        floor("ln_fold", block_rel_err(bf16_round(ko.linear64(xn, w, b)), y64, (1, None)), ("dispatch ln", M), "gemv | mfma ln")


def test_ideal_decode_attention_edges():
    for L, g, d, lens in ko.DECODE_EDGE_CASES:
        q, kc, vc, ln = ko.decode_edge_data(L, g, d, lens)
        assert kc.numel() <= 3 * 4224 * 2 * 64 and (lens is None or ln == list(lens))
        o64 = ko.decode64(q, kc, vc, ln)
        floor("decode", block_rel_err(ko.ideal_attention(q[:, None], kc, vc, ln)[:, 0], o64, (1, 1, None)), (L, g, d), "decode edges")
        for bug in ({"extra_key": True}, {"drop_last": True}):
            assert block_rel_err(ko.ideal_attention(q[:, None], kc, vc, ln, **bug)[:, 0], o64, (1, 1, None)) > BOUND["decode"]


SAMPLER_VARIANTS = [(dt, T) for dt in (BF16, torch.float32) for T in (1.0, 0.8)]


def test_rank_probes_hold_for_the_reference_and_the_ideal_sampler():
    """ops.reference.lm_sample under the probes: the ids ranked k - 1 and k win, the one ranked
    k + 1 does not (where their values are finite), and the model of the kernel agrees with it"""
    for c in ko.SAMPLER_CASES:
        for dt, T in SAMPLER_VARIANTS:
            lg = c.logits.to(dt)
            noise, ids, inside = ko.rank_probes(lg, T, c.k, c.eos, c.eos_bias)
            out = ko.run_sampler(ref.lm_sample, lg, noise, T, c.k, c.eos, c.eos_bias)
            assert out[1:] == (out[0][-1], len(out[0]), 1 + len(out[0]), len(out[0]))
            v = ko.sample_values(lg, T, c.eos, c.eos_bias)
            for got, t, ins in zip(out[0], ids, inside):
                if math.isfinite(float(v[t])):
                    assert (got == t) == ins, (c.name, dt, T, got, t, ins)
            model = [ko.sampler_model(lg, noise[i], T, c.k, c.eos, c.eos_bias) for i in range(noise.shape[0])]
            assert model == out[0], (c.name, dt, T)


def test_sampler_cases_reach_the_paths_they_are_for():
    by = {c.name: c for c in ko.SAMPLER_CASES}
    assert {c.logits.numel() for c in ko.SAMPLER_CASES} >= {1, 255, 1024, 1025, 2049}
    c = by["tie-across-chunks"]
    v = ko.sample_values(c.logits, 1.0, c.eos, c.eos_bias)
    order = torch.sort(v, descending=True, stable=True).indices
    kth = float(v[order[c.k - 1]])
    tied = (v == kth).nonzero().flatten()
    need = c.k - int((v > kth).sum())
    assert tied.numel() == 1500 and need > int((tied < ko.SAMPLE_CHUNK).sum()) and int(order[c.k - 1]) >= ko.SAMPLE_CHUNK
    c = by["equal-k1500"]
    assert int(torch.sort(c.logits, descending=True, stable=True).indices[c.k - 1]) == c.k - 1 >= ko.SAMPLE_CHUNK
    for name, keep in (("minus-zero-at-lower-id", [2, 5, 9]), ("minus-zero-at-higher-id", [2, 5, 9])):
        c = by[name]
        for dt in (BF16, torch.float32):
            order = torch.sort(ko.sample_values(c.logits.to(dt), 0.8, c.eos, 0.0), descending=True, stable=True).indices
            assert sorted(order[:3].tolist()) == keep and bool((c.logits[[5, 9, 11]] == 0).all())
    assert math.copysign(1, float(by["minus-zero-at-lower-id"].logits[5])) == -1
    assert math.copysign(1, float(by["minus-zero-at-higher-id"].logits[9])) == -1


def test_cosine_fp32_floor():
    """the kernels' formula in fp32 against fp64 on every scorer case: under COS_FLOOR, half the tolerance"""
    worst = 0.0
    for dt in (torch.float32, BF16):
        for D in ko.COS_D:
            t = ko.cos_table(D, dt)
            ia, ib = (torch.tensor(p) for p in zip(*ko.COS_PAIRS))
            worst = max(worst, float((ko.cosine32(t[ia], t[ib]) - ko.cosine64(t[ia], t[ib])).abs().max()))
            assert float(ko.cosine64(t[2], t[2])) == pytest.approx(1.0, abs=1e-12)
            assert float(ko.cosine64(t[ko.COS_ZERO_ROW], t[1])) == 0.0 == float(ko.cosine32(t[ko.COS_ZERO_ROW], t[1]))
            vec = ko.cos_table(D, dt, rows=1, seed=1)[0]
            worst = max(worst, float((ko.cosine32(t, vec[None]) - ko.cosine64(t, vec[None])).abs().max()))
        for V, _k in ko.TOPK_CASES:
            t, vec, _ = ko.topk_inputs(V, dt)
            worst = max(worst, float((ko.cosine32(t, vec[None]) - ko.cosine64(t, vec[None])).abs().max()))
    print(f"cosine: fp32 formula's worst error {worst:.2e} (floor {ko.COS_FLOOR:g}, tolerance {ko.COS_ATOL:g})")
    assert worst < ko.COS_FLOOR


def test_ideal_mean_pool_and_topk():
    for D in ko.POOL_D:
        h, lens = ko.pool_inputs(D)
        y64 = ko.mean_pool64(h, lens)
        assert torch.isfinite(y64).all() and not y64[3].any()
        floor("pool", block_rel_err(ko.mean_pool32(h, lens), y64, (1, None)), D)
        assert torch.allclose(ref.mean_pool_l2(torch.nan_to_num(h.float()), lens).to(F64), y64, atol=1e-6)   # the contract, zero row included
    for dt in (torch.float32, BF16):
        for V, k in ko.TOPK_CASES:
            t, vec, planted = ko.topk_inputs(V, dt)
            s64 = ko.cosine64(t, vec[None])
            s32 = ko.cosine32(t, vec[None])
            idx = torch.tensor(ko.topk_model(s32, k))
            ko.check_topk(s32[idx], idx, s64, k, planted)
            assert torch.equal(idx, ref.cosine_topk(t, vec, k).indices)


# ------------------------------------------------------------------------------ decode, sampler, scorer: planted bugs
def test_gemv_tail_column_skipped_fails():
    hit = 0
    for c in ko.GEMV_CASES:
        if c.K != 72:
            continue
        x, w, b, r = ko.gemv_inputs(c)
        e = block_rel_err(ko.gemv_model(c, x, w, b, r, skip_tail_column=True).view, ko.linear64(x, w, b, r, c.act), c.block)
        assert (e == math.inf) == (c.N % c.cols != 0), c.id
        hit += e == math.inf
    assert hit >= 20


def test_gemv_last_k_chunk_dropped_fails():
    for c in ko.GEMV_CASES:
        if c.N not in (3, 7) or c.K == 72:
            continue
        x, w, b, r = ko.gemv_inputs(c)
        e = block_rel_err(ko.gemv_model(c, x, w, b, r, drop_last_chunk=True).view, ko.linear64(x, w, b, r, c.act), c.block)
        assert e > BOUND["gemm"], (c.id, e)


def test_gemv_rms_of_row_0_for_every_row_fails():
    for c in ko.RMS_CASES:
        x, gam, w, b, r = ko.rms_inputs(c)
        e = block_rel_err(ko.gemv_model(c, x, w, b, r, gamma=gam, rms_of_row0=True).view,
                          ko.rms_linear64(x, gam, w, b, r, c.act), c.block)
        assert (e > BOUND["gemm"]) == (c.M > 1), (c.id, e)


def test_sampler_that_admits_rank_k_plus_1_fails():
    caught = 0
    for c in ko.SAMPLER_CASES:
        lg = c.logits.to(BF16)
        noise, ids, inside = ko.rank_probes(lg, 0.8, c.k, c.eos, c.eos_bias)
        want = ko.run_sampler(ref.lm_sample, lg, noise, 0.8, c.k, c.eos, c.eos_bias)[0]
        bad = [ko.sampler_model(lg, noise[i], 0.8, c.k, c.eos, c.eos_bias, admit=1) for i in range(noise.shape[0])]
        if not all(inside):                                   # a rank k + 1 exists
            assert bad != want, c.name
            caught += 1
    assert caught >= 15


def test_sampler_that_ranks_minus_zero_below_zero_fails():
    for c in ko.SAMPLER_CASES:
        for dt, T in SAMPLER_VARIANTS:
            lg = c.logits.to(dt)
            noise, _, _ = ko.rank_probes(lg, T, c.k, c.eos, c.eos_bias)
            want = ko.run_sampler(ref.lm_sample, lg, noise, T, c.k, c.eos, c.eos_bias)[0]
            bad = [ko.sampler_model(lg, noise[i], T, c.k, c.eos, c.eos_bias, canonical_zero=False) for i in range(noise.shape[0])]
            assert (bad != want) == c.signed_zero, (c.name, dt, T)


def test_topk_padding_key_that_surfaces_fails():
    t, vec, planted = ko.topk_inputs(1024, torch.float32)
    s64, s32 = ko.cosine64(t, vec[None]), ko.cosine32(t, vec[None])
    idx = torch.tensor(ko.topk_model(s32, 1024, padding_surfaces=True))
    assert int(idx.max()) >= 1024
    with pytest.raises(AssertionError):
        ko.check_topk(s32[idx.clamp(max=1023)], idx, s64, 1024, planted)
    t, vec, planted = ko.topk_inputs(2049, torch.float32)            # the last chunk holds one real row
    s64, s32 = ko.cosine64(t, vec[None]), ko.cosine32(t, vec[None])
    idx = torch.tensor(ko.topk_model(s32, 1024, padding_surfaces=True))
    with pytest.raises(AssertionError):
        ko.check_topk(s32[idx.clamp(max=2048)], idx, s64, 1024, planted)


def test_mean_pool_that_reads_one_token_of_an_empty_row_fails():
    for D in ko.POOL_D:
        h, lens = ko.pool_inputs(D)
        y64 = ko.mean_pool64(h, lens)
        assert block_rel_err(ko.mean_pool64(h, lens, min_len=1), y64, (1, None)) == math.inf
        assert block_rel_err(ko.mean_pool64(h, lens), y64, (1, None)) == 0.0


def test_ideal_kv8_writer():
    """the ideal single-rounding writer of the fp8 K/V image, e4m3(y64), on the A-in-registers cases
    of test_kernel_edges_kv8_gpu.py: BOUND["kv8"] is twice its worst 16-key x 64-d block, rounded up
    to one digit (the bf16-then-e4m3 writers are byte-exact against the model and need no bound)"""
    geom = ko.KV8_EPI_GEOMS[0]
    worst = 0.0
    for C in ko.KV8_AREG_C:
        y64 = ko.ln_linear64(*ko.kv8_epi_inputs(geom, C))
        for t in ko.qkv_split(y64, geom, C)[1:]:
            e = block_rel_err(ko.e4m3(t), t, ko.KV8_BLOCK)
            worst = max(worst, e)
            floor("kv8", e, C)
    digit = 10.0 ** math.floor(math.log10(2 * worst))
    assert BOUND["kv8"] == pytest.approx(math.ceil(2 * worst / digit) * digit, rel=1e-12), worst


# ------------------------------------------------------------------------------ norm.hip by launch geometry
GN_BLOCK = lambda c: (1, 16, c.C // c.G)      # noqa: E731


def _gn_ref(c):
    x, g, b = ko.gn_case_inputs(c)
    return x, g, b, ref.group_norm(x, c.G, g, b, 1e-5, False, dtype=F64)


def test_gn_geometry_cases_reach_their_branches():
    """under the CPU transcript of group_norm_geometry every case reaches the branches it names,
    every branch of GN_BRANCHES has a case, and the two iid cases reach none of the launch
    branches (one chunk, one block, VPT = 1: what the table exists to change)"""
    seen = set()
    for c in ko.GN_GEOM_CASES:
        got = ko.gn_branches(c.B, c.S, c.C, c.G, c.Ca, ko.gn_geometry_model(c.B, c.S, c.C))
        assert set(c.reaches) <= got, (c.id, set(c.reaches) - got)
        assert set(c.reaches) <= set(ko.GN_BRANCHES)
        seen |= set(c.reaches)
        assert c.C <= ko.GN_MAX_C and c.C % 8 == 0 and c.C % c.G == 0 and c.Ca % 8 == 0
    assert seen == set(ko.GN_BRANCHES), set(ko.GN_BRANCHES) - seen
    for B, S, C, G in ko.GN_CASES:
        got = ko.gn_branches(B, S, C, G, 0, ko.gn_geometry_model(B, S, C))
        assert got <= {"idle row lanes", "Cg straddles vectors", "partial last apply block", "last block of one row"}, got
    # the shapes past the cap: a third vector per thread that launch_group_norm / launch_channel_stats
    # have no instantiation for, and an LDS request over 64 KiB
    two = ko.gn_geometry_model(1, 8, ko.GN_MAX_C + 8)["two_pass"]
    assert two["VPT"] == 3 and 2 * two["T"] < (ko.GN_MAX_C + 8) // 8
    assert 4 * (2 * two["R"] + 2) * (ko.GN_MAX_C + 8) > 65536 >= 4 * (2 * 1 + 2) * ko.GN_MAX_C
    assert ko.gn_geometry_model(1, 8, ko.GN_MAX_C)["two_pass"]["VPT"] == 2


def test_gn_data_recipe():
    for B, G in ((2, 32), (3, 32), (256, 8), (2, 2)):
        mu, sigma = ko.gn_moments(B, G)
        assert bool((mu[:, 1:] * mu[:, :-1] < 0).all())
        ratio = mu.abs() / sigma
        assert 1 <= float(ratio.min()) and float(ratio.max()) <= 8
        r = sigma[1:] / sigma[:-1]
        assert bool((torch.maximum(r, 1 / r) >= math.sqrt(2)).all())
    c = ko.GN_GEOM_CASES[0]
    x = ko.gn_case_inputs(c)[0].to(F64).view(c.B, c.S, c.G, -1)
    mu, sigma = ko.gn_moments(c.B, c.G)
    assert float(((x.mean((1, 3)) - mu) / sigma).abs().max()) < 0.1 and float((x.std((1, 3)) / sigma - 1).abs().max()) < 0.1


def test_group_norm_planted_bugs_fail_on_every_case():
    """the model without a bug is the reference (half the bound to spare); each planted bug is
    over the bound in the worst block of every case it applies to"""
    applied = {k: 0 for k in ("neighbour", "image0", "chunk", "vector", "ca", "clamp")}
    for c in ko.GN_GEOM_CASES:
        x, g, b, y64 = _gn_ref(c)
        geom = ko.gn_geometry_model(c.B, c.S, c.C)
        got = ko.gn_branches(c.B, c.S, c.C, c.G, c.Ca, geom)
        err = lambda **bug: block_rel_err(ko.group_norm_model(x, c.G, g, b, 1e-5, False, geom, **bug), y64, GN_BLOCK(c))  # noqa: E731
        assert err() < 0.5 * BOUND["group_norm"], c.id
        figures = {"neighbour": err(neighbour_stats=True)}
        if c.B > 1:
            figures["image0"] = err(image0_stats=True)
        if ko._cdiv(c.S, geom["two_pass"]["rows_per_chunk"]) > 1:
            figures["chunk"] = err(drop_last_chunk=True)
        if (c.C // 8) % 2:
            figures["vector"] = err(last_vector="raw")
            assert err(last_vector="unwritten") == math.inf
        if c.Ca:
            figures["ca"] = err(stats_a_past_ca=c.Ca)
        fed = geom["stats_fed"]
        if "partial last apply block" in got and c.S - (fed["blocks"] - 1) * fed["rows_per_block"] > 1:
            figures["clamp"] = err(clamped_row=True)
        print(c.id, {k: f"{v:.2e}" for k, v in figures.items()})
        for k, v in figures.items():
            applied[k] += 1
            assert v > BOUND["group_norm"], (c.id, k, v)
    assert all(n >= 2 for n in applied.values()), applied


def test_iid_data_lets_wrong_statistics_through():
    """why the recipe changed.  At test_group_norm's own (2, 4096, 320) / 32 with its kind of data
    (every group of every image the same mean and variance) the neighbouring group's statistics
    and image 0's statistics for every image pass the whole-tensor 1e-2; with gn_moments' data
    both are orders of magnitude over the bound in their worst block."""
    B, S, C, G = 2, 4096, 320, 32
    x, g, b = ko.gn_inputs(B, S, C)
    y64 = ref.group_norm(x, G, g, b, 1e-5, False, dtype=F64)
    c = ko.GnCase(B, S, C, G, 0, ())
    x2, g2, b2, y2 = _gn_ref(c)
    for bug in ({"neighbour_stats": True}, {"image0_stats": True}):
        iid = ko.group_norm_model(x, G, g, b, 1e-5, False, **bug)
        own = ko.group_norm_model(x2, G, g2, b2, 1e-5, False, **bug)
        e_glob, e_blk, e_own = global_rel_err(iid, y64), block_rel_err(iid, y64, GN_BLOCK(c)), block_rel_err(own, y2, GN_BLOCK(c))
        print(f"{bug}: iid data whole tensor {e_glob:.2e}, worst block {e_blk:.2e}; own moments worst block {e_own:.2e}")
        assert e_glob < 1e-2 and e_own > 100 * BOUND["group_norm"]
    assert block_rel_err(ko.group_norm_model(x2, G, g2, b2, 1e-5, False), y2, GN_BLOCK(c)) < 0.5 * BOUND["group_norm"]


def test_channel_stats_bound_holds_for_the_kernels_chain_and_rejects_a_dropped_row():
    """channel_stats_kernel's own fp32 chain on the CPU stays inside the per-channel bound on every
    case; one row (the image's last) or the last chunk left out is orders of magnitude outside"""
    worst = 0.0
    for c in {(c.B, c.S, c.C): c for c in ko.GN_GEOM_CASES}.values():
        x = ko.gn_case_inputs(c)[0]
        two = ko.gn_geometry_model(c.B, c.S, c.C)["two_pass"]
        ok = ko.channel_stats_excess(ops.stats_to_float(ko.channel_stats_model(x, two)), x, two)
        row = ko.channel_stats_excess(ops.stats_to_float(ko.channel_stats_model(x, two, drop_row=c.S - 1)), x, two)
        print(f"{c.id}: chain at {ok:.3f} of the bound, a dropped row at {row:.0f}")
        worst = max(worst, ok)
        assert ok <= 1.0 and row > 100, (c.id, ok, row)
        if ko._cdiv(c.S, two["rows_per_chunk"]) > 1:
            rows = (ko._cdiv(c.S, two["rows_per_chunk"]) - 1) * two["rows_per_chunk"]
            short = ko.gn_sums64(x, rows)[..., :2]
            assert ko.channel_stats_excess(short, x, two) > 100, c.id
    print(f"channel_stats: the chain's worst statistic at {worst:.3f} of its bound")


def test_row_norm_cases_instantiate_every_vpl_and_t():
    geoms = {D: ko.ln_geometry_model(D) for D in ko.ROW_NORM_D}
    assert {g["VPL"] for g in geoms.values()} == set(range(1, 9))
    assert {g["T"] for g in geoms.values()} == {1, 2, 4, 8, 16, 32, 64}
    assert {320, 384, 768, 1024, 1280, 2048} <= set(ko.ROW_NORM_D) and max(ko.ROW_NORM_D) == ko.LN_MAX_D
    for D, g in geoms.items():
        rows = [r for r, d in ko.ROW_NORM_CASES if d == D]
        assert g["rows_per_block"] + 1 in rows and 1 in rows and g["T"] * g["VPL"] * 8 >= D
    assert (257, 8) in ko.ROW_NORM_CASES
    assert {(r, D) for r in (1, 5) for D in (8, 136, 4096)} <= set(ko.ROW_NORM_CASES)      # the cases before the table grew


def test_row_stats_floor():
    """the two-pass formula in fp32 against fp64 over the row cases: ROW_STATS_FLOOR is its worst
    row, rounded up to one digit, and the kernel's bound four times that"""
    worst = [0.0, 0.0]
    for rows, D in ko.ROW_NORM_CASES:
        x = ko.norm_inputs(rows, D)[0]
        e = ko.row_stats_err(*ko.row_stats32(x), x)
        worst = [max(w, v) for w, v in zip(worst, e)]
    print(f"row_stats in fp32: mean {worst[0]:.2e} of a deviation, rstd {worst[1]:.2e} relative")
    for w, f in zip(worst, ko.ROW_STATS_FLOOR):
        assert w <= f <= 3 * w, (worst, ko.ROW_STATS_FLOOR)
    assert ko.ROW_STATS_BOUND == tuple(4 * f for f in ko.ROW_STATS_FLOOR)
    FLOOR["row_stats mean"] = ("row_stats mean", worst[0])
    FLOOR["row_stats rstd"] = ("row_stats rstd", worst[1])


def test_layer_norm_that_reduces_two_rows_together_fails():
    n = 0
    for rows, D in ko.ROW_NORM_CASES:
        x, g, b = ko.norm_inputs(rows, D)
        for beta, rms in ((b, False), (None, False), (None, True)):
            y64 = ref.rms_norm(x, g, 1e-5, dtype=F64) if rms else ref.layer_norm(x, g, beta, 1e-5, dtype=F64)
            assert block_rel_err(ko.layer_norm_model(x, g, beta, rms=rms), y64, (1, None)) < 0.5 * BOUND["norm"]
            if rows > 1:
                e = block_rel_err(ko.layer_norm_model(x, g, beta, rms=rms, pair_rows=True), y64, (1, None))
                assert e > BOUND["norm"], (rows, D, rms, e)
                n += 1
        if rows > 1:        # row_stats: the pooled statistics of rows 0 and 1 for both
            xd = x.to(F64)[:2].reshape(1, -1)
            mean = xd.sum(-1) / D
            ms = ((xd - mean) ** 2).sum(-1) / D
            m, r = ko.row_stats64(x)
            m[:2], r[:2] = mean, (ms + 1e-5).rsqrt()
            e = ko.row_stats_err(m, r, x)
            assert e[0] > 1e3 * ko.ROW_STATS_BOUND[0] and e[1] > 1e3 * ko.ROW_STATS_BOUND[1], (rows, D, e)
    assert n >= 100


def test_glue_instruments():
    x = ko.all_bf16()
    assert x.numel() == 65282 and torch.isinf(x[-2:].float()).all() and x[:-2].unique().numel() == 65279   # (-0.0 == 0.0)
    o = ko.bf16_ordinal(torch.tensor([-0.0, 0.0, 1.0, 1.0078125, -1.0, -1.0078125], dtype=BF16))
    assert o.tolist()[:2] == [0, 0] and o[3] - o[2] == 1 and o[5] - o[4] == -1
    assert float(ko.silu64(torch.tensor([-0.0], dtype=BF16))[0]) == 0.0


def test_floor_table():
    """prints the table of kernel_oracle.py's docstring (run the whole file with -s)"""
    if not FLOOR:
        pytest.skip("run together with the ideal-kernel tests")
    for row in sorted(FLOOR):
        fam, worst = FLOOR[row]
        print(f"{row:16s} bound {BOUND[fam]:.3g}  ideal kernel's worst block {worst:.2e}")
        assert worst < 0.5 * BOUND[fam]
