"""Numerics of every HIP kernel against the plain-PyTorch fp32 reference of the same op
(``cassmantle_amd.ops.reference``), on the GPU.  Inputs are asymmetric random data so a
transposed MFMA layout or swapped index cannot pass (cdna_hip_programming.md §3)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cassmantle_amd import ops  # noqa: E402
from cassmantle_amd.ops import reference as ref  # noqa: E402

DEV = "cuda"


def rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def rnd(*shape, scale=1.0, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    from cassmantle_amd.ops._ext import ext_available, ext_error
    assert ext_available(), ext_error()
    ops.set_mode("hip")


@pytest.mark.parametrize("M,N,K", [(257, 320, 320), (100, 64, 96), (4096, 640, 1280), (77, 768, 768), (5, 1280, 320)])
@pytest.mark.parametrize("act", [None, "gelu", "silu", "quick_gelu"])
def test_gemm(M, N, K, act):
    x = rnd(M, K, seed=1)
    w = rnd(N, K, scale=K ** -0.5, seed=2)
    b = rnd(N, scale=0.1, seed=3)
    r = rnd(M, N, seed=4)
    out = ops.linear(x, w, b, residual=r, act=act)
    exp = ref.linear(x, w, b, residual=r, act=act)
    assert rel_err(out, exp) < 1e-2


@pytest.mark.parametrize("M,N,K", [(300, 320, 320), (4096, 1280, 320), (33, 64, 64)])
def test_gemm_geglu(M, N, K):
    x = rnd(M, K, seed=5)
    w = rnd(2 * N, K, scale=K ** -0.5, seed=6)
    b = rnd(2 * N, scale=0.1, seed=7)
    out = ops.linear(x, w, b, act="geglu")
    exp = ref.linear(x, w, b, act="geglu")
    assert rel_err(out, exp) < 1e-2


def test_gemm_small_k():
    # K % 8 != 0 -> SIMT path (post_quant_conv 4->4)
    x = rnd(1000, 4, seed=8)
    w = rnd(4, 4, seed=9)
    assert rel_err(ops.linear(x, w), ref.linear(x, w)) < 1e-2


def test_bmm_nt_f32():
    from cassmantle_amd.ops._ext import ext
    a = rnd(2, 300, 512, seed=10)
    b = rnd(2, 200, 512, seed=11)
    out = torch.empty(2, 300, 200, device=DEV, dtype=torch.float32)
    ext().bmm_nt(a, b, out, 0.5)
    exp = 0.5 * torch.matmul(a.float(), b.float().transpose(1, 2))
    assert rel_err(out, exp) < 1e-3


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,up", [
    (2, 17, 13, 64, 128, 1, False),
    (2, 16, 16, 320, 320, 2, False),
    (1, 8, 8, 128, 64, 1, True),
    (2, 9, 11, 32, 64, 1, False),     # Cin % 64 != 0 general path
    (1, 12, 12, 4, 64, 1, False),     # conv_in (SIMT)
    (1, 12, 12, 128, 3, 1, False),    # VAE conv_out (SIMT)
])
def test_conv(B, H, W, Cin, Cout, stride, up):
    x = rnd(B, H, W, Cin, seed=12)
    w = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=13)
    b = rnd(Cout, scale=0.1, seed=14)
    out = ops.conv2d(x, w, b, stride=stride, padding=1, upsample=up)
    exp = ref.conv2d(x, w, b, stride=stride, padding=1, upsample=up)
    assert out.shape == exp.shape
    assert rel_err(out, exp) < 1e-2


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 8, 8, 128, 64), (8, 16, 16, 1280, 1280), (1, 32, 32, 256, 256),
                                          (2, 6, 10, 64, 96), (4, 64, 64, 512, 512)])
def test_conv_upsample_as_parity_2x2_convs(B, H, W, Cin, Cout):
    """nearest-2x upsample + 3x3 conv computed as four parity-class 2x2 convs on the low-res
    input (folded weights, interleaved output) vs the upsampled 3x3 conv reference, with every
    epilogue input (bias, per-image bias, residual, GroupNorm statistics)."""
    x = rnd(B, H, W, Cin, seed=80)
    w = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=81)
    b = rnd(Cout, scale=0.1, seed=82)
    cb = rnd(B, Cout, scale=0.1, seed=83)
    res = rnd(B, 2 * H, 2 * W, Cout, seed=84)
    st = ops.new_stats(B, Cout, DEV)
    out = ops.conv2d_up2(x, w, None, b, residual=res, chan_bias=cb, stats=st)
    exp = ref.conv2d(x, w, b, 1, 1, res, True, cb)
    assert out.shape == exp.shape and rel_err(out, exp) < 1e-2
    exp_st = ops.new_stats(B, Cout, DEV)
    ops.channel_stats_ref(out, exp_st)
    assert rel_err(ops.stats_to_float(st), ops.stats_to_float(exp_st)) < 1e-4


@pytest.mark.parametrize("cfg,split", [(1, 2), (1, 8), (0, 5), (8, 4)])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(8, 8, 8, 1280, 1280), (2, 6, 10, 64, 96)])
def test_conv_upsample_parity_split_k(B, H, W, Cin, Cout, cfg, split, force_cfg):
    """split-K on the batched (4 parity classes) upsampling conv: fp32 slabs [parity][split], the
    reduce pass applies every epilogue input and the GroupNorm statistics per parity class"""
    x = rnd(B, H, W, Cin, seed=85)
    w = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=86)
    b = rnd(Cout, scale=0.1, seed=87)
    cb = rnd(B, Cout, scale=0.1, seed=88)
    res = rnd(B, 2 * H, 2 * W, Cout, seed=89)
    st = ops.new_stats(B, Cout, DEV)
    force_cfg(cfg, split)
    out = ops.conv2d_up2(x, w, None, b, residual=res, chan_bias=cb, stats=st)
    exp = ref.conv2d(x, w, b, 1, 1, res, True, cb)
    assert out.shape == exp.shape and rel_err(out, exp) < 1e-2
    exp_st = ops.new_stats(B, Cout, DEV)
    ops.channel_stats_ref(out, exp_st)
    assert rel_err(ops.stats_to_float(st), ops.stats_to_float(exp_st)) < 1e-4
    out2 = ops.conv2d_up2(x, w, None, b)
    assert rel_err(out2, ref.conv2d(x, w, b, 1, 1, None, True, None)) < 1e-2


def test_conv_epilogue_fusions():
    B, H, W, C = 2, 16, 16, 64
    x = rnd(B, H, W, C, seed=15)
    w = rnd(C, 3, 3, C, scale=(9 * C) ** -0.5, seed=16)
    cb = rnd(B, C, seed=17)
    res = rnd(B, H, W, C, seed=18)
    out = ops.conv2d(x, w, None, residual=res, chan_bias=cb)
    exp = ref.conv2d(x, w, None, residual=res, chan_bias=cb)
    assert rel_err(out, exp) < 1e-2


@pytest.mark.parametrize("shape,G,silu,eps", [
    ((2, 8, 8, 320), 32, True, 1e-5),
    ((1, 64, 64, 128), 32, False, 1e-6),
    ((2, 8, 8, 2560), 32, True, 1e-5),
    ((3, 5, 7, 64), 8, True, 1e-5),
    ((2, 4096, 320), 32, False, 1e-6),
    ((1, 128, 128, 128), 32, True, 1e-6),      # VAE-like: Cg = 4, many chunks
    ((8, 8, 8, 1920), 32, True, 1e-5),        # up-block concat width, Cg = 60
    ((8, 64, 64, 640), 32, True, 1e-5),       # Cg = 20 straddles the 8-channel vectors
])
def test_group_norm(shape, G, silu, eps):
    x = rnd(*shape, seed=19) + 0.5
    C = shape[-1]
    g = rnd(C, seed=20) * 0.5 + 1
    b = rnd(C, seed=21) * 0.1
    out = ops.group_norm(x, G, g, b, eps, silu)
    exp = ref.group_norm(x, G, g, b, eps, silu)
    assert rel_err(out, exp) < 1e-2


@pytest.mark.parametrize("kind,B,H,Cin,Cout", [
    ("conv", 2, 16, 64, 128),       # single-image tiles
    ("conv", 8, 8, 128, 320),       # 64-pixel images: tiles straddle images (per-thread flush)
    ("conv", 2, 8, 1280, 1280),     # split-K grid: statistics in the reduce pass
    ("conv", 8, 16, 1280, 1280),    # UNet 16x16 level (split-K)
    ("conv", 8, 8, 1280, 1280),     # UNet 8x8 level (split-K, 64-pixel images)
    ("conv", 4, 6, 640, 640),       # 36-pixel images: reduce blocks straddle images
    ("linear", 2, 32, 320, 320),
    ("linear", 1, 2, 64, 96),       # 4 rows: GEMV path + separate statistics pass
])
def test_epilogue_group_norm_statistics(kind, B, H, Cin, Cout):
    """GEMM/conv epilogue statistics (sum, sum of squares per image and channel) feeding the
    apply-only GroupNorm must equal the plain two-pass GroupNorm of the same tensor."""
    x = rnd(B, H, H, Cin, seed=50) + 0.25
    st = ops.new_stats(B, Cout, DEV)
    if kind == "conv":
        w = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=51)
        y = ops.conv2d(x, w, rnd(Cout, scale=0.3, seed=52), stats=st)
    else:
        w = rnd(Cout, Cin, scale=Cin ** -0.5, seed=51)
        y = ops.linear(x, w, rnd(Cout, scale=0.3, seed=52), residual=rnd(B, H, H, Cout, seed=53), stats=st)
    exp_st = torch.zeros_like(st)
    ops.channel_stats_ref(y, exp_st)
    assert rel_err(ops.stats_to_float(st), ops.stats_to_float(exp_st)) < 1e-4
    G = 32 if Cout % 32 == 0 else 4
    g = rnd(Cout, seed=54) * 0.5 + 1
    b = rnd(Cout, seed=55) * 0.1
    out = ops.group_norm(y, G, g, b, 1e-5, True, stats=st)
    assert rel_err(out, ref.group_norm(y, G, g, b, 1e-5, True)) < 1e-2


def test_group_norm_statistics_of_a_concatenation():
    a = rnd(2, 16, 16, 640, seed=56) + 0.5
    s = rnd(2, 16, 16, 320, seed=57) - 0.25
    sa, sb = ops.new_stats(2, 640, DEV), ops.new_stats(2, 320, DEV)
    ops.channel_stats(a, sa)
    ops.channel_stats(s, sb)
    x = torch.cat([a, s], dim=-1)
    g = rnd(960, seed=58) * 0.5 + 1
    b = rnd(960, seed=59) * 0.1
    out = ops.group_norm(x, 32, g, b, 1e-5, True, stats=sa, stats2=sb)
    assert rel_err(out, ref.group_norm(x, 32, g, b, 1e-5, True)) < 1e-2


@pytest.mark.parametrize("B,H,Ca,Cb,N", [(8, 16, 1280, 640, 640), (2, 32, 640, 320, 320), (3, 8, 64, 192, 96),
                                         (2, 5, 320, 320, 320),
                                         # the SD up-block 8x8 concatenation 1280|1280 (the two vectors
                                         # of a thread come from different tensors), and a short last
                                         # block (clamped-row loads) at that width
                                         (8, 8, 1280, 1280, 1280), (3, 5, 1280, 1280, 1280)])
def test_concat_free_gemm_and_group_norm(B, H, Ca, Cb, N):
    """UNet up-block [h | skip] consumers read the two tensors directly: the 1x1 shortcut GEMM
    stages k-tiles from both, the GroupNorm normalises both into one output."""
    a = rnd(B, H, H, Ca, seed=60) + 0.3
    s = rnd(B, H, H, Cb, seed=61) - 0.2
    x = torch.cat([a, s], dim=-1)
    w = rnd(N, Ca + Cb, scale=(Ca + Cb) ** -0.5, seed=62)
    bias = rnd(N, scale=0.1, seed=63)
    st = ops.new_stats(B, N, DEV)
    out = ops.linear_cat(a, s, w, bias, stats=st)
    exp = ref.linear(x, w, bias)
    assert out.shape == exp.shape and rel_err(out, exp) < 1e-2
    exp_st = torch.zeros_like(st)
    ops.channel_stats_ref(out, exp_st)
    assert rel_err(ops.stats_to_float(st), ops.stats_to_float(exp_st)) < 1e-4
    sa, sb = ops.new_stats(B, Ca, DEV), ops.new_stats(B, Cb, DEV)
    ops.channel_stats(a, sa)
    ops.channel_stats(s, sb)
    g = rnd(Ca + Cb, seed=64) * 0.5 + 1
    be = rnd(Ca + Cb, seed=65) * 0.1
    G = 32 if (Ca + Cb) % 32 == 0 else 8
    y = ops.group_norm_cat(a, s, G, g, be, 1e-5, True, stats=sa, stats2=sb)
    assert rel_err(y, ref.group_norm(x, G, g, be, 1e-5, True)) < 1e-2


@pytest.mark.parametrize("rows,K,N,act,res", [(4096, 320, 960, None, False), (300, 640, 640, None, True),
                                             (2048, 1280, 1280, "geglu", False), (64, 1280, 1280, None, False),
                                             (4096, 320, 1280, "geglu", False)])
def test_layer_norm_folded_into_gemm(rows, K, N, act, res):
    """LN(x) @ W^T + b computed as rstd * (x @ (W*gamma)^T - mean * wsum) + (b + W.beta): row
    statistics pass + GEMM epilogue correction, vs the explicit LayerNorm -> GEMM reference (also
    through the split-K reduce pass for the 64-row shape)."""
    x = rnd(rows, K, seed=70) * 1.5 + 0.3
    g = rnd(K, seed=71) * 0.3 + 1
    be = rnd(K, seed=72) * 0.2
    Nw = 2 * N if act == "geglu" else N
    w = rnd(Nw, K, scale=K ** -0.5, seed=73)
    b = rnd(Nw, scale=0.1, seed=74)
    r = rnd(rows, N, seed=75) if res else None
    fold = ops.ln_fold(g, be, w, b)
    out = ops.ln_linear(x, g, be, 1e-5, w, b, residual=r, act=act, fold=fold)
    exp = ref.linear(ref.layer_norm(x, g, be, 1e-5), w, b, residual=r, act=act)
    assert rel_err(out, exp) < 1.5e-2


@pytest.mark.parametrize("cfg", [31, 33, 8])
def test_layer_norm_folded_into_producer_wave_gemm(cfg, force_cfg):
    """the level-3 projection / GEGLU shapes on the warp-specialised tiles (31, 33: 8 MFMA + 8
    producer waves) and the gated ping-pong tile (8: 8x1 waves): folded LayerNorm epilogue (row
    statistics + wsum correction) and bias; a gated call forced onto a deep-ring config takes the
    gated deep-ring tile (12)"""
    rows, K, N = 2048, 1280, 1280
    x = rnd(rows, K, seed=76) * 1.5 + 0.3
    g = rnd(K, seed=77) * 0.3 + 1
    be = rnd(K, seed=78) * 0.2
    for act in ("geglu", None):
        Nw = 2 * N if act == "geglu" else N
        w = rnd(Nw, K, scale=K ** -0.5, seed=79)
        b = rnd(Nw, scale=0.1, seed=80)
        fold = ops.ln_fold(g, be, w, b)
        force_cfg(cfg)
        out = ops.ln_linear(x, g, be, 1e-5, w, b, act=act, fold=fold)
        force_cfg(-1)
        exp = ref.linear(ref.layer_norm(x, g, be, 1e-5), w, b, act=act)
        assert rel_err(out, exp) < 1.5e-2, (cfg, act)


@pytest.mark.parametrize("rows,K,N,act,res", [(32768, 320, 960, None, False), (1000, 320, 320, None, True),
                                              (2000, 320, 1280, "geglu", False), (8192, 640, 1920, None, False),
                                              (333, 640, 2560, "geglu", True), (500, 640, 640, "silu", True)])
def test_layer_norm_stats_inside_areg_gemm(rows, K, N, act, res):
    """K = 320 / 640: the folded LayerNorm's row statistics come from the A rows resident in the
    A-in-registers kernel (no stats pass); the plan must be cfg 15 and the result the explicit
    LayerNorm -> GEMM reference"""
    from cassmantle_amd.ops._ext import ext
    x = rnd(rows, K, seed=76) * 1.5 + 0.3
    g = rnd(K, seed=77) * 0.3 + 1
    be = rnd(K, seed=78) * 0.2
    Nw = 2 * N if act == "geglu" else N
    w = rnd(Nw, K, scale=K ** -0.5, seed=79)
    b = rnd(Nw, scale=0.1, seed=80)
    r = rnd(rows, N, seed=81) if res else None
    fold = ops.ln_fold(g, be, w, b)
    out = ops.ln_linear(x, g, be, 1e-5, w, b, residual=r, act=act, fold=fold)
    assert tuple(ext().gemm_last_plan())[0] == 15
    exp = ref.linear(ref.layer_norm(x, g, be, 1e-5), w, b, residual=r, act=act)
    assert rel_err(out, exp) < 1.5e-2


@pytest.mark.parametrize("D,rows", [(320, 333), (384, 333), (768, 333), (1280, 333), (32, 333), (640, 1),
                                    (4096, 7), (136, 45)])
def test_layer_norm(D, rows):
    x = rnd(rows, D, seed=22) * 2 + 1
    g = rnd(D, seed=23) * 0.5 + 1
    b = rnd(D, seed=24) * 0.1
    assert rel_err(ops.layer_norm(x, g, b, 1e-5), ref.layer_norm(x, g, b, 1e-5)) < 1e-2


@pytest.mark.parametrize("B,Nq,Nk,H,d,causal", [
    (2, 300, 300, 8, 40, False),
    (2, 1024, 77, 8, 80, False),
    (2, 256, 256, 8, 160, False),
    (2, 77, 77, 12, 64, True),
    (3, 16, 16, 12, 32, False),
    (1, 64, 64, 8, 160, False),
    (1, 4096, 4096, 8, 40, False),
    (2, 4096, 77, 8, 40, False),                 # level-1 cross-attention (ragged last key tile)
    (3, 200, 130, 2, 40, False),
])
def test_attention(B, Nq, Nk, H, d, causal):
    q = rnd(B, Nq, H, d, seed=25)
    k = rnd(B, Nk, H, d, seed=26)
    v = rnd(B, Nk, H, d, seed=27)
    out = ops.attention(q, k, v, causal=causal)
    exp = ref.attention(q, k, v, causal=causal)
    assert rel_err(out, exp) < 2e-2


@pytest.mark.parametrize("B,Nq,Nk,H,d,lens", [
    (8, 256, 256, 8, 160, None),                  # SD-1.5 level 3 at the bench batch
    (2, 256, 256, 8, 160, None),                  # level 3 at batch 1 (64 two-wave blocks)
    (2, 1024, 1024, 8, 80, None),                 # level 2 at batch 1
    (8, 256, 77, 8, 160, None),                   # level-3 cross-attention
    (1, 300, 1000, 2, 96, None),                  # 16 ragged key tiles
    (3, 100, 300, 2, 128, [300, 70, 1]),          # kv_lens down to one key
])
def test_attention_short_grids(B, Nq, Nk, H, d, lens):
    """the generic kernel on the short grids of batch 1 / level 3 (2-wave blocks) vs the fp32
    reference.  (A key split over blocks with an fp32 partial merge was built for these grids in
    round 5, passed this test, and measured 1.9x slower on the level-3 shape -- 35.0 vs 18.0 us --
    and +8 ms per bench step: removed, profiles/r5_attn_key_split_negative.txt)"""
    q = rnd(B, Nq, H, d, seed=71)
    k = rnd(B, Nk, H, d, seed=72)
    v = rnd(B, Nk, H, d, seed=73)
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens else None
    out = ops.attention(q, k, v, kv_lens=kl)
    exp = ref.attention(q, k, v, kv_lens=kl)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out, exp) < 2e-2


def test_attention_strided_qkv_and_kv_lens():
    B, N, H, d = 3, 20, 12, 32
    qkv = rnd(B, N, 3, H, d, seed=28)
    lens = torch.tensor([20, 7, 13], dtype=torch.int32, device=DEV)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    out = ops.attention(q, k, v, kv_lens=lens)
    exp = ref.attention(q, k, v, kv_lens=lens)
    assert rel_err(out, exp) < 2e-2


def test_attention_large_head_dim_gemm_fallback():
    """head dims above 160 other than 512 keep the GEMM + row-softmax + GEMM fallback"""
    B, N, d = 1, 512, 256
    qkv = rnd(B, N, 3, 1, d, seed=29)
    out = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    exp = ref.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    assert rel_err(out, exp) < 2e-2


@pytest.mark.parametrize("B,Nq,Nk,H,causal,lens,qs", [
    (1, 1024, 1024, 1, False, None, 1.0),        # 8 key splits + merge
    (2, 300, 300, 1, False, None, 3.0),          # ragged tiles, 2 splits, peaked scores
    (3, 200, 130, 1, False, [130, 65, 3], 1.0),  # kv_lens
    (1, 256, 256, 2, True, None, 1.0),           # causal, 2 heads
    (2, 4096, 4096, 1, False, None, 2.0),        # SD-1.5 VAE mid-block shape (2 images)
    (1, 2048, 2048, 1, False, None, 1.0),
])
def test_attention_d512_flash(B, Nq, Nk, H, causal, lens, qs):
    """attention_d512.hip (VAE mid-block, head dim 512): flash kernel with the head dim split over
    wave pairs and key-split partials merged for short grids, vs the fp32 reference; K/V read
    through the fused-QKV strides the VAE uses"""
    d = 512
    kv = rnd(B, Nk, 2, H, d, seed=31)
    q = rnd(B, Nq, H, d, seed=30) * qs
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens else None
    out = ops.attention(q, kv[:, :, 0], kv[:, :, 1], causal=causal, kv_lens=kl)
    exp = ref.attention(q, kv[:, :, 0], kv[:, :, 1], causal=causal, kv_lens=kl)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out, exp) < 2e-2


def test_attention_d512_vae_layout():
    B, N, d = 2, 1024, 512
    qkv = rnd(B, N, 3, 1, d, seed=32)
    out = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    exp = ref.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    assert rel_err(out, exp) < 2e-2


@pytest.mark.parametrize("B,Nq,Nk,H,causal,lens", [(2, 4096, 4096, 10, False, None), (2, 1024, 1024, 20, False, None),
                                                   (2, 1024, 77, 10, False, None), (3, 300, 300, 4, True, None),
                                                   (3, 200, 130, 2, False, [130, 65, 3])])
def test_attention_fp8(B, Nq, Nk, H, causal, lens):
    """OCP-e4m3 attention (BASELINE config 4, SDXL head dim 64): fp8 quantisation of Q/K/V/P
    rounds every element to 3 mantissa bits (<= 3.1% each); with the deliberately peaked scores
    (q x2) the output error measured 8.8% vs 0.4% for bf16, so the bound is 12%."""
    d = 64
    q = rnd(B, Nq, H, d, scale=2.0, seed=41)
    k = rnd(B, Nk, H, d, seed=42)
    v = rnd(B, Nk, H, d, seed=43)
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens else None
    exp = ref.attention(q, k, v, causal=causal, kv_lens=kl)
    out8 = ops.attention(q, k, v, causal=causal, kv_lens=kl, fp8="force")
    out16 = ops.attention(q, k, v, causal=causal, kv_lens=kl)
    e8, e16 = rel_err(out8, exp), rel_err(out16, exp)
    assert e8 < 0.12, (e8, e16)
    assert torch.isfinite(out8.float()).all()


@pytest.mark.parametrize("variant", ["8x1", "4x1", "4x2", "2x2", "2x4", "1x4"])
@pytest.mark.parametrize("B,Nq,Nk,H,causal,lens", [(2, 1024, 1024, 20, False, None), (3, 300, 300, 4, True, None),
                                                   (3, 200, 130, 2, False, [130, 65, 3]),
                                                   (2, 256, 77, 4, False, [77, 5])])
def test_attention_fp8_block_variants(variant, B, Nq, Nk, H, causal, lens):
    """every fp8 block shape (NQ query groups x NS key splits merged through LDS) against the
    fp32 reference, including splits that get no tile (short / ragged / causal key ranges)"""
    d = 64
    q = rnd(B, Nq, H, d, scale=2.0, seed=46)
    k = rnd(B, Nk, H, d, seed=47)
    v = rnd(B, Nk, H, d, seed=48)
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens else None
    exp = ref.attention(q, k, v, causal=causal, kv_lens=kl)
    ops.set_fp8_attention_variant(variant)
    try:
        out = ops.attention(q, k, v, causal=causal, kv_lens=kl, fp8="force")
    finally:
        ops.set_fp8_attention_variant(None)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out, exp) < 0.12, rel_err(out, exp)


@pytest.mark.parametrize("B,Nq,Nk,H,lens", [(2, 4096, 77, 10, None), (2, 1024, 77, 20, None),
                                          (3, 200, 130, 2, [130, 65, 3])])
def test_attention_fp8_prepacked_kv(B, Nq, Nk, H, lens):
    """cross-attention fp8: K/V packed ONCE (ops.pack_kv_fp8, as UNet.set_context does) and
    reused; must equal the per-call-pack result bit for bit, through fused-KV strides"""
    d = 64
    q = rnd(B, Nq, H, d, scale=2.0, seed=44)
    kv = rnd(B, Nk, 2, H, d, seed=45)
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens else None
    k, v = kv[:, :, 0], kv[:, :, 1]
    kv8 = ops.pack_kv_fp8(k, v, kl)
    out_pre = ops.attention(q, k, v, kv_lens=kl, fp8=True, kv8=kv8)
    out_call = ops.attention(q, k, v, kv_lens=kl, fp8="force")
    assert torch.equal(out_pre, out_call)
    assert rel_err(out_pre, ref.attention(q, k, v, kv_lens=kl)) < 0.12
    kv8b = ops.pack_kv_fp8(k, v, kl, out=kv8)            # refill in place (captured graphs)
    assert kv8b.data_ptr() == kv8.data_ptr()


def test_unet_set_context_fp8_packs_cross_kv():
    import dataclasses
    from cassmantle_amd.models.unet import SDXL_UNET, UNet
    cfg = dataclasses.replace(SDXL_UNET, transformer_depth=(0, 1, 1), mid_transformer_depth=1, sample_size=16)
    m = UNet(cfg, seed=6).cuda()
    ctx = rnd(2, 77, 2048, scale=0.5, seed=46)
    m.set_context(ctx, fp8=True)
    ca = m.cross_attns()
    assert ca and all(c._kv8 is not None for c in ca)
    ptrs = [c._kv8.data_ptr() for c in ca]
    m.set_context(rnd(2, 77, 2048, scale=0.5, seed=47), fp8=True)
    assert [c._kv8.data_ptr() for c in ca] == ptrs     # refilled in place
    m.set_context(ctx, fp8=False)
    assert all(c._kv8 is None for c in ca)


def test_attention_softmax_spike():
    # force the online-softmax rescale: one key dominates late in the sequence
    B, N, H, d = 1, 512, 2, 64
    q = rnd(B, N, H, d, seed=30)
    k = rnd(B, N, H, d, seed=31)
    k[:, 400] = q[:, 5] * 4
    v = rnd(B, N, H, d, seed=32)
    assert rel_err(ops.attention(q, k, v), ref.attention(q, k, v)) < 2e-2


def test_scorer_kernels():
    t = rnd(1000, 300, dtype=torch.float32, seed=33)
    ia = torch.tensor([0, 5, -1, 999], dtype=torch.int32, device=DEV)
    ib = torch.tensor([1, 5, 3, 0], dtype=torch.int32, device=DEV)
    out = ops.gather_cosine(t, ia, ib)
    exp = ref.gather_cosine(t, ia, ib)
    assert torch.isnan(out[2]) and torch.isnan(exp[2])
    m = ~torch.isnan(exp)
    assert torch.allclose(out[m], exp[m], atol=1e-5)
    tb = t.to(torch.bfloat16)
    out = ops.gather_cosine(tb, ia, ib)
    exp = ref.gather_cosine(tb, ia, ib)
    assert torch.allclose(out[m], exp[m], atol=1e-3)
    a, b = rnd(64, 384, dtype=torch.float32, seed=34), rnd(64, 384, dtype=torch.float32, seed=35)
    assert torch.allclose(ops.pair_cosine(a, b), ref.pair_cosine(a, b), atol=1e-5)
    v, i = ops.cosine_topk(t, t[7], 5)
    ve, ie = ref.cosine_topk(t, t[7], 5)
    assert i[0].item() == 7 and torch.equal(i, ie)
    h = rnd(4, 16, 384, seed=36)
    lens = torch.tensor([16, 3, 9, 1], dtype=torch.int32, device=DEV)
    assert torch.allclose(ops.mean_pool_l2(h, lens), ref.mean_pool_l2(h, lens), atol=1e-4)


def test_image_kernels():
    img = (torch.rand(64, 48, 3, generator=torch.Generator().manual_seed(37)) * 255).to(torch.uint8).to(DEV)
    out = ops.gaussian_blur(img, 3.0)
    exp = ref.gaussian_blur(img, 3.0)
    assert (out.int() - exp.int()).abs().max().item() <= 1
    x = rnd(2, 16, 16, 3, seed=38) * 1.5
    u = ops.vae_postprocess(x)
    ue = ((x.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)
    assert (u.int() - ue.int()).abs().max().item() <= 1


def test_timestep_embedding():
    t = torch.tensor([981.0, 1.0, 500.0], device=DEV)
    assert torch.allclose(ops.timestep_embedding(t, 320), ref.timestep_embedding(t, 320), atol=2e-3)


@pytest.mark.parametrize("sched", ["pndm", "ddim", "euler"])
def test_latent_step_matches_reference(sched):
    from cassmantle_amd.models.schedulers import latent_step_reference, make_plan
    plan = make_plan(sched, 10, 7.5)
    B, n = 2, 8 * 8 * 4
    g = torch.Generator().manual_seed(39)
    x0 = torch.randn(B, 8, 8, 4, generator=g)
    state = []
    for dev in ("cpu", DEV):
        x = x0.clone().to(dev)
        hist = torch.zeros(4, B, 8, 8, 4, device=dev)
        xs = torch.zeros_like(x)
        unet_in = torch.zeros(2 * B, 8, 8, 4, device=dev, dtype=torch.bfloat16)
        coef = torch.from_numpy(plan.table).to(dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        for i in range(plan.evals):
            eps = torch.randn(2 * B, 8, 8, 4, generator=torch.Generator().manual_seed(100 + i)).to(torch.bfloat16).to(dev)
            if dev == "cpu":
                latent_step_reference(eps, x, hist, xs, coef, step, unet_in, True)
                step += 1
            else:
                ops.latent_step(eps, x, hist, xs, coef, step, unet_in, True)
                ops.advance_step(step)
        state.append(x.cpu())
    assert rel_err(state[1], state[0]) < 1e-4


# ---------------------------------------------------------------- ping-pong 8-wave GEMM (gemm_pp.h)
PP_CFGS = [7, 8, 9, 10, 12, 13, 14, 16, 20, 21, 22, 26, 27, 31, 32, 33]   # ping-pong (7-10, 20-22), deep-ring (12-14, 16, 8-wave 26/27, producer-wave 31-33)


@pytest.fixture
def force_cfg():
    from cassmantle_amd.ops._ext import ext
    yield lambda c, s=0: ext().gemm_set_override(c, s)
    ext().gemm_set_override(-1, 0)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6])
def test_gemm_static_tiles_forced(cfg, force_cfg):
    """every static tile forced once (the cost model alone never picks 5 / 6); the N <= 16 tile
    takes only such shapes, so it gets N = 16.  Partial M and N tiles, 2 k-tiles."""
    from cassmantle_amd.ops._ext import ext
    M, N, K = 300, (16 if cfg == 4 else 200), 128
    x = rnd(M, K, seed=141)
    w = rnd(N, K, scale=K ** -0.5, seed=142)
    b = rnd(N, scale=0.1, seed=143)
    r = rnd(M, N, seed=144)
    force_cfg(cfg, 1)
    out = ops.linear(x, w, b, residual=r, act="silu")
    assert tuple(ext().gemm_last_plan()) == (cfg, 1)
    assert rel_err(out, ref.linear(x, w, b, residual=r, act="silu")) < 1e-2


@pytest.mark.parametrize("cfg", PP_CFGS)
@pytest.mark.parametrize("M,N,K,split", [(1000, 320, 320, 1), (4096, 640, 1280, 1), (300, 1280, 2560, 4),
                                         (77, 768, 768, 1), (2048, 200, 640, 2)])
def test_gemm_pp_linear(cfg, M, N, K, split, force_cfg):
    """every ping-pong tile (partial M / N tiles, tails of 1..5 k-tiles, split-K slabs) with bias,
    residual and an activation vs the fp32 reference; asymmetric data catches layout swaps"""
    x = rnd(M, K, seed=101)
    w = rnd(N, K, scale=K ** -0.5, seed=102)
    b = rnd(N, scale=0.1, seed=103)
    r = rnd(M, N, seed=104)
    force_cfg(cfg, split)
    out = ops.linear(x, w, b, residual=r, act="silu")
    exp = ref.linear(x, w, b, residual=r, act="silu")
    assert rel_err(out, exp) < 1e-2


@pytest.mark.parametrize("cfg", PP_CFGS)
def test_gemm_pp_geglu_cat_stats(cfg, force_cfg):
    force_cfg(cfg)
    # gated (the planner maps forced config 8 to the 256x160 8x1-wave gated tile, every other
    # one to the 256x128 gated tile); N = 360 leaves a partial 80-output block
    for N_g, seed in ((640, 105), (360, 205)):
        x = rnd(700, 320, seed=seed)
        w = rnd(2 * N_g, 320, scale=320 ** -0.5, seed=seed + 1)
        b = rnd(2 * N_g, scale=0.1, seed=seed + 2)
        assert rel_err(ops.linear(x, w, b, act="geglu"), ref.linear(x, w, b, act="geglu")) < 1e-2
    # two-source A (channel concatenation) with fused GroupNorm statistics
    B, HW, Ca, Cb, N = 2, 300, 640, 320, 320
    a = rnd(B, HW, Ca, seed=108)
    s2 = rnd(B, HW, Cb, seed=109)
    w2 = rnd(N, Ca + Cb, scale=(Ca + Cb) ** -0.5, seed=110)
    b2 = rnd(N, scale=0.1, seed=111)
    st = ops.new_stats(B, N, DEV)
    out = ops.linear_cat(a, s2, w2, b2, stats=st)
    exp = ref.linear(torch.cat([a, s2], -1), w2, b2)
    assert rel_err(out, exp) < 1e-2
    exp_st = ops.new_stats(B, N, DEV)
    ops.channel_stats_ref(out, exp_st)
    assert rel_err(ops.stats_to_float(st), ops.stats_to_float(exp_st)) < 1e-4


# ---------------------------------------------------------------- A-in-registers short-K GEMM (cfg 15)
@pytest.mark.parametrize("M,N,K", [(1000, 320, 320), (4096, 960, 320), (333, 640, 640), (4096, 1280, 640),
                                   (77, 64, 320), (8192, 320, 640)])
@pytest.mark.parametrize("act", ["none", "silu"])
def test_gemm_areg_linear(M, N, K, act, force_cfg):
    """gemm_areg.hip: partial last row block, N not a multiple of the chunk-group split, bias +
    activation + residual, vs the fp32 reference; the planner must report cfg 15 actually ran"""
    from cassmantle_amd.ops._ext import ext
    x = rnd(M, K, seed=131)
    w = rnd(N, K, scale=K ** -0.5, seed=132)
    b = rnd(N, scale=0.1, seed=133)
    r = rnd(M, N, seed=134)
    force_cfg(15)
    out = ops.linear(x, w, b, residual=r, act=act)
    assert tuple(ext().gemm_last_plan())[0] == 15
    assert rel_err(out, ref.linear(x, w, b, residual=r, act=act)) < 1e-2
    out = ops.linear(x, w)
    assert rel_err(out, ref.linear(x, w)) < 1e-2


@pytest.mark.parametrize("M,N,K", [(2000, 1280, 320), (1000, 2560, 640), (130, 32, 320)])
def test_gemm_areg_geglu(M, N, K, force_cfg):
    from cassmantle_amd.ops._ext import ext
    x = rnd(M, K, seed=135)
    w = rnd(2 * N, K, scale=K ** -0.5, seed=136)
    b = rnd(2 * N, scale=0.1, seed=137)
    force_cfg(15)
    out = ops.linear(x, w, b, act="geglu")
    assert tuple(ext().gemm_last_plan())[0] == 15
    assert rel_err(out, ref.linear(x, w, b, act="geglu")) < 1e-2


def test_gemm_areg_stats(force_cfg):
    """fused GroupNorm statistics (per image: rows of one image are a multiple of 32)"""
    from cassmantle_amd.ops._ext import ext
    B, HW, K, N = 3, 320, 640, 640
    x = rnd(B, HW, K, seed=138)
    w = rnd(N, K, scale=K ** -0.5, seed=139)
    b = rnd(N, scale=0.1, seed=140)
    st = ops.new_stats(B, N, DEV)
    force_cfg(15)
    out = ops.linear(x, w, b, stats=st)
    assert tuple(ext().gemm_last_plan())[0] == 15
    assert rel_err(out, ref.linear(x, w, b)) < 1e-2
    exp_st = ops.new_stats(B, N, DEV)
    ops.channel_stats_ref(out, exp_st)
    assert rel_err(ops.stats_to_float(st), ops.stats_to_float(exp_st)) < 1e-4


@pytest.mark.parametrize("cfg", PP_CFGS)
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(2, 17, 13, 64, 128, 1), (2, 16, 16, 320, 320, 2),
                                                   (3, 12, 12, 128, 320, 1)])
def test_conv_pp(cfg, B, H, W, Cin, Cout, stride, force_cfg):
    x = rnd(B, H, W, Cin, seed=112)
    w = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=113)
    b = rnd(Cout, scale=0.1, seed=114)
    cb = rnd(B, Cout, scale=0.1, seed=115)
    Ho = (H - 1) // stride + 1
    Wo = (W - 1) // stride + 1
    res = rnd(B, Ho, Wo, Cout, seed=116)
    st = ops.new_stats(B, Cout, DEV)
    force_cfg(cfg)
    out = ops.conv2d(x, w, b, stride=stride, padding=1, residual=res, chan_bias=cb, stats=st)
    exp = ref.conv2d(x, w, b, stride, 1, res, False, cb)
    assert out.shape == exp.shape and rel_err(out, exp) < 1e-2
    exp_st = ops.new_stats(B, Cout, DEV)
    ops.channel_stats_ref(out, exp_st)
    assert rel_err(ops.stats_to_float(st), ops.stats_to_float(exp_st)) < 1e-4


@pytest.mark.parametrize("cfg", PP_CFGS)
def test_conv_up2_pp(cfg, force_cfg):
    B, H, W, Cin, Cout = 2, 8, 12, 128, 192
    x = rnd(B, H, W, Cin, seed=117)
    w = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=118)
    b = rnd(Cout, scale=0.1, seed=119)
    force_cfg(cfg)
    out = ops.conv2d_up2(x, w, None, b)
    exp = ref.conv2d(x, w, b, 1, 1, None, True, None)
    assert out.shape == exp.shape and rel_err(out, exp) < 1e-2


@pytest.mark.parametrize("H,W,C,sigma", [(1024, 1024, 3, 15.0), (97, 130, 3, 0.6), (200, 75, 4, 9.3),
                                         (64, 64, 1, 16.5), (50, 40, 3, 20.0)])
def test_gaussian_blur_tiled(H, W, C, sigma):
    """LDS-tiled blur (radius <= 48) and the two-pass fallback (sigma 20 -> radius 60) vs the fp32
    separable reference with edge clamping; partial edge tiles included."""
    img = (torch.rand(H, W, C, generator=torch.Generator().manual_seed(39)) * 255).to(torch.uint8).to(DEV)
    out = ops.gaussian_blur(img, sigma)
    exp = ref.gaussian_blur(img, sigma)
    assert (out.int() - exp.int()).abs().max().item() <= 1


def test_gpu_blur_fn_serves_blur_cache():
    """the serving blur (runtime.factory.build_blur_fn) feeding the per-bucket JPEG cache,
    prewarmed over every bucket of a 1024^2 image like a round boundary does"""
    import numpy as np
    from cassmantle_amd.config import Config
    from cassmantle_amd.game.imaging import BlurCache, encode_jpeg, decode_jpeg, blur_pil
    from cassmantle_amd.runtime.factory import build_blur_fn
    fn = build_blur_fn(Config(), "cuda")
    assert fn is not None
    rng = np.random.default_rng(0)
    img = (rng.random((1024, 1024, 3)) * 255).astype(np.uint8)
    g = fn(img, 7.5)
    c = blur_pil(img, 7.5)
    # PIL approximates the Gaussian with box blurs: close, not bit-equal
    assert np.abs(g.astype(np.int32) - c.astype(np.int32)).mean() < 2.0
    cache = BlurCache(blur_fn=fn, bucket=1.0)
    jpeg = encode_jpeg(img)
    assert cache.prewarm("v1", jpeg, 15.0) == 16
    assert cache.misses == 16 and decode_jpeg(cache.get("v1", jpeg, 3.2)).shape == (1024, 1024, 3)
    assert cache.hits >= 1


def test_latent_step_padded_input_and_row_select():
    """channel-padded UNet input (cstride 8: channels 4..7 stay zero) and the next step's
    time-conditioning rows copied by the same launch (clamped at the last row)"""
    from cassmantle_amd.models.schedulers import make_plan
    plan = make_plan("pndm", 6, 7.5)
    B = 2
    x = torch.randn(B, 8, 8, 4, generator=torch.Generator().manual_seed(41)).to(DEV)
    x4 = x.clone()
    hist, xs = torch.zeros(4, B, 8, 8, 4, device=DEV), torch.zeros(B, 8, 8, 4, device=DEV)
    hist4, xs4 = hist.clone(), xs.clone()
    u8 = torch.zeros(2 * B, 8, 8, 8, device=DEV, dtype=torch.bfloat16)
    u4 = torch.zeros(2 * B, 8, 8, 4, device=DEV, dtype=torch.bfloat16)
    coef = torch.from_numpy(plan.table).to(DEV)
    E = plan.evals
    tab0 = torch.randn(E, 2 * B, 320, generator=torch.Generator().manual_seed(42)).to(torch.bfloat16).to(DEV)
    tab1 = torch.randn(E, 2 * B, 1000, generator=torch.Generator().manual_seed(43)).to(torch.bfloat16).to(DEV)
    b0, b1 = tab0[0].clone(), tab1[0].clone()
    step, step4 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for i in range(E):
        eps = torch.randn(2 * B, 8, 8, 4, generator=torch.Generator().manual_seed(200 + i)).to(torch.bfloat16).to(DEV)
        ops.latent_step(eps, x, hist, xs, coef, step, u8, True, rows=[(tab0, b0), (tab1, b1)])
        ops.latent_step(eps, x4, hist4, xs4, coef, step4, u4, True)
        ops.advance_step(step)
        ops.advance_step(step4)
        nxt = min(i + 1, E - 1)
        assert torch.equal(b0, tab0[nxt]) and torch.equal(b1, tab1[nxt])
        assert torch.equal(u8[..., :4], u4) and not u8[..., 4:].any()
    assert torch.equal(x, x4)


@pytest.mark.parametrize("n,dtype", [(1, torch.int32), (7, torch.int64), (4099, torch.int64), (12345, torch.float32),
                                     (33, torch.bfloat16)])
def test_zero_fill_kernel(n, dtype):
    """ops.zero_ (HIP zero_kernel: 16-byte stores plus a byte tail) clears exactly the tensor and
    nothing past it (the StatsArena slab clear inside the captured step)."""
    big = torch.full((n + 64,), 7, device=DEV, dtype=dtype)
    t = big[:n]
    ops.zero_(t)
    torch.cuda.synchronize()
    assert torch.count_nonzero(big[:n]).item() == 0
    assert bool((big[n:] == 7).all())


def test_ln_gemm_bitwise_stable_under_concurrency():
    """The in-kernel-LayerNorm A-in-registers GEMM (K = 320, 2 blocks/CU) must give bit-identical
    results while a 4-wave GEMM runs on a second stream.  Before the fix, 16-row groups came out
    with different LayerNorm statistics in ~60 % of such runs (profiles/r2_lnk_concurrency_fix.txt,
    tools/dbg_conc_matrix.py)."""
    from cassmantle_amd.ops._ext import ext
    M, K, N = 8192, 320, 960
    x = (rnd(M, K, seed=301).float() * 2 + 0.5).to(torch.bfloat16)
    g = (torch.rand(K, generator=torch.Generator().manual_seed(302)) + 0.5).to(torch.bfloat16).to(DEV)
    b = rnd(K, scale=0.1, seed=303)
    w = rnd(N, K, scale=K ** -0.5, seed=304)
    wb = rnd(N, scale=0.1, seed=305)
    fold = ops.ln_fold(g, b, w, wb)
    ref_out = ops.ln_linear(x, g, b, 1e-5, w, fold=fold).clone()
    bgA, bgW = rnd(8192, 2048, seed=306), rnd(2048, 2048, scale=0.02, seed=307)
    s_bg = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s_bg):
        for _ in range(20):
            ext().gemm_set_override(0, 1)          # the 4-wave tile: the aggressor of the bisect
            ops.linear(bgA, bgW)
            ext().gemm_set_override(-1, 0)
    outs = [ops.ln_linear(x, g, b, 1e-5, w, fold=fold) for _ in range(30)]
    torch.cuda.synchronize()
    bad = sum(int(not torch.equal(y, ref_out)) for y in outs)
    assert bad == 0, f"{bad}/30 concurrent runs differ from the quiet result"


# ---------------------------------------------------------------- generation glue (round 3)
def test_gather_add_embedding_and_row_gather():
    table = rnd(1000, 64, seed=11)
    pos = rnd(77, 64, scale=0.1, seed=12)
    ids = torch.randint(0, 1000, (3, 77), generator=torch.Generator().manual_seed(1)).to(DEV)
    got = ops.gather_add(table, ids.int(), pos)
    exp = table[ids.long()] + pos[None]                    # bf16 add, as the eager model
    assert torch.equal(got, exp)
    rows = torch.tensor([5, 0, 999, 5], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.gather_add(table, rows), table[rows.long()])


@pytest.mark.parametrize("bdtype", [torch.bfloat16, torch.float32])
def test_concat_last(bdtype):
    a = rnd(6, 1280, seed=13)
    b = rnd(6, 1536, seed=14, dtype=bdtype)
    got = ops.concat_last(a, b)
    assert torch.equal(got, torch.cat([a, b.to(torch.bfloat16)], dim=-1))


def test_silu_inplace():
    x = rnd(12, 1280, scale=3.0, seed=15)
    exp = torch.nn.functional.silu(x.float())
    ops.silu_(x)
    assert rel_err(x, exp) < 1e-2


def test_timestep_embedding_bf16_out():
    t = torch.tensor([1.0, 500.0, 981.0], device=DEV)
    a = ops.timestep_embedding(t, 320)
    b = ops.timestep_embedding(t, 320, out_dtype=torch.bfloat16)
    assert b.dtype == torch.bfloat16 and torch.equal(b, a.to(torch.bfloat16))


@pytest.mark.parametrize("cfg", [True, False])
def test_latent_init_matches_reference(cfg):
    B, h, C8 = 2, 8, 8
    nb = 2 * B if cfg else B
    x0 = torch.randn(B, h, h, 4, generator=torch.Generator().manual_seed(3)).to(DEV)
    outs = []
    for mode in ("hip", "torch"):
        x = torch.full((B, h, h, 4), 7.0, device=DEV)
        xs = torch.full_like(x, 7.0)
        hist = torch.full((4, B, h, h, 4), 7.0, device=DEV)
        u = torch.zeros((nb, h, h, C8), device=DEV, dtype=torch.bfloat16)
        if mode == "hip":
            ops.latent_init(x0, 0.5, x, xs, hist, u, cfg)
        else:
            x.copy_(x0); xs.zero_(); hist.zero_()
            for k in range(2 if cfg else 1):
                u[k * B:(k + 1) * B, ..., :4] = (x0 * 0.5).to(torch.bfloat16)
        outs.append((x, xs, hist, u))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_finalize_latents_flag():
    x = torch.randn(2, 16, 16, 4, device=DEV)
    z = torch.empty_like(x, dtype=torch.bfloat16)
    f = torch.empty((1,), device=DEV, dtype=torch.uint8)
    ops.finalize_latents(x, z, f)
    assert torch.equal(z, x.to(torch.bfloat16)) and int(f.item()) == 1
    x[1, 7, 3, 2] = float("nan")
    ops.finalize_latents(x, z, f)
    assert int(f.item()) == 0
    x[1, 7, 3, 2] = float("inf")
    ops.finalize_latents(x, z, f)
    assert int(f.item()) == 0


def test_cu_masked_streams_run_kernels():
    """the scorer / generation CU reservation (runtime/cumask.py): both masked streams run HIP
    kernels correctly, and a captured graph replays on the masked generation stream"""
    from cassmantle_amd.runtime.cumask import reserved_streams, split_cus
    mine, rest = split_cus(256, 8)
    assert mine == list(range(8)) and len(rest) == 248 and not set(mine) & set(rest)
    assert reserved_streams(DEV, 8)[0] is None          # default: scorer keeps every CU
    s_score, s_gen = reserved_streams(DEV, 8, exclusive=True)
    x = rnd(512, 640, seed=16)
    w = rnd(640, 640, scale=640 ** -0.5, seed=17)
    exp = ops.linear(x, w)
    torch.cuda.synchronize()
    for s in (s_score, s_gen):
        with torch.cuda.stream(s):
            y = ops.linear(x, w)
        s.synchronize()
        assert torch.equal(y, exp)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s_gen):
        ops.linear(x, w)
        s_gen.synchronize()
        with torch.cuda.graph(g, stream=s_gen):
            y = ops.linear(x, w)
        g.replay()
    s_gen.synchronize()
    assert torch.equal(y, exp)


@pytest.mark.parametrize("n", [1, 15, 16, 4096 + 7])
def test_device_copy_kernel(n):
    src = torch.randint(0, 255, (n,), device=DEV, dtype=torch.uint8)
    dst = torch.zeros_like(src)
    ops.copy_(dst, src)
    assert torch.equal(dst, src)
    a = rnd(77, 768, seed=21)
    b = torch.empty_like(a)
    ops.copy_(b, a)
    assert torch.equal(a, b)


@pytest.mark.parametrize("N,C,split", [(1024, 1280, 0), (1024, 1280, 2), (4096, 640, 0), (256, 640, 0)])
def test_qkv_epilogue_emits_fp8_kv(N, C, split):
    """SDXL fp8 self-attention: the LayerNorm-folded QKV GEMM writes K/V straight into the fp8
    attention image (row-stats + LDS-staged epilogue at C = 1280, V transposed through the
    tile in LDS; a forced split-K is overridden -- kv8 GEMMs never split; in-kernel-LN
    A-in-registers epilogue at C = 640, which ops.kv8_ok leaves to the pack in the UNet).  Q columns are bit-identical to the
    plain projection; the image matches the per-call pack of the bf16 K/V except for double-
    rounding ties (fp32 -> e4m3 directly vs via bf16), and the attention outputs agree."""
    from cassmantle_amd.ops._ext import ext
    B, H = 2, C // 64
    x = rnd(B, N, C, seed=60)
    lw = (rnd(C, scale=0.3, seed=61).float() + 1.0).to(torch.bfloat16)
    lb = rnd(C, scale=0.1, seed=62)
    w = rnd(3 * C, C, scale=C ** -0.5, seed=63)
    fold = ops.ln_fold(lw, lb, w)
    plain = ops.ln_linear(x, lw, lb, 1e-5, w, fold=fold).view(B, N, 3, H, 64)
    kv8 = ops.kv8_image(B, N, C, DEV)
    if split:
        ext().gemm_set_override(-1, split)
    try:
        qkv = ops.ln_linear(x, lw, lb, 1e-5, w, fold=fold, kv8=kv8).view(B, N, 3, H, 64)
    finally:
        if split:
            ext().gemm_set_override(-1, 0)
    assert torch.equal(qkv[:, :, 0], plain[:, :, 0])
    pk = ops.pack_kv_fp8(plain[:, :, 1], plain[:, :, 2])
    assert pk.numel() == kv8.numel()
    # fp32 -> e4m3 rounds once, fp32 -> bf16 -> e4m3 twice: they may differ by one code (an
    # e4m3 ulp) where the bf16 rounding lands on an e4m3 tie (measured ~3 % of the bytes)
    diff = (pk.int() - kv8.int()).abs()
    assert (diff != 0).float().mean().item() < 0.06
    assert diff.max().item() <= 1
    o1 = ops.attention(plain[:, :, 0], plain[:, :, 1], plain[:, :, 2], fp8=True, kv8=kv8)
    o2 = ops.attention(plain[:, :, 0], plain[:, :, 1], plain[:, :, 2], fp8=True, kv8=pk)
    exp = ref.attention(plain[:, :, 0], plain[:, :, 1], plain[:, :, 2])
    # one-ulp e4m3 differences in ~3 % of K/V move the output by fp8 noise (2.7 % at 256 keys)
    assert rel_err(o1, o2) < 0.05
    assert rel_err(o1, exp) < 0.12 and rel_err(o2, exp) < 0.12


@pytest.mark.parametrize("M,N,K,resid", [(2048, 1280, 1280, True), (512, 1280, 1280, False), (300, 640, 320, True)])
def test_gemm_row_stats_feed_folded_layernorm(M, N, K, resid):
    """a producer GEMM's epilogue accumulates the LayerNorm row statistics of its stored output
    (``row_stats``), and the LayerNorm-folded consumer reads them (``ln_linear(row_stats=)``)
    instead of running a statistics pass: same result as LayerNorm + GEMM"""
    from cassmantle_amd.ops._ext import ext
    x = rnd(M, K, seed=141)
    w = rnd(N, K, scale=K ** -0.5, seed=142)
    b = rnd(N, scale=0.1, seed=143)
    r = rnd(M, N, seed=144) if resid else None
    rs = ops.new_stats(1, M, DEV).view(M, 2)
    y = ops.linear(x, w, b, residual=r, row_stats=rs)
    assert tuple(ext().gemm_last_plan())[1] == 1          # row statistics: never split-K
    exp = ref.linear(x, w, b, residual=r)
    assert rel_err(y, exp) < 1e-2
    yf = y.float()
    got = ops.stats_to_float(rs.view(1, M, 2))[0].float()
    assert torch.allclose(got[:, 0], yf.sum(1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(got[:, 1], (yf * yf).sum(1), rtol=1e-4, atol=1e-1)
    # consumer: LayerNorm(y) @ W2^T through the fold, statistics from the producer
    g = rnd(N, seed=145) * 0.5 + 1
    be = rnd(N, seed=146) * 0.1
    w2 = rnd(3 * N // 2 // 8 * 8, N, scale=N ** -0.5, seed=147)
    fold = ops.ln_fold(g, be, w2)
    out = ops.ln_linear(y, g, be, 1e-5, w2, fold=fold, row_stats=rs)
    exp2 = ref.linear(ref.layer_norm(y, g, be, 1e-5), w2)
    assert rel_err(out, exp2) < 1e-2
    out_pass = ops.ln_linear(y, g, be, 1e-5, w2, fold=fold)      # the statistics-pass path
    assert rel_err(out, out_pass) < 5e-3      # (bf16 rounding of two different kernels)


@pytest.mark.parametrize("offset", [8.0, 24.0])
def test_row_stats_layernorm_with_large_row_means(offset):
    """the folded LayerNorm derives var = E[x^2] - mean^2 from the producer's fixed-point
    row sums; rows whose |mean| is many times their std (a residual stream plus a large constant)
    must still normalise like the statistics-pass path and the fp32 reference (the variance is now
    formed in fp64).  bf16 itself only resolves std ~ |mean| / 256, so offsets stay <= 24 std."""
    M, N, K = 1024, 1280, 1280
    x = rnd(M, K, seed=161)
    w = rnd(N, K, scale=K ** -0.5, seed=162)
    r = rnd(M, N, seed=163) + offset                      # residual stream with a large row mean
    rs = ops.new_stats(1, M, DEV).view(M, 2)
    y = ops.linear(x, w, None, residual=r, row_stats=rs)
    yf = y.float()
    assert (yf.mean(1).abs() / yf.std(1)).min().item() > 0.5 * offset / 1.5
    g = rnd(N, seed=164) * 0.5 + 1
    be = rnd(N, seed=165) * 0.1
    w2 = rnd(640, N, scale=N ** -0.5, seed=166)
    fold = ops.ln_fold(g, be, w2)
    out = ops.ln_linear(y, g, be, 1e-5, w2, fold=fold, row_stats=rs)
    out_pass = ops.ln_linear(y, g, be, 1e-5, w2, fold=fold)
    exp = ref.linear(ref.layer_norm(y, g, be, 1e-5), w2)
    assert rel_err(out, exp) < 2e-2, rel_err(out, exp)
    assert rel_err(out, out_pass) < 1e-2, rel_err(out, out_pass)


@pytest.mark.parametrize("B,S,C,N", [(2, 4096, 320, 320), (2, 1024, 640, 640), (1, 256, 320, 192)])
def test_gn_linear_folds_groupnorm_into_areg(B, S, C, N):
    """GroupNorm (producer statistics, no SiLU) applied to the A rows inside the A-in-registers
    GEMM (transformer GroupNorm -> proj_in) vs GroupNorm then GEMM in fp32"""
    from cassmantle_amd.ops._ext import ext
    x = rnd(B, S, C, seed=151) * 1.5 + 0.3
    st = ops.new_stats(B, C, DEV)
    ops.channel_stats_ref(x, st)
    g = rnd(C, seed=152) * 0.5 + 1
    be = rnd(C, seed=153) * 0.2
    w = rnd(N, C, scale=C ** -0.5, seed=154)
    b = rnd(N, scale=0.1, seed=155)
    out = ops.gn_linear(x, st, g, be, 32, 1e-6, w, b)
    assert tuple(ext().gemm_last_plan())[0] == 15
    exp = ref.linear(ref.group_norm(x.float(), 32, g.float(), be.float(), 1e-6, False).to(torch.bfloat16), w, b)
    assert rel_err(out, exp) < 1e-2


@pytest.mark.parametrize("V,D,k,dtype", [(1, 300, 1, torch.float32), (5000, 300, 51, torch.bfloat16),
                                         (100_003, 300, 64, torch.float32), (1_000_000, 300, 51, torch.bfloat16),
                                         (70_000, 64, 1024, torch.bfloat16),
                                         (70_000, 64, 2000, torch.bfloat16)])   # k > 1024: GEMV + stable sort
def test_cosine_topk_in_tree(V, D, k, dtype):
    """K15 (``most_similar``, reference src/backend.py:297-301): fused cosine GEMV + bitonic
    top-k + merge passes, no ATen kernel.  Exact ties (duplicated rows) rank the lower row
    first, as the reference oracle's stable sort does."""
    g = torch.Generator(device=DEV).manual_seed(V)
    t = torch.randn(V, D, device=DEV, generator=g).to(dtype)
    q = min(V - 1, 7)
    if V > 100:                       # exact ties at the top: copies of the query row and of row 11
        for j in (V // 3, V // 2, V - 1):
            t[j] = t[q]
        for j in (V // 5, V - 2):
            t[j] = t[11]
    vec = t[q]
    v, i = ops.cosine_topk(t, vec, k)
    ve, ie = ref.cosine_topk(t, vec, k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and v.shape == (k,) and i.shape == (k,)
    assert torch.allclose(v, ve, atol=2e-5), (v[:8], ve[:8])
    assert bool((v[:-1] >= v[1:]).all())                     # sorted, best first
    # the same rows, up to rounding-level near-ties of the two reductions
    same = i == ie
    if not bool(same.all()):
        bad = (~same).nonzero().flatten()
        assert torch.allclose(v[bad], ve[bad], atol=2e-5)
        assert set(i.tolist()) ^ set(ie.tolist()) <= set(i[bad].tolist()) | set(ie[bad].tolist())
    if V > 100:
        # exact ties (bit-identical rows): ascending row order inside each tie group
        top = [q, V // 3, V // 2, V - 1]
        assert i[:4].tolist() == sorted(top), i[:8]
        assert torch.equal(v[:4], v[:1].expand(4))


@pytest.mark.parametrize("variant", ["16x16", "32x32"])
@pytest.mark.parametrize("B,Nq,Nk,H,lens,qscale", [(2, 4096, 4096, 8, None, 1.0), (2, 1000, 77, 8, None, 1.0),
                                                   (3, 333, 200, 4, [200, 77, 3], 1.0),
                                                   (2, 512, 512, 8, None, 6.0),    # large scores: rescale path
                                                   (3, 300, 1000, 2, [1000, 300, 5], 1.0)])   # key split, empty split
def test_attention_d40_kernels(variant, B, Nq, Nk, H, lens, qscale):
    """head dim 40 (SD-1.5 level 1) on both kernels: the 16x16-block kernel (O^T over 48 rows,
    P^T from the S accumulators, V^T by transposed LDS reads) and the 32x32x16 kernel, on strided
    Q/K/V views of a fused QKV tensor, ragged key tiles, kv_lens and deferred-max rescales"""
    d = 40
    qkv = rnd(B, Nq, 3, H, d, seed=90)
    q = qkv[:, :, 0] * qscale
    kv = rnd(B, Nk, 2, H, d, seed=91)
    k, v = kv[:, :, 0], kv[:, :, 1]
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens else None
    ops.set_attention_d40_variant(variant)
    try:
        out = ops.attention(qkv[:, :, 0] if qscale == 1.0 else q, k, v, kv_lens=kl)
    finally:
        ops.set_attention_d40_variant(None)
    exp = ref.attention(q, k, v, kv_lens=kl)
    assert rel_err(out, exp) < 2e-2


@pytest.mark.parametrize("V,k,dtype,ties", [(300, 40, torch.bfloat16, False), (32000, 40, torch.bfloat16, True),
                                            (1000, 1, torch.float32, False), (5000, 1000, torch.float32, True),
                                            (128256, 50, torch.bfloat16, True)])
def test_lm_sample_kernel_matches_reference(V, k, dtype, ties):
    """the LM decode step samples in one in-tree kernel (radix-select top-k
    + Gumbel-max + state update) instead of ATen topk / gather / argmax.  Same contract as
    ops.reference.lm_sample, including ties at the k-th value (bf16 logits, repeated values) and
    the EOS bias of early steps; several steps chained on the device counters."""
    g = torch.Generator(device=DEV).manual_seed(V + k)
    steps = 6
    lg = torch.randn(steps, 1, V, device=DEV, generator=g) * 3
    if ties:                       # coarse values: many exact ties around the k-th largest
        lg = (lg * 2).round() / 2
    lg = lg.to(dtype)
    u = torch.rand(steps, 1, V, device=DEV, generator=g).clamp_(1e-10, 1 - 1e-7)
    noise = -torch.log(-torch.log(u))
    eos = 7
    eb = torch.zeros(steps, device=DEV)
    eb[:2] = float("-inf")
    state = {}
    for name, fn in (("hip", ops.lm_sample), ("ref", ref.lm_sample)):
        step = torch.zeros(1, device=DEV, dtype=torch.long)
        out = torch.full((steps, 1), -1, device=DEV, dtype=torch.long)
        tok = torch.zeros(1, device=DEV, dtype=torch.long)
        pos = torch.zeros(1, device=DEV, dtype=torch.int32)
        lens = torch.ones(1, device=DEV, dtype=torch.int32)
        for s in range(steps):
            fn(lg[s], noise, eb, eos, 0.8, k, step, out, tok, pos, lens)
        state[name] = (out.flatten().tolist(), int(tok), int(pos), int(lens), int(step))
    assert state["hip"] == state["ref"], state
    assert all(t != eos for t in state["hip"][0][:2])          # EOS suppressed by the -inf bias
