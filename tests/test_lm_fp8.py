"""Weight-only fp8 for the prompt LM (ops/csrc/lm_fp8.hip's weight contract) without a GPU: the
ideal kernel model against the per-block bound and its planted bugs, the quantiser model, the
quantised model against its own fp32 oracle, and the flag through generator, factory and config.
test_lm_fp8_gpu.py holds the kernels to the same cases and models."""
import math

import pytest
import torch

import gemv_fp8_cases as fc
import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.models.lm import TINY_LM, CausalLM, LMTextGenerator
from cassmantle_amd.ops import reference as ref
from kernel_oracle import BF16, BOUND, F64, block_rel_err
from test_lm import _incremental_vs_full


# ------------------------------------------------------------------------------ the ideal kernel
def test_ideal_kernel_stays_under_half_the_bound_in_every_block():
    """raw x, exact e4m3, the scales and the bf16 store: half of BOUND["gemm"] in every 1x4 block of
    every case (measured: the worst is printed)"""
    worst = (0.0, None)
    for c in fc.FP8_CASES:
        i = fc.fp8_inputs(c)
        g = fc.fp8_model(c, i)
        ko.check_guards(g)
        e = block_rel_err(g.view, fc.linear_fp8_64(c, i), fc.BLOCK)
        worst = max(worst, (e, c.id))
        assert e < BOUND["gemm"] / 2, (c.id, e)
    print(f"ideal fp8 GEMV: worst 1x4 block {worst[0]:.3e} at {worst[1]} (bound {BOUND['gemm'] / 2:g})")


def test_cases_cover_the_shapes():
    cs = fc.FP8_CASES
    assert {c.M for c in cs} == set(fc.FP8_M) and set(fc.FP8_N) | {3, 9} <= {c.N for c in cs}
    assert {c.K for c in cs} == set(fc.FP8_K) and {c.act for c in cs} == {"none", "silu", "swiglu", "geglu"}
    for K in fc.FP8_K:
        assert {c.rms for c in cs if c.K == K} == {True, False}, K
    assert all(c.K % 16 == 0 for c in cs)
    i = fc.fp8_inputs(fc.Fp8Case(8, 9, 48, "swiglu", True))
    assert len(set(i.scale.tolist())) == 18                      # every row and gate row its own scale
    x = i.x.double()
    assert len(set((x * x).mean(-1).tolist())) == 8               # every activation row its own 1/rms


def test_every_row_taking_row_0_scale_fails():
    for c in fc.FP8_CASES:
        if c.N == 1 and not c.gated:
            continue                                              # one weight row: row 0's scale is right
        i = fc.fp8_inputs(c)
        e = block_rel_err(fc.fp8_model(c, i, scale_of_row0=True).view, fc.linear_fp8_64(c, i), fc.BLOCK)
        assert e > BOUND["gemm"], (c.id, e)


def test_gate_rows_taking_the_value_rows_scales_fails():
    hit = 0
    for c in fc.FP8_CASES:
        i = fc.fp8_inputs(c)
        e = block_rel_err(fc.fp8_model(c, i, gate_takes_value_scale=True).view, fc.linear_fp8_64(c, i), fc.BLOCK)
        # N % 4 == 0 apart, gate row N + n has another W_ROW_SCALE than value row n
        assert (e > BOUND["gemm"]) == c.gated, (c.id, e)
        hit += c.gated
    assert hit >= 40


def test_last_16_k_elements_dropped_fails():
    """16 of K elements carry about sqrt(16 / K) of a dot product: 12 % at K = 1040, 3.3 % at
    14336, beside a residual of the dot product's size.  Every case up to one body of the loop is
    caught; beyond it a one-row case with two blocks may land just under the bound, so there
    every K is caught in some case, and nearly all cases are"""
    worst, missed = {}, []
    for c in fc.FP8_CASES:
        if c.K == 48:
            continue                                              # the N sweep; every K has its own cases
        i = fc.fp8_inputs(c)
        e = block_rel_err(fc.fp8_model(c, i, drop_last_16=True).view, fc.linear_fp8_64(c, i), fc.BLOCK)
        worst[c.K] = max(worst.get(c.K, 0.0), e)
        if not e > BOUND["gemm"]:
            assert c.K > fc.FP8_BODY + 16, (c.id, e)
            missed.append((c.id, e))
    assert set(worst) == set(fc.FP8_K) - {48} and all(e > BOUND["gemm"] for e in worst.values()), worst
    assert len(missed) <= 2, missed


# ------------------------------------------------------------------------------ the quantiser model
def test_every_finite_code_times_a_power_of_two_survives_a_round_trip():
    codes = fc.all_e4m3_codes()
    vals = ref.e4m3_decode(codes)
    assert vals.abs().max() == 448 and bool(torch.isfinite(vals).all())
    for p in (-9, 0, 5):
        # a row whose maximum is 448 * 2^p has scale 2^p exactly, so every code comes back
        w = (vals * 2.0 ** p).to(BF16)[None]
        assert torch.equal(w.float(), vals[None] * 2.0 ** p)      # e4m3 * 2^p is exact in bf16
        q, s = ref.quantize_rows_fp8(w)
        assert s.item() == 2.0 ** p
        back = q[0].clone()
        back[back == 0x80] = 0                                    # -0 and +0 are one value
        assert torch.equal(back, torch.where(codes == 0x80, torch.zeros_like(codes), codes)), p
        assert torch.equal(ref.dequantize_rows_fp8(q, s), w)


def test_row_maximum_maps_to_448_and_a_zero_row_to_scale_1():
    w, gamma = fc.fp8_weight(9, 4112, seed=3)
    w[4] = 0
    q, s = ref.quantize_rows_fp8(w, gamma)
    v = w.float() * gamma.float()
    assert s[4].item() == 1.0 and int(q[4].max()) == 0
    assert not bool(((q & 0x7F) == 0x7F).any())                   # never a NaN code
    dec = ref.e4m3_decode(q)
    for n in (0, 1, 2, 3, 5, 8):
        k = int(v[n].abs().argmax())
        assert dec[n, k].item() == math.copysign(448.0, v[n, k].item()), n
        assert s[n].item() == (v[n].abs().max() / torch.tensor(448.0)).item()
    assert len(set(s.tolist())) == 9


def test_quantisation_error_is_half_an_e4m3_ulp_elementwise():
    for N, K in ((5, 48), (70, 4112)):
        w, gamma = fc.fp8_weight(N, K, seed=N + K)
        q, s = ref.quantize_rows_fp8(w, gamma)
        v = w.double() * gamma.double()
        sd = s.double()[:, None]
        err = (v - ref.dequantize_rows_fp8(q, s, dtype=F64)).abs()
        # half an ulp of a 3-bit mantissa at |v / scale| (below 2^-6: the subnormal spacing 2^-9)
        half_ulp = sd * 2.0 ** -4 * (v / sd).abs().clamp_min(2.0 ** -6)
        assert bool((err <= half_ulp).all()), (N, K, (err / half_ulp).max().item())


def test_non_finite_rows_and_odd_k_raise():
    w, _ = fc.fp8_weight(3, 48, seed=1)
    for bad in (math.inf, -math.inf, math.nan):
        wb = w.clone()
        wb[1, 7] = bad
        assert not bool(torch.isfinite(ref.quantize_rows_fp8(wb)[1][1]))
        with pytest.raises(ValueError, match="non-finite"):
            ops.quantize_rows_fp8(wb)
    with pytest.raises(ValueError, match="K % 16"):
        ops.quantize_rows_fp8(ko.rnd(3, 40))
    q, s = ops.quantize_rows_fp8(ko.rnd(3, 48))
    with pytest.raises(ValueError, match="K % 16"):
        ops.linear_fp8(ko.rnd(2, 40), q[:, :40].contiguous(), s)


def test_ops_run_the_references_on_the_cpu():
    c = fc.Fp8Case(3, 5, 48, "swiglu", True)
    i = fc.fp8_inputs(c)
    y = ops.linear_fp8(i.x, i.q, i.scale, i.bias, residual=i.res, act=c.act, rms_eps=fc.RMS_EPS)
    assert y.dtype == BF16 and block_rel_err(y, fc.linear_fp8_64(c, i), fc.BLOCK) < BOUND["gemm"]
    out = torch.empty(3, 5, dtype=BF16)
    assert ops.linear_fp8(i.x, i.q, i.scale, i.bias, residual=i.res, act=c.act, rms_eps=fc.RMS_EPS, out=out) is out
    assert torch.equal(out, y)
    buf = torch.zeros(1000, dtype=BF16)
    w = ops.dequantize_rows_fp8(i.q, i.scale, out=buf)
    assert w.shape == i.q.shape and w.data_ptr() == buf.data_ptr() and torch.equal(w, ref.dequantize_rows_fp8(i.q, i.scale))


# ------------------------------------------------------------------------------ the model
def _quantised(seed=1):
    return CausalLM(TINY_LM, seed=seed).quantize_fp8_()


def test_quantised_lm_incremental_decode_matches_its_full_forward():
    """full_logits of a quantised model multiplies e4m3(q) * scale in fp32: the oracle of the fp8
    path, under test_lm.py's own tolerance"""
    m = _quantised()
    tokens = torch.randint(0, TINY_LM.vocab, (1, 12), generator=torch.Generator().manual_seed(0))
    errs, scale = _incremental_vs_full(m, tokens, 8)
    assert max(errs) < 0.03 * scale, (errs, scale)
    # (and it is another model than the bf16 one: the oracle is the quantised weights')
    assert (m.full_logits(tokens) - CausalLM(TINY_LM, seed=1).full_logits(tokens)).abs().max() > 0


def test_quantise_folds_the_gains_frees_bf16_and_a_second_call_raises():
    m = CausalLM(TINY_LM, seed=2)
    for blk in m.blocks:
        blk.attn_norm.data.copy_(ko.rnd(TINY_LM.dim, scale=0.3, shift=1.0, seed=11))
        blk.mlp_norm.data.copy_(ko.rnd(TINY_LM.dim, scale=0.3, shift=1.0, seed=12))
    m.norm.data.copy_(ko.rnd(TINY_LM.dim, scale=0.3, shift=1.0, seed=13))
    tokens = torch.randint(0, TINY_LM.vocab, (1, 10), generator=torch.Generator().manual_seed(3))
    before = m.full_logits(tokens)
    want_q, want_s = ref.quantize_rows_fp8(m.blocks[0].qkv.data, m.blocks[0].attn_norm.data)
    bf16_bytes = m.weight_bytes()
    assert m.quantize_fp8_() is m and m.quantized
    names = {n for n, _ in m.named_parameters()}
    assert names == {"embed", "norm"} | {f"blocks.{i}.{n}" for i in range(TINY_LM.layers) for n in ("attn_norm", "mlp_norm")}
    assert torch.equal(m.blocks[0].qkv_q, want_q) and torch.equal(m.blocks[0].qkv_s, want_s)
    assert all(bool((p == 1).all()) for n, p in m.named_parameters() if n.endswith("norm"))
    assert m.embed.dtype == BF16 and m.lm_head_q.dtype == torch.uint8 and m.lm_head_s.dtype == torch.float32
    assert 0.5 * bf16_bytes < m.weight_bytes() < 0.52 * bf16_bytes
    # the gains went into the weights: the quantised model stays near the bf16 one (random Gaussian
    # rows cost ~3e-2 per projection; a lost gain of 1 +- 0.3 would cost ~3e-1)
    after = m.full_logits(tokens)
    assert ((after - before).norm() / before.norm()).item() < 0.1
    with pytest.raises(RuntimeError, match="quantised already"):
        m.quantize_fp8_()


def test_checkpoint_round_trip_is_load_then_quantise():
    from cassmantle_amd.models.weights import export_causal_lm, load_causal_lm
    a, b = CausalLM(TINY_LM, seed=1), CausalLM(TINY_LM, seed=2)
    assert load_causal_lm(b, export_causal_lm(a)) == []
    a.quantize_fp8_()
    b.quantize_fp8_()
    for (na, ta), (nb, tb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert na == nb and torch.equal(ta, tb), na
    assert "blocks.1.gate_up_q" in a.state_dict() and "blocks.1.gate_up" not in a.state_dict()


# ------------------------------------------------------------------------------ the interface
def test_generator_weight_dtype():
    g = LMTextGenerator(TINY_LM, device="cpu", seed=3, weight_dtype="fp8")
    assert g.weight_dtype == "fp8" and g.model.quantized and g.quant_ms > 0
    assert len(g.generate_ids([256, 72, 105], 6, 6)) == 6        # EOS suppressed until min_new_tokens
    assert len(g.generate_ids([256, 72, 105], 0, 5)) <= 5
    assert isinstance(g.generate_text("The lantern", 2, 8), str)
    with pytest.raises(RuntimeError, match="before the first"):
        g.quantize_fp8()
    with pytest.raises(ValueError, match="bf16, fp8"):
        LMTextGenerator(TINY_LM, device="cpu", weight_dtype="int8")
    from cassmantle_amd.game.prompts import LMPromptGenerator
    out = LMPromptGenerator(g, min_new_tokens=4, max_new_tokens=12).generate("The Clockwork Orchard", True)
    assert out.endswith(".") and out.count(".") >= 1


def test_bf16_generator_is_the_default_one():
    """weight_dtype="bf16" quantises nothing and samples the tokens of a generator built without the
    argument, from the table and from Philox noise"""
    for kw in ({}, {"noise": "philox", "max_batch": 2}):
        a = LMTextGenerator(TINY_LM, device="cpu", seed=7, **kw)
        b = LMTextGenerator(TINY_LM, device="cpu", seed=7, weight_dtype="bf16", **kw)
        assert not b.model.quantized and b.weight_dtype == "bf16" and b.quant_ms == 0.0
        assert [n for n, _ in a.model.state_dict().items()] == [n for n, _ in b.model.state_dict().items()]
        assert a.generate_ids([256, 84, 104, 101], 8, 8) == b.generate_ids([256, 84, 104, 101], 8, 8)
    c = LMTextGenerator(TINY_LM, device="cpu", seed=7, weight_dtype="fp8")
    assert len(c.generate_ids([256, 84, 104, 101], 8, 8)) == 8


def test_flag_parses_and_the_factory_builds_an_fp8_generator(tmp_path):
    from cassmantle_amd.config import Config
    from cassmantle_amd.game.prompts import LMPromptGenerator
    from cassmantle_amd.runtime.factory import build_prompt_generator
    assert Config().model.lm_weight_dtype == "bf16"
    assert Config.from_args(["--lm_weight_dtype", "fp8"], base=Config()).model.lm_weight_dtype == "fp8"
    assert Config.from_env({"CASSMANTLE_LM_WEIGHT_DTYPE": "fp8"}).model.lm_weight_dtype == "fp8"
    cfg = Config()
    cfg.model.prompt_generator, cfg.model.lm_model = "lm", "tiny-lm"
    assert not build_prompt_generator(cfg, device="cpu").lm.model.quantized
    cfg.model.lm_weight_dtype = "fp8"
    pg = build_prompt_generator(cfg, device="cpu")
    assert isinstance(pg, LMPromptGenerator) and pg.lm.model.quantized and pg.lm.weight_dtype == "fp8"
    assert isinstance(pg.generate("Chapter One: The Lantern", True), str)
    cfg.model.lm_weight_dtype = "int8"
    with pytest.raises(ValueError, match="bf16, fp8"):
        build_prompt_generator(cfg, device="cpu")
