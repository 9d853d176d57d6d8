"""The weight-only fp8 kernels (ops/csrc/lm_fp8.hip) on the GPU with the instruments of
kernel_oracle.py: the GEMV on every case of gemv_fp8_cases.py (inputs inside NaN, outputs between
canaries, per-block error against fp64 of the same codes and scales), its row independence bit for
bit, the quantiser and dequantiser byte for byte against the CPU model, the dispatch edge at 8 | 9
rows, and the quantised TINY_LM through the captured decode loop.  test_lm_fp8.py proves the
checks on planted bugs without a GPU."""
import pytest
import torch

import gemv_fp8_cases as fc
import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.models.lm import TINY_LM, ByteTokenizer, CausalLM, LMTextGenerator
from cassmantle_amd.ops import reference as ref
from cassmantle_amd.ops._ext import ext, ext_available, ext_error
from kernel_oracle import BF16
from test_kernel_edges_gpu import DEV, G, P, check
from test_lm import _incremental_vs_full

pytestmark = pytest.mark.gpu
TOK = ByteTokenizer()


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    assert ext_available(), ext_error()
    ops.set_mode("hip")


def Q(q):
    return fc.poisoned_codes(q, DEV)


def _eps(c):
    return fc.RMS_EPS if c.rms else None


# ------------------------------------------------------------------------------ the GEMV
@pytest.mark.parametrize("c", fc.FP8_CASES, ids=lambda c: c.id)
def test_linear_fp8_edges(c):
    """the binding with contiguous and row-strided x, then ops.linear_fp8 with a strided x"""
    i = fc.fp8_inputs(c)
    y64 = fc.linear_fp8_64(c, i)
    qp, sp, bp, rp = Q(i.q), P(i.scale), P(i.bias), P(i.res)
    for xs in (P(i.x), P(i.x, strided=True)):
        g = G((c.M, c.N))
        assert xs.is_contiguous() or xs.stride(0) > c.K
        ext().gemv_fp8(xs, qp, sp, bp, rp, g.view, ops._ACT[c.act], -1.0 if not c.rms else fc.RMS_EPS)
        check(g, y64, "gemm", f"gemv_fp8 {c.id} lda={xs.stride(0)}", fc.BLOCK)
    g = G((c.M, c.N))
    ops.linear_fp8(P(i.x, strided=True), qp, sp, bp, residual=rp, act=c.act, rms_eps=_eps(c), out=g.view)
    check(g, y64, "gemm", f"linear_fp8 {c.id}", fc.BLOCK)


def test_fp32_output_and_a_strided_output():
    c = fc.Fp8Case(5, 70, 1040, "swiglu", True)
    i = fc.fp8_inputs(c)
    y64 = fc.linear_fp8_64(c, i)
    g = G((c.M, c.N), torch.float32)
    ops.linear_fp8(P(i.x), Q(i.q), P(i.scale), P(i.bias), residual=P(i.res), act=c.act, rms_eps=_eps(c), out=g.view)
    check(g, y64, "gemm", "linear_fp8 fp32 out", fc.BLOCK)
    wide = G((c.M, c.N + 24))                                     # ldc = N + 24: the columns beyond N stay canaries
    ops.linear_fp8(P(i.x), Q(i.q), P(i.scale), P(i.bias), residual=P(i.res), act=c.act, rms_eps=_eps(c),
                   out=wide.view[:, :c.N])
    torch.cuda.synchronize()
    ko.check_guards(wide)
    assert bool((ko.int_view(wide.view[:, c.N:]) == wide.pattern).all())
    assert ko.block_rel_err(wide.view[:, :c.N], y64, fc.BLOCK) < ko.BOUND["gemm"]


@pytest.mark.parametrize("act,rms", [("none", False), ("silu", True), ("swiglu", True), ("geglu", False)])
def test_a_row_is_the_same_bits_alone_and_in_any_batch(act, rms):
    """one template serves every M and a row's k order depends on K alone: row m of an M = 8, 5 or
    3 call equals the M = 1 call on that row, bit for bit"""
    for K in (48, fc.FP8_BODY + 16, 14336):
        c = fc.Fp8Case(8, 7, K, act, rms)
        i = fc.fp8_inputs(c)
        x, r = i.x.to(DEV), i.res.to(DEV)
        q, s, b = i.q.to(DEV), i.scale.to(DEV), i.bias.to(DEV)
        alone = torch.cat([ops.linear_fp8(x[m:m + 1], q, s, b, residual=r[m:m + 1], act=act, rms_eps=_eps(c))
                           for m in range(8)])
        for M in (8, 5, 3):
            y = ops.linear_fp8(x[:M], q, s, b, residual=r[:M], act=act, rms_eps=_eps(c))
            assert torch.equal(ko.int_view(y), ko.int_view(alone[:M])), (K, M)


# ------------------------------------------------------------------------------ quantiser, dequantiser
@pytest.mark.parametrize("K", fc.QUANT_K)
@pytest.mark.parametrize("N", fc.QUANT_N)
def test_quantiser_and_dequantiser_equal_the_cpu_model_byte_for_byte(N, K):
    for with_gain in (True, False):
        w, gamma = fc.fp8_weight(N, K, seed=N + K, rms=with_gain)
        if N > 1:
            w[N // 2] = 0                                         # an all-zero row: scale 1, codes 0
        want_q, want_s = ref.quantize_rows_fp8(w, gamma)
        gq, gs = G((N, K), torch.uint8), G((N,), torch.float32)
        ext().quant_rows_fp8(P(w), P(gamma), gq.view, gs.view)
        torch.cuda.synchronize()
        ko.check_guards(gq, gs)
        assert torch.equal(gs.view.cpu(), want_s) and torch.equal(gq.view.cpu(), want_q), (N, K, with_gain)
        q, s = ops.quantize_rows_fp8(P(w), P(gamma))
        assert torch.equal(s.cpu(), want_s) and torch.equal(q.cpu(), want_q)
        gd = G((N, K))
        ext().dequant_rows_fp8(Q(want_q), P(want_s), gd.view)
        torch.cuda.synchronize()
        ko.check_guards(gd)
        assert torch.equal(ko.int_view(gd.view.cpu()), ko.int_view(ref.dequantize_rows_fp8(want_q, want_s)))


def test_every_code_converts_exactly_and_subnormal_quotients_round_to_even():
    codes = fc.all_e4m3_codes()
    q = codes.repeat(3, 1)                                        # [3, 256]
    s = torch.tensor([1.0, 2.0 ** -9, 3.0])
    gd = G((3, 256))
    ext().dequant_rows_fp8(Q(q), P(s), gd.view)
    torch.cuda.synchronize()
    ko.check_guards(gd)
    assert torch.equal(ko.int_view(gd.view.cpu()), ko.int_view(ref.dequantize_rows_fp8(q, s)))
    # quotients on and around every e4m3 midpoint, subnormal ones included: the row maximum 448 makes
    # the scale 1, so the codes are RNE_e4m3 of the bf16 values themselves
    vals = ref.e4m3_decode(codes)[:0x7F].double()
    mids = (vals[:-1] + vals[1:]) / 2
    pts = torch.cat([vals, mids, mids * (1 + 2.0 ** -7), mids * (1 - 2.0 ** -7)]).to(BF16)
    pts = torch.cat([pts, -pts, torch.tensor([448.0], dtype=BF16)])
    w = torch.cat([pts, torch.zeros(-len(pts) % 16, dtype=BF16)])[None]
    want_q, want_s = ref.quantize_rows_fp8(w)
    assert want_s.item() == 1.0
    q2, s2 = ops.quantize_rows_fp8(w.to(DEV))
    assert torch.equal(s2.cpu(), want_s) and torch.equal(q2.cpu(), want_q)


def test_non_finite_rows_raise_on_the_device():
    w, _ = fc.fp8_weight(3, 48, seed=1)
    for bad in (float("inf"), float("nan")):
        wb = w.clone()
        wb[1, 47] = bad
        with pytest.raises(ValueError, match="non-finite"):
            ops.quantize_rows_fp8(wb.to(DEV))


# ------------------------------------------------------------------------------ dispatch edge
@pytest.mark.parametrize("c", fc.DISPATCH_CASES, ids=lambda c: c.id)
def test_dispatch_edge_between_the_gemv_and_dequantise_plus_gemm(c):
    """8 rows stream the codes; 9 rows dequantise into the scratch and run the bf16 GEMM, held
    against fp64 of the bf16-rounded W'.  With the RMS scale the 9-row side is two kernels with a
    stored bf16 tensor between them (the RMSNorm with a gain of ones, as rms_linear above 8 rows):
    its reference takes those bf16 rows, since an A operand rounded after normalisation moves
    outputs whose dot product nearly cancels by more than the bound (9e-2 in the worst 1x4 block
    of this case, on the CPU) - the reason the GEMV takes raw x."""
    i = fc.fp8_inputs(c)
    if c.M <= ops.FP8_GEMV_ROWS:
        y64 = fc.linear_fp8_64(c, i)
    else:
        w16 = ref.dequantize_rows_fp8(i.q, i.scale)
        xn = ref.rms_norm(i.x, torch.ones(c.K, dtype=BF16), fc.RMS_EPS) if c.rms else i.x
        assert xn.dtype == BF16
        y64 = ko.linear64(xn, w16, i.bias, i.res, c.act)
    g, scratch = G((c.M, c.N)), G((i.q.numel() + 64,))
    ops.linear_fp8(P(i.x), Q(i.q), P(i.scale), P(i.bias), residual=P(i.res), act=c.act, rms_eps=_eps(c), out=g.view,
                   scratch=scratch.view)
    check(g, y64, "gemm", f"linear_fp8 dispatch {c.id}", fc.BLOCK)
    ko.check_guards(scratch)
    if c.M > ops.FP8_GEMV_ROWS:
        assert torch.equal(ko.int_view(scratch.view[:i.q.numel()].cpu()), ko.int_view(w16.flatten()))
        assert bool((ko.int_view(scratch.view[i.q.numel():]) == scratch.pattern).all())


# ------------------------------------------------------------------------------ the quantised model
def test_fp8_lm_decode_matches_its_full_forward():
    m = CausalLM(TINY_LM, device=DEV, seed=4).quantize_fp8_()
    tokens = torch.randint(0, TINY_LM.vocab, (1, 20), generator=torch.Generator().manual_seed(1)).to(DEV)
    errs, scale = _incremental_vs_full(m, tokens, 12)             # a 12-row prefill: dequantise + GEMM
    print(f"fp8 tiny-lm: worst logit error {max(errs):.4f} of scale {scale:.3f}")
    assert max(errs) < 0.05 * scale, (errs, scale)
    assert m._scratch is not None and m._scratch.numel() == max(TINY_LM.vocab * TINY_LM.dim, 2 * TINY_LM.ffn * TINY_LM.dim)


@pytest.fixture(scope="module")
def gens():
    return {graphs: LMTextGenerator(TINY_LM, device=DEV, seed=5, use_graphs=graphs, noise="philox", max_batch=8,
                                    weight_dtype="fp8", max_new_cap=32) for graphs in (True, False)}


def test_fp8_graph_and_eager_give_the_same_tokens_and_seeds_repeat(gens):
    prompts = [[TOK.bos, 10, 20, 30], [TOK.bos, 65, 66]]
    a = gens[True].generate_ids_batch(prompts, 24, 24, seeds=[3, 4])
    b = gens[False].generate_ids_batch(prompts, 24, 24, seeds=[3, 4])
    assert gens[True].buckets[2].graph is not None and gens[False].buckets[2].graph is None
    assert all(len(r) == 24 for r in a) and a == b                # the same kernels in the same order
    assert gens[True].generate_ids_batch(prompts, 24, 24, seeds=[3, 4]) == a
    assert gens[True].generate_ids_batch(prompts, 24, 24, seeds=[5, 4])[1] == a[1]


def test_fp8_alone_equals_bucket_eight(gens):
    """two-token prompts: prefill (one position) and decode both run gemv_fp8_kernel, whose rows do
    not depend on M, so a sequence alone and in a bucket of 8 samples the same tokens"""
    prompts = [[TOK.bos, 65 + i] for i in range(8)]
    seeds = list(range(31, 39))
    batch = gens[True].generate_ids_batch(prompts, 4, 16, seeds=seeds)
    assert sorted(gens[True].buckets)[-1] == 8
    for i in (0, 3, 7):
        assert gens[True].generate_ids_batch([prompts[i]], 4, 16, seeds=[seeds[i]])[0] == batch[i], i
