"""The CPU model of the fp8 attention kernel's K/V image (kernel_oracle.kv8_image_model), proven
without a GPU: the slot order is the header comment's kappa and a bijection, the decoded image is
e4m3 of K and V on the valid keys and zero elsewhere, attention computed from it is
ideal_attention(fp8=True) exactly, and the byte comparison test_kernel_edges_kv8_gpu.py makes
rejects each planted bug -- of which the fp8 attention check (BOUND["fp8"] per 16 queries, the
only check the pack had) lets every one through."""
import pytest
import torch

import kernel_oracle as ko
from cassmantle_amd.ops import reference as ref
from kernel_oracle import BOUND, F64, block_rel_err

QBLOCK = (1, 16, 1, None)
ATTN_CASES = ko.attn_cases(64)


def _image(c, **kw):
    _, k, v = ko.attn_data(c)
    return ko.kv8_image_model(k, v, c.lens, **kw)


def planted(c, bug):
    if bug == "natural_order":
        return _image(c, key_of_slot=lambda s: s)
    if bug == "halves_swapped":
        return _image(c, key_of_slot=ko.kv8_key_halves_swapped)
    if bug == "padding_not_zero":
        return _image(c, zero_past_lens=False)
    if bug == "stale_run":
        return ko.kv8_stale_run(_image(c), c.B, c.Nk, c.Hk)
    assert bug == "neighbour_head"
    return ko.kv8_neighbour_head(_image(c), c.B, c.Nk, c.Hk)


BUGS = ("natural_order", "halves_swapped", "padding_not_zero", "stale_run", "neighbour_head")
# the planted bugs the fp8 attention check does not see: every one of them.  attn_data's dominant keys
# (0, 62, 63, 64, 128 and key 0 of a batch) are fixed points of kappa and of both wrong orders, their V
# is LAST_V in every head, and the queries that follow them carry the norm of each 16-query block
PASSES_THE_ATTENTION_CHECK = BUGS


def test_slot_order_is_a_bijection_and_matches_the_header():
    s = torch.arange(64)
    keys = ko.kv8_key(s)
    assert sorted(keys.tolist()) == list(range(64))
    assert torch.equal(ko.kv8_key(ko.kv8_slot(s)), s) and torch.equal(ko.kv8_slot(ko.kv8_key(s)), s)
    # slot 32h + j: S accumulator register j & 15 of key half j >> 4 in lane half h (attention.hip)
    assert int(ko.kv8_key(torch.tensor(0))) == 0 and int(ko.kv8_key(torch.tensor(32))) == 4
    assert ko.kv8_key(torch.arange(4, 8)).tolist() == [8, 9, 10, 11] and int(ko.kv8_key(torch.tensor(16))) == 32
    swapped = ko.kv8_key_halves_swapped(s)
    assert sorted(swapped.tolist()) == list(range(64)) and not torch.equal(swapped, keys)


def test_e4m3_encode_is_the_cast_quantize_rows_fp8_makes():
    x = ko.all_bf16(with_inf=False)
    q = ref.e4m3_encode(x)
    assert q.dtype == torch.uint8 and torch.equal(ref.e4m3_decode(q, F64), ko.e4m3(x.to(F64)))
    big = x.float().abs() > 448
    assert bool(((q[big] & 0x7F) == 0x7E).all()) and torch.equal(q[big] >> 7, (x[big].float() < 0).to(torch.uint8))
    w = ko.rnd(4, 32, seed=1)
    qr, scale = ref.quantize_rows_fp8(w)
    assert torch.equal(qr, ref.e4m3_encode(w.float() / scale[:, None]))


@pytest.mark.parametrize("B,Nk,Hk,lens", ko.KV8_PACK_CASES, ids=str)
def test_unpacked_model_is_e4m3_of_k_and_v(B, Nk, Hk, lens):
    k, v = ko.rnd(B, Nk, Hk, 64, seed=Nk), ko.rnd(B, Nk, Hk, 64, scale=3.0, seed=Nk + 1)
    v[:, -1] = ko.SENTINEL_V if lens is not None else 500.0        # past lens: zeroed; valid: saturates
    img = ko.kv8_image_model(k, v, lens)
    Nkp = (Nk + 63) // 64 * 64
    assert img.dtype == torch.uint8 and img.numel() == 2 * B * Hk * Nkp * 64
    K, V = ko.kv8_unpack(img, B, Nk, Hk)
    for b in range(B):
        n = Nk if lens is None else min(Nk, lens[b])
        assert torch.equal(K[b, :n], ko.e4m3(k[b, :n].to(F64))) and torch.equal(V[b, :n], ko.e4m3(v[b, :n].to(F64)))
        assert not K[b, n:].any() and not V[b, n:].any()
        K8, V8t = ko.kv8_views(img, B, Nk, Hk)
        assert not K8[b, :, n:].any(), "padding is byte 0x00 (not -0.0)"
        if n == 0:
            assert not V8t[b].any()


@pytest.mark.parametrize("c", ATTN_CASES, ids=lambda c: c.id)
def test_attention_from_the_image_is_the_ideal_fp8_attention(c):
    q, k, v = ko.attn_data(c)
    o = ko.ideal_attention(q, k, v, c.lens, c.causal, fp8=True)
    assert torch.equal(ko.ideal_attention(q, k, v, c.lens, c.causal, fp8=True, kv8=ko.kv8_image_model(k, v, c.lens)), o)


@pytest.mark.parametrize("bug", BUGS)
def test_byte_comparison_rejects_the_planted_image(bug):
    """on every case with something to get wrong: ``padding_not_zero`` needs a key past lens, the
    two orders a second key (key 0 is slot 0 in all of them)"""
    hit = 0
    for c in ATTN_CASES[:len(ko.ATTN_NK)] + ATTN_CASES[-1:]:
        good, bad = _image(c), planted(c, bug)
        assert bad.shape == good.shape and bad.dtype == torch.uint8
        # (Nk = 1: key 0 is slot 0 in every order, and its V is LAST_V in every head)
        expect = c.lens is not None if bug == "padding_not_zero" else c.Nk > 1 or bug == "stale_run"
        assert torch.equal(bad, good) != expect, c.id
        hit += expect
    assert hit >= 4


@pytest.mark.parametrize("bug", BUGS)
def test_which_planted_images_the_fp8_attention_check_lets_through(bug):
    """the check test_attention_fp8_edges makes, with the attention evaluated from the bugged image
    as the fp8 kernel would read it (it masks keys past lens itself, so what the padding holds
    never reaches a product; a stale 16-slot run of one d-row drowns in a 16 x 64 block; the wrong
    orders and the neighbouring head move only the V of keys that carry little weight).  Measured:
    natural_order 6.7e-2, halves_swapped 5.8e-2, padding_not_zero 5.28e-2 (the ideal's own figure),
    stale_run 5.28e-2, neighbour_head 6.9e-2, against a bound of 0.12"""
    worst, failed = 0.0, []
    for c in ATTN_CASES:
        q, k, v = ko.attn_data(c)
        o64 = ko.attention64(q, k, v, c.lens, c.causal)
        e = block_rel_err(ko.ideal_attention(q, k, v, c.lens, c.causal, fp8=True, kv8=planted(c, bug)), o64, QBLOCK)
        worst = max(worst, e)
        if not e < BOUND["fp8"]:
            failed.append(c.id)
    print(f"{bug}: worst block {worst:.3e} (bound {BOUND['fp8']:g}), {len(failed)} of {len(ATTN_CASES)} cases fail")
    assert (failed == []) == (bug in PASSES_THE_ATTENTION_CHECK), (bug, worst, failed)
