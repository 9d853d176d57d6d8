"""CPU tests of the batched LM prompt path: the Gumbel noise model (models/schedulers.py
philox_gumbel, the numpy side of ops/csrc/philox_gumbel.h), the contract of the seeded sampler
(ops.reference.lm_sample_seeded), LMTextGenerator's batch decode on a stub model whose logits are
exactly row-independent, the default (noise table) path held to token ids recorded from the
parent commit, the rooms' batching front (game/prompts.py BatchingPromptGenerator) and the flags."""
import json
import math
import os
import threading
import time

import numpy as np
import pytest
import torch

import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.game.prompts import BatchingPromptGenerator, LMPromptGenerator, PromptGenerator
from cassmantle_amd.models import schedulers as S
from cassmantle_amd.models.lm import TINY_LM, ByteTokenizer, LMTextGenerator
from cassmantle_amd.ops import reference as ref
from cassmantle_amd.runtime.factory import build_prompt_generator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 0x1234_5678_9ABC_DEF0


# ------------------------------------------------------------------------------ noise model
def test_gumbel_words_are_the_contracts_philox_words():
    ids = np.asarray([0, 1, 2, 3, 4, 7, 31999, 2 ** 17 - 1])
    for seed in (0, -1, SEED, 2 ** 63 - 1, -2 ** 63):
        for step in (0, 1, 95, 2 ** 32 - 1):
            w = S.philox_gumbel_words([seed], step, ids)[0]
            for i, got in zip(ids.tolist(), w.tolist()):
                assert got == int(S.philox4x32((i >> 2, step, 0, 0), S.seed_key(seed))[i & 3])
    both = S.philox_gumbel([SEED + 1, SEED], 3, ids)
    assert np.array_equal(both[1], S.philox_gumbel([SEED], 3, ids)[0])          # a row knows nothing of the batch
    assert not np.array_equal(both[0], both[1])
    assert not np.array_equal(S.philox_gumbel([SEED], 4, ids), S.philox_gumbel([SEED], 3, ids))
    assert np.array_equal(S.philox_gumbel([SEED], 3, ids[[5, 2]])[0], both[1][[5, 2]])


def test_gumbel_moments():
    n = 2 ** 18
    g = S.philox_gumbel([SEED], 7, np.arange(n))[0]
    var = math.pi ** 2 / 6
    assert abs(g.mean() - 0.5772156649) < 4 * math.sqrt(var / n)
    assert abs(g.var() / var - 1) < 0.02
    assert -2.853 <= g.min() and g.max() <= 17.329


def test_gumbel_max_samples_the_softmax():
    """2^16 steps of Gumbel-max on 4 fixed logits: frequencies within 4 sigma of the softmax"""
    logits = np.asarray([0.3, -1.0, 1.2, 0.0])
    n = 2 ** 16
    picks = np.stack([S.philox_gumbel([SEED], s, np.arange(4))[0] for s in range(n)]) + logits
    freq = np.bincount(picks.argmax(1), minlength=4) / n
    p = np.exp(logits) / np.exp(logits).sum()
    assert np.all(np.abs(freq - p) < 4 * np.sqrt(p * (1 - p) / n)), (freq, p)


# ------------------------------------------------------------------------------ reference sampler
def _state(B, steps, step0=0):
    return dict(step=torch.full((B,), step0, dtype=torch.long), out=torch.full((steps, B), -1, dtype=torch.long),
                tok=torch.zeros(B, dtype=torch.long), pos=torch.arange(B, dtype=torch.int32),
                lens=torch.arange(B, dtype=torch.int32) + 1)


def _sample(fn, logits, seeds, T=0.8, k=40, eos=7, eb=0.0, steps=4, step0=None):
    B = logits.shape[0]
    st = _state(B, steps)
    if step0 is not None:
        st["step"] = torch.tensor(step0, dtype=torch.long)
    fn(logits, torch.tensor(S.seeds_int64(seeds)), torch.full((steps,), eb), eos, T, k, **st)
    return st


def test_reference_updates_every_rows_own_state():
    lg = ko.rnd(3, 300, scale=3.0, seed=1, dtype=torch.float32)
    st = _sample(ref.lm_sample_seeded, lg, [1, 2, 3], step0=[0, 2, 3])
    assert st["step"].tolist() == [1, 3, 4] and st["pos"].tolist() == [1, 2, 3] and st["lens"].tolist() == [2, 3, 4]
    for b, s in enumerate((0, 2, 3)):
        assert st["out"][s, b] == st["tok"][b] and 0 <= int(st["tok"][b]) < 300
        assert (st["out"][:, b] == -1).sum() == 3                                   # one entry per row written
    ops.lm_sample_seeded(lg, torch.tensor([1, 2, 3]), torch.zeros(4), 7, 0.8, 40, **(st2 := _state(3, 4)))
    assert st2["step"].tolist() == [1, 1, 1]                                       # ops routes CPU tensors to the reference


def test_reference_k1_is_the_argmax_whatever_the_seed():
    lg = ko.rnd(2, 1025, scale=3.0, seed=2, dtype=torch.float32)
    for seed in (0, -1, SEED):
        st = _sample(ref.lm_sample_seeded, lg, [seed, seed + 1], k=1, eos=-1)
        assert st["tok"].tolist() == lg.argmax(1).tolist()


def test_reference_eos_bias_follows_the_rows_step():
    lg = torch.zeros(2, 16)
    eb = torch.tensor([-math.inf, 1e4])
    st = _state(2, 2)
    st["step"] = torch.tensor([1, 0])
    ref.lm_sample_seeded(lg, torch.tensor([5, 5]), eb, 3, 1.0, 16, **st)
    assert int(st["tok"][0]) == 3 and int(st["tok"][1]) != 3


@pytest.mark.parametrize("c", ko.SAMPLER_CASES, ids=lambda c: c.name)
def test_reference_keeps_the_lower_ids_at_the_kth_value(c):
    """the rank-probe cases of kernel_oracle.py: over 64 seeds the token is always one of the first
    k ids of the stable descending order, and the float64 model's argmax among them"""
    v = ko.sample_values(c.logits, 0.8, c.eos, c.eos_bias)
    order = torch.sort(v, descending=True, stable=True).indices[:c.k]
    inside = set(order.tolist())
    seeds = list(range(64))
    lg = c.logits.reshape(1, -1).repeat(8, 1)
    for s0 in range(0, 64, 8):
        st = _sample(ref.lm_sample_seeded, lg, seeds[s0:s0 + 8], k=c.k, eos=c.eos, eb=c.eos_bias)
        for b, t in enumerate(st["tok"].tolist()):
            assert t in inside, (c.name, t)
            sc = v[order].double().numpy() + S.philox_gumbel([seeds[s0 + b]], 0, order.numpy())[0]
            assert t == int(order[int(np.argmax(sc))])


def test_reference_row_is_the_same_alone_in_any_slot_and_next_to_other_rows():
    row = ko.rnd(1025, scale=3.0, seed=3, dtype=torch.float32)
    alone = _sample(ref.lm_sample_seeded, row[None], [SEED], step0=[2])
    for B in (3, 8):
        for slot in range(B):
            lg = ko.rnd(B, 1025, scale=3.0, seed=10 + B + slot, dtype=torch.float32)
            lg[slot] = row
            seeds = [100 + b for b in range(B)]
            seeds[slot] = SEED
            step0 = [1] * B
            step0[slot] = 2
            st = _sample(ref.lm_sample_seeded, lg, seeds, step0=step0)
            assert int(st["tok"][slot]) == int(alone["tok"][0]) == int(st["out"][2, slot])


# ------------------------------------------------------------------------------ generator, stub model
class StubModel:
    """logits = table[token]: exactly row-independent, whatever the batch (no GEMM blocking)"""

    def __init__(self, vocab, seed=0):
        self.table = ko.rnd(vocab, vocab, scale=3.0, seed=seed, dtype=torch.float32)
        self.prefills = []

    def alloc_cache(self, B, L):
        return torch.zeros(1, B, L, 1, 1), torch.zeros(1, B, L, 1, 1)

    def __call__(self, tokens, kc, vc, pos0, lens=None, decode=False):
        if not decode:
            self.prefills.append(tuple(tokens.shape))
        return self.table[tokens[:, -1]]


def stub_generator(**kw):
    gen = LMTextGenerator(TINY_LM, device="cpu", seed=3, noise="philox", **kw)
    gen.model = StubModel(TINY_LM.vocab)
    return gen


P1, P2, P3 = [256, 72, 105], [256, 65], [256, 80, 81, 82, 83]


def test_a_prompts_ids_do_not_depend_on_bucket_slot_or_neighbours():
    gen = stub_generator(max_batch=8)
    alone = gen.generate_ids_batch([P1], 4, 12, seeds=[11])[0]
    assert len(alone) <= 12 and gen.generate_ids_batch([P1], 4, 12, seeds=[12])[0] != alone
    for n in (2, 3, 4, 5, 8):
        for slot in range(n):
            prompts = [(P2, P3)[i % 2] for i in range(n)]
            seeds = [20 + i for i in range(n)]
            prompts[slot], seeds[slot] = P1, 11
            assert gen.generate_ids_batch(prompts, 4, 12, seeds=seeds)[slot] == alone, (n, slot)
    assert sorted(gen.buckets) == [1, 2, 4, 8]


def test_three_requests_run_in_bucket_four_with_one_padded_prefill():
    gen = stub_generator(max_batch=8)
    a = gen.generate_ids_batch([P1, P2, P3], 4, 12, seeds=[1, 2, 3])
    assert sorted(gen.buckets) == [4] and gen.buckets[4].kc.shape[1] == 4
    assert gen.model.prefills == [(4, len(P3) - 1)]
    assert a == gen.generate_ids_batch([P1, P2, P3], 4, 12, seeds=[1, 2, 3])       # same seeds, same ids
    capped = stub_generator(max_batch=3)
    assert capped.bucket_sizes == (1, 2, 3)
    assert capped.generate_ids_batch([P1, P2, P3], 4, 12, seeds=[1, 2, 3]) == a
    with pytest.raises(ValueError, match="max_batch"):
        capped.generate_ids_batch([P1] * 4, 4, 12)


def test_default_seeds_count_one_call_number_per_sequence():
    gen, one = stub_generator(max_batch=4), stub_generator(max_batch=4)
    batch = gen.generate_ids_batch([P1, P2, P3], 4, 12)
    assert gen.calls == 3
    assert batch == [one.generate_ids(p, 4, 12) for p in (P1, P2, P3)]            # bucket 1, calls 0, 1, 2
    assert batch[0] == one.generate_ids_batch([P1], 4, 12, seeds=[3 * 1000003 + 0])[0]
    texts = stub_generator(max_batch=4).generate_texts(["Hi", "A"], 4, 12)
    assert len(texts) == 2 and all(isinstance(t, str) for t in texts)


def test_token_budget_and_eos_cut_hold_per_row():
    gen = stub_generator(max_batch=4)
    eos = gen.tok.eos
    gen.model.table[:, eos] = -40.0
    gen.model.table[65, eos] = 80.0                  # after token 65 the next one is EOS, once allowed
    gen.model.table[:, 65] += 3.0
    rows = gen.generate_ids_batch([P1, P2, P3, P2], 3, 10, seeds=[1, 2, 3, 4])
    raw = gen.buckets[4].out[:10].t().tolist()
    for got, full in zip(rows, raw):
        assert len(got) <= 10 and eos not in got
        assert eos not in full[:3]                   # min_new: no EOS in the first 3 tokens of any row
        assert got == (full[:full.index(eos)] if eos in full else full)
    assert len({len(r) for r in rows}) > 1 and any(3 <= len(r) < 10 for r in rows)   # rows end at their own EOS
    assert len(gen.generate_ids_batch([P1], 0, 500, seeds=[1])[0]) <= gen.max_new_cap


def test_table_noise_refuses_the_batch_entry_points():
    gen = LMTextGenerator(TINY_LM, device="cpu", seed=0)
    with pytest.raises(ValueError, match="philox"):
        gen.generate_ids_batch([P1], 4, 12)
    with pytest.raises(ValueError, match="philox"):
        gen.generate_texts(["a"], 4, 12)
    with pytest.raises(ValueError, match="philox"):
        LMTextGenerator(TINY_LM, device="cpu", max_batch=2)
    with pytest.raises(ValueError, match="table, philox"):
        LMTextGenerator(TINY_LM, device="cpu", noise="gumbel")
    assert not hasattr(LMTextGenerator(TINY_LM, device="cpu", noise="philox"), "noise")   # no table


def test_default_path_gives_the_parent_commits_ids():
    gen = LMTextGenerator(TINY_LM, device="cpu", seed=0)
    for rec in json.load(open(os.path.join(GOLDEN, "lm_default_ids.json"))):
        assert gen.generate_ids(gen.tok.encode(rec["prompt"]), rec["min_new"], rec["max_new"]) == rec["ids"]


def test_real_model_on_the_cpu_batches_and_repeats():
    gen = LMTextGenerator(TINY_LM, device="cpu", seed=0, noise="philox", max_batch=4)
    tok = ByteTokenizer()
    prompts = [tok.encode("The silver dunes"), tok.encode("A fox"), tok.encode("In the quiet harbor, bells")]
    a = gen.generate_ids_batch(prompts, 4, 8, seeds=[1, 2, 3])
    assert a == gen.generate_ids_batch(prompts, 4, 8, seeds=[1, 2, 3])
    assert all(4 <= len(r) <= 8 for r in a)


# ------------------------------------------------------------------------------ rooms
class FakeLM:
    def __init__(self, delay=0.0, fail=False):
        self.calls, self.delay, self.fail = [], delay, fail

    def generate_texts(self, prompts, min_new, max_new):
        self.calls.append(list(prompts))
        time.sleep(self.delay)
        if self.fail:
            raise RuntimeError("lm down")
        return ["" if p.startswith("empty") else f" Story of {p} went on and on. Then it ended well. More" for p in prompts]


class Fallback(PromptGenerator):
    def generate(self, seed, is_seed):
        return f"fallback for {seed}."


def _rooms(front, names):
    res, errs = {}, {}

    def room(name):
        try:
            res[name] = front.generate(name, True)
        except BaseException as e:  # noqa: BLE001
            errs[name] = e

    ts = [threading.Thread(target=room, args=(n,)) for n in names]
    for t in ts:
        t.start()
    for t in ts:
        t.join(30)
    return res, errs


def test_generate_many_post_processes_and_falls_back_per_row():
    pg = LMPromptGenerator(FakeLM(), fallback=Fallback())
    out = pg.generate_many(["room a", "empty b", "room c"], [True, False, True])
    assert out == ["Story of room a went on and on. Then it ended well.", "fallback for empty b.",
                   "Story of room c went on and on. Then it ended well."]
    assert pg.lm.calls == [["room a", "empty b", "room c"]]


def test_eight_rooms_make_batches_of_at_most_four_and_get_their_own_rows():
    lm = FakeLM(delay=0.02)
    front = BatchingPromptGenerator(LMPromptGenerator(lm, fallback=Fallback()), max_batch=4, window_s=0.05)
    names = [f"room {i}" for i in range(8)]
    res, errs = _rooms(front, names)
    assert not errs and sorted(res) == sorted(names)
    for n in names:
        assert res[n] == f"Story of {n} went on and on. Then it ended well."
    assert sum(front.batch_sizes) == 8 and max(front.batch_sizes) <= 4 and len(front.batch_sizes) < 8
    assert [len(c) for c in lm.calls] == front.batch_sizes


def test_one_caller_and_no_window_does_not_wait():
    front = BatchingPromptGenerator(LMPromptGenerator(FakeLM(), fallback=Fallback()), max_batch=4, window_s=0.0)
    t0 = time.perf_counter()
    assert front.generate("empty room", True) == "fallback for empty room."
    assert time.perf_counter() - t0 < 0.04 and front.batch_sizes == [1]


def test_an_inner_exception_reaches_every_room_of_the_batch():
    front = BatchingPromptGenerator(LMPromptGenerator(FakeLM(fail=True)), max_batch=4, window_s=0.05)
    res, errs = _rooms(front, ["a", "b", "c"])
    assert not res and sorted(errs) == ["a", "b", "c"]
    assert all(isinstance(e, RuntimeError) and "lm down" in str(e) for e in errs.values())


# ------------------------------------------------------------------------------ flags
def test_lm_flags_parse_from_arguments_and_environment():
    assert (Config().model.lm_noise, Config().model.lm_batch_max, Config().model.lm_batch_window_ms) == ("table", 1, 50.0)
    cfg = Config.from_args(["--lm_noise", "philox", "--lm_batch_max", "8", "--lm_batch_window_ms", "20"], base=Config())
    assert (cfg.model.lm_noise, cfg.model.lm_batch_max, cfg.model.lm_batch_window_ms) == ("philox", 8, 20.0)
    env = Config.from_env({"CASSMANTLE_LM_NOISE": "philox", "CASSMANTLE_LM_BATCH_MAX": "4"})
    assert env.model.lm_noise == "philox" and env.model.lm_batch_max == 4
    assert Config.from_args(["--model.lm_noise=philox"], base=Config()).model.lm_noise == "philox"


def test_factory_builds_the_batching_front_and_refuses_bad_flags():
    cfg = Config()
    cfg.model.prompt_generator, cfg.model.lm_model = "lm", "tiny-lm"
    plain = build_prompt_generator(cfg, device="cpu")
    assert isinstance(plain, LMPromptGenerator) and plain.lm.noise_mode == "table"
    cfg.model.lm_noise, cfg.model.lm_batch_max, cfg.game.num_rooms = "philox", 4, 1
    front = build_prompt_generator(cfg, device="cpu")
    assert isinstance(front, BatchingPromptGenerator) and front.max_batch == 4 and front.window_s == 0.0
    assert front.inner.lm.noise_mode == "philox" and front.inner.lm.max_batch == 4
    assert isinstance(front.generate("Chapter One: The Lantern", True), str)
    cfg.game.num_rooms = 8
    assert build_prompt_generator(cfg, device="cpu").window_s == pytest.approx(0.05)
    cfg.model.lm_batch_max = 1
    assert isinstance(build_prompt_generator(cfg, device="cpu"), LMPromptGenerator)
    cfg.model.lm_noise = "gumbel"
    with pytest.raises(ValueError, match="table, philox"):
        build_prompt_generator(cfg, device="cpu")
    cfg.model.lm_noise, cfg.model.lm_batch_max = "table", 4
    with pytest.raises(ValueError, match="lm_noise=philox"):
        build_prompt_generator(cfg, device="cpu")
    cfg.model.lm_noise, cfg.model.lm_batch_max = "philox", 9
    with pytest.raises(ValueError, match="1..8"):
        build_prompt_generator(cfg, device="cpu")
