"""Decode throughput of the local prompt LM (random-init weights, hipGraph decode loop).

    python tools/bench_lm.py --model mistral-7b --new 96 --prompt-len 64
    python tools/bench_lm.py --model mistral-7b --new 96 --prompt-len 64 --noise philox --batch 8
    python tools/bench_lm.py --model mistral-7b --new 96 --prompt-len 64 --parent /path/to/built/parent
    python tools/bench_lm.py --model mistral-7b --new 96 --prompt-len 64 --noise philox --batch 8 --weights fp8

Prints one JSON line.  --weights bf16 | fp8 (this tree only): the projections as they are or quantised
to weight-only fp8 at load; the record gains the weight bytes a step streams, the TB/s they imply
and the quantisation time.  Without --batch / --noise / --parent / --weights: batch 1 with the noise table, ms/token,
tokens/s and the HBM-bandwidth bound (weights bytes / 8 TB/s).  With one of them the record holds
what batching changes: decode ms per step, tokens/s summed over the batch, prefill ms, the host ms a
call spends before its first launch (the noise table, in the table path) and the whole call.
--parent imports the package from another built checkout of the parent commit, so both trees are
measured by this one script.  This tree's generator times its own host part (``host_ms``) in both
noise modes; the parent's table path has no timer, so there the script stamps it (below).
"""
import argparse
import json
import os
import sys
import time


def stamp_table_upload(g):
    """The parent's table path only, whose code is fixed: makes ``g.max_new_cap`` record when it is
    read.  Its generate_ids reads it once on entry and next right after the noise table is drawn
    and uploaded, so the second stamp of a call ends its host part."""
    stamps = []

    class Stamped(type(g)):
        @property
        def max_new_cap(self):
            stamps.append(time.perf_counter())
            return self._cap

    g._cap = g.__dict__.pop("max_new_cap")
    g.__class__ = Stamped
    return stamps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--new", type=int, default=96)
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--batch", type=int, default=None, help="sequences decoded as one batch (needs --noise philox above 1)")
    ap.add_argument("--noise", choices=("table", "philox"), default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit to import the package from")
    ap.add_argument("--weights", choices=("bf16", "fp8"), default=None,
                    help="projection weights: bf16, or weight-only fp8 quantised at load (the record gains weight_bytes, "
                         "weight_tb_per_s and quantize_ms)")
    a = ap.parse_args()
    extended = a.batch is not None or a.noise is not None or a.parent is not None or a.weights is not None
    root = os.path.abspath(a.parent) if a.parent else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)

    import torch
    from cassmantle_amd.models.lm import LM_CONFIGS, LMTextGenerator

    B, noise = a.batch or 1, a.noise or "table"
    cfg = LM_CONFIGS[a.model]
    kw = {"noise": noise, "max_batch": B} if extended else {}
    if a.weights is not None:
        kw["weight_dtype"] = a.weights
    t0 = time.time()
    g = LMTextGenerator(cfg, device="cuda", use_graphs=not a.no_graphs, max_new_cap=max(a.new, 8), **kw)
    torch.cuda.synchronize()
    init_s = time.time() - t0
    params = sum(p.numel() for p in g.model.parameters())
    prompts = [[256] + [65 + ((i + 3 * b) % 26) for i in range(a.prompt_len - 1)] for b in range(B)]
    host = []
    stamps = stamp_table_upload(g) if a.parent and noise == "table" else None

    def call(n_new):
        t = time.perf_counter()
        if noise == "philox":
            g.generate_ids_batch(prompts, n_new, n_new)
        else:
            g.generate_ids(prompts[0], n_new, n_new)
        if stamps is None:
            host.append(g.host_ms)
        else:
            host.append((stamps[1] - t) * 1e3)
            del stamps[:]

    call(a.new)          # warmup + graph capture
    torch.cuda.synchronize()
    # prefill alone
    t0 = time.time()
    for _ in range(a.reps):
        call(1)
    torch.cuda.synchronize()
    t_one = (time.time() - t0) / a.reps
    host_one = sum(host[-a.reps:]) / a.reps
    t0 = time.time()
    for _ in range(a.reps):
        call(a.new)
    torch.cuda.synchronize()
    t_all = (time.time() - t0) / a.reps
    host_all = sum(host[-a.reps:]) / a.reps
    # the decode steps between a 1-token and a --new-token call, without the host part that grows
    # with --new (the noise table)
    ms_tok = ((t_all - t_one) * 1e3 - (host_all - host_one)) / max(1, a.new - 1) if extended \
        else (t_all - t_one) / max(1, a.new - 1) * 1e3
    bound_ms = params * 2 / 8.0e12 * 1e3
    if not extended:
        print(json.dumps({"model": cfg.name, "params": params, "init_s": round(init_s, 2),
                          "prompt_len": a.prompt_len, "new_tokens": a.new,
                          "prefill_plus_1_ms": round(t_one * 1e3, 2), "decode_ms_per_token": round(ms_tok, 3),
                          "decode_tokens_per_s": round(1e3 / ms_tok, 1), "hbm_bound_ms_per_token": round(bound_ms, 3),
                          "graphs": not a.no_graphs}))
        return
    rec = {"model": cfg.name, "params": params, "tree": "parent" if a.parent else "this", "noise": noise,
           "batch": B, "init_s": round(init_s, 2), "prompt_len": a.prompt_len, "new_tokens": a.new,
           "decode_ms_per_step": round(ms_tok, 3), "decode_tokens_per_s": round(B * 1e3 / ms_tok, 1),
           "prefill_ms": round(t_one * 1e3 - host_one - ms_tok, 2),
           "host_ms_before_first_launch": round(host_all, 2), "call_ms": round(t_all * 1e3, 2),
           "call_ms_per_sequence": round(t_all * 1e3 / B, 2),
           "hbm_bound_ms_per_token": round(bound_ms, 3), "graphs": not a.no_graphs}
    if a.weights is not None:
        # the bytes a decode step streams (every projection; codes and scales when quantised) and the
        # rate they imply; with fp8 "params" counts what is left in bf16 (embed, the gains)
        wb = g.model.weight_bytes()
        rec.update({"weights": a.weights, "weight_bytes": wb, "weight_tb_per_s": round(wb / (ms_tok * 1e-3) / 1e12, 3),
                    "quantize_ms": round(g.quant_ms, 1), "hbm_bound_ms_per_token": round(wb / 8.0e12 * 1e3, 3)})
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
