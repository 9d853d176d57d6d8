"""Where a table-noise prompt call of the local LM spends its time, without subtracting one call from another.

    python tools/probe_lm_call.py [--parent /path/to/built/parent] [--calls 6]

tools/bench_lm.py derives its decode time from a --new-token call minus a 1-token call minus the host time of
the noise table, so whatever else differs between those calls lands in it.  This script times single calls
directly: device events at the call's entry (the device is idle there), around the prefill, before the first
and after the last graph replay, and the host clock at entry and return.  One JSON line: per 96-token call
`call_ms` (host, entry to return), `device_ms` (entry to the end of the last replay on the device),
`prefill_ms` and `replays_ms` (device), and `tail_ms = call_ms - device_ms`, the time the host needs to notice
that the device has finished and to read the tokens back.  Works on the parent's generator too (--parent
imports the package from another built checkout), which is how the two trees are compared.
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--new", type=int, default=96)
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit to import the package from")
    a = ap.parse_args()
    root = os.path.abspath(a.parent) if a.parent else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)

    import torch
    from cassmantle_amd.models.lm import LM_CONFIGS, LMTextGenerator

    g = LMTextGenerator(LM_CONFIGS[a.model], device="cuda", max_new_cap=max(a.new, 8))
    prompt = [256] + [65 + (i % 26) for i in range(a.prompt_len - 1)]
    rec = {}

    def mark(name):
        rec[name] = torch.cuda.Event(enable_timing=True)
        rec[name].record()

    g.generate_ids(prompt, a.new, a.new)          # warm-up + graph capture
    torch.cuda.synchronize()
    forward, replay = g.model.forward, torch.cuda.CUDAGraph.replay

    def timed_forward(*args, **kw):               # the one eager forward of a call is its prefill
        if kw.get("decode"):
            return forward(*args, **kw)
        mark("pre0")
        out = forward(*args, **kw)
        mark("pre1")
        return out

    def timed_replay(self):
        if "first" not in rec:
            mark("first")
        replay(self)
        mark("last")

    g.model.forward, torch.cuda.CUDAGraph.replay = timed_forward, timed_replay
    rows = []
    for _ in range(a.calls):
        rec.clear()
        torch.cuda.synchronize()
        mark("entry")
        t0 = time.perf_counter()
        g.generate_ids(prompt, a.new, a.new)
        call_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        device_ms = rec["entry"].elapsed_time(rec["last"])
        rows.append({"call_ms": call_ms, "device_ms": device_ms, "tail_ms": call_ms - device_ms,
                     "prefill_ms": rec["pre0"].elapsed_time(rec["pre1"]),
                     "replays_ms": rec["first"].elapsed_time(rec["last"])})
    print(json.dumps({"tree": "parent" if a.parent else "this", "model": a.model, "new_tokens": a.new,
                      **{k: [round(r[k], 2) for r in rows] for k in rows[0]}}))


if __name__ == "__main__":
    main()
