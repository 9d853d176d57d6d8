"""The samplers of models/schedulers.py on the GPU: what the noise costs in the latent-step kernel,
and what fewer evaluations buy per generation.

* kernel: the device time (HIP events) of 200 ``ops.latent_step`` launches at the SD-1.5 shape
  (4 x 64 x 64 x 4 latents, CFG), eagerly launched and as one captured graph of 200 nodes, for
  - ``parent``: the kernel of a built checkout of the parent commit (``--parent PATH``; the
    yardstick),
  - ``deterministic``: a deterministic row without seeds (the same kernel in this tree),
  - ``seeded_deterministic``: a deterministic row of a plan with seeds (the per-pixel kernel, no
    Philox),
  - ``noise``: a stochastic row (the per-pixel kernel with Philox + Box-Muller),
  each in a process of its own, interleaved ``--reps`` times.
* generation: seconds per 4-image SD-1.5 generation (text encode, denoise, VAE decode; random-init
  weights) for pndm 50, dpmpp_2m_karras 20, dpmpp_2m_sde_karras 20 and euler_a 30 steps,
  interleaved ``--reps`` times after a warm-up of each.

One JSON line per record.

    python tools/bench_samplers.py [--parent PATH] [--reps 2] [--out profiles/samplers.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = 200
GENERATIONS = [("pndm", 50), ("dpmpp_2m_karras", 20), ("dpmpp_2m_sde_karras", 20), ("euler_a", 30)]


def kernel_child(tree: str, mode: str) -> None:
    """Runs in a process of its own with ``tree`` (this checkout or the parent's) first on the path."""
    sys.path.insert(0, tree)
    import torch
    from cassmantle_amd import ops
    from cassmantle_amd.models import schedulers as S
    ops.set_mode("hip")
    dev = "cuda"
    B, h = 4, 64
    plan = S.make_plan("euler_a" if mode == "noise" else "pndm", 50, 7.5)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, h, h, 4, generator=g) * plan.init_sigma).to(dev)
    hist, xs = torch.zeros(4, B, h, h, 4, device=dev), torch.zeros(B, h, h, 4, device=dev)
    unet_in = torch.zeros(2 * B, h, h, 8, device=dev, dtype=torch.bfloat16)
    eps = torch.randn(2 * B, h, h, 4, generator=g).to(torch.bfloat16).to(dev)
    table = plan.table.copy()
    table[5, 4] = 0.9                     # ax < 1: the same row applied thousands of times stays finite
    coef = torch.from_numpy(table).to(dev)
    step = torch.full((1,), 5, dtype=torch.int32, device=dev)       # a full multistep row of either plan
    kw = {}
    if mode in ("noise", "seeded_deterministic"):
        kw["noise_seeds"] = torch.arange(B, dtype=torch.int64, device=dev)

    def launches():
        for _ in range(LAUNCHES):
            ops.latent_step(eps, x, hist, xs, coef, step, unet_in, True, **kw)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        launches()                                                  # warm-up
        eager = min(timed(launches) for _ in range(3))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            launches()
        graph.replay()
        replay = min(timed(graph.replay) for _ in range(3))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all())
    print(json.dumps({"kind": "kernel", "mode": mode, "launches": LAUNCHES, "shape": [B, h, h, 4], "cfg": True,
                      "eager_ms": round(eager, 4), "graph_ms": round(replay, 4),
                      "graph_us_per_launch": round(1e3 * replay / LAUNCHES, 3)}))


def generations(reps: int, emit) -> None:
    sys.path.insert(0, ROOT)
    import torch
    from cassmantle_amd import ops
    from cassmantle_amd.pipeline import SPECS, StableDiffusion
    ops.set_mode("hip")
    sd = StableDiffusion(SPECS["sd15"], device="cuda:0", use_graphs=True)
    prompts = [f"A gothic style piece depicting the following: a silent lantern tower, view {i}." for i in range(4)]
    negative = "blurry, distorted, fake, abstract, negative"

    def one(name, steps, seed0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sd.generate_tensor(prompts, negative, [seed0 + i for i in range(4)], steps=steps, scheduler=name)
        torch.cuda.synchronize()
        assert bool(sd.last_finite.cpu()[0])
        return time.perf_counter() - t0

    for name, steps in GENERATIONS:                   # warm-up of each: graph capture, tuning tables
        one(name, steps, 0)
        one(name, steps, 4)
    for rep in range(reps):
        for name, steps in GENERATIONS:
            sec = one(name, steps, 100 + 10 * rep)
            emit({"kind": "generation", "model": "sd15", "images": 4, "scheduler": name, "steps": steps,
                  "evals": steps + (name == "pndm"), "rep": rep, "seconds": round(sec, 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (kernel yardstick)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samplers.jsonl"))
    ap.add_argument("--skip-generations", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("TREE", "MODE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kernel_child(*a.child)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    modes = [("deterministic", ROOT), ("seeded_deterministic", ROOT), ("noise", ROOT)]
    if a.parent:
        modes.insert(0, ("parent", os.path.abspath(a.parent)))
    for rep in range(a.reps):
        for mode, tree in modes:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, mode], capture_output=True,
                               text=True, timeout=300, cwd=tree)
            if r.returncode != 0:
                raise SystemExit(f"kernel run {mode} failed ({r.returncode}):\n{r.stderr[-3000:]}")
            emit(dict(json.loads(r.stdout.strip().splitlines()[-1]), rep=rep))
    if not a.skip_generations:
        generations(a.reps, emit)
    out.close()


if __name__ == "__main__":
    main()
