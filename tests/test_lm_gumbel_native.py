"""The LM sampler's noise (ops/csrc/philox_gumbel.h, the text lm_sample_seeded_kernel compiles) as
a host program: tests/native/philox_gumbel_host.cpp built plain and with ASan + UBSan on the host,
with the builds and the runner of test_sampler_noise_native.py.  Its Philox words equal the numpy
model's (models/schedulers.py philox_gumbel_words) exactly and g agrees with the float64 model
within 2e-6 * max(1, |g|): the tolerance the sampler's decision margin is derived from
(1e-4 >= 2 * (17.33 * 2e-6 + 2^-18)).  Nothing runs on a GPU."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from cassmantle_amd.models import schedulers as S
from test_jpeg_entropy_native import CSRC, CXX, OUT, ROOT, SANITIZE
from test_sampler_noise_native import run

DRIVER = os.path.join(ROOT, "tests", "native", "philox_gumbel_host.cpp")
BUILDS = [("philox_gumbel_plain", []), ("philox_gumbel_asan", SANITIZE)]
GUMBEL_TOL = 2e-6
SEEDS = [0, 1, -1, 2 ** 63 - 1, -2 ** 63, -2 ** 63 + 1, 0x1234_5678_9ABC_DEF0]
STEPS = [0, 1, 95, 2 ** 32 - 1]
IDS = list(range(8)) + [31999, 2 ** 17 - 1]
EDGE_K = [0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 - 2, 2 ** 24 - 1]


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [DRIVER, os.path.join(CSRC, "philox_gumbel.h"), os.path.join(CSRC, "philox_normal.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-I", CSRC, *flags, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.all(np.abs(got - want) <= GUMBEL_TOL * np.maximum(1.0, np.abs(want)))


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_words_and_gumbels_match_the_model(name, flags, tmp_path):
    grid = [(s, st, i) for s in SEEDS for st in STEPS for i in IDS]
    out = run(_build(name, flags), [f"G {s} {st} {i}" for s, st, i in grid], tmp_path)
    worst = 0.0
    for (s, st, i), ln in zip(grid, out):
        f = ln.split()
        word = int(S.philox4x32((i >> 2, st, 0, 0), S.seed_key(s))[i & 3])
        assert int(f[0], 16) == word == int(S.philox_gumbel_words([s], st, [i])[0, 0]), (s, st, i)
        g = S.philox_gumbel([s], st, [i])[0, 0]
        assert f[1] == f[2]
        assert close(float(f[1]), g), (s, st, i, f[1], g)
        worst = max(worst, abs(float(f[1]) - g) / max(1.0, abs(g)))
    print(f"{name}: worst |g - model| / max(1, |g|) over {len(grid)} values: {worst:.3e}")


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_gumbel_at_the_edges_of_its_word(name, flags, tmp_path):
    """u next to 0 (the smallest g), around u = 1/2 where ln u changes from logf to log1pf of the
    complement, and u next to 1 (the largest g); the range of the contract"""
    words = [k << 8 | low for k in EDGE_K for low in (0x00, 0xA5, 0xFF)]
    out = run(_build(name, flags), [f"W {w:x}" for w in words], tmp_path)
    for w, ln in zip(words, out):
        want = S.gumbel_of_words(np.asarray([w], dtype=np.uint32))[0]
        assert close(float(ln), want), (hex(w), ln, want)
        assert -2.853 <= float(ln) <= 17.329
    lo, hi = S.gumbel_of_words(np.asarray([0, 0xFFFFFFFF], dtype=np.uint32))
    assert abs(lo + 2.8528) < 1e-3 and abs(hi - 17.3287) < 1e-3
