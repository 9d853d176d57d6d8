"""The samplers' noise (ops/csrc/philox_normal.h, the text the latent-step kernel compiles) as a
host program: tests/native/philox_normal_host.cpp built plain and with ASan + UBSan on the host.
Its Philox words equal the numpy model's (models/schedulers.py) exactly, and its normals agree
with the model's float64 Box-Muller within 1e-5 * max(1, |z|): the angle is reduced exactly and
rounded once (<= 2^-22 rad, times r <= 5.9), logf / log1pf / sqrtf / sinf / cosf add a few ulp,
together under 4e-6.  Nothing runs on a GPU."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from cassmantle_amd.models import schedulers as S
from test_jpeg_entropy_native import CSRC, CXX, OUT, ROOT, SANITIZE

DRIVER = os.path.join(ROOT, "tests", "native", "philox_normal_host.cpp")
BUILDS = [("philox_normal_plain", []), ("philox_normal_asan", SANITIZE)]
SEEDS = [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 0x1234_5678_9ABC_DEF0, 42]
STEPS = [0, 1, 50, 1000, 2 ** 32 - 1]
PIXELS = [0, 1, 2, 4095, 65535, 2 ** 31, 2 ** 32 - 1]
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [DRIVER, os.path.join(CSRC, "philox_normal.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-I", CSRC, *flags, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, lines, tmp_path):
    path = tmp_path / "requests.txt"
    path.write_text("".join(ln + "\n" for ln in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.all(np.abs(got - want) <= 1e-5 * np.maximum(1.0, np.abs(want)))


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_known_answers(name, flags, tmp_path):
    lines = ["K " + " ".join(f"{v:x}" for v in c + k) for c, k, _ in KNOWN]
    assert run(_build(name, flags), lines, tmp_path) == [w for _, _, w in KNOWN]


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_words_and_normals_match_the_model(name, flags, tmp_path):
    grid = [(s, st, p) for s in SEEDS for st in STEPS for p in PIXELS]
    out = run(_build(name, flags), [f"N {s} {st} {p}" for s, st, p in grid], tmp_path)
    for (s, st, p), ln in zip(grid, out):
        f = ln.split()
        lo, hi = S.seed_key(s)
        words = S.philox4x32((p, st, 0, 0), (lo, hi))
        assert [int(w, 16) for w in f[:4]] == words.tolist(), (s, st, p)
        z = S.philox_normal([s], st, np.asarray([p]))[0, 0]
        assert close([float(v) for v in f[4:]], z), (s, st, p, f[4:], z)


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_box_muller_at_the_edges_of_its_words(name, flags, tmp_path):
    """u near 0 (the largest radius), around u = 1/2 where the evaluation changes from ln u to
    log1p(u - 1), u next to 1 (the smallest radius), and every quadrant boundary of the angle."""
    ks = [0, 1, 2, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 - 2, 2 ** 24 - 1]
    ks += [q * 2 ** 22 + d for q in (1, 2, 3) for d in (-1, 0)] + [123457, 9999999]
    pairs = [(k0 << 8 | 0xA5, k1 << 8 | 0x5A) for k0 in ks for k1 in ks]
    out = run(_build(name, flags), [f"B {a:x} {b:x}" for a, b in pairs], tmp_path)
    for (a, b), ln in zip(pairs, out):
        u0, u1 = ((a >> 8) + 0.5) * 2.0 ** -24, ((b >> 8) + 0.5) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u0))
        want = [r * np.cos(2 * np.pi * u1), r * np.sin(2 * np.pi * u1)]
        assert close([float(v) for v in ln.split()], want), (hex(a), hex(b), ln, want)
        assert abs(float(ln.split()[0])) <= 5.9 and abs(float(ln.split()[1])) <= 5.9
