"""The table builder of the optimised Huffman tables (ops/csrc/jpeg_huff_opt.h) and the counting
sink of the per-block coder (ops/csrc/jpeg_entropy_blk.h), the text the kernels compile, as a host
program: tests/native/jpeg_huff_opt_host.cpp built plain and with ASan + UBSan on the host, a
stand-alone executable.  On 2000 fixed-seed frequency vectors (and all-zero, one-symbol and
Fibonacci-skewed ones) its tables are jpeg_format.optimal_table's, on the coefficients of PIL's
optimised streams its histogram is jpeg_format.symbol_counts and its DHT segment the stream's,
with no sanitizer report.  And the build-level guard: jpeg.hip compiles for gfx950 and the two new
kernels use no scratch.  Nothing runs on a GPU."""
from __future__ import annotations

import os
import re
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_huffman_cases as hc
from cassmantle_amd.ops import jpeg_format as jf
from test_jpeg_build import HIPCC
from test_jpeg_entropy_native import CSRC, CXX, OUT, ROOT, SANITIZE

DRIVER = os.path.join(ROOT, "tests", "native", "jpeg_huff_opt_host.cpp")
KERNELS = ("jpeg_huff_count_kernel", "jpeg_huff_build_kernel")


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [DRIVER, os.path.join(CSRC, "jpeg_huff_opt.h"), os.path.join(CSRC, "jpeg_entropy_blk.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    # a plain C++ translation unit: the routines' qualifier macros expand to nothing
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-I", CSRC, *flags, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def coefficient_cases():
    """(name, coef, restart_mcus): the oracle streams' coefficients without restart markers, and the
    encoder's own with them"""
    out = [(name, coef, 0) for name, st, coef in hc.oracle()]
    img = jc.noise(24, 40)
    for s in jc.SAMPLINGS:
        coef = jf.coefficients(img, 95, s)
        for r in jc.restart_values(24, 40, s, with_zero=False):
            out.append((f"noise_24x40-{s}-r{r}", coef, r))
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    vectors = hc.frequency_vectors()
    coefs = coefficient_cases()
    path = tmp_path_factory.mktemp("jpeg_huff_opt") / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"JHO1" + struct.pack("<I", len(vectors) + len(coefs)))
        for v in vectors:
            f.write(struct.pack("<I", 0) + v.astype("<u4").tobytes())
        for _, coef, r in coefs:
            mcus, nb, _ = coef.shape
            f.write(struct.pack("<4I", 1, nb, mcus, min(r, mcus) if r else mcus))
            f.write(np.ascontiguousarray(coef).astype("<i2").tobytes())
    return vectors, coefs, str(path), [_expected(v) + (max(jf.code_sizes(v)) > 16,) for v in vectors]


def _expected(freq):
    """(bad, bits, vals, words[256]) of the numpy model"""
    try:
        bits, vals = jf.optimal_table(freq)
    except ValueError:
        return 1, None, None, None
    words = np.zeros(256, dtype=np.uint32)
    for sym, (code, length) in jf._huff_codes(bits, vals).items():
        words[sym] = (length << 16) | code
    return 0, bits, vals, words


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", [("jpeg_huff_opt_plain", []), ("jpeg_huff_opt_asan", SANITIZE)])
def test_host_program_builds_the_reference_tables(name, flags, cases, tmp_path):
    vectors, coefs, path, expected = cases
    assert len(vectors) >= 2000
    exe = _build(name, flags)
    out = str(tmp_path / "out.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(vectors) + len(coefs)
    assert int(words[5]) == jf.block_bits_bound_optimized(), r.stdout
    raw = open(out, "rb").read()
    pos = 0
    refused = limited = 0
    for i, v in enumerate(vectors):
        bad, n = struct.unpack_from("<2I", raw, pos)
        bits = tuple(raw[pos + 8: pos + 24])
        vals = tuple(raw[pos + 24: pos + 24 + n])
        got = np.frombuffer(raw, dtype="<u4", count=256, offset=pos + 24 + n)
        pos += 24 + n + 1024
        ebad, ebits, evals, ewords, long_codes = expected[i]
        assert bad == ebad, i
        refused += bad
        if not bad:
            assert (bits, vals) == (ebits, evals), i
            assert np.array_equal(got, ewords), i
            limited += long_codes
    assert refused == 2 and limited >= 4                 # the 40-symbol Fibonacci vectors; the 30-symbol ones
    for cname, coef, rst in coefs:
        hist = np.frombuffer(raw, dtype="<u4", count=544, offset=pos).astype(np.int64)
        bad, n = struct.unpack_from("<2I", raw, pos + 2176)
        dht = raw[pos + 2184: pos + 2184 + n]
        got = np.frombuffer(raw, dtype="<u4", count=544, offset=pos + 2184 + n)
        pos += 2184 + n + 2176
        freq = jf.symbol_counts(coef, rst)
        for t, base in enumerate(jf.HUFF_BASES):
            k = 16 if t < 2 else 256
            assert np.array_equal(hist[base: base + k], freq[t, :k]), (cname, t)
        tables = jf.optimal_tables(freq)
        assert bad == 0 and dht == jf.dht_segment(tables), cname
        assert np.array_equal(got.astype(np.int64), jf.huff_table(tables).astype(np.int64)), cname
    assert pos == len(raw)
    assert int(words[3]) == refused


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_new_kernels_build_without_scratch():
    out = os.path.join(ROOT, "build", "regcheck", "jpeg_huff.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-mllvm",
                        "-pragma-unroll-threshold=100000", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "jpeg.hip"), "-o", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    s = open(out).read()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_count:\s+(\d+)", s, re.S):
        pr = re.search(r"private_segment_fixed_size:\s+(\d+)", m.group(2))
        assert pr is not None, m.group(1)
        seen[m.group(1)] = (int(pr.group(1)), int(m.group(3)))
    for k in KERNELS:
        hit = [n for n in seen if k in n]
        assert hit, (k, sorted(seen))
        print({n: seen[n] for n in hit})
        assert all(seen[n][0] == 0 for n in hit), {n: seen[n] for n in hit}
