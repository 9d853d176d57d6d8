"""The arithmetic of the libjpeg forward contract (ops/csrc/jpeg_fdct_lj.h, the text
jpeg_transform_lj_kernel compiles) as a host program: tests/native/jpeg_fdct_lj_host.cpp built plain
and with ASan + UBSan on the host, a stand-alone executable that transforms every image of
jpeg_libjpeg_cases.py MCU by MCU.  The pixels are a heap block of exactly the image's size, so a
source coordinate outside the image is a sanitizer report, and UBSan watches the 32-bit arithmetic.
Its coefficients are the numpy model's, and the four DHT segments it writes for their optimised
tables (the per-table layout of ops/csrc/jpeg_huff_opt.h) are the model's.  The new kernels build
without scratch.  Nothing runs on a GPU, and nothing is loaded into Python."""
from __future__ import annotations

import os
import re
import struct
import subprocess

import numpy as np
import pytest

import jpeg_libjpeg_cases as lc
from cassmantle_amd.ops import jpeg_format as jf
from test_jpeg_build import HIPCC
from test_jpeg_entropy_native import CSRC, CXX, OUT, ROOT, SANITIZE

DRIVER = os.path.join(ROOT, "tests", "native", "jpeg_fdct_lj_host.cpp")
HEADERS = ("jpeg_fdct_lj.h", "jpeg_huff_opt.h", "jpeg_entropy_blk.h")


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [DRIVER] + [os.path.join(CSRC, h) for h in HEADERS]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    # a plain C++ translation unit: the routines' qualifier macros expand to nothing
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-I", CSRC, *flags, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    items = list(lc.cases())
    path = tmp_path_factory.mktemp("jpeg_fdct_lj") / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"JLJ1" + struct.pack("<I", len(items)))
        for _, img, q, s in items:
            H, W, _ = img.shape
            lq, cq = jf.quant_tables(q)
            f.write(struct.pack("<3I", H, W, int(s == "420")))
            f.write(np.asarray(lq + cq, dtype="<i4").tobytes() + np.ascontiguousarray(img).tobytes())
    return items, str(path)


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", [("jpeg_fdct_lj_plain", []), ("jpeg_fdct_lj_asan", SANITIZE)])
def test_host_program_computes_the_models_coefficients(name, flags, cases, tmp_path):
    items, path = cases
    exe = _build(name, flags)
    out = str(tmp_path / "out.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(items)
    raw = open(out, "rb").read()
    pos = dummies = 0
    for cname, img, q, s in items:
        st = {}
        exp = jf.coefficients(img, q, s, transform="libjpeg", stats=st)
        dummies += st["dummy_blocks"]
        (n,) = struct.unpack_from("<I", raw, pos)
        assert n == exp.size, cname
        got = np.frombuffer(raw, dtype="<i2", count=n, offset=pos + 4).reshape(exp.shape)
        pos += 4 + 2 * n
        assert np.array_equal(got, exp), cname
        (m,) = struct.unpack_from("<I", raw, pos)
        dht = raw[pos + 4: pos + 4 + m]
        pos += 4 + m
        assert dht == jf.dht_segment(jf.optimal_tables(jf.symbol_counts(exp, 0)), "pil"), cname
    assert pos == len(raw)
    assert int(words[3]) == dummies > 0                                  # the dummy rule ran, as often as the model's


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_new_kernels_build_without_scratch():
    """jpeg_transform_lj_kernel (both samplings) and the build kernel that now writes either DHT
    layout keep everything in registers and LDS"""
    out = os.path.join(ROOT, "build", "regcheck", "jpeg_lj.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-mllvm",
                        "-pragma-unroll-threshold=100000", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "jpeg.hip"), "-o", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_count:\s+(\d+)", open(out).read(), re.S):
        pr = re.search(r"private_segment_fixed_size:\s+(\d+)", m.group(2))
        assert pr is not None, m.group(1)
        seen[m.group(1)] = (int(pr.group(1)), int(m.group(3)))
    for k in ("jpeg_transform_lj_kernelILb1", "jpeg_transform_lj_kernelILb0", "jpeg_huff_build_kernel"):
        hit = [n for n in seen if k in n]
        assert hit, (k, sorted(seen))
        assert all(seen[n][0] == 0 for n in hit), {n: seen[n] for n in hit}
        print(k, "vgprs", [seen[n][1] for n in hit])
