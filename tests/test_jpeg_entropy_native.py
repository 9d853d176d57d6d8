"""The per-interval entropy decoder (ops/csrc/jpeg_entropy_dec.h, the text the kernel compiles) as
a host program: tests/native/jpeg_entropy_host.cpp built plain and with ASan + UBSan on the host,
run on the corpus and the malformed streams of jpeg_stream_cases.py.  Its coefficients equal the
numpy reference's, the malformed streams end with their status, and a fixed-seed mutation pass
(single-bit flips and truncations of the smaller streams, at most 2000 runs, every interval in a
heap block of exactly its size) ends without a sanitizer report.  Nothing runs on a GPU."""
from __future__ import annotations

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_stream_cases as sc
from cassmantle_amd.ops import jpeg_format as jf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cassmantle_amd", "ops", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "jpeg_entropy_host.cpp")
OUT = os.path.join(ROOT, "build", "native")
CXX = next((c for c in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++",
                        shutil.which("g++")) if c and os.path.exists(c)), None)
SANITIZE = ["-fsanitize=address", "-fsanitize=undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [DRIVER, os.path.join(CSRC, "jpeg_entropy_dec.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    # a plain C++ translation unit: the routine's qualifier macro expands to nothing
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-I", CSRC, *flags, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _case(data: bytes, mutate: bool) -> bytes:
    st = jf.parse(data)
    _, nb, mx, my = jf.geometry(st.H, st.W, st.sampling)
    mcus = mx * my
    end = st.intervals[-1][0] + st.intervals[-1][1]
    body = data[st.scan_offset: end]
    tables = np.concatenate([np.asarray([t[jf.ZIGZAG[z]] for t in st.qtables for z in range(64)], dtype=np.int32),
                             jf.decode_tables(st.huff)])
    iv = np.asarray(st.intervals, dtype=np.int64) - np.asarray([st.scan_offset, 0])
    return (struct.pack("<6I", nb, mcus, st.restart or mcus, len(st.intervals), len(body), int(mutate))
            + tables.astype("<u4").tobytes() + iv.astype("<u4").tobytes() + body)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    streams = [(s.name, s.data, jf.OK) for s in sc.corpus() + sc.batch_streams()]
    streams += [(m.name, m.data, m.code) for m in sc.malformed()]
    streams += [(n, d, jf.OK if t <= jf.WIDE_T else jf.WIDE) for n, d, t in sc.energy_streams()]
    small = [len(d) < 1500 for _, d, _ in streams]
    path = tmp_path_factory.mktemp("jpeg_entropy") / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"JED1" + struct.pack("<I", len(streams)))
        for (_, data, _), m in zip(streams, small):
            f.write(_case(data, m))
    return streams, str(path), sum(small)


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", [("jpeg_entropy_plain", []), ("jpeg_entropy_asan", SANITIZE)])
def test_host_program_matches_the_reference(name, flags, cases, tmp_path):
    streams, path, nsmall = cases
    exe = _build(name, flags)
    out = str(tmp_path / "out.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(streams)
    runs = int(words[3])
    assert nsmall > 50 and 2000 - nsmall < runs <= 2000, r.stdout
    assert int(words[5]) < runs                               # some mutation was caught
    raw = open(out, "rb").read()
    pos = 0
    for sname, data, code in streams:
        st = jf.parse(data)
        _, nb, mx, my = jf.geometry(st.H, st.W, st.sampling)
        n = mx * my * nb * 64
        status, where = struct.unpack_from("<II", raw, pos)
        coef = np.frombuffer(raw, dtype="<i2", count=n, offset=pos + 8).reshape(mx * my, nb, 64)
        pos += 8 + 2 * n
        assert status == code, (sname, status, where)
        if code == jf.OK:
            assert np.array_equal(coef, sc.reference(data)[1]), sname
        else:
            with pytest.raises(ValueError) as e:
                jf.entropy_decode(st)
            assert e.value.interval == where, sname
    assert pos == len(raw)
