"""The lane run of the chunked entropy decode (ops/csrc/jpeg_entropy_sync.h, the text the kernel
compiles) as a host program: tests/native/jpeg_entropy_sync_host.cpp built plain and with ASan +
UBSan on the host, a stand-alone executable that runs rounds, scan, write, DC and check passes
serially over the lanes.  On the corpus its coefficients equal the numpy reference's with no flag,
and its rounds and chunks are the numpy model's; every malformed and over-threshold stream is
flagged; and a fixed-seed mutation pass (single-bit flips and truncations of the smaller streams,
at most 2000 runs, every interval in a heap block of exactly its size) keeps "serial OK => no
flag, equal coefficients" and "serial error => flag" without a sanitizer report.  Nothing runs on
a GPU."""
from __future__ import annotations

import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_stream_cases as sc
from cassmantle_amd.ops import jpeg_format as jf
from test_jpeg_entropy_native import CSRC, CXX, OUT, ROOT, SANITIZE, _case

DRIVER = os.path.join(ROOT, "tests", "native", "jpeg_entropy_sync_host.cpp")
CHUNK = 16


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [DRIVER, os.path.join(CSRC, "jpeg_entropy_sync.h"), os.path.join(CSRC, "jpeg_entropy_dec.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    # a plain C++ translation unit: the routine's qualifier macro expands to nothing
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-I", CSRC, *flags, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    streams = [(s.name, s.data, jf.OK) for s in sc.corpus() + sc.batch_streams()]
    streams += [(m.name, m.data, m.code) for m in sc.malformed()]
    streams += [(n, d, jf.OK if t <= jf.WIDE_T else jf.WIDE) for n, d, t in sc.energy_streams()]
    small = [len(d) < 1500 for _, d, _ in streams]
    path = tmp_path_factory.mktemp("jpeg_entropy_sync") / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"JED1" + struct.pack("<I", len(streams)))
        for (_, data, _), m in zip(streams, small):
            f.write(_case(data, m))
    return streams, str(path), sum(small)


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", [("jpeg_entropy_sync_plain", []), ("jpeg_entropy_sync_asan", SANITIZE)])
def test_host_program_matches_the_reference(name, flags, cases, tmp_path):
    streams, path, nsmall = cases
    exe = _build(name, flags)
    out = str(tmp_path / "out.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path, out, str(CHUNK)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(streams)
    runs, ok, flagged = int(words[3]), int(words[5]), int(words[7])
    assert nsmall > 50 and 2000 - nsmall < runs <= 2000, r.stdout
    assert 0 < ok < runs and ok + flagged == runs, r.stdout        # some mutations decode, some are caught
    raw = open(out, "rb").read()
    pos = 0
    for sname, data, code in streams:
        st = jf.parse(data)
        _, nb, mx, my = jf.geometry(st.H, st.W, st.sampling)
        n = mx * my * nb * 64
        flag, rounds, chunks = struct.unpack_from("<III", raw, pos)
        coef = np.frombuffer(raw, dtype="<i2", count=n, offset=pos + 12).reshape(mx * my, nb, 64)
        pos += 12 + 2 * n
        assert flag == (code != jf.OK), (sname, flag)
        if code == jf.OK:
            assert np.array_equal(coef, sc.reference(data)[1]), sname
            stats = {}
            jf.entropy_decode_chunked(st, CHUNK, stats=stats)
            assert (rounds, chunks) == (stats["rounds"], stats["chunks"]), sname
    assert pos == len(raw)
