"""The per-block coder and the stuffing piece of the block-parallel entropy coder
(ops/csrc/jpeg_entropy_blk.h, the text the kernels compile) as a host program:
tests/native/jpeg_entropy_blk_host.cpp built plain and with ASan + UBSan on the host, a stand-alone
executable that runs the passes (bits, scan, pack, stuffed lengths, scan, write) serially over the
lanes.  Every interval's unstuffed string and the payload are heap blocks of exactly the computed
sizes, and the string is zeroed only where the scan pass zeroes.  On the coefficient arrays of the
encoder's test images (restart 0 included) and on a block at the bits-per-block bound its bytes are
the numpy reference's, with no refused index and no sanitizer report.  Nothing runs on a GPU."""
from __future__ import annotations

import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
from cassmantle_amd.ops import jpeg_format as jf
from test_jpeg_entropy_native import CSRC, CXX, OUT, ROOT, SANITIZE

DRIVER = os.path.join(ROOT, "tests", "native", "jpeg_entropy_blk_host.cpp")


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [DRIVER, os.path.join(CSRC, "jpeg_entropy_blk.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    # a plain C++ translation unit: the routine's qualifier macro expands to nothing
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-I", CSRC, *flags, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def worst_block() -> np.ndarray:
    """int16 [1, 3, 64]: a luma block with DC difference category 11 and 63 AC values of category
    10 whose codes are the table's longest, and two flat chroma blocks."""
    coef = np.zeros((1, 3, 64), dtype=np.int16)
    coef[0, 0, 0] = -2047
    coef[0, 0, 1:] = np.where(np.arange(63) % 2, 1023, -512)
    return coef


def inputs():
    """(name, coef, restart_mcus) of every case."""
    images = dict(jc.hard_cases())
    images["noise_24x40"] = jc.noise(24, 40)
    images["flat_24x40"] = jc.flat(24, 40)
    images["noise_1x1"] = jc.noise(1, 1)
    out = []
    for name, img in images.items():
        H, W, _ = img.shape
        for q in jc.QUALITIES:
            for s in jc.SAMPLINGS:
                coef = jf.coefficients(img, q, s)
                for r in jc.restart_values(H, W, s, with_zero=True) + [coef.shape[0] + 3]:
                    out.append((f"{name}-q{q}-{s}-r{r}", coef, r))
    out.append(("worst_block", worst_block(), 0))
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    items = inputs()
    path = tmp_path_factory.mktemp("jpeg_entropy_blk") / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"JEB1" + struct.pack("<I", len(items)))
        for _, coef, r in items:
            mcus, nb, _ = coef.shape
            per = min(r, mcus) if r else mcus
            f.write(struct.pack("<4I", nb, mcus, per, (mcus + per - 1) // per))
            f.write(jf.huff_table().astype("<u4").tobytes() + np.ascontiguousarray(coef).astype("<i2").tobytes())
    return items, str(path)


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", [("jpeg_entropy_blk_plain", []), ("jpeg_entropy_blk_asan", SANITIZE)])
def test_host_program_writes_the_reference_bytes(name, flags, cases, tmp_path):
    items, path = cases
    exe = _build(name, flags)
    out = str(tmp_path / "out.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(items)
    assert int(words[3]) == 0, r.stdout                               # no pass refused an index
    assert int(words[5]) == jf.BLK_STUFF_CHUNK and int(words[7]) == jf.block_bits_bound(), r.stdout
    raw = open(out, "rb").read()
    pos = 0
    for cname, coef, rst in items:
        (n,) = struct.unpack_from("<I", raw, pos)
        got = raw[pos + 4: pos + 4 + n]
        pos += 4 + n
        assert got == jf.entropy(coef, rst)[0] + b"\xff\xd9", cname
    assert pos == len(raw)
