"""Register guard for the PIL-exact blur kernels (CPU, hipcc only), in the manner of
test_jpeg_build.py: blur_pil.hip compiles for gfx950 and no kernel of it uses scratch (the
running window sum, the edge sample and the box parameters of a segment stay in registers)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cassmantle_amd", "ops", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
KERNELS = ("blur_pil_tile_kernelILi64ELi512", "blur_pil_line_kernel")


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_blur_pil_kernels_build_without_scratch():
    out = os.path.join(ROOT, "build", "regcheck", "blur_pil.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-mllvm",
                        "-pragma-unroll-threshold=100000", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "blur_pil.hip"), "-o", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    s = open(out).read()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_count:\s+(\d+)", s, re.S):
        pr = re.search(r"private_segment_fixed_size:\s+(\d+)", m.group(2))
        assert pr is not None, m.group(1)
        seen[m.group(1)] = int(pr.group(1))
    for k in KERNELS:
        hit = [n for n in seen if k in n]
        assert hit, (k, sorted(seen))
        assert all(seen[n] == 0 for n in hit), {n: seen[n] for n in hit}
