"""Register guard for the kernels of the block-parallel entropy coder (CPU, hipcc only), in the
manner of test_jpeg_build.py, whose kernel list predates them: jpeg.hip compiles for gfx950 and
none of the jpeg_blk_* kernels uses scratch (the per-block coder keeps its bit buffer and one
coefficient chunk in registers; a dynamically indexed array there would silently move to scratch)."""
import os
import re
import subprocess

import pytest

from test_jpeg_build import CSRC, HIPCC, ROOT

KERNELS = ("jpeg_blk_bits_kernel", "jpeg_blk_scan_kernel", "jpeg_blk_pack_kernel", "jpeg_blk_stuff_kernelILb0",
           "jpeg_blk_stuff_kernelILb1")


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_block_coder_kernels_build_without_scratch():
    out = os.path.join(ROOT, "build", "regcheck", "jpeg_blk.s")
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
