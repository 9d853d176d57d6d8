"""Decode contract of the baseline JPEG encoder, CPU side: the numpy reference of the pixels a
decoder produces (ops.jpeg_format.reconstruct, from the quantised coefficients alone) against
PIL / libjpeg decoding the encoder's bytes, the 32-bit word width the kernel relies on, the
``return_decoded`` fallback of ops.jpeg_encode, and the ``gpu_jpeg_content`` flag / room wiring."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.game.imaging import encode_jpeg
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.ops import reference as ref
from jpeg_decode_cases import Scorer, decode_inputs, make_content, reconstructed


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
@pytest.mark.parametrize("quality", jc.QUALITIES)
def test_reconstruct_equals_pil_decode(quality, sampling):
    """exact equality with libjpeg's decode of the encoder's own bytes, every input"""
    for name, img in decode_inputs().items():
        got, _ = reconstructed(name, quality, sampling)
        exp = jc.decode(jf.jpeg_encode(img, quality, sampling, 4)[0])
        assert got.shape == exp.shape and got.dtype == np.uint8
        diff = int(np.count_nonzero(got != exp))
        assert diff == 0, (name, quality, sampling, diff, int(np.abs(got.astype(int) - exp.astype(int)).max()))


def test_decoded_pixels_do_not_depend_on_the_restart_interval():
    img = decode_inputs()["noise_64x48"]
    got, _ = reconstructed("noise_64x48", 75, "420")
    for r in jc.restart_values(64, 48, "420", with_zero=True):
        assert np.array_equal(jc.decode(jf.jpeg_encode(img, 75, "420", r)[0]), got), r


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
@pytest.mark.parametrize("quality", jc.QUALITIES)
def test_intermediates_fit_in_int32(quality, sampling):
    """the reference computes in int64; the kernel's 32-bit words hold every intermediate"""
    for name in decode_inputs():
        _, peak = reconstructed(name, quality, sampling)
        assert 0 < peak < 2 ** 31, (name, quality, sampling, peak)


def test_jpeg_decoded_batches():
    batch = np.stack([jc.black_white_blocks(24, 40), jc.noise(24, 40), jc.flat(24, 40)])
    out = ref.jpeg_decoded(batch, 75, "420")
    assert out.shape == (3, 24, 40, 3) and out.dtype == np.uint8
    for i in range(3):
        assert np.array_equal(out[i], jc.decode(ref.jpeg_encode(batch[i], 75, "420", 4)[0]))
    assert np.array_equal(ref.jpeg_decoded(batch[1], 75, "420")[0], out[1])
    with pytest.raises(ValueError):
        ref.jpeg_decoded(batch.astype(np.float32))


def test_ops_return_decoded_cpu_fallback():
    """CPU tensors and arrays: the reference's bytes and pixels; without the flag, the list of
    bytes as before"""
    img = jc.hard_cases()["noise_64x48"]
    t = torch.from_numpy(img)
    exp_bytes = ref.jpeg_encode(img, 50, "444", 2)
    exp_px = ref.jpeg_decoded(img, 50, "444")
    outs, dec = ops.jpeg_encode(t, 50, "444", 2, return_decoded=True)
    assert outs == exp_bytes
    assert isinstance(dec, torch.Tensor) and dec.dtype == torch.uint8 and tuple(dec.shape) == (1, 64, 48, 3)
    assert dec.device == t.device and np.array_equal(dec.numpy(), exp_px)
    outs, dec = ops.jpeg_encode(img, 50, "444", 2, return_decoded=True)
    assert outs == exp_bytes and np.array_equal(np.asarray(dec), exp_px)
    plain = ops.jpeg_encode(t, 50, "444", 2)
    assert isinstance(plain, list) and plain == exp_bytes
    assert ops.jpeg_encode(t, 50, "444", 2, return_decoded=False) == exp_bytes
    assert ops.jpeg_encode(img, 50, "444", 2) == exp_bytes


def test_flag_and_factory():
    from cassmantle_amd.runtime.factory import build_content_jpeg_fn
    d = Config()
    assert d.model.gpu_jpeg_content is False
    c = Config.from_args(["--gpu_jpeg", "--gpu_jpeg_content"], base=Config())
    assert c.model.gpu_jpeg is True and c.model.gpu_jpeg_content is True
    e = Config.from_env({"CASSMANTLE_GPU_JPEG_CONTENT": "1"})
    assert e.model.gpu_jpeg_content is True and e.model.gpu_jpeg is False
    assert build_content_jpeg_fn(c, "cpu") is None            # all flags set, no GPU
    assert build_content_jpeg_fn(d, "cpu") is None
    assert build_content_jpeg_fn(e, "cuda") is None           # needs gpu_jpeg
    c.model.gpu_blur = False
    assert build_content_jpeg_fn(c, "cuda") is None           # needs gpu_blur


class _HbmImage:
    """stands in for a DeviceImage on a GPU: a ``.tensor`` that says so, and a host copy that
    counts its uses"""

    def __init__(self, arr):
        self.tensor = SimpleNamespace(is_cuda=True)
        self.arr = arr
        self.host_calls = 0

    def host(self):
        self.host_calls += 1
        return self.arr

    def __array__(self, dtype=None, copy=None):
        return self.host()


def test_room_uses_content_jpeg_fn():
    from cassmantle_amd.game.service import GameService
    decoded = object()
    calls = []

    def fake(image, quality):
        calls.append((image, quality))
        return b"device-jpeg", decoded
    cfg = Config()
    cfg.game.jpeg_quality = 60
    svc = GameService(cfg, Scorer(), content_jpeg_fn=fake)
    room = svc.room("")
    assert room.content_jpeg_fn is fake
    image = _HbmImage(jc.gradient(16, 16))
    _, _, jpeg = make_content(room, image)
    assert jpeg == b"device-jpeg" and calls == [(image, 60)]
    version = room._version(b"device-jpeg")
    assert room.blur_cache._sources[version] is decoded        # the decoded pixels, not the original
    assert image.host_calls == 0
    # a host array is not the function's business: today's PIL bytes, no blur source
    arr = jc.gradient(16, 16)
    _, _, jpeg = make_content(room, arr)
    assert jpeg == encode_jpeg(arr, 60) and len(calls) == 1
    assert room._version(jpeg) not in room.blur_cache._sources


def test_room_without_content_jpeg_fn_is_unchanged():
    from cassmantle_amd.game.service import GameService
    room = GameService(Config(), Scorer()).room("")
    assert room.content_jpeg_fn is None
    image = _HbmImage(jc.gradient(16, 16))
    _, _, jpeg = make_content(room, image)
    assert jpeg == encode_jpeg(image.arr, 75) and image.host_calls >= 1
    assert room.blur_cache._sources[room._version(jpeg)] is image


def test_reconstruct_kernels_build_without_scratch():
    """the register guard of test_jpeg_build.py for the idct and colour kernels (their per-lane
    arrays are indexed by unrolled constants only; a dynamic index would move them to scratch)"""
    import os
    import re
    import subprocess
    import test_jpeg_build as tb
    if tb.HIPCC is None:
        pytest.skip("hipcc not available")
    out = os.path.join(tb.ROOT, "build", "regcheck", "jpeg_decode.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([tb.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", tb.CSRC, "-mllvm",
                        "-pragma-unroll-threshold=100000", "--cuda-device-only", "-S",
                        os.path.join(tb.CSRC, "jpeg.hip"), "-o", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_count:\s+(\d+)", open(out).read(), re.S):
        pr = re.search(r"private_segment_fixed_size:\s+(\d+)", m.group(2))
        assert pr is not None, m.group(1)
        seen[m.group(1)] = int(pr.group(1))
    for k in ("jpeg_idct_kernelILb1", "jpeg_idct_kernelILb0", "jpeg_colour_kernelILb1", "jpeg_colour_kernelILb0"):
        hit = [n for n in seen if k in n]
        assert hit, (k, sorted(seen))
        assert all(seen[n] == 0 for n in hit), {n: seen[n] for n in hit}
