"""The libjpeg forward contract on the GPU (jpeg_transform_lj_kernel and the PIL header layout of
both header paths): ``ops.jpeg_encode(transform="libjpeg", entropy="block", restart_mcus=0)`` is
the file Pillow writes, byte for byte, on every case of jpeg_libjpeg_cases.py, with standard and
optimised Huffman tables, batched, from a view, a DeviceImage and a side stream; with restart
markers it is the reference's bytes; ``return_decoded`` is Pillow's decode; and a serving prewarm
with ``jpeg_transform=libjpeg`` is byte-identical to a BlurCache that has no GPU function at all."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import jpeg_libjpeg_cases as lc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
LJ = "libjpeg"
PIL = dict(entropy="block", restart_mcus=0, transform=LJ)      # the call that writes Pillow's file


@pytest.fixture(autouse=True)
def _hip_mode():
    ops.set_mode("hip")
    yield


@pytest.mark.parametrize("sampling", lc.SAMPLINGS)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_bytes_equal_pillow(kind, sampling):
    """every size and quality; standard tables and optimize=True"""
    for H, W in lc.SIZES:
        t = torch.from_numpy(lc.image(kind, H, W).copy()).to(DEV)
        for q in lc.QUALITIES:
            got = ops.jpeg_encode(t, q, sampling, **PIL)
            assert got == [lc.pil_bytes(kind, H, W, q, sampling)], (kind, H, W, q, sampling)
            got = ops.jpeg_encode(t, q, sampling, huffman="optimized", **PIL)
            assert got == [lc.pil_bytes(kind, H, W, q, sampling, optimize=True)], (kind, H, W, q, sampling, "optimized")


@pytest.mark.parametrize("sampling", lc.SAMPLINGS)
def test_batch_of_three_different(sampling):
    """three different images in one call (48x23: dummy blocks and an odd width); with optimised
    tables every image has its own four DHT segments and header length"""
    H, W = 48, 23
    batch = np.stack([lc.image(k, H, W) for k in lc.KINDS])
    t = torch.from_numpy(batch).to(DEV)
    for q in (75, 100):
        exp = [lc.pil_bytes(k, H, W, q, sampling) for k in lc.KINDS]
        assert ops.jpeg_encode(t, q, sampling, **PIL) == exp, (q, sampling)
        exp = [lc.pil_bytes(k, H, W, q, sampling, optimize=True) for k in lc.KINDS]
        assert len({jf.parse(e).scan_offset for e in exp}) > 1
        assert ops.jpeg_encode(t, q, sampling, huffman="optimized", **PIL) == exp, (q, sampling, "optimized")


def test_more_than_one_workgroup():
    """100x75 at 4:2:0: 35 MCUs, nine transform workgroups, the last one partly idle; even H that
    is no multiple of 16"""
    img = np.random.default_rng(5).integers(0, 256, (100, 75, 3), dtype=np.uint8)
    t = torch.from_numpy(img).to(DEV)
    for s in lc.SAMPLINGS:
        assert ops.jpeg_encode(t, 75, s, **PIL) == [lc.pil_encode(img, 75, s)], s


def test_input_forms_and_stream():
    """a non-contiguous view, a DeviceImage and a call on a side stream give the plain call's bytes"""
    from cassmantle_amd.game.content import DeviceImage
    img = lc.image("noise", 33, 16)
    plain = [lc.pil_bytes("noise", 33, 16, 75, "420")]
    assert ops.jpeg_encode(torch.from_numpy(img.copy()).to(DEV), 75, **PIL) == plain
    wide = torch.from_numpy(np.concatenate([img, 255 - img], axis=1)).to(DEV)      # [33, 32, 3]
    view = wide[:, :16]
    assert not view.is_contiguous()
    assert ops.jpeg_encode(view, 75, **PIL) == plain
    assert ops.jpeg_encode(DeviceImage(view.contiguous()), 75, **PIL) == plain
    s = torch.cuda.Stream()
    host = torch.from_numpy(img.copy()).pin_memory()
    with torch.cuda.stream(s):
        t = host.to(DEV, non_blocking=True)           # ordered before the encode only on s
        got = ops.jpeg_encode(t, 75, **PIL)
        opt = ops.jpeg_encode(t, 75, huffman="optimized", **PIL)
    assert got == plain and opt == [lc.pil_bytes("noise", 33, 16, 75, "420", optimize=True)]


@pytest.mark.parametrize("sampling", lc.SAMPLINGS)
def test_restart_intervals_equal_the_reference(sampling):
    """the interval coder at restart 1, 2 and one MCU row, and the block coder on the same"""
    for H, W in ((17, 33), (48, 23), (1, 1)):
        img = lc.image("blurred", H, W)
        t = torch.from_numpy(img.copy()).to(DEV)
        m = 16 if sampling == "420" else 8
        for r in dict.fromkeys((1, 2, (W + m - 1) // m)):
            for huffman in jf.HUFFMAN_MODES:
                exp = ref.jpeg_encode(img, 75, sampling, r, huffman=huffman, transform=LJ)
                for coder in ("interval", "block"):
                    got = ops.jpeg_encode(t, 75, sampling, r, entropy=coder, huffman=huffman, transform=LJ)
                    assert got == exp, (H, W, sampling, r, huffman, coder)


@pytest.mark.parametrize("sampling", lc.SAMPLINGS)
def test_decoded_pixels_are_pillows(sampling):
    for H, W in ((24, 40), (9, 7)):
        t = torch.from_numpy(lc.image("noise", H, W).copy()).to(DEV)
        outs, px = ops.jpeg_encode(t, 75, sampling, return_decoded=True, **PIL)
        assert outs == [lc.pil_bytes("noise", H, W, 75, sampling)]
        assert np.array_equal(px[0].cpu().numpy(), lc.decode(outs[0])), (H, W, sampling)
        outs, px = ops.jpeg_encode(t, 75, sampling, 2, return_decoded=True, transform=LJ)
        assert np.array_equal(px[0].cpu().numpy(), lc.decode(outs[0])), (H, W, sampling, "interval")


def test_bad_value_is_refused():
    t = torch.from_numpy(lc.image("noise", 8, 8).copy()).to(DEV)
    for bad in ("islow", None):
        with pytest.raises(ValueError, match="transform"):
            ops.jpeg_encode(t, transform=bad)


def _serving_cfg(libjpeg: bool) -> Config:
    cfg = Config()
    cfg.model.gpu_jpeg = cfg.model.gpu_jpeg_content = True
    cfg.model.blur_kernel = "pil"
    if libjpeg:
        cfg.model.jpeg_entropy, cfg.model.jpeg_restart_mcus, cfg.model.jpeg_transform = "block", -1, LJ
    return cfg


def test_serving_prewarm_equals_a_cache_without_gpu_functions():
    """gpu_jpeg + blur_kernel=pil + jpeg_entropy=block + jpeg_restart_mcus=-1 + jpeg_transform=libjpeg:
    the 60 buckets 0.25 .. 15 of a 64x64 prewarm are the bytes of PIL's blur + encode_jpeg, and the
    content JPEG is encode_jpeg's"""
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.game.imaging import BlurCache, encode_jpeg
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn, build_content_jpeg_fn
    cfg = _serving_cfg(True)
    img = np.random.default_rng(7).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    content = encode_jpeg(img, 75)
    gpu = BlurCache(blur_jpeg_fn=build_blur_jpeg_fn(cfg, DEV))
    cpu = BlurCache()
    assert gpu.prewarm("v", content, 15.0) == cpu.prewarm("v", content, 15.0) == 61
    for k in range(1, 61):
        assert gpu.get("v", content, 0.25 * k) == cpu.get("v", content, 0.25 * k), k
    assert gpu.misses == 60 + 1 and gpu.hits >= 60                        # one call made them all
    data, dimg = build_content_jpeg_fn(cfg, DEV)(DeviceImage(torch.from_numpy(img).to(DEV)), 75)
    assert data == content
    assert np.array_equal(dimg.tensor.cpu().numpy(), lc.decode(content))


def test_serving_default_bytes_are_unchanged():
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn, build_content_jpeg_fn
    cfg = _serving_cfg(False)
    img = np.random.default_rng(7).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    x = torch.from_numpy(img).to(DEV)
    radii = [0.25, 2.0]
    outs = build_blur_jpeg_fn(cfg, DEV)(img, radii, 75)
    blurred = ops.gaussian_blur_pil(x, radii).cpu().numpy()
    assert outs == jf.jpeg_encode(blurred, 75, "420", 64 // 16)
    assert outs == ops.jpeg_encode(torch.from_numpy(blurred).to(DEV), 75, "420", 64 // 16, transform="matrix")
    data, _ = build_content_jpeg_fn(cfg, DEV)(DeviceImage(x), 75)
    assert data == jf.jpeg_encode(img, 75, "420", 64 // 16)[0]
    assert data.startswith(jf.header(64, 64, 75, "420", 64 // 16))         # one DQT, one DHT: the compact layout
