"""Optimised Huffman tables on the GPU (ops.jpeg_encode(huffman="optimized"), the optimised Huffman
tables section of ops/csrc/jpeg.hip): byte-exact against the numpy reference with both entropy
coders, every restart interval, batches whose images differ (tables and header lengths per image),
an interval longer than a scan tile, the image whose table needs the 16-bit length limit, input
forms and the current-stream rule, the decoded pixels, round trips, and the serving functions with
``jpeg_huffman=optimized``, whose default still gives the standard tables' bytes."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_huffman_cases as hc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPT = "optimized"


@pytest.fixture(autouse=True)
def _hip_mode():
    ops.set_mode("hip")
    yield


def _coders(restart: int):
    return ("block",) if restart == 0 else ("interval", "block")


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
@pytest.mark.parametrize("quality", jc.QUALITIES)
def test_byte_exact_against_reference(quality, sampling):
    """24x40 and 1x1, noise and flat x restart_mcus {0 (block coder), 1, 2, 5, one MCU row} x both coders"""
    images = {"noise_24x40": jc.noise(24, 40), "flat_24x40": jc.flat(24, 40), "noise_1x1": jc.noise(1, 1),
              "flat_1x1": jc.flat(1, 1)}
    for name, img in images.items():
        H, W, _ = img.shape
        t = torch.from_numpy(img).to(DEV)
        for r in jc.restart_values(H, W, sampling, with_zero=True):
            exp = ref.jpeg_encode(img, quality, sampling, r, huffman=OPT)
            for coder in _coders(r):
                got = ops.jpeg_encode(t, quality, sampling, r, entropy=coder, huffman=OPT)
                assert len(got) == 1 and got[0] == exp[0], (name, quality, sampling, r, coder, len(got[0]), len(exp[0]))


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
def test_byte_exact_batch_of_three_different(sampling):
    """three different images in one call: every image has its own tables and header length"""
    batch = np.stack([jc.black_white_blocks(24, 40), jc.noise(24, 40), jc.flat(24, 40)])
    t = torch.from_numpy(batch).to(DEV)
    for q in jc.QUALITIES:
        for r in jc.restart_values(24, 40, sampling, with_zero=True):
            exp = ref.jpeg_encode(batch, q, sampling, r, huffman=OPT)
            hdr = [jf.parse(e).scan_offset for e in exp]
            assert len(set(hdr)) > 1, hdr                                # the header lengths differ
            assert len({jf.parse(e).huff for e in exp}) == 3             # and so do the tables
            for coder in _coders(r):
                got = ops.jpeg_encode(t, q, sampling, r, entropy=coder, huffman=OPT)
                assert got == exp, (q, sampling, r, coder, [len(g) for g in got], [len(e) for e in exp])


def test_interval_longer_than_a_scan_tile():
    """224x224 at 4:2:0 without restart markers: 1176 blocks in one interval (more than one
    histogram workgroup and more than a scan tile), and with one MCU row per interval"""
    img = jc.noise(224, 224)
    t = torch.from_numpy(img).to(DEV)
    exp = ref.jpeg_encode(img, 95, "420", 0, huffman=OPT)
    assert ops.jpeg_encode(t, 95, "420", 0, entropy="block", huffman=OPT) == exp
    exp = ref.jpeg_encode(img, 95, "420", 14, huffman=OPT)
    for coder in ("interval", "block"):
        assert ops.jpeg_encode(t, 95, "420", 14, entropy=coder, huffman=OPT) == exp, coder


def test_table_that_needs_the_length_limit():
    """the 256x256 skewed image at 4:4:4, quality 100: codes longer than 16 bits before the limit"""
    img = hc.skewed()
    coef = jf.coefficients(img, 100, "444")
    freq = jf.symbol_counts(coef, 0)
    assert max(max(jf.code_sizes(row)) for row in freq) > 16
    t = torch.from_numpy(img).to(DEV)
    exp = ref.jpeg_encode(img, 100, "444", 0, huffman=OPT)
    assert ops.jpeg_encode(t, 100, "444", 0, entropy="block", huffman=OPT) == exp
    exp = ref.jpeg_encode(img, 100, "444", 32, huffman=OPT)
    assert ops.jpeg_encode(t, 100, "444", 32, entropy="interval", huffman=OPT) == exp


def test_input_forms_and_stream():
    """a non-contiguous view, a DeviceImage and a call on a side stream give the plain call's bytes"""
    from cassmantle_amd.game.content import DeviceImage
    img = jc.hard_cases()["noise_64x48"]
    plain = ops.jpeg_encode(torch.from_numpy(img).to(DEV), 75, "420", 3, huffman=OPT)
    assert plain == ref.jpeg_encode(img, 75, "420", 3, huffman=OPT)
    wide = torch.from_numpy(np.concatenate([img, 255 - img], axis=1)).to(DEV)      # [64, 96, 3]
    view = wide[:, :48]
    assert not view.is_contiguous()
    assert ops.jpeg_encode(view, 75, "420", 3, huffman=OPT) == plain
    assert ops.jpeg_encode(DeviceImage(view.contiguous()), 75, "420", 3, huffman=OPT) == plain
    s = torch.cuda.Stream()
    host = torch.from_numpy(img).pin_memory()
    with torch.cuda.stream(s):
        t = host.to(DEV, non_blocking=True)           # ordered before the encode only on s
        got = ops.jpeg_encode(t, 75, "420", 3, huffman=OPT)
        blk = ops.jpeg_encode(t, 75, "420", 3, entropy="block", huffman=OPT)
    assert got == plain and blk == plain


@pytest.mark.parametrize("coder", ("interval", "block"))
def test_decoded_pixels_and_round_trips(coder):
    """return_decoded is the standard call's pixels; PIL and ops.jpeg_decode (both modes) decode
    the optimised stream to them"""
    img = jc.hard_cases()["noise_64x48"]
    t = torch.from_numpy(img).to(DEV)
    std, std_px = ops.jpeg_encode(t, 75, "420", 3, return_decoded=True, entropy=coder)
    outs, px = ops.jpeg_encode(t, 75, "420", 3, return_decoded=True, entropy=coder, huffman=OPT)
    assert torch.equal(px, std_px) and len(outs[0]) < len(std[0])
    pil = jc.decode(outs[0])
    assert np.array_equal(px[0].cpu().numpy(), pil)
    for mode in ("interval", "chunked"):
        back = ops.jpeg_decode(outs[0], device=DEV, mode=mode)
        assert np.array_equal(back.cpu().numpy(), pil), mode


def test_bad_value_is_refused():
    t = torch.from_numpy(jc.noise(8, 8)).to(DEV)
    with pytest.raises(ValueError):
        ops.jpeg_encode(t, huffman="optimised")
    with pytest.raises(ValueError):
        ops.jpeg_encode(t, huffman=None)


def _serving_cfg(optimized: bool, block: bool = False) -> Config:
    cfg = Config()
    cfg.model.gpu_jpeg = cfg.model.gpu_jpeg_content = True
    cfg.model.blur_kernel = "pil"
    if optimized:
        cfg.model.jpeg_huffman = "optimized"
    if block:
        cfg.model.jpeg_entropy, cfg.model.jpeg_restart_mcus = "block", -1
    return cfg


@pytest.mark.parametrize("block", (False, True))
def test_serving_prewarm_buckets(block):
    """gpu_jpeg + jpeg_huffman=optimized: the 60 blur buckets 0.25 .. 15 of a 64x64 prewarm, one
    call, equal the reference encode of the blurred pixels; the content JPEG likewise"""
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn, build_content_jpeg_fn
    cfg = _serving_cfg(True, block)
    img = jc.noise(64, 64)
    x = torch.from_numpy(img).to(DEV)
    radii = [0.25 * k for k in range(1, 61)]
    restart = 0 if block else 64 // 16
    outs = build_blur_jpeg_fn(cfg, DEV)(img, radii, 75)
    blurred = ops.gaussian_blur_pil(x, radii).cpu().numpy()
    assert outs == ref.jpeg_encode(blurred, 75, "420", restart, huffman=OPT)
    data, dimg = build_content_jpeg_fn(cfg, DEV)(DeviceImage(x), 75)
    assert data == ref.jpeg_encode(img, 75, "420", restart, huffman=OPT)[0]
    assert np.array_equal(dimg.tensor.cpu().numpy(), jc.decode(data))


def test_serving_default_bytes_are_unchanged():
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn, build_content_jpeg_fn
    cfg = _serving_cfg(False)
    img = jc.noise(64, 64)
    x = torch.from_numpy(img).to(DEV)
    radii = [0.25, 2.0]
    row = 64 // 16
    outs = build_blur_jpeg_fn(cfg, DEV)(img, radii, 75)
    blurred = ops.gaussian_blur_pil(x, radii).cpu().numpy()
    assert outs == ref.jpeg_encode(blurred, 75, "420", row)
    assert outs == ops.jpeg_encode(torch.from_numpy(blurred).to(DEV), 75, "420", row, huffman="standard")
    data, _ = build_content_jpeg_fn(cfg, DEV)(DeviceImage(x), 75)
    assert data == ref.jpeg_encode(img, 75, "420", row)[0]
    assert jf.parse(data).huff == tuple((tuple(b), tuple(v)) for b, v in jf.STANDARD_TABLES)
