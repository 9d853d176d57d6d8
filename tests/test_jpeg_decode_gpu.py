"""Decode contract on the GPU (ops/csrc/jpeg.hip, idct + colour kernels): ops.jpeg_encode's
``return_decoded`` pixels equal the numpy reference exactly (hence PIL's decode of the bytes,
test_jpeg_decode.py), over inputs, batch, input forms and streams; and ``gpu_jpeg_content``: a
blur cache that holds the decoded device source and one that decodes the stored JPEG serve
identical masked bytes."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.game.content import DeviceImage
from cassmantle_amd.game.imaging import BlurCache, encode_jpeg
from cassmantle_amd.ops import reference as ref
from jpeg_decode_cases import Scorer, decode_inputs, make_content, reconstructed

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _hip_mode():
    ops.set_mode("hip")
    yield


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
@pytest.mark.parametrize("quality", jc.QUALITIES)
def test_decoded_pixels_exact_against_reference(quality, sampling):
    """every input, one restart value per case: same bytes as without the flag, the reference's pixels"""
    for i, (name, img) in enumerate(decode_inputs().items()):
        H, W, _ = img.shape
        rs = jc.restart_values(H, W, sampling, with_zero=False)
        r = rs[i % len(rs)]
        t = torch.from_numpy(img).to(DEV)
        outs, dec = ops.jpeg_encode(t, quality, sampling, r, return_decoded=True)
        assert outs == ops.jpeg_encode(t, quality, sampling, r), (name, quality, sampling, r)
        assert dec.device == t.device and dec.dtype == torch.uint8 and tuple(dec.shape) == (1, H, W, 3)
        exp, _ = reconstructed(name, quality, sampling)
        got = dec[0].cpu().numpy()
        diff = int(np.count_nonzero(got != exp))
        assert diff == 0, (name, quality, sampling, r, diff, int(np.abs(got.astype(int) - exp.astype(int)).max()))


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
def test_decoded_batch_of_three_mixed(sampling):
    """three different 24x40 images in one call: the plane and batch indexing"""
    batch = np.stack([jc.black_white_blocks(24, 40), jc.noise(24, 40), jc.flat(24, 40)])
    exp = ref.jpeg_decoded(batch, 75, sampling)
    outs, dec = ops.jpeg_encode(torch.from_numpy(batch).to(DEV), 75, sampling, 2, return_decoded=True)
    assert outs == ref.jpeg_encode(batch, 75, sampling, 2)
    got = dec.cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], exp[i]), (sampling, i, int(np.count_nonzero(got[i] != exp[i])))


def test_decoded_input_forms():
    """a non-contiguous view and a DeviceImage give the pixels of the contiguous tensor"""
    img = jc.hard_cases()["noise_64x48"]
    exp, _ = reconstructed("noise_64x48", 75, "420")
    wide = torch.from_numpy(np.concatenate([img, 255 - img], axis=1)).to(DEV)      # [64, 96, 3]
    view = wide[:, :48]
    assert not view.is_contiguous()
    for form in (view, DeviceImage(view.contiguous()), view.contiguous()[None]):
        outs, dec = ops.jpeg_encode(form, 75, "420", 4, return_decoded=True)
        assert outs == ref.jpeg_encode(img, 75, "420", 4)
        assert tuple(dec.shape) == (1, 64, 48, 3) and np.array_equal(dec[0].cpu().numpy(), exp)


def test_decoded_on_a_side_stream():
    """the reconstruct kernels run on the current stream: inside torch.cuda.stream(s), with the
    input produced on s, the pixels are right after synchronising s alone"""
    img = jc.hard_cases()["noise_64x48"]
    exp, _ = reconstructed("noise_64x48", 95, "444")
    s = torch.cuda.Stream()
    host = torch.from_numpy(img).pin_memory()
    back = torch.empty((1, 64, 48, 3), dtype=torch.uint8).pin_memory()
    with torch.cuda.stream(s):
        t = host.to(DEV, non_blocking=True)           # ordered before the encode only on s
        outs, dec = ops.jpeg_encode(t, 95, "444", 2, return_decoded=True)
        back.copy_(dec, non_blocking=True)
    s.synchronize()
    assert outs == ref.jpeg_encode(img, 95, "444", 2)
    assert np.array_equal(back[0].numpy(), exp)


def _content_cfg() -> Config:
    cfg = Config()
    cfg.model.gpu_jpeg = True
    cfg.model.gpu_jpeg_content = True
    return cfg


def test_masked_bytes_do_not_depend_on_who_serves_the_miss():
    """gpu_jpeg + gpu_jpeg_content on one 48x64 image: cache A blurs the decoded device source,
    cache B has only the stored JPEG and decodes it with PIL; the real blur_jpeg_fn gives both
    the same bytes at radii 0.25, 3 and 15, and radius 0 is the stored JPEG itself"""
    from cassmantle_amd.runtime.factory import build_blur_fn, build_blur_jpeg_fn, build_content_jpeg_fn
    cfg = _content_cfg()
    content_fn = build_content_jpeg_fn(cfg, DEV)
    blur_fn, blur_jpeg_fn = build_blur_fn(cfg, DEV), build_blur_jpeg_fn(cfg, DEV)
    assert content_fn is not None and blur_jpeg_fn is not None
    img = jc.noise(48, 64)
    original = DeviceImage(torch.from_numpy(img).to(DEV))
    jpeg, decoded = content_fn(original, cfg.game.jpeg_quality)
    assert original._host is None                                    # the pixels never crossed
    assert jpeg == ref.jpeg_encode(img, cfg.game.jpeg_quality, "420", 4)[0]      # one MCU row = 4
    px = decoded.tensor.cpu().numpy()
    assert np.array_equal(px, jc.decode(jpeg)) and not np.array_equal(px, img)
    a = BlurCache(blur_fn=blur_fn, bucket=0.25, quality=cfg.game.jpeg_quality, blur_jpeg_fn=blur_jpeg_fn)
    b = BlurCache(blur_fn=blur_fn, bucket=0.25, quality=cfg.game.jpeg_quality, blur_jpeg_fn=blur_jpeg_fn)
    a.set_source("v", decoded)
    for radius in (0.25, 3.0, 15.0):
        ja, jb = a.get("v", jpeg, radius), b.get("v", jpeg, radius)
        assert ja == jb and jc.decode(ja).shape == (48, 64, 3), radius
    assert a.get("v", jpeg, 0.0) is jpeg and b.get("v", jpeg, 0.0) is jpeg
    assert a.misses == 4 and b.misses == 4 and a.hits == 0


def test_room_content_with_and_without_the_flag():
    """flags on: the room stores the device encoder's bytes and registers their decoded pixels,
    no host copy of the image; flags off: encode_jpeg's bytes and the original image, as before"""
    from cassmantle_amd.game.service import GameService
    from cassmantle_amd.runtime.factory import build_content_jpeg_fn
    img = jc.noise(48, 64)
    cfg = _content_cfg()
    room = GameService(cfg, Scorer(), content_jpeg_fn=build_content_jpeg_fn(cfg, DEV)).room("")
    image = DeviceImage(torch.from_numpy(img).to(DEV))
    jpeg = make_content(room, image)[2]
    assert jpeg == ref.jpeg_encode(img, 75, "420", 4)[0] and image._host is None
    source = room.blur_cache._sources[room._version(jpeg)]
    assert source is not image and np.array_equal(source.tensor.cpu().numpy(), jc.decode(jpeg))

    off = Config()
    off.model.gpu_jpeg = True                                        # gpu_jpeg alone: the parent's path
    assert build_content_jpeg_fn(off, DEV) is None and build_content_jpeg_fn(Config(), DEV) is None
    room = GameService(off, Scorer(), content_jpeg_fn=build_content_jpeg_fn(off, DEV)).room("")
    image = DeviceImage(torch.from_numpy(img).to(DEV))
    jpeg = make_content(room, image)[2]
    assert jpeg == encode_jpeg(img, 75)
    assert room.blur_cache._sources[room._version(jpeg)] is image
