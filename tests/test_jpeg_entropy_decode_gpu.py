"""Entropy decode contract on the GPU (ops/csrc/jpeg.hip, jpeg_entropy_decode_kernel):
ops.jpeg_decode equals PIL on the corpus of jpeg_stream_cases.py (single, batched, ``out=``, through
build_jpeg_decode_fn), round-trips ops.jpeg_encode's ``return_decoded`` pixels, refuses a block over
the threshold and the malformed streams with their status (the same bytes the sanitized host build
of the same routine has processed, test_jpeg_entropy_native.py), and ``gpu_jpeg_decode``: a blur
cache with only the stored bytes serves the masked bytes of one that holds the device source."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_stream_cases as sc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.game import imaging
from cassmantle_amd.game.content import DeviceImage
from cassmantle_amd.game.imaging import BlurCache
from cassmantle_amd.ops import jpeg_format as jf

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _hip_mode():
    ops.set_mode("hip")
    yield


def _check(streams):
    for s in streams:
        out = ops.jpeg_decode(s.data, device=DEV)
        exp = sc.pil_pixels(s.data)
        assert out.device.type == "cuda" and out.dtype == torch.uint8 and tuple(out.shape) == exp.shape, s.name
        got = out.cpu().numpy()
        diff = int(np.count_nonzero(got != exp))
        assert diff == 0, (s.name, diff, int(np.abs(got.astype(int) - exp.astype(int)).max()))


def test_pil_written_streams_equal_pil():
    """every size, quality, optimised tables, 4:4:4, restart markers; no DRI = one lane decodes it"""
    _check(sc.pil_streams())


def test_in_tree_streams_equal_pil():
    """both samplings, restart_mcus 0..4, and 81 intervals: two thread blocks, the second partial"""
    _check(sc.intree_streams())


def test_batch_out_and_parsed_input():
    batch = sc.batch_streams()
    got = ops.jpeg_decode([b.data for b in batch], device=DEV)
    assert tuple(got.shape) == (3, 24, 40, 3) and got.device.type == "cuda"
    for i, b in enumerate(batch):
        assert np.array_equal(got[i].cpu().numpy(), sc.pil_pixels(b.data)), i
    buf = torch.zeros((3, 24, 40, 3), device=DEV, dtype=torch.uint8)
    assert ops.jpeg_decode([b.data for b in batch], out=buf) is buf and torch.equal(buf, got)
    one = torch.zeros((24, 40, 3), device=DEV, dtype=torch.uint8)
    assert ops.jpeg_decode(jf.parse(batch[1].data), device=DEV, out=one) is one and torch.equal(one, got[1])
    with pytest.raises(ValueError):
        ops.jpeg_decode([batch[0].data, sc.intree_streams()[0].data], device=DEV)
    with pytest.raises(ValueError):
        ops.jpeg_decode(batch[0].data, out=torch.zeros((24, 40, 3), device=DEV, dtype=torch.int16))


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
@pytest.mark.parametrize("shape", [(17, 33), (48, 40)])
def test_round_trip_of_the_gpu_encoder(shape, sampling):
    """the pixels ops.jpeg_encode computes from its coefficients are those of its bytes, decoded"""
    H, W = shape
    img = jc.noise(H, W, seed=H)
    t = torch.from_numpy(img).to(DEV)
    row = (W + (16 if sampling == "420" else 8) - 1) // (16 if sampling == "420" else 8)
    for r in (1, 2, row):
        outs, dec = ops.jpeg_encode(t, 75, sampling, r, return_decoded=True)
        back = ops.jpeg_decode(outs[0], device=DEV)
        assert torch.equal(back, dec[0]), (shape, sampling, r)
        assert np.array_equal(back.cpu().numpy(), sc.pil_pixels(outs[0]))


def test_energy_rule():
    """crafted blocks under the threshold are PIL's pixels, over it a refusal naming the interval"""
    for name, data, target in sc.energy_streams():
        if target <= jf.WIDE_T:
            assert np.array_equal(ops.jpeg_decode(data, device=DEV).cpu().numpy(), sc.pil_pixels(data)), name
        else:
            with pytest.raises(jf.JpegUnsupported) as e:
                ops.jpeg_decode(data, device=DEV)
            assert (e.value.code, e.value.interval) == (jf.WIDE, 0), name


def test_malformed_streams_are_refused_with_their_status():
    for m in sc.malformed():
        with pytest.raises(jf.JpegError) as e:
            ops.jpeg_decode(m.data, device=DEV)
        with pytest.raises(jf.JpegError) as r:
            jf.entropy_decode(jf.parse(m.data))
        assert e.value.code == m.code and e.value.interval == r.value.interval, (m.name, e.value.code)
    # the lowest failing interval of a batch is reported, numbered image * intervals + interval
    good = jf.jpeg_encode(jc.noise(17, 33, seed=50), 75, "420", 2)[0]
    bad = sc.malformed()[0].data
    with pytest.raises(jf.JpegError) as e:
        ops.jpeg_decode([good, bad, bad], device=DEV)
    assert (e.value.code, e.value.interval) == (jf.TRUNCATED, 3 + 2)
    # and a good call after a refused one is unaffected
    assert np.array_equal(ops.jpeg_decode(good, device=DEV).cpu().numpy(), sc.pil_pixels(good))


def _cfg(decode: bool) -> Config:
    cfg = Config()
    cfg.model.gpu_jpeg = cfg.model.gpu_jpeg_content = True
    cfg.model.blur_kernel = "pil"
    cfg.model.gpu_jpeg_decode = decode
    cfg.model.jpeg_decode_min_intervals = 2
    return cfg


def test_decode_fn_gives_a_device_image_or_leaves_the_stream_to_pil():
    from cassmantle_amd.runtime.factory import build_jpeg_decode_fn
    fn = build_jpeg_decode_fn(_cfg(True), DEV)
    assert fn is not None and build_jpeg_decode_fn(_cfg(False), DEV) is None
    s = sc.intree_streams()[-1]
    img = fn(s.data)
    assert isinstance(img, DeviceImage) and img.tensor.device.type == "cuda" and img._host is None
    assert np.array_equal(img.tensor.cpu().numpy(), sc.pil_pixels(s.data))
    no_dri = next(x for x in sc.pil_streams() if x.name == "pil_noise_48x40_q75")
    assert fn(no_dri.data) is None                            # one interval < jpeg_decode_min_intervals
    assert fn(sc.malformed()[0].data) is None and fn(b"not a jpeg") is None
    c = np.zeros((4, 3, 64), dtype=np.int16)
    c[3, 2, 1] = 1023                                         # one block over the threshold, 4 intervals
    assert fn(sc.craft(c, 50, 16, 16, "444", restart=1)) is None


def test_masked_bytes_from_stored_bytes_alone(monkeypatch):
    """gpu_jpeg + gpu_jpeg_content + blur_kernel=pil on one 48x64 image: cache A holds the device
    source, cache B only the stored bytes and decode_fn (PIL's decode_jpeg raises); all 61 buckets
    are the same bytes.  Flag off: no decode_fn, decode_jpeg is used."""
    from cassmantle_amd.runtime.factory import (build_blur_fn, build_blur_jpeg_fn, build_content_jpeg_fn,
                                                build_jpeg_decode_fn)
    cfg = _cfg(True)
    content_fn, decode_fn = build_content_jpeg_fn(cfg, DEV), build_jpeg_decode_fn(cfg, DEV)
    blur_fn, blur_jpeg_fn = build_blur_fn(cfg, DEV), build_blur_jpeg_fn(cfg, DEV)
    assert None not in (content_fn, decode_fn, blur_fn, blur_jpeg_fn)
    jpeg, decoded = content_fn(DeviceImage(torch.from_numpy(jc.noise(48, 64)).to(DEV)), cfg.game.jpeg_quality)
    q = cfg.game.jpeg_quality
    a = BlurCache(blur_fn=blur_fn, bucket=0.25, quality=q, blur_jpeg_fn=blur_jpeg_fn)
    b = BlurCache(blur_fn=blur_fn, bucket=0.25, quality=q, blur_jpeg_fn=blur_jpeg_fn, decode_fn=decode_fn)
    a.set_source("v", decoded)
    real = imaging.decode_jpeg

    def refuse(data):
        raise AssertionError("decode_jpeg called")
    monkeypatch.setattr(imaging, "decode_jpeg", refuse)
    assert a.prewarm("v", jpeg, 15.0) == 61 and b.prewarm("v", jpeg, 15.0) == 61
    for i in range(61):
        ja, jb = a.get("v", jpeg, i * 0.25), b.get("v", jpeg, i * 0.25)
        assert ja == jb, i
    assert len({a.get("v", jpeg, i * 0.25) for i in range(61)}) > 30
    assert isinstance(b._decoded[1], DeviceImage) and b._decoded[1]._host is None
    # flag off: the parent's path
    calls = []
    monkeypatch.setattr(imaging, "decode_jpeg", lambda data: calls.append(data) or real(data))
    off = _cfg(False)
    assert build_jpeg_decode_fn(off, DEV) is None
    c = BlurCache(blur_fn=blur_fn, bucket=0.25, quality=q, blur_jpeg_fn=blur_jpeg_fn,
                  decode_fn=build_jpeg_decode_fn(off, DEV))
    assert c.get("v", jpeg, 3.0) == a.get("v", jpeg, 3.0) and calls == [jpeg]
