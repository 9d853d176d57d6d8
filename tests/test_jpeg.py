"""Baseline JPEG encoder, CPU side: the numpy reference of the byte contract (ops.reference
.jpeg_encode) against PIL / libjpeg, the hard-case preconditions of the shared inputs, and the
blur cache / config wiring of ``gpu_jpeg``."""
from __future__ import annotations

import io

import numpy as np
import pytest
import torch
from PIL import Image, JpegImagePlugin

import jpeg_cases as jc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.game import imaging
from cassmantle_amd.game.imaging import BlurCache, encode_jpeg
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.ops import reference as ref

MAX_DEFICIT_DB, MAX_SIZE_RATIO = jc.MAX_DEFICIT_DB, jc.MAX_SIZE_RATIO


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
def test_reference_decodes_in_pil(sampling):
    """every shape x restart interval opens and loads in PIL with the true size, mode RGB"""
    for name, img in jc.hard_cases().items():
        H, W, _ = img.shape
        for r in jc.restart_values(H, W, sampling, with_zero=True):
            (data,), (st,) = ref.jpeg_encode(img, 75, sampling, r, return_stats=True)
            im = Image.open(io.BytesIO(data))
            im.load()
            assert im.size == (W, H) and im.mode == "RGB", (name, r)
            assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
            _, _, mx, my = jf.geometry(H, W, sampling)
            assert st["intervals"] == (1 if r == 0 else -(-mx * my // r))
            assert (b"\xff\xdd" in data) == (r != 0)


def test_restart_index_wraps_and_last_interval_short():
    img = jc.hard_cases()["noise_64x48"]
    (data,), (st,) = ref.jpeg_encode(img, 75, "420", 1, return_stats=True)
    assert st["intervals"] == 12                       # RST0..RST7, then RST0..RST2
    scan = data[data.index(b"\xff\xda"):]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (i & 7) for i in range(11)]
    (_,), (st5,) = ref.jpeg_encode(img, 75, "420", 5, return_stats=True)
    assert st5["intervals"] == 3                       # 5 + 5 + 2 MCUs
    assert np.array_equal(jc.decode(ref.jpeg_encode(img, 75, "420", 5)[0]), jc.decode(data))


@pytest.mark.parametrize("quality", [10, 50, 75, 95])
def test_quantisation_tables_and_sampling_match_pil(quality):
    img = jc.gradient(24, 40)
    for sampling in jc.SAMPLINGS:
        ours = Image.open(io.BytesIO(ref.jpeg_encode(img, quality, sampling)[0]))
        pil = Image.open(io.BytesIO(jc.pil_encode(img, quality, sampling, 0)))
        assert ours.quantization == pil.quantization
        assert JpegImagePlugin.get_sampling(ours) == JpegImagePlugin.get_sampling(pil) == {"420": 2, "444": 0}[sampling]


def test_huffman_tables_are_the_standard_ones():
    """our DHT carries the four Annex K tables PIL writes without optimisation"""
    def dht(data: bytes):
        tabs, i = {}, 2
        while data[i + 1] != 0xDA:
            n = (data[i + 2] << 8) | data[i + 3]
            if data[i + 1] == 0xC4:
                seg, j = data[i + 4: i + 2 + n], 0
                while j < len(seg):
                    k = 17 + sum(seg[j + 1: j + 17])
                    tabs[seg[j]] = seg[j: j + k]
                    j += k
            i += 2 + n
        return tabs
    img = jc.gradient(16, 16)
    ours, pil = dht(ref.jpeg_encode(img)[0]), dht(jc.pil_encode(img, 75, "420", 0))
    assert sorted(ours) == [0x00, 0x01, 0x10, 0x11] and ours == pil


def test_fidelity_and_size_against_pil():
    """PSNR deficit and size ratio of the reference encoder against PIL's encode at the same
    quality, sampling and restart interval, over jc.fidelity_inputs() x q {10, 75, 95} x
    {420, 444} x restart_mcus {0, 4}.  Measured on the CPU with this loop:
      largest PSNR deficit: 0.259 dB (gradient, q 95, 4:2:0)  -> bound 0.259 + 0.2 dB
      largest size ratio:   0.9983   (noise, q 95, 4:4:4)     -> bound 0.9983 + 0.02
    (jpeg_cases.MAX_DEFICIT_DB / MAX_SIZE_RATIO; the 0.2 dB absorb decoder rounding)."""
    worst_d, worst_r = (-1e9, None), (0.0, None)
    for name, img in jc.fidelity_inputs().items():
        for q in jc.QUALITIES:
            for s in jc.SAMPLINGS:
                for r in (0, 4):
                    ours, pil = ref.jpeg_encode(img, q, s, r)[0], jc.pil_encode(img, q, s, r)
                    d = jc.psnr(jc.decode(pil), img) - jc.psnr(jc.decode(ours), img)
                    worst_d = max(worst_d, (d, (name, q, s, r)))
                    worst_r = max(worst_r, (len(ours) / len(pil), (name, q, s, r)))
    print("largest deficit", worst_d, "largest size ratio", worst_r)
    assert worst_d[0] <= MAX_DEFICIT_DB, worst_d
    assert worst_r[0] <= MAX_SIZE_RATIO, worst_r


def test_transform_matches_float_dct():
    """the fixed-point transform is the orthonormal 8x8 DCT-II of the level-shifted samples: at
    quality 100 (all quantisers 1) the luma coefficients are within 1 of the float result"""
    img = jc.noise(8, 8, seed=11)
    got = jf.coefficients(img, 100, "444")[0, 0].astype(np.int64)
    p = img.astype(np.float64)
    y = 0.299 * p[..., 0] + 0.587 * p[..., 1] + 0.114 * p[..., 2] - 128.0
    k, n = np.mgrid[0:8, 0:8]
    D = np.cos((2 * n + 1) * k * np.pi / 16) * np.where(k == 0, np.sqrt(1 / 8), 0.5)
    exp = (D @ y @ D.T).reshape(64)[jf.ZIGZAG]
    assert np.abs(got - exp).max() <= 1.0


def test_hard_case_preconditions():
    """the shared inputs reach the coder's hard cases (so no case can silently go missing)"""
    cases = jc.hard_cases()

    def stats(name, q, s="420", r=4):
        return ref.jpeg_encode(cases[name], q, s, r, return_stats=True)[1][0]
    assert stats("noise_64x48", 95)["stuffed"] > 0
    assert stats("highfreq_16x16", 75)["zrl"] >= 3
    hf = jf.coefficients(cases["highfreq_16x16"], 75, "444")[0, 0]
    assert hf[63] != 0 and not hf[1:63].any()          # only the highest frequency survives
    assert stats("blackwhite_24x40", 95)["max_dc_cat"] >= 10
    assert stats("blackwhite_24x40", 95, "444")["max_dc_cat"] >= 10
    fl = jf.coefficients(cases["flat_17x33"], 75, "420")
    assert not fl[..., 1:].any() and fl[..., 0].any()   # DC + EOB only
    st = stats("flat_17x33", 75)
    assert st["zrl"] == 0 and st["stuffed"] == 0


def test_ops_entry_point_on_cpu():
    """CPU tensors (and plain arrays) go to the reference; [H, W, 3] and [B, H, W, 3] agree"""
    img = jc.hard_cases()["blackwhite_24x40"]
    t = torch.from_numpy(img)
    one = ops.jpeg_encode(t, quality=50, sampling="444", restart_mcus=2)
    assert isinstance(one, list) and len(one) == 1 and isinstance(one[0], bytes)
    batch = ops.jpeg_encode(torch.stack([t, 255 - t]), quality=50, sampling="444", restart_mcus=2)
    assert batch[0] == one[0] == ref.jpeg_encode(img, 50, "444", 2)[0] and batch[1] != one[0]
    assert ops.jpeg_encode(t.transpose(0, 1).contiguous().transpose(0, 1), 50, "444", 2) == one
    assert ops.jpeg_encode(img, 50, "444", 2) == one
    with pytest.raises(ValueError):
        ops.jpeg_encode(t.float())
    with pytest.raises(ValueError):
        ops.jpeg_encode(t, sampling="422")


def test_blur_cache_with_injected_blur_jpeg_fn(monkeypatch):
    img = jc.gradient(16, 16)
    original = encode_jpeg(img)
    calls = []

    def fake(arr, radii, quality):
        calls.append((list(radii), quality))
        return [b"jpeg-%.2f" % r for r in radii]
    pil_calls = []
    monkeypatch.setattr(imaging, "encode_jpeg", lambda *a, **k: pil_calls.append(a) or b"pil")
    cache = BlurCache(bucket=0.5, quality=60, blur_jpeg_fn=fake)
    assert cache.get("v", original, 1.0) == b"jpeg-1.00"          # a single miss goes through it too
    assert calls == [([1.0], 60)]
    assert cache.prewarm("v", original, 2.0) == 5
    assert calls[1:] == [([0.5, 1.5, 2.0], 60)]                  # ONE call: the missing radii > 0
    hits = cache.hits
    assert [cache.get("v", original, r) for r in (0.5, 1.0, 1.5, 2.0)] == [b"jpeg-%.2f" % r for r in (0.5, 1, 1.5, 2)]
    assert cache.hits == hits + 4 and len(calls) == 2
    assert cache.get("v", original, 0.0) is original              # radius 0: the stored bytes
    assert cache.prewarm("v", original, 2.0) == 5 and len(calls) == 2
    assert not pil_calls
    # default: the PIL path
    plain = BlurCache(bucket=0.5)
    assert plain.blur_jpeg_fn is None
    assert plain.get("v", original, 1.0) == b"pil" and len(pil_calls) == 1
    assert plain.prewarm("v", original, 1.0) == 3 and len(pil_calls) == 2


def test_room_passes_blur_jpeg_fn_to_its_cache():
    from cassmantle_amd.game.service import GameService

    class _Scorer:
        def embed_words(self, words):
            return None
    fn = lambda arr, radii, quality: [b"x"] * len(radii)   # noqa: E731
    svc = GameService(Config(), _Scorer(), blur_jpeg_fn=fn)
    assert svc.room("").blur_cache.blur_jpeg_fn is fn
    assert GameService(Config(), _Scorer()).room("").blur_cache.blur_jpeg_fn is None


def test_config_and_factory():
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn
    d = Config()
    assert d.model.gpu_jpeg is False and d.model.jpeg_restart_mcus == 0     # 0: one MCU row
    c = Config.from_args(["--jpeg_restart_mcus", "8", "--gpu_jpeg"], base=Config())
    assert c.model.gpu_jpeg is True and c.model.jpeg_restart_mcus == 8
    e = Config.from_env({"CASSMANTLE_GPU_JPEG": "1", "CASSMANTLE_JPEG_RESTART_MCUS": "2"})
    assert e.model.gpu_jpeg is True and e.model.jpeg_restart_mcus == 2
    assert build_blur_jpeg_fn(c, "cpu") is None
    assert build_blur_jpeg_fn(d, "cpu") is None
