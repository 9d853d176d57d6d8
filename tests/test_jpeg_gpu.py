"""HIP baseline JPEG encoder (ops/csrc/jpeg.hip) on the GPU: byte-exact against the numpy
reference over the hard-case inputs of jpeg_cases.py, input forms, the current-stream rule, and
the ``gpu_jpeg`` serving path (blur + encode in HBM, blur cache, /fetch/contents)."""
from __future__ import annotations

import base64
import time

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _hip_mode():
    ops.set_mode("hip")
    yield


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
@pytest.mark.parametrize("quality", jc.QUALITIES)
def test_byte_exact_against_reference(quality, sampling):
    """every hard-case input x restart_mcus {1, 2, 5, one MCU row}, batch 1"""
    for name, img in jc.hard_cases().items():
        H, W, _ = img.shape
        t = torch.from_numpy(img).to(DEV)
        for r in jc.restart_values(H, W, sampling, with_zero=False):
            got = ops.jpeg_encode(t, quality, sampling, r)
            exp = ref.jpeg_encode(img, quality, sampling, r)
            assert len(got) == 1 and got[0] == exp[0], (name, quality, sampling, r, len(got[0]), len(exp[0]))


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
def test_byte_exact_batch_of_three_mixed(sampling):
    """three different images in one call: checks the batch scan and the image offsets"""
    batch = np.stack([jc.black_white_blocks(24, 40), jc.noise(24, 40), jc.flat(24, 40)])
    t = torch.from_numpy(batch).to(DEV)
    for q in jc.QUALITIES:
        for r in jc.restart_values(24, 40, sampling, with_zero=False):
            got = ops.jpeg_encode(t, q, sampling, r)
            exp = ref.jpeg_encode(batch, q, sampling, r)
            assert len(got) == 3 and len({len(g) for g in got}) > 1      # offsets are not uniform
            assert got == exp, (q, sampling, r, [len(g) for g in got], [len(e) for e in exp])


def test_restart_zero_is_refused_on_the_device():
    with pytest.raises(ValueError):
        ops.jpeg_encode(torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV), restart_mcus=0)


def test_input_forms():
    """a non-contiguous view and a DeviceImage give the bytes of the contiguous tensor"""
    from cassmantle_amd.game.content import DeviceImage
    img = jc.hard_cases()["noise_64x48"]
    exp = ref.jpeg_encode(img, 75, "420", 4)
    wide = torch.from_numpy(np.concatenate([img, 255 - img], axis=1)).to(DEV)      # [64, 96, 3]
    view = wide[:, :48]
    assert not view.is_contiguous()
    assert ops.jpeg_encode(view, 75, "420", 4) == exp
    assert ops.jpeg_encode(DeviceImage(view.contiguous()), 75, "420", 4) == exp
    assert ops.jpeg_encode(view.contiguous()[None], 75, "420", 4) == exp


def test_non_default_stream():
    """the encoder works on the current stream: a call inside torch.cuda.stream(s) whose input
    is produced on s gives the same bytes"""
    img = jc.hard_cases()["noise_64x48"]
    exp = ref.jpeg_encode(img, 95, "444", 2)
    s = torch.cuda.Stream()
    host = torch.from_numpy(img).pin_memory()
    with torch.cuda.stream(s):
        t = host.to(DEV, non_blocking=True)           # ordered before the encode only on s
        got = ops.jpeg_encode(t, 95, "444", 2)
    assert got == exp


def test_blur_jpeg_fn_end_to_end():
    """build_blur_jpeg_fn on a 64x64 image, radii {0.25, 2, 15}: each output decodes and is
    within the fidelity bound of a PIL encode of ops.gaussian_blur's output for that radius"""
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn
    cfg = Config()
    assert build_blur_jpeg_fn(cfg, DEV) is None                  # off by default
    cfg.model.gpu_jpeg = True
    fn = build_blur_jpeg_fn(cfg, DEV)
    img = jc.background_crop()
    radii = [0.25, 2.0, 15.0]
    restart = cfg.model.jpeg_restart_mcus or 64 // 16            # default 0: one MCU row
    outs = fn(img, radii, 75)
    assert len(outs) == 3
    x = torch.from_numpy(img).to(DEV)
    for r, data in zip(radii, outs):
        blurred = ops.gaussian_blur(x, r).cpu().numpy()
        ours = jc.decode(data)
        assert ours.shape == (64, 64, 3)
        pil = jc.decode(jc.pil_encode(blurred, 75, "420", restart))
        deficit = jc.psnr(pil, blurred) - jc.psnr(ours, blurred)
        print(f"radius {r}: deficit {deficit:.3f} dB, {len(data)} bytes")
        assert deficit <= jc.MAX_DEFICIT_DB, (r, deficit)
        assert data == ref.jpeg_encode(blurred, 75, "420", restart)[0]


def test_room_flow_serves_device_encoded_buckets():
    """gpu_jpeg=True, a generator whose images stay in HBM (DeviceImage): after the round
    boundary's prewarm every bucket is a decodable JPEG of the right size, radius 0 is the
    stored original, and /fetch/contents serves a device-encoded bucket"""
    from fastapi.testclient import TestClient
    from cassmantle_amd.api.app import create_app
    from cassmantle_amd.game.content import DeviceImage, ImageGenerator
    from cassmantle_amd.game.service import GameService
    from cassmantle_amd.runtime.factory import build_blur_fn, build_blur_jpeg_fn
    from cassmantle_amd.scoring.batcher import BatchingScorer
    from cassmantle_amd.scoring.wordvec import WordVectorBackend

    class HbmGenerator(ImageGenerator):
        resolution = 64

        def generate(self, prompts, negative_prompt, seeds):
            return [DeviceImage(torch.from_numpy(jc.noise(64, 64, seed=s % 7)).to(DEV)) for s in seeds]

    cfg = Config()
    cfg.game.rate_limit_enabled = False
    cfg.game.blur_bucket = 1.0
    cfg.model.gpu_jpeg = True
    backend = WordVectorBackend(vocab=["lantern", "tower"], vectors=np.eye(2, dtype=np.float32))
    svc = GameService(cfg, BatchingScorer(backend, cfg.game.min_score), image_gen_for_room=lambda rid: HbmGenerator(),
                      seed=0, blur_fn=build_blur_fn(cfg, DEV), blur_jpeg_fn=build_blur_jpeg_fn(cfg, DEV))
    client = TestClient(create_app(svc, cfg, run_timers=False))
    with client:
        room = svc.room("")
        client.portal.call(room.buffer_contents)
        client.portal.call(room.end_round)
        cache = room.blur_cache
        deadline = time.time() + 60
        while len(cache) < 16 and time.time() < deadline:     # 0..15 in 1.0 buckets
            time.sleep(0.02)
        assert len(cache) == 16
        with cache._lock:
            items = dict(cache._lru)
        original = [v for (ver, r), v in items.items() if r == 0]
        assert len(original) == 1 and b"\xff\xdd" not in original[0]       # PIL's bytes, no DRI
        for (ver, r), data in items.items():
            assert jc.decode(data).shape == (64, 64, 3)
            assert (b"\xff\xdd" in data) == (r > 0)                        # DRI: the device encoder's
        client.get("/init")
        hits = cache.hits
        served = base64.b64decode(client.get("/fetch/contents").json()["image"])
        assert cache.hits == hits + 1 and served in items.values() and b"\xff\xdd" in served
        assert jc.decode(served).shape == (64, 64, 3)
