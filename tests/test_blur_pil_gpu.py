"""HIP PIL-exact blur (ops/csrc/blur_pil.hip) on the GPU: bit-exact against the numpy reference
(which test_blur_pil.py holds equal to Pillow) over blur_cases.py, the batched call, input forms,
the current-stream rule, and the point of the feature: with ``blur_kernel=pil`` a GPU process
and a PIL process serve the same bytes.  Every comparison is equality."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import blur_cases as bc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILED_RADII = (0.25, 0.5, 1.0, 2.75, 7.5, 15.0)        # box radius 0 .. 14: the LDS-tiled kernel
GENERAL_RADII = (20.0, 31.7)                           # box radius 19, 31: the one-pass kernels
# smaller than a tile (64 x 64) and than the radius; one tile exactly wide; 40 x 130: three tiles
# across, the last two pixels wide, so the halo of the middle one (45 pixels at radius 15) reaches
# past its whole neighbour to the border; 80 x 72: two tiles each way; 136 x 200: three tiles down
# and four across with interior tiles, the last ones 8 wide
SIZES = ((7, 5), (1, 9), (9, 1), (33, 64), (40, 130), (80, 72), (136, 200))
CASES = [(n, H, W) for H, W in SIZES for n in ("noise", "impulses")] + \
        [(n, H, W) for H, W in ((33, 64), (80, 72)) for n in ("checkerboard", "flat255")]


@pytest.fixture(autouse=True)
def _hip_mode():
    ops.set_mode("hip")
    yield


@lru_cache(maxsize=None)
def expected(name: str, H: int, W: int, radii: tuple) -> np.ndarray:
    e = ref.gaussian_blur_pil(bc.image(name, H, W), radii)
    e.setflags(write=False)
    return e


def dev_image(name: str, H: int, W: int) -> torch.Tensor:
    return torch.from_numpy(bc.image(name, H, W).copy()).to(DEV)


def test_the_radii_take_both_paths():
    rmax = ops.ext().blur_pil_max_tiled_radius()
    assert all(ref.box_params(r)[0] <= rmax for r in TILED_RADII)
    assert all(ref.box_params(r)[0] > rmax for r in GENERAL_RADII)


@pytest.mark.parametrize("name,H,W", CASES, ids=[f"{n}_{h}x{w}" for n, h, w in CASES])
def test_bit_exact_against_reference(name, H, W):
    """single calls, one radius each"""
    x = dev_image(name, H, W)
    radii = TILED_RADII + GENERAL_RADII
    exp = expected(name, H, W, radii)
    bad = []
    for i, r in enumerate(radii):
        got = ops.gaussian_blur_pil(x, r)
        assert got.shape == (H, W, 3) and got.dtype == torch.uint8 and got.device.type == "cuda"
        if not np.array_equal(got.cpu().numpy(), exp[i]):
            bad.append(r)
    assert bad == []


def test_batch_unsorted_with_repeat_and_zero():
    radii = [7.5, 0.25, 15.0, 7.5, 0, 2.75]
    x = dev_image("noise", 40, 130)
    got = ops.gaussian_blur_pil(x, radii)
    assert got.shape == (6, 40, 130, 3)
    for i, r in enumerate(radii):
        assert torch.equal(got[i], ops.gaussian_blur_pil(x, r)), r
    assert np.array_equal(got.cpu().numpy(), expected("noise", 40, 130, tuple(radii)))
    assert torch.equal(got[4], x) and got[4].data_ptr() != x.data_ptr()


def test_batch_into_a_preallocated_buffer():
    radii = [7.5, 0.25, 15.0, 7.5, 0, 2.75]
    x = dev_image("noise", 40, 130)
    out = torch.full((7, 40, 130, 3), 0xA5, dtype=torch.uint8, device=DEV)
    got = ops.gaussian_blur_pil(x, radii, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape[0] == 6
    assert np.array_equal(out[:6].cpu().numpy(), expected("noise", 40, 130, tuple(radii)))
    assert bool((out[6] == 0xA5).all())
    one = torch.full((40, 130, 3), 0xA5, dtype=torch.uint8, device=DEV)
    assert ops.gaussian_blur_pil(x, 2.75, out=one) is one
    assert np.array_equal(one.cpu().numpy(), expected("noise", 40, 130, tuple(radii))[5])
    with pytest.raises(ValueError):
        ops.gaussian_blur_pil(x, radii, out=out.transpose(1, 2))
    with pytest.raises(RuntimeError):
        ops.gaussian_blur_pil(out[0], radii, out=out)              # the source is never a destination


def test_batch_mixing_tiled_and_general_radii():
    radii = (2.75, 31.7, 0, 15.0, 20.0)
    x = dev_image("noise", 80, 72)
    got = ops.gaussian_blur_pil(x, radii)
    assert np.array_equal(got.cpu().numpy(), expected("noise", 80, 72, radii))


def test_input_forms():
    """a non-contiguous view and a DeviceImage give the bytes of the contiguous tensor"""
    from cassmantle_amd.game.content import DeviceImage
    img = bc.image("noise", 33, 64)
    radii = (1.0, 15.0, 20.0)
    exp = expected("noise", 33, 64, radii)
    wide = torch.from_numpy(np.concatenate([img, 255 - img], axis=1)).to(DEV)      # [33, 128, 3]
    view = wide[:, :64]
    assert not view.is_contiguous()
    assert np.array_equal(ops.gaussian_blur_pil(view, radii).cpu().numpy(), exp)
    assert np.array_equal(ops.gaussian_blur_pil(DeviceImage(view.contiguous()), radii).cpu().numpy(), exp)
    with pytest.raises(ValueError):
        ops.gaussian_blur_pil(view.float(), radii)


def test_non_default_stream():
    """the blur works on the current stream: a call inside torch.cuda.stream(s) whose input is
    produced on s is correct without a device-wide synchronise"""
    img = bc.image("noise", 80, 72)
    radii = (7.5, 0.25, 20.0)
    exp = expected("noise", 80, 72, radii)
    ops.gaussian_blur_pil(dev_image("noise", 80, 72), radii)      # the parameter table is uploaded
    s = torch.cuda.Stream()
    host = torch.from_numpy(img.copy()).pin_memory()
    with torch.cuda.stream(s):
        t = host.to(DEV, non_blocking=True)           # ordered before the blur only on s
        got = ops.gaussian_blur_pil(t, radii)
        got = got.cpu()
    assert np.array_equal(got.numpy(), exp)


# ----------------------------------------------------------------------------- serving parity
def _pil_config() -> Config:
    cfg = Config()
    cfg.model.blur_kernel = "pil"
    return cfg


def test_gpu_cache_and_pil_cache_serve_the_same_bytes():
    """blur_kernel=pil: a BlurCache that blurs on the GPU and one that blurs with PIL, prewarmed
    from the same stored JPEG, hold byte-identical JPEGs in all 61 buckets"""
    from cassmantle_amd.game.imaging import BlurCache, encode_jpeg
    from cassmantle_amd.runtime.factory import build_blur_fn
    cfg = _pil_config()
    jpeg = encode_jpeg(bc.image("noise", 48, 64))
    a = BlurCache(blur_fn=build_blur_fn(cfg, DEV))
    b = BlurCache()
    assert a.prewarm("v1", jpeg, 15.0) == 61 and b.prewarm("v1", jpeg, 15.0) == 61
    assert len(a) == 61 and list(a._lru.keys()) == list(b._lru.keys())
    differ = [key for key in a._lru if a._lru[key] != b._lru[key]]
    assert differ == []
    assert len(set(a._lru.values())) > 50                       # the buckets are different pictures


def test_gpu_jpeg_buckets_are_the_encode_of_pil_pixels():
    """with gpu_jpeg as well: every byte string of the one-launch blur + device encode is the
    reference encoder's output for PIL's blurred pixels"""
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn
    cfg = _pil_config()
    cfg.model.gpu_jpeg = True
    fn = build_blur_jpeg_fn(cfg, DEV)
    img = bc.image("noise", 48, 64)
    radii = list(bc.BUCKET_RADII)
    restart = cfg.model.jpeg_restart_mcus or (64 + 15) // 16
    outs = fn(img, radii, 75)
    assert len(outs) == len(radii)
    for r, data in zip(radii, outs):
        assert data == ref.jpeg_encode(bc.pil_blur(img, r), 75, "420", restart)[0], r


def test_default_blur_fn_is_unchanged():
    from cassmantle_amd.runtime.factory import build_blur_fn
    cfg = Config()
    assert cfg.model.blur_kernel == "gaussian"
    img = bc.image("noise", 48, 64)
    x = torch.from_numpy(img.copy()).to(DEV)
    fn = build_blur_fn(cfg, DEV)
    for r in (0.25, 7.5):
        assert np.array_equal(fn(img, r), ops.gaussian_blur(x, r).cpu().numpy())
