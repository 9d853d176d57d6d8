"""PIL's GaussianBlur as integer box passes (ops/blur_format.py, the contract of
ops/csrc/blur_pil.hip) on the CPU: the numpy reference equals the installed Pillow exactly, its
properties, and the ``blur_kernel`` wiring.  Every comparison is equality."""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

import blur_cases as bc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.ops import reference as ref
from cassmantle_amd.runtime import factory

RADII = bc.BUCKET_RADII + bc.EXTRA_RADII
CASES = [("noise", H, W) for H, W in bc.NOISE_SIZES] + [(n, 33, 64) for n in bc.BUILDERS if n != "noise"]


@pytest.mark.parametrize("name,H,W", CASES, ids=[f"{n}_{h}x{w}" for n, h, w in CASES])
def test_reference_equals_pillow(name, H, W):
    """every bucket radius 0.25 .. 15.0 and 0.1, 1/3, 2.9, 20.0, 31.7, 48.0 (lines shorter than
    the box included)"""
    img = bc.image(name, H, W)
    got = ref.gaussian_blur_pil(img, RADII)
    assert got.shape == (len(RADII), H, W, 3) and got.dtype == np.uint8
    bad = [r for i, r in enumerate(RADII) if not np.array_equal(got[i], bc.pil_blur(img, r))]
    assert bad == []


def test_radius_zero_returns_the_input():
    img = bc.image("noise", 7, 5)
    assert np.array_equal(ref.gaussian_blur_pil(img, 0), img)
    assert np.array_equal(ref.gaussian_blur_pil(img, [0, -1.0])[1], img)
    assert np.array_equal(bc.pil_blur(img, 0), img)


def test_box_weights_sum_to_one():
    """2^24 - 1 <= (2r + 1) ww + 2 fw <= 2^24: the accumulator of a pass fits in 32 unsigned bits"""
    for radius in RADII:
        r, ww, fw = ref.box_params(radius)
        assert r >= 0 and ww > 0 and fw >= 0, radius
        assert (1 << 24) - 1 <= (2 * r + 1) * ww + 2 * fw <= 1 << 24, (radius, r, ww, fw)
    with pytest.raises(ValueError):
        ref.box_params(0)


def test_flat_255_stays_flat():
    img = bc.image("flat255", 33, 64)
    assert (ref.gaussian_blur_pil(img, RADII) == 255).all()


def test_scalar_and_sequence_forms_agree():
    img = bc.image("noise", 33, 64)
    seq = ref.gaussian_blur_pil(img, [2.75, 0, 7.5])
    assert seq.shape == (3, 33, 64, 3)
    for i, r in enumerate((2.75, 0, 7.5)):
        one = ref.gaussian_blur_pil(img, r)
        assert one.shape == (33, 64, 3) and np.array_equal(one, seq[i])
    t = ref.gaussian_blur_pil(torch.from_numpy(img.copy()), [2.75])
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy()[0], seq[0])


def test_wrong_dtype_or_shape_raises():
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8),
                np.zeros((1, 4, 4, 3), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            ref.gaussian_blur_pil(bad, 1.0)
        with pytest.raises(ValueError):
            ops.gaussian_blur_pil(torch.from_numpy(bad), 1.0)


def test_dispatch_on_the_cpu_is_the_reference():
    """a CPU tensor, and an array, go to the reference; out= is written in place and returned"""
    img = bc.image("noise", 16, 100)
    t = torch.from_numpy(img.copy())
    radii = [7.5, 0.25, 0, 20.0]
    exp = ref.gaussian_blur_pil(img, radii)
    assert np.array_equal(ops.gaussian_blur_pil(t, radii).numpy(), exp)
    assert np.array_equal(ops.gaussian_blur_pil(img, radii), exp)
    assert np.array_equal(ops.gaussian_blur_pil(t, 7.5).numpy(), exp[0])
    out = torch.full((5, 16, 100, 3), 0xA5, dtype=torch.uint8)
    got = ops.gaussian_blur_pil(t, radii, out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(out[:4].numpy(), exp) and (out[4] == 0xA5).all()
    for bad in (torch.zeros((3, 16, 100, 3), dtype=torch.uint8), torch.zeros((4, 16, 100, 3)),
                torch.zeros((4, 16, 100, 6), dtype=torch.uint8)[..., :3]):
        with pytest.raises(ValueError):
            ops.gaussian_blur_pil(t, radii, out=bad)


# ----------------------------------------------------------------------------- wiring
def test_config_field_parses_and_defaults_to_gaussian():
    assert Config().model.blur_kernel == "gaussian"
    assert Config.from_args(["--blur_kernel", "pil"]).model.blur_kernel == "pil"


@pytest.mark.parametrize("kernel", ["gaussian", "pil"])
def test_builders_on_the_cpu_are_none_as_before(kernel):
    cfg = Config()
    cfg.model.blur_kernel = kernel
    cfg.model.gpu_jpeg = True
    assert factory.build_blur_fn(cfg, "cpu") is None
    assert factory.build_blur_jpeg_fn(cfg, "cpu") is None


def test_unknown_blur_kernel_raises():
    cfg = Config()
    cfg.model.blur_kernel = "box"
    cfg.model.gpu_jpeg = True
    for build in (factory.build_blur_fn, factory.build_blur_jpeg_fn):
        for dev in ("cpu", "cuda"):
            with pytest.raises(ValueError):
                build(cfg, dev)


def test_pil_blur_jpeg_fn_is_one_blur_call(monkeypatch):
    """60 radii: exactly one ops.gaussian_blur_pil call, whose buffer goes to ops.jpeg_encode"""
    class FakeDeviceTensor:
        device = types.SimpleNamespace(type="cuda")
        shape = (48, 64, 3)

        def to(self, dev, non_blocking=False):
            return self

    calls = {"blur": [], "jpeg": []}
    buffer = object()

    def fake_blur(x, radii, out=None):
        calls["blur"].append((x, list(radii)))
        return buffer

    def fake_jpeg(buf, quality=75, sampling="420", restart_mcus=4, return_decoded=False):
        calls["jpeg"].append((buf, quality, restart_mcus))
        return [b"x"] * 60

    def no_gaussian(*a, **k):
        raise AssertionError("blur_kernel=pil must not call ops.gaussian_blur")

    monkeypatch.setattr(ops, "gaussian_blur_pil", fake_blur, raising=False)
    monkeypatch.setattr(ops, "jpeg_encode", fake_jpeg)
    monkeypatch.setattr(ops, "gaussian_blur", no_gaussian)
    cfg = Config()
    cfg.model.gpu_jpeg = True
    cfg.model.blur_kernel = "pil"
    fn = factory.build_blur_jpeg_fn(cfg, "cuda")
    src = FakeDeviceTensor()
    outs = fn(types.SimpleNamespace(tensor=src), list(bc.BUCKET_RADII), 75)
    assert len(outs) == 60
    assert len(calls["blur"]) == 1 and calls["blur"][0][0] is src and calls["blur"][0][1] == list(bc.BUCKET_RADII)
    assert calls["jpeg"] == [(buffer, 75, 4)]                      # W = 64: one MCU row = 4 MCUs
