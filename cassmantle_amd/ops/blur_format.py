"""PIL's ``ImageFilter.GaussianBlur`` in numpy, bit for bit: the reference of the BLUR CONTRACT
written down in ``ops/csrc/blur_pil.hip`` (``ops.reference.gaussian_blur_pil``).

Pillow's "Gaussian" is three box-blur passes along the rows and three along the columns
(``BoxBlur.c``).  A box of fractional radius ``fr`` has 2r + 1 full taps of weight ``ww`` and two
edge taps of weight ``fw`` in 2^-24 fixed point; every pass rounds to uint8 and reads pixels
outside the line as the edge pixel of ITS input.  The oracle of this file is the installed
Pillow (tests/test_blur_pil.py), not the formulas.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

PASSES = 3
ONE = 1 << 24
IDENTITY = (0, ONE, 0)         # the box of radius 0: one full-weight tap


def box_params(radius: float) -> Tuple[int, int, int]:
    """Gaussian radius -> (r, ww, fw) of the box every pass applies: r full taps per side of
    weight ww, one edge tap per side of weight fw.  Each step is rounded to float32 where
    Pillow's C code computes in ``float``."""
    f = np.float32
    radius = f(radius)
    if not radius > 0:
        raise ValueError("box_params: radius > 0 expected (radius <= 0 is the identity)")
    s2 = f(f(radius * radius) / f(PASSES))
    L = f(math.sqrt(12.0 * float(s2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))                                   # noqa: E741
    a = f(f(f(f(2) * l) + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * s2)))
    a = f(a / f(f(6) * f(s2 - f(f(l + f(1)) * f(l + f(1))))))
    fr = f(l + a)
    r = int(fr)
    ww = int(f(ONE) / f(f(fr * f(2)) + f(1))) & 0xFFFFFFFF
    fw = (ONE - (2 * r + 1) * ww) // 2
    return r, ww, fw


def _box_pass(x: np.ndarray, r: int, ww: int, fw: int) -> np.ndarray:
    """One pass along axis 1 of uint8 [lines, n, C] (window sums as prefix-sum differences)."""
    n = x.shape[1]
    idx = np.clip(np.arange(-r - 1, n + r + 1), 0, n - 1)
    p = x[:, idx].astype(np.int64)                                  # p[j] = in[clamp(j - r - 1)]
    cs = np.concatenate([np.zeros_like(p[:, :1]), np.cumsum(p, axis=1)], axis=1)
    full = cs[:, 2 * r + 2: 2 * r + 2 + n] - cs[:, 1: 1 + n]        # sum of in[x - r .. x + r]
    edges = p[:, :n] + p[:, 2 * r + 2: 2 * r + 2 + n]               # in[x - r - 1] + in[x + r + 1]
    acc = ww * full + fw * edges + (1 << 23)
    assert int(acc.max()) < (1 << 32)                               # the 32-bit word of the kernels
    return (acc >> 24).astype(np.uint8)


def _blur_one(img: np.ndarray, radius: float) -> np.ndarray:
    if not radius > 0:
        return img.copy()
    r, ww, fw = box_params(radius)
    x = img
    for _ in range(PASSES):
        x = _box_pass(x, r, ww, fw)
    x = x.transpose(1, 0, 2)
    for _ in range(PASSES):
        x = _box_pass(x, r, ww, fw)
    return np.ascontiguousarray(x.transpose(1, 0, 2))


def gaussian_blur_pil(img, radii):
    """``Image.filter(GaussianBlur(radius))`` of a uint8 ``[H, W, 3]`` image, exactly: ``[H, W, 3]``
    for a scalar radius, ``[n, H, W, 3]`` for a sequence (radius <= 0: the input).  A tensor gives
    a tensor on its device, anything else a numpy array."""
    tensor = hasattr(img, "detach")
    a = img.detach().cpu().numpy() if tensor else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[-1] != 3 or a.size == 0:
        raise ValueError("gaussian_blur_pil: uint8 [H, W, 3] expected")
    scalar = np.ndim(radii) == 0
    rs = [float(radii)] if scalar else [float(r) for r in radii]
    cache: dict = {}
    for r in rs:
        if r not in cache:
            cache[r] = _blur_one(a, r)
    out = cache[rs[0]] if scalar else (np.stack([cache[r] for r in rs]) if rs
                                       else np.empty((0, *a.shape), dtype=np.uint8))
    if tensor:
        import torch
        return torch.from_numpy(np.ascontiguousarray(out)).to(img.device)
    return out
