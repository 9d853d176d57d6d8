"""Inputs shared by test_blur_pil.py (CPU) and test_blur_pil_gpu.py: the images on which an
integer box blur can go wrong (rounding on halves, a weight sum past 2^24, borders, lines
shorter than the box) and the radii of the blur cache's buckets."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
from PIL import Image, ImageFilter

NOISE_SEED = 11
BUCKET_RADII = tuple(i * 0.25 for i in range(1, 61))            # the default cache: 0.25 .. 15.0
EXTRA_RADII = (0.1, 1.0 / 3.0, 2.9, 20.0, 31.7, 48.0)
NOISE_SIZES = ((7, 5), (1, 9), (9, 1), (33, 64), (16, 100))      # (H, W)


def noise(H: int, W: int, seed: int = NOISE_SEED) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def checkerboard(H: int, W: int) -> np.ndarray:
    """0 / 255 one-pixel checkerboard: window sums land on halves, where the rounding shows"""
    y, x = np.mgrid[0:H, 0:W]
    v = (((y + x) % 2) * 255).astype(np.uint8)
    return np.repeat(v[..., None], 3, -1)


def flat255(H: int, W: int) -> np.ndarray:
    """a weight sum over 2^24, or a carry out of 32 bits, would show here"""
    return np.full((H, W, 3), 255, dtype=np.uint8)


def impulses(H: int, W: int) -> np.ndarray:
    """single 255 impulses in a black image: the four corners and the centre (one channel each,
    so a channel mix-up shows too)"""
    a = np.zeros((H, W, 3), dtype=np.uint8)
    for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2))):
        a[y, x, i % 3] = 255
    return a


def ramp(H: int, W: int) -> np.ndarray:
    x = np.round(255.0 * np.arange(W) / max(W - 1, 1)).astype(np.uint8)
    row = np.stack([x, 255 - x, x // 2], -1)
    return np.broadcast_to(row[None], (H, W, 3)).copy()


BUILDERS = {"noise": noise, "checkerboard": checkerboard, "flat255": flat255, "impulses": impulses, "ramp": ramp}


@lru_cache(maxsize=None)
def image(name: str, H: int, W: int) -> np.ndarray:
    a = BUILDERS[name](H, W)
    a.setflags(write=False)
    return a


def pil_blur(img: np.ndarray, radius: float) -> np.ndarray:
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).filter(ImageFilter.GaussianBlur(radius)))
