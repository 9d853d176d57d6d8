"""Inputs shared by test_jpeg.py (CPU) and test_jpeg_gpu.py: the smallest images that reach every
path of the baseline JPEG coder (partial MCUs, RST index wrap, short last interval, stuffed 0xFF
bytes, ZRL symbols, DC category >= 10, DC + EOB only blocks)."""
from __future__ import annotations

import io
import math
import os
from functools import lru_cache

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (10, 75, 95)
SAMPLINGS = ("420", "444")
# Bounds of the fidelity / size tests: the reference encoder's largest PSNR deficit against PIL's
# own encode, measured on the CPU (test_jpeg.test_fidelity_and_size_against_pil records the
# figures), + 0.2 dB for decoder rounding; its largest size ratio + 2 percentage points.
MAX_DEFICIT_DB = 0.259 + 0.2
MAX_SIZE_RATIO = 0.9983 + 0.02
NOISE_SEED = 3        # chosen so that the q = 95 encode of `noise` has stuffed 0xFF bytes (asserted)


def gradient(H: int, W: int) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    r = 255.0 * x / max(W - 1, 1)
    g = 255.0 * y / max(H - 1, 1)
    b = 255.0 * (x + y) / max(H + W - 2, 1)
    return np.stack([r, g, 255.0 - b], -1).round().astype(np.uint8)


def noise(H: int, W: int, seed: int = NOISE_SEED) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def highest_frequency(H: int, W: int) -> np.ndarray:
    """Grey image whose 8x8 blocks are the (7, 7) DCT basis function: after quantisation the
    only AC energy sits at zig-zag position 63, behind a run of 62 zeros (three ZRL symbols)."""
    c = np.cos((2 * np.arange(8) + 1) * 7 * math.pi / 16)
    blk = 128.0 + 100.0 * np.outer(c, c)
    t = np.tile(blk, ((H + 7) // 8, (W + 7) // 8))[:H, :W]
    return np.repeat(t.round().astype(np.uint8)[..., None], 3, -1)


def black_white_blocks(H: int, W: int) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    v = (((y // 8) + (x // 8)) % 2 * 255).astype(np.uint8)
    return np.repeat(v[..., None], 3, -1)


def flat(H: int, W: int) -> np.ndarray:
    return np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8), (H, W, 3)).copy()


@lru_cache(maxsize=None)
def background_crop() -> np.ndarray:
    img = Image.open(os.path.join(ROOT, "cassmantle_amd", "media", "background.png")).convert("RGB")
    a = np.asarray(img)
    y0, x0 = a.shape[0] // 2 - 32, a.shape[1] // 2 - 32
    return np.ascontiguousarray(a[y0:y0 + 64, x0:x0 + 64])


@lru_cache(maxsize=None)
def hard_cases():
    """name -> image, at the shapes the issue lists (H x W): 8x8, 16x16, 17x33, 24x40, 64x48."""
    return {
        "gradient_8x8": gradient(8, 8),
        "highfreq_16x16": highest_frequency(16, 16),
        "flat_17x33": flat(17, 33),
        "blackwhite_24x40": black_white_blocks(24, 40),
        "noise_64x48": noise(64, 48),
    }


def fidelity_inputs():
    return {"gradient": gradient(64, 64), "background": background_crop(), "noise": noise(64, 64)}


def restart_values(H: int, W: int, sampling: str, with_zero: bool):
    m = 16 if sampling == "420" else 8
    row = (W + m - 1) // m
    vals = [1, 2, 5, row]
    return ([0] if with_zero else []) + list(dict.fromkeys(vals))


def pil_encode(img: np.ndarray, quality: int, sampling: str, restart_mcus: int) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling={"420": 2, "444": 0}[sampling],
                              restart_marker_blocks=restart_mcus)
    return buf.getvalue()


def decode(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB"
    return np.asarray(im)


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 10.0 * math.log10(255.0 ** 2 / max(mse, 1e-12))
