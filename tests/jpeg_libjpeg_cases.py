"""Inputs shared by the tests of the libjpeg forward contract (test_jpeg_libjpeg*.py): the smallest
images that reach every rule by which libjpeg's encoder differs from the matrix transform.

Sizes (H x W) and the rule each is there for:
  8x8, 24x40                   the chroma bottom rule (H even, no multiple of 16: the chroma rows
                               below ceil(H/2) repeat the last downsampled row)
  9x7, 17x33, 33x16, 48x23     dummy luma blocks and odd sizes (a chroma mean over a replicated row
                               or column)
  1x1                          the chained dummy DC (Y01, Y10, Y11 all carry Y00's DC)
  2x2, 16x16                   the smallest even image and a whole MCU (no edge rule at all)
"""
from __future__ import annotations

import io
from functools import lru_cache

import numpy as np
from PIL import Image, ImageFilter

SIZES = ((1, 1), (2, 2), (8, 8), (9, 7), (16, 16), (17, 33), (24, 40), (33, 16), (48, 23))
QUALITIES = (10, 75, 95, 100)
SAMPLINGS = ("420", "444")
KINDS = ("noise", "blurred", "flat")
FLAT = (255, 0, 37)
SEED = 11


@lru_cache(maxsize=None)
def image(kind: str, H: int, W: int) -> np.ndarray:
    """uint8 [H, W, 3], read-only."""
    if kind == "noise":
        a = np.random.default_rng(SEED + 1000 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "blurred":
        a = np.asarray(Image.fromarray(image("noise", H, W)).filter(ImageFilter.GaussianBlur(1.5))).copy()
    elif kind == "flat":
        a = np.empty((H, W, 3), dtype=np.uint8)
        a[:] = FLAT
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    return a


def cases():
    """(name, image, quality, sampling) of every case: 3 kinds x 9 sizes x 4 qualities x 2 samplings."""
    for kind in KINDS:
        for H, W in SIZES:
            for q in QUALITIES:
                for s in SAMPLINGS:
                    yield f"{kind}_{H}x{W}-q{q}-{s}", image(kind, H, W), q, s


def images():
    """(name, image) of every kind and size."""
    for kind in KINDS:
        for H, W in SIZES:
            yield f"{kind}_{H}x{W}", image(kind, H, W)


@lru_cache(maxsize=None)
def _pil(kind: str, H: int, W: int, quality: int, sampling, optimize: bool) -> bytes:
    buf = io.BytesIO()
    kw = {} if sampling is None else {"subsampling": {"420": 2, "444": 0}[sampling]}
    Image.fromarray(image(kind, H, W)).save(buf, format="JPEG", quality=quality, optimize=optimize, **kw)
    return buf.getvalue()


def pil_bytes(kind: str, H: int, W: int, quality: int, sampling, optimize: bool = False) -> bytes:
    """The file Pillow writes (``sampling=None``: no subsampling argument, Pillow's default).
    Computed once per case and shared."""
    return _pil(kind, H, W, int(quality), sampling, bool(optimize))


def pil_encode(img: np.ndarray, quality: int, sampling: str = "420", optimize: bool = False) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.asarray(img)).save(buf, format="JPEG", quality=quality, optimize=optimize,
                                          subsampling={"420": 2, "444": 0}[sampling])
    return buf.getvalue()


def decode(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB"
    return np.asarray(im)


def extremal_blocks():
    """int [126, 8, 8] level-shifted blocks: samples in {0, 255} following the sign of every DCT
    basis function but the constant one, and their negatives (63 x 2): the blocks that drive one
    coefficient to its largest magnitude."""
    n = np.arange(8)
    out = []
    for u in range(8):
        for v in range(8):
            if u == 0 and v == 0:
                continue
            basis = np.outer(np.cos((2 * n + 1) * u * np.pi / 16), np.cos((2 * n + 1) * v * np.pi / 16))
            pos = basis > 0
            out.append(np.where(pos, 255, 0))
            out.append(np.where(pos, 0, 255))
    return np.stack(out)
