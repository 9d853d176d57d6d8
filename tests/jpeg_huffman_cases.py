"""Inputs shared by the tests of the optimised Huffman tables (test_jpeg_huffman*.py): the images
whose PIL ``optimize=True`` streams are the oracle, the skewed image whose chroma AC table needs
the 16-bit length limit, and the frequency vectors of the native test."""
from __future__ import annotations

import io
import os
from functools import lru_cache

import numpy as np
from PIL import Image, ImageFilter

import jpeg_cases as jc
from cassmantle_amd.ops import jpeg_format as jf

ORACLE_QUALITIES = (10, 75, 95, 100)


def pil_optimized(img: np.ndarray, quality: int, sampling: str) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling={"420": 2, "444": 0}[sampling],
                              optimize=True)
    return buf.getvalue()


def background_blurred(side: int) -> np.ndarray:
    img = Image.open(os.path.join(jc.ROOT, "cassmantle_amd", "media", "background.png")).convert("RGB")
    return np.asarray(img.resize((side, side), Image.BICUBIC).filter(ImageFilter.GaussianBlur(7.5)))


def skewed(step: int = 2, fall: float = 2.0) -> np.ndarray:
    """256 x 256 of value 128 plus uniform noise in row bands: heights 1, step, step^2, ... with
    amplitudes 127, 127 / fall, ...: symbol counts that fall off geometrically, so that at 4:4:4,
    quality 100 the chroma AC table has codes longer than 16 bits before they are limited."""
    rng = np.random.default_rng(5)
    img = np.full((256, 256, 3), 128.0)
    y, h, a = 0, 1, 127.0
    while y < 256:
        hh = min(h, 256 - y)
        img[y:y + hh] += rng.uniform(-a, a, (hh, 256, 3))
        y, h, a = y + hh, h * step, a / fall
    return np.clip(img.round(), 0, 255).astype(np.uint8)


@lru_cache(maxsize=None)
def oracle_images():
    return {
        "background_64": background_blurred(64),
        "background_200": background_blurred(200),
        "noise_48x40": jc.noise(48, 40),
        "noise_96": jc.noise(96, 96),
        "flat_16": jc.flat(16, 16),
        "noise_1x1": jc.noise(1, 1),
    }


@lru_cache(maxsize=None)
def oracle():
    """[(name, PIL's optimised stream parsed, its coefficients)]: every oracle image x quality x
    sampling, and the two skewed images at 4:4:4, quality 100."""
    out = []
    for name, img in oracle_images().items():
        for q in ORACLE_QUALITIES:
            for s in jc.SAMPLINGS:
                st = jf.parse(pil_optimized(img, q, s))
                out.append((f"{name}-q{q}-{s}", st, jf.entropy_decode(st)))
    for name, img in (("skewed_2", skewed()), ("skewed_3", skewed(3, 2.5))):
        st = jf.parse(pil_optimized(img, 100, "444"))
        out.append((name, st, jf.entropy_decode(st)))
    return out


def frequency_vectors(n: int = 2000, seed: int = 11):
    """uint32 [n + extras, 256]: fixed-seed random vectors (dense, sparse, heavy-tailed), then all
    zero, one symbol, two symbols, and Fibonacci-skewed ones (30 symbols: lengths up to 30, limited
    to 16; 40 symbols: a code longer than 32 bits, refused)."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            v = rng.integers(0, 1000, 256)
        elif kind == 1:
            v = rng.integers(0, 1 << 20, 256) * (rng.random(256) < 0.1)
        elif kind == 2:
            # log-uniform up to e^14: codes longer than 16 bits before the limit, the sum below 2^31
            v = np.floor(np.exp(rng.uniform(0, 14, 256))).astype(np.int64) * (rng.random(256) < 0.5)
        else:
            v = rng.integers(0, 4, 256)
        rows.append(v)
    z = np.zeros(256, dtype=np.int64)
    one = z.copy(); one[0x21] = 7
    one1 = z.copy(); one1[255] = 1
    two = z.copy(); two[0] = 1; two[255] = 1
    rows += [z, one, one1, two]
    fib = [1, 2]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for k, at in ((30, 0), (30, 200), (40, 3)):
        v = z.copy()
        v[at: at + k] = fib[:k]
        rows.append(v)
        rows.append(v[::-1].copy())
    return np.stack(rows).astype(np.uint32)
