"""Streams shared by test_jpeg_entropy_decode.py (CPU), test_jpeg_entropy_native.py (the host
program) and test_jpeg_entropy_decode_gpu.py: the corpus of baseline JPEGs the entropy decode
contract is checked on, the crafted streams at the edge of the refusal rule, and the malformed
streams; with the reference results computed once.  Everything is deterministic."""
from __future__ import annotations

import io
from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np
from PIL import Image

import jpeg_cases as jc
from cassmantle_amd.ops import jpeg_format as jf

SIZES = ((1, 1), (8, 8), (16, 16), (17, 33), (9, 7), (48, 40), (5, 3), (6, 4), (64, 64), (100, 75))
PIL_QUALITIES = (10, 50, 75, 95, 100)
PIL_VARIANTS = ({"optimize": True}, {"subsampling": 0}, {"restart_marker_blocks": 2}, {"restart_marker_rows": 1})
INTREE_SIZES = ((17, 33), (9, 7), (48, 40), (64, 64))


class Stream(NamedTuple):
    name: str
    data: bytes
    img: Optional[np.ndarray] = None      # in-tree streams: the image, quality and sampling they encode
    quality: int = 0
    sampling: str = ""


def _pil_save(img: np.ndarray, **kw) -> Optional[bytes]:
    """None when this Pillow rejects a restart_marker_* keyword"""
    buf = io.BytesIO()
    try:
        Image.fromarray(img).save(buf, format="JPEG", **kw)
    except TypeError:
        if any(k.startswith("restart_marker") for k in kw):
            return None
        raise
    data = buf.getvalue()
    if any(k.startswith("restart_marker") for k in kw) and b"\xff\xdd" not in data:
        return None                       # keyword ignored: no DRI written
    return data


@lru_cache(maxsize=None)
def pil_streams():
    """Pillow-written: every size as noise and as a gradient, five qualities, and at quality 75
    optimised Huffman tables, 4:4:4, and restart markers every 2 MCUs / every MCU row"""
    out = []
    for H, W in SIZES:
        for kind, img in (("noise", jc.noise(H, W, seed=H * 131 + W)), ("gradient", jc.gradient(H, W))):
            for q in PIL_QUALITIES:
                out.append(Stream(f"pil_{kind}_{H}x{W}_q{q}", _pil_save(img, quality=q)))
            for kw in PIL_VARIANTS:
                data = _pil_save(img, quality=75, **kw)
                if data is not None:
                    out.append(Stream(f"pil_{kind}_{H}x{W}_" + "_".join(f"{k}{int(v)}" for k, v in kw.items()), data))
    return tuple(out)


@lru_cache(maxsize=None)
def intree_streams():
    """jf.jpeg_encode's: both samplings, restart_mcus 0..4, four sizes; and the smallest stream
    with two thread blocks of intervals (144x144 4:2:0, one MCU per interval: 81)"""
    out = []
    for H, W in INTREE_SIZES:
        img = jc.noise(H, W, seed=H + W)
        for sampling in jc.SAMPLINGS:
            for r in range(5):
                out.append(Stream(f"intree_{H}x{W}_{sampling}_r{r}", jf.jpeg_encode(img, 75, sampling, r)[0],
                                  img, 75, sampling))
    img = jc.noise(144, 144, seed=144)
    out.append(Stream("intree_144x144_420_r1", jf.jpeg_encode(img, 75, "420", 1)[0], img, 75, "420"))
    return tuple(out)


@lru_cache(maxsize=None)
def batch_streams():
    """three in-tree streams of one geometry (24x40, 4:2:0, 2 MCUs per interval)"""
    imgs = [jc.black_white_blocks(24, 40), jc.noise(24, 40), jc.flat(24, 40)]
    return tuple(Stream(f"batch_{i}", jf.jpeg_encode(im, 75, "420", 2)[0], im, 75, "420") for i, im in enumerate(imgs))


def corpus():
    return pil_streams() + intree_streams()


@lru_cache(maxsize=None)
def pil_pixels(data: bytes) -> np.ndarray:
    out = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def reference(data: bytes):
    """(parsed stream, coefficients, reference pixels, largest intermediate), computed once"""
    st = jf.parse(data)
    coef = jf.entropy_decode(st)
    stats = {}
    px = jf.reconstruct(coef, st.H, st.W, 0, st.sampling, stats, tables=st.qtables)
    coef.setflags(write=False)
    px.setflags(write=False)
    return st, coef, px, stats["max_abs"]


# ----------------------------------------------------------------------------- crafted streams
def craft(coef: np.ndarray, quality: int, H: int = 8, W: int = 8, sampling: str = "444", restart: int = 0) -> bytes:
    """a valid in-tree stream of hand-made coefficients int16 [mcus, nb, 64] (zig-zag)"""
    scan, _ = jf.entropy(np.asarray(coef, dtype=np.int16), restart)
    return jf.header(H, W, quality, sampling, restart) + scan + b"\xff\xd9"


def _orthonormal_dct() -> np.ndarray:
    c = jf.dct_matrix().astype(np.float64)
    return c / np.sqrt((c ** 2).sum(1, keepdims=True))


def _block(nat: np.ndarray) -> np.ndarray:
    """natural-order 8x8 luma block -> coefficients of one 4:4:4 MCU"""
    c = np.zeros((1, 3, 64), dtype=np.int16)
    c[0, 0] = np.rint(nat).astype(np.int64).reshape(64)[jf.ZIGZAG]
    return c


def block_norm(data: bytes) -> float:
    """the largest dequantised L2 norm of a block of a stream (of its coefficients as coded)"""
    st = jf.parse(data)
    saved = jf.WIDE_T
    jf.WIDE_T = 1 << 20                   # decoded with the rule switched off
    try:
        coef = jf.entropy_decode(st).astype(np.int64)
    finally:
        jf.WIDE_T = saved
    _, nb, _, _ = jf.geometry(st.H, st.W, st.sampling)
    qz = np.asarray([[t[jf.ZIGZAG[z]] for z in range(64)] for t in st.qtables], dtype=np.int64)
    q = np.stack([qz[0]] * (nb - 2) + [qz[1]] * 2)
    return float(np.sqrt(((coef * q) ** 2).sum(-1)).max())


@lru_cache(maxsize=None)
def energy_streams():
    """(name, bytes, target norm): blocks whose first-pass outputs and their pairwise sums are as
    large as a given norm allows (one or two coefficient columns carrying a vertical impulse, the
    worst case of libjpeg's 16-bit SIMD words), and DC-only blocks; quality 100 (Q = 1) except the
    DC blocks (quality 50: Q = 16)."""
    C = _orthonormal_dct()
    out = []
    for target in (2040, 2100):
        for sign in (1, -1):
            for r in (0, 3):
                for cols in ((3, 7), (1, 5), (3,)):
                    if len(cols) == 1 and target * 0.4904 > 1023:      # AC magnitudes stop at 1023
                        continue
                    amp = target / np.sqrt(len(cols))
                    d = np.zeros((8, 8))
                    for c in cols:
                        d[:, c] = C[:, r] * amp * sign
                    name = f"energy_{target}_{'p' if sign > 0 else 'n'}_r{r}_c{''.join(map(str, cols))}"
                    out.append((name, craft(_block(d), 100), target))
    for dc in (127, -127, 128, -128):          # 16 * 127 = 2032 <= T < 2048 = 16 * 128
        d = np.zeros((8, 8))
        d[0, 0] = dc
        out.append((f"energy_dc{dc}", craft(_block(d), 50), 16 * abs(dc)))
    return tuple(out)


# ----------------------------------------------------------------------------- malformed streams
class Malformed(NamedTuple):
    name: str
    data: bytes
    code: int


def _truncated() -> Malformed:
    """the last interval loses its last three bytes: a symbol is cut"""
    data = jf.jpeg_encode(jc.noise(17, 33, seed=50), 75, "420", 2)[0]
    assert data[-2:] == b"\xff\xd9" and 0xFF not in data[-6:-2]
    return Malformed("truncated", data[:-5] + data[-2:], jf.TRUNCATED)


def _bad_code() -> Malformed:
    """the first single-bit flip of a Pillow optimize=True stream (its Huffman tables leave codes
    unassigned) after which the decoder meets 16 bits that start no code word"""
    data = _pil_save(jc.noise(16, 16, seed=7), quality=75, optimize=True)
    st = jf.parse(data)
    off, ln = st.intervals[0]
    for bit in range(8 * ln):
        b = bytearray(data)
        b[off + bit // 8] ^= 0x80 >> (bit % 8)
        try:
            jf.entropy_decode(jf.parse(bytes(b)))
        except jf.JpegError as e:
            if e.code == jf.BAD_CODE:
                return Malformed("bad_code", bytes(b), jf.BAD_CODE)
        except jf.JpegUnsupported:
            pass
    raise AssertionError("no bit flip gives BAD_CODE")


def _overrun() -> Malformed:
    """three ZRL symbols (k = 49), then a run of 15 before a coefficient: k = 64"""
    h = jf.huff_table()
    w = jf._Bits()
    w.put(int(h[0]) & 0xFFFF, int(h[0]) >> 16)                 # DC category 0
    for sym in (0xF0, 0xF0, 0xF0, 0xF1):
        e = int(h[32 + sym])
        w.put(e & 0xFFFF, e >> 16)
    w.put(1, 1)
    for _ in range(4):
        w.put(0xA5, 8)
    w.flush()
    return Malformed("overrun", jf.header(8, 8, 75, "444", 0) + bytes(w.out) + b"\xff\xd9", jf.OVERRUN)


@lru_cache(maxsize=None)
def malformed():
    return (_truncated(), _bad_code(), _overrun())
