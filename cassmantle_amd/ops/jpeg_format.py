"""Baseline JPEG (JFIF) byte contract shared by the HIP encoder (``ops/csrc/jpeg.hip``) and its
pure numpy reference (:func:`jpeg_encode`, exported as ``ops.reference.jpeg_encode``).

Everything is integer arithmetic with defined rounding, so the kernel and this reference produce
identical coefficients and identical bytes.  The formulas are documented once, in the header
comment of ``jpeg.hip``; this module mirrors them line by line.  The tables (Annex K quantisation
and Huffman tables, zig-zag order) and the header bytes live here only: the kernels receive them
as small device tensors (``ops.jpeg_encode``), so there is one copy of each.
"""
from __future__ import annotations

import struct
from functools import lru_cache
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np

# ----------------------------------------------------------------------------- tables (T.81 Annex K)
_LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
           14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
_CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
             24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])


def _zigzag() -> List[int]:
    """Natural (row-major) index of the coefficient at each zig-zag position."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8,
                                             (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return order


ZIGZAG = _zigzag()                     # ZIGZAG[z] = natural index
SAMPLINGS = ("420", "444")

# 8-point DCT-II matrix in 13-bit fixed point: DCT_A[j] = round(8192 * cos(j*pi/16) / 2) for
# j = 1..7, and 2896 = round(8192 / (2*sqrt(2))) for the DC row (jpeg.hip holds the same 8 numbers)
DCT_A = (2896, 4017, 3784, 3406, 2896, 2276, 1567, 799)
DCT_BITS = 13
PASS1_KEEP = 4                         # fraction bits kept between the row and the column pass
OUT_KEEP = 3                           # fraction bits of the DCT output going into the quantiser


def dct_matrix() -> np.ndarray:
    """C[k][n] = c(k)/2 * cos((2n+1) k pi / 16) * 2^13, folded onto DCT_A by integer symmetry."""
    C = np.zeros((8, 8), dtype=np.int64)
    for k in range(8):
        for n in range(8):
            if k == 0:
                C[k, n] = DCT_A[0]
                continue
            j = ((2 * n + 1) * k) % 32
            if j > 16:
                j = 32 - j
            sign = 1
            if j > 8:
                sign, j = -1, 16 - j
            C[k, n] = 0 if j == 8 else sign * DCT_A[j]
    return C


def quant_tables(quality: int) -> Tuple[List[int], List[int]]:
    """Annex K tables scaled by the libjpeg quality rule, natural order."""
    q = max(1, min(100, int(quality)))
    s = 5000 // q if q < 50 else 200 - 2 * q
    scale = lambda base: [max(1, min(255, (b * s + 50) // 100)) for b in base]   # noqa: E731
    return scale(_LUMA_Q), scale(_CHROMA_Q)


def _huff_codes(bits: Sequence[int], vals: Sequence[int]) -> Dict[int, Tuple[int, int]]:
    """Canonical code assignment (T.81 Annex C): symbol -> (code, length)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


STANDARD_TABLES = (_DC_LUMA, _DC_CHROMA, _AC_LUMA, _AC_CHROMA)      # (bits, vals): DC luma, DC chroma, AC luma, AC chroma
HUFF_BASES = (0, 16, 32, 32 + 256)     # first word of every table in huff_table()
HUFFMAN_MODES = ("standard", "optimized")


def _frozen_tables(tables):
    """Four (bits, vals) as nested tuples (hashable), or None for the standard tables."""
    if tables is None:
        return None
    tables = tuple((tuple(int(b) for b in bits), tuple(int(v) for v in vals)) for bits, vals in tables)
    if len(tables) != 4 or any(len(bits) != 16 or sum(bits) != len(vals) for bits, vals in tables):
        raise ValueError("jpeg: tables = four (bits[16], vals): DC luma, DC chroma, AC luma, AC chroma")
    return tables


@lru_cache(maxsize=64)
def _huff_table(tables) -> np.ndarray:
    t = np.zeros(2 * 16 + 2 * 256, dtype=np.int32)
    for base, (bits, vals) in zip(HUFF_BASES, STANDARD_TABLES if tables is None else tables):
        for sym, (code, length) in _huff_codes(bits, vals).items():
            t[base + sym] = (length << 16) | code
    return t


def huff_table(tables=None) -> np.ndarray:
    """int32 [2*16 + 2*256]: ``(length << 16) | code`` per symbol for DC luma, DC chroma (16
    slots each, 12 used), AC luma, AC chroma (256 each); 0 marks a symbol that has no code.
    ``tables``: four ``(bits, vals)`` (DC luma, DC chroma, AC luma, AC chroma) in place of the
    standard ones."""
    return _huff_table(_frozen_tables(tables))


def geometry(H: int, W: int, sampling: str) -> Tuple[int, int, int, int]:
    """(MCU edge in pixels, blocks per MCU, MCUs per row, MCU rows)."""
    if sampling not in SAMPLINGS:
        raise ValueError(f"sampling={sampling!r}: expected one of {SAMPLINGS}")
    m = 16 if sampling == "420" else 8
    return m, (6 if sampling == "420" else 3), (W + m - 1) // m, (H + m - 1) // m


def _seg(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


TRANSFORMS = ("matrix", "libjpeg")
HEADER_LAYOUTS = ("compact", "pil")    # one DQT and one DHT segment | a segment per table, as libjpeg writes them
DHT_EXTRA_PIL = 3 * 4                  # the three more segment headers of the PIL layout's DHT


def transform_layout(transform: str) -> str:
    """The header layout that goes with a forward transform: ``"libjpeg"`` writes PIL's file."""
    if transform not in TRANSFORMS:
        raise ValueError(f"jpeg: transform must be one of {TRANSFORMS}, not {transform!r}")
    return "pil" if transform == "libjpeg" else "compact"


def header(H: int, W: int, quality: int, sampling: str, restart_mcus: int, tables=None,
           layout: str = "compact") -> bytes:
    """SOI / APP0 / DQT / SOF0 / DHT / DRI / SOS for one image (the entropy-coded data and EOI
    follow).  ``tables``: four ``(bits, vals)`` (DC luma, DC chroma, AC luma, AC chroma) written into
    the one DHT segment in place of the standard ones, in the same order (DC luma, AC luma, DC
    chroma, AC chroma).  ``layout="pil"``: the segments libjpeg (PIL) writes: a DQT segment per
    quantisation table and a DHT segment per Huffman table, in that same order."""
    pre, suf = header_parts(H, W, quality, sampling, restart_mcus, layout)
    return pre + dht_segment(tables, layout) + suf


def dht_segment(tables=None, layout: str = "compact") -> bytes:
    """The DHT segment of four ``(bits, vals)`` (default: the standard tables); with
    ``layout="pil"`` the four segments, one per table."""
    if layout not in HEADER_LAYOUTS:
        raise ValueError(f"jpeg: layout must be one of {HEADER_LAYOUTS}, not {layout!r}")
    t = STANDARD_TABLES if tables is None else _frozen_tables(tables)
    parts = [bytes([tc_th]) + bytes(bits) + bytes(vals)
             for tc_th, (bits, vals) in ((0x00, t[0]), (0x10, t[2]), (0x01, t[1]), (0x11, t[3]))]
    if layout == "pil":
        return b"".join(_seg(0xC4, p) for p in parts)
    return _seg(0xC4, b"".join(parts))


@lru_cache(maxsize=64)
def header_parts(H: int, W: int, quality: int, sampling: str, restart_mcus: int,
                 layout: str = "compact") -> Tuple[bytes, bytes]:
    """(the header bytes before the DHT segment(s), those after): the same for every image of a
    geometry, whatever its Huffman tables."""
    if layout not in HEADER_LAYOUTS:
        raise ValueError(f"jpeg: layout must be one of {HEADER_LAYOUTS}, not {layout!r}")
    if not (0 < H < 65536 and 0 < W < 65536):
        raise ValueError("jpeg: image sides must be in 1..65535")
    if not 0 <= restart_mcus < 65536:
        raise ValueError("jpeg: restart_mcus must be in 0..65535")
    geometry(H, W, sampling)
    lq, cq = quant_tables(quality)
    out = b"\xff\xd8"
    out += _seg(0xE0, b"JFIF\x00\x01\x01\x00" + struct.pack(">HHBB", 1, 1, 0, 0))
    if layout == "pil":
        out += _seg(0xDB, bytes([0]) + bytes(lq[i] for i in ZIGZAG)) + _seg(0xDB, bytes([1]) + bytes(cq[i] for i in ZIGZAG))
    else:
        out += _seg(0xDB, bytes([0]) + bytes(lq[i] for i in ZIGZAG) + bytes([1]) + bytes(cq[i] for i in ZIGZAG))
    hv = 0x22 if sampling == "420" else 0x11
    out += _seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    suf = b""
    if restart_mcus:
        suf += _seg(0xDD, struct.pack(">H", restart_mcus))
    suf += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out, suf


# ----------------------------------------------------------------------------- transform
def _div_floor_shift(x: np.ndarray, sh: int) -> np.ndarray:
    return (x + (1 << (sh - 1))) >> sh        # arithmetic shift: floor((x + half) / 2^sh)


def coefficients(img: np.ndarray, quality: int, sampling: str, transform: str = "matrix",
                 stats: dict = None) -> np.ndarray:
    """uint8 [H, W, 3] -> int16 [mcus, blocks per MCU, 64] quantised zig-zag coefficients.
    ``transform="libjpeg"``: libjpeg's forward path (:func:`coefficients_libjpeg`) in place of the
    matrix DCT of the byte contract; ``stats`` is handed on to it."""
    if transform not in TRANSFORMS:
        raise ValueError(f"jpeg: transform must be one of {TRANSFORMS}, not {transform!r}")
    if transform == "libjpeg":
        return coefficients_libjpeg(img, quality, sampling, stats)
    H, W, _ = img.shape
    m, nb, mx, my = geometry(H, W, sampling)
    # edge replication up to a whole MCU
    ys = np.minimum(np.arange(my * m), H - 1)
    xs = np.minimum(np.arange(mx * m), W - 1)
    p = img[ys][:, xs].astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    if sampling == "420":
        sub = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2   # noqa: E731
        Cb, Cr = sub(Cb), sub(Cr)

    def blocks(c: np.ndarray) -> np.ndarray:       # [h, w] -> [h/8, w/8, 8, 8], level-shifted
        h, w = c.shape
        return (c - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)

    yb, cbb, crb = blocks(Y), blocks(Cb), blocks(Cr)
    if sampling == "420":
        # MCU (i, j): Y blocks (2i,2j) (2i,2j+1) (2i+1,2j) (2i+1,2j+1), then Cb, Cr
        yq = yb.reshape(my, 2, mx, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my, mx, 4, 8, 8)
        blk = np.concatenate([yq, cbb[:, :, None], crb[:, :, None]], axis=2)
    else:
        blk = np.stack([yb, cbb, crb], axis=2)
    blk = blk.reshape(my * mx, nb, 8, 8)
    C = dct_matrix()
    t = _div_floor_shift(np.einsum("kn,mbrn->mbrk", C, blk), DCT_BITS - PASS1_KEEP)      # rows
    f = _div_floor_shift(np.einsum("kn,mbnc->mbkc", C, t), DCT_BITS + PASS1_KEEP - OUT_KEEP)     # columns, x8
    lq, cq = quant_tables(quality)
    q = np.empty((nb, 8, 8), dtype=np.int64)
    nluma = nb - 2
    q[:nluma] = np.asarray(lq).reshape(8, 8)
    q[nluma:] = np.asarray(cq).reshape(8, 8)
    q <<= OUT_KEEP
    v = np.sign(f) * ((np.abs(f) + (q >> 1)) // q)          # round half away from zero
    v = v.reshape(my * mx, nb, 64)
    v[..., 1:] = np.clip(v[..., 1:], -1023, 1023)           # baseline AC magnitude categories 1..10
    return v[..., ZIGZAG].astype(np.int16)


# ----------------------------------------------------------------------------- libjpeg forward contract
# The coefficients libjpeg (PIL's encoder) computes: the LIBJPEG FORWARD CONTRACT section of
# jpeg.hip's header comment; ops/csrc/jpeg_fdct_lj.h is the arithmetic the kernel and the host
# program compile.
FDCT_BITS = 13                         # libjpeg jfdctint CONST_BITS
FDCT_PASS1 = 2                         # PASS1_BITS


def _fdct_pass(d, first: bool, see):
    """One 8-point pass of the jfdctint forward DCT on the arrays d[0..7] (``first``: the row
    pass); ``see`` is handed every intermediate (the word-width check) and returns it."""
    def D(x, n):
        return see(x + (1 << (n - 1))) >> n
    t0, t1, t2, t3 = d[0] + d[7], d[1] + d[6], d[2] + d[5], d[3] + d[4]
    t7, t6, t5, t4 = d[0] - d[7], d[1] - d[6], d[2] - d[5], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    if first:
        o0, o4 = see((t10 + t11) << FDCT_PASS1), see((t10 - t11) << FDCT_PASS1)
        sh = FDCT_BITS - FDCT_PASS1
    else:
        o0, o4 = D(t10 + t11, FDCT_PASS1), D(t10 - t11, FDCT_PASS1)
        sh = FDCT_BITS + FDCT_PASS1
    z1 = see((t12 + t13) * 4433)
    o2, o6 = D(z1 + see(t13 * 6270), sh), D(z1 - see(t12 * 15137), sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = see((z3 + z4) * 9633)
    t4, t5, t6, t7 = see(t4 * 2446), see(t5 * 16819), see(t6 * 25172), see(t7 * 12299)
    z1, z2 = see(z1 * -7373), see(z2 * -20995)
    z3, z4 = see(see(z3 * -16069) + z5), see(see(z4 * -3196) + z5)
    o7, o5 = D(see(see(t4 + z1) + z3), sh), D(see(see(t5 + z2) + z4), sh)
    o3, o1 = D(see(see(t6 + z2) + z3), sh), D(see(see(t7 + z1) + z4), sh)
    return [o0, o1, o2, o3, o4, o5, o6, o7]


def fdct_libjpeg(blk: np.ndarray, see=lambda v: v) -> np.ndarray:
    """Level-shifted samples [..., 8, 8] -> 8 x the DCT coefficients [..., 8, 8] (jfdctint: rows,
    then columns)."""
    blk = np.asarray(blk, dtype=np.int64)
    t = np.stack(_fdct_pass([blk[..., n] for n in range(8)], True, see), axis=-1)
    return np.stack(_fdct_pass([t[..., n, :] for n in range(8)], False, see), axis=-2)


def quantise_libjpeg(f: np.ndarray, q: np.ndarray) -> np.ndarray:
    """8 x coefficients [..., 8, 8] and quantisation values ``q`` (natural order, broadcast) ->
    quantised values: round half away from zero, AC guarded at +-1023."""
    q8 = np.asarray(q, dtype=np.int64) << 3
    v = np.sign(f) * ((np.abs(f) + (q8 >> 1)) // q8)
    flat = v.reshape(v.shape[:-2] + (64,))
    flat[..., 1:] = np.clip(flat[..., 1:], -1023, 1023)
    return flat


def coefficients_libjpeg(img: np.ndarray, quality: int, sampling: str, stats: dict = None) -> np.ndarray:
    """uint8 [H, W, 3] -> int16 [mcus, blocks per MCU, 64]: the quantised zig-zag coefficients of
    the file ``Image.save(format="JPEG", quality=quality)`` writes for these pixels (libjpeg's
    edge expansion, h2v2 downsampling, ISLOW forward DCT and dummy blocks).  ``stats`` receives
    ``max_abs`` (the largest intermediate of the DCT: the kernel works in 32-bit words),
    ``dummy_blocks``, ``dummy_chain`` (dummy blocks whose DC comes from another dummy block),
    ``chroma_bottom_rows`` (downsampled chroma rows that are replicas while their two source rows
    lie inside the 16-row MCU: the even-H rule), ``odd_row_pairs`` (chroma rows averaging a
    replicated image row), ``bias1`` / ``bias2`` (chroma means whose result depends on the bias
    being 1 / 2 and not the other), ``ac_clamped``."""
    H, W, _ = img.shape
    m, nb, mx, my = geometry(H, W, sampling)
    p = img.astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    st = {"max_abs": 0, "dummy_blocks": 0, "dummy_chain": 0, "chroma_bottom_rows": 0, "odd_row_pairs": 0,
          "bias1": 0, "bias2": 0, "ac_clamped": 0}

    def see(v):
        st["max_abs"] = max(st["max_abs"], int(np.abs(v).max()))
        return v

    def pad(c: np.ndarray, h: int, w: int) -> np.ndarray:      # replicate the last row / column
        return c[np.minimum(np.arange(h), c.shape[0] - 1)][:, np.minimum(np.arange(w), c.shape[1] - 1)]

    def blocks(c: np.ndarray) -> np.ndarray:       # [h, w] -> [h/8, w/8, 8, 8], level-shifted
        h, w = c.shape
        return (c - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)

    bh, bw = (H + 7) // 8, (W + 7) // 8            # real luma blocks
    if sampling == "420":
        ch, cw = (H + 1) // 2, (W + 1) // 2
        cbh, cbw = (ch + 7) // 8, (cw + 7) // 8

        def sub(c: np.ndarray) -> np.ndarray:
            c = pad(c, 2 * ch, 16 * cbw)
            s4 = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
            bias = np.where(np.arange(8 * cbw) & 1, 2, 1)
            real = s4[:, :cw]
            st["bias1"] += int(((real[:, 0::2] & 3) == 2).sum())       # +1 stays below, +2 carries
            st["bias2"] += int(((real[:, 1::2] & 3) == 2).sum())
            return pad((s4 + bias) >> 2, 8 * cbh, 8 * cbw)
        Cb, Cr = sub(Cb), sub(Cr)
        st["odd_row_pairs"] += H & 1
        st["chroma_bottom_rows"] += 8 * cbh - ch if (H % 16) else 0
        assert (cbh, cbw) == (my, mx)
        Yp = pad(pad(Y, 8 * bh, 8 * bw), 16 * my, 16 * mx)          # dummy blocks are replaced below
        yb = blocks(Yp).reshape(my, 2, mx, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my, mx, 4, 8, 8)
        blk = np.concatenate([yb, blocks(Cb)[:, :, None], blocks(Cr)[:, :, None]], axis=2)
    else:
        blk = np.stack([blocks(pad(c, 8 * bh, 8 * bw)) for c in (Y, Cb, Cr)], axis=2)
    blk = blk.reshape(my * mx, nb, 8, 8)
    f = fdct_libjpeg(blk, see)
    if st["max_abs"] >= 1 << 31:
        raise AssertionError("jpeg: a forward DCT intermediate does not fit 32 bits")
    lq, cq = quant_tables(quality)
    q = np.empty((nb, 8, 8), dtype=np.int64)
    q[:nb - 2] = np.asarray(lq).reshape(8, 8)
    q[nb - 2:] = np.asarray(cq).reshape(8, 8)
    raw = np.sign(f) * ((np.abs(f) + (q << 2)) // (q << 3))
    st["ac_clamped"] = int((np.abs(raw.reshape(-1, nb, 64)[..., 1:]) > 1023).sum())
    v = quantise_libjpeg(f, q)
    if sampling == "420":
        # dummy luma blocks: no AC, the DC of the MCU's previous block (which may be a dummy itself)
        v = v.reshape(my, mx, nb, 64)
        for k in range(1, 4):
            dy, dx = k >> 1, k & 1
            dummy = ((2 * np.arange(my) + dy >= bh)[:, None] | (2 * np.arange(mx) + dx >= bw)[None, :])
            prev_dummy = ((2 * np.arange(my) + ((k - 1) >> 1) >= bh)[:, None]
                          | (2 * np.arange(mx) + ((k - 1) & 1) >= bw)[None, :])
            st["dummy_blocks"] += int(dummy.sum())
            st["dummy_chain"] += int((dummy & prev_dummy).sum())
            fill = np.zeros_like(v[:, :, k])
            fill[..., 0] = v[:, :, k - 1, 0]
            v[:, :, k] = np.where(dummy[..., None], fill, v[:, :, k])
        v = v.reshape(my * mx, nb, 64)
    if stats is not None:
        stats.update(st)
    return v[..., ZIGZAG].astype(np.int16)


# ----------------------------------------------------------------------------- entropy coder
class _Bits:
    __slots__ = ("out", "acc", "n", "stuffed")

    def __init__(self) -> None:
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.stuffed = 0

    def put(self, code: int, length: int) -> None:
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self) -> None:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)      # pad with 1-bits


def _category(v: int) -> int:
    return abs(v).bit_length()


def entropy(coef: np.ndarray, restart_mcus: int, tables=None):
    """int16 [mcus, nb, 64] -> (scan bytes with RSTn markers, stats).  ``tables``: four
    ``(bits, vals)`` in place of the standard Huffman tables."""
    huff = huff_table(tables)
    mcus, nb, _ = coef.shape
    per = restart_mcus if restart_mcus else mcus
    nint = (mcus + per - 1) // per
    out = bytearray()
    stats = {"stuffed": 0, "zrl": 0, "max_dc_cat": 0, "intervals": nint}
    rows = coef.tolist()
    for it in range(nint):
        w = _Bits()
        pred = [0, 0, 0]
        for mcu in rows[it * per: (it + 1) * per]:
            for b, blk in enumerate(mcu):
                comp = 0 if b < nb - 2 else b - (nb - 2) + 1
                dc_base, ac_base = (0, 32) if comp == 0 else (16, 32 + 256)
                d = blk[0] - pred[comp]
                pred[comp] = blk[0]
                cat = _category(d)
                stats["max_dc_cat"] = max(stats["max_dc_cat"], cat)
                h = int(huff[dc_base + cat])
                w.put(h & 0xFFFF, h >> 16)
                if cat:
                    w.put((d if d >= 0 else d - 1) & ((1 << cat) - 1), cat)
                run = 0
                for k in range(1, 64):
                    v = blk[k]
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        h = int(huff[ac_base + 0xF0])
                        w.put(h & 0xFFFF, h >> 16)
                        stats["zrl"] += 1
                        run -= 16
                    cat = _category(v)
                    h = int(huff[ac_base + (run << 4 | cat)])
                    w.put(h & 0xFFFF, h >> 16)
                    w.put((v if v >= 0 else v - 1) & ((1 << cat) - 1), cat)
                    run = 0
                if run:
                    h = int(huff[ac_base])
                    w.put(h & 0xFFFF, h >> 16)
        w.flush()
        stats["stuffed"] += w.stuffed
        out += w.out
        if it + 1 < nint:
            out += bytes([0xFF, 0xD0 + (it & 7)])
    return bytes(out), stats


# ----------------------------------------------------------------------------- block-parallel entropy coder
# The same bytes with the work divided per 8x8 block: the BLOCK-PARALLEL ENTROPY CODER section of
# jpeg.hip's header comment; ops/csrc/jpeg_entropy_blk.h is the per-block coder and the stuffing
# piece the kernels and the host program compile.
BLK_STUFF_CHUNK = 32                   # unstuffed bytes per stuffing piece (jpeg_entropy_blk.h: JPEG_BLK_PIECE)


@lru_cache(maxsize=None)
def block_bits_bound() -> int:
    """The most bits one block can code to, from the Huffman tables: the longest DC code + 11 value
    bits, and 63 times the longest AC code + 10 value bits (no ZRL or EOB: every position is taken)."""
    h = huff_table()
    dc = max(int(v) >> 16 for v in np.concatenate([h[0:16], h[16:32]]))
    ac = max(int(v) >> 16 for v in h[32:])
    return dc + 11 + 63 * (ac + 10)


def dc_predictors(coef: np.ndarray, restart_mcus: int) -> np.ndarray:
    """int [mcus, nb]: the DC value every block's difference is taken against, from the geometry
    alone: the previous block of the component in coding order (4:2:0: the Y blocks of an MCU
    follow each other, the first follows the previous MCU's last; Cb / Cr follow the previous
    MCU's), 0 for a component's first block of a restart interval."""
    mcus, nb, _ = coef.shape
    per = restart_mcus if restart_mcus else mcus
    dc = coef[..., 0].astype(np.int64)
    pred = np.zeros((mcus, nb), dtype=np.int64)
    head = (np.arange(mcus) % per) == 0
    prev = np.roll(dc, 1, axis=0)                       # the MCU before (row 0 is masked by head)
    nl = nb - 2
    pred[:, 0] = np.where(head, 0, prev[:, nl - 1])
    pred[:, 1:nl] = dc[:, 0:nl - 1]
    pred[:, nl:] = np.where(head[:, None], 0, prev[:, nl:])
    return pred


def _block_code(blk, pred: int, luma: bool, huff, stats: dict):
    """One block's code bits as (value, bit count): the coder of :func:`entropy` on one block."""
    dc_base, ac_base = (0, 32) if luma else (16, 32 + 256)
    acc = n = 0
    d = blk[0] - pred
    cat = _category(d)
    stats["max_dc_cat"] = max(stats["max_dc_cat"], cat)
    h = int(huff[dc_base + cat])
    acc, n = (acc << (h >> 16)) | (h & 0xFFFF), n + (h >> 16)
    if cat:
        acc, n = (acc << cat) | ((d if d >= 0 else d - 1) & ((1 << cat) - 1)), n + cat
    run = 0
    for k in range(1, 64):
        v = blk[k]
        if v == 0:
            run += 1
            continue
        while run >= 16:
            h = int(huff[ac_base + 0xF0])
            acc, n = (acc << (h >> 16)) | (h & 0xFFFF), n + (h >> 16)
            stats["zrl"] += 1
            run -= 16
        cat = _category(v)
        h = int(huff[ac_base + (run << 4 | cat)])
        acc, n = (acc << (h >> 16)) | (h & 0xFFFF), n + (h >> 16)
        acc, n = (acc << cat) | ((v if v >= 0 else v - 1) & ((1 << cat) - 1)), n + cat
        run = 0
    if run:
        h = int(huff[ac_base])
        acc, n = (acc << (h >> 16)) | (h & 0xFFFF), n + (h >> 16)
    return acc, n


def entropy_blocks(coef: np.ndarray, restart_mcus: int, stuff_chunk: int = BLK_STUFF_CHUNK, stats: dict = None,
                   tables=None):
    """What :func:`entropy` returns, computed the way the BLOCK-PARALLEL ENTROPY CODER says: per
    restart interval the bit length of every block (DC difference against :func:`dc_predictors`),
    the exclusive scan of the lengths, every block's bits packed at its offset into the unstuffed
    string (the last byte padded with 1-bits), and the stuffing in pieces of ``stuff_chunk``
    unstuffed bytes: 0xFF count per piece, scan, copy with the zeros inserted.

    ``stats`` receives what tells where an input reaches: ``min_bits`` / ``max_bits`` (block bit
    lengths), ``max_starts_per_word`` (blocks starting in one 32-bit word of an interval's string),
    ``ff_two_blocks`` (unstuffed 0xFF bytes with a block boundary inside), ``ff_interval_end``
    (intervals whose last unstuffed byte is 0xFF), ``ff_piece_end`` (0xFF bytes that are the last
    byte of a full piece), ``ff_pairs`` (two consecutive unstuffed 0xFF bytes), ``unstuffed`` (bytes).
    ``tables``: four ``(bits, vals)`` in place of the standard Huffman tables."""
    if int(stuff_chunk) != stuff_chunk or stuff_chunk < 1:
        raise ValueError("jpeg: stuff_chunk must be a positive integer")
    huff = huff_table(tables)
    mcus, nb, _ = coef.shape
    per = restart_mcus if restart_mcus else mcus
    nint = (mcus + per - 1) // per
    out = bytearray()
    st = {"stuffed": 0, "zrl": 0, "max_dc_cat": 0, "intervals": nint}
    cov = {"min_bits": 1 << 30, "max_bits": 0, "max_starts_per_word": 0, "ff_two_blocks": 0, "ff_interval_end": 0,
           "ff_piece_end": 0, "ff_pairs": 0, "unstuffed": 0}
    pred = dc_predictors(coef, restart_mcus).tolist()
    rows = coef.tolist()
    for it in range(nint):
        m0, m1 = it * per, min((it + 1) * per, mcus)
        # 1. bits per block
        codes = [_block_code(rows[m][b], pred[m][b], b < nb - 2, huff, st) for m in range(m0, m1) for b in range(nb)]
        lens = np.asarray([n for _, n in codes], dtype=np.int64)
        # 2. scan
        offs = np.concatenate([[0], np.cumsum(lens)])
        bits = int(offs[-1])
        nbytes = (bits + 7) // 8
        # 3. pack: every block ORs its bits into the zeroed string at its offset, then the padding
        total = 0
        for (val, n), o in zip(codes, offs[:-1].tolist()):
            total |= val << (8 * nbytes - o - n)
        total |= (1 << (8 * nbytes - bits)) - 1
        u = np.frombuffer(total.to_bytes(nbytes, "big"), dtype=np.uint8)
        # 4. stuff: count per piece, scan, copy
        ff = u == 0xFF
        npiece = (nbytes + stuff_chunk - 1) // stuff_chunk
        cnt = np.add.reduceat(ff.astype(np.int64), np.arange(npiece) * stuff_chunk)
        poff = np.arange(npiece) * stuff_chunk + np.concatenate([[0], np.cumsum(cnt)[:-1]])
        body = bytearray(nbytes + int(cnt.sum()))
        for p in range(npiece):
            piece = u[p * stuff_chunk: (p + 1) * stuff_chunk].tobytes().replace(b"\xff", b"\xff\x00")
            body[int(poff[p]): int(poff[p]) + len(piece)] = piece
        st["stuffed"] += int(cnt.sum())
        out += body
        if it + 1 < nint:
            out += bytes([0xFF, 0xD0 + (it & 7)])
        cov["min_bits"] = min(cov["min_bits"], int(lens.min()))
        cov["max_bits"] = max(cov["max_bits"], int(lens.max()))
        cov["max_starts_per_word"] = max(cov["max_starts_per_word"], int(np.bincount(offs[:-1] >> 5).max()))
        inner = offs[1:-1][(offs[1:-1] & 7) != 0] >> 3          # bytes with a block boundary inside
        cov["ff_two_blocks"] += int(ff[np.unique(inner)].sum())
        cov["ff_interval_end"] += int(ff[-1])
        cov["ff_piece_end"] += int(ff[stuff_chunk - 1:: stuff_chunk].sum())
        cov["ff_pairs"] += int((ff[:-1] & ff[1:]).sum())
        cov["unstuffed"] += nbytes
    if stats is not None:
        stats.update(cov)
    return bytes(out), st


def jpeg_encode(images, quality: int = 75, sampling: str = "420", restart_mcus: int = 4,
                return_stats: bool = False, huffman: str = "standard", transform: str = "matrix"):
    """Baseline JPEG of uint8 ``[B, H, W, 3]`` (or ``[H, W, 3]``) images: one byte string per
    image.  ``restart_mcus`` MCUs per restart interval (0: no DRI, one interval).  With
    ``return_stats`` also a dict per image: ``stuffed`` (0xFF bytes that needed a stuffed zero),
    ``zrl`` (ZRL symbols), ``max_dc_cat`` (largest DC difference category), ``intervals``.
    ``huffman="optimized"``: every image is coded with, and carries in its DHT, the tables
    :func:`optimal_table` builds from its own :func:`symbol_counts` (what libjpeg's ``optimize``
    writes for those coefficients).  ``transform="libjpeg"``: libjpeg's forward transform and
    header layout (the libjpeg forward contract): with ``restart_mcus=0`` the file PIL's
    ``Image.save(format="JPEG", quality=quality)`` writes, byte for byte (``huffman="optimized"``:
    with ``optimize=True``)."""
    if huffman not in HUFFMAN_MODES:
        raise ValueError(f"jpeg_encode: huffman must be one of {HUFFMAN_MODES}, not {huffman!r}")
    layout = transform_layout(transform)
    arr = images.detach().cpu().numpy() if hasattr(images, "detach") else np.asarray(images)
    if arr.ndim == 3:
        arr = arr[None]
    if arr.ndim != 4 or arr.shape[-1] != 3 or arr.dtype != np.uint8:
        raise ValueError("jpeg_encode: uint8 [B, H, W, 3] or [H, W, 3] expected")
    _, H, W, _ = arr.shape
    hdr = header(H, W, int(quality), sampling, int(restart_mcus), None, layout)
    if huffman == "optimized":
        _, nb, mx, my = geometry(H, W, sampling)
        check_count_range(mx * my * nb)
    outs, stats = [], []
    for img in arr:
        coef = coefficients(img, int(quality), sampling, transform)
        tables = None
        if huffman == "optimized":
            tables = optimal_tables(symbol_counts(coef, int(restart_mcus)))
            hdr = header(H, W, int(quality), sampling, int(restart_mcus), tables, layout)
        scan, st = entropy(coef, int(restart_mcus), tables)
        outs.append(hdr + scan + b"\xff\xd9")
        stats.append(st)
    return (outs, stats) if return_stats else outs


# ----------------------------------------------------------------------------- optimised Huffman tables
# The tables libjpeg builds for an image's own symbols (jpeg_gen_optimal_table, T.81 K.2): the
# OPTIMISED HUFFMAN TABLES section of jpeg.hip's header comment; ops/csrc/jpeg_huff_opt.h is the
# routine the build kernel and the host program compile.
def block_bits_bound_optimized() -> int:
    """The most bits one block can code to with tables of its image's own: any code, a DC one
    included, can be 16 bits long: 16 + 11 value bits, and 63 times 16 + 10."""
    return 16 + 11 + 63 * (16 + 10)


def check_count_range(blocks: int) -> None:
    """Symbol counts are 32-bit words: an image has fewer than 2^31 coefficients."""
    if int(blocks) * 64 >= 1 << 31:
        raise ValueError("jpeg: optimised Huffman tables count symbols in 32-bit words: blocks * 64 must be below 2^31")


def symbol_counts(coef: np.ndarray, restart_mcus: int) -> np.ndarray:
    """int64 [4, 257]: how often :func:`entropy` emits every symbol for int16 [mcus, nb, 64]
    coefficients; rows DC luma, DC chroma, AC luma, AC chroma (column 256 stays 0: the reserved
    symbol of :func:`optimal_table`).  DC: the category of the difference against
    :func:`dc_predictors`; AC: ``(run << 4) | size``, ZRL (0xF0) per 16 zeros before a value, EOB
    (0x00) when the block ends in zeros."""
    mcus, nb, _ = coef.shape
    check_count_range(mcus * nb)
    freq = np.zeros((4, 257), dtype=np.int64)
    c = coef.astype(np.int64)

    def cat(v):
        a = np.abs(v)
        return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)
    d = c[..., 0] - dc_predictors(coef, restart_mcus)
    chroma = np.arange(nb) >= nb - 2
    dcat = cat(d)
    freq[0, :32] += np.bincount(dcat[:, ~chroma].ravel(), minlength=32)
    freq[1, :32] += np.bincount(dcat[:, chroma].ravel(), minlength=32)
    ac = c[..., 1:]
    nz = ac != 0
    pos = np.arange(1, 64)
    # zig-zag position of the previous non-zero AC value (0: none) before every position
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=-1)
    prev = np.concatenate([np.zeros(last.shape[:-1] + (1,), dtype=np.int64), last[..., :-1]], axis=-1)
    run = pos - prev - 1
    for t, sel in ((2, ~chroma), (3, chroma)):
        m = nz[:, sel]
        r = run[:, sel][m]
        freq[t, :256] += np.bincount(((r & 15) << 4) | cat(ac[:, sel][m]), minlength=256)
        freq[t, 0xF0] += int((r >> 4).sum())
        freq[t, 0x00] += int((last[:, sel][..., -1] != 63).sum())
    return freq


def code_sizes(freq) -> List[int]:
    """Steps 1 - 3 of :func:`optimal_table`: the code length of the 257 indices (the reserved
    symbol last) before the lengths are limited to 16; 0 for an index that does not occur."""
    f = [int(v) for v in np.asarray(freq).ravel()[:256]]
    f += [0] * (256 - len(f)) + [1]              # f[256]: the reserved symbol, no code is all ones
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, 1 << 62
        for i in range(257):
            if f[i] and f[i] <= v:
                v, c1 = f[i], i
        c2, v = -1, 1 << 62
        for i in range(257):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def optimal_table(freq) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """``(bits[16], vals)`` of the Huffman table libjpeg builds for the symbol frequencies
    ``freq[0..255]`` (``jpeg_gen_optimal_table``; the steps and tie rules: jpeg.hip's header
    comment).  No symbol: an empty table."""
    codesize = code_sizes(freq)
    if max(codesize) > 32:
        raise ValueError("jpeg: a Huffman code longer than 32 bits")
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i > 0:
        bits[i] -= 1                             # the reserved symbol leaves
    vals = [j for length in range(1, 33) for j in range(256) if codesize[j] == length]
    return tuple(bits[1:17]), tuple(vals)


def optimal_tables(freq) -> tuple:
    """Four ``(bits, vals)`` from :func:`symbol_counts`' [4, 257]."""
    return tuple(optimal_table(row) for row in np.asarray(freq))


# ----------------------------------------------------------------------------- decode contract
# The pixels a libjpeg decoder (ISLOW inverse DCT, fancy upsampling: PIL's defaults) produces from
# the bytes above, computed from the quantised coefficients alone.  Formulas: the DECODE CONTRACT
# section of jpeg.hip's header comment.
IDCT_BITS = 13                         # libjpeg jidctint CONST_BITS
IDCT_PASS1 = 2                         # PASS1_BITS


def _idct_pass(i, shift: int, see):
    """One 8-point pass of the jidctint inverse DCT on the arrays i[0..7]; ``see`` is handed every
    intermediate (the word-width check) and returns it."""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = see((i2 + i6) * 4433)
    t2 = see(z1 - see(i6 * 15137))
    t3 = see(z1 + see(i2 * 6270))
    t0 = see((i0 + i4) << IDCT_BITS)
    t1 = see((i0 - i4) << IDCT_BITS)
    t10, t13, t11, t12 = see(t0 + t3), see(t0 - t3), see(t1 + t2), see(t1 - t2)
    a, b, c, d = i7, i5, i3, i1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = see((z3 + z4) * 9633)
    a, b, c, d = see(a * 2446), see(b * 16819), see(c * 25172), see(d * 12299)
    z1, z2 = see(z1 * -7373), see(z2 * -20995)
    z3, z4 = see(see(z3 * -16069) + z5), see(see(z4 * -3196) + z5)
    a, b, c, d = see(see(a + z1) + z3), see(see(b + z2) + z4), see(see(c + z2) + z3), see(see(d + z1) + z4)
    outs = (t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d)
    return [see(see(v) + (1 << (shift - 1))) >> shift for v in outs]


def _planes(samples: np.ndarray, mx: int, my: int, sampling: str):
    """uint8-range samples [mcus, nb, 8, 8] -> padded Y, Cb, Cr planes."""
    def plane(b: np.ndarray) -> np.ndarray:     # [my, mx, 8, 8] -> [8 my, 8 mx]
        return b.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)
    if sampling == "420":
        yb = samples[:, :4].reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16)
        return yb, plane(samples[:, 4].reshape(my, mx, 8, 8)), plane(samples[:, 5].reshape(my, mx, 8, 8))
    return tuple(plane(samples[:, k].reshape(my, mx, 8, 8)) for k in range(3))


def _upsample_h2v2(c: np.ndarray, see) -> np.ndarray:
    """[ch, cw] real chroma samples -> [2 ch, 2 cw] (libjpeg h2v2 fancy upsampling; two or fewer
    columns are replicated, as libjpeg does there)."""
    ch, cw = c.shape
    y, x = np.arange(2 * ch), np.arange(2 * cw)
    if cw <= 2:
        return c[y >> 1][:, x >> 1]
    near = np.clip(np.where(y & 1, (y >> 1) + 1, (y >> 1) - 1), 0, ch - 1)
    s = 3 * c[y >> 1] + c[near]
    side = np.clip(np.where(x & 1, (x >> 1) + 1, (x >> 1) - 1), 0, cw - 1)
    return see(3 * s[:, x >> 1] + s[:, side] + np.where(x & 1, 7, 8)) >> 4


def reconstruct(coef: np.ndarray, H: int, W: int, quality: int, sampling: str, stats: dict = None,
                tables=None) -> np.ndarray:
    """int16 [mcus, blocks per MCU, 64] quantised zig-zag coefficients (:func:`coefficients`) ->
    uint8 [H, W, 3], the pixels a libjpeg decoder gives for the JPEG of those coefficients.
    Computed in int64; ``stats["max_abs"]`` receives the largest magnitude of any intermediate
    (the kernel works in 32-bit words).  ``tables``: ``(luma, chroma)`` quantisation tables in
    natural order, used in place of ``quant_tables(quality)`` (a foreign stream's DQT)."""
    _, nb, mx, my = geometry(H, W, sampling)
    peak = [0]

    def see(v):
        peak[0] = max(peak[0], int(np.abs(v).max()))
        return v

    lq, cq = quant_tables(quality) if tables is None else tables
    q = np.empty((nb, 64), dtype=np.int64)
    q[:nb - 2], q[nb - 2:] = np.asarray(lq), np.asarray(cq)
    nat = np.empty(coef.shape, dtype=np.int64)
    nat[..., ZIGZAG] = coef
    d = see(nat * q).reshape(-1, nb, 8, 8)
    ws = np.stack(_idct_pass([d[..., k, :] for k in range(8)], IDCT_BITS - IDCT_PASS1, see), axis=-2)     # columns
    px = np.stack(_idct_pass([ws[..., k] for k in range(8)], IDCT_BITS + IDCT_PASS1 + 3, see), axis=-1)   # rows
    Y, Cb, Cr = _planes(np.clip(px + 128, 0, 255), mx, my, sampling)
    if sampling == "420":
        ch, cw = (H + 1) // 2, (W + 1) // 2
        Cb, Cr = _upsample_h2v2(Cb[:ch, :cw], see), _upsample_h2v2(Cr[:ch, :cw], see)
    Y, cb, cr = Y[:H, :W], Cb[:H, :W] - 128, Cr[:H, :W] - 128
    R = Y + (see(91881 * cr + 32768) >> 16)
    G = Y + (see(-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + (see(116130 * cb + 32768) >> 16)
    if stats is not None:
        stats["max_abs"] = max(stats.get("max_abs", 0), peak[0])
    return np.clip(np.stack([R, G, B], -1), 0, 255).astype(np.uint8)


def jpeg_decoded(images, quality: int = 75, sampling: str = "420", transform: str = "matrix") -> np.ndarray:
    """uint8 ``[B, H, W, 3]`` (or ``[H, W, 3]``) images -> uint8 ``[B, H, W, 3]``: what a libjpeg
    decoder returns for each image's :func:`jpeg_encode` bytes (any restart interval) with the
    same ``transform``."""
    transform_layout(transform)
    arr = images.detach().cpu().numpy() if hasattr(images, "detach") else np.asarray(images)
    if arr.ndim == 3:
        arr = arr[None]
    if arr.ndim != 4 or arr.shape[-1] != 3 or arr.dtype != np.uint8:
        raise ValueError("jpeg_decoded: uint8 [B, H, W, 3] or [H, W, 3] expected")
    _, H, W, _ = arr.shape
    return np.stack([reconstruct(coefficients(img, int(quality), sampling, transform), H, W, int(quality), sampling)
                     for img in arr])


# ----------------------------------------------------------------------------- entropy decode contract
# Bytes -> quantised coefficients: the mirror of :func:`entropy` for any baseline stream in scope
# (its own DQT / DHT).  Formulas: the ENTROPY DECODE CONTRACT section of jpeg.hip's header comment;
# ops/csrc/jpeg_entropy_dec.h is the per-interval routine the kernel and the host program compile.
class JpegError(ValueError):
    """Malformed JPEG bytes.  ``code`` is a status of the entropy decode contract (0 for a fault the
    header parse found), ``interval`` the restart interval (image * intervals + index) it is in."""

    def __init__(self, msg: str, code: int = 0, interval: int = -1) -> None:
        super().__init__(msg)
        self.code, self.interval = code, interval


class JpegUnsupported(ValueError):
    """A JPEG outside the decoder's scope (or a block the 32-bit arithmetic refuses: WIDE)."""

    def __init__(self, msg: str, code: int = 0, interval: int = -1) -> None:
        super().__init__(msg)
        self.code, self.interval = code, interval


OK, TRUNCATED, BAD_CODE, OVERRUN, WIDE = 0, 1, 2, 3, 4
STATUS_NAMES = ("OK", "TRUNCATED", "BAD_CODE", "OVERRUN", "WIDE")
# The refusal rule: a block whose dequantised coefficients d have sum d^2 > WIDE_T^2 is refused.
# Two bounds meet in WIDE_T.  (1) The 32-bit inverse DCT: every intermediate is at most
# idct_gain()[0] * ||d||_2 (+ the rounding carried between the passes), below 2^31 up to
# ||d||_2 = 6392.  (2) The decoder the pixels are defined by: libjpeg-turbo's SIMD inverse DCT
# keeps the first pass's outputs, and sums of two of them, in 16-bit words.  A first-pass output
# is at most 4 sqrt(8) times the norm of its coefficient column, a sum of two at most
# 16 ||d||_2, so ||d||_2 <= 2047 keeps them below 2^15; measured, crafted blocks agree with PIL
# up to 2047 and stop agreeing at 2100 (tests/test_jpeg_entropy_decode.py).  A block of 8-bit
# samples has at most 1024 (Parseval) + 1020 (half the norm of an all-255 table) = 2044.
WIDE_T = 2047
DEC_LOOK_BITS = 8
DEC_TABLE_WORDS = 128 + 16 + 16 + 64      # per Huffman table: look-ahead | limits | value offsets | values


def raise_status(code: int, interval: int):
    """The exception of a status word other than OK."""
    name = STATUS_NAMES[code] if 0 < code < len(STATUS_NAMES) else f"status {code}"
    if code == WIDE:
        raise JpegUnsupported(f"jpeg: interval {interval}: a block's dequantised energy is over {WIDE_T}^2 (WIDE)",
                              code, interval)
    raise JpegError(f"jpeg: interval {interval}: {name}", code, interval)


@lru_cache(maxsize=None)
def idct_gain() -> Tuple[float, float]:
    """(largest L2 gain from the 64 dequantised inputs of a block to any intermediate of the two
    inverse DCT passes, largest L1 gain from the 8 inputs of one pass to any of its intermediates):
    unit impulses through :func:`_idct_pass` in exact arithmetic.  |intermediate| <= L2 gain *
    ||d||_2, plus the L1 gain times the rounding error (below 1) of the values between the passes."""
    class Lin:                           # a linear form over the basis, integer coefficients
        def __init__(self, v):
            self.v = v
        __add__ = lambda a, b: Lin(a.v + (b.v if isinstance(b, Lin) else 0))      # noqa: E731
        __sub__ = lambda a, b: Lin(a.v - b.v)                                     # noqa: E731
        __mul__ = lambda a, k: Lin(a.v * k)                                       # noqa: E731
        __lshift__ = lambda a, k: Lin(a.v * (1 << k))                             # noqa: E731
        __rshift__ = lambda a, k: Lin(a.v / float(1 << k))                        # noqa: E731
    l2, l1 = [0.0], [0.0]

    def see2(x):
        l2[0] = max(l2[0], float(np.sqrt((x.v.astype(np.float64) ** 2).sum(0)).max()))
        return x

    def see1(x):
        l1[0] = max(l1[0], float(np.abs(x.v).sum(0).max()))
        return x
    d = np.eye(64, dtype=np.float64).reshape(64, 8, 8)
    ws = _idct_pass([Lin(d[:, k, :]) for k in range(8)], IDCT_BITS - IDCT_PASS1, see2)
    w = np.stack([x.v for x in ws], axis=-2)
    _idct_pass([Lin(w[..., k]) for k in range(8)], IDCT_BITS + IDCT_PASS1 + 3, see2)
    _idct_pass([Lin(np.eye(8)[:, k]) for k in range(8)], 1, see1)
    return l2[0], l1[0]


@dataclass(frozen=True)
class JpegStream:
    """What :func:`parse` reads from a baseline JPEG: geometry, the stream's own tables and where
    its restart intervals lie."""
    data: bytes
    H: int
    W: int
    sampling: str
    qtables: Tuple[Tuple[int, ...], Tuple[int, ...]]       # luma, chroma, natural order
    huff: Tuple[Tuple[Tuple[int, ...], Tuple[int, ...]], ...]      # (bits, values): DC luma, DC chroma, AC luma, AC chroma
    restart: int                                           # MCUs per interval, 0: no DRI
    scan_offset: int                                       # first byte of the entropy-coded segment
    intervals: Tuple[Tuple[int, int], ...]                 # (offset, length) in data, markers excluded

    @property
    def header_key(self):
        """Equal for streams one batched decode accepts: same geometry, tables, interval count."""
        return (self.H, self.W, self.sampling, self.qtables, self.huff, self.restart, len(self.intervals))


def _check_dht(bits: Sequence[int], vals: Sequence[int], ac: bool) -> None:
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length):
            raise JpegError("jpeg: DHT assigns more codes than a length has")
        code <<= 1
    if len(set(vals)) != len(vals):
        raise JpegError("jpeg: DHT lists a symbol twice")
    for v in vals:
        if (v > 11) if not ac else ((v & 15) > 10 or ((v & 15) == 0 and v not in (0x00, 0xF0))):
            raise JpegUnsupported(f"jpeg: Huffman symbol 0x{v:02x} is not a baseline 8-bit symbol")


def parse(data) -> JpegStream:
    """The header of a baseline JPEG in scope and the position of every restart interval.  Scope:
    SOF0, 8-bit samples, 8-bit DQT, three components with sampling factors (2x2, 1x1, 1x1) or all
    1x1, the two chroma components sharing their tables, one interleaved scan, no Adobe APP14
    segment.  :class:`JpegUnsupported` outside it, :class:`JpegError` for malformed bytes."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise JpegError("jpeg: no SOI marker")
    qt: Dict[int, Tuple[int, ...]] = {}
    ht: Dict[Tuple[int, int], Tuple[Tuple[int, ...], Tuple[int, ...]]] = {}
    frame = None
    restart = 0
    pos = 2
    while True:
        if pos + 4 > n:
            raise JpegError("jpeg: the header ends before SOS")
        if data[pos] != 0xFF:
            raise JpegError(f"jpeg: marker expected at byte {pos}")
        m = data[pos + 1]
        if m == 0xFF:                    # fill byte
            pos += 1
            continue
        if m in (0xD8, 0xD9, 0x01) or 0xD0 <= m <= 0xD7:
            raise JpegError(f"jpeg: marker 0x{m:02x} in the header")
        ln = (data[pos + 2] << 8) | data[pos + 3]
        if ln < 2 or pos + 2 + ln > n:
            raise JpegError(f"jpeg: segment 0x{m:02x} runs past the end")
        seg = data[pos + 4: pos + 2 + ln]
        pos += 2 + ln
        if m == 0xDB:
            k = 0
            while k < len(seg):
                pq, tq = seg[k] >> 4, seg[k] & 15
                if pq != 0:
                    raise JpegUnsupported("jpeg: 16-bit quantisation table")
                if tq > 3 or k + 65 > len(seg):
                    raise JpegError("jpeg: malformed DQT")
                zz = seg[k + 1: k + 65]
                if 0 in zz:
                    raise JpegError("jpeg: zero in a quantisation table")
                nat = [0] * 64
                for z in range(64):
                    nat[ZIGZAG[z]] = zz[z]
                qt[tq] = tuple(nat)
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                if k + 17 > len(seg):
                    raise JpegError("jpeg: malformed DHT")
                tc, th = seg[k] >> 4, seg[k] & 15
                bits = tuple(seg[k + 1: k + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or k + 17 + cnt > len(seg):
                    raise JpegError("jpeg: malformed DHT")
                vals = tuple(seg[k + 17: k + 17 + cnt])
                _check_dht(bits, vals, tc == 1)
                ht[(tc, th)] = (bits, vals)
                k += 17 + cnt
        elif m == 0xC0:
            if frame is not None:
                raise JpegError("jpeg: two frame headers")
            if len(seg) < 6:
                raise JpegError("jpeg: malformed SOF0")
            prec, H, W, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8:
                raise JpegUnsupported(f"jpeg: {prec}-bit samples")
            if nc != 3:
                raise JpegUnsupported(f"jpeg: {nc} components (three expected)")
            if len(seg) != 6 + 3 * nc:
                raise JpegError("jpeg: malformed SOF0")
            if H == 0 or W == 0:
                raise JpegUnsupported("jpeg: zero image side (DNL)")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i], seg[8 + 3 * i]) for i in range(3)]
            hv = tuple(c[1] for c in comps)
            if hv == (0x22, 0x11, 0x11):
                sampling = "420"
            elif hv == (0x11, 0x11, 0x11):
                sampling = "444"
            else:
                raise JpegUnsupported("jpeg: sampling factors other than 4:2:0 and 4:4:4")
            frame = (H, W, sampling, comps)
        elif 0xC1 <= m <= 0xCF and m != 0xC8:
            raise JpegUnsupported(f"jpeg: frame type 0x{m:02x} (baseline SOF0 only)")
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegError("jpeg: malformed DRI")
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xEE and seg[:5] == b"Adobe":
            raise JpegUnsupported("jpeg: Adobe APP14 segment (colour transform)")
        elif m == 0xDC:
            raise JpegUnsupported("jpeg: DNL")
        elif m == 0xDA:
            break
    if frame is None:
        raise JpegError("jpeg: SOS before SOF0")
    H, W, sampling, comps = frame
    if len(seg) < 1 or seg[0] != 3:
        raise JpegUnsupported("jpeg: a scan that is not the three components interleaved")
    if len(seg) != 10:
        raise JpegError("jpeg: malformed SOS")
    if tuple(seg[1 + 2 * i] for i in range(3)) != tuple(c[0] for c in comps):
        raise JpegUnsupported("jpeg: scan components out of frame order")
    if tuple(seg[7:10]) != (0, 63, 0):
        raise JpegUnsupported("jpeg: spectral selection / successive approximation")
    sel = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(3)]
    if sel[1] != sel[2] or comps[1][2] != comps[2][2]:
        raise JpegUnsupported("jpeg: the chroma components do not share their tables")
    try:
        qtables = (qt[comps[0][2]], qt[comps[1][2]])
        huff = (ht[(0, sel[0][0])], ht[(0, sel[1][0])], ht[(1, sel[0][1])], ht[(1, sel[1][1])])
    except KeyError:
        raise JpegError("jpeg: the scan names a table the stream does not define") from None
    # marker scan of the entropy-coded segment: every 0xFF there is followed by 0x00 or a marker
    a = np.frombuffer(data, dtype=np.uint8)[pos:]
    ff = np.flatnonzero(a[:-1] == 0xFF)
    mk = ff[a[ff + 1] != 0]
    codes = a[mk + 1]
    end = np.flatnonzero(codes == 0xD9)
    if end.size == 0:
        raise JpegError("jpeg: no EOI marker")
    k = int(end[0])
    rst = codes[:k].astype(np.int64) - 0xD0
    if k and (int(rst.min()) < 0 or int(rst.max()) > 7):
        other = int(codes[:k][(rst < 0) | (rst > 7)][0])
        if other == 0xFF:
            raise JpegUnsupported("jpeg: fill bytes in the entropy-coded segment")
        if other in (0xDA, 0xC4, 0xDB, 0xDD):
            raise JpegUnsupported("jpeg: more than one scan")
        raise JpegError(f"jpeg: marker 0x{other:02x} in the entropy-coded segment")
    if k and not np.array_equal(rst, np.arange(k) & 7):
        raise JpegError("jpeg: restart markers out of sequence")
    _, _, mx, my = geometry(H, W, sampling)
    want = (mx * my + restart - 1) // restart if restart else 1
    if k + 1 != want:
        raise JpegError(f"jpeg: {k + 1} restart intervals, {want} expected")
    starts = np.concatenate([[0], mk[:k] + 2]) + pos
    lens = mk[:k + 1] + pos - starts
    return JpegStream(data, H, W, sampling, qtables, huff, restart, pos,
                      tuple(zip(starts.tolist(), lens.tolist())))


def decode_tables(huff) -> np.ndarray:
    """int32 [4 * DEC_TABLE_WORDS], the decode tables of jpeg_entropy_dec.h for the four Huffman
    specifications (DC luma, DC chroma, AC luma, AC chroma).  Per table, with ``code`` the canonical
    code counter of T.81 Annex C: 256 uint16 look-ahead entries ``(length << 8) | symbol`` indexed
    by the next 8 bits (0: the code is longer); ``limit[l-1]`` = the counter after the codes of
    length l, left-justified to 16 bits; ``valoff[l-1]`` = index of the first value of length l
    minus its code; the 256 value bytes."""
    out = np.zeros((4, DEC_TABLE_WORDS), dtype=np.int32)
    for t, (bits, vals) in enumerate(huff):
        look = np.zeros(256, dtype=np.uint16)
        code, k = 0, 0
        for length in range(1, 17):
            out[t, 128 + 16 + length - 1] = k - code
            for _ in range(bits[length - 1]):
                if length <= DEC_LOOK_BITS:
                    lo = code << (DEC_LOOK_BITS - length)
                    look[lo: lo + (1 << (DEC_LOOK_BITS - length))] = (length << 8) | vals[k]
                code += 1
                k += 1
            out[t, 128 + length - 1] = code << (16 - length)
            code <<= 1
        out[t, :128] = look.view(np.int32)
        hv = np.zeros(256, dtype=np.uint8)
        hv[:len(vals)] = vals
        out[t, 160:] = hv.view(np.int32)
    return out.reshape(-1)


class _BitReader:
    """MSB-first bits of one unstuffed restart interval."""
    __slots__ = ("buf", "pos", "acc", "n")

    def __init__(self, raw: bytes) -> None:
        stray = -1                       # a 0xFF not followed by 0x00 ends the data
        i = raw.find(b"\xff")
        while i >= 0:
            if raw[i + 1: i + 2] != b"\x00":
                stray = i
                break
            i = raw.find(b"\xff", i + 2)
        if stray >= 0:
            raw = raw[:stray]
        self.buf = raw.replace(b"\xff\x00", b"\xff")
        self.pos, self.acc, self.n = 0, 0, 0

    def fill(self) -> None:
        take = self.buf[self.pos: self.pos + 8]
        self.pos += len(take)
        self.acc = ((self.acc & ((1 << self.n) - 1)) << (8 * len(take))) | int.from_bytes(take, "big")
        self.n += 8 * len(take)

    def peek16(self) -> int:
        if self.n < 16:
            self.fill()
        return (self.acc >> (self.n - 16)) & 0xFFFF if self.n >= 16 else (self.acc << (16 - self.n)) & 0xFFFF

    def receive(self, s: int) -> int:
        if self.n < s:
            self.fill()
            if self.n < s:
                return -1
        self.n -= s
        return (self.acc >> self.n) & ((1 << s) - 1)


def _decode_interval(raw: bytes, codebooks, qz, nb: int, nmcu: int, out: np.ndarray) -> int:
    """One restart interval into ``out`` [nmcu, nb, 64] (zeroed); the status."""
    rd = _BitReader(raw)
    t2 = WIDE_T * WIDE_T

    def symbol(book) -> int:
        w = rd.peek16()
        hit = book[0][w >> 8]
        if hit:
            length, sym = hit
        else:
            for length in range(9, 17):
                sym = book[length].get(w >> (16 - length))
                if sym is not None:
                    break
            else:
                return -TRUNCATED if rd.n < 16 else -BAD_CODE
        if length > rd.n:
            return -TRUNCATED
        rd.n -= length
        return sym
    pred = [0, 0, 0]
    for m in range(nmcu):
        for b in range(nb):
            comp = 0 if b < nb - 2 else b - (nb - 2) + 1
            tc = 1 if comp else 0
            q = qz[tc]
            s = symbol(codebooks[tc])
            if s < 0:
                return -s
            if s > 11:
                return BAD_CODE
            if s:
                v = rd.receive(s)
                if v < 0:
                    return TRUNCATED
                pred[comp] += v if v >= (1 << (s - 1)) else v - (1 << s) + 1
            d = pred[comp] * q[0]
            if abs(d) > WIDE_T:
                return WIDE
            energy = d * d
            out[m, b, 0] = pred[comp]
            k = 1
            while k < 64:
                rs = symbol(codebooks[2 + tc])
                if rs < 0:
                    return -rs
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if rs == 0:
                        break
                    if r != 15:
                        return BAD_CODE
                    k += 16
                    if k > 63:
                        return OVERRUN
                    continue
                if s > 10:
                    return BAD_CODE
                k += r
                if k > 63:
                    return OVERRUN
                v = rd.receive(s)
                if v < 0:
                    return TRUNCATED
                v = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                d = v * q[k]
                if abs(d) > WIDE_T:
                    return WIDE
                energy += d * d
                if energy > t2:
                    return WIDE
                out[m, b, k] = v
                k += 1
            if energy > t2:
                return WIDE
    return OK


def _codebook(bits, vals):
    """[look-ahead list of (length, symbol) by the next 8 bits] + {code: symbol} per length 9..16."""
    book = [[None] * 256] + [dict() for _ in range(16)]
    for sym, (code, length) in _huff_codes(bits, vals).items():
        if length <= 8:
            lo = code << (8 - length)
            for i in range(lo, lo + (1 << (8 - length))):
                book[0][i] = (length, sym)
        else:
            book[length][code] = sym
    return book


def entropy_decode(stream: JpegStream, first_interval: int = 0) -> np.ndarray:
    """The quantised zig-zag coefficients int16 [mcus, blocks per MCU, 64] of a parsed stream: the
    inverse of :func:`entropy`.  The first interval with a status other than OK raises
    (``first_interval`` offsets the interval number reported, for a batch)."""
    _, nb, mx, my = geometry(stream.H, stream.W, stream.sampling)
    mcus = mx * my
    per = stream.restart or mcus
    books = [_codebook(b, v) for b, v in stream.huff]
    qz = [[t[ZIGZAG[z]] for z in range(64)] for t in stream.qtables]
    out = np.zeros((mcus, nb, 64), dtype=np.int16)
    for it, (off, ln) in enumerate(stream.intervals):
        m0 = it * per
        st = _decode_interval(stream.data[off: off + ln], books, qz, nb, min(per, mcus - m0), out[m0: m0 + per])
        if st != OK:
            raise_status(st, first_interval + it)
    return out


# ----------------------------------------------------------------------------- chunked entropy decode contract
# The same coefficients from one lane per fixed-size byte chunk: the CHUNKED ENTROPY DECODE CONTRACT
# section of jpeg.hip's header comment; ops/csrc/jpeg_entropy_sync.h is the lane run the kernel and
# the host program compile.
SYNC_MAX_CHUNKS = 1024                 # chunks per interval, lanes per workgroup
SYNC_MAX_LEN = 1 << 28                 # bytes per interval: raw bit positions are 32-bit words


def chunk_bytes_for(longest: int, chunk_bytes: int = 32) -> int:
    """The effective chunk size: the smallest multiple of 16 that is >= ``chunk_bytes`` and cuts an
    interval of ``longest`` bytes into at most SYNC_MAX_CHUNKS chunks."""
    if int(chunk_bytes) != chunk_bytes or chunk_bytes < 16:
        raise ValueError("jpeg: chunk_bytes must be an integer >= 16")
    need = (longest + SYNC_MAX_CHUNKS - 1) // SYNC_MAX_CHUNKS
    return (max(int(chunk_bytes), need, 16) + 15) // 16 * 16


class _SyncInterval:
    """One interval for the lane runs: the unstuffed data and both maps between raw and data bytes."""

    def __init__(self, raw: bytes, books, nb: int) -> None:
        self.nb, self.books, self.n = nb, books, len(raw)
        a = np.frombuffer(raw, dtype=np.uint8)
        ff = np.flatnonzero(a == 0xFF)
        nxt = np.append(a, 1)[ff + 1]          # a 0xFF that ends the interval is stray too
        stray = ff[nxt != 0]
        end = int(stray[0]) if stray.size else len(raw)
        keep = np.ones(end, dtype=bool)
        keep[ff[ff < end] + 1] = False           # the stuffed zeros (all inside [0, end): nxt == 0 there)
        self.rawidx = np.append(np.flatnonzero(keep), end).tolist()      # data byte -> raw byte; [-1] = the data's end
        didx = np.full(len(raw) + 1, -1, dtype=np.int64)
        didx[self.rawidx] = np.arange(len(self.rawidx))
        self.dataidx = didx.tolist()             # raw byte -> data byte, -1: a stuffed zero or past the data
        self.buf = a[:end][keep].tobytes()
        self.raw = raw

    def guess(self, begin: int) -> int:
        stuffed = 0 < begin < self.n and self.raw[begin] == 0 and self.raw[begin - 1] == 0xFF
        return 8 * (begin + (1 if stuffed else 0))

    def run(self, state, end: int, out=None, first: int = 0):
        """Symbols from ``state`` = (raw bit, blk, k) while the position is before raw byte ``end``.
        -> (exit state or None, blocks started, blocks completed inside ``out``, error, its block).
        A start that is no data position (past a stray 0xFF) is TRUNCATED at once."""
        p, blk, k = state
        buf, nbits, rawidx, nb = self.buf, 8 * len(self.buf), self.rawidx, self.nb
        blocks = done = 0
        g = first
        nblk = len(out) if out is not None else 0
        if p >= 8 * end:
            return state, 0, 0, OK, 0
        di = self.dataidx[p >> 3]
        if di < 0:
            return None, 0, 0, TRUNCATED, g
        pd = 8 * di + (p & 7)

        def bits(at: int, n: int) -> int:
            i = at >> 3
            v = int.from_bytes(buf[i: i + 5].ljust(5, b"\0"), "big")
            return (v >> (40 - (at & 7) - n)) & ((1 << n) - 1)

        def symbol(book, at: int):
            left = nbits - at
            w = bits(at, 16)
            hit = book[0][w >> 8]
            if hit:
                length, sym = hit
            else:
                for length in range(9, 17):
                    sym = book[length].get(w >> (16 - length))
                    if sym is not None:
                        break
                else:
                    return -(TRUNCATED if left < 16 else BAD_CODE), 0
            if length > left:
                return -TRUNCATED, 0
            return sym, length
        while rawidx[pd >> 3] < end:
            tc = 0 if blk < nb - 2 else 1
            complete = False
            v = 0
            if k == 0:
                s, used = symbol(self.books[tc], pd)
                if s < 0:
                    return None, blocks, done, -s, g
                if s > 11:
                    return None, blocks, done, BAD_CODE, g
                if s:
                    if used + s > nbits - pd:
                        return None, blocks, done, TRUNCATED, g
                    v = bits(pd + used, s)
                    v = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                    used += s
                blocks += 1
                if v and 0 <= g < nblk:
                    out[g, 0] = v
                k = 1
            else:
                rs, used = symbol(self.books[2 + tc], pd)
                if rs < 0:
                    return None, blocks, done, -rs, g
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if rs == 0:
                        complete = True
                    elif r != 15:
                        return None, blocks, done, BAD_CODE, g
                    elif k + 16 > 63:
                        return None, blocks, done, OVERRUN, g
                    else:
                        k += 16
                elif s > 10:
                    return None, blocks, done, BAD_CODE, g
                elif k + r > 63:
                    return None, blocks, done, OVERRUN, g
                elif used + s > nbits - pd:
                    return None, blocks, done, TRUNCATED, g
                else:
                    v = bits(pd + used, s)
                    v = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                    used += s
                    k += r
                    if 0 <= g < nblk:
                        out[g, k] = v
                    k += 1
                    complete = k > 63
            if complete:
                if 0 <= g < nblk:
                    done += 1
                g += 1
                k = 0
                blk = 0 if blk + 1 == nb else blk + 1
            pd += used
        return (8 * rawidx[pd >> 3] + (pd & 7), blk, k), blocks, done, OK, 0


def entropy_decode_chunked(stream: JpegStream, chunk_bytes: int = 32, first_interval: int = 0,
                           stats: dict = None) -> np.ndarray:
    """What :func:`entropy_decode` returns, and raises, computed the way the CHUNKED ENTROPY DECODE
    CONTRACT says: one lane per chunk, Jacobi rounds until every lane starts where its predecessor
    ended, valid chain, placement, write pass, DC prefix sums, check pass; a flagged stream is
    handed to :func:`entropy_decode`, whose verdict stands.  ``stats`` receives ``chunks`` (all
    intervals), ``rounds`` (the largest of any interval), ``lane_runs``, ``chunk_bytes`` (the
    effective value) and ``serial_fallback``."""
    _, nb, mx, my = geometry(stream.H, stream.W, stream.sampling)
    mcus = mx * my
    per = stream.restart or mcus
    longest = max(ln for _, ln in stream.intervals)
    cb = chunk_bytes_for(longest, chunk_bytes)
    if longest >= SYNC_MAX_LEN:
        raise JpegUnsupported("jpeg: a restart interval of 2^28 bytes or more")
    books = [_codebook(b, v) for b, v in stream.huff]
    qz = np.asarray([[t[ZIGZAG[z]] for z in range(64)] for t in stream.qtables], dtype=np.int64)
    work = np.zeros((mcus * nb, 64), dtype=np.int64)
    chunks = rounds = lane_runs = completed = 0
    flag = False
    for it, (off, ln) in enumerate(stream.intervals):
        m0 = it * per
        nblk = min(per, mcus - m0) * nb
        out = work[m0 * nb: m0 * nb + nblk]
        n = (ln + cb - 1) // cb
        chunks += n
        if n == 0:
            continue
        iv = _SyncInterval(stream.data[off: off + ln], books, nb)
        ends = [min(ln, (c + 1) * cb) for c in range(n)]
        starts = [(0, 0, 0)] + [(iv.guess(c * cb), 0, 0) for c in range(1, n)]
        exits, counts = [None] * n, [0] * n
        run, r = list(range(n)), 0
        while run and r < n:                   # lane c is final after round c
            r += 1
            lane_runs += len(run)
            for c in run:
                exits[c], counts[c] = iv.run(starts[c], ends[c])[:2]
            nxt = []
            for c in run:
                if c + 1 < n and exits[c] is not None and exits[c] != starts[c + 1]:
                    starts[c + 1] = exits[c]
                    nxt.append(c + 1)
            run = nxt
        rounds = max(rounds, r)
        first = 0
        for c in range(n):                      # the valid chain, in order
            if c and exits[c - 1] is None:
                break
            at = first - (1 if starts[c][2] else 0)
            if at < nblk:
                _, _, done, err, where = iv.run(starts[c], ends[c], out, at)
                completed += done
                flag |= err != OK and where < nblk
            first += counts[c]
        # DC pass: 32-bit inclusive prefix sums per component, a failing predictor is not stored
        blk = np.arange(nblk) % nb
        for comp in range(3):
            sel = np.flatnonzero(blk < nb - 2 if comp == 0 else blk == nb - 3 + comp)
            pred = (np.cumsum(out[sel, 0]) + 2 ** 31) % 2 ** 32 - 2 ** 31
            ok = np.abs(pred) <= WIDE_T // int(qz[min(comp, 1), 0])
            flag |= not bool(ok.all())
            out[sel, 0] = np.where(ok, pred, 0)
    # check pass
    d = work * qz[(np.arange(mcus * nb) % nb >= nb - 2).astype(np.int64)]
    flag |= bool((np.abs(d) > WIDE_T).any() or ((d * d).sum(-1) > WIDE_T * WIDE_T).any())
    flag |= completed < mcus * nb
    if stats is not None:
        stats.update(chunks=chunks, rounds=rounds, lane_runs=lane_runs, chunk_bytes=cb, serial_fallback=bool(flag))
    if flag:
        return entropy_decode(stream, first_interval)
    return work.reshape(mcus, nb, 64).astype(np.int16)


def jpeg_decode(data) -> np.ndarray:
    """Baseline JPEG bytes -> uint8 [H, W, 3], the pixels a libjpeg decoder (PIL) returns for them:
    ``reconstruct(entropy_decode(parse(data)))`` with the stream's own quantisation tables."""
    st = data if isinstance(data, JpegStream) else parse(data)
    return reconstruct(entropy_decode(st), st.H, st.W, 0, st.sampling, tables=st.qtables)
