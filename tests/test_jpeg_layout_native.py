"""The JPEG codec's buffer layout (ops/csrc/jpeg_layout.h, the text the bindings compile) as a host
program: tests/native/jpeg_layout_host.cpp built plain and with ASan + UBSan on the host, a
stand-alone executable that prints every field of the layout for a list of argument tuples.  Every
field equals what jpeg_format gives independently (geometry, the bits-per-block bounds, the header
lengths), every limit accepts its largest value and refuses the next with its message, and the
accepted extremes run without a sanitizer report: the arithmetic stays in 64 bits.  Nothing runs on
a GPU.

Three of the limits the layout reports cannot be the first to refuse, because an earlier one is
tighter: the payload bound keeps B * blocks * 416 below 2^31, so the symbol count of one image
(blocks * 64 < 2^31) and the launch grids (B * blocks < 256 * (2^31 - 1), B * intervals < 2^31 - 1)
are far inside theirs, and the bit-offset bound (bits per interval < 2^32) keeps stride =
ceil(bits / 32) at or below 2^27 < 2^30.  test_limits_behind_tighter_ones checks that at the extremes
the tighter limits accept."""
from __future__ import annotations

import itertools
import os
import subprocess

import pytest

from cassmantle_amd.ops import jpeg_format as jf
from test_jpeg_entropy_native import CSRC, CXX, OUT, ROOT, SANITIZE

DRIVER = os.path.join(ROOT, "tests", "native", "jpeg_layout_host.cpp")
QUALITY = 75
SIDES = [(1, 1), (8, 8), (16, 16), (17, 9), (24, 40), (64, 48)]
BUILDS = [("jpeg_layout_plain", []), ("jpeg_layout_asan", SANITIZE)]
INTERVAL_RESTART = "jpeg: the HIP encoder needs 1 <= restart_mcus <= 65535"
BLOCK_RESTART = "jpeg: restart_mcus 0..65535"
SIDES_MSG = "jpeg: image sides must be below 65536"
PAYLOAD = "jpeg: batch too large for 32-bit payload offsets"
BIT_OFFSETS = "jpeg: restart interval too long for 32-bit bit offsets"
OPT_BATCH = "jpeg: at most 65535 images per call with optimised Huffman tables"


def _build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [DRIVER] + [os.path.join(CSRC, h) for h in ("jpeg_layout.h", "jpeg_entropy_blk.h", "jpeg_huff_opt.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-I", CSRC, *flags, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, lines, tmp_path):
    """One dict of fields, or the refusal message, per input line."""
    path = tmp_path / "args.txt"
    path.write_text("".join(" ".join(str(int(v)) if not isinstance(v, str) else v for v in ln) + "\n" for ln in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = []
    for ln in r.stdout.splitlines():
        head, _, rest = ln.partition(" ")
        out.append(rest if head == "refused" else {k: int(v) for k, v in (w.split("=") for w in rest.split())})
        assert head in ("ok", "refused"), ln
    assert len(out) == len(lines)
    return out


def header_bytes(H, W, sampling, restart, optimized, lj):
    """The header ops.jpeg_encode uploads: whole, or with optimised tables without its DHT segment."""
    layout = "pil" if lj else "compact"
    if optimized:
        return sum(len(p) for p in jf.header_parts(H, W, QUALITY, sampling, restart, layout))
    return len(jf.header(H, W, QUALITY, sampling, restart, None, layout))


def geometry(H, W, sampling, restart):
    _, nb, mx, my = jf.geometry(H, W, sampling)
    mcus = mx * my
    per = min(restart, mcus) if restart else mcus
    return dict(nb=nb, mx=mx, my=my, mcus=mcus, restart=restart or mcus, per=per, nint=-(-mcus // per))


def bits_bound(optimized):
    return jf.block_bits_bound_optimized() if optimized else jf.block_bits_bound()


def payload_per_image(g, hdr, optimized, lj):
    """The coder's worst case for one image, in bytes: header, 416 (417) per block, 3 per interval."""
    cap = hdr + ((4 + (jf.DHT_EXTRA_PIL if lj else 0) + 4 * (17 + 256)) if optimized else 0)
    return cap + g["mcus"] * g["nb"] * (417 if optimized else 416) + g["nint"] * 3


def expected(B, H, W, sampling, restart, blocks, optimized, lj, hdr):
    g = geometry(H, W, sampling, restart)
    nblk, nivals = B * g["mcus"] * g["nb"], B * g["nint"]
    stride = (g["per"] * g["nb"] * bits_bound(optimized) + 31) // 32 if blocks else 0
    prefix = B + 1 + int(blocks) + (B if optimized else 0)
    dht = 4 + (jf.DHT_EXTRA_PIL if lj else 0) + 4 * (17 + 256)
    return dict(g, coef=nblk * 64, work=prefix + 2 * nivals, blk=nblk + nivals if blocks else 0,
                scratch=nivals * stride, hopt=2 * B * 544 if optimized else 0,
                hdrs=B * (hdr + dht) if optimized else 0, stride=stride, hdr_cap=hdr + (dht if optimized else 0),
                prefix=prefix, err=B + 1 if blocks else -1, hdr_lens=B + 1 + int(blocks) if optimized else -1,
                lens=prefix, offs=prefix + nivals, slack=int(blocks))


def encode_line(B, H, W, sampling, restart, blocks, optimized, lj, hdr=None):
    hdr = header_bytes(H, W, sampling, min(max(restart, 0), 65535), optimized, lj) if hdr is None else hdr
    return ("E", B, H, W, sampling == "420", restart, blocks, optimized, lj, hdr)


def cases():
    out = []
    for (H, W), sampling, B in itertools.product(SIDES, jf.SAMPLINGS, (1, 3)):
        _, _, mx, my = jf.geometry(H, W, sampling)
        for restart in (0, 1, 2, 5, mx, mx * my + 3):
            for blocks, optimized, lj in itertools.product((False, True), repeat=3):
                out.append((B, H, W, sampling, restart, blocks, optimized, lj))
    return out


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_every_field_is_what_jpeg_format_gives(name, flags, tmp_path):
    items = cases()
    assert len(items) == 6 * 2 * 2 * 6 * 8
    got = run(_build(name, flags), [encode_line(*c) for c in items], tmp_path)
    for c, g in zip(items, got):
        B, H, W, sampling, restart, blocks, optimized, lj = c
        if restart == 0 and not blocks:
            assert g == INTERVAL_RESTART, c
            continue
        assert g == expected(*c, header_bytes(H, W, sampling, restart, optimized, lj)), c
        # the host reads work[:prefix]; lens starts right behind it, offs B * nint words later
        assert g["lens"] == g["prefix"] and g["offs"] == g["lens"] + B * g["nint"], c
        assert g["work"] == g["offs"] + B * g["nint"], c


def largest(ok, lo, hi):
    """The largest v in [lo, hi) with ok(v), ok being monotone and ok(lo) true."""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def limit_cases():
    """(line, None if accepted else the message): the largest accepted value of every limit and the
    first refused one."""
    out = []
    for blocks in (False, True):
        # sides
        for H, W in ((65535, 8), (8, 65535)):
            out.append((encode_line(1, H, W, "444", 1, blocks, False, False), None))
        for H, W in ((65536, 8), (8, 65536)):
            out.append((encode_line(1, H, W, "444", 1, blocks, False, False, hdr=600), SIDES_MSG))
        # the restart range of either coder
        low, msg = (0, BLOCK_RESTART) if blocks else (1, INTERVAL_RESTART)
        for restart, want in ((low, None), (low - 1, msg), (65535, None), (65536, msg)):
            out.append((encode_line(1, 64, 48, "420", restart, blocks, False, False), want))
    # the payload bound, along the batch (standard tables) and along the image width
    for blocks, optimized, lj in itertools.product((False, True), repeat=3):
        sampling, restart = "444", 1
        if not optimized:
            hdr = header_bytes(8, 8, sampling, restart, optimized, lj)
            bmax = (2 ** 31 - 1) // payload_per_image(geometry(8, 8, sampling, restart), hdr, optimized, lj)
            out.append((encode_line(bmax, 8, 8, sampling, restart, blocks, optimized, lj), None))
            out.append((encode_line(bmax + 1, 8, 8, sampling, restart, blocks, optimized, lj), PAYLOAD))
        H = 8 * 700

        def fits(mx):
            hdr = header_bytes(H, 8 * mx, sampling, restart, optimized, lj)
            return payload_per_image(geometry(H, 8 * mx, sampling, restart), hdr, optimized, lj) < 2 ** 31
        mx = largest(fits, 1, 8192)
        assert 1 < mx < 8191
        out.append((encode_line(1, H, 8 * mx, sampling, restart, blocks, optimized, lj), None))
        out.append((encode_line(1, H, 8 * mx + 1, sampling, restart, blocks, optimized, lj), PAYLOAD))
    # bit offsets within an interval: the block coder without restart markers, along the image width
    for optimized in (False, True):
        H = 8 * 930
        mx = largest(lambda m: m * 930 * 3 * bits_bound(optimized) < 2 ** 32, 1, 8192)
        assert 1 < mx < 8191
        out.append((encode_line(1, H, 8 * mx, "444", 0, True, optimized, False), None))
        out.append((encode_line(1, H, 8 * mx + 1, "444", 0, True, optimized, False), BIT_OFFSETS))
    # images per call with optimised tables
    for blocks in (False, True):
        out.append((encode_line(65535, 1, 1, "444", 1, blocks, True, False), None))
        out.append((encode_line(65536, 1, 1, "444", 1, blocks, True, False), OPT_BATCH))
    return out


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_every_limit_accepts_its_largest_value_and_refuses_the_next(name, flags, tmp_path):
    items = limit_cases()
    got = run(_build(name, flags), [ln for ln, _ in items], tmp_path)
    for (ln, want), g in zip(items, got):
        if want is not None:
            assert g == want, ln
            continue
        assert isinstance(g, dict), (ln, g)
        _, B, H, W, s420, restart, blocks, optimized, lj, hdr = ln
        assert g == expected(B, H, W, "420" if s420 else "444", restart, blocks, optimized, lj, hdr), ln


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_limits_behind_tighter_ones(name, flags, tmp_path):
    """Symbol counts, stride and the launch grids (see the module text): at every accepted extreme
    they are inside their bounds, so no input reaches their messages."""
    items = [ln for ln, want in limit_cases() if want is None]
    for ln, g in zip(items, run(_build(name, flags), items, tmp_path)):
        B = ln[1]
        assert g["mcus"] * g["nb"] * 64 < 2 ** 31 and g["stride"] <= 2 ** 27, ln
        assert B * g["mcus"] * g["nb"] < 256 * (2 ** 31 - 1) and B * g["nint"] < 2 ** 31 - 1, ln


def decode_expected(B, H, W, sampling, restart, chunked, nbytes, ngroups):
    g = geometry(H, W, sampling, restart)
    ncoef, nivals = B * g["mcus"] * g["nb"] * 64, B * g["nint"]
    return dict(g, nivals=nivals, ncoef=ncoef, buf=ncoef + (16 if chunked else 8), planes=ncoef,
                staged_min=8 * nivals + nbytes, sync_bytes=4 * nivals + 8 * ngroups)


@pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
@pytest.mark.parametrize("name,flags", BUILDS)
def test_decode_sizes_and_limits(name, flags, tmp_path):
    items = []
    for (H, W), sampling, B, chunked in itertools.product(SIDES, jf.SAMPLINGS, (1, 3), (False, True)):
        _, _, mx, my = jf.geometry(H, W, sampling)
        for restart in (0, 1, 2, 5, mx, mx * my + 3):
            items.append(((B, H, W, sampling, restart, chunked, 1000 + H, 7), None))
    for chunked in (False, True):
        grid = "jpeg: too many restart intervals or blocks for one launch" if chunked \
            else "jpeg: too many restart intervals for one launch"
        sides, rst = "jpeg: image sides must be in 1..65535", "jpeg: restart interval 0..65535"
        bmax = (256 * (2 ** 31 - 1) - 1) // (64 * 6)           # 128 x 128, 4:2:0: 384 blocks per image
        items += [((1, 65535, 65535, "444", 0, chunked, 2 ** 32 - 2, 1), None),
                  ((1, 65536, 8, "444", 0, chunked, 0, 0), sides), ((1, 8, 65536, "444", 0, chunked, 0, 0), sides),
                  ((1, 0, 8, "444", 0, chunked, 0, 0), sides), ((0, 8, 8, "444", 0, chunked, 0, 0), sides),
                  ((1, 8, 8, "444", 65535, chunked, 0, 0), None), ((1, 8, 8, "444", 65536, chunked, 0, 0), rst),
                  ((1, 8, 8, "444", -1, chunked, 0, 0), rst),
                  ((2 ** 31 - 2, 1, 1, "444", 0, chunked, 0, 0), None), ((2 ** 31 - 1, 1, 1, "444", 0, chunked, 0, 0), grid),
                  ((bmax, 128, 128, "420", 0, chunked, 0, 0), None), ((bmax + 1, 128, 128, "420", 0, chunked, 0, 0), grid)]
    lines = [("D", B, H, W, s == "420", r, c, n, ng) for (B, H, W, s, r, c, n, ng), _ in items]
    for (args, want), g in zip(items, run(_build(name, flags), lines, tmp_path)):
        assert g == (decode_expected(*args) if want is None else want), args
