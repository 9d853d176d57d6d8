"""The libjpeg forward contract on the CPU (ops/jpeg_format.py: coefficients_libjpeg, the PIL header
layout): ``reference.jpeg_encode(..., restart_mcus=0, transform="libjpeg")`` is the file Pillow
writes, byte for byte, on every case of jpeg_libjpeg_cases.py, with standard and with optimised
Huffman tables; the coefficients are the ones in Pillow's stream; the cases reach every rule; the
AC guard never fires; restart markers change no pixel; ``transform="matrix"`` is untouched; and the
configuration spells the mode.  Nothing runs on a GPU."""
from __future__ import annotations

import numpy as np
import pytest

import jpeg_libjpeg_cases as lc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.ops import reference as ref

LJ = "libjpeg"


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("size", lc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bytes_equal_pillow(kind, size):
    """standard tables against save(quality, subsampling), optimised against optimize=True"""
    H, W = size
    img = lc.image(kind, H, W)
    for q in lc.QUALITIES:
        for s in lc.SAMPLINGS:
            got = ref.jpeg_encode(img, q, s, restart_mcus=0, transform=LJ)
            assert got == [lc.pil_bytes(kind, H, W, q, s)], (kind, H, W, q, s)
            got = ref.jpeg_encode(img, q, s, restart_mcus=0, huffman="optimized", transform=LJ)
            assert got == [lc.pil_bytes(kind, H, W, q, s, optimize=True)], (kind, H, W, q, s, "optimized")


@pytest.mark.parametrize("kind", lc.KINDS)
def test_bytes_equal_a_plain_save(kind):
    """save(quality=q) with no subsampling argument is the 4:2:0 file"""
    for H, W in lc.SIZES:
        for q in lc.QUALITIES:
            got = ref.jpeg_encode(lc.image(kind, H, W), q, restart_mcus=0, transform=LJ)
            assert got == [lc.pil_bytes(kind, H, W, q, None)], (kind, H, W, q)


@pytest.mark.parametrize("sampling", lc.SAMPLINGS)
def test_coefficients_equal_pillows_stream(sampling):
    for kind in lc.KINDS:
        for H, W in lc.SIZES:
            for q in lc.QUALITIES:
                stream = jf.parse(lc.pil_bytes(kind, H, W, q, sampling))
                assert stream.sampling == sampling and stream.restart == 0
                exp = jf.entropy_decode(stream)
                got = jf.coefficients(lc.image(kind, H, W), q, sampling, transform=LJ)
                assert np.array_equal(got.reshape(exp.shape), exp), (kind, H, W, q, sampling)


def _stats(kind, H, W, q=75, sampling="420"):
    st = {}
    jf.coefficients(lc.image(kind, H, W), q, sampling, transform=LJ, stats=st)
    return st


def test_cases_reach_every_rule():
    """from the model's own statistics: dummy blocks, the chained dummy DC, the even-H chroma row,
    a chroma mean over a replicated row, both bias values, 32-bit intermediates"""
    for H, W in ((9, 7), (17, 33), (33, 16), (48, 23), (1, 1), (8, 8), (24, 40)):
        assert _stats("noise", H, W)["dummy_blocks"] > 0, (H, W)
    assert _stats("noise", 16, 16)["dummy_blocks"] == 0
    one = _stats("noise", 1, 1)
    assert one["dummy_blocks"] == 3 and one["dummy_chain"] == 2          # Y10 and Y11 follow a dummy
    for H, W in ((8, 8), (24, 40)):
        st = _stats("noise", H, W)
        assert st["chroma_bottom_rows"] > 0 and st["odd_row_pairs"] == 0, (H, W)
        # the rule matters there: padding the image rows to 16 first gives other coefficients
        img = lc.image("noise", H, W)
        padded = np.concatenate([img, np.repeat(img[-1:], 16 - H % 16, axis=0)])
        a = jf.coefficients(img, 75, "420", transform=LJ)
        b = jf.coefficients(padded, 75, "420", transform=LJ)
        assert a.shape == b.shape and not np.array_equal(a[:, 4:], b[:, 4:]), (H, W)
    for H, W in ((9, 7), (17, 33), (33, 16)):
        assert _stats("noise", H, W)["odd_row_pairs"] == 1, (H, W)
    total = {"bias1": 0, "bias2": 0}
    for H, W in lc.SIZES:
        st = _stats("noise", H, W)
        assert st["max_abs"] < 1 << 31 and st["ac_clamped"] == 0
        total["bias1"] += st["bias1"]
        total["bias2"] += st["bias2"]
    assert total["bias1"] > 0 and total["bias2"] > 0, total
    assert _stats("noise", 16, 16, sampling="444")["dummy_blocks"] == 0


def test_ac_guard_never_fires():
    """the 126 extremal blocks (samples in {0, 255} on the sign of a DCT basis function) at quality
    100, where every quantisation value is 1: |AC| <= 1020, and Pillow codes the same values"""
    blocks = lc.extremal_blocks()
    assert blocks.shape == (126, 8, 8)
    f = jf.fdct_libjpeg(blocks - 128)
    v = jf.quantise_libjpeg(f, np.ones((8, 8), dtype=np.int64))
    raw = np.sign(f) * ((np.abs(f) + 4) // 8)
    assert np.array_equal(v, raw.reshape(126, 64))                       # nothing was clamped
    peak = int(np.abs(v[:, 1:]).max())
    assert 1000 < peak <= 1020, peak
    grey = np.repeat(blocks.transpose(1, 0, 2).reshape(8, 126 * 8)[..., None], 3, -1).astype(np.uint8)
    st = {}
    coef = jf.coefficients(grey, 100, "444", transform=LJ, stats=st)
    assert st["ac_clamped"] == 0 and int(np.abs(coef[:, 0, 1:]).max()) == peak
    pil = jf.entropy_decode(jf.parse(lc.pil_encode(grey, 100, "444")))
    assert np.array_equal(coef, pil.reshape(coef.shape))


@pytest.mark.parametrize("sampling", lc.SAMPLINGS)
def test_restart_markers_change_no_pixel(sampling):
    for H, W in ((17, 33), (48, 23), (1, 1)):
        img = lc.image("noise", H, W)
        plain = ref.jpeg_encode(img, 75, sampling, restart_mcus=0, transform=LJ)[0]
        want = lc.decode(plain)
        assert np.array_equal(ref.jpeg_decoded(img, 75, sampling, transform=LJ)[0], want)
        for r in (1, 2, 3):
            for huffman in jf.HUFFMAN_MODES:
                data = ref.jpeg_encode(img, 75, sampling, restart_mcus=r, huffman=huffman, transform=LJ)[0]
                assert jf.parse(data).restart == r
                assert np.array_equal(lc.decode(data), want), (H, W, sampling, r, huffman)
                assert np.array_equal(jf.jpeg_decode(data), want)


def test_pil_header_layout():
    img = lc.image("noise", 17, 33)
    for r in (0, 2):
        data = ref.jpeg_encode(img, 75, "420", restart_mcus=r, transform=LJ)[0]
        hdr = jf.header(17, 33, 75, "420", r, None, "pil")
        assert data.startswith(hdr)
        assert hdr.count(b"\xff\xdb\x00\x43") == 2 and hdr.count(b"\xff\xc4") == 4
        assert (b"\xff\xdd\x00\x04" in hdr) == bool(r)
        pre, suf = jf.header_parts(17, 33, 75, "420", r, "pil")
        assert hdr == pre + jf.dht_segment(None, "pil") + suf
        assert len(jf.dht_segment(None, "pil")) == len(jf.dht_segment()) + jf.DHT_EXTRA_PIL


def test_matrix_transform_is_untouched():
    for name, img in lc.images():
        for s in lc.SAMPLINGS:
            for r in (0, 2):
                for huffman in jf.HUFFMAN_MODES:
                    old = jf.jpeg_encode(img, 75, s, r, huffman=huffman)
                    assert ref.jpeg_encode(img, 75, s, r, huffman=huffman, transform="matrix") == old, (name, s, r)
                    assert ops.jpeg_encode(img, 75, s, r, huffman=huffman) == old
        assert np.array_equal(jf.coefficients(img, 75, "420"), jf.coefficients(img, 75, "420", "matrix"))
    img = lc.image("noise", 24, 40)
    assert ref.jpeg_encode(img, 75, "420", 0, transform=LJ) != ref.jpeg_encode(img, 75, "420", 0)
    assert jf.header(24, 40, 75, "420", 0) == jf.header(24, 40, 75, "420", 0, None, "compact")


def test_cpu_path_hands_the_transform_to_the_reference():
    import torch
    img = lc.image("noise", 17, 33)
    exp = [lc.pil_bytes("noise", 17, 33, 75, "420")]
    assert ops.jpeg_encode(img, 75, "420", 0, transform=LJ) == exp
    outs, px = ops.jpeg_encode(torch.from_numpy(img.copy()), 75, "420", 0, return_decoded=True, transform=LJ)
    assert outs == exp and np.array_equal(px[0].numpy(), lc.decode(exp[0]))


def test_bad_values_are_refused():
    img = lc.image("noise", 8, 8)
    for bad in ("islow", "LIBJPEG", None, 1):
        with pytest.raises(ValueError, match="transform"):
            ops.jpeg_encode(img, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            ref.jpeg_encode(img, transform=bad)
        with pytest.raises(ValueError, match="transform"):
            jf.coefficients(img, 75, "420", transform=bad)
        with pytest.raises(ValueError, match="transform"):
            ref.jpeg_decoded(img, transform=bad)
    with pytest.raises(ValueError, match="layout"):
        jf.header(8, 8, 75, "420", 0, None, "jfif")


def test_flag_environment_and_factory_spelling():
    from cassmantle_amd.runtime import factory
    d = Config()
    assert d.model.jpeg_transform == "matrix"
    assert "transform" not in factory._jpeg_encode_args(d, 64)           # the default call is the parent's
    c = Config.from_args(["--jpeg_transform", "libjpeg", "--gpu_jpeg"], base=Config())
    assert c.model.jpeg_transform == "libjpeg"
    assert Config.from_args(["--jpeg-transform=libjpeg"], base=Config()).model.jpeg_transform == "libjpeg"
    assert Config.from_env({"CASSMANTLE_JPEG_TRANSFORM": "libjpeg"}).model.jpeg_transform == "libjpeg"
    assert factory.jpeg_transform(c) == "libjpeg"
    assert factory._jpeg_encode_args(c, 64)["transform"] == "libjpeg"
    c.model.jpeg_entropy, c.model.jpeg_restart_mcus, c.model.jpeg_huffman = "block", -1, "optimized"
    assert factory._jpeg_encode_args(c, 64) == {"restart_mcus": 0, "entropy": "block", "huffman": "optimized",
                                                 "transform": "libjpeg"}
    bad = Config()
    bad.model.gpu_jpeg = bad.model.gpu_jpeg_content = True
    bad.model.jpeg_transform = "jfdctint"
    with pytest.raises(ValueError, match="jpeg_transform"):
        factory.jpeg_transform(bad)
    with pytest.raises(ValueError, match="jpeg_transform"):
        factory.build_blur_jpeg_fn(bad, "cuda")
    with pytest.raises(ValueError, match="jpeg_transform"):
        factory.build_content_jpeg_fn(bad, "cuda")
