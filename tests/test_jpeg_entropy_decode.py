"""Entropy decode contract, CPU side: jpeg_format.parse / entropy_decode / ops.reference.jpeg_decode
against PIL on a corpus of Pillow-written and in-tree baseline streams, the parse refusals, the
refusal rule of the 32-bit (and libjpeg's 16-bit) arithmetic with crafted streams at its edge, the
malformed streams, the CPU path of ops.jpeg_decode, and the ``gpu_jpeg_decode`` flag / factory /
BlurCache / room wiring."""
from __future__ import annotations

import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as jc
import jpeg_stream_cases as sc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.game import imaging
from cassmantle_amd.game.imaging import BlurCache
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.ops import reference as ref
from jpeg_decode_cases import Scorer


def test_corpus_is_the_one_described():
    pil, intree = sc.pil_streams(), sc.intree_streams()
    assert len(pil) >= 20 * 7 and len(intree) == 41          # 180 when Pillow takes both restart keywords
    assert len({s.name for s in pil + intree}) == len(pil) + len(intree)
    big = sc.reference(intree[-1].data)[0]
    assert len(big.intervals) == 81 and big.restart == 1
    opt = jf.parse(next(s.data for s in pil if "optimize" in s.name and "100x75" in s.name))
    std = jf.parse(intree[0].data)
    assert opt.huff != std.huff                               # tables read from DHT, not assumed
    assert any(jf.parse(s.data).sampling == "444" for s in pil)


def test_reference_decode_equals_pil_on_every_stream():
    for s in sc.corpus() + sc.batch_streams():
        st, _, px, peak = sc.reference(s.data)
        exp = sc.pil_pixels(s.data)
        assert px.shape == exp.shape == (st.H, st.W, 3) and px.dtype == np.uint8, s.name
        assert np.array_equal(px, exp), (s.name, int(np.count_nonzero(px != exp)))
        assert 0 < peak < 2 ** 31, (s.name, peak)


def test_reference_jpeg_decode_is_the_composition():
    s = sc.corpus()[7]
    assert np.array_equal(ref.jpeg_decode(s.data), sc.reference(s.data)[2])
    assert np.array_equal(ref.jpeg_decode(jf.parse(s.data)), sc.reference(s.data)[2])


def test_entropy_decode_inverts_the_in_tree_coder():
    for s in sc.intree_streams() + sc.batch_streams():
        _, coef, _, _ = sc.reference(s.data)
        exp = jf.coefficients(s.img, s.quality, s.sampling)
        assert coef.dtype == np.int16 and coef.shape == exp.shape and np.array_equal(coef, exp), s.name


def test_parse_fields():
    img = jc.noise(17, 33)
    data = jf.jpeg_encode(img, 60, "420", 2)[0]
    st = jf.parse(data)
    assert (st.H, st.W, st.sampling, st.restart) == (17, 33, "420", 2)
    lq, cq = jf.quant_tables(60)
    assert st.qtables == (tuple(lq), tuple(cq))
    assert st.huff[0] == (tuple(jf._DC_LUMA[0]), tuple(jf._DC_LUMA[1]))
    assert st.huff[3] == (tuple(jf._AC_CHROMA[0]), tuple(jf._AC_CHROMA[1]))
    assert st.scan_offset == len(jf.header(17, 33, 60, "420", 2))
    assert len(st.intervals) == 3                             # 2 x 3 MCUs, 2 per interval
    # the intervals tile the entropy-coded segment: 2 marker bytes between them and after the last
    pos = st.scan_offset
    for i, (off, ln) in enumerate(st.intervals):
        assert off == pos and data[off + ln] == 0xFF
        assert data[off + ln + 1] == (0xD0 + i if i < 2 else 0xD9)
        pos = off + ln + 2
    assert pos == len(data)
    one = jf.parse(jf.jpeg_encode(img, 60, "444", 0)[0])
    assert one.restart == 0 and len(one.intervals) == 1 and one.sampling == "444"


def _save(img, mode="RGB", **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).convert(mode).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.mark.parametrize("name", ["progressive", "greyscale", "422", "cmyk"])
def test_parse_refuses_what_is_out_of_scope(name):
    img = jc.noise(24, 40)
    data = {"progressive": lambda: _save(img, progressive=True),
            "greyscale": lambda: _save(img, mode="L"),
            "422": lambda: _save(img, subsampling=1),
            "cmyk": lambda: _save(img, mode="CMYK")}[name]()
    assert Image.open(io.BytesIO(data)).size == (40, 24)      # a JPEG PIL reads
    with pytest.raises(jf.JpegUnsupported):
        jf.parse(data)
    with pytest.raises(ValueError):
        ops.jpeg_decode(data)


def test_parse_malformed_headers_and_markers():
    data = jf.jpeg_encode(jc.noise(17, 33), 75, "420", 2)[0]
    st = jf.parse(data)
    with pytest.raises(jf.JpegError):
        jf.parse(b"")
    with pytest.raises(jf.JpegError):
        jf.parse(data[1:])
    with pytest.raises(jf.JpegError):
        jf.parse(data[:st.scan_offset - 3])                   # header cut
    with pytest.raises(jf.JpegError):
        jf.parse(data[:-2])                                   # no EOI
    off, ln = st.intervals[0]
    swapped = bytearray(data)
    swapped[off + ln + 1] = 0xD1                              # RST1 where RST0 belongs
    with pytest.raises(jf.JpegError):
        jf.parse(bytes(swapped))
    with pytest.raises(jf.JpegError):                         # an interval and its marker missing
        jf.parse(data[:off] + data[off + ln + 2:])
    assert issubclass(jf.JpegError, ValueError) and issubclass(jf.JpegUnsupported, ValueError)


# ----------------------------------------------------------------------------- the refusal rule
def test_threshold_is_covered_by_the_32_bit_words():
    """the gain is re-derived from _idct_pass: below T every intermediate fits, with the rounding
    (< 1 per value) the first pass hands to the second, and T refuses no block of 8-bit samples"""
    l2, l1 = jf.idct_gain()
    assert 300000 < l2 < 400000 and l1 > 0
    assert jf.WIDE_T <= 6000
    assert jf.WIDE_T * l2 + l1 + 2 ** 17 < 2 ** 31
    assert jf.WIDE_T >= 1024 + 255 * 8 / 2                    # Parseval + half the norm of an all-255 table
    # libjpeg-turbo's 16-bit first-pass words: output <= 4 sqrt(8) ||column||, a sum of two <= 16 ||d||
    assert 16 * jf.WIDE_T < 2 ** 15


def test_streams_under_the_threshold_equal_pil_and_over_it_are_refused():
    seen_under = seen_over = 0
    for name, data, target in sc.energy_streams():
        norm = sc.block_norm(data)
        assert abs(norm - target) < 8, (name, norm)
        if target <= jf.WIDE_T:
            assert norm <= jf.WIDE_T, (name, norm)
            stats = {}
            st = jf.parse(data)
            got = jf.reconstruct(jf.entropy_decode(st), st.H, st.W, 0, st.sampling, stats, tables=st.qtables)
            assert np.array_equal(got, sc.pil_pixels(data)), (name, norm)
            assert stats["max_abs"] < 2 ** 31
            seen_under += 1
        else:
            assert norm > jf.WIDE_T, (name, norm)
            with pytest.raises(jf.JpegUnsupported) as e:
                ref.jpeg_decode(data)
            assert e.value.code == jf.WIDE and e.value.interval == 0, name
            seen_over += 1
    assert seen_under >= 14 and seen_over >= 10


def test_wide_block_in_a_later_interval_names_it():
    c = np.zeros((4, 3, 64), dtype=np.int16)
    c[:, 0, 0] = 5
    c[2, 1, 1] = 1023                                         # chroma Q(q50)[1] = 18: 18414 > T
    data = sc.craft(c, 50, 16, 16, "444", restart=1)
    with pytest.raises(jf.JpegUnsupported) as e:
        ref.jpeg_decode(data)
    assert (e.value.code, e.value.interval) == (jf.WIDE, 2)


# ----------------------------------------------------------------------------- malformed input
def test_malformed_streams_raise_jpeg_error_with_their_code():
    for m in sc.malformed():
        st = jf.parse(m.data)                                 # the header and the markers are fine
        with pytest.raises(jf.JpegError) as e:
            jf.entropy_decode(st)
        assert e.value.code == m.code, (m.name, e.value.code)
        with pytest.raises(ValueError):
            ops.jpeg_decode(m.data)
    t = sc.malformed()[0]
    with pytest.raises(jf.JpegError) as e:
        ref.jpeg_decode(t.data)
    assert e.value.interval == len(jf.parse(t.data).intervals) - 1


def test_arbitrary_damage_never_leaves_the_value_error_family():
    """every single-byte change and every truncation of a small stream: pixels or a ValueError"""
    data = jf.jpeg_encode(jc.noise(9, 7), 75, "420", 1)[0]
    rng = np.random.default_rng(5)
    for i in range(len(data)):
        b = bytearray(data)
        b[i] = int(rng.integers(0, 256))
        for cut in (bytes(b), data[:i]):
            try:
                out = ref.jpeg_decode(cut)
                assert out.dtype == np.uint8 and out.ndim == 3
            except ValueError as e:
                assert isinstance(e, (jf.JpegError, jf.JpegUnsupported)), (i, type(e))


def test_decode_tables_layout():
    t = jf.decode_tables(jf.parse(sc.intree_streams()[0].data).huff)
    assert t.dtype == np.int32 and t.shape == (4 * jf.DEC_TABLE_WORDS,)
    dc = t[:jf.DEC_TABLE_WORDS]
    look = dc[:128].view(np.uint16)
    assert look[0] == (2 << 8) | 0                            # DC luma: code 00 = category 0
    assert look[0b01000000] == (3 << 8) | 1 and look[0xFF] == 0          # 010 = category 1; 9 ones: longer
    assert dc[128 + 15] == 0xFF80 and dc[128 + 8] == 0xFF80   # limits, left-justified (last code 111111110)


# ----------------------------------------------------------------------------- ops.jpeg_decode on the CPU
def test_ops_jpeg_decode_cpu_is_the_reference():
    s = sc.corpus()[3]
    exp = sc.pil_pixels(s.data)
    out = ops.jpeg_decode(s.data)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device.type == "cpu"
    assert np.array_equal(out.numpy(), exp)
    assert np.array_equal(ops.jpeg_decode(jf.parse(s.data), device="cpu").numpy(), exp)
    buf = torch.zeros(exp.shape, dtype=torch.uint8)
    assert ops.jpeg_decode(s.data, out=buf) is buf and np.array_equal(buf.numpy(), exp)
    batch = [b.data for b in sc.batch_streams()]
    got = ops.jpeg_decode(batch)
    assert tuple(got.shape) == (3, 24, 40, 3)
    for i, b in enumerate(batch):
        assert np.array_equal(got[i].numpy(), sc.pil_pixels(b))
    with pytest.raises(ValueError):
        ops.jpeg_decode([batch[0], s.data])                   # another geometry
    with pytest.raises(ValueError):
        ops.jpeg_decode([batch[0], jf.jpeg_encode(jc.noise(24, 40), 50, "420", 2)[0]])      # other tables
    with pytest.raises(ValueError):
        ops.jpeg_decode([])
    with pytest.raises(ValueError):
        ops.jpeg_decode(s.data, out=torch.zeros((3, 3, 3), dtype=torch.uint8))


# ----------------------------------------------------------------------------- flag, factory, wiring
def test_flag_and_factory():
    from cassmantle_amd.runtime.factory import build_jpeg_decode_fn
    d = Config()
    assert d.model.gpu_jpeg_decode is False and d.model.jpeg_decode_min_intervals >= 1
    c = Config.from_args(["--gpu_jpeg_decode", "--jpeg_decode_min_intervals", "4"], base=Config())
    assert c.model.gpu_jpeg_decode is True and c.model.jpeg_decode_min_intervals == 4
    e = Config.from_env({"CASSMANTLE_GPU_JPEG_DECODE": "1"})
    assert e.model.gpu_jpeg_decode is True
    assert build_jpeg_decode_fn(c, "cpu") is None             # flag set, no GPU
    assert build_jpeg_decode_fn(d, "cpu") is None and build_jpeg_decode_fn(d, "cuda") is None
    c.model.gpu_blur = False
    assert build_jpeg_decode_fn(c, "cuda") is None            # needs gpu_blur


def _jpeg_and_pixels():
    jpeg = imaging.encode_jpeg(jc.gradient(16, 24), 75)
    return jpeg, imaging.decode_jpeg(jpeg)


def test_blur_cache_without_decode_fn_calls_decode_jpeg(monkeypatch):
    jpeg, px = _jpeg_and_pixels()
    calls = []
    monkeypatch.setattr(imaging, "decode_jpeg", lambda data: calls.append(data) or px)
    seen = []
    cache = BlurCache(blur_fn=lambda arr, r: seen.append(arr) or np.asarray(arr), bucket=0.25)
    assert cache.decode_fn is None
    cache.get("v", jpeg, 1.0)
    cache.get("v", jpeg, 2.0)
    assert calls == [jpeg] and seen[0] is px and seen[1] is px          # decoded once per version


def test_blur_cache_uses_decode_fn_and_falls_back_on_none(monkeypatch):
    jpeg, px = _jpeg_and_pixels()
    host_calls = []
    monkeypatch.setattr(imaging, "decode_jpeg", lambda data: host_calls.append(data) or px)
    device_px = px.copy()
    fn_calls = []

    def fake(data):
        fn_calls.append(data)
        return device_px
    seen = []
    cache = BlurCache(blur_fn=lambda arr, r: seen.append(arr) or np.asarray(arr), bucket=0.25, decode_fn=fake)
    cache.get("v", jpeg, 1.0)
    cache.get("v", jpeg, 2.0)
    assert fn_calls == [jpeg] and host_calls == [] and seen[0] is device_px and seen[1] is device_px
    assert cache._decoded[0] == "v" and cache._decoded[1] is device_px          # cached as today
    # a registered device source still wins
    src = px.copy()
    cache.set_source("w", src)
    cache.get("w", jpeg, 1.0)
    assert seen[-1] is src and fn_calls == [jpeg]
    # None = "use PIL"
    refusing = BlurCache(blur_fn=lambda arr, r: seen.append(arr) or np.asarray(arr), bucket=0.25,
                         decode_fn=lambda data: fn_calls.append(data))
    refusing.get("v", jpeg, 1.0)
    assert host_calls == [jpeg] and seen[-1] is px and len(fn_calls) == 2


def test_room_and_service_pass_decode_fn_through():
    from cassmantle_amd.game.service import GameService

    def fake(data):
        return None
    svc = GameService(Config(), Scorer(), decode_fn=fake)
    assert svc.room("").blur_cache.decode_fn is fake
    assert GameService(Config(), Scorer()).room("").blur_cache.decode_fn is None


def test_build_service_builds_the_decode_fn(monkeypatch):
    from cassmantle_amd.runtime import factory
    seen = {}
    marker = object()
    monkeypatch.setattr(factory, "build_jpeg_decode_fn", lambda cfg, device=None: marker)
    monkeypatch.setattr(factory, "GameService", lambda cfg, scorer, **kw: seen.update(kw) or "svc")
    cfg = Config()
    cfg.model.image_model = "solid"
    assert factory.build_service(cfg, scorer=Scorer(), prompt_gen=None, blur_fn=None, blur_jpeg_fn=None,
                                 content_jpeg_fn=None) == "svc"
    assert seen["decode_fn"] is marker
