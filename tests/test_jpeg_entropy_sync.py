"""The chunked entropy decode contract on the CPU: jpeg_format.entropy_decode_chunked (one lane per
chunk, Jacobi rounds, valid chain, placement, write, DC and check passes) returns what
entropy_decode returns and raises what it raises, on the corpus, the malformed and crafted streams
of jpeg_stream_cases.py, streams with stuffed bytes at the chunk seams and a fixed-seed mutation
pass; its statistics; the CPU path of ops.jpeg_decode(mode="chunked"); and the
``jpeg_decode_chunked`` flag / factory wiring."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_stream_cases as sc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.ops import jpeg_format as jf


def _outcome(fn):
    """('ok', coefficients) or ('raised', class, code, interval)"""
    try:
        return ("ok", fn())
    except ValueError as e:
        return ("raised", type(e), getattr(e, "code", None), getattr(e, "interval", None))


def _same(a, b) -> bool:
    if a[0] != b[0]:
        return False
    return np.array_equal(a[1], b[1]) if a[0] == "ok" else a[1:] == b[1:]


# ----------------------------------------------------------------------------- equality
@pytest.mark.parametrize("chunk", [16, 32, 64])
def test_chunked_equals_the_serial_decode_on_the_corpus(chunk):
    streams = sc.corpus() + sc.batch_streams()
    assert len(streams) > 150
    for s in streams:
        stats = {}
        got = jf.entropy_decode_chunked(jf.parse(s.data), chunk, stats=stats)
        assert got.dtype == np.int16 and np.array_equal(got, sc.reference(s.data)[1]), s.name
        assert stats["serial_fallback"] is False and 1 <= stats["rounds"] <= stats["chunks"], (s.name, stats)
        assert stats["lane_runs"] >= stats["chunks"] and stats["chunk_bytes"] % 16 == 0


def test_malformed_and_wide_streams_raise_what_the_serial_decode_raises():
    cases = [(m.name, m.data, m.code) for m in sc.malformed()]
    cases += [(n, d, jf.WIDE) for n, d, t in sc.energy_streams() if t > jf.WIDE_T]
    assert len(cases) >= 13
    for name, data, code in cases:
        st = jf.parse(data)
        with pytest.raises(ValueError) as want:
            jf.entropy_decode(st, 7)
        for chunk in (16, 32, 64):
            stats = {}
            with pytest.raises(ValueError) as got:
                jf.entropy_decode_chunked(st, chunk, 7, stats)
            assert type(got.value) is type(want.value), name
            assert (got.value.code, got.value.interval) == (want.value.code, want.value.interval) == \
                (code, want.value.interval), name
            assert stats["serial_fallback"] is True, name
    under = [(n, d) for n, d, t in sc.energy_streams() if t <= jf.WIDE_T]
    assert len(under) >= 14
    for name, data in under:                                   # 2040 and 16 * 127: they decode
        stats = {}
        got = jf.entropy_decode_chunked(jf.parse(data), 16, stats=stats)
        assert np.array_equal(got, sc.reference(data)[1]) and not stats["serial_fallback"], name


def test_wide_block_in_a_later_interval_names_it():
    c = np.zeros((4, 3, 64), dtype=np.int16)
    c[:, 0, 0] = 5
    c[2, 1, 1] = 1023
    st = jf.parse(sc.craft(c, 50, 16, 16, "444", restart=1))
    with pytest.raises(jf.JpegUnsupported) as e:
        jf.entropy_decode_chunked(st)
    assert (e.value.code, e.value.interval) == (jf.WIDE, 2)


# ----------------------------------------------------------------------------- statistics
def test_stats_and_the_chunk_size_rule():
    one = next(s for s in sc.corpus() if len(jf.parse(s.data).intervals) == 1 and jf.parse(s.data).intervals[0][1] <= 16)
    stats = {}
    jf.entropy_decode_chunked(jf.parse(one.data), 16, stats=stats)
    assert stats == dict(chunks=1, rounds=1, lane_runs=1, chunk_bytes=16, serial_fallback=False)
    # 16-byte chunks would be more than 1024: the chunk grows to the next multiple of 16 that fits
    data = sc._pil_save(jc.noise(256, 256, seed=1), quality=75)
    st = jf.parse(data)
    assert len(st.intervals) == 1
    ln = st.intervals[0][1]
    assert ln > 32 * 1024 and ln <= 48 * 1024                   # so the rule gives 48
    want = next(cb for cb in range(16, 1 << 20, 16) if (ln + cb - 1) // cb <= 1024)
    stats = {}
    got = jf.entropy_decode_chunked(st, 16, stats=stats)
    assert np.array_equal(got, jf.entropy_decode(st))
    assert stats["chunk_bytes"] == want == 48 and stats["chunks"] == (ln + 47) // 48 <= 1024
    assert stats["rounds"] <= stats["chunks"] and not stats["serial_fallback"]
    assert jf.chunk_bytes_for(100, 17) == 32 and jf.chunk_bytes_for(1024 * 64 + 1, 64) == 80
    for bad in (0, 8, 15, 16.5):
        with pytest.raises(ValueError):
            jf.entropy_decode_chunked(st, bad)


# ----------------------------------------------------------------------------- stuffing at the seams
def _seam_search(wanted):
    """the first noise stream, seeds and qualities in a fixed order, with the wanted bytes at a
    16-byte chunk boundary of its (single) interval"""
    for seed in range(40):
        for q in (95, 96, 97, 98, 99, 100):
            data = sc._pil_save(jc.noise(24, 24, seed=seed), quality=q)
            off, ln = jf.parse(data).intervals[0]
            raw = data[off: off + ln]
            for b in range(16, ln, 16):
                if wanted(raw, b):
                    return data, raw, b
    raise AssertionError("no stream with the wanted seam")


def test_a_chunk_that_starts_on_a_stuffed_zero():
    data, raw, b = _seam_search(lambda raw, b: raw[b - 1] == 0xFF and raw[b] == 0x00)
    assert raw[b - 1] == 0xFF and raw[b] == 0 and b % 16 == 0
    stats = {}
    assert np.array_equal(jf.entropy_decode_chunked(jf.parse(data), 16, stats=stats), jf.entropy_decode(jf.parse(data)))
    assert not stats["serial_fallback"] and stats["chunk_bytes"] == 16


def test_a_chunk_boundary_directly_after_a_stuffed_pair():
    data, raw, b = _seam_search(lambda raw, b: raw[b - 2] == 0xFF and raw[b - 1] == 0x00)
    assert raw[b - 2] == 0xFF and raw[b - 1] == 0 and b % 16 == 0
    stats = {}
    assert np.array_equal(jf.entropy_decode_chunked(jf.parse(data), 16, stats=stats), jf.entropy_decode(jf.parse(data)))
    assert not stats["serial_fallback"] and stats["chunk_bytes"] == 16


# ----------------------------------------------------------------------------- mutations
def test_mutations_give_the_serial_result_or_the_serial_exception():
    """single-bit flips and truncations of the entropy-coded bytes of every stream under 1500
    bytes, fixed seed: the serial result, or the serial exception; nothing but a ValueError"""
    rng = np.random.default_rng(11)
    streams = [s for s in sc.corpus() + sc.batch_streams() if len(s.data) < 1500]
    assert len(streams) > 50
    decoded = refused = 0
    for s in streams:
        st = jf.parse(s.data)
        lo, hi = st.scan_offset, st.intervals[-1][0] + st.intervals[-1][1]
        for k in range(4):
            b = bytearray(s.data)
            if k == 3:                                          # bytes cut out in front of EOI
                cut = int(rng.integers(lo, hi))
                b = b[:cut] + b[hi:]
            else:
                b[int(rng.integers(lo, hi))] ^= 1 << int(rng.integers(0, 8))
            try:
                mst = jf.parse(bytes(b))
            except ValueError:
                continue                                       # a marker appeared or vanished: no stream to decode
            want = _outcome(lambda: jf.entropy_decode(mst))
            got = _outcome(lambda: jf.entropy_decode_chunked(mst, 16))
            assert _same(want, got), (s.name, k, want[0], got)
            decoded += want[0] == "ok"
            refused += want[0] != "ok"
    assert decoded > 20 and refused > 20, (decoded, refused)


# ----------------------------------------------------------------------------- ops.jpeg_decode on the CPU
def test_ops_jpeg_decode_chunked_on_the_cpu_is_the_model():
    s = sc.corpus()[3]
    exp = sc.pil_pixels(s.data)
    info = {}
    out = ops.jpeg_decode(s.data, mode="chunked", chunk_bytes=16, info=info)
    assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and np.array_equal(out.numpy(), exp)
    stats = {}
    jf.entropy_decode_chunked(jf.parse(s.data), 16, stats=stats)
    assert info == {k: stats[k] for k in ("chunks", "rounds", "chunk_bytes", "serial_fallback")}
    batch = [b.data for b in sc.batch_streams()]
    got = ops.jpeg_decode(batch, mode="chunked", info=info)
    for i, b in enumerate(batch):
        assert np.array_equal(got[i].numpy(), sc.pil_pixels(b))
    assert info["chunk_bytes"] == 32 and info["serial_fallback"] is False
    assert np.array_equal(ops.jpeg_decode(s.data, mode="interval").numpy(), exp)
    with pytest.raises(ValueError):
        ops.jpeg_decode(s.data, mode="serial")
    with pytest.raises(ValueError):
        ops.jpeg_decode(s.data, mode="chunked", chunk_bytes=8)
    m = sc.malformed()[0]
    with pytest.raises(jf.JpegError) as e:
        ops.jpeg_decode(m.data, mode="chunked", info=info)
    assert e.value.code == m.code and info["serial_fallback"] is True


# ----------------------------------------------------------------------------- flag, factory
def test_flag_and_factory():
    from cassmantle_amd.runtime.factory import build_jpeg_decode_fn
    d = Config()
    assert d.model.jpeg_decode_chunked is False and d.model.jpeg_decode_chunk_bytes >= 16
    assert d.model.jpeg_decode_chunk_bytes % 16 == 0
    c = Config.from_args(["--gpu_jpeg_decode", "--jpeg_decode_chunked", "--jpeg_decode_chunk_bytes", "64"], base=Config())
    assert c.model.jpeg_decode_chunked is True and c.model.jpeg_decode_chunk_bytes == 64 and c.model.gpu_jpeg_decode
    e = Config.from_env({"CASSMANTLE_JPEG_DECODE_CHUNKED": "1", "CASSMANTLE_JPEG_DECODE_CHUNK_BYTES": "48"})
    assert e.model.jpeg_decode_chunked is True and e.model.jpeg_decode_chunk_bytes == 48
    assert build_jpeg_decode_fn(e, "cuda") is None             # needs gpu_jpeg_decode
    assert build_jpeg_decode_fn(c, "cpu") is None              # flags set, no GPU
    # the flag off: a stream under jpeg_decode_min_intervals is left to PIL, as before
    off = Config.from_args(["--gpu_jpeg_decode"], base=Config())
    fn = build_jpeg_decode_fn(off, "cuda")
    pil = sc._pil_save(jc.gradient(16, 24), quality=75)
    assert len(jf.parse(pil).intervals) == 1 < off.model.jpeg_decode_min_intervals
    assert fn is not None and fn(pil) is None
