"""Chunked entropy decode contract on the GPU (ops/csrc/jpeg.hip: jpeg_entropy_sync_kernel,
jpeg_dc_prefix_kernel, jpeg_block_check_kernel): ops.jpeg_decode(mode="chunked") equals PIL on the
corpus of jpeg_stream_cases.py at 16 and 64 bytes per chunk without ever falling back to the
interval kernel, takes the rounds and chunks the numpy model takes, handles a batch, ``out=`` and
a non-default stream, the smallest shapes that can still go wrong (1x1, one chunk, 81 intervals,
several workgroups of several intervals, more than 1024 chunks of 16 bytes), refuses every
malformed and over-threshold stream with what mode="interval" raises, and under
``jpeg_decode_chunked`` the factory's function decodes a PIL stream without restart markers."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_stream_cases as sc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.game.content import DeviceImage
from cassmantle_amd.ops import jpeg_format as jf

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _hip_mode():
    ops.set_mode("hip")
    yield


def _named(name):
    return next(s for s in sc.corpus() if s.name == name)


def _check(streams, chunk):
    for s in streams:
        info = {}
        out = ops.jpeg_decode(s.data, device=DEV, mode="chunked", chunk_bytes=chunk, info=info)
        exp = sc.pil_pixels(s.data)
        assert out.device.type == "cuda" and out.dtype == torch.uint8 and tuple(out.shape) == exp.shape, s.name
        got = out.cpu().numpy()
        diff = int(np.count_nonzero(got != exp))
        assert diff == 0, (s.name, chunk, diff, info)
        assert info["serial_fallback"] is False and 1 <= info["rounds"] <= info["chunks"], (s.name, info)


@pytest.mark.parametrize("chunk", [16, 64])
def test_pil_written_streams_equal_pil(chunk):
    _check(sc.pil_streams(), chunk)


@pytest.mark.parametrize("chunk", [16, 64])
def test_in_tree_streams_equal_pil(chunk):
    _check(sc.intree_streams(), chunk)


@pytest.mark.parametrize("name", ["pil_noise_100x75_q75", "pil_gradient_100x75_q75", "pil_noise_100x75_subsampling0",
                                  "pil_noise_100x75_optimize1", "intree_144x144_420_r1"])
def test_rounds_and_chunks_are_the_models(name):
    s = _named(name)
    for chunk in (16, 64):
        info, stats = {}, {}
        ops.jpeg_decode(s.data, device=DEV, mode="chunked", chunk_bytes=chunk, info=info)
        jf.entropy_decode_chunked(jf.parse(s.data), chunk, stats=stats)
        assert info == {k: stats[k] for k in ("chunks", "rounds", "chunk_bytes", "serial_fallback")}, (name, chunk)


def test_batch_out_stream_and_the_models_counts():
    batch = [b.data for b in sc.batch_streams()]
    info = {}
    got = ops.jpeg_decode(batch, device=DEV, mode="chunked", chunk_bytes=16, info=info)
    assert tuple(got.shape) == (3, 24, 40, 3) and got.device.type == "cuda"
    for i, b in enumerate(batch):
        assert np.array_equal(got[i].cpu().numpy(), sc.pil_pixels(b)), i
    stats = [{} for _ in batch]
    for b, st in zip(batch, stats):
        jf.entropy_decode_chunked(jf.parse(b), 16, stats=st)
    assert info == dict(chunks=sum(st["chunks"] for st in stats), rounds=max(st["rounds"] for st in stats),
                        chunk_bytes=16, serial_fallback=False)
    buf = torch.zeros((3, 24, 40, 3), device=DEV, dtype=torch.uint8)
    assert ops.jpeg_decode(batch, out=buf, mode="chunked") is buf and torch.equal(buf, got)
    one = torch.zeros((24, 40, 3), device=DEV, dtype=torch.uint8)
    assert ops.jpeg_decode(jf.parse(batch[1]), device=DEV, out=one, mode="chunked") is one and torch.equal(one, got[1])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.jpeg_decode(batch, device=DEV, mode="chunked", chunk_bytes=48)
    side.synchronize()
    assert torch.equal(other, got)
    with pytest.raises(ValueError):
        ops.jpeg_decode(batch, device=DEV, mode="parallel")
    with pytest.raises(ValueError):
        ops.jpeg_decode(batch, device=DEV, mode="chunked", chunk_bytes=15)


def test_smallest_shapes_that_can_go_wrong():
    # 1 x 1, and a stream of one chunk: one lane, one round
    for name in ("pil_noise_1x1_q75", "pil_gradient_8x8_q10"):
        s = _named(name)
        info = {}
        out = ops.jpeg_decode(s.data, device=DEV, mode="chunked", chunk_bytes=64, info=info)
        assert np.array_equal(out.cpu().numpy(), sc.pil_pixels(s.data)), name
        assert jf.parse(s.data).intervals[0][1] <= 64
        assert info == dict(chunks=1, rounds=1, chunk_bytes=64, serial_fallback=False), (name, info)
    # 81 intervals in one workgroup (813 lanes at 16 bytes, every interval its own chain)
    s = _named("intree_144x144_420_r1")
    st = jf.parse(s.data)
    assert len(st.intervals) == 81
    _check([s], 16)
    # the same image at quality 95: its 81 intervals no longer fit 1024 lanes, so several
    # workgroups of several intervals each
    data = jf.jpeg_encode(jc.noise(144, 144, seed=144), 95, "420", 1)[0]
    st = jf.parse(data)
    lens = np.asarray([[ln for _, ln in st.intervals]], dtype=np.int64)
    _, groups, _, chunks = ops._jpeg_chunk_groups(lens, 16)
    assert len(groups) > 1 and chunks > 1024 and int(groups[:, 1].min()) > 1 and int(groups[:, 1].sum()) == 81
    _check([sc.Stream("intree_144x144_420_r1_q95", data)], 16)
    # one interval of more than 1024 chunks of 16 bytes: the chunk grows
    data = sc._pil_save(jc.noise(256, 256, seed=1), quality=75)
    ln = jf.parse(data).intervals[0][1]
    assert ln > 16 * 1024
    info, stats = {}, {}
    out = ops.jpeg_decode(data, device=DEV, mode="chunked", chunk_bytes=16, info=info)
    assert np.array_equal(out.cpu().numpy(), sc.pil_pixels(data))
    jf.entropy_decode_chunked(jf.parse(data), 16, stats=stats)
    assert info["chunk_bytes"] == jf.chunk_bytes_for(ln, 16) > 16 and info["chunks"] <= 1024
    assert info == {k: stats[k] for k in ("chunks", "rounds", "chunk_bytes", "serial_fallback")}


def test_refusals_are_those_of_the_interval_mode():
    cases = [(m.name, m.data) for m in sc.malformed()]
    cases += [(n, d) for n, d, t in sc.energy_streams() if t > jf.WIDE_T]
    c = np.zeros((4, 3, 64), dtype=np.int16)
    c[:, 0, 0] = 5
    c[2, 1, 1] = 1023                                          # a block over the threshold in interval 2
    cases.append(("wide_in_interval_2", sc.craft(c, 50, 16, 16, "444", restart=1)))
    assert len(cases) >= 14
    for name, data in cases:
        with pytest.raises(ValueError) as want:
            ops.jpeg_decode(data, device=DEV)
        for chunk in (16, 64):
            info = {}
            with pytest.raises(ValueError) as got:
                ops.jpeg_decode(data, device=DEV, mode="chunked", chunk_bytes=chunk, info=info)
            assert type(got.value) is type(want.value), name
            assert (got.value.code, got.value.interval) == (want.value.code, want.value.interval), name
            assert info["serial_fallback"] is True, name
    for name, data, target in sc.energy_streams():             # at the threshold: PIL's pixels, no fallback
        if target <= jf.WIDE_T:
            info = {}
            out = ops.jpeg_decode(data, device=DEV, mode="chunked", chunk_bytes=16, info=info)
            assert np.array_equal(out.cpu().numpy(), sc.pil_pixels(data)) and not info["serial_fallback"], name
    # the lowest failing interval of a batch, and a good call after a refused one
    good = jf.jpeg_encode(jc.noise(17, 33, seed=50), 75, "420", 2)[0]
    bad = sc.malformed()[0].data
    with pytest.raises(jf.JpegError) as e:
        ops.jpeg_decode([good, bad, bad], device=DEV, mode="chunked")
    assert (e.value.code, e.value.interval) == (jf.TRUNCATED, 3 + 2)
    assert np.array_equal(ops.jpeg_decode(good, device=DEV, mode="chunked").cpu().numpy(), sc.pil_pixels(good))


def test_decode_fn_decodes_a_stream_without_restart_markers():
    from cassmantle_amd.runtime.factory import build_jpeg_decode_fn
    cfg = Config.from_args(["--gpu_jpeg_decode", "--jpeg_decode_chunked"], base=Config())
    fn = build_jpeg_decode_fn(cfg, DEV)
    s = _named("pil_noise_48x40_q75")
    assert len(jf.parse(s.data).intervals) == 1 < cfg.model.jpeg_decode_min_intervals
    img = fn(s.data)
    assert isinstance(img, DeviceImage) and img.tensor.device.type == "cuda" and img._host is None
    assert np.array_equal(img.tensor.cpu().numpy(), sc.pil_pixels(s.data))
    assert fn(sc.malformed()[2].data) is None and fn(b"not a jpeg") is None        # refused: left to PIL
    cfg.model.jpeg_decode_chunked = False
    assert build_jpeg_decode_fn(cfg, DEV)(s.data) is None                          # the flag off: as before
    cfg.model.jpeg_decode_chunked, cfg.model.jpeg_decode_min_intervals = True, 2
    many = _named("intree_144x144_420_r1")                      # enough intervals: the interval path as today
    assert np.array_equal(build_jpeg_decode_fn(cfg, DEV)(many.data).tensor.cpu().numpy(), sc.pil_pixels(many.data))
