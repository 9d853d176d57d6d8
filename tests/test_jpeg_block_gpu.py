"""The block-parallel entropy coder (ops.jpeg_encode(entropy="block"), ops/csrc/jpeg.hip) on the
GPU: byte-exact against the numpy reference for every restart interval, none included; an interval
longer than one scan tile; the round trip of a restart-less stream through PIL and the chunked
decoder; input forms and the current-stream rule; and the serving functions with
``jpeg_entropy=block`` / ``jpeg_restart_mcus=-1``, whose defaults still give the interval coder's
bytes."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from cassmantle_amd import ops
from cassmantle_amd.config import Config
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _hip_mode():
    ops.set_mode("hip")
    yield


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
@pytest.mark.parametrize("quality", jc.QUALITIES)
def test_byte_exact_against_reference(quality, sampling):
    """every hard-case input x restart_mcus {0, 1, 2, 5, one MCU row}, batch 1"""
    for name, img in jc.hard_cases().items():
        H, W, _ = img.shape
        t = torch.from_numpy(img).to(DEV)
        for r in jc.restart_values(H, W, sampling, with_zero=True):
            got = ops.jpeg_encode(t, quality, sampling, r, entropy="block")
            exp = ref.jpeg_encode(img, quality, sampling, r)
            assert len(got) == 1 and got[0] == exp[0], (name, quality, sampling, r, len(got[0]), len(exp[0]))


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
def test_byte_exact_batch_of_three_mixed(sampling):
    """three different images in one call: the batch scan and the image offsets"""
    batch = np.stack([jc.black_white_blocks(24, 40), jc.noise(24, 40), jc.flat(24, 40)])
    t = torch.from_numpy(batch).to(DEV)
    for q in jc.QUALITIES:
        for r in jc.restart_values(24, 40, sampling, with_zero=True):
            got = ops.jpeg_encode(t, q, sampling, r, entropy="block")
            exp = ref.jpeg_encode(batch, q, sampling, r)
            assert len(got) == 3 and len({len(g) for g in got}) > 1      # offsets are not uniform
            assert got == exp, (q, sampling, r, [len(g) for g in got], [len(e) for e in exp])


def test_interval_longer_than_a_scan_tile():
    """224x224 at 4:2:0 without restart markers: 1176 blocks in one interval, more than the 1024
    lanes of a scan tile; at quality 95 its bytes are more than the 1024 pieces of a stuffing tile"""
    img = jc.noise(224, 224)
    _, nb, mx, my = jf.geometry(224, 224, "420")
    assert mx * my * nb == 1176 > 1024
    got = ops.jpeg_encode(torch.from_numpy(img).to(DEV), 95, "420", 0, entropy="block")
    exp = ref.jpeg_encode(img, 95, "420", 0)
    assert len(exp[0]) > 1024 * jf.BLK_STUFF_CHUNK
    assert got == exp, (len(got[0]), len(exp[0]))


def test_restart_zero_round_trip():
    """no DRI in the header, PIL decodes the bytes to the returned pixels, and so does the chunked
    decoder on the device"""
    img = jc.hard_cases()["noise_64x48"]
    outs, decoded = ops.jpeg_encode(torch.from_numpy(img).to(DEV), 75, "420", 0, return_decoded=True, entropy="block")
    assert outs == ref.jpeg_encode(img, 75, "420", 0)
    st = jf.parse(outs[0])
    assert st.restart == 0 and len(st.intervals) == 1 and b"\xff\xdd" not in outs[0]
    pil = jc.decode(outs[0])
    assert np.array_equal(decoded[0].cpu().numpy(), pil)
    back = ops.jpeg_decode(outs[0], device=DEV, mode="chunked")
    assert np.array_equal(back.cpu().numpy(), pil)


def test_input_forms_and_stream():
    """a non-contiguous view, a DeviceImage and a call on a side stream give the plain call's bytes"""
    from cassmantle_amd.game.content import DeviceImage
    img = jc.hard_cases()["noise_64x48"]
    plain = ops.jpeg_encode(torch.from_numpy(img).to(DEV), 75, "420", 0, entropy="block")
    assert plain == ref.jpeg_encode(img, 75, "420", 0)
    wide = torch.from_numpy(np.concatenate([img, 255 - img], axis=1)).to(DEV)      # [64, 96, 3]
    view = wide[:, :48]
    assert not view.is_contiguous()
    assert ops.jpeg_encode(view, 75, "420", 0, entropy="block") == plain
    assert ops.jpeg_encode(DeviceImage(view.contiguous()), 75, "420", 0, entropy="block") == plain
    s = torch.cuda.Stream()
    host = torch.from_numpy(img).pin_memory()
    with torch.cuda.stream(s):
        t = host.to(DEV, non_blocking=True)           # ordered before the encode only on s
        got = ops.jpeg_encode(t, 75, "420", 0, entropy="block")
    assert got == plain


def _serving_cfg(block: bool) -> Config:
    cfg = Config()
    cfg.model.gpu_jpeg = cfg.model.gpu_jpeg_content = True
    cfg.model.blur_kernel = "pil"
    if block:
        cfg.model.jpeg_entropy = "block"
        cfg.model.jpeg_restart_mcus = -1
    return cfg


def test_serving_without_restart_markers():
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn, build_content_jpeg_fn
    cfg = _serving_cfg(block=True)
    img = jc.noise(64, 64)
    x = torch.from_numpy(img).to(DEV)
    radii = [0.25, 2.0, 15.0]
    outs = build_blur_jpeg_fn(cfg, DEV)(img, radii, 75)
    blurred = ops.gaussian_blur_pil(x, radii).cpu().numpy()
    assert outs == ref.jpeg_encode(blurred, 75, "420", 0)
    for data in outs:
        assert b"\xff\xdd" not in data and jc.decode(data).shape == (64, 64, 3)
    data, dimg = build_content_jpeg_fn(cfg, DEV)(DeviceImage(x), 75)
    assert data == ref.jpeg_encode(img, 75, "420", 0)[0] and jf.parse(data).restart == 0
    assert np.array_equal(dimg.tensor.cpu().numpy(), jc.decode(data))


def test_serving_defaults_are_the_interval_coder():
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.runtime.factory import build_blur_jpeg_fn, build_content_jpeg_fn
    cfg = _serving_cfg(block=False)
    img = jc.noise(64, 64)
    x = torch.from_numpy(img).to(DEV)
    radii = [0.25, 2.0]
    row = 64 // 16                                                  # one MCU row
    outs = build_blur_jpeg_fn(cfg, DEV)(img, radii, 75)
    assert outs == ops.jpeg_encode(ops.gaussian_blur_pil(x, radii), 75, "420", row, entropy="interval")
    data, _ = build_content_jpeg_fn(cfg, DEV)(DeviceImage(x), 75)
    assert data == ops.jpeg_encode(x, 75, "420", row, entropy="interval")[0]
    assert jf.parse(data).restart == row


@pytest.mark.parametrize("H,W", [(8, 8), (24, 40)])
def test_bindings_take_the_layout_and_refuse_anything_else(H, W):
    """ext().jpeg_count / jpeg_write directly, three images: with buffers sized by
    ext().jpeg_encode_layout every coder / table combination writes the reference's bytes; a work
    buffer one word short, half of an optional pair, a split without optimised tables and an out of
    the wrong length are refused on the host, before anything is launched"""
    from cassmantle_amd.ops._ext import ext
    B, restart = 3, 2
    batch = np.stack([jc.noise(H, W), jc.flat(H, W), jc.black_white_blocks(H, W)])
    t = torch.from_numpy(batch).to(DEV)

    def call(blocks, optimized):
        tables, header, split = ops._jpeg_plan(t.device, H, W, 75, "420", restart, "compact", optimized)
        lay = ext().jpeg_encode_layout(B, H, W, True, restart, blocks, optimized, False, header.numel())

        def buf(name, dtype=torch.int32):
            return torch.empty(lay[name], device=DEV, dtype=dtype)
        blk, scratch = (buf("blk"), buf("scratch")) if blocks else (None, None)
        hopt, hdrs = (buf("hopt"), buf("hdrs", torch.uint8)) if optimized else (None, None)
        return lay, [t, tables, header, buf("coef", torch.int16), buf("work"), 1, restart, 0, blk, scratch, hopt, hdrs,
                     split]

    def replaced(args, **kw):
        names = ["images", "tables", "header", "coef", "work", "s420", "restart", "lj", "blk", "scratch", "hopt", "hdrs",
                 "split"]
        return [kw.get(n, a) for n, a in zip(names, args)]

    for blocks in (False, True):
        for optimized in (False, True):
            lay, args = call(blocks, optimized)
            assert lay["lens"] == lay["prefix"] and lay["work"] == lay["prefix"] + 2 * B * lay["nint"]
            with pytest.raises(RuntimeError):
                ext().jpeg_count(*replaced(args, work=args[4][:-1]))
            if blocks:
                with pytest.raises(RuntimeError):
                    ext().jpeg_count(*replaced(args, scratch=None))
            if optimized:
                with pytest.raises(RuntimeError):
                    ext().jpeg_count(*replaced(args, hdrs=None))
                with pytest.raises(RuntimeError):
                    ext().jpeg_count(*replaced(args, hopt=None, hdrs=None))          # split stays
            ext().jpeg_count(*args)
            head = args[4][: lay["prefix"]].cpu().tolist()
            total = head[B]
            for wrong in (total + lay["slack"] - 1, total + lay["slack"] + 1):
                with pytest.raises(RuntimeError):
                    ext().jpeg_write(*args, torch.empty(wrong, device=DEV, dtype=torch.uint8), total)
            out = torch.empty(total + lay["slack"], device=DEV, dtype=torch.uint8)
            ext().jpeg_write(*args, out, total)
            host = out.cpu().numpy().tobytes()
            assert not (blocks and (head[lay["err"]] or host[-1]))
            got = [host[head[i]: head[i + 1]] for i in range(B)]
            exp = ref.jpeg_encode(batch, 75, "420", restart, huffman="optimized" if optimized else "standard")
            assert got == exp, (blocks, optimized, [len(g) for g in got], [len(e) for e in exp])
