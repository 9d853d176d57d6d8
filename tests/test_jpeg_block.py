"""The block-parallel entropy coder on the CPU: its numpy model (jpeg_format.entropy_blocks: bit
lengths, offsets, pack, stuff) writes the bytes of jpeg_format.entropy for every restart interval,
none included; the model's statistics show that the test images reach the places where the kernel
can go wrong; the bits-per-block bound follows from the Huffman tables and a crafted block comes
within 2 bits of it; and the factory's restart rule (runtime.factory.jpeg_restart)."""
from __future__ import annotations

import os
import re

import pytest

import jpeg_cases as jc
from cassmantle_amd.config import Config
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.runtime.factory import jpeg_restart
from test_jpeg_block_native import worst_block

CHUNKS = (jf.BLK_STUFF_CHUNK, 5)          # the kernel's piece and one that is no multiple of anything
CSRC = os.path.join(jc.ROOT, "cassmantle_amd", "ops", "csrc")


def images():
    out = dict(jc.hard_cases())
    out["noise_24x40"] = jc.noise(24, 40)
    out["flat_24x40"] = jc.flat(24, 40)
    out["noise_1x1"] = jc.noise(1, 1)
    return out


def _settings(img):
    H, W, _ = img.shape
    for q in jc.QUALITIES:
        for s in jc.SAMPLINGS:
            coef = jf.coefficients(img, q, s)
            # every restart value of the interval coder's tests, none, and one past the MCU count
            for r in jc.restart_values(H, W, s, with_zero=True) + [coef.shape[0] + 3]:
                yield q, s, coef, r


@pytest.fixture(scope="module")
def coverage():
    """name -> the model's statistics at the kernel's piece size, summed (min / max where they are
    extremes) over q x sampling x restart; the byte equality is asserted on the way."""
    agg = {}
    for name, img in images().items():
        a = agg[name] = {"zrl": 0}
        for q, s, coef, r in _settings(img):
            exp = jf.entropy(coef, r)
            for chunk in CHUNKS:
                st = {}
                got = jf.entropy_blocks(coef, r, stuff_chunk=chunk, stats=st)
                assert got[0] == exp[0], (name, q, s, r, chunk)
                assert got[1] == exp[1], (name, q, s, r, chunk)
                if chunk != jf.BLK_STUFF_CHUNK:
                    continue
                a["zrl"] += got[1]["zrl"]
                for k, v in st.items():
                    if k == "min_bits":
                        a[k] = min(a.get(k, v), v)
                    elif k.startswith("max_"):
                        a[k] = max(a.get(k, v), v)
                    else:
                        a[k] = a.get(k, 0) + v
    return agg


def test_model_writes_the_reference_bytes(coverage):
    assert set(coverage) == set(images())


def test_inputs_reach_the_hard_places(coverage):
    flat, noise, small = coverage["flat_17x33"], coverage["noise_64x48"], coverage["noise_24x40"]
    assert flat["min_bits"] == 4 and flat["max_starts_per_word"] == 7        # 7 blocks merge into one word
    assert noise["ff_two_blocks"] > 0            # a 0xFF byte that exists only after two lanes' merges
    assert noise["ff_interval_end"] > 0          # the padding completes a 0xFF: stuffed zero, then the marker
    assert noise["ff_piece_end"] > 0             # the stuffed zero of a piece's last byte stays in that piece
    assert small["ff_pairs"] > 0                 # two stuffed zeros in a row
    assert coverage["highfreq_16x16"]["zrl"] > 0
    assert all(c["max_bits"] <= jf.block_bits_bound() for c in coverage.values())


def test_bits_per_block_bound():
    h = jf.huff_table()
    dc = max(int(v) >> 16 for v in h[:32])
    ac = max(int(v) >> 16 for v in h[32:])
    bound = dc + 11 + 63 * (ac + 10)
    assert (dc, ac) == (11, 16) and bound == jf.block_bits_bound() == 1660
    src = open(os.path.join(CSRC, "jpeg_entropy_blk.h")).read()
    m = re.search(r"JPEG_BLK_MAX_BITS = (\d+) \+ (\d+) \+ (\d+) \* \((\d+) \+ (\d+)\)", src)
    assert m and [int(g) for g in m.groups()] == [dc, 11, 63, ac, 10]
    assert int(re.search(r"JPEG_BLK_PIECE = (\d+)", src).group(1)) == jf.BLK_STUFF_CHUNK
    coef = worst_block()
    st = {}
    got = jf.entropy_blocks(coef, 0, stats=st)
    assert got == jf.entropy(coef, 0) and got[1]["max_dc_cat"] == 11
    # the luma DC table's longest code is 9 bits (the 11 is the chroma table's), and the chroma AC
    # table codes (0, 10) in 12 bits: no block comes closer to the bound than this one, 2 under it
    assert st["max_bits"] == bound - 2
    assert st["max_bits"] == 9 + 11 + 63 * 26


def test_factory_restart_rule():
    cfg = Config()
    assert cfg.model.jpeg_entropy == "interval" and cfg.model.jpeg_restart_mcus == 0
    assert jpeg_restart(cfg, 512) == (32, "interval")            # 0: one MCU row
    assert jpeg_restart(cfg, 33) == (3, "interval")
    cfg.model.jpeg_restart_mcus = 4
    assert jpeg_restart(cfg, 512) == (4, "interval")
    cfg.model.jpeg_entropy = "block"
    assert jpeg_restart(cfg, 512) == (4, "block")
    cfg.model.jpeg_restart_mcus = 0
    assert jpeg_restart(cfg, 512) == (32, "block")
    cfg.model.jpeg_restart_mcus = -1
    assert jpeg_restart(cfg, 512) == (0, "block")                # no restart markers
    cfg.model.jpeg_entropy = "interval"
    with pytest.raises(ValueError):
        jpeg_restart(cfg, 512)
    cfg.model.jpeg_restart_mcus = 0
    cfg.model.jpeg_entropy = "blocks"
    with pytest.raises(ValueError):
        jpeg_restart(cfg, 512)


def test_factory_raises_when_the_function_is_built():
    """like blur_kernel(): a bad value is an error of the build call, on any device"""
    from cassmantle_amd.runtime import factory
    cfg = Config()
    cfg.model.gpu_jpeg = cfg.model.gpu_jpeg_content = True
    cfg.model.jpeg_restart_mcus = -1
    for build in (factory.build_blur_jpeg_fn, factory.build_content_jpeg_fn):
        with pytest.raises(ValueError):
            build(cfg, "cuda")
    cfg.model.blur_kernel = "pil"
    with pytest.raises(ValueError):
        factory.build_blur_jpeg_fn(cfg, "cuda")


def test_flag_and_environment_spelling():
    cfg = Config.from_args(["--gpu_jpeg", "--jpeg_entropy", "block", "--jpeg_restart_mcus", "-1"], base=Config())
    assert cfg.model.jpeg_entropy == "block" and cfg.model.jpeg_restart_mcus == -1 and cfg.model.gpu_jpeg
    assert jpeg_restart(cfg, 64) == (0, "block")
    cfg = Config.from_args(["--jpeg-entropy=block", "--jpeg_restart_mcus=-1"], base=Config())
    assert (cfg.model.jpeg_entropy, cfg.model.jpeg_restart_mcus) == ("block", -1)
    env = Config.from_env({"CASSMANTLE_JPEG_ENTROPY": "block", "CASSMANTLE_JPEG_RESTART_MCUS": "-1"})
    assert (env.model.jpeg_entropy, env.model.jpeg_restart_mcus) == ("block", -1)


def test_entropy_argument_is_checked_before_the_route():
    from cassmantle_amd import ops
    img = jc.gradient(8, 8)
    with pytest.raises(ValueError):
        ops.jpeg_encode(img, entropy="lane")
    assert ops.jpeg_encode(img, 75, "420", 0, entropy="block") == jf.jpeg_encode(img, 75, "420", 0)
