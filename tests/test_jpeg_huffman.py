"""Optimised Huffman tables, the numpy model (jpeg_format.symbol_counts / optimal_table and the
``tables=`` / ``huffman=`` arguments): PIL's ``optimize=True`` streams are the oracle for the
tables and the bytes; tables with one symbol and with none; the same pixels in fewer bytes on the
encoder's cases; both coders' bytes; refusals, bounds and the configuration's spelling.  Nothing
runs on a GPU."""
from __future__ import annotations

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_huffman_cases as hc
from cassmantle_amd.config import Config
from cassmantle_amd.ops import jpeg_format as jf
from cassmantle_amd.ops import reference as ref

OPT = "optimized"


def _cases():
    """(name, image, quality, sampling, restart) over every case and restart interval of jpeg_cases"""
    for name, img in jc.hard_cases().items():
        H, W, _ = img.shape
        for q in jc.QUALITIES:
            for s in jc.SAMPLINGS:
                for r in jc.restart_values(H, W, s, with_zero=True):
                    yield name, img, q, s, r


def test_pil_oracle_tables_and_bytes():
    """optimal_table(symbol_counts) is the DHT PIL wrote, and entropy() with those tables writes
    PIL's entropy-coded bytes: 6 images x 4 qualities x 2 samplings + the two skewed images"""
    items = hc.oracle()
    assert len(items) == 6 * 4 * 2 + 2
    for name, st, coef in items:
        tables = jf.optimal_tables(jf.symbol_counts(coef, 0))
        assert tables == st.huff, name
        scan, _ = jf.entropy(coef, 0, tables=tables)
        assert scan == st.data[st.scan_offset: -2], name
        assert jf.dht_segment(tables) in st.data or st.data.count(b"\xff\xc4") > 1, name


def test_length_limit_is_reached():
    """the skewed images' chroma AC tables have codes of 17 bits or more before step 5, and the
    model still equals PIL's table (asserted above): the limit is tested, not assumed"""
    longest = {}
    for name, st, coef in hc.oracle():
        if name.startswith("skewed"):
            freq = jf.symbol_counts(coef, 0)
            longest[name] = [max(jf.code_sizes(row)) for row in freq]
            assert st.huff[3][0][15] > 0                    # PIL's table: limited to 16, and reaching it
    print(longest)
    assert longest["skewed_2"][3] >= 17, longest
    assert longest["skewed_3"][3] >= 17, longest


def test_symbol_counts_are_what_the_coder_emits():
    """the vectorised counts equal a plain walk over the blocks in the coder's order, restart
    intervals (their DC resets) included"""
    img = jc.noise(24, 40)
    for s in jc.SAMPLINGS:
        coef = jf.coefficients(img, 75, s)
        for r in (0, 1, 5):
            freq = jf.symbol_counts(coef, r)
            walk = np.zeros((4, 257), dtype=np.int64)
            pred = jf.dc_predictors(coef, r)
            nb = coef.shape[1]
            for m in range(coef.shape[0]):
                for b in range(nb):
                    c = 0 if b < nb - 2 else 1
                    walk[c, abs(int(coef[m, b, 0]) - int(pred[m, b])).bit_length()] += 1
                    run = 0
                    for v in coef[m, b, 1:].tolist():
                        if v == 0:
                            run += 1
                            continue
                        walk[2 + c, 0xF0] += run >> 4
                        walk[2 + c, ((run & 15) << 4) | abs(v).bit_length()] += 1
                        run = 0
                    walk[2 + c, 0] += run > 0
            assert np.array_equal(freq, walk), (s, r)


def test_tables_with_one_symbol_and_with_none():
    """One symbol: the flat image's AC tables hold EOB alone, and crafted coefficients give a luma
    AC table that holds (0, 1) alone and no EOB; PIL and the reference decoder decode both streams
    to the same pixels.  No symbol: zero counts give the empty table (17 bytes of DHT, no code
    word).  A scan cannot own one, since every block codes a DC symbol and at least one AC symbol
    of its component's tables, so beyond the table itself there is no stream to decode."""
    flat = jc.flat(16, 16)
    data = jf.jpeg_encode(flat, 75, "444", 0, huffman=OPT)[0]
    st = jf.parse(data)
    one = (1,) + (0,) * 15
    assert st.huff[2] == (one, (0,)) and st.huff[3] == (one, (0,))
    assert np.array_equal(jc.decode(data), ref.jpeg_decode(data))
    assert np.array_equal(jc.decode(data), jc.decode(jf.jpeg_encode(flat, 75, "444", 0)[0]))
    coef = np.zeros((1, 3, 64), dtype=np.int16)
    coef[0, :, 0] = (3, -2, 1)
    coef[0, 0, 1:] = 1                                 # luma: 63 x (0, 1), no EOB
    coef[0, 1:, 63] = 1                                # chroma: ZRL x 3, then (14, 1), no EOB
    freq = jf.symbol_counts(coef, 0)
    assert freq[2, 0] == 0 and freq[3, 0] == 0 and freq[3, 0xF0] == 6
    tables = jf.optimal_tables(freq)
    assert tables[2] == (one, (0x01,))
    body, _ = jf.entropy(coef, 0, tables=tables)
    data = jf.header(8, 8, 75, "444", 0, tables) + body + b"\xff\xd9"
    assert np.array_equal(jc.decode(data), ref.jpeg_decode(data))
    assert np.array_equal(jf.entropy_decode(jf.parse(data)), coef)
    empty = ((0,) * 16, ())
    assert jf.optimal_table(np.zeros(257, dtype=np.int64)) == empty
    assert len(jf.dht_segment((empty,) * 4)) == 4 + 4 * 17
    assert not jf.huff_table((empty,) * 4).any()


def test_same_pixels_and_strictly_shorter():
    """every case and restart interval of jpeg_cases: the optimised stream decodes in PIL to the
    standard stream's pixels and is strictly shorter"""
    n = 0
    for name, img, q, s, r in _cases():
        std = jf.jpeg_encode(img, q, s, r)[0]
        opt = jf.jpeg_encode(img, q, s, r, huffman=OPT)[0]
        assert np.array_equal(jc.decode(opt), jc.decode(std)), (name, q, s, r)
        assert len(opt) < len(std), (name, q, s, r, len(opt), len(std))
        assert jf.parse(opt).restart == r
        n += 1
    assert n >= 5 * 3 * 2 * 4


def test_both_coders_write_the_same_bytes():
    for name, img, q, s, r in _cases():
        if q != 75:
            continue
        coef = jf.coefficients(img, q, s)
        tables = jf.optimal_tables(jf.symbol_counts(coef, r))
        assert jf.entropy_blocks(coef, r, tables=tables)[0] == jf.entropy(coef, r, tables=tables)[0], (name, s, r)


def test_default_bytes_are_unchanged():
    img = jc.noise(24, 40)
    assert jf.jpeg_encode(img, 75, "420", 2, huffman="standard") == jf.jpeg_encode(img, 75, "420", 2)
    assert jf.header(24, 40, 75, "420", 2) == jf.header(24, 40, 75, "420", 2, tables=jf.STANDARD_TABLES)
    assert np.array_equal(jf.huff_table(), jf.huff_table(jf.STANDARD_TABLES))
    assert jf.block_bits_bound() == 1660


def test_refusals():
    with pytest.raises(ValueError):
        jf.jpeg_encode(jc.noise(8, 8), huffman="optimised")
    from cassmantle_amd import ops
    with pytest.raises(ValueError):
        ops.jpeg_encode(jc.noise(8, 8), huffman="best")
    assert ops.jpeg_encode(jc.noise(8, 8), huffman=OPT) == jf.jpeg_encode(jc.noise(8, 8), huffman=OPT)
    # counts are 32-bit: blocks * 64 >= 2^31 is refused from the shape alone (nothing is allocated)
    huge = np.broadcast_to(np.zeros((1, 1, 1, 1), dtype=np.uint8), (1, 30000, 30000, 3))
    with pytest.raises(ValueError, match="2\\^31"):
        jf.jpeg_encode(huge, 75, "444", 0, huffman=OPT)
    coef = np.broadcast_to(np.zeros((1, 1, 1), dtype=np.int16), (1 << 24, 3, 64))
    with pytest.raises(ValueError, match="2\\^31"):
        jf.symbol_counts(coef, 0)
    jf.check_count_range((1 << 25) - 1)
    with pytest.raises(ValueError):
        jf.check_count_range(1 << 25)
    # a code longer than 32 bits (Fibonacci counts) is refused, as libjpeg refuses it
    fib = [1, 2]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    with pytest.raises(ValueError, match="32 bits"):
        jf.optimal_table(fib)


def test_block_bound_with_own_tables():
    """a crafted block reaches 16 + 11 + 63 * 26 = 1665 bits: a DC code and every AC code 16 bits long"""
    assert jf.block_bits_bound_optimized() == 1665

    def long_table(sym):                 # a complete-but-one canonical table whose `sym` has a 16-bit code
        others = [v for v in range(1, 17) if v != sym][:15]
        return (tuple([1] * 15 + [1]), tuple(others + [sym]))
    dc = long_table(11)
    ac = long_table(0x0A)
    coef = np.zeros((1, 3, 64), dtype=np.int16)
    coef[0, 0, 0] = -2047
    coef[0, 0, 1:] = np.where(np.arange(63) % 2, 1023, -512)
    huff = jf.huff_table((dc, dc, ac, ac))
    assert huff[11] >> 16 == 16 and huff[32 + 0x0A] >> 16 == 16
    _, n = jf._block_code(coef[0, 0].tolist(), 0, True, huff, {"max_dc_cat": 0, "zrl": 0})
    assert n == 1665 == jf.block_bits_bound_optimized()


def test_flag_environment_and_factory_spelling():
    from cassmantle_amd.runtime import factory
    d = Config()
    assert d.model.jpeg_huffman == "standard"
    assert factory._jpeg_encode_args(d, 64) == {"restart_mcus": 4}            # today's keyword dictionary
    c = Config.from_args(["--jpeg_huffman", "optimized", "--gpu_jpeg"], base=Config())
    assert c.model.jpeg_huffman == "optimized"
    assert Config.from_args(["--jpeg-huffman=optimized"], base=Config()).model.jpeg_huffman == "optimized"
    assert Config.from_env({"CASSMANTLE_JPEG_HUFFMAN": "optimized"}).model.jpeg_huffman == "optimized"
    assert factory._jpeg_encode_args(c, 64) == {"restart_mcus": 4, "huffman": "optimized"}
    c.model.jpeg_entropy, c.model.jpeg_restart_mcus = "block", -1
    assert factory._jpeg_encode_args(c, 64) == {"restart_mcus": 0, "entropy": "block", "huffman": "optimized"}
    bad = Config()
    bad.model.gpu_jpeg = bad.model.gpu_jpeg_content = True
    bad.model.jpeg_huffman = "optimised"
    with pytest.raises(ValueError, match="jpeg_huffman"):
        factory.build_blur_jpeg_fn(bad, "cuda")
    with pytest.raises(ValueError, match="jpeg_huffman"):
        factory.build_content_jpeg_fn(bad, "cuda")
    with pytest.raises(ValueError, match="jpeg_huffman"):
        factory.jpeg_huffman(bad)
