"""The implicit-GEMM conv held to the localised oracle in every tile: each live non-areg row of
the tile menu is forced on the conv A loader (kernel_oracle.conv_tile_cases) at shapes with a full
and a partial M tile, an image boundary inside a tile, a full and a partial N tile, at stride 1
and 2, through the parity classes of conv2d_up2, and through split-K plans whose slices start in
the middle of the taps, are shorter than the deep rings or are empty; the static tiles also in
their other A modes (Cin % 8, fused upsample, 1x1) and, in a child process with
``CASSMANTLE_GEMM_BUF=0``, without buffer resources.  Inputs sit in NaN, the output and the
statistics between canaries, the error is per 16 pixels x 16 channels against fp64 of the same
inputs under the conv family's existing bound; every launch must run the plan that was forced.
test_kernel_oracle.py proves the checks on planted conv bugs without a GPU."""
import json
import os
import subprocess
import sys

import pytest

import conv_edge_child as cec
import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.ops._ext import ext_available, ext_error
from kernel_oracle import BOUND
from test_kernel_edges_gpu import MENU, check, check_stats

pytestmark = pytest.mark.gpu

CASES = ko.conv_tile_cases(MENU)
CHILD_TIMEOUT = 180          # seconds: start-up, one code-object load, 56 launches and their checks


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    assert ext_available(), ext_error()
    ops.set_mode("hip")


def group(name):
    return pytest.mark.parametrize("c", [c for c in CASES if c.group == name], ids=lambda c: c.id)


def run_case(c):
    g, st, y64, plan = cec.launch_case(c)
    assert plan == (c.cfg, c.split), (c.id, plan)          # the forced plan ran, not the planner's fallback
    check(g, y64.flatten(0, 2), "conv", c.id)
    if st is not None:
        ko.check_guards(st)
        check_stats(st.view, g.view, y64.shape[0])


@group("plain")
def test_conv_tile_edges(c):
    """3x3, Cin % 64 == 0: every tile at stride 1 and 2 and under the two split-K plans"""
    run_case(c)


@group("up2")
def test_conv_up2_tile_edges(c):
    """the four parity classes with their asymmetric padding; the block error is taken on the
    interleaved output, so one wrong class stands out"""
    run_case(c)


@group("modes")
def test_conv_static_mode_edges(c):
    """the A modes only the static tiles have: per-lane tap decode (Cin % 8), the fused 2x
    upsample, a 1x1 pad-0 conv, and N % 8 != 0 through the plain split-K reduce"""
    run_case(c)


def test_conv_without_buffer_resources():
    """gemm_c2 (global loads, zero page) in a child process with CASSMANTLE_GEMM_BUF=0"""
    cases = cec.child_cases()
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(cec.__file__)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=dict(os.environ, CASSMANTLE_GEMM_BUF="0"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["buf_off"], "the child ran with buffer resources"
    rows = {row["id"]: row for row in rep["cases"]}
    assert sorted(rows) == sorted(c.id for c in cases)
    bad = []
    for c in cases:
        row = rows[c.id]
        print(f"conv (no buffer resources) {c.id}: worst block {row['err']:.3e} (bound {BOUND['conv']:g}) "
              f"plan={row['plan']} stats {row['stats_err']}")
        ok = (tuple(row["plan"]) == (c.cfg, c.split) and row["guards"] and row["err"] < BOUND["conv"] and
              (row["stats_err"] is not None) == c.stats and (row["stats_err"] is None or row["stats_err"] < 1e-4))
        if not ok:
            bad.append(row)
    assert bad == []
