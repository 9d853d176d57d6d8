"""The GEMM tile menu (ops/csrc/gemm_tiles.h) against everything that speaks in its ids (CPU).

* the rows, read out of the header with one regex, are strictly ascending (the cost model's
  first-wins tie-break walks them in that order) and agree with the literal ``PP_CFGS`` of
  tests/test_kernels_gpu.py, with every entry of ops/gemm_tuning.json, and -- where the extension
  imports -- with the ``gemm_tile_menu()`` binding;
* the planner golden: tests/native/planner_dump.cpp (linked like planner_sanitize.cpp, launchers
  stubbed, nothing touches a GPU) prints the plan of every call class under the cost model, every
  forced index and every table index; its output must equal tests/golden/planner_plans.txt, which
  was printed by the same driver built against the sources before the menu became a table;
* the route golden: tests/native/route_dump.cpp prints ``gemm_route`` of the same classes and of the
  edges between the kernels and passes; tests/golden/gemm_routes.txt was printed from the decisions
  of the commit before ``gemm_route`` existed (its launch dispatch and binding, instrumented)."""
import ast
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cassmantle_amd", "ops", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
FAMILY = {"kTileStatic": "static", "kTilePingPong": "pingpong", "kTileDeep": "deep", "kTileAreg": "areg"}
ROW = re.compile(r"^\s*\{\s*(\d+),\s*(kTile\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),"
                 r"\s*(true|false),\s*[\d.]+f,\s*\d+\},", re.M)


def header_rows():
    """-> [(id, family, BM, BN, "WMxWN", stages, producers, gated)] as gemm_tile_menu() returns them"""
    src = open(os.path.join(CSRC, "gemm_tiles.h")).read()
    rows = []
    for m in ROW.finditer(src):
        i, fam, bm, bn, wm, wn, st, np_, gwm, gwn, _ = m.groups()
        rows.append((int(i), FAMILY[fam], int(bm), int(bn), f"{wm}x{wn}", int(st), int(np_), int(gwm) != 0))
    body = src[src.index("kGemmTiles[] = {") + 16:]
    assert len(rows) == len(re.findall(r"^\s*\{", body[:body.index("};")], re.M))   # the regex took every row
    return rows


def test_ids_strictly_ascending():
    ids = [r[0] for r in header_rows()]
    assert len(ids) > 0 and all(a < b for a, b in zip(ids, ids[1:]))


def test_pp_cfgs_literal_is_the_ping_pong_and_deep_ring_rows():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_kernels_gpu.py")).read())
    lit = [ast.literal_eval(n.value) for n in tree.body
           if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "PP_CFGS"]
    assert len(lit) == 1
    assert lit[0] == [r[0] for r in header_rows() if r[1] in ("pingpong", "deep")]


def test_tuning_table_names_live_ids_only():
    live = {r[0] for r in header_rows()}
    entries = json.load(open(os.path.join(ROOT, "cassmantle_amd", "ops", "gemm_tuning.json")))["entries"]
    assert len(entries) > 0
    assert sorted({e["cfg"] for e in entries} - live) == []


def test_binding_returns_the_header_rows():
    from cassmantle_amd.ops._ext import ext, ext_available
    if not ext_available():
        pytest.skip("extension not built")
    assert [tuple(r) for r in ext().gemm_tile_menu()] == header_rows()


PP_8WAVE = {"CASSMANTLE_GEMM_PP": "1", "CASSMANTLE_GEMM_8WAVE": "1"}


def dump(driver, runs):
    """build tests/native/<driver>.cpp against the planner's sources, run it once per (label, knobs, args)"""
    out = os.path.join(ROOT, "build", "native")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, driver)
    native = os.path.join(ROOT, "tests", "native")
    srcs = [os.path.join(CSRC, "gemm.hip"), os.path.join(CSRC, "gemm_areg.hip"), os.path.join(native, driver + ".cpp")]
    deps = srcs + [os.path.join(d, f) for d in (CSRC, native) for f in os.listdir(d) if f.endswith(".h")]
    if not (os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps)):
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC, *srcs, "-o", exe,
                            "-mllvm", "-pragma-unroll-threshold=100000"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith(("CASSMANTLE_GEMM_", "CASSMANTLE_LN_"))}
    got = ""
    for label, knobs, args in runs:
        r = subprocess.run([exe, label, *args], capture_output=True, text=True, timeout=120, env=dict(env, **knobs))
        assert r.returncode == 0, r.stderr[-2000:]
        got += r.stdout
    return got


def assert_golden(got, want):
    bad = [(g.split(" | ")[0], i) for i, (g, w) in enumerate(zip(got.splitlines(), want.splitlines())) if g != w]
    assert bad == [] and got == want


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_planner_plans_match_golden():
    got = dump("planner_dump", (("clean", {}, ()), ("pp1_8wave1", PP_8WAVE, ())))
    assert_golden(got, open(os.path.join(ROOT, "tests", "golden", "planner_plans.txt")).read())


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_routes_match_golden():
    """gemm_route over every call class, the planner golden's two environments plus the folded
    LayerNorm classes under CASSMANTLE_LN_INKERNEL=0 (read once per process).  The ``##`` lines of
    the golden mark the two classes whose route is not the parent commit's, with the parent's."""
    got = dump("route_dump", (("clean", {}, ()), ("pp1_8wave1", PP_8WAVE, ()),
                              ("ln_inkernel0", {"CASSMANTLE_LN_INKERNEL": "0"}, ("ln_kernel",))))
    want = open(os.path.join(ROOT, "tests", "golden", "gemm_routes.txt")).read()
    marked = [b.split(" | ")[0].split()[0] for a, b in zip(want.splitlines(), want.splitlines()[1:]) if a.startswith("##")]
    assert sorted(set(marked)) == ["geglu_lda1284", "k4_stats"]
    assert_golden(got, "".join(line for line in want.splitlines(True) if not line.startswith("##")))
