"""The e4m3 K/V image of the fp8 attention kernel, byte for byte against its CPU model
(kernel_oracle.kv8_image_model; test_kv8_oracle.py proves the model and that this comparison
rejects the planted bugs the fp8 attention check lets through).  Both writers: the pack
(attn_fp8_pack_kernel) over the attention edge grid and over every bf16 value, and the GEMM
epilogues (GemmArgs::kv8) in every tile of the menu at a width whose Q|K and K|V column
boundaries fall inside the tiles (C = 192), with partial M tiles and image boundaries inside a
tile.  The LDS-staged epilogue converts the bf16 tile it would have stored, so its image equals the
model of the plain run's own bf16 K and V exactly; the A-in-registers epilogue rounds fp32 once and
is held to BOUND["kv8"] against fp64 and to one e4m3 code of that model.  Inputs sit in NaN,
outputs and images between canaries (0xA5: a small finite e4m3 value, so only a byte compare
shows an unwritten run)."""
import pytest
import torch

import kernel_oracle as ko
from cassmantle_amd import ops
from cassmantle_amd.ops import reference as ref
from cassmantle_amd.ops._ext import ext, ext_available, ext_error
from kernel_oracle import BF16, BOUND, block_rel_err
from test_kernel_edges_gpu import DEV, G, MENU, P, check, gemm_raw, last_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _ext_loaded():
    assert ext_available(), ext_error()
    ops.set_mode("hip")


@pytest.fixture
def force_cfg():
    yield lambda c, s=0: ext().gemm_set_override(c, s)
    ext().gemm_set_override(-1, 0)


C = ko.KV8_EPI_C
HK = C // 64
EPS = 1e-5
# every live tile of the LDS-staged epilogue (static, ping-pong, deep ring); cfg 4 takes N <= 16 only
STAGED = [r[0] for r in MENU if r[1] != "areg" and r[0] != 4]
_EPI = {}


def image(B, Nk, Hk):
    return G((int(ext().attention_fp8_bytes(B, Nk, Hk)),), torch.uint8)


def assert_image(img, model, B, Nk, Hk, what):
    """guards intact and every byte the model's; a failure names the first differing byte"""
    torch.cuda.synchronize()
    ko.check_guards(img)
    got = img.view.cpu()
    if torch.equal(got, model):
        return
    bad = (got != model).nonzero().flatten()
    half = model.numel() // 2
    Nkp = (Nk + 63) // 64 * 64
    i = int(bad[0])
    j = i % half
    where = (("K8 [b, h, key, d]", j // (Hk * Nkp * 64), j // (Nkp * 64) % Hk, j // 64 % Nkp, j % 64) if i < half else
             ("V8t [b, h, d, slot]", j // (Hk * Nkp * 64), j // (Nkp * 64) % Hk, j // Nkp % 64, j % Nkp))
    raise AssertionError(f"{what}: {bad.numel()} of {model.numel()} bytes differ ({int((bad < half).sum())} in K8), first at "
                         f"{where}: 0x{int(got[i]):02X}, model 0x{int(model[i]):02X}")


def untouched(g):
    torch.cuda.synchronize()
    return bool((ko.int_view(g.buf) == g.pattern).all())


# ------------------------------------------------------------------------------ a. the pack
@pytest.mark.parametrize("B,Nk,Hk,lens", ko.KV8_PACK_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_pack_is_the_model_byte_for_byte(B, Nk, Hk, lens):
    k, v = ko.rnd(B, Nk, Hk, 64, seed=10 + Nk + Hk), ko.rnd(B, Nk, Hk, 64, scale=3.0, seed=11 + Nk + Hk)
    k[:, :, :, ::7] = (k[:, :, :, ::7].float() * 2.0 ** -7).to(BF16)          # e4m3 subnormals and values that round to zero
    if lens is not None:
        for b, n in enumerate(lens):
            v[b, n:] = ko.SENTINEL_V
            k[b, n:] = -ko.SENTINEL_V
    img = image(B, Nk, Hk)
    kp, vp = P(k, strided=True, row_dims=2), P(v, strided=True, row_dims=2)
    assert Nk == 1 or kp.stride(1) > Hk * 64
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    assert ops.pack_kv_fp8(kp, vp, ld, out=img.view).data_ptr() == img.view.data_ptr()
    assert_image(img, ko.kv8_image_model(k, v, lens), B, Nk, Hk, "pack")


# ------------------------------------------------------------------------------ b. the conversion
def _as_keys(x):
    """values as K [1, Nk, 1, 64] (zero padded to whole keys) and, reversed, as V"""
    n = -(-x.numel() // 64) * 64
    k = torch.cat([x, torch.zeros(n - x.numel(), dtype=BF16)]).view(1, n // 64, 1, 64)
    return k, k.flip(1, 3).contiguous()


def test_pack_converts_every_bf16_value_in_range_as_the_model():
    """v_cvt_pk_fp8_f32 against the CPU cast on every finite bf16 value with |x| <= 448: round to
    nearest even, subnormals, values that round to zero, both zeros"""
    x = ko.all_bf16(with_inf=False)
    x = x[x.float().abs() <= 448]
    assert x.numel() > 34000
    k, v = _as_keys(x)
    img = image(1, k.shape[1], 1)
    ops.pack_kv_fp8(P(k, strided=True, row_dims=2), P(v, strided=True, row_dims=2), None, out=img.view)
    torch.cuda.synchronize()
    K8 = ko.kv8_views(img.view.cpu(), 1, k.shape[1], 1)[0].flatten()[:x.numel()]
    exp = ref.e4m3_encode(x)
    bad = (K8 != exp).nonzero().flatten()
    assert bad.numel() == 0, [(float(x[i]), hex(int(K8[i])), hex(int(exp[i]))) for i in bad[:8].tolist()]
    assert_image(img, ko.kv8_image_model(k, v), 1, k.shape[1], 1, "all bf16 in range")


def test_pack_saturates_every_bf16_value_above_448():
    """the emitters saturate as ko.e4m3 and the fp8 attention oracle assume: 0x7E with the sign"""
    x = ko.all_bf16(with_inf=False)
    x = x[x.float().abs() > 448]
    k, v = _as_keys(x)
    img = image(1, k.shape[1], 1)
    ops.pack_kv_fp8(P(k, strided=True, row_dims=2), P(v, strided=True, row_dims=2), None, out=img.view)
    torch.cuda.synchronize()
    K8 = ko.kv8_views(img.view.cpu(), 1, k.shape[1], 1)[0].flatten()[:x.numel()]
    exp = torch.where(x.float() < 0, 0xFE, 0x7E).to(torch.uint8)
    bad = (K8 != exp).nonzero().flatten()
    assert bad.numel() == 0, (bad.numel(), [(float(x[i]), hex(int(K8[i]))) for i in bad[:8].tolist()])
    assert_image(img, ko.kv8_image_model(k, v), 1, k.shape[1], 1, "all bf16 above 448")


# ------------------------------------------------------------------------------ c. the staged epilogue
def epi_data(geom, Cc=C, K=None):
    """inputs (CPU), the fold (CPU), the device operands and the fp64 reference; once per shape"""
    key = (geom, Cc, K)
    if key not in _EPI:
        x, g, be, w, b = ko.kv8_epi_inputs(geom, Cc, K)
        wf, wsum, bf = ops.ln_fold(g, be, w, b)
        _EPI[key] = (x, (P(wf), wsum.to(DEV), P(bf)), ko.ln_linear64(x, g, be, w, b, EPS))
    return _EPI[key]


def run_qkv(x_dev, fold, geom, Cc, img=None, ln_rows=None):
    """the folded QKV GEMM through the raw binding into a guarded out (and image)"""
    wf, wsum, bf = fold
    out = G((geom[0] * geom[1], 3 * Cc))
    kw = {} if img is None else dict(kv8=img.view, kv8_col0=Cc, kv8_ntok=geom[1], kv8_hk=Cc // 64)
    kw.update(dict(ln_eps=EPS) if ln_rows is None else dict(ln_rows=ln_rows))
    gemm_raw(x_dev, wf, bf, None, out.view, None, ln_wsum=wsum, **kw)
    return out


def model_of(plain, geom, Cc):
    """the model image of a plain run's own bf16 K and V columns"""
    _, k, v = ko.qkv_split(plain.view.cpu(), geom, Cc)
    return ko.kv8_image_model(k, v)


@pytest.mark.parametrize("geom", ko.KV8_EPI_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("cfg", STAGED)
def test_staged_epilogue_image_is_exact_in_every_tile(cfg, geom, force_cfg):
    """K = 192 is three whole k-tiles, which every family takes under a forced plan.  Three kv8
    launches: the raw binding, ops.ln_linear, and the raw binding on a row-strided x with the row
    statistics handed in (the binding's own statistics pass takes contiguous rows only)."""
    B, ntok = geom
    x, fold, y64 = epi_data(geom)
    xp = P(x)
    force_cfg(cfg, 1)
    plain = run_qkv(xp, fold, geom, C)
    assert last_plan() == (cfg, 1)
    check(plain, y64, "ln_fold", f"cfg{cfg} {geom} plain")
    model = model_of(plain, geom, C)
    q_plain = plain.view[:, :C]

    img = image(B, ntok, HK)
    out = run_qkv(xp, fold, geom, C, img)
    assert last_plan() == (cfg, 1)
    assert_image(img, model, B, ntok, HK, f"cfg{cfg} {geom} raw")
    ko.check_guards(out)
    assert torch.equal(out.view[:, :C], q_plain), "Q columns differ from the plain run's"

    img = image(B, ntok, HK)
    y = ops.ln_linear(xp.view(B, ntok, C), None, None, EPS, None, fold=fold, kv8=img.view)
    assert last_plan() == (cfg, 1)
    assert_image(img, model, B, ntok, HK, f"cfg{cfg} {geom} ln_linear")
    assert torch.equal(y.view(B * ntok, 3 * C)[:, :C], q_plain)

    rows = torch.empty(B * ntok, 2, device=DEV)
    ext().row_stats(xp, rows, EPS)
    xs = P(x, strided=True)
    assert xs.stride(0) > C
    img = image(B, ntok, HK)
    out = run_qkv(xs, fold, geom, C, img, ln_rows=rows)
    assert last_plan() == (cfg, 1)
    assert_image(img, model, B, ntok, HK, f"cfg{cfg} {geom} strided x")
    ko.check_guards(out)
    assert torch.equal(out.view[:, :C], q_plain)


def test_staged_epilogue_image_under_the_planners_own_plan(force_cfg):
    geom = ko.KV8_EPI_GEOMS[1]
    B, ntok = geom
    x, fold, y64 = epi_data(geom)
    xp = P(x)
    img = image(B, ntok, HK)
    out = run_qkv(xp, fold, geom, C, img)
    plan = last_plan()
    assert plan[0] in STAGED, plan
    force_cfg(plan[0], 1)
    plain = run_qkv(xp, fold, geom, C)
    assert last_plan() == (plan[0], 1)
    check(plain, y64, "ln_fold", f"planner {plan}")
    assert_image(img, model_of(plain, geom, C), B, ntok, HK, f"planner {plan}")
    ko.check_guards(out)
    assert torch.equal(out.view[:, :C], plain.view[:, :C])


def test_forced_split_k_runs_unsplit_for_kv8(force_cfg):
    """a forced (cfg, 2) is a plan only with eight k-tiles (K = 512); the binding runs kv8 with
    split 1, so the image is that of the unsplit plain run"""
    geom = ko.KV8_EPI_GEOMS[1]
    B, ntok = geom
    x, fold, y64 = epi_data(geom, C, ko.KV8_SPLIT_K)
    xp = P(x)
    force_cfg(0, 2)
    img = image(B, ntok, HK)
    out = run_qkv(xp, fold, geom, C, img)
    assert last_plan() == (0, 2)
    force_cfg(0, 1)
    plain = run_qkv(xp, fold, geom, C)
    assert last_plan() == (0, 1)
    check(plain, y64, "ln_fold", "K = 512 plain")
    assert_image(img, model_of(plain, geom, C), B, ntok, HK, "forced (0, 2)")
    ko.check_guards(out)
    assert torch.equal(out.view[:, :C], plain.view[:, :C])


# ------------------------------------------------------------------------------ d. the A-in-registers writer
@pytest.mark.parametrize("Cc", ko.KV8_AREG_C)
def test_areg_epilogue_image(Cc):
    """rounds its fp32 accumulators to e4m3 once: under BOUND["kv8"] per 16 keys x 64 d against the
    fp64 K/V, and within one code of the model of the plain run's bf16 K/V"""
    geom = ko.KV8_EPI_GEOMS[0]
    B, ntok = geom
    Hk = Cc // 64
    x, fold, y64 = epi_data(geom, Cc)
    x3 = P(x).view(B, ntok, Cc)
    plain = ops.ln_linear(x3, None, None, EPS, None, fold=fold).view(B * ntok, 3 * Cc)
    assert last_plan()[0] == 15
    img = image(B, ntok, Hk)
    y = ops.ln_linear(x3, None, None, EPS, None, fold=fold, kv8=img.view).view(B * ntok, 3 * Cc)
    assert last_plan()[0] == 15
    torch.cuda.synchronize()
    ko.check_guards(img)
    assert torch.equal(y[:, :Cc], plain[:, :Cc]), "Q columns differ from the plain run's"
    _, k64, v64 = ko.qkv_split(y64, geom, Cc)
    for name, got, exp in zip("KV", ko.kv8_unpack(img.view, B, ntok, Hk), (k64, v64)):
        e = block_rel_err(got, exp, ko.KV8_BLOCK)
        print(f"kv8 areg C={Cc} {name}: worst block {e:.3e} (bound {BOUND['kv8']:g})")
        assert e < BOUND["kv8"], (name, e)
    _, k, v = ko.qkv_split(plain.cpu(), geom, Cc)
    apart = ko.kv8_codes_apart(img.view, ko.kv8_image_model(k, v))
    assert apart <= 1, apart


# ------------------------------------------------------------------------------ e. refusals
@pytest.mark.parametrize("what", ["ntok % 64", "residual", "fp32 out", "image size", "col0 + 128 hk != N"])
def test_kv8_refusals_leave_the_image_untouched(what):
    geom = ko.KV8_EPI_GEOMS[0]
    M = geom[0] * geom[1]
    x, (wf, wsum, bf), _ = epi_data(geom)
    img = image(geom[0], geom[1], HK)
    out = G((M, 3 * C), torch.float32 if what == "fp32 out" else BF16)
    res = P(ko.rnd(M, 3 * C, seed=1)) if what == "residual" else None
    kw = dict(kv8=img.view, kv8_col0=C, kv8_ntok=geom[1], kv8_hk=HK)
    if what == "ntok % 64":
        kw["kv8_ntok"] = 96
    elif what == "image size":
        kw["kv8"] = img.view[:-64]
    elif what == "col0 + 128 hk != N":
        kw["kv8_col0"] = C - 64
    with pytest.raises(RuntimeError, match="kv8"):
        gemm_raw(P(x), wf, bf, res, out.view, None, ln_wsum=wsum, ln_eps=EPS, **kw)
    assert untouched(img) and untouched(out)
