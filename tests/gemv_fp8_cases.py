"""Cases, inputs and fp64 models of the weight-only fp8 path (ops/csrc/lm_fp8.hip), shared by
test_lm_fp8.py (CPU: the models against the bound, the planted bugs) and test_lm_fp8_gpu.py (the
kernels on these cases).  The instruments are kernel_oracle.py's."""
import math
from typing import NamedTuple

import torch

import kernel_oracle as ko
from cassmantle_amd.ops import reference as ref
from kernel_oracle import BF16, F64

GATED = ko.GATED
FP8_STEP = 128               # k elements of one wave step of gemv_fp8_kernel
FP8_PASS = 8 * FP8_STEP      # one pass of the block: its 8 waves take one step each
FP8_BODY = 4 * FP8_PASS      # the unrolled body: four steps per wave
FP8_COLS = 16                # output columns of a block
BLOCK = (1, 4)               # the error block: a row x 4 columns (finer than the kernel's 16)

FP8_M = (1, 2, 3, 5, 8)
FP8_N = (1, 5, 7, 70)        # a block's column tail, one block and five
# one lane / three lanes / one pass of the block -+ a lane / the unrolled body once and twice -+ a lane /
# Mistral's down projection (14 whole steps per wave: three bodies and two single steps)
FP8_K = (16, 48, FP8_PASS, FP8_PASS - 16, FP8_PASS + 16, FP8_BODY, FP8_BODY - 16, FP8_BODY + 16,
         2 * FP8_BODY, 2 * FP8_BODY - 16, 2 * FP8_BODY + 16, 14336)
W_ROW_SCALE = (1.0, 8.0, 1.0 / 32, 3.0)      # weight row n is scaled by W_ROW_SCALE[n % 4]: every row its own scale
RMS_EPS = 1e-5


class Fp8Case(NamedTuple):
    M: int
    N: int            # outputs (the weight has 2N rows for the gated activations)
    K: int
    act: str
    rms: bool         # fused RMS scale (the gain folded into the weight)

    @property
    def gated(self):
        return self.act in GATED

    @property
    def id(self):
        return f"{self.M}x{self.N}x{self.K}-{self.act}{'-rms' if self.rms else ''}"


def fp8_cases() -> list:
    """per (M, gated or not): every N at K = 48 and every K at N = 7 (gated: 3, and 3 and 9 at
    K = 48 for M = 5 and 8); the two activations and the RMS scale take turns, shifted by M so that
    every K meets both"""
    cases = []
    for mi, M in enumerate(FP8_M):
        for acts in (("none", "silu"), GATED):
            gated = acts == GATED
            shapes = [(N, 48) for N in FP8_N + ((3, 9) if gated and M in (5, 8) else ())]
            shapes += [(3 if gated else 7, K) for K in FP8_K]
            shapes = list(dict.fromkeys(shapes))
            cases += [Fp8Case(M, N, K, acts[(i + mi) % 2], bool(((i + mi) // 2) % 2)) for i, (N, K) in enumerate(shapes)]
    return cases


FP8_CASES = fp8_cases()
DISPATCH_CASES = [Fp8Case(M, 72, 128, act, rms) for M in (8, 9) for act, rms in (("none", False), ("swiglu", True))]
QUANT_N = (1, 5, 70)
QUANT_K = (16, 48, 4112)     # 4112: two passes of the quantiser's 256 lanes x 8 and a tail


class Fp8Inputs(NamedTuple):
    x: torch.Tensor       # [M, K] bf16, row m scaled by 3 * RMS_ROW_SCALE[m % 3]
    q: torch.Tensor       # [Nw, K] uint8
    scale: torch.Tensor   # [Nw] fp32
    bias: torch.Tensor    # [Nw] bf16
    res: torch.Tensor     # [M, N] bf16


def fp8_weight(Nw, K, seed, rms=True):
    """bf16 weight rows scaled by W_ROW_SCALE and the gain (None without the RMS scale)"""
    sc = torch.tensor([W_ROW_SCALE[n % 4] for n in range(Nw)])
    w = (ko.rnd(Nw, K, scale=K ** -0.5, seed=seed).float() * sc[:, None]).to(BF16)
    return w, (ko.rnd(K, scale=0.3, shift=1.0, seed=seed + 5) if rms else None)


_INPUTS = {}


def fp8_inputs(c: Fp8Case) -> Fp8Inputs:
    """computed once per case, shared by the tests, never changed"""
    if c not in _INPUTS:
        Nw = 2 * c.N if c.gated else c.N
        s = 9000 + 7 * c.M + 3 * c.N + c.K + len(c.act) + c.rms
        rs = torch.tensor([3 * ko.RMS_ROW_SCALE[m % 3] for m in range(c.M)])
        x = (ko.rnd(c.M, c.K, seed=s).float() * rs[:, None]).to(BF16)
        w, gamma = fp8_weight(Nw, c.K, s + 1, c.rms)
        q, scale = ref.quantize_rows_fp8(w, gamma)
        _INPUTS[c] = Fp8Inputs(x, q, scale, ko.rnd(Nw, scale=0.1, seed=s + 2), ko.rnd(c.M, c.N, seed=s + 3))
    return _INPUTS[c]


def linear_fp8_64(c: Fp8Case, i: Fp8Inputs) -> torch.Tensor:
    """fp64 of the same (q, scale): the reference of every bound"""
    return ref.linear_fp8(i.x, i.q, i.scale, i.bias, i.res, c.act, RMS_EPS if c.rms else None, dtype=F64)


def fp8_model(c: Fp8Case, i: Fp8Inputs, scale_of_row0=False, gate_takes_value_scale=False,
              drop_last_16=False) -> ko.Guarded:
    """the ideal gemv_fp8_kernel in fp64: raw x, exact e4m3, the row scales, one rounding (the bf16
    store), written into a guarded output.  The planted bugs: ``scale_of_row0`` gives every weight
    row row 0's scale, ``gate_takes_value_scale`` gives gate row N + n the scale of value row n,
    ``drop_last_16`` leaves the 16 k-elements at K - 16 out of every dot product."""
    xd, wd, sc = i.x.to(F64), ref.e4m3_decode(i.q, F64), i.scale.to(F64).clone()
    if scale_of_row0:
        sc[:] = sc[0]
    if gate_takes_value_scale and c.gated:
        sc[c.N:] = sc[:c.N]
    r = torch.ones(c.M, 1, dtype=F64)
    if c.rms:
        r = (xd * xd).mean(-1, keepdim=True).add(RMS_EPS).rsqrt()
    if drop_last_16:
        xd = xd.clone()
        xd[:, c.K - 16:] = 0
    y = (xd @ wd.t()) * sc * r + i.bias.to(F64)
    if c.gated:
        h, g = y.chunk(2, dim=-1)
        y = h * (torch.nn.functional.gelu(g) if c.act == "geglu" else torch.nn.functional.silu(g))
    elif c.act == "silu":
        y = torch.nn.functional.silu(y)
    y = y + i.res.to(F64)
    out = ko.guarded((c.M, c.N))
    out.view.copy_(y.to(BF16))
    return out


def poisoned_codes(q: torch.Tensor, device) -> torch.Tensor:
    """``q`` inside a buffer of 0x7F bytes (the e4m3 NaN code) with kernel_oracle's guard-sized margins"""
    g = ko.guard_elems(q.shape, torch.uint8)
    buf = torch.full((g + q.numel() + g,), 0x7F, dtype=torch.uint8, device=device)
    view = buf[g:g + q.numel()].view(q.shape)
    view.copy_(q)
    assert view.data_ptr() % 16 == 0
    return view


def all_e4m3_codes() -> torch.Tensor:
    """the 254 finite codes (0x7F and 0xFF are NaN), padded with zeros to 256"""
    c = torch.arange(256, dtype=torch.uint8)
    c[0x7F] = 0
    c[0xFF] = 0
    return c
