"""Plain-PyTorch reference implementations of every fused op.

These define the semantics the HIP kernels in ``ops/csrc`` must match (numerics tests compare
the kernels against these, computed in fp32) and are the CPU execution path (tests, the
no-GPU front-end).  On a GPU the HIP path is mandatory unless the caller explicitly opts into
``CASSMANTLE_OPS=torch`` (used only to measure the stock-PyTorch baseline).

Layout conventions (MI355X-first, see ``ops/__init__``):
* image activations are NHWC ``[B, H, W, C]`` contiguous (GEMM-friendly for implicit-GEMM
  conv; transformer tokens ``[B, H*W, C]`` are then a free view);
* conv weights are ``[Cout, kh, kw, Cin]`` (K-contiguous GEMM "B^T" operand);
* linear weights are ``[N, K]``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from .blur_format import box_params, gaussian_blur_pil  # noqa: F401  (PIL's GaussianBlur: the contract of ops/csrc/blur_pil.hip)
from .jpeg_format import jpeg_decode, jpeg_decoded, jpeg_encode  # noqa: F401  (baseline JPEG: the contracts of ops/csrc/jpeg.hip)


def _act(y: torch.Tensor, act: Optional[str]) -> torch.Tensor:
    if act is None or act == "none":
        return y
    if act == "gelu":
        return F.gelu(y)
    if act == "gelu_tanh":
        return F.gelu(y, approximate="tanh")
    if act == "silu":
        return F.silu(y)
    if act == "quick_gelu":
        return y * torch.sigmoid(1.702 * y)
    raise ValueError(act)


def _ct(dtype):
    """``dtype=`` of the reference ops: the compute type (fp32 when None).  When given, the result
    also comes back in it, unrounded (``torch.float64``: the oracle of tests/kernel_oracle.py)."""
    return torch.float32 if dtype is None else dtype


def linear(x, w, bias=None, residual=None, act=None, out_dtype=None, dtype=None):
    """y = act(x @ w^T + bias) + residual;  act='geglu': w is [2N, K] ->
    y = (x@w[:N]^T + b[:N]) * gelu(x@w[N:]^T + b[N:])."""
    od = out_dtype or dtype or x.dtype
    ct = _ct(dtype)
    y = torch.matmul(x.to(ct), w.to(ct).t())
    if bias is not None:
        y = y + bias.to(ct)
    if act == "geglu":
        h, g = y.chunk(2, dim=-1)
        y = h * F.gelu(g)
    elif act == "swiglu":
        h, g = y.chunk(2, dim=-1)
        y = h * F.silu(g)
    else:
        y = _act(y, act)
    if residual is not None:
        y = y + residual.to(ct)
    return y.to(od)


def conv2d(x, w, bias=None, stride=1, padding=1, residual=None, upsample=False, chan_bias=None, dtype=None):
    """NHWC conv.  x [B,H,W,Cin], w [Cout,kh,kw,Cin].  ``upsample`` = nearest 2x on the input
    first (fused in the HIP kernel's address generation).  ``chan_bias`` [B, Cout] is a
    per-sample bias (ResNet time-embedding add fused into the epilogue)."""
    ct = _ct(dtype)
    xi = x.to(ct).permute(0, 3, 1, 2)
    if upsample:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    wi = w.to(ct).permute(0, 3, 1, 2)
    y = F.conv2d(xi, wi, None if bias is None else bias.to(ct), stride=stride, padding=padding)
    y = y.permute(0, 2, 3, 1)
    if chan_bias is not None:
        y = y + chan_bias.to(ct)[:, None, None, :]
    if residual is not None:
        y = y + residual.to(ct)
    return y.to(dtype or x.dtype).contiguous()


def group_norm(x, num_groups, weight, bias, eps, silu=False, dtype=None):
    """NHWC GroupNorm (+ fused SiLU).  x [B, ..., C] (any spatial rank, channels last)."""
    B, C = x.shape[0], x.shape[-1]
    ct = _ct(dtype)
    xf = x.to(ct).reshape(B, -1, num_groups, C // num_groups)
    mean = xf.mean(dim=(1, 3), keepdim=True)
    var = xf.var(dim=(1, 3), keepdim=True, unbiased=False)
    y = (xf - mean) * torch.rsqrt(var + eps)
    y = y.reshape(B, -1, C) * weight.to(ct) + bias.to(ct)
    if silu:
        y = F.silu(y)
    return y.reshape(x.shape).to(dtype or x.dtype)


def layer_norm(x, weight, bias, eps, dtype=None):
    ct = _ct(dtype)
    return F.layer_norm(x.to(ct), (x.shape[-1],), weight.to(ct), None if bias is None else bias.to(ct),
                        eps).to(dtype or x.dtype)


def rms_norm(x, weight, eps, dtype=None):
    xf = x.to(_ct(dtype))
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.to(xf.dtype)).to(dtype or x.dtype)


# weight-only fp8 (the weight contract of ops/csrc/lm_fp8.hip's header comment, in torch)
E4M3_MAX = 448.0


def quantize_rows_fp8(w, gamma=None):
    """w [Nw, K] (and the gain gamma [K] folded in) -> (q uint8 [Nw, K] e4m3fn codes, scale fp32
    [Nw]): scale = rowmax |w * gamma| / 448 (1 for an all-zero row), q = RNE_e4m3(w * gamma /
    scale), all in fp32.  A non-finite row gives a non-finite scale (ops.quantize_rows_fp8 raises)."""
    if w.dim() != 2 or w.shape[1] % 16:
        raise ValueError(f"quantize_rows_fp8: w [Nw, K] with K % 16 == 0, not {tuple(w.shape)}")
    v = w.float()
    if gamma is not None:
        v = v * gamma.float()[None, :]
    a = v.abs().amax(dim=1)
    scale = torch.where(a == 0, torch.ones_like(a), a / torch.full_like(a, E4M3_MAX))   # (a true fp32 division)
    return e4m3_encode(v / scale[:, None]).contiguous(), scale.contiguous()


def e4m3_encode(t):
    """values -> uint8 OCP e4m3fn codes: fp32, clamped to +-448 (saturating), then round to nearest
    even by torch's cast (subnormals down to 2^-9 included, -0.0 keeps its sign).  The oracle
    calls it on CPU tensors only, so that it does not lean on the device's own fp8 casts."""
    return t.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_decode(q, dtype=None):
    """uint8 e4m3fn codes -> their values (exact in bf16 and wider).  Off the CPU through a table of
    the 256 codes made on the CPU, so the oracle does not lean on the device's own fp8 casts."""
    if q.device.type == "cpu":
        return q.view(torch.float8_e4m3fn).to(_ct(dtype))
    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(_ct(dtype)).to(q.device)
    return lut[q.long()]


def dequantize_rows_fp8(q, scale, dtype=None):
    """W' = e4m3(q) * scale[n]: bf16 (one fp32 product, rounded) or unrounded in ``dtype``"""
    if dtype is None:
        return (e4m3_decode(q) * scale.float()[:, None]).to(torch.bfloat16)
    return e4m3_decode(q, dtype) * scale.to(dtype)[:, None]


def linear_fp8(x, q, scale, bias=None, residual=None, act=None, rms_eps=None, out_dtype=None, dtype=None):
    """y = act(r * scale * (x @ e4m3(q)^T) + bias) + residual, r = rsqrt(mean x^2 + rms_eps) per
    row when ``rms_eps`` is given (the gain lives in q), else 1.  Gated acts: value row n, gate
    row N + n."""
    if x.shape[-1] % 16:
        raise ValueError(f"linear_fp8: K % 16 == 0, not K = {x.shape[-1]}")
    od = out_dtype or dtype or x.dtype
    ct = _ct(dtype)
    xf = x.to(ct)
    y = torch.matmul(xf, e4m3_decode(q, ct).t()) * scale.to(ct)
    if rms_eps is not None:
        y = y * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + rms_eps)
    if bias is not None:
        y = y + bias.to(ct)
    if act in ("geglu", "swiglu"):
        h, g = y.chunk(2, dim=-1)
        y = h * (F.gelu(g) if act == "geglu" else F.silu(g))
    else:
        y = _act(y, act)
    if residual is not None:
        y = y + residual.to(ct)
    return y.to(od)


def rope(x, pos, theta, dtype=None):
    """Rotate-half rotary embedding.  x [B, T, h, d]; pos [B, T] int positions."""
    d = x.shape[-1]
    ct = _ct(dtype)
    inv = theta ** (-torch.arange(0, d // 2, device=x.device, dtype=ct) * 2.0 / d)
    ang = pos.to(ct)[..., None] * inv                        # [B, T, d/2]
    cos, sin = ang.cos()[:, :, None, :], ang.sin()[:, :, None, :]
    xf = x.to(ct)
    x0, x1 = xf[..., : d // 2], xf[..., d // 2:]
    return torch.cat([x0 * cos - x1 * sin, x1 * cos + x0 * sin], dim=-1).to(dtype or x.dtype)


def rope_kv(qkv, pos0, q_out, k_cache, v_cache, H, Hk, theta):
    """Reference of the fused RoPE + KV-cache append (in place on q_out / caches)."""
    B, T, _ = qkv.shape
    d = q_out.shape[-1]
    x = qkv.view(B, T, H + 2 * Hk, d)
    pos = pos0.long()[:, None] + torch.arange(T, device=qkv.device)[None, :]
    q_out.copy_(rope(x[:, :, :H], pos, theta))
    kr = rope(x[:, :, H:H + Hk], pos, theta)
    for b in range(B):
        p0 = int(pos0[b])
        n = max(0, min(T, k_cache.shape[1] - p0))
        k_cache[b, p0:p0 + n] = kr[b, :n]
        v_cache[b, p0:p0 + n] = x[b, :n, H + Hk:]


def decode_attention(q, k_cache, v_cache, lens, scale, dtype=None):
    """q [B, H, d] one token vs cache [B, L, Hk, d] with lens[b] valid keys -> [B, H, d].
    A sequence with no valid key (``lens[b] == 0``) gets zeros, as from the HIP kernel."""
    B, H, d = q.shape
    out = torch.empty_like(q, dtype=dtype or q.dtype)
    for b in range(B):
        n = int(lens[b])
        o = attention(q[b:b + 1, None], k_cache[b:b + 1, :n], v_cache[b:b + 1, :n], scale, dtype=dtype)
        out[b] = o[0, 0]
    return out


def attention(q, k, v, scale=None, causal=False, kv_lens=None, dtype=None):
    """q [B,Nq,H,d], k/v [B,Nk,H,d] (any strides, last dim contiguous) -> o [B,Nq,H,d].
    ``kv_lens`` [B] int: keys >= len are masked (padding mask).  A query with no valid key
    (``kv_lens[b] == 0``, or no keys at all) gets zeros, not the NaN of a softmax over nothing:
    the contract of every HIP attention kernel (their ``inv = l > 0 ? 1 / l : 0``).  Keys past
    ``kv_lens`` never reach the result: their K/V values may be anything, NaN and inf included."""
    d = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if k.shape[2] != q.shape[2]:   # grouped-query attention: expand the kv heads
        g = q.shape[2] // k.shape[2]
        k, v = k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)
    ct = _ct(dtype)
    qf = q.to(ct).permute(0, 2, 1, 3)
    kf = k.to(ct).permute(0, 2, 1, 3)
    vf = v.to(ct).permute(0, 2, 1, 3)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    Nq, Nk = s.shape[-2], s.shape[-1]
    if causal:
        m = torch.ones(Nq, Nk, dtype=torch.bool, device=s.device).triu(1)
        s = s.masked_fill(m, float("-inf"))
    if kv_lens is not None:
        ar = torch.arange(Nk, device=s.device)
        m = ar[None, :] >= kv_lens.to(s.device)[:, None]
        s = s.masked_fill(m[:, None, None, :], float("-inf"))
    empty = torch.isneginf(s).all(dim=-1, keepdim=True)      # queries with no valid key
    p = torch.softmax(s.masked_fill(empty, 0.0), dim=-1)
    if kv_lens is not None:
        # a masked key contributes nothing whatever its V holds (p = 0 times inf would be NaN)
        vf = vf.masked_fill(m[:, None, :, None], 0.0)
    o = torch.matmul(p, vf).masked_fill(empty, 0.0).permute(0, 2, 1, 3)
    return o.to(dtype or q.dtype).contiguous()


def gather_cosine(table, ia, ib):
    """cos(table[ia[i]], table[ib[i]]); NaN where either index < 0."""
    ia = ia.long()
    ib = ib.long()
    valid = (ia >= 0) & (ib >= 0)
    a = table[ia.clamp(min=0)].float()
    b = table[ib.clamp(min=0)].float()
    s = (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1)).clamp_min(1e-12)
    return torch.where(valid, s, torch.full_like(s, float("nan")))


def pair_cosine(a, b):
    """Row-wise cosine of two [N, D] matrices -> [N] fp32."""
    a = a.float()
    b = b.float()
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1)).clamp_min(1e-12)


def cosine_topk(table, vec, k):
    t = table.float()
    v = vec.float()
    s = (t @ v) / (t.norm(dim=-1) * v.norm()).clamp_min(1e-12)
    # deterministic ties (the HIP kernel's contract): equal scores rank the lower row first
    vals, idx = torch.sort(s, descending=True, stable=True)
    return torch.return_types.topk((vals[:k], idx[:k]))


def gaussian_kernel1d(sigma: float, device=None):
    r = max(1, int(math.ceil(3.0 * sigma)))
    xs = torch.arange(-r, r + 1, dtype=torch.float32, device=device)
    w = torch.exp(-0.5 * (xs / sigma) ** 2)
    return w / w.sum()


def gaussian_blur(img, sigma: float):
    """Separable Gaussian blur with edge clamping.  img uint8/float [H, W, C]."""
    if sigma <= 0:
        return img
    dt = img.dtype
    x = img.float().permute(2, 0, 1)[None]
    w = gaussian_kernel1d(sigma, x.device)
    r = (w.numel() - 1) // 2
    C = x.shape[1]
    x = F.pad(x, (r, r, 0, 0), mode="replicate")
    x = F.conv2d(x, w.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)
    x = F.pad(x, (0, 0, r, r), mode="replicate")
    x = F.conv2d(x, w.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    y = x[0].permute(1, 2, 0)
    if dt == torch.uint8:
        y = y.round().clamp(0, 255)
    return y.to(dt)


def timestep_embedding(t, dim, flip_sin_to_cos=True, shift=0.0, max_period=10000.0):
    """Sinusoidal timestep features (SD convention: [cos, sin] with flip, shift 0)."""
    half = dim // 2
    ex = -math.log(max_period) * torch.arange(half, dtype=torch.float32, device=t.device) / (half - shift)
    arg = t.float()[:, None] * torch.exp(ex)[None, :]
    e = torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)
    if flip_sin_to_cos:
        e = torch.cat([e[:, half:], e[:, :half]], dim=-1)
    return e


def cfg_combine(eps, guidance):
    """eps [2B, ...] = [uncond; cond] -> eps_u + g (eps_c - eps_u)  (fp32 result)."""
    u, c = eps.float().chunk(2)
    return u + guidance * (c - u)


def latent_step(sample, eps, coef, guidance, cfg=True):
    """Fused CFG + linear scheduler update used by every scheduler here:
        e    = cfg(eps)                                   (if cfg)
        x'   = a * x + b * e + c * h1 + d * h2 + f * h3   (h* = scheduler history of e)
    ``coef`` is a float tensor [8]: (a, b, c, d, f, save_slot, _, _) – see schedulers.py.
    Returns (x', e)."""
    e = cfg_combine(eps, guidance) if cfg else eps.float()
    return (coef[0] * sample.float() + coef[1] * e), e


def silu(x):
    return F.silu(x.float()).to(x.dtype)


def mean_pool_l2(hidden, lens):
    """Masked mean over tokens then L2-normalise: hidden [B, T, D], lens [B] -> [B, D] fp32.
    ``lens > T`` counts T tokens; a row with ``lens == 0`` is the zero vector (no token is read),
    here and in misc.hip's mean_pool_l2_kernel."""
    T = hidden.shape[1]
    m = (torch.arange(T, device=hidden.device)[None, :] < lens.to(hidden.device)[:, None]).float()
    s = (hidden.float() * m[..., None]).sum(1) / m.sum(1, keepdim=True).clamp_min(1.0)
    return s / s.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def _lm_topk(v, eos: int, bias, k: int):
    """The samplers' top-k set: v [1, V] (logits / T, a fresh tensor: changed in place) with ``bias``
    added at ``eos``, sorted descending and stable (ties keep the LOWER id), the first k: (values,
    ids), each [1, k]."""
    if 0 <= eos < v.shape[-1]:
        v[:, eos] += bias
    srt = torch.sort(v, dim=-1, descending=True, stable=True)
    return srt.values[:, :k], srt.indices[:, :k]


def lm_sample(logits, noise, eos_bias, eos: int, temperature: float, k: int, step, out, tok, pos, lens) -> None:
    """Decode-step sampler (the contract of lm_sample.hip's lm_sample_kernel), graph-capturable: v =
    logits / T with the step's EOS bias added at ``eos``; the k largest v (stable: ties keep the
    LOWER id); the id maximising v + noise[step] among them (first in that order on ties); then
    out[step] = tok = id and pos, lens, step advance by one.  -0.0 and +0.0 are equal in that
    sort, so of two zeros the lower id ranks first whatever their signs; the kernel turns -0.0
    into +0.0 before it builds its keys to rank them the same way."""
    vals, ids = _lm_topk(logits.float().reshape(1, -1) / temperature, eos, eos_bias.index_select(0, step), k)
    g = noise.index_select(0, step)[0].gather(1, ids)
    choice = (vals + g).argmax(dim=-1, keepdim=True)
    nxt = ids.gather(1, choice)[:, 0]
    out.index_copy_(0, step, nxt[None])
    tok.copy_(nxt)
    pos.add_(1)
    lens.add_(1)
    step.add_(1)


def lm_gumbel(seeds, step: int, ids) -> torch.Tensor:
    """The sampler's noise alone (GUMBEL CONTRACT, ops/csrc/philox_gumbel.h): fp32 [B, n] of the
    float64 model ``schedulers.philox_gumbel`` for seeds [B] int64, a decode step and ids [n]."""
    from ..models.schedulers import philox_gumbel
    g = philox_gumbel(seeds.detach().cpu().numpy(), int(step), ids.detach().cpu().numpy())
    return torch.from_numpy(g).to(device=seeds.device, dtype=torch.float32)


def lm_sample_seeded(logits, seeds, eos_bias, eos: int, temperature: float, k: int, step, out, tok, pos, lens) -> None:
    """Batched decode-step sampler with seeded noise (the contract of lm_sample_seeded_kernel), per
    row b of logits [B, V]: v = logits / T with eos_bias[step[b]] added at ``eos``; the k largest
    v by ``lm_sample``'s stable sort (ties keep the LOWER id); among them the id maximising
    v + g(seeds[b], step[b], id) with the float64 model noise (first in that order on ties: the
    larger v, then the lower id); then out[step[b], b] = tok[b] = id and pos[b], lens[b], step[b]
    advance by one.  Every row has its own step counter and seed, and a row's token does not
    depend on the other rows.  Reads the counters on the host: not graph-capturable."""
    from ..models.schedulers import philox_gumbel
    lg = logits.float() / temperature
    steps, sds = step.tolist(), seeds.tolist()
    for b in range(lg.shape[0]):
        vals, ids = (t[0].cpu() for t in _lm_topk(lg[b:b + 1], eos, eos_bias[steps[b]], k))
        g = philox_gumbel([sds[b]], steps[b], ids.numpy())[0]
        nxt = int(ids[int((vals.double().numpy() + g).argmax())])
        out[steps[b], b] = nxt
        tok[b] = nxt
    pos.add_(1)
    lens.add_(1)
    step.add_(1)
