"""Local causal language model for round prompts (optional generator, SURVEY §2.3 'Prompt LLM').

The reference calls a remote Mistral-7B-Instruct endpoint (``src/backend.py:240-268``:
``{"inputs": seed, "parameters": {"min_new_tokens": 32, "max_new_tokens": 96}}``) and keeps the
first two sentences of the continuation.  Here the same model family runs on the GPU that
already hosts the diffusion pipeline (7B bf16 = 14.5 GB of the 288 GB HBM):

* Mistral/Llama architecture: RMSNorm (HIP), fused QKV projection, rotate-half RoPE fused with
  the KV-cache append (HIP ``rope_kv``), grouped-query attention (prefill: the flash kernel with a
  head group; decode: the split-KV ``decode_attention`` kernel), SwiGLU MLP as one gated GEMM
  epilogue (``act="swiglu"``), residual adds fused into the output projections.
* Decode is weight-streaming (M = batch rows): every projection goes through the skinny-M GEMV
  path of the GEMM dispatcher.
* The whole per-token step (embedding gather → 32 layers → logits → temperature/top-k Gumbel
  sampling → position bump) reads and writes only device buffers, so it is captured ONCE as a
  hipGraph and replayed ``max_new_tokens`` times with a single host sync at the end
  (min-new-tokens is an on-device EOS bias table, sampling noise a pre-drawn table).
* ``noise="philox"``: the sampler draws its Gumbel noise in the kernel from a per-sequence seed
  (``ops.lm_sample_seeded``, ops/csrc/philox_gumbel.h), so there is no table to draw and upload and
  several rooms' prompts decode as ONE batch of up to 8 rows: one pass over the weights per token
  position for all of them (``generate_ids_batch``, buckets of 1, 2, 4, 8 rows with a captured
  graph each).

* ``weight_dtype="fp8"`` (``CausalLM.quantize_fp8_``): every projection becomes e4m3 codes with one
  scale per row (the RMSNorm gains folded in, ``embed`` stays bf16) and decode streams them through
  ``ops.linear_fp8`` (ops/csrc/lm_fp8.hip): half the bytes per token.  Prefill over more than 8
  rows dequantises one projection at a time into one scratch buffer and runs the bf16 GEMM.

Weights are random-init by default (no checkpoints on the box); ``models/weights.py``
``load_causal_lm`` maps a HF-layout safetensors checkpoint in.  Without a real tokenizer a
byte-level tokenizer is used, so random weights emit unusable text and
``game.prompts.LMPromptGenerator`` falls back to the template generator (2-sentence contract).
"""
from __future__ import annotations

import math
import threading
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from .. import ops
from ..utils.tracing import TRACER


@dataclass(frozen=True)
class CausalLMConfig:
    name: str
    vocab: int
    dim: int
    layers: int
    heads: int
    kv_heads: int
    ffn: int
    rope_theta: float = 10000.0
    eps: float = 1e-5
    max_ctx: int = 512            # KV-cache capacity used for prompt generation

    @property
    def head_dim(self) -> int:
        return self.dim // self.heads


# mistralai/Mistral-7B-v0.1 shapes (public config) — the reference's remote model family
MISTRAL_7B = CausalLMConfig("mistral-7b", 32000, 4096, 32, 32, 8, 14336, 10000.0, 1e-5, 512)
TINY_LM = CausalLMConfig("tiny-lm", 320, 256, 2, 4, 2, 512, 10000.0, 1e-5, 256)
LM_CONFIGS = {"mistral-7b": MISTRAL_7B, "tiny-lm": TINY_LM}


class ByteTokenizer:
    """UTF-8 bytes + BOS/EOS.  Used when no sentencepiece model is available."""

    bos, eos = 256, 257

    def encode(self, text: str) -> List[int]:
        return [self.bos] + list(text.encode("utf-8"))

    def decode(self, ids: Sequence[int]) -> str:
        return bytes(i for i in ids if 0 <= i < 256).decode("utf-8", errors="ignore")


class SentencePieceTokenizer:
    def __init__(self, path: str) -> None:
        import sentencepiece as spm
        self.sp = spm.SentencePieceProcessor(model_file=path)
        self.bos, self.eos = self.sp.bos_id(), self.sp.eos_id()

    def encode(self, text: str) -> List[int]:
        return [self.bos] + list(self.sp.encode(text))

    def decode(self, ids: Sequence[int]) -> str:
        return self.sp.decode([int(i) for i in ids])


def _randn(shape, std, gen, device, dtype) -> nn.Parameter:
    t = torch.empty(shape, device=device, dtype=dtype)
    t.normal_(0.0, std, generator=gen)
    return nn.Parameter(t, requires_grad=False)


class LMBlock(nn.Module):
    def __init__(self, c: CausalLMConfig, gen, device, dtype):
        super().__init__()
        hd = c.head_dim
        self.c = c
        self.attn_norm = nn.Parameter(torch.ones(c.dim, device=device, dtype=dtype), requires_grad=False)
        self.mlp_norm = nn.Parameter(torch.ones(c.dim, device=device, dtype=dtype), requires_grad=False)
        self.qkv = _randn(((c.heads + 2 * c.kv_heads) * hd, c.dim), 1.0 / math.sqrt(c.dim), gen, device, dtype)
        self.o = _randn((c.dim, c.heads * hd), 1.0 / math.sqrt(c.dim * 2 * c.layers), gen, device, dtype)
        self.gate_up = _randn((2 * c.ffn, c.dim), 1.0 / math.sqrt(c.dim), gen, device, dtype)  # [up; gate]
        self.down = _randn((c.dim, c.ffn), 1.0 / math.sqrt(c.ffn * 2 * c.layers), gen, device, dtype)
        self.quantized = False

    def quantize_fp8_(self) -> None:
        """bf16 projections -> (codes, scale) buffers ``<name>_q`` / ``<name>_s`` (ops.quantize_rows_fp8);
        the RMSNorm gains go into qkv / gate_up and become ones; the bf16 projections are freed."""
        for name, gain in (("qkv", self.attn_norm), ("o", None), ("gate_up", self.mlp_norm), ("down", None)):
            _quantize_param(self, name, gain)
        self.quantized = True

    def forward(self, x, kc, vc, pos0, lens, decode: bool, scratch=None):
        """x [B, T, dim]; kc/vc [B, L, Hk, hd] cache of this layer.  ``scratch``: the quantised
        model's dequantisation buffer (prefill over more than 8 rows)."""
        c = self.c
        B, T, _ = x.shape
        hd = c.head_dim
        if self.quantized:
            qkv = ops.linear_fp8(x, self.qkv_q, self.qkv_s, rms_eps=c.eps, scratch=scratch)
        else:
            qkv = ops.rms_linear(x, self.attn_norm, c.eps, self.qkv)
        q = torch.empty((B, T, c.heads, hd), device=x.device, dtype=x.dtype)
        ops.rope_kv(qkv, pos0, q, kc, vc, c.heads, c.kv_heads, c.rope_theta)
        if decode:
            o = ops.decode_attention(q.view(B, c.heads, hd), kc, vc, lens)
        else:
            # prefill from position 0: causal flash attention over the freshly written cache rows
            o = ops.attention(q, kc[:, :T], vc[:, :T], causal=True)
        if self.quantized:
            x = ops.linear_fp8(o.reshape(B, T, c.heads * hd), self.o_q, self.o_s, residual=x, scratch=scratch)
            h = ops.linear_fp8(x, self.gate_up_q, self.gate_up_s, act="swiglu", rms_eps=c.eps, scratch=scratch)
            return ops.linear_fp8(h, self.down_q, self.down_s, residual=x, scratch=scratch)
        x = ops.linear(o.reshape(B, T, c.heads * hd), self.o, residual=x)
        h = ops.rms_linear(x, self.mlp_norm, c.eps, self.gate_up, act="swiglu")
        return ops.linear(h, self.down, residual=x)


def _quantize_param(mod: nn.Module, name: str, gain: Optional[nn.Parameter]) -> None:
    """``mod.<name>`` [Nw, K] bf16 (times ``gain`` [K], which becomes ones) -> buffers ``<name>_q``
    uint8 and ``<name>_s`` fp32; the parameter is deleted."""
    w = getattr(mod, name)
    q, s = ops.quantize_rows_fp8(w.data, None if gain is None else gain.data)
    delattr(mod, name)
    mod.register_buffer(name + "_q", q)
    mod.register_buffer(name + "_s", s)
    if gain is not None:
        gain.data.fill_(1.0)


def _weight_f32(mod: nn.Module, name: str) -> torch.Tensor:
    """fp32 projection ``name`` of a block or model: the bf16 parameter, or e4m3(q) * scale"""
    if hasattr(mod, name + "_q"):
        from ..ops import reference as R
        return R.dequantize_rows_fp8(getattr(mod, name + "_q"), getattr(mod, name + "_s"), dtype=torch.float32)
    return getattr(mod, name).float()


class CausalLM(nn.Module):
    def __init__(self, c: CausalLMConfig, device=None, dtype=torch.bfloat16, seed: int = 0):
        super().__init__()
        device = torch.device(device) if device is not None else torch.device("cpu")
        gen = torch.Generator(device=device).manual_seed(seed)
        self.c = c
        self.embed = _randn((c.vocab, c.dim), 1.0, gen, device, dtype)
        self.blocks = nn.ModuleList([LMBlock(c, gen, device, dtype) for _ in range(c.layers)])
        self.norm = nn.Parameter(torch.ones(c.dim, device=device, dtype=dtype), requires_grad=False)
        self.lm_head = _randn((c.vocab, c.dim), 1.0 / math.sqrt(c.dim), gen, device, dtype)
        self.quantized = False
        self._scratch: Optional[torch.Tensor] = None

    @torch.no_grad()
    def quantize_fp8_(self) -> "CausalLM":
        """Weight-only fp8, in place (weight contract: ops/csrc/lm_fp8.hip): qkv, gate_up and lm_head
        with their RMSNorm gain folded in (the gains become ones), o and down as they are; the bf16
        projections are freed one by one, ``embed`` stays bf16.  Load a checkpoint first, then
        quantise: a second call raises."""
        if self.quantized:
            raise RuntimeError("CausalLM.quantize_fp8_: the model is quantised already")
        for blk in self.blocks:
            blk.quantize_fp8_()
        _quantize_param(self, "lm_head", self.norm)
        self.quantized = True
        return self

    def weight_bytes(self) -> int:
        """bytes one decode step streams: every projection (codes and scales, or bf16), not ``embed``"""
        skip = {id(self.embed)}
        ts = [p for p in self.parameters() if id(p) not in skip] + list(self.buffers())
        return sum(t.numel() * t.element_size() for t in ts)

    def _prefill_scratch(self, rows: int) -> Optional[torch.Tensor]:
        """the one dequantisation buffer of a quantised model, sized for its largest projection (235 MB
        at Mistral's gate_up) and made when a prefill over more than 8 rows first needs it"""
        if not self.quantized or rows <= ops.FP8_GEMV_ROWS:
            return None
        if self._scratch is None:
            n = max(b.numel() for name, b in self.named_buffers() if name.endswith("_q"))
            self._scratch = torch.empty((n,), device=self.embed.device, dtype=torch.bfloat16)
        return self._scratch

    def alloc_cache(self, B: int, L: int):
        c = self.c
        shape = (c.layers, B, L, c.kv_heads, c.head_dim)
        dev, dt = self.embed.device, self.embed.dtype
        return torch.zeros(shape, device=dev, dtype=dt), torch.zeros(shape, device=dev, dtype=dt)

    def forward(self, tokens: torch.Tensor, kcache, vcache, pos0: torch.Tensor,
                lens: Optional[torch.Tensor] = None, decode: bool = False) -> torch.Tensor:
        """tokens [B, T] -> logits of the last position [B, vocab] (bf16).  ``decode``: T == 1 at
        device positions ``pos0`` with ``lens = pos0 + 1`` valid keys; else prefill from 0."""
        B, T = tokens.shape
        x = self.embed.index_select(0, tokens.reshape(-1)).view(B, T, self.c.dim)
        if self.quantized:
            scratch = self._prefill_scratch(B * T)
            for i, blk in enumerate(self.blocks):
                x = blk(x, kcache[i], vcache[i], pos0, lens, decode, scratch)
            return ops.linear_fp8(x[:, -1], self.lm_head_q, self.lm_head_s, rms_eps=self.c.eps, scratch=scratch)
        for i, blk in enumerate(self.blocks):
            x = blk(x, kcache[i], vcache[i], pos0, lens, decode)
        return ops.rms_linear(x[:, -1], self.norm, self.c.eps, self.lm_head)

    @torch.no_grad()
    def full_logits(self, tokens: torch.Tensor) -> torch.Tensor:
        """Cache-free reference forward (all positions) -> [B, T, vocab] f32.  Test oracle; on a
        quantised model it multiplies e4m3(q) * scale in fp32 (the gains are ones there)."""
        from ..ops import reference as R
        c = self.c
        B, T = tokens.shape
        hd = c.head_dim
        x = self.embed.index_select(0, tokens.reshape(-1)).view(B, T, c.dim).float()
        pos = torch.arange(T, device=tokens.device)[None].expand(B, T)
        for blk in self.blocks:
            n = R.rms_norm(x, blk.attn_norm, c.eps).float()
            qkv = (n @ _weight_f32(blk, "qkv").t()).view(B, T, c.heads + 2 * c.kv_heads, hd)
            q = R.rope(qkv[:, :, :c.heads], pos, c.rope_theta).float()
            k = R.rope(qkv[:, :, c.heads:c.heads + c.kv_heads], pos, c.rope_theta).float()
            v = qkv[:, :, c.heads + c.kv_heads:]
            o = R.attention(q, k, v, causal=True).float()
            x = x + o.reshape(B, T, -1) @ _weight_f32(blk, "o").t()
            n = R.rms_norm(x, blk.mlp_norm, c.eps).float()
            hg = n @ _weight_f32(blk, "gate_up").t()
            h, g = hg.chunk(2, dim=-1)
            x = x + (h * torch.nn.functional.silu(g)) @ _weight_f32(blk, "down").t()
        x = R.rms_norm(x, self.norm, c.eps).float()
        return x @ _weight_f32(self, "lm_head").t()


LM_NOISE = ("table", "philox")
LM_WEIGHT_DTYPES = ("bf16", "fp8")
BUCKETS = (1, 2, 4, 8)            # batch sizes of the philox decode path, capped at max_batch


class _Bucket:
    """Static buffers and the captured decode graph of one batch size.  ``noise="table"`` has the
    one-row bucket only, which also owns the [max_new_cap, 1, vocab] noise table."""

    def __init__(self, gen: "LMTextGenerator", B: int) -> None:
        dev, max_new_cap = gen.device, gen.max_new_cap
        self.B = B
        self.noise = None
        if gen.noise_mode == "table":
            self.noise = torch.zeros((max_new_cap, 1, gen.cfg.vocab), device=dev, dtype=torch.float32)
        self.kc, self.vc = gen.model.alloc_cache(B, gen.cfg.max_ctx)   # [layers, B, L, Hk, hd]
        self.tok = torch.zeros((B,), device=dev, dtype=torch.long)
        self.pos = torch.zeros((B,), device=dev, dtype=torch.int32)
        self.lens = torch.ones((B,), device=dev, dtype=torch.int32)
        self.step = torch.zeros((B,), device=dev, dtype=torch.long)
        self.seeds = torch.zeros((B,), device=dev, dtype=torch.long)
        self.out = torch.zeros((max_new_cap, B), device=dev, dtype=torch.long)
        self.graph = None
        pin = dev.type == "cuda"
        # one pinned staging row per buffer: filled on the host, one copy each per call
        self.h_tok = torch.zeros((B,), dtype=torch.long, pin_memory=pin)
        self.h_pos = torch.zeros((B,), dtype=torch.int32, pin_memory=pin)
        self.h_lens = torch.zeros((B,), dtype=torch.int32, pin_memory=pin)
        self.h_seeds = torch.zeros((B,), dtype=torch.long, pin_memory=pin)

    def state(self):
        return self.tok, self.pos, self.lens, self.step


class LMTextGenerator:
    """``generate_text(prompt, min_new_tokens, max_new_tokens)`` for
    :class:`~cassmantle_amd.game.prompts.LMPromptGenerator` (continuation only, no echo).

    ``noise="table"`` (default): one batch-1 sequence per call, Gumbel noise drawn on the host and
    uploaded as a [max_new, 1, vocab] table.  ``noise="philox"``: the sampler draws its noise in
    the kernel from a per-sequence seed (``ops.lm_sample_seeded``), so up to ``max_batch``
    sequences decode as one batch (``generate_ids_batch`` / ``generate_texts``), in the smallest
    bucket of 1, 2, 4, 8 rows that holds them; a sequence's tokens depend on its prompt and seed
    alone, not on the bucket, its row or the other sequences (given row-independent logits).  Both
    modes run one decode loop (``_decode``) over a bucket; the table path is its one-row case."""

    def __init__(self, cfg: CausalLMConfig = TINY_LM, device=None, seed: int = 0, use_graphs: bool = True,
                 tokenizer=None, temperature: float = 0.8, top_k: int = 40, max_new_cap: int = 128,
                 noise: str = "table", max_batch: int = 1, weight_dtype: str = "bf16") -> None:
        if noise not in LM_NOISE:
            raise ValueError(f"unknown lm noise {noise!r}: one of {', '.join(LM_NOISE)}")
        if weight_dtype not in LM_WEIGHT_DTYPES:
            raise ValueError(f"unknown lm weight dtype {weight_dtype!r}: one of {', '.join(LM_WEIGHT_DTYPES)}")
        if not 1 <= int(max_batch) <= BUCKETS[-1]:
            raise ValueError(f"max_batch must be 1..{BUCKETS[-1]}, not {max_batch}")
        if max_batch > 1 and noise != "philox":
            raise ValueError("max_batch > 1 needs noise='philox'")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.cfg = cfg
        self.model = CausalLM(cfg, device=self.device, seed=seed)
        self.tok = tokenizer or ByteTokenizer()
        self.temperature, self.top_k = temperature, min(top_k, cfg.vocab)
        self.use_graphs = use_graphs and self.device.type == "cuda"
        self.max_new_cap = max_new_cap
        self.seed = seed
        self.noise_mode = noise
        self.max_batch = int(max_batch)
        dev = self.device
        self.eos_bias = torch.zeros((max_new_cap,), device=dev, dtype=torch.float32)
        self.calls = 0
        self._lock = threading.Lock()
        # host time of the last call before its first launch (table path: the table drawn and uploaded too)
        self.host_ms = 0.0
        # one set of static buffers and one graph per bucket, made when first used
        self.bucket_sizes = tuple(sorted({min(b, self.max_batch) for b in BUCKETS}))
        self.buckets: Dict[int, _Bucket] = {}
        if noise == "philox":
            # a reference sampler that reads its counters on the host cannot be captured
            self.use_graphs = self.use_graphs and ops.get_mode() == "hip"
        self.weight_dtype = "bf16"
        self.quant_ms = 0.0               # what quantize_fp8 took (with its one check of the scales)
        if weight_dtype == "fp8":
            self.quantize_fp8()

    def quantize_fp8(self) -> None:
        """The model's projections to weight-only fp8 (``CausalLM.quantize_fp8_``), after any
        checkpoint is loaded and before the first call: a captured graph holds the bf16 weights."""
        if self.buckets:
            raise RuntimeError("quantize_fp8: quantise before the first generate call")
        t0 = time.perf_counter()
        self.model.quantize_fp8_()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.quant_ms = (time.perf_counter() - t0) * 1e3
        self.weight_dtype = "fp8"

    def _bucket(self, n: int) -> _Bucket:
        B = next(b for b in self.bucket_sizes if b >= n)
        if B not in self.buckets:
            self.buckets[B] = _Bucket(self, B)
        return self.buckets[B]

    # one decode step entirely on device buffers (captured as a graph on GPU)
    def _step(self, bk: _Bucket) -> None:
        logits = self.model(bk.tok.view(bk.B, 1), bk.kc, bk.vc, bk.pos, bk.lens, decode=True)
        # top-k + Gumbel-max per row and the token / position / length / step update: one in-tree
        # kernel on the GPU (lm_sample.hip), no ATen sampling ops.  The noise is this step's row of
        # the table, or drawn in the kernel from the row's seed and step
        sample, noise = (ops.lm_sample, bk.noise) if self.noise_mode == "table" else (ops.lm_sample_seeded, bk.seeds)
        sample(logits, noise, self.eos_bias, self.tok.eos, self.temperature, self.top_k, bk.step, bk.out, bk.tok,
               bk.pos, bk.lens)

    def _capture(self, bk: _Bucket) -> None:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        saved = [t.clone() for t in bk.state()]
        with torch.cuda.stream(s):
            self._step(bk)
        torch.cuda.current_stream().wait_stream(s)
        for t, v in zip(bk.state(), saved):
            t.copy_(v)
        g = torch.cuda.CUDAGraph()
        with TRACER.capturing(), torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._step(bk)
        for t, v in zip(bk.state(), saved):
            t.copy_(v)
        bk.graph = g

    @torch.no_grad()
    def generate_ids(self, prompt_ids: Sequence[int], min_new: int, max_new: int) -> List[int]:
        if self.noise_mode == "philox":
            return self.generate_ids_batch([prompt_ids], min_new, max_new)[0]
        t_host = time.perf_counter()
        max_new = max(1, min(max_new, self.max_new_cap))
        gen = torch.Generator(device="cpu").manual_seed(self.seed * 1000003 + self.calls)
        u = torch.rand((max_new, 1, self.cfg.vocab), generator=gen).clamp_(1e-10, 1.0 - 1e-7)
        self._bucket(1).noise[:max_new].copy_((-torch.log(-torch.log(u))).to(self.device))
        return self._decode([prompt_ids], min_new, max_new, None, t_host)[0]

    def generate_text(self, prompt: str, min_new_tokens: int, max_new_tokens: int) -> str:
        # rooms call generators from worker threads; the static decode buffers are single-user
        with self._lock:
            ids = self.generate_ids(self.tok.encode(prompt), min_new_tokens, max_new_tokens)
        return self.tok.decode(ids)

    @torch.no_grad()
    def generate_ids_batch(self, prompts: Sequence[Sequence[int]], min_new: int, max_new: int,
                           seeds: Optional[Sequence[int]] = None) -> List[List[int]]:
        """Continuations of up to ``max_batch`` prompts decoded as one batch.  ``seeds``: one
        64-bit seed per sequence (default ``self.seed * 1000003 + call number``, one call number
        per sequence in request order).  Every row is cut at its first EOS."""
        if self.noise_mode != "philox":
            raise ValueError("generate_ids_batch needs noise='philox' (the noise table is batch 1)")
        n = len(prompts)
        if n == 0:
            return []
        if n > self.max_batch:
            raise ValueError(f"{n} sequences exceed max_batch={self.max_batch}")
        if seeds is not None and len(seeds) != n:
            raise ValueError("one seed per sequence")
        return self._decode(prompts, min_new, max_new, seeds, time.perf_counter())

    def _decode(self, prompts, min_new: int, max_new: int, seeds, t_host: float) -> List[List[int]]:
        """The one decode loop: rows and their state set up on the host, one padded prefill, the
        state uploaded, the bucket's step captured once and replayed ``max_new`` times.  ``t_host``:
        when the call began; its host part (``host_ms``) ends before the first launch here."""
        n = len(prompts)
        bk = self._bucket(n)
        B, dev = bk.B, self.device
        max_new = max(1, min(max_new, self.max_new_cap))
        L, bos = self.cfg.max_ctx, self.tok.bos
        # spare rows hold a one-token BOS prompt and are ignored
        rows = [list(p)[-(L - max_new):] or [bos] for p in prompts] + [[bos]] * (B - n)
        if seeds is None:
            seeds = [self.seed * 1000003 + self.calls + i for i in range(n)]
        self.calls += n
        for b, r in enumerate(rows):
            bk.h_tok[b], bk.h_pos[b], bk.h_lens[b] = r[-1], len(r) - 1, len(r)
            s = (int(seeds[b]) if b < n else 0) & 0xFFFFFFFFFFFFFFFF
            bk.h_seeds[b] = s - (1 << 64) if s >= 1 << 63 else s
        eb = torch.zeros((self.max_new_cap,))
        eb[:min(min_new, self.max_new_cap)] = float("-inf")
        Tmax = max(len(r) for r in rows)
        pre = None
        if Tmax > 1:
            # one padded prefill: all but each row's last token, left-aligned, padded with BOS.  A valid
            # position never attends a later (padded) one, the padded cache rows lie at or beyond
            # lens[b] (masked by decode_attention), and decode overwrites pos[b] before lens[b] covers it
            pre = torch.full((B, Tmax - 1), bos, dtype=torch.long)
            for b, r in enumerate(rows):
                pre[b, :len(r) - 1] = torch.tensor(r[:-1], dtype=torch.long)
        self.host_ms = (time.perf_counter() - t_host) * 1e3
        self.eos_bias.copy_(eb.to(dev))
        bk.step.zero_()
        if bk.noise is None:                          # the table sampler reads no seeds
            bk.seeds.copy_(bk.h_seeds, non_blocking=True)
        if pre is not None:
            bk.pos.zero_()
            self.model(pre.to(dev), bk.kc, bk.vc, bk.pos, None, decode=False)
        bk.pos.copy_(bk.h_pos, non_blocking=True)
        bk.lens.copy_(bk.h_lens, non_blocking=True)
        bk.tok.copy_(bk.h_tok, non_blocking=True)
        if self.use_graphs and bk.graph is None:
            self._capture(bk)
        for _ in range(max_new):
            if bk.graph is not None:
                bk.graph.replay()
            else:
                self._step(bk)
        out = bk.out[:max_new, :n].t().tolist()       # the one sync; also orders the pinned rows' reuse
        eos = self.tok.eos
        return [r[:r.index(eos)] if eos in r else r for r in out]

    def generate_texts(self, prompts: Sequence[str], min_new_tokens: int, max_new_tokens: int) -> List[str]:
        with self._lock:
            ids = self.generate_ids_batch([self.tok.encode(p) for p in prompts], min_new_tokens, max_new_tokens)
        return [self.tok.decode(r) for r in ids]
