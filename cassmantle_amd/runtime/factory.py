"""Wiring: config -> GameService with the right scorer and image generator for this host.

* GPU present: on-device SD pipeline (``pipeline.DiffusionImageGenerator``) and the batched
  GPU scorer (MiniLM encoder or word-vector table, ``scoring``).
* CPU only (tests, dev): placeholder images, CPU scorer.
* Multi-GPU serving (``torchrun``): rank 0 builds the service with
  ``parallel.rooms.RankImageGenerator`` so each room's images come from its owner rank.
"""
from __future__ import annotations

import contextlib
import os

from typing import Callable, Optional, Sequence

import numpy as np
import torch

from ..config import Config
from ..game.content import BatchingImageGenerator, ImageGenerator, SolidImageGenerator
from ..game.service import GameService
from ..scoring.batcher import BatchingScorer


_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}


def model_dtype(cfg: Config, device: str) -> torch.dtype:
    """``ModelConfig.dtype``: the HIP kernels are bf16-only; fp32 selects the CPU reference path
    (tests / parity) and is rejected on a GPU rather than silently ignored."""
    dt = _DTYPES.get(cfg.model.dtype.lower())
    if dt is None:
        raise ValueError(f"dtype={cfg.model.dtype!r}: expected bf16 or fp32")
    if dt != torch.bfloat16 and str(device).startswith("cuda"):
        raise ValueError("dtype=fp32 runs only on the CPU reference path; the GPU kernels are bf16")
    return dt


_STREAMS: dict = {}


def reserved_streams(cfg: Config, device: str):
    """(scorer stream, generation stream) with ``scorer_reserved_cus`` CUs for the scorer, one
    pair per device and process; (None, None) when no reservation is configured."""
    n = cfg.model.scorer_reserved_cus
    if n <= 0 or not str(device).startswith("cuda"):
        return None, None
    key = (str(device), n)
    if key not in _STREAMS:
        from .cumask import reserved_streams as _rs
        _STREAMS[key] = _rs(device, n)
    return _STREAMS[key]


def build_scorer(cfg: Config, device: Optional[str] = None, wrap=None):
    """MiniLM-encoder (or word-vector) backend behind the micro-batching scorer.  ``wrap`` maps
    the local backend to the one the scorer calls (multi-GPU: ``parallel.scoring.ShardedSimilarity``)."""
    dev = device or ("cuda" if torch.cuda.is_available() else "cpu")
    if cfg.model.scorer == "wordvec":
        from ..scoring.wordvec import WordVectorBackend
        backend = WordVectorBackend(device=dev, dtype=torch.bfloat16 if dev.startswith("cuda") else torch.float32)
    else:
        from ..scoring.encoder import EncoderBackend
        # high-priority stream: guess scoring is dispatched ahead of queued denoise kernels (the
        # supervised front-end sets cfg.model.scorer_stream_priority = 0, serve._serve_supervised)
        prio = cfg.model.scorer_stream_priority
        prio = (-1 if prio is None else prio) if dev.startswith("cuda") else None
        backend = EncoderBackend(device=dev, stream_priority=prio,
                                 dtype=model_dtype(cfg, dev), stream=reserved_streams(cfg, dev)[0])
        if cfg.model.scorer_weights:
            from ..models.weights import load_bert, read_safetensors
            missing = load_bert(backend.model, read_safetensors(cfg.model.scorer_weights))
            if missing:
                raise KeyError(f"scorer_weights: {len(missing)} tensors missing, e.g. {missing[:3]}")
    if wrap is not None:
        backend = wrap(backend)
    return BatchingScorer(backend, cfg.game.min_score, window_ms=cfg.model.scorer_batch_window_ms)


def blur_kernel(cfg: Config) -> str:
    """``ModelConfig.blur_kernel``: gaussian (ops.gaussian_blur) | pil (ops.gaussian_blur_pil, the
    bytes of PIL's GaussianBlur); anything else is an error, not the default."""
    k = str(cfg.model.blur_kernel).lower()
    if k not in ("gaussian", "pil"):
        raise ValueError(f"blur_kernel={cfg.model.blur_kernel!r}: expected gaussian or pil")
    return k


def jpeg_restart(cfg: Config, width: int):
    """``(restart_mcus, entropy)`` for ops.jpeg_encode of an image ``width`` pixels wide, from
    ``ModelConfig.jpeg_restart_mcus`` (0: one MCU row of the 4:2:0 encode, -1: no restart markers,
    else that many MCUs) and ``ModelConfig.jpeg_entropy`` (interval | block).  An unknown coder is
    an error, not the default, and so is -1 with the interval coder, which cannot write it."""
    entropy = str(cfg.model.jpeg_entropy).lower()
    if entropy not in ("interval", "block"):
        raise ValueError(f"jpeg_entropy={cfg.model.jpeg_entropy!r}: expected interval or block")
    r = int(cfg.model.jpeg_restart_mcus)
    if r < -1:
        raise ValueError(f"jpeg_restart_mcus={r}: expected -1 (no restart markers), 0 (one MCU row) or a count")
    if r == -1:
        if entropy != "block":
            raise ValueError("jpeg_restart_mcus=-1 (no restart markers) needs jpeg_entropy=block")
        return 0, entropy
    return r or (int(width) + 15) // 16, entropy


def jpeg_huffman(cfg: Config) -> str:
    """``ModelConfig.jpeg_huffman`` (standard | optimized) for ops.jpeg_encode; an unknown value is
    an error, not the default."""
    h = str(cfg.model.jpeg_huffman).lower()
    if h not in ("standard", "optimized"):
        raise ValueError(f"jpeg_huffman={cfg.model.jpeg_huffman!r}: expected standard or optimized")
    return h


def jpeg_transform(cfg: Config) -> str:
    """``ModelConfig.jpeg_transform`` (matrix | libjpeg) for ops.jpeg_encode; an unknown value is
    an error, not the default."""
    t = str(cfg.model.jpeg_transform).lower()
    if t not in ("matrix", "libjpeg"):
        raise ValueError(f"jpeg_transform={cfg.model.jpeg_transform!r}: expected matrix or libjpeg")
    return t


def _jpeg_encode_args(cfg: Config, width: int) -> dict:
    """jpeg_restart, jpeg_huffman and jpeg_transform as keyword arguments of ops.jpeg_encode; the
    default coder, tables and transform are not named, so the default configuration makes the call
    it always made."""
    restart, entropy = jpeg_restart(cfg, width)
    kw = {"restart_mcus": restart} if entropy == "interval" else {"restart_mcus": restart, "entropy": entropy}
    huffman = jpeg_huffman(cfg)
    if huffman != "standard":
        kw["huffman"] = huffman
    transform = jpeg_transform(cfg)
    if transform != "matrix":
        kw["transform"] = transform
    return kw


def _device_pixels(img, dev: str) -> torch.Tensor:
    """The pixels of ``img`` on ``dev``: a DeviceImage is already in this GPU's HBM, anything else
    (an array, a PIL decode) is uploaded."""
    t = getattr(img, "tensor", None)
    if t is not None and t.device.type == "cuda":
        return t.to(dev, non_blocking=False)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(img))).to(dev, non_blocking=False)


def build_blur_fn(cfg: Config, device: Optional[str] = None):
    """The /fetch/contents blur (``mask_image``, ``src/backend.py:322-324``) on the GPU: the HIP
    LDS-tiled Gaussian (ops.gaussian_blur) on its own stream, or with ``blur_kernel=pil`` PIL's own
    GaussianBlur bit for bit (ops.gaussian_blur_pil).  ``None`` -> PIL on the CPU."""
    dev = device or ("cuda" if torch.cuda.is_available() else "cpu")
    kernel = blur_kernel(cfg)
    if not cfg.model.gpu_blur or not dev.startswith("cuda"):
        return None
    from .. import ops
    if kernel == "pil":
        def blur_exact(img, radius: float):
            return ops.gaussian_blur_pil(_device_pixels(img, dev), float(radius)).cpu().numpy()
        return blur_exact
    # the blur runs on the calling thread's current stream: a stream of its own in a process that
    # shares its GPU with a generation worker cost that worker 14 % of its images/s
    # (profiles/r6_live_ipc_stream_ab.txt); CASSMANTLE_BLUR_STREAM=own restores one
    stream = torch.cuda.Stream(device=dev) if os.environ.get("CASSMANTLE_BLUR_STREAM") == "own" else None

    def blur(img, radius: float):
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            t = getattr(img, "tensor", None)        # DeviceImage: already in this GPU's HBM
            if t is not None and t.device.type == "cuda":
                x = t.to(dev, non_blocking=False)
            else:
                x = torch.from_numpy(np.ascontiguousarray(np.asarray(img))).to(dev, non_blocking=False)
            y = ops.gaussian_blur(x, radius)
            return y.cpu().numpy()
    return blur


def build_blur_jpeg_fn(cfg: Config, device: Optional[str] = None):
    """Blur + JPEG of a whole set of radii on the GPU (``gpu_jpeg``): ``fn(img, radii, quality)
    -> [bytes]``.  Each radius is blurred by ops.gaussian_blur into one ``[len(radii), H, W, 3]``
    buffer (``blur_kernel=pil``: ONE ops.gaussian_blur_pil call is that buffer), which one
    ops.jpeg_encode call encodes: the entropy-coded bytes cross to the host,
    not the pixels.  Everything runs on the calling thread's current stream (see build_blur_fn).
    ``None`` unless ``gpu_jpeg`` and ``gpu_blur`` are set and the device is a GPU."""
    dev = device or ("cuda" if torch.cuda.is_available() else "cpu")
    kernel = blur_kernel(cfg)
    if not (cfg.model.gpu_jpeg and cfg.model.gpu_blur) or not str(dev).startswith("cuda"):
        return None
    from .. import ops
    jpeg_restart(cfg, 16)                   # a bad jpeg_entropy / jpeg_restart_mcus raises here, not per request
    jpeg_huffman(cfg)                       # and so does a bad jpeg_huffman
    jpeg_transform(cfg)                     # or a bad jpeg_transform
    if kernel == "pil":
        def blur_jpeg_exact(img, radii: Sequence[float], quality: int):
            x = _device_pixels(img, dev)
            buf = ops.gaussian_blur_pil(x, [float(r) for r in radii])      # ONE launch: [len(radii), H, W, 3]
            return ops.jpeg_encode(buf, quality=quality, **_jpeg_encode_args(cfg, x.shape[1]))
        return blur_jpeg_exact

    def blur_jpeg(img, radii: Sequence[float], quality: int):
        t = getattr(img, "tensor", None)        # DeviceImage: already in this GPU's HBM
        if t is not None and t.device.type == "cuda":
            x = t.to(dev, non_blocking=False)
        else:
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(img))).to(dev, non_blocking=False)
        x = x.contiguous()
        buf = torch.empty((len(radii), *x.shape), device=x.device, dtype=torch.uint8)
        for i, r in enumerate(radii):
            ops.copy_(buf[i], ops.gaussian_blur(x, float(r)))
        return ops.jpeg_encode(buf, quality=quality, **_jpeg_encode_args(cfg, x.shape[1]))
    return blur_jpeg


def build_content_jpeg_fn(cfg: Config, device: Optional[str] = None):
    """The content JPEG of a device-resident image made on the GPU (``gpu_jpeg_content``):
    ``fn(image, quality) -> (jpeg bytes, DeviceImage of the decoded pixels)``.  One
    ops.jpeg_encode call with ``return_decoded``: the bytes cross to the host, the pixels a
    decoder gives for them stay in HBM and become the blur source, so a front-end that has only
    the stored bytes (PIL decode) blurs the same pixels.  The restart rule is build_blur_jpeg_fn's;
    everything runs on the calling thread's current stream.  ``None`` unless ``gpu_jpeg_content``,
    ``gpu_jpeg`` and ``gpu_blur`` are set and the device is a GPU."""
    dev = device or ("cuda" if torch.cuda.is_available() else "cpu")
    m = cfg.model
    if not (m.gpu_jpeg_content and m.gpu_jpeg and m.gpu_blur) or not str(dev).startswith("cuda"):
        return None
    from .. import ops
    from ..game.content import DeviceImage
    jpeg_restart(cfg, 16)                   # a bad jpeg_entropy / jpeg_restart_mcus raises here, not per request
    jpeg_huffman(cfg)                       # and so does a bad jpeg_huffman
    jpeg_transform(cfg)                     # or a bad jpeg_transform

    def content_jpeg(img, quality: int):
        x = img.tensor.to(dev, non_blocking=False)
        outs, decoded = ops.jpeg_encode(x, quality=quality, return_decoded=True, **_jpeg_encode_args(cfg, x.shape[1]))
        return outs[0], DeviceImage(decoded[0])
    return content_jpeg


def build_jpeg_decode_fn(cfg: Config, device: Optional[str] = None):
    """Stored JPEG bytes -> their decoded pixels in HBM (``gpu_jpeg_decode``): ``fn(jpeg) ->
    DeviceImage``, one ops.jpeg_decode call on the calling thread's current stream, PIL's pixels
    bit for bit.  ``fn`` returns ``None``, which leaves the stream to PIL on the host as without
    the flag, for a stream with fewer than ``jpeg_decode_min_intervals`` restart intervals and for
    bytes the decoder refuses (outside its scope, or malformed).  With ``jpeg_decode_chunked`` a
    stream under that interval count is decoded too, in chunks of ``jpeg_decode_chunk_bytes``
    (``mode="chunked"``), and only a refused one returns ``None``.  ``None`` unless
    ``gpu_jpeg_decode`` and ``gpu_blur`` are set and the device is a GPU."""
    dev = device or ("cuda" if torch.cuda.is_available() else "cpu")
    m = cfg.model
    if not (m.gpu_jpeg_decode and m.gpu_blur) or not str(dev).startswith("cuda"):
        return None
    from .. import ops
    from ..game.content import DeviceImage
    from ..ops import jpeg_format as jf

    def jpeg_decode(jpeg: bytes):
        try:
            stream = jf.parse(jpeg)
            if len(stream.intervals) < m.jpeg_decode_min_intervals:
                if not m.jpeg_decode_chunked:
                    return None
                return DeviceImage(ops.jpeg_decode(stream, device=dev, mode="chunked",
                                                   chunk_bytes=m.jpeg_decode_chunk_bytes))
            return DeviceImage(ops.jpeg_decode(stream, device=dev))
        except (jf.JpegUnsupported, jf.JpegError):
            return None
    return jpeg_decode


def build_prompt_generator(cfg: Config, device: Optional[str] = None):
    """synthetic (default, template grammar) | lm (local causal LM, models/lm.py) | remote
    (HF text-generation endpoint, reference parity).  ``None`` -> per-room synthetic."""
    m = cfg.model
    if m.prompt_generator == "lm":
        from ..game.prompts import BatchingPromptGenerator, LMPromptGenerator
        from ..models.lm import LM_CONFIGS, LM_NOISE, LM_WEIGHT_DTYPES, LMTextGenerator, SentencePieceTokenizer
        # bad LM flags raise here, not at the first round
        if m.lm_noise not in LM_NOISE:
            raise ValueError(f"unknown lm_noise {m.lm_noise!r}: one of {', '.join(LM_NOISE)}")
        if not 1 <= int(m.lm_batch_max) <= 8:
            raise ValueError(f"lm_batch_max must be 1..8, not {m.lm_batch_max}")
        if m.lm_batch_max > 1 and m.lm_noise != "philox":
            raise ValueError("lm_batch_max > 1 needs lm_noise=philox (the noise table is batch 1)")
        if m.lm_weight_dtype not in LM_WEIGHT_DTYPES:
            raise ValueError(f"unknown lm_weight_dtype {m.lm_weight_dtype!r}: one of {', '.join(LM_WEIGHT_DTYPES)}")
        tok = SentencePieceTokenizer(m.lm_tokenizer) if m.lm_tokenizer else None
        # a checkpoint loads into the bf16 projections; they are quantised after it
        gen = LMTextGenerator(LM_CONFIGS[m.lm_model], device=device, seed=m.seed, use_graphs=m.use_graphs,
                              tokenizer=tok, noise=m.lm_noise, max_batch=int(m.lm_batch_max),
                              weight_dtype="bf16" if m.lm_weights else m.lm_weight_dtype)
        if m.lm_weights:
            from ..models.weights import load_causal_lm, read_safetensors
            load_causal_lm(gen.model, read_safetensors(m.lm_weights))
            if m.lm_weight_dtype == "fp8":
                gen.quantize_fp8()
        pg = LMPromptGenerator(gen)
        if m.lm_batch_max > 1:
            # the rooms of this process ask at the same moment of the shared round clock: one LM batch
            return BatchingPromptGenerator(pg, max_batch=int(m.lm_batch_max),
                                           window_s=m.lm_batch_window_ms / 1e3 if cfg.game.num_rooms > 1 else 0.0)
        return pg
    if m.prompt_generator == "remote":
        if not m.remote_prompt_url:
            raise ValueError("prompt_generator=remote needs remote_prompt_url")
        from .remote import RemotePromptGenerator
        return RemotePromptGenerator(m.remote_prompt_url, token=m.remote_token, timeout_s=m.remote_timeout_s,
                                     max_retries=cfg.game.max_retries, retry_unit_s=m.remote_retry_s)
    return None


def build_image_generator(cfg: Config, device: Optional[str] = None) -> ImageGenerator:
    m = cfg.model
    from ..models.schedulers import check_scheduler
    check_scheduler(m.scheduler)            # a bad ModelConfig.scheduler raises here, not at the first round
    use_gpu = (m.device == "cuda") or (m.device == "auto" and torch.cuda.is_available())
    if m.image_model == "remote":
        if not m.remote_image_url:
            raise ValueError("image_model=remote needs remote_image_url")
        from .remote import RemoteImageGenerator
        return RemoteImageGenerator(m.remote_image_url, resolution=m.resolution, token=m.remote_token,
                                    timeout_s=m.remote_timeout_s, max_retries=cfg.game.max_retries,
                                    retry_unit_s=m.remote_retry_s)
    if m.image_model == "solid" or not use_gpu:
        return SolidImageGenerator(resolution=min(m.resolution, 256))
    from ..pipeline import DiffusionImageGenerator
    dev = device or "cuda"
    return DiffusionImageGenerator(m.image_model, device=dev, steps=m.steps,
                                   guidance=m.guidance_scale, scheduler=m.scheduler,
                                   use_graphs=m.use_graphs, fp8_attention=m.fp8_attention, seed=m.seed,
                                   dtype=model_dtype(cfg, dev), weights_path=m.weights_path,
                                   stream=reserved_streams(cfg, dev)[1])


def build_service(cfg: Config, image_gen_for_room: Optional[Callable[[str], ImageGenerator]] = None,
                  scorer=None, **kw) -> GameService:
    scorer = scorer if scorer is not None else build_scorer(cfg)
    if image_gen_for_room is None:
        # one device pipeline shared by every room: requests are serialised and batched
        gen = BatchingImageGenerator(build_image_generator(cfg), max_batch=cfg.model.gen_batch_max,
                                     window_s=cfg.model.gen_batch_window_ms / 1e3 if cfg.game.num_rooms > 1 else 0.0)
        image_gen_for_room = lambda rid: gen  # noqa: E731
    if "prompt_gen" not in kw:
        kw["prompt_gen"] = build_prompt_generator(cfg)
    if "blur_fn" not in kw:
        kw["blur_fn"] = build_blur_fn(cfg)
    if "blur_jpeg_fn" not in kw:
        kw["blur_jpeg_fn"] = build_blur_jpeg_fn(cfg)
    if "content_jpeg_fn" not in kw:
        kw["content_jpeg_fn"] = build_content_jpeg_fn(cfg)
    if "decode_fn" not in kw:
        kw["decode_fn"] = build_jpeg_decode_fn(cfg)
    return GameService(cfg, scorer, image_gen_for_room=image_gen_for_room, **kw)
