"""One blur-cache prewarm (61 buckets: max_blur 15, blur_bucket 0.25) of a device-resident image,
the parent's path against ``gpu_jpeg``:

* parent: per bucket a HIP blur, the uint8 image copied to the host, PIL ``save(format="JPEG")``;
* gpu_jpeg: 60 HIP blurs into one buffer, one ``ops.jpeg_encode`` (ops/csrc/jpeg.hip), the
  entropy-coded bytes copied to the host.

Per resolution (512, 1024; the image is media/background.png resized): the two paths interleaved
``--reps`` times after a warm-up of each, then a sweep of ``jpeg_restart_mcus``.  Each record is
one JSON line: host wall time, front-end CPU time (``time.process_time``), bytes moved device to
host (counted from shapes / output sizes), and for the new path the encode kernels' device time
(HIP events around the two launch groups of a stand-alone encode of the same blurred batch).

    python tools/bench_jpeg.py [--res 512 1024] [--reps 2] [--out profiles/jpeg_prewarm.jsonl]

``--content`` measures the step before the prewarm instead, the content JPEG of one new
device-resident image (``GameRoom._make_content``), the parent's path against ``gpu_jpeg_content``:

* parent: the image copied to the host (``DeviceImage.host()``), PIL ``save(format="JPEG")``;
* gpu_jpeg_content: one ``ops.jpeg_encode(..., return_decoded=True)``: the JPEG bytes copied to
  the host, the decoded pixels (the blur source) left in HBM; timed to the end of its kernels.

Per record: host wall time, front-end CPU time, bytes moved device to host, the JPEG's size, the
PSNR of its decoded pixels against the original, and for the new path the device time of the idct
+ colour kernels (HIP events around a stand-alone ``jpeg_reconstruct``) and whether the device's
decoded pixels equal PIL's decode of the bytes.

    python tools/bench_jpeg.py --content [--res 512 1024] [--reps 2] [--out profiles/jpeg_content.jsonl]

``--blur-kernel pil`` runs the prewarm comparison with a third row, ``gpu_jpeg`` + ``blur_kernel=pil``
(one batched ops.gaussian_blur_pil launch, ops/csrc/blur_pil.hip, instead of 60 Gaussian
launches and 60 copies), the three paths interleaved ``--reps`` times after a warm-up of each.  It also records the device time of
the blur stage alone (HIP events around the 60 Gaussian launches + copies, and around the one
batched launch) and whether the batched blur equals Pillow's GaussianBlur on this image.

    python tools/bench_jpeg.py --blur-kernel pil [--res 512 1024] [--reps 2] [--out profiles/blur_pil_prewarm.jsonl]

``--decode`` measures what a blur cache does for a content version it holds only the stored bytes
of: the parent's path (PIL ``decode_jpeg`` on the host, then the upload of the full-resolution
pixels) against ``ops.jpeg_decode`` (``gpu_jpeg_decode``: the entropy-coded bytes are uploaded and
decoded in HBM), each timed to a device synchronise, interleaved ``--reps`` times after a warm-up
of each.  Streams: the GPU encoder's content JPEG at one MCU row, 16 and 4 MCUs per restart
interval, and a PIL-encoded stream without restart markers (one lane decodes the whole image).
Per record: host wall time, CPU time, bytes moved host to device, and per stream the device time
(HIP events) of the zero + entropy decode launch and of the zero alone.  The same streams again
through ``ops.jpeg_decode(mode="chunked")`` (``jpeg_decode_chunked``) at 16, 32, 64 and 128 bytes
per chunk, with the rounds and chunks of every call and the device time of the chunked launch
alone; and one more image, the worst case of that path: 512 x 512 noise (``tests/jpeg_cases.py``),
PIL-encoded at quality 75 without restart markers.

    python tools/bench_jpeg.py --decode [--res 512 1024] [--reps 2] [--out profiles/jpeg_decode.jsonl]

``--entropy block`` compares the two entropy coders of ``ops.jpeg_encode`` in the prewarm (default)
or the ``--content`` mode: per ``--jpeg_restart_mcus`` setting (0: one MCU row, N: N MCUs, -1: no
restart markers) the block-parallel coder (``jpeg_entropy=block``) against the interval coder at the
same setting (for -1, which the interval coder cannot write, against its one-MCU-row default), with
``blur_kernel=pil``, all rows interleaved ``--reps`` times after a warm-up of each; ``--content``
adds the parent's ``.cpu()`` + PIL encode.  Per record: host wall time, CPU time, JPEG bytes, the
block coder's device memory (allocated / zeroed per call), and the device time (HIP events,
nothing else queued) of the encode's two launch groups on the same pixels: count phase (transform,
the same kernel for both coders, + everything up to the image offsets) and write phase.

    python tools/bench_jpeg.py --entropy block [--content] [--jpeg_restart_mcus 0 4 -1] [--out profiles/jpeg_block.jsonl]

``--huffman optimized`` compares ``jpeg_huffman=optimized`` (every image's own Huffman tables, built
on the device) against the standard tables in the prewarm (default, with ``--blur-kernel pil`` for
that blur) or the ``--content`` mode, for both entropy coders (interval at one MCU row, block
without restart markers), standard and optimised rows interleaved ``--reps`` times after a warm-up
of each; the yardstick is the standard row of the same run.  Per record: host wall time, CPU time,
JPEG bytes; then per coder the device time (HIP events, nothing else queued) of the count phase
with both tables: their difference is the histogram + table build (and the count pass reading an
image's own table).

    python tools/bench_jpeg.py --huffman optimized [--blur-kernel pil] [--content] [--out profiles/jpeg_huffman.jsonl]

``--transform libjpeg`` compares ``jpeg_transform=libjpeg`` (libjpeg's forward transform and header
layout: PIL's file, byte for byte) against the matrix transform in the prewarm (default) or the
``--content`` mode, both with ``blur_kernel=pil``, ``jpeg_entropy=block`` and no restart markers,
matrix and libjpeg rows interleaved ``--reps`` times after a warm-up of each; the yardstick is the
matrix row of the same run.  Per record: host wall time, CPU time, JPEG bytes, the bytes of the
parent's PIL path for the same pixels and whether the stream equals them; then the device time (HIP
events, nothing else queued) of the count phase with both transforms.

    python tools/bench_jpeg.py --transform libjpeg [--content] [--out profiles/jpeg_libjpeg.jsonl]
"""
import argparse
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_BLUR, BUCKET, QUALITY = 15.0, 0.25, 75
CHUNKS = (16, 32, 64, 128)        # --decode: the chunk sizes of the chunked entropy decode rows


def source_image(res: int):
    import numpy as np
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    img = Image.open(os.path.join(root, "cassmantle_amd", "media", "background.png")).convert("RGB")
    return np.asarray(img.resize((res, res), Image.LANCZOS))


def prewarm_once(blur_fn, blur_jpeg_fn, dimg, jpeg, tag):
    import torch
    from cassmantle_amd.game.imaging import BlurCache
    cache = BlurCache(blur_fn=blur_fn, bucket=BUCKET, quality=QUALITY, blur_jpeg_fn=blur_jpeg_fn)
    cache.set_source(tag, dimg)
    torch.cuda.synchronize()
    w0, c0 = time.perf_counter(), time.process_time()
    n = cache.prewarm(tag, jpeg, MAX_BLUR)
    wall, cpu = time.perf_counter() - w0, time.process_time() - c0
    with cache._lock:
        outs = {r: v for (_, r), v in cache._lru.items()}
    return n, wall, cpu, outs


def encode_layout(B: int, H: int, W: int, restart: int, block: bool = False, optimized: bool = False,
                  transform: str = "matrix") -> dict:
    """The buffer layout (ops/csrc/jpeg_layout.h) of an encode of this file's settings."""
    from cassmantle_amd.ops import jpeg_format as jf
    from cassmantle_amd.ops._ext import ext
    lj, layout = transform == "libjpeg", jf.transform_layout(transform)
    hdr = sum(len(p) for p in jf.header_parts(H, W, QUALITY, "420", restart, layout)) if optimized \
        else len(jf.header(H, W, QUALITY, "420", restart, None, layout))
    return ext().jpeg_encode_layout(B, H, W, True, restart, block, optimized, lj, hdr)


def encode_args(batch, restart: int, block: bool = False, optimized: bool = False, transform: str = "matrix"):
    """(layout, the arguments of ext().jpeg_count; jpeg_write takes out and the payload size behind
    them) for ``batch``, buffers allocated as ops.jpeg_encode does."""
    import torch
    from cassmantle_amd import ops
    from cassmantle_amd.ops import jpeg_format as jf
    B, H, W, _ = batch.shape
    lay = encode_layout(B, H, W, restart, block, optimized, transform)
    tables, header, split = ops._jpeg_plan(batch.device, H, W, QUALITY, "420", restart, jf.transform_layout(transform),
                                           optimized)

    def buf(name, dtype=torch.int32):
        return torch.empty(lay[name], device="cuda", dtype=dtype)
    blk, scratch = (buf("blk"), buf("scratch")) if block else (None, None)
    hopt, hdrs = (buf("hopt"), buf("hdrs", torch.uint8)) if optimized else (None, None)
    return lay, (batch, tables, header, buf("coef", torch.int16), buf("work"), 1, restart, int(transform == "libjpeg"),
                 blk, scratch, hopt, hdrs, split)


def encode_device_ms(batch, restart: int, iters: int = 5, block: bool = False):
    """Device time of the two launch groups of ops.jpeg_encode on ``batch`` (HIP events; nothing
    else is queued): (transform + count + scans, write + headers) in ms."""
    import torch
    from cassmantle_amd.ops._ext import ext
    B = batch.shape[0]
    lay, args = encode_args(batch, restart, block)
    work = args[4]
    best = [1e9, 1e9]
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        ext().jpeg_count(*args)
        ev[1].record()
        total = int(work[B].item())
        out = torch.empty(total + lay["slack"], device="cuda", dtype=torch.uint8)
        torch.cuda.synchronize()
        ev[2].record()
        ext().jpeg_write(*args, out, total)
        ev[3].record()
        torch.cuda.synchronize()
        best = [min(best[0], ev[0].elapsed_time(ev[1])), min(best[1], ev[2].elapsed_time(ev[3]))]
    return best


def block_buffers(B: int, H: int, W: int, restart: int):
    """(nint, stride, bytes allocated, bytes zeroed per call) of the block coder's device memory
    beyond coefficients and payload; ``restart`` 0 = no restart markers."""
    lay = encode_layout(B, H, W, restart, block=True)
    return lay["nint"], lay["stride"], 4 * (lay["scratch"] + lay["blk"] + 1), 4 * lay["blk"] + 4 + 1


def encode_blocks_device_ms(batch, restart: int, iters: int = 5):
    """encode_device_ms for ``entropy="block"`` (``restart`` 0 = no restart markers): (transform +
    bits + scan + pack + piece counts + scans, stuffed write + headers) in ms."""
    return encode_device_ms(batch, restart, iters, block=True)


def block_main(a, emit) -> int:
    """--entropy block: the block-parallel coder against the interval coder (see the module text)."""
    import numpy as np
    import torch
    from cassmantle_amd import ops
    from cassmantle_amd.config import Config
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.game.imaging import encode_jpeg
    from cassmantle_amd.runtime.factory import build_blur_fn, build_blur_jpeg_fn, build_content_jpeg_fn, jpeg_restart

    def config(entropy, setting):
        c = Config()
        c.model.gpu_jpeg = c.model.gpu_jpeg_content = True
        c.model.blur_kernel = "pil"
        c.model.jpeg_entropy, c.model.jpeg_restart_mcus = entropy, setting
        return c

    for res in a.res:
        img = source_image(res).copy()
        jpeg = encode_jpeg(img, QUALITY)
        dimg = DeviceImage(torch.from_numpy(img).cuda())
        dimg.host()
        blur_fn = build_blur_fn(config("interval", 0), "cuda")
        radii = [i * BUCKET for i in range(1, int(MAX_BLUR / BUCKET) + 1)]
        # rows: (entropy, setting, the yardstick's setting); the interval coder has no -1
        rows = []
        for setting in a.jpeg_restart_mcus:
            yard = ("interval", setting if setting >= 0 else 0)
            if yard not in rows:
                rows.append(yard)
            rows.append(("block", setting))
        pixels = dimg.tensor[None].contiguous() if a.content else ops.gaussian_blur_pil(dimg.tensor, radii)

        def run(entropy, setting, tag):
            cfg = config(entropy, setting)
            restart, _ = jpeg_restart(cfg, res)
            rec = {"res": res, "mode": "content" if a.content else "prewarm", "entropy": entropy,
                   "jpeg_restart_mcus": setting, "restart_mcus": restart}
            if a.content:
                fn = build_content_jpeg_fn(cfg, "cuda")
                d = DeviceImage(dimg.tensor)
                torch.cuda.synchronize()
                w0, c0 = time.perf_counter(), time.process_time()
                data, _ = fn(d, QUALITY)
                torch.cuda.synchronize()
                wall, cpu = time.perf_counter() - w0, time.process_time() - c0
                size, outs = len(data), [data]
            else:
                n, wall, cpu, got = prewarm_once(blur_fn, build_blur_jpeg_fn(cfg, "cuda"), dimg, jpeg, tag)
                outs = [v for r, v in sorted(got.items()) if r > 0]
                size = sum(len(v) for v in outs)
                rec["buckets"] = n
            rec.update(wall_ms=round(wall * 1e3, 3), cpu_ms=round(cpu * 1e3, 3), jpeg_bytes=size)
            return rec, outs

        def run_parent():
            d = DeviceImage(dimg.tensor)                # fresh: no cached host copy
            torch.cuda.synchronize()
            w0, c0 = time.perf_counter(), time.process_time()
            data = encode_jpeg(d, QUALITY)
            wall, cpu = time.perf_counter() - w0, time.process_time() - c0
            return {"res": res, "mode": "content", "entropy": "parent (.cpu() + PIL)", "wall_ms": round(wall * 1e3, 3),
                    "cpu_ms": round(cpu * 1e3, 3), "jpeg_bytes": len(data)}

        equal = {}
        for entropy, setting in rows:                   # warm-up, and the bytes once
            _, outs = run(entropy, setting, f"warm-{entropy}-{setting}")
            restart, _ = jpeg_restart(config(entropy, setting), res)
            if entropy == "block":
                cpu_pixels = pixels[:1].cpu().numpy()        # the numpy reference takes seconds per image
                equal[setting] = outs[:1] == ops.reference.jpeg_encode(cpu_pixels, QUALITY, "420", restart)
        if a.content:
            run_parent()
        for rep in range(a.reps):
            if a.content:
                emit(dict(run_parent(), rep=rep))
            for entropy, setting in rows:
                rec, _ = run(entropy, setting, f"{entropy}-{setting}-{rep}")
                if entropy == "block":
                    rec["first_image_equals_reference"] = bool(equal[setting])
                emit(dict(rec, rep=rep))
        for entropy, setting in rows:                   # device time of the two launch groups
            restart, _ = jpeg_restart(config(entropy, setting), res)
            rec = {"res": res, "mode": "content" if a.content else "prewarm", "entropy": entropy,
                   "jpeg_restart_mcus": setting, "restart_mcus": restart, "images": int(pixels.shape[0])}
            if entropy == "block":
                cnt, wr = encode_blocks_device_ms(pixels, restart)
                _, _, alloc, zeroed = block_buffers(pixels.shape[0], res, res, restart)
                rec.update(scratch_bytes_allocated=alloc, scratch_bytes_zeroed=zeroed)
            else:
                cnt, wr = encode_device_ms(pixels, restart)
                nint = encode_layout(pixels.shape[0], res, res, restart)["nint"]
                rec.update(scratch_bytes_allocated=8 * pixels.shape[0] * nint, scratch_bytes_zeroed=0)
            emit(dict(rec, count_phase_device_ms=round(cnt, 4), write_phase_device_ms=round(wr, 4)))
    return 0


def count_phase_device_ms(batch, restart: int, entropy: str, optimized: bool, iters: int = 5,
                          transform: str = "matrix") -> float:
    """Device time (HIP events; nothing else is queued) of the count phase of ops.jpeg_encode on
    ``batch``: transform (+ histogram + table build with ``optimized``) + the coder's count pass +
    scans, in ms; ``restart`` 0 = no restart markers (block coder)."""
    import torch
    from cassmantle_amd.ops._ext import ext
    _, args = encode_args(batch, restart, entropy == "block", optimized, transform)
    best = 1e9
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        ext().jpeg_count(*args)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def huffman_main(a, emit) -> int:
    """--huffman optimized: the image's own Huffman tables against the standard ones (see the module text)."""
    import torch
    from cassmantle_amd import ops
    from cassmantle_amd.config import Config
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.game.imaging import encode_jpeg
    from cassmantle_amd.runtime.factory import build_blur_fn, build_blur_jpeg_fn, build_content_jpeg_fn, jpeg_restart

    def config(entropy, huffman):
        c = Config()
        c.model.gpu_jpeg = c.model.gpu_jpeg_content = True
        if a.blur_kernel:
            c.model.blur_kernel = a.blur_kernel
        c.model.jpeg_entropy, c.model.jpeg_restart_mcus = entropy, (-1 if entropy == "block" else 0)
        c.model.jpeg_huffman = huffman
        return c

    rows = [(e, h) for e in ("interval", "block") for h in ("standard", a.huffman)]
    for res in a.res:
        img = source_image(res).copy()
        jpeg = encode_jpeg(img, QUALITY)
        dimg = DeviceImage(torch.from_numpy(img).cuda())
        dimg.host()
        blur_fn = build_blur_fn(config("interval", "standard"), "cuda")
        radii = [i * BUCKET for i in range(1, int(MAX_BLUR / BUCKET) + 1)]
        mode = "content" if a.content else "prewarm"

        def run(entropy, huffman, tag):
            cfg = config(entropy, huffman)
            rec = {"res": res, "mode": mode, "blur_kernel": cfg.model.blur_kernel, "entropy": entropy, "huffman": huffman,
                   "restart_mcus": jpeg_restart(cfg, res)[0]}
            if a.content:
                fn = build_content_jpeg_fn(cfg, "cuda")
                d = DeviceImage(dimg.tensor)
                torch.cuda.synchronize()
                w0, c0 = time.perf_counter(), time.process_time()
                data, _ = fn(d, QUALITY)
                torch.cuda.synchronize()
                wall, cpu = time.perf_counter() - w0, time.process_time() - c0
                outs = [data]
            else:
                n, wall, cpu, got = prewarm_once(blur_fn, build_blur_jpeg_fn(cfg, "cuda"), dimg, jpeg, tag)
                outs = [v for r, v in sorted(got.items()) if r > 0]
                rec["buckets"] = n
            rec.update(wall_ms=round(wall * 1e3, 3), cpu_ms=round(cpu * 1e3, 3), jpeg_bytes=sum(len(v) for v in outs))
            return rec, outs

        for entropy, huffman in rows:                   # warm-up of each
            run(entropy, huffman, f"warm-{entropy}-{huffman}")
        for rep in range(a.reps):
            for entropy, huffman in rows:
                emit(dict(run(entropy, huffman, f"{entropy}-{huffman}-{rep}")[0], rep=rep))
        pixels = dimg.tensor[None].contiguous() if a.content else ops.gaussian_blur_pil(dimg.tensor, radii)
        for entropy in ("interval", "block"):           # device time of the count phase, both tables
            restart = jpeg_restart(config(entropy, "standard"), res)[0]
            std = count_phase_device_ms(pixels, restart, entropy, False)
            opt = count_phase_device_ms(pixels, restart, entropy, True)
            emit({"res": res, "mode": mode, "entropy": entropy, "images": int(pixels.shape[0]),
                  "count_phase_device_ms_standard": round(std, 4), "count_phase_device_ms_optimized": round(opt, 4),
                  "histogram_and_build_device_ms": round(opt - std, 4)})
    return 0


def transform_main(a, emit) -> int:
    """--transform libjpeg: libjpeg's forward transform against the matrix one (see the module text)."""
    import torch
    from cassmantle_amd import ops
    from cassmantle_amd.config import Config
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.game.imaging import BlurCache, encode_jpeg
    from cassmantle_amd.runtime.factory import build_blur_fn, build_blur_jpeg_fn, build_content_jpeg_fn, jpeg_restart

    def config(transform):
        c = Config()
        c.model.gpu_jpeg = c.model.gpu_jpeg_content = True
        c.model.blur_kernel = "pil"
        c.model.jpeg_entropy, c.model.jpeg_restart_mcus = "block", -1
        c.model.jpeg_transform = transform
        return c

    rows = ("matrix", a.transform)
    for res in a.res:
        img = source_image(res).copy()
        jpeg = encode_jpeg(img, QUALITY)
        dimg = DeviceImage(torch.from_numpy(img).cuda())
        dimg.host()
        blur_fn = build_blur_fn(config("matrix"), "cuda")
        radii = [i * BUCKET for i in range(1, int(MAX_BLUR / BUCKET) + 1)]
        mode = "content" if a.content else "prewarm"
        # the parent's bytes: PIL's encode of the same pixels (prewarm: of PIL's own blur of them)
        if a.content:
            parent = [jpeg]
        else:
            cache = BlurCache(bucket=BUCKET, quality=QUALITY)
            cache.set_source("parent", dimg)
            cache.prewarm("parent", jpeg, MAX_BLUR)
            parent = [v for (_, r), v in sorted(cache._lru.items()) if r > 0]

        def run(transform, tag):
            cfg = config(transform)
            rec = {"res": res, "mode": mode, "blur_kernel": "pil", "entropy": "block", "transform": transform,
                   "restart_mcus": jpeg_restart(cfg, res)[0]}
            if a.content:
                fn = build_content_jpeg_fn(cfg, "cuda")
                d = DeviceImage(dimg.tensor)
                torch.cuda.synchronize()
                w0, c0 = time.perf_counter(), time.process_time()
                data, _ = fn(d, QUALITY)
                torch.cuda.synchronize()
                wall, cpu = time.perf_counter() - w0, time.process_time() - c0
                outs = [data]
            else:
                n, wall, cpu, got = prewarm_once(blur_fn, build_blur_jpeg_fn(cfg, "cuda"), dimg, jpeg, tag)
                outs = [v for r, v in sorted(got.items()) if r > 0]
                rec["buckets"] = n
            rec.update(wall_ms=round(wall * 1e3, 3), cpu_ms=round(cpu * 1e3, 3), jpeg_bytes=sum(len(v) for v in outs),
                       parent_pil_bytes=sum(len(v) for v in parent), equals_parent_pil_bytes=outs == parent)
            return rec

        for transform in rows:                          # warm-up of each
            run(transform, f"warm-{transform}")
        for rep in range(a.reps):
            for transform in rows:
                emit(dict(run(transform, f"{transform}-{rep}"), rep=rep))
        pixels = dimg.tensor[None].contiguous() if a.content else ops.gaussian_blur_pil(dimg.tensor, radii)
        cnt = {t: count_phase_device_ms(pixels, 0, "block", False, transform=t) for t in rows}
        emit({"res": res, "mode": mode, "entropy": "block", "images": int(pixels.shape[0]),
              "count_phase_device_ms_matrix": round(cnt["matrix"], 4),
              "count_phase_device_ms_" + a.transform: round(cnt[a.transform], 4)})
    return 0


def reconstruct_device_ms(t, restart: int, iters: int = 5) -> float:
    """Device time of the idct + colour kernels behind ``return_decoded`` for the [1, H, W, 3]
    image ``t`` (HIP events around the two launches; nothing else is queued), in ms."""
    import torch
    from cassmantle_amd.ops._ext import ext
    B, H, W, _ = t.shape
    _, args = encode_args(t, restart)
    tables, coef = args[1], args[3]
    ext().jpeg_count(*args)
    planes = torch.empty(coef.numel(), device="cuda", dtype=torch.uint8)
    out = torch.empty((B, H, W, 3), device="cuda", dtype=torch.uint8)
    best = 1e9
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        ext().jpeg_reconstruct(coef, tables, planes, out, H, W, 1)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def blur_stage_device_ms(x, radii, iters: int = 5):
    """Device time of the blur stage alone for one prewarm (HIP events; nothing else is queued), in
    ms: the 60 ops.gaussian_blur launches + copies of build_blur_jpeg_fn, and the one batched
    ops.gaussian_blur_pil launch."""
    import torch
    from cassmantle_amd import ops
    buf = torch.empty((len(radii), *x.shape), device=x.device, dtype=torch.uint8)

    def gaussian():
        for i, r in enumerate(radii):
            ops.copy_(buf[i], ops.gaussian_blur(x, float(r)))

    def timed(fn):
        best = 1e9
        for _ in range(iters + 1):                   # the first round warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return round(best, 4)

    return {"gaussian_60_launches_ms": timed(gaussian),
            "pil_one_launch_ms": timed(lambda: ops.gaussian_blur_pil(x, radii, out=buf))}


def blur_kernel_main(a, emit) -> int:
    import numpy as np
    import torch
    from PIL import Image, ImageFilter
    from cassmantle_amd import ops
    from cassmantle_amd.config import Config
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.game.imaging import encode_jpeg
    from cassmantle_amd.runtime.factory import build_blur_fn, build_blur_jpeg_fn

    for res in a.res:
        img = source_image(res).copy()
        jpeg = encode_jpeg(img, QUALITY)
        dimg = DeviceImage(torch.from_numpy(img).cuda())
        dimg.host()
        blur_fn = build_blur_fn(Config(), "cuda")
        radii = [i * BUCKET for i in range(1, int(MAX_BLUR / BUCKET) + 1)]

        def jpeg_fn(kernel):
            c = Config()
            c.model.gpu_jpeg, c.model.blur_kernel = True, kernel
            return build_blur_jpeg_fn(c, "cuda")

        fns = {"parent": None, "gpu_jpeg": jpeg_fn("gaussian"), "gpu_jpeg+blur_kernel=pil": jpeg_fn("pil")}

        def run(path, tag):
            n, wall, cpu, outs = prewarm_once(blur_fn, fns[path], dimg, jpeg, tag)
            size = sum(len(v) for r, v in outs.items() if r > 0)
            return {"res": res, "path": path, "buckets": n, "wall_ms": round(wall * 1e3, 2),
                    "cpu_ms": round(cpu * 1e3, 2), "jpeg_bytes": size,
                    "d2h_bytes": (n - 1) * res * res * 3 if path == "parent" else size + 4 * n}

        for path in fns:
            run(path, f"warm-{path}")
        for rep in range(a.reps):
            for path in fns:
                emit(dict(run(path, f"{path}-{rep}"), rep=rep))
        got = ops.gaussian_blur_pil(dimg.tensor, [0.25, 7.5, 15.0]).cpu().numpy()
        same = all(np.array_equal(g, np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(r))))
                   for g, r in zip(got, (0.25, 7.5, 15.0)))
        emit({"res": res, "check": "batched_blur_equals_pillow", "radii": [0.25, 7.5, 15.0], "equal": bool(same)})
        emit(dict(blur_stage_device_ms(dimg.tensor, radii), res=res, stage="blur, device time (HIP events)"))
    return 0


def content_main(a, emit) -> int:
    import numpy as np
    import torch
    from PIL import Image
    from cassmantle_amd.config import Config
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.game.imaging import encode_jpeg
    from cassmantle_amd.runtime.factory import build_content_jpeg_fn

    def psnr(x, y):
        mse = float(np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2))
        return round(10 * np.log10(255.0 ** 2 / max(mse, 1e-9)), 2)

    def new_fn(restart_mcus):
        c = Config()
        c.model.gpu_jpeg = c.model.gpu_jpeg_content = True
        c.model.jpeg_restart_mcus = restart_mcus
        return build_content_jpeg_fn(c, "cuda")

    for res in a.res:
        img = source_image(res).copy()
        t = torch.from_numpy(img).cuda()
        mcu_row = (res + 15) // 16

        def run_parent():
            dimg = DeviceImage(t)                    # fresh: no cached host copy
            torch.cuda.synchronize()
            w0, c0 = time.perf_counter(), time.process_time()
            jpeg = encode_jpeg(dimg, QUALITY)
            wall, cpu = time.perf_counter() - w0, time.process_time() - c0
            dec = np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))
            return {"res": res, "path": "parent", "wall_ms": round(wall * 1e3, 3), "cpu_ms": round(cpu * 1e3, 3),
                    "d2h_bytes": res * res * 3, "jpeg_bytes": len(jpeg), "psnr_db": psnr(dec, img)}

        def run_new(restart=0):                      # 0: the default, one MCU row per interval
            fn = new_fn(restart)
            restart = restart or mcu_row
            dimg = DeviceImage(t)
            torch.cuda.synchronize()
            w0, c0 = time.perf_counter(), time.process_time()
            jpeg, decoded = fn(dimg, QUALITY)
            torch.cuda.synchronize()                 # to the end of the idct + colour kernels
            wall, cpu = time.perf_counter() - w0, time.process_time() - c0
            dec = decoded.tensor.cpu().numpy()
            pil = np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))
            return {"res": res, "path": "gpu_jpeg_content", "restart_mcus": restart,
                    "wall_ms": round(wall * 1e3, 3), "cpu_ms": round(cpu * 1e3, 3),
                    "d2h_bytes": len(jpeg) + 8, "jpeg_bytes": len(jpeg), "psnr_db": psnr(dec, img),
                    "decoded_equals_pil_decode": bool(np.array_equal(dec, pil)), "host_copy_made": dimg._host is not None}

        run_parent()
        run_new()
        pil_size = None
        for rep in range(a.reps):
            p = run_parent()
            pil_size = p["jpeg_bytes"]
            emit(dict(p, rep=rep))
            n = run_new()
            emit(dict(n, rep=rep, size_vs_pil=round(n["jpeg_bytes"] / pil_size, 4)))
        for restart in (4, 16):                      # shorter intervals: more lanes code, more bytes
            run_new(restart)
            n = run_new(restart)
            emit(dict(n, sweep=True, size_vs_pil=round(n["jpeg_bytes"] / pil_size, 4)))
        emit({"res": res, "reconstruct_device_ms": round(reconstruct_device_ms(t[None].contiguous(), mcu_row), 4),
              "kernels": "jpeg_idct_kernel + jpeg_colour_kernel"})
    return 0


def decode_main(a, emit) -> int:
    """--decode: stored JPEG bytes -> blur source pixels in HBM (what BlurCache._source does for a
    version with no device-resident source)."""
    import numpy as np
    import torch
    from cassmantle_amd import ops
    from cassmantle_amd.game.imaging import decode_jpeg, encode_jpeg
    from cassmantle_amd.ops import jpeg_format as jf
    from cassmantle_amd.ops._ext import ext
    from cassmantle_amd.runtime.factory import _device_pixels

    def entropy_device_ms(stream, iters: int = 5):
        """(zero + entropy decode launch, zero alone) device time in ms, HIP events, nothing else queued"""
        _, nb, mx, my = jf.geometry(stream.H, stream.W, stream.sampling)
        staged, base, tables, _ = ops._jpeg_decode_inputs([stream], torch.device("cuda"))
        buf = torch.empty(mx * my * nb * 64 + 8, device="cuda", dtype=torch.int16)
        best = [1e9, 1e9]
        for _ in range(iters + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            ev[0].record()
            ext().jpeg_entropy_decode(staged, base, tables, buf, 1, stream.H, stream.W,
                                      int(stream.sampling == "420"), stream.restart)
            ev[1].record()
            ext().zero_(buf)
            ev[2].record()
            torch.cuda.synchronize()
            best = [min(best[0], ev[0].elapsed_time(ev[1])), min(best[1], ev[1].elapsed_time(ev[2]))]
        return best

    def chunked_device_ms(stream, chunk: int, iters: int = 5) -> float:
        """device time in ms of the chunked launch alone (zero, sync + write, DC prefix, check), HIP events"""
        _, nb, mx, my = jf.geometry(stream.H, stream.W, stream.sampling)
        lens = np.asarray([[ln for _, ln in stream.intervals]], dtype=np.int64)
        cb = jf.chunk_bytes_for(int(lens.max()), chunk)
        lane0, groups, threads, _ = ops._jpeg_chunk_groups(lens, cb)
        staged, base, tables, extra = ops._jpeg_decode_inputs([stream], torch.device("cuda"),
                                                              np.concatenate([lane0, groups.reshape(-1)]))
        buf = torch.empty(mx * my * nb * 64 + 16, device="cuda", dtype=torch.int16)
        best = 1e9
        for _ in range(iters + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            ext().jpeg_entropy_decode_chunked(staged, base, tables, buf, 1, stream.H, stream.W,
                                              int(stream.sampling == "420"), stream.restart, extra, len(groups), cb,
                                              threads)
            ev[1].record()
            torch.cuda.synchronize()
            best = min(best, ev[0].elapsed_time(ev[1]))
        return best

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import jpeg_cases as jc
    # the resolutions asked for, then the worst case for the chunked path: noise (long blocks)
    for res, kind in [(r, "background") for r in a.res] + [(512, "noise")]:
        img = source_image(res).copy() if kind == "background" else jc.noise(res, res)
        t = torch.from_numpy(img).cuda()
        mcu_row = (res + 15) // 16
        streams = {}
        if kind == "background":
            streams = {f"in-tree, {r} MCUs per interval" + (" (one MCU row)" if r == mcu_row else ""):
                       ops.jpeg_encode(t, QUALITY, "420", r)[0] for r in (mcu_row, 16, 4)}
        streams["PIL, no DRI (one interval)" + ("" if kind == "background" else ", noise")] = encode_jpeg(img, QUALITY)
        for name, jpeg in streams.items():
            st = jf.parse(jpeg)
            staged_bytes = 8 * len(st.intervals) + st.intervals[-1][0] + st.intervals[-1][1] - st.scan_offset

            def run_parent():
                torch.cuda.synchronize()
                w0, c0 = time.perf_counter(), time.process_time()
                x = _device_pixels(decode_jpeg(jpeg), "cuda")
                torch.cuda.synchronize()
                wall, cpu = time.perf_counter() - w0, time.process_time() - c0
                return x, {"res": res, "stream": name, "path": "parent (PIL decode + upload)",
                           "intervals": len(st.intervals), "jpeg_bytes": len(jpeg), "wall_ms": round(wall * 1e3, 3),
                           "cpu_ms": round(cpu * 1e3, 3), "h2d_bytes": res * res * 3}

            def run_new():
                torch.cuda.synchronize()
                w0, c0 = time.perf_counter(), time.process_time()
                x = ops.jpeg_decode(jpeg, device="cuda")
                torch.cuda.synchronize()
                wall, cpu = time.perf_counter() - w0, time.process_time() - c0
                return x, {"res": res, "stream": name, "path": "ops.jpeg_decode", "intervals": len(st.intervals),
                           "jpeg_bytes": len(jpeg), "wall_ms": round(wall * 1e3, 3), "cpu_ms": round(cpu * 1e3, 3),
                           "h2d_bytes": (staged_bytes + 15) // 16 * 16}

            def run_chunked(chunk):
                info = {}
                torch.cuda.synchronize()
                w0, c0 = time.perf_counter(), time.process_time()
                x = ops.jpeg_decode(jpeg, device="cuda", mode="chunked", chunk_bytes=chunk, info=info)
                torch.cuda.synchronize()
                wall, cpu = time.perf_counter() - w0, time.process_time() - c0
                return x, dict(info, res=res, stream=name, path=f"ops.jpeg_decode(mode=chunked, {chunk})",
                               intervals=len(st.intervals), jpeg_bytes=len(jpeg), wall_ms=round(wall * 1e3, 3),
                               cpu_ms=round(cpu * 1e3, 3))

            xp, _ = run_parent()
            xn, _ = run_new()
            equal = bool(torch.equal(xp, xn))
            equal_chunked = {c: bool(torch.equal(xp, run_chunked(c)[0])) for c in CHUNKS}
            for rep in range(a.reps):
                emit(dict(run_parent()[1], rep=rep))
                emit(dict(run_new()[1], rep=rep, equals_pil_decode=equal))
                for c in CHUNKS:
                    emit(dict(run_chunked(c)[1], rep=rep, equals_pil_decode=equal_chunked[c]))
            for c in CHUNKS:
                emit({"res": res, "stream": name, "intervals": len(st.intervals), "chunk_bytes_asked": c,
                      "chunked_launch_device_ms": round(chunked_device_ms(st, c), 4),
                      "kernels": "zero_kernel + jpeg_entropy_sync_kernel + jpeg_dc_prefix_kernel + jpeg_block_check_kernel"})
            both, zero = entropy_device_ms(st)
            emit({"res": res, "stream": name, "intervals": len(st.intervals),
                  "zero_plus_entropy_decode_device_ms": round(both, 4), "zero_alone_device_ms": round(zero, 4),
                  "kernels": "zero_kernel + jpeg_entropy_decode_kernel"})
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", action="store_true",
                    help="stored JPEG bytes -> device pixels: PIL decode + upload against ops.jpeg_decode")
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON records to this file")
    ap.add_argument("--content", action="store_true", help="the content JPEG of one new image (see above)")
    ap.add_argument("--blur-kernel", choices=["pil"], default=None,
                    help="the prewarm comparison with blur_kernel=pil as a third row (see above)")
    ap.add_argument("--entropy", choices=["block"], default=None,
                    help="the block-parallel entropy coder against the interval coder, prewarm or --content (see above)")
    ap.add_argument("--huffman", choices=["optimized"], default=None,
                    help="the image's own Huffman tables against the standard ones, prewarm or --content (see above)")
    ap.add_argument("--transform", choices=["libjpeg"], default=None,
                    help="libjpeg's forward transform against the matrix one, prewarm or --content (see above)")
    ap.add_argument("--jpeg_restart_mcus", type=int, nargs="+", default=[0, 4, -1],
                    help="--entropy block: the settings compared (0: one MCU row, -1: no restart markers)")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        print("bench_jpeg: needs a GPU", file=sys.stderr)
        return 2
    from cassmantle_amd import ops
    from cassmantle_amd.config import Config
    from cassmantle_amd.game.content import DeviceImage
    from cassmantle_amd.game.imaging import encode_jpeg
    from cassmantle_amd.runtime.factory import build_blur_fn, build_blur_jpeg_fn
    ops.set_mode("hip")
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if a.transform:
        rc = transform_main(a, emit)
        if sink:
            sink.close()
        return rc
    if a.entropy or a.huffman:
        rc = huffman_main(a, emit) if a.huffman else block_main(a, emit)
        if sink:
            sink.close()
        return rc
    if a.decode or a.content or a.blur_kernel:
        rc = decode_main(a, emit) if a.decode else (content_main(a, emit) if a.content else blur_kernel_main(a, emit))
        if sink:
            sink.close()
        return rc
    for res in a.res:
        img = source_image(res).copy()
        jpeg = encode_jpeg(img, QUALITY)
        dimg = DeviceImage(torch.from_numpy(img).cuda())
        dimg.host()
        cfg = Config()
        blur_fn = build_blur_fn(cfg, "cuda")
        mcu_row = (res + 15) // 16

        def new_fn(restart):
            c = Config()
            c.model.gpu_jpeg, c.model.jpeg_restart_mcus = True, restart
            return build_blur_jpeg_fn(c, "cuda")

        def run_parent(tag):
            n, wall, cpu, outs = prewarm_once(blur_fn, None, dimg, jpeg, tag)
            return {"res": res, "path": "parent", "buckets": n, "wall_ms": round(wall * 1e3, 2),
                    "cpu_ms": round(cpu * 1e3, 2), "d2h_bytes": (n - 1) * res * res * 3,
                    "jpeg_bytes": sum(len(v) for r, v in outs.items() if r > 0)}, outs

        def run_new(tag, restart):
            n, wall, cpu, outs = prewarm_once(blur_fn, new_fn(restart), dimg, jpeg, tag)
            size = sum(len(v) for r, v in outs.items() if r > 0)
            return {"res": res, "path": "gpu_jpeg", "restart_mcus": restart or mcu_row, "buckets": n,
                    "wall_ms": round(wall * 1e3, 2), "cpu_ms": round(cpu * 1e3, 2),
                    "d2h_bytes": size + 4 * n, "jpeg_bytes": size}, outs

        run_parent("warm-p")
        _, outs = run_new("warm-n", cfg.model.jpeg_restart_mcus)
        # what the new path serves is the parent's picture: decode one bucket of each
        _, pouts = run_parent("check")
        for r in (0.25, 7.5, 15.0):
            d = np.asarray(Image.open(io.BytesIO(outs[r])).convert("RGB")).astype(np.float64)
            p = np.asarray(Image.open(io.BytesIO(pouts[r])).convert("RGB")).astype(np.float64)
            mse = float(np.mean((d - p) ** 2))
            emit({"res": res, "check": "psnr_new_vs_parent_decode", "radius": r,
                  "psnr_db": round(10 * np.log10(255.0 ** 2 / max(mse, 1e-9)), 2)})
        for rep in range(a.reps):
            emit(dict(run_parent(f"p{rep}")[0], rep=rep))
            emit(dict(run_new(f"n{rep}", cfg.model.jpeg_restart_mcus)[0], rep=rep))
        # the blurred batch once, for the kernels' device time
        radii = [i * BUCKET for i in range(1, int(MAX_BLUR / BUCKET) + 1)]
        batch = torch.stack([ops.gaussian_blur(dimg.tensor, r) for r in radii])
        sizes = {}
        for restart in (1, 2, 4, 8, 16, mcu_row):
            run_new(f"w{restart}", restart)
            rec, _ = run_new(f"s{restart}", restart)
            cnt, wr = encode_device_ms(batch, restart)
            sizes[restart] = rec["jpeg_bytes"]
            rec.update(sweep=True, row=restart == mcu_row, count_phase_device_ms=round(cnt, 3),
                       write_phase_device_ms=round(wr, 3))
            emit(rec)
        emit({"res": res, "size_overhead_vs_row": {str(k): round(v / sizes[mcu_row] - 1, 4) for k, v in sizes.items()}})
    if sink:
        sink.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
