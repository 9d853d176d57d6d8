"""Image masking (score → blur) and JPEG transport.

Reference: ``score_to_blur`` = ``min + (1 - s²)(max - min)`` (``src/backend.py:319-320``) and
``mask_image`` = PIL ``GaussianBlur`` (``src/backend.py:322-324``), recomputed from the full
JPEG on every ``/fetch/contents`` (``src/server.py:129-133``, Appendix C.13), then JPEG +
base64 (``main.py:101-107``).  Here the blur radius is quantised into buckets and each
(content version, bucket) JPEG is cached, so a page view costs a dict lookup; the blur itself
runs on the GPU (``ops.gaussian_blur``, HIP separable kernel) when the content was generated
there, else PIL on the CPU.
"""
from __future__ import annotations

import io
import math
import threading
from collections import OrderedDict
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
from PIL import Image, ImageFilter

from ..utils.tracing import TRACER


def score_to_blur(score: float, min_blur: float = 0.0, max_blur: float = 15.0) -> float:
    return min_blur + (1.0 - score ** 2) * (max_blur - min_blur)


def encode_jpeg(img, quality: int = 75) -> bytes:
    """``encode_image`` parity (``src/utils.py:12-16``; PIL default quality is 75).  ``img``: a
    PIL image, a uint8 array, or anything ``np.asarray`` turns into one (``DeviceImage``)."""
    if not isinstance(img, Image.Image):
        img = Image.fromarray(np.asarray(img))
    if img.mode != "RGB":
        img = img.convert("RGB")
    buf = io.BytesIO()
    img.save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def decode_jpeg(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def blur_pil(img: np.ndarray, radius: float) -> np.ndarray:
    img = np.asarray(img)
    if radius <= 0:
        return img
    return np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius)))


def quantize_radius(radius: float, bucket: float) -> float:
    if bucket <= 0:
        return radius
    return round(radius / bucket) * bucket


BlurFn = Callable[[np.ndarray, float], np.ndarray]
# (image, radii > 0, quality) -> one JPEG per radius, blurred and encoded on the GPU
# (runtime.factory.build_blur_jpeg_fn)
BlurJpegFn = Callable[[object, Sequence[float], int], List[bytes]]


class BlurCache:
    """LRU of blurred JPEGs keyed by (content version, radius bucket)."""

    def __init__(self, blur_fn: Optional[BlurFn] = None, bucket: float = 0.25,
                 quality: int = 75, capacity: int = 256, blur_jpeg_fn: Optional[BlurJpegFn] = None,
                 decode_fn: Optional[Callable[[bytes], object]] = None) -> None:
        self.blur_fn = blur_fn or blur_pil
        self.blur_jpeg_fn = blur_jpeg_fn
        # jpeg bytes -> their decoded pixels in HBM (runtime.factory.build_jpeg_decode_fn), or None
        # for a stream it leaves to decode_jpeg; None: decode_jpeg (PIL on the host) always
        self.decode_fn = decode_fn
        self.bucket = bucket
        self.quality = quality
        self.capacity = capacity
        self._lru: "OrderedDict[Tuple[str, float], bytes]" = OrderedDict()
        self._decoded: Tuple[Optional[str], Optional[np.ndarray]] = (None, None)
        # version -> device-resident source image (DeviceImage) of content generated on a GPU:
        # the blur reads it in HBM instead of decoding the JPEG (bounded: current + next content).
        # It holds the original pixels, which differ from the decoded JPEG another process would
        # blur, or with gpu_jpeg_content the decoded pixels themselves (GameRoom._make_content)
        self._sources: "OrderedDict[str, object]" = OrderedDict()
        self._lock = threading.Lock()
        self.hits = 0
        self.misses = 0

    def __len__(self) -> int:
        with self._lock:
            return len(self._lru)

    def set_source(self, version: str, img) -> None:
        """Register the device-resident pixels of content ``version`` (see ``_sources``)."""
        with self._lock:
            self._sources[version] = img
            self._sources.move_to_end(version)
            while len(self._sources) > 4:
                self._sources.popitem(last=False)

    def get(self, version: str, jpeg: bytes, radius: float) -> bytes:
        r = quantize_radius(radius, self.bucket)
        key = (version, r)
        with self._lock:
            if key in self._lru:
                self._lru.move_to_end(key)
                self.hits += 1
                return self._lru[key]
            self.misses += 1
            arr = self._source(version, jpeg)
        with TRACER.span("blur_jpeg"):
            if r > 0 and self.blur_jpeg_fn is not None:
                out = self.blur_jpeg_fn(arr, [r], self.quality)[0]
            else:
                out = encode_jpeg(self.blur_fn(arr, r), self.quality) if r > 0 else jpeg
        self._store([(key, out)])
        return out

    def _store(self, items) -> None:
        with self._lock:
            for key, out in items:
                self._lru[key] = out
            while len(self._lru) > self.capacity:
                self._lru.popitem(last=False)

    def _source(self, version: str, jpeg: bytes):
        """The pixels of content ``version``: its device-resident original, else the decoded JPEG
        (call with the lock held)."""
        arr = self._sources.get(version)
        if arr is None:
            ver, arr = self._decoded
            if ver != version:
                arr = self.decode_fn(jpeg) if self.decode_fn is not None else None
                if arr is None:
                    arr = decode_jpeg(jpeg)
                self._decoded = (version, arr)
        return arr

    def prewarm(self, version: str, jpeg: bytes, max_blur: float) -> int:
        """Precompute every bucket for a freshly promoted image (round boundary).  With a
        ``blur_jpeg_fn`` all missing buckets are blurred and encoded in ONE call."""
        n = 0
        steps = int(math.ceil(max_blur / self.bucket)) if self.bucket > 0 else 0
        if self.blur_jpeg_fn is not None:
            radii = [quantize_radius(i * self.bucket, self.bucket) for i in range(steps + 1)]
            with self._lock:
                missing = [r for r in dict.fromkeys(radii) if r > 0 and (version, r) not in self._lru]
                arr = self._source(version, jpeg) if missing else None
                self.misses += len(missing)
            if missing:
                with TRACER.span("blur_jpeg"):
                    outs = self.blur_jpeg_fn(arr, missing, self.quality)
                self._store([((version, r), o) for r, o in zip(missing, outs)])
        for i in range(steps + 1):
            self.get(version, jpeg, i * self.bucket)
            n += 1
        return n
