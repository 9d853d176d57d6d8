"""Shared by test_jpeg_decode.py (CPU) and test_jpeg_decode_gpu.py: the inputs of the decode
contract tests, their reference pixels (computed once), and a stub round for
``GameRoom._make_content``."""
from __future__ import annotations

import asyncio
from functools import lru_cache

import jpeg_cases as jc
from cassmantle_amd.ops import jpeg_format as jf


@lru_cache(maxsize=None)
def decode_inputs():
    """hard cases + fidelity inputs + a single sample, odd chroma sizes (ch 5, cw 4), a partial
    MCU in both directions, and the two widths (cw 2) at which libjpeg replicates chroma"""
    cases = dict(jc.hard_cases())
    cases.update({"fid_" + k: v for k, v in jc.fidelity_inputs().items()})
    cases.update({"noise_1x1": jc.noise(1, 1), "noise_9x7": jc.noise(9, 7), "gradient_18x34": jc.gradient(18, 34),
                  "noise_5x3": jc.noise(5, 3), "noise_6x4": jc.noise(6, 4)})
    return cases


@lru_cache(maxsize=None)
def reconstructed(name: str, quality: int, sampling: str):
    """(reference pixels, largest intermediate magnitude), computed once per case"""
    img = decode_inputs()[name]
    stats = {}
    out = jf.reconstruct(jf.coefficients(img, quality, sampling), img.shape[0], img.shape[1], quality, sampling, stats)
    out.setflags(write=False)
    return out, stats["max_abs"]


class Scorer:
    def embed_words(self, words):
        return None


def make_content(room, image):
    """``room._make_content`` with the prompt, the picture and the mask choice stubbed out:
    (prompt, prompt json, jpeg)"""
    async def prompt(seed, is_seed):
        return "a silent lantern tower"

    async def picture(prompt):
        return image
    room.generate_prompt, room.generate_image = prompt, picture
    room._prompt_dict = lambda p: {"tokens": p.split(), "masks": [1]}
    return asyncio.run(room._make_content("seed", True))
