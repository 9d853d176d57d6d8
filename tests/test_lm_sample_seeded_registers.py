"""Compiler resource check of the seeded sampler's translation unit (CPU, hipcc only), with the
machinery of test_kernel_registers.py: lm_sample_seeded_kernel (bf16 and fp32 logits) and
lm_gumbel_kernel exist, none uses scratch, and the sampler's 1024-thread block (4 waves per SIMD)
fits: at most 128 VGPRs (512 per SIMD lane / 4 waves)."""
import pytest

from test_kernel_registers import HIPCC, KERNEL, _asm, _scratch

TU = "lm_sample_seeded"


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_seeded_sampler_kernels_do_not_spill():
    assert _scratch(TU) == []
    kernels = {m.group(1): int(m.group(3)) for m in KERNEL.finditer(_asm(TU))}
    print(kernels)
    sampler = [n for n in kernels if "lm_sample_seeded_kernel" in n]
    assert len(sampler) == 2 and any("lm_gumbel_kernel" in n for n in kernels)
    assert all(kernels[n] <= 128 for n in sampler), kernels
