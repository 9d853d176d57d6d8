"""Compiler resource check of the LM sampler's translation unit (CPU, hipcc only), with the
machinery of test_kernel_registers.py: lm_sample_kernel and lm_sample_seeded_kernel (bf16 and fp32
logits each, four instantiations of one core) and lm_gumbel_kernel exist, none uses scratch, and
the samplers' 1024-thread block (4 waves per SIMD) fits: at most 128 VGPRs (512 per SIMD lane / 4
waves)."""
import pytest

from test_kernel_registers import HIPCC, KERNEL, _asm, _scratch

TU = "lm_sample"


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_sampler_kernels_do_not_spill():
    assert _scratch(TU) == []
    kernels = {m.group(1): int(m.group(3)) for m in KERNEL.finditer(_asm(TU))}
    print(kernels)
    table = [n for n in kernels if "lm_sample_kernel" in n]
    seeded = [n for n in kernels if "lm_sample_seeded_kernel" in n]
    assert len(table) == 2 and len(seeded) == 2 and any("lm_gumbel_kernel" in n for n in kernels)
    assert all(kernels[n] <= 128 for n in table + seeded), kernels
