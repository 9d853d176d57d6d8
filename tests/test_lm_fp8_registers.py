"""Compiler resource check of the weight-only fp8 translation unit (CPU, hipcc only), with the
machinery of test_kernel_registers.py: gemv_fp8_kernel (plain and gated, each with and without the
fused RMS scale: four instantiations of one template), quant_rows_fp8_kernel and
dequant_rows_fp8_kernel exist and none uses scratch; the GEMV's 512-thread block (2 waves per SIMD)
leaves room for a second block per CU: at most 128 VGPRs.  Prints the counts."""
import pytest

from test_kernel_registers import HIPCC, KERNEL, _asm, _scratch

TU = "lm_fp8"


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_fp8_kernels_exist_and_do_not_spill():
    assert _scratch(TU) == []
    kernels = {m.group(1): int(m.group(3)) for m in KERNEL.finditer(_asm(TU))}
    print(kernels)
    gemv = [n for n in kernels if "gemv_fp8_kernel" in n]
    assert len(gemv) == 4
    assert any("quant_rows_fp8_kernel" in n and "dequant" not in n for n in kernels)
    assert any("dequant_rows_fp8_kernel" in n for n in kernels)
    assert all(kernels[n] <= 128 for n in gemv), kernels
    asm = _asm(TU)
    assert "v_mfma_f32_16x16x32_bf16" in asm and "v_cvt_scalef32_pk_bf16_fp8" in asm
