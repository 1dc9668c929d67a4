"""Build-level properties of the 16-bit-weight kernels, cross-compiled here with the flags of test_build_props.py.  The decode mat-vec
(csrc/matvec_h16.hip): no scratch, no spilled VGPRs, and the 128 VGPRs that let its 16-wave workgroup run four waves per SIMD.  The
prompt GEMM (pf_gemm_half_kernel, csrc/prefill.hip): its 128 accumulators in the accumulation registers beside a three-step ring of
weights, within one wave's 256 VGPRs and without scratch."""
from test_build_props import _usage


def test_half_matvec_uses_no_scratch_and_fits_four_waves_per_simd():
    usage = _usage("matvec_h16.hip")
    mvh = {fn: u for fn, u in usage.items() if "mvh_kernel" in fn}
    assert len(mvh) == 2 and len(usage) == 3   # F16, BF16, and the upload repack
    for fn, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (fn, u)
    for fn, u in mvh.items():
        assert u["VGPRs"] <= 128 and u.get("Occupancy", 4) >= 4, (fn, u)


def test_half_prompt_gemm_keeps_its_accumulators_in_registers():
    gemm = {fn: u for fn, u in _usage("prefill.hip").items() if "pf_gemm_half_kernel" in fn}
    assert len(gemm) == 3   # F16, BF16, and both in one launch
    for fn, u in gemm.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (fn, u)
        assert u.get("AGPRs", 0) >= 128 and u["VGPRs"] <= 256, (fn, u)
