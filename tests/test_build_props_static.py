"""Build-level properties of the static-plan instantiations of the matrix-core mat-vec (mvqs_kernel, csrc/matvec_mfma.hip):
what tests/test_build_props.py holds mvq_kernel to.  (That file's scratch / spill check already sees every kernel of the source;
its register and occupancy check selects kernels by the name mvq_kernel and counts them, so these are held to it here.)"""
import test_build_props as bp


def test_static_plans_fit_two_waves_per_simd():
    usage = bp._usage("matvec_mfma.hip")
    mvqs = {fn: u for fn, u in usage.items() if "mvqs_kernel" in fn}
    assert 1 <= len(mvqs) <= 8, sorted(mvqs)   # the plan table: at most eight instantiations
    for fn, u in mvqs.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (fn, u)
        assert u["VGPRs"] <= 256 and u.get("Occupancy", 2) >= 2, (fn, u)
