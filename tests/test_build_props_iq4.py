"""Build-level properties of the IQ4_NL / IQ4_XS kernels (LGH_WEIGHTS_IQ4_TILES), cross-compiled with test_build_props.py's flags:
instantiated for the two formats under names of their own, no scratch, no spilled VGPRs; the decode kernels within the 256 VGPRs of
two waves per SIMD, the prompt GEMM with its 128 accumulators in the accumulation registers."""
import pytest

from test_build_props import _usage

MASKS = (1024, 2048)   # IQ4_NL, IQ4_XS: 1 << F_* of mvq_core.h; the prompt GEMM's own format numbers (prefill.hip) give four times that


@pytest.mark.parametrize("src,names", [("matvec_mfma.hip", {"mvq_iq4_kernel": 1}), ("prefill.hip", {"pf_gemm_iq4_kernel": 1}),
                                       ("matvec_batch.hip", {"mvqb_iq4_kernel": 3, "mvqb2_iq4_kernel": 6})])   # name: instantiations per format
def test_iq4_kernels_meet_their_register_limits(src, names):
    usage = _usage(src)
    for name, per_format in names.items():
        kernels = {fn: u for fn, u in usage.items() if name + "ILj" in fn}
        masks = ["ILj%dE" % (m * (4 if src == "prefill.hip" else 1)) for m in MASKS]   # <1024u> ... in the mangled names
        assert [sum(m in fn for fn in kernels) for m in masks] == [per_format] * 2 and len(kernels) == 2 * per_format, sorted(kernels)
        for fn, u in kernels.items():
            assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u["VGPRs"] <= 256, (fn, u)
            assert u.get("AGPRs", 0) >= 128 if src == "prefill.hip" else u.get("Occupancy", 2) >= 2, (fn, u)
