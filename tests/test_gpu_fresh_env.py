"""The kernels that only an environment variable selects, each in a fresh child process (tests/fresh_process.py), held to the checks
of the in-suite tests of the same launches (tests/fresh_scenarios.py calls those tests' own code).

The library reads LGH_MVQB2_MIN, LGH_MVQB2_SEQ_GROUPS, LGH_MOE_GROUP_MIN and LGH_PF_ATTN_VALU once per process into a `static`, so
the suite's one process cannot reach what they select: mvqb_kernel<MASK, NB> at NB = 8 and 16 and at more than one sequence (the
structure mvqb_launch falls back to without a word when the partial-sum buffer is too small or the segments do not share their input),
the sequence-by-sequence MoE FFN under capture from 3 sequences on, both mvqb2 grids on shapes that by default take the other one, and
the VALU prompt-attention kernel.  Each child prints the `WORST <path>: err / bound` lines of its checks."""
import numpy as np
import pytest

import fresh_process
import fresh_scenarios
import matvec_ref as mr
from test_gpu_attention import SHAPES

pytestmark = pytest.mark.gpu

MVQB = {"LGH_MVQB2_MIN": "17"}
NO_GROUPS = {"LGH_MOE_GROUP_MIN": "17"}


# ---- 1. LGH_MVQB2_MIN=17: Linear.check's four requirements (float64 bound, bits of the single-sequence launch, a bit-identical second
# call, the poison pattern everywhere else) of mvqb at n_seq 2 .. 16; in every child only the first structure's counter may move
@pytest.mark.parametrize("tname", mr.FUSED)
def test_mvqb_formats_and_sequence_counts(gpu, tname):
    r = fresh_process.run("mvqb_formats", MVQB, args=(tname,))
    assert r["moved"][0] >= 2 * len(fresh_scenarios.MVQB_SEQS) and r["moved"][1:] == [0, 0], r


def test_mvqb_epilogues_ragged_rows_and_chains(gpu):
    r = fresh_process.run("mvqb_epilogues", MVQB)
    assert r["moved"][0] > 0 and r["moved"][1:] == [0, 0], r


def test_mvqb_fused_qkv(gpu):
    r = fresh_process.run("mvqb_qkv", MVQB)
    assert r["moved"][0] > 0 and r["moved"][1:] == [0, 0], r


# ---- 2. the engine on mvqb alone: DESIGN §4.4's promise covers the fallback as well
@pytest.mark.parametrize("name,mix,B", [("test-dense", "Q4_K_M", 5), ("test-dense-d128", "Q4_K_M", 16), ("test-dense", "Q8_0", 9),
                                        ("test-moe-e1024", "Q5_K_M", 7)])
def test_engine_on_mvqb_is_bitwise_the_single_sequence_engine(gpu, name, mix, B):
    r = fresh_process.run("engine_bitwise", dict(MVQB, **NO_GROUPS), args=(name, mix, B))
    assert r["moved"][0] > 0 and r["moved"][1:] == [0, 0], r
    if "moe" in name:
        assert r["launches"].get("router") == B * r["layers"], r


# ---- 3. LGH_MOE_GROUP_MIN=17 alone: mvqb2 for attention and output, the MoE FFN sequence by sequence under capture
@pytest.mark.parametrize("name,mix,B", [("test-moe-e1024", "Q5_K_M", 3), ("test-moe-e1024-k4", "Q4_K_M", 16)])
def test_moe_ffn_sequence_by_sequence_is_bitwise_the_single_sequence_engine(gpu, name, mix, B):
    """That the switch took effect shows in the launches by class of a step of B sequences: one router launch per sequence and layer
    (the grouped step has one per layer)."""
    r = fresh_process.run("engine_bitwise", NO_GROUPS, args=(name, mix, B))
    assert r["moved"][1] + r["moved"][2] > 0, r                       # (counter 0 moves too: the ragged test's steps of ONE sequence)
    assert r["launches"].get("router") == B * r["layers"], r


# ---- 4. LGH_MVQB2_SEQ_GROUPS: every launch on the SEQ grid, then every launch on the split grid
@pytest.mark.parametrize("forced,value", [("seq", "0"), ("split", "1000000")])
def test_forced_mvqb2_grid(gpu, forced, value):
    r = fresh_process.run("seq_groups", {"LGH_MVQB2_SEQ_GROUPS": value}, args=(forced,))
    assert r["structures"][0] == 0, r                                # (no launch fell back to mvqb)
    if forced == "seq":
        assert r["structures"][1] == 0 and r["structures"][2] > 0, r


# ---- 5. LGH_PF_ATTN_VALU=1
@pytest.mark.parametrize("d,g", SHAPES)
def test_valu_prompt_attention(gpu, pkg, d, g):
    """The child runs test_gpu_attention.test_prefill's cases of (d, g) with its bound.  No counter tells which kernel ran, so the
    evidence that the VALU kernel did is in the bits: the child's output of one case at (d, g) = (128, 4) and this process's output of
    the same case (attn_pf_mfma_kernel) are both inside the bound (each side's run asserts it) and differ in at least one element —
    two summation orders."""
    child = fresh_process.run("prefill_attention", {"LGH_PF_ATTN_VALU": "1"}, args=(d, g))
    if (d, g) != (128, 4):
        return
    here = fresh_scenarios.prefill_attention(pkg, d, g)
    assert child["shape"] == here["shape"]
    a, b = np.array(child["bits"], np.uint32), np.array(here["bits"], np.uint32)
    assert np.isfinite(a.view(np.float32)).all() and np.isfinite(b.view(np.float32)).all()
    assert int(np.count_nonzero(a != b)) > 0, "the child's output is bit for bit the matrix-core kernel's: did the variable take effect?"
