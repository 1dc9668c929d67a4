"""Cold graph captures: a kernel whose first launch of the process happens inside a capture is not replayed with the graph
(engine.hip: warm_kernels), so lgh_finalize and lgh_batch_create launch, eagerly, every kernel a captured step of theirs can launch.
In-suite that rule cannot be seen to hold — the pytest process is warm long before —, and a miss costs wrong tokens, not an error.

Each scenario (tests/fresh_scenarios.py: cold_*) runs in a fresh child (tests/fresh_process.py) with the path under test as the
child's first GPU work: no single-sequence or eager engine exists before the captured steps have ended; lgh_finalize and
lgh_batch_create of the context itself are all the warm-up there is.  The child then computes the same on a FLAG_NO_GRAPH context
(eager, never captured).  Logits (as digests of their bytes) and tokens of the two must be equal bit for bit, and equal to what this
— warm — process gets from the same scenario."""
import pytest

import fresh_process
import fresh_scenarios

pytestmark = pytest.mark.gpu


def _cold(pkg, scenario, *args):
    child = fresh_process.run(scenario, args=args)
    assert child["cold"]["tokens"] == child["eager"]["tokens"], (scenario, args, child["cold"]["tokens"], child["eager"]["tokens"])
    steps = [i for i, (a, b) in enumerate(zip(child["cold"]["logits"], child["eager"]["logits"])) if a != b]
    assert not steps, "%s%s: the captured steps %s differ from the eager ones" % (scenario, args, steps)
    here = getattr(fresh_scenarios, scenario)(pkg, *args)
    assert here["cold"] == here["eager"], (scenario, args, "in-process")
    assert child["cold"] == here["cold"], "%s%s: the child's bits differ from this process's" % (scenario, args)


# greedy = True: mode 1 (logits + arg-max), False: mode 0 (logits alone); ragged histories of 3 .. 8 tokens, the first step with all B
@pytest.mark.parametrize("name,mix,B,greedy,max_batch", [
    ("test-dense", "Q4_K_M", 5, True, 0), ("test-dense-d128", "Q6_K", 16, True, 0), ("test-dense", "Q8_0", 9, False, 0),
    # the expert-grouped step: moe_group_kernel, moe_combine_kernel, the multi-token router, the indirect (grid z) mvqb2 launches
    ("test-moe-e1024", "Q5_K_M", 3, True, 0), ("test-moe-e1024-k4", "Q4_K_M", 16, True, 0),
    # ... and a grouped step in the smallest bucket of a context made for 16
    ("test-moe-e1024", "Q5_K_M", 4, True, 16)])
def test_first_gpu_work_is_a_multi_sequence_step(gpu, pkg, name, mix, B, greedy, max_batch):
    _cold(pkg, "cold_forward_multi", name, mix, B, greedy, max_batch)


@pytest.mark.parametrize("name,mix,B,kv", [("test-dense", "Q4_K_M", 5, "int8"), ("test-dense-d128", "Q4_K_M", 5, "tq3")])
def test_first_multi_sequence_step_is_a_greedy_loop_over_quantized_slots(gpu, pkg, name, mix, B, kv):
    _cold(pkg, "cold_quantized_slots", name, mix, B, kv)


def test_first_gpu_work_is_a_tensor_parallel_decode(gpu, pkg):
    _cold(pkg, "cold_tensor_parallel")


# ---- both decode-attention graphs (tests/switch_scenarios.py): the head form up to the switch, splits + merge beyond
def test_first_gpu_work_captures_the_head_graph_then_the_split_graph(gpu, pkg):
    _cold(pkg, "cold_switch_single")


def test_first_captured_step_is_the_split_graph_behind_a_batched_prompt(gpu, pkg):
    _cold(pkg, "cold_split_first")


def test_first_gpu_work_is_a_tensor_parallel_decode_across_the_switch(gpu, pkg):
    _cold(pkg, "cold_tensor_parallel_switch")
