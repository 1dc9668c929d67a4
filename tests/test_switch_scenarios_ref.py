"""What gives the oracle comparisons at the attention switch their meaning, and the scenario tables (tests/switch_scenarios.py); no GPU.

An engine that picks the wrong attention form, or runs the right one from a stale position, attends a cache with a row too few or a
row shifted.  The oracle bound 2e-3 * max|logit| + 2e-3 only catches that if such a cache moves the next logits by far more than the
bound.  Measured here on the oracle itself, for both models and for 64, 65, 256 and 257 visible rows (either side of S = 64 and of
the default 256): the logits of the next token (a) as they are, (b) after kv_shift_left(1), (c) with t_0 never fed.  (b) and (c)
must each differ from (a) by at least 10 times the bound; the test prints the multiple."""
import os

import numpy as np
import pytest

import switch_scenarios as sw

FACTOR = 10.0


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_a_lost_row_moves_the_logits_far_beyond_the_oracle_bound(pkg, orc, name, mix):
    cfg, _, ref = sw.oracle_model(pkg, orc, name, mix, sw.DEFAULT_MAX_SEQ)
    orc.set_threads(min(8, len(os.sched_getaffinity(0))))   # (one task per output element: the result does not depend on the count)
    try:
        for rows in (sw.S, sw.S + 1, sw.DEFAULT_S, sw.DEFAULT_S + 1):
            hist, nxt = sw.tokens(0, rows - 1, cfg.vocab_size), sw.token(rows - 1, cfg.vocab_size)   # the next step attends `rows` rows
            ref.reset()
            ref.forward(hist)
            a = ref.forward([nxt]).copy()
            ref.kv_truncate(rows - 1)
            ref.kv_shift_left(1)
            assert ref.position == rows - 2
            b = ref.forward([nxt]).copy()
            ref.reset()
            ref.forward(hist[1:])
            c = ref.forward([nxt]).copy()
            bound = sw.tol(a)
            mb, mc = float(np.abs(b - a).max()) / bound, float(np.abs(c - a).max()) / bound
            print("%s/%s %d rows: kv_shift_left(1) moves the logits by %.1f x the oracle bound, t_0 never fed by %.1f x (bound %.3e)"
                  % (name, mix, rows, mb, mc, bound))
            assert mb >= FACTOR and mc >= FACTOR, (name, rows, mb, mc)
    finally:
        orc.set_threads(1)
        ref.close()


def test_scenarios_that_claim_to_cross_the_switch_do():
    for table, s in ((sw.SCENARIOS, sw.S), (sw.DEFAULT_SCENARIOS, sw.DEFAULT_S)):
        for name, (crosses, ops) in table.items():
            rows = sw.rows_attended(ops)
            both = s in rows and s + 1 in rows
            assert both == crosses, (name, crosses, sorted(set(rows))[:4], max(rows))
            assert max(rows) <= (sw.MAX_SEQ if s == sw.S else sw.DEFAULT_MAX_SEQ), name
            assert sw.final_position(ops) <= (sw.MAX_SEQ if s == sw.S else sw.DEFAULT_MAX_SEQ), name
    # every scenario that does not cross in one direction still runs the split form, and the two graph-order scenarios run it FIRST
    for name in ("restore_above", "split_graph_first", "head_graph_late", "batched_64", "batched_65"):
        assert max(sw.rows_attended(sw.SCENARIOS[name][1])) > sw.S, name
    for name in ("split_graph_first", "head_graph_late"):
        assert sw.rows_attended(sw.SCENARIOS[name][1])[0] > sw.S, name
    assert min(sw.rows_attended(sw.SCENARIOS["head_graph_late"][1])) <= sw.S
    assert sw.rows_attended(sw.DEFAULT_SCENARIOS["cold_split_first"][1])[0] == sw.DEFAULT_S + 2
    with pytest.raises(ValueError):
        sw.replay([("forward", 0, 3), ("rewind", 1)])                 # an operation the replay does not know


def test_tokens_and_position_replay():
    assert sw.tokens(0, 3, 2048) == [5, 18, 31] and sw.token(200, 1024) == (13 * 200 + 5) % 1024
    assert sw.rows_attended([("forward", 0, 3), ("truncate", 1), ("forward", 1, 3)]) == [1, 2, 3, 2, 3]
    assert sw.rows_attended([("batch", 63), ("forward", 63, 65)]) == [64, 65]
    assert sw.rows_attended([("forward", 0, 80), ("shift", 20), ("forward", 60, 62)])[-2:] == [61, 62]
    assert sw.final_position(sw.SCENARIOS["rewind"][1]) == 70 and sw.final_position(sw.SCENARIOS["greedy_loop"][1]) == 72
    assert not set(sw.other_tokens(10, 2048)) & set(sw.tokens(0, 10, 2048))
