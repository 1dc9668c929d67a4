"""Every engine and state operation across the decode-attention switch (tests/switch_scenarios.py has the scenarios and their tokens).

Decode attention over the f32 cache is one launch (attn_head_kernel) while the step attends at most `direct_attn_max_kv` rows and
attn_split_launch + attn_merge_launch beyond.  Each form has its own captured graph per mode; step() / tp_step() pick the form from the
host-side position while the kernels read the position from the device state.  A mistake between the two — the form picked from a
stale host position after a rewind, a graph captured while the other form's XQ images were marked fresh, a restore that sets one of the
two positions — gives wrong tokens and no error.  Here the switch is put at S = 64 rows (attn_direct=1) of a 160-row cache, and every
state operation, loop and handle is taken across it, in both directions, with both graphs captured in either order.

Everything compared is BIT FOR BIT unless it says "oracle": the same kernels over the same bytes in the same order.  The oracle checks
use the project's bounds, 2e-3 * max|logit| + 2e-3, and 1e-2 * max|logit| + 1e-2 behind a batched prompt; a cache that lost or shifted
one row misses the first by a factor of 50 to 200 (tests/test_switch_scenarios_ref.py measures it).

Which form ran is witnessed twice: by the profiling counters (`attn_combine` launches: 0 in the head form, num_layers in the split
form) where an engine has them, and by bits elsewhere — engines with the switch at 64 and at 128 rows are identical while both run the
head form and differ beyond, because the two forms sum in different trees."""
import ctypes as C

import numpy as np
import pytest

import switch_scenarios as sw

pytestmark = pytest.mark.gpu

S = sw.S


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    """Two runs' outputs (logits arrays and token lists, in order) are the same bits."""
    if len(a) != len(b):
        return False
    return all((x == y) if isinstance(x, list) else np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _first_diff(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b)) if not _same([x], [y])][:5]


def _engine(pkg, model, flags=0, attn_direct=sw.ATTN_DIRECT, max_seq=sw.MAX_SEQ, exact=True, **kw):
    hb = pkg.hip_backend
    return pkg.HipGpuInference.from_model(model, max_seq, flags=flags | (hb.FLAG_EXACT_PREFILL if exact else 0), attn_direct=attn_direct, **kw)


def _twins(pkg, model, **kw):
    """A graph engine and its FLAG_NO_GRAPH twin."""
    eng = _engine(pkg, model, **kw)
    try:
        return eng, _engine(pkg, model, flags=pkg.hip_backend.FLAG_NO_GRAPH, **kw)
    except Exception:
        eng.close()
        raise


class _Handles(list):
    """Handles made one after the other inside a `try`: `close` closes whatever was made, also when making the next one failed."""

    def make(self, fn, *args, **kw):
        self.append(fn(*args, **kw))
        return self[-1]

    def make_twins(self, pkg, model, **kw):
        self.extend(_twins(pkg, model, **kw))
        return self[-2], self[-1]

    def close(self):
        for h in reversed(self):
            h.close()


def _combine_launches(eng, step):
    """`step()` under profiling -> (its result, the attn launches it made, the attn_combine launches it made)."""
    def counts():
        k = eng.stats()["kernels"]
        return [int(k.get(n, {"launches": 0})["launches"]) for n in ("attn", "attn_combine")]
    before = counts()
    out = step()
    after = counts()
    return out, after[0] - before[0], after[1] - before[1]


# ---- the base run R0 (once per model, never changed): t_0 .. t_79 through forward on a fresh graph engine, and on its eager twin
_BASE = {}


def _base(pkg, name, mix):
    key = (name, mix)
    if key not in _BASE:
        cfg = pkg.make_config(name, max_seq_len=sw.MAX_SEQ)
        model = pkg.SynthModel(cfg, mix=mix)
        V = cfg.vocab_size
        eng, eager = _twins(pkg, model)
        try:
            L, own = sw.run(eng, sw.BASE, V)
            blobs = {n: own[n].to_bytes() for n in sw.SAVE_AT}
            # rows are written once: a prefix of n rows saved at the end holds what one saved at position n held
            late = {n: eng.prefix_save(n).to_bytes() for n in (60, 66, 70, 76)}
            eng.kv_truncate(56)
            greedy = [int(t) for t in eng.decode_greedy(sw.token(56, V), 16)]
            L_eager, own_e = sw.run(eager, sw.BASE, V)
            blobs_eager = {n: own_e[n].to_bytes() for n in sw.SAVE_AT}
            nodes = int(eng.stats()["graph_nodes"])
        finally:
            eng.close()
            eager.close()
        two = _engine(pkg, model, attn_direct=2)                      # the switch at 128 rows: the head form through row 80
        try:
            L2, _ = sw.run(two, [("forward", 0, 70)], V)
        finally:
            two.close()
        for v in L + L_eager + L2:
            v.setflags(write=False)
        _BASE[key] = dict(cfg=cfg, model=model, V=V, L=L, L_eager=L_eager, L2=L2, blobs=blobs, blobs_eager=blobs_eager, late=late,
                          greedy=greedy, graph_nodes=nodes)
    return _BASE[key]


def _oracle(pkg, orc, name, mix, n, max_seq=sw.MAX_SEQ):
    return sw.oracle_logits(pkg, orc, name, mix, max_seq, n)


# =====================================================================================================================================
# 1. the switch is where the flags say, and both forms really run
# =====================================================================================================================================
@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_base_run_graph_equals_eager_and_follows_the_oracle_at_the_switch(pkg, orc, name, mix):
    b = _base(pkg, name, mix)
    assert b["graph_nodes"] > 0
    assert not _first_diff(b["L"], b["L_eager"]), _first_diff(b["L"], b["L_eager"])
    assert b["blobs"] == b["blobs_eager"]
    assert b["late"][60] == b["blobs"][60] and b["late"][70] == b["blobs"][70]
    want = _oracle(pkg, orc, name, mix, 67)
    worst = 0.0
    for i in (S - 2, S - 1, S, S + 1, S + 2):                         # steps attending 63 .. 67 rows
        err, tol = float(np.abs(b["L"][i] - want[i]).max()), sw.tol(want[i])
        worst = max(worst, err / tol)
        print("%s step attending %d rows: max|dlogit| %.3e, %.3f of the oracle bound" % (name, i + 1, err, err / tol))
        assert err <= tol, (i, err, tol)
    print("ORACLE_RATIO %s single context rows 63..67: worst %.3f of the bound" % (name, worst))


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_profiling_counters_show_the_form_of_every_step(pkg, name, mix):
    """attn_direct=1 under profiling (the eager path), t_0 .. t_69: `attn` launches == num_layers at every step; `attn_combine` 0 while
    the step attends <= 64 rows and num_layers from 65 rows on; logits those of the graph path and of FLAG_NO_GRAPH at every step."""
    b = _base(pkg, name, mix)
    layers = b["cfg"].num_layers
    eng = _engine(pkg, b["model"])
    try:
        eng.set_profiling(True)
        forms = []
        for i in range(70):
            got, attn, comb = _combine_launches(eng, lambda: eng.forward(sw.token(i, b["V"])))
            assert attn == layers, (i, attn)
            assert comb == (0 if i + 1 <= S else layers), "step attending %d rows made %d attn_combine launches" % (i + 1, comb)
            assert np.array_equal(_bits(got), _bits(b["L"][i])), "step %d: profiled (eager) logits differ from the graph's" % i
            assert np.array_equal(_bits(got), _bits(b["L_eager"][i])), i
            forms.append("split" if comb else "head")
        print("FORMS %s profiled forward: head at positions 0..%d, split at %d..69" % (name, forms.index("split") - 1, forms.index("split")))
        eng.set_profiling(False)
    finally:
        eng.close()


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_bits_show_the_form_engines_switching_at_64_and_128_rows(pkg, name, mix):
    """Identical at every step attending <= 64 rows (both run the head form), different at some step attending 65 .. 70 rows (the
    split form sums in another tree: about 1e-6 relative)."""
    b = _base(pkg, name, mix)
    for i in range(S):
        assert np.array_equal(_bits(b["L"][i]), _bits(b["L2"][i])), i
    differ = [i + 1 for i in range(S, 70) if not np.array_equal(_bits(b["L"][i]), _bits(b["L2"][i]))]
    print("FORMS %s switch at 64 vs at 128 rows: logits differ at the steps attending %s rows" % (name, differ))
    assert differ, "engines with the switch at 64 and at 128 rows never differ: the split form did not run"
    rel = max(float(np.abs(b["L"][i] - b["L2"][i]).max() / np.abs(b["L"][i]).max()) for i in range(S, 70))
    assert rel < 1e-4, rel                                            # another summation tree, not another context


def test_default_switch_is_at_256_rows(pkg):
    """A default engine and attn_direct=4 are the same engine: identical at every step through position 257.  Under profiling the
    default engine's attn_combine count flips between positions 255 (256 rows: head form) and 256 (257 rows: split + merge)."""
    name, mix = sw.MAIN
    cfg = pkg.make_config(name, max_seq_len=sw.DEFAULT_MAX_SEQ)
    model = pkg.SynthModel(cfg, mix=mix)
    V, layers = cfg.vocab_size, cfg.num_layers
    hs = _Handles()
    try:
        dflt = hs.make(_engine, pkg, model, attn_direct=0, max_seq=sw.DEFAULT_MAX_SEQ)
        four = hs.make(_engine, pkg, model, attn_direct=4, max_seq=sw.DEFAULT_MAX_SEQ)
        prof = hs.make(_engine, pkg, model, attn_direct=0, max_seq=sw.DEFAULT_MAX_SEQ)
        ops = sw.DEFAULT_SCENARIOS["default_switch"][1]
        kept, _ = sw.run(dflt, ops, V, max_seq=sw.DEFAULT_MAX_SEQ)
        same, _ = sw.run(four, ops, V, max_seq=sw.DEFAULT_MAX_SEQ)
        assert len(kept) == 258 and not _first_diff(kept, same), _first_diff(kept, same)
        assert dflt.position() == four.position() == 258
        assert dflt.prefix_save().to_bytes() == four.prefix_save().to_bytes()
        for i in range(250):
            prof.prefill_token(sw.token(i, V))
        prof.set_profiling(True)
        for i in range(250, 258):
            got, attn, comb = _combine_launches(prof, lambda: prof.forward(sw.token(i, V)))
            assert attn == layers and comb == (0 if i + 1 <= sw.DEFAULT_S else layers), (i, attn, comb)
            assert np.array_equal(_bits(got), _bits(kept[i])), i
        print("FORMS default engine: head at positions 0..255, split at 256..257 (attn_combine launches 0 -> %d)" % layers)
    finally:
        hs.close()


def test_threshold_above_the_cache_is_the_head_form_to_the_last_row(pkg, orc):
    """attn_direct=4 (256 rows) in a cache of 160: position 159 within the oracle bound and equal to eager."""
    name, mix = sw.MAIN
    b = _base(pkg, name, mix)
    want = _oracle(pkg, orc, name, mix, sw.MAX_SEQ)
    hs = _Handles()
    try:
        eng, eager = hs.make_twins(pkg, b["model"], attn_direct=4)
        prof = hs.make(_engine, pkg, b["model"], attn_direct=4)
        for i in range(sw.MAX_SEQ - 1):
            eng.prefill_token(sw.token(i, b["V"]))
            eager.prefill_token(sw.token(i, b["V"]))
            prof.prefill_token(sw.token(i, b["V"]))
        t = sw.token(sw.MAX_SEQ - 1, b["V"])
        got, got_e = eng.forward(t), eager.forward(t)
        prof.set_profiling(True)
        got_p, attn, comb = _combine_launches(prof, lambda: prof.forward(t))
        assert attn == b["cfg"].num_layers and comb == 0, (attn, comb)
        assert np.array_equal(_bits(got), _bits(got_e)) and np.array_equal(_bits(got), _bits(got_p))
        err, tol = float(np.abs(got - want[-1]).max()), sw.tol(want[-1])
        print("ORACLE_RATIO head form at 160 rows: %.3f of the bound" % (err / tol))
        assert err <= tol, (err, tol)
        assert eng.position() == sw.MAX_SEQ
        for call in (lambda: eng.forward(1), lambda: eng.prefill_token(1), lambda: eng.decode_greedy(1, 1)):
            with pytest.raises(pkg.BackendError) as ei:
                call()
            assert ei.value.variant == "InvalidArgument" and eng.position() == sw.MAX_SEQ
        assert eng.prefix_save().to_bytes() == eager.prefix_save().to_bytes()
    finally:
        hs.close()


def test_threshold_equal_to_the_cache_never_switches(pkg, orc):
    """attn_direct=1 with max_seq 64: decode to position 64 in the head form alone; the next forward, prefill_token and
    decode_greedy(.., 1) are InvalidArgument and leave the position alone."""
    name, mix = sw.MAIN
    cfg = pkg.make_config(name, max_seq_len=S)
    model = pkg.SynthModel(cfg, mix=mix)
    V = cfg.vocab_size
    want = _oracle(pkg, orc, name, mix, S, max_seq=S)
    eng, eager = _twins(pkg, model, max_seq=S)
    try:
        for i in range(S):
            a, e = eng.forward(sw.token(i, V)), eager.forward(sw.token(i, V))
            assert np.array_equal(_bits(a), _bits(e)), i
        err = float(np.abs(a - want[S - 1]).max())
        assert err <= sw.tol(want[S - 1]), (err, sw.tol(want[S - 1]))
        eng.reset()
        eager.reset()
        dev = eng.decode_greedy(sw.token(0, V), S).tolist()
        assert dev == eager.decode_greedy(sw.token(0, V), S).tolist()
        for e in (eng, eager):
            assert e.position() == S
            for call in (lambda: e.forward(1), lambda: e.prefill_token(1), lambda: e.decode_greedy(1, 1)):
                with pytest.raises(pkg.BackendError) as ei:
                    call()
                assert ei.value.variant == "InvalidArgument" and e.position() == S
    finally:
        eng.close()
        eager.close()


# =====================================================================================================================================
# 2. state operations across the switch, single context, both models
# =====================================================================================================================================
def _run_twins(pkg, b, ops, **kw):
    """`ops` on a graph engine and on its FLAG_NO_GRAPH twin: the same at every step and in the final cache bytes -> (outputs, bytes)."""
    eng, eager = _twins(pkg, b["model"], **kw)
    try:
        out, own = sw.run(eng, ops, b["V"], b["blobs"])
        out_e, own_e = sw.run(eager, ops, b["V"], b["blobs"])
        assert not _first_diff(out, out_e) and len(out) == len(out_e), "graph and eager differ at steps %s" % _first_diff(out, out_e)
        blob, blob_e = eng.prefix_save().to_bytes(), eager.prefix_save().to_bytes()
        assert blob == blob_e, "graph and eager engines end with different cache bytes"
        for n in own:
            assert own[n].to_bytes() == own_e[n].to_bytes(), n
        nodes = int(eng.stats()["graph_nodes"])
        assert nodes > 0 and eager.stats()["graph_nodes"] == 0
        return out, blob
    finally:
        eng.close()
        eager.close()


def _expect(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    bad = _first_diff(got, want)
    assert not bad, "%s: steps %s differ from the base run" % (what, bad)


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_rewind_and_restore_below_the_switch_with_both_graphs_captured(pkg, name, mix):
    """From position 80, kv_truncate(60) / prefix_restore(p60), then t_60 .. t_69: head form at 60 .. 63, split form again from 64."""
    b = _base(pkg, name, mix)
    for scenario in ("rewind", "restore_below"):
        out, blob = _run_twins(pkg, b, sw.SCENARIOS[scenario][1])
        _expect(out[:80], b["L"], scenario + " first pass")
        _expect(out[80:], b["L"][60:70], scenario)
        assert blob == b["blobs"][70], scenario + ": the cache bytes at 70 are not the base run's"
        print("FORMS %s %s: head at 0..63, split at 64..79; after the rewind head at 60..63, split at 64..69" % (name, scenario))


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_reset_then_replay(pkg, name, mix):
    b = _base(pkg, name, mix)
    out, blob = _run_twins(pkg, b, sw.SCENARIOS["reset"][1])
    _expect(out[:80], b["L"], "first pass")
    _expect(out[80:], b["L"], "replay after reset")
    assert blob == b["blobs"][80]
    print("FORMS %s reset: head at 0..63, split at 64..79, twice" % name)


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_restore_above_the_switch_over_other_rows(pkg, name, mix):
    """From 10 rows of other tokens (head form, head graph captured), prefix_restore(p70), then t_70 .. t_75 in the split form."""
    b = _base(pkg, name, mix)
    out, blob = _run_twins(pkg, b, sw.SCENARIOS["restore_above"][1])
    _expect(out[10:], b["L"][70:76], "restore above")
    assert blob == b["late"][76]
    print("FORMS %s restore_above: head at 0..9, split at 70..75" % name)


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_split_graph_captured_first_and_head_graph_late(pkg, name, mix):
    """A fresh engine whose first step ever comes behind prefix_from_bytes(p70) + restore: the split graph is captured and the head
    graph never is.  Then, on the same engine, kv_truncate(5) and six tokens: the head graph is captured after the split one.  Those
    six steps have the history t_0 .. t_4, t_5 .. t_10: the base run's steps 5 .. 10."""
    b = _base(pkg, name, mix)
    out, blob = _run_twins(pkg, b, sw.SCENARIOS["split_graph_first"][1])
    _expect(out, b["L"][70:76], "split graph first")
    assert blob == b["late"][76]
    out, blob = _run_twins(pkg, b, sw.SCENARIOS["head_graph_late"][1])
    _expect(out[:6], b["L"][70:76], "split graph first")
    _expect(out[6:], b["L"][5:11], "head graph late")
    print("FORMS %s split_graph_first: split at 70..75; head_graph_late: then head at 5..10" % name)


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_never_switching_twin_on_the_same_cache_bytes(pkg, name, mix):
    """p70's bytes imported into an attn_direct=255 engine, then t_70 .. t_75: the same cache bytes, and both engines run the split
    form there — bit for bit the base run."""
    b = _base(pkg, name, mix)
    out, blob = _run_twins(pkg, b, sw.SCENARIOS["split_graph_first"][1], attn_direct=255)
    _expect(out, b["L"][70:76], "never-switching twin")
    assert blob == b["late"][76]


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_shift_left_back_across_the_switch(pkg, orc, name, mix):
    """From 80, kv_shift_left(20), then six tokens from position 60 across 64: the eager twin bit for bit, and the oracle with the same
    kv_shift_left within the oracle bound."""
    b = _base(pkg, name, mix)
    out, _ = _run_twins(pkg, b, sw.SCENARIOS["shift"][1])
    _expect(out[:80], b["L"], "first pass")
    _, _, ref = sw.oracle_model(pkg, orc, name, mix, sw.MAX_SEQ)
    try:
        ref.forward(sw.tokens(0, 80, b["V"]))
        ref.kv_shift_left(20)
        worst = 0.0
        for j, i in enumerate(range(60, 66)):
            want = ref.forward([sw.token(i, b["V"])])
            err, tol = float(np.abs(out[80 + j] - want).max()), sw.tol(want)
            worst = max(worst, err / tol)
            assert err <= tol, (i, err, tol)
        print("ORACLE_RATIO %s after kv_shift_left(20), rows 61..66: worst %.3f of the bound" % (name, worst))
        print("FORMS %s shift: head at 60..63, split at 64..65 (both graphs captured before)" % name)
    finally:
        ref.close()


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_greedy_loop_crosses_the_switch_inside_one_call(pkg, orc, name, mix):
    """At position 56, decode_greedy(t_56, 16): steps 56 .. 71.  == the host arg-max loop over forward after kv_truncate(56), == a
    forward_argmax loop, == stage_read_tokens(56, 16); graph == eager in tokens, in the host loop's logits and in the cache bytes
    at 72 rows, which are the same behind the device loop and behind the host loops."""
    b = _base(pkg, name, mix)
    V = b["V"]
    eng, eager = _twins(pkg, b["model"])
    try:
        res = []
        for e in (eng, eager):
            out, _ = sw.run(e, sw.SCENARIOS["greedy_loop"][1], V)
            _expect(out[:56], b["L"][:56], "prompt")
            dev = out[56]
            assert e.position() == 72 and e.stage_read_tokens(56, 16).tolist() == dev
            after_loop = e.prefix_save().to_bytes()
            e.kv_truncate(56)
            host, logits, tok = [], [], sw.token(56, V)
            for _ in range(16):
                logits.append(e.forward(tok))
                tok = orc.argmax_last(logits[-1])
                host.append(tok)
            assert np.array_equal(_bits(logits[0]), _bits(b["L"][56]))
            e.kv_truncate(56)
            one, tok = [], sw.token(56, V)
            for _ in range(16):
                tok = e.forward_argmax(tok)
                one.append(tok)
            assert dev == host == one, (dev, host, one)
            assert e.stage_read_tokens(56, 16).tolist() == dev and e.position() == 72
            # the same tokens through three loops: the rows the device loop wrote are those the host loops write
            assert e.prefix_save().to_bytes() == after_loop, "the cache after decode_greedy differs from the cache after the host loops"
            res.append((dev, logits, after_loop))
        assert res[0][0] == res[1][0] == b["greedy"]
        assert not _first_diff(res[0][1], res[1][1])
        assert res[0][2] == res[1][2], "graph and eager engines end the greedy loop with different cache bytes"
        print("FORMS %s greedy_loop: one decode_greedy call, head at 56..63, split at 64..71" % name)
    finally:
        eng.close()
        eager.close()


def _forced_draws(ref_engine, cfg_s, prompt, n_steps, rng):
    """Teacher forcing with tests/sampler_ref.py: on ref_engine's own forward logits the restatement draws each uniform away from the
    cumulative sums -> (its tokens, the uniforms, how many leading steps are settled: a step whose top-p cut lies within 1e-5 of its
    boundary may go either way on the device whatever the draw, and the comparison with the restatement ends before it)."""
    from sampler_ref import Sampler, draw_unambiguous
    s = Sampler(ref_engine.vocab_size, **cfg_s)
    ref_engine.reset()
    ref_engine.forward_batch(prompt[:-1])
    ctx, tok, toks, unis, n_settled = list(prompt), prompt[-1], [], [], None
    for i in range(n_steps):
        r, tok, settled = draw_unambiguous(s, ref_engine.forward(tok), ctx, rng, tol=1e-5)
        if not settled and n_settled is None:
            n_settled = i
        unis.append(r)
        toks.append(tok)
        ctx.append(tok)
    return toks, np.array(unis, np.float32), n_steps if n_settled is None else n_settled


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_sampled_loop_crosses_the_switch_inside_one_call(pkg, name, mix):
    """set_sampler(creative), then decode_sample over steps 56 .. 71 with teacher-forced uniforms (drawn away from the decision
    boundaries on the eager twin's own logits): the graph engine's tokens == the eager twin's at every step, their cache bytes at 72
    rows agree, and the tokens are the restatement's (tests/sampler_ref.py) for as long as it decides away from its boundaries.
    On test-dense that is all 16 steps (asserted: at least past the switch).  On test-dense-d128 the top-p cut of step 0 lies within
    1e-5 of 0.9 — a property of that step's logits, whatever the seed — so the comparison with the restatement is empty there and
    the exact comparisons with the eager twin are what that case checks."""
    from sampler_ref import PRESETS
    b = _base(pkg, name, mix)
    V = b["V"]
    prompt = sw.tokens(0, 57, V)
    eng, eager = _twins(pkg, b["model"])
    try:
        want, unis, n = _forced_draws(eager, PRESETS["creative"], prompt, 16, np.random.default_rng(56))
        assert eager.position() == 72
        got, blobs = [], []
        for e in (eng, eager):
            e.reset()
            e.forward_batch(prompt[:-1])                               # (FLAG_EXACT_PREFILL: token by token)
            assert e.position() == 56
            e.set_sampler(**PRESETS["creative"])
            got.append(e.decode_sample(prompt[-1], prompt[:-1], 16, unis).tolist())
            assert e.position() == 72
            blobs.append(e.prefix_save().to_bytes())
        assert got[0] == got[1], (got[0], got[1])
        assert blobs[0] == blobs[1], "graph and eager engines end the sampled loop with different cache bytes"
        if name == "test-dense":
            assert n >= 10, n                                          # steps 56 .. 65: both forms against the restatement
        assert got[0][:n] == want[:n]
        print("FORMS %s sampled_loop: one decode_sample call, head at 56..63, split at 64..71 (%d of 16 steps settled)" % (name, n))
    finally:
        eng.close()
        eager.close()


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_batched_prompt_that_ends_next_to_the_switch(pkg, orc, name, mix):
    """Without FLAG_EXACT_PREFILL, forward_batch of 63, 64 and 65 tokens, then three forwards: the eager twin bit for bit (logits and the
    cache bytes at the end), the oracle
    within the 1e-2 bound; under profiling the first step after the 63-token prompt makes 0 attn_combine launches and the first after
    the 64-token prompt num_layers."""
    b = _base(pkg, name, mix)
    V, layers = b["V"], b["cfg"].num_layers
    want = _oracle(pkg, orc, name, mix, 68)
    hs = _Handles()
    try:
        eng, eager = hs.make_twins(pkg, b["model"], exact=False)
        prof = hs.make(_engine, pkg, b["model"], exact=False)
        assert eng.prefill_is_batched() and eager.prefill_is_batched() and prof.prefill_is_batched()
        worst = 0.0
        for n in (63, 64, 65):
            ops = sw.SCENARIOS["batched_%d" % n][1]
            outs = []
            for e in (eng, eager):
                outs.append(sw.run(e, [("reset",)] + ops, V)[0])
            assert not _first_diff(outs[0], outs[1]), (n, _first_diff(outs[0], outs[1]))
            assert eng.prefix_save().to_bytes() == eager.prefix_save().to_bytes(), "cache bytes behind a batched prompt of %d tokens" % n
            for j in range(3):
                err, tol = float(np.abs(outs[0][j] - want[n + j]).max()), sw.tol_batched(want[n + j])
                worst = max(worst, err / tol)
                assert err <= tol, (n, j, err, tol)
            prof.set_profiling(False)
            prof.reset()
            prof.forward_batch(sw.tokens(0, n, V))
            prof.set_profiling(True)
            got, attn, comb = _combine_launches(prof, lambda: prof.forward(sw.token(n, V)))
            assert attn == layers and comb == (0 if n + 1 <= S else layers), (n, attn, comb)
            assert np.array_equal(_bits(got), _bits(outs[0][0])), n
        print("ORACLE_RATIO %s behind batched prompts of 63..65 tokens: worst %.3f of the 1e-2 bound" % (name, worst))
        print("FORMS %s batched prompt: first step head after 63 tokens, split after 64 and 65" % name)
    finally:
        hs.close()


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_refusals_at_the_switch_change_nothing(pkg, name, mix):
    """At position 64: forward(vocab_size), prefill_token(vocab_size + 7) and a decode_greedy past max_seq are refused with
    InvalidArgument and the position stays; then forward(t_64) and forward(t_65) give the base run's steps, and the cache bytes at 66
    rows are the base run's."""
    b = _base(pkg, name, mix)
    out, blob = _run_twins(pkg, b, sw.SCENARIOS["refusals"][1])
    _expect(out, b["L"][:66], "refusals")
    assert blob == b["late"][66]


@pytest.mark.parametrize("name,mix", sw.MODELS)
def test_profiling_toggled_around_the_switch(pkg, name, mix):
    """set_profiling(True) for positions 62 .. 66 (eager launches between graph replays), then off: the base run at every step and
    in the cache bytes at 70 rows, on the graph engine and on its eager twin; the profiled steps made the launches of their form."""
    b = _base(pkg, name, mix)
    layers = b["cfg"].num_layers
    eng, eager = _twins(pkg, b["model"])
    try:
        for e in (eng, eager):
            out, _ = sw.run(e, sw.SCENARIOS["profiling_toggled"][1], b["V"])
            _expect(out, b["L"][:70], "profiling toggled")
            k = e.stats()["kernels"]
            assert k["attn"]["launches"] == 5 * layers and k["attn_combine"]["launches"] == 3 * layers
            assert e.prefix_save().to_bytes() == b["late"][70]
        assert eng.stats()["graph_nodes"] > 0 and eager.stats()["graph_nodes"] == 0
        print("FORMS %s profiling toggled: graph head 0..61, eager head 62..63, eager split 64..66, graph split 67..69" % name)
    finally:
        eng.close()
        eager.close()


# =====================================================================================================================================
# 3. pipelines and stage contexts
# =====================================================================================================================================
@pytest.mark.parametrize("stages", [2, 3])
def test_pipeline_equals_the_single_context_across_the_switch(pkg, stages):
    """HipPipeline with the switch at 64 rows in every stage (once through flags = 1 << 16, once through attn_direct=1: the same
    selector): forward at positions 0 .. 74, kv_truncate(60) + replay, reset + replay, decode_greedy from 56 over 16 steps, all the
    single context's bits; and the bits witness against a pipeline with the switch at 128 rows."""
    name, mix = sw.MAIN
    b = _base(pkg, name, mix)
    V = b["V"]
    L, ops = b["L"], sw.SCENARIOS["pipeline"][1]
    want = L[:75] + L[60:75] + L[:71] + [b["greedy"]]
    hs = _Handles()
    try:
        pipe = hs.make(pkg.HipPipeline.from_model, b["model"], sw.MAX_SEQ, stages, flags=sw.TP_FLAGS)
        named = hs.make(pkg.HipPipeline.from_model, b["model"], sw.MAX_SEQ, stages, attn_direct=sw.ATTN_DIRECT)
        two = hs.make(pkg.HipPipeline.from_model, b["model"], sw.MAX_SEQ, stages, attn_direct=2)
        with pytest.raises(ValueError):
            pkg.HipPipeline.from_model(b["model"], sw.MAX_SEQ, stages, flags=sw.TP_FLAGS, attn_direct=2)
        assert pipe.stages() == stages
        for p in (pipe, named):
            out, _ = sw.run(p, ops, V)
            _expect(out, want, "pipeline")
            assert p.position() == 72
        # the bits witness: the switch at 128 rows in every stage
        other, _ = sw.run(two, [("forward", 0, 70)], V)
        _expect(other, b["L2"], "pipeline with the switch at 128 rows")
        differ = [i + 1 for i in range(70) if not np.array_equal(_bits(other[i]), _bits(L[i]))]
        assert differ and min(differ) > S, differ
        print("FORMS pipeline of %d stages: head at 0..63, split from 64 (differs from the 128-row switch at rows %s)" % (stages, differ))
    finally:
        hs.close()


def test_stage_contexts_by_hand_rewound_across_the_switch(pkg):
    """Two stage contexts (layers [0, 2) and [2, 3)) driven with stage_forward and a device-to-device copy of the hidden vector.  At 70
    the first stage goes back to 60 by prefix_restore of its own layers, the second by kv_truncate; t_60 .. t_69 again."""
    name, mix = sw.MAIN
    b = _base(pkg, name, mix)
    V, H = b["V"], b["cfg"].hidden_size
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hs = _Handles()

    def step(i):
        s0, s1 = hs
        s0.stage_forward(sw.token(i, V))
        s0.synchronize()
        assert hip.hipMemcpy(s1.stage_hidden_ptr(), s0.stage_hidden_ptr(), H * 4, 3) == 0   # device to device
        assert hip.hipDeviceSynchronize() == 0
        return s1.stage_forward(0, want_logits=True)

    try:
        s0 = hs.make(_engine, pkg, b["model"], layer_range=(0, 2))
        s1 = hs.make(_engine, pkg, b["model"], layer_range=(2, 3))
        p60 = None
        for i in range(70):
            if i == 60:
                p60 = s0.prefix_save()
                assert (p60.info().layer_begin, p60.info().layer_end, p60.n_rows) == (0, 2, 60)
            assert np.array_equal(_bits(step(i)), _bits(b["L"][i])), i
        s0.prefix_restore(p60)
        s1.kv_truncate(60)
        assert s0.position() == s1.position() == 60
        for i in range(60, 70):
            assert np.array_equal(_bits(step(i)), _bits(b["L"][i])), "after the rewind, step %d" % i
        print("FORMS stage contexts: head at 0..63, split at 64..69; after the rewind head at 60..63, split at 64..69")
    finally:
        hs.close()


# =====================================================================================================================================
# 4. tensor-parallel handles
# =====================================================================================================================================
D128 = dict(intermediate_size=2048, num_kv_heads=4)                    # test_gpu_tp.py's overrides: the shards keep tile layouts


def _tp_setup(pkg, orc, n_oracle):
    name, mix = sw.MAIN
    cfg, model, ref = sw.oracle_model(pkg, orc, name, mix, sw.MAX_SEQ, **D128)
    ref.close()
    return cfg, model, sw.oracle_logits(pkg, orc, name, mix, sw.MAX_SEQ, n_oracle, **D128)


@pytest.mark.parametrize("n", [1, 2, 4])
def test_tensor_parallel_across_the_switch(pkg, orc, n):
    """N ranks with the switch at 64 rows: graph == FLAG_NO_GRAPH at every step, the bits witness against the switch at 128 rows, the
    oracle bound at the steps attending 64, 65 and 66 rows, kv_truncate(60) from 75 + replay == the first pass, decode_greedy from 56
    over 16 steps == the host loop."""
    hb = pkg.hip_backend
    cfg, model, want = _tp_setup(pkg, orc, 68)
    V = cfg.vocab_size
    TP = pkg.HipTensorParallel
    ops = sw.SCENARIOS["tensor_parallel"][1]
    hs = _Handles()
    try:
        tp = hs.make(TP.from_model, model, sw.MAX_SEQ, n, flags=sw.TP_FLAGS)
        eager = hs.make(TP.from_model, model, sw.MAX_SEQ, n, flags=hb.FLAG_NO_GRAPH, attn_direct=sw.ATTN_DIRECT)   # the same selector
        two = hs.make(TP.from_model, model, sw.MAX_SEQ, n, attn_direct=2)
        with pytest.raises(ValueError):
            TP.from_model(model, sw.MAX_SEQ, n, flags=sw.TP_FLAGS, attn_direct=2)
        assert tp.ranks() == n
        out, _ = sw.run(tp, ops, V)
        out_e, _ = sw.run(eager, ops, V)
        assert tp.graph_nodes() > 0 and eager.graph_nodes() == 0
        assert len(out) == len(out_e) == 91 and not _first_diff(out, out_e), "graph and eager ranks differ at steps %s" % _first_diff(out, out_e)
        first = out[:75]
        _expect(out[75:90], first[60:75], "ranks after kv_truncate(60)")
        other, _ = sw.run(two, [("forward", 0, 70)], V)
        for i in range(S):
            assert np.array_equal(_bits(other[i]), _bits(first[i])), i
        differ = [i + 1 for i in range(S, 70) if not np.array_equal(_bits(other[i]), _bits(first[i]))]
        assert differ, "ranks with the switch at 64 and at 128 rows never differ: the ranks' split + merge did not run"
        worst = 0.0
        for i in (S - 1, S, S + 1):
            err, tol = float(np.abs(first[i] - want[i]).max()), sw.tol(want[i])
            worst = max(worst, err / tol)
            assert err <= tol, (n, i, err, tol)
        print("ORACLE_RATIO tensor parallel N=%d rows 64..66: worst %.3f of the bound" % (n, worst))
        print("FORMS tensor parallel N=%d: head at 0..63, split from 64 (differs from the 128-row switch at rows %s)" % (n, differ))
        dev = out[90]
        for e in (tp, eager):
            assert e.position() == 72
            e.kv_truncate(56)
            host, tok = [], sw.token(56, V)
            for _ in range(16):
                tok = orc.argmax_last(e.forward(tok))
                host.append(tok)
            assert dev == host, (n, dev, host)
    finally:
        hs.close()


@pytest.mark.parametrize("n", [1, 2, 4])
def test_tensor_parallel_batched_prompt_next_to_the_switch(pkg, orc, n):
    """Where the ranks take the batched prompt pass: forward_batch of 63, 64 and 65 tokens, then three forwards; graph == eager bit for
    bit, the oracle within the 1e-2 bound."""
    hb = pkg.hip_backend
    cfg, model, want = _tp_setup(pkg, orc, 68)
    V = cfg.vocab_size
    hs = _Handles()
    try:
        tp = hs.make(pkg.HipTensorParallel.from_model, model, sw.MAX_SEQ, n, flags=sw.TP_FLAGS)
        eager = hs.make(pkg.HipTensorParallel.from_model, model, sw.MAX_SEQ, n, flags=sw.TP_FLAGS | hb.FLAG_NO_GRAPH)
        assert tp.prefill_is_batched() == eager.prefill_is_batched()
        if not tp.prefill_is_batched():
            print("tensor parallel N=%d: the ranks feed prompts token by token; nothing batched to check" % n)
            return
        worst = 0.0
        for m in (63, 64, 65):
            outs = []
            for e in (tp, eager):
                e.reset()
                e.forward_batch(sw.tokens(0, m, V))
                assert e.position() == m
                outs.append([e.forward(sw.token(i, V)) for i in range(m, m + 3)])
            assert not _first_diff(outs[0], outs[1]), (n, m, _first_diff(outs[0], outs[1]))
            for j in range(3):
                err, tol = float(np.abs(outs[0][j] - want[m + j]).max()), sw.tol_batched(want[m + j])
                worst = max(worst, err / tol)
                assert err <= tol, (n, m, j, err, tol)
        print("ORACLE_RATIO tensor parallel N=%d behind batched prompts of 63..65 tokens: worst %.3f of the 1e-2 bound" % (n, worst))
    finally:
        hs.close()
