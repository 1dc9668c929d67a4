"""Shared by the tests that take an engine across the decode-attention switch (test_gpu_attn_switch.py, the cold_switch_single / cold_split_first /
cold_tensor_parallel_switch scenarios of fresh_scenarios.py) and by their CPU check (test_switch_scenarios_ref.py).

Decode attention over the f32 cache runs as ONE launch (attn_head_kernel) while the step attends at most `direct_attn_max_kv` rows and
as splits + merge beyond; each form has its own captured graph, picked per token from the HOST-side position, while the kernels read the
position from the device state.  Here the switch sits at S = 64 rows (attn_direct=1; HipPipeline / HipTensorParallel: flags = 1 << 16)
in a cache of 160 rows, so a scenario of a few tokens passes it in either direction.  The step at position p attends p + 1 rows:
positions 0 .. 63 take the head form, 64 .. the split form.

A scenario is a list of operations; `rows_attended` replays their effect on the position (nothing else) and gives the rows every step
attends, which is how the CPU test checks that a scenario claiming to cross S does: a step attending S rows and one attending S + 1.
`run` applies the same list to an engine.

  ("forward", i0, i1)      forward(t_i) for i in [i0, i1): one step each, logits kept
  ("other", n)             forward of n tokens that are NOT t_i (u_j = (29 j + 11) % vocab): rows in the way
  ("truncate", n)          kv_truncate(n)
  ("reset",)               reset()
  ("shift", n)             kv_shift_left(n)
  ("restore", rows)        prefix_restore of the prefix `rows` rows long that this engine saved itself when it passed that position
  ("import", rows)         prefix_from_bytes(the base run's blob of `rows` rows) + prefix_restore
  ("greedy", i, n)         decode_greedy(t_i, n): n steps inside one call
  ("batch", n)             forward_batch(t_0 .. t_{n-1})
  ("prefill", i0, i1)      prefill_token(t_i) for i in [i0, i1): one step each, nothing kept
  ("refused",)             three calls that must be refused and leave the position alone
  ("profiling", on)        set_profiling(on)
"""
import numpy as np

S = 64                      # rows: the last context of the head form under attn_direct=1
ATTN_DIRECT = 1
MAX_SEQ = 160
TP_FLAGS = ATTN_DIRECT << 16          # HipPipeline / HipTensorParallel take the selector in the flags word
MODELS = [("test-dense-d128", "Q4_K_M"), ("test-dense", "Q4_K_M")]
MAIN = MODELS[0]
SAVE_AT = (60, 70, 80)      # the base run saves a prefix when its position is one of these
BASE_TOKENS = 80


def token(i, vocab):
    return (13 * i + 5) % vocab


def tokens(i0, i1, vocab):
    return [token(i, vocab) for i in range(i0, i1)]


def other_tokens(n, vocab):
    return [(29 * j + 11) % vocab for j in range(n)]


def tol(want):
    """The decode tolerance against the oracle."""
    return 2e-3 * float(np.abs(want).max()) + 2e-3


def tol_batched(want):
    """... and behind a batched prompt (the f16 matrix-core GEMMs)."""
    return 1e-2 * float(np.abs(want).max()) + 1e-2


# name -> (crosses S, operations).  Every scenario starts from a fresh engine at position 0; every entry is run by a GPU test.
BASE = [("forward", 0, BASE_TOKENS)]
SCENARIOS = {
    "base": (True, BASE),
    "rewind": (True, BASE + [("truncate", 60), ("forward", 60, 70)]),
    "reset": (True, BASE + [("reset",), ("forward", 0, BASE_TOKENS)]),
    "restore_below": (True, BASE + [("restore", 60), ("forward", 60, 70)]),
    "restore_above": (False, [("other", 10), ("import", 70), ("forward", 70, 76)]),
    "split_graph_first": (False, [("import", 70), ("forward", 70, 76)]),
    "head_graph_late": (False, [("import", 70), ("forward", 70, 76), ("truncate", 5), ("forward", 5, 11)]),
    "shift": (True, BASE + [("shift", 20), ("forward", 60, 66)]),
    "greedy_loop": (True, [("forward", 0, 56), ("greedy", 56, 16)]),
    "batched_63": (True, [("batch", 63), ("forward", 63, 66)]),
    "batched_64": (False, [("batch", 64), ("forward", 64, 67)]),
    "batched_65": (False, [("batch", 65), ("forward", 65, 68)]),
    "refusals": (True, [("forward", 0, 64), ("refused",), ("forward", 64, 66)]),
    "profiling_toggled": (True, [("forward", 0, 62), ("profiling", True), ("forward", 62, 67), ("profiling", False), ("forward", 67, 70)]),
    "pipeline": (True, [("forward", 0, 75), ("truncate", 60), ("forward", 60, 75), ("reset",), ("forward", 0, 71), ("truncate", 56),
                        ("greedy", 56, 16)]),
    "tensor_parallel": (True, [("forward", 0, 75), ("truncate", 60), ("forward", 60, 75), ("truncate", 56), ("greedy", 56, 16)]),
    "cold_switch": (True, [("prefill", 0, 60), ("greedy", 60, 10), ("forward", 70, 71)]),
}
# the default switch (attn_direct=0 -> 256 rows), used by one test and one cold scenario
DEFAULT_S = 256
DEFAULT_MAX_SEQ = 288
DEFAULT_SCENARIOS = {
    "default_switch": (True, [("forward", 0, 258)]),
    "cold_split_first": (False, [("batch", 257), ("greedy", 257, 4)]),
}


def replay(ops):
    """(the rows each decode step of `ops` attends, in order; the position `ops` ends at).  A batched prompt's tokens are no decode
    steps."""
    pos, rows = 0, []
    for op in ops:
        kind = op[0]
        if kind in ("forward", "prefill"):
            rows += list(range(pos + 1, pos + op[2] - op[1] + 1))
            pos += op[2] - op[1]
        elif kind in ("other", "greedy"):
            rows += list(range(pos + 1, pos + op[-1] + 1))
            pos += op[-1]
        elif kind == "truncate":
            pos = min(pos, op[1])
        elif kind == "reset":
            pos = 0
        elif kind == "shift":
            pos = max(pos - op[1], 0)
        elif kind in ("restore", "import"):
            pos = op[1]
        elif kind == "batch":
            pos += op[1]
        elif kind not in ("refused", "profiling"):
            raise ValueError(kind)
    return rows, pos


def rows_attended(ops):
    return replay(ops)[0]


def final_position(ops):
    return replay(ops)[1]


def _refused(eng, vocab, max_seq):
    """forward(vocab_size), prefill_token(vocab_size + 7) and a decode_greedy past max_seq: InvalidArgument, the position unchanged."""
    pos = eng.position()
    for call in (lambda: eng.forward(vocab), lambda: eng.prefill_token(vocab + 7), lambda: eng.decode_greedy(1, max_seq - pos + 1)):
        try:
            call()
        except Exception as e:   # the package's BackendError
            assert getattr(e, "variant", None) == "InvalidArgument", e
        else:
            raise AssertionError("a call that must be refused at position %d was taken" % pos)
        assert eng.position() == pos


def run(eng, ops, vocab, blobs=None, max_seq=MAX_SEQ):
    """`ops` on `eng` -> what every step gave, in order: the logits of a forward, the token list of a greedy call.  The engine saves
    a prefix of its own whenever its position first reaches one of SAVE_AT during a "forward"; those are what "restore" restores, and
    they are returned next to the outputs."""
    out, own = [], {}
    for op in ops:
        kind = op[0]
        if kind == "forward":
            for i in range(op[1], op[2]):
                out.append(eng.forward(token(i, vocab)))
                if eng.position() in SAVE_AT and eng.position() not in own and hasattr(eng, "prefix_save"):
                    own[eng.position()] = eng.prefix_save()
        elif kind == "prefill":
            for i in range(op[1], op[2]):
                eng.prefill_token(token(i, vocab))
        elif kind == "other":
            for t in other_tokens(op[1], vocab):
                out.append(eng.forward(t))
        elif kind == "truncate":
            eng.kv_truncate(op[1])
        elif kind == "reset":
            eng.reset()
        elif kind == "shift":
            eng.kv_shift_left(op[1])
        elif kind == "restore":
            eng.prefix_restore(own[op[1]])
        elif kind == "import":
            eng.prefix_restore(eng.prefix_from_bytes(blobs[op[1]]))
        elif kind == "greedy":
            out.append([int(t) for t in eng.decode_greedy(token(op[1], vocab), op[2])])
        elif kind == "batch":
            eng.forward_batch(tokens(0, op[1], vocab))
        elif kind == "refused":
            _refused(eng, vocab, max_seq)
        elif kind == "profiling":
            eng.set_profiling(op[1])
        else:
            raise ValueError(kind)
    assert eng.position() == final_position(ops), (eng.position(), final_position(ops))
    return out, own


_ORACLE = {}


def oracle_model(pkg, orc, name, mix, max_seq, **over):
    """(config, synthetic model, a fresh oracle model on the same weights).  The synthetic model is made once per key."""
    key = (name, mix, max_seq, tuple(sorted(over.items())))
    if key not in _ORACLE:
        cfg = pkg.make_config(name, max_seq_len=max_seq, **over)
        _ORACLE[key] = (cfg, pkg.SynthModel(cfg, mix=mix))
    cfg, model = _ORACLE[key]
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    return cfg, model, ref


_ORACLE_LOGITS = {}


def oracle_logits(pkg, orc, name, mix, max_seq, n, **over):
    """The oracle's logits for t_0 .. t_{n-1} fed one by one (computed once per key, read-only)."""
    key = (name, mix, max_seq, n, tuple(sorted(over.items())))
    if key not in _ORACLE_LOGITS:
        cfg, _, ref = oracle_model(pkg, orc, name, mix, max_seq, **over)
        L = [ref.forward([token(i, cfg.vocab_size)]).copy() for i in range(n)]
        ref.close()
        for v in L:
            v.setflags(write=False)
        _ORACLE_LOGITS[key] = L
    return _ORACLE_LOGITS[key]
