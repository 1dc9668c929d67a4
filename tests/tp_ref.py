"""Shared by the tensor-parallel tests: numpy restatements of lgh_tp_shard's slicing and of the rank-order sum, the partial-vector
generators, and the oracle's logits of a config (computed once per session and never changed)."""
import numpy as np

BLOCK = {"F32": (1, 4), "Q4_0": (32, 18), "Q8_0": (32, 34), "Q4_K": (256, 144), "Q5_K": (256, 176), "Q6_K": (256, 210)}
TYPE = {"F32": 0, "Q4_0": 2, "Q8_0": 8, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14}


def row_range(ne1: int, rank: int, n: int):
    """Rows of rank `rank`: equal ranges where n divides ne1, otherwise the same number of whole 16-row tiles per rank and the
    remainder to the last one."""
    if ne1 % n == 0:
        return ne1 // n * rank, ne1 // n * (rank + 1)
    per = (ne1 + 15) // 16 // n
    return per * 16 * rank, ne1 if rank + 1 == n else per * 16 * (rank + 1)


def shard_elems(dense: np.ndarray, axis: int, rank: int, n: int) -> np.ndarray:
    """The slice of the dequantized [ne1, ne0] tensor that rank `rank` holds."""
    ne1, ne0 = dense.shape
    if axis == 0:
        r0, r1 = row_range(ne1, rank, n)
        return dense[r0:r1]
    return dense[:, ne0 // n * rank:ne0 // n * (rank + 1)]


def ordered_sum(partials: np.ndarray, resid=None) -> np.ndarray:
    """resid + (((p0 + p1) + p2) ...) in f32, one rounding per add."""
    s = partials[0].astype(np.float32).copy()
    for p in partials[1:]:
        s = (s + p.astype(np.float32)).astype(np.float32)
    return s if resid is None else (resid.astype(np.float32) + s).astype(np.float32)


def partials(kind: str, n: int, H: int, seed: int) -> np.ndarray:
    """gauss: N(0, 1).  orders: per element values of magnitude 1 and 2^-20 with either sign — (1 + -1) + t and 1 + (-1 + t) differ,
    so any order other than rank order changes bits."""
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, H)).astype(np.float32)
    big = rng.integers(0, 2, (n, H)).astype(bool)
    mag = np.where(big, 1.0, 2.0 ** -20 * (1.0 + rng.random((n, H))))
    return (mag * rng.choice([-1.0, 1.0], (n, H))).astype(np.float32)


_REF = {}


def oracle_logits(pkg, orc, name: str, mix: str, overrides: dict, n_prompt: int, n_steps: int, max_seq: int, with_bias: bool = False):
    """(config, model, prompt, fed tokens, logits): the oracle's logits after the prompt and after each of n_steps further greedy
    tokens (its own arg-max fed back), on the UNSHARDED model."""
    key = (name, mix, tuple(sorted(overrides.items())), n_prompt, n_steps, max_seq, with_bias)
    if key not in _REF:
        cfg = pkg.make_config(name, max_seq_len=max_seq, **overrides)
        model = pkg.SynthModel(cfg, mix=mix, with_bias=with_bias)
        ref = orc.Model(cfg.as_dict())
        for nm, t, ne, data in model.tensors(keep=True):
            ref.add_tensor(nm, t, ne, data)
        ref.finalize()
        prompt = [(7 + 37 * i) % cfg.vocab_size for i in range(n_prompt)]
        logits, fed = [ref.forward(prompt).copy()], []
        for _ in range(n_steps):
            fed.append(orc.argmax_last(logits[-1]))
            logits.append(ref.forward([fed[-1]]).copy())
        ref.close()
        for v in logits:
            v.setflags(write=False)
        _REF[key] = (cfg, model, prompt, fed, logits)
    return _REF[key]
