"""A float64 restatement of a block of prompt tokens over a TurboQuantMSE cache: the reference's write_kv followed by attention_layer
for every token of the block (kv_turboquant.rs:88-201), which is `attention_ref.prefill` over the values the code rows stand for,
R^-1(centroid[code]).  Every row takes part through its codes, a token's own row included.  Shared by tests/test_tq_prefill_ref.py
(against the oracle, on the CPU) and tests/test_gpu_tq_prefill.py (the arbiter of the batched path's kernels)."""
from __future__ import annotations

import numpy as np

import attention_ref as ar


def row_bytes(bits: int, d: int) -> int:
    return d // 4 if bits == 2 else d // 8 * 3


def make_signs(rng, n_kv: int, d: int) -> np.ndarray:
    return np.where(rng.random((n_kv, 2, d)) < 0.5, -1.0, 1.0).astype(np.float32)


def compress_rows(orc, rows, bits: int, signs) -> np.ndarray:
    """rows [n_kv, n, d] f32, signs [n_kv, d] -> the oracle's code rows [n_kv, n, row bytes]."""
    return np.stack([np.stack([orc.tq_compress(x, bits, signs[h]) for x in rows[h]]) for h in range(rows.shape[0])])


def values(orc, k_codes, v_codes, bits: int, d: int, signs, n: int, v_sign_index: int = 1):
    """K / V [n_kv, n, d] float64: what rows 0..n-1 of the code caches stand for.  v_sign_index 0 plants the mistake of
    inverting V's rotation with K's signs."""
    K = np.stack([ar.tq_values(orc, k_codes[h, :n], bits, d, signs[h, 0]) for h in range(k_codes.shape[0])])
    V = np.stack([ar.tq_values(orc, v_codes[h, :n], bits, d, signs[h, v_sign_index]) for h in range(v_codes.shape[0])])
    return K, V


def visibility(pos0: int, m: int, shift: int = 0, drop_last: bool = False) -> np.ndarray:
    """[m, pos0 + m] bool: token t sees rows <= pos0 + t.  shift 1 plants a mask that is off by one (a token sees the row after its
    own); drop_last hides the last row from the last token."""
    n = pos0 + m
    vis = np.arange(n)[None, :] <= (pos0 + np.arange(m) + shift)[:, None]
    if drop_last:
        vis[m - 1, n - 1] = False
    return vis


def attend(q, K, V, scale: float, vis) -> np.ndarray:
    """out [m, n_heads, d] in float64 under a given visibility matrix (attention_ref.prefill is the case visibility(pos0, m))."""
    q = np.asarray(q, np.float64)
    g = q.shape[1] // K.shape[0]
    Kh, Vh = np.repeat(K, g, axis=0), np.repeat(V, g, axis=0)
    s = np.matmul(q.transpose(1, 0, 2), Kh.transpose(0, 2, 1)) * scale
    s = np.where(vis[None], s, -np.inf)
    s = s - s.max(axis=-1, keepdims=True)
    w = np.exp(s)
    w = w / w.sum(axis=-1, keepdims=True)
    return np.matmul(w, Vh).transpose(1, 0, 2)


def block(orc, q, k_codes, v_codes, bits: int, signs, scale: float, pos0: int, m: int) -> np.ndarray:
    """The reference: out [m, n_heads, d] float64 of the block's tokens; q [m, n_heads, d]; codes [n_kv, rows, row bytes]."""
    K, V = values(orc, k_codes, v_codes, bits, np.asarray(q).shape[2], signs, pos0 + m)
    return ar.prefill(q, K, V, scale, pos0, m)


def magnitudes(orc, q, k_codes, v_codes, bits: int, signs, scale: float, n: int):
    """(S, vmax) of the bound, as attention_ref.tq_decode computes them, over every token of the block and rows 0..n-1."""
    q = np.asarray(q, np.float64)
    m, nh, d = q.shape
    n_kv = k_codes.shape[0]
    g = nh // n_kv
    s_mag = vmax = 0.0
    for kvh in range(n_kv):
        ck = np.abs(ar.tq_centroids(orc, k_codes[kvh, :n], bits, d))
        cv = ar.tq_centroids(orc, v_codes[kvh, :n], bits, d)
        vmax = max(vmax, float(np.abs(cv).sum(axis=1).max() / np.sqrt(d)))
        qg = q[:, kvh * g:(kvh + 1) * g].reshape(-1, d)
        rq_abs = np.abs(ar.tq_rotate(qg, signs[kvh, 0])) + np.log2(d) * ar.U * np.abs(qg).sum(axis=1, keepdims=True) / np.sqrt(d)
        s_mag = max(s_mag, float(scale * (rq_abs @ ck.T).max()))
    return s_mag, vmax


# ---- model level: the logits after a prompt, against a reference that was fed the same tokens
def logit_tol(want) -> float:
    """The batched prompt path's tolerance (tests/test_gpu_prefill.py): 1e-2 max|logit| + 1e-2."""
    return 1e-2 * float(np.abs(want).max()) + 1e-2


def follow(orc, forward_got, ref, prompt, n_steps: int = 4):
    """`ref` (an oracle model at position 0) is fed `prompt`; the side under test has been fed it already and answers
    forward_got(token) -> logits.  n_steps tokens, the reference's greedy token to both sides.
    -> per step (max|dlogit|, tol, the reference's top-1 / top-2 gap, same arg-max)."""
    want = ref.forward(list(prompt))
    out = []
    for _ in range(n_steps):
        tok = orc.argmax_last(want)
        got, want = forward_got(tok), ref.forward([tok])
        srt = np.sort(want)
        out.append((float(np.abs(got - want).max()), logit_tol(want), float(srt[-1] - srt[-2]), orc.argmax_last(got) == orc.argmax_last(want)))
    return out


def oracle_model(orc, cfg, model, perturb=None):
    """The oracle's model of a synthetic model; perturb(name, data) -> data replaces a tensor's payload."""
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, perturb(nm, data) if perturb else data)
    ref.finalize()
    return ref


def model_signs(cfg, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.where(rng.integers(0, 2, cfg.num_layers * cfg.num_kv_heads * 2 * cfg.head_dim) == 1, 1.0, -1.0).astype(np.float32)


def prompt_tokens(cfg, n: int):
    return [(7 * i + 3) % cfg.vocab_size for i in range(n)]
