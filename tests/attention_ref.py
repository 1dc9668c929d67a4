"""A float64 restatement of the engine's attention, the arbiter of the kernel-level attention tests (tests/test_gpu_attention.py).

Every kernel path computes  out = softmax(scale * q . K^T) . V  over cached rows whose stored values the tests know bit for bit
(the row encoders are bit-exact with the oracle).  Here that is done in float64 with a max-subtracted softmax, the GQA mapping
kv head = head // G, and, for a prompt block, the causal visibility  row <= pos0 + t.  The readers below turn stored bytes into
the values a kernel reads; TurboQuant rows are read as R^-1(centroid[code]) with R = H D / sqrt(d) (H the Sylvester Hadamard
matrix, D the sign vector), in float64.  R is orthogonal, so q . R^-1 c = (R q) . c: the kernel's rotated-space product.

Error bound (`bound`): a kernel's result is an f32 computation of the same sum.  Per score it adds |terms| = scale * sum_i |q_i k_i|
in some order, so its score error is at most a small multiple of u * S, S = max over visible rows of that sum (u = 2^-24).  A
softmax weight then carries a relative error of the same order (the max shift cancels exactly; exp adds ~2 ulp plus u times the
distance from the max, which the weights fall off much faster than), and a convex combination of V rows turns relative weight
errors into an absolute error <= that times max|V|.  The f32 accumulation of n weighted rows adds its own rounding; those
rounding errors are independent and grow as sqrt(n) (a worst-case n would hide a dropped row at long context).  Together:

    |got - ref| <= C * u * (1 + S + sqrt(n)) * max|V|,   C = 32

For TurboQuant the kernel multiplies the rotated query R q (an f32 Walsh-Hadamard transform: log2(d) additions per coordinate,
each coordinate off by at most e = log2(d) u ||q||_1 / sqrt(d)) with centroids c, and adds the QJL correction
coeff * |r| * sum_i (S R q)_i sign_i, so S sums the absolute terms of those products:
scale * (sum_i (|(R q)_i| + e) |c_i| + coeff * |r| * sum_ij |S_ij| (|(R q)_j| + e)); and max|V| is replaced by
max ||c_V||_1 / sqrt(d), which bounds every coordinate of R^-1 c_V.  The prompt pass stores f16: add 2^-11 |ref| + 2^-24."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
C = 32.0
F16_REL, F16_ABS = 2.0 ** -11, 2.0 ** -24
QJL_COEFF = float(np.sqrt(np.pi / 2))   # / d: QjlProjector::inner_product_fast (sqrt(pi / 2) / dim)


# ---- the operations
def _softmax_rows(s: np.ndarray) -> np.ndarray:
    s = s - s.max(axis=-1, keepdims=True)
    w = np.exp(s)
    return w / w.sum(axis=-1, keepdims=True)


def weights(q, K, scale: float, kv_len: int) -> np.ndarray:
    """Softmax weights [n_heads, kv_len] of one decode query q [n_heads, d] over rows 0..kv_len-1 of K [n_kv, rows, d]."""
    q, K = np.asarray(q, np.float64), np.asarray(K[:, :kv_len], np.float64)
    g = q.shape[0] // K.shape[0]
    s = np.matmul(np.repeat(K, g, axis=0), q[:, :, None])[:, :, 0] * scale
    return _softmax_rows(s)


def decode(q, K, V, scale: float, kv_len: int) -> np.ndarray:
    """out [n_heads, d] of one query at position kv_len - 1; K / V [n_kv, rows, d] (values as the kernel reads them)."""
    g = np.asarray(q).shape[0] // K.shape[0]
    w = weights(q, K, scale, kv_len)
    return np.matmul(w[:, None, :], np.repeat(np.asarray(V[:, :kv_len], np.float64), g, axis=0))[:, 0]


def decode_scores(scores, V) -> np.ndarray:
    """out [n_heads, d] from scaled scores [n_heads, n] and per-head V rows [n_heads, n, d]."""
    return np.einsum("hp,hpd->hd", _softmax_rows(np.asarray(scores, np.float64)), np.asarray(V, np.float64))


def prefill(q, K, V, scale: float, pos0: int, m: int) -> np.ndarray:
    """out [m, n_heads, d] of the prompt tokens pos0..pos0+m-1, q [m, n_heads, d]; token t sees rows <= pos0 + t."""
    q = np.asarray(q, np.float64)
    n = pos0 + m
    g = q.shape[1] // K.shape[0]
    Kh = np.repeat(np.asarray(K[:, :n], np.float64), g, axis=0)   # [heads, n, d]
    Vh = np.repeat(np.asarray(V[:, :n], np.float64), g, axis=0)
    s = np.matmul(q.transpose(1, 0, 2), Kh.transpose(0, 2, 1)) * scale   # [heads, m, n]
    vis = np.arange(n)[None, :] <= (pos0 + np.arange(m))[:, None]        # [m, n]
    s = np.where(vis[None], s, -np.inf)
    return np.matmul(_softmax_rows(s), Vh).transpose(1, 0, 2)


# ---- error bounds
def magnitude(q, K, scale: float, kv_len: int) -> float:
    """S = max over heads and visible rows of scale * sum_i |q_i k_i|."""
    q, K = np.abs(np.asarray(q, np.float64)), np.abs(np.asarray(K[:, :kv_len], np.float64))
    g = q.shape[-2] // K.shape[0]
    qq = q.reshape(-1, q.shape[-2], q.shape[-1])
    return float(scale * np.matmul(qq.transpose(1, 0, 2), np.repeat(K, g, axis=0).transpose(0, 2, 1)).max())


def bound(S: float, vmax: float, n: int) -> float:
    return C * U * (1.0 + S + np.sqrt(n)) * vmax


def worst_ratio(got, ref, S: float, vmax: float, n: int, f16: bool = False) -> float:
    """max |got - ref| / bound; NaN in `got` counts as infinitely wrong."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    b = bound(S, vmax, n) + (F16_REL * np.abs(ref) + F16_ABS if f16 else 0.0)
    err = np.abs(got - ref)
    err = np.where(np.isfinite(got), err, np.inf)
    return float((err / b).max())


# ---- readers: stored bytes -> the values a kernel reads
def int8_values(b, scales) -> np.ndarray:
    """QuantizedKVCache int8: scale * q.  b [..., d] int8 / uint8, scales [...]."""
    return np.asarray(b).view(np.int8).astype(np.float64) * np.asarray(scales, np.float64)[..., None]


def fp8_table(orc, kv_cache_type: int) -> np.ndarray:
    """The 256 values an FP8 byte decodes to (kv_cache_type 2 = E4M3, 3 = E5M2), from the oracle's dequantizer."""
    fmt = {2: orc.FP8_E4M3, 3: orc.FP8_E5M2}[kv_cache_type]
    return np.array([orc.kv_dequantize_fp8(fmt, b) for b in range(256)], np.float64)


def hadamard(d: int) -> np.ndarray:
    H = np.ones((1, 1))
    while H.shape[0] < d:
        H = np.block([[H, H], [H, -H]])
    return H


def tq_rotate(x, signs) -> np.ndarray:
    """R x = H (D x) / sqrt(d) along the last axis, float64."""
    x, signs = np.asarray(x, np.float64), np.asarray(signs, np.float64)
    d = x.shape[-1]
    return (x * signs) @ hadamard(d) / np.sqrt(d)


def tq_rotate_inverse(y, signs) -> np.ndarray:
    """R^-1 y = D H y / sqrt(d) (H is symmetric and H H = d I)."""
    y = np.asarray(y, np.float64)
    d = y.shape[-1]
    return (y @ hadamard(d)) / np.sqrt(d) * np.asarray(signs, np.float64)


def tq_indices(codes, bits: int, d: int) -> np.ndarray:
    """Packed rows [..., row bytes] -> code indices [..., d] (2 bits: 4 per byte; 3 bits: 8 per little-endian 24-bit group)."""
    c = np.asarray(codes, np.uint8).astype(np.uint32)
    i = np.arange(d)
    if bits == 2:
        return (c[..., i >> 2] >> ((i & 3) * 2)) & 3
    grp = i >> 3
    w = c[..., grp * 3] | c[..., grp * 3 + 1] << 8 | c[..., grp * 3 + 2] << 16
    return (w >> ((i & 7) * 3)) & 7


def tq_centroids(orc, codes, bits: int, d: int) -> np.ndarray:
    """centroid[code] in the rotated space, float64 [..., d] (the oracle's codebook: the f32 values every kernel uses)."""
    cen, _ = orc.tq_codebook(d, bits)
    return cen.astype(np.float64)[tq_indices(codes, bits, d)]


def tq_values(orc, codes, bits: int, d: int, signs) -> np.ndarray:
    """R^-1(centroid[code]) [..., d]: the original-space row a TurboQuant code row stands for."""
    return tq_rotate_inverse(tq_centroids(orc, codes, bits, d), signs)


def qjl_signs(words, d: int) -> np.ndarray:
    """QJL rows [..., d / 32 + 1] uint32 -> +1 / -1 [..., d] (bit i of the row's sign words)."""
    w = np.asarray(words, np.uint32)[..., : d // 32]
    i = np.arange(d)
    return np.where((w[..., i >> 5] >> (i & 31)) & 1, 1.0, -1.0)


def qjl_norms(words, d: int) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(words, np.uint32)[..., d // 32]).view(np.float32).astype(np.float64)


def tq_decode(orc, q, k_codes, v_codes, bits: int, signs, scale: float, kv_len: int, k_qjl=None, S=None):
    """A TurboQuant decode step in float64.  q [n_heads, d]; codes [n_kv, rows, row bytes]; signs [n_kv, 2, d];
    k_qjl [n_kv, rows, d / 32 + 1] and S [n_kv, d, d] for the QJL types.  -> (out [n_heads, d], S_mag, vmax)."""
    q = np.asarray(q, np.float64)
    n_kv, d = k_codes.shape[0], q.shape[1]
    g = q.shape[0] // n_kv
    out = np.zeros_like(q)
    s_mag, vmax = 0.0, 0.0
    for kvh in range(n_kv):
        ck = tq_centroids(orc, k_codes[kvh, :kv_len], bits, d)              # [n, d], rotated space
        cv = tq_centroids(orc, v_codes[kvh, :kv_len], bits, d)
        vrows = tq_rotate_inverse(cv, signs[kvh, 1])
        vmax = max(vmax, float(np.abs(cv).sum(axis=1).max() / np.sqrt(d)))
        for gi in range(g):
            h = kvh * g + gi
            rq = tq_rotate(q[h], signs[kvh, 0])
            sc = ck @ rq
            rq_abs = np.abs(rq) + np.log2(d) * U * np.abs(q[h]).sum() / np.sqrt(d)   # what the kernel's f32 R q can hold
            mag = np.abs(ck) @ rq_abs
            if S is not None:
                Sk = np.asarray(S[kvh], np.float64)
                nrm = qjl_norms(k_qjl[kvh, :kv_len], d)
                coeff = QJL_COEFF / d
                sc = sc + coeff * nrm * (qjl_signs(k_qjl[kvh, :kv_len], d) @ (Sk @ rq))
                mag = mag + coeff * np.abs(nrm) * (np.abs(Sk) @ rq_abs).sum()
            s_mag = max(s_mag, float(scale * mag.max()))
            out[h] = decode_scores((sc * scale)[None], vrows[None])[0]
    return out, s_mag, vmax
