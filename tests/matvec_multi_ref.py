"""What the multi-sequence step adds to tests/matvec_ref.py, in float64: the arbiter of tests/test_gpu_matvec_multi.py.

A sequence's result is the single-sequence launch's on that sequence's vector, so the arithmetic and the bound are matvec_ref's, per
sequence; no tolerance is introduced here.  New:
  * grouping: the step's (sequence, top-k slot) pairs v = s * top_k + slot listed per expert, sequences ascending, with counts;
  * per-sequence RoPE positions and cache slots: sequence s rotates at pos[s] and owns row pos[s] of cache slot slot[s], nothing else;
  * the combine: sum_p w_p * down_p in selection order from zero, plus the residual (matvec_ref.moe_down and its bound).
The checks the GPU tests apply are functions here (`ratio`, `cache_failures`), and so are the tests' inputs (`activations`,
`positions`, `slots`, `selections`): tests/test_matvec_multi_ref.py feeds the same checks, on the same inputs, results that are wrong
in the ways a multi-sequence kernel goes wrong and shows that each one is caught."""
from __future__ import annotations

import numpy as np

import matvec_ref as mr

NAN_BITS = np.uint32(0x7FC0BEEF)
# sequence s of a test gets kind s % 6: "zeros" and "outlier" are among any three
SEQ_KINDS = ("normal", "outlier", "zeros", "scales", "pow2", "tiny")


def activations(k: int, n_seq: int, seed: int) -> np.ndarray:
    """[n_seq, k] f32: every sequence a different kind of activation vector."""
    return np.stack([mr.activation(SEQ_KINDS[s % len(SEQ_KINDS)], k, seed + 31 * s) for s in range(n_seq)])


def positions(n_seq: int, max_seq: int) -> np.ndarray:
    """Ragged positions far apart: 0, 1 and max_seq - 1 among them, the rest spread over the cache."""
    base = [max_seq - 1, 0, 1]
    rest = [int(2 + (i * 7919) % (max_seq - 3)) for i in range(max(0, n_seq - 3))]
    return np.array((base + rest)[:n_seq], np.int32)


def slots(n_seq: int, n_slots: int, seed: int) -> np.ndarray:
    """A non-identity placement of the sequences into n_slots >= n_seq cache slots in which NO sequence sits in slot s."""
    rng = np.random.default_rng(seed)
    while True:
        p = rng.permutation(n_slots)[:n_seq].astype(np.int32)
        if not np.any(p == np.arange(n_seq)):
            return p


def selections(kind: str, n_seq: int, n_experts: int, top_k: int, seed: int):
    """(sel [n_seq, top_k] int32, w [n_seq, top_k] f32): 'random'; 'same' (every sequence on the same experts: the others count 0);
    'single' (as 'same', but one pair — the last sequence's last slot — alone on another expert)."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        sel = np.stack([rng.permutation(n_experts)[:top_k] for _ in range(n_seq)])
    else:
        sel = np.tile(rng.permutation(n_experts - 1)[:top_k] + 1, (n_seq, 1))     # (expert 0 stays free)
        if kind == "single":
            sel[-1, -1] = 0
    # weights of a sequence far from equal, so that swapping them shows: a geometric ladder, normalised
    w = np.stack([rng.permutation(0.5 ** np.arange(top_k)) for _ in range(n_seq)])
    return sel.astype(np.int32), (w / w.sum(axis=1, keepdims=True)).astype(np.float32)


# ---- grouping
def group(sel, n_experts: int):
    """(cnt [n_experts], lists): lists[e] = the pairs v = s * top_k + slot with sel[s, slot] == e, ascending."""
    sel = np.asarray(sel)
    flat = sel.reshape(-1)
    lists = [[int(v) for v in np.nonzero(flat == e)[0]] for e in range(n_experts)]
    return np.array([len(l) for l in lists], np.int32), lists


def group_failures(cnt, idx, sel, n_experts: int, idx_sentinel: int, cnt_sentinel: int = 0x55):
    """The device tables against the restatement, exactly: counts, the lists' entries, and the sentinels everywhere else."""
    want_cnt, lists = group(sel, n_experts)
    cnt, idx = np.asarray(cnt), np.asarray(idx)
    fails = []
    if not np.array_equal(cnt[:n_experts], want_cnt):
        fails.append("cnt %s, want %s" % (list(cnt[:n_experts]), list(want_cnt)))
    if not np.all(cnt[n_experts:] == cnt_sentinel):
        fails.append("cnt written past the experts")
    for e in range(idx.shape[0]):
        want = lists[e] if e < n_experts else []
        if list(idx[e, :len(want)]) != want:
            fails.append("idx[%d] %s, want %s" % (e, list(idx[e, :len(want)]), want))
        if not np.all(idx[e, len(want):] == idx_sentinel):
            fails.append("idx[%d] written past its count" % e)
    return fails


# ---- checks
def ratio(got, ref, err) -> float:
    """max |got - ref| / err (inf where got is not finite): the GPU tests require <= 1."""
    got = np.asarray(got, np.float64)
    r = np.abs(got - ref) / err
    r[~np.isfinite(got)] = np.inf
    return float(r.max()) if r.size else 0.0


def poisoned(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) == NAN_BITS


def cache_failures(cache, pos, slot, ref_rows, err_rows, what: str):
    """cache [n_slots, n_kv, max_seq, head_dim] after the launch on a poisoned cache: row pos[s] of slot slot[s] holds sequence s's row
    (ref_rows / err_rows [n_seq, n_kv * head_dim]) within the bound, every other row the pattern."""
    fails = []
    touched = np.zeros(cache.shape[:1] + cache.shape[2:3], bool)
    for s in range(len(pos)):
        touched[slot[s], pos[s]] = True
        r = ratio(cache[slot[s], :, pos[s], :].reshape(-1), ref_rows[s], err_rows[s])
        if not r <= 1.0:
            fails.append("%s: sequence %d (slot %d, row %d) ratio %.3g" % (what, s, slot[s], pos[s], r))
    rest = poisoned(cache).all(axis=3).all(axis=1)           # [n_slots, max_seq]: the whole row still holds the pattern
    if not np.all(rest[~touched]):
        bad = np.argwhere(~rest & ~touched)
        fails.append("%s: rows other than (slot[s], pos[s]) changed: (slot, row) %s" % (what, [tuple(int(v) for v in b) for b in bad[:4]]))
    return fails


# ---- XQ images (csrc/xq.h): a 1280-byte record per 256 elements
def xq_decode(img, n: int):
    """(x [n], xs [n / 16]) float64 of an image's first n elements (n a multiple of 16): x = sx * I with I the four balanced base-256
    digits of the element (byte ((g * 4 + i) * 32 + e) = digit 3 - i of element 32 g + e), and the stored chunk sums; chunk j's scale
    and sum sit at slot (j & 3) * 4 + (j >> 2) of the record's two f32 tables."""
    rec = np.ascontiguousarray(img, dtype=np.uint8).reshape(-1, 1280)[:(n + 255) // 256]
    d = rec[:, :1024].view(np.int8).astype(np.int64).reshape(-1, 8, 4, 32)          # [record, g, i, e]
    I = (d[:, :, 0] << 24) + (d[:, :, 1] << 16) + (d[:, :, 2] << 8) + d[:, :, 3]        # [record, g, e]
    slot = np.array([(j & 3) * 4 + (j >> 2) for j in range(16)])
    xs = np.ascontiguousarray(rec[:, 1024:1088]).view(np.float32).astype(np.float64)[:, slot]
    sx = np.ascontiguousarray(rec[:, 1088:1152]).view(np.float32).astype(np.float64)[:, slot]
    x = I.reshape(-1, 16, 16) * sx[:, :, None]
    return x.reshape(-1)[:n], xs.reshape(-1)[:n // 16]


def image_ref(out, nw=None):
    """What the image of a launch's f32 output `out` must hold, with bounds: elements v = out * nw within one f32 product rounding plus
    half a step of the chunk's scale (sx / 2 <= 2^-30 max|v|, or 2^-127 under the exponent clamp); chunk sums of v and of out^2 within
    the roundings of a 16-element tree (4 levels) and of the terms: 6 u sum|terms| (+ flushed subnormals).  The element bound IS the
    format's half step when a chunk's maximum sits just above a power of two (s = 2 max|v|), so over thousands of elements the worst
    ratio comes close to 1 (0.99 observed) without anything being wrong; it cannot pass 1 for a correct image.
    -> ((v, err_v), (sums, err_sums), (ssq, err_ssq))"""
    o = np.asarray(out, np.float64)
    v = o if nw is None else o * np.asarray(nw, np.float64)
    m = mr.chunk_max(v)
    ev = mr.U * np.abs(v) + 2.0 ** -30 * m * (1 + 2 * mr.U) + mr.TINY
    ch, sq = v.reshape(-1, 16), (o * o).reshape(-1, 16)
    return ((v, ev), (ch.sum(axis=1), 6 * mr.U * np.abs(ch).sum(axis=1) + 16 * mr.TINY),
            (sq.sum(axis=1), 6 * mr.U * sq.sum(axis=1) + 16 * mr.TINY))


# ---- the launches, per sequence
def sample_rows(n: int, count: int = 192, seed: int = 0) -> np.ndarray:
    """All rows of a narrow matrix; of a wide one its first and last two tiles and a random sample."""
    if n <= count:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    edge = np.concatenate([np.arange(32), np.arange(n - 32 - n % 16, n)])
    return np.unique(np.concatenate([edge, rng.choice(n, count - edge.size, replace=False)]))


def take_rows(raw, n: int, rows) -> np.ndarray:
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    return np.ascontiguousarray(raw.reshape(n, raw.size // n)[rows]).reshape(-1)


def linear(tname: str, raw, k: int, n: int, X, nw=None, bias=None, rows=None, eps: float = 1e-5, xerr=None):
    """(Y, E) [n_seq, rows]: matvec_ref.matvec of every sequence's vector (matrix-core family), on the sampled rows."""
    rows = np.arange(n) if rows is None else np.asarray(rows)
    a, o = mr.decode(tname, take_rows(raw, n, rows), k, rows.size)
    out = [mr.matvec(a, o, X[s], nw=nw, eps=eps, bias=None if bias is None else np.asarray(bias)[rows], family="mfma",
                     xerr=None if xerr is None else xerr[s]) for s in range(len(X))]
    return np.stack([y for y, _ in out]), np.stack([e for _, e in out])


def linear_blocks(tname: str, raw, k: int, n: int, x, keep_blocks, nw=None, rows=None, eps: float = 1e-5) -> np.ndarray:
    """One sequence's result when only the 256-element blocks in keep_blocks reach the sum (the norm's 1/rms is the full vector's): what
    a kernel computes that drops staged records or restarts its running sum."""
    rows = np.arange(n) if rows is None else np.asarray(rows)
    a, o = mr.decode(tname, take_rows(raw, n, rows), k, rows.size)
    x64 = np.asarray(x, np.float64)
    v = x64 if nw is None else x64 * np.asarray(nw, np.float64)
    keep = np.zeros(k // 256, bool)
    keep[list(keep_blocks)] = True
    v = v * np.repeat(keep, 256)
    return ((a - o) @ v) * (1.0 if nw is None else mr.inv_rms(x64, eps))


def k_slices(k: int):
    """(T, nbw): the k-slices of the single-sequence plan (matvec_ref.mvq_geometry)."""
    g = mr.mvq_geometry(k, 16)
    return g["T"], g["nbw"]


def rope_rows(orc, Y, E, pos, head_dim: int, base: float, scale: float):
    """RoPE of every sequence's row at its own position."""
    ys, es = [], []
    for s in range(len(pos)):
        c, sn = mr.rope_cs(orc, int(pos[s]), head_dim, base, scale)
        y, e = mr.rope(Y[s], E[s], c, sn, head_dim)
        ys.append(y)
        es.append(e)
    return np.stack(ys), np.stack(es)


class Experts:
    """The float64 parts of an expert stack, decoded on first use."""

    def __init__(self, tg, gate, up, td, down, E, H, F):
        self.t, self.raw, self.E, self.H, self.F = (tg, tg, td), (gate, up, down), E, H, F
        self.cache = {}

    def part(self, which: int, e: int, rows=None):
        key = (which, e, None if rows is None else tuple(rows))
        if key not in self.cache:
            k, n = (self.F, self.H) if which == 2 else (self.H, self.F)
            raw = np.ascontiguousarray(self.raw[which], dtype=np.uint8)
            one = raw.reshape(self.E, raw.size // self.E)[e]
            r = np.arange(n) if rows is None else np.asarray(rows)
            self.cache[key] = mr.decode(self.t[which], take_rows(one, n, r), k, r.size)
        return self.cache[key]


def moe(ex: Experts, x, x_in, nw, sel, w, eps: float = 1e-5, rows=None):
    """One sequence's MoE half: resid x + sum_p w_p down_e(silu(gate_e x') up_e x') in selection order, the experts reading x_in[p]
    (the sequence's own vector x for every pair, in a correct step)."""
    ys, es = [], []
    for p, e in enumerate(sel):
        g, eg = mr.matvec(*ex.part(0, int(e)), x_in[p], nw=nw, eps=eps, family="mfma")
        u, eu = mr.matvec(*ex.part(1, int(e)), x_in[p], nw=nw, eps=eps, family="mfma")
        act, eact = mr.swiglu(g, eg, u, eu)
        y, ey = mr.matvec(*ex.part(2, int(e), rows), act, family="mfma", xerr=eact)
        ys.append(y)
        es.append(ey)
    r = np.asarray(x, np.float64)
    return mr.moe_down(ys, es, w, r if rows is None else r[np.asarray(rows)])
