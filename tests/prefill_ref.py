"""A float64 restatement of the batched-prompt GEMM (csrc/prefill.hip), the arbiter of tests/test_gpu_prefill_ref.py.

The GEMM rounds both operands to f16 in front of the matrix cores and accumulates in f32.  f16 rounding is deterministic, so
the reference works in two tiers: the operands are emulated EXACTLY (tier 1), and the kernel is compared with the float64
product of those operands (tier 2) — an f32 bound, not an f16 one.  What the f16 rounding itself costs against the true
dequantized product (the path's contract) is a third, CPU-only statement.

Tier 1, operands.  Weights, generators and activations are those of tests/matvec_ref.py (a, o with w = a - o).
  X'  = f16(f32(h * nw)), round to nearest even twice (pf_resid_kernel / xh_store_chunk, which keeps the f32 product out of the
        conversion: folded into it, the product would be rounded once); f16(x) for pf_to_xh.  Stored at
        xh_offset(t, k): slab k / 256, token t owns 512 B, chunk q = (k / 8) % 32 at q ^ (t & 15), elements of a chunk in the
        order 0,2,1,3,4,6,5,7.
  w'  = f16(fma(u, S, O)), ONE rounding (pf_fin4: a packed-f16 fma): u S + O is formed exactly in float64 (at most 8 + 11 bits
        against 11 bits inside the f16 exponent range: < 53 bits) and rounded once.  u is the unsigned stored quant and
            Q4_K / Q5_K   S = f16(d * sc * 256)    O = f16(-dmin * mn * 256)      (u = q, 0..15 / 0..31)
            Q6_K          S = f16(d * sc * 256)    O = S * -32 in f16             (u = q', 0..63)
            Q8_0          S = f16(d * 256)         O = S * -128 in f16            (u = q + 128, 0..255)
            Q4_0          S = f16(d * 256)         O = S * -8 in f16              (u = q, 0..15)
        (pf_scale).  d * sc and dmin * mn are exact in f32 (11 x 8 bits), the factor 256 is a power of two, so for the K
        formats S and O round once each (d * sc * 256 has up to 17 bits); for Q8_0 / Q4_0 S = 256 d and O = S * const are exact
        (a power-of-two factor) unless they overflow.  The matrix-core operand is W' = w' / 256 (the kernel scales the f32
        accumulator by 1 / 256, exact).
  u and the per-element scale s (d * sc, or d) are read with matvec_ref.decode itself: u = a of the same bytes with every header
  field set to one, s = a of the same bytes with every quant set to one.

  Bound of tier 1 against the exact weight (test_prefill_ref.py checks it against the oracle's dequantization), u_h = 2^-11:
      Q8_0 / Q4_0   |W' - w| <= u_h |w|                       (the fma)
      Q6_K          |W' - w| <= 2 u_h |w|  (1 + u_h)          (S; O = -32 S follows S exactly; the fma)
      Q4_K / Q5_K   |W' - w| <= u_h (|a| + |o| + |w|)(1 + u_h) (S, O, the fma)
  plus, where S, O or w' is an f16 subnormal, 2^-25 / 256 per rounding (times u <= 255 for S).

Tier 2, the kernel against Y' = X' . W'^T in float64.  Products of two f16 are exact in f32 (22 bits).  One accumulator
(row, token) runs a chain of 8 MFMAs per 256-element block (v_mfma_f32_16x16x32_f16: 32 products each) over the `per` blocks of
its k-split.  The order of the 32 additions inside an MFMA is undocumented; ASSUMED here: any order, every addition rounded to
nearest in f32 — the worst case is one sequential chain, depth 32 per MFMA, 256 per block.  Then
    256 * per    the split's chain (pf_plan: per = ceil(nblk / S0), S0 = min(nblk, max(1, 256 / row groups)))
    S            the partial sums of the S splits added by the consumer (the scale 1 / 256 is exact)
    epilogue     pf_resid: the residual (1), bias (1); the kernels that apply 1/rms: EPI_NORM (Steps, below)
    C_pf(k, S, epi) = 256 * ceil(k / 256 / S) + S + epi
    |got - Y'| <= C_pf u M' + A,   u = 2^-24,  M' = sum_i |W'_i| |X'_i|
  A = 8 k 2^-126 (f32 flush-to-zero, as matvec_ref) + the f16 subnormal term: whether the packed f16 fma and the matrix cores
  keep or flush f16 subnormals has not been measured, so every product that touches one is allowed to vanish:
  sum_i |X'_i| (|w'_i| [w' subnormal] + |u_i S_i| [S subnormal] + |O_i| [O subnormal]) / 256 + sum_i |W'_i X'_i| [X'_i subnormal].
  C_pf is counted from the kernel, not fitted to its output.

The contract (CPU only): Y' against the true y = (a - o) . (h * nw).  With ex_i = (u_h + 2u) |v_i| + 2^-25 (the f32 product,
the f16 rounding, the subnormal floor) and ew_i the tier-1 bound above,
    |Y' - y| <= sum_i ew_i |v_i| + |w_i| ex_i + ew_i ex_i.
Steps (tests run the engine's own launch sequences through lgh_op_pf_qkv / _linear / _ffn):
  1/rms.  The producer of h leaves sums of squares per 2048 columns: per lane 8 squares and 7 additions (<= 11 roundings on any term),
  a wave tree (6), the four waves (2); pf_inv_rms adds <= 8 chunks (8), divides, adds eps, takes the square root and the reciprocal
  (4): 31 roundings, halved by the root and taken whole.  With the product by 1/rms (1) and the bias (1):  EPI_NORM = 33.
      y = Y' inv (+ bias),   |got - y| <= (C_pf(k, S, EPI_NORM) u M' + A) inv + 2u (|bias| + |y|)
  RoPE, SwiGLU and the residual go through matvec_ref's epilogue bounds; NeoX pairs (i, i + d/2) are the same rotation on
  re-ordered columns.
  Where a step rounds an f32 value it computed itself into f16 for the next GEMM (SwiGLU -> XH), the kernel's own f16 rows are
  returned by the entry point: they are checked against the reference within its bound plus one f16 rounding, and
  the next GEMM is judged on THEM — so every GEMM keeps its f32 bound.
  ssq of a row chunk: every term is positive and passes through at most 19 roundings: |got - sum v^2| <= 19 u sum v^2 + 4096 * 2^-126.

domain(): the inputs for which this holds — |w| < 256, |h * nw| < 65504 and no 256-times intermediate (S, O) overflowing f16.
"""
from __future__ import annotations

import numpy as np

import matvec_ref as mr

U = mr.U
UH = 2.0 ** -11
TINY = mr.TINY
SCALE = 256.0                      # kPfScale
TOKENS = 128                       # kPfTokens
NUM_CU = 256                       # kNumCU
F16_MAX = 65504.0
F16_TINY = 2.0 ** -14              # smallest normal f16
U_OFF = {"Q4_K": None, "Q5_K": None, "Q6_K": -32.0, "Q8_0": -128.0, "Q4_0": -8.0}
U_MAX = {"Q4_K": 15, "Q5_K": 31, "Q6_K": 63, "Q8_0": 255, "Q4_0": 15}


def f16(x) -> np.ndarray:
    """Round to nearest even into f16, straight from float64 (no double rounding); returned as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _sub(h) -> np.ndarray:
    """Nonzero f16 values below the smallest normal."""
    a = np.abs(h)
    return (a > 0) & (a < F16_TINY)


# ---- the plan
def pf_plan(n_rows, k: int):
    """pf_plan of prefill.hip: (row groups, splits S, blocks per split, blocks of the last split)."""
    nblk = k // 256
    rg = sum((n // 16 + 15) // 16 for n in n_rows)
    S = 1 if rg >= NUM_CU else NUM_CU // rg
    S = min(S, nblk)
    per = (nblk + S - 1) // S
    S = (nblk + per - 1) // per
    return rg, S, per, nblk - (S - 1) * per


def m_tile_width(m: int) -> int:
    """MT of pf_body chosen for m tokens (token tiles computed)."""
    mt = (m + 15) // 16
    return 2 if mt <= 2 else 4 if mt <= 4 else 8


def c_pf(k: int, S: int, epi: int = 0) -> float:
    per = -(-(k // 256) // S)
    return 256.0 * per + S + epi


# ---- XH
def xh_offset(t, k):
    """Element (f16) index of (token t, column k) in an XH matrix: xh_offset of prefill.h, in units of 2 bytes."""
    t, k = np.asarray(t, np.int64), np.asarray(k, np.int64)
    ch, j = k >> 3, k & 7
    pj = np.where((j == 1) | (j == 5), j + 1, np.where((j == 2) | (j == 6), j - 1, j))
    return (ch >> 5) * (TOKENS * 256) + t * 256 + (((ch & 31) ^ (t & 15)) << 3) + pj


def xh_pack(xq: np.ndarray, swap: bool = True, plain_token: int = -1) -> np.ndarray:
    """X' [m][k] -> the XH image (float64 per f16 slot, NaN where nothing was stored), as the producers write it.
    swap = False / plain_token = t plant a producer that does not swap elements 1 and 2 of a chunk / drops the swizzle of token t."""
    m, k = xq.shape
    buf = np.full((k // 256) * TOKENS * 256, np.nan)
    t, kk = np.arange(m)[:, None], np.arange(k)[None, :]
    off = xh_offset(t, kk)
    if not swap:
        ch, j = kk >> 3, kk & 7
        off = (ch >> 5) * (TOKENS * 256) + t * 256 + (((ch & 31) ^ (t & 15)) << 3) + j
    if plain_token >= 0:
        ch, j = kk >> 3, kk & 7
        pj = (xh_offset(0, kk) & 7)
        off = np.where(t == plain_token, (ch >> 5) * (TOKENS * 256) + t * 256 + ((ch & 31) << 3) + pj, off)
    buf[off] = xq
    return buf


def xh_read(buf: np.ndarray, m: int, k: int) -> np.ndarray:
    """The XH image as the GEMM reads it: [m][k]."""
    return buf[xh_offset(np.arange(m)[:, None], np.arange(k)[None, :])]


def x_operand(h, nw=None) -> np.ndarray:
    """X' = f16(f32(h * nw)) (f16(h) without a norm weight), as float64."""
    h = np.asarray(h, np.float32)
    v = h if nw is None else h * np.asarray(nw, np.float32)
    return f16(v.astype(np.float64))


# ---- weights
def fields(tname: str, raw: np.ndarray, k: int, n: int, need_ao: bool = True):
    """(u, s, a, o): the unsigned stored quant, the per-element scale (d * sc, or d), and matvec_ref's (a, o), each [n, k] float64.
    u and s come out of matvec_ref.decode itself: the bytes with every header field set to one / every quant set to one.
    need_ao = False leaves a and o out (None) where the operand does not need them (every format but Q4_K / Q5_K: wide matrices)."""
    raw = np.ascontiguousarray(raw, np.uint8)
    a, o = mr.decode(tname, raw, k, n) if need_ao or U_OFF[tname] is None else (None, None)
    be, bb = mr.BLOCK[tname]
    hb, qb = raw.reshape(n, k // be, bb).copy(), raw.reshape(n, k // be, bb).copy()
    one = (0x00, 0x3C)                                                 # f16 1.0, little endian
    if tname in ("Q4_0", "Q8_0"):
        hb[..., 0], hb[..., 1] = one
        qb[..., 2:] = 0x11 if tname == "Q4_0" else 0x01
    elif tname in ("Q4_K", "Q5_K"):
        hb[..., 0], hb[..., 1] = one
        hb[..., 4:8] = 1                                               # scales 1, mins 0 (get_scale_min_k4)
        hb[..., 8:12] = 0
        hb[..., 12:16] = 1
        if tname == "Q5_K":
            qb[..., 16:48] = 0
        qb[..., (16 if tname == "Q4_K" else 48):] = 0x11
    else:
        hb[..., 192:208] = 1
        hb[..., 208], hb[..., 209] = one
        qb[..., 0:128] = 0x11
        qb[..., 128:192] = 0
    u = mr.decode(tname, hb.reshape(-1), k, n)[0] + (128.0 if tname == "Q8_0" else 0.0)
    s = mr.decode(tname, qb.reshape(-1), k, n)[0]
    return u, s, a, o


def scale_offset(tname: str, s, o):
    """(S, O) of pf_scale as float64 values of f16 numbers (inf where they overflow)."""
    S = f16(np.asarray(s, np.float64) * SCALE)
    O = f16(-o * SCALE) if U_OFF[tname] is None else f16(S * U_OFF[tname])
    return S, O


def w_operand(tname: str, u, S, O) -> np.ndarray:
    """w' = f16(fma(u, S, O)): u S + O exactly, one rounding."""
    with np.errstate(invalid="ignore"):
        return f16(u * S + O)


def w_sub_term(u, S, O, wq) -> np.ndarray:
    """Per-element magnitude (already / 256) that vanishes if f16 subnormals are flushed anywhere in pf_fin4."""
    out = np.zeros_like(wq)
    for val, mag in ((wq, wq), (S, None), (O, O)):
        m = _sub(val)
        if m.any():
            out[m] += np.abs(u[m] * S[m] if mag is None else mag[m])
    return out / SCALE


def w_err(tname: str, a, o) -> np.ndarray:
    """Tier-1 bound |W' - w| per element (header)."""
    w = np.abs(a - o)
    if tname in ("Q8_0", "Q4_0"):
        e = UH * w
    elif tname == "Q6_K":
        e = 2 * UH * w * (1 + UH)
    else:
        e = UH * (np.abs(a) + np.abs(o) + w) * (1 + UH)
    return e + (U_MAX[tname] + 2) * 2.0 ** -25 / SCALE


def domain(a, o, v, S=None, O=None) -> bool:
    """True where the batched path's input limits hold: |w| < 256, |h * nw| < 65504, no 256-times intermediate overflowing f16."""
    ok = np.abs(np.asarray(a) - np.asarray(o)).max() < 256.0 and np.abs(np.asarray(v, np.float64)).max() < F16_MAX
    ok = ok and SCALE * np.abs(a).max() <= F16_MAX and SCALE * np.abs(o).max() <= F16_MAX
    for z in (S, O):
        if z is not None:
            ok = ok and bool(np.all(np.isfinite(z)))
    return bool(ok)


class Operand:
    """The emulated A operand of an [n, k] weight and everything the bounds need."""

    def __init__(self, tname: str, raw, k: int, n: int, need_ao: bool = True):
        self.tname, self.k, self.n = tname, k, n
        self.u, self.s, self.a, self.o = fields(tname, raw, k, n, need_ao)
        self.S, self.O = scale_offset(tname, self.s, self.o)
        self.wq = w_operand(tname, self.u, self.S, self.O)
        self.W = self.wq / SCALE
        self.sub = w_sub_term(self.u, self.S, self.O, self.wq)


# ---- the GEMM and its bound
def gemm(W, X, S: int = 1, skip_split: int = -1, drop_last_block: bool = False) -> np.ndarray:
    """Y' [m][n] = sum over the S k-splits of X'[:, split] . W'[:, split]^T in float64.
    skip_split / drop_last_block plant a consumer that leaves one split out / a producer that stops one block short in the last split."""
    k = W.shape[1]
    nblk = k // 256
    per = -(-nblk // S)
    y = np.zeros((X.shape[0], W.shape[0]))
    for s in range(S):
        b0, b1 = s * per, min(nblk, (s + 1) * per)
        if s == skip_split:
            continue
        if drop_last_block and s == S - 1:
            b1 -= 1
        y += X[:, 256 * b0:256 * b1] @ W[:, 256 * b0:256 * b1].T
    return y


def gemm_floor(W, wsub, X) -> np.ndarray:
    """[m][n] the absolute part A of the bound: f32 flush-to-zero and every product that touches an f16 subnormal."""
    aX = np.abs(X)
    return 8 * W.shape[1] * TINY + aX @ wsub.T + (aX * _sub(X)) @ np.abs(W).T


def gemm_bound(W, wsub, X, S: int, epi: int = 1) -> np.ndarray:
    """[m][n] bound of |kernel - Y'| (header, tier 2)."""
    return c_pf(W.shape[1], S, epi) * U * (np.abs(X) @ np.abs(W).T) + gemm_floor(W, wsub, X)


def gemm_ref(tname: str, raw, k: int, n: int, X, S: int, epi: int = 1, rows: int = 2048):
    """(Y', bound) over row slices of the weight (keeps the float64 copies of a wide matrix small)."""
    raw = np.ascontiguousarray(raw, np.uint8)
    rb = raw.size // n
    ys, es = [], []
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        op = Operand(tname, raw[r0 * rb:r1 * rb], k, r1 - r0, need_ao=False)
        assert domain(op.W, 0.0, X, op.S, op.O), "input outside the batched path's domain"   # (W' finite and < 256: so is w)
        ys.append(gemm(op.W, X, S))
        es.append(gemm_bound(op.W, op.sub, X, S, epi))
    return np.concatenate(ys, axis=1), np.concatenate(es, axis=1)


def contract_bound(tname: str, a, o, v) -> np.ndarray:
    """[m][n] bound of |Y' - (a - o) . v| (header, the contract)."""
    av = np.abs(np.asarray(v, np.float64))
    ew = w_err(tname, a, o)
    ex = (UH + 2 * U) * av + 2.0 ** -25
    return av @ ew.T + ex @ np.abs(a - o).T + ex @ ew.T


def act_block(k: int, m: int, seed: int) -> np.ndarray:
    """m token rows [m][k] f32, row t of activation kind ACT_KINDS[t % 6]: every kind is present from m = 6 on."""
    return np.stack([mr.activation(mr.ACT_KINDS[t % len(mr.ACT_KINDS)], k, seed + t) for t in range(m)])


# ---- the layer steps
EPI_NORM = 33
EPI_RESID = 2
SSQ_COLS = 2048


def inv_rms_rows(h, eps: float) -> np.ndarray:
    h = np.asarray(h, np.float64)
    return 1.0 / np.sqrt(np.mean(h * h, axis=1) + eps)


def normed(ops, Xq, inv, S: int, biases=None):
    """(y, err) [m][sum n]: the GEMM over the operands `ops` side by side (one launch: the same S), times 1/rms, plus bias."""
    ys, es = [], []
    for i, op in enumerate(ops):
        y = gemm(op.W, Xq, S) * inv[:, None]
        e = gemm_bound(op.W, op.sub, Xq, S, EPI_NORM) * inv[:, None]
        if biases is not None and biases[i] is not None:
            b = np.asarray(biases[i], np.float64)[None, :]
            y = y + b
            e = e + 2 * U * (np.abs(b) + np.abs(y))
        ys.append(y)
        es.append(e)
    return ys, es


def rope_rows(y, err, cs, head_dim: int, neox: bool):
    """RoPE of every token row of y [m][heads * head_dim] with cs[t] = (cos, sin) of the token's position."""
    m, n = y.shape
    half = head_dim // 2
    out, eo = np.empty_like(y), np.empty_like(err)
    # NeoX: pair i of a head is (i, i + half): bring the pairs side by side, rotate, and put them back
    perm = np.arange(n)
    if neox:
        j = np.arange(head_dim)
        perm = (np.arange(n // head_dim)[:, None] * head_dim + np.where(j % 2 == 0, j // 2, j // 2 + half)[None, :]).reshape(-1)
    for t in range(m):
        r, e = mr.rope(y[t, perm], err[t, perm], cs[t][0], cs[t][1], head_dim)
        out[t, perm], eo[t, perm] = r, e
    return out, eo


def qkv_step(ops, h, nw, eps, biases, cs, head_dim: int, n_kv: int, neox: bool):
    """(q, k, v) each (value, bound): q [m][QD]; k, v [m][n_kv][head_dim] = the cache rows pos0 + t of every kv head."""
    Xq = x_operand(h, nw)
    _, S, _, _ = pf_plan([op.n for op in ops], ops[0].k)
    (q, k, v), (eq, ek, ev) = normed(ops, Xq, inv_rms_rows(h, eps), S, biases)
    q, eq = rope_rows(q, eq, cs, head_dim, neox)
    k, ek = rope_rows(k, ek, cs, head_dim, neox)
    m = q.shape[0]
    sh = (m, n_kv, head_dim)
    return (q, eq), (k.reshape(sh), ek.reshape(sh)), (v.reshape(sh), ev.reshape(sh))


def resid_step(op, Xq, resid, bias=None):
    """(hidden, bound) = resid + X' . W'^T (+ bias): pf_resid_kernel."""
    _, S, _, _ = pf_plan([op.n], op.k)
    y = gemm(op.W, Xq, S)
    r = np.asarray(resid, np.float64)
    mag = np.abs(Xq) @ np.abs(op.W).T + np.abs(r)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[None, :]
        mag = mag + np.abs(np.asarray(bias, np.float64))[None, :]
    return y + r, c_pf(op.k, S, EPI_RESID) * U * mag + gemm_floor(op.W, op.sub, Xq)


def ssq_ref(hidden):
    """(sums of squares [m][chunks], bound) of the f32 rows the kernel returned."""
    h = np.asarray(hidden, np.float64)
    m, H = h.shape
    n = -(-H // SSQ_COLS)
    s = np.stack([(h[:, c * SSQ_COLS:(c + 1) * SSQ_COLS] ** 2).sum(axis=1) for c in range(n)], axis=1)
    return s, 19 * U * s + 2 * SSQ_COLS * TINY


def swiglu_step(og, ou, h, nw, eps, inv=None):
    """(act, bound) [m][F] in float64, before the f16 rounding of the XH store.  inv: 1/rms per row instead of the rows' own (planted
    mistakes)."""
    Xq = x_operand(h, nw)
    _, S, _, _ = pf_plan([og.n, ou.n], og.k)
    (g, u), (eg, eu) = normed([og, ou], Xq, inv_rms_rows(h, eps) if inv is None else inv, S)
    with np.errstate(over="ignore"):                # (exp(-g) of a very negative gate: silu is 0 there)
        return mr.swiglu(g, eg, u, eu)


def f16_store_bound(ref, err):
    """Bound of |f16(kernel's f32 value) - ref| given |kernel - ref| <= err: one more f16 rounding (2^-25 in the subnormals)."""
    return err + UH * (np.abs(ref) + err) + 2.0 ** -24


# ---- the MoE step
MOE_ROWS = 384                     # kPfMoeRows
# what lgh_op_pf_moe fills the index tables with before the first launch (rowmap: 0, so that every -1 of a padding row is the kernel's)
LIST_FILL, TOKMAP_FILL = 0x7F7F, MOE_ROWS - 1


def moe_eligible(n_experts: int, top_k: int) -> bool:
    """pf_eligible's routing condition: the rows of a full block, padded to 16 per expert, fit the shared row space."""
    return 0 < top_k <= 8 and n_experts <= 64 and TOKENS * top_k + 15 * n_experts <= MOE_ROWS


def moe_group(sel: np.ndarray, n_experts: int):
    """pf_moe_group_kernel restated: (counts, bases, lists [E][128], rowmap [384], tokmap [m][top_k]) of a selection [m][top_k].
    lists[e][i] = token | slot << 8 in token order, bases padded to 16 rows, rowmap[r] = e | i << 8 (-1 on padding), tokmap = the row."""
    m, top_k = sel.shape
    flat = sel.reshape(-1)
    counts, bases = np.zeros(n_experts, np.int32), np.zeros(n_experts, np.int32)
    lists = np.full((n_experts, TOKENS), LIST_FILL, np.int32)
    rowmap, tokmap = np.full(MOE_ROWS, -1, np.int32), np.full(m * top_k, TOKMAP_FILL, np.int32)
    b = 0
    for e in range(n_experts):
        idx = np.nonzero(flat == e)[0]
        c = len(idx)
        assert c <= TOKENS
        counts[e], bases[e] = c, b
        lists[e, :c] = (idx // top_k) | ((idx % top_k) << 8)
        rowmap[b:b + c] = e | (np.arange(c) << 8)
        tokmap[idx] = b + np.arange(c)
        b += (c + 15) & ~15
    assert b <= MOE_ROWS
    return counts, bases, lists, rowmap, tokmap.reshape(m, top_k)


def route(h, nw, eps, wr, top_k: int):
    """matvec_ref.router per token: (sel [m][k], weights [m][k], marginal [m], weight bound [m]).  A token is marginal where two
    logits whose order decides the selection or its order lie within the sum of their f32 bounds."""
    sels, ws, marg, werr = [], [], [], []
    for t in range(h.shape[0]):
        sel, w, logits, lerr = mr.router(h[t], nw, eps, wr, top_k)
        order = sorted(range(len(logits)), key=lambda e: (-logits[e], e))
        pairs = zip(order[:top_k], order[1:top_k + 1])
        marg.append(any(logits[a] - logits[b] <= lerr[a] + lerr[b] for a, b in pairs))
        sels.append(sel)
        ws.append(w)
        werr.append(8 * U + 2 * float(np.max(lerr)))
    return np.array(sels, np.int32), np.array(ws), np.array(marg), np.array(werr)


def route_weights(h, nw, eps, wr, sel):
    """Softmax over the float64 logits of a GIVEN selection (a marginal token's, as the kernel chose)."""
    out = np.empty(sel.shape)
    for t in range(sel.shape[0]):
        logits = mr.router(h[t], nw, eps, wr, sel.shape[1])[2][sel[t]]
        p = np.exp(logits - logits.max())
        out[t] = p / p.sum()
    return out


def moe_step(gate, up, down, h, nw, eps, sel, w, act_got=None, inv_of=None):
    """(hidden, bound, acts): h + sum_s w[t][s] * down_e(silu(gate_e x') * (up_e x')) in selection order, e = sel[t][s]; gate / up / down
    are lists of Operands per expert; acts[e] = (act, bound) of the expert's rows in token order.  act_got [E][128][EI]: the f16 rows
    the kernel's down GEMMs read (None: f16 of the reference).  inv_of(tokens, rows) -> 1/rms per row plants a wrong one."""
    Xq, inv = x_operand(h, nw), inv_rms_rows(h, eps)
    (m, top_k), H = sel.shape, h.shape[1]
    ys, es, acts = np.zeros((m, top_k, H)), np.zeros((m, top_k, H)), {}
    flat = sel.reshape(-1)
    for e in sorted(set(flat.tolist())):
        idx = np.nonzero(flat == e)[0]
        T, sl = idx // top_k, idx % top_k
        _, S, _, _ = pf_plan([gate[e].n, up[e].n], H)
        iv = inv[T] if inv_of is None else inv_of(T, np.arange(len(T)))
        (g, u), (eg, eu) = normed([gate[e], up[e]], Xq[T], iv, S)
        with np.errstate(over="ignore"):
            acts[e] = mr.swiglu(g, eg, u, eu)
        a16 = f16(acts[e][0]) if act_got is None else np.asarray(act_got[e][:len(T)], np.float64)
        _, Sd, _, _ = pf_plan([down[e].n], down[e].k)
        ys[T, sl] = gemm(down[e].W, a16, Sd)
        es[T, sl] = gemm_bound(down[e].W, down[e].sub, a16, Sd, 0)
    w = np.asarray(w, np.float64)
    r = np.asarray(h, np.float64)
    acc = (w[:, :, None] * ys).sum(axis=1)
    mag = np.abs(w[:, :, None] * ys).sum(axis=1) + np.abs(r)
    err = (np.abs(w)[:, :, None] * es).sum(axis=1) + (2 * top_k + 2) * U * mag + 8 * TINY
    return acc + r, err, acts
