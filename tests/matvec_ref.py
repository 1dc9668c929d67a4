"""A float64 restatement of the engine's quantized mat-vec launches, the arbiter of tests/test_gpu_matvec.py.

Weights.  The decoders below read native GGUF blocks and return, for every weight, the two parts the kernels form separately:
the scale part `a` and the offset part `o`, with  w = a - o  exactly (f16 times small integers is exact in float64):
    Q4_0  a = d * q            o = 8 * d                 (q 0..15)
    Q8_0  a = d * q            o = 0                     (q -128..127)
    Q4_K  a = d * sc * q       o = dmin * mn             (q 0..15, sc / mn 6-bit)
    Q5_K  a = d * sc * q       o = dmin * mn             (q 0..31)
    Q6_K  a = d * sc * q'      o = 32 * d * sc           (q' 0..63, sc int8)
The VALU kernel forms Q8_0 as d (q + 128) - 128 d: there a = d (q + 128), o = 128 d (decode(..., family="valu")).
Types expanded to f32 at upload (Q4_1, Q5_0, Q5_1, Q2_K, Q3_K, F16, F32) are read as the oracle's f32 dequantization (a = w, o = 0).

Operation.  y = W . (x * nw) * inv + bias,  inv = 1 / sqrt(mean(x^2) + eps) (1 without a norm), then the epilogue: residual;
silu(g) * u; RoPE on pairs (2i, 2i+1) with the engine's f32 cos / sin; the K / V cache row at `pos`; the MoE sum
sum_p w_p y_p in selection order, plus the residual.  Everything here is float64.

Error bound.  Let v = x * nw and, for element i, m(i) = max |v| over i's 16-element XQ chunk (int8 matrix-core kernel) or |v_i|
(VALU and f32 kernels).  Every partial sum any kernel forms is a sum of terms a_i v_i and o_i v_i (the offsets go through the
chunk sums of x), so every intermediate is bounded by  M = sum_i (|a_i| + |o_i|) m(i).  A sum evaluated along a chain of depth D
in f32 is off by at most  gamma_D * (sum of |terms|) ~ D * u * M  (u = 2^-24), whatever the order; so

    |got - ref| <= C * u * (M * inv + |bias|) + A

with D counted per kernel:
  * int8 MFMA (matvec_mfma.hip, mvq_core.h).  XQ stores v_i as sx * I with |v_i - sx I| <= 2^-31 * 2 m(i) (one rounding,
    absorbed by 1 in D) and the f32 product x * nw (1).  Per 16-element chunk: V = exact int32 sums recombined (1 rounding),
    the scale / offset fmas (2), the chunk sum of x for the offset (a 4-level DPP tree: 4); per block the four steps (4) and the
    block's d / dmin products (2); along k the lane's accumulator over its blocks (at most k / 256 when one wave holds all of
    k); then the 4-lane-group shuffle (2), the k-slice partial sums (<= 8), inv (1), bias (1).  The norm: inv = 1/sqrt(ss/k+eps)
    from chunk partials (4) summed by lanes (k / 1024 per lane at most), a wave tree (6), the division, sqrt and reciprocal
    (3); inv's relative error is half that of ss plus 2: <= (k / 2048 + 16) u, times |y| <= M inv.
        C_mfma(k) = k / 256 + k / 2048 + 48
  * VALU mv_kernel (matvec.hip): a lane's unit (32 elements, 64 for Q6_K) as one chain (64), the wave tree (6), the k-slices
    (<= 16), inv, bias, product x * nw (4); the norm's sum of squares is a per-thread chain of k / 64 at most plus trees (24).
        C_valu(k) = k / 128 + 96
  * f32 fallback (f32_matvec_kernel): per lane k / 64 fmas, a wave tree (6); x * inv * nw (2); the block's sum of squares
    (k / 256 per thread, trees 16).
        C_f32(k) = k / 64 + k / 512 + 48
  * The oracle (CPU, orc.vec_mat_q / orc.dot_q) sums sequentially in f32 along k: D = k (+ its block structure, 32).
        C_orc(k) = k + 32
  A = 8 k 2^-126 covers flush-to-zero of f32 subnormal intermediates (at most one per operation, 8 operations per weight).
  XQ clamps the exponent of chunks whose maximum is below 2^-97: their elements are off by sx / 2 absolute, sx = 2^-126; that
  adds 2^-127 sum_i |a_i| over such chunks (folded into A by |a_i| <= 1 for the test matrices: bound() adds it exactly).

Epilogues (err_y = the bound of the pre-epilogue value y):
  residual:  err_y + 2u (|y| + |r|)
  SwiGLU:    |silu'(g)| err_g + |silu(g)| err_u + 8u |silu(g) u|, |silu'| <= 1.1 (expf: a few ulp, the division, the product)
  RoPE:      |c| err_0 + |s| err_1 + 4u (|x0 c| + |x1 s|), c / s the engine's f32 values (exact here)
  MoE down:  sum_p |w_p| err_p + (P + 2) u (sum_p |w_p y_p| + |r|), the weights w_p as the kernel read them
Router: float64 logits; a stable descending top-k (ties keep the lower index); softmax over the k logits.  Its f32 logits are off
by at most C_f32(hidden) u sum_i |x'_i w_i| (the same chain as the f32 mat-vec), the weights by 8u + 2 max logit error.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
TYPE = {"F32": 0, "F16": 1, "Q4_0": 2, "Q4_1": 3, "Q5_0": 6, "Q5_1": 7, "Q8_0": 8, "Q2_K": 10, "Q3_K": 11, "Q4_K": 12, "Q5_K": 13,
        "Q6_K": 14}
FUSED = ("Q4_0", "Q8_0", "Q4_K", "Q5_K", "Q6_K")
EXPANDED = ("Q4_1", "Q5_0", "Q5_1", "Q2_K", "Q3_K", "F16", "F32")
BLOCK = {"Q4_0": (32, 18), "Q8_0": (32, 34), "Q4_K": (256, 144), "Q5_K": (256, 176), "Q6_K": (256, 210)}
TINY = 2.0 ** -126


def c_mfma(k: int) -> float:
    return k / 256 + k / 2048 + 48


def c_valu(k: int) -> float:
    return k / 128 + 96


def c_f32(k: int) -> float:
    return k / 64 + k / 512 + 48


def c_orc(k: int) -> float:
    return k + 32


def kernel_family(tname: str, k: int) -> str:
    """Which kernel the engine runs a [.., k] weight of this type on."""
    if tname in FUSED:
        return "mfma" if k % 256 == 0 else "valu"
    return "f32"


def c_for(family: str, k: int) -> float:
    return {"mfma": c_mfma, "valu": c_valu, "f32": c_f32, "orc": c_orc}[family](k)


# ---- decoders: native GGUF bytes -> (a, o) float64 [n, k]
def _f16(b: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(b).view(np.float16).astype(np.float64)


def _k4_scales(sc: np.ndarray):
    """get_scale_min_k4 over the 12 scale bytes [.., 12] -> (scale, min) [.., 8] of the 8 sub-blocks."""
    s = sc.astype(np.int64)
    scale, mn = np.empty(s.shape[:-1] + (8,), np.int64), np.empty(s.shape[:-1] + (8,), np.int64)
    for j in range(4):
        scale[..., j] = s[..., j] & 63
        mn[..., j] = s[..., j + 4] & 63
    for j in range(4, 8):
        scale[..., j] = (s[..., j + 4] & 0xF) | ((s[..., j - 4] >> 6) << 4)
        mn[..., j] = (s[..., j + 4] >> 4) | ((s[..., j] >> 6) << 4)
    return scale, mn


def decode(tname: str, raw: np.ndarray, k: int, n: int, orc=None, family: str = "mfma"):
    """(a, o) float64 [n, k] with w = a - o, the exact values the kernels read.  The VALU kernel multiplies Q8_0 quants as
    q + 128 (0..255) and subtracts 128 d sum(x): there a = d (q + 128), o = 128 d."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if tname == "Q8_0" and family == "valu":
        a, _ = decode(tname, raw, k, n)
        d = np.repeat(_f16(raw.reshape(n, k // 32, 34)[..., 0:2].copy())[..., 0], 32, axis=-1)
        return a + 128.0 * d, 128.0 * d
    if tname not in BLOCK:
        w = orc.dequantize(TYPE[tname], raw, k * n).reshape(n, k).astype(np.float64)
        return w, np.zeros_like(w)
    be, bb = BLOCK[tname]
    b = raw.reshape(n, k // be, bb)
    if tname in ("Q4_0", "Q8_0"):
        d = _f16(b[..., 0:2].copy())[..., 0]
        if tname == "Q4_0":
            qs = b[..., 2:18].astype(np.int64)
            q = np.concatenate([qs & 15, qs >> 4], axis=-1)
            a, o = d[..., None] * q, np.broadcast_to(8.0 * d[..., None], q.shape)
        else:
            q = b[..., 2:34].view(np.int8).astype(np.int64)
            a, o = d[..., None] * q, np.zeros(q.shape)
        return a.reshape(n, k), np.ascontiguousarray(o).reshape(n, k)
    if tname in ("Q4_K", "Q5_K"):
        d, dmin = _f16(b[..., 0:2].copy())[..., 0], _f16(b[..., 2:4].copy())[..., 0]
        sc, mn = _k4_scales(b[..., 4:16])
        qoff = 16 if tname == "Q4_K" else 48
        qs = b[..., qoff:qoff + 128].astype(np.int64).reshape(n, k // 256, 4, 32)
        q = np.stack([qs & 15, qs >> 4], axis=3).reshape(n, k // 256, 8, 32)     # sub-block 2j: low nibbles of qs[32j..], 2j+1: high
        if tname == "Q5_K":
            qh = b[..., 16:48].astype(np.int64)                                   # bit `sub-block` of qh[l]
            for sb in range(8):
                q[:, :, sb, :] |= ((qh >> sb) & 1) << 4
        a = (d[..., None, None] * sc[..., None]) * q
        o = np.broadcast_to((dmin[..., None] * mn)[..., None], q.shape)
        return a.reshape(n, k), np.ascontiguousarray(o).reshape(n, k)
    # Q6_K: ql[128], qh[64], scales int8[16], d
    ql, qh = b[..., 0:128].astype(np.int64), b[..., 128:192].astype(np.int64)
    sc = b[..., 192:208].view(np.int8).astype(np.int64)
    d = _f16(b[..., 208:210].copy())[..., 0]
    q = np.empty((n, k // 256, 256), np.int64)
    for hn in range(2):
        L, H = ql[..., 64 * hn:64 * hn + 64], qh[..., 32 * hn:32 * hn + 32]
        base = 128 * hn
        q[..., base:base + 32] = (L[..., 0:32] & 15) | ((H & 3) << 4)
        q[..., base + 32:base + 64] = (L[..., 32:64] & 15) | (((H >> 2) & 3) << 4)
        q[..., base + 64:base + 96] = (L[..., 0:32] >> 4) | (((H >> 4) & 3) << 4)
        q[..., base + 96:base + 128] = (L[..., 32:64] >> 4) | (((H >> 6) & 3) << 4)
    dsc = d[..., None] * sc                                                       # [n, nb, 16], one per 16 elements
    dsc = np.repeat(dsc, 16, axis=-1)
    return (dsc * q).reshape(n, k), (32.0 * dsc).reshape(n, k)


# ---- weight generators (native GGUF bytes, row-major [n][k])
def _rand_f16(rng, shape, lo_exp: int, hi_exp: int, subnormal_frac: float = 1 / 64) -> np.ndarray:
    """f16 bit patterns of both signs, |value| log-uniform in [2^lo, 2^hi), a fraction of them subnormal."""
    mag = 2.0 ** rng.uniform(lo_exp, hi_exp, shape)
    v = (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float16)
    bits = v.view(np.uint16).copy()
    sub = rng.random(shape) < subnormal_frac
    bits[sub] = (rng.integers(1, 0x400, shape).astype(np.uint16) | (rng.integers(0, 2, shape).astype(np.uint16) << 15))[sub]
    return bits


def _put_f16(b: np.ndarray, off: int, bits: np.ndarray) -> None:
    b[..., off] = (bits & 0xFF).astype(np.uint8)
    b[..., off + 1] = (bits >> 8).astype(np.uint8)


# |w| <= 1: log2 of the largest |d| (and |dmin|) per format
_D_EXP = {"Q4_0": -3, "Q8_0": -7, "Q4_K": -10, "Q5_K": -11, "Q6_K": -12}
_DMIN_EXP = -6


def _full(tname: str, k: int, n: int, rng) -> np.ndarray:
    be, bb = BLOCK[tname]
    b = rng.integers(0, 256, (n, k // be, bb), dtype=np.uint8)                   # every quant and scale byte random
    hi = _D_EXP[tname]
    if tname in ("Q4_0", "Q8_0"):
        _put_f16(b, 0, _rand_f16(rng, b.shape[:2], hi - 6, hi))
        if tname == "Q8_0":
            b[:, 0, 2] = 0x80                                                     # -128 present in every row
            b[:, 0, 3] = 0x7F
    elif tname in ("Q4_K", "Q5_K"):
        _put_f16(b, 0, _rand_f16(rng, b.shape[:2], hi - 6, hi))
        _put_f16(b, 2, _rand_f16(rng, b.shape[:2], _DMIN_EXP - 6, _DMIN_EXP))
        b[:, 0, 4] = 63; b[:, 0, 8] = 0                                           # sub-block 0: scale 63, min 0
        b[:, 0, 5] = 0; b[:, 0, 9] = 63                                           # sub-block 1: scale 0, min 63
    else:
        _put_f16(b, 208, _rand_f16(rng, b.shape[:2], hi - 6, hi))
        b[:, 0, 192] = 0x80                                                       # int8 scales -128 and 127 in every row
        b[:, 0, 193] = 0x7F
    return b.reshape(-1)


def _extreme(tname: str, k: int, n: int, rng) -> np.ndarray:
    """Even rows: every quant and scale at its largest value; odd rows: at the value of largest magnitude below the offset."""
    be, bb = BLOCK[tname]
    b = np.zeros((n, k // be, bb), np.uint8)
    hi, lo = np.arange(n) % 2 == 0, np.arange(n) % 2 == 1
    hi_exp = _D_EXP[tname]
    if tname in ("Q4_0", "Q8_0"):
        _put_f16(b, 0, _rand_f16(rng, b.shape[:2], hi_exp - 1, hi_exp, 0.0))
        if tname == "Q4_0":
            b[hi, :, 2:18] = 0xFF                                                 # q = 15; odd rows q = 0 (q - 8 = -8)
        else:
            b[hi, :, 2:34] = 0x7F
            b[lo, :, 2:34] = 0x80
    elif tname in ("Q4_K", "Q5_K"):
        _put_f16(b, 0, _rand_f16(rng, b.shape[:2], hi_exp - 1, hi_exp, 0.0))
        _put_f16(b, 2, _rand_f16(rng, b.shape[:2], _DMIN_EXP - 1, _DMIN_EXP, 0.0))
        b[..., 4:16] = 0xFF                                                       # every scale and min 63
        b[hi, :, 16:] = 0xFF                                                      # q = 15 / 31 (Q5_K: qh too)
    else:
        _put_f16(b, 208, _rand_f16(rng, b.shape[:2], hi_exp - 1, hi_exp, 0.0))
        b[hi, :, 0:192] = 0xFF                                                    # q' = 63, scale 127
        b[hi, :, 192:208] = 0x7F
        b[lo, :, 192:208] = 0x80                                                  # q' = 0 (q' - 32 = -32), scale -128
    return b.reshape(-1)


def weights(tname: str, kind: str, k: int, n: int, seed: int, orc=None, synth_fill=None) -> np.ndarray:
    """Native GGUF bytes of an [n, k] matrix.  kind: 'synth' (the synthetic-model generator, synth_fill(name, type, count, k)),
    'full' (every header field over its full range), 'extreme' (quants and scales at their extremes), 'quantized'
    (orc.quantize of a heavy-tailed matrix)."""
    rng = np.random.default_rng(seed)
    if kind == "synth":
        return synth_fill("blk.%d.test.weight" % (seed % 1000), TYPE[tname], k * n, k)
    if kind == "quantized" or tname not in BLOCK:
        w = rng.standard_t(2.5, (n, k)) * 0.05
        if tname in ("F32", "F16"):
            return np.ascontiguousarray(w.astype(np.float32 if tname == "F32" else np.float16)).reshape(-1).view(np.uint8)
        return orc.quantize(TYPE[tname], w.astype(np.float32))
    return (_full if kind == "full" else _extreme)(tname, k, n, rng)


WEIGHT_KINDS = ("synth", "full", "extreme", "quantized")


# ---- activation generators
def activation(kind: str, k: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(k)
    ch = x.reshape(-1, 16) if k % 16 == 0 else None
    if kind == "normal":
        pass
    elif kind == "outlier":                      # one element per 7th chunk at 1e3 x the rest of its chunk
        for c in range(0, ch.shape[0], 7):
            j = rng.integers(16)
            ch[c, j] = 1e3 * np.abs(np.delete(ch[c], j)).max() * rng.choice([-1.0, 1.0])
    elif kind == "scales":                       # neighbouring chunks 1e4 apart
        ch *= np.where(np.arange(ch.shape[0]) % 2 == 0, 1e2, 1e-2)[:, None]
    elif kind == "zeros":                        # all-zero chunks and chunks of signed zeros
        ch[0::3] = 0.0
        ch[1::6] = -0.0
    elif kind == "tiny":                         # chunks below the XQ exponent clamp
        ch[0::2] *= 1e-30
    elif kind == "pow2":                         # chunk maxima exactly at and just below a power of two
        for c in range(ch.shape[0]):
            j = int(np.abs(ch[c]).argmax())
            e = 2.0 ** int(np.floor(np.log2(abs(ch[c, j]))) + 1)
            top = e if c % 2 == 0 else float(np.nextafter(np.float32(e), np.float32(0)))
            ch[c] *= top / abs(ch[c, j])
            ch[c, j] = np.copysign(top, ch[c, j])
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


ACT_KINDS = ("normal", "outlier", "scales", "zeros", "tiny", "pow2")


# ---- the operations and their bounds
def chunk_max(v: np.ndarray) -> np.ndarray:
    """m(i) of the int8 kernel: max |v| over each element's 16-element chunk."""
    a = np.abs(np.asarray(v, np.float64))
    return np.repeat(a.reshape(-1, 16).max(axis=1), 16)


def _xq_clamp_err(v: np.ndarray) -> np.ndarray:
    """Absolute XQ error of elements in chunks below the exponent clamp (sx / 2, sx = 2^-126), else 0."""
    m = chunk_max(v)
    return np.where(m < 2.0 ** -97, 2.0 ** -127, 0.0)


def inv_rms(x, eps: float) -> float:
    x = np.asarray(x, np.float64)
    return float(1.0 / np.sqrt(np.mean(x * x) + eps))


def matvec(a, o, x, nw=None, eps: float = 1e-5, bias=None, family: str = "mfma", xerr=None):
    """(y, err): y = W . (x * nw) * inv + bias in float64 and the bound of |got - y| for the kernel `family`.
    xerr: a bound of the error of the kernel's input x itself (an earlier launch's output): it adds sum_i |w_i| xerr_i |nw_i| inv, and
    m(i) is taken over |v| + that error."""
    x64 = np.asarray(x, np.float64)
    v = x64 if nw is None else x64 * np.asarray(nw, np.float64)
    inv = 1.0 if nw is None else inv_rms(x64, eps)
    y = ((a - o) @ v) * inv
    k = a.shape[1]
    ve = np.zeros(k) if xerr is None else np.asarray(xerr, np.float64) * (1.0 if nw is None else np.abs(np.asarray(nw, np.float64)))
    if xerr is not None and nw is not None:    # inv of the perturbed input: relative change <= max_i xerr_i / rms-scale
        inv = inv * (1.0 + float(np.sqrt(np.mean(np.asarray(xerr, np.float64) ** 2))) * inv)
    m = chunk_max(np.abs(v) + ve) if family == "mfma" else np.abs(v) + ve
    M = (np.abs(a) + np.abs(o)) @ m
    err = c_for(family, k) * U * M * inv + 8 * k * TINY + (np.abs(a - o) @ ve) * inv + (np.abs(y) * (
        float(np.sqrt(np.mean(np.asarray(xerr, np.float64) ** 2))) * inv if xerr is not None and nw is not None else 0.0))
    if family == "mfma":
        err = err + (np.abs(a) @ _xq_clamp_err(v)) * inv
    if bias is not None:
        b = np.asarray(bias, np.float64)
        y = y + b
        err = err + 2 * U * (np.abs(b) + np.abs(y))
    return y, err


def resid(y, err, r):
    r = np.asarray(r, np.float64)
    return y + r, err + 2 * U * (np.abs(y) + np.abs(r))


def _silu(g):
    return g / (1.0 + np.exp(-g))


def swiglu(g, eg, u, eu):
    s = _silu(g)
    return s * u, 1.1 * np.abs(u) * eg + np.abs(s) * eu + 8 * U * np.abs(s * u) + 8 * TINY


def rope_cs(orc, pos: int, head_dim: int, base: float, scale: float):
    """The engine's f32 (cos, sin) [head_dim / 2] at `pos`, recovered exactly from the oracle: rotating the unit vector (1, 0)
    of every pair gives (c, s) bit for bit."""
    q = np.zeros((1, 1, head_dim), np.float32)
    q[..., 0::2] = 1.0
    rq, _ = orc.rope(q, q.copy(), pos, base, scale, False)
    return rq[0, 0, 0::2].astype(np.float64), rq[0, 0, 1::2].astype(np.float64)


def rope(y, err, c, s, head_dim: int):
    """RoPE on pairs (2i, 2i+1) of every head of y with the f32 table values c, s [head_dim / 2]."""
    y2, e2 = np.asarray(y, np.float64).reshape(-1, head_dim // 2, 2), np.asarray(err, np.float64).reshape(-1, head_dim // 2, 2)
    x0, x1, e0, e1 = y2[..., 0], y2[..., 1], e2[..., 0], e2[..., 1]
    out = np.stack([x0 * c - x1 * s, x0 * s + x1 * c], axis=-1).reshape(-1)
    eb = np.abs(c) * e0 + np.abs(s) * e1 + 4 * U * (np.abs(x0 * c) + np.abs(x1 * s)) + 4 * TINY
    eb2 = np.abs(s) * e0 + np.abs(c) * e1 + 4 * U * (np.abs(x0 * s) + np.abs(x1 * c)) + 4 * TINY
    return out, np.stack([eb, eb2], axis=-1).reshape(-1)


def moe_down(ys, errs, w, r=None):
    """sum_p w_p y_p in selection order (+ r) and its bound."""
    w = np.asarray(w, np.float64)
    acc = np.zeros_like(np.asarray(ys[0], np.float64))
    mag = np.zeros_like(acc)
    err = np.zeros_like(acc)
    for p in range(len(ys)):
        acc = acc + w[p] * np.asarray(ys[p], np.float64)
        mag = mag + np.abs(w[p] * np.asarray(ys[p], np.float64))
        err = err + abs(w[p]) * errs[p]
    if r is not None:
        acc = acc + np.asarray(r, np.float64)
        mag = mag + np.abs(np.asarray(r, np.float64))
    return acc, err + (len(ys) + 2) * U * mag + 8 * TINY


def router(x, nw, eps: float, wr, top_k: int):
    """(sel, weights, logits, logit_err): float64 logits of RMSNorm(x) * nw against wr [E, hidden], a stable descending top-k (ties
    keep the lower index), softmax over the k logits; logit_err bounds the kernel's f32 logits."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(wr, np.float64)
    xn = x64 * inv_rms(x64, eps) * np.asarray(nw, np.float64)
    logits = w64 @ xn
    order = sorted(range(len(logits)), key=lambda e: (-logits[e], e))
    sel = np.array(order[:top_k], np.int32)
    top = logits[sel]
    p = np.exp(top - top.max())
    lerr = c_f32(x64.size) * U * (np.abs(w64) @ np.abs(xn)) + 8 * TINY
    return sel, p / p.sum(), logits, lerr


# ---- the matrix-core planner (csrc/matvec_mfma.hip: mvq_plan), restated
MVQ_WAVES = 8        # waves of a full workgroup
MVQ_CUS = 256        # the planner aims at one workgroup per CU


def mvq_geometry(k: int, n: int, launch_rows=None) -> dict:
    """The workgroup shape of a [n, k] weight (k a multiple of 256) in a launch of launch_rows rows in all (default: n).
    T k-slices: the largest divisor of k / 256 up to 8, or 8 uneven slices when that divisor is below 4 and there are more than 8
    blocks; G = 8 // T row groups; nbw = ceil(nblk / T) blocks per slice, `slices` the blocks each slice really has (the last busy one
    may be short, the ones behind it idle); 64 T G threads.  A workgroup takes R = Rg G tiles of 16 rows: one workgroup per CU, rounded
    up to whole row groups and capped at rmax (the epilogue gives every row a thread); n_wg workgroups, the last with `last` tiles."""
    if k <= 0 or k % 256 or n <= 0:
        raise ValueError("k must be a positive multiple of 256, n positive")
    nblk = k // 256
    T = max(t for t in range(1, min(MVQ_WAVES, nblk) + 1) if nblk % t == 0)
    if T < MVQ_WAVES // 2 and nblk > MVQ_WAVES:
        T = MVQ_WAVES
    G = MVQ_WAVES // T
    nbw = -(-nblk // T)
    slices = tuple(max(0, min(nbw, nblk - s * nbw)) for s in range(T))
    threads = 64 * T * G
    tiles = -(-n // 16)
    R = -(-(-(-max(launch_rows or n, n) // 16)) // MVQ_CUS)
    R = -(-R // G) * G
    rmax = threads // 16 // G * G
    R = min(R, rmax)
    n_wg = -(-tiles // R)
    return dict(T=T, G=G, nbw=nbw, slices=slices, idle=sum(1 for b in slices if b == 0), threads=threads, Rg=R // G, R=R, rmax=rmax,
                n_wg=n_wg, last=tiles - (n_wg - 1) * R)


def mvq_class(k: int) -> str:
    """The geometry class of k: '(T,G)', and for T = 8 how its slices divide the blocks."""
    g = mvq_geometry(k, 16)
    if g["T"] < 8:
        return "(%d,%d)" % (g["T"], g["G"])
    if len(set(g["slices"])) == 1:
        return "(8,1) even"
    return "(8,1) uneven busy" if g["idle"] == 0 else "(8,1) uneven idle%d" % g["idle"]
