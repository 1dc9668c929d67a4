"""A float64 restatement of the launches of a decode step AROUND the fused mat-vecs, the arbiter of tests/test_gpu_step_launches.py:
the embedding launches (the table row, its XQ image and sums of squares), qkv_forward's branches (three mat-vecs, RoPE in either
pairing, the cache row or the staged rows), the unfused gate / up pair, and the last-maximal arg-max.

Nothing here introduces a tolerance: a table row is the oracle's dequantization, bit for bit; images are held to
matvec_multi_ref.image_ref; mat-vecs to matvec_ref.matvec with the family matvec_ref.kernel_family names; RoPE to matvec_ref.rope
(pairs (2i, 2i + 1)) or prefill_ref.rope_rows (NeoX: pairs (i, i + head_dim / 2)); SwiGLU to matvec_ref.swiglu.  The arg-max is exact.
The tests' inputs are functions here too, so that tests/test_step_ref.py can show on the same inputs that the checks tell a correct
result from the ways these launches go wrong."""
from __future__ import annotations

import numpy as np

import matvec_multi_ref as mm
import matvec_ref as mr
import prefill_ref as pr

EPS = 1e-5
NAN_BITS = np.uint32(0x7FC0BEEF)
FILL = 0x5A          # the byte every embedding output starts as: 0x5A5A5A5A reads as 1.5e16 in f32, far outside every bound

# ---- embedding tables: every type blk_elems knows
TYPE = dict(mr.TYPE, Q8_1=9, Q8_K=15, BF16=30)
SCALAR_TYPES = ("F32", "F16", "BF16")
BLOCK32_TYPES = ("Q4_0", "Q4_1", "Q5_0", "Q5_1", "Q8_0", "Q8_1")
BLOCK256_TYPES = ("Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K", "Q8_K")
EMBED_TYPES = SCALAR_TYPES + BLOCK32_TYPES + BLOCK256_TYPES
VOCAB = 40
EMBED_TOKENS = (0, VOCAB - 1, 17)


def embed_hiddens(tname: str):
    """512: two workgroups, chunk indices >= 16, an image; 896: no image, the last workgroup half full (not a multiple of 256, so
    only for the scalar and 32-element types)."""
    return (512,) if tname in BLOCK256_TYPES else (512, 896)


def table(tname: str, hidden: int, orc, synth_fill) -> np.ndarray:
    """Native GGUF bytes of a [VOCAB, hidden] table: the synthetic-model generator where it has one; the oracle's quantizer for the
    activation formats Q8_1 / Q8_K; the high halves of f32 words for BF16."""
    n = VOCAB * hidden
    if tname in ("Q8_1", "Q8_K"):
        return orc.quantize(TYPE[tname], (np.random.default_rng(hidden).standard_normal(n) * 3).astype(np.float32))
    if tname == "BF16":
        w = (np.random.default_rng(hidden + 1).standard_normal(n) * 0.05).astype(np.float32)
        return np.ascontiguousarray((w.view(np.uint32) >> 16).astype(np.uint16)).view(np.uint8)
    return synth_fill("token_embd.weight", TYPE[tname], n, hidden)


def norm_weight(n: int, seed: int) -> np.ndarray:
    return (1 + 0.2 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def embed_row(orc, tname: str, raw, hidden: int, token: int) -> np.ndarray:
    """Row `token` of the table, f32: the oracle's dequantization of that row's bytes."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    rb = raw.size // VOCAB
    return orc.dequantize(TYPE[tname], raw[token * rb:(token + 1) * rb], hidden)


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def filled(a) -> bool:
    """Every byte of `a` still holds FILL."""
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


def decoded_ratios(x, xs, ssq, row, nw):
    """The worst ratios (elements, chunk sums, sums of squares) of an image's decoded values and the partials against
    image_ref(row, nw)."""
    (v, ev), (sums, es), (sq, eq) = mm.image_ref(row, nw)
    return mm.ratio(x, v, ev), mm.ratio(xs, sums, es), mm.ratio(np.asarray(ssq)[:len(row) // 16], sq, eq)


def image_ratios(img, ssq, row, nw):
    x, xs = mm.xq_decode(img, len(row))
    return decoded_ratios(x, xs, ssq, row, nw)


def image_tails_kept(img) -> bool:
    """The bytes of an image its producer does not own — the last 128 of every 1280-byte record — still hold FILL."""
    return filled(np.ascontiguousarray(img, dtype=np.uint8).reshape(-1, 1280)[:, 1152:])


def pack_ssq(per_seq, stride: int, n_buf: int) -> np.ndarray:
    """Sequences' partials laid out `stride` floats apart in a FILL-ed buffer of n_buf sequences at hidden / 16 + 64 each."""
    k16 = len(per_seq[0])
    buf = np.full(n_buf * (k16 + 64) * 4, FILL, np.uint8).view(np.float32).copy()
    for s, p in enumerate(per_seq):
        buf[s * stride:s * stride + k16] = p
    return buf.reshape(n_buf, k16 + 64)


# ---- qkv_forward
MAX_SEQ, ROPE_BASE, ROPE_SCALE = 40, 500000.0, 1.0
QKV_HIDDEN = 512
QKV_POS = (0, 1, MAX_SEQ - 1)
QKV_SHAPES = ((64, 8, 2), (128, 4, 2))          # (head_dim, heads, kv heads)
# (types, neox, biases): (a) NeoX over fused types; (b) interleaved pairs over the expanded types; (d) the fused interleaved launch
QKV_UNFUSED = [(("Q4_K", "Q4_K", "Q6_K"), True, False), (("Q4_K", "Q4_K", "Q6_K"), True, True), (("Q8_0", "Q8_0", "Q8_0"), True, False),
               (("Q8_0", "Q8_0", "Q8_0"), True, True), (("Q5_0", "Q5_0", "Q5_0"), False, False), (("F16", "F16", "F16"), False, False)]
QKV_FUSED = [(("Q4_K", "Q4_K", "Q6_K"), False, False), (("Q8_0", "Q8_0", "Q8_0"), False, True)]


def qkv_inputs(types, hd: int, nh: int, nkv: int, with_bias: bool, orc):
    """(ws, nw, biases, rows) of a case: 'full' weights for the fused types, the oracle's quantizer / f16 for the expanded ones."""
    rows = (nh * hd, nkv * hd, nkv * hd)
    ws = [mr.weights(types[s], "full" if types[s] in mr.BLOCK else "quantized", QKV_HIDDEN, rows[s], 10 + s + hd, orc=orc) for s in range(3)]
    rng = np.random.default_rng(hd + nh)
    nw = (1 + 0.2 * rng.standard_normal(QKV_HIDDEN)).astype(np.float32)
    biases = [rng.standard_normal(r).astype(np.float32) if with_bias else None for r in rows]
    return ws, nw, biases, rows


def qkv_x(pi: int, with_bias: bool, pos: int) -> np.ndarray:
    return mr.activation(mr.ACT_KINDS[(pi * 2 + with_bias) % len(mr.ACT_KINDS)], QKV_HIDDEN, pos + 7)


def rotate(y, e, c, s, hd: int, neox: bool):
    if not neox:
        return mr.rope(y, e, c, s, hd)
    r, er = pr.rope_rows(np.asarray(y, np.float64)[None], np.asarray(e, np.float64)[None], [(c, s)], hd, True)
    return r[0], er[0]


def qkv_ref(orc, types, ws, nw, biases, rows, x, pos: int, hd: int, neox: bool, bias_after_rope: bool = False, pos_shift: int = 0):
    """((q, eq), (k, ek), (v, ev)): the three mat-vecs (+ bias), Q and K rotated at pos.  The two flags restate mistakes, for
    tests/test_step_ref.py: the bias added after the rotation; the rotation of position pos + pos_shift."""
    out = []
    c, s = mr.rope_cs(orc, pos + pos_shift, hd, ROPE_BASE, ROPE_SCALE)
    for i in range(3):
        fam = mr.kernel_family(types[i], QKV_HIDDEN)
        a, o = mr.decode(types[i], ws[i], QKV_HIDDEN, rows[i], orc, fam)
        late = bias_after_rope and biases[i] is not None and i < 2
        y, e = mr.matvec(a, o, x, nw=nw, eps=EPS, bias=None if late else biases[i], family=fam)
        if i < 2:
            y, e = rotate(y, e, c, s, hd, neox)
            if late:
                y = y + np.asarray(biases[i], np.float64)
        out.append((y, e))
    return out


def nan_cache(nkv: int, hd: int) -> np.ndarray:
    return np.full((nkv, MAX_SEQ, hd), NAN_BITS, np.uint32).view(np.float32)


def cache_failures(cache, pos: int, ref, err, what: str):
    """Row pos of every head holds ref within err; every other row the NaN pattern."""
    fails = []
    r = mm.ratio(cache[:, pos, :].reshape(-1), ref, err)
    if not r <= 1.0:
        fails.append("%s: row %d ratio %.3g" % (what, pos, r))
    others = np.ones(cache.shape[1], bool)
    others[pos] = False
    if not np.all(bits(cache[:, others]) == NAN_BITS):
        fails.append("%s: a cache row other than %d changed" % (what, pos))
    return fails


# ---- gate / up
FFN_HIDDEN, FFN = 512, 352
GATEUP_CASES = (("Q4_K", "Q6_K"), ("Q5_0", "Q5_0"), ("F16", "F16"))


def gateup_inputs(tg: str, tu: str, orc):
    kind = lambda t: "full" if t in mr.BLOCK else "quantized"
    return (mr.weights(tg, kind(tg), FFN_HIDDEN, FFN, 21, orc=orc), mr.weights(tu, kind(tu), FFN_HIDDEN, FFN, 22, orc=orc),
            norm_weight(FFN_HIDDEN, 23))


def gateup_ref(orc, tg: str, wg, tu: str, wu, nw, x):
    parts = []
    for t, w in ((tg, wg), (tu, wu)):
        fam = mr.kernel_family(t, FFN_HIDDEN)
        a, o = mr.decode(t, w, FFN_HIDDEN, FFN, orc, fam)
        parts.append(mr.matvec(a, o, x, nw=nw, eps=EPS, family=fam))
    return mr.swiglu(parts[0][0], parts[0][1], parts[1][0], parts[1][1])


# ---- arg-max
ARGMAX_N = (1, 255, 16384, 16385, 40000)
ARGMAX_SEQS = (0, 1, 3, 16)
PEAK = np.float32(0.5)


def argmax_last(v) -> int:
    """The last index of the row's maximum (NaN-free rows)."""
    v = np.asarray(v)
    return int(len(v) - 1 - np.argmax(v[::-1]))


def argmax_first(v) -> int:
    return int(np.argmax(np.asarray(v)))


def argmax_rows(n: int, seed: int):
    """[(name, row, is_tie)]: rows of -|N(0, 1)| - 1 with maxima planted.  Stage 1 gives index i to workgroup (i // 256) % 64, thread
    i % 256; `is_tie` rows hold their maximum more than once (n = 1 cannot)."""
    rng = np.random.default_rng(seed)
    base = lambda: (-np.abs(rng.standard_normal(n)) - 1).astype(np.float32)
    rows = []

    def plant(name, idx, val=PEAK, vals=None):
        r = base()
        idx = sorted(set(int(i) for i in idx if 0 <= i < n))
        for j, i in enumerate(idx):
            r[i] = val if vals is None else vals[j % len(vals)]
        rows.append((name, r, len(idx) > 1))

    mid = n // 2
    plant("two lanes of one workgroup", (mid, mid + 3) if mid % 256 < 253 else (mid - 3, mid))
    plant("one thread twice", (5, 5 + 16384) if n > 5 + 16384 else (n // 3, n // 3 + 1))
    plant("two workgroups", (3, 256 + 200, n - 256 - 2))
    plant("first and last index", (0, n - 1))
    plant("last index alone", (n - 1,))
    plant("+0 then -0", (n // 4, n // 4 + n // 2), vals=(np.float32(0.0), np.float32(-0.0)))
    plant("-0 then +0", (n // 5, n - 1 - n // 7), vals=(np.float32(-0.0), np.float32(0.0)))
    plant("+inf twice", (n // 6, n - 1 - n // 6), val=np.float32(np.inf))
    rows.append(("all -inf", np.full(n, -np.inf, np.float32), n > 1))
    return rows


def argmax_batches(n: int, n_seq: int, seed: int):
    """Matrices [n_seq, n] over argmax_rows: sequence s of batch b holds row (b + s) of the list, so neighbouring sequences have their
    maxima elsewhere, and every row kind meets every sequence index that n_seq allows."""
    rows = argmax_rows(n, seed)
    n_batches = len(rows) if n_seq < len(rows) else 2
    return [np.stack([rows[(b + s) % len(rows)][1] for s in range(n_seq)]) for b in range(n_batches)]
