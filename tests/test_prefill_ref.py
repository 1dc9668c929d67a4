"""CPU checks of tests/prefill_ref.py, the float64 judge of tests/test_gpu_prefill_ref.py: the emulated f16 operands against the
oracle's dequantization, the plan restatement, the path's contract (the f16 rounding against the true product) over every weight
and activation generator with every input inside the stated domain, where that contract ends for small activations, and the
power of the GPU bound: every planted mistake must exceed it at the smallest shape of its GPU test (the factor is printed)."""
import numpy as np
import pytest

import matvec_ref as mr
import prefill_ref as pr

SHAPES = [(256, 16), (512, 272), (1280, 32), (2048, 48)]      # the GPU shapes' k (the wide ones cut to a few rows)
M = 17


def _raw(pkg, orc, tname, kind, k, n, seed):
    return mr.weights(tname, kind, k, n, seed, orc=orc, synth_fill=pkg.synth.fill_tensor)


@pytest.mark.parametrize("kind", mr.WEIGHT_KINDS)
@pytest.mark.parametrize("tname", mr.FUSED)
def test_operand_matches_oracle(pkg, orc, tname, kind):
    """w' / 256 against the oracle's f32 dequantization within the tier-1 bound; u and s rebuild matvec_ref's a exactly."""
    k, n = 512, 24
    raw = _raw(pkg, orc, tname, kind, k, n, 3)
    op = pr.Operand(tname, raw, k, n)
    assert op.u.min() >= 0 and op.u.max() <= pr.U_MAX[tname] and np.array_equal(op.u, np.rint(op.u))
    assert np.array_equal(op.s * (op.u - (128.0 if tname == "Q8_0" else 0.0)), op.a)
    assert pr.domain(op.a, op.o, np.zeros(1), op.S, op.O)
    want = orc.dequantize(mr.TYPE[tname], raw, k * n).reshape(n, k).astype(np.float64)
    e = pr.w_err(tname, op.a, op.o) + mr.U * np.abs(want)
    r = float((np.abs(op.W - want) / e).max())
    print("OPERAND %s %s: worst |W' - w| / bound %.3g" % (tname, kind, r))
    assert r <= 1.0
    if kind != "extreme":                                       # the rounding is really there (not an f32 copy of the weight)
        assert (op.W != want).any() or tname in ("Q8_0", "Q4_0")


def test_operand_rounds_once():
    """u S + O is rounded once: a value whose double rounding (through f32 or through a rounded product) differs."""
    S, O, u = pr.f16(1.0 + 2.0 ** -10), pr.f16(-2.0 ** -12), 3.0
    exact = u * S + O                                           # 3 + 1.375 ulp; the product alone is a tie (3 + 1.5 ulp) that rounds up
    assert pr.w_operand("Q4_0", u, S, O) == float(np.float16(exact))
    assert pr.w_operand("Q4_0", u, S, O) != pr.f16(pr.f16(u * S) + O)


def test_xh_layout():
    m, k = 19, 512
    x = np.arange(m * k, dtype=np.float64).reshape(m, k)
    buf = pr.xh_pack(x)
    assert np.array_equal(pr.xh_read(buf, m, k), x)
    assert np.isnan(buf).sum() == buf.size - m * k               # every slot written once, rows m.. untouched
    t, q = 5, 9                                                  # token 5, chunk 9 of slab 1: position 9 ^ 5, order 0,2,1,3,4,6,5,7
    base = 1 * 128 * 256 + t * 256 + ((q ^ (t & 15)) << 3)
    assert list(buf[base:base + 8]) == [x[t, 256 + 8 * q + j] for j in (0, 2, 1, 3, 4, 6, 5, 7)]


def test_plan():
    """pf_plan restated: the shapes of the GPU tests and the real plans the issue names."""
    assert pr.pf_plan([16], 256) == (1, 1, 1, 1)
    assert pr.pf_plan([272], 512) == (2, 2, 1, 1)
    assert pr.pf_plan([13312], 1280) == (52, 3, 2, 1)            # double buffer, a short last split
    assert pr.pf_plan([16640], 2048) == (65, 3, 3, 2)            # an odd count per split
    assert pr.pf_plan([8192, 1024, 1024], 8192) == (40, 6, 6, 2)  # Llama-3-70B QKV
    for k, n in [(256, 16), (1024, 272), (2048, 64), (5632, 80), (4096, 1040)]:
        assert pr.pf_plan([n], k)[2] == 1                        # test_gpu_prefill.py's first five shapes: one block per split
    assert [pr.m_tile_width(m) for m in (1, 32, 33, 64, 65, 128)] == [2, 2, 4, 4, 8, 8]
    assert pr.c_pf(1280, 3, 1) == 512 + 3 + 1


@pytest.mark.parametrize("tname", mr.FUSED)
def test_contract(pkg, orc, tname):
    """The emulated product against the true (a - o) . x inside the derived u_h bound, every generated input inside the domain."""
    worst = 0.0
    for k, n in SHAPES:
        X = pr.act_block(k, M, k + n)
        Xq = pr.x_operand(X)
        for wi, kind in enumerate(mr.WEIGHT_KINDS):
            op = pr.Operand(tname, _raw(pkg, orc, tname, kind, k, n, 50 + wi), k, n)
            assert pr.domain(op.a, op.o, X, op.S, op.O), (tname, kind, k, n)
            y = X.astype(np.float64) @ (op.a - op.o).T
            r = float((np.abs(pr.gemm(op.W, Xq) - y) / pr.contract_bound(tname, op.a, op.o, X)).max())
            worst = max(worst, r)
    print("CONTRACT %s: worst |Y' - y| / bound %.3g" % (tname, worst))
    assert worst <= 1.0


def test_domain_edges():
    a, o = np.array([[1.0, 2.0]]), np.zeros((1, 2))
    assert pr.domain(a, o, [1.0])
    assert not pr.domain(a * 128, o, [1.0])                      # |w| = 256
    assert not pr.domain(a, o, [65504.0])
    assert pr.domain(a, o, [65503.0])
    S, O = pr.scale_offset("Q8_0", np.array([2.0]), np.array([0.0]))
    assert np.isfinite(S).all() and not np.isfinite(O).all()     # 256 * 2 * 128 overflows f16 although |w| may be tiny
    assert not pr.domain(np.zeros((1, 1)), np.zeros((1, 1)), [1.0], S, O)


def _rel_rms(op, scale, k, seed=0):
    h = (np.random.default_rng(seed).standard_normal((32, k)) * scale).astype(np.float32)
    y = h.astype(np.float64) @ (op.a - op.o).T
    d = pr.gemm(op.W, pr.x_operand(h)) - y
    return float(np.sqrt(np.mean(d * d)) / np.sqrt(np.mean(y * y)))


def scale_floor(op, k):
    """The largest row scale 10^(-j/8) of Gaussian h * nw at which the emulated GEMM exceeds rms(d) <= 2e-3 rms(y)."""
    for j in range(16, 64):
        s = 10.0 ** (-j / 8)
        if _rel_rms(op, s, k) > 2e-3:
            return s
    raise AssertionError("no floor above 1e-8")


def test_scale_floor_and_synthetic_models(pkg, orc):
    """Where the relative contract ends: XH stores h * nw BEFORE the 1/rms, so rows far below 1 fall into the f16 subnormals.
    The figure recorded in DESIGN.md (a computed one, Gaussian rows, 4096 columns), and the synthetic models' own first-layer
    rows against it."""
    k, n = 4096, 64
    op = pr.Operand("Q4_K", _raw(pkg, orc, "Q4_K", "quantized", k, n, 9), k, n)
    assert _rel_rms(op, 1.0, k) < 6e-4 and _rel_rms(op, 1e-3, k) < 6e-4
    floor = scale_floor(op, k)
    print("FLOOR row scale %.3g (rel rms there %.3g; at 1e-4: %.3g)" % (floor, _rel_rms(op, floor, k), _rel_rms(op, 1e-4, k)))
    assert 1e-6 < floor < 1e-5                                    # DESIGN.md states 7.5e-6
    for name, mix in [("test-dense", "Q4_K_M"), ("test-moe", "Q5_K_M"), ("test-dense-d128", "Q4_K_M")]:
        model = pkg.SynthModel(pkg.make_config(name), mix=mix)
        t = {nm: (ty, ne, data) for nm, ty, ne, data in model.tensors(layers=range(1))}
        ty, ne, data = t["token_embd.weight"]
        H = ne[0]
        rb = orc.nbytes_for(ty, H)
        rows = np.stack([orc.dequantize(ty, data[i * rb:(i + 1) * rb], H) for i in range(0, ne[1], max(1, ne[1] // 64))])
        nw = np.ascontiguousarray(t["blk.0.attn_norm.weight"][2]).view(np.float32)
        rms = np.sqrt(np.mean((rows * nw) ** 2, axis=1))
        print("SYNTH %s/%s: rms(h * nw) of embedding rows min %.3g" % (name, mix, rms.min()))
        assert rms.min() > 100 * floor and np.abs(rows * nw).max() < pr.F16_MAX


# ---- the bound's power: planted mistakes
def _factor(what, y_bad, y, err):
    r = float((np.abs(y_bad - y) / err).max())
    print("MUTATION %s: %.3g x the bound" % (what, r))
    return r


@pytest.fixture(scope="module")
def base(pkg, orc):
    """k = 256, n = 16, m = 17: the smallest GEMM shape of the GPU tests, per format."""
    k, n = 256, 16
    X = pr.x_operand(pr.act_block(k, M, 1))
    out = {}
    for tname in mr.FUSED:
        op = pr.Operand(tname, mr.weights(tname, "full", k, n, 21), k, n)
        out[tname] = (op, pr.gemm(op.W, X), pr.gemm_bound(op.W, op.sub, X, 1))
    return X, out


def test_mutation_chunk_elements_not_swapped(base):
    X, out = base
    op, y, err = out["Q4_K"]
    bad = pr.xh_read(pr.xh_pack(X, swap=False), M, 256)
    assert _factor("XH elements 1, 2 not swapped", pr.gemm(op.W, bad), y, err) > 1.0


def test_mutation_swizzle_dropped_for_one_token(base):
    X, out = base
    op, y, err = out["Q4_K"]
    buf = pr.xh_pack(X, plain_token=3)
    bad = pr.xh_read(buf, M, 256)
    assert np.array_equal(np.delete(bad, 3, axis=0), np.delete(X, 3, axis=0))
    r = np.abs(pr.gemm(op.W, np.nan_to_num(bad)) - y) / err
    assert _factor("XH swizzle dropped for token 3", pr.gemm(op.W, np.nan_to_num(bad)), y, err) > 1.0 and r[3].max() > 1.0


@pytest.mark.parametrize("tname", ["Q4_K", "Q5_K"])
def test_mutation_subblock_scales_of_steps_2_3_from_0_1(base, tname):
    X, out = base
    op, y, err = out[tname]
    S, O = op.S.copy(), op.O.copy()
    S[:, 128:], O[:, 128:] = op.S[:, :128], op.O[:, :128]
    W = pr.w_operand(tname, op.u, S, O) / pr.SCALE
    assert _factor("%s scales of steps 2, 3 from steps 0, 1" % tname, pr.gemm(W, X), y, err) > 1.0


def test_mutation_q6k_high_bits_shifted_one_chunk(base):
    X, out = base
    op, y, err = out["Q6_K"]
    lo, hi = op.u % 16, op.u // 16
    u = lo + 16 * np.roll(hi.reshape(16, 16, 16), 1, axis=1).reshape(16, 256)
    W = pr.w_operand("Q6_K", u, op.S, op.O) / pr.SCALE
    assert _factor("Q6_K high bits shifted by one chunk", pr.gemm(W, X), y, err) > 1.0


def test_mutation_q5k_fifth_bit_of_odd_steps_from_even(base):
    X, out = base
    op, y, err = out["Q5_K"]
    st = op.u.reshape(16, 4, 64).copy()
    st[:, 1::2] = st[:, 1::2] % 16 + 16 * (st[:, 0::2] // 16)
    W = pr.w_operand("Q5_K", st.reshape(16, 256), op.S, op.O) / pr.SCALE
    assert _factor("Q5_K fifth bit of odd steps from even steps", pr.gemm(W, X), y, err) > 1.0


@pytest.mark.parametrize("tname", mr.FUSED)
def test_mutation_split_mistakes(tname):
    """k = 1280, S = 3 (blocks 2, 2, 1), a few of the 13312 rows: the short last split loses its block / one split is not added."""
    k, n = 1280, 16
    rg, S, per, last = pr.pf_plan([13312], k)
    X = pr.x_operand(pr.act_block(k, M, 2))
    op = pr.Operand(tname, mr.weights(tname, "full", k, n, 22), k, n)
    y, err = pr.gemm(op.W, X, S), pr.gemm_bound(op.W, op.sub, X, S)
    assert np.array_equal(y, pr.gemm(op.W, X, S, skip_split=-1))
    assert _factor("%s last block of the short split dropped" % tname, pr.gemm(op.W, X, S, drop_last_block=True), y, err) > 1.0
    for s in range(S):
        assert _factor("%s split %d not added" % (tname, s), pr.gemm(op.W, X, S, skip_split=s), y, err) > 1.0


# ---- the layer steps
@pytest.fixture(scope="module")
def qkv_case(orc):
    """H = 256, head_dim 64, 4 q heads on 1 kv head, m = 19 at pos0 = 5: the smallest QKV shape of the GPU tests."""
    H, hd, m, pos0 = 256, 64, 19, 5
    mix, rows = ("Q4_K", "Q8_0", "Q4_0"), (256, 64, 64)
    ops = [pr.Operand(t, mr.weights(t, "full", H, n, 31 + s), H, n) for s, (t, n) in enumerate(zip(mix, rows))]
    h = pr.act_block(H, m, 4)
    nw = (1 + 0.2 * np.random.default_rng(4).standard_normal(H)).astype(np.float32)
    cs = [mr.rope_cs(orc, pos0 + t, hd, 10000.0, 1.0) for t in range(m)]
    return ops, h, nw, cs, hd


def test_mutation_inv_rms_of_previous_token(qkv_case):
    ops, h, nw, cs, hd = qkv_case
    (q, eq), _, _ = pr.qkv_step(ops, h, nw, 1e-5, [None] * 3, cs, hd, 1, False)
    inv = pr.inv_rms_rows(h, 1e-5)
    bad = q / inv[:, None] * np.roll(inv, 1)[:, None]              # (the rotation is linear: scaling commutes with it)
    assert _factor("1/rms of token t - 1", bad[1:], q[1:], eq[1:]) > 1.0


def test_mutation_cache_row_off_by_one(qkv_case):
    ops, h, nw, cs, hd = qkv_case
    _, (k, ek), (v, ev) = pr.qkv_step(ops, h, nw, 1e-5, [None] * 3, cs, hd, 1, False)
    # rows written at pos0 + t + 1: row pos0 + t then holds token t - 1's
    assert _factor("K row pos0 + t + 1", np.roll(k, 1, axis=0)[1:], k[1:], ek[1:]) > 1.0
    assert _factor("V row pos0 + t + 1", np.roll(v, 1, axis=0)[1:], v[1:], ev[1:]) > 1.0


def test_mutation_neox_pairs_rotated_as_neighbours(qkv_case):
    ops, h, nw, cs, hd = qkv_case
    (q, eq), (k, ek), _ = pr.qkv_step(ops, h, nw, 1e-5, [None] * 3, cs, hd, 1, True)
    (qb, _), (kb, _), _ = pr.qkv_step(ops, h, nw, 1e-5, [None] * 3, cs, hd, 1, False)
    assert _factor("NeoX q rotated as (2i, 2i+1)", qb, q, eq) > 1.0 and _factor("NeoX k rotated as (2i, 2i+1)", kb, k, ek) > 1.0


def test_neox_rotation_matches_oracle(orc):
    hd, pos = 64, 11
    x = np.random.default_rng(2).standard_normal((1, 2 * hd))
    c, s = mr.rope_cs(orc, pos, hd, 10000.0, 1.0)
    got, _ = pr.rope_rows(x, np.zeros_like(x), [(c, s)], hd, True)
    q = x.reshape(2, 1, hd).astype(np.float32)
    rq, _ = orc.rope(q, q.copy(), pos, 10000.0, 1.0, True)
    assert np.all(np.abs(rq.reshape(-1) - got.reshape(-1)) <= 4 * mr.U * np.abs(x).max())


def test_mutation_swiglu_inv_rms_of_another_token():
    H, F, m = 256, 256, 19
    og, ou = (pr.Operand("Q4_K", mr.weights("Q4_K", "full", H, F, 41 + i), H, F) for i in range(2))
    h = pr.act_block(H, m, 8)
    nw = np.ones(H, np.float32)
    act, e = pr.swiglu_step(og, ou, h, nw, 1e-5)
    bad, _ = pr.swiglu_step(og, ou, h, nw, 1e-5, inv=np.roll(pr.inv_rms_rows(h, 1e-5), 1))
    assert _factor("SwiGLU rows with another row's 1/rms", bad, act, pr.f16_store_bound(act, e)) > 1.0


def test_ssq_bound_separates_a_dropped_wave():
    h = np.random.default_rng(3).standard_normal((4, 4096)).astype(np.float32)
    s, e = pr.ssq_ref(h)
    assert s.shape == (4, 2)
    bad = s - (h[:, 512:1024].astype(np.float64) ** 2).sum(axis=1)[:, None] * np.array([1.0, 0.0])
    assert _factor("one wave's sum of squares dropped", bad, s, e) > 1.0


# ---- the MoE step
def test_moe_group_restatement():
    sel = np.array([[2, 5], [5, 0], [2, 0], [7, 2]], np.int32)
    counts, bases, lists, rowmap, tokmap = pr.moe_group(sel, 8)
    assert list(counts) == [2, 0, 3, 0, 0, 2, 0, 1] and list(bases) == [0, 16, 16, 32, 32, 32, 48, 48]
    assert list(lists[2, :3]) == [0, 2, 3 | 1 << 8] and lists[2, 3] == pr.LIST_FILL      # token order, slot in bits 8..
    assert list(rowmap[16:20]) == [2, 2 | 1 << 8, 2 | 2 << 8, -1] and rowmap[0] == 0 and rowmap[1] == 1 << 8
    assert tokmap.tolist() == [[16, 32], [33, 0], [17, 1], [48, 18]]
    assert pr.moe_eligible(8, 2) and not pr.moe_eligible(9, 2) and not pr.moe_eligible(8, 4) and pr.moe_eligible(4, 1)


@pytest.fixture(scope="module")
def moe_case():
    """H = 256, expert width 256, 8 experts, 2 per token, m = 20: the smallest MoE shape of the GPU tests."""
    H, EI, E, m = 256, 256, 8, 20
    gate = [pr.Operand("Q5_K", mr.weights("Q5_K", "full", H, EI, 60 + e), H, EI) for e in range(E)]
    up = [pr.Operand("Q5_K", mr.weights("Q5_K", "full", H, EI, 70 + e), H, EI) for e in range(E)]
    down = [pr.Operand("Q6_K", mr.weights("Q6_K", "full", EI, H, 80 + e), EI, H) for e in range(E)]
    rng = np.random.default_rng(12)
    h = (rng.standard_normal((m, H)) * 2.0 ** rng.integers(-2, 3, (m, 1))).astype(np.float32)   # rows of different scales: 1/rms differs
    nw = (1 + 0.2 * rng.standard_normal(H)).astype(np.float32)
    wr = (rng.standard_normal((E, H)) / 16).astype(np.float32)
    sel, w, marg, _ = pr.route(h, nw, 1e-5, wr, 2)
    assert not marg.any()
    return gate, up, down, h, nw, sel, w


def test_mutation_moe_slot_weights_swapped(moe_case):
    gate, up, down, h, nw, sel, w = moe_case
    y, e, _ = pr.moe_step(gate, up, down, h, nw, 1e-5, sel, w)
    assert _factor("MoE slot weights swapped", pr.moe_step(gate, up, down, h, nw, 1e-5, sel, w[:, ::-1])[0], y, e) > 1.0


def test_mutation_moe_tokmap_row_of_the_other_slot(moe_case):
    gate, up, down, h, nw, sel, w = moe_case
    y, e, _ = pr.moe_step(gate, up, down, h, nw, 1e-5, sel, w)
    bad = pr.moe_step(gate, up, down, h, nw, 1e-5, sel[:, ::-1], w)[0]      # slot s reads the row of slot 1 - s, weights stay
    assert _factor("tokmap row of the other slot", bad, y, e) > 1.0


def test_mutation_moe_swiglu_inv_rms_of_the_row_index(moe_case):
    gate, up, down, h, nw, sel, w = moe_case
    y, e, acts = pr.moe_step(gate, up, down, h, nw, 1e-5, sel, w)
    inv = pr.inv_rms_rows(h, 1e-5)
    bad, _, bad_acts = pr.moe_step(gate, up, down, h, nw, 1e-5, sel, w, inv_of=lambda tokens, rows: inv[rows])
    ex = max(ee for ee in acts if len(acts[ee][0]) > 1)
    a, ea = acts[ex]
    assert _factor("expert SwiGLU rows with the 1/rms of the row index (act)", bad_acts[ex][0], a, pr.f16_store_bound(a, ea)) > 1.0
    assert _factor("expert SwiGLU rows with the 1/rms of the row index (hidden)", bad, y, e) > 1.0
