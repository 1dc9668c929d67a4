"""Self-test of tests/tp_prefill_ref.py (no GPU): the restatement agrees with the rank-order sum the decode kernel is held to, places
its XH where the GEMM reads it, and on tp_ref's "orders" data any other rank order or split order changes bits — which is what lets
the bit-for-bit GPU comparison of test_gpu_tp_prefill.py see a kernel that adds in another order."""
import itertools

import numpy as np
import pytest

import prefill_ref as pr
import tp_prefill_ref as tpr
import tp_ref

H, NCOLS, COL0, M = 256, 328, 64, 17


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _resid(seed):
    return (3 * np.random.default_rng(seed).standard_normal((M, H))).astype(np.float32)


def test_one_split_is_the_decode_kernels_rank_order_sum():
    for n in (1, 2, 3, 8):
        P = tpr.split_partials("orders", n, 1, NCOLS, 10 + n)
        resid = _resid(n)
        got = tpr.hidden_ref(P, COL0, resid)
        for t in (0, M - 1):
            want = tp_ref.ordered_sum(P[:, 0, t, COL0:COL0 + H], resid[t])
            assert np.array_equal(_bits(got[t]), _bits(want))


def test_zero_start_and_bias_belong_to_rank_zero():
    P = tpr.split_partials("gauss", 2, 3, NCOLS, 5)
    P[0, 0, :, COL0] = -0.0                      # 0 + -0 = +0: the zero start is part of the order
    P[0, 1:, :, COL0] = -0.0
    a = tpr.compact(P[0], COL0, H, M)
    assert not np.signbit(a[:, 0]).any()
    bias = np.random.default_rng(6).standard_normal(H).astype(np.float32)
    resid = _resid(7)
    with_b = tpr.hidden_ref(P, COL0, resid, bias)
    a0 = (tpr.compact(P[0], COL0, H, M) + bias[None, :]).astype(np.float32)
    a1 = tpr.compact(P[1], COL0, H, M)
    assert np.array_equal(_bits(with_b), _bits((resid + (a0 + a1).astype(np.float32)).astype(np.float32)))
    assert not np.array_equal(_bits(with_b), _bits(tpr.hidden_ref(P, COL0, resid)))


@pytest.mark.parametrize("n", [3, 8])
def test_another_rank_order_changes_bits(n):
    P = tpr.split_partials("orders", n, 1, NCOLS, 20 + n)
    resid = np.zeros((M, H), np.float32)
    want = tpr.hidden_ref(P, COL0, resid)
    orders = list(itertools.permutations(range(n))) if n <= 3 else [tuple(np.roll(np.arange(n), k)) for k in range(1, n)] + [tuple(range(n))[::-1]]
    seen = 0
    for o in orders:
        if set(o[:2]) == {0, 1} and list(o[2:]) == list(range(2, n)):
            continue                            # (the first add is commutative: swapping ranks 0 and 1 alone is the same sum)
        seen += 1
        assert not np.array_equal(_bits(tpr.hidden_ref(P, COL0, resid, rank_order=o)), _bits(want)), o
    assert seen >= 4


def test_rank_order_of_two_with_the_residual_last():
    """n = 2: the two blocks commute, but the residual has to come LAST: (resid + a_0) + a_1 differs."""
    P = tpr.split_partials("orders", 2, 1, NCOLS, 31)
    resid = tp_ref.partials("orders", M, H, 32)
    want = tpr.hidden_ref(P, COL0, resid)
    a0, a1 = (tpr.compact(P[r], COL0, H, M) for r in range(2))
    other = ((resid + a0).astype(np.float32) + a1).astype(np.float32)
    assert not np.array_equal(_bits(other), _bits(want))


@pytest.mark.parametrize("n", [1, 3])
def test_another_split_order_changes_bits(n):
    P = tpr.split_partials("orders", n, 3, NCOLS, 40 + n)
    resid = np.zeros((M, H), np.float32)
    want = tpr.hidden_ref(P, COL0, resid)
    for o in itertools.permutations(range(3)):
        if o in ((0, 1, 2), (1, 0, 2)):
            continue
        assert not np.array_equal(_bits(tpr.hidden_ref(P, COL0, resid, split_order=o)), _bits(want)), o
    # ... and so does adding across the ranks before across the splits
    if n > 1:
        s = np.zeros((M, H), np.float32)
        for sp in range(3):
            for r in range(n):
                s = (s + P[r, sp, :M, COL0:COL0 + H]).astype(np.float32)
        assert not np.array_equal(_bits(s), _bits(want))


def test_xh_image_is_where_the_gemm_reads_it():
    rng = np.random.default_rng(3)
    Hh = 2304
    hidden = rng.standard_normal((M, Hh)).astype(np.float32)
    nw = (1 + 0.2 * rng.standard_normal(Hh)).astype(np.float32)
    img = tpr.xh_image(hidden, nw, 0x5A)
    assert img.size == 9 * 65536
    back = pr.xh_read(img.view(np.float16).astype(np.float64), M, Hh)
    assert np.array_equal(back, pr.x_operand(hidden, nw))
    owned = np.zeros(img.size // 2, bool)
    owned[pr.xh_offset(np.arange(M)[:, None], np.arange(Hh)[None, :])] = True
    assert owned.sum() == M * Hh and np.all(img.view(np.uint16)[~owned] == 0x5A5A)
    assert np.all(tpr.xh_image(hidden, None, 0x5A) == 0x5A)
