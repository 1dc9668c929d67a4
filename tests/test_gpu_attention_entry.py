"""Nothing a cache holds at or past kv_len may reach the output of the f32 decode attention (attn_partial_kernel,
csrc/attention.hip) — not through 0 * NaN either.  The kernel requests rows unconditionally and clamps the row index, so this is a
property of its clamp and of its masking, at every length at which a wave, a first batch or the cache ends.

Every case runs three times through the per-path entry point (the engine's own launch sequence, position in the device word), with
the cache rows at and past kv_len set to zeros, to NaN and to +Inf: the three outputs must be bitwise equal, and the first within
the bound of the float64 restatement (tests/attention_ref.py, the bound of tests/test_gpu_attention.py).  The entry points keep
each cache in a device allocation with 1024 rows of NaN behind the last head, so a wrong clamp reads those.

F = n_splits x waves x rows per wave-instruction is the first batch: the rows the first iteration of all waves covers.  kv_len runs
over both sides of one wave-instruction (RPW), of F, and of the cache's end; one cache is shorter than F, one is long enough for
the 8-wave instantiation with a second batch.  The same through the multi-sequence launch."""
import numpy as np
import pytest

import attention_ref as ar

pytestmark = pytest.mark.gpu

SHAPES = [(8, 2, 128), (8, 1, 64)]   # heads, kv heads, head_dim
FILLS = (0.0, np.nan, np.inf)


def _rpw(d):
    return 64 // (d // 4)


def _case(seed, nh, nkv, d, max_seq):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nh, d)).astype(np.float32)
    k = rng.standard_normal((nkv, max_seq, d)).astype(np.float32)
    v = rng.standard_normal((nkv, max_seq, d)).astype(np.float32)
    return q, k, v, float(1.0 / np.sqrt(d))


def _filled(x, n, fill):
    y = x.copy()
    y[..., n:, :] = fill
    return y


def _three_way(gpu, q, k, v, scale, n, n_splits, what):
    outs = [gpu.op_attention_decode(gpu.ATTN_SPLIT, q, _filled(k, n, f), _filled(v, n, f), scale, n - 1, n_splits) for f in FILLS]
    for f, o in zip(FILLS[1:], outs[1:]):
        assert np.array_equal(outs[0].view(np.uint32), o.view(np.uint32)), f"{what}: rows past kv_len = {f} change the output"
    ref = ar.decode(q, k, v, scale, n)
    ratio = ar.worst_ratio(outs[0], ref, ar.magnitude(q, k, scale, n), float(np.abs(v[:, :n]).max()), n)
    print(f"{what}: err / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: err / bound = {ratio:.3g}"
    return outs[0]


@pytest.mark.parametrize("n_splits", [8, 32])
@pytest.mark.parametrize("nh,nkv,d", SHAPES)
def test_rows_past_kv_len_never_reach_the_output(gpu, nh, nkv, d, n_splits):
    max_seq, rpw = 640, _rpw(d)
    F = n_splits * 4 * rpw   # max_seq < 2048: 4 waves
    assert F + 1 < max_seq - 1
    q, k, v, scale = _case([nh, nkv, d, n_splits], nh, nkv, d, max_seq)
    for n in (1, rpw, rpw + 1, F - 1, F, F + 1, max_seq - 1, max_seq):
        _three_way(gpu, q, k, v, scale, n, n_splits, f"d={d} splits={n_splits} max_seq={max_seq} kv_len={n}")


@pytest.mark.parametrize("nh,nkv,d", SHAPES)
def test_cache_shorter_than_the_first_batch(gpu, nh, nkv, d):
    max_seq, n_splits = 96, 32
    assert n_splits * 4 * _rpw(d) > max_seq   # waves whose first rows lie past the cache
    q, k, v, scale = _case([nh, nkv, d, 96], nh, nkv, d, max_seq)
    for n in (1, 50, max_seq - 1, max_seq):
        _three_way(gpu, q, k, v, scale, n, n_splits, f"d={d} splits={n_splits} max_seq={max_seq} kv_len={n}")


@pytest.mark.parametrize("nh,nkv,d", SHAPES)
def test_eight_wave_instantiation_with_a_second_batch(gpu, nh, nkv, d):
    max_seq, n_splits = 2048, 32 if d == 128 else 16
    F = n_splits * 8 * _rpw(d)
    assert F == 512
    q, k, v, scale = _case([nh, nkv, d, 2048], nh, nkv, d, max_seq)
    for n in (F + 1, F + 2 * _rpw(d) + 1):
        _three_way(gpu, q, k, v, scale, n, n_splits, f"d={d} splits={n_splits} max_seq={max_seq} kv_len={n}")


@pytest.mark.parametrize("nh,nkv,d", SHAPES)
def test_multi_sequence_launch(gpu, nh, nkv, d):
    """Two sequences at different positions in slots 2 and 0 of three; slot 1 holds the fill value only."""
    max_seq, n_splits, rpw = 320, 8, _rpw(d)
    F = n_splits * 4 * rpw
    lens, slots = [F + 1, rpw + 1], [2, 0]
    rng = np.random.default_rng([nh, nkv, d, 7])
    q = rng.standard_normal((2, nh, d)).astype(np.float32)
    k = rng.standard_normal((3, nkv, max_seq, d)).astype(np.float32)
    v = rng.standard_normal((3, nkv, max_seq, d)).astype(np.float32)
    scale = float(1.0 / np.sqrt(d))

    def filled(x, f):
        y = np.full_like(x, f)
        for n, s in zip(lens, slots):
            y[s, :, :n] = x[s, :, :n]
        return y

    outs = [gpu.op_attention_decode_multi(q, filled(k, f), filled(v, f), scale, [n - 1 for n in lens], slots, n_splits) for f in FILLS]
    for f, o in zip(FILLS[1:], outs[1:]):
        assert np.array_equal(outs[0].view(np.uint32), o.view(np.uint32)), f"d={d}: rows past kv_len = {f} change the multi-sequence output"
    for i, (n, s) in enumerate(zip(lens, slots)):
        ref = ar.decode(q[i], k[s], v[s], scale, n)
        ratio = ar.worst_ratio(outs[0][i], ref, ar.magnitude(q[i], k[s], scale, n), float(np.abs(v[s][:, :n]).max()), n)
        print(f"multi d={d} sequence {i} kv_len={n}: err / bound = {ratio:.4f}")
        assert ratio <= 1.0, f"multi d={d} sequence {i}: err / bound = {ratio:.3g}"
        # per sequence the arithmetic is the single-sequence kernel's
        single = gpu.op_attention_decode(gpu.ATTN_SPLIT, q[i], k[s], v[s], scale, n - 1, n_splits)
        assert np.array_equal(single.view(np.uint32), outs[0][i].view(np.uint32)), f"multi d={d} sequence {i} differs from the single-sequence launch"
