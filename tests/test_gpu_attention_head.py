"""attn_head_kernel<D, G> (csrc/attention.hip), the single-launch decode attention with one workgroup per query head, against the
float64 restatement (tests/attention_ref.py) through lgh_op_attention_decode path 3 (ATTN_HEAD), with the position in the device
word, held to the bound of tests/test_gpu_attention.py (attention_ref.worst_ratio <= 1).

Paths of lgh_op_attention_decode:  0 split + merge  attn_partial_kernel<D,G,4 / 8> + attn_combine_kernel;  1 direct
attn_partial_kernel<D,G,16,false,true> (one workgroup per kv head);  2 any shape  attn_decode_any_kernel;  3 head
attn_head_kernel<D,G> (one workgroup per query head, two-pass softmax: the engine's single launch).

The inputs are those of test_gpu_attention.py (normal, dominant, equal, hot; two kv heads; NaN in every cache row past the visible
range, so that a read of any of them shows in the output).  The kernel deals rows in chunks of 128: a wave-instruction covers 8 K rows
and 256 / D V rows, a sweep of the 16 waves 128 K rows and 4096 / D V rows.  Up to 256 rows (2 chunks) everything is requested at
entry; beyond that four chunk buffers go round: up to 4 chunks the loops over K and V run no pass and their tails do the work, from 5
chunks on a pass of a loop consumes four chunks and refills their buffers, and from 9 chunks on a buffer refilled inside the loop is
refilled again.  KV_LENS puts kv_len one below, at and one above each of the sizes of the first sentence, at 1 and 2, at every tail
length behind zero, one and two passes (3..8 chunks in a 1024-row cache; 10 and 15 chunks in a 2048-row one), and at max_seq."""
import numpy as np
import pytest

import attention_ref as ar
import test_gpu_attention as tga
from test_gpu_attention_kv_tq_multi import _check_image

pytestmark = pytest.mark.gpu

MAX_SEQ = 1024
# 1, 2; V rows of a wave-instruction (2 at D = 128, 4 at D = 64) and K rows (8); V rows of a sweep (32 / 64) and K rows (128 = one chunk);
# the single-shot limit (256; 257 = 3 chunks); 4, 5, 6, 7 chunks, 7 chunks + 1 row; max_seq (8 chunks)
KV_LENS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 400, 600, 700, 850, 897, MAX_SEQ)
# (max_seq, kv_len) of the long cache: 10 chunks (two passes, a tail of two) and 15 (three passes, a tail of three)
LONG_CASES = ((2048, 1153), (2048, 1800))
IMAGE_LENS = (1, 9, 129, 256, 600, MAX_SEQ, 1153)
KINDS = ("normal", "dominant", "equal", "hot")


@pytest.mark.parametrize("d,g", tga.SHAPES)
def test_decode_head(gpu, d, g):
    W = tga.Worst(f"decode_head d={d} g={g}")
    for ci, (max_seq, n) in enumerate([(MAX_SEQ, n) for n in KV_LENS] + list(LONG_CASES)):
        for kind in KINDS:
            rng = np.random.default_rng([d, g, ci, len(kind), 6])
            q, k, v, scale = tga._f32_case(rng, kind, g, d, max_seq, n - 1)
            ref = ar.decode(q, k, v, scale, n)
            S, vmax = ar.magnitude(q, k, scale, n), float(np.abs(v[:, :n]).max())
            got = gpu.op_attention_decode(gpu.ATTN_HEAD, q, k, v, scale, n - 1)
            W.add("head", ar.worst_ratio(got, ref, S, vmax, n), f"kind={kind} max_seq={max_seq} kv_len={n}")
            if n in IMAGE_LENS and kind in ("normal", "hot"):
                out, img = gpu.op_attention_decode(gpu.ATTN_HEAD, q, k, v, scale, n - 1, image=True)
                assert np.array_equal(out.view(np.uint32), got.view(np.uint32)), f"kind={kind} kv_len={n}: the output changes with the image"
                _check_image(img, out, f"head kind={kind} kv_len={n}")
    W.check()


def test_head_path_refuses(gpu, pkg):
    """A shape without a kernel and a cache whose scores would not fit in LDS are refused, never served by another kernel."""
    rng = np.random.default_rng(7)
    q = rng.standard_normal((7 * 2, 96)).astype(np.float32)
    k = rng.standard_normal((2, 64, 96)).astype(np.float32)
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_attention_decode(gpu.ATTN_HEAD, q, k, k, 0.1, 3)
    assert ei.value.variant == "Unsupported"
    q = rng.standard_normal((2, 64)).astype(np.float32)
    k = np.zeros((1, 16385, 64), np.float32)
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_attention_decode(gpu.ATTN_HEAD, q, k, k, 0.1, 3)
    assert ei.value.variant == "Unsupported"
    out = gpu.op_attention_decode(gpu.ATTN_HEAD, q, k[:, :16384], k[:, :16384], 0.1, 3)   # (the largest cache it takes: V = 0)
    assert np.array_equal(out, np.zeros_like(out))


DEFAULT_SWITCH = 256   # engine.hip: kDirectAttnDefaultKv


def test_default_engine_follows_the_oracle_across_the_switch(pkg, orc):
    """A default engine runs attn_head_kernel up to DEFAULT_SWITCH rows of context and split + combine beyond (two graph variants, picked
    by the host-side position): logits within test_gpu_model's bound of the oracle at both ends and at DEFAULT_SWITCH - 1, DEFAULT_SWITCH
    and DEFAULT_SWITCH + 1 rows (the token at position p attends to p + 1 rows)."""
    n_tok = DEFAULT_SWITCH + 2
    cfg = pkg.make_config("test-dense-d128", max_seq_len=n_tok)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    eng = pkg.HipGpuInference.from_model(model, n_tok, flags=pkg.hip_backend.FLAG_EXACT_PREFILL)
    check = {0, DEFAULT_SWITCH - 2, DEFAULT_SWITCH - 1, DEFAULT_SWITCH, n_tok - 1}   # positions: 1, SWITCH - 1, SWITCH, SWITCH + 1, SWITCH + 2 rows
    worst = 0.0
    for i in range(n_tok):
        t = (13 * i + 5) % cfg.vocab_size
        if i in check:
            got, want = eng.forward(t), ref.forward([t])
            err, tol = float(np.abs(got - want).max()), 2e-3 * float(np.abs(want).max()) + 2e-3
            worst = max(worst, err / tol)
            assert err <= tol, f"position {i}: max|dlogit| = {err:.3e} > {tol:.3e}"
        else:
            eng.prefill_token(t)
            ref.forward([t])
    print(f"worst max|dlogit| / tolerance across the switch: {worst:.4f}")
    eng.close()
