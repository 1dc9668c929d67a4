"""attn_slice_kernel<D, G, S> (csrc/attention_slice.hip): the single-launch decode attention for contexts of at most 256 rows, S workgroups
per query head, each repeating the head's scores and softmax and accumulating a slice of the output's columns.  Reached through
lgh_op_attention_decode path 3 (ATTN_HEAD) with max_seq <= 256 — the engine's rule: the threshold of the context, not the position.

Every case is checked three ways:
  * against the float64 restatement (tests/attention_ref.py), held to the bound of tests/test_gpu_attention.py (worst_ratio <= 1);
  * output and XQ image bitwise equal to the same call on the same rows in a cache of max_seq = 384, which runs attn_head_kernel (the extra
    rows are NaN): the slice kernel keeps that kernel's summation tree, so the bits are its bits;
  * a second call gives the same bits.
The inputs are those of test_gpu_attention.py (normal, dominant, equal, hot; two kv heads; NaN in every cache row past the visible range).
KV_LENS: 1, 2; around the V rows of a chain sweep's wave-instruction in attn_head_kernel's layout (2 / 4) and in the slice's (8 / 16 row
slices per wave-instruction), the K rows of a wave-instruction (8), the chains (32 / 64), the chunk (128) and the limit (256)."""
import numpy as np
import pytest

import attention_ref as ar
import test_gpu_attention as tga
from test_gpu_attention_kv_tq_multi import _check_image

pytestmark = pytest.mark.gpu

MAX_SEQ = 256        # common.h: kAttnSliceMaxRows — path 3 with a cache this long selects attn_slice_kernel
HEAD_MAX_SEQ = 384   # ... and with this one attn_head_kernel
KV_LENS = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
KINDS = ("normal", "dominant", "equal", "hot")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.uint32)


def _image_bits(img, n):
    """The bytes of an XQ image that the launch writes for n elements (csrc/xq.h: per 16-element chunk j of a 1280-byte record its 64 limb
    bytes, its sum and its scale); the records' padding and the chunks past n belong to nobody and hold what the buffer held."""
    mask = np.zeros(img.size, bool)
    for c in range(n // 16):
        rec, j = (c >> 4) * 1280, c & 15
        for i in range(4):
            at = rec + ((j >> 1) * 4 + i) * 32 + (j & 1) * 16
            mask[at:at + 16] = True
        slot = (j & 3) * 4 + (j >> 2)
        mask[rec + 1024 + slot * 4:rec + 1024 + slot * 4 + 4] = True
        mask[rec + 1088 + slot * 4:rec + 1088 + slot * 4 + 4] = True
    return np.ascontiguousarray(img).reshape(-1)[mask]


@pytest.mark.parametrize("d,g", tga.SHAPES)
def test_decode_slice(gpu, d, g):
    W = tga.Worst(f"decode_slice d={d} g={g}")
    for ci, n in enumerate(KV_LENS):
        for kind in KINDS:
            rng = np.random.default_rng([d, g, ci, len(kind), 11])
            q, k, v, scale = tga._f32_case(rng, kind, g, d, HEAD_MAX_SEQ, n - 1)
            ks, vs = np.ascontiguousarray(k[:, :MAX_SEQ]), np.ascontiguousarray(v[:, :MAX_SEQ])
            case = f"kind={kind} kv_len={n}"
            ref = ar.decode(q, k, v, scale, n)
            S, vmax = ar.magnitude(q, k, scale, n), float(np.abs(v[:, :n]).max())
            got, img = gpu.op_attention_decode(gpu.ATTN_HEAD, q, ks, vs, scale, n - 1, image=True)
            W.add("slice", ar.worst_ratio(got, ref, S, vmax, n), case)
            head, head_img = gpu.op_attention_decode(gpu.ATTN_HEAD, q, k, v, scale, n - 1, image=True)
            if kind == "normal":
                _check_image(img, got, f"slice {case}")
            assert np.array_equal(_bits(got), _bits(head)), f"{case}: output bits differ from attn_head_kernel's"
            assert np.array_equal(_image_bits(img, q.size), _image_bits(head_img, q.size)), f"{case}: XQ image differs from attn_head_kernel's"
            again, again_img = gpu.op_attention_decode(gpu.ATTN_HEAD, q, ks, vs, scale, n - 1, image=True)
            assert np.array_equal(_bits(got), _bits(again)), f"{case}: a second call's output differs"
            assert np.array_equal(_image_bits(img, q.size), _image_bits(again_img, q.size)), f"{case}: a second call's XQ image differs"
            plain = gpu.op_attention_decode(gpu.ATTN_HEAD, q, ks, vs, scale, n - 1)
            assert np.array_equal(_bits(got), _bits(plain)), f"{case}: the output changes with the image"
    W.check()


def test_default_engine_runs_the_slice_kernel_with_the_head_kernels_bits(pkg, orc):
    """test-dense-d128 Q4_K_M, two layers, 40 tokens: a default engine (threshold 256 rows: attn_slice_kernel) gives bitwise the logits of
    an engine with attn_direct=5 (threshold 320 rows: attn_head_kernel at the same positions), and both follow the oracle within
    test_gpu_model's bound at the first and the last position."""
    n_tok = 40
    cfg = pkg.make_config("test-dense-d128", max_seq_len=64, num_layers=2)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    dflt = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    head = pkg.HipGpuInference.from_model(model, cfg.max_seq_len, attn_direct=5)
    try:
        for i in range(n_tok):
            t = (13 * i + 5) % cfg.vocab_size
            a, b = dflt.forward(t), head.forward(t)
            assert np.array_equal(_bits(a), _bits(b)), f"position {i}: the default engine's logits differ from attn_direct=5's"
            want = ref.forward([t])
            if i in (0, n_tok - 1):
                err, tol = float(np.abs(a - want).max()), 2e-3 * float(np.abs(want).max()) + 2e-3
                print(f"position {i}: max|dlogit| = {err:.3e}, tolerance {tol:.3e}")
                assert err <= tol, f"position {i}: max|dlogit| = {err:.3e} > {tol:.3e}"
    finally:
        dflt.close()
        head.close()
