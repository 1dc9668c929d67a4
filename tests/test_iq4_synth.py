"""IQ4_NL / IQ4_XS on the CPU: the float64 NumPy dequantizer that tests/test_gpu_iq4_weights.py measures the kernels against, pinned to the
reference's known-answer tests (iq_quants.rs:424-445), and the synthetic generator's two mixes."""
import numpy as np
import pytest

KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float64)   # the codebook, iq_quants.rs:16-18
BLOCK = {"IQ4_NL": (32, 18), "IQ4_XS": (256, 136)}   # elements, bytes


def dequant(tname, raw, n, k):
    """(q, s): codes 0..15 and the scale of every weight, both [n, k]; w = s * KV[q].  IQ4_NL {d f16, qs[16]}: s = d.  IQ4_XS {d f16,
    scales_h u16, scales_l[4], qs[128]}: s = d * (ls - 32), ls of sub-block ib = (scales_l[ib / 2] >> 4 (ib % 2) & 15) | (scales_h >> 2 ib
    & 3) << 4.  Sub-block of 32: elements 0..15 the low nibbles of its 16 bytes, 16..31 the high nibbles."""
    be, bb = BLOCK[tname]
    b = np.asarray(raw, np.uint8).reshape(n, k // be, bb)
    d = np.ascontiguousarray(b[..., :2]).view(np.float16)[..., 0].astype(np.float64)
    if tname == "IQ4_NL":
        s, qs = d, b[..., 2:]
    else:
        ib, sh = np.arange(8), np.ascontiguousarray(b[..., 2:4]).view(np.uint16).astype(np.int64)
        ls = ((b[..., 4 + ib // 2].astype(np.int64) >> (4 * (ib % 2))) & 15) | (((sh >> (2 * ib)) & 3) << 4)
        s, qs = (d[..., None] * (ls - 32)).reshape(n, k // 32), b[..., 8:].reshape(n, k // 32, 16)
    q = np.concatenate([qs & 15, qs >> 4], axis=-1).reshape(n, k)
    return q, np.repeat(s, 32, axis=-1)


def test_dequantizer_matches_the_reference_kats():
    """test_iq4_nl_values: entries 0, 8, 15 of the codebook; test_iq4_xs_dequantize: d 1, scales_h 0xAAAA, everything else 0 -> ls 32,
    all zeros.  And one hand-built block of each type read back element by element."""
    assert (KV[0], KV[8], KV[15]) == (-127, 1, 113)
    xs = np.zeros(136, np.uint8)
    xs[0:2], xs[2:4] = (0x00, 0x3C), (0xAA, 0xAA)
    q, s = dequant("IQ4_XS", xs, 1, 256)
    assert np.all(s == 0.0) and np.all(s * KV[q] == 0.0)
    nl = np.zeros(18, np.uint8)
    nl[0:2], nl[2], nl[17] = (0x00, 0x38), 0xF0, 0x08          # d 0.5; byte 0: elements 0 / 16 = codes 0 / 15; byte 15: elements 15 / 31 = 8 / 0
    q, s = dequant("IQ4_NL", nl, 1, 32)
    w = (s * KV[q])[0]
    assert (w[0], w[16], w[15], w[31], w[1]) == (-63.5, 56.5, 0.5, -63.5, -63.5)
    xs[2:4], xs[4], xs[8 + 16 + 3] = (0x0C, 0x00), 0x50, 0x9F  # sub-block 1: ls = 5 | 3 << 4 = 53; its byte 3: elements 3 / 19 = codes 15 / 9
    q, s = dequant("IQ4_XS", xs, 1, 256)
    w = (s * KV[q])[0]
    assert (w[32 + 3], w[32 + 19], w[32], w[0]) == (21 * 113.0, 21 * 13.0, 21 * -127.0, 32 * 127.0)


@pytest.mark.parametrize("mix", ("IQ4_NL", "IQ4_XS"))
def test_generator_mix(pkg, mix):
    """Every 2-D tensor of the mix has the type and its native byte count; the weights' RMS is that of the other formats (1 / sqrt(k))."""
    be, bb = BLOCK[mix]
    model = pkg.SynthModel(pkg.make_config("test-dense", max_seq_len=8), mix=mix)
    specs = list(model.specs())
    mats = [s for s in specs if len(s.ne) == 2]
    assert mats and all(s.ggml_type == pkg.synth.TYPE_IDS[mix] and s.nbytes == s.n_elems // be * bb for s in mats)
    assert model.weight_bytes() == sum(s.n_elems // be * bb for s in mats) + sum(4 * s.n_elems for s in specs if len(s.ne) == 1)
    k, n = 1024, 64
    raw = pkg.synth.fill_tensor("blk.0.ffn_down.weight", pkg.synth.TYPE_IDS[mix], n * k, k, 0, 3)
    q, s = dequant(mix, raw, n, k)
    assert raw.size == n * k // be * bb and set(np.unique(q)) == set(range(16))
    assert 0.9 < float(np.sqrt(np.mean((s * KV[q]) ** 2))) * np.sqrt(k) < 1.1
