"""numpy restatement of the two row-wise launches of a tensor-parallel prompt block (csrc/tp_prefill.hip), shared by
test_tp_prefill_ref.py (CPU) and test_gpu_tp_prefill.py.

Every sum is f32 and sequential, one rounding per add, in the order the kernels state:
  a_r[t][i]    = ((0 + part[r][0][t][col0 + i]) + part[r][1][t][col0 + i]) + ...  (+ bias[i] on rank 0)      tp_pf_partial_kernel
  hidden[t][i] = resid[t][i] + (((a_0 + a_1) + a_2) ...)                          rank order, residual last    tp_pf_reduce_kernel
  XH[t][i]     = f16(f32(hidden[t][i] * nw[i])) at prefill_ref.xh_offset(t, i)
rank_order / split_order permute the ranks / the splits of every rank: the planted mistakes the self-test must see."""
import numpy as np

import prefill_ref as pr
import tp_ref

TOKENS = pr.TOKENS


def split_partials(kind: str, n: int, S: int, ncols: int, seed: int) -> np.ndarray:
    """[n][S][128][ncols] f32 of tp_ref.partials' kinds: 'orders' makes every regrouping of the n * S terms of an element visible."""
    flat = tp_ref.partials(kind, n * S, TOKENS * ncols, seed)
    return np.ascontiguousarray(flat.reshape(n, S, TOKENS, ncols))


def compact(part_r: np.ndarray, col0: int, H: int, m: int, bias=None, split_order=None) -> np.ndarray:
    """a_r [m][H] of one rank's split partials [S][128][ncols]."""
    S = part_r.shape[0]
    a = np.zeros((m, H), np.float32)
    for s in (range(S) if split_order is None else split_order):
        a = (a + part_r[s, :m, col0:col0 + H].astype(np.float32)).astype(np.float32)
    if bias is not None:
        a = (a + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
    return a


def hidden_ref(part: np.ndarray, col0: int, resid: np.ndarray, bias=None, rank_order=None, split_order=None) -> np.ndarray:
    """hidden [m][H] after both launches; bias belongs to rank 0."""
    n = part.shape[0]
    m, H = resid.shape
    blocks = [compact(part[r], col0, H, m, bias if r == 0 else None, split_order) for r in range(n)]
    order = list(range(n)) if rank_order is None else list(rank_order)
    s = blocks[order[0]].copy()
    for r in order[1:]:
        s = (s + blocks[r]).astype(np.float32)
    return (np.asarray(resid, np.float32) + s).astype(np.float32)


def xh_image(hidden: np.ndarray, nw, fill: int) -> np.ndarray:
    """The XH image (uint8) of f16(f32(hidden * nw)) for hidden [m][H]: every f16 slot the m tokens own, everything else `fill`."""
    m, H = hidden.shape
    img = np.full((H + 255) // 256 * TOKENS * 256 * 2, fill, np.uint8)
    if nw is None:
        return img
    v = (np.asarray(hidden, np.float32) * np.asarray(nw, np.float32)[None, :]).astype(np.float32)
    with np.errstate(over="ignore"):
        h16 = v.astype(np.float16)
    off = pr.xh_offset(np.arange(m)[:, None], np.arange(H)[None, :])
    img.view(np.uint16)[off] = h16.view(np.uint16)
    return img
