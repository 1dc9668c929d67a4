"""CPU tests of the workgroup geometry of the single-sequence matrix-core mat-vec: tests/matvec_ref.py's restatement of the planner
against the planner itself (lgh_debug_mv_plan, no device), the census of geometry classes up to k = 32768 against the shape lists of
tests/test_gpu_matvec_geometry.py, and planted mistakes — on that file's own inputs, results that are wrong in the ways a geometry
goes wrong must exceed the bound its tests apply.  A condition on the chosen inputs, not a measurement."""
import numpy as np
import pytest

import matvec_multi_ref as mm
import matvec_ref as mr
import test_gpu_matvec_geometry as tg
from test_gpu_matvec import EPS

KS = [256 * j for j in range(1, 129)]
NS = (1, 16, 17, 4096, 4112, 8208, 16400, 81936, 128256, 152064)

# class -> (smallest k, other k <= 32768 that real models bring); the classes of tests/test_gpu_matvec_geometry.py
CLASSES = {
    "(1,8)": (256, ()),
    "(2,4)": (512, ()),
    "(3,2)": (768, ()),
    "(4,2)": (1024, ()),
    "(5,1)": (1280, (2560, 5120)),
    "(6,1)": (1536, (13824,)),
    "(7,1)": (1792, (3584, 7168, 8960)),
    "(8,1) even": (2048, (4096, 14336, 28672)),
    "(8,1) uneven busy": (5632, (18944,)),
    "(8,1) uneven idle1": (3328, ()),
    "(8,1) uneven idle2": (2816, (4352,)),
    "(8,1) uneven idle3": (2304, ()),
}


# ---- (a) the restatement is the planner
def test_restatement_equals_the_planner(pkg):
    hb = pkg.hip_backend
    for k in KS:
        for n in NS:
            for launch_rows in (0, n + 6144):
                p, g = hb.mv_plan(k, n, launch_rows), mr.mvq_geometry(k, n, launch_rows or None)
                want = dict(T=g["T"], G=g["G"], nbw=g["nbw"], rows_per_wg=16 * g["R"], n_wg=g["n_wg"], threads=g["threads"],
                            red_floats=g["T"] * 16 * g["R"])
                assert p == want, (k, n, launch_rows)
                # what the kernel relies on
                assert g["T"] * g["G"] <= mr.MVQ_WAVES and g["G"] & (g["G"] - 1) == 0 and g["R"] % g["G"] == 0 and g["R"] >= g["G"]
                assert 16 * g["R"] <= g["threads"] and sum(g["slices"]) == k // 256 and 1 <= g["last"] <= g["R"]
                assert (g["n_wg"] - 1) * g["R"] + g["last"] == -(-n // 16)
    with pytest.raises(pkg.BackendError) as ei:
        hb.mv_plan(896, 16)
    assert ei.value.variant == "Unsupported"
    assert [mm.k_slices(k) for k in (256, 1280, 2304, 18944)] == [(1, 1), (5, 1), (8, 2), (8, 10)]


# ---- (b) the classes, and the GPU file's shapes
def test_class_table_is_complete_and_the_gpu_lists_cover_it():
    seen = {}
    for k in KS:
        seen.setdefault(mr.mvq_class(k), []).append(k)
    assert set(seen) == set(CLASSES)
    for cls, (smallest, others) in CLASSES.items():
        assert seen[cls][0] == smallest and set(others) <= set(seen[cls]), cls
    for k in KS:     # an uneven plan: the last busy slice is short, at most three waves have no block, the idle ones are the last
        g = mr.mvq_geometry(k, 16)
        if mr.mvq_class(k).startswith("(8,1) uneven"):
            busy = [b for b in g["slices"] if b]
            assert busy[-1] < g["nbw"] and all(b == g["nbw"] for b in busy[:-1]) and g["idle"] <= 3
            assert g["slices"] == tuple(busy) + (0,) * g["idle"]
        else:
            assert g["idle"] == 0 and len(set(g["slices"])) == 1
    assert sorted(c for c, _ in tg.PLAIN) == sorted(CLASSES)
    for ci, (cls, ks) in enumerate(tg.PLAIN):
        assert ks[0] == CLASSES[cls][0] and all(mr.mvq_class(k) == cls for k in ks)
        items = tg.plain_items(ci, ks)
        assert {(t, n) for t, k, n, _, _ in items if k == ks[0]} == {(t, n) for t in mr.FUSED for n in tg.PLAIN_N}
        assert {a for t, k, n, a, _ in items if (k, n) == (ks[0], 17)} == set(mr.ACT_KINDS)
        assert all({n for _, k, n, _, _ in items if k == kk} == set(tg.PLAIN_N) for kk in ks)
    assert len({s for ci, (_, ks) in enumerate(tg.PLAIN) for s in (i[4] for i in tg.plain_items(ci, ks))}) == \
        sum(len(tg.plain_items(ci, ks)) for ci, (_, ks) in enumerate(tg.PLAIN))                       # every launch its own inputs
    # the norm prologue's gather: partial counts below 64, between, and past the 256 wave 0 loads up front
    counts = {k // 16 for _, ks in tg.PLAIN for k in ks}
    assert {32, 48, 80, 144, 320} <= counts and max(counts) > 1024
    # every format at every T; the chain, QKV and MoE shapes sit in the classes nothing ran before
    for T in range(1, 9):
        assert {t for ci, (_, ks) in enumerate(tg.PLAIN) for t, k, _, _, _ in tg.plain_items(ci, ks) if mr.mvq_geometry(k, 16)["T"] == T} == set(mr.FUSED)
    new = {"(5,1)", "(7,1)", "(8,1) uneven idle1", "(8,1) uneven idle3"}
    assert new <= {mr.mvq_class(k) for c in tg.CHAIN for k in (c[1], c[2])}
    assert {mr.mvq_class(q[0]) for q in tg.QKV} == {"(7,1)", "(5,1)", "(8,1) uneven idle1", "(3,2)", "(2,4)"}
    assert {mr.mvq_class(k) for m in tg.MOE for k in (m[3], m[4])} == {"(3,2)", "(5,1)", "(7,1)", "(8,1) uneven idle3"}
    for cls, k, n, Rg, R, n_wg, last in tg.WIDE:
        g = mr.mvq_geometry(k, n)
        assert (g["Rg"], g["R"], g["n_wg"], g["last"]) == (Rg, R, n_wg, last), cls
    wide = {w[0]: mr.mvq_geometry(w[1], w[2]) for w in tg.WIDE}
    assert any(g["Rg"] > 1 and g["G"] == 4 for g in wide.values()) and any(g["Rg"] > 1 and g["G"] == 2 for g in wide.values())
    assert any(g["Rg"] > 1 and g["T"] % 2 and g["last"] < g["R"] for g in wide.values())
    assert sum(1 for g in wide.values() if g["R"] == g["rmax"] and g["n_wg"] > mr.MVQ_CUS) == 2


# ---- (c) the widths of real models
def test_real_widths_land_on_these_classes():
    for k in (7168, 3584, 1792, 8960):                       # Llama-3 ffn_down shards, Qwen2-7B hidden, Qwen2.5-1.5B ffn
        assert mr.mvq_class(k) == "(7,1)" and mr.mvq_geometry(k, 16)["threads"] == 448
    g = mr.mvq_geometry(18944, 3584)                         # Qwen2-7B ffn_down
    assert mr.mvq_class(18944) == "(8,1) uneven busy" and g["nbw"] == 10 and g["slices"][-1] == 4
    g = mr.mvq_geometry(3584, 152064)                        # Qwen2-7B output head
    assert g["R"] == g["rmax"] == 28 and g["n_wg"] > mr.MVQ_CUS
    assert mr.mvq_class(1536) == "(6,1)" and mr.mvq_class(5120) == "(5,1)"
    g = mr.mvq_geometry(13824, 5120)                         # 13B-class ffn_down
    assert mr.mvq_class(13824) == "(6,1)" and g["nbw"] == 9 and g["threads"] == 384


# ---- (d) planted mistakes
def emulate(tname, raw, k, n, x, rows, nw=None, mistake=None):
    """The launch's result on `rows` from its float64 partial sums per (k-slice, row group): slice s sums its own blocks of the tile
    row group rg of workgroup wg owns, the epilogue adds the T partials and scales by 1 / rms from the k / 16 partial sums of x^2.
    `mistake` plants one error of the geometry."""
    g = mr.mvq_geometry(k, n)
    rows = np.asarray(rows)
    tile, tiles = rows // 16, -(-n // 16)
    src, live = rows, np.ones(rows.size, bool)
    if mistake == "rowgroup":            # row group rg streams the tiles of rg + 1
        src = rows + 16 * g["Rg"]
        live = src < n
        src = np.minimum(src, n - 1)
    elif mistake == "last_wg":           # floor instead of ceil: the last workgroup's tiles beyond a full R are skipped
        live = tile < tiles // g["R"] * g["R"]
    elif mistake == "rmax":              # one workgroup per CU, R capped: tiles past rmax * 256 are never computed
        live = tile < g["rmax"] * mr.MVQ_CUS
    a, o = mr.decode(tname, mm.take_rows(raw, n, src), k, rows.size)
    x64 = np.asarray(x, np.float64)
    v = x64 if nw is None else x64 * np.asarray(nw, np.float64)
    parts = np.zeros((g["T"], rows.size))
    for s, nb in enumerate(g["slices"]):
        b0, b1 = s * g["nbw"], s * g["nbw"] + nb
        if mistake == "short_slice" and 0 < nb < g["nbw"]:      # the short last slice loses its last block
            b1 -= 1
        parts[s] = (a - o)[:, 256 * b0:256 * b1] @ v[256 * b0:256 * b1]
        if nb == 0 and mistake == "idle_keeps":                 # an idle slice's slot keeps the slice before it
            parts[s] = parts[s - 1]
    inv = 1.0
    if nw is not None:
        ssq = (x64 * x64).reshape(-1, 16).sum(axis=1)
        if mistake == "ssq256":                                 # the partials past the 256 loaded up front are dropped
            ssq = ssq[:256]
        elif mistake == "ssq64":                                # ... or every lane's second to fourth
            ssq = ssq[:64]
        inv = 1.0 / np.sqrt(ssq.sum() / k + EPS)
    return np.where(live, parts.sum(axis=0) * inv, 0.0)


def _launches():
    """(class, format, raw, k, n, x, nw, rows) of every plain and wide launch of the GPU file."""
    for ci, (cls, ks) in enumerate(tg.PLAIN):
        for item in tg.plain_items(ci, ks):
            raw, x, nw = tg.plain_inputs(item)
            yield cls, item[0], raw, item[1], item[2], x, nw, np.arange(item[2])
    for w in tg.WIDE:
        raw, x, nw = tg.wide_inputs(w[1], w[2])
        yield w[0], tg.WIDE_FMT, raw, w[1], w[2], x, nw, tg.wide_rows(w[1], w[2])


def _applies(mistake, g, k, n, norm):
    return {"short_slice": 0 < min(b for b in g["slices"] if b) < g["nbw"], "idle_keeps": g["idle"] > 0,
            "rowgroup": g["G"] > 1, "last_wg": g["last"] < g["R"], "rmax": g["n_wg"] > mr.MVQ_CUS,
            "ssq256": norm and k // 16 > 256, "ssq64": norm and k // 16 > 64}[mistake]


MISTAKES = ("short_slice", "idle_keeps", "rowgroup", "last_wg", "rmax", "ssq256", "ssq64")


def test_every_planted_mistake_exceeds_the_bound():
    caught, missed = {m: set() for m in MISTAKES}, []
    for cls, tname, raw, k, n, x, nw, rows in _launches():
        g = mr.mvq_geometry(k, n)
        for norm in (False, True):
            todo = [m for m in MISTAKES if _applies(m, g, k, n, norm)]
            if norm and not any(m.startswith("ssq") for m in todo):
                continue                                        # (the other mistakes are the same with and without the norm)
            w = nw if norm else None
            Y, E = mm.linear(tname, raw, k, n, x[None], nw=w, rows=rows, eps=EPS)
            what = (cls, tname, k, n, norm)
            # the emulation itself is the reference, to float64 rounding
            assert mm.ratio(emulate(tname, raw, k, n, x, rows, w), Y[0], E[0]) < 1e-6, what
            for m in todo:
                if norm and not m.startswith("ssq"):
                    continue
                if mm.ratio(emulate(tname, raw, k, n, x, rows, w, m), Y[0], E[0]) > 1.0:
                    caught[m].add(cls)
                else:
                    missed.append((m,) + what)
    # Every launch of more than one row shows every mistake that applies to it.  A launch of ONE row may hide one: its bound follows
    # the chunk maxima of x, so under an "outlier" vector a single block of a single row can weigh less than the bound.
    assert all(n == 1 for _, _, _, _, n, _ in missed) and len(missed) <= 2, missed
    # every mistake was planted in every class it can occur in
    uneven = {c for c in CLASSES if "uneven" in c}
    assert {c.split(" Rg")[0].split(" R=")[0] for c in caught["short_slice"]} == uneven
    assert caught["idle_keeps"] == {c for c in uneven if "idle" in c}
    assert {"(1,8)", "(2,4)", "(3,2)", "(4,2)", "(2,4) Rg=2", "(3,2) Rg=2", "(4,2) Rg=2", "(1,8) R=rmax"} <= caught["rowgroup"]
    assert {"(2,4) Rg=2", "(5,1) Rg=2 short last", "(7,1) Rg=2 short last", "(5,1) R=rmax", "(1,8) R=rmax"} <= caught["last_wg"]
    assert caught["rmax"] == {"(5,1) R=rmax", "(1,8) R=rmax"}
    assert {"(5,1)", "(6,1)", "(7,1)", "(8,1) uneven busy"} <= caught["ssq256"]
    assert {c for c, (k0, _) in CLASSES.items() if k0 > 1024} <= caught["ssq64"]
