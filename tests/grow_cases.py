"""Crafted frames, the NumPy restatement and the launchers for region_grow_kernel (csrc/mvosr_rescale.hip,
mvosr_region_grow_batch) — shared by tests/test_grow_cases.py (CPU) and tests/test_gpu_grow.py.  Test infrastructure.

A given-form case is a small planar triangulation with hand-set heights and angles.  The work horse is the strip: row i is
(i, i + 1, i + 2), so that rows i and i + 1 share the edge (i + 1, i + 2) and no other two rows share one — a chain of T rows,
diameter T.
"""
import ctypes as C

import numpy as np

import flat_cases as fc

THRESHOLD_ANGLE, SEED_DEG, LEVEL_DEG, HEIGHT_FACTOR = 8.0, -85.0, -80.0, 0.4      # graph.py:40,90,91,93
ST_SINGULAR, ST_MASK, ST_EMPTY = 7, 8, 9
BLOCK = 512                                                                      # kRsBlock


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _refused(T, status):
    return {"status": status, "region": np.zeros(T, bool), "label": np.full(T, -1, np.int32), "neighbors": np.full((T, 3), -1, np.int32),
            "n_region": 0, "n_flat": 0, "level": np.nan, "threshold_height": np.nan}


def numpy_grow(tri, heights, angles, n_feat=None, threshold_angle=THRESHOLD_ANGLE):
    """GraphGrow.process (graph.py:85-107) under the declared rule: edges by sorting (lo, hi) pairs, SciPy's connected
    components over the joined edges, then the largest component with a flat row (smallest row index among equals)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    h, ang = np.asarray(heights, dtype=np.float64), np.asarray(angles, dtype=np.float64)
    T = len(tri)
    if T == 0:
        return _refused(0, ST_EMPTY)
    n_feat = int(tri.max()) + 1 if n_feat is None else int(n_feat)
    twice = (tri[:, 0] == tri[:, 1]) | (tri[:, 0] == tri[:, 2]) | (tri[:, 1] == tri[:, 2])
    if (tri < 0).any() or (tri >= n_feat).any() or twice.any() or not (np.isfinite(h) & (h > 0)).all():
        return _refused(T, ST_MASK)
    e = np.sort(np.stack([tri[:, [0, 1]], tri[:, [0, 2]], tri[:, [1, 2]]], 1), axis=2).reshape(-1, 2)      # edge 3 t + e
    key = e[:, 0] * n_feat + e[:, 1]
    order = np.argsort(key, kind="stable")
    _, start, cnt = np.unique(key[order], return_index=True, return_counts=True)
    if cnt.max() > 2:
        return _refused(T, ST_MASK)
    i, j = order[start[cnt == 2]], order[start[cnt == 2] + 1]
    nb = np.full(3 * T, -1, np.int32)
    nb[i], nb[j] = j // 3, i // 3
    with np.errstate(all="ignore"):
        hinv = 1 / h                                                                                      # graph.py:88
        sub = ang < LEVEL_DEG
        level = np.median(hinv[sub]) if sub.any() else np.nan                                             # :91
        thr = HEIGHT_FACTOR * np.median(hinv)                                                             # :93
        flat = (ang < SEED_DEG) & (hinv < level)                                                          # :90-92
        ri, rj = i // 3, j // 3
        joined = (np.abs(ang[ri] - ang[rj]) < threshold_angle) & (np.abs(hinv[ri] - hinv[rj]) < thr)      # :73-77
    g = coo_matrix((np.ones(int(joined.sum())), (ri[joined], rj[joined])), shape=(T, T))
    nc, comp = connected_components(g, directed=False)
    first = np.full(nc, T)
    np.minimum.at(first, comp, np.arange(T))
    size, seeded = np.bincount(comp, minlength=nc), np.bincount(comp, weights=flat, minlength=nc) > 0
    region = np.zeros(T, bool)
    if seeded.any():
        cand = np.nonzero(seeded)[0]
        region = comp == cand[np.lexsort((first[cand], -size[cand]))[0]]
    return {"status": 0, "region": region, "label": first[comp].astype(np.int32), "neighbors": nb.reshape(T, 3),
            "n_region": int(region.sum()), "n_flat": int(flat.sum()), "level": level, "threshold_height": thr}


# ---- given-form cases ----------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, tri, h, ang, n_feat=None, note=""):
        self.name, self.note = name, note
        self.tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        self.h = np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
        self.ang = np.ascontiguousarray(ang, dtype=np.float64).reshape(-1)
        assert len(self.h) == len(self.tri) == len(self.ang), name
        self.n_feat = (int(self.tri.max()) + 1 if len(self.tri) else 0) if n_feat is None else int(n_feat)

    def expected(self):
        return numpy_grow(self.tri, self.h, self.ang, self.n_feat)

    def permuted(self, seed):
        """The same frame with its rows shuffled (and the vertices of every row rotated): (case, perm) with new row k = old perm[k]."""
        rng = np.random.default_rng(seed)
        perm = rng.permutation(len(self.tri))
        tri = np.stack([np.roll(r, rng.integers(0, 3)) for r in self.tri[perm]]) if len(perm) else self.tri
        return Case(self.name + "+shuffled", tri, self.h[perm], self.ang[perm], self.n_feat, self.note), perm


def strip(T, first_vertex=0):
    return np.arange(T)[:, None] + np.arange(3)[None, :] + first_vertex


def h_for(hinv):
    """A height whose IEEE reciprocal is exactly `hinv`."""
    h = 1.0 / hinv
    for cand in (h, np.nextafter(h, 0.0), np.nextafter(h, np.inf)):
        if 1.0 / cand == hinv:
            return cand
    raise AssertionError(hinv)


def _strip_case(T):
    """One chain: pitch -86 (a seed) with every third row at -79.5 (joined, outside the level's subset), heights in a short cycle."""
    i = np.arange(T)
    return Case("strip%d" % T, strip(T), 1.7 + 0.01 * (i % 5), np.where(i % 3 == 1, -79.5, -86.0), note="one chain of %d rows" % T)


def given_cases():
    """name -> Case.  Row counts straddle 1, 63/64/65, the block size and one case near 4000."""
    rng = np.random.default_rng(11)
    c = {}

    def add(case):
        c[case.name] = case
    add(Case("single_steep", [[0, 1, 2]], [1.7], [-90.0], note="one row below -85: its 1/height IS the level, nothing is strictly below"))
    add(Case("single_other", [[0, 1, 2]], [1.7], [-10.0], note="one row, no pitch below -80: NaN level"))
    add(Case("one_flat_of_three", strip(3), [h_for(2.0), h_for(3.0), h_for(2.5)], [-88.0, -88.0, -88.0],
             note="level 2.5, threshold 1.0: row 0 is the only seed and stays alone (|2 - 3| = 1.0 is not < 1.0)"))
    for T in (2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3990):
        add(_strip_case(T))
    for T in (65, 3990):
        add(_strip_case(T).permuted(100 + T)[0])
    add(Case("ramp7", strip(14), [2.0] + [1.9] * 13, -89.0 + 7.0 * np.arange(14), note="7 deg per step: all join, the ends differ by 91 deg"))
    add(Case("angle_exact", strip(6), [2.0, 1.9, 1.9, 1.9, 1.9, 1.9], [-90.0, -82.0, -89.5, -86.0, np.nextafter(-78.0, 0.0), -86.0],
             note="|d angle| == 8 exactly (rows 0-1, 3-4 one ulp above) does not join; 7.5 does"))
    add(Case("angle_just_inside", strip(2), [2.0, 1.9], [-90.0, np.nextafter(-82.0, -90.0)], note="|d angle| one ulp below 8: joined"))
    hv = [2.0, 3.0, 2.5, 2.5, 2.25]
    assert HEIGHT_FACTOR * np.median(hv) == 1.0 and abs(hv[0] - hv[1]) == 1.0
    add(Case("hinv_exact_odd", strip(5), [h_for(v) for v in hv], [-88.0] * 5, note="0.4 * median = 1.0 = |2 - 3|: rows 0, 1 not joined"))
    hv = [2.0, 3.0, 2.75, 2.0, 3.0, 2.25]
    assert HEIGHT_FACTOR * np.median(hv) == 1.0
    add(Case("hinv_exact_even", strip(6), [h_for(v) for v in hv], [-86.0, -86.0, -79.5, -86.0, -86.0, -86.0],
             note="even count: median (2.25 + 2.75) / 2; rows 0-1 and 3-4 differ by exactly the threshold"))
    big, small = strip(40), strip(10, first_vertex=50)
    add(Case("unseeded_larger", np.concatenate([big, small]), [1.7] * 40 + list(1.6 + 0.02 * np.arange(10)), [-70.0] * 40 + [-88.0] * 10,
             note="40 joined rows without a seed lose to 10 with one"))
    a, b = strip(8), strip(8, first_vertex=20)
    rows = np.empty((16, 3), np.int64)
    rows[0::2], rows[1::2] = b, a
    hh = np.empty(16)
    hh[0::2] = hh[1::2] = 1.6 + 0.02 * np.arange(8)
    add(Case("tie_equal", rows, hh, [-88.0] * 16, note="two seeded components of 8 rows: the one with row 0 wins"))
    add(Case("nothing_flat", strip(9), 1.6 + 0.02 * np.arange(9), [-84.0] * 9, note="a level, no pitch below -85"))
    add(Case("no_level", strip(9), 1.6 + 0.02 * np.arange(9), [-70.0] * 9, note="no pitch below -80: NaN level, nothing flat"))
    ang = np.full(21, -88.0)
    ang[10] = np.nan
    add(Case("nan_angle", strip(21), 1.6 + 0.01 * np.arange(21), ang, note="a NaN pitch in mid-chain: never joined, two components of 10"))
    from scipy.spatial import Delaunay
    gx, gz = np.meshgrid(np.arange(14.0), np.arange(12.0), indexing="ij")
    pts = np.column_stack([gx.ravel(), gz.ravel()]) + rng.uniform(-0.2, 0.2, (168, 2))
    tri = Delaunay(pts).simplices
    tri = tri[rng.uniform(size=len(tri)) > 0.35]
    add(Case("holes", tri, rng.uniform(1.5, 1.9, len(tri)), rng.uniform(-90.0, -76.0, len(tri)), n_feat=168,
             note="a triangulation with 35 % of its rows removed: holes, rows with 0 to 2 neighbours"))
    return c


def refused_cases():
    """name -> Case that mvosr_region_grow_batch refuses with MVOSR_ST_ERR_MASK (or _EMPTY: `no_rows`)."""
    good, h, ang = strip(12), 1.6 + 0.02 * np.arange(12), np.full(12, -88.0)
    c = {}
    c["three_on_edge"] = Case("three_on_edge", np.concatenate([good, [[20, 21, 22], [20, 21, 23], [21, 20, 24]]]), list(h) + [1.7] * 3, list(ang) + [-88.0] * 3)
    c["vertex_twice"] = Case("vertex_twice", np.concatenate([good, [[30, 31, 31]]]), list(h) + [1.7], list(ang) + [-88.0])
    c["id_too_large"] = Case("id_too_large", np.concatenate([good, [[3, 4, 14]]]), list(h) + [1.7], list(ang) + [-88.0], n_feat=14)
    c["id_negative"] = Case("id_negative", np.concatenate([good, [[3, -1, 5]]]), list(h) + [1.7], list(ang) + [-88.0], n_feat=14)
    for name, v in (("height_zero", 0.0), ("height_negative", -1.7), ("height_nan", np.nan), ("height_inf", np.inf)):
        hb = h.copy()
        hb[5] = v
        c[name] = Case(name, good, hb, ang)
    c["no_rows"] = Case("no_rows", np.zeros((0, 3)), [], [], n_feat=5)
    return c


# ---- real triangulations -------------------------------------------------------------------------------------------------------
def synth_rows(idx, n, base_seed=1234):
    """(xyz of the features below the vanishing row, SciPy's rows over their pixels, the Delaunay object) of a synth frame."""
    from scipy.spatial import Delaunay
    from mvoscalerecovery_amd import synth
    f3, f2 = synth.synth_frame(idx, n, base_seed=base_seed)
    low = f2[:, 1] > 185                                                                    # rescale.py:115
    d = Delaunay(f2[low])
    return np.ascontiguousarray(f3[low]), d.simplices.astype(np.int32), d


def golden_frames():
    """tests/golden/grow.npz (make_golden_grow.py: the reference's own GraphGrow.process) as a list of dicts."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grow.npz"), allow_pickle=False)
    out = []
    for i in range(int(z["n_frames"])):
        d = {k: z["f%d_%s" % (i, k)] for k in ("spec", "crc", "rows", "heights", "angles", "region", "threshold_height")}
        d["rows"] = d["rows"].astype(np.int32)
        out.append(d)
    return out


# ---- launchers (GPU) -----------------------------------------------------------------------------------------------------------
_PER_ROW = {"region": np.uint8, "label": np.int32, "neighbors": np.int32, "tri_height": np.float64, "tri_angle": np.float64}
_PER_FRAME = {"n_region": np.int32, "n_flat": np.int32, "status": np.int32, "level": np.float64, "threshold_height": np.float64}


def _launch(ctx, b, d, toff, F, hp, ap, max_tri, values, sentinel, threshold_angle):
    from mvoscalerecovery_amd import _lib
    T = max(int(toff[-1]), 1)
    spec = {k: (((T, 3) if k == "neighbors" else T), dt) for k, dt in _PER_ROW.items() if values or not k.startswith("tri_")}
    spec.update({k: (F, dt) for k, dt in _PER_FRAME.items()})
    o = fc._alloc(ctx, spec, sentinel)
    go = _lib.GrowOutputs(**{k: v.ptr for k, v in o.items()})
    gp = _lib.GrowParams(float(threshold_angle), SEED_DEG, LEVEL_DEG, HEIGHT_FACTOR)
    _lib.check(ctx.lib.mvosr_region_grow_batch(ctx.handle, C.byref(b), hp, ap, C.byref(gp), C.byref(go), int(max_tri)), "mvosr_region_grow_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + list(d))
    res = []
    for i in range(F):
        one = {k: r[k][toff[i]:toff[i + 1]] for k in spec if k in _PER_ROW}
        one.update({k: r[k][i] for k in _PER_FRAME})
        res.append(one)
    if sentinel is None:
        return res
    return res, fc._tails(r, {k: (int(toff[-1]) if k in _PER_ROW else F) for k in r})


def run_given(ctx, cases, max_feat=None, max_tri=None, sentinel=None, threshold_angle=THRESHOLD_ANGLE):
    """mvosr_region_grow_batch, given form, over `cases` as one batch -> one dict per case.  max_feat / max_tri: what the header
    and the call state (None: the largest frame's).  sentinel: as flat_cases.run_stage."""
    from mvoscalerecovery_amd import _lib
    cnt = np.array([c.n_feat for c in cases], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(c.tri) for c in cases])]).astype(np.int64)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt).reshape(-1) for x in xs] + [np.zeros(1, dt)])
    d = [ctx.to_device(off), ctx.to_device(cnt), ctx.to_device(toff), ctx.to_device(cat([c.tri for c in cases], np.int32)),
         ctx.to_device(cat([c.h for c in cases], np.float64)), ctx.to_device(cat([c.ang for c in cases], np.float64))]
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.tri2_off, b.tri2 = len(cases), d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr
    b.max_feat, b.total_feat = int(cnt.max() if max_feat is None else max_feat), int(off[-1])
    mt = int(np.max(np.diff(toff))) if max_tri is None else int(max_tri)
    return _launch(ctx, b, d, toff, len(cases), d[4].ptr, d[5].ptr, mt, False, sentinel, threshold_angle)


def run_points(ctx, frames, max_feat=None, max_tri=None, sentinel=None, threshold_angle=THRESHOLD_ANGLE):
    """The from-points form over flat_cases.Frame objects (survivors compacted on the host) -> one dict per frame, with
    tri_height and tri_angle."""
    b, d, toff, true_max_tri = fc._batch(ctx, frames, compact=True)
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    mt = true_max_tri if max_tri is None else int(max_tri)
    return _launch(ctx, b, list(d.values()), toff, len(frames), None, None, mt, True, sentinel, threshold_angle)
