"""Crafted frames, the NumPy restatement and the launcher for tri_graph_kernel (csrc/mvosr_trigraph.hip, mvosr_tri_graph_batch)
— shared by tests/test_trigraph_cases.py (CPU) and tests/test_gpu_trigraph.py.  Test infrastructure.

The restatement follows /root/reference/src/scale_calculator.py:177-222.  ``region_graph`` walks triangle2region_graph's rule
(:56-81) with a dictionary; ``neighbors_table`` is the closed form the device builds (lower-index neighbours in the row's own
edge-slot order, then higher-index ones ascending).  ``sequential`` is the reference's loop over the flat rows; ``scheduled`` is
what the device does — rounds that finish every flat row whose flat lower-index neighbours are final.  Both use ``update``, whose
two dot products are written with an EXACT fused multiply-add (``fma``, through ``fractions``) in the association of the strided
ddot NumPy's ``@`` reaches for these operands — never ``@`` itself.
"""
import ctypes as C
import os
import warnings
from fractions import Fraction

import numpy as np

ST_SINGULAR, ST_MASK, ST_EMPTY = 7, 8, 9
BLOCK = 512                                                                      # kTgBlock
THR = -80.0                                                                      # scale_calculator.py:190
OBS = np.array([[0.33, 0.33, 0.33], [0.03, 0.07, 0.90], [0.90, 0.07, 0.03], [0.05, 0.9, 0.05]])      # :193
LDS_LIMIT = 163840


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """a * b + c rounded once (IEEE fusedMultiplyAdd) for Python floats."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))          # (a NaN or an infinity: no rounding to fuse)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def edge_slots(row):
    a, b, c = (int(x) for x in row)
    return (a, b), (a, c), (b, c)                                                # :66, :70, :74


def region_graph(tris):
    """triangle2region_graph (:56-81) as a dictionary walk: graph[i] in the reference's list order."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    seen, graph = {}, [[] for _ in range(len(tris))]
    for i, row in enumerate(tris):
        keys = [(min(p, q), max(p, q)) for p, q in edge_slots(row)]
        for k in keys:
            if k in seen:                                                        # (an edge on two rows at most: one earlier row)
                graph[i].append(seen[k][0])
                graph[seen[k][0]].append(i)
        for k in keys:
            seen.setdefault(k, []).append(i)
    return graph


def neighbors_table(tris):
    """(T, 3) int32, -1 padded: per row the row across (ab, ac, bc), the lower-index ones first in slot order, then the
    higher-index ones ascending — what the device stores and mvosr_trigraph_outputs.neighbors returns."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    rows_of = {}
    for i, row in enumerate(tris):
        for p, q in edge_slots(row):
            rows_of.setdefault((min(p, q), max(p, q)), []).append(i)
    out = np.full((len(tris), 3), -1, np.int32)
    for i, row in enumerate(tris):
        across = [[r for r in rows_of[(min(p, q), max(p, q))] if r != i] for p, q in edge_slots(row)]
        lower = [r[0] for r in across if len(r) == 1 and r[0] < i]
        higher = sorted(r[0] for r in across if len(r) == 1 and r[0] > i)
        lst = lower + higher
        out[i, :len(lst)] = lst
    return out


def refused(tris, n_feat):
    """An id outside [0, n_feat), a vertex twice in a row, an edge on more than two rows."""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0:
        return False
    if (t < 0).any() or (t >= n_feat).any() or ((t[:, 0] == t[:, 1]) | (t[:, 0] == t[:, 2]) | (t[:, 1] == t[:, 2])).any():
        return True
    s = np.sort(t, axis=1)
    e = np.concatenate([s[:, [0, 1]], s[:, [0, 2]], s[:, [1, 2]]])
    _, counts = np.unique(e[:, 0] * (int(t.max()) + 1) + e[:, 1], return_counts=True)
    return bool((counts > 2).any())


def initial(pitch):
    with np.errstate(all="ignore"):
        p = (-70 - np.asarray(pitch, dtype=np.float64)) / 20 - 0.2               # :188
        p[p < 0] = 0                                                             # :189
    return p


def compare(a, b, threshold=0.1):
    with np.errstate(all="ignore"):
        d = np.float64(a) - np.float64(b)                                        # :169-175
    return -1 if d < -threshold else (1 if d > threshold else 0)


def dots(o, m, form="blas"):
    """(num, den) = (o[2:4] @ m[2:4], o @ m) in a stated association.  "blas": the declared rule."""
    o0, o1, o2, o3 = (np.float64(x) for x in o)
    m0, m1, m2, m3 = (np.float64(x) for x in m)
    with np.errstate(all="ignore"):
        if form == "blas":
            return np.float64(fma(o3, m3, o2 * m2)), np.float64(fma(o0, m0, o2 * m2)) + np.float64(fma(o1, m1, o3 * m3))
        if form == "left_to_right":
            return o2 * m2 + o3 * m3, ((o0 * m0 + o1 * m1) + o2 * m2) + o3 * m3
        if form == "chained_fma":
            return np.float64(fma(o3, m3, o2 * m2)), np.float64(fma(o3, m3, fma(o2, m2, fma(o1, m1, o0 * m0))))
        if form == "pairwise":
            return o2 * m2 + o3 * m3, (o0 * m0 + o1 * m1) + (o2 * m2 + o3 * m3)
    raise ValueError(form)


def update(pa, ha, pc, hc, form="blas"):
    """One neighbour's update (:206-210)."""
    pa, pc = np.float64(pa), np.float64(pc)
    with np.errstate(all="ignore"):
        m = ((1 - pa) * (1 - pc), (1 - pa) * pc, pa * (1 - pc), pa * pc)         # :209
        num, den = dots(OBS[:, compare(hc, ha) + 1], m, form)
        return num / den                                                         # :210


def sequential(graph, heights, pitch, order="list", higher="initial", form="blas"):
    """p_road (T,) by the reference's loop (:194-213).  order="ascending" (a row's neighbours by ascending index) and
    higher="final" (a flat higher-index neighbour read at the value the correct run ends it with) are NOT the reference: they
    are the two mistakes the crafted flip cases tell apart."""
    h, pitch = np.asarray(heights, dtype=np.float64), np.asarray(pitch, dtype=np.float64)
    p0 = initial(pitch)
    p = p0.copy()
    flat = pitch < THR
    final = sequential(graph, h, pitch, order) if higher == "final" else None
    for v in np.nonzero(flat)[0]:
        pa = p[v]
        for u in (sorted(graph[v]) if order == "ascending" else graph[v]):
            pc = final[u] if (final is not None and u > v and flat[u]) else p[u]
            pa = update(pa, h[v], pc, h[u], form)
        p[v] = pa
    return p


def scheduled(graph, heights, pitch):
    """-> (p_road, rounds, widest round): every round finishes the flat rows whose flat lower-index neighbours are final;
    initial and final values are kept apart."""
    h, pitch = np.asarray(heights, dtype=np.float64), np.asarray(pitch, dtype=np.float64)
    p0 = initial(pitch)
    p1 = p0.copy()
    flat = pitch < THR
    lvl = np.zeros(len(h), np.int64)
    todo = [int(v) for v in np.nonzero(flat)[0]]
    rounds, widest = 0, 0
    while todo:
        ready = [v for v in todo if all(0 < lvl[u] <= rounds for u in graph[v] if u < v and flat[u])]
        assert ready and ready[0] == todo[0]                                     # progress: the lowest open row is always ready
        for v in ready:
            pa = p0[v]
            for u in graph[v]:
                pa = update(pa, h[v], p1[u] if (u < v and flat[u]) else p0[u], h[u])
            p1[v] = pa
        for v in ready:
            lvl[v] = rounds + 1
        done = set(ready)
        todo = [v for v in todo if v not in done]
        rounds, widest = rounds + 1, max(widest, len(ready))
    return p1, rounds, widest


def height_level(heights, pitch):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.float64(np.mean(np.asarray(heights, dtype=np.float64)[np.asarray(pitch, dtype=np.float64) >= THR]))   # :216


# ---- crafted cases -------------------------------------------------------------------------------------------------------------
class Case:
    """One frame: rows ``tri`` over ``n_feat`` features, per row a mean height and a pitch in degrees (the given form);
    ``points`` (n_feat, 3), already remapped: the from-points form's input."""

    def __init__(self, name, tri, heights, pitch, n_feat=None, points=None, note=""):
        self.name, self.note = name, note
        self.tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        self.heights = np.ascontiguousarray(heights, dtype=np.float64).reshape(-1)
        self.pitch = np.ascontiguousarray(pitch, dtype=np.float64).reshape(-1)
        assert len(self.heights) == len(self.pitch) == len(self.tri), name
        if n_feat is None:
            n_feat = len(points) if points is not None else (int(self.tri.max()) + 1 if len(self.tri) else 3)
        self.n_feat = int(n_feat)
        self.points = None if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)

    def refused(self):
        return refused(self.tri, self.n_feat)

    def expected(self, **variant):
        T = len(self.tri)
        none = {"p_road": None, "p_initial": None, "neighbors": None, "valid": np.zeros(T, np.uint8), "selected": np.zeros(self.n_feat, np.uint8),
                "height_level": np.float64(np.nan), "n_flat": 0, "n_valid": 0, "n_rounds": 0}
        if T == 0:
            return dict(none, status=ST_EMPTY)
        if self.refused():
            return dict(none, status=ST_MASK)
        graph = region_graph(self.tri)
        if variant:
            p, rounds = sequential(graph, self.heights, self.pitch, **variant), -1
        else:
            p, rounds, _ = scheduled(graph, self.heights, self.pitch)
        with np.errstate(all="ignore"):
            valid = p > 0.5                                                      # :219
        sel = np.zeros(self.n_feat, np.uint8)
        sel[np.unique(self.tri[valid].reshape(-1))] = 1                          # :221
        return {"status": 0, "p_road": p, "p_initial": initial(self.pitch), "valid": valid.astype(np.uint8), "selected": sel,
                "neighbors": neighbors_table(self.tri), "height_level": height_level(self.heights, self.pitch),
                "n_flat": int((self.pitch < THR).sum()), "n_valid": int(valid.sum()), "n_rounds": rounds}


def strip(T, first_vertex=0):
    return np.arange(T)[:, None] + np.arange(3)[None, :] + first_vertex


def _values(rng, T, flat=0.6):
    """Heights around a road level with steps across the 0.1 threshold, pitches on both sides of -80."""
    h = 1.6 + 0.15 * rng.integers(-2, 3, T) + 0.01 * rng.standard_normal(T)
    pitch = np.where(rng.uniform(size=T) < flat, rng.uniform(-90.0, -80.5, T), rng.uniform(-79.5, -20.0, T))
    return h, pitch


def _delaunay(rng, n):
    from scipy.spatial import Delaunay
    return Delaunay(np.column_stack([rng.uniform(0.0, 1200.0, n), rng.uniform(190.0, 370.0, n)])).simplices.astype(np.int32)


# Two seven-row frames, found by search, in which one named mistake flips a `valid` bit (tests/test_trigraph_cases.py proves
# both flips on the restatement).
# ORDER: row 2 = (0, 1, 2) meets row 1 across ab and row 0 across ac, so graph[2] = [1, 0].  The update is a likelihood-ratio
# product, commutative in exact arithmetic: the order shows in the last bits only, so row 2's pitch was placed (bisection, then
# steps of one ulp) where the list order ends at 0.5 + 1 ulp — valid — and the ascending order at 0.5 - 1 ulp.
ORDER_CASE, HIGHER_CASE = "list_order_flip", "higher_initial_flip"
ORDER_ROWS = [[0, 2, 3], [0, 1, 4], [0, 1, 2], [2, 3, 5], [3, 5, 6], [5, 6, 7], [1, 4, 8]]
ORDER_HEIGHTS = [1.4, 1.6, 1.6, 1.5, 1.7, 1.6, 1.8]
ORDER_PITCH = [-78.13, -74.57, -85.20654666111878, -60.0, -75.0, -50.0, -79.0]
# HIGHER: row 1 is flat and reads its flat higher-index neighbour, row 6, before row 6's own turn: at 6's initial value row 1
# is valid, at 6's final value it is not (both ends more than 0.01 from 0.5).
HIGHER_ROWS = [[1, 6, 2], [5, 6, 3], [4, 1, 2], [1, 0, 3], [1, 4, 0], [0, 4, 2], [6, 1, 3]]
HIGHER_HEIGHTS = [1.801, 1.596, 1.408, 1.8, 1.6, 1.38, 1.586]
HIGHER_PITCH = [-83.95, -83.07, -84.9, -80.37, -80.77, -79.98, -86.36]


def crafted_cases():
    """name -> Case the launch accepts (status 0), given form."""
    rng = np.random.default_rng(2025)
    c = {}

    def add(case):
        assert case.name not in c and len(case.tri) <= 2 * case.n_feat, case.name      # (alone, max_tri is 2 n_feat)
        c[case.name] = case
    add(Case("one_row", [[2, 0, 1]], [1.7], [-85.0], note="a flat row without neighbours keeps its initial probability: 0.55, valid"))
    h, p = _values(rng, 1500, flat=1.0)
    add(Case("strip1500", strip(1500), h, p, note="all flat, numbered along its length: one row per round, 1500 rounds — there is no cap"))
    perm = rng.permutation(1502)
    order = rng.permutation(1500)
    add(Case("strip1500_shuffled", perm[strip(1500)][order], h[order], p[order], note="the same strip, rows and vertex ids shuffled"))
    for T in (63, 64, 65, BLOCK, BLOCK + 1):
        h, p = _values(rng, T)
        add(Case("strip%d" % T, strip(T), h, p))
    add(Case(ORDER_CASE, ORDER_ROWS, ORDER_HEIGHTS, ORDER_PITCH, note="neighbours by ascending index instead of list order flip a valid bit"))
    add(Case(HIGHER_CASE, HIGHER_ROWS, HIGHER_HEIGHTS, HIGHER_PITCH, note="a higher flat neighbour's final value instead of its initial one flips a valid bit"))
    # heights 0.1 and one ulp either side of it above and below the middle row's (compare is strict on both sides)
    base = 1.5
    up, dn = base + 0.1, base - 0.1
    hs = [base, up, np.nextafter(up, 9.0), np.nextafter(up, 0.0), base, dn, np.nextafter(dn, 0.0), np.nextafter(dn, 9.0), base]
    add(Case("threshold_steps", strip(9), hs, np.full(9, -84.0), note="height differences of exactly +-0.1 and one ulp either side"))
    tri = _delaunay(rng, 60)
    h, p = _values(rng, len(tri), flat=0.0)
    add(Case("no_flat_row", tri, h, p, n_feat=60, note="nothing flat: no round, every row keeps its initial probability (< 0.5), nothing selected"))
    h, p = _values(rng, len(tri), flat=1.0)
    add(Case("only_flat_rows", tri, h, p, n_feat=60, note="nothing steep: height_level is np.mean of nothing, NaN"))
    tri = _delaunay(rng, 80)
    h, p = _values(rng, len(tri))
    h[[3, 17, 40]], p[[5, 17, 41, 77]] = np.nan, np.nan
    h[9], h[12] = np.inf, -np.inf
    add(Case("nan_inputs", tri, h, p, n_feat=80, note="NaN heights (compare: equal) and NaN pitch (never flat, never steep, never valid)"))
    tri = np.concatenate([strip(5), strip(4, 20)])
    h, p = _values(rng, 9, flat=1.0)
    add(Case("two_components", tri, h, p, n_feat=30, note="two strips and features no row names"))
    tri = _delaunay(rng, 700)
    h, p = _values(rng, len(tri))
    add(Case("mesh700", tri, h, p, n_feat=700, note="an ordinary triangulation, more rows than threads"))
    return c


def refused_cases():
    """name -> Case that mvosr_tri_graph_batch refuses with MVOSR_ST_ERR_MASK."""
    rng = np.random.default_rng(78)
    good = strip(12)

    def case(name, tri, n_feat=16):
        h, p = _values(rng, len(tri))
        return Case(name, tri, h, p, n_feat=n_feat)
    return {"vertex_twice": case("vertex_twice", np.concatenate([good, [[13, 14, 14]]])),
            "id_too_large": case("id_too_large", np.concatenate([good[:6], [[3, 4, 16]], good[6:]])),
            "id_negative": case("id_negative", np.concatenate([[[3, -1, 5]], good])),
            "edge_on_three_rows": case("edge_on_three_rows", np.concatenate([good, [[0, 1, 15]], [[1, 0, 14]]]))}


# ---- real frames ---------------------------------------------------------------------------------------------------------------
GOLDEN_SIZES = (120, 300, 600, 2000)


def synth_survivors(idx, n, **kw):
    """(remapped feature3d of the survivors, their feature2d, SciPy's second triangulation) of synth_frame(idx, n): what
    feature_selection hands the selection at :273."""
    from mvoscalerecovery_amd import synth
    from oracle import scale_oracle as so
    f3, f2 = synth.synth_frame(idx, n, **kw)
    r3, low = so.remap(f3), so.lower_mask(f2)
    l3, l2 = r3[low], f2[low]
    valid = so.votes_valid(so.outlier_votes(l2[:, 1], l3[:, 2], so.delaunay(l2)))
    s3, s2 = np.ascontiguousarray(l3[valid]), np.ascontiguousarray(l2[valid])
    return s3, s2, so.delaunay(s2).astype(np.int32)


def sequence_frames():
    """The 36 frames of the sequence golden (the reliability golden's)."""
    import reliability_cases as rc
    return rc.sequence_frames()


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trigraph.npz"), allow_pickle=False)


# ---- launcher (GPU) ------------------------------------------------------------------------------------------------------------
ROW_OUT = {"p_road": np.float64, "p_initial": np.float64, "valid": np.uint8, "neighbors": np.int32, "tri_height": np.float64,
           "tri_pitch_deg": np.float64}
FRAME_OUT = {"height_level": np.float64, "n_flat": np.int32, "n_valid": np.int32, "n_rounds": np.int32, "status": np.int32}


def run_cases(ctx, cases, form="given", max_feat=None, sentinel=None, camera_pitch=0.0, outputs=None):
    """mvosr_tri_graph_batch over `cases` as ONE batch -> one dict per case.  form: "given" (heights and pitch per row) or
    "points" (from the cases' points).  max_feat: what the header states (None: the largest frame's).  sentinel: every output
    byte is pre-set to it and each buffer has a guard element -> (results, guards).  outputs: names to ask for (None: all)."""
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.engine import make_params
    import flat_cases as fc
    cnt = np.array([c.n_feat for c in cases], dtype=np.int32)
    padded = (cnt.astype(np.int64) + 1) & ~np.int64(1)
    off = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(c.tri) for c in cases])]).astype(np.int64)
    total, T = max(int(off[-1]), 2), max(int(toff[-1]), 1)

    def plane(k):
        a = np.zeros(total)
        for c, o in zip(cases, off):
            if c.points is not None:
                a[o:o + c.n_feat] = c.points[:, k]
        return a
    tri = np.concatenate([c.tri.reshape(-1) for c in cases] + [np.zeros(3, np.int32)]).astype(np.int32)
    d = [ctx.to_device(off[:-1].copy()), ctx.to_device(cnt), ctx.to_device(toff), ctx.to_device(tri)]
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.tri2_off, b.tri2 = len(cases), d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr
    b.max_feat, b.total_feat = int(cnt.max() if max_feat is None else max_feat), total
    h_in = p_in = None
    if form == "points":
        d += [ctx.to_device(plane(k)) for k in range(3)]
        b.x, b.y, b.z = d[4].ptr, d[5].ptr, d[6].ptr
    else:
        d += [ctx.to_device(np.concatenate([c.heights for c in cases] + [np.zeros(1)])),
              ctx.to_device(np.concatenate([c.pitch for c in cases] + [np.zeros(1)]))]
        h_in, p_in = d[4].ptr, d[5].ptr
    spec = {k: ((T, 3) if k == "neighbors" else T, dt) for k, dt in ROW_OUT.items()}
    spec["selected"] = (total, np.uint8)
    spec.update({k: (len(cases), dt) for k, dt in FRAME_OUT.items()})
    if outputs is not None:
        spec = {k: v for k, v in spec.items() if k in outputs or k in ("status", "selected", "height_level")}
    o = fc._alloc(ctx, spec, sentinel)
    out = _lib.TriGraphOutputs(**{k: v.ptr for k, v in o.items()})
    p = make_params(1.75, camera_pitch=float(camera_pitch))
    try:
        _lib.check(ctx.lib.mvosr_tri_graph_batch(ctx.handle, C.byref(p), C.byref(b), h_in, p_in, C.byref(out)), "mvosr_tri_graph_batch")
        ctx.sync()
        r = {k: v.download() for k, v in o.items()}
    finally:
        fc._free(list(o.values()) + d)
    res = []
    for i in range(len(cases)):
        one = {k: r[k][toff[i]:toff[i + 1]] for k in ROW_OUT if k in r}
        one["selected"] = r["selected"][off[i]:off[i] + cnt[i]]
        one.update({k: r[k][i] for k in FRAME_OUT if k in r})
        one["status"] = int(one["status"])
        res.append(one)
    if sentinel is None:
        return res
    lead = {k: (T if k in ROW_OUT else total if k == "selected" else len(cases)) for k in r}
    return res, fc._tails(r, lead)
