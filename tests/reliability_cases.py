"""Crafted frames, the NumPy restatement and the launcher for reliability_kernel (csrc/mvosr_reliability.hip,
mvosr_reliability_batch) — shared by tests/test_reliability_cases.py (CPU) and tests/test_gpu_reliability.py.  Test infrastructure.

The restatement has two forms.  ``sequential``: the edge list in the reference's order — (lower end i, first row that names both
ends, upper end j), /root/reference/src/scale_calculator.py:86-99,130-131 — and the loop over it, one edge at a time.
``scheduled``: what the device does — per vertex the list of its edges in the order the loop meets them, and rounds in which every
edge that is next at both its ends is applied.  Both must give the same bits.
"""
import ctypes as C
import os

import numpy as np

ST_MASK = 8
BLOCK = 512                                                                      # kRelBlock
START = 0.8                                                                      # scale_calculator.py:129


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def edges_in_order(tris, n, block_order="first_seen"):
    """(E, 3) int64 rows (i, j, first row), i < j, in the order the reference's loop meets them.  ``block_order="ascending_j"`` is
    NOT the reference's order (a vertex's own edges by ascending neighbour instead of first seen): for the test that shows the
    order matters."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if len(tris) == 0:
        return np.zeros((0, 3), np.int64)
    s = np.sort(tris, axis=1)                                                    # :92
    rows = np.arange(len(tris))
    e = np.concatenate([np.stack([s[:, 0], s[:, 1], rows], 1), np.stack([s[:, 0], s[:, 2], rows], 1), np.stack([s[:, 1], s[:, 2], rows], 1)])
    key = e[:, 0] * max(int(n), 1) + e[:, 1]
    order = np.lexsort((e[:, 2], key))
    e, key = e[order], key[order]
    first = np.ones(len(e), bool)
    first[1:] = key[1:] != key[:-1]
    e = e[first]                                                                 # one entry per edge, with its smallest row
    if block_order == "ascending_j":
        return e[np.lexsort((e[:, 1], e[:, 0]))]
    # (the two edges a row gives its s0, (s0, s1) then (s0, s2): s1 < s2, so j ascending breaks the tie as :93-96 do)
    return e[np.lexsort((e[:, 1], e[:, 2], e[:, 0]))]


def _update(ri, rj, abnormal):
    """scale_calculator.py:132-143 for arrays of edges: every operation a NumPy operation of its own."""
    with np.errstate(all="ignore"):
        a = ri * rj
        b = (1 - ri) * rj
        c = (1 - rj) * ri
        d = (1 - ri) * (1 - rj)
        ni = np.where(abnormal, (0.25 * c) / (0.25 * (b + c) + 0.5 * d), (a + 0.25 * c) / (a + 0.25 * (b + c) + 0.5 * d))
        nj = np.where(abnormal, (0.25 * b) / (0.25 * (b + c) + 0.5 * d), (a + 0.25 * b) / (a + 0.25 * (b + c) + 0.5 * d))
    return ni, nj


def _abnormal(z, v, i, j):
    with np.errstate(all="ignore"):
        return (v[i] - v[j]) * (z[i] - z[j]) > 0                                 # :122 — the product; 0 and NaN are "normal"


def sequential(tris, z, v, n, block_order="first_seen"):
    """Reliabilities (n,) by the reference's loop over the ordered edge list."""
    z, v = np.asarray(z, dtype=np.float64), np.asarray(v, dtype=np.float64)
    r = START * np.ones(int(n))
    for i, j, _ in edges_in_order(tris, n, block_order):
        ni, nj = _update(r[i:i + 1], r[j:j + 1], _abnormal(z, v, i, j))
        r[i], r[j] = ni[0], nj[0]
    return r


def incidence_lists(E, n):
    """Per vertex the positions (into E) of its edges in the order the loop meets them: as the upper end by ascending lower end,
    then its own block in list order — i.e. E's own order restricted to the vertex.  -> (start[n + 1], flat positions)."""
    ends = np.concatenate([E[:, 0], E[:, 1]])
    pos = np.concatenate([np.arange(len(E)), np.arange(len(E))])
    order = np.lexsort((pos, ends))
    start = np.zeros(int(n) + 1, np.int64)
    np.add.at(start, ends + 1, 1)
    return np.cumsum(start), pos[order]


def scheduled(tris, z, v, n):
    """-> (reliabilities, rounds, widest round): every round applies the edges that are next at both their ends."""
    z, v = np.asarray(z, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n = int(n)
    E = edges_in_order(tris, n)
    r = START * np.ones(n)
    if len(E) == 0:
        return r, 0, 0
    start, inc = incidence_lists(E, n)
    ptr = start[:-1].copy()
    abn = _abnormal(z, v, E[:, 0], E[:, 1])
    done, rounds, widest = 0, 0, 0
    while done < len(E):
        live = np.nonzero(ptr < start[1:])[0]
        nxt = inc[ptr[live]]
        own = E[nxt, 0] == live                                                  # the edge's lower end decides
        k, i = nxt[own], live[own]
        j = E[k, 1]
        ready = (ptr[j] < start[j + 1]) & (inc[np.minimum(ptr[j], len(inc) - 1)] == k)
        k, i, j = k[ready], i[ready], j[ready]
        assert len(k) > 0 and len(np.unique(np.concatenate([i, j]))) == 2 * len(k)      # progress; no vertex twice in a round
        r[i], r[j] = _update(r[i], r[j], abn[k])
        ptr[i] += 1
        ptr[j] += 1
        done, rounds, widest = done + len(k), rounds + 1, max(widest, len(k))
    return r, rounds, widest


# ---- crafted cases -------------------------------------------------------------------------------------------------------------
class Case:
    """One frame: rows ``tri`` over ``n_feat`` features with raw depth ``z``, height ``y`` and pixel row ``v``; ``pitch``: the
    engine's camera pitch (the kernel remaps z at load)."""

    def __init__(self, name, tri, z, v, n_feat=None, y=None, pitch=0.0, note=""):
        self.name, self.note, self.pitch = name, note, float(pitch)
        self.tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        self.z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
        self.v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        self.n_feat = len(self.z) if n_feat is None else int(n_feat)
        assert len(self.z) == len(self.v) == self.n_feat, name
        self.y = 0.5 + 0.125 * (np.arange(self.n_feat) % 7) if y is None else np.ascontiguousarray(y, dtype=np.float64).reshape(-1)

    def remapped_z(self):
        """scale_calculator.py:392 with the doubles engine.make_params hands the kernel."""
        return self.y * float(np.sin(self.pitch)) + self.z * float(np.cos(self.pitch))

    def refused(self):
        t = self.tri.astype(np.int64)
        twice = (t[:, 0] == t[:, 1]) | (t[:, 0] == t[:, 2]) | (t[:, 1] == t[:, 2])
        return bool(len(t) and ((t < 0).any() or (t >= self.n_feat).any() or twice.any()))

    def expected(self, block_order="first_seen"):
        """{"status", "keep" (int32: 0 survives, -1 not), "reliability" (None where the frame is refused)}."""
        if self.refused():
            return {"status": ST_MASK, "keep": np.full(self.n_feat, -1, np.int32), "reliability": None}
        r = sequential(self.tri, self.remapped_z(), self.v, self.n_feat, block_order)
        return {"status": 0, "keep": np.where(r > START, 0, -1).astype(np.int32), "reliability": r}


def strip(T, first_vertex=0):
    return np.arange(T)[:, None] + np.arange(3)[None, :] + first_vertex


def _depth_rows(rng, n, wrong=0.2):
    """Pixel rows and depths that mostly disagree in sign across an edge (nearer is lower in the image), `wrong` of them off."""
    v = rng.uniform(200.0, 370.0, n)
    z = 400.0 / (v - 180.0) * np.where(rng.uniform(size=n) < wrong, rng.uniform(0.3, 3.0, n), 1.0)
    return z, v


def _delaunay(rng, n):
    from scipy.spatial import Delaunay
    u = rng.uniform(0.0, 1200.0, n)
    z, v = _depth_rows(rng, n)
    return Delaunay(np.column_stack([u, v])).simplices, z, v


ORDER_CASE = "first_seen_order"


def crafted_cases():
    """name -> Case the launch accepts (status 0)."""
    rng = np.random.default_rng(2024)
    c = {}

    def add(case):
        assert case.name not in c and len(case.tri) <= 2 * case.n_feat, case.name      # (alone, max_tri is 2 n_feat)
        c[case.name] = case
    add(Case("one_triangle", [[2, 0, 1]], [5.0, 4.0, 6.0], [300.0, 310.0, 290.0], note="three edges, three rounds"))
    z, v = _depth_rows(rng, 7)
    add(Case("unnamed_vertices", [[0, 1, 2], [1, 2, 4]], z, v, note="vertex 3 is in no row, 5 and 6 lie above the largest id: exactly 0.8, rejected"))
    for k in (5, 70):
        z, v = _depth_rows(rng, k + 1)
        rim = np.arange(1, k)
        add(Case("fan_low_hub%d" % k, np.column_stack([np.zeros(k - 1, int), rim, rim + 1]), z, v, note="hub 0: its own block is the whole fan"))
        rim = np.arange(0, k - 1)
        add(Case("fan_high_hub%d" % k, np.column_stack([rim + 1, np.full(k - 1, k), rim]), z, v, note="hub k: every hub edge comes from the upper part"))
    z, v = _depth_rows(rng, 1502)
    add(Case("strip1500", strip(1500), z, v, note="numbered along its length: one edge per round, 3001 rounds — there is no cap"))
    perm = rng.permutation(1502)
    add(Case("strip1500_shuffled", perm[strip(1500)], z, v, note="the same strip under shuffled vertex ids"))
    for T in (63, 64, 65, BLOCK, BLOCK + 1):
        z, v = _depth_rows(rng, T + 2)
        add(Case("strip%d" % T, strip(T), z, v))
    # vertex 0 first meets 5 and 6, then 1 and 2: graph[0] = [5, 6, 1, 2, 3, 4] (found by search: the ascending-j order
    # changes the mask; tests/test_reliability_cases.py asserts that it does)
    rows = [[0, 5, 6], [0, 1, 2], [0, 3, 4], [1, 2, 3], [3, 4, 5], [5, 6, 1], [2, 4, 6]]
    add(Case(ORDER_CASE, rows, *_order_values(), note="first-seen order differs from ascending j, and the mask depends on it"))
    tri, z, v = _delaunay(rng, 40)
    add(Case("edge_on_three_rows", np.concatenate([[[0, 1, 41], [1, 0, 40], [40, 41, 0]], tri, [[0, 1, 42], [42, 1, 0]]]),
             np.concatenate([z, [3.0, 4.0, 5.0]]), np.concatenate([v, [300.0, 280.0, 310.0]]),
             note="(0, 1) on four rows, two of them after the triangulation that may name it too: its first row is row 0"))
    k, rim = 60, np.arange(60)
    zz, vv = np.full(k + 3, 5.0), np.full(k + 3, 300.0)
    zz[k:], vv[k:] = [3.0, 4.0, 4.5], [310.0, 320.0, 330.0]                      # normal against the rim, abnormal among themselves
    add(Case("saturated_nan", np.concatenate([np.column_stack([rim, np.full(k, k + 1), np.full(k, k)]),
                                              np.column_stack([np.full(k, k + 2), rim, np.full(k, k + 1)])]), zz, vv,
             note="three hubs on the highest ids, driven to 1 - ulp, 1.0 and 1.0 by 60 normal edges each; the hubs' own edges, each on 60 "
                  "rows, come last and are abnormal: (k, k + 1) ends at exactly 0.0 and 1.0, (k + 1, k + 2) is 0/0 — NaN, kept and rejected"))
    tri, z, v = _delaunay(rng, 30)
    v = 1e-200 * rng.integers(-5, 6, 30)
    z = 5.0e-200 * rng.integers(1, 9, 30)
    add(Case("underflow", tri, z, v, note="differences of 1e-200: every product underflows to 0 — normal, whatever the signs say"))
    tri, z, v = _delaunay(rng, 60)
    z[[3, 17]], z[[5, 29, 41]], z[[8, 30]] = np.nan, np.inf, -np.inf
    v[[29, 30]] = v[5]                                                           # inf * 0
    add(Case("nonfinite_depth", tri, z, v, note="NaN, +inf and -inf depths; inf - inf and inf * 0 are NaN: normal"))
    z, v = _depth_rows(rng, 5)
    add(Case("no_rows", np.zeros((0, 3)), z, v, note="every reliability 0.8, every keep -1, status 0"))
    tri, z, v = _delaunay(rng, 150)
    add(Case("pitched", tri, z, v, y=rng.uniform(0.5, 2.0, 150), pitch=0.05, note="a camera pitch: z is remapped at load"))
    tri, z, v = _delaunay(rng, 700)
    add(Case("mesh700", tri, z, v, y=rng.uniform(0.5, 2.0, 700), note="an ordinary triangulation, more features than threads"))
    return c


def _order_values():
    """(z, v) of the ORDER_CASE: drawn from a fixed seed chosen so that the two block orders give different masks."""
    rng = np.random.default_rng(ORDER_SEED)
    return _depth_rows(rng, 7, wrong=0.5)


ORDER_SEED = 2            # (the first seed whose draw discriminates: vertex 6 ends at 0.8498 in the reference's order, 0.6712 in ascending j)


def refused_cases():
    """name -> Case that mvosr_reliability_batch refuses with MVOSR_ST_ERR_MASK."""
    rng = np.random.default_rng(77)
    z, v = _depth_rows(rng, 16)
    good = strip(12)
    return {"vertex_twice": Case("vertex_twice", np.concatenate([good, [[13, 14, 14]]]), z, v),
            "id_too_large": Case("id_too_large", np.concatenate([good[:6], [[3, 4, 16]], good[6:]]), z, v),
            "id_negative": Case("id_negative", np.concatenate([[[3, -1, 5]], good]), z, v)}


# ---- real frames ---------------------------------------------------------------------------------------------------------------
GOLDEN_SIZES = (120, 300, 600, 2000)
VANISH = 185.0


def synth_vote_frame(idx, n):
    """(remapped feature3d, feature2d, SciPy's rows) of synth_frame(idx, n) below the vanishing row: what feature_selection hands
    the vote (scale_calculator.py:252-259)."""
    from scipy.spatial import Delaunay
    from mvoscalerecovery_amd import constants as K
    from mvoscalerecovery_amd import synth
    f3, f2 = synth.synth_frame(idx, n)
    f3 = f3.copy()
    y = f3[:, 1] * np.cos(K.CAMERA_PITCH) - f3[:, 2] * np.sin(K.CAMERA_PITCH)   # :391-394
    zz = f3[:, 1] * np.sin(K.CAMERA_PITCH) + f3[:, 2] * np.cos(K.CAMERA_PITCH)
    f3[:, 1], f3[:, 2] = y, zz
    low = f2[:, 1] > VANISH
    f3, f2 = np.ascontiguousarray(f3[low]), np.ascontiguousarray(f2[low])
    return f3, f2, Delaunay(f2).simplices.astype(np.int32)


def sequence_frames():
    """The 36 frames of the sequence golden."""
    from mvoscalerecovery_amd import synth
    return [synth.synth_frame(i, 2000 if i % 9 == 8 else 300 + 37 * (i % 8), base_seed=4242, upper_fraction=0.1) for i in range(36)]


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reliability.npz"), allow_pickle=False)


# ---- launcher (GPU) ------------------------------------------------------------------------------------------------------------
def run_cases(ctx, cases, max_feat=None, sentinel=None, pitch=None):
    """mvosr_reliability_batch over `cases` as ONE batch (they share a camera pitch) -> one dict per case: "reliability", "keep",
    "status".  max_feat: what the header states (None: the largest frame's).  sentinel: every output byte is pre-set to it and
    each buffer has a guard element -> (results, guards)."""
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.engine import make_params
    import flat_cases as fc
    pitches = {c.pitch for c in cases} if pitch is None else {float(pitch)}
    assert len(pitches) == 1, "one launch, one camera pitch"
    cnt = np.array([c.n_feat for c in cases], dtype=np.int32)
    padded = (cnt.astype(np.int64) + 1) & ~np.int64(1)
    off = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(c.tri) for c in cases])]).astype(np.int64)
    total = max(int(off[-1]), 2)

    def plane(get):
        a = np.zeros(total)
        for c, o in zip(cases, off):
            a[o:o + c.n_feat] = get(c)
        return a
    tri = np.concatenate([c.tri.reshape(-1) for c in cases] + [np.zeros(3, np.int32)]).astype(np.int32)
    d = [ctx.to_device(off[:-1].copy() if len(cases) else off), ctx.to_device(cnt), ctx.to_device(toff), ctx.to_device(tri),
         ctx.to_device(plane(lambda c: c.y)), ctx.to_device(plane(lambda c: c.z)), ctx.to_device(plane(lambda c: c.v))]
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.tri1_off, b.tri1 = len(cases), d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr
    b.y, b.z, b.v = d[4].ptr, d[5].ptr, d[6].ptr
    b.max_feat, b.total_feat = int(cnt.max() if max_feat is None else max_feat), total
    o = fc._alloc(ctx, {"reliability": (total, np.float64), "keep": (total, np.int32), "status": (len(cases), np.int32)}, sentinel)
    p = make_params(1.75, camera_pitch=pitches.pop())
    _lib.check(ctx.lib.mvosr_reliability_batch(ctx.handle, C.byref(p), C.byref(b), o["reliability"].ptr, o["keep"].ptr, o["status"].ptr),
               "mvosr_reliability_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + d)
    res = [{"reliability": r["reliability"][off[i]:off[i] + cnt[i]], "keep": r["keep"][off[i]:off[i] + cnt[i]], "status": int(r["status"][i])}
           for i in range(len(cases))]
    if sentinel is None:
        return res
    return res, fc._tails(r, {"reliability": total, "keep": total, "status": len(cases)})
