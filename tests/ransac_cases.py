"""Crafted point clouds, sample tables and references for ransac_plane_kernel (plane and line) and plane_inliers_kernel
(csrc/mvosr_rescale.hip) — shared by tests/test_ransac_cases.py (CPU: the references against one another) and
tests/test_gpu_ransac.py (the C entry points on the device).  Test infrastructure.

A case is a point cloud and a table of sample triples.  Most clouds are unions of horizontal planes y = L: three points of one
level give e1_y = e2_y = 0 exactly, so n_x = n_z = 0 exactly and the hypothesis IS the plane y = L whatever the three points are;
a point of level L' lies |L' - L| / sqrt(1 + L^2) from it, and the levels are placed so that this is far (> 1e-3) from the
threshold on either side.  The inlier count of such a hypothesis is then a sum of level sizes — known exactly, and confirmed by
np.longdouble bounds that coincide.  The 2-D view of a case (x, y; the first two columns of its table, the third replaced by
garbage) is the same construction for the line variant: a pair of one level gives a = y1 - y0 = 0 exactly.

Tolerances (u = 2^-53), none of them fitted to a kernel:
  * plane counts and model: flat_cases.count_bounds / flat_cases.plane_ld (derived above flat_cases._plane_terms);
  * line counts and model: `_line_terms` below — a = y1 - y0 and b = -(x1 - x0) carry one rounding each, c = -(a x0 + b y0) two
    products and one sum; the rest as for the plane;
  * inlier mask: the model is given, only the four-term sum rounds: eps = 2 * 4.1 u (sum |p_i n_i| + |d|), count_bounds' last term.
Measured on the CPU (tests/test_ransac_cases.py prints it): the float64 restatement of the kernel's expressions (`numpy_model`)
uses at most 0.04 of the plane model's tolerance and 0.07 of the line model's over the first 64 hypotheses of every case here.
"""
import ctypes as C

import numpy as np

import flat_cases as fc
from flat_cases import N_HYPS, THRESHOLD, GOAL, U53, count_bounds, plane_ld, replay          # noqa: F401  (re-exported)

POINT_COUNTS = (1, 2, 3, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8193 + 37)
CHUNK = 4096                                   # kRsBlock * kRansacPPT: the points a workgroup holds in registers at a time
H_OF = {1: 63, 2: 64, 3: 65, 63: 100, 64: 129, 65: 1, 511: 512, 512: 63, 513: 64, 4095: 65, 4096: 100, 4097: 129, 8230: 512}
GOAL_M = (5, 10, 65, 100, 5120)                # M * 0.8 is an integer in float64 (64 * 0.8 and 4096 * 0.8 are not)
BATCH_H = 65                                   # the hypothesis count of the one ragged batch (every table resized to it)
MODEL_SHARE_MEASURED = {"plane": 0.04, "line": 0.07}
WIDE_H = 130                                   # the replay runs 64 hypotheses at a time: two full blocks and a ragged one of 2
WIDE_M = 65                                    # the smallest SIZES entry with all five levels


class Case:
    """pts (M, 3); samples (H, 3) int32 (any value: the kernel guards them); pinned: both count bounds must coincide for EVERY
    hypothesis (else for 98 %); zero: every count is exactly 0 (threshold 0 — not a question of bounds); expect: per hypothesis
    the count known from the construction (or None)."""

    def __init__(self, name, pts, samples, threshold=THRESHOLD, goal=GOAL, pinned=False, zero=False, expect=None, note=""):
        self.name, self.note, self.threshold, self.goal, self.pinned, self.zero = name, note, float(threshold), float(goal), pinned, zero
        self.pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        self.samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3)
        self.expect = None if expect is None else np.asarray(expect, dtype=np.int64)
        self.M, self.H = len(self.pts), len(self.samples)

    def line_samples(self):
        """The table as the line variant gets it: the pair, and garbage (but in range) in the third column."""
        s = self.samples.copy()
        s[:, 2] = np.random.default_rng(self.H + self.M).integers(0, max(self.M, 1), self.H)
        return s

    def resized(self, H):
        return Case(self.name, self.pts, np.resize(self.samples, (H, 3)) if self.H else np.zeros((H, 3), np.int32), self.threshold,
                    self.goal, self.pinned, self.zero, None if self.expect is None else np.resize(self.expect, H), self.note)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def _level(rng, n, y):
    return np.column_stack([rng.uniform(-12, 12, n), np.full(n, float(y)), rng.uniform(5, 30, n)])


def _pick3(rng, ids):
    return list(rng.choice(ids, 3, replace=False))


def two_plane(M, H, seed):
    """Roads A (y = 1.7) and B (y = 2.5) with EQUAL numbers of points in the body and outliers between y = -3 and 0.5; the last
    points of the cloud — the partly filled last chunk when M > 4096 — are all B's: B beats A by the tail alone, and every B
    hypothesis counts the tail's rows.  Table: A, B and mixed triples, and every 11th a triple that repeats an index."""
    rng = np.random.default_rng(seed)
    n_tail = (M - 1) % CHUNK + 1 if M > CHUNK else max(M // 8, 3)
    n_out = max(M // 5, 3)
    n_a = (M - n_tail - n_out) // 2
    n_out = M - n_tail - 2 * n_a
    body = np.concatenate([_level(rng, n_a, 1.7), _level(rng, n_a, 2.5),
                           np.column_stack([rng.uniform(-12, 12, n_out), rng.uniform(-3.0, 0.5, n_out), rng.uniform(5, 30, n_out)])])
    kind = np.concatenate([np.zeros(n_a, int), np.ones(n_a, int), np.full(n_out, 2)])
    p = rng.permutation(len(body))
    pts, kind = np.concatenate([body[p], _level(rng, n_tail, 2.5)]), np.concatenate([kind[p], np.ones(n_tail, int)])
    ia, ib = np.nonzero(kind == 0)[0], np.nonzero(kind == 1)[0]
    rows, expect = [], []
    for h in range(H):
        if h % 11 == 10:
            i, j = rng.choice(M, 2, replace=False)
            rows.append([[i, j, i], [i, i, j], [j, i, i]][h % 3]); expect.append(0)
        elif h % 3 == 0:
            rows.append(_pick3(rng, ia)); expect.append(n_a)
        elif h % 3 == 1:
            t = _pick3(rng, ib)
            if h % 2:
                t[h % 3] = M - 1 - int(rng.integers(0, n_tail))            # a sample point from the tail itself
            rows.append(t if len(set(t)) == 3 else _pick3(rng, ib)); expect.append(n_a + n_tail)
        else:
            rows.append(_pick3(rng, M)); expect.append(-1)
    return Case("road_%d" % M, pts, rows, pinned=True, expect=expect,
                note="A: %d, B: %d + %d in the tail, %d outliers; %d hypotheses" % (n_a, n_a, n_tail, n_out, H))


def tiny(M, H):
    """M = 1, 2, 3: every triple of fewer than three points repeats one (all hypotheses degenerate: NaN model, best_ic 0,
    used == H); three points give their own plane with all three on it."""
    rng = np.random.default_rng(M)
    pts = np.array([[0.5, 1.7, 6.0], [-3.0, 1.2, 9.0], [2.0, 1.9, 14.0]])[:M]
    rows = [rng.permutation(3) % M for _ in range(H)]
    return Case("road_%d" % M, pts, rows, pinned=True, expect=[3 if M == 3 else 0] * H, note="%d points" % M)


def grid_case(H=100, seed=3):
    """A jittered 12 x 10 grid on a tilted plane (every coordinate rounds), eight vertices lifted off it by 0.05."""
    rng = np.random.default_rng(seed)
    gx, gz = np.meshgrid(np.arange(12) - 6.0, np.arange(10) + 6.0, indexing="ij")
    xz = np.column_stack([gx.ravel(), gz.ravel()]) + rng.uniform(-0.15, 0.15, (120, 2))
    y = 1.7 + 0.03 * xz[:, 0] - 0.02 * xz[:, 1]
    off = rng.choice(120, 8, replace=False)
    y[off] += 0.05
    on = np.setdiff1d(np.arange(120), off)
    rows, expect = [], []
    for h in range(H):
        # well-shaped triples only: three vertices at least four cells apart (nearly collinear triples are left out)
        while True:
            t = _pick3(rng, on if h % 4 else 120)
            a, b, c = xz[t]
            if abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])) > 16.0:
                break
        rows.append(t); expect.append(112 if h % 4 else -1)
    return Case("grid", np.column_stack([xz[:, 0], y, xz[:, 1]]), rows, pinned=True, expect=expect, note="tilted plane, 112 of 120 on it")


LEVELS = (1.7, 1.706, 1.712, 3.0, 4.0)         # L0, L1, L2 (0.006 apart: 0.0030 from a neighbour's plane, 0.0061 from the next), F1, F2
SIZES = {5: (3, 1, 1, 0, 0), 10: (4, 4, 2, 0, 0), 65: (34, 18, 5, 4, 4), 100: (50, 30, 8, 6, 6), 5120: (3000, 1096, 600, 212, 212)}


def level_counts(sizes, threshold=THRESHOLD):
    """The count of a hypothesis sampled from level k: the sizes of the levels within threshold * sqrt(1 + L_k^2) of it —
    every |L_j - L_k| / sqrt(1 + L_k^2) is further than 1e-3 from the threshold (asserted)."""
    out = []
    for k, lk in enumerate(LEVELS):
        d = np.array([abs(lj - lk) / np.sqrt(1.0 + lk * lk) for lj in LEVELS])
        assert np.all(np.abs(d - threshold) > 1e-3)
        out.append(int(sum(s for s, dj in zip(sizes, d) if dj < threshold)))
    return out


def replay_cases():
    """Tables whose counts are sums of level sizes.  With goal 0.8 and sizes a + b = 0.8 M: a hypothesis of L0 counts EXACTLY the
    goal (no stop), one of L1 counts a + b + c (above it: stop), F1 and F2 tie."""
    out = []
    for M, sizes in SIZES.items():
        rng = np.random.default_rng(1000 + M)
        pts = np.concatenate([_level(rng, n, y) for n, y in zip(sizes, LEVELS)])
        pts = pts[rng.permutation(M)]
        ids = [np.nonzero(pts[:, 1] == y)[0] for y in LEVELS]
        cnt = level_counts(sizes)

        def table(name, spec, goal=GOAL, note="", spent=lambda i, j: [i, j, j]):
            rows, expect = [], []
            for k in spec:
                if k < 0:
                    i, j = rng.choice(M, 2, replace=False)
                    rows.append(spent(i, j)); expect.append(0)
                else:
                    rows.append(_pick3(rng, ids[k])); expect.append(cnt[k])
            out.append(Case("%s_%d" % (name, M), pts, rows, goal=goal, pinned=True, expect=expect, note=note))

        if M == 5:
            table("goal_equal", (0, -1, 0, 0), note="counts 4 == 0.8 * 5: never a stop, the first occurrence stays")
        elif M == 10:
            table("goal_equal", (-1, 0, 0, 1, 1, 0), note="8 == goal: no stop; then 10 > goal: stop at index 3, used 4")
        else:
            table("tie", (-1, 3, 4, 4, 3, -1), note="F1 and F2 tie on the best count: F1, the first, wins; used == H")
            table("goal_equal", (3, 0, 2, 0, -1, 4), note="L0 counts exactly the goal: no stop, used == H")
            table("goal_stop", (3, 2, 0, 1, 1, 0, -1), note="L1 is the first count above the goal: used == 4")
            table("later_larger", (3, 2, 0, 1, -1), goal=0.25, note="goal 0.25 M: L2 stops the loop at index 1; the larger L0, L1 after it are ignored")
            table("never", (-1, 3, 2, 4, 2), note="the goal is never reached: used == H")
        if M == WIDE_M:
            # WIDE_H hypotheses, for the replay 64 at a time.  `at`: index -> level; the other rows cycle through `before` up to the
            # last index of `at` and through `after` behind it; a spent row repeats its FIRST index (spent for the line's pair too).
            def wide(name, at, before=(-1,), after=(-1,), goal=GOAL, note=""):
                last = max(at)
                spec = [at.get(h, before[h % len(before)] if h < last else after[h % len(after)]) for h in range(WIDE_H)]
                table("wide_" + name, spec, goal, note, spent=lambda i, j: [i, i, j])

            for i in WIDE_STOPS:
                wide("stop%d" % i, {i: 1}, before=(0, 2, 3, -1, 4), after=(1, 0),
                     note="L1 at %d is the first count above the goal (L0 before it counts exactly the goal): best %d, used %d" % (i, i, i + 1))
            wide("tie_adjacent", {63: 3, 64: 4}, note="F1 at 63 and F2 at 64 tie across the blocks' edge, the rest is spent: 63 wins, used == H")
            wide("tie_apart", {64: 3, 128: 4}, note="F1 at 64 and F2 at 128 tie two blocks apart: 64 wins, used == H")
            wide("stop_then_larger", {62: 2}, before=(3, -1, 4), after=(0, 1), goal=0.25,
                 note="goal 0.25 M: L2 at 62 stops the loop; the larger L0, L1 from 63 on (the rest of its block and blocks 1, 2) are ignored")
            wide("goal_exact", {0: 0}, note="L0 at 0 counts exactly the goal, the rest is spent: best 0, used == H")
    return out


WIDE_STOPS = (63, 64, 65, 129)                 # the last lane of block 0, the first two of block 1, the last of the ragged block


def wide_expected(case):
    """(best, best_ic, used) the notes of the wide tables promise, from the construction alone."""
    kind = case.name[len("wide_"):].rsplit("_", 1)[0]
    cnt = level_counts(SIZES[WIDE_M])
    if kind.startswith("stop") and kind[4:].isdigit():
        return int(kind[4:]), cnt[1], int(kind[4:]) + 1
    return {"tie_adjacent": (63, cnt[3], WIDE_H), "tie_apart": (64, cnt[3], WIDE_H), "stop_then_larger": (62, cnt[2], 63),
            "goal_exact": (0, cnt[0], WIDE_H)}[kind]


def edge_cases():
    out = []
    rng = np.random.default_rng(77)
    base = two_plane(200, 24, 5)
    P = base.pts
    ia = np.nonzero(P[:, 1] == 1.7)[0]
    # ---- the sign rule: n_y of the best plane negative (all four negated), positive, exactly zero (kept as it is) ----------
    i, j, k = ia[:3]
    e1, e2 = P[j] - P[i], P[k] - P[i]
    pos = [i, j, k] if e1[2] * e2[0] - e1[0] * e2[2] > 0 else [i, k, j]
    out.append(Case("sign_pos", P, [pos], pinned=True, expect=[base.expect[0]], note="n_y > 0 as sampled"))
    out.append(Case("sign_neg", P, [[pos[0], pos[2], pos[1]]], pinned=True, expect=[base.expect[0]], note="n_y < 0 as sampled: negated"))
    # the line variant's b = -(x1 - x0): the same two cases by the order of the pair
    lo, hi = (i, j) if P[i, 0] < P[j, 0] else (j, i)
    out.append(Case("sign_line_neg", P, [[lo, hi, k]], pinned=True, note="x1 > x0: b < 0 as sampled"))
    out.append(Case("sign_line_pos", P, [[hi, lo, k]], pinned=True, note="x1 < x0: b > 0 as sampled"))
    # a wall x = 2 (e1_x = e2_x = 0 exactly: n_y = +-0; in 2-D x0 == x1: b = -0.0) next to scattered points, both orientations
    wall = np.column_stack([np.full(40, 2.0), rng.uniform(-2, 2, 40), rng.uniform(5, 30, 40)])
    pw = np.concatenate([wall, np.column_stack([rng.uniform(3, 12, 25), rng.uniform(-2, 2, 25), rng.uniform(5, 30, 25)])])
    out.append(Case("sign_zero_a", pw, [[0, 1, 2]], pinned=True, expect=[40], note="n_y == 0: kept as sampled"))
    out.append(Case("sign_zero_b", pw, [[1, 0, 2]], pinned=True, expect=[40], note="n_y == 0, the other orientation: kept as sampled"))
    # ---- threshold 0: |r| < 0 is false even for the sample points ------------------------------------------------------------
    out.append(Case("threshold_zero", P, base.samples, threshold=0.0, zero=True, note="nothing counts"))
    # ---- NaN coordinates -----------------------------------------------------------------------------------------------------
    nn = P.copy()
    free = np.setdiff1d(np.arange(200), base.samples.reshape(-1))
    for c, idx in enumerate(free[:9]):
        nn[idx, c % 3] = np.nan                                       # x, y or z of points no sample names
    out.append(Case("nan_point", nn, base.samples, pinned=True, note="NaN in x, y or z of nine non-sample points: never inliers"))
    ns = P.copy()
    ns[base.samples[0, 0], 0] = np.nan
    ns[base.samples[1, 1], 1] = np.nan
    ns[base.samples[4, 2], 2] = np.nan
    out.append(Case("nan_sample", ns, base.samples, pinned=True, note="NaN in a sample point of hypotheses 0, 1, 4 (and whoever shares it): NaN model, count 0"))
    # ---- every hypothesis degenerate -------------------------------------------------------------------------------------------
    deg = [[i, i, j] if h % 2 else [i, j, i] for h, (i, j) in enumerate(rng.integers(0, 200, (65, 2)))]
    out.append(Case("all_degenerate", P, deg, pinned=True, expect=[0] * 65, note="best_ic 0, NaN model, used == H"))
    # ---- sample indices outside [0, M) among valid ones ----------------------------------------------------------------------
    s = np.resize(base.samples, (64, 3)).copy()
    bad = [200, -1, 2 ** 31 - 1]
    for h in range(0, 64, 3):
        s[h, (h // 3) % 3] = bad[(h // 3) % 3]
    s[63] = [-1, 200, 2 ** 31 - 1]
    out.append(Case("index_guard", P, s, pinned=True, note="M, -1 and 2^31 - 1 in every column: spent like a repeated index"))
    return out


_CASES = None


def cases():
    """name -> Case, built once."""
    global _CASES
    if _CASES is None:
        lst = [tiny(M, H_OF[M]) if M <= 3 else two_plane(M, H_OF[M], 100 + M) for M in POINT_COUNTS]
        lst += [grid_case()] + replay_cases() + edge_cases()
        _CASES = {c.name: c for c in lst}
        assert len(_CASES) == len(lst)
    return _CASES


# ---- references -----------------------------------------------------------------------------------------------------------
def _spent(case, line):
    """Per hypothesis: the sample cannot give a model — an index out of range or repeated, or a NaN coordinate in a sample
    point (the contract of include/mvosr.h: NaN model, count 0)."""
    s = case.samples.astype(np.int64)[:, :2 if line else 3]
    oob = ((s < 0) | (s >= case.M)).any(1)
    sc = np.where((s < 0) | (s >= case.M), 0, s)
    rep = (sc[:, 0] == sc[:, 1]) if line else ((sc[:, 0] == sc[:, 1]) | (sc[:, 0] == sc[:, 2]) | (sc[:, 1] == sc[:, 2]))
    nan = np.isnan(case.pts[:, :2 if line else 3][sc] if case.M else np.zeros((case.H, 1, 1))).any((1, 2))
    return oob | rep | nan, sc


# The 2-D analogue of flat_cases._plane_terms for the kernel's line (a = y1 - y0, b = -(x1 - x0), c = -(a x0 + b y0), all scaled by
# 1 / sqrt(((a^2 + b^2) + 0) + c^2), r = ((px a + py b) + 0 * 0) + c), u = 2^-53:
#   * a and b are one subtraction each of exact inputs: |da| <= u |a|, |db| <= u |b| (1.1 u with second-order terms);
#   * |dc| <= |da| |x0| + |db| |y0| + 2.1 u (|a x0| + |b y0|) (two products, one addition);
#   * unnormalised, the residual at p moves by at most |da| |px| + |db| |py| + |dc|;
#   * the normaliser N = |(a, b, c)| moves by at most |(da, db, dc)|_2; the computed 1/N and the scaled components add 8 u
#     relative, as for the plane (the same expression with one exact zero in it);
#   * the final sum has two products and two additions that round (the z term is an exact + 0): 3.1 u (|px a| + |py b| + |c|) / N.
# eps = [|da| |px| + |db| |py| + |dc|] / N + (|r| / N) (|(da, db, dc)| / N + 8 u) + 3.1 u (|px a| + |py b| + |c|) / N, doubled as in
# count_bounds for the reference's own rounding and second-order terms.
def _line_terms(P2, pairs):
    L = np.longdouble
    p0, p1 = P2[pairs[:, 0]].astype(L), P2[pairs[:, 1]].astype(L)
    n = np.stack([p1[:, 1] - p0[:, 1], -(p1[:, 0] - p0[:, 0])], 1)
    dn = L(1.1 * U53) * np.abs(n)
    c = -np.sum(n * p0, 1)
    dc = np.sum(dn * np.abs(p0), 1) + L(2.1 * U53) * np.sum(np.abs(n * p0), 1)
    N = np.sqrt(np.sum(n * n, 1) + c * c)
    return n, c, dn, dc, N


def line_ld(P2, pair):
    """Unit (a, b, 0, c) with b >= 0 of the line through two points in np.longdouble, and the bound on the float64 line's
    components against it (the analogue of flat_cases.plane_ld)."""
    n, c, dn, dc, N = _line_terms(P2, np.asarray(pair).reshape(1, 2))
    m = np.array([n[0, 0], n[0, 1], np.longdouble(0), c[0]]) / N[0]
    err = np.sqrt(np.sum(dn[0] ** 2) + dc[0] ** 2) / N[0]
    tol = 2.0 * float(2 * err + 8 * U53)
    return (m if m[1] >= 0 else -m), tol


def line_count_bounds(P2, ids, pairs, threshold=THRESHOLD, chunk=64):
    """flat_cases.count_bounds for lines: per pair the number of points `ids` closer to its line than threshold - eps / + eps."""
    L = np.longdouble
    pairs = np.asarray(pairs).reshape(-1, 2)
    Q = P2[np.asarray(ids)].astype(L)
    lo, hi = np.zeros(len(pairs), np.int64), np.zeros(len(pairs), np.int64)
    for s in range(0, len(pairs), chunk):
        pr = pairs[s:s + chunk]
        n, c, dn, dc, N = _line_terms(P2, pr)
        with np.errstate(all="ignore"):
            r = np.abs(Q @ n.T + c[None, :]) / N[None, :]
            eps = (np.abs(Q) @ dn.T + dc[None, :]) / N[None, :] + r * (np.sqrt(np.sum(dn * dn, 1) + dc * dc) / N + 8 * U53)[None, :] \
                + L(3.1 * U53) * (np.abs(Q) @ np.abs(n).T + np.abs(c)[None, :]) / N[None, :]
            eps = 2 * eps
            a = (r < threshold - eps).sum(0)
            b = (~(r >= threshold + eps)).sum(0)
        rep = pr[:, 0] == pr[:, 1]
        lo[s:s + chunk], hi[s:s + chunk] = np.where(rep, 0, a), np.where(rep, 0, b)
    return lo, hi


_BOUNDS = {}


def bounds(case, line=False):
    """(lo, hi) per hypothesis, cached: count_bounds over the points without a NaN coordinate (a NaN point is never an inlier —
    `ids` leaves it out instead of letting it count for the upper bound), 0 for a spent sample, 0 everywhere at threshold 0."""
    key = (case.name, case.H, line)
    if key not in _BOUNDS:
        spent, sc = _spent(case, line)
        if case.zero or case.M == 0 or spent.all():
            lo = hi = np.zeros(case.H, np.int64)
        else:
            dims = 2 if line else 3
            P = case.pts[:, :dims]
            ids = np.nonzero(~np.isnan(P).any(1))[0]
            use = np.where(spent[:, None], 0, sc)                       # (a spent sample: any valid stand-in, its result is dropped)
            with np.errstate(all="ignore"):
                lo, hi = line_count_bounds(P, ids, use, case.threshold) if line else count_bounds(P, ids, use, case.threshold)
            lo, hi = np.where(spent, 0, lo), np.where(spent, 0, hi)
        _BOUNDS[key] = (lo, hi)
    return _BOUNDS[key]


def model_ld(case, h, line=False):
    """(unit model with the sign rule applied, tolerance) of hypothesis h in np.longdouble."""
    return line_ld(case.pts[:, :2], case.samples[h, :2]) if line else plane_ld(case.pts, case.samples[h])


def numpy_model(case, line=False):
    """The kernel's expressions in float64 NumPy, operation for operation: (models [H][4] before the sign rule, counts [H])."""
    spent, sc = _spent(case, line)
    P = case.pts if case.M else np.zeros((1, 3))
    p0, p1, p2 = (P[sc[:, k]] if k < sc.shape[1] else None for k in range(3))
    with np.errstate(all="ignore"):
        if line:
            nx, ny, nz = p1[:, 1] - p0[:, 1], -(p1[:, 0] - p0[:, 0]), np.zeros(case.H)
            d = -(nx * p0[:, 0] + ny * p0[:, 1])
        else:
            e1, e2 = p1 - p0, p2 - p0
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
        inv = 1.0 / np.sqrt(((nx * nx + ny * ny) + nz * nz) + d * d)
        m = np.stack([nx * inv, ny * inv, nz * inv, d * inv], 1)
        m[spent] = np.nan
        z = np.zeros(len(P)) if line else P[:, 2]
        r = np.abs(((P[:, 0, None] * m[None, :, 0] + P[:, 1, None] * m[None, :, 1]) + z[:, None] * m[None, :, 2]) + m[None, :, 3])
        counts = (r < case.threshold).sum(0) if case.M else np.zeros(case.H, np.int64)
    return m, counts


def sign_rule(m):
    """rescale.py:159-161 on a model of the kernel: negated when n_y < 0 (-0.0 is not)."""
    return -m if m[1] < 0 else m


# ---- the inlier mask ------------------------------------------------------------------------------------------------------
MASK_SIZES = (1, 255, 256, 257, 100003)
MASK_THRESHOLD = 0.01                          # estimate_road_norm.get_inliers as road_model_calculation_ransac calls it


def mask_case(n, seed=9):
    """n points round a tilted plane: two thirds within +-0.008 of it along y, the rest up to +-0.5 — and the float64 model of the
    plane through three of them (flat_cases.plane_ld).  -> (pts, model4)"""
    rng = np.random.default_rng(seed + n)
    xz = np.column_stack([rng.uniform(-12, 12, n + 3), rng.uniform(5, 30, n + 3)])
    y = 1.7 + 0.03 * xz[:, 0] - 0.02 * xz[:, 1]
    anchors = np.array([[-10.0, 1.7 - 0.3 - 0.2, 10.0], [9.0, 1.7 + 0.27 - 0.5, 25.0], [1.0, 1.7 + 0.03 - 0.12, 6.0]])
    m, _ = plane_ld(anchors, [0, 1, 2])
    y = y[:n] + np.where(rng.uniform(size=n) < 0.67, rng.uniform(-0.008, 0.008, n), rng.uniform(-0.5, 0.5, n))
    return np.column_stack([xz[:n, 0], y, xz[:n, 1]]), np.asarray(m, dtype=np.float64)


def mask_reference(pts, model, threshold=MASK_THRESHOLD):
    """(verdict, decided) in np.longdouble for the GIVEN float64 model: only the kernel's four-term sum rounds —
    eps = 2 * 4.1 u (sum |p_i n_i| + |d|), the last term of flat_cases.count_bounds."""
    L = np.longdouble
    P, m = pts.astype(L), model.astype(L)
    with np.errstate(invalid="ignore"):
        r = np.abs(P @ m[:3] + m[3])
        eps = 2 * L(4.1 * U53) * (np.abs(P) @ np.abs(m[:3]) + abs(m[3]))
        return r < threshold, np.abs(r - threshold) > eps


# ---- launchers (GPU) --------------------------------------------------------------------------------------------------------
def run_ransac(ctx, frames, line=False, n_hyp=None, ragged=False, want_counts=True):
    """mvosr_ransac_plane_batch / mvosr_ransac_line_batch over `frames` (Cases, or None for a frame of no points) with hand-built
    buffers -> one dict per frame.  Every frame's table must have n_hyp rows (None: the first frame's).  ragged: the frames lie
    in the point planes in a scrambled order with odd gaps of garbage between them; the threshold and goal are the first
    Case's.  counts is pre-filled with 0xFF bytes."""
    from mvoscalerecovery_amd import _lib
    real = [f for f in frames if f is not None]
    H = int(n_hyp if n_hyp is not None else real[0].H)
    F = len(frames)
    cnt = np.array([0 if f is None else f.M for f in frames], dtype=np.int32)
    order = np.arange(F)
    gaps = np.zeros(F, np.int64)
    if ragged:
        rng = np.random.default_rng(F)
        order = rng.permutation(F)
        gaps = rng.integers(1, 40, F) | 1
    off = np.zeros(F, np.int64)
    pos = 0
    for f in order:
        pos += int(gaps[f])
        off[f] = pos
        pos += int(cnt[f])
    planes = np.full((3, max(pos, 1) + 1), 1.0e300 if ragged else 0.0)
    tab = np.zeros((F, H, 3), np.int32)
    for i, f in enumerate(frames):
        if f is None:
            tab[i] = 7                                                   # (never read: the frame has no points)
            continue
        assert f.H == H, (f.name, f.H, H)
        planes[:, off[i]:off[i] + f.M] = f.pts.T
        tab[i] = f.line_samples() if line else f.samples
    d = [ctx.to_device(off), ctx.to_device(cnt), ctx.to_device(planes[0].copy()), ctx.to_device(planes[1].copy()),
         ctx.to_device(planes[2].copy()), ctx.to_device(tab)]
    o = {"counts": ctx.empty((F, H), np.int32).fill(0xFF), "model": ctx.empty((F, 4), np.float64).fill(0x55),
         "best_ic": ctx.empty(F, np.int32).fill(0x55), "used": ctx.empty(F, np.int32).fill(0x55)}
    cp = o["counts"].ptr if want_counts else None
    thr, goal = real[0].threshold, real[0].goal
    assert all(f.threshold == thr and f.goal == goal for f in real)
    if line:
        _lib.check(ctx.lib.mvosr_ransac_line_batch(ctx.handle, F, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[5].ptr, H, thr, goal, cp,
                                                   o["model"].ptr, o["best_ic"].ptr, o["used"].ptr), "mvosr_ransac_line_batch")
    else:
        _lib.check(ctx.lib.mvosr_ransac_plane_batch(ctx.handle, F, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, H, thr, goal,
                                                    cp, o["model"].ptr, o["best_ic"].ptr, o["used"].ptr), "mvosr_ransac_plane_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + d)
    return [{"counts": r["counts"][i], "model": r["model"][i], "best_ic": int(r["best_ic"][i]), "used": int(r["used"][i])} for i in range(F)]


def run_mask(ctx, pts, model, threshold=MASK_THRESHOLD, n=None, guard=64):
    """mvosr_plane_inliers on `pts` -> (mask bytes [n], the `guard` bytes behind them, pre-filled with 0xA5)."""
    from mvoscalerecovery_amd import _lib
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts) if n is None else n
    d = [ctx.to_device(np.ascontiguousarray(pts[:, k]) if len(pts) else np.zeros(1)) for k in range(3)]
    mask = ctx.empty(n + guard, np.uint8).fill(0xA5)
    par = np.ascontiguousarray(model, dtype=np.float64)
    _lib.check(ctx.lib.mvosr_plane_inliers(ctx.handle, n, d[0].ptr, d[1].ptr, d[2].ptr, _lib.addr(par), float(threshold), mask.ptr),
               "mvosr_plane_inliers")
    ctx.sync()
    out = mask.download()
    fc._free(d + [mask])
    return out[:n], out[n:]
