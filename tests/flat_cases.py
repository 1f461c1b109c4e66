"""Crafted frames and references for flat_selection_kernel (csrc/mvosr_rescale.hip) — shared by tests/test_flat_select_cases.py
(CPU: NumPy in the kernel's place) and tests/test_gpu_flat_select.py (both entry points on the device).  Test infrastructure.

The rows of tri2 are an input, so a frame here is a list of small triangles with three vertices of their own: a triangle whose
three y are h has n = A^-1.1 = (0, 1/h, 0) — height h, pitch -90 deg —, a repeated row gives a bit-identical height, and a rotation
about the x axis through the origin keeps the height and moves the pitch to -(90 - tilt) deg.

References: `mp_rows` (mpmath, 60 digits) for the continuous part, `count_bounds` / `plane_ld` (np.longdouble) for the tail,
`numpy_flat` (float64 LAPACK) as the stand-in of the kernel on the CPU and as the measure of the error constant C_HEIGHT.
`select_plan` is a coverage probe only — no expected value comes from it.
"""
import ctypes as C

import numpy as np

LOOSE_DEG, TIGHT_DEG = -80.0, -85.0
U53 = 2.0 ** -53
# Largest |h_numpy - h_mpmath| / (|h| kappa_inf(A) 2^-53) over every row of every family below, NumPy's float64 linalg.solve against
# mpmath (test_flat_select_cases.py measures it again and asserts that it has not grown): 0.93.  The kernel's pivot order and its
# (a + b) + c sums are not LAPACK's: a factor 4 on the measured maximum, rounded up.
C_HEIGHT_MEASURED = 0.93
C_HEIGHT = 3.75
THRESHOLD, GOAL, MIN_POINTS, ABS_REF = 0.005, 0.8, 12, 1.75           # rescale.py:152,155,167; estimate_road_norm.py:68
ST_SINGULAR, ST_MASK, ST_EMPTY, ST_RS_FEW = 7, 8, 9, 11
N_HYPS = (1, 63, 64, 65, 100, 129, 512)


class Frame:
    """xyz: every feature; keep: None or int32 words (-1 dropped, 0 / 1 survive); tri: rows numbered over the survivors;
    skip: rows with a bad id or a singular matrix (no continuous reference); status: what both forms must report apart from
    MVOSR_ST_RS_FEW (0 / _SINGULAR / _MASK)."""

    def __init__(self, name, xyz, tri, keep=None, skip=None, status=0, bad=None, note=""):
        self.name, self.note, self.status = name, note, status
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        self.keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.int32)
        self.skip = np.zeros(len(self.tri), bool) if skip is None else np.asarray(skip, bool)
        self.bad = np.zeros(len(self.tri), bool) if bad is None else np.asarray(bad, bool)

    def survivors(self):
        return self.xyz if self.keep is None else self.xyz[self.keep >= 0]

    def with_keep(self, seed, dropped, mode="mixed"):
        """The same frame behind keep words: `dropped` extra features (keep = -1) scattered among the survivors."""
        rng = np.random.default_rng(seed)
        P = self.survivors()
        n = len(P) + dropped
        pos = np.sort(rng.choice(n, len(P), replace=False))
        xyz = rng.uniform(-50.0, 50.0, (n, 3))
        xyz[pos] = P
        keep = np.full(n, -1, np.int32)
        keep[pos] = rng.integers(0, 2, len(P)) if mode == "mixed" else 1
        return Frame(self.name + "+keep", xyz, self.tri, keep, self.skip, self.status, self.bad, self.note)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def _rot_x(p, tilt_deg):
    t = np.deg2rad(tilt_deg)
    c, s = np.cos(t), np.sin(t)
    return np.column_stack([p[:, 0], p[:, 1] * c - p[:, 2] * s, p[:, 1] * s + p[:, 2] * c])


def _shape(rng, near=False):
    """Three (x, z) of a well-shaped triangle of size ~1 (near: close to the origin, for a small condition number)."""
    c = np.array([rng.uniform(-1, 1), rng.uniform(2, 4)]) if near else np.array([rng.uniform(-5, 5), rng.uniform(5, 20)])
    ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, 3)
    r = rng.uniform(0.6, 1.4, 3)
    return c + r[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])


def flat_tri(rng, h, tilt_deg=0.0, shape=None, near=False):
    xz = _shape(rng, near) if shape is None else shape
    p = np.column_stack([xz[:, 0], np.full(3, float(h)), xz[:, 1]])
    return _rot_x(p, tilt_deg) if tilt_deg else p


def disjoint(name, specs, seed, note="", shuffle=True, near=False):
    """specs: (height, tilt_deg, repeats) per triangle; every triangle has its own three vertices, a repeated row is the same
    three ids again.  Rows are shuffled so that repeats do not sit next to one another."""
    rng = np.random.default_rng(seed)
    pts, rows = [], []
    for i, (h, tilt, reps) in enumerate(specs):
        pts.append(flat_tri(rng, h, tilt, near=near))
        rows += [[3 * i, 3 * i + 1, 3 * i + 2]] * int(reps)
    rows = np.array(rows, dtype=np.int32).reshape(-1, 3)
    if shuffle:
        rows = rows[rng.permutation(len(rows))]
    return Frame(name, np.concatenate(pts) if pts else np.zeros((0, 3)), rows, note=note)


def _mu_numpy(p):
    n = np.linalg.solve(p, np.ones(3))
    return -n[1] / np.sqrt(np.sum(n * n))


def tilt_for_mu(shape, h, target):
    """Bisection on the tilt: the triangle whose NumPy mu = -n_y/|n| is (to rounding) `target`; mu = -cos(tilt) grows with it."""
    lo, hi = 0.0, 30.0
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        p = _rot_x(np.column_stack([shape[:, 0], np.full(3, float(h)), shape[:, 1]]), mid)
        if _mu_numpy(p) < target:
            lo = mid
        else:
            hi = mid
    return hi


def threshold_frame(seed=41):
    """Rows whose mu sits on sin(-80 deg) and sin(-85 deg) (found by bisection: the kernel's asin branch, |mu - s| <= 1e-12), at
    +-5e-13 of them (the same branch), and at +-1e-10, +-1e-8, +-1e-4 and ~0.5 deg on both sides (the comparison on mu)."""
    rng = np.random.default_rng(seed)
    pts, rows = [], []
    for deg in (LOOSE_DEG, TIGHT_DEG):
        s = np.sin(deg * np.pi / 180.0)
        for d in (0.0, 5e-13, -5e-13, 1e-10, -1e-10, 1e-8, -1e-8, 1e-4, -1e-4, 1.5e-3, -1.5e-3):
            shape, h = _shape(rng, near=True), rng.uniform(1.5, 1.9)
            t = tilt_for_mu(shape, h, s + d)
            pts.append(_rot_x(np.column_stack([shape[:, 0], np.full(3, h), shape[:, 1]]), t))
            rows.append([3 * len(rows), 3 * len(rows) + 1, 3 * len(rows) + 2])
    for h, tilt in ((1.7, 0.0), (1.6, 0.0), (1.8, 2.0), (1.65, 7.0), (1.75, 20.0)):      # and plain rows of all three classes
        pts.append(flat_tri(rng, h, tilt, near=True))
        rows.append([3 * len(rows), 3 * len(rows) + 1, 3 * len(rows) + 2])
    return Frame("thresholds", np.concatenate(pts), rows, note="mu on and around sin(-80), sin(-85)")


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def _val(u):
    return float(np.uint64(u).view(np.float64))


def _one_bin_start(lo_val, hi_val, near_val):
    """Start (as a value) and width (in patterns) of the first-pass bin that holds `near_val` when the loose heights span
    [lo_val, hi_val]."""
    lo, hi = _bits(lo_val), _bits(hi_val)
    shift = max((hi - lo).bit_length() - 11, 0)
    b = (_bits(near_val) - lo) >> shift
    return _val(lo + (b << shift)), 1 << shift


def select_families():
    """name -> Frame.  What the CPU prototype (`select_plan` on NumPy heights) reports is in each note; the tests assert the
    coverage over the SET, not per case."""
    rng = np.random.default_rng(7)
    fam = {}

    def add(name, specs, seed, note, **kw):
        fam[name] = disjoint(name, specs, seed, note, **kw)

    add("control", [(h, 0.0, 1) for h in rng.uniform(1.5, 1.9, 700)], 1, "direct, 1 candidate, 1 pass")
    add("one_row_x100", [(1.7, 0.0, 100)], 2, "range == 0, 0 passes; even k, both middles one pattern")
    add("k1", [(1.7, 0.0, 1), (1.5, 20.0, 1), (1.6, 7.0, 0)], 3, "range == 0, k = 1")
    add("cluster300", [(1.6 * (1 + j * 2.0 ** -49), 0.0, 1) for j in range(300)] + [(1e-3, 0.0, 1), (1e3, 0.0, 1)], 4,
        "direct, 5 passes", near=True)
    add("cluster200", [(1.6 * (1 + j * 2.0 ** -52), 0.0, 1) for j in range(200)] + [(1e-6, 0.0, 1), (1e6, 0.0, 1)], 5,
        "direct with tied / near candidates, 5 passes; even k", near=True)
    add("shift0", [(2.0, 0.0, 100)] + [(h, 0.0, 1) for h in rng.uniform(1.0, 1.9, 20)] + [(h, 0.0, 1) for h in rng.uniform(2.1, 3.0, 20)] +
        [(1e-3, 0.0, 1), (1e3, 0.0, 1)], 6, "one pattern (shift == 0), 5 passes; even k, both middles one pattern")
    for k in (0, 2, 3, 64, 65, 66):
        hs = rng.uniform(1.5, 1.9, k)
        specs = [(h, 7.0 if i < min(k, 2) else 0.0, 1) for i, h in enumerate(hs)] + [(h, 20.0, 1) for h in rng.uniform(1.5, 1.9, 5)]
        add("k%d" % k, specs, 10 + k, "k = %d loose rows (two of them not tight) among 5 that are not loose" % k)
    # the direct ranking at exactly 64 candidates, and 65 (another pass): a coarse first pass (outliers 1e-3, 1e3: bins of 2^46
    # patterns, 2^-6 wide at 1.5) and a cluster with a step of 1e-4 in the middle of one bin; the rank falls into the cluster
    start, _ = _one_bin_start(1e-3, 1e3, 1.5)
    side = [(h, 0.0, 1) for h in np.linspace(1.05, 1.40, 10)] + [(h, 0.0, 1) for h in np.linspace(1.6, 3.0, 10)] + [(1e-3, 0.0, 1), (1e3, 0.0, 1)]
    for c in (63, 64, 65):
        add("direct%d" % c, [(start + 0.004 + 1e-4 * i, 0.0, 1) for i in range(c)] + side, 20 + c,
            "%d candidates in the rank's bin after one pass: %s" % (c, "direct" if c <= 64 else "another pass, then direct with 1"))
    # bit-identical values inside the direct list, the rank on the tie: 11 below, one row four times, 10 above -> k = 25, klo = 12
    add("direct_tie", [(h, 0.0, 1) for h in np.linspace(1.05, 1.40, 10)] + [(1e-3, 0.0, 1)] + [(start + 0.006, 0.0, 4), (start + 0.007, 0.0, 1)] +
        [(h, 0.0, 1) for h in np.linspace(1.6, 3.0, 8)] + [(1e3, 0.0, 1)], 30, "direct, >= 4 tied candidates, rank on the tie; odd k")
    # even k: (a) both middles one pattern, its copies ending exactly at rank khi (le == khi + 1); (a3) one copy more;
    # (b) the upper middle in another bin; (c) the lower middle repeated, the copies ending at klo (le == khi)
    low, high = [(h, 0.0, 1) for h in (1.2, 1.3, 1.4)], [(h, 0.0, 1) for h in (1.9, 2.0, 2.1)]
    add("even_a", low + [(1.5, 0.0, 2)] + high, 31, "k = 8: klo = 3, khi = 4 on the two copies, le == khi + 1")
    add("even_a3", low + [(1.5, 0.0, 3)] + high[:2], 32, "k = 8: copies at ranks 3, 4, 5, le == khi + 2")
    add("even_b", low + [(1.5, 0.0, 1), (1.8, 0.0, 1)] + high, 33, "k = 8: lower middle 1.5, upper middle 1.8 in another bin")
    add("even_c", low[:2] + [(1.5, 0.0, 2)] + high + [(2.2, 0.0, 1)], 34, "k = 8: copies at ranks 2, 3 = klo, khi is the next value: le == khi")
    fam["thresholds"] = threshold_frame()
    # bad ids and singular rows next to valid heights
    base = disjoint("x", [(h, 0.0, 1) for h in rng.uniform(1.5, 1.9, 41)], 35)
    n = len(base.xyz)
    rows = np.concatenate([base.tri, [[0, 1, n], [-1, 4, 5], [7, 70000, 8]]]).astype(np.int32)
    bad = np.arange(len(rows)) >= len(base.tri)
    fam["bad_ids"] = Frame("bad_ids", base.xyz, rows, skip=bad, bad=bad, status=ST_MASK, note="three rows with an id out of range")
    p = np.array([0.75, 1.5, 3.25])
    xyz = np.concatenate([base.xyz, [p, 2 * p, 4 * p], [[0.0, 0.0, 0.0]]])
    rows = np.concatenate([base.tri, [[n, n + 1, n + 2], [0, 1, n + 3]]]).astype(np.int32)
    sing = np.arange(len(rows)) >= len(base.tri)
    fam["singular"] = Frame("singular", xyz, rows, skip=sing, status=ST_SINGULAR, note="P, 2P, 4P and a vertex at the origin")
    rows = np.concatenate([rows, [[0, 1, -5]]]).astype(np.int32)
    fam["bad_and_singular"] = Frame("bad_and_singular", xyz, rows, skip=np.arange(len(rows)) >= len(base.tri),
                                    bad=np.arange(len(rows)) == len(rows) - 1, status=ST_MASK, note="_MASK wins over _SINGULAR")
    return fam


# ---- frames for the RANSAC tail ---------------------------------------------------------------------------------------------
def count_layout(M, n, tn, n_distinct, block=1024):
    """The counting layout the device-resident form's conditions (mvosr_rescale.hip: `dedup`, `packed`) give a frame with M list
    entries, n survivors, tn rows and n_distinct vertices on kept rows."""
    dedup = 2 * ((M + 1) & ~1) + 2 * n <= 8 * tn and n <= 2 * 2048 - 2
    if not dedup:
        return "list"
    return "packed" if (n_distinct <= 2 * block and 28 * n_distinct + 8 <= 8 * tn) else "dedup"


def road_frame(name, n_road, n_other, seed, h=1.7, n_in=12, n_out=12, note=""):
    """A planar road (y = h exactly) of n_road vertices, n_in of them lifted by 0.002 (inliers of the road plane at threshold
    0.005: |dy| / sqrt(1 + h^2) = 0.001) and n_out by 0.05 (0.025: outliers) — both far more than 10 eps from the threshold —,
    next to n_other vertices of rough ground; rows: SciPy's Delaunay triangulation of (x, z)."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    xz = np.column_stack([rng.uniform(-12, 12, n_road), rng.uniform(5, 30, n_road)])
    y = np.full(n_road, h)
    lift = rng.choice(n_road, n_in + n_out, replace=False)
    y[lift[:n_in]] += 0.002
    y[lift[n_in:]] += 0.05
    if n_other:
        xz = np.concatenate([xz, np.column_stack([rng.uniform(-30, 30, n_other), rng.uniform(31, 60, n_other)])])
        y = np.concatenate([y, rng.uniform(-3.0, 1.0, n_other)])
    tri = Delaunay(xz).simplices
    return Frame(name, np.column_stack([xz[:, 0], y, xz[:, 1]]), tri, note=note)


def grid_frame(name="grid", nx=12, nz=10, seed=51, h=1.7, n_out=8):
    """A jittered nx x nz grid on the plane y = h, two rows per cell, n_out interior vertices lifted by 0.05 (tilt < 4 deg: still
    tight): the frame whose id_triples the tail tests choose."""
    rng = np.random.default_rng(seed)
    gx, gz = np.meshgrid(np.arange(nx) - nx / 2.0, np.arange(nz) + 6.0, indexing="ij")
    xz = np.column_stack([gx.ravel(), gz.ravel()]) + rng.uniform(-0.15, 0.15, (nx * nz, 2))
    y = np.full(nx * nz, h)
    inner = [i * nz + j for i in range(1, nx - 1) for j in range(1, nz - 1)]
    off = rng.choice(inner, n_out, replace=False)
    y[off] += 0.05
    rows = []
    for i in range(nx - 1):
        for j in range(nz - 1):
            a = i * nz + j
            rows += [[a, a + nz, a + 1], [a + 1, a + nz, a + nz + 1]]
    f = Frame(name, np.column_stack([xz[:, 0], y, xz[:, 1]]), rows, note="dedup, not packed (28 n_items + 8 > 8 tn)")
    f.off_plane = np.sort(off)
    return f


def fan_frame(name, n_ring, n_steep_rows, seed, h=1.7):
    """n_ring rows round one vertex on the plane y = h (its multiplicity in the list: n_ring), and one steep triangle repeated
    n_steep_rows times (never kept) to give the heights' room the size the layouts ask for."""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n_ring))
    r = rng.uniform(3.0, 5.0, n_ring)
    ring = np.column_stack([r * np.cos(ang), np.full(n_ring, h), 12.0 + r * np.sin(ang)])
    ring[rng.choice(n_ring, 6, replace=False), 1] += 0.05
    xyz = np.concatenate([[[0.0, h, 12.0]], ring, flat_tri(rng, 1.6, 30.0)])
    rows = [[0, 1 + i, 1 + (i + 1) % n_ring] for i in range(n_ring)] + [[n_ring + 1, n_ring + 2, n_ring + 3]] * n_steep_rows
    return Frame(name, xyz, rows)


def tail_families(max_points):
    """name -> Frame, with the counting layout the source's conditions give it (asserted by the tests from the kernel's own kept
    rows, over the set)."""
    fam = {}
    fam["road_packed"] = road_frame("road_packed", 600, 1400, 61, note="~600 distinct vertices on kept rows of 2000: packed")
    fam["road_dedup"] = road_frame("road_dedup", 2600, 0, 62, n_in=30, n_out=30,
                                   note="a planar road, nearly every row kept, > 2048 distinct vertices: dedup, not packed")
    fam["road_small"] = road_frame("road_small", 20, 0, 63, n_in=2, n_out=2, note="a 20-vertex Delaunay frame")
    fam["grid"] = grid_frame()
    fam["fan_dedup"] = fan_frame("fan_dedup", 320, 40, 64)
    fam["fan_dedup"].note = "one vertex on 320 kept rows; dedup, not packed"
    fam["fan_packed"] = fan_frame("fan_packed", 320, 900, 65)
    fam["fan_packed"].note = "one vertex on 320 kept rows; packed"
    fam["at_max_points"] = road_frame("at_max_points", 700, max_points - 700, 66, note="ScaleEstimator._max_points() features")
    big = road_frame("x", 500, 0, 67)
    fam["keep_over_4096"] = big.with_keep(68, 4300 - 500)
    fam["keep_over_4096"].name = "keep_over_4096"
    fam["keep_over_4096"].note = "4300 features before keep (the looping compaction at load), 500 survivors"
    fam["keep_few"] = road_frame("x", 40, 0, 69, n_in=3, n_out=3).with_keep(70, 900, mode="ones")
    fam["keep_few"].name = "keep_few"
    fam["keep_few"].note = "all -1 but 40"
    return fam


# ---- the select's coverage probe -----------------------------------------------------------------------------------------
def select_plan(heights, bins=2048, direct=64):
    """Which exit a `bins`-bin histogram select on the bit patterns takes for the lower middle of `heights`, after how many
    passes, and with how many candidates.  A coverage probe: no expected value may come from it."""
    u = sorted(int(x) for x in np.asarray(heights, dtype=np.float64).view(np.uint64))
    k = len(u)
    if k == 0:
        return {"exit": "empty", "passes": 0, "cand": 0, "tie": False, "k": 0}
    rank, lo, hi, passes = (k - 1) // 2, u[0], u[-1], 0
    width = max((bins - 1).bit_length(), 1)
    while True:
        if hi == lo:
            return {"exit": "range0", "passes": passes, "cand": len(u), "tie": len(u) > 1, "k": k}
        shift = max((hi - lo).bit_length() - width, 0)
        passes += 1
        b = (u[rank] - lo) >> shift
        rank -= sum(1 for x in u if ((x - lo) >> shift) < b)
        u = [x for x in u if ((x - lo) >> shift) == b]
        lo += b << shift
        hi = min(lo + (1 << shift) - 1, hi)
        if shift == 0:
            return {"exit": "pattern", "passes": passes, "cand": len(u), "tie": len(u) > 1, "k": k}
        if len(u) <= direct:
            return {"exit": "direct", "passes": passes, "cand": len(u), "tie": u.count(u[rank]) > 1, "k": k}


def coverage(plans):
    """What a set of select_plan results covers; `missing` lists what the issue asks of the family set and the set lacks."""
    plans = list(plans)
    cov = {"exits": sorted({p["exit"] for p in plans}), "max_passes": max(p["passes"] for p in plans),
           "direct_cands": sorted({p["cand"] for p in plans if p["exit"] == "direct"}),
           "tie_in_direct": any(p["exit"] == "direct" and p["tie"] for p in plans),
           "two_passes": any(p["passes"] >= 2 for p in plans)}
    d = cov["direct_cands"]
    need = {"exit range0": "range0" in cov["exits"], "exit pattern": "pattern" in cov["exits"], "exit direct": "direct" in cov["exits"],
            "empty": "empty" in cov["exits"], ">= 2 passes": cov["two_passes"], ">= 5 passes": cov["max_passes"] >= 5,
            "direct with 1": 1 in d, "direct with 2..63": any(2 <= c <= 63 for c in d), "direct with 64": 64 in d,
            "tie in the direct list": cov["tie_in_direct"]}
    cov["missing"] = [k for k, ok in need.items() if not ok]
    return cov


# ---- references --------------------------------------------------------------------------------------------------------------
def numpy_flat(frame):
    """Heights and flag bits 0/1 of every row with float64 LAPACK (np.linalg.solve): the kernel's stand-in on the CPU."""
    P, tri = frame.survivors(), frame.tri
    hk = np.full(len(tri), np.nan)
    fl = np.zeros(len(tri), np.uint8)
    ok = ~frame.skip
    if ok.any():
        n = np.linalg.solve(P[tri[ok]], np.ones((int(ok.sum()), 3, 1)))[:, :, 0]
        ln = np.sqrt(np.sum(n * n, 1))
        pitch = np.arcsin(-n[:, 1] / ln) * 180.0 / np.pi
        hk[ok] = 1.0 / ln
        fl[ok] = (pitch < LOOSE_DEG).astype(np.uint8) | ((pitch < TIGHT_DEG).astype(np.uint8) << 1)
    return hk, fl


def expected_discrete(hk, fl, height_factor):
    """rescale.py:91-96 on given heights and flags: (level, kept)."""
    loose = (fl & 1) != 0
    level = height_factor * np.median(hk[loose]) if loose.any() else np.nan
    with np.errstate(invalid="ignore"):
        kept = ((fl & 2) != 0) & (hk > level)
    return level, kept


_MP_CACHE = {}


def _ld(x):
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - hi))


def mp_rows(frame):
    """Per row with mpmath at 60 digits: A n = 1 (adjugate over determinant), height = 1/|n| (np.longdouble), pitch = asin(-n_y/|n|)
    in degrees, kappa_inf(A) = |A|_inf |A^-1|_inf.  Rows in frame.skip are nan.  Cached per distinct row of a frame."""
    import mpmath as mp
    key = frame.name
    if key in _MP_CACHE:
        return _MP_CACHE[key]
    P, tri = frame.survivors(), frame.tri
    h = np.full(len(tri), np.nan, dtype=np.longdouble)
    pitch = np.full(len(tri), np.nan)
    kappa = np.full(len(tri), np.nan)
    seen = {}
    with mp.workdps(60):
        deg = 180 / mp.pi
        for t in range(len(tri)):
            if frame.skip[t]:
                continue
            row = tuple(int(v) for v in tri[t])
            if row not in seen:
                (a, b, c), (d, e, f), (g, hh, i) = [[mp.mpf(float(v)) for v in P[r]] for r in row]
                c00, c01, c02 = e * i - f * hh, f * g - d * i, d * hh - e * g
                det = a * c00 + b * c01 + c * c02
                c10, c11, c12 = c * hh - b * i, a * i - c * g, b * g - a * hh
                c20, c21, c22 = b * f - c * e, c * d - a * f, a * e - b * d
                nx, ny, nz = (c00 + c10 + c20) / det, (c01 + c11 + c21) / det, (c02 + c12 + c22) / det
                ln = mp.sqrt(nx * nx + ny * ny + nz * nz)
                ninv = max(abs(c00) + abs(c10) + abs(c20), abs(c01) + abs(c11) + abs(c21), abs(c02) + abs(c12) + abs(c22)) / abs(det)
                na = max(abs(a) + abs(b) + abs(c), abs(d) + abs(e) + abs(f), abs(g) + abs(hh) + abs(i))
                seen[row] = (_ld(1 / ln), float(mp.asin(-ny / ln) * deg), float(na * ninv))
            h[t], pitch[t], kappa[t] = seen[row]
    _MP_CACHE[key] = (h, pitch, kappa)
    return _MP_CACHE[key]


def height_bound(kappa, c=C_HEIGHT):
    """Relative bound on a float64 LU's height against the exact one: c kappa_inf(A) 2^-53."""
    return c * kappa * U53


def pitch_margin_deg(kappa, threshold_deg, c=C_HEIGHT):
    """The same bound carried to degrees at a threshold: mu = -n_y/|n| has the absolute error of n_y/|n| plus that of |n| (twice the
    height's bound, |mu| <= 1), d pitch / d mu = (180/pi) / cos(pitch); plus 1e-12 deg for the rounding of asin and of the two
    multiplications of the reference's own expression (a few ulps of 85)."""
    return 2.0 * height_bound(kappa, c) * (180.0 / np.pi) / np.cos(np.deg2rad(threshold_deg)) + 1e-12


def flag_reference(pitch, kappa):
    """(bits, decided): the mpmath verdict for bits 0/1 and, per bit, whether the row is further from the threshold than the bound."""
    bits = (pitch < LOOSE_DEG).astype(np.uint8) | ((pitch < TIGHT_DEG).astype(np.uint8) << 1)
    dec0 = np.abs(pitch - LOOSE_DEG) > pitch_margin_deg(kappa, LOOSE_DEG)
    dec1 = np.abs(pitch - TIGHT_DEG) > pitch_margin_deg(kappa, TIGHT_DEG)
    return bits, dec0, dec1


# The error of a float64 cross-product plane evaluated at a point (the kernel: e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2,
# d = -((nx x0 + ny y0) + nz z0), all four scaled by 1 / sqrt(((nx^2 + ny^2) + nz^2) + d^2), r = ((px nx + py ny) + pz nz) + d), u = 2^-53:
#   * a component of e carries a relative error u; a component of n is two products and a subtraction of such numbers:
#     |dn_i| <= 4.1 u S_i with S_i the sum of the two products' magnitudes (cancellation is what S_i / |n_i| measures);
#   * |dd| <= sum |dn_i| |p0_i| + 3.1 u sum |n_i p0_i| (three products, two additions);
#   * unnormalised, the residual at p moves by at most sum |dn_i| |p_i| + |dd|;
#   * the normaliser N = |(n, d)| moves by at most |(dn, dd)|_2, and the computed 1/N and the four scaled components add 8 u relative;
#   * the final sum of four terms adds 4.1 u (sum |p_i n_i| + |d|) / N.
# eps = [sum |dn_i| |p_i| + |dd|] / N + (|r| / N) (|(dn, dd)| / N + 8 u) + 4.1 u (sum |p_i n_i| + |d|) / N, doubled for the reference's
# own rounding (np.longdouble: 2^-64) and second-order terms.
def _plane_terms(P, triples):
    L = np.longdouble
    p0, p1, p2 = (P[triples[:, k]].astype(L) for k in range(3))
    e1, e2 = p1 - p0, p2 - p0
    a = np.stack([e1[:, 1] * e2[:, 2], e1[:, 2] * e2[:, 0], e1[:, 0] * e2[:, 1]], 1)
    b = np.stack([e1[:, 2] * e2[:, 1], e1[:, 0] * e2[:, 2], e1[:, 1] * e2[:, 0]], 1)
    n = a - b
    dn = L(4.1 * U53) * (np.abs(a) + np.abs(b))
    d = -np.sum(n * p0, 1)
    dd = np.sum(dn * np.abs(p0), 1) + L(3.1 * U53) * np.sum(np.abs(n * p0), 1)
    N = np.sqrt(np.sum(n * n, 1) + d * d)
    return n, d, dn, dd, N


def plane_ld(P, triple):
    """Unit 4-vector (n, d) / |(n, d)| with n_y >= 0 of the plane through three vertices in np.longdouble, and the bound on a float64
    cross-product plane's components against it."""
    n, d, dn, dd, N = _plane_terms(P, np.asarray(triple).reshape(1, 3))
    m = np.concatenate([n[0], d]) / N[0]
    err = np.sqrt(np.sum(dn[0] ** 2) + dd[0] ** 2) / N[0]
    tol = 2.0 * float(2 * err + 8 * U53)
    return (m if m[1] >= 0 else -m), tol


def count_bounds(P, ids, triples, threshold=THRESHOLD, chunk=32):
    """Per hypothesis (a vertex triple) the number of list entries (`ids`, repeats counted) whose distance from its plane is
    < threshold - eps and < threshold + eps.  A triple that names one vertex twice has the zero normal (an exactly zero cross
    product): NaN model, count 0."""
    L = np.longdouble
    triples = np.asarray(triples).reshape(-1, 3)
    uniq, mult = np.unique(np.asarray(ids), return_counts=True)
    Q = P[uniq].astype(L)
    lo, hi = np.zeros(len(triples), np.int64), np.zeros(len(triples), np.int64)
    for s in range(0, len(triples), chunk):
        tr = triples[s:s + chunk]
        n, d, dn, dd, N = _plane_terms(P, tr)
        with np.errstate(all="ignore"):
            r = np.abs(Q @ n.T + d[None, :]) / N[None, :]
            eps = (np.abs(Q) @ dn.T + dd[None, :]) / N[None, :] + r * (np.sqrt(np.sum(dn * dn, 1) + dd * dd) / N + 8 * U53)[None, :] \
                + L(4.1 * U53) * (np.abs(Q) @ np.abs(n).T + np.abs(d)[None, :]) / N[None, :]
            eps = 2 * eps
            a = np.where(r < threshold - eps, mult[:, None], 0).sum(0)
            b = np.where(~(r >= threshold + eps), mult[:, None], 0).sum(0)          # (an undecidable NaN counts for the upper bound)
        rep = (tr[:, 0] == tr[:, 1]) | (tr[:, 0] == tr[:, 2]) | (tr[:, 1] == tr[:, 2])
        lo[s:s + chunk], hi[s:s + chunk] = np.where(rep, 0, a), np.where(rep, 0, b)
    return lo, hi


def replay(counts, M, goal_fraction=GOAL):
    """ransac.py:9-22 on given inlier counts: strictly larger replaces the best; stop at the first new best above the goal.
    -> (best hypothesis or -1, best_ic, used)"""
    goal = float(M) * goal_fraction
    best, best_ic = -1, 0
    for h, c in enumerate(counts):
        if c > best_ic:
            best, best_ic = h, int(c)
            if c > goal:
                return best, best_ic, h + 1
    return best, best_ic, len(counts)


def point_list(frame, fl):
    """rescale.py:101: the kept rows' vertices in row order."""
    return frame.tri[(fl & 4) != 0].reshape(-1)


# ---- launchers (GPU) ----------------------------------------------------------------------------------------------------------
def _batch(ctx, frames, compact):
    from mvoscalerecovery_amd import _lib
    pts = [(f.survivors() if compact else f.xyz) for f in frames]
    cnt = np.array([len(p) for p in pts], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    allp = np.concatenate(pts) if len(pts) else np.zeros((0, 3))
    tcnt = np.array([len(f.tri) for f in frames], dtype=np.int64)
    toff = np.concatenate([[0], np.cumsum(tcnt)]).astype(np.int64)
    rows = np.concatenate([f.tri for f in frames]).astype(np.int32)
    d = {"off": ctx.to_device(off), "cnt": ctx.to_device(cnt), "toff": ctx.to_device(toff), "tri": ctx.to_device(rows.reshape(-1)),
         "x": ctx.to_device(allp[:, 0].copy()), "y": ctx.to_device(allp[:, 1].copy()), "z": ctx.to_device(allp[:, 2].copy())}
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt = len(frames), d["off"].ptr, d["cnt"].ptr
    b.x, b.y, b.z, b.v = d["x"].ptr, d["y"].ptr, d["z"].ptr, d["x"].ptr
    b.tri1_off, b.tri1, b.tri2_off, b.tri2 = d["toff"].ptr, d["tri"].ptr, d["toff"].ptr, d["tri"].ptr
    b.max_feat, b.total_feat = int(cnt.max()), int(off[-1])
    return b, d, toff, int(tcnt.max())


def _split(arr, toff):
    return [arr[toff[i]:toff[i + 1]] for i in range(len(toff) - 1)]


def _free(bufs):
    for v in bufs:
        v.free()


def _alloc(ctx, spec, sentinel):
    """Output buffers, name -> (shape, dtype).  sentinel None: zeros.  Else every byte is `sentinel` and every buffer has one more
    leading element than the launch may write: the guard."""
    o = {}
    for k, (shape, dt) in spec.items():
        shape = shape if isinstance(shape, tuple) else (shape,)
        o[k] = ctx.zeros(shape, dt) if sentinel is None else ctx.empty((shape[0] + 1,) + shape[1:], dt).fill(sentinel)
    return o


def _tails(r, lead):
    """What lies behind the last element a launch may write, per output (lead: name -> elements it may write)."""
    return {k: v[lead[k]:] for k, v in r.items()}


def all_bytes(a, byte):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == byte))


def run_stage(ctx, frames, height_factor=0.9, max_feat=None, max_tri=None, sentinel=None):
    """mvosr_flat_selection_batch over `frames` (survivors compacted on the host, as its header says) -> one dict per frame.
    max_feat / max_tri: what the header and the call state (None: the largest frame's).  sentinel: the outputs are pre-filled
    with that byte and carry one guard element each; -> (one dict per frame, the guards)."""
    from mvoscalerecovery_amd import _lib
    b, d, toff, true_max_tri = _batch(ctx, frames, compact=True)
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    max_tri = true_max_tri if max_tri is None else int(max_tri)
    F, T = len(frames), max(int(toff[-1]), 1)
    o = _alloc(ctx, {"tri_height": (T, np.float64), "tri_flags": (T, np.uint8), "height_level": (F, np.float64),
                     "n_kept": (F, np.int32), "status": (F, np.int32)}, sentinel)
    _lib.check(ctx.lib.mvosr_flat_selection_batch(ctx.handle, C.byref(b), LOOSE_DEG, TIGHT_DEG, float(height_factor), o["tri_height"].ptr,
                                                  o["tri_flags"].ptr, o["height_level"].ptr, o["n_kept"].ptr, o["status"].ptr, max_tri),
               "mvosr_flat_selection_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    _free(list(o.values()) + list(d.values()))
    hs, fs = _split(r["tri_height"], toff), _split(r["tri_flags"], toff)
    res = [{"tri_height": hs[i], "tri_flags": fs[i], "height_level": r["height_level"][i], "n_kept": int(r["n_kept"][i]),
            "status": int(r["status"][i])} for i in range(F)]
    if sentinel is None:
        return res
    return res, _tails(r, {k: (int(toff[-1]) if k.startswith("tri_") else F) for k in r})


def run_dev(ctx, frames, height_factor=0.9, n_hyp=100, use_keep=True, id_triples=None, frame_ids=None, seed=5, frame_base=0,
            min_points=MIN_POINTS, threshold=THRESHOLD, goal=GOAL, max_feat=None, max_tri=None, sentinel=None):
    """mvosr_flat_ransac_batch over `frames` with tri_height, tri_flags and hyp_counts requested.  use_keep: the frames' keep
    words are passed (frames without them: all ones) — else the survivors are compacted on the host and keep is NULL.
    id_triples: per frame an (n_hyp, 3) array of survivor-numbered vertex ids, or None for the drawn path.
    max_feat / max_tri / sentinel: as run_stage."""
    from mvoscalerecovery_amd import _lib
    b, d, toff, true_max_tri = _batch(ctx, frames, compact=not use_keep)
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    max_tri = true_max_tri if max_tri is None else int(max_tri)
    F, T, H = len(frames), max(int(toff[-1]), 1), int(n_hyp)
    extra = []
    keep_ptr = tr_ptr = ids_ptr = None
    if use_keep:
        words = np.concatenate([(f.keep if f.keep is not None else np.ones(len(f.xyz), np.int32)) for f in frames]).astype(np.int32)
        extra.append(ctx.to_device(words))
        keep_ptr = extra[-1].ptr
    if id_triples is not None:
        extra.append(ctx.to_device(np.ascontiguousarray(np.stack([np.asarray(t, dtype=np.int32).reshape(H, 3) for t in id_triples]))))
        tr_ptr = extra[-1].ptr
    if frame_ids is not None:
        extra.append(ctx.to_device(np.asarray(frame_ids, dtype=np.int64)))
        ids_ptr = extra[-1].ptr
    o = _alloc(ctx, {"raw_scale": (F, np.float64), "height_level": (F, np.float64), "model": ((F, 4), np.float64),
                     "best_ic": (F, np.int32), "used": (F, np.int32), "n_kept": (F, np.int32), "status": (F, np.int32),
                     "tri_height": (T, np.float64), "tri_flags": (T, np.uint8), "hyp_counts": ((F, H), np.int32)}, sentinel)
    if sentinel is None:
        o["hyp_counts"].fill(0xFF)
    ro = _lib.RescaleOutputs(*[o[k].ptr for k in ("raw_scale", "height_level", "model", "best_ic", "used", "n_kept", "status",
                                                   "tri_height", "tri_flags", "hyp_counts")])
    rp = _lib.RescaleParams(0, 10, LOOSE_DEG, TIGHT_DEG, float(height_factor), int(min_points), H, float(threshold), float(goal),
                            ABS_REF, int(seed), int(frame_base))
    _lib.check(ctx.lib.mvosr_flat_ransac_batch(ctx.handle, C.byref(b), keep_ptr, C.byref(rp), tr_ptr, ids_ptr, None, C.byref(ro), max_tri),
               "mvosr_flat_ransac_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    _free(list(o.values()) + list(d.values()) + extra)
    hs, fs = _split(r["tri_height"], toff), _split(r["tri_flags"], toff)
    res = [{"tri_height": hs[i], "tri_flags": fs[i], "height_level": r["height_level"][i], "n_kept": int(r["n_kept"][i]),
            "status": int(r["status"][i]), "raw_scale": r["raw_scale"][i], "model": r["model"][i], "best_ic": int(r["best_ic"][i]),
            "used": int(r["used"][i]), "hyp_counts": r["hyp_counts"][i]} for i in range(F)]
    if sentinel is None:
        return res
    return res, _tails(r, {k: (int(toff[-1]) if k.startswith("tri_") else F) for k in r})


def max_points(ctx):
    """ScaleEstimator._max_points() of the device-resident estimator on this device."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    return int(ScaleEstimator(ABS_REF, window_size=5, ransac_seed=1, delaunay_workers=0)._max_points())


# ---- the vote's keep words (mvosr_graph_keep_batch) ---------------------------------------------------------------------------
def _passing_exactly(target, seed):
    """Disjoint triangles (every vertex on one row: it passes iff its marginal under the row's edge code is > 0.6) collected until
    exactly `target` vertices pass."""
    from oracle import rescale_oracle as ro
    rng = np.random.default_rng(seed)
    v, z, have = [], [], 0
    for _ in range(4000):
        tv, tz = rng.uniform(0, 100, 3), rng.uniform(1, 50, 3)
        p = int(ro.graph_inliers(tv, tz, np.array([[0, 1, 2]]))[0].sum())
        if have + p <= target and (p or len(v) < 6):
            v.append(tv)
            z.append(tz)
            have += p
        if have == target and len(v) >= 8:
            break
    assert have == target
    v, z = np.concatenate(v), np.concatenate(z)
    return v, z, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def graph_cases():
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(95)
    cases = []

    def add(name, v, z, tri, declined=False):
        cases.append({"name": name, "v": np.asarray(v, np.float64), "z": np.asarray(z, np.float64),
                      "tri": np.asarray(tri, np.int32).reshape(-1, 3), "declined": declined})

    uv = rng.uniform(0, 100, (80, 2))
    tri = Delaunay(uv).simplices
    add("random", uv[:, 1], rng.uniform(1, 50, 80), tri)
    add("random_declined", uv[:, 1], rng.uniform(1, 50, 80), tri, declined=True)
    # equal v, equal z (products exactly +0 or -0), differences whose product underflows to -0.0, and a vertex on no row
    v = np.round(uv[:, 1] / 20.0) * 20.0
    z = np.round(rng.uniform(1, 50, 80) / 10.0) * 10.0
    v[:6] = [0.0, 1e-200, 2e-200, 0.0, 1e-200, 3e-200]
    z[:6] = [3e-200, 2e-200, 1e-200, 1e-200, 1e-200, 0.0]
    rows = np.concatenate([tri, [[0, 1, 2], [3, 4, 5], [0, 4, 2], [1, 3, 5]]])
    add("ties_and_minus_zero", np.append(v, 7.0), np.append(z, 7.0), rows)
    for target in (10, 11):
        add("exactly_%d" % target, *_passing_exactly(target, 96 + target))
    return cases


def run_graph(ctx, cases, min_valid=10, max_feat=None, sentinel=None):
    """mvosr_graph_keep_batch and mvosr_graph_inliers_batch over the cases as one batch -> per case keep, n_valid, total, good and
    the two calls' status words.  max_feat: what the header states (None: the largest frame's).  sentinel: the outputs are
    pre-filled with that byte and carry one guard element each; -> (one dict per case, the guards)."""
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.rescale import good_bits
    cnt = np.array([len(c["v"]) for c in cases], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(c["tri"]) for c in cases])]).astype(np.int64)
    d = [ctx.to_device(off), ctx.to_device(cnt), ctx.to_device(np.concatenate([c["z"] for c in cases])),
         ctx.to_device(np.concatenate([c["v"] for c in cases])), ctx.to_device(toff),
         ctx.to_device(np.concatenate([c["tri"] for c in cases]).astype(np.int32).reshape(-1)),
         ctx.to_device(np.array([7 if c["declined"] else 0 for c in cases], dtype=np.int32))]
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.z, b.v, b.x, b.y = len(cases), d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[2].ptr, d[2].ptr
    b.tri1_off, b.tri1, b.max_feat, b.total_feat = d[4].ptr, d[5].ptr, int(cnt.max() if max_feat is None else max_feat), int(off[-1])
    N, F = int(off[-1]), len(cases)
    o = _alloc(ctx, {"keep": (N, np.int32), "n_valid": (F, np.int32), "status": (F, np.int32), "total": (N, np.int32), "good": (N, np.int32),
                     "status_inliers": (F, np.int32)}, sentinel)
    if sentinel is None:
        o["keep"].fill(0x55)
        o["n_valid"].fill(0x55)
    bits = C.c_uint32(good_bits())
    _lib.check(ctx.lib.mvosr_graph_keep_batch(ctx.handle, C.byref(b), bits, int(min_valid), d[6].ptr, o["keep"].ptr, o["n_valid"].ptr,
                                              o["status"].ptr), "mvosr_graph_keep_batch")
    _lib.check(ctx.lib.mvosr_graph_inliers_batch(ctx.handle, C.byref(b), bits, o["total"].ptr, o["good"].ptr, o["status_inliers"].ptr),
               "mvosr_graph_inliers_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    _free(list(o.values()) + d)
    res = [{"keep": r["keep"][off[i]:off[i + 1]], "n_valid": int(r["n_valid"][i]), "total": r["total"][off[i]:off[i + 1]],
            "good": r["good"][off[i]:off[i + 1]], "status": int(r["status"][i]), "status_inliers": int(r["status_inliers"][i])} for i in range(F)]
    if sentinel is None:
        return res
    return res, _tails(r, {k: (N if k in ("keep", "total", "good") else F) for k in r})
