"""Crafted point sets for the three triangulators (delaunay_kernel, qhull_rows_kernel, mvosr_qhull_rows_host) — sets that sit ON
their decline bands —, an exact verifier for any (T, 3) rows, and the class of every case, computed on the CPU.

The contract of all three is "SciPy's rows, or DECLINED, never guessed".  Inside Qhull's merge band SciPy's rows are not the Delaunay
triangulation, so SciPy alone cannot say whether accepted rows are right: ``defects`` decides that in exact arithmetic.

Plain Python + NumPy + SciPy; no GPU.  tests/test_delaunay_cases.py checks this file, tests/test_gpu_delaunay_cases.py uses it."""
import functools
from fractions import Fraction

import numpy as np

# the image box the frames live in (the lower part of a 1241 x 376 image)
BOX_LO = np.array([0.0, 186.0])
BOX_HI = np.array([1241.0, 376.0])

K_TIE_TOL = 1e-9          # kDtTieTol (csrc/mvosr_delaunay.hip)
K_COL_TOL = 1e-12         # kDtColTol
DT_LANE_DEG, DT_LANE_ROWS, DT_WAVE_DEG, DT_WAVE_ROWS = 24, 12, 60, 32
DT_WHY_DUP, DT_WHY_TIE, DT_WHY_COLLINEAR, DT_WHY_DEGREE, DT_WHY_ROWS, DT_WHY_EULER, DT_WHY_HARD, DT_WHY_SIZE = 1, 2, 4, 8, 16, 32, 64, 128


class Case:
    """One frame: ``points`` (n, 2) float64, ``crafted`` = ids of the sites of the crafted neighbourhood, ``keep`` = None or the vote
    of an ``unmask`` case (int32, >= 0 stays), ``params`` = what built it."""

    def __init__(self, family, name, points, crafted, keep=None, **params):
        self.family, self.name, self.points, self.crafted, self.keep, self.params = family, name, np.ascontiguousarray(points), np.asarray(crafted), keep, params

    def survivors(self):
        """(points, crafted) of what is triangulated: all of it, or the sites the mask keeps under their ranks."""
        if self.keep is None:
            return self.points, self.crafted
        kept = self.keep >= 0
        rank = np.cumsum(kept) - 1
        return np.ascontiguousarray(self.points[kept]), rank[self.crafted[kept[self.crafted]]]

    def __repr__(self):
        return "<%s>" % self.name


# ---------------------------------------------------------------------------------------------------------------- exact arithmetic

def exact_ints(points):
    """The doubles as exact integers over one common power-of-two denominator (Fraction(x) is the double's value)."""
    fr = [(Fraction(float(x)), Fraction(float(y))) for x, y in np.asarray(points, dtype=np.float64)]
    den = 1
    for fx, fy in fr:
        den = max(den, fx.denominator, fy.denominator)
    return [(int(fx * den), int(fy * den)) for fx, fy in fr]


def _orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _incircle(a, b, c, d):
    """> 0: d strictly inside the circle through a, b, c given COUNTER-CLOCKWISE; 0: on it."""
    ax, ay, bx, by, cx, cy = a[0] - d[0], a[1] - d[1], b[0] - d[0], b[1] - d[1], c[0] - d[0], c[1] - d[1]
    a2, b2, c2 = ax * ax + ay * ay, bx * bx + by * by, cx * cx + cy * cy
    return ax * (by * c2 - b2 * cy) - ay * (bx * c2 - b2 * cx) + a2 * (bx * cy - by * cx)


def exact_hull(P):
    """The convex hull of integer points as a cycle of ids, sites ON a hull edge included (Qhull's 'Qt' rows keep them as
    vertices on the boundary), counter-clockwise.  Repeated sites appear once."""
    ids = sorted(range(len(P)), key=lambda i: P[i])
    ids = [i for k, i in enumerate(ids) if k == 0 or P[i] != P[ids[k - 1]]]
    if len(ids) < 3:
        return ids

    def half(seq):
        h = []
        for i in seq:
            while len(h) >= 2 and _orient(P[h[-2]], P[h[-1]], P[i]) < 0:
                h.pop()
            h.append(i)
        return h
    lo, up = half(ids), half(ids[::-1])
    return lo[:-1] + up[:-1]


def defects(points, rows):
    """Exact check of (T, 3) rows over ``points``.  Returns a dict: ``structure`` — a list of what is wrong with the rows as a
    triangulation of ALL the sites (a zero-area row, an id out of range, an edge in more than two rows, a wrong row count, a boundary
    that is not the exact convex hull, a site in no row); ``non_delaunay`` — interior edges whose opposite apex is strictly inside
    the circumcircle; ``ties`` — interior edges with that determinant exactly 0; ``clean`` — nothing at all: the rows are THE
    Delaunay triangulation."""
    P = exact_ints(points)
    n = len(P)
    rows = np.asarray(rows).reshape(-1, 3)
    bad = []
    edges = {}
    used = set()
    for r, (a, b, c) in enumerate(rows.tolist()):
        if not (0 <= a < n and 0 <= b < n and 0 <= c < n) or len({a, b, c}) < 3:
            bad.append("row %d: ids %s" % (r, (a, b, c)))
            continue
        if _orient(P[a], P[b], P[c]) == 0:
            bad.append("row %d: zero area" % r)
        used.update((a, b, c))
        for x, y, z in ((a, b, c), (b, c, a), (c, a, b)):
            edges.setdefault((min(x, y), max(x, y)), []).append(z)
    hull = exact_hull(P)
    h = len(hull)
    if len(rows) != 2 * n - 2 - h:
        bad.append("%d rows, 2n - 2 - h = %d (n %d, h %d)" % (len(rows), 2 * n - 2 - h, n, h))
    if len(used) != n:
        bad.append("%d sites in no row" % (n - len(used)))
    for e, ap in edges.items():
        if len(ap) > 2:
            bad.append("edge %s in %d rows" % (e, len(ap)))
    boundary = {e for e, ap in edges.items() if len(ap) == 1}
    want = {(min(hull[k], hull[(k + 1) % h]), max(hull[k], hull[(k + 1) % h])) for k in range(h)} if h >= 3 else set()
    if boundary != want:
        bad.append("boundary differs from the exact hull in %d edges" % len(boundary ^ want))
    non_delaunay = ties = 0
    for (p, q), ap in edges.items():
        if len(ap) != 2:
            continue
        a, b = ap
        o = _orient(P[p], P[q], P[a])
        if o == 0 or _orient(P[p], P[q], P[b]) == 0:
            continue                                                   # (a zero-area row: already reported)
        d = _incircle(P[p], P[q], P[a], P[b]) * (1 if o > 0 else -1)
        if d > 0:
            non_delaunay += 1
        elif d == 0:
            ties += 1
    return dict(structure=bad, non_delaunay=non_delaunay, ties=ties, clean=not bad and non_delaunay == 0 and ties == 0)


# ------------------------------------------------------------------------------------------------------- margins, in float64

def cot_gap(points, rows, crafted):
    """See :func:`margins` — its first value."""
    return margins(points, rows, crafted)[0]


def power_gap(points, rows, crafted):
    """See :func:`margins` — its second value."""
    return margins(points, rows, crafted)[1]


def qhull_band(points):
    """delaunay_kernel's absolute tie band of a frame (dt_qhull_band, csrc/mvosr_delaunay.hip), in px^2: 64 DISTround of Qhull's run
    on these sites, taken from the lifted and 'Qbb'-scaled space back to the power of a site with respect to a circle whose centre
    lies within the sites' range."""
    p = np.asarray(points, dtype=np.float64)
    mx, my = float(np.abs(p[:, 0]).max()), float(np.abs(p[:, 1]).max())
    maxabs = max(mx, my)
    maxdistsum = min(np.sqrt(3.0) * maxabs, mx + my + maxabs)
    distround = 2.220446049250313e-16 * (3 * maxdistsum * 1.01 + maxabs)
    d2 = mx * mx + my * my
    inv_scale = 1.1 * d2 / maxabs
    return 64.0 * distround * float(np.sqrt(inv_scale * inv_scale + 4.0 * d2))


def margins(points, rows, crafted):
    """(cot gap, power gap).  Cot gap: the smallest relative difference |t1 - t2| / (min(|t1|, |t2|) + 1) between the cot under which the APEX of a row sees one of
    the row's edges and the cot under which another site of the crafted neighbourhood on the same side of that edge sees it — the
    quantity kDtTieTol bounds, formed in float64 as dt_confirm_tie forms it (b = c - p, cr = sgn cross(a, b), num = |b|^2 - b.a,
    t = num / cr).  Power gap: over the same pairs, the smallest |t1 - t2| cr of the other site — the power of that site with respect
    to the circle through the row's three sites, in px^2: what the kernel's absolute band (:func:`qhull_band`) bounds.  Over the edges
    of the rows that touch the crafted neighbourhood (an end or the apex in it).  They CLASSIFY cases (how far from the bands?);
    they are no reference for results.  inf: no such pair."""
    pts = np.asarray(points, dtype=np.float64)
    rows = np.asarray(rows).reshape(-1, 3)
    crafted = np.asarray(crafted)
    if len(rows) == 0 or len(crafted) == 0:
        return np.inf, np.inf
    inc = np.zeros(len(pts), bool)
    inc[crafted] = True
    e = np.concatenate([rows[:, [0, 1, 2]], rows[:, [1, 2, 0]], rows[:, [2, 0, 1]]])         # (p, q, apex)
    e = e[inc[e].any(axis=1)]
    if len(e) == 0:
        return np.inf, np.inf
    p, q, ap = pts[e[:, 0]], pts[e[:, 1]], pts[e[:, 2]]
    a = q - p

    def cot(c):                                                     # c: (E, C, 2) candidates against E edges
        b = c - p[:, None, :]
        cr = a[:, None, 0] * b[..., 1] - a[:, None, 1] * b[..., 0]
        b2 = b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]
        num = b2 - (b[..., 0] * a[:, None, 0] + b[..., 1] * a[:, None, 1])
        return num, cr, b2
    n1, c1, _ = cot(ap[:, None, :])
    sgn = np.where(c1 >= 0, 1.0, -1.0)
    c1 = c1 * sgn
    num, cr, b2 = cot(np.broadcast_to(pts[crafted][None, :, :], (len(e), len(crafted), 2)))
    cr = cr * sgn
    a2 = (a * a).sum(axis=1)[:, None]
    other = (crafted[None, :] != e[:, 0:1]) & (crafted[None, :] != e[:, 1:2]) & (crafted[None, :] != e[:, 2:3])
    ok = other & (cr > 0) & (cr * cr > (K_COL_TOL * K_COL_TOL) * a2 * b2) & (c1 > 0)
    with np.errstate(all="ignore"):
        t1, t2 = n1 / c1, num / cr
        gap = np.abs(t1 - t2) / (np.minimum(np.abs(t1), np.abs(t2)) + 1.0)
        power = np.abs(t1 - t2) * cr
    return float(np.where(ok, gap, np.inf).min()), float(np.where(ok, power, np.inf).min())


def collinear_margin(points, crafted):
    """The smallest |cross(a, b)| / (|a| |b|) over the site triples of the crafted neighbourhood (a, b: two sites seen from the
    third) — what kDtColTol bounds.  0 for a repeated site.  inf with fewer than three crafted sites."""
    c = np.asarray(points, dtype=np.float64)[np.asarray(crafted)]
    m = len(c)
    if m < 3:
        return np.inf
    best = np.inf
    for i in range(m):
        d = c - c[i]
        d = np.delete(d, i, axis=0)
        nrm = np.hypot(d[:, 0], d[:, 1])
        cr = np.abs(d[:, None, 0] * d[None, :, 1] - d[:, None, 1] * d[None, :, 0])
        with np.errstate(all="ignore"):
            r = cr / (nrm[:, None] * nrm[None, :])
        r[np.isnan(r)] = 0.0
        r[np.arange(m - 1), np.arange(m - 1)] = np.inf
        best = min(best, float(r.min()))
    return best


# ------------------------------------------------------------------------------------------------------------------- builders

def _background(rng, n_bg, centre, clear, lo=BOX_LO, hi=BOX_HI):
    """n_bg uniform sites of the box, none within ``clear`` of ``centre``."""
    out = np.zeros((0, 2))
    while len(out) < n_bg:
        p = rng.uniform(lo, hi, (2 * n_bg, 2))
        out = np.concatenate([out, p[np.hypot(*(p - centre).T) > clear]])
    return out[:n_bg]


def _assemble(rng, family, name, bg, crafted_pts, first=None, last=None, **params):
    """Background + crafted sites in an order permuted by the seed; ``first`` / ``last``: the crafted site that gets id 0 / n - 1."""
    pts = np.concatenate([bg, crafted_pts])
    n, m = len(pts), len(crafted_pts)
    perm = rng.permutation(n)
    pin = first if first is not None else last
    if pin is not None:
        src = len(bg) + pin
        perm = perm[perm != src]
        perm = np.concatenate([[src], perm]) if first is not None else np.concatenate([perm, [src]])
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    return Case(family, name, pts[perm], inv[len(bg):len(bg) + m], **params)


def _centre(rng):
    return np.array([rng.uniform(300.0, 900.0), rng.uniform(270.0, 292.0)])


def ring(R, k, eps, seed, n_bg=130):
    """k sites on a circle of radius R (evenly spaced from a random phase, each angle moved by up to a fifth of the spacing), each
    radius multiplied by 1 + eps U(-1, 1), in n_bg uniform sites none of which is within R + 20 px of the centre."""
    rng = np.random.default_rng([11, seed, k, int(round(R * 100)), int(round(-np.log10(eps) * 10)) if eps > 0 else 999])
    c = _centre(rng)
    th = rng.uniform(0, 2 * np.pi) + (np.arange(k) + rng.uniform(-0.2, 0.2, k)) * (2 * np.pi / k)
    r = R * (1.0 + eps * rng.uniform(-1, 1, k))
    crafted = c + np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    return _assemble(rng, "ring", "ring R=%g k=%d eps=%g s=%d" % (R, k, eps, seed), _background(rng, n_bg, c, R + 20.0), crafted,
                     R=R, k=k, eps=eps, seed=seed)


def rect(eps, seed, n_bg=130):
    """An integer rectangle (exactly cocircular corners) with one corner moved outwards by eps * 40 px: an exact tie at eps = 0."""
    rng = np.random.default_rng([12, seed, int(round(-np.log10(eps) * 10)) if eps > 0 else 999])
    c = np.floor(_centre(rng))
    crafted = c + np.array([[-16.0, -12.0], [16.0, -12.0], [16.0, 12.0], [-16.0, 12.0]])
    crafted[2] += eps * 40.0 * np.array([0.8, 0.6])
    return _assemble(rng, "ring", "rect eps=%g s=%d" % (eps, seed), _background(rng, n_bg, c, 40.0), crafted, R=20.0, k=4, eps=eps,
                     seed=seed, rect=True)


def hub(k, first, seed=0, n_bg=150, R=30.0):
    """One site at the centre of a ring of k sites: its star degree is k.  The radii differ by +-2 % — or, where a ring site 2 %
    further out would lose its edge to the hub (the chord of its neighbours passes inside it: 1 - cos(2 pi / k) < 4 %), by a
    quarter of that sagitta: 0.12 % at k = 64, still a million times every band.  first: the hub is site 0 and owns all k rows (a
    row is written by its smallest id); otherwise it is the last site and owns none."""
    rng = np.random.default_rng([13, seed, k, int(first)])
    c = _centre(rng)
    amp = min(0.02, 0.25 * (1.0 - np.cos(2 * np.pi / k)))
    th = rng.uniform(0, 2 * np.pi) + (np.arange(k) + rng.uniform(-0.1, 0.1, k)) * (2 * np.pi / k)
    r = R * (1.0 + amp * rng.uniform(-1, 1, k))
    crafted = np.concatenate([c + np.stack([r * np.cos(th), r * np.sin(th)], axis=1), [c]])
    return _assemble(rng, "hub", "hub k=%d %s" % (k, "first" if first else "last"), _background(rng, n_bg, c, R + 20.0), crafted,
                     first=k if first else None, last=None if first else k, k=k, first_id=bool(first), seed=seed)


def hull_line(m, eps, seed=0, n_bg=130):
    """m sites on a line below (v smaller than) all others, from u = 100 to 1100 (span 1000); the inner ones moved off it by
    +-eps * span (times a weight of 0.45 to 1 per site), alternately outwards (a hull vertex) and inwards (a site next to a hull
    edge)."""
    rng = np.random.default_rng([14, seed, m, int(round(-np.log10(eps) * 10)) if eps > 0 else 999])
    span = 1000.0
    crafted = np.stack([100.0 + span * np.arange(m) / (m - 1), np.full(m, 180.0)], axis=1)
    weight = np.array([1.0, 0.7, 0.45, 0.85, 0.6])[:m - 2]       # (unequal: no three of the moved sites on a line of their own)
    crafted[1:-1, 1] += eps * span * weight * np.where(np.arange(1, m - 1) % 2, -1.0, 1.0)
    bg = rng.uniform(BOX_LO + [0, 4], BOX_HI, (n_bg, 2))
    return _assemble(rng, "hull_line", "hull_line m=%d eps=%g" % (m, eps), bg, crafted, m=m, eps=eps, seed=seed)


def segment(eps, seed=0, n_bg=130):
    """A site on the segment between two interior neighbours 10 px apart (exact coordinates), moved off it by eps px (sign by seed):
    the candidate on the segment p..q of dt_step<true> (flag & 1)."""
    rng = np.random.default_rng([15, seed, int(round(-np.log10(eps) * 10)) if eps > 0 else 999])
    c = np.floor(_centre(rng))
    crafted = np.array([c + [-4.0, -3.0], c + [4.0, 3.0], c])
    crafted[2] += eps * np.array([-0.6, 0.8]) * (1.0 if seed % 2 == 0 else -1.0)
    return _assemble(rng, "segment", "segment eps=%g s=%d" % (eps, seed), _background(rng, n_bg, c, 25.0), crafted, eps=eps, seed=seed)


def twins(eps, seed=0, n_bg=130):
    """Two sites eps px apart (eps = 0: a repeated site)."""
    rng = np.random.default_rng([16, seed, int(round(-np.log10(eps) * 10)) if eps > 0 else 999])
    c = _centre(rng)
    crafted = np.array([c, c + [eps, 0.0]])
    return _assemble(rng, "twins", "twins eps=%g s=%d" % (eps, seed), _background(rng, n_bg, c, 20.0), crafted, eps=eps, seed=seed)


def unmask(family, seed=0, n_bg=150):
    """A first triangulation over a family made harmless by ONE extra site, and a vote that takes that site out: the second (seeded)
    triangulation meets the family itself.  "ring": a near-cocircular ring with a site in its centre; "rect": the exact rectangle
    likewise; "twins": a repeated site whose partner is voted out (the first triangulation is declined, the second is harmless);
    "segment": a site exactly on a segment, voted out."""
    base = dict(ring=lambda: ring(4.0, 12, 1e-12, 40 + seed, n_bg), rect=lambda: rect(0.0, 40 + seed, n_bg),
                twins=lambda: twins(0.0, 40 + seed, n_bg), segment=lambda: segment(0.0, 40 + seed, n_bg),
                wide=lambda: ring(40.0, 12, 1e-3, 40 + seed, n_bg))[family]()
    pts, crafted = base.points, base.crafted
    rng = np.random.default_rng([17, seed])
    keep = np.where(rng.uniform(size=len(pts) + 1) < 0.9, 2, -1).astype(np.int32)
    keep[crafted] = 1
    if family in ("ring", "rect", "wide"):
        extra = pts[crafted].mean(axis=0)
        pts = np.concatenate([pts, [extra]])
        keep[-1] = -1
        crafted_all = np.concatenate([crafted, [len(pts) - 1]])
    else:
        keep = keep[:-1]
        keep[crafted[-1]] = -1                                    # the twin's partner / the site on the segment
        crafted_all = crafted
    return Case("unmask", "unmask %s s=%d" % (family, seed), pts, crafted_all, keep=keep, of=family, seed=seed)


RING_R = (40.0, 4.0, 0.5, 0.05)
RING_K = (4, 5, 12)
EPS_LADDER = (0.0, 1e-15, 1e-12, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2)
# more seeds where SciPy's rows are not Delaunay although no candidate pair is near delaunay_kernel's relative band (small rings)
RING_EXTRA = ((0.05, 5, 1e-6), (0.05, 12, 1e-6), (0.05, 12, 1e-5), (0.5, 12, 1e-7))
RING_EXTRA_SEEDS = tuple(range(2, 14))
HUB_K = (11, 12, 13, 23, 24, 25, 31, 32, 33, 59, 60, 61, 64)
LINE_EPS = (0.0, 1e-16, 1e-14, 1e-13, 1e-12, 1e-10, 1e-8, 1e-6, 1e-3)        # (1e-14 * span = the 1e-11 px of test_delaunay_collinear_triples_on_a_pixel_grid)
SEGMENT_EPS = (0.0, 1e-13, 1e-12, 1e-11, 1e-10, 1e-8, 1e-6, 1e-3, 1e-1)
TWIN_EPS = (0.0, 1e-13, 1e-12, 1e-10, 1e-8, 1e-6, 1e-4, 1e-2)


@functools.lru_cache(maxsize=None)
def all_cases():
    """The case list, in a fixed order.  Every eighth frame has a larger background (a slice of 16 holds a frame of 256 sites and
    more: what the launcher's PARTS variant asks for)."""
    out = []

    def bg(small=130):
        return 270 if len(out) % 8 == 0 else small
    for R in RING_R:
        for k in RING_K:
            for eps in EPS_LADDER:
                for seed in (0, 1):
                    out.append(ring(R, k, eps, seed, bg()))
    for R, k, eps in RING_EXTRA:
        for seed in RING_EXTRA_SEEDS:
            out.append(ring(R, k, eps, seed, bg()))
    for eps in EPS_LADDER:
        out.append(rect(eps, 0, bg()))
    for k in HUB_K:
        for first in (True, False):
            out.append(hub(k, first, 0, bg(150)))
    for m in (3, 7):
        for eps in LINE_EPS:
            out.append(hull_line(m, eps, 0, bg()))
    for eps in SEGMENT_EPS:
        for seed in (0, 1):
            out.append(segment(eps, seed, bg()))
    for eps in TWIN_EPS:
        out.append(twins(eps, 0, bg()))
    for fam in ("ring", "rect", "twins", "segment", "wide"):
        out.append(unmask(fam, 0, bg(150)))
    return tuple(out)


# --------------------------------------------------------------------------------------------------------------------- classes

MUST_ACCEPT, SCIPY_NOT_DELAUNAY, FREE = "must_accept", "scipy_not_delaunay", "free"

# mvosr_qhull_rows_host's decline reasons (csrc/mvosr_qhull_host.c) and what oracle/qhull_rows.py says at the same decision
HOST_REASON_TEXT = {1: "need (n >= 3, 2) points", 2: "zero width", 3: "flat initial simplex", 4: "narrow initial simplex", 5: "one extreme point",
                    6: "initial simplex needs the all-points search", 7: "degenerate facet", 8: "near-zero pivot",
                    9: "point within roundoff of an initial facet", 10: "points inside the initial simplex",
                    11: "partition decision within roundoff", 12: "point above no facet", 13: "visibility within roundoff",
                    14: "coplanar horizon", 15: "open cone", 16: "cone not strictly convex (merge)"}

# The decisions of one Qhull run under the names both replays can be held to.  The host replay takes a run's decisions one after the
# other and names the band it stopped in; the device replay takes a wavefront's at once and has ONE name for "a distance inside the
# guard band" (QH_BAND) and one for an unusable plane (QH_GAUSS).  Capacity: the device's tables of 64 entries per insertion
# (kQhTab), its facet and arena slices; the host's rows buffer.
HOST_REASON_KIND = {0: "ok", 1: "few", 2: "width", 5: "width", 3: "simplex", 4: "simplex", 6: "simplex", 7: "plane", 8: "plane", 9: "band",
                    11: "band", 13: "band", 10: "inside", 12: "above", 14: "horizon", 15: "cone", 16: "cone", 17: "capacity"}
DEVICE_REASON_KIND = {0: "ok", 1: "few", 2: "width", 3: "simplex", 4: "simplex", 5: "simplex", 6: "inside", 7: "band", 8: "horizon",
                      9: "capacity", 10: "capacity", 11: "cone", 12: "cone", 13: "plane", 14: "sharp", 15: "above", 16: "capacity",
                      17: "capacity"}


def scipy_rows(points):
    from scipy.spatial import Delaunay
    return np.ascontiguousarray(Delaunay(points).simplices, dtype=np.int32)


class Entry:
    """What the CPU knows about a case: SciPy's rows over the survivors, their exact defects, the margins, the host replay's
    decision (rows or None, reason), and the classes — ``cls`` for delaunay_kernel, ``cls_replay`` for the two Qhull replays."""


def classify(case):
    """The Entry of one case (SciPy, the exact verifier, the margins and the host replay on the survivors' set)."""
    from mvoscalerecovery_amd import packing
    e = Entry()
    e.case = case
    e.points, e.crafted = case.survivors()
    e.scipy = scipy_rows(e.points)
    e.defects = defects(e.points, e.scipy)
    e.cot_gap, e.power_gap = margins(e.points, e.scipy, e.crafted)
    e.band = qhull_band(e.points)
    e.col = collinear_margin(e.points, e.crafted)
    e.host_rows = packing.qhull_rows_host(e.points)
    e.host_reason = int(packing.qhull_rows_host.last_reason)
    # outside every band delaunay_kernel states, with room: 1000 times the two relative ones; 4 times the absolute one, which is 64
    # DISTround already and a quantity this file forms exactly as the kernel does (only rounding, ~1e-12 px^2, lies between the two)
    general = e.defects["clean"] and e.cot_gap >= 1000 * K_TIE_TOL and e.col >= 1000 * K_COL_TOL and e.power_gap >= 4 * e.band
    wrong = e.defects["non_delaunay"] > 0 or e.defects["ties"] > 0
    e.cls = MUST_ACCEPT if general else (SCIPY_NOT_DELAUNAY if wrong else FREE)
    e.cls_replay = MUST_ACCEPT if general and e.host_rows is not None else (SCIPY_NOT_DELAUNAY if wrong else FREE)
    # delaunay_kernel's structural limits (a star of more than kDtWaveDeg sites, more than kDtWaveRows rows owned by one site):
    # a hub beyond them may only be declined, whatever its margins
    e.beyond_limits = case.family == "hub" and (case.params["k"] > DT_WAVE_DEG or (case.params["first_id"] and case.params["k"] > DT_WAVE_ROWS))
    if e.beyond_limits and e.cls == MUST_ACCEPT:
        e.cls = FREE
    return e


@functools.lru_cache(maxsize=None)
def table():
    """One Entry per case of all_cases(), computed once per process."""
    return tuple(classify(case) for case in all_cases())
