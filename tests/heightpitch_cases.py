"""Frames and references for height_pitch_kernel (csrc/mvosr_heightpitch.hip) — shared by tests/test_heightpitch_cases.py (CPU),
tests/test_gpu_heightpitch.py (the device) and tests/golden/make_golden_heightpitch.py (the reference's own run).  Test infrastructure.

* `restate`: the script /root/reference/src/calculate_height_pitch.py in NumPy float64, line by line, with the sample positions
  as an input.  Its refinement takes the plane through the first three inliers as a cross product (the kernel's form; the script
  asks an SVD for the same null vector): the gap between the two on the script's own frames is what the golden stores as gap_*.
* `reference`: the same in np.longdouble with error bounds — the rows' pitches with flat_cases.pitch_margin_deg, the hypotheses'
  counts with flat_cases.count_bounds, the model with flat_cases.plane_ld, the mask with test_gpu_ransac.py's band widened by the
  model's own bound — and the assertion that every integer is DECIDED (lower and upper bound coincide).
* crafted frames: small triangles with three vertices of their own, rows given (no triangulation), inputs [u, v, depth].
"""
import zlib

import numpy as np

import flat_cases as fc
from flat_cases import U53
from oracle import rescale_oracle as ro

L = np.longdouble
FOCUS, CX, CY = 718.856, 607.1928, 185.2157        # calculate_height_pitch.py:15-17
PI_S = 3.1415926                                    # :63, :91
THRESHOLD, INLIER_THRESHOLD, GOAL, MIN_POINTS, N_HYP = 0.005, 0.01, 0.8, 12, 500    # :145, :149, estimate_road_norm.py:68, :140
ST_SINGULAR, ST_MASK, ST_EMPTY, ST_RS_FEW = 7, 8, 9, 11
N_HYPS = (1, 63, 64, 65, 500, 512)


def back_project(pts):
    p = np.array(pts, dtype=np.float64).reshape(-1, 3)                               # :66
    p[:, 0] = p[:, 2] * (p[:, 0] - CX) / FOCUS                                       # :67
    p[:, 1] = p[:, 2] * (p[:, 1] - CY) / FOCUS                                       # :68
    return p


def prior_of(est):
    import math
    deg = est * 180 / PI_S                                                           # :63
    return deg - 95, deg - 85, math.sin(est), math.cos(est)


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return int(c)


def wall_frame(seed, n):
    """[u, v, depth] of a fronto-parallel wall with 1 % depth noise: every triangle's normal points along z, pitch ~ 0 — no row
    passes the window and the list is empty (the script's `else` branch, :163-165)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.0, 1241.0, n), rng.uniform(0.0, 376.0, n), 20.0 * (1.0 + 0.01 * rng.standard_normal(n))], 1)


def motions(seed, n):
    """A synthetic motion file: rows of a 3x4 [R | t], forward motion with a little drift (the script reads columns 3, 7, 11)."""
    rng = np.random.default_rng(seed)
    m = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64), (n, 1))
    m[:, 3], m[:, 7], m[:, 11] = 0.02 * rng.standard_normal(n), 0.03 * rng.standard_normal(n), 1.0 + 0.1 * rng.standard_normal(n)
    return m


# ---- the script in float64 ------------------------------------------------------------------------------------------------
def planes_from(P, v):
    """Unit (n, d) of the planes through the vertex triples v (H, 3), as the kernels build them; a repeated vertex gives NaN."""
    p0, p1, p2 = P[v[:, 0]], P[v[:, 1]], P[v[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
    with np.errstate(all="ignore"):
        inv = 1.0 / np.sqrt(((nx * nx + ny * ny) + nz * nz) + d * d)
        m = np.stack([nx * inv, ny * inv, nz * inv, d * inv], 1)
    rep = (v[:, 0] == v[:, 1]) | (v[:, 0] == v[:, 2]) | (v[:, 1] == v[:, 2])
    m[rep] = np.nan
    return m


def residuals(P, m):
    return np.abs(((P[:, 0] * m[0] + P[:, 1] * m[1]) + P[:, 2] * m[2]) + m[3])       # estimate_road_norm.py:18, :74-75


def vertex_triples(ids, positions):
    """List positions -> vertex triples; a position outside the list gives (0, 0, 0): a repeated vertex, the spent sample."""
    pos = np.asarray(positions, dtype=np.int64).reshape(-1, 3)
    ok = np.all((pos >= 0) & (pos < len(ids)), 1)
    v = np.zeros_like(pos)
    if len(ids):
        v[ok] = np.asarray(ids, dtype=np.int64)[pos[ok]]
    return v


def select(P, rows, est):
    """:77-116 -> (keep per row, the list, pitch_deg, height).  Raises LinAlgError where the script does (:83)."""
    lo, hi = prior_of(est)[:2]
    n = np.linalg.solve(P[rows], np.ones((len(rows), 3, 1)))[:, :, 0]                # :83-84
    nn2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]                # :85
    height = 1 / np.sqrt(nn2)                                                        # :86
    flip = n[:, 1] < 0                                                               # :87-89
    n[flip], height[flip] = -n[flip], -height[flip]
    pitch_deg = np.arcsin(-n[:, 1] / np.sqrt(nn2)) * 180 / PI_S                      # :90-91
    keep = (pitch_deg > lo) & (pitch_deg < hi) & (height > 0)                        # :111-112
    return keep, rows[keep].reshape(-1), pitch_deg, height


def refine(P, mask, est):
    """:178-204 on the inliers P[mask] -> (n^, pitch, mean, std, t_mean)."""
    import math
    inl = P[mask]
    e1, e2 = inl[1] - inl[0], inl[2] - inl[0]
    n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    if n[1] < 0:                                                                     # :180-181
        n = -n
    n = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])                       # :183-185
    hs = (inl[:, 0] * n[0] + inl[:, 1] * n[1]) + inl[:, 2] * n[2]                    # :192
    t_mean = np.mean(inl[:, 2] * math.sin(est) + inl[:, 1] * math.cos(est))          # :202-203
    return n, math.asin(n[1]), np.mean(hs), np.std(hs), t_mean


def restate(pts, rows, est, positions, prev=None):
    """One pass of the script's loop body (:62-204).  positions: (H, 3) list positions (the script's random.sample, recorded).
    prev: the previous frame's dict (the carry, :163-165).  -> dict; raises IndexError on a first frame with too few points."""
    import math
    P = back_project(pts)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    keep, ids, _, _ = select(P, rows, est)
    r = {"n_selected": len(ids), "ids": ids.astype(np.int32), "carried": len(ids) < MIN_POINTS}
    if not r["carried"]:                                                             # :140
        v = vertex_triples(ids, positions)
        m = planes_from(P, v)
        Q = P[ids]
        with np.errstate(invalid="ignore"):
            counts = np.array([int(np.sum(residuals(Q, mm) < THRESHOLD)) for mm in m])   # ransac.py:12-15
        best, best_ic, used = fc.replay(counts, len(ids), GOAL)                      # ransac.py:18-22
        model = m[best] if m[best][1] >= 0 else -m[best]                             # :157-159
        r.update(hyp_counts=counts.astype(np.int32), best=best, best_ic=best_ic, used=used, model=model, vtriples=v,
                 mask=residuals(P, model) < INLIER_THRESHOLD,                        # :149
                 ransac_height=1 / (math.sqrt((model[0] * model[0] + model[1] * model[1]) + model[2] * model[2]) / -model[3]))   # :156-166
        r["inliers"] = P[r["mask"]]
    else:
        if prev is None:
            raise IndexError("too many indices for array")                           # :167 on the 1-D norm_prev of :45
        r.update(ransac_height=prev["ransac_height"], inliers=prev["inliers"], mask=None)
    inl = r["inliers"]
    nh, pitch, mean, std, t_mean = refine(inl, np.ones(len(inl), bool), est)
    r.update(n_inliers=len(inl), refined_normal=nh, refined_pitch=pitch, refined_mean=mean, refined_std=std, height_t_mean=t_mean)
    return r


# ---- np.longdouble, with bounds ---------------------------------------------------------------------------------------------
def rows_ld(P, rows):
    """Per row in np.longdouble (adjugate over determinant): signed height, n_y / |n| after the flip, pitch_deg with the script's
    constant, kappa_inf(A), and whether the determinant is exactly zero."""
    A = P[np.asarray(rows, dtype=np.int64).reshape(-1, 3)].astype(L)
    (a, b, c), (d, e, f), (g, h, i) = [[A[:, r, k] for k in range(3)] for r in range(3)]
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    c10, c11, c12 = c * h - b * i, a * i - c * g, b * g - a * h
    c20, c21, c22 = b * f - c * e, c * d - a * f, a * e - b * d
    det = a * c00 + b * c01 + c * c02
    with np.errstate(all="ignore"):
        n = np.stack([c00 + c10 + c20, c01 + c11 + c21, c02 + c12 + c22], 1) / det[:, None]
        ln = np.sqrt(np.sum(n * n, 1))
        ninv = np.max(np.stack([np.abs(c00) + np.abs(c10) + np.abs(c20), np.abs(c01) + np.abs(c11) + np.abs(c21),
                                np.abs(c02) + np.abs(c12) + np.abs(c22)]), 0) / np.abs(det)
        kappa = (np.max(np.sum(np.abs(A), 2), 1) * ninv).astype(np.float64)
        mu = -np.abs(n[:, 1]) / ln
        pitch = (np.arcsin(mu) * 180 / L(PI_S)).astype(np.float64)
        height = np.where(n[:, 1] < 0, -1 / ln, 1 / ln)
    return {"height": height, "ny_rel": (n[:, 1] / ln).astype(np.float64), "pitch": pitch, "kappa": kappa, "singular": det == 0}


def keep_bounds(P, rows, est):
    """(kept for sure, possibly kept) per row: the window test is decided when the pitch is further from an edge than
    flat_cases.pitch_margin_deg, the sign of n_y when |n_y| / |n| exceeds twice the height's bound."""
    lo, hi = prior_of(est)[:2]
    q = rows_ld(P, rows)
    with np.errstate(invalid="ignore"):
        m_lo = fc.pitch_margin_deg(q["kappa"], max(min(lo, 89.0), -89.0)), fc.pitch_margin_deg(q["kappa"], max(min(hi, 89.0), -89.0))
        in_sure = (q["pitch"] > lo + m_lo[0]) & (q["pitch"] < hi - m_lo[1])
        in_maybe = (q["pitch"] > lo - m_lo[0]) & (q["pitch"] < hi + m_lo[1])
        sgn = 2 * fc.height_bound(q["kappa"])
        return in_sure & (q["ny_rel"] > sgn), in_maybe & ~(q["ny_rel"] < -sgn), q


def asin_bound(x, delta):
    """|asin(x + delta) - asin(x - delta)| in np.longdouble, the arguments clipped to [-1, 1]."""
    x, delta = L(x), L(delta)
    return float(np.arcsin(min(x + delta, L(1))) - np.arcsin(max(x - delta, L(-1))))


def reference(pts, rows, est, positions, n_hyp=None):
    """The frame in np.longdouble -> dict of expected values and bounds; `decided`: every integer output is fixed by the bounds
    (asserted by the case generators, so a crafted or pinned frame in which rounding could decide never reaches a test)."""
    import math
    P = back_project(pts)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    sure, maybe, q = keep_bounds(P, rows, est)
    r = {"decided": bool(np.array_equal(sure, maybe)), "keep": sure, "rows_q": q}
    ids = rows[sure].reshape(-1)
    r.update(n_selected=len(ids), ids=ids.astype(np.int32))
    if not r["decided"] or len(ids) < MIN_POINTS:
        r["status"] = ST_RS_FEW
        return r
    v = vertex_triples(ids, positions)
    lo, hi = fc.count_bounds(P, ids, v, threshold=THRESHOLD)
    r["decided"] &= bool(np.array_equal(lo, hi))
    best, best_ic, used = fc.replay(lo, len(ids), GOAL)
    r.update(hyp_counts=lo.astype(np.int32), best=best, best_ic=best_ic, used=used, status=0 if best >= 0 else ST_RS_FEW)
    if best < 0 or not r["decided"]:
        return r
    m, tol = fc.plane_ld(P, v[best])
    PL = P.astype(L)
    res = np.abs(PL @ m[:3] + m[3])
    eps = 2 * L(4.1 * U53) * (np.abs(PL) @ np.abs(m[:3]) + abs(m[3])) + L(tol) * (np.sum(np.abs(PL), 1) + 1)
    r["decided"] &= bool(np.all(np.abs(res - L(INLIER_THRESHOLD)) > eps))
    mask = np.asarray(res < INLIER_THRESHOLD)
    nn = np.sqrt(np.sum(m[:3] * m[:3]))
    r.update(model=m.astype(np.float64), model_tol=tol, mask=mask, n_inliers=int(mask.sum()),
             ransac_height=float(-m[3] / nn), ransac_height_tol=2 * float(tol * (1 / abs(m[3]) + 1 / nn) + 8 * U53))
    if mask.sum() < 3:
        return r
    first = np.nonzero(mask)[0][:3]
    n, _, dn, _, _ = fc._plane_terms(P, first.reshape(1, 3))
    n, dn = n[0], dn[0]
    ln = np.sqrt(np.sum(n * n))
    nh = (n if n[1] >= 0 else -n) / ln
    e_n = 2 * float(2 * np.sqrt(np.sum(dn * dn)) / ln + 8 * U53)                      # every component of n^, absolute
    inl = PL[mask]
    hs = inl @ nh
    d_h = e_n * np.sum(np.abs(inl), 1) + L(4.1 * U53) * (np.abs(inl) @ np.abs(nh))     # every inlier's distance, absolute
    k = int(mask.sum())
    mean = np.mean(hs)
    ts = inl[:, 2] * L(math.sin(est)) + inl[:, 1] * L(math.cos(est))
    r.update(refined_normal=nh.astype(np.float64), refined_normal_tol=e_n,
             refined_pitch=float(np.arcsin(nh[1])), refined_pitch_tol=asin_bound(nh[1], e_n) + 4 * U53,
             refined_mean=float(mean), refined_mean_tol=float(np.mean(d_h) + (k + 4) * U53 * np.mean(np.abs(hs))),
             refined_std=float(np.sqrt(np.mean((hs - mean) ** 2))),
             refined_std_tol=2 * float(np.max(d_h) + (k + 8) * U53 * np.max(np.abs(hs))),
             height_t_mean=float(np.mean(ts)),
             height_t_mean_tol=float((k + 6) * U53 * np.mean(np.abs(inl[:, 2] * L(math.sin(est))) + np.abs(inl[:, 1] * L(math.cos(est))))))
    return r


# ---- the device draw (include/mvosr.h, mvosr_flat_ransac_batch): the oracle's restatement ---------------------------------------
def draw_positions(seed, frame_counter, n_hyp, M):
    return ro.device_triples(seed, frame_counter, M, n_hyp).astype(np.int32)


# ---- crafted frames ---------------------------------------------------------------------------------------------------------
class Frame:
    """pts: (N, 3) [u, v, depth]; rows: (T, 3); est: the prior in radians; positions: (H, 3) list positions."""

    def __init__(self, name, pts, rows, est=0.0, positions=None):
        self.name, self.est = name, float(est)
        self.pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        self.rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 3)
        self.positions = None if positions is None else np.ascontiguousarray(positions, dtype=np.int32).reshape(-1, 3)


def project(xyz):
    """Camera coordinates -> [u, v, depth] (back_project undoes it up to rounding; the references start from ITS doubles)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return np.stack([CX + FOCUS * xyz[:, 0] / xyz[:, 2], CY + FOCUS * xyz[:, 1] / xyz[:, 2], xyz[:, 2]], 1)


def plane_tri(rng, h, tilt_deg=0.0, up=False):
    """Three points of the plane y cos t + z sin t = h (pitch -(90 - t) deg, height h); up: y -> -y (n_y < 0: negative height)."""
    t = np.deg2rad(tilt_deg)
    x, z = rng.uniform(-6.0, 6.0, 3), np.array([6.0, 14.0, 24.0]) + rng.uniform(-2.0, 2.0, 3)
    x[1] += 8.0 if x[1] < x[0] else -8.0                                             # (keeps the three well apart: kappa ~ 1e2)
    y = (h - z * np.sin(t)) / np.cos(t)
    return np.stack([x, -y if up else y, z], 1)


def wall_tri(rng, z=30.0):
    """Three points of the plane z = const: pitch 0, outside every window used here."""
    return np.stack([rng.uniform(-8.0, 8.0, 3) + np.array([-9.0, 0.0, 9.0]), rng.uniform(-9.0, -3.0, 3) + np.array([0.0, 2.5, -2.5]),
                     np.full(3, z)], 1)                                               # (y < 0: never near a road plane y = h)


def rand_positions(rng, M, H):
    return np.stack([rng.choice(M, 3, replace=False) for _ in range(H)]).astype(np.int32) if M >= 3 else np.zeros((H, 3), np.int32)


def scene(name, specs, seed, est=0.0, H=64, n_loose=0, order=None, shuffle=True, first=None, extra_rows=(), given=()):
    """specs: list of ("road", h, tilt) / ("up", h, tilt) / ("wall", z): one triangle each with vertices of its own, rows in a seeded
    order.  given: triangles as (3, 3) camera-space arrays, behind the specs'.  n_loose: extra points no row names (far behind the
    walls).  extra_rows: rows over vertex numbers (triangle k has 3k .. 3k + 2), behind the others.  order: a permutation of the
    vertices (where they lie in the frame).  first: list positions of the first hypotheses (the rest are seeded draws)."""
    rng = np.random.default_rng(seed)
    tris = []
    for s in specs:
        tris.append(wall_tri(rng, s[1]) if s[0] == "wall" else plane_tri(rng, s[1], s[2], up=s[0] == "up"))
    tris += [np.asarray(g, dtype=np.float64).reshape(3, 3) for g in given]
    xyz = np.concatenate(tris + [np.stack([rng.uniform(-20, 20, n_loose), rng.uniform(-30, -20, n_loose), rng.uniform(40, 60, n_loose)], 1)])
    rows = np.arange(3 * len(tris)).reshape(-1, 3)
    if shuffle:
        rows = rows[rng.permutation(len(rows))]
    if len(extra_rows):
        rows = np.concatenate([rows, np.asarray(extra_rows, dtype=np.int64).reshape(-1, 3)])
    if order is not None:
        order = np.asarray(order)
        inv = np.empty(len(order), dtype=np.int64)
        inv[order] = np.arange(len(order))                                           # vertex k goes to place inv[k]
        xyz, rows = xyz[order], inv[rows]
    f = Frame(name, project(xyz), rows, est)
    keep, ids, _, _ = select(back_project(f.pts), f.rows.astype(np.int64), est)
    pos = rand_positions(rng, len(ids), H)
    if first is not None:
        pos[:len(first)] = np.asarray(first, dtype=np.int32).reshape(-1, 3)
    f.positions = pos
    return f


def tilt_at(rng_seed, h, edge_deg, offset_margins, est):
    """A road triangle whose pitch lies `offset_margins` pitch margins from the window edge `edge_deg` (positive: above it): the
    tilt is bisected on the np.longdouble pitch of the float64 inputs the kernel sees."""
    def build(tilt):
        return project(plane_tri(np.random.default_rng(rng_seed), h, tilt))
    def pitch_of(tilt):
        q = rows_ld(back_project(build(tilt)), np.arange(3).reshape(1, 3))
        return float(q["pitch"][0]), float(q["kappa"][0])
    guess = 90.0 + edge_deg * PI_S / np.pi
    _, kappa = pitch_of(guess)
    target = edge_deg + offset_margins * fc.pitch_margin_deg(kappa, edge_deg)
    lo, hi = guess - 0.5, guess + 0.5
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if pitch_of(mid)[0] < target:
            lo = mid
        else:
            hi = mid
    return back_project(build(hi if offset_margins > 0 else lo))


def est_of(deg):
    return deg * PI_S / 180


_CRAFTED = {}


def crafted():
    """name -> Frame.  Every frame's integers are decided by `reference` (test_heightpitch_cases.py asserts it)."""
    if _CRAFTED:
        return _CRAFTED
    road, wall = ("road", 1.7, 0.0), ("wall", 30.0)
    c = _CRAFTED
    c["empty"] = Frame("empty", np.zeros((0, 3)), np.zeros((0, 3)), positions=np.zeros((64, 3)))
    c["one_row"] = scene("one_row", [road], 1)
    c["rows3"] = scene("rows3", [road] * 3 + [wall] * 2, 2)                          # 9 list points: :140 fails
    c["rows4"] = scene("rows4", [road] * 4 + [wall] * 2, 3)                          # 12: fitted
    c["tail65"] = scene("tail65", [road] * 12 + [wall] * 9, 4, n_loose=2)
    c["tail129"] = scene("tail129", [road] * 20 + [("road", 1.6, 1.0)] * 5 + [wall] * 15 + [("up", 1.7, 0.0)] * 3, 5, H=512)
    rng = np.random.default_rng(6)
    mixed = [road] * 40 + [("road", float(rng.uniform(1.5, 1.9)), float(rng.uniform(-2, 2))) for _ in range(20)] + [wall] * 30 + [("up", 1.7, 0.0)] * 10
    c["big300"] = scene("big300", mixed, 7, H=512)                                   # 100 rows: kept rows in wavefronts 0 and 1
    c["neg_height"] = scene("neg_height", [road] * 5 + [("up", 1.7, 0.0), ("up", 1.2, 1.0)] + [wall], 8)
    # the prior: the window (est_deg - 95, est_deg - 85); below -90 deg there is no triangle, so the low edge is met only at +6 deg
    for deg in (-2.0, 0.0, 2.0, 6.0):
        est = est_of(deg)
        lo, hi = prior_of(est)[:2]
        base = ("road", 1.7, 0.0 if lo < -90.5 else 90.0 + 0.5 * (lo + hi))
        edges = [(hi, 2.0), (hi, -2.0)] + ([(lo, 2.0), (lo, -2.0)] if lo > -89.5 else [])
        given = [tilt_at(100 + k, 1.5 + 0.1 * k, e, o, est) for k, (e, o) in enumerate(edges)]
        c["prior%+d" % deg] = scene("prior%+d" % deg, [base] * 5 + [wall], 9, est=est, given=given)
    levels = [("road", 1.0 + 0.3 * k, 0.0) for k in range(5)] + [wall] * 3           # parallel planes 0.3 apart: no plane holds more than 3 list points ... or few
    c["tie"] = scene("tie", levels, 10, shuffle=False, first=[[0, 1, 2], [2, 0, 1], [6, 7, 8]], H=3)    # equal counts: the first stays
    c["never"] = scene("never", levels, 11)
    c["goal0"] = scene("goal0", [road] * 6 + [wall] * 2, 12, shuffle=False, first=[[0, 4, 8]])
    # a row over vertices of two coplanar triangles: vertex 0 is in the list twice (positions 0 and 18)
    c["spent"] = scene("spent", [road] * 6 + [wall] * 2, 13, shuffle=False, extra_rows=[[0, 4, 8]],
                       first=[[0, 18, 5], [18, 0, 7], [21, 0, 1], [-1, 0, 1], [2, 3, 1 << 20], [0, 0, 1]])
    c["three"] = scene("three", levels, 14, shuffle=False, first=[[3, 4, 5]], H=8)
    # where the first three inliers lie: 8 coplanar road rows (24 inliers) among 92 walls
    spec300 = [road] * 8 + [wall] * 92
    def placed(places):
        rest_in = [p for p in range(261, 300)][:24 - len(places)]
        inl = list(places) + rest_in
        others = [p for p in range(300) if p not in set(inl)]
        order = np.empty(300, dtype=np.int64)
        order[inl] = np.arange(24)
        order[others] = np.arange(24, 300)
        return order
    c["wave0"] = scene("wave0", spec300, 15, order=placed([3, 10, 40]))
    c["spread"] = scene("spread", spec300, 16, order=placed([1, 70, 260]))
    # refusals
    s = scene("singular", [road] * 5 + [wall], 17, n_loose=1, shuffle=False, extra_rows=[[0, 18, 1]])
    s.pts[18] = s.pts[0]                                                             # two equal matrix rows: a zero pivot, exactly
    c["singular"] = s
    b = scene("badid", [road] * 5 + [wall], 18)
    b.rows[2, 1] = len(b.pts)
    c["badid"] = b
    return c


def load_golden():
    """tests/golden/heightpitch.npz -> {case: dict(frames=[(N, 3)], motion, rows, positions, ...)}; the inputs are regenerated from
    the stored seeds and checked against the stored checksums."""
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    if os.path.dirname(here) not in sys.path:
        sys.path.insert(0, os.path.dirname(here))
    from mvoscalerecovery_amd import synth
    z = np.load(os.path.join(here, "golden", "heightpitch.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    out = {}
    for name, m in meta.items():
        frames = []
        for fr in m["frames"]:
            if fr["kind"] == "synth":
                f3, f2 = synth.synth_frame(fr["args"][0], fr["args"][1], base_seed=fr["args"][2])
                d = np.stack([f2[:, 0], f2[:, 1], f3[:, 2]], 1)
            else:
                d = wall_frame(fr["args"][0], fr["args"][1])
            assert crc(d) == fr["crc"], "synthetic generator drifted from the fixture"
            frames.append(d)
        g = {"frames": frames, "meta": m, "rows": [z["%s_rows%d" % (name, i)] for i in range(len(frames))]}
        for k in ("ransac_camera_heights", "refined_camera_height_means", "refined_camera_height_stds", "refined_camera_height_t_means",
                  "refined_pitchs", "inlier_numbers", "suitable", "priors"):
            g[k] = z["%s_%s" % (name, k)]
        for k in ("positions", "model", "best_ic", "mask"):
            g[k] = [(z["%s_%s%d" % (name, k, i)] if "%s_%s%d" % (name, k, i) in z.files else None) for i in range(len(frames))]
        out[name] = g
    return out
