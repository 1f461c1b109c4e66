"""Crafted frames and references for triangle_batch_kernel (csrc/mvosr_rescale.hip) — shared by tests/test_tribatch_cases.py (CPU:
NumPy float64 in the kernel's place) and tests/test_gpu_triangle_batch.py (mvosr_triangle_batch on the device).  Test infrastructure.

The rows of tri1 are an input, so a frame is a list of small triangles with three features of their own, each row repeated as
often as the family wants.  A triangle with vertices (x, h0 - k z, z) lies on the plane n.p = 1 with n = (0, 1, k) / h0: s = n_y / |n| =
1 / sqrt(1 + k^2) and the row's height is h0 - k mean(z) — flat and kept (k = 0), steep (k = tan 25 deg: s = 0.906), or flat enough
but ABOVE the camera (k = 0.1, s = 0.995, z ~ 40: h < 0).  The features are its projection [u, v, depth]; the references take the
float64 features as exact inputs, so the projection's own rounding is part of the frame, not of the error.

Reference: mpmath at 60 digits per distinct row (back-projection, A n = 1 by the adjugate, s, h = mean Y, kappa_inf(A)), then the
keep rule, mean, standard deviation, clip and final mean in np.longdouble over the rows.

Tolerances (u = 2^-53), none of them fitted to a kernel:
  * s: C_HEIGHT kappa_inf(A) u relative (flat_cases.C_HEIGHT: the same plane_normal); a row is decided kept / dropped when s is
    further than that from s_min and h further than 6.1 u mean|Y| from 0 (three roundings per Y, two for the sum, one for the
    third); every family but `threshold_band` has no undecided row, so counts[0] is exact;
  * the clip: with E = (cnt + 8) u max h bounding the error of a height and of the mean, a deviation moves by <= 2E, the standard
    deviation (an RMS) by <= 2E + (cnt + 4) u sd, an edge mean -+ 3 sd by E + 3 (2E + (cnt + 4) u sd) + 4 u (|mean| + 3 sd); no
    kept row of those families is within that (+ E for the row itself) of an edge, so counts[1] is exact;
  * height: Y = d (v - cy) / focus has 3 roundings, (Ya + Yb) + Yc 2, the third at most 1 ulp = 2 u more: 7 u per row; a sum of
    cnt2 positive terms in any order (cnt2 - 1) u, the final division 1: (cnt2 + 7) u, with one more for second-order terms:
    HEIGHT_C = 8, the bound (cnt2 + 8) u relative.
Measured on the CPU (tests/test_tribatch_cases.py prints it): NumPy float64 (oracle.triangle_batch_oracle.camera_height) uses at
most 0.003 of the height bound over the families here (`control`; HEIGHT_SHARE_MEASURED is that, rounded up to 0.004).
"""
import ctypes as C

import numpy as np

import flat_cases as fc
from flat_cases import C_HEIGHT, U53, ST_SINGULAR, ST_MASK, ST_EMPTY                       # noqa: F401  (not redefined here)

FOCUS, CX, CY = 718.856, 607.1928, 182.2157        # mvoscalerecovery_amd.triangle_batch
S_MIN, N_SIGMA = 0.98, 3.0
HEIGHT_C = 8
HEIGHT_SHARE_MEASURED = 0.004
KEEP = 8 * 512                                     # kTbKeep * kRsBlock: rows from here on are recomputed in each of the three sweeps
K_STEEP, K_ABOVE = float(np.tan(np.deg2rad(25.0))), 0.1


class Frame:
    """feats (n, 3) = [u, v, depth]; tri (T, 3); status: what the kernel must report; skip: rows without a reference (bad id,
    singular); band: the threshold family (count bounds only); expect: (counts, height is NaN) known from the construction alone —
    the frames whose kept heights are all one bit pattern, sd == 0 exactly and both clip comparisons strict."""

    def __init__(self, name, feats, tri, status=0, skip=None, band=False, expect=None, note=""):
        self.name, self.status, self.band, self.expect, self.note = name, status, band, expect, note
        self.feats = np.ascontiguousarray(feats, dtype=np.float64).reshape(-1, 3)
        self.tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        self.skip = np.zeros(len(self.tri), bool) if skip is None else np.asarray(skip, bool)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def _shape(rng, zc):
    ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, 3)
    r = rng.uniform(0.6, 1.4, 3)
    return np.array([rng.uniform(-5, 5), zc]) + r[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])


def _project(p):
    return np.column_stack([p[:, 0] * FOCUS / p[:, 2] + CX, p[:, 1] * FOCUS / p[:, 2] + CY, p[:, 2]])


def plane_tri(rng, h, k=0.0, zc=None, mean_y=None):
    """Three features of a triangle on n = (0, 1, k) / h0.  h is h0 — or, with mean_y, h0 is chosen so that the row's height is mean_y."""
    xz = _shape(rng, rng.uniform(5, 20) if zc is None else zc)
    h0 = h if mean_y is None else mean_y + k * float(np.mean(xz[:, 1]))
    return _project(np.column_stack([xz[:, 0], h0 - k * xz[:, 1], xz[:, 1]]))


def flat(rng, h):
    return plane_tri(rng, h)


def steep(rng):
    return plane_tri(rng, rng.uniform(1.5, 1.9), K_STEEP, zc=rng.uniform(3, 4))


def above(rng):
    return plane_tri(rng, rng.uniform(1.5, 1.9), K_ABOVE, zc=rng.uniform(38, 42))


def build(name, tris, rows, **kw):
    """tris: list of (3, 3) feature blocks; rows: indices into it (a row is the block's three features in order)."""
    rows = np.asarray(rows, dtype=np.int64)
    tri = 3 * rows[:, None] + np.arange(3)[None, :]
    return Frame(name, np.concatenate(tris), tri, **kw)


def control():
    rng = np.random.default_rng(11)
    tris = [flat(rng, h) for h in np.clip(rng.normal(1.7, 0.03, 60), 1.62, 1.78)]
    tris += [steep(rng) for _ in range(15)] + [above(rng) for _ in range(15)]
    tris += [flat(rng, h) for h in (2.7, 0.7, 3.1, 0.5, 2.9)] + [steep(rng) for _ in range(5)]
    rows = [i for i in range(60) for _ in range(7)] + [i for i in range(60, 75) for _ in range(6)] + [i for i in range(75, 90) for _ in range(5)]
    rows += list(range(90, 95)) + list(range(95, 100)) * 2
    return build("control", tris, rng.permutation(rows), note="100 triangles, %d rows: 420 on the road, 5 flat rows far outside 3 sigma" % len(rows))


def many_rows():
    """4096 + 512 + 37 rows over 100 triangles.  The first 4096 rows: tight road rows (1.7 +- 0.01), steep rows and rows above
    the camera.  The rows from 4096 on — the ones each sweep recomputes —: ten DISTINCT heights 1.6 .. 1.8 fifty times each (most of
    the variance apart from the outlier's), the one outlier the clip must drop (h = 6), steep rows, rows above the camera and
    eight tight ones.  -> (frame, the same rows reversed: the distinctive ones below 4096)"""
    rng = np.random.default_rng(12)
    tris = [flat(rng, h) for h in rng.uniform(1.69, 1.71, 60)] + [steep(rng) for _ in range(10)] + [above(rng) for _ in range(10)]
    tris += [flat(rng, h) for h in np.linspace(1.6, 1.8, 10)] + [flat(rng, 6.0)] + [steep(rng) for _ in range(9)]
    body = np.where(rng.uniform(size=KEEP) < 0.8, rng.integers(0, 60, KEEP), rng.integers(60, 80, KEEP))
    tail = [i for i in range(80, 90) for _ in range(50)] + [90] + [60 + i % 10 for i in range(20)] + [70 + i % 10 for i in range(20)] + list(range(8))
    tail = rng.permutation(tail)
    assert len(tail) == 512 + 37
    rows = np.concatenate([body, tail])
    a = build("many_rows", tris, rows, note="the kept rows of distinct heights, the clipped outlier and steep rows at t >= 4096")
    b = build("many_rows_moved", tris, rows[::-1].copy(), note="the same rows, the distinctive ones below 4096")
    return a, b


def small(name, n_flat, seed, reps=1, **kw):
    rng = np.random.default_rng(seed)
    tris = [flat(rng, 1.7) for _ in range(n_flat)] + [steep(rng) for _ in range(6)] + [above(rng) for _ in range(6)]
    rows = list(range(n_flat, n_flat + 12)) * 2
    for j in range(reps if n_flat else 0):
        rows.insert(15 if j else 3, 0)                                   # (the copies of the one flat row, apart from one another)
    return build(name, tris, rows, **kw)


def threshold_band():
    """Rows whose s sits at 0.98 + d for d = 0, +-1e-10 .. +-1e-2 (height clearly positive) and rows whose height sits at 0 + d
    for d = 0, +-1e-9 .. +-1e-1 (s = 0.995), next to plain rows of every class."""
    rng = np.random.default_rng(14)
    tris = []
    for d in (0.0, 1e-10, -1e-10, 1e-8, -1e-8, 1e-6, -1e-6, 1e-4, -1e-4, 1e-2, -1e-2):
        s = S_MIN + d
        tris.append(plane_tri(rng, rng.uniform(1.5, 1.9), float(np.sqrt(1.0 / (s * s) - 1.0)), zc=rng.uniform(3, 4)))
    for d in (0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 1e-1, -1e-1):
        tris.append(plane_tri(rng, None, K_ABOVE, zc=rng.uniform(15, 19), mean_y=d))
    tris += [flat(rng, h) for h in (1.6, 1.65, 1.7, 1.75, 1.8)] + [steep(rng), steep(rng), above(rng), above(rng)]
    return build("threshold_band", tris, np.arange(len(tris)), band=True, note="s across 0.98, h across 0")


def families():
    """name -> Frame (the order of the one batch)."""
    fam = {}
    empty = lambda name: Frame(name, np.zeros((0, 3)), np.zeros((0, 3), np.int32), status=ST_EMPTY, note="no features, no rows")
    fam["empty_first"] = empty("empty_first")
    fam["control"] = control()
    fam["many_rows"], fam["many_rows_moved"] = many_rows()
    fam["none_kept"] = small("none_kept", 0, 21, note="steep rows and rows above the camera only")
    fam["one_kept"] = small("one_kept", 1, 22, expect=((1, 0), True), note="cnt = 1: mean = h, sd = 0, h > h is false")
    fam["empty_middle"] = empty("empty_middle")
    fam["two_equal"] = small("two_equal", 1, 23, reps=2, expect=((2, 0), True), note="one row twice: (h + h) / 2 = h exactly, sd = 0")
    fam["threshold_band"] = threshold_band()
    c = control()
    n = len(c.feats)
    feats = np.concatenate([c.feats[:60], c.feats[:1]])                  # feature 60: a copy of feature 0
    rows = np.concatenate([c.tri[(c.tri < 60).all(1)][:40], [[0, 60, 1]]])
    fam["singular"] = Frame("singular", feats, rows, status=ST_SINGULAR, skip=np.arange(41) == 40, note="a row with two identical vertices")
    rows = np.concatenate([c.tri[:80], [[0, 1, n], [-1, 4, 5]]])
    fam["bad_id"] = Frame("bad_id", c.feats, rows, status=ST_MASK, skip=np.arange(82) >= 80, note="ids n and -1")
    feats = np.concatenate([c.feats, c.feats[:1]])
    rows = np.concatenate([c.tri[:80], [[0, n, 1], [3, 4, n + 1]]])
    fam["bad_and_singular"] = Frame("bad_and_singular", feats, rows, status=ST_MASK, skip=np.arange(82) >= 80, note="_MASK wins over _SINGULAR")
    fam["empty_last"] = empty("empty_last")
    return fam


# ---- references -----------------------------------------------------------------------------------------------------------
_MP_CACHE = {}


def mp_rows(frame):
    """Per row with mpmath at 60 digits, from the float64 features: s = n_y / |n| and h = mean Y (np.longdouble), kappa_inf(A) and
    mean |Y| (float64).  Rows in frame.skip are nan.  Cached per frame, computed once per distinct row."""
    import mpmath as mp
    if frame.name in _MP_CACHE:
        return _MP_CACHE[frame.name]
    T = len(frame.tri)
    s, h = np.full(T, np.nan, dtype=np.longdouble), np.full(T, np.nan, dtype=np.longdouble)
    kappa, absy = np.full(T, np.nan), np.full(T, np.nan)
    seen = {}
    with mp.workdps(60):
        fo, cx, cy = mp.mpf(FOCUS), mp.mpf(CX), mp.mpf(CY)
        P = {}

        def vertex(i):
            if i not in P:
                u, v, d = (mp.mpf(float(x)) for x in frame.feats[i])
                P[i] = (d * (u - cx) / fo, d * (v - cy) / fo, d)
            return P[i]

        for t in range(T):
            if frame.skip[t]:
                continue
            row = tuple(int(v) for v in frame.tri[t])
            if row not in seen:
                (a, b, c), (d, e, f), (g, hh, i) = [vertex(r) for r in row]
                c00, c01, c02 = e * i - f * hh, f * g - d * i, d * hh - e * g
                det = a * c00 + b * c01 + c * c02
                c10, c11, c12 = c * hh - b * i, a * i - c * g, b * g - a * hh
                c20, c21, c22 = b * f - c * e, c * d - a * f, a * e - b * d
                nx, ny, nz = (c00 + c10 + c20) / det, (c01 + c11 + c21) / det, (c02 + c12 + c22) / det
                ninv = max(abs(c00) + abs(c10) + abs(c20), abs(c01) + abs(c11) + abs(c21), abs(c02) + abs(c12) + abs(c22)) / abs(det)
                na = max(abs(a) + abs(b) + abs(c), abs(d) + abs(e) + abs(f), abs(g) + abs(hh) + abs(i))
                seen[row] = (fc._ld(ny / mp.sqrt(nx * nx + ny * ny + nz * nz)), fc._ld((b + e + hh) / 3), float(na * ninv),
                             float((abs(b) + abs(e) + abs(hh)) / 3))
            s[t], h[t], kappa[t], absy[t] = seen[row]
    _MP_CACHE[frame.name] = (s, h, kappa, absy)
    return _MP_CACHE[frame.name]


def height_tol(cnt2):
    """Relative bound on the kernel's (and NumPy's) height against the exact mean of the same rows: (cnt2 + HEIGHT_C) u."""
    return (cnt2 + HEIGHT_C) * U53


def reference(frame):
    """-> dict: kept_lo / kept_hi (bounds of counts[0]), undecided (rows), and — when no row is undecided — cnt2, height
    (np.longdouble), clip_clear (no kept row within the derived bound of an edge)."""
    L = np.longdouble
    s, h, kappa, absy = mp_rows(frame)
    ok = ~frame.skip
    s, h, kappa, absy = s[ok], h[ok], kappa[ok], absy[ok]
    s_tol = (C_HEIGHT * kappa * U53).astype(L) * np.abs(s)
    h_tol = L(6.1 * U53) * absy
    kept = (s - L(S_MIN) > s_tol) & (h > h_tol)
    out = (s - L(S_MIN) < -s_tol) | (h < -h_tol)
    und = ~(kept | out)
    r = {"kept_lo": int(kept.sum()), "kept_hi": int(kept.sum() + und.sum()), "undecided": int(und.sum()),
         "s_sides": (int((s - L(S_MIN) > s_tol).sum()), int((s - L(S_MIN) < -s_tol).sum())),
         "h_sides": (int((h > h_tol).sum()), int((h < -h_tol).sum()))}
    if und.any():
        return r
    hk = h[kept]
    cnt = len(hk)
    if cnt == 0:
        r.update(cnt2=0, height=L(np.nan), clip_clear=True)
        return r
    mean = hk.sum() / cnt
    sd = np.sqrt(((hk - mean) ** 2).sum() / cnt)
    lo, hi = mean - N_SIGMA * sd, mean + N_SIGMA * sd
    E = L((cnt + 8) * U53) * hk.max()
    margin = E + 3 * (2 * E + L((cnt + 4) * U53) * sd) + L(4 * U53) * (abs(mean) + 3 * sd) + E
    inside = (hk > lo) & (hk < hi)
    r.update(cnt2=int(inside.sum()), clip_clear=bool(np.all(np.minimum(np.abs(hk - lo), np.abs(hk - hi)) > margin)),
             height=(hk[inside].sum() / inside.sum()) if inside.any() else L(np.nan), mean=mean, sd=sd)
    return r


def sweeps(hk_rows, drop, sweep):
    """The kernel's three sweeps in np.longdouble over per-row kept heights (nan: not kept), with the rows `drop` (a mask) left out
    of sweep 1, 2 or 3 (0: none) — what a recompute loop that does not run would compute.  -> (cnt, cnt2, height)"""
    k = ~np.isnan(hk_rows)
    use = [k & ~(drop & (sweep == j)) for j in (1, 2, 3)]
    cnt = int(use[0].sum())
    mean = hk_rows[use[0]].sum() / cnt
    sd = np.sqrt(((hk_rows[use[1]] - mean) ** 2).sum() / cnt)
    ins = use[2] & (hk_rows > mean - N_SIGMA * sd) & (hk_rows < mean + N_SIGMA * sd)
    return cnt, int(ins.sum()), hk_rows[ins].sum() / max(int(ins.sum()), 1)


def kept_rows(frame):
    """Per row of the frame the exact kept height or nan (families without undecided rows)."""
    s, h, kappa, absy = mp_rows(frame)
    with np.errstate(invalid="ignore"):
        return np.where((s > np.longdouble(S_MIN)) & (h > 0), h, np.longdouble(np.nan))


# ---- launcher (GPU) -------------------------------------------------------------------------------------------------------------
def run_tri(ctx, frames, max_feat=None):
    """mvosr_triangle_batch over `frames` with a hand-built batch header -> one dict per frame.  max_feat: the header's value
    (None: the largest frame's).  The outputs are pre-filled with 0x55 bytes."""
    from mvoscalerecovery_amd import _lib
    cnt = np.array([len(f.feats) for f in frames], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f.tri) for f in frames])]).astype(np.int64)
    feats = np.concatenate([f.feats for f in frames] + [np.zeros((1, 3))])
    rows = np.concatenate([f.tri for f in frames] + [np.zeros((1, 3), np.int32)]).astype(np.int32)
    d = [ctx.to_device(off), ctx.to_device(cnt), ctx.to_device(toff), ctx.to_device(rows.reshape(-1)),
         ctx.to_device(feats[:, 0].copy()), ctx.to_device(feats[:, 1].copy()), ctx.to_device(feats[:, 2].copy())]
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt = len(frames), d[0].ptr, d[1].ptr
    b.x, b.y, b.z, b.v = d[4].ptr, d[5].ptr, d[6].ptr, d[5].ptr
    b.tri1_off, b.tri1 = d[2].ptr, d[3].ptr
    b.max_feat, b.total_feat = int(cnt.max() if max_feat is None else max_feat), int(off[-1])
    F = len(frames)
    o = {"height": ctx.empty(F, np.float64).fill(0x55), "counts": ctx.empty((F, 2), np.int32).fill(0x55), "status": ctx.empty(F, np.int32).fill(0x55)}
    _lib.check(ctx.lib.mvosr_triangle_batch(ctx.handle, C.byref(b), FOCUS, CX, CY, S_MIN, N_SIGMA, o["height"].ptr, o["counts"].ptr,
                                            o["status"].ptr), "mvosr_triangle_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + d)
    return [{"height": r["height"][i], "counts": (int(r["counts"][i, 0]), int(r["counts"][i, 1])), "status": int(r["status"][i])} for i in range(F)]
