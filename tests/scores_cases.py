"""Crafted sequences, a plain NumPy restatement and launch helpers for the device scoring of the repeated runs
(csrc/mvosr_score.hip, evaluate.Scorer; tests/test_scores_cases.py on the CPU, tests/test_gpu_scores.py on the device).

Two restatements: ``paths_numpy`` / ``score_numpy`` / ``pose2motion_numpy`` are the reference's own formulation without its loops
over cases and segments (np.linalg.inv and matmul on stacks of 4 x 4 matrices) — what a NumPy rewrite of the host route would be;
``paths_restated`` / ``score_restated`` / ``pose2motion_restated`` state the kernels' operation orders for any float type — the
generator runs them in np.longdouble to measure the gaps.

Sequences come from seeds with +, -, *, / and sqrt on uniform draws only (no libm call: the same bytes on every machine); the
fixture tests/golden/scores.npz (make_golden_scores.py) holds their checksums, the reference's outputs, the same quantities in
np.longdouble and, per quantity and sequence, gap = max |reference - extended|.

The tolerance rule (one function, :func:`within`): integers are exact; every float lies within 4 gaps of the reference's value.
The reference and a correct float64 evaluation each sit about one gap from the exact value — opposite signs give two, a little
more where one of them is unlucky — so four gaps separate "another rounding order" from "another formula".  The gap is measured
against the reference, never against the code under test.
"""
import zlib

import numpy as np

LENGTHS = np.array([100, 200, 300, 400, 500, 600, 700, 800])
STEP = 10
GAPS = 4.0

# name -> (n, cases, seed, kind).  Translations are about 12 m a frame, so a few hundred frames span every length.
SEQUENCES = {
    "n257": (257, 10, 2570, "noisy"),          # every length; late firsts lack the long ones
    "n130": (130, 3, 1300, "noisy"),
    "n65": (65, 3, 650, "noisy"),              # 7 of the 8 lengths: tra has 7 columns
    "n9": (9, 1, 90, "noisy"),                 # one segment
    "n1": (1, 1, 10, "noisy"),                 # no segments
    "n0": (0, 1, 1, "noisy"),
    "same130": (130, 3, 1301, "same_rotation"),  # the ground truth's rotations ARE the result's: r_err is arccos's rounding noise
    "exact60": (60, 3, 600, "exact"),          # ground truth: identity rotations, steps of exactly 16 m: dist is exact in any order
    "n4541": (4541, 3, 45410, "noisy"),        # the chain's drift at KITTI-00's length
}
FULL_POSES_UP_TO = 300       # sequences up to this length keep whole reference paths (cases 0 and C - 1); longer ones every 64th row


def rotations(w):
    """Rotation matrices (k, 3, 3) of the quaternions (1, w) / |(1, w)|: rational in w."""
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    n = 1.0 + ((x * x + y * y) + z * z)
    R = np.empty((w.shape[0], 3, 3))
    R[:, 0, 0] = 1.0 - 2.0 * (y * y + z * z) / n
    R[:, 0, 1] = 2.0 * (x * y - z) / n
    R[:, 0, 2] = 2.0 * (x * z + y) / n
    R[:, 1, 0] = 2.0 * (x * y + z) / n
    R[:, 1, 1] = 1.0 - 2.0 * (x * x + z * z) / n
    R[:, 1, 2] = 2.0 * (y * z - x) / n
    R[:, 2, 0] = 2.0 * (x * z - y) / n
    R[:, 2, 1] = 2.0 * (y * z + x) / n
    R[:, 2, 2] = 1.0 - 2.0 * (x * x + y * y) / n
    return R


def _motions(R, t):
    m = np.empty((R.shape[0], 3, 4))
    m[:, :, :3] = R
    m[:, :, 3] = t
    return m.reshape(-1, 12)


def make_sequence(name):
    """{"motions" (n, 12), "scales" (C, n), "gt" (n + 1, 12)}: a result whose translations have unit length, per-case scales around
    12 with zeros (not-moving frames), and a ground truth whose rotations differ from the result's by about 1e-3 rad a step."""
    n, cases, seed, kind = SEQUENCES[name]
    rng = np.random.default_rng(seed)
    u = rng.random((n, 12))
    w = (u[:, 0:3] - 0.5) * np.array([0.004, 0.04, 0.004])            # half-angles: mostly yaw
    d = np.stack([(u[:, 3] - 0.5) * 0.04, (u[:, 4] - 0.5) * 0.04, np.ones(n)], axis=1)
    d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    motions = _motions(rotations(w), d)
    us = rng.random((cases, n))
    scales = 12.0 * (1.0 + 0.2 * (us - 0.5))
    scales[rng.random((cases, n)) < 0.03] = 0.0
    if kind == "exact":
        gt_m = _motions(rotations(np.zeros((n, 3))), np.tile(np.array([0.0, 0.0, 16.0]), (n, 1)))
    else:
        dw = 0.0 if kind == "same_rotation" else (u[:, 5:8] - 0.5) * 0.001       # half-angle 5e-4: about 1e-3 rad a step
        dg = np.stack([(u[:, 8] - 0.5) * 0.04, (u[:, 9] - 0.5) * 0.04, np.ones(n)], axis=1)
        gt_m = _motions(rotations(w + dw), dg * (12.0 * (1.0 + 0.04 * (u[:, 10] - 0.5)))[:, None])
    gt = paths_restated(gt_m, None)[0]
    return {"motions": motions, "scales": scales, "gt": gt}


def checksum(seq):
    return int(zlib.crc32(b"".join(np.ascontiguousarray(seq[k], dtype=np.float64).tobytes() for k in ("motions", "scales", "gt"))))


def pose_rows(name):
    """The rows of a path the fixture keeps."""
    n = SEQUENCES[name][0]
    return np.arange(n + 1) if n <= FULL_POSES_UP_TO else np.unique(np.concatenate([np.arange(0, n + 1, 64), [n]]))


def pose_cases(name):
    c = SEQUENCES[name][1]
    return np.unique([0, c - 1])


# ---- the kernels' operation orders in NumPy, vectorised over everything but the chain; any float type (the generator runs them in
# ---- np.longdouble for the gaps) --------------------------------------------------------------------------------------------------
def mul(a, b):
    """(..., 3, 4) x (..., 3, 4) affine product, k ascending, the fourth term with b's last row 0 0 0 1 written out."""
    last = np.zeros(4, dtype=a.dtype)
    last[3] = 1
    out = np.empty(np.broadcast_shapes(a.shape, b.shape), dtype=a.dtype)
    for j in range(4):
        out[..., j] = ((a[..., 0] * b[..., 0, j, None] + a[..., 1] * b[..., 1, j, None]) + a[..., 2] * b[..., 2, j, None]) + a[..., 3] * last[j]
    return out


def inv(a):
    """The inverse of the affine matrix as it is: adj(R) / det(R), det by the first row; -(R^-1 t)."""
    r = a[..., :3]
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = (r[..., i, j] for i in range(3) for j in range(3))
    c = np.empty(a.shape[:-2] + (3, 3), dtype=a.dtype)
    c[..., 0, 0], c[..., 0, 1], c[..., 0, 2] = r11 * r22 - r12 * r21, r02 * r21 - r01 * r22, r01 * r12 - r02 * r11
    c[..., 1, 0], c[..., 1, 1], c[..., 1, 2] = r12 * r20 - r10 * r22, r00 * r22 - r02 * r20, r02 * r10 - r00 * r12
    c[..., 2, 0], c[..., 2, 1], c[..., 2, 2] = r10 * r21 - r11 * r20, r01 * r20 - r00 * r21, r00 * r11 - r01 * r10
    det = (r00 * c[..., 0, 0] + r01 * c[..., 1, 0]) + r02 * c[..., 2, 0]
    out = np.empty_like(a)
    with np.errstate(all="ignore"):
        out[..., :3] = c / det[..., None, None]
    t = a[..., 3]
    out[..., 3] = -((out[..., 0] * t[..., 0, None] + out[..., 1] * t[..., 1, None]) + out[..., 2] * t[..., 2, None])
    return out


def norm3(t):
    return np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])


def paths_restated(motions, scales, dtype=np.float64):
    """mvosr_paths_batch: (C, n + 1, 12).  ``motions`` (n, 12) shared, or (C, n, 12) per case; ``scales`` (C, n) or None."""
    m = np.asarray(motions, dtype=dtype)
    m = m.reshape((1,) + m.shape) if m.ndim == 2 else m
    cases = m.shape[0] if scales is None else np.shape(scales)[0]
    n = m.shape[1]
    steps = np.broadcast_to(m.reshape(m.shape[0], n, 3, 4), (cases, n, 3, 4)).copy()
    if scales is not None:
        steps[..., 3] = steps[..., 3] * np.asarray(scales, dtype=dtype)[:, :, None]
    out = np.zeros((cases, n + 1, 3, 4), dtype=dtype)
    out[:, 0, 0, 0] = out[:, 0, 1, 1] = out[:, 0, 2, 2] = 1
    for i in range(n):                                                   # the chain: strictly left to right
        out[:, i + 1] = mul(out[:, i], steps[:, i])
    return out.reshape(cases, n + 1, 12)


def distances(gt, dtype=np.float64):
    g = np.asarray(gt, dtype=dtype).reshape(-1, 3, 4)
    steps = norm3(g[:-1, :, 3] - g[1:, :, 3])
    return np.concatenate([np.zeros(1, dtype=dtype), np.cumsum(steps, dtype=dtype)])      # (cumsum adds left to right)


def segment_table(dist):
    """last (F, 8): the first i >= first with dist[i] > dist[first] + length, else -1; and how far the decisive comparisons —
    dist[last] above the limit, dist[last - 1] not — clear it."""
    dist = np.asarray(dist)
    n = dist.shape[0]
    firsts = np.arange(0, n, STEP)
    limit = dist[firsts][:, None] + LENGTHS[None, :].astype(dist.dtype)
    last = np.searchsorted(dist, limit.reshape(-1), side="right").reshape(limit.shape)   # first index with dist > limit
    last = np.maximum(last, firsts[:, None])
    found = last < n
    li = np.where(found, last, n - 1)
    margin = np.where(found, np.minimum(dist[li] - limit, limit - dist[np.maximum(li - 1, 0)]), limit - dist[n - 1])
    return np.where(found, last, -1).astype(np.int32), margin


def score_restated(gt, paths, last, dtype=np.float64):
    """mvosr_score_cases_batch: r_seg, t_seg (C, F, 8) with NaN where there is no segment, means (C, 2, 8).  The kernel carries a
    segment's g, q, e, trace and sum of squares in double-double and rounds once in front of acos and sqrt; np.longdouble (64 bits
    instead of about 100) stands for that here, then ``dtype`` takes over."""
    wide = np.longdouble
    g = np.asarray(gt, dtype=wide).reshape(-1, 3, 4)
    p = np.asarray(paths, dtype=wide)
    p = p.reshape(p.shape[0], -1, 3, 4)
    has = last >= 0
    f, li = np.nonzero(has)
    first, lst = f * STEP, last[f, li]
    gd = mul(inv(g[first]), g[lst])
    q = mul(inv(p[:, first]), p[:, lst])
    e = mul(inv(q), gd[None])
    d = (0.5 * (((e[..., 0, 0] + e[..., 1, 1]) + e[..., 2, 2]) - 1)).astype(dtype)
    sq = ((e[..., 0, 3] * e[..., 0, 3] + e[..., 1, 3] * e[..., 1, 3]) + e[..., 2, 3] * e[..., 2, 3]).astype(dtype)
    length = LENGTHS[li].astype(dtype)
    r = np.arccos(np.maximum(np.minimum(d, 1), -1)) / length
    t = np.sqrt(sq) / length
    r_seg = np.full((p.shape[0],) + last.shape, np.nan, dtype=dtype)
    t_seg = r_seg.copy()
    r_seg[:, f, li], t_seg[:, f, li] = r, t
    means = np.full((p.shape[0], 2, 8), np.nan, dtype=dtype)
    for k in range(8):
        if has[:, k].any():
            rows = np.nonzero(has[:, k])[0]
            means[:, 0, k] = np.cumsum(r_seg[:, rows, k], axis=1, dtype=dtype)[:, -1] / dtype(rows.size)    # left to right
            means[:, 1, k] = np.cumsum(t_seg[:, rows, k], axis=1, dtype=dtype)[:, -1] / dtype(rows.size)
    return r_seg, t_seg, means


def pose2motion_restated(poses, speed=None, dtype=np.float64):
    """mvosr_pose2motion_batch: motions (C, n, 12) — re-scaled like change_scale.py with ``speed`` — and the norms (C, n)."""
    p = np.asarray(poses, dtype=dtype)
    p = p.reshape((-1,) + p.shape[-2:]) if p.ndim == 3 else p.reshape((1,) + p.shape)
    p = p.reshape(p.shape[0], -1, 3, 4)
    m = mul(inv(p[:, :-1]), p[:, 1:])
    norms = norm3(m[..., 3])
    if speed is not None:
        m[..., 3] = (np.asarray(speed, dtype=dtype)[None, :, None] * m[..., 3]) / (norms + dtype(0.00001))[..., None]
    return m.reshape(p.shape[0], -1, 12), norms


def change_scale_restated(poses, speed, dtype=np.float64):
    m, _ = pose2motion_restated(poses, speed, dtype)
    return paths_restated(m, None, dtype)


# ---- the reference's own formulation, vectorised: np.linalg.inv and matmul on stacks of 4 x 4 matrices ----------------------------------
def to44(p):
    p = np.asarray(p, dtype=np.float64)
    out = np.zeros(p.shape[:-1] + (4, 4))
    out[..., :3, :] = p.reshape(p.shape[:-1] + (3, 4))
    out[..., 3, 3] = 1.0
    return out


def paths_numpy(motions, scales):
    """offline.get_path for every case at once: the loop over the frames stays (the chain), the cases are a stack."""
    m = np.asarray(motions, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64)
    steps = np.broadcast_to(m, scales.shape + (12,)).copy()
    steps[..., 3:12:4] = steps[..., 3:12:4] * scales[..., None]
    steps = to44(steps)
    pose = np.broadcast_to(np.eye(4), (scales.shape[0], 4, 4)).copy()
    out = np.zeros((scales.shape[0], m.shape[0] + 1, 12))
    out[:, 0] = pose[:, :3].reshape(-1, 12)
    for i in range(m.shape[0]):
        pose = pose @ steps[:, i]
        out[:, i + 1] = pose[:, :3].reshape(-1, 12)
    return out


def score_numpy(gt, paths, last):
    """evaluate.repeat_scores without its loops: (r_seg, t_seg, means) shaped like :func:`score_restated`'s."""
    g, p = to44(gt), to44(paths)
    has = last >= 0
    f, li = np.nonzero(has)
    first, lst = f * STEP, last[f, li]
    r_seg = np.full((p.shape[0],) + last.shape, np.nan)
    t_seg = r_seg.copy()
    means = np.full((p.shape[0], 2, 8), np.nan)
    if f.size == 0:
        return r_seg, t_seg, means
    gd = np.linalg.inv(g[first]) @ g[lst]
    q = np.linalg.inv(p[:, first]) @ p[:, lst]
    e = np.linalg.inv(q) @ gd[None]
    d = 0.5 * (e[..., 0, 0] + e[..., 1, 1] + e[..., 2, 2] - 1)
    length = LENGTHS[li].astype(np.float64)
    r_seg[:, f, li] = np.arccos(np.maximum(np.minimum(d, 1.0), -1.0)) / length
    t_seg[:, f, li] = np.sqrt(e[..., 0, 3] * e[..., 0, 3] + e[..., 1, 3] * e[..., 1, 3] + e[..., 2, 3] * e[..., 2, 3]) / length
    for k in range(8):
        rows = np.nonzero(has[:, k])[0]
        if rows.size:
            means[:, 0, k] = np.cumsum(r_seg[:, rows, k], axis=1)[:, -1] / rows.size
            means[:, 1, k] = np.cumsum(t_seg[:, rows, k], axis=1)[:, -1] / rows.size
    return r_seg, t_seg, means


def pose2motion_numpy(poses):
    p = to44(poses)
    return (np.linalg.inv(p[..., :-1, :, :]) @ p[..., 1:, :, :])[..., :3, :].reshape(p.shape[:-3] + (p.shape[-3] - 1, 12))


def scores_from_means(means, columns):
    """The tra / rot tables of evaluate.repeat_scores from the kernel's means."""
    return np.asarray(means[:, 1, :][:, columns], dtype=np.float64), np.asarray(means[:, 0, :][:, columns] * 180 / np.pi, dtype=np.float64)


# ---- the tolerance rule -------------------------------------------------------------------------------------------------------------
def within(value, reference, gap, what="", gaps=GAPS):
    """Every float within ``gaps`` x gap of the reference's value; NaN exactly where the reference has NaN.  Returns the largest
    deviation in gaps (printed by the tests before they assert)."""
    value, reference = np.asarray(value, dtype=np.float64), np.asarray(reference, dtype=np.float64)
    assert value.shape == reference.shape, (what, value.shape, reference.shape)
    assert np.array_equal(np.isnan(value), np.isnan(reference)), (what, "NaN pattern")
    if value.size == 0 or np.isnan(reference).all():
        return 0.0
    dev = float(np.nanmax(np.abs(value - reference)))
    assert gap > 0, (what, "the fixture's gap must be positive", gap)
    print("%-28s deviation %.3e  gap %.3e  = %.2f gaps" % (what, dev, gap, dev / gap))
    assert dev <= gaps * gap, (what, dev, gap, dev / gap)
    return dev / gap


# ---- launch helpers: every output between sentinel guards ----------------------------------------------------------------------------
GUARD = 64          # bytes on either side
SENTINEL = 0xA5


class Guarded:
    """A device output of ``shape`` with GUARD sentinel bytes before and after it; ``read()`` checks them."""

    def __init__(self, ctx, shape, dtype):
        self.ctx, self.shape, self.dtype = ctx, tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.buf = ctx.empty(self.nbytes + 2 * GUARD, np.uint8).fill(SENTINEL)
        self.ptr = self.buf.ptr + GUARD

    def read(self):
        raw = self.buf.download()
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + self.nbytes:] == SENTINEL).all(), "a guard byte was overwritten"
        return raw[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape).copy()


def launch_paths(ctx, motions, scales, cases=None, case_stride=0):
    m = np.ascontiguousarray(motions, dtype=np.float64)
    n = m.shape[-2]
    cases = np.shape(scales)[0] if scales is not None else (cases or 1)
    d_m = ctx.to_device(m.reshape(-1))
    d_s = ctx.to_device(np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)) if scales is not None else None
    out = Guarded(ctx, (cases, n + 1, 12), np.float64)
    rc = ctx.lib.mvosr_paths_batch(ctx.handle, n, cases, d_m.ptr, case_stride, d_s.ptr if d_s is not None else None, out.ptr)
    assert rc == 0, (rc, ctx.lib.mvosr_last_error())
    return out.read()


def launch_table(ctx, gt):
    g = np.ascontiguousarray(gt, dtype=np.float64).reshape(-1, 12)
    n = g.shape[0]
    F = int(ctx.lib.mvosr_score_firsts(n))
    assert F == (n + STEP - 1) // STEP
    d_g = ctx.to_device(g)
    dist, last, gd, st = Guarded(ctx, (n,), np.float64), Guarded(ctx, (F, 8), np.int32), Guarded(ctx, (F, 8, 24), np.float64), Guarded(ctx, (1,), np.int32)
    rc = ctx.lib.mvosr_segment_table(ctx.handle, n, d_g.ptr, dist.ptr, last.ptr, gd.ptr, st.ptr)
    assert rc == 0, (rc, ctx.lib.mvosr_last_error())
    return {"dist": dist.read(), "last": last.read(), "gdelta": gd.read(), "status": st.read(), "_dev": (last, gd)}


def launch_score(ctx, table, paths, rows=True):
    p = np.ascontiguousarray(paths, dtype=np.float64)
    cases, n_rows = p.shape[0], p.shape[1]
    F = table["last"].shape[0]
    d_p = ctx.to_device(p)
    last, gd = table["_dev"]
    r, t = Guarded(ctx, (cases, F, 8), np.float64), Guarded(ctx, (cases, F, 8), np.float64)
    means, counts, st = Guarded(ctx, (cases, 2, 8), np.float64), Guarded(ctx, (cases, 8), np.int32), Guarded(ctx, (cases,), np.int32)
    rc = ctx.lib.mvosr_score_cases_batch(ctx.handle, cases, n_rows, d_p.ptr, F, last.ptr, gd.ptr, r.ptr if rows else None,
                                         t.ptr if rows else None, means.ptr, counts.ptr, st.ptr)
    assert rc == 0, (rc, ctx.lib.mvosr_last_error())
    return {"r_seg": r.read(), "t_seg": t.read(), "means": means.read(), "counts": counts.read(), "status": st.read()}


def launch_pose2motion(ctx, poses, speed=None):
    p = np.ascontiguousarray(poses, dtype=np.float64)
    p = p.reshape((1,) + p.shape) if p.ndim == 2 else p
    cases, n = p.shape[0], p.shape[1] - 1
    d_p = ctx.to_device(p)
    d_s = ctx.to_device(np.ascontiguousarray(speed, dtype=np.float64)) if speed is not None else None
    m, nr, st = Guarded(ctx, (cases, n, 12), np.float64), Guarded(ctx, (cases, n), np.float64), Guarded(ctx, (cases,), np.int32)
    rc = ctx.lib.mvosr_pose2motion_batch(ctx.handle, cases, n, d_p.ptr, d_s.ptr if d_s is not None else None, m.ptr, nr.ptr, st.ptr)
    assert rc == 0, (rc, ctx.lib.mvosr_last_error())
    return {"motions": m.read(), "norms": nr.read(), "status": st.read()}

