"""Crafted scale sets for the scales' own score — evaluate.scale_errors / filter_scales, mvosr_scale_errors_batch and
mvosr_window_median_cases (csrc/mvosr_scalescore.hip) —, a NumPy restatement of the kernels' summation order, and launch helpers
through the C ABI.  tests/golden/scalescores.npz (make_golden_scalescores.py) holds what the reference's own script prints for
every set; the inputs are regenerated here from the seeds and checked against the stored checksum.

The sizes are the ones at which the kernel takes another path: no scale at all; fewer scales than the shortest window (no segment),
exactly one segment (n = 11, 21); window 100 over 137 values (a slice across the 128-element leaf); window 800 with one and two
segments (n = 811); more scales than a workgroup holds in LDS (n = 6000 > 5120); and more than 8192 segments of a window, so that a
mean's input crosses np.add.reduce's chunk (n = 83000 > 8192 x 10 + 10)."""
import zlib

import numpy as np

import scores_cases as sc

WINDOWS = [10, 20, 50, 100, 200, 300, 400, 500, 600, 700, 800]
STEP = 10
THRESHOLDS = [0.1, 0.2, 0.3, 0.5]
LDS_ERRORS = 5120                # kSsLdsErrors

# name -> n, n_gt, cases, seed, kind, filter windows kept in the golden
SETS = {
    "ten1000": (1000, 1000, 10, 101, "noisy", (10,)),
    "n0": (0, 5, 1, 102, "noisy", ()),
    "n1": (1, 1, 1, 103, "noisy", (1, 10)),
    "n9": (9, 40, 10, 104, "noisy", (1, 2, 5, 10)),          # every window longer than the sequence
    "n10": (10, 10, 1, 105, "noisy", ()),
    "n11": (11, 11, 3, 106, "noisy", ()),                     # exactly one segment of window 10
    "n21": (21, 30, 11, 107, "noisy", (1, 2, 5, 10)),
    "n137": (137, 137, 3, 108, "noisy", (5,)),                # window 100: a slice across the 128-element leaf
    "n811": (811, 900, 2, 109, "noisy", ()),                  # window 800: two segments; window 700 ... more
    "n801": (801, 801, 1, 110, "noisy", ()),                  # window 800: one segment
    "n6000": (6000, 6100, 2, 111, "noisy", ()),               # above the LDS-resident bound
    "n83000": (83000, 83000, 1, 112, "noisy", ()),            # 8299 segments of window 10: the mean's input crosses a chunk
    "nan": (300, 300, 3, 113, "nan", (2, 10)),
    "inf": (300, 310, 3, 114, "inf", (2, 10)),
    "cancel": (240, 240, 3, 115, "cancel", (10,)),
}
GT_RESCALED = "n257"             # the sequence of tests/scores_cases.py whose ground truth is re-scaled to its ten cases' scales


def make_set(name):
    """{"gt" (n_gt,), "scales" (C, n)}: speeds around 1 and scales off them by about 0.25, so that every threshold counts some."""
    n, n_gt, cases, seed, kind, _ = SETS[name]
    rng = np.random.RandomState(seed)
    gt = 0.8 + 0.4 * rng.rand(n_gt)
    scales = gt[:n] + 0.25 * rng.randn(cases, n)
    if kind == "nan":
        scales[1, 123] = np.nan                                   # one NaN scale, in one case
    elif kind == "inf":
        scales[0, 7] = np.inf
        scales[1, 150] = -np.inf
        scales[2, 20], scales[2, 25] = np.inf, -np.inf            # both in one window: its sum is NaN
    elif kind == "cancel":
        d = np.where(np.arange(n) % 2 == 0, 0.25, -0.25)          # errors of mixed sign that cancel in every window: exact sums
        gt = np.full(n_gt, 1.0)
        scales = np.stack([1.0 - d, 1.0 + d, 1.0 - 2 * d * (np.arange(n) % 4 < 2)])
    return {"gt": gt, "scales": np.ascontiguousarray(scales)}


def checksum(s):
    return int(zlib.crc32(np.ascontiguousarray(s["gt"]).tobytes() + np.ascontiguousarray(s["scales"]).tobytes()))


def rescaled_scales():
    """The ten cases' scales the ground truth of GT_RESCALED is re-scaled to: speeds around 12 m a frame."""
    n, cases = sc.SEQUENCES[GT_RESCALED][:2]
    rng = np.random.RandomState(257)
    return 12.0 + 1.5 * rng.randn(cases, n)


# ---- the kernels' summation order, restated in NumPy over a stack of lists (last axis) --------------------------------------------
def leaf_sum(a):
    """np_leaf_sum: below 8 values a plain loop from 0; else eight strided accumulators, combined pairwise, the rest one by one."""
    n = a.shape[-1]
    if n < 8:
        res = np.zeros(a.shape[:-1])
        for i in range(n):
            res = res + a[..., i]
        return res
    r = [a[..., j].copy() for j in range(8)]
    full = n - n % 8
    for i in range(8, full, 8):
        for j in range(8):
            r[j] = r[j] + a[..., i + j]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(full, n):
        res = res + a[..., i]
    return res


def pairwise(a):
    """One chunk (<= 8192 values): leaves of at most 128, halves with the first rounded down to a multiple of 8."""
    n = a.shape[-1]
    if n <= 128:
        return leaf_sum(a)
    m2 = n // 2
    m2 -= m2 % 8
    return pairwise(a[..., :m2]) + pairwise(a[..., m2:])


def np_sum(a):
    """block_np_sum: the chunks' pairwise sums added left to right, from 0."""
    total = np.zeros(a.shape[:-1])
    for c0 in range(0, a.shape[-1], 8192):
        total = total + pairwise(a[..., c0:c0 + 8192])
    return total


def errors_restated(gt, scales, windows=WINDOWS, step=STEP, thresholds=THRESHOLDS):
    """mvosr_scale_errors_batch: {"mean", "max" (C,), "counts" (C, T), "drift" (C, W)}."""
    gt, s = np.asarray(gt, dtype=np.float64), np.asarray(scales, dtype=np.float64)
    C, n = s.shape
    e = gt[:n] - s
    a = np.abs(e)
    nan = np.full(C, np.nan)
    with np.errstate(all="ignore"):
        out = {"mean": np_sum(a) / n if n else nan, "max": np.max(a, axis=1) if n else nan,
               "counts": np.array([[int(np.sum(a[c] > t)) for t in thresholds] for c in range(C)], dtype=np.int64).reshape(C, len(thresholds))}
        drift = np.full((C, len(windows)), np.nan)
        for k, w in enumerate(windows):
            m = len(range(0, n - w, step))
            if m:
                seg = np.lib.stride_tricks.sliding_window_view(e, w, axis=1)[:, 0:n - w:step]      # (C, m, w), a view
                drift[:, k] = np_sum(np.abs(pairwise(seg)) / w) / m
        out["drift"] = drift
    return out


def same(a, b):
    """Bit for bit, except that any NaN equals any NaN (the sign and payload of a NaN are the platform's)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


# ---- launch helpers: every output between sentinel guards (scores_cases.Guarded) ----------------------------------------------------
def launch_errors(ctx, gt, scales, windows=WINDOWS, step=STEP, thresholds=THRESHOLDS, flags=0):
    gt = np.ascontiguousarray(gt, dtype=np.float64)
    s = np.ascontiguousarray(scales, dtype=np.float64)
    C, n = s.shape
    w, t = np.ascontiguousarray(windows, dtype=np.int32), np.ascontiguousarray(thresholds, dtype=np.float64)
    d_gt, d_s = ctx.to_device(gt), ctx.to_device(s.reshape(-1))
    stats, counts = sc.Guarded(ctx, (C, 2), np.float64), sc.Guarded(ctx, (C, t.size), np.int32)
    drift, status = sc.Guarded(ctx, (C, w.size), np.float64), sc.Guarded(ctx, (C,), np.int32)
    rc = ctx.lib.mvosr_scale_errors_batch(ctx.handle, gt.size, d_gt.ptr, C, n, d_s.ptr, n, w.size, w.ctypes.data, step, t.size,
                                          t.ctypes.data, flags, stats.ptr, counts.ptr, drift.ptr, status.ptr)
    assert rc == 0, (rc, ctx.lib.mvosr_last_error())
    st = stats.read()
    return {"mean": st[:, 0].copy(), "max": st[:, 1].copy(), "counts": counts.read().astype(np.int64), "drift": drift.read(),
            "status": status.read()}


def launch_filter(ctx, data, window):
    d = np.ascontiguousarray(data, dtype=np.float64)
    C, n = d.shape
    d_in = ctx.to_device(d.reshape(-1))
    out = sc.Guarded(ctx, (C, n), np.float64)
    rc = ctx.lib.mvosr_window_median_cases(ctx.handle, d_in.ptr, C, n, n, int(window), out.ptr, n)
    assert rc == 0, (rc, ctx.lib.mvosr_last_error())
    return out.read()
