"""Crafted lists, the plain restatement and the launcher for featdist_kernel (csrc/mvosr_featdist.hip,
mvosr_feature_distribution_batch) — shared by tests/test_featdist_cases.py (CPU), tests/test_gpu_featdist.py and
tests/golden/make_golden_featdist.py.  Test infrastructure.

The restatement states the kernel's contract (include/mvosr.h) without NumPy's routines: a value's bin is decided by comparing it
against ``float(k) * 0.1``; mean and std are summed in an explicit statement of np.add.reduce's pairwise order, in Python floats;
the median is taken from a sorted copy.  The CPU test holds it to NumPy and, through the golden, to the reference.
"""
from __future__ import annotations

import math
import os

import numpy as np

N_BINS, WORDS, POPS = 169, 172, 3
EDGES = [float(k) * 0.1 for k in range(N_BINS + 1)]            # np.array(range(0, 170)) * 0.1, scale_calculator.py:492
CLOSING = (29, 49, 99)                                         # the closing edges of :514, :528, :506
ST_ERR_MASK = 8
NAN = float("nan")
ABS_REF, WINDOW = 1.75, 5
LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 130, 136, 255, 256, 257, 1000, 1024, 2000)


def cap():
    """The largest frame the kernel's LDS plan holds (needs the built library, not a device)."""
    from mvoscalerecovery_amd import _lib
    return int(_lib.load().mvosr_featdist_max_features())


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def bin_of(y):
    """edges[k] <= y < edges[k+1]; the last bin also holds edges[169]; -1 outside (NaN: outside)."""
    if not (y >= EDGES[0] and y <= EDGES[N_BINS]):
        return -1
    lo, hi = 0, N_BINS                                          # edges[lo] <= y, by comparisons alone
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if y >= EDGES[mid]:
            lo = mid
        else:
            hi = mid
    return lo


def words_of(values):
    """The 172 words of a list: the 169 bins, then how many values are exactly edge 29, 49, 99."""
    w = [0] * WORDS
    for v in values:
        k = bin_of(v)
        if k >= 0:
            w[k] += 1
        for s, e in enumerate(CLOSING):
            if v == EDGES[e]:
                w[N_BINS + s] += 1
    return np.array(w, dtype=np.int32)


def pairwise_sum(a):
    """np.add.reduce of a float64 list of at most 8192 values: below 8 a plain loop from 0.0; up to 128 eight strided accumulators
    combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the remainder added one by one; above that the halves, the first rounded down
    to a multiple of 8, summed the same way and added."""
    n = len(a)
    assert n <= 8192
    if n < 8:
        res = 0.0
        for v in a:
            res += v
        return res
    if n <= 128:
        r = list(a[:8])
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] += a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += a[i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def left_to_right_sum(a):
    res = 0.0
    for v in a:
        res += v
    return res


def _div(a, b):
    """IEEE a / b in Python floats (0 / 0 and x / 0 as the hardware gives them)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def stats_of(values, total=pairwise_sum):
    """(mean, std, median) of a list of Python floats as np.mean / np.std / np.median give them; an empty list: NaNs."""
    a = [float(v) for v in values]
    n = len(a)
    if n == 0:
        return NAN, NAN, NAN
    mean = _div(total(a), float(n))
    sq = []
    for v in a:
        d = v - mean
        sq.append(d * d)
    var = _div(total(sq), float(n))
    std = math.sqrt(var) if var >= 0 else NAN                  # (a NaN variance: NaN)
    if any(v != v for v in a):
        median = NAN
    else:
        s = sorted(a)
        median = (0.0 + s[n // 2]) / 1.0 if n & 1 else _div((0.0 + s[n // 2 - 1]) + s[n // 2], 2.0)
    return mean, std, median


def featdist_of(y, level, scale):
    """What mvosr_feature_distribution_batch writes for one frame: {"n"[3], "hist"[3,172], "hist_scaled"[3,172], "stats"[3,3], "status"}."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    level = np.asarray(level, dtype=np.uint8).reshape(-1)
    assert y.size == level.size
    out = {"n": np.zeros(POPS, np.int32), "hist": np.zeros((POPS, WORDS), np.int32), "hist_scaled": np.zeros((POPS, WORDS), np.int32),
           "stats": np.full((POPS, 3), NAN), "status": 0}
    if np.any(level > 2):
        out["status"] = ST_ERR_MASK
        return out
    for p in range(POPS):
        vals = [float(v) for v, l in zip(y, level) if l >= p]
        out["n"][p] = len(vals)
        out["hist"][p] = words_of(vals)
        with np.errstate(all="ignore"):
            out["hist_scaled"][p] = words_of([float(np.float64(v) * np.float64(scale)) for v in vals])
        out["stats"][p] = stats_of(vals)
    return out


# ---- what the reference's methods derive from the kernel's outputs ------------------------------------------------------------
def narrow(words, bins):
    """np.histogram over np.array(range(0, bins + 1)) * 0.1 from the 172 words."""
    from mvoscalerecovery_amd import distribution
    return distribution.narrow_histogram(words, bins)


# ---- crafted lists ---------------------------------------------------------------------------------------------------------------
def mixed(n, seed):
    """n values around a road height with a share of far larger and far smaller ones, some negative: sums whose bits depend on the
    order of the additions."""
    rng = np.random.default_rng([20261019, seed])
    y = rng.normal(1.7, 0.6, n)
    far = rng.random(n) < 0.15
    y[far] *= 10.0 ** rng.uniform(-4, 3, int(far.sum()))
    y[rng.random(n) < 0.05] *= -1.0
    return y


def levels_for(n, seed, probs=(0.3, 0.4, 0.3)):
    return np.random.default_rng([77, seed]).choice(np.arange(3, dtype=np.uint8), size=n, p=probs)


def crafted(with_cap=True):
    """name -> (y float64, level uint8, scale)."""
    c = {}
    for n in LENGTHS + ((cap(),) if with_cap else ()):
        c["len%d" % n] = (mixed(n, n), levels_for(n, n, (0.0, 0.0, 1.0)), 1.0 + 0.001 * (n % 7))      # every feature in every population
    for n in (9, 130, 257, 1000):
        c["ragged%d" % n] = (mixed(n, 5000 + n), levels_for(n, n), 0.93)
    # every edge, the doubles next to it on both sides, and what lies outside the bins
    e = np.array(EDGES)
    edge_vals = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                                [-0.0, -1.5, -1e-300, 16.9, 17.0, 1e300, np.inf, -np.inf]])
    c["edges_all"] = (edge_vals, (np.arange(edge_vals.size) % 3).astype(np.uint8), 1.0)
    c["edges_finite"] = (edge_vals[:-3].copy(), ((np.arange(edge_vals.size - 3) + 1) % 3).astype(np.uint8), 1.0)   # (the reference's own calls take it)
    close = np.array([EDGES[k] for k in CLOSING] * 3 + [np.nextafter(EDGES[k], 0.0) for k in CLOSING]
                     + [np.nextafter(EDGES[k], 99.0) for k in CLOSING] * 2 + [0.05, 1.7, 1.7, 2.85])
    c["closing_edges"] = (close, np.full(close.size, 2, np.uint8), 1.0)
    # the median
    c["median_n1"] = (np.array([1.25]), np.array([2], np.uint8), 1.0)
    c["median_n2"] = (np.array([2.5, 1.0000000000000002]), np.array([2, 2], np.uint8), 1.0)
    c["median_odd"] = (np.array([3.0, -1.0, 2.0, 7.5, 0.1, 2.0000000000000004, 1.9]), np.full(7, 2, np.uint8), 1.0)
    c["median_even"] = (np.array([3.0, -1.0, 2.0, 7.5, 0.1, 2.0000000000000004, 1.9, 1e-9]), np.full(8, 2, np.uint8), 1.0)
    c["median_duplicates"] = (np.array([1.0, 2.0, 2.0, 2.0, 2.0, 3.0, 0.5, 9.0, 2.0, 2.0]), np.full(10, 2, np.uint8), 1.0)
    c["median_all_equal"] = (np.full(66, 1.7), np.full(66, 2, np.uint8), 1.0)
    c["median_negative"] = (np.array([-3.0, -1.0, -2.0, -7.5, -0.1, -2.0000000000000004]), np.full(6, 2, np.uint8), 1.0)
    c["minus_zero"] = (np.array([-0.0]), np.array([2], np.uint8), 1.0)
    # the levels
    c["no_selection"] = (mixed(70, 901), levels_for(70, 901, (0.4, 0.6, 0.0)), 1.1)
    c["nothing_kept"] = (mixed(70, 902), np.zeros(70, np.uint8), 1.1)
    c["alternating"] = (mixed(200, 903), (np.arange(200) % 3).astype(np.uint8), 0.9)
    lv = levels_for(100, 904)
    lv[63] = 3
    c["level_3"] = (mixed(100, 904), lv, 1.0)
    # the scale
    on_edge = np.array([EDGES[k] / 2.0 for k in (1, 29, 49, 99, 168, 169)] * 2 + [0.3, 1.7])
    c["product_on_edge"] = (on_edge, np.full(on_edge.size, 2, np.uint8), 2.0)
    for name, s in (("scale_nan", np.nan), ("scale_inf", np.inf), ("scale_zero", 0.0), ("scale_negative", -1.0), ("scale_small", 0.37)):
        c[name] = (mixed(90, 905), levels_for(90, 905), s)
    return c


def checksum(cases):
    from mvoscalerecovery_amd import synth
    arrays = []
    for y, lv, s in cases.values():
        arrays += [np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(lv, dtype=np.uint8), np.array([s], dtype=np.float64)]
    return synth.checksum(*arrays)


# ---- crafted frames and the sequence (through the estimators) ----------------------------------------------------------------
N_SEQUENCE = 60
SEQ_SEED = 2468
THIN_AT = {9: 8, 17: 3, 30: 2, 44: 3}              # frame -> features kept: 8 reach no selection, 3 return early, 2 raise


def sequence_frames():
    """The 60 frames of the sequence golden, about 300 features each; the frames THIN_AT thinned to a handful."""
    from mvoscalerecovery_amd import synth
    frames = []
    for i in range(N_SEQUENCE):
        f3, f2 = synth.synth_frame(900 + i, 260 + 11 * (i % 9), base_seed=SEQ_SEED, upper_fraction=0.1)
        if i in THIN_AT:
            low = np.nonzero(f2[:, 1] > 185)[0][:THIN_AT[i]]
            keep = np.sort(np.concatenate([low, np.nonzero(f2[:, 1] <= 185)[0][:5]]))
            f3, f2 = f3[keep].copy(), f2[keep].copy()
        frames.append((f3, f2))
    return frames


def sequence_scales():
    return [float(s) for s in 0.8 + 0.4 * np.random.default_rng(SEQ_SEED).random(N_SEQUENCE)]


def crafted_frames():
    """name -> (f3, f2, scale): small frames at the reference's exits."""
    from mvoscalerecovery_amd import synth
    out = {}
    for name, n_low, idx in (("eight", 8, 1), ("three", 3, 2), ("two", 2, 3), ("none_below", 0, 4), ("four", 4, 5), ("forty", 40, 6)):
        f3, f2 = synth.synth_frame(idx, 300, base_seed=SEQ_SEED + 1, upper_fraction=0.1)
        low = np.nonzero(f2[:, 1] > 185)[0][:n_low]
        keep = np.sort(np.concatenate([low, np.nonzero(f2[:, 1] <= 185)[0][:4]]))
        out[name] = (f3[keep].copy(), f2[keep].copy(), 1.0 + 0.05 * idx)
    f3, f2 = synth.synth_frame(7, 500, base_seed=SEQ_SEED + 1, upper_fraction=0.1)
    out["full"] = (f3, f2, 1.07)
    return out


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "featdist.npz"), allow_pickle=False)


def replay(golden, pre, frames, scales):
    """The frames' restatements from the golden's levels, with the attributes as the reference leaves them (a frame that returns
    early or selects nothing keeps the earlier frame's)."""
    state = {"all": None, "cor": None, "flat": None}
    cum = np.zeros((3, WORDS), dtype=np.int64)
    out = []
    for i, ((f3, f2), s) in enumerate(zip(frames, scales)):
        low = f2[:, 1] > 185
        lv = golden[pre + "levels"][golden[pre + "levels_off"][i]:golden[pre + "levels_off"][i + 1]]
        assert lv.size == int(low.sum())
        r = featdist_of(f3[low, 1], lv, s)
        cum += r["hist_scaled"]
        state["all"] = (r["hist"][0], r["stats"][0])
        if lv.any():
            state["cor"] = (r["hist"][1], r["stats"][1])
        if r["n"][2] > 0:
            state["flat"] = (r["hist"][2], r["stats"][2])
        out.append((r, dict(state)))
    return out, cum


# ---- launcher (GPU) --------------------------------------------------------------------------------------------------------------
FIELDS = ("n", "hist", "hist_scaled", "stats", "status")


def run_frames(ctx, frames, sentinel=None, seq=None, max_feat=None, with_cnt=True):
    """mvosr_feature_distribution_batch over ``frames`` = [(y, level, scale)] as ONE launch -> one dict per frame.  ``with_cnt``: the
    lengths in cnt, with a gap of unused entries (level 3: the launch must not reach them) between the frames; else off has one
    more entry.  ``seq``: a device buffer [3][172] int64 the launch adds to.  ``sentinel``: every output byte is pre-set to it and
    each buffer has a guard element -> (results, guards)."""
    from mvoscalerecovery_amd import _lib
    import flat_cases as fc
    F = len(frames)
    lens = [int(np.asarray(y).size) for y, _, _ in frames]
    gap = 3 if with_cnt else 0
    off = np.zeros(F + 1, dtype=np.int64)
    for i, n in enumerate(lens):
        off[i + 1] = off[i] + n + gap
    total = max(int(off[-1]), 1)
    ys, lvs = np.full(total, np.nan), np.full(total, 3, np.uint8)
    for i, (y, lv, _) in enumerate(frames):
        ys[off[i]:off[i] + lens[i]] = y
        lvs[off[i]:off[i] + lens[i]] = lv
    d = {"off": ctx.to_device(off[:-1].copy() if (with_cnt and F) else off), "y": ctx.to_device(ys), "level": ctx.to_device(lvs),
         "scale": ctx.to_device(np.array([s for _, _, s in frames] or [1.0], dtype=np.float64))}
    if with_cnt:
        d["cnt"] = ctx.to_device(np.array(lens or [0], dtype=np.int32))
    G = max(F, 1)
    spec = {"n": ((G, POPS), np.int32), "hist": ((G, POPS, WORDS), np.int32), "hist_scaled": ((G, POPS, WORDS), np.int32),
            "stats": ((G, POPS, 3), np.float64), "status": (G, np.int32)}
    o = fc._alloc(ctx, spec, sentinel)
    mf = max(lens or [0]) if max_feat is None else int(max_feat)
    _lib.check(ctx.lib.mvosr_feature_distribution_batch(ctx.handle, F, d["off"].ptr, d["cnt"].ptr if with_cnt else None, d["y"].ptr,
                                                        d["level"].ptr, d["scale"].ptr, mf, o["n"].ptr, o["hist"].ptr, o["hist_scaled"].ptr,
                                                        o["stats"].ptr, o["status"].ptr, seq.ptr if seq is not None else None),
               "mvosr_feature_distribution_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + list(d.values()))
    res = [{k: (r[k][i] if k != "status" else int(r[k][i])) for k in FIELDS} for i in range(F)]
    if sentinel is None:
        return res
    return res, fc._tails(r, {k: F for k in FIELDS})


def same(got, want):
    """The outputs of one frame, by bytes (NaN to NaN: every NaN the kernel and the restatement produce is compared as NaN)."""
    if int(got["status"]) != int(want["status"]):
        return False
    for k in ("n", "hist", "hist_scaled"):
        if not np.array_equal(np.asarray(got[k], dtype=np.int32), np.asarray(want[k], dtype=np.int32)):
            return False
    return same_floats(got["stats"], want["stats"])


def same_floats(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()
