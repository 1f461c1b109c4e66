"""Crafted lists, the plain restatement and the launcher for static_tri_kernel (csrc/mvosr_statictri.hip, mvosr_static_tri_batch)
— shared by tests/test_statictri_cases.py (CPU), tests/test_gpu_statictri.py and tests/golden/make_golden_statictri.py.  Test
infrastructure.

The restatement states road_model_calculation_static_tri (/root/reference/src/scale_calculator.py:294-310 with check_mode
:446-483) without NumPy's histogram routine: a value's bin is decided by comparing it against ``float(k) * 0.1``.
"""
from __future__ import annotations

import os

import numpy as np

N_BINS = 19
EDGES = [float(k) * 0.1 for k in range(N_BINS + 1)]            # np.array(range(0, 20)) * 0.1, :297
ST_MODE, ST_MEDIAN, ST_ERR_MASK, ST_RS_FEW = 0, 2, 8, 11
ABS_REF, WINDOW = 1.75, 5
NAN = float("nan")


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def bin_of(hi):
    """edges[k] <= hi < edges[k+1]; the last bin also holds edges[19]; -1 outside."""
    for k in range(N_BINS):
        if EDGES[k] <= hi < EDGES[k + 1]:
            return k
    return N_BINS - 1 if hi == EDGES[N_BINS] else -1


def hist_of(hi):
    dis = [0] * N_BINS
    for v in hi:
        k = bin_of(float(v))
        if k >= 0:
            dis[k] += 1
    return [0 if d == 1 else d for d in dis]                    # :299


def mode_of(dis):
    """None where check_mode finds no modes, else (mode_left + mode_right) / 2 / 10 of the FIRST run of flagged bins."""
    mx = max(dis)
    if mx <= 2:                                                 # :451-452
        return None
    flag = [False] * N_BINS
    flag[0] = dis[0] == mx                                      # :454-458
    flag[-1] = dis[-1] == mx
    for k in range(1, N_BINS - 1):                              # :459-463
        flag[k] = dis[k] >= dis[k - 1] and dis[k] >= dis[k + 1] and float(dis[k]) >= 0.33 * float(mx) and dis[k] >= 2
    i = flag.index(True)
    j = i
    while j + 1 < N_BINS and flag[j + 1]:                       # :473-481: upper edges of adjacent bins differ by less than 0.11
        j += 1
    return ((i + 1) + (j + 1)) / 2.0 / 10.0                     # :306-310 with int(edges[k] * 10) == k


def static_tri_of(h, min_count=0, absolute_reference=ABS_REF):
    """What mvosr_static_tri_batch writes for one list of counted heights: {"scale_norm", "raw_scale", "status", "n_used", "hist"}."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    n = int(h.size)
    out = {"n_used": n, "hist": np.zeros(N_BINS, np.int32), "scale_norm": np.float64(NAN), "raw_scale": np.float64(NAN)}
    if not bool(np.all(np.isfinite(h) & (h > 0))):
        out["status"] = ST_ERR_MASK
        return out
    if n == 0 or n <= min_count:
        out["status"] = ST_RS_FEW
        return out
    with np.errstate(over="ignore"):
        hi = np.float64(1.0) / h                                # :296
    dis = hist_of(hi)
    out["hist"] = np.array(dis, dtype=np.int32)
    m = mode_of(dis)
    if m is None:                                               # :302-303: np.median over ALL values
        s = np.sort(hi)
        with np.errstate(over="ignore"):
            m = s[n // 2] if n & 1 else (s[n // 2 - 1] + s[n // 2]) / np.float64(2.0)
        out["status"] = ST_MEDIAN
    else:
        out["status"] = ST_MODE
    out["scale_norm"] = np.float64(m)
    out["raw_scale"] = np.float64(m) * np.float64(absolute_reference)
    return out


def carry(raw_scale, status, scale=1):
    """rescale.py:181-187 over a run of lists: a list with more than 12 heights sets the scale, any other returns it as it stands."""
    out = np.empty(len(raw_scale), dtype=np.float64)
    for f in range(len(raw_scale)):
        if status[f] != ST_RS_FEW:
            scale = raw_scale[f]
        out[f] = scale
    return out


# ---- crafted lists ---------------------------------------------------------------------------------------------------------------
def h_for(hi):
    """A height whose IEEE reciprocal is exactly ``hi``, or None: 1/h skips doubles wherever a step of h moves it by more than an ulp."""
    hi = np.float64(hi)
    with np.errstate(all="ignore"):
        h0 = np.float64(1.0) / hi
        if not np.isfinite(h0) or h0 <= 0:
            return None
        for toward in (np.float64(0.0), np.float64(np.inf)):
            x = h0
            for _ in range(6):
                if np.float64(1.0) / x == hi:
                    return x
                x = np.nextafter(x, toward)
    return None


def reachable(hi, toward):
    """(h, 1/h) with 1/h the value nearest to ``hi`` on the side ``toward`` (hi itself where a height gives it)."""
    v = np.float64(hi)
    for _ in range(64):
        h = h_for(v)
        if h is not None:
            return h, v
        v = np.nextafter(v, np.float64(toward))
    raise AssertionError("no reachable value near %r" % hi)


def heights_of(hi_values):
    """Heights whose reciprocals are exactly ``hi_values`` (asserted)."""
    hs = []
    for v in hi_values:
        h = h_for(v)
        assert h is not None and np.float64(1.0) / h == np.float64(v), v
        hs.append(h)
    return np.array(hs, dtype=np.float64)


def from_counts(counts, seed, tail=(), shuffle=True):
    """A list with counts[k] values strictly inside bin k (a hundredth away from its edges) and the inverse heights ``tail``
    outside the bins.  Asserted: the restatement's raw histogram of the list is ``counts``."""
    rng = np.random.default_rng(seed)
    hi = []
    for k, c in enumerate(counts):
        hi += list(rng.uniform(EDGES[k] + 0.01, EDGES[k + 1] - 0.01, int(c)))
    hi += [float(t) for t in tail]
    hi = np.array(hi, dtype=np.float64)
    if shuffle:
        rng.shuffle(hi)
    h = np.float64(1.0) / hi
    raw = [0] * N_BINS
    for v in np.float64(1.0) / h:
        if bin_of(float(v)) >= 0:
            raw[bin_of(float(v))] += 1
    assert raw == [int(c) for c in counts] + [0] * (N_BINS - len(counts)), (raw, counts)
    return h


def _counts(**at):
    c = [0] * N_BINS
    for k, v in at.items():
        c[int(k[1:])] = v
    return c


def edge_values():
    """[(k, side, h, hi)]: for every edge k = 1..19 the inverse height on it, the nearest one below and the nearest one above
    (side -1 / 0 / +1) that some height produces; an edge no height produces exactly is left out (its neighbours stay)."""
    out = []
    for k in range(1, N_BINS + 1):
        e = np.float64(EDGES[k])
        below = reachable(np.nextafter(e, np.float64(0.0)), 0.0)
        above = reachable(np.nextafter(e, np.float64(2.0)), 2.0)
        assert below[1] < e < above[1]
        out.append((k, -1) + below)
        if h_for(e) is not None:
            out.append((k, 0, h_for(e), e))
        out.append((k, 1) + above)
    return out


def crafted():
    """name -> heights (float64).  Every list but the short ones has more than 12 entries."""
    c = {}
    ev = edge_values()
    on_edge = [k for k, side, _, _ in ev if side == 0]
    assert len(on_edge) >= 16 and 19 in on_edge and 3 in on_edge, on_edge
    base = from_counts(_counts(b5=9, b6=14, b7=8), 1)
    c["empty"] = np.zeros(0)
    c["n12"] = base[:12].copy()
    c["n13"] = base[:13].copy()
    for n in (63, 64, 65, 129):                                 # the lanes of a step and the step boundary; one far-out tail value each
        per = [0] * N_BINS
        for i in range(n - 1):
            per[(3 + i % 5)] += 1
        c["len%d" % n] = from_counts(per, 10 + n, tail=[7.5 + n])
    # every edge: the value on it (where a height gives it), the nearest below and above — three copies each, so that a value in
    # the wrong bin changes a count that is not zeroed
    c["edges_all"] = np.array([h for _, _, h, _ in ev for _ in range(3)], dtype=np.float64)
    for k in (1, 3, 6, 10, 14, 19):                            # one edge at a time on top of a low floor: the bins next to it decide
        vals = [(h, hi) for kk, _, h, hi in ev if kk == k]
        floor = from_counts([2] * N_BINS, 100 + k)
        c["edge%d" % k] = np.concatenate([floor, np.array([h for h, _ in vals for _ in range(2)])])
    c["above_e19"] = np.concatenate([from_counts(_counts(b17=3, b18=5), 3, tail=[2.5] * 6),
                                     np.array([h for kk, s, h, _ in ev if kk == 19 and s >= 0] * 4)])
    tiny = reachable(np.float64(1.0) / np.finfo(np.float64).max, 1.0)
    c["bin0_low_end"] = np.concatenate([from_counts(_counts(b0=4, b1=2), 4, tail=[3.0] * 8), np.array([tiny[0]] * 3)])
    c["all_ones"] = from_counts([1] * N_BINS, 5)                # every bin exactly 1: zeroed, no modes, the median of 19
    c["max2"] = from_counts(_counts(b4=2, b5=2, b6=2, b9=1, b12=2), 6, tail=[2.2, 2.4, 3.1, 5.0, 9.0])        # median exit, n = 14
    c["max3"] = from_counts(_counts(b4=2, b5=3, b6=2, b9=1, b12=2), 7, tail=[2.2, 2.4, 3.1, 5.0, 9.0])        # mode exit
    c["median_odd"] = from_counts(_counts(b2=2, b5=2, b8=2, b11=2, b14=2, b3=1, b6=1, b9=1), 8, tail=[2.0, 2.7])   # n = 15
    c["median_even"] = from_counts(_counts(b2=2, b5=2, b8=2, b11=2, b14=2, b3=1, b6=1, b9=1), 9, tail=[2.0, 2.7, 4.0])   # n = 16
    c["median_above"] = from_counts(_counts(b2=2, b7=2, b16=1), 10, tail=list(np.linspace(1.95, 40.0, 30)) + [1e300])
    c["median_above_even"] = from_counts(_counts(b2=2, b7=2), 11, tail=list(np.linspace(1.95, 40.0, 29)) + [1e300])
    c["median_repeats"] = heights_of([reachable(0.55, 1.0)[1]] * 2 + [reachable(0.85, 1.0)[1]] * 2 + [reachable(2.5, 3.0)[1]] * 9
                                     + [reachable(3.5, 4.0)[1]] * 3)                                            # even n, the middle pair equal
    c["plateau2"] = from_counts(_counts(b3=20, b4=20, b2=5, b5=6), 12)      # (4 + 5) / 2 / 10 = 0.45
    c["plateau3"] = from_counts(_counts(b6=15, b7=15, b8=15, b5=3), 13)     # 0.8
    c["max_bin0"] = from_counts(_counts(b0=30, b1=10, b5=8), 14)            # 0.1 (bin 5: a second run)
    c["max_bin0_1"] = from_counts(_counts(b0=30, b1=30, b2=4), 15)          # 0.15
    c["max_bin18"] = from_counts(_counts(b18=25, b17=6, b3=2), 16)          # 1.9
    c["first_run_not_max"] = from_counts(_counts(b3=40, b10=100, b2=7, b9=30), 17)      # 0.4, not 1.1
    for v in (32, 33, 34):                                      # around 0.33 * max: the reference decides them
        c["rel%d" % v] = from_counts(_counts(b2=v, b1=5, b3=4, b10=100), 18 + v)
    c["runs_k_k2"] = from_counts(_counts(b4=20, b5=3, b6=20), 60)           # bins 4 and 6: separate runs -> 0.5
    c["local_max_2"] = from_counts(_counts(b2=2, b8=6, b7=3), 61, tail=[2.3, 2.9, 4.4])  # bin 2: exactly 2 beside a maximum of 6 -> 0.3
    c["local_max_2_low"] = from_counts(_counts(b2=2, b8=7, b7=3), 62, tail=[2.3, 2.9])   # 2 < 0.33 * 7: bin 8 alone -> 0.9
    return c


def refused():
    """name -> a list with one invalid counted height: MVOSR_ST_ERR_MASK / ValueError."""
    base = from_counts(_counts(b5=9, b6=14, b7=8), 1)
    out = {}
    for name, bad in (("zero", 0.0), ("negative", -1.7), ("nan", np.nan), ("inf", np.inf), ("neg_zero", -0.0)):
        h = base.copy()
        h[len(h) // 2] = bad
        out[name] = h
    return out


N_RANDOM = 600


def random_lists(seed=20261018):
    """The 600 random lists of the golden: five mixes of inverse heights, 13 to 200 entries each (the first and the last mix
    every other time 13 to 29: few enough to leave every bin at 2 or below)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N_RANDOM):
        n = int(rng.integers(13, 201))
        kind = i % 5
        if kind in (0, 4) and (i // 5) % 2 == 0:                # short lists of the two wide mixes: the ones that find no mode
            n = int(rng.integers(13, 30))
        if kind == 0:
            hi = rng.uniform(0.0, 2.2, n)
        elif kind == 1:
            hi = rng.normal(0.6, 0.04, n)
        elif kind == 2:
            hi = np.round(rng.uniform(0.1, 2.0, n), 1)
        elif kind == 3:
            hi = np.where(rng.random(n) < 0.4, rng.normal(0.45, 0.05, n), rng.normal(1.1, 0.12, n))
        else:
            hi = rng.uniform(1.7, 2.5, n)
        hi = np.maximum(np.abs(hi), 1e-3)
        out.append(np.float64(1.0) / hi)
    return out


def checksum(lists):
    from mvoscalerecovery_amd import synth
    return synth.checksum(*[np.ascontiguousarray(a, dtype=np.float64) for a in lists])


N_SEQUENCE = 60
THIN_AT = {7: 12, 8: 12, 21: 12, 22: 14, 40: 12, 55: 14}          # frame -> features kept: 9 to 16 heights, around rescale.py:181's 12


def sequence_frames():
    """The 60 frames of the sequence golden: 300-600 features, the frames THIN_AT thinned to a dozen."""
    from mvoscalerecovery_amd import synth
    frames = []
    for i in range(N_SEQUENCE):
        f3, f2 = synth.synth_frame(700 + i, 300 + 23 * (i % 14), base_seed=1357, upper_fraction=0.1)
        if i in THIN_AT:
            f3, f2 = f3[:THIN_AT[i]].copy(), f2[:THIN_AT[i]].copy()
        frames.append((f3, f2))
    return frames


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "statictri.npz"), allow_pickle=False)


# ---- launcher (GPU) --------------------------------------------------------------------------------------------------------------
FIELDS = ("scale_norm", "raw_scale", "n_used", "hist", "status")


def run_lists(ctx, lists, min_count=0, absolute_reference=ABS_REF, rows=None, with_cnt=False, sentinel=None, hist=True):
    """mvosr_static_tri_batch over ``lists`` as ONE launch -> one dict per list.  ``rows`` None: the packed form (flags NULL).
    ``rows`` = a generator seed: the row form — uncounted rows (flags & 1 == 0) carrying garbage heights, NaN among them, are
    interleaved between the counted ones, and the counted rows' flags carry other bits at random.  ``with_cnt``: the lengths in
    cnt, with a gap of unused rows between the lists; else off has one more entry.  ``sentinel``: every output byte is pre-set
    to it and each buffer has a guard element -> (results, guards)."""
    from mvoscalerecovery_amd import _lib
    import flat_cases as fc
    F = len(lists)
    hs, fls, lens = [], [], []
    rng = np.random.default_rng(rows) if rows is not None else None
    for h in lists:
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if rng is None:
            hs.append(h)
            fls.append(np.ones(h.size, np.uint8))
        else:
            m = h.size + int(rng.integers(0, h.size + 5))
            counted = np.zeros(m, bool)
            counted[rng.permutation(m)[:h.size]] = True
            row_h = rng.choice([np.nan, -1.0, 0.0, np.inf, 0.37, 1e-320], m)
            row_h[counted] = h
            fl = (rng.integers(0, 4, m).astype(np.uint8) << 1) | counted.astype(np.uint8)
            hs.append(row_h)
            fls.append(fl)
        lens.append(hs[-1].size)
    gap = 3 if with_cnt else 0
    off = np.zeros(F + 1, dtype=np.int64)
    for i, n in enumerate(lens):
        off[i + 1] = off[i] + n + gap
    total = max(int(off[-1]), 1)
    height = np.full(total, np.nan)
    flags = np.full(total, 1, np.uint8)                          # (a gap row would count: the launch must not reach it)
    for i in range(F):
        height[off[i]:off[i] + lens[i]] = hs[i]
        flags[off[i]:off[i] + lens[i]] = fls[i]
    d = {"off": ctx.to_device(off if not with_cnt else off[:-1].copy() if F else off), "height": ctx.to_device(height)}
    if with_cnt:
        d["cnt"] = ctx.to_device(np.array(lens, dtype=np.int32) if F else np.zeros(1, np.int32))
    if rows is not None:
        d["flags"] = ctx.to_device(flags)
    spec = {"scale_norm": (max(F, 1), np.float64), "raw_scale": (max(F, 1), np.float64), "n_used": (max(F, 1), np.int32),
            "hist": ((max(F, 1), N_BINS), np.int32), "status": (max(F, 1), np.int32)}
    o = fc._alloc(ctx, spec, sentinel)
    ptr = lambda k: d[k].ptr if k in d else None
    _lib.check(ctx.lib.mvosr_static_tri_batch(ctx.handle, F, d["off"].ptr, ptr("cnt"), d["height"].ptr, ptr("flags"), int(min_count),
                                              float(absolute_reference), o["scale_norm"].ptr, o["raw_scale"].ptr, o["n_used"].ptr,
                                              o["hist"].ptr if hist else None, o["status"].ptr), "mvosr_static_tri_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + list(d.values()))
    res = [{k: (r[k][i] if k != "status" and k != "n_used" else int(r[k][i])) for k in FIELDS} for i in range(F)]
    if sentinel is None:
        return res
    return res, fc._tails(r, {k: F for k in FIELDS})


def same(got, want):
    """The five outputs of one list, by bytes (NaN to NaN)."""
    def eq(a, b):
        a, b = np.float64(a), np.float64(b)
        return bool(np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()
    return (eq(got["scale_norm"], want["scale_norm"]) and eq(got["raw_scale"], want["raw_scale"])
            and int(got["status"]) == int(want["status"]) and int(got["n_used"]) == int(want["n_used"])
            and np.array_equal(np.asarray(got["hist"], dtype=np.int32), np.asarray(want["hist"], dtype=np.int32)))
