"""Crafted frames, the plain NumPy restatement and the launcher for depthcheck_kernel (csrc/mvosr_depthcheck.hip,
mvosr_depth_check_batch) — shared by tests/test_depthcheck_cases.py (CPU), tests/test_gpu_depthcheck.py and
tests/golden/make_golden_depthcheck.py.  Test infrastructure.

The restatement states the kernel's contract (include/mvosr.h) with NumPy's own operations, a block of rows at a time, so that the
n x n matrix of script/data_check.py:24-29 never exists: a 2100-point frame is 35 MB as a matrix, a block here at most 2 MB.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = np.array(list(range(-40, 20))) * 50                     # data_check.py:30
N_BINS, WORDS, POPS = 59, 62, 3
ST_NO_POINT, ST_ERR_MASK = 12, 8
NAN = float("nan")
BLOCK_VALUES = 1 << 18                                         # values of one block of rows: 2 MB of doubles


def plan():
    """The row block and the j tile, read from the plan header."""
    text = open(os.path.join(ROOT, "mvoscalerecovery_amd", "csrc", "mvosr_depthcheck_plan.hpp")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    return get("kDcRows"), get("kDcTile")


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _key(v):
    """Orders doubles as numbers, +0.0 above -0.0."""
    return (v, 0 if np.signbit(v) else 1)


def depth_check_of(y, z, level):
    """What mvosr_depth_check_batch writes for one frame: {"hist" [3, 59], "below" / "above" / "nan" / "n" [3] int64, "max" [3],
    "status"}.  data_check.py:20-32 on the points of each population, a block of rows at a time."""
    y, z = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(z, dtype=np.float64).reshape(-1)
    level = np.asarray(level, dtype=np.uint8).reshape(-1)
    assert y.size == z.size == level.size
    out = {"hist": np.zeros((POPS, N_BINS), np.int64), "below": np.zeros(POPS, np.int64), "above": np.zeros(POPS, np.int64),
           "nan": np.zeros(POPS, np.int64), "n": np.zeros(POPS, np.int64), "max": np.full(POPS, NAN), "status": 0}
    if np.any(level > 2):
        out["status"] = ST_ERR_MASK
        return out
    select_id = y > 0                                          # :20
    depth, lv = z[select_id], level[select_id]                 # :21
    with np.errstate(all="ignore"):
        v_n = y[select_id] / depth                             # :23
    n = depth.size
    if n == 0:
        out["status"] = ST_NO_POINT
        return out
    best = [None] * POPS
    rows = max(1, BLOCK_VALUES // n)
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        with np.errstate(all="ignore"):
            q = (depth[None, :] - depth[i0:i1, None]) / ((v_n[None, :] - v_n[i0:i1, None]) + 0.000001)     # :26-28
        m = np.minimum(lv[i0:i1, None], lv[None, :])
        for p in range(POPS):
            vals = q[m >= p]
            isnan = np.isnan(vals)
            good = vals[~isnan]
            out["hist"][p] += np.histogram(good, BINS)[0]
            out["below"][p] += int(np.count_nonzero(good < BINS[0]))
            out["above"][p] += int(np.count_nonzero(good > BINS[-1]))
            out["nan"][p] += int(np.count_nonzero(isnan))
            if good.size:
                top = float(good.max())
                if top == 0.0:                                 # a zero maximum: +0.0 if any +0.0 is there
                    top = 0.0 if np.any((good == 0.0) & ~np.signbit(good)) else -0.0
                if best[p] is None or _key(top) > _key(best[p]):
                    best[p] = top
    for p in range(POPS):
        out["n"][p] = int(np.count_nonzero(lv >= p))
        if out["n"][p] > 0 and out["nan"][p] == 0:
            out["max"][p] = best[p]
    assert np.array_equal(out["hist"].sum(1) + out["below"] + out["above"] + out["nan"], out["n"] * out["n"])
    return out


def table_of(results):
    """The frames' counts as the sequence tables hold them: int64 [3, 62] — the bins, below, above, nan — of the frames with status 0."""
    t = np.zeros((POPS, WORDS), np.int64)
    for r in results:
        if int(r["status"]) == 0:
            t[:, :N_BINS] += np.asarray(r["hist"], dtype=np.int64)
            t[:, N_BINS] += r["below"]
            t[:, N_BINS + 1] += r["above"]
            t[:, N_BINS + 2] += r["nan"]
    return t


def slope(p1, p2):
    """q of the pair (i = p1, j = p2), points as (y, depth)."""
    with np.errstate(all="ignore"):
        a, b = np.float64(p1), np.float64(p2)
        return float((b[1] - a[1]) / ((b[0] / b[1] - a[0] / a[1]) + 0.000001))


# ---- crafted frames --------------------------------------------------------------------------------------------------------------
EDGE_FIRST = (1.015625, 13.0)
EDGE_VALUES = (-2000.0, -50.0, 50.0, 950.0)


def edge_pair(edge, seed=0):
    """A second point (y, depth) whose pair with EDGE_FIRST has q == edge exactly: a seeded search — the depth difference is drawn,
    y is solved for and then moved ulp by ulp until the IEEE evaluation lands on the edge."""
    rng = np.random.default_rng([20261019, int(abs(edge)), seed])
    y1, z1 = EDGE_FIRST
    vn1 = y1 / z1
    for _ in range(20000):
        dz = rng.uniform(0.1, 0.9) * vn1 * abs(edge) if edge < 0 else rng.uniform(5.0, 200.0)
        z2 = z1 + dz
        vn2 = ((z2 - z1) / edge - 0.000001) + vn1
        if not vn2 > 0:
            continue
        y2 = vn2 * z2
        for toward in (np.inf, -np.inf):
            c = y2
            for _ in range(24):
                if slope(EDGE_FIRST, (c, z2)) == edge:
                    return float(c), float(z2)
                c = float(np.nextafter(c, toward))
    raise AssertionError("no pair found on edge %r" % edge)


def road(n, seed, levels=(0.3, 0.4, 0.3)):
    """n points of a rough road: heights around 1.7 below the camera, depths of 4 .. 80, a share of points off the road."""
    rng = np.random.default_rng([4242, seed, n])
    z = rng.uniform(4.0, 80.0, n)
    y = np.abs(rng.normal(1.7, 0.25, n)) + 0.05
    off = rng.random(n) < 0.1
    y[off] *= rng.uniform(0.1, 3.0, int(off.sum()))
    lv = rng.choice(np.arange(3, dtype=np.uint8), size=n, p=levels)
    return y, z, lv


def with_unselected(n_selected, extra, seed):
    """``n_selected`` road points with ``extra`` points of y <= 0 or NaN between them."""
    y, z, lv = road(n_selected + extra, seed)
    rng = np.random.default_rng([99, seed])
    drop = rng.permutation(n_selected + extra)[:extra]
    y[drop] = np.resize(np.array([0.0, -0.0, -1.5, np.nan, -np.inf]), extra)
    return y, z, lv


def crafted():
    """name -> (y float64, z float64, level uint8)."""
    rows, tile = plan()
    c = {}
    for n in (0, 1, 2, 63, 64, 65):
        c["selected%d" % n] = with_unselected(n, 5, n)
    for n in (rows - 1, rows, rows + 1, tile - 1, tile, tile + 1, 2 * tile + 1):
        c["plan%d" % n] = road(n, 1000 + n)
    c["synthetic2100"] = with_unselected(2100, 37, 2100)
    for k, e in enumerate(EDGE_VALUES):
        y2, z2 = edge_pair(e)
        c["edge%d" % k] = (np.array([EDGE_FIRST[0], y2]), np.array([EDGE_FIRST[1], z2]), np.array([2, 2], np.uint8))
    # equal depths: d_minus is +0.0 both ways, divided by a positive and a negative denominator: +0.0 and -0.0, both in the bin of 0
    # (a third point gives a positive slope: the maximum does not rest on which zero NumPy's reduction keeps)
    c["equal_depths"] = (np.array([1.0, 2.0, 9.0]), np.array([10.0, 10.0, 30.0]), np.array([2, 2, 2], np.uint8))
    c["duplicate"] = (np.array([1.5, 1.5, 1.25, 1.5]), np.array([20.0, 20.0, 9.0, 20.0]), np.array([2, 1, 2, 2], np.uint8))
    # one point of depth 0: v_n = +inf there; its diagonal is 0 / (inf - inf) = NaN, its row and column are -d / -inf and d / inf
    c["depth_zero"] = (np.array([1.5, 1.0, 2.0]), np.array([20.0, 0.0, 7.0]), np.array([2, 2, 2], np.uint8))
    c["depth_negative"] = (np.array([1.5, 1.0, 2.0, 1.7]), np.array([20.0, -5.0, 7.0, 33.0]), np.array([2, 2, 1, 0], np.uint8))
    c["unselected"] = (np.array([1.5, 0.0, -0.0, np.nan, -2.0, 1.0, np.inf]), np.array([20.0, 5.0, 6.0, 7.0, 8.0, 9.0, 11.0]),
                       np.array([2, 2, 2, 2, 2, 1, 0], np.uint8))
    c["none_selected"] = (np.array([0.0, -1.0, np.nan, -0.0]), np.array([5.0, 6.0, 7.0, 8.0]), np.array([2, 1, 0, 2], np.uint8))
    # slopes beyond both ends: nearly equal v_n with a large depth difference, either sign
    c["beyond"] = (np.array([1.0, 2.00001, 3.0003, 0.5]), np.array([10.0, 20.0, 30.0, 5.00001]), np.array([2, 2, 2, 2], np.uint8))
    y, z, _ = road(70, 31)
    c["population2_empty"] = (y, z, (np.arange(70) % 2).astype(np.uint8))
    c["population1_is_0"] = (y, z, np.where(np.arange(70) % 3 == 0, 2, 1).astype(np.uint8))
    c["endpoint_lower"] = (np.array([1.5, 1.7, 1.6]), np.array([20.0, 30.0, 8.0]), np.array([2, 0, 1], np.uint8))
    return c


def checksum(cases):
    from mvoscalerecovery_amd import synth
    arrays = []
    for y, z, lv in cases.values():
        arrays += [np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(lv, dtype=np.uint8)]
    return synth.checksum(*arrays)


def sequence_points(golden_featdist=None):
    """The 60 frames of featdist_cases.sequence_frames() as (y, z, level): the features below the vanishing row, with the levels the
    reference's run left in tests/golden/featdist.npz."""
    import featdist_cases as fdc
    g = golden_featdist if golden_featdist is not None else fdc.golden()
    out = []
    for i, (f3, f2) in enumerate(fdc.sequence_frames()):
        low = f2[:, 1] > 185
        lv = g["s_levels"][g["s_levels_off"][i]:g["s_levels_off"][i + 1]]
        assert lv.size == int(low.sum())
        out.append((f3[low, 1].copy(), f3[low, 2].copy(), lv.astype(np.uint8)))
    return out


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depthcheck.npz"), allow_pickle=False)


# ---- launcher (GPU) --------------------------------------------------------------------------------------------------------------
FIELDS = ("hist", "below", "above", "nan", "max", "n", "status")


def run_frames(ctx, frames, sentinel=None, tables=None, max_feat=None, with_cnt=True):
    """mvosr_depth_check_batch over ``frames`` = [(y, z, level)] as ONE launch -> one dict per frame.  ``with_cnt``: the lengths in
    cnt, with a gap of unused entries (level 3, y 1: the launch must not reach them) between the frames; else off has one more
    entry.  ``tables``: a device buffer [3][62] int64 the launch adds to.  ``sentinel``: every output byte is pre-set to it and
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
    ys, zs, lvs = np.full(total, 1.0), np.full(total, 1.0), np.full(total, 3, np.uint8)
    for i, (y, z, lv) in enumerate(frames):
        ys[off[i]:off[i] + lens[i]] = y
        zs[off[i]:off[i] + lens[i]] = z
        lvs[off[i]:off[i] + lens[i]] = lv
    d = {"off": ctx.to_device(off[:-1].copy() if (with_cnt and F) else off), "y": ctx.to_device(ys), "z": ctx.to_device(zs),
         "level": ctx.to_device(lvs)}
    if with_cnt:
        d["cnt"] = ctx.to_device(np.array(lens or [0], dtype=np.int32))
    G = max(F, 1)
    spec = {"hist": ((G, POPS, N_BINS), np.int64), "below": ((G, POPS), np.int64), "above": ((G, POPS), np.int64),
            "nan": ((G, POPS), np.int64), "max": ((G, POPS), np.float64), "n": ((G, POPS), np.int64), "status": (G, np.int32)}
    o = fc._alloc(ctx, spec, sentinel)
    params = _lib.DepthCheckParams(max(lens or [0]) if max_feat is None else int(max_feat), 0)
    outs = _lib.DepthCheckOutputs(*(o[k].ptr for k in FIELDS))
    _lib.check(ctx.lib.mvosr_depth_check_batch(ctx.handle, F, d["off"].ptr, d["cnt"].ptr if with_cnt else None, d["y"].ptr, d["z"].ptr,
                                               d["level"].ptr, C.byref(params), C.byref(outs), tables.ptr if tables is not None else None),
               "mvosr_depth_check_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + list(d.values()))
    res = [{k: (r[k][i] if k != "status" else int(r[k][i])) for k in FIELDS} for i in range(F)]
    if sentinel is None:
        return res
    return res, fc._tails(r, {k: F for k in FIELDS})


def same(got, want):
    """The outputs of one frame, by bytes (NaN to NaN)."""
    if int(got["status"]) != int(want["status"]):
        return False
    for k in ("hist", "below", "above", "nan", "n"):
        if np.ascontiguousarray(got[k], dtype=np.int64).tobytes() != np.ascontiguousarray(want[k], dtype=np.int64).tobytes():
            return False
    return same_floats(got["max"], want["max"])


def same_floats(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()
