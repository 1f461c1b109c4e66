#!/usr/bin/env python3
"""Times mvosr_region_grow_batch with the context's HIP events on resident batches: 512 real triangulations
of 2000 features and of the ragged 300-1500 mix, in both forms (given heights / from points) — after warm-up, >= 20
repetitions, median and spread — and prints ONE JSON line: µs per frame, algorithmic bytes, the fraction of 8 TB/s (HBM peak),
and the host route the kernel replaces: tests/grow_cases.numpy_grow on the same frames on one core.

    python profiles/grow_bench.py [--frames 512] [--reps 20] [--out profiles/grow_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/grow_bench.py --reps 3 --no-cpu      # the kernel's share

Rows: SciPy's Delaunay of each frame's features below the vanishing row (64 distinct synthetic frames, repeated).  Algorithmic
bytes count each input and output once: given form, rows 12 B + heights and angles 16 B + region 1 B per row; from-points
form, rows 12 B + 24 B per feature + region 1 B per row."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mvoscalerecovery_amd import _lib, synth  # noqa: E402
from mvoscalerecovery_amd import graph as gg  # noqa: E402

HBM_PEAK = 8.0e12
VANISH = 185


def make_frames(sizes, seed):
    from scipy.spatial import Delaunay
    out = []
    for i, n in enumerate(sizes):
        f3, f2 = synth.synth_frame(i, int(n), base_seed=seed)
        low = f2[:, 1] > VANISH
        out.append((np.ascontiguousarray(f3[low]), Delaunay(f2[low]).simplices.astype(np.int32)))
    return out


def time_form(ctx, frames, given, reps, warmup=3):
    """One resident batch, one form; the values of the given form are the from-points form's own outputs."""
    F = len(frames)
    cnt = np.array([len(p) for p, _ in frames], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(t) for _, t in frames])]).astype(np.int64)
    P = np.concatenate([p for p, _ in frames])
    d = {"off": ctx.to_device(off), "cnt": ctx.to_device(cnt), "toff": ctx.to_device(toff),
         "tri": ctx.to_device(np.concatenate([t for _, t in frames]).reshape(-1)),
         "x": ctx.to_device(P[:, 0].copy()), "y": ctx.to_device(P[:, 1].copy()), "z": ctx.to_device(P[:, 2].copy())}
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.x, b.y, b.z = F, d["off"].ptr, d["cnt"].ptr, d["x"].ptr, d["y"].ptr, d["z"].ptr
    b.tri2_off, b.tri2, b.max_feat, b.total_feat = d["toff"].ptr, d["tri"].ptr, int(cnt.max()), int(off[-1])
    T, max_tri = int(toff[-1]), int(np.max(np.diff(toff)))
    o = {"region": ctx.empty(T, np.uint8), "n_region": ctx.empty(F, np.int32), "n_flat": ctx.empty(F, np.int32), "status": ctx.empty(F, np.int32),
         "level": ctx.empty(F, np.float64), "threshold_height": ctx.empty(F, np.float64),
         "tri_height": ctx.empty(T, np.float64), "tri_angle": ctx.empty(T, np.float64)}
    gp = _lib.GrowParams(8.0, gg.SEED_DEG, gg.LEVEL_DEG, gg.HEIGHT_FACTOR)
    go = _lib.GrowOutputs(**{k: v.ptr for k, v in o.items()})
    launch = lambda h, a, out: _lib.check(ctx.lib.mvosr_region_grow_batch(ctx.handle, C.byref(b), h, a, C.byref(gp), C.byref(out), max_tri),
                                          "mvosr_region_grow_batch")
    launch(None, None, go)                                  # (from points: fills tri_height / tri_angle)
    ctx.sync()
    if given:
        go = _lib.GrowOutputs(**{k: v.ptr for k, v in o.items() if not k.startswith("tri_")})
        call = lambda: launch(o["tri_height"].ptr, o["tri_angle"].ptr, go)
    else:
        go = _lib.GrowOutputs(**{k: v.ptr for k, v in o.items() if not k.startswith("tri_")})
        call = lambda: launch(None, None, go)
    for _ in range(warmup):
        call()
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()
    ms = []
    for _ in range(reps):
        ctx.record(e0)
        call()
        ctx.record(e1)
        ms.append(ctx.elapsed_ms(e0, e1))
    status, n_region = o["status"].download(), o["n_region"].download()
    assert (status == 0).all(), status
    heights, angles = o["tri_height"].download(), o["tri_angle"].download()
    for buf in list(d.values()) + list(o.values()):
        buf.free()
    for ev in (e0, e1):
        ctx.lib.mvosr_event_destroy(ctx.handle, ev)
    ms = np.array(ms)
    med = float(np.median(ms))
    nbytes = (29 * T) if given else (13 * T + 24 * int(off[-1]))
    res = {"frames": F, "form": "given" if given else "from_points", "features": int(off[-1]), "rows": T, "region_rows": int(n_region.sum()),
           "ms_median": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()), "reps": int(reps), "us_per_frame": med * 1e3 / F,
           "frames_per_s": F / (med * 1e-3), "algorithmic_bytes": int(nbytes), "GBps": nbytes / (med * 1e-3) / 1e9,
           "fraction_of_8TBps": nbytes / (med * 1e-3) / HBM_PEAK}
    return res, [(heights[toff[i]:toff[i + 1]], angles[toff[i]:toff[i + 1]]) for i in range(F)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    result = {"device": ctx.name.strip(), "hbm_peak_Bps": HBM_PEAK, "legs": {}}
    rng = np.random.default_rng(7)
    mixes = {"uniform2000": np.full(args.distinct, 2000), "ragged300_1500": rng.integers(300, 1501, args.distinct)}
    for name, sizes in mixes.items():
        distinct = make_frames(sizes, seed=77)
        rep = -(-args.frames // args.distinct)
        frames = (distinct * rep)[:args.frames]
        values = None
        for given in (False, True):
            leg, values = time_form(ctx, frames, given, args.reps)
            result["legs"]["%s_%s" % (name, leg["form"])] = leg
        if not args.no_cpu:
            import grow_cases as gc
            t0 = time.perf_counter()
            for (p, t), (h, a) in zip(distinct, values):
                gc.numpy_grow(t, h, a, n_feat=len(p))
            result["legs"]["%s_given" % name]["host_numpy_us_per_frame"] = (time.perf_counter() - t0) / len(distinct) * 1e6
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
