#!/usr/bin/env python3
"""Times mvosr_static_tri_batch and the estimator call built on it, and prints ONE JSON line.

    python profiles/statictri_bench.py [--frames 512] [--reps 30] [--parent-tree DIR] [--out profiles/statictri_bench.json]

kernel   512 resident lists in ROW form: 2000-feature synthetic frames (64 distinct ones, repeated) taken through the estimator's
         host stages and mvosr_flat_selection_batch, whose tri_height / tri_flags the kernel reads in place with the batch's
         tri2_off.  The context's HIP events around one launch, 3 warm-up launches, the median of --reps repetitions and their
         spread.  Algorithmic bytes count every input and output once: 9 B per row (height, flag byte), 8 B per list of offsets,
         28 B per list out (two doubles, three words) — over the median time, as a fraction of 8 TB/s (HBM peak).
host     the same lists, counted rows packed, through a vectorised NumPy form of the restatement on one core (searchsorted over
         the edges, np.median); its results are compared with the kernel's by bytes on the way.
e2e      ``ScaleEstimator(model="static_tri").scale_calculation_batch`` on the same frames against ``model="ransac"`` on the staged
         path (triangulation="scipy", sampling="host"), wall clock, the median of 3 calls after one warm-up call each.  With
         --parent-tree (a checkout of the parent commit, built) the staged RANSAC call is ALSO timed there, in a child process.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
ABS_REF, WINDOW = 1.75, 5


def frames_of(n_frames, distinct, n_feat=2000):
    from mvoscalerecovery_amd import synth
    base = [synth.synth_frame(900 + i, n_feat, base_seed=97531, upper_fraction=0.1) for i in range(distinct)]
    return [base[i % distinct] for i in range(n_frames)]


def e2e(frames, reps=3, **kw):
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    est = ScaleEstimator(ABS_REF, window_size=WINDOW, triangulation="scipy", sampling="host", ransac_seed=5, **kw)
    est.scale_calculation_batch(f3s, f2s)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        est.scale_calculation_batch(f3s, f2s)
        ts.append(time.perf_counter() - t0)
    return {"frames": len(frames), "s_median": float(np.median(ts)), "s_min": float(min(ts)), "s_max": float(max(ts)),
            "us_per_frame": float(np.median(ts)) / len(frames) * 1e6, "reps": reps}


def host_restatement(h, edges, ref):
    """One list, vectorised: the restatement of tests/statictri_cases.py with searchsorted in place of the comparison loop."""
    hi = 1.0 / h
    k = np.searchsorted(edges, hi, side="right") - 1
    k[hi == edges[-1]] = 18
    dis = np.bincount(k[(k >= 0) & (k < 19)], minlength=19)
    dis[dis == 1] = 0
    mx = dis.max()
    if mx <= 2:
        return np.median(hi) * ref
    flag = np.zeros(19, bool)
    flag[0], flag[18] = dis[0] == mx, dis[18] == mx
    flag[1:18] = (dis[1:18] >= dis[0:17]) & (dis[1:18] >= dis[2:19]) & (dis[1:18] >= 0.33 * mx) & (dis[1:18] >= 2)
    i = int(np.argmax(flag))
    j = i
    while j + 1 < 19 and flag[j + 1]:
        j += 1
    return ((i + 1) + (j + 1)) / 2.0 / 10.0 * ref


def kernel_leg(frames, reps, warmup=3):
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.engine import DeviceBatch
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    est = ScaleEstimator(ABS_REF, window_size=WINDOW, model="static_tri")      # (forks the Delaunay workers, then opens the device)
    ctx = est.ctx
    pf2, _, _, _ = est._second_triangulations([f[0] for f in frames], [f[1] for f in frames])
    F, T = pf2.n_frames, int(pf2.tri2_off[-1])
    db = DeviceBatch(ctx, pf2, with_tri2=True)
    tri_h, tri_f = ctx.zeros(T, np.float64), ctx.zeros(T, np.uint8)
    per = {k: ctx.zeros(F, dt) for k, dt in (("level", np.float64), ("nkept", np.int32), ("status", np.int32))}
    b = db.struct()
    _lib.check(ctx.lib.mvosr_flat_selection_batch(ctx.handle, C.byref(b), -80.0, -85.0, 0.9, tri_h.ptr, tri_f.ptr, per["level"].ptr,
                                                  per["nkept"].ptr, per["status"].ptr, int(np.max(np.diff(pf2.tri2_off)))), "mvosr_flat_selection_batch")
    ctx.sync()
    assert (per["status"].download() == 0).all()
    o = {"scale_norm": ctx.empty(F, np.float64), "raw_scale": ctx.empty(F, np.float64), "n_used": ctx.empty(F, np.int32),
         "status": ctx.empty(F, np.int32)}
    call = lambda: _lib.check(ctx.lib.mvosr_static_tri_batch(ctx.handle, F, db.bufs["tri2_off"].ptr, None, tri_h.ptr, tri_f.ptr, 12, ABS_REF,
                                                             o["scale_norm"].ptr, o["raw_scale"].ptr, o["n_used"].ptr, None, o["status"].ptr),
                              "mvosr_static_tri_batch")
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
    r = {k: v.download() for k, v in o.items()}
    heights, flags = tri_h.download(), tri_f.download()
    for buf in [tri_h, tri_f] + list(per.values()) + list(o.values()):
        buf.free()
    db.free()
    for ev in (e0, e1):
        ctx.lib.mvosr_event_destroy(ctx.handle, ev)
    ms = np.array(ms)
    med = float(np.median(ms))
    nbytes = 9 * T + 8 * (F + 1) + 28 * F
    res = {"frames": F, "rows": T, "rows_per_frame": T / F, "counted_per_frame": float(r["n_used"].mean()),
           "statuses": {str(k): int(v) for k, v in zip(*np.unique(r["status"], return_counts=True))},
           "ms_median": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()), "reps": int(reps), "warmup": warmup,
           "us_per_frame": med * 1e3 / F, "frames_per_s": F / (med * 1e-3), "algorithmic_bytes": int(nbytes),
           "GBps": nbytes / (med * 1e-3) / 1e9, "fraction_of_8TBps": nbytes / (med * 1e-3) / HBM_PEAK}
    lists = [heights[pf2.tri2_off[f]:pf2.tri2_off[f + 1]][(flags[pf2.tri2_off[f]:pf2.tri2_off[f + 1]] & 1) != 0] for f in range(F)]
    res["device"] = ctx.name.strip()
    return res, lists, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its staged RANSAC call is timed too")
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--only-ransac-e2e", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    frames = frames_of(args.frames, args.distinct)
    if args.only_ransac_e2e:                                     # (the child process of --parent-tree: no keyword the parent lacks)
        print(json.dumps(e2e(frames)))
        return
    kernel, lists, r = kernel_leg(frames, args.reps)
    result = {"device": kernel.pop("device"), "hbm_peak_Bps": HBM_PEAK}
    edges = np.array(range(0, 20)) * 0.1
    some = lists[:args.distinct]
    t0 = time.perf_counter()
    host = [host_restatement(h, edges, ABS_REF) if len(h) > 12 else np.nan for h in some]
    kernel["host_numpy_us_per_frame"] = (time.perf_counter() - t0) / len(some) * 1e6
    assert np.array(host, dtype=np.float64).tobytes() == r["raw_scale"][:len(some)].tobytes(), "kernel and host restatement differ"
    kernel["host_lists_compared"] = len(some)
    result["kernel_row_form"] = kernel
    result["e2e_static_tri"] = e2e(frames, model="static_tri")
    result["e2e_ransac_staged"] = e2e(frames)
    if args.parent_tree:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", args.parent_tree, "--only-ransac-e2e", "--frames",
                              str(args.frames), "--distinct", str(args.distinct)], capture_output=True, text=True, check=True).stdout
        result["e2e_ransac_staged_parent"] = json.loads(out.strip().splitlines()[-1])
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
