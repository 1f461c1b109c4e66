#!/usr/bin/env python3
"""Times the scales' own score on the device and prints ONE JSON line.

    python profiles/scalescores_bench.py [--cases 10] [--filter-window 10] [--out profiles/scalescores_bench.json]

data     the 4541-frame sequence of tests/scores_cases.py ("n4541": KITTI-00's length), its ground truth's speeds
         (evaluate.calculate_speed) and --cases rows of scales off them by 10 % noise.
launches the context's HIP events around K launches, K chosen so that the window is at least 0.3 s, after 3 warm-up launches; the
         median, minimum and maximum of 20 such windows: mvosr_scale_errors_batch in its LDS form, in its global-memory form (the
         fill launch and the kernel), for ONE case (how a case's workgroups alone fare), and mvosr_window_median_cases.
calls    evaluate.scale_errors and evaluate.filter_scales from host arrays to host results, and RepeatedRuns.scale_scores with the
         filter and the re-scaled ground truth (the scales and motions put where ``run`` leaves them: the runs themselves are
         bench.py's business) — a host clock around calls that end in a download, 20 calls after 3.
host     the comparators evaluate.evaluate_scale and evaluate.scale_filter on the same rows on one core of the same host in the same
         call, 3 passes over the cases.
Before any timing the device's figures are compared with the comparators': every float bit for bit.
Needs a GPU: fails without one.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(ctx, call, window_s=0.35, samples=20, warmup=3):
    for _ in range(warmup):
        call()
    ctx.sync()
    e0, e1 = ctx.event(), ctx.event()

    def window(k):
        ctx.record(e0)
        for _ in range(k):
            call()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) / k
    once = max(window(2), 1e-3)
    k = max(2, int(np.ceil(window_s * 1e3 / once)))
    ms = np.array([window(k) for _ in range(samples)])
    for ev in (e0, e1):
        ctx.lib.mvosr_event_destroy(ctx.handle, ev)
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()), "samples": int(samples),
            "launches_per_sample": int(k), "window_s": float(np.median(ms)) * k * 1e-3, "warmup": warmup}


def clocked(call, samples=20, warmup=3):
    for _ in range(warmup):
        call()
    s = []
    for _ in range(samples):
        t0 = time.perf_counter()
        call()
        s.append(time.perf_counter() - t0)
    s = np.array(s) * 1e3
    return {"ms_median": float(np.median(s)), "ms_min": float(s.min()), "ms_max": float(s.max()), "samples": samples, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=10)
    ap.add_argument("--filter-window", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scalescore_cases as ssc
    import scores_cases as sc
    from mvoscalerecovery_amd import _lib, evaluate
    from mvoscalerecovery_amd.rescale import RepeatedRuns
    ctx = _lib.default_context(0)
    seq = sc.make_sequence("n4541")
    gt_poses, motions = seq["gt"], seq["motions"]
    speed = evaluate.calculate_speed(gt_poses, ctx=ctx)
    C, n, fw = args.cases, speed.size, args.filter_window
    scales = speed * (1.0 + 0.1 * np.random.RandomState(4541).randn(C, n))
    result = {"device": ctx.name.strip(), "cases": C, "n": n, "filter_window": fw}

    # -- the figures first: the device's against the comparators', bit for bit
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        host = [evaluate.evaluate_scale(speed, scales[c]) for c in range(C)]
    host_f = np.array([evaluate.scale_filter(scales[c], fw) for c in range(C)])
    for variant in (None, "global"):
        dev = evaluate.scale_errors(speed, scales, ctx=ctx, variant=variant)
        assert ssc.same(dev["mean"], [h[0][0] for h in host]) and ssc.same(dev["max"], [h[0][1] for h in host])
        assert ssc.same(dev["within"], [h[0][2:] for h in host]) and ssc.same(dev["drift"], [h[1] for h in host])
    assert ssc.same(evaluate.filter_scales(scales, fw, ctx=ctx), host_f)
    result["verified"] = "scale_errors (both forms) and filter_scales equal the host comparators bit for bit at the timed size"

    # -- each launch by HIP events
    w, t = np.array(evaluate.SCALE_WINDOWS, dtype=np.int32), np.array(evaluate.SCALE_THRESHOLDS, dtype=np.float64)
    d_gt, d_s, d_f = ctx.to_device(speed), ctx.to_device(scales), ctx.empty((C, n), np.float64)
    res = ctx.block([("stats", (C, 2), np.float64), ("drift", (C, w.size), np.float64), ("counts", (C, t.size), np.int32), ("status", (C,), np.int32)])

    def errors(flags, cases=C, w=w):
        _lib.check(ctx.lib.mvosr_scale_errors_batch(ctx.handle, n, d_gt.ptr, cases, n, d_s.ptr, n, w.size, _lib.addr(w) if w.size else None,
                                                    evaluate.SCALE_STEP, t.size, _lib.addr(t), flags, res["stats"].ptr, res["counts"].ptr,
                                                    res["drift"].ptr, res["status"].ptr), "mvosr_scale_errors_batch")

    def median():
        _lib.check(ctx.lib.mvosr_window_median_cases(ctx.handle, d_s.ptr, C, n, n, fw, d_f.ptr, n), "mvosr_window_median_cases")
    result["launch"] = {"scale_errors_lds": timed(ctx, lambda: errors(0)),
                        "scale_errors_global": timed(ctx, lambda: errors(_lib.SCALE_ERRORS_GLOBAL)),
                        "scale_errors_lds_one_case": timed(ctx, lambda: errors(0, 1)),
                        "window_median_cases": timed(ctx, median)}
    # which unit binds: the statistics alone, then with the shortest / the longest window as the only other unit
    only = {k: np.array(v, dtype=np.int32) for k, v in (("stats_only", []), ("stats_and_window_10", [10]), ("stats_and_window_100", [100]),
                                                         ("stats_and_window_800", [800]))}
    result["launch"]["units_lds"] = {k: timed(ctx, lambda v=v: errors(0, C, v), samples=10) for k, v in only.items()}
    result["launch"]["workgroups"] ={"scale_errors": C * (1 + int(w.size)), "window_median_cases": C * ((n + 255) // 256)}

    # -- the calls end to end
    runs = RepeatedRuns(1.75, window_size=5, seed=1, cases=C, triangulation="gpu", delaunay_workers=0)
    runs._scales, runs._motions = [scales], [motions]                  # where ``run`` leaves them
    both = runs.scale_scores(speed, poses_gt=gt_poses, filter_window=fw)
    assert ssc.same(both["scales"]["drift"], [h[1] for h in host]) and np.isfinite(both["gt_rescaled"]["tra"]).all()
    result["call"] = {"scale_errors": clocked(lambda: evaluate.scale_errors(speed, scales, ctx=ctx)),
                      "filter_scales": clocked(lambda: evaluate.filter_scales(scales, fw, ctx=ctx)),
                      "repeated_runs_scale_scores_errors_only": clocked(lambda: runs.scale_scores(speed)),
                      "repeated_runs_scale_scores_filter_and_gt": clocked(lambda: runs.scale_scores(speed, poses_gt=gt_poses, filter_window=fw))}

    # -- the host comparators, one core, the same rows
    def host_pass(fn):
        s = []
        for _ in range(3):
            t0 = time.perf_counter()
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                for c in range(C):
                    fn(c)
            s.append(time.perf_counter() - t0)
        s = np.array(s) * 1e3
        return {"ms_median": float(np.median(s)), "ms_min": float(s.min()), "ms_max": float(s.max()), "samples": 3, "ms_per_case": float(np.median(s)) / C}
    result["host"] = {"evaluate_scale": host_pass(lambda c: evaluate.evaluate_scale(speed, scales[c])),
                      "scale_filter": host_pass(lambda c: evaluate.scale_filter(scales[c], fw))}
    result["host_over_device"] = {"scale_errors": result["host"]["evaluate_scale"]["ms_median"] / result["call"]["scale_errors"]["ms_median"],
                                  "filter_scales": result["host"]["scale_filter"]["ms_median"] / result["call"]["filter_scales"]["ms_median"]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
