"""Scoring the repeated runs on the device against the host route: n = 4541 frames (KITTI-00's length), C = 10 cases.

  launches   mvosr_paths_batch, mvosr_score_cases_batch, mvosr_segment_table and mvosr_pose2motion_batch, each between two
             mvosr_event_* records on the context's stream
  calls      evaluate.Scorer.score_scales (uploads, two launches, the download of the means), RepeatedRuns.scores (the same from the
             scales and motions a run keeps; the object is filled with the sequence's scales directly, no frames are processed),
             evaluate.Scorer's construction
  host       the route before: offline.get_path x 10, then evaluate.repeat_scores — Python loops over frames and segments
  numpy      the vectorised restatement of tests/scores_cases.py (paths_numpy, segment_table, score_numpy): what a NumPy rewrite
             alone buys; 4 x 4 stacks, which BLAS does not thread

One warm-up of every route, then `--repeats` (20) rounds that run the routes one after the other, so that they see the same machine
state; median / min / max.  Writes profiles/scores_bench.json.  python profiles/scores_bench.py [--repeats 20] [--n 4541] [--cases 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import scores_cases as sc                                                   # noqa: E402
from mvoscalerecovery_amd import _lib, evaluate, offline                    # noqa: E402
from mvoscalerecovery_amd.rescale import RepeatedRuns                       # noqa: E402


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--n", type=int, default=4541)
    ap.add_argument("--cases", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scores_bench.json"))
    a = ap.parse_args()
    sc.SEQUENCES["bench"] = (a.n, a.cases, 45411, "noisy")
    seq = sc.make_sequence("bench")
    motions, scales, gt = seq["motions"], seq["scales"], seq["gt"]
    n, C = a.n, a.cases

    runs = RepeatedRuns(1.75, window_size=5, cases=C, seed=1, triangulation="gpu", delaunay_workers=0)
    ctx = runs.estimator.ctx
    runs._scales, runs._motions = [scales], [motions]                       # (what run() keeps; no frames are processed here)
    scorer = evaluate.Scorer(gt, ctx=ctx)
    F, S = scorer.n_first, int(scorer.has.sum())

    # -- resident buffers for the launches
    d_m, d_s, d_gt = ctx.to_device(motions), ctx.to_device(scales), ctx.to_device(gt)
    d_paths, d_mo = ctx.empty((C, n + 1, 12), np.float64), ctx.empty((C, n, 12), np.float64)
    d_means, d_counts, d_status = ctx.empty((C, 2, 8), np.float64), ctx.empty((C, 8), np.int32), ctx.empty(C, np.int32)
    d_dist, d_last, d_gd = ctx.empty(n + 1, np.float64), ctx.empty((F, 8), np.int32), ctx.empty((F, 8, 24), np.float64)
    lib, h = ctx.lib, ctx.handle
    launches = {
        "paths": lambda: lib.mvosr_paths_batch(h, n, C, d_m.ptr, 0, d_s.ptr, d_paths.ptr),
        "score": lambda: lib.mvosr_score_cases_batch(h, C, n + 1, d_paths.ptr, F, scorer._last.ptr, scorer._gdelta.ptr, None, None,
                                                     d_means.ptr, d_counts.ptr, d_status.ptr),
        "segment_table": lambda: lib.mvosr_segment_table(h, n + 1, d_gt.ptr, d_dist.ptr, d_last.ptr, d_gd.ptr, d_status.ptr),
        "pose2motion": lambda: lib.mvosr_pose2motion_batch(h, C, n, d_paths.ptr, None, d_mo.ptr, None, d_status.ptr),
    }
    ev0, ev1 = ctx.event(), ctx.event()

    def timed_launch(fn):
        ctx.record(ev0)
        _lib.check(fn(), "launch")
        ctx.record(ev1)
        ctx.sync()
        return ctx.elapsed_ms(ev0, ev1)

    def wall(fn):
        t = time.perf_counter()
        fn()
        return time.perf_counter() - t

    def host_route():
        return evaluate.repeat_scores(gt, [offline.get_path(motions, scales[c]) for c in range(C)])

    def numpy_route():
        last = sc.segment_table(sc.distances(gt))[0]
        return sc.score_numpy(gt, sc.paths_numpy(motions, scales), last)[2]

    routes = {
        "score_scales_s": lambda: scorer.score_scales(motions, scales),
        "repeated_runs_scores_s": lambda: runs.scores(gt),
        "scorer_construction_s": lambda: evaluate.Scorer(gt, ctx=ctx),
        "host_get_path_x10_repeat_scores_s": host_route,
        "numpy_restatement_s": numpy_route,
    }
    for fn in launches.values():                                             # warm-up
        timed_launch(fn)
    got = {k: fn() for k, fn in routes.items()}
    dev, host = got["score_scales_s"], got["host_get_path_x10_repeat_scores_s"]
    agree = {k: float(np.abs(dev[k] - host[k]).max()) for k in ("tra", "rot")}
    ms = {k: [] for k in launches}
    sec = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in launches.items():
            ms[k].append(timed_launch(fn))
        for k, fn in routes.items():
            sec[k].append(wall(fn))
    out = {"device": ctx.name.strip(), "n": n, "cases": C, "firsts": F, "segments": S, "repeats": a.repeats,
           "launch_ms": {k: stats(v) for k, v in ms.items()}, "wall_s": {k: stats(v) for k, v in sec.items()},
           "max_abs_difference_device_vs_host": agree,
           # what each launch must move: motions + scales in and paths out; the two poses and the ground truth's delta per segment in
           # and the means out (the paths' other rows are never read)
           "algorithmic_bytes": {"paths": int(n * 96 + C * n * 8 + C * (n + 1) * 96), "score": int(C * S * (2 * 96 + 192 + 4) + C * 160)}}
    out["achieved_GBps"] = {k: out["algorithmic_bytes"][k] / (out["launch_ms"][k]["median"] * 1e-3) / 1e9 for k in ("paths", "score")}
    d, hst = out["wall_s"]["score_scales_s"], out["wall_s"]["host_get_path_x10_repeat_scores_s"]
    out["speedup_median"] = hst["median"] / d["median"]
    out["outside_spread"] = bool(d["max"] < hst["min"])
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
