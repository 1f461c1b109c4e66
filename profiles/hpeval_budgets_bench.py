"""The budget sweep of the RANSAC evaluation against the runs it stands in for, on 3.15's workload: 512 resident
2000-feature frames, C = 10 cases, the device draw, budgets 25, 50, 100, 200, 500, 1000, 2000.

  launch      ONE launch of mvosr_height_pitch_eval_budgets_batch against the SEVEN launches of mvosr_height_pitch_eval_batch
              (n_hyp = each budget) on the same resident batch, both models: HIP events around each side, 3 warm-up rounds, then 20
              rounds in which the two sides take turns; median (min - max).  After the timing the outputs are compared bytewise:
              slot k of the sweep against the launch at budgets[k].
  end_to_end  RansacBudgetSweep.run against seven RansacEvaluation.run calls on the 512 frames as one sequence (model "plane"):
              wall clock, one warm-up, median (min - max) of 20.  Both sides are handed the same precomputed triangulations (--tris
              given, the default), so the figure covers packing, upload, launch, download and the cross-frame rules; --tris scipy
              lets every run triangulate on the host as a user without rows would (seven times against once; minutes per round).

Writes profiles/hpeval_budgets_bench.json.  python profiles/hpeval_budgets_bench.py [--frames 512] [--features 2000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
from scipy.spatial import Delaunay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mvoscalerecovery_amd import _lib, height_pitch as hp, synth      # noqa: E402

BUDGETS = (25, 50, 100, 200, 500, 1000, 2000)
PER_SLOT = ("ransac_height", "model", "best_ic", "used", "n_inliers", "refined_normal", "refined_pitch", "refined_mean", "refined_std",
            "height_t_mean", "sum_y", "sum_z", "status")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def out_spec(F, Cn, B):
    FC = (F, Cn) if B is None else (F, Cn, B)
    spec = [("ransac_height", FC, np.float64), ("model", FC + (4,), np.float64), ("best_ic", FC, np.int32), ("used", FC, np.int32),
            ("n_selected", F, np.int32), ("n_inliers", FC, np.int32), ("refined_normal", FC + (3,), np.float64),
            ("refined_pitch", FC, np.float64), ("refined_mean", FC, np.float64), ("refined_std", FC, np.float64),
            ("height_t_mean", FC, np.float64), ("sum_y", FC, np.float64), ("sum_z", FC, np.float64), ("status", FC, np.int32)]
    return spec + ([("best", FC, np.int32)] if B is not None else [])


def launch_level(ctx, model, frames, rows, priors, Cn, seed, warmup, rounds):
    lib, F, B = ctx.lib, len(frames), len(BUDGETS)
    spec_in, arrays, off, toff, planes, T = hp._pack_frames(frames, rows, priors)
    din = ctx.block(spec_in)
    d_sweep = ctx.block(out_spec(F, Cn, B))
    d_one = [ctx.block(out_spec(F, Cn, None)) for _ in BUDGETS]
    try:
        din.upload(arrays)
        d_sweep.zero()
        for d in d_one:
            d.zero()
        b = hp._batch_header(din, F, max(len(p) for p in frames), planes.shape[1])
        par = [_lib.HeightPitchEvalParams(hp.FOCUS, hp.CX, hp.CY, hp.MIN_POINTS, h, 0.005, hp.GOAL_FRACTION, 0.01, seed, 0, hp.EVAL_MODELS[model], Cn, 0)
               for h in BUDGETS]
        o_sweep = _lib.HeightPitchEvalBudgetsOutputs()
        for k, _ in o_sweep._fields_:
            if k in d_sweep:
                setattr(o_sweep, k, d_sweep[k].ptr)
        o_one = []
        for d in d_one:
            o = _lib.HeightPitchEvalOutputs()
            for k, _ in o._fields_:
                if k != "list_stride" and k in d:
                    setattr(o, k, d[k].ptr)
            o_one.append(o)
        bud = (C.c_int32 * B)(*BUDGETS)

        def sweep():
            _lib.check(lib.mvosr_height_pitch_eval_budgets_batch(ctx.handle, C.byref(b), C.byref(par[-1]), bud, B, din["prior"].ptr, None,
                                                                 C.byref(o_sweep)), "mvosr_height_pitch_eval_budgets_batch")

        def seven():
            for p, o in zip(par, o_one):
                _lib.check(lib.mvosr_height_pitch_eval_batch(ctx.handle, C.byref(b), C.byref(p), din["prior"].ptr, None, C.byref(o)),
                           "mvosr_height_pitch_eval_batch")

        ev = ctx.event(), ctx.event()

        def timed(fn):
            ctx.record(ev[0])
            fn()
            ctx.record(ev[1])
            return ctx.elapsed_ms(*ev)

        for _ in range(warmup):
            sweep()
            seven()
        ctx.sync()
        t_sweep, t_seven = [], []
        for _ in range(rounds):                                                      # the two sides in turns
            t_sweep.append(timed(sweep))
            t_seven.append(timed(seven))
        for e in ev:
            lib.mvosr_event_destroy(ctx.handle, e)
        # the outputs, bytewise
        got = {k: d_sweep[k].download() for k, _, _ in out_spec(F, Cn, B)}
        same = True
        for q, d in enumerate(d_one):
            for k in PER_SLOT:
                same &= np.ascontiguousarray(got[k][:, :, q]).tobytes() == d[k].download().tobytes()
            same &= got["n_selected"].tobytes() == d["n_selected"].download().tobytes()
        used, st = got["used"], got["status"]
    finally:
        din.free()
        d_sweep.free()
        for d in d_one:
            d.free()
    s, v = stats(t_sweep), stats(t_seven)
    return {"sweep_ms": s, "seven_launches_ms": v, "ratio_of_medians": v["median"] / s["median"],
            "outside_both_spreads": bool(s["max"] < v["min"]), "outputs_bytewise_equal": bool(same),
            "unfitted_slots": int(np.sum((st & ~hp.ST_HP_REFINE_DEGENERATE) != 0)),
            "stopped_share_per_budget": [float(np.mean(used[:, :, q] < h)) for q, h in enumerate(BUDGETS)],
            "mean_used_per_budget": [float(np.mean(used[:, :, q])) for q in range(B)],
            "distinct_best_models_per_case": float(np.mean([len(set(r)) for r in got["best"].reshape(-1, B)])),
            "lds_bytes": int(lib.mvosr_height_pitch_eval_budgets_lds_bytes(max(len(p) for p in frames), BUDGETS[-1], B, hp.EVAL_MODELS[model]))}


def end_to_end(model, frames, rows, motion, Cn, seed, rounds):
    sw = hp.RansacBudgetSweep(model, BUDGETS, cases=Cn, seed=seed)
    evs = [hp.RansacEvaluation(model, h, cases=Cn, seed=seed) for h in BUDGETS]

    def sweep():
        return sw.run(frames, motion, tris=rows)

    def seven():
        return [e.run(frames, motion, tris=rows) for e in evs]

    a, b = sweep(), seven()                                                          # the warm-up, and the rows compared
    same = all(np.array_equal(a[f][k], b[k][f], equal_nan=True) for k in range(len(BUDGETS)) for f in a)
    t_sweep, t_seven = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        sweep()
        t1 = time.perf_counter()
        seven()
        t2 = time.perf_counter()
        t_sweep.append(1e3 * (t1 - t0))
        t_seven.append(1e3 * (t2 - t1))
    s, v = stats(t_sweep), stats(t_seven)
    return {"sweep_run_ms": s, "seven_runs_ms": v, "ratio_of_medians": v["median"] / s["median"], "outside_both_spreads": bool(s["max"] < v["min"]),
            "rows_equal": bool(same), "table": sw.table(), "smallest_budget_within_10_percent": sw.smallest_budget()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--tris", choices=("given", "scipy"), default="given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpeval_budgets_bench.json"))
    a = ap.parse_args()
    F, N, Cn, seed = a.frames, a.features, 10, 1
    frames = []
    for i in range(F):
        f3, f2 = synth.synth_frame(9000 + i, N, base_seed=4242)                      # (hpeval_bench.py's frames)
        frames.append(np.ascontiguousarray(np.stack([f2[:, 0], f2[:, 1], f3[:, 2]], 1)))
    rows = [Delaunay(p[:, 0:2]).simplices.astype(np.int32) for p in frames]
    ests = [0.002 * np.sin(i) for i in range(F)]
    priors = [hp.frame_prior(e) for e in ests]
    ctx = _lib.default_context(0)
    out = {"device": ctx.name, "frames": F, "features": N, "n_cases": Cn, "budgets": list(BUDGETS), "hypotheses_sweep": BUDGETS[-1],
           "hypotheses_seven_runs": int(sum(BUDGETS)), "warmup": a.warmup, "rounds": a.rounds, "launch": {}}
    for model in ("plane", "line"):
        out["launch"][model] = launch_level(ctx, model, frames, rows, priors, Cn, seed, a.warmup, a.rounds)
        print(model, json.dumps(out["launch"][model]), flush=True)
    # a sequence whose priors are small pitches: motions straight ahead with a little vertical drift
    rng = np.random.default_rng(7)
    motion = np.stack([np.zeros(F + 1), 0.002 * rng.standard_normal(F + 1), np.ones(F + 1)], 1)
    out["end_to_end"] = dict(end_to_end("plane", frames, rows if a.tris == "given" else None, motion, Cn, seed, a.rounds), tris=a.tris)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
