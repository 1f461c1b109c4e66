"""The evaluation objects' device-resident path against the staged device path, one MI355X, wall clock:

  resident    RansacBudgetSweep / RansacEvaluation(triangulation="gpu", resident=True).run
  staged_gpu  the same objects with triangulation="gpu" alone — rows to the host and back, every output downloaded, the host's rules

on the same synthetic frames (1800-2200 features, 10 cases; the sweep at budgets 25 ... 2000, the evaluation at 500 iterations), on 512
and on 4096 frames, a fresh object per run, the sides taken in turns after one warm-up; median (min - max) per side.  The two sides'
arrays are compared byte for byte before anything is timed.  Then, by device events, mvosr_height_pitch_eval_tail_batch alone on 512
resident frames of the sweep with 0 % and with 10 % carried frames.

Writes profiles/hpeval_resident_bench.json.  python profiles/hpeval_resident_bench.py [--frames 512 4096] [--repeats 7]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mvoscalerecovery_amd import height_pitch as hp, synth              # noqa: E402
import heightpitch_cases as hc                                           # noqa: E402
from resident_tail import tail_us                                        # noqa: E402

BUDGETS = (25, 50, 100, 200, 500, 1000, 2000)
ITERATIONS, CASES = 500, 10


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "runs": len(ts)}


def make(kind, resident):
    if kind == "sweep":
        return hp.RansacBudgetSweep("plane", BUDGETS, cases=CASES, seed=1, triangulation="gpu", resident=resident)
    return hp.RansacEvaluation("plane", ITERATIONS, cases=CASES, seed=1, triangulation="gpu", resident=resident)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpeval_resident_bench.json"))
    a = ap.parse_args()
    F = max(a.frames)
    sizes = np.random.default_rng(7).integers(1800, 2201, F)
    frames = []
    for i in range(F):
        f3, f2 = synth.synth_frame(9000 + i, int(sizes[i]), base_seed=4242)
        frames.append(np.stack([f2[:, 0], f2[:, 1], f3[:, 2]], 1))
    motion = hc.motions(3, F + 1)[:, 3::4]
    out = {"features": "1800-2200", "cases": CASES, "budgets": list(BUDGETS), "iterations": ITERATIONS, "model": "plane", "wall": {}}

    def run(kind, resident, n):
        ev = make(kind, resident)
        t0 = time.perf_counter()
        ev.run(frames[:n], motion[:n + 1])                                           # (ends in a download that waits for the device)
        return time.perf_counter() - t0, ev

    for kind in ("sweep", "evaluation"):
        for n in a.frames:
            # warm-up, and the results: faster and different is not faster
            _, res = run(kind, True, n)
            _, ref = run(kind, False, n)
            for k in ref.results:
                assert res.results[k].tobytes() == ref.results[k].tobytes(), "the resident path differs from the staged path: " + k
            assert np.array_equal(res.carried, ref.carried) and np.array_equal(res.degenerate, ref.degenerate)
            if kind == "sweep":
                assert np.array_equal(res.used, ref.used) and np.array_equal(res.best, ref.best)
            times = {"resident": [], "staged_gpu": []}
            for _ in range(a.repeats):
                for side in ("resident", "staged_gpu"):
                    times[side].append(run(kind, side == "resident", n)[0])
            w = {k: dict(spread(v), frames_per_s=n / statistics.median(v)) for k, v in times.items()}
            w["bytewise_equal"], w["declined"], w["chunks"] = True, res.declined_total, len(res.last["errors"])
            w["speedup_of_medians"] = w["staged_gpu"]["median_s"] / w["resident"]["median_s"]
            w["outside_both_spreads"] = bool(w["resident"]["max_s"] < w["staged_gpu"]["min_s"] or w["staged_gpu"]["max_s"] < w["resident"]["min_s"])
            out["wall"]["%s_%d" % (kind, n)] = w
            out["device"] = res.ctx.name
            print(kind, n, json.dumps(w), flush=True)

    # the tail alone on 512 resident frames of the sweep
    ev = make("sweep", True)
    sub = frames[:512]
    rng = np.random.default_rng(100)                                                  # every tenth frame a wall at constant depth: an empty list, carried
    few = [(np.stack([rng.uniform(0, 1241, 2000), rng.uniform(0, 376, 2000), np.full(2000, 20.0)], 1) if i % 10 == 5 else p) for i, p in enumerate(sub)]
    out["tail"] = {}
    for name, fr in (("carried_0_percent", sub), ("carried_10_percent", few)):
        call = hp._EvalCall(ev, ev.budgets[-1], ev.budgets, fr, hp.estimated_pitches(motion[:513], 1, len(fr)), None)
        us, carried = tail_us(call, len(fr), 50, lambda st: int(st["small"]["carried"].download().sum()))
        out["tail"][name] = {"us_per_call": us, "launches_per_call": 3, "frames": len(fr), "elements_per_frame": CASES * len(BUDGETS), "carried": carried}
    out["note"] = ("wall clock around run() on a fresh object per run; the staged side is the code this change does not touch; "
                   "no hardware counters were read, so what bounds the tail's kernels was not measured")
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
