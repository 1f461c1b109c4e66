"""The height-and-pitch estimator's device-resident path against the staged paths, one MI355X, wall clock:

  resident      HeightPitchEstimator(triangulation="gpu", resident=True).run_sequence
  staged_gpu    HeightPitchEstimator(triangulation="gpu").run_sequence — rows to the host and back, one launch, the host's carry
  staged_scipy  HeightPitchEstimator(triangulation="scipy").run_sequence — SciPy's rows (fewer repeats: Qhull is seconds per run)

on the same synthetic frames (1800-2200 features, 500 hypotheses), a fresh object per run, the sides taken in turns after a warm-up;
median (min - max) per side.  The resident and the staged_gpu results are compared byte for byte before anything is timed.
Then, by device events, mvosr_height_pitch_tail_batch alone on 512 resident frames with 0 % and with 10 % carried frames.

Writes profiles/heightpitch_resident_bench.json.  python profiles/heightpitch_resident_bench.py [--frames 4096] [--repeats 10]"""
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


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--scipy-repeats", type=int, default=2)
    ap.add_argument("--hyp", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heightpitch_resident_bench.json"))
    a = ap.parse_args()
    F, H = a.frames, a.hyp
    sizes = np.random.default_rng(7).integers(1800, 2201, F)
    frames = []
    for i in range(F):
        f3, f2 = synth.synth_frame(9000 + i, int(sizes[i]), base_seed=4242)
        frames.append(np.stack([f2[:, 0], f2[:, 1], f3[:, 2]], 1))
    motion = hc.motions(3, F + 1)
    make = {"resident": lambda: hp.HeightPitchEstimator(max_iterations=H, seed=1, triangulation="gpu", resident=True),
            "staged_gpu": lambda: hp.HeightPitchEstimator(max_iterations=H, seed=1, triangulation="gpu"),
            "staged_scipy": lambda: hp.HeightPitchEstimator(max_iterations=H, seed=1, triangulation="scipy")}

    def run(side):
        est = make[side]()
        t0 = time.perf_counter()
        out = est.run_sequence(frames, motion)                                        # (ends in a download that waits for the device)
        return time.perf_counter() - t0, out, est

    # warm-up, and the results: faster and different is not faster
    _, res, est_r = run("resident")
    _, ref, _ = run("staged_gpu")
    assert all(np.array_equal(x, y) for x, y in zip(res, ref)), "the resident path differs from the staged path"
    run("staged_scipy")
    times = {k: [] for k in make}
    for r in range(a.repeats):
        for side in ("resident", "staged_gpu") + (("staged_scipy",) if r < a.scipy_repeats else ()):
            times[side].append(run(side)[0])
    out = {"device": est_r.ctx.name, "frames": F, "features": "1800-2200", "n_hyp": H, "declined": est_r.declined_total,
           "chunks": len(est_r.last["errors"]), "bytewise_equal_to_staged_gpu": True,
           "wall": {k: dict(spread(v), frames_per_s=F / statistics.median(v)) for k, v in times.items()}}

    # the tail alone on 512 resident frames
    est = make["resident"]()
    sub, ests = frames[:512], [float(e) for e in hp.estimated_pitches(motion, 1, 512)]
    rng = np.random.default_rng(100)                                                  # every tenth frame a wall at constant depth: an empty list, carried
    few = [(np.stack([rng.uniform(0, 1241, 2000), rng.uniform(0, 376, 2000), np.full(2000, 20.0)], 1) if i % 10 == 5 else p) for i, p in enumerate(sub)]
    out["tail"] = {}
    for name, fr in (("carried_0_percent", sub), ("carried_10_percent", few)):
        us, carried = tail_us(est._resident_call(fr, ests, None), len(fr), 50, lambda st: int(st["small"]["frames"].download()["carried"].sum()))
        out["tail"][name] = {"us_per_launch": us, "frames": len(fr), "carried": carried}
    out["note"] = "wall clock around run_sequence on a fresh object per run; no hardware counters were read"
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
