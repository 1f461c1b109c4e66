"""us per 2000-feature frame of the RANSAC evaluation runs on 512 resident frames, C = 10 cases, H = 500:

  eval       mvosr_height_pitch_eval_batch, one launch for all cases (events around repeated launches on the resident batch), for
             both models, with cases_per_group G = 1 (frames x C workgroups, the frame pass redone per case) and G = C (one
             workgroup per frame, the frame resident over its ten cases); the same on the first 16 frames alone;
  ten_runs   ten launches of mvosr_height_pitch_batch over the same frames — what a user had before: a time reference only (it
             takes the inliers among all points, not the list, and has no line model);
  numpy      tests/hpeval_cases.py's float64 restatement on one core (a few (frame, case) pairs).

Writes profiles/hpeval_bench.json.  python profiles/hpeval_bench.py [--frames 512] [--features 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy.spatial import Delaunay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mvoscalerecovery_amd import _lib, height_pitch as hp, synth      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpeval_bench.json"))
    a = ap.parse_args()
    F, N, H, Cn = a.frames, a.features, 500, 10
    frames = []
    for i in range(F):
        f3, f2 = synth.synth_frame(9000 + i, N, base_seed=4242)                      # (heightpitch_bench.py's frames)
        frames.append(np.stack([f2[:, 0], f2[:, 1], f3[:, 2]], 1))
    rows = [Delaunay(p[:, 0:2]).simplices.astype(np.int32) for p in frames]
    ests = [0.002 * np.sin(i) for i in range(F)]
    priors = [hp.frame_prior(e) for e in ests]

    base = hp.HeightPitchEstimator(seed=1)
    res = base.launch(frames, priors, tris=rows, timing=a.repeats)
    assert not res["status"].any()
    one_run_us = 1e3 * res["kernel_ms"] / F
    M = res["n_selected"].astype(np.int64)

    out = {"device": base.ctx.name, "frames": F, "features": N, "n_hyp": H, "n_cases": Cn, "mean_list": float(M.mean()),
           "height_pitch_batch_us_per_frame": one_run_us, "ten_runs_us_per_frame": Cn * one_run_us, "eval": {}}
    for model in ("plane", "line"):
        ev = hp.RansacEvaluation(model, H, cases=Cn, seed=1)
        per = {}
        for G in (1, Cn):
            r = ev.launch(frames, priors, tris=rows, timing=a.repeats, cases_per_group=G)
            assert not (r["status"] & ~hp.ST_HP_REFINE_DEGENERATE).any(), np.unique(r["status"], return_counts=True)
            per["G%d" % G] = {"us_per_frame": 1e3 * r["kernel_ms"] / F, "us_per_frame_and_case": 1e3 * r["kernel_ms"] / (F * Cn)}
        # a batch far smaller than the device (16 frames): G decides how many CUs have work at all
        for G in (1, Cn):
            r16 = ev.launch(frames[:16], priors[:16], tris=rows[:16], timing=a.repeats, cases_per_group=G)
            per["G%d" % G]["us_per_frame_16_frames"] = 1e3 * r16["kernel_ms"] / 16
        per["degenerate_pairs"] = float(np.mean((r["status"] & hp.ST_HP_REFINE_DEGENERATE) != 0))
        per["mean_list_inliers"] = float(r["n_inliers"].mean())
        per["lds_bytes"] = int(ev.ctx.lib.mvosr_height_pitch_eval_lds_bytes(N, H, hp.EVAL_MODELS[model]))
        out["eval"][model] = per

    import hpeval_cases as he
    for model in ("plane", "line"):
        t0 = time.perf_counter()
        for k in range(a.numpy_pairs):
            he.restate(model, frames[k], rows[k], ests[k], he.draw_positions(model, 1, k, 0, H, int(M[k])))
        out["eval"][model]["numpy_us_per_frame_and_case"] = 1e6 * (time.perf_counter() - t0) / a.numpy_pairs
    # the launch's floors: per (frame, case) M H count tests of 5 (line: 3) flops, H models, 3 passes over M list entries
    out["count_tests_per_frame_and_case"] = float(M.mean()) * H
    out["hbm_bytes_per_frame_and_group"] = 24 * N + 12 * float(np.mean([len(t) for t in rows]))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
