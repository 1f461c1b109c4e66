#!/usr/bin/env python3
"""Times mvosr_feature_distribution_batch and the estimator call built on it, and prints ONE JSON line.

    python profiles/featdist_bench.py [--frames 512] [--reps 30] [--e2e-frames 4096] [--out profiles/featdist_bench.json]

kernel   512 resident frames of 2000 synthetic features (64 distinct ones, repeated), the levels taken from a real staged pass
         (reliability vote, feature_selection_by_tri).  The context's HIP events around one launch, 3 warm-up launches, the median of
         --reps repetitions and their spread; the same for a launch of ONE frame — if the two take about the same time, the kernel
         is bound by one frame's chain of dependent steps (latency), not by bytes or operations.
counts   from the shapes: bytes in (9 per feature: y and level; 20 per frame: offset, count, scale) and out (per frame and
         population n, two 172-word histograms, three doubles; a status per frame), the atomic adds to the tables; fp64 operations
         (two pairwise sums, the deviations and their squares, the scaling) and the ballots of the radix select.
host     the same frames through NumPy on one core (np.histogram twice, np.mean / np.std / np.median per population); its numbers
         are compared with the kernel's by bytes on the way.
e2e      ``check_full_distribution_batch`` on --e2e-frames frames, wall clock, against the same call with the distribution launch
         skipped (the staged pass alone): the difference is what the feature costs on top of the staged path.
Needs a GPU: fails without one.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
FP64_PEAK = 78.6e12            # vector fp64, MI355X data sheet
ABS_REF, WINDOW = 1.75, 5


def frames_of(n_frames, distinct, n_feat=2000):
    from mvoscalerecovery_amd import synth
    base = [synth.synth_frame(900 + i, n_feat, base_seed=97531, upper_fraction=0.1) for i in range(distinct)]
    return [base[i % distinct] for i in range(n_frames)]


def lds_bytes(max_feat):
    """featdist_plan(max_feat).total of csrc/mvosr_featdist_plan.hpp: three slices of list, leaf sums, stack, two histograms, leaf offsets."""
    leaves = max_feat // 64 + 1
    per_wave = 8 * ((max_feat + 1) & ~1) + 8 * leaves + 8 * 16 + 2 * 4 * 172 + 4 * (leaves + 1) + 2 * 4 * 16
    return 3 * ((per_wave + 15) & ~15)


def timed_launches(ctx, call, reps, warmup=3):
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
    for ev in (e0, e1):
        ctx.lib.mvosr_event_destroy(ctx.handle, ev)
    ms = np.array(ms)
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()), "reps": int(reps), "warmup": warmup}


def kernel_leg(est, frames, scales, reps):
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.engine import FeatDistOutputs
    eng, ctx = est._dist_engine(), est.engine.ctx
    pf, masks, levels, outcome, errors, picks, level = est._distribution_levels([f[0] for f in frames], [f[1] for f in frames])
    F, cnt, total = pf.n_frames, np.asarray(pf.feat_cnt), len(pf.y)
    blk = ctx.block([("off", F, np.int64), ("cnt", F, np.int32), ("y", total, np.float64), ("scale", F, np.float64), ("level", total, np.uint8)])
    blk.upload({"off": pf.feat_off, "cnt": cnt, "y": pf.y, "scale": np.asarray(scales, dtype=np.float64), "level": levels[:total]})
    out = FeatDistOutputs(ctx, F)
    seq = ctx.zeros((_lib.FD_POPULATIONS, _lib.FD_HIST_WORDS), np.int64)
    mf = int(pf.max_feat)
    full = lambda: eng.feature_distribution_batch(F, blk["off"], blk["cnt"], blk["y"], blk["level"], blk["scale"], mf, out, seq)
    one = lambda: eng.feature_distribution_batch(1, blk["off"], blk["cnt"], blk["y"], blk["level"], blk["scale"], mf, out, seq)
    res = {"frames": F, "features_per_frame": float(cnt.mean()), "outcomes": {str(k): int(v) for k, v in zip(*np.unique(outcome, return_counts=True))}}
    res["one_frame"] = timed_launches(ctx, one, reps)
    res.update(timed_launches(ctx, full, reps))
    got = {k: out.get(k) for k in ("n", "hist", "hist_scaled", "stats", "status")}
    members = got["n"].astype(np.int64)                                    # [F][3]
    W = _lib.FD_HIST_WORDS
    bytes_in = 9 * int(cnt.sum()) + 20 * F
    bytes_out = F * (3 * (4 + 2 * 4 * W + 24) + 4)
    atomics = int(np.count_nonzero(got["hist_scaled"]))
    fp64_ops = int((2 * members + 2 * members + members).sum())           # two sums; y - mean and its square; y * scale
    ballots = int((16 * 16 * members + 16 * members).sum())                # sixteen 4-bit passes of sixteen ballots; the even count's pass
    med = res["ms_median"] * 1e-3
    res.update({"us_per_frame": med / F * 1e6, "frames_per_s": F / med, "members_per_frame": members.mean(axis=0).tolist(),
                "bytes_in": bytes_in, "bytes_out": bytes_out, "table_atomics": atomics, "GBps": (bytes_in + bytes_out) / med / 1e9,
                "fraction_of_8TBps": (bytes_in + bytes_out) / med / HBM_PEAK, "fp64_operations": fp64_ops,
                "fraction_of_fp64_peak": fp64_ops / med / FP64_PEAK, "select_ballots": ballots,
                "lds_bytes_per_workgroup": lds_bytes(mf),
                "time_of_512_over_time_of_1": res["ms_median"] / res["one_frame"]["ms_median"]})
    res["bound"] = ("latency: %d frames take %.2f times what one frame takes, at %.4f of the HBM peak and %.5f of the fp64 peak"
                    % (F, res["time_of_512_over_time_of_1"], res["fraction_of_8TBps"], res["fraction_of_fp64_peak"]))
    res["summation"] = "parallel (eight leaves a step, eight lanes a leaf); the redundant every-lane form was not built or timed"
    res["device"] = ctx.name.strip()
    host = (pf, cnt, levels, got)
    seq.free()
    out.free()
    blk.free()
    return res, host


def host_leg(pf, cnt, levels, got, scales, n_compare):
    edges = np.array(range(0, 170)) * 0.1
    t0 = time.perf_counter()
    stats = np.full((n_compare, 3, 3), np.nan)
    hist = np.zeros((n_compare, 3, 169), dtype=np.int64)
    hist_s = np.zeros((n_compare, 3, 169), dtype=np.int64)
    for f in range(n_compare):
        sl = pf.frame_slice(f)
        y, lv = pf.y[sl], levels[sl]
        for p in range(3):
            v = y[lv >= p]
            hist[f, p] = np.histogram(v, bins=edges)[0]
            hist_s[f, p] = np.histogram(v * scales[f], bins=edges)[0]
            if v.size:
                stats[f, p] = np.mean(v), np.std(v), np.median(v)
    dt = time.perf_counter() - t0
    assert np.array_equal(hist, got["hist"][:n_compare, :, :169]) and np.array_equal(hist_s, got["hist_scaled"][:n_compare, :, :169]), "histograms differ"
    a, b = stats, got["stats"][:n_compare]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.where(np.isnan(a), 0, a).tobytes() == np.where(np.isnan(b), 0, b).tobytes(), "statistics differ"
    return {"frames_compared": n_compare, "numpy_us_per_frame": dt / n_compare * 1e6}


def e2e_leg(est, frames, scales, reps=3):
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    res = {"frames": len(frames), "reps": reps}
    for name, launch in (("with_distribution", True), ("staged_pass_only", False)):
        est.check_full_distribution_batch(f3s[:512], f2s[:512], scales[:512], accumulate=False, _launch=launch)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            est.check_full_distribution_batch(f3s, f2s, scales, accumulate=False, _launch=launch)
            ts.append(time.perf_counter() - t0)
        res[name] = {"s_median": float(np.median(ts)), "s_min": float(min(ts)), "s_max": float(max(ts)), "us_per_frame": float(np.median(ts)) / len(frames) * 1e6}
    res["distribution_us_per_frame"] = res["with_distribution"]["us_per_frame"] - res["staged_pass_only"]["us_per_frame"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--e2e-frames", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    est = ScaleEstimator(ABS_REF, window_size=WINDOW, triangulation="scipy")      # (forks the Delaunay workers, then opens the device)
    frames = frames_of(args.frames, args.distinct)
    scales = [float(s) for s in 0.8 + 0.4 * np.random.default_rng(5).random(max(args.frames, args.e2e_frames))]
    kernel, host = kernel_leg(est, frames, scales[:args.frames], args.reps)
    result = {"device": kernel.pop("device"), "hbm_peak_Bps": HBM_PEAK, "fp64_peak_ops": FP64_PEAK, "kernel": kernel}
    result["host"] = host_leg(*host, scales, min(args.distinct, args.frames))
    if args.e2e_frames > 0:
        result["e2e"] = e2e_leg(est, frames_of(args.e2e_frames, args.distinct), scales[:args.e2e_frames])
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
