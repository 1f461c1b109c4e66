"""The rescale estimator's large-frame kernels: what they cost where the resident kernels also run, what a
20 000-feature frame costs, and whether the default path moved.

  (a) below the limit   512 resident frames of 2000 and of 3000 features: mvosr_graph_keep_large_batch against
                        mvosr_graph_keep_batch and mvosr_flat_ransac_large_batch against mvosr_flat_ransac_batch on the same
                        batch.  HIP events around each launch, the two alternating, 3 warm-up launches, median / min / max of
                        `--repeats` (>= 20).  The ratio says where the router's threshold belongs (it stays at _max_points()
                        unless the large kernels measure faster below it).  The outputs of the two are compared after the timing.
  (b) C5's shape        `--big-frames` frames of 20 000 features: the two large launches alone (HIP events);
                        ScaleEstimator(large_frames=True).scale_calculation_batch end to end (wall clock) against
                        oracle/rescale_oracle.py on one core of the same host, and, for orientation, against
                        scale_calculator.ScaleEstimator(triangulation="gpu", check_triangle="fixed") on the same frames.
  (c) --default-path-only   bench.py's e2e_rescale leg and RepeatedRuns.run with the default construction and nothing else,
                        importing nothing this change added: the same file run from a checkout of the parent commit gives the
                        parent's figures.  `--merge-ab DIR` folds the runs found there (this_*.json, parent_*.json, taken in
                        turns in one session) into the result.

No hardware counters are read here: which unit bounds the kernels is not measured (DESIGN.md 3.23 says what is known).
Writes profiles/rescale_large_bench.json.  python profiles/rescale_large_bench.py [--frames 512] [--big-frames 32]"""
import argparse
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mvoscalerecovery_amd import _lib, synth                                # noqa: E402
from mvoscalerecovery_amd.rescale import RepeatedRuns, ScaleEstimator       # noqa: E402


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def alternating(fns, warmup, repeats, clock):
    """name -> stats of `repeats` measurements of every fn, taken in turns (a drift of the machine hits all of them alike)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    got = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            got[k].append(clock(fn))
    return {k: stats(v) for k, v in got.items()}


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def event_clock(ctx):
    e0, e1 = ctx.event(), ctx.event()

    def clock(fn):
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1)
    return clock


def resident_inputs(est, raw):
    """The frames `raw` as the two launches' inputs: per frame the vote's case (first triangulation: SciPy's, canonical rows) and
    the flat selection's Frame (keep words and second triangulation: the estimator's own stage outputs)."""
    import flat_cases as fc
    import large_cases as lc
    from oracle import rescale_oracle as ro
    from scipy.spatial import Delaunay
    est.scale_calculation_batch([f[0] for f in raw], [f[1] for f in raw], stage=True)
    cases, frames = [], []
    for i, (f3, f2) in enumerate(raw):
        low = f2[:, 1] > est.vanish
        valid = np.asarray(est.last["valid"][i], bool)
        keep = np.where(valid, 1, -1 if int(valid.sum()) > 10 else 0).astype(np.int32)
        frames.append(fc.Frame("f%d" % i, f3[low], est.last["tris2"][i], keep=keep))
        cases.append(lc.graph_case("f%d" % i, f2[low][:, 1], f3[low][:, 2], ro.canonical_rows(Delaunay(f2[low]).simplices)))
    return cases, frames


def launch_pair(ctx, cases, frames, which, warmup, repeats, n_hyp=100):
    """Timings (ms per batch) of the vote's and the flat selection's launches named in `which` on one resident batch, in turns, and
    whether their outputs are the same bytes."""
    import flat_cases as fc
    import large_cases as lc
    clock = event_clock(ctx)
    F = len(frames)
    kb, kd, koff = lc.keep_batch(ctx, cases)
    ko = {w: {k: ctx.zeros(sh, np.int32) for k, sh in {"keep": int(koff[-1]) + 1, "n_valid": F, "status": F}.items()} for w in which}
    fb, fd, toff, max_tri = fc._batch(ctx, frames, compact=False)
    keep = ctx.to_device(np.concatenate([f.keep for f in frames]).astype(np.int32))
    fo = {w: {k: ctx.zeros(sh, dt) for k, (sh, dt) in {"raw_scale": (F, np.float64), "height_level": (F, np.float64), "model": ((F, 4), np.float64),
                                                       "best_ic": (F, np.int32), "used": (F, np.int32), "n_kept": (F, np.int32),
                                                       "status": (F, np.int32)}.items()} for w in which}
    rp = _lib.RescaleParams(0, 10, -80.0, -85.0, 0.9, 12, n_hyp, 0.005, 0.8, 1.75, 100, 0)

    def flat(w):
        o = fo[w]
        ro = _lib.RescaleOutputs(o["raw_scale"].ptr, o["height_level"].ptr, o["model"].ptr, o["best_ic"].ptr, o["used"].ptr, o["n_kept"].ptr,
                                 o["status"].ptr, None, None, None)
        _lib.check(getattr(ctx.lib, lc.FLAT[w])(ctx.handle, C.byref(fb), keep.ptr, C.byref(rp), None, None, None, C.byref(ro), max_tri), lc.FLAT[w])
    r = {"vote": alternating({w: (lambda w=w: lc.launch_keep(ctx, kb, None, ko[w], w == "large")) for w in which}, warmup, repeats, clock),
         "flat_ransac": alternating({w: (lambda w=w: flat(w)) for w in which}, warmup, repeats, clock)}
    if len(which) == 2:
        for k in r:
            r[k]["large_over_resident"] = r[k]["large"]["median"] / r[k]["resident"]["median"]
        r["vote"]["same_bytes"] = all(ko["large"][k].download().tobytes() == ko["resident"][k].download().tobytes() for k in ko["large"])
        r["flat_ransac"]["same_bytes"] = all(fo["large"][k].download().tobytes() == fo["resident"][k].download().tobytes() for k in fo["large"])
    r["frames"], r["rows_per_frame"] = F, float(np.mean(np.diff(toff)))
    r["frames_with_plane"] = int((fo[which[-1]]["status"].download() == 0).sum())
    for bufs in list(ko.values()) + list(fo.values()):
        for buf in bufs.values():
            buf.free()
    for buf in kd + list(fd.values()) + [keep]:
        buf.free()
    return r


def below_the_limit(a, out):
    est = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=1, delaunay_workers=0)
    out["resident_limit"] = int(est._max_points())
    for N in (2000, 3000):
        raw = [synth.synth_frame(7000 + i, N, base_seed=4242, upper_fraction=0.1) for i in range(a.frames)]
        cases, frames = resident_inputs(est, raw)
        r = launch_pair(est.ctx, cases, frames, ("resident", "large"), a.warmup, a.repeats)
        r["features"], r["unit"] = N, "ms per batch of frames"
        out["below_the_limit_%d" % N] = r


def c5_shape(a, out):
    from oracle import rescale_oracle as ro
    from mvoscalerecovery_amd import scale_calculator
    npool = min(a.big_frames, 8)
    pool = [synth.synth_frame(9000 + i, 20000, base_seed=4242) for i in range(npool)]
    raw = [pool[i % npool] for i in range(a.big_frames)]
    f3s, f2s = [f[0] for f in raw], [f[1] for f in raw]
    est = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=1, delaunay_workers=0, large_frames=True)
    cases, frames = resident_inputs(est, pool)
    k = launch_pair(est.ctx, [cases[i % npool] for i in range(a.big_frames)], [frames[i % npool] for i in range(a.big_frames)], ("large",),
                    a.warmup, a.repeats)
    k["features"], k["unit"], k["distinct_frames"] = 20000, "ms per batch of frames (one workgroup per frame)", npool
    out["c5_launches"] = k
    sib = scale_calculator.ScaleEstimator(1.75, window_size=5, mutate_inputs=False, triangulation="gpu", check_triangle="fixed", delaunay_workers=0)
    e = alternating({"rescale_large_frames": lambda: est.scale_calculation_batch(f3s, f2s),
                     "scale_calculator_gpu_fixed": lambda: sib.scale_calculation_batch(f3s, f2s)}, 2, max(5, a.repeats // 4), wall)
    ref = ro.OracleRescaleEstimator(1.75, window_size=5, device_seed=1)
    t = [wall(lambda f=f: ref.scale_calculation(*f)) for f in pool[:4]]
    e["cpu_oracle_one_core_s_per_frame"] = stats(t)
    e["frames"], e["unit"], e["declined"] = a.big_frames, "s per batch of frames (wall clock, results on the host)", int(est.last_declined)
    e["frames_per_s"] = {k2: a.big_frames / e[k2]["median"] for k2 in ("rescale_large_frames", "scale_calculator_gpu_fixed")}
    e["speedup_over_cpu_oracle_one_core"] = e["cpu_oracle_one_core_s_per_frame"]["median"] * a.big_frames / e["rescale_large_frames"]["median"]
    out["c5_end_to_end"] = e


def default_path_only(a, out):
    """bench.py's e2e_rescale leg and RepeatedRuns.run, default constructions: nothing this change added is imported."""
    import bench
    legs = [bench.e2e_rescale_leg(None, 0, [2000] * 1024, 2024, 32768) for _ in range(a.ab_repeats)]
    out["e2e_rescale_frames_per_s"] = stats([x for leg in legs for x in leg["timed_calls_frames_per_s"]])
    data = synth.synth_sequence_dict(4096, base_seed=43, n_lo=1800, n_hi=2200)
    rr = RepeatedRuns(1.75, window_size=5, cases=10, seed=7, triangulation="gpu", delaunay_workers=0)
    out["repeated_runs_s"] = alternating({"run": lambda: rr.run(data)}, 2, max(5, 3 * a.ab_repeats), wall)["run"]


def merge_ab(d, out):
    """The runs of --default-path-only found in `d`, this build's and the parent's, and whether the difference of the medians lies
    inside the parent's own run-to-run spread (max - min over its runs)."""
    ab = {}
    for side in ("this", "parent"):
        runs = [json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, side + "_*.json")))]
        if not runs:
            return
        ab[side] = {k: {"runs": [r[k] for r in runs], "median_of_medians": float(np.median([r[k]["median"] for r in runs])),
                        "min": min(r[k]["min"] for r in runs), "max": max(r[k]["max"] for r in runs)}
                    for k in ("e2e_rescale_frames_per_s", "repeated_runs_s")}
    for k in ("e2e_rescale_frames_per_s", "repeated_runs_s"):
        diff = ab["this"][k]["median_of_medians"] - ab["parent"][k]["median_of_medians"]
        spread = ab["parent"][k]["max"] - ab["parent"][k]["min"]
        ab[k + "_verdict"] = {"this_minus_parent": diff, "parent_spread": spread, "inside_parent_spread": bool(abs(diff) <= spread)}
    out["default_path"] = ab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--big-frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ab-repeats", type=int, default=2)
    ap.add_argument("--default-path-only", action="store_true")
    ap.add_argument("--merge-ab", metavar="DIR", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescale_large_bench.json"))
    a = ap.parse_args()
    out = {"device": _lib.default_context(0).name}
    if a.default_path_only:
        default_path_only(a, out)
    else:
        below_the_limit(a, out)
        c5_shape(a, out)
        out["counters"] = "none read: which unit bounds the kernels is not measured"
        if a.merge_ab:
            merge_ab(a.merge_ab, out)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
