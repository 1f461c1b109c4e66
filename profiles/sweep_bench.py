"""The estimator's constants swept in one run against one run per setting, rescale.ScaleEstimator's device-resident mode:

  (a) kernel   512 resident 2000-feature frames: ONE launch of mvosr_flat_selection_sweep_batch at n_sel = 1, 4, 8, 16 — against
               n_sel launches of mvosr_flat_ransac_batch asked for tri_flags, each with one setting's thresholds and factor: what a
               caller had to do on device rows before the sweep kernel (that call also fits a plane nobody reads).  HIP events
               around each variant, the two alternating, warm-up, median / min / max of `--repeats` (>= 20) measurements.
  (b) e2e      ConstantSweep.run at K = 1, 4, 16 configs on a 4096-frame dict, ten cases — against K RepeatedRuns(constants=...)
               .run calls (built before the clock starts): wall clock around calls that end with the results on the host, the
               two alternating, warm-up, median / min / max.
  --repeated-runs-only   times RepeatedRuns(...).run with the default constants and nothing else, importing nothing this change
               added: the same file run from a checkout of the parent commit gives the parent's figure for (b) at K = 1.

Writes profiles/sweep_bench.json.  python profiles/sweep_bench.py [--frames 512] [--features 2000] [--seq 4096]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mvoscalerecovery_amd import _lib, synth                                # noqa: E402
from mvoscalerecovery_amd.rescale import RepeatedRuns, ScaleEstimator       # noqa: E402

SETTINGS = [(lo, ti, fa) for lo in (-80.0, -75.0) for ti in (-85.0, -88.0) for fa in (0.9, 1.0, 0.8, 0.95)]     # 16 distinct selections


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


def kernel_level(a, out):
    import flat_cases as fc
    F, N, H = a.frames, a.features, 100
    est = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=1, delaunay_workers=0)
    ctx = est.ctx
    raw = [synth.synth_frame(7000 + i, N, base_seed=4242, upper_fraction=0.1) for i in range(F)]
    est.scale_calculation_batch([f[0] for f in raw], [f[1] for f in raw], stage=True)
    frames = []
    for i, (f3, f2) in enumerate(raw):
        valid = np.asarray(est.last["valid"][i], bool)
        keep = np.where(valid, 1, -1 if int(valid.sum()) > 10 else 0).astype(np.int32)
        frames.append(fc.Frame("f%d" % i, f3[f2[:, 1] > est.vanish], est.last["tris2"][i], keep=keep))
    b, d, toff, max_tri = fc._batch(ctx, frames, compact=False)
    T = max(int(toff[-1]), 1)
    keep = ctx.to_device(np.concatenate([f.keep for f in frames]).astype(np.int32))
    S = len(SETTINGS)
    o = {k: ctx.zeros(sh, dt) for k, (sh, dt) in {"raw_scale": (F, np.float64), "height_level": (F, np.float64), "model": ((F, 4), np.float64),
                                                   "best_ic": (F, np.int32), "used": (F, np.int32), "n_kept": (F, np.int32), "status": (F, np.int32),
                                                   "tri_flags": ((S, T), np.uint8)}.items()}
    so = {k: ctx.zeros(sh, dt) for k, (sh, dt) in {"tri_flags": ((S, T), np.uint8), "height_level": ((F, S), np.float64),
                                                    "n_kept": ((F, S), np.int32), "status": (F, np.int32)}.items()}

    def single(s):
        lo, ti, fa = SETTINGS[s]
        ro = _lib.RescaleOutputs(o["raw_scale"].ptr, o["height_level"].ptr, o["model"].ptr, o["best_ic"].ptr, o["used"].ptr, o["n_kept"].ptr,
                                 o["status"].ptr, None, o["tri_flags"].ptr + s * T, None)
        rp = _lib.RescaleParams(0, 10, lo, ti, fa, 12, H, 0.005, 0.8, 1.75, 100, 0)
        _lib.check(ctx.lib.mvosr_flat_ransac_batch(ctx.handle, C.byref(b), keep.ptr, C.byref(rp), None, None, None, C.byref(ro), max_tri), "flat_ransac")

    def sweep(n):
        lo, ti, fa = (np.array([x[i] for x in SETTINGS[:n]], dtype=np.float64) for i in range(3))
        _lib.check(ctx.lib.mvosr_flat_selection_sweep_batch(ctx.handle, C.byref(b), keep.ptr, None, n, _lib.addr(lo), _lib.addr(ti), _lib.addr(fa),
                                                            so["tri_flags"].ptr, so["height_level"].ptr, so["n_kept"].ptr, so["status"].ptr, None,
                                                            max_tri), "flat_selection_sweep")
    e0, e1 = ctx.event(), ctx.event()

    def clock(fn):
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1)
    k = {"frames": F, "features": N, "rows_per_frame": float(np.mean(np.diff(toff))), "unit": "ms per batch of frames, all settings",
         "lds_bytes_sweep": int(ctx.lib.mvosr_flat_selection_sweep_lds_bytes(int(b.max_feat), max_tri, S))}
    for n in (1, 4, 8, 16):
        r = alternating({"sweep_one_launch": lambda: sweep(n), "flat_ransac_n_launches": lambda: [single(s) for s in range(n)]},
                        a.warmup, a.repeats, clock)
        r["ratio_of_medians"] = r["flat_ransac_n_launches"]["median"] / r["sweep_one_launch"]["median"]
        r["sweep_faster_by_more_than_the_spread"] = bool(r["sweep_one_launch"]["max"] < r["flat_ransac_n_launches"]["min"])
        r["sweep_slower_by_more_than_the_spread"] = bool(r["sweep_one_launch"]["min"] > r["flat_ransac_n_launches"]["max"])
        k["n_sel_%d" % n] = r
    # (the two routes wrote the same planes: what is timed computes the same thing)
    k["planes_equal"] = bool(np.array_equal(o["tri_flags"].download(), so["tri_flags"].download()))
    k["mean_kept_rows"] = float(so["n_kept"].download().mean())
    out["kernel"] = k
    for buf in list(o.values()) + list(so.values()) + list(d.values()) + [keep]:
        buf.free()


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def sequence(a):
    return synth.synth_sequence_dict(a.seq, base_seed=43, n_lo=a.features - 200, n_hi=a.features + 200)


def repeated_runs_only(a, out):
    data = sequence(a)
    rr = RepeatedRuns(1.75, window_size=5, cases=10, seed=7, triangulation="gpu", delaunay_workers=0)
    r = alternating({"repeated_runs": lambda: rr.run(data)}, a.warmup_e2e, a.repeats, wall)
    out["e2e_repeated_runs_only"] = dict(r, frames=a.seq, features="%d-%d" % (a.features - 200, a.features + 200), n_cases=10,
                                         unit="s per sequence x 10 cases")


def end_to_end(a, out):
    from mvoscalerecovery_amd.rescale import ConstantSweep
    data = sequence(a)
    grids = {1: ConstantSweep.grid(), 4: ConstantSweep.grid(loose_deg=[-80.0, -75.0], height_factor=[0.9, 1.0]),
             16: ConstantSweep.grid(loose_deg=[-80.0, -75.0], tight_deg=[-85.0, -88.0], height_factor=[0.9, 1.0], n_hyp=[100, 30])}
    e = {"frames": a.seq, "features": "%d-%d" % (a.features - 200, a.features + 200), "n_cases": 10, "unit": "s per sequence x K configs x 10 cases"}
    for K, configs in grids.items():
        assert len(configs) == K
        sweep = ConstantSweep(1.75, configs, window_size=5, cases=10, seed=7, triangulation="gpu", delaunay_workers=0)
        runs = [RepeatedRuns(1.75, window_size=5, cases=10, seed=7, triangulation="gpu", delaunay_workers=0, constants=k) for k in configs]
        r = alternating({"constant_sweep": lambda: sweep.run(data), "k_repeated_runs": lambda: [rr.run(data) for rr in runs]},
                        a.warmup_e2e, a.repeats, wall)
        r["selections"], r["pairs"] = len(sweep._sels), len(sweep._pairs)
        r["ratio_of_medians"] = r["k_repeated_runs"]["median"] / r["constant_sweep"]["median"]
        r["sweep_faster_by_more_than_the_spread"] = bool(r["constant_sweep"]["max"] < r["k_repeated_runs"]["min"])
        r["sweep_slower_by_more_than_the_spread"] = bool(r["constant_sweep"]["min"] > r["k_repeated_runs"]["max"])
        e["K_%d" % K] = r
    out["e2e"] = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--warmup-e2e", type=int, default=2)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--repeated-runs-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_bench.json"))
    a = ap.parse_args()
    out = {"device": _lib.default_context(0).name}
    if a.repeated_runs_only:
        repeated_runs_only(a, out)
    else:
        kernel_level(a, out)
        if not a.skip_e2e:
            end_to_end(a, out)
            repeated_runs_only(a, out)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
