"""Ten RANSAC runs of a sequence in one pass against ten passes, rescale.ScaleEstimator's device-resident mode:

  (a) kernel   512 resident 2000-feature frames, C = 10 cases, H = 100: one launch of mvosr_flat_ransac_batch (asked for tri_flags)
               plus one of mvosr_flat_ransac_cases_batch, for cases_per_group G in {1, 2, 5, 10} — against TEN launches of
               mvosr_flat_ransac_batch over the same resident batch, the route before the cases kernel.  HIP events around each
               variant, warm-up, median / min / max of `--repeats` (>= 20) measurements.
  (b) e2e      RepeatedRuns(cases=10).run on a 4096-frame dict against ten offline.run_sequence_batched calls on ten estimators
               (built before the clock starts): wall clock, warm-up, median / min / max.

Writes profiles/repeats_bench.json.  python profiles/repeats_bench.py [--frames 512] [--features 2000] [--seq 4096]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mvoscalerecovery_amd import _lib, offline, synth                       # noqa: E402
from mvoscalerecovery_amd.rescale import RepeatedRuns, ScaleEstimator       # noqa: E402


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def kernel_level(a, out):
    import flat_cases as fc
    F, N, H, Cn = a.frames, a.features, 100, 10
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
    seeds = ctx.to_device(np.arange(100, 100 + Cn, dtype=np.uint64))
    o = {k: ctx.zeros(sh, dt) for k, (sh, dt) in {"raw_scale": (F, np.float64), "height_level": (F, np.float64), "model": ((F, 4), np.float64),
                                                   "best_ic": (F, np.int32), "used": (F, np.int32), "n_kept": (F, np.int32), "status": (F, np.int32),
                                                   "tri_flags": (T, np.uint8)}.items()}
    co = {k: ctx.zeros(sh, dt) for k, (sh, dt) in {"raw_scale": ((F, Cn), np.float64), "model": ((F, Cn, 4), np.float64), "best_ic": ((F, Cn), np.int32),
                                                    "used": ((F, Cn), np.int32), "status": ((F, Cn), np.int32), "count_form": (F, np.int32)}.items()}
    ro = _lib.RescaleOutputs(o["raw_scale"].ptr, o["height_level"].ptr, o["model"].ptr, o["best_ic"].ptr, o["used"].ptr, o["n_kept"].ptr,
                             o["status"].ptr, None, o["tri_flags"].ptr, None)
    cro = _lib.RescaleCasesOutputs(co["raw_scale"].ptr, co["model"].ptr, co["best_ic"].ptr, co["used"].ptr, co["status"].ptr, None, co["count_form"].ptr)

    def single(seed):
        rp = _lib.RescaleParams(0, 10, -80.0, -85.0, 0.9, 12, H, 0.005, 0.8, 1.75, seed, 0)
        _lib.check(ctx.lib.mvosr_flat_ransac_batch(ctx.handle, C.byref(b), keep.ptr, C.byref(rp), None, None, None, C.byref(ro), max_tri), "flat_ransac")

    def cases(G):
        rp = _lib.RescaleParams(0, 10, -80.0, -85.0, 0.9, 12, H, 0.005, 0.8, 1.75, 0, 0)
        _lib.check(ctx.lib.mvosr_flat_ransac_cases_batch(ctx.handle, C.byref(b), keep.ptr, C.byref(rp), seeds.ptr, Cn, G, None, None, None,
                                                         o["tri_flags"].ptr, C.byref(cro), max_tri), "flat_ransac_cases")

    e0, e1 = ctx.event(), ctx.event()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.repeats):
            ctx.record(e0)
            fn()
            ctx.record(e1)
            ctx.sync()
            ms.append(ctx.elapsed_ms(e0, e1))
        return stats(ms)

    k = {"frames": F, "features": N, "n_hyp": H, "n_cases": Cn, "unit": "ms per batch",
         "lds_bytes_cases": int(ctx.lib.mvosr_flat_ransac_cases_lds_bytes(int(b.max_feat), max_tri, H))}
    k["ten_launches_flat_ransac"] = timed(lambda: [single(100 + c) for c in range(Cn)])
    k["one_launch_flat_ransac"] = timed(lambda: single(100))
    for G in (1, 2, 5, 10):
        k["flat_ransac_plus_cases_G%d" % G] = timed(lambda: (single(100), cases(G)))
        k["cases_alone_G%d" % G] = timed(lambda: cases(G))
    st = co["status"].download()
    k["fitted_fraction"] = float(np.mean(st == 0))
    k["count_forms"] = {int(v): int(c) for v, c in zip(*np.unique(co["count_form"].download(), return_counts=True))}
    k["mean_list"] = float(3 * o["n_kept"].download().mean())
    best = min((1, 2, 5, 10), key=lambda G: k["flat_ransac_plus_cases_G%d" % G]["median"])
    k["fastest_G"] = best
    k["speedup_vs_ten_launches"] = k["ten_launches_flat_ransac"]["median"] / k["flat_ransac_plus_cases_G%d" % best]["median"]
    out["kernel"] = k
    for buf in list(o.values()) + list(co.values()) + list(d.values()) + [keep, seeds]:
        buf.free()


def end_to_end(a, out):
    Cn = 10
    data = synth.synth_sequence_dict(a.seq, base_seed=43, n_lo=a.features - 200, n_hi=a.features + 200)
    rr = RepeatedRuns(1.75, window_size=5, cases=Cn, seed=7, triangulation="gpu", delaunay_workers=0)
    ests = [ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=s, delaunay_workers=0) for s in rr.seeds]

    def timed(fn, reps):
        for _ in range(a.warmup_e2e):
            fn()
        s = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            s.append(time.perf_counter() - t0)
        return stats(s)
    e = {"frames": a.seq, "features": "%d-%d" % (a.features - 200, a.features + 200), "n_cases": Cn, "unit": "s per sequence x 10 cases"}
    e["repeated_runs"] = timed(lambda: rr.run(data), a.repeats)
    e["ten_run_sequence_batched"] = timed(lambda: [offline.run_sequence_batched(data, est) for est in ests], a.repeats)
    e["speedup"] = e["ten_run_sequence_batched"]["median"] / e["repeated_runs"]["median"]
    e["faster_by_more_than_the_spread"] = bool(e["repeated_runs"]["max"] < e["ten_run_sequence_batched"]["min"])
    out["e2e"] = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--warmup-e2e", type=int, default=1)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeats_bench.json"))
    a = ap.parse_args()
    out = {"device": _lib.default_context(0).name}
    kernel_level(a, out)
    if not a.skip_e2e:
        end_to_end(a, out)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
