#!/usr/bin/env python3
"""Times mvosr_depth_check_batch and prints ONE JSON line.

    python profiles/depthcheck_bench.py [--frames 512] [--features 2000] [--big 20000] [--out profiles/depthcheck_bench.json]
                                        [--variants name=libmvosr_a.so,name=libmvosr_b.so]

kernel   --frames resident frames of --features synthetic features (synth.synth_frame, 32 distinct ones, repeated; the features below
         the vanishing row, levels drawn 17 / 8 / 75 % as a staged pass leaves them), ONE frame of them, and one frame of --big
         features.  The context's HIP events around K launches, K chosen so that the window is at least 0.3 s, after 3 warm-up
         launches; the median and the spread of 20 such windows.
         Before any timing the launch's outputs are compared by bytes with the blocked NumPy restatement
         (tests/depthcheck_cases.py) at the timed sizes: every distinct frame, the one frame, the big frame.
rates    pairs per second (n^2 per frame, n the selected points), and the share of the fp64 VALU issue peak: FP64_OPS_PER_PAIR fp64
         instructions per pair and lane in the inner loop of the saved ISA (3 subtractions / additions, 11 of the division, 10 of the
         bin, 3 maxima), over half the data sheet's 78.6 TFLOP/s (an FMA counts two there, an issue slot one).
host     on one core of the same host in the same call: a function shaped like the reference's (a Python loop over the rows, then
         np.histogram and np.max of the n x n matrix) and the blocked restatement, one population of one frame each.
variants the same launch of --frames frames through other builds of the library (the histogram-update A/B): a fresh process per
         build, alternating over two rounds.
Needs a GPU: fails without one.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_PEAK = 78.6e12            # vector fp64 FLOP/s, MI355X data sheet: half of it instructions per lane and second
FP64_OPS_PER_PAIR = 27         # fp64 VALU instructions per pair in depthcheck_kernel's inner loop (saved ISA, the loop unrolled by 4: 108)
VALU_OPS_PER_PAIR = 43
FIELDS = ("hist", "below", "above", "nan", "max", "n", "status")


def road_frames(n_frames, distinct, n_feat, seed=97531):
    """The project's synthetic frames (synth.synth_frame), the features below the vanishing row as (y, depth, level): their slopes
    gather in a few bins as a real road's do (bins_hit and largest_bin_share in the result say how much)."""
    from mvoscalerecovery_amd import synth
    base = []
    for i in range(distinct):
        f3, f2 = synth.synth_frame(900 + i, n_feat, base_seed=seed, upper_fraction=0.1)
        low = f2[:, 1] > 185
        lv = np.random.default_rng([seed, i, n_feat]).choice(np.arange(3, dtype=np.uint8), size=int(low.sum()), p=(0.17, 0.08, 0.75))
        base.append((f3[low, 1].copy(), f3[low, 2].copy(), lv))
    return [base[i % distinct] for i in range(n_frames)]


class Launch:
    """The frames resident on the device, the outputs, and the call."""

    def __init__(self, ctx, frames, tables=True):
        from mvoscalerecovery_amd import _lib
        self.ctx, self.F = ctx, len(frames)
        cnt = np.array([len(f[0]) for f in frames], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(cnt[:-1], dtype=np.int64)]).astype(np.int64)
        F, P = self.F, 3
        self.blk = ctx.block([("off", F, np.int64), ("cnt", F, np.int32), ("y", int(cnt.sum()), np.float64), ("z", int(cnt.sum()), np.float64),
                              ("level", int(cnt.sum()), np.uint8)])
        self.blk.upload({"off": off, "cnt": cnt, "y": np.concatenate([f[0] for f in frames]), "z": np.concatenate([f[1] for f in frames]),
                         "level": np.concatenate([f[2] for f in frames])})
        self.out = ctx.block([("hist", (F, P, 59), np.int64), ("below", (F, P), np.int64), ("above", (F, P), np.int64), ("nan", (F, P), np.int64),
                              ("max", (F, P), np.float64), ("n", (F, P), np.int64), ("status", F, np.int32)])
        self.tables = ctx.zeros((3, 62), np.int64) if tables else None
        self.params = _lib.DepthCheckParams(int(cnt.max()), 0)
        self.outs = _lib.DepthCheckOutputs(*(self.out[k].ptr for k in FIELDS))
        self._lib = _lib

    def __call__(self):
        b, ctx = self.blk, self.ctx
        self._lib.check(ctx.lib.mvosr_depth_check_batch(ctx.handle, self.F, b["off"].ptr, b["cnt"].ptr, b["y"].ptr, b["z"].ptr, b["level"].ptr,
                                                        C.byref(self.params), C.byref(self.outs), self.tables.ptr if self.tables is not None else None),
                        "mvosr_depth_check_batch")

    def results(self):
        self.ctx.sync()
        self.out.invalidate()
        return {k: self.out[k].download() for k in FIELDS}

    def free(self):
        self.out.free()
        self.blk.free()
        if self.tables is not None:
            self.tables.free()


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


def verify(got, frames, which):
    """The launch's outputs against the restatement, by bytes, on the frames ``which``; -> seconds per frame of the restatement."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import depthcheck_cases as dcc
    t0 = time.perf_counter()
    for f in which:
        want = dcc.depth_check_of(*frames[f])
        assert dcc.same({k: got[k][f] for k in FIELDS}, want), "frame %d differs from the restatement" % f
    return (time.perf_counter() - t0) / max(len(which), 1)


def rates(t, pairs):
    s = t["ms_median"] * 1e-3
    t.update({"pairs": int(pairs), "pairs_per_s": pairs / s, "fp64_issue_share": pairs * FP64_OPS_PER_PAIR / s / (FP64_PEAK / 2),
              "valu_issue_share": pairs * VALU_OPS_PER_PAIR / s / (FP64_PEAK / 2)})
    return t


def row_loop_numpy(y, z):
    """Shaped like the reference's function: the matrix row by row in a Python loop, then np.histogram and np.max of all of it."""
    sel = y > 0
    d, v = z[sel], y[sel] / z[sel]
    rows = []
    for i in range(v.shape[0]):
        rows.append((d - d[i]) / ((v - v[i]) + 0.000001))
    m = np.array(rows)
    return np.histogram(m.reshape(-1), np.array(list(range(-40, 20))) * 50)[0], np.max(m)


def batch_leg(ctx, args, check=True):
    frames = road_frames(args.frames, args.distinct, args.features)
    run = Launch(ctx, frames)
    run()
    got = run.results()
    res = {"frames": args.frames, "features": args.features}
    if check:
        res["restatement_s_per_frame"] = verify(got, frames, range(min(args.distinct, args.frames)))
        res["verified_frames"] = min(args.distinct, args.frames)
    pairs = int((got["n"][:, 0].astype(np.int64) ** 2).sum())
    res.update(rates(timed(ctx, run), pairs))
    res["selected_per_frame"] = float(got["n"][:, 0].mean())
    res["bins_hit"] = int(np.count_nonzero(got["hist"][:, 0].sum(0)))
    res["largest_bin_share"] = float(got["hist"][:, 0].sum(0).max() / max(pairs, 1))
    run.free()
    return res, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--big", type=int, default=20000)
    ap.add_argument("--variants", default="")
    ap.add_argument("--leg", default="all", choices=["all", "batch"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from mvoscalerecovery_amd import _lib
    ctx = _lib.default_context(0)
    if args.leg == "batch":                                       # (a variant's child process: the batch launch alone, checked on two frames)
        args.distinct = min(args.distinct, 2)
        res, _ = batch_leg(ctx, args)
        print(json.dumps(res))
        return
    result = {"device": ctx.name.strip(), "fp64_peak_flops": FP64_PEAK, "fp64_issue_peak_per_s": FP64_PEAK / 2,
              "fp64_instructions_per_pair": FP64_OPS_PER_PAIR, "valu_instructions_per_pair": VALU_OPS_PER_PAIR}
    result["batch"], frames = batch_leg(ctx, args)
    # one frame
    run = Launch(ctx, frames[:1])
    run()
    got = run.results()
    verify(got, frames, [0])
    result["one_frame"] = rates(timed(ctx, run), int(got["n"][0, 0]) ** 2)
    run.free()
    # one large frame
    big = road_frames(1, 1, args.big, seed=7)
    run = Launch(ctx, big)
    run()
    got = run.results()
    t = verify(got, big, [0])
    result["big_frame"] = rates(timed(ctx, run), int(got["n"][0, 0]) ** 2)
    result["big_frame"].update({"features": args.big, "restatement_s": t})
    run.free()
    # the host, one core: one population of one frame
    y, z, lv = frames[0]
    n_sel = int(np.count_nonzero(y > 0))
    t0 = time.perf_counter()
    h, mx = row_loop_numpy(y, z)
    t_loop = time.perf_counter() - t0
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import depthcheck_cases as dcc
    t0 = time.perf_counter()
    r = dcc.depth_check_of(y, z, np.full(y.size, 2, np.uint8))
    t_blocked = time.perf_counter() - t0
    assert np.array_equal(h, r["hist"][0]) and dcc.same_floats([mx], [r["max"][0]])
    result["host"] = {"selected": n_sel, "pairs": n_sel * n_sel, "row_loop_numpy_s": t_loop, "row_loop_numpy_pairs_per_s": n_sel * n_sel / t_loop,
                      "blocked_restatement_s_three_populations": t_blocked,
                      "blocked_restatement_three_populations_s_per_frame_over_the_batch": result["batch"]["restatement_s_per_frame"]}
    result["kernel_over_row_loop"] = result["batch"]["pairs_per_s"] / result["host"]["row_loop_numpy_pairs_per_s"]
    if args.variants:
        result["variants"] = {}
        named = [v.split("=", 1) for v in args.variants.split(",")]
        for rnd in range(2):
            for name, path in named:
                env = dict(os.environ, MVOSR_LIB_PATH=os.path.abspath(path))
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "batch", "--frames", str(args.frames), "--features",
                                      str(args.features)], env=env, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    raise RuntimeError("variant %s failed: %s" % (name, out.stderr[-2000:]))
                r = json.loads(out.stdout.strip().splitlines()[-1])
                result["variants"].setdefault(name, []).append({k: r[k] for k in ("ms_median", "ms_min", "ms_max", "pairs_per_s", "launches_per_sample")})
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
