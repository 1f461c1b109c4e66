#!/usr/bin/env python3
"""Times mvosr_reliability_batch with the context's HIP events on resident batches: 512 real triangulations
of 2000 features and of the ragged 300-1500 mix — 3 warm-up launches, >= 20 repetitions, median and spread — and prints ONE JSON
line: µs per frame, edges and rounds per frame, algorithmic bytes and the fraction of 8 TB/s (HBM peak; the kernel is bound by LDS
latency and barriers, far from it), and the host route the kernel replaces: tests/reliability_cases' NumPy restatement on the same
frames on one core, in both its forms (the sequential loop on a few frames, the level-scheduled form on all distinct ones).

    python profiles/reliability_bench.py [--frames 512] [--reps 20] [--out profiles/reliability_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/reliability_bench.py --reps 3 --no-cpu      # the kernel's share

Rows: SciPy's Delaunay of each frame's features below the vanishing row (64 distinct synthetic frames, repeated).  Algorithmic
bytes count each input and output once: rows 12 B, y / z / v 24 B per feature, reliability and keep 12 B per feature."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mvoscalerecovery_amd import _lib, synth  # noqa: E402
from mvoscalerecovery_amd import constants as K  # noqa: E402
from mvoscalerecovery_amd.engine import make_params  # noqa: E402

HBM_PEAK = 8.0e12


def make_frames(sizes, seed):
    """Per frame (y, z, v of the features below the vanishing row — raw, the kernel remaps —, SciPy's rows)."""
    from scipy.spatial import Delaunay
    out = []
    for i, n in enumerate(sizes):
        f3, f2 = synth.synth_frame(i, int(n), base_seed=seed)
        low = f2[:, 1] > K.VANISH
        out.append((np.ascontiguousarray(f3[low, 1]), np.ascontiguousarray(f3[low, 2]), np.ascontiguousarray(f2[low, 1]),
                    Delaunay(f2[low]).simplices.astype(np.int32)))
    return out


def time_batch(ctx, frames, reps, warmup=3):
    F = len(frames)
    cnt = np.array([len(f[0]) for f in frames], dtype=np.int32)
    padded = (cnt.astype(np.int64) + 15) & ~np.int64(15)
    off = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f[3]) for f in frames])]).astype(np.int64)
    total = int(off[-1])

    def plane(k):
        a = np.zeros(total)
        for f, o in zip(frames, off):
            a[o:o + len(f[k])] = f[k]
        return a
    d = {"off": ctx.to_device(off[:-1].copy()), "cnt": ctx.to_device(cnt), "toff": ctx.to_device(toff),
         "tri": ctx.to_device(np.concatenate([f[3] for f in frames]).reshape(-1)),
         "y": ctx.to_device(plane(0)), "z": ctx.to_device(plane(1)), "v": ctx.to_device(plane(2))}
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.y, b.z, b.v = F, d["off"].ptr, d["cnt"].ptr, d["y"].ptr, d["z"].ptr, d["v"].ptr
    b.tri1_off, b.tri1, b.max_feat, b.total_feat = d["toff"].ptr, d["tri"].ptr, int(cnt.max()), total
    o = {"reliability": ctx.empty(total, np.float64), "keep": ctx.empty(total, np.int32), "status": ctx.empty(F, np.int32)}
    p = make_params(1.75)
    call = lambda: _lib.check(ctx.lib.mvosr_reliability_batch(ctx.handle, C.byref(p), C.byref(b), o["reliability"].ptr, o["keep"].ptr,
                                                              o["status"].ptr), "mvosr_reliability_batch")
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
    status, keep, rel = o["status"].download(), o["keep"].download(), o["reliability"].download()
    assert (status == 0).all(), status
    for buf in list(d.values()) + list(o.values()):
        buf.free()
    for ev in (e0, e1):
        ctx.lib.mvosr_event_destroy(ctx.handle, ev)
    ms = np.array(ms)
    med = float(np.median(ms))
    n_feat, T = int(cnt.sum()), int(toff[-1])
    kept = sum(int((keep[off[i]:off[i] + cnt[i]] == 0).sum()) for i in range(F))
    nbytes = 12 * T + 36 * n_feat
    res = {"frames": F, "features": n_feat, "rows": T, "kept": kept, "ms_median": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()),
           "reps": int(reps), "us_per_frame": med * 1e3 / F, "frames_per_s": F / (med * 1e-3), "algorithmic_bytes": int(nbytes),
           "GBps": nbytes / (med * 1e-3) / 1e9, "fraction_of_8TBps": nbytes / (med * 1e-3) / HBM_PEAK}
    return res, [rel[off[i]:off[i] + cnt[i]] for i in range(F)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    result = {"device": ctx.name.strip(), "hbm_peak_Bps": HBM_PEAK, "legs": {}}
    rng = np.random.default_rng(7)
    mixes = {"uniform2000": np.full(args.distinct, 2000), "ragged300_1500": rng.integers(300, 1501, args.distinct)}
    for name, sizes in mixes.items():
        distinct = make_frames(sizes, seed=77)
        rep = -(-args.frames // args.distinct)
        leg, rel = time_batch(ctx, (distinct * rep)[:args.frames], args.reps)
        if not args.no_cpu:
            import reliability_cases as rc
            remap = lambda y, z: y * float(np.sin(K.CAMERA_PITCH)) + z * float(np.cos(K.CAMERA_PITCH))
            t0 = time.perf_counter()
            rounds, edges = [], []
            for k, (y, z, v, rows) in enumerate(distinct):
                r, n_rounds, _ = rc.scheduled(rows, remap(y, z), v, len(z))
                assert r.tobytes() == rel[k].tobytes(), (name, k)
                rounds.append(n_rounds)
            leg["host_numpy_scheduled_us_per_frame"] = (time.perf_counter() - t0) / len(distinct) * 1e6
            edges = [len(rc.edges_in_order(rows, len(z))) for _, z, _, rows in distinct]
            leg["rounds_per_frame"], leg["edges_per_frame"] = float(np.mean(rounds)), float(np.mean(edges))
            few = distinct[:4]
            t0 = time.perf_counter()
            for k, (y, z, v, rows) in enumerate(few):
                assert rc.sequential(rows, remap(y, z), v, len(z)).tobytes() == rel[k].tobytes(), (name, k)
            leg["host_numpy_sequential_us_per_frame"] = (time.perf_counter() - t0) / len(few) * 1e6
        result["legs"][name] = leg
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
