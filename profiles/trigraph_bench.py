#!/usr/bin/env python3
"""Times mvosr_tri_graph_batch with the context's HIP events on resident batches: 512 real second triangulations
of 2000-feature frames and of the ragged 300-1500 mix, in both forms (heights and pitch given; from the points) — 3 warm-up
launches, >= 20 repetitions, median and spread — and prints ONE JSON line: µs per frame, rows, flat rows and rounds per frame,
algorithmic bytes and the fraction of 8 TB/s (HBM peak), and the host route the kernel replaces: tests/trigraph_cases' restatement
on the same frames on one core, in both its forms (the sequential loop on a few frames, the level-scheduled form on more).  The
given form's probabilities are compared with the restatement bit for bit on the way; the from-points form's are reported as the
largest difference from them (the device's asin).

    python profiles/trigraph_bench.py [--frames 512] [--reps 20] [--out profiles/trigraph_bench.json]

Frames: the survivors of find_outliers below the vanishing row with SciPy's Delaunay over them (64 distinct synthetic frames,
repeated).  Algorithmic bytes count each input and output once: rows 12 B; given form 16 B per row in; from-points form 24 B per
feature in; out 17 B per row (p_road, p_initial, valid) and 1 B per feature (selected)."""
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

from mvoscalerecovery_amd import _lib  # noqa: E402
from mvoscalerecovery_amd.engine import make_params  # noqa: E402

HBM_PEAK = 8.0e12


def make_frames(sizes, seed):
    """Per frame (remapped survivors (n, 3), SciPy's rows, host heights, host pitch)."""
    import trigraph_cases as tc
    from oracle import scale_oracle as so
    out = []
    for i, n in enumerate(sizes):
        f3, _, rows = tc.synth_survivors(i, int(n), base_seed=seed)
        sel = so.tri_select(f3, rows)
        out.append((f3, rows, sel.heights, sel.pitch_deg))
    return out


def time_batch(ctx, frames, reps, pts, warmup=3):
    F = len(frames)
    cnt = np.array([len(f[0]) for f in frames], dtype=np.int32)
    padded = (cnt.astype(np.int64) + 15) & ~np.int64(15)
    off = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f[1]) for f in frames])]).astype(np.int64)
    total, T = int(off[-1]), int(toff[-1])

    def plane(k):
        a = np.zeros(total)
        for f, o in zip(frames, off):
            a[o:o + len(f[0])] = f[0][:, k]
        return a
    d = {"off": ctx.to_device(off[:-1].copy()), "cnt": ctx.to_device(cnt), "toff": ctx.to_device(toff),
         "tri": ctx.to_device(np.concatenate([f[1] for f in frames]).reshape(-1))}
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt = F, d["off"].ptr, d["cnt"].ptr
    b.tri2_off, b.tri2, b.max_feat, b.total_feat = d["toff"].ptr, d["tri"].ptr, int(cnt.max()), total
    h_in = p_in = None
    if pts:
        d.update(x=ctx.to_device(plane(0)), y=ctx.to_device(plane(1)), z=ctx.to_device(plane(2)))
        b.x, b.y, b.z = d["x"].ptr, d["y"].ptr, d["z"].ptr
    else:
        d.update(h=ctx.to_device(np.concatenate([f[2] for f in frames])), p=ctx.to_device(np.concatenate([f[3] for f in frames])))
        h_in, p_in = d["h"].ptr, d["p"].ptr
    o = {"p_road": ctx.empty(T, np.float64), "p_initial": ctx.empty(T, np.float64), "valid": ctx.empty(T, np.uint8),
         "selected": ctx.empty(total, np.uint8), "height_level": ctx.empty(F, np.float64), "n_flat": ctx.empty(F, np.int32),
         "n_rounds": ctx.empty(F, np.int32), "status": ctx.empty(F, np.int32)}
    out = _lib.TriGraphOutputs(**{k: v.ptr for k, v in o.items()})
    p = make_params(1.75, camera_pitch=0.0)                          # (the survivors are remapped already)
    call = lambda: _lib.check(ctx.lib.mvosr_tri_graph_batch(ctx.handle, C.byref(p), C.byref(b), h_in, p_in, C.byref(out)), "mvosr_tri_graph_batch")
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
    r = {k: v.download() for k, v in o.items()}
    assert (r["status"] == 0).all(), r["status"]
    for buf in list(d.values()) + list(o.values()):
        buf.free()
    for ev in (e0, e1):
        ctx.lib.mvosr_event_destroy(ctx.handle, ev)
    ms = np.array(ms)
    med = float(np.median(ms))
    n_feat = int(cnt.sum())
    nbytes = 12 * T + (24 * n_feat if pts else 16 * T) + 17 * T + n_feat
    res = {"frames": F, "features": n_feat, "rows": T, "flat_rows_per_frame": float(r["n_flat"].mean()), "rounds_per_frame": float(r["n_rounds"].mean()),
           "rounds_max": int(r["n_rounds"].max()), "valid_rows": int(r["valid"].sum()), "ms_median": med, "ms_min": float(ms.min()),
           "ms_max": float(ms.max()), "reps": int(reps), "us_per_frame": med * 1e3 / F, "frames_per_s": F / (med * 1e-3),
           "algorithmic_bytes": int(nbytes), "GBps": nbytes / (med * 1e-3) / 1e9, "fraction_of_8TBps": nbytes / (med * 1e-3) / HBM_PEAK}
    return res, [r["p_road"][toff[i]:toff[i + 1]] for i in range(F)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--cpu-frames", type=int, default=8)
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
        batch = (distinct * rep)[:args.frames]
        given, p_given = time_batch(ctx, batch, args.reps, pts=False)
        points, p_points = time_batch(ctx, batch, args.reps, pts=True)
        points["max_abs_dp_vs_given"] = max(float(np.abs(a - b).max()) for a, b in zip(p_given[:len(distinct)], p_points[:len(distinct)]))
        points["rows_whose_decision_differs_from_given"] = int(sum(((a > 0.5) != (b > 0.5)).sum() for a, b in zip(p_given[:len(distinct)], p_points[:len(distinct)])))
        if not args.no_cpu:
            import trigraph_cases as tc
            some = distinct[:args.cpu_frames]
            graphs = [tc.region_graph(rows) for _, rows, _, _ in some]
            t0 = time.perf_counter()
            for k, (_, rows, h, pitch) in enumerate(some):
                assert tc.scheduled(graphs[k], h, pitch)[0].tobytes() == p_given[k].tobytes(), (name, k)
            given["host_restatement_scheduled_us_per_frame"] = (time.perf_counter() - t0) / len(some) * 1e6
            few = some[:4]
            t0 = time.perf_counter()
            for k, (_, rows, h, pitch) in enumerate(few):
                assert tc.sequential(graphs[k], h, pitch).tobytes() == p_given[k].tobytes(), (name, k)
            given["host_restatement_sequential_us_per_frame"] = (time.perf_counter() - t0) / len(few) * 1e6
            given["host_frames_compared"] = len(some)
        result["legs"][name] = {"given": given, "from_points": points}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
