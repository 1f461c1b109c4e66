#!/usr/bin/env python3
"""Times mvosr_dense_depth_batch with the context's HIP events on resident batches: 512 frames of 2000
features and of the ragged 300-1500 mix at 1241x376, with and without the id image — after warm-up, >= 20 repetitions,
median and spread — and prints ONE JSON line: frames/s, ms per call, algorithmic bytes, achieved GB/s, the fraction of
8 TB/s (HBM peak) and of the 6.29 TB/s copy rate measured on this device (profiles/hbm_rate.py), and the CPU rate of
tests/depth_cases.py on the same box.

    python profiles/depth_bench.py [--frames 512] [--reps 20] [--out profiles/r07_depth_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/depth_bench.py --reps 3 --no-cpu      # the per-kernel split

Rows: SciPy's Delaunay of each frame's features below the vanishing row (64 distinct synthetic frames, repeated); the
timed call is the two launches of the entry point (triangle_model_kernel + depth_raster_kernel), nothing else."""
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

from mvoscalerecovery_amd import _lib, packing, synth  # noqa: E402
from mvoscalerecovery_amd import constants as K  # noqa: E402
from mvoscalerecovery_amd.engine import DeviceBatch  # noqa: E402
from mvoscalerecovery_amd.reconstruct import pack_all  # noqa: E402

W, H, FX, CX, CY = 1241, 376, 718.856, 607.1928, 185.2157
HBM_PEAK, COPY_RATE = 8.0e12, 6.29e12


def algorithmic_bytes(n_frames, n_rows, n_feat, ids):
    """8 W H [+ 4 W H with ids] per frame + 32 T (datas) + 12 T (rows) + 40 M (x, y, z, u, v)."""
    return n_frames * W * H * (12 if ids else 8) + 44 * n_rows + 40 * n_feat


def make_frames(sizes, seed):
    f3s, f2s = [], []
    for i, n in enumerate(sizes):
        f3, f2 = synth.synth_frame(i, int(n), base_seed=seed, upper_fraction=0.1)
        low = f2[:, 1] > K.VANISH
        f3s.append(np.ascontiguousarray(f3[low]))
        f2s.append(np.ascontiguousarray(f2[low]))
    return f3s, f2s


def time_batch(ctx, f3s, f2s, rows, ids, reps, warmup=3):
    F = len(f3s)
    pf = pack_all(f3s, f2s)
    pf.tri1_off, pf.tri1 = packing._pack_tris(rows)
    db = DeviceBatch(ctx, pf, with_tri2=False)
    d_u = ctx.to_device(pf.u)
    depth = ctx.empty((F, H, W), np.float64)
    tri_id = ctx.empty((F, H, W), np.int32) if ids else None
    cov, st = ctx.empty(F, np.int32), ctx.empty(F, np.int32)
    o = _lib.DepthOutputs(depth.ptr, tri_id.ptr if ids else None, None, cov.ptr, st.ptr)
    cam = _lib.Camera(W, H, FX, FX, CX, CY)
    b = db.struct()
    call = lambda: _lib.check(ctx.lib.mvosr_dense_depth_batch(ctx.handle, C.byref(b), 1, d_u.ptr, None, C.byref(cam), C.byref(o), 0, 0),
                              "mvosr_dense_depth_batch")
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
    status, covered = st.download(), cov.download()
    assert (status == 0).all(), status
    for buf in (d_u, depth, cov, st) + ((tri_id,) if ids else ()):
        buf.free()
    db.free()
    for ev in (e0, e1):
        ctx.lib.mvosr_event_destroy(ctx.handle, ev)
    ms = np.array(ms)
    n_rows, n_feat = int(pf.tri1_off[-1]), int(pf.feat_cnt.sum())
    nbytes = algorithmic_bytes(F, n_rows, n_feat, ids)
    med = float(np.median(ms))
    return {"frames": F, "ids": bool(ids), "features": n_feat, "rows": n_rows, "covered_fraction": float(covered.sum() / (F * W * H)),
            "ms_median": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()), "reps": int(reps),
            "frames_per_s": F / (med * 1e-3), "us_per_frame": med * 1e3 / F, "algorithmic_bytes": int(nbytes),
            "GBps": nbytes / (med * 1e-3) / 1e9, "fraction_of_8TBps": nbytes / (med * 1e-3) / HBM_PEAK,
            "fraction_of_copy_rate": nbytes / (med * 1e-3) / COPY_RATE}


def render_table(path):
    """The markdown table of DESIGN.md §3.8 from a result file."""
    with open(path) as fh:
        r = json.loads(fh.readline())
    print("| batch (512 frames, 1241×376) | features / rows per frame | ms per call | µs per frame | frames/s | algorithmic MB per frame | GB/s | of 8 TB/s | of the 6.29 TB/s copy rate |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, g in r["legs"].items():
        print("| `%s` | %.0f / %.0f | %.3f [%.3f–%.3f] | %.2f | %.0f k | %.2f | %.0f | %.3f | %.3f |" % (
            name, g["features"] / g["frames"], g["rows"] / g["frames"], g["ms_median"], g["ms_min"], g["ms_max"], g["us_per_frame"],
            g["frames_per_s"] / 1e3, g["algorithmic_bytes"] / g["frames"] / 1e6, g["GBps"], g["fraction_of_8TBps"], g["fraction_of_copy_rate"]))
    if "cpu_depth_cases_s_per_frame" in r:
        print("\nCPU, same box: `tests/depth_cases.py` (NumPy) %.3f s per 2000-feature frame; seconds per frame of the reference: %s." % (
            r["cpu_depth_cases_s_per_frame"], r["reference_s_per_frame"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None, help="print DESIGN.md's table from a result file and exit (no GPU)")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.table:
        return render_table(args.table)
    ctx = _lib.default_context(0)
    result = {"device": ctx.name.strip(), "image": [W, H], "hbm_peak_Bps": HBM_PEAK, "copy_rate_Bps": COPY_RATE, "legs": {}}
    rng = np.random.default_rng(7)
    mixes = {"uniform2000": np.full(args.distinct, 2000), "ragged300_1500": rng.integers(300, 1501, args.distinct)}
    first = None
    for name, sizes in mixes.items():
        f3s, f2s = make_frames(sizes, seed=77)
        rows = [np.ascontiguousarray(t, dtype=np.int32) for t in packing.delaunay_many(f2s, 0)]
        first = first or (f3s[0], f2s[0], rows[0])
        rep = -(-args.frames // args.distinct)
        f3b, f2b, rb = (f3s * rep)[:args.frames], (f2s * rep)[:args.frames], (rows * rep)[:args.frames]
        for ids in (False, True):
            result["legs"]["%s_%s" % (name, "ids" if ids else "depth")] = time_batch(ctx, f3b, f2b, rb, ids, args.reps)
    if not args.no_cpu:
        import depth_cases as dc
        f3, f2, r = first
        cam = dc.camera(W, H)
        t0 = time.perf_counter()
        tri, _ = dc.locate(f2, r, W, H)
        dc.depth64(dc.model64(f3, r), tri, cam)
        result["cpu_depth_cases_s_per_frame"] = time.perf_counter() - t0
    result["reference_s_per_frame"] = "2.4-2.8 (the reference's depth_generate, 2000 features, measured on the build container's CPU only)"
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
