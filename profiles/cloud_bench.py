#!/usr/bin/env python3
"""Times mvosr_point_cloud_batch with the context's HIP events on resident batches: 512 frames of 2000
features and of the ragged 300-1500 mix at 1241x376, depth and id images written by mvosr_dense_depth_batch and left on the
device — legs: float64, float64 with colours, float32, stride 4 — after 3 warm-ups, 20 repetitions, median [min-max]; and, in
the same call, the HOST route the cloud took before: ``depth_maps(ids=True)`` (both images downloaded) plus the NumPy lines of
``depth_generate``, on the same frames.  Prints ONE JSON line.

    python profiles/cloud_bench.py [--frames 512] [--reps 20] [--out profiles/cloud_bench.json]
    python profiles/cloud_bench.py --table profiles/cloud_bench.json          # DESIGN.md §3.9's table (no GPU)
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/cloud_bench.py --reps 3 --no-host      # the per-kernel split

Bytes.  ALGORITHMIC, from shapes: the depth image read once (8 P), the id image with it (4 P), 3 K of colour image, 24 K or
12 K per output array written (P pixels, K points).  REQUESTED by the two-pass design, per lane: the count pass reads the ids
of the grid pixels (4 G), the fill pass reads them again and the depths of the covered ones (4 G + 8 C), then the same colour
and output bytes (G pixels on the stride grid, C of them covered).  What DRAM moves beyond that is sector granularity: at
stride 4 a lane asks for 4 of every 16 bytes of a row it visits."""
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

from mvoscalerecovery_amd import _lib, packing, synth  # noqa: E402
from mvoscalerecovery_amd import constants as K  # noqa: E402
from mvoscalerecovery_amd.engine import DeviceBatch  # noqa: E402
from mvoscalerecovery_amd.reconstruct import Reconstruct, grid_points, pack_all  # noqa: E402

W, H, FX, CX, CY = 1241, 376, 718.856, 607.1928, 185.2157
HBM_PEAK = 8.0e12
LEGS = {"f64": dict(), "f64_colours": dict(colours=True), "f32": dict(f32=True), "f64_stride4": dict(stride=4)}


class Cam:
    width, height, fx, fy, cx, cy = W, H, FX, FX, CX, CY


def make_frames(sizes, seed):
    f3s, f2s = [], []
    for i, n in enumerate(sizes):
        f3, f2 = synth.synth_frame(i, int(n), base_seed=seed, upper_fraction=0.1)
        low = f2[:, 1] > K.VANISH
        f3s.append(np.ascontiguousarray(f3[low]))
        f2s.append(np.ascontiguousarray(f2[low]))
    return f3s, f2s


def resident_images(ctx, f3s, f2s, rows):
    """depth and id images of the batch, written by mvosr_dense_depth_batch, left on the device; and the covered counts."""
    F = len(f3s)
    pf = pack_all(f3s, f2s)
    pf.tri1_off, pf.tri1 = packing._pack_tris(rows)
    db = DeviceBatch(ctx, pf, with_tri2=False)
    d_u = ctx.to_device(pf.u)
    depth, tri_id = ctx.empty((F, H, W), np.float64), ctx.empty((F, H, W), np.int32)
    cov, st = ctx.empty(F, np.int32), ctx.empty(F, np.int32)
    o = _lib.DepthOutputs(depth.ptr, tri_id.ptr, None, cov.ptr, st.ptr)
    cam = _lib.Camera(W, H, FX, FX, CX, CY)
    b = db.struct()
    _lib.check(ctx.lib.mvosr_dense_depth_batch(ctx.handle, C.byref(b), 1, d_u.ptr, None, C.byref(cam), C.byref(o), 0, 0), "mvosr_dense_depth_batch")
    ctx.sync()
    assert (st.download() == 0).all()
    covered = cov.download().astype(np.int64)
    for buf in (d_u, cov, st):
        buf.free()
    db.free()
    return depth, tri_id, covered


def time_leg(ctx, depth, tri_id, image, covered, reps, colours=False, f32=False, stride=1, warmup=3):
    F = depth.shape[0]
    dtype = np.float32 if f32 else np.float64
    cap = int(np.minimum(covered, grid_points(W, H, stride)).sum())
    pts = ctx.empty((cap, 3), dtype)
    cols = ctx.empty((cap, 3), dtype) if colours else None
    off, ovf = ctx.empty(F + 1, np.int64), ctx.empty(1, np.int32)
    i = _lib.CloudInputs(depth.ptr, tri_id.ptr, image.ptr if colours else None, None, F)
    p = _lib.CloudParams(0.0, 0.0, stride, _lib.CLOUD_F32 if f32 else 0)
    o = _lib.CloudOutputs(pts.ptr, cols.ptr if colours else None, off.ptr, ovf.ptr, cap)
    cam = _lib.Camera(W, H, FX, FX, CX, CY)
    call = lambda: _lib.check(ctx.lib.mvosr_point_cloud_batch(ctx.handle, C.byref(i), C.byref(cam), C.byref(p), C.byref(o)), "mvosr_point_cloud_batch")
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
    n_pts = int(off.download()[-1])
    assert int(ovf.download()[0]) == 0 and n_pts <= cap
    for buf in (pts, off, ovf) + ((cols,) if colours else ()):
        buf.free()
    for ev in (e0, e1):
        ctx.lib.mvosr_event_destroy(ctx.handle, ev)
    ms = np.array(ms)
    med = float(np.median(ms))
    P, G = F * W * H, F * grid_points(W, H, stride)
    row = 12 if f32 else 24
    out_bytes = n_pts * row * (2 if colours else 1) + (3 * n_pts if colours else 0)
    algorithmic = 12 * P + out_bytes
    requested = 4 * G + (4 * G + 8 * n_pts) + out_bytes
    return {"frames": F, "points": n_pts, "points_per_frame": n_pts / F, "dtype": np.dtype(dtype).name, "colours": bool(colours), "stride": stride,
            "ms_median": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()), "reps": int(reps),
            "frames_per_s": F / (med * 1e-3), "us_per_frame": med * 1e3 / F, "Mpoints_per_s": n_pts / (med * 1e-3) / 1e6,
            "algorithmic_bytes": int(algorithmic), "requested_bytes": int(requested),
            "GBps": algorithmic / (med * 1e-3) / 1e9, "fraction_of_8TBps": algorithmic / (med * 1e-3) / HBM_PEAK,
            "requested_GBps": requested / (med * 1e-3) / 1e9, "requested_fraction_of_8TBps": requested / (med * 1e-3) / HBM_PEAK}


def host_route(ctx, f3s, f2s, rows):
    """What the cloud cost before: depth_maps with ids (both images cross the link) and depth_generate's NumPy lines per frame."""
    rec = Reconstruct(Cam, ctx=ctx)
    t0 = time.perf_counter()
    res = rec.depth_maps(f3s, f2s, tris=rows, ids=True)
    t1 = time.perf_counter()
    n = 0
    for f in range(len(f3s)):
        yy, xx = np.nonzero(res.tri_id[f] >= 0)
        d = res.depth[f][yy, xx]
        px = (xx.astype(np.float64) - CX) / FX
        py = (yy.astype(np.float64) - CY) / FX
        n += len(np.stack([px * d, py * d, d], axis=1))
    t2 = time.perf_counter()
    F = len(f3s)
    return {"frames": F, "points": n, "depth_maps_s": t1 - t0, "numpy_s": t2 - t1, "total_s": t2 - t0, "frames_per_s": F / (t2 - t0),
            "ms_per_frame": (t2 - t0) * 1e3 / F}


def device_route(ctx, f3s, f2s, rows):
    """point_clouds end to end on the same frames (rasterise, compact, download the points), wall clock."""
    rec = Reconstruct(Cam, ctx=ctx)
    t0 = time.perf_counter()
    res = rec.point_clouds(f3s, f2s, tris=rows, budget_bytes=32 << 30)
    t1 = time.perf_counter()
    return {"frames": len(f3s), "points": int(res.offsets[-1]), "total_s": t1 - t0, "frames_per_s": len(f3s) / (t1 - t0),
            "ms_per_frame": (t1 - t0) * 1e3 / len(f3s)}


def render_table(path):
    with open(path) as fh:
        r = json.loads(fh.readline())
    print("| batch (512 frames, 1241×376, ids) | leg | points per frame | ms per call | µs per frame | Mpoints/s | algorithmic MB per frame | GB/s | of 8 TB/s | requested MB per frame | requested, of 8 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, g in r["legs"].items():
        batch, leg = name.split("/")
        print("| `%s` | %s | %.0f | %.3f [%.3f–%.3f] | %.2f | %.0f | %.2f | %.0f | %.3f | %.2f | %.3f |" % (
            batch, leg, g["points_per_frame"], g["ms_median"], g["ms_min"], g["ms_max"], g["us_per_frame"], g["Mpoints_per_s"],
            g["algorithmic_bytes"] / g["frames"] / 1e6, g["GBps"], g["fraction_of_8TBps"], g["requested_bytes"] / g["frames"] / 1e6,
            g["requested_fraction_of_8TBps"]))
    for name, g in r.get("host_route", {}).items():
        d = r["device_route"][name]
        print("\n`%s`, %d frames end to end: host route (images downloaded, NumPy) %.2f s = %.2f ms per frame (%.2f s of it `depth_maps`); "
              "`point_clouds` (points downloaded) %.2f s = %.2f ms per frame." % (name, g["frames"], g["total_s"], g["ms_per_frame"], g["depth_maps_s"],
                                                                                 d["total_s"], d["ms_per_frame"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None, help="print DESIGN.md's table from a result file and exit (no GPU)")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.table:
        return render_table(args.table)
    ctx = _lib.default_context(0)
    result = {"device": ctx.name.strip(), "image": [W, H], "hbm_peak_Bps": HBM_PEAK, "legs": {}, "host_route": {}, "device_route": {}}
    rng = np.random.default_rng(7)
    mixes = {"uniform2000": np.full(args.distinct, 2000), "ragged300_1500": rng.integers(300, 1501, args.distinct)}
    for name, sizes in mixes.items():
        f3s, f2s = make_frames(sizes, seed=77)
        rows = [np.ascontiguousarray(t, dtype=np.int32) for t in packing.delaunay_many(f2s, 0)]
        rep = -(-args.frames // args.distinct)
        f3b, f2b, rb = (f3s * rep)[:args.frames], (f2s * rep)[:args.frames], (rows * rep)[:args.frames]
        depth, tri_id, covered = resident_images(ctx, f3b, f2b, rb)
        image = ctx.to_device(np.random.default_rng(1).integers(0, 256, (args.frames, H, W, 3), dtype=np.uint8))
        for leg, kw in LEGS.items():
            result["legs"]["%s/%s" % (name, leg)] = time_leg(ctx, depth, tri_id, image, covered, args.reps, **kw)
        for buf in (depth, tri_id, image):
            buf.free()
        if not args.no_host:
            result["device_route"][name] = device_route(ctx, f3b, f2b, rb)
            result["host_route"][name] = host_route(ctx, f3b, f2b, rb)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
