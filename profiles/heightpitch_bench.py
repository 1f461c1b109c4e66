"""us per 2000-feature frame of the height-and-pitch estimator on 512 resident frames:

  fused    mvosr_height_pitch_batch, one launch (events around repeated launches on the resident batch);
  staged   the chain of the entry points that existed before it, on the same frames: mvosr_triangle_batch (back-projection and
           per-row normals; it does not hand out the selection, so the lists are the fused launch's, taken as given), a host round
           trip for the list lengths, the upload of the lists' planes and the triples, mvosr_ransac_plane_batch, a round trip for
           the models, and one mvosr_plane_inliers call per frame with its model from the host — no refinement;
  numpy    tests/heightpitch_cases.py's float64 restatement of the script on one core (a few frames).

Writes profiles/heightpitch_bench.json.  python profiles/heightpitch_bench.py [--frames 512] [--features 2000]"""
import argparse
import ctypes as C
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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--numpy-frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heightpitch_bench.json"))
    a = ap.parse_args()
    F, N, H = a.frames, a.features, 500
    frames = []
    for i in range(F):
        f3, f2 = synth.synth_frame(9000 + i, N, base_seed=4242)
        frames.append(np.stack([f2[:, 0], f2[:, 1], f3[:, 2]], 1))
    rows = [Delaunay(p[:, 0:2]).simplices.astype(np.int32) for p in frames]
    priors = [hp.frame_prior(0.002 * np.sin(i)) for i in range(F)]
    est = hp.HeightPitchEstimator(seed=1)
    ctx, lib = est.ctx, est.ctx.lib
    res = est.launch(frames, priors, tris=rows, stage=True, timing=a.repeats)
    assert not res["status"].any(), np.unique(res["status"], return_counts=True)
    fused_us = 1e3 * res["kernel_ms"] / F

    # ---- the staged chain
    lists = res["point_list"]
    M = np.array([len(l) for l in lists], dtype=np.int32)
    rng = np.random.default_rng(5)
    triples = np.stack([np.stack([rng.choice(int(m), 3, replace=False) for _ in range(H)]) for m in M]).astype(np.int32)
    cnt = np.full(F, N, dtype=np.int32)
    off = (np.arange(F, dtype=np.int64) * N)
    planes = np.concatenate(frames).T.copy()
    toff = np.concatenate([[0], np.cumsum([len(t) for t in rows])]).astype(np.int64)
    d = {k: ctx.to_device(v) for k, v in dict(off=off, cnt=cnt, u=planes[0], v=planes[1], z=planes[2], toff=toff,
                                              tri=np.concatenate(rows).reshape(-1)).items()}
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.x, b.v, b.z = F, d["off"].ptr, d["cnt"].ptr, d["u"].ptr, d["v"].ptr, d["z"].ptr
    b.tri1_off, b.tri1, b.max_feat, b.total_feat = d["toff"].ptr, d["tri"].ptr, N, F * N
    height, counts, status = ctx.zeros(F, np.float64), ctx.zeros((F, 2), np.int32), ctx.zeros(F, np.int32)
    P = [hp.back_project(p) for p in frames]                                           # (the host's copy, for the lists' planes)
    mask = ctx.zeros(F * N, np.uint8)
    px, py, pz = (ctx.to_device(np.concatenate(P)[:, k].copy()) for k in range(3))
    stage = {}

    def chain():
        t0 = time.perf_counter()
        _lib.check(lib.mvosr_triangle_batch(ctx.handle, C.byref(b), hp.FOCUS, hp.CX, hp.CY, 0.98, 3.0, height.ptr, counts.ptr, status.ptr))
        status.download()                                                               # round trip 1: the host learns the lists
        t1 = time.perf_counter()
        loff = np.concatenate([[0], np.cumsum(M)]).astype(np.int64)
        lp = np.concatenate([P[f][lists[f]] for f in range(F)])
        bufs = [ctx.to_device(loff[:-1].copy()), ctx.to_device(M), ctx.to_device(lp[:, 0].copy()), ctx.to_device(lp[:, 1].copy()),
                ctx.to_device(lp[:, 2].copy()), ctx.to_device(triples)]
        model, best, used = ctx.zeros((F, 4), np.float64), ctx.zeros(F, np.int32), ctx.zeros(F, np.int32)
        t2 = time.perf_counter()
        _lib.check(lib.mvosr_ransac_plane_batch(ctx.handle, F, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, H,
                                                0.005, 0.8, None, model.ptr, best.ptr, used.ptr))
        m = model.download()                                                            # round trip 2: the models
        t3 = time.perf_counter()
        for f in range(F):
            mm = np.ascontiguousarray(m[f])
            _lib.check(lib.mvosr_plane_inliers(ctx.handle, N, px.ptr + 8 * f * N, py.ptr + 8 * f * N, pz.ptr + 8 * f * N, _lib.addr(mm), 0.01,
                                               mask.ptr + f * N))
        ctx.sync()
        t4 = time.perf_counter()
        for x in bufs + [model, best, used]:
            x.free()
        stage.update(triangle_batch=t1 - t0, host_lists_upload=t2 - t1, ransac=t3 - t2, inliers=t4 - t3)
        return t4 - t0
    chain()
    staged = min(chain() for _ in range(3))

    # ---- NumPy on one core
    import heightpitch_cases as hc
    t0 = time.perf_counter()
    for f in range(a.numpy_frames):
        hc.restate(frames[f], rows[f], 0.002 * np.sin(f), hc.draw_positions(1, f, H, int(M[f])))
    numpy_us = 1e6 * (time.perf_counter() - t0) / a.numpy_frames

    # the launch's byte and flop floors: 24 N + 12 T bytes in, ~N bytes out; 6 M H flops of counting
    T = float(np.mean([len(t) for t in rows]))
    out = {"device": ctx.name, "frames": F, "features": N, "n_hyp": H, "mean_rows": T, "mean_list": float(M.mean()),
           "fused_us_per_frame": fused_us, "staged_us_per_frame": 1e6 * staged / F,
           "staged_parts_us_per_frame": {k: 1e6 * v / F for k, v in stage.items()}, "numpy_us_per_frame": numpy_us,
           "hbm_bytes_per_frame": 24 * N + 12 * T + N, "count_tests_per_frame": float(M.mean()) * H,
           "lds_bytes": int(lib.mvosr_height_pitch_lds_bytes(N, H)), "note": "staged chain: no selection on the device (lists given), no refinement"}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
