"""Launchers, frames and comparators for the rescale variant's large-frame kernels (csrc/mvosr_rescale_large.hip) — shared by
tests/test_rescale_large_cases.py (CPU) and tests/test_gpu_rescale_large.py (device).  Test infrastructure.

The comparator below the resident limit is the resident entry point itself, byte for byte: `run_flat` / `run_keep` launch either
entry point on the same batch into sentinel-filled outputs and return the WHOLE downloaded arrays — guard elements, unwritten rows
and all — so that equality of two runs also says that neither wrote anything the other did not.  Beyond the limit it is
oracle/rescale_oracle.py, compared the way tests/gpu_helpers._check_rescale_device_against_oracle compares (restated in
`check_flat_against_oracle` and `check_estimator_against_oracle`)."""
import ctypes as C

import numpy as np

import flat_cases as fc

FLAT = {"resident": "mvosr_flat_ransac_batch", "large": "mvosr_flat_ransac_large_batch"}
FLAT_FIELDS = ("raw_scale", "height_level", "model", "best_ic", "used", "n_kept", "status", "tri_height", "tri_flags", "hyp_counts")
SENTINEL = 0x5A


def run_flat(ctx, frames, which, n_hyp=100, use_keep=True, id_triples=None, frame_ids=None, seed=5, frame_base=0, max_feat=None,
             max_tri=None, optional=True, height_factor=0.9, dt_status=None):
    """``FLAT[which]`` over `frames` into outputs pre-filled with SENTINEL bytes, one guard element behind each -> (name -> the
    whole downloaded array, row offsets).  optional: tri_height, tri_flags and hyp_counts are requested (else NULL: the large
    kernel then keeps heights and flags in its workspace).  Other arguments as flat_cases.run_dev."""
    from mvoscalerecovery_amd import _lib
    b, d, toff, true_max_tri = fc._batch(ctx, frames, compact=not use_keep)
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    max_tri = true_max_tri if max_tri is None else int(max_tri)
    F, T, H = len(frames), max(int(toff[-1]), 1), int(n_hyp)
    extra = []
    keep_ptr = tr_ptr = ids_ptr = dt_ptr = None
    if use_keep:
        words = np.concatenate([(f.keep if f.keep is not None else np.ones(len(f.xyz), np.int32)) for f in frames]).astype(np.int32)
        extra.append(ctx.to_device(words))
        keep_ptr = extra[-1].ptr
    if id_triples is not None:
        extra.append(ctx.to_device(np.ascontiguousarray(np.stack([np.asarray(t, dtype=np.int32).reshape(H, 3) for t in id_triples]))))
        tr_ptr = extra[-1].ptr
    if frame_ids is not None:
        extra.append(ctx.to_device(np.asarray(frame_ids, dtype=np.int64)))
        ids_ptr = extra[-1].ptr
    if dt_status is not None:
        extra.append(ctx.to_device(np.asarray(dt_status, dtype=np.int32)))
        dt_ptr = extra[-1].ptr
    o = fc._alloc(ctx, {"raw_scale": (F, np.float64), "height_level": (F, np.float64), "model": ((F, 4), np.float64),
                        "best_ic": (F, np.int32), "used": (F, np.int32), "n_kept": (F, np.int32), "status": (F, np.int32),
                        "tri_height": (T, np.float64), "tri_flags": (T, np.uint8), "hyp_counts": ((F, H), np.int32)}, SENTINEL)
    ptrs = [o[k].ptr for k in FLAT_FIELDS[:7]] + [(o[k].ptr if optional else None) for k in FLAT_FIELDS[7:]]
    ro = _lib.RescaleOutputs(*ptrs)
    rp = _lib.RescaleParams(0, 10, fc.LOOSE_DEG, fc.TIGHT_DEG, float(height_factor), fc.MIN_POINTS, H, fc.THRESHOLD, fc.GOAL, fc.ABS_REF,
                            int(seed), int(frame_base))
    _lib.check(getattr(ctx.lib, FLAT[which])(ctx.handle, C.byref(b), keep_ptr, C.byref(rp), tr_ptr, ids_ptr, dt_ptr, C.byref(ro), max_tri),
               FLAT[which])
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + list(d.values()) + extra)
    return r, toff


def same_bytes(a, b, fields=None):
    """Names of the arrays of two `run_flat` / `run_keep` results that differ in any byte."""
    return [k for k in (fields or a) if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]


def keep_batch(ctx, cases, max_feat=None):
    """The cases of flat_cases.graph_cases' form as one resident batch -> (header, device buffers — [6]: dt_status —, feature offsets)."""
    from mvoscalerecovery_amd import _lib
    cnt = np.array([len(c["v"]) for c in cases], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(c["tri"]) for c in cases])]).astype(np.int64)
    rows = np.concatenate([c["tri"].reshape(-1, 3) for c in cases]).astype(np.int32).reshape(-1)
    d = [ctx.to_device(off), ctx.to_device(cnt), ctx.to_device(np.concatenate([c["z"] for c in cases] + [np.zeros(1)])),
         ctx.to_device(np.concatenate([c["v"] for c in cases] + [np.zeros(1)])), ctx.to_device(toff),
         ctx.to_device(np.concatenate([rows, np.zeros(3, np.int32)])),
         ctx.to_device(np.array([7 if c["declined"] else 0 for c in cases], dtype=np.int32))]
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.z, b.v, b.x, b.y = len(cases), d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[2].ptr, d[2].ptr
    b.tri1_off, b.tri1, b.max_feat, b.total_feat = d[4].ptr, d[5].ptr, int(cnt.max() if max_feat is None else max_feat), int(off[-1])
    return b, d, off


def launch_keep(ctx, b, dt_ptr, o, large, tile=0, min_valid=10):
    """One launch of mvosr_graph_keep_batch (large False) or mvosr_graph_keep_large_batch into the buffers o: keep, n_valid, status."""
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.rescale import good_bits
    bits = C.c_uint32(good_bits())
    if large:
        _lib.check(ctx.lib.mvosr_graph_keep_large_batch(ctx.handle, C.byref(b), bits, int(min_valid), dt_ptr, o["keep"].ptr, o["n_valid"].ptr,
                                                        o["status"].ptr, int(tile)), "mvosr_graph_keep_large_batch")
    else:
        _lib.check(ctx.lib.mvosr_graph_keep_batch(ctx.handle, C.byref(b), bits, int(min_valid), dt_ptr, o["keep"].ptr, o["n_valid"].ptr,
                                                  o["status"].ptr), "mvosr_graph_keep_batch")


def run_keep(ctx, cases, large, tile=0, min_valid=10, max_feat=None):
    """mvosr_graph_keep_batch (large False) or mvosr_graph_keep_large_batch with `tile` over the cases of flat_cases.graph_cases'
    form as one batch, into SENTINEL-filled outputs with a guard element each -> the whole arrays keep, n_valid, status."""
    b, d, off = keep_batch(ctx, cases, max_feat)
    N, F = int(off[-1]), len(cases)
    o = fc._alloc(ctx, {"keep": (N, np.int32), "n_valid": (F, np.int32), "status": (F, np.int32)}, SENTINEL)
    launch_keep(ctx, b, d[6].ptr, o, large, tile, min_valid)
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + d)
    return r, off


def graph_case(name, v, z, tri, declined=False):
    return {"name": name, "v": np.asarray(v, np.float64), "z": np.asarray(z, np.float64), "tri": np.asarray(tri, np.int32).reshape(-1, 3),
            "declined": declined}


def graph_cases():
    """flat_cases.graph_cases() and, behind them: a row with an id out of range among good rows, a frame without rows, a frame
    without features, and a ~300-feature Delaunay frame (the tile sweep's)."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(195)
    cases = fc.graph_cases()
    uv = rng.uniform(0, 100, (60, 2))
    tri = Delaunay(uv).simplices
    cases.append(graph_case("bad_id", uv[:, 1], rng.uniform(1, 50, 60), np.concatenate([tri, [[0, 1, 60], [-1, 2, 3]]])))
    cases.append(graph_case("no_rows", uv[:20, 1], rng.uniform(1, 50, 20), np.zeros((0, 3))))
    cases.append(graph_case("no_features", np.zeros(0), np.zeros(0), np.zeros((0, 3))))
    cases.append(delaunay_graph_case("delaunay300", 300, 196))
    return cases


def delaunay_graph_case(name, n, seed):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0, 1000, (n, 2))
    return graph_case(name, uv[:, 1], 2000.0 / (uv[:, 1] + 50.0) + rng.normal(0, 0.4, n), Delaunay(uv).simplices)


def keep_oracle(case, min_valid=10):
    """The keep words of oracle.rescale_oracle.graph_inliers: 1 passed, else -1 where more than min_valid passed, else 0."""
    from oracle import rescale_oracle as ro
    valid = ro.graph_inliers(case["v"], case["z"], case["tri"])[0]
    nv = int(valid.sum())
    return np.where(valid, 1, -1 if nv > min_valid else 0).astype(np.int32), nv


def flat_frames():
    """name -> Frame: every crafted family of flat_cases (select, thresholds, tail — the tail's sized by `max_points` at the call)
    is added by the tests; here the extra refusals: no rows, every feature dropped, fewer than 12 list entries."""
    rng = np.random.default_rng(7)
    fam = {}
    base = fc.disjoint("x", [(h, 0.0, 1) for h in rng.uniform(1.5, 1.9, 9)], 81)
    fam["no_rows"] = fc.Frame("no_rows", base.xyz, np.zeros((0, 3), np.int32), note="MVOSR_ST_ERR_EMPTY")
    fam["all_dropped"] = fc.Frame("all_dropped", base.xyz, base.tri, keep=np.full(len(base.xyz), -1, np.int32), status=fc.ST_MASK,
                                  note="no survivor: every row names a vertex out of range")
    fam["too_few"] = fc.disjoint("too_few", [(1.7, 0.0, 1), (1.71, 0.0, 1), (1.72, 0.0, 1)], 82, note="9 list entries: MVOSR_ST_RS_FEW")
    return fam


def big_grid(nx=110, nz=110):
    """An all-road jittered grid (flat_cases.grid_frame): 2 (nx - 1)(nz - 1) rows, nearly every one kept — at 110 x 110 that is
    23 762 rows (> MVOSR_GRAPH_MAX_ROWS = 21 845) and a point list of 70 935 entries (> 65 535)."""
    return fc.grid_frame("big_grid", nx=nx, nz=nz, seed=151, n_out=40)


def oracle_flat(frame, seed, frame_counter, n_hyp=100):
    """oracle.rescale_oracle on a Frame's survivors and rows with the device's sample sequence -> dict (status 0 / 11)."""
    from oracle import rescale_oracle as ro
    P = frame.survivors()
    fs = ro.flat_selection(P, frame.tri)
    out = {"ids": fs.ids, "level": fs.height_level, "heights": fs.heights, "kept": fs.tri_valid, "status": 11, "M": len(fs.ids)}
    if len(fs.ids) >= fc.MIN_POINTS:
        triples = ro.device_triples(seed, frame_counter, fs.ids, n_hyp)
        m, ic, used = ro.run_ransac(P[fs.ids], triples, repeated_counts_zero=True)
        if m is not None:
            out.update(status=0, model=np.array(m), best_ic=ic, used=used, scale=ro.scale_from_model(m, fc.ABS_REF))
    return out


def check_flat_against_oracle(r, toff, i, frame, want):
    """Frame i of a `run_flat` result against `oracle_flat`: the point list, the inlier count and the consumed hypotheses exact;
    heights, level, plane and scale to 1e-9 / the plane as gpu_helpers compares it (rtol 1e-7, atol 1e-11)."""
    fl = r["tri_flags"][toff[i]:toff[i + 1]]
    ids = frame.tri[(fl & 4) != 0].reshape(-1)
    assert np.array_equal(ids, want["ids"]), "point list"
    assert int(r["n_kept"][i]) * 3 == want["M"]
    np.testing.assert_allclose(r["tri_height"][toff[i]:toff[i + 1]], want["heights"], rtol=1e-9)
    np.testing.assert_allclose(r["height_level"][i], want["level"], rtol=1e-9)
    assert int(r["status"][i]) == want["status"]
    if want["status"] == 0:
        m_ref = want["model"] if want["model"][1] >= 0 else -want["model"]
        np.testing.assert_allclose(r["model"][i], m_ref, rtol=1e-7, atol=1e-11)
        assert int(r["best_ic"][i]) == want["best_ic"] and int(r["used"][i]) == want["used"]
        assert abs(r["raw_scale"][i] - want["scale"]) <= 1e-9 * abs(want["scale"])


def oracle_estimator_run(frames, window, seed):
    """OracleRescaleEstimator(device_seed=seed) over (feature3d, feature2d) frames -> (scales, per-frame snapshots, the oracle)."""
    from oracle import rescale_oracle as ro
    ref = ro.OracleRescaleEstimator(fc.ABS_REF, window_size=window, device_seed=seed)
    want, snap = [], []
    for f3, f2 in frames:
        want.append(ref.scale_calculation(f3, f2)[0])
        snap.append(dict(valid=ref.last["valid"].copy(), ids=ref.last["flat"].ids.copy(), level=ref.last["flat"].height_level,
                         model=None if "model" not in ref.last else np.array(ref.last["model"]),
                         best_ic=ref.last.get("best_ic"), used=ref.last.get("used")))
    return want, snap, ref


def check_estimator_against_oracle(est, frames, want, snap, ref):
    """gpu_helpers._check_rescale_device_against_oracle, batch form, restated: masks, point lists, inlier counts and consumed
    hypotheses exact; level and scales to 1e-9, the plane to rtol 1e-7 / atol 1e-11."""
    got, _ = est.scale_calculation_batch([f[0] for f in frames], [f[1] for f in frames], stage=True)
    L = est.last
    for j, (w, sn) in enumerate(zip(want, snap)):
        assert np.array_equal(L["valid"][j], sn["valid"]), j
        ids = L["tris2"][j][(L["tri_flags"][j] & 4) != 0].reshape(-1)
        assert np.array_equal(ids, sn["ids"]), j
        np.testing.assert_allclose(L["height_level"][j], sn["level"], rtol=1e-9)
        if sn["model"] is not None:
            assert int(L["status"][j]) == 0
            m_ref = sn["model"] if sn["model"][1] >= 0 else -sn["model"]
            np.testing.assert_allclose(L["model"][j], m_ref, rtol=1e-7, atol=1e-11)
            assert int(L["best_ic"][j]) == sn["best_ic"] and int(L["used"][j]) == sn["used"], j
        else:
            assert int(L["status"][j]) == 11
        assert abs(got[j] - w) <= 1e-9 * abs(w), (j, got[j], w)
    np.testing.assert_allclose(list(est.scale_queue), list(ref.scale_queue), rtol=1e-9)
