"""GPU: HeightPitchEstimator(triangulation="gpu", resident=True) — the device-resident path — against the unchanged
staged path byte for byte, against the np.longdouble reference of tests/heightpitch_cases.py, and mvosr_height_pitch_tail_batch alone
through the C ABI on the crafted chunks of tests/heightpitch_tail_cases.py.

Every estimator here runs 64 hypotheses on frames of a few hundred features.  The frames with fewer than 12 list points are the crafted
`three` (9 list points under a Delaunay triangulation of its pixels) and `one_row` (3): the resident path triangulates on the device,
so a crafted frame's own rows do not enter, and `rows3` — 9 list points with its own rows — has 24 under Delaunay's.  For the same
reason the singular frame is the crafted `singular` with its repeated point moved to a pixel of its own at depth 0: a triangulation
never names both copies of a pixel in one row, while a point at the camera centre makes every row through it exactly singular."""
import ctypes as C

import numpy as np
import pytest

import heightpitch_cases as hc
import heightpitch_tail_cases as tc

pytestmark = pytest.mark.gpu

H, SEED = 64, 3
FLOATS = ("refined_pitch", "refined_mean", "refined_std", "height_t_mean")


def estimator(resident, chunk=None, **kw):
    from mvoscalerecovery_amd.height_pitch import HeightPitchEstimator
    est = HeightPitchEstimator(max_iterations=H, seed=SEED, triangulation="gpu", resident=resident, **kw)
    if chunk is not None:
        est.GPU_CHUNK = est.GPU_MIN_CHUNK = chunk
    return est


def same_state(a, b):
    assert a.frame_count == b.frame_count
    for x, y in zip(a.result_arrays(), b.result_arrays()):
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (x, y)
    assert (a._prev is None) == (b._prev is None)
    if a._prev is not None:
        assert a._prev[0] == b._prev[0] and a._prev[1].dtype == b._prev[1].dtype and np.array_equal(a._prev[1], b._prev[1])


@pytest.fixture(scope="module")
def golden():
    return hc.load_golden()["seq"]


@pytest.fixture(scope="module")
def staged(golden):
    """The staged path's run of the 12 golden frames, computed once."""
    est = estimator(False)
    out = est.process_batch(golden["frames"], golden["priors"])
    return est, out


def singular_frame():
    s = hc.crafted()["singular"]
    pts = s.pts.copy()
    pts[18] = [pts[0, 0] + 3.0, pts[0, 1] + 2.0, 0.0]
    return pts, s.est


# ---- 1. the staged path, byte for byte ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one_chunk", "chunks_of_5", "frame_by_frame"])
def test_equals_the_staged_path_bytewise(golden, staged, mode):
    est = estimator(True, 5 if mode == "chunks_of_5" else None)
    if mode == "frame_by_frame":
        out = [est.process(p, e) for p, e in zip(golden["frames"], golden["priors"])]
    else:
        out = est.process_batch(golden["frames"], golden["priors"])
    assert out == staged[1] and not any(r.carried for r in out)
    same_state(est, staged[0])
    assert est.declined_total == 0 and set(est.last) == {"records", "dt_status", "errors"}
    if mode == "chunks_of_5":
        assert [len(s) for s in est.last["dt_status"]] == [5, 5, 2] and est.last["errors"] == [-1, -1, -1]


# ---- 2. the independent oracle --------------------------------------------------------------------------------------------------
def test_against_the_longdouble_reference(golden):
    from scipy.spatial import Delaunay
    from mvoscalerecovery_amd import packing
    est = estimator(True, 5)
    out = est.process_batch(golden["frames"], golden["priors"])
    for i, (pts, prior, r) in enumerate(zip(golden["frames"], golden["priors"], out)):
        rows = packing.canonical_rows(Delaunay(pts[:, 0:2]).simplices)
        M = hc.reference(pts, rows, float(prior), np.zeros((1, 3), np.int32))["n_selected"]
        ref = hc.reference(pts, rows, float(prior), hc.draw_positions(SEED, i, H, M))
        assert ref["decided"] and ref["status"] == 0, i
        assert (r.n_selected, r.n_inliers, r.carried) == (ref["n_selected"], ref["n_inliers"], False), i
        print("frame %d: ransac_height off by %.3e (allowed %.3e)" % (i, abs(r.ransac_height - ref["ransac_height"]) / abs(ref["ransac_height"]),
                                                                       ref["ransac_height_tol"]))
        assert abs(r.ransac_height - ref["ransac_height"]) <= ref["ransac_height_tol"] * abs(ref["ransac_height"]), i
        for k in FLOATS:
            print("frame %d: %s off by %.3e (allowed %.3e)" % (i, k, abs(getattr(r, k) - ref[k]), ref[k + "_tol"]))
            assert abs(getattr(r, k) - ref[k]) <= ref[k + "_tol"], (i, k, getattr(r, k), ref[k], ref[k + "_tol"])


# ---- 3. the carry ---------------------------------------------------------------------------------------------------------------
def test_carry_across_chunks_calls_and_paths(golden, tmp_path):
    from mvoscalerecovery_amd import height_pitch as hp
    c = hc.crafted()
    fit = [(golden["frames"][i], float(golden["priors"][i])) for i in range(4)]
    few = [(c["three"].pts, 0.01), (c["one_row"].pts, -0.02), (c["three"].pts, 0.03), (c["one_row"].pts, 0.015)]
    calls = [[fit[0], few[0], few[1], fit[1], few[2]],                               # two carries in a row; a source in the previous chunk;
             [few[3], fit[2]],                                                       # a carried frame first in its chunk; a carried last frame
             [few[0], fit[3], few[1]]]                                               # a second call that starts with a carry; then a staged one
    res, ref = estimator(True, 2), estimator(False)
    for k, call in enumerate(calls):
        pts, ests = [p for p, _ in call], [e for _, e in call]
        want = ref.process_batch(pts, ests)
        if k == 2:
            res.resident = False                                                     # a staged call on the same object
        got = res.process_batch(pts, ests)
        assert got == want and [r.carried for r in got] == [len(p) < 30 for p in pts], k
        assert all(r.n_selected < hp.MIN_POINTS for r in got if r.carried)
        same_state(res, ref)
    for est, d in ((res, tmp_path / "res"), (ref, tmp_path / "ref")):
        d.mkdir()
        est.write_results(str(d))
    for name in hp.RESULT_FILES:
        assert (tmp_path / "res" / name).read_bytes() == (tmp_path / "ref" / name).read_bytes(), name


# ---- 4. the tail alone, through the C ABI ---------------------------------------------------------------------------------------
def run_tail(chunk, carry, cap=None, min_points=tc.MIN_POINTS):
    """mvosr_height_pitch_tail_batch on a hand-made chunk -> (records, error word, carry-out as tc.tail's dict)."""
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd import height_pitch as hp
    ctx = _lib.default_context(0)
    F = len(chunk["status"])
    cnt = np.array([len(x) for x in chunk["v"]], dtype=np.int32)
    even = (cnt.astype(np.int64) + 1) & ~1
    off = np.concatenate([[0], np.cumsum(even)[:-1]]).astype(np.int64)
    total = int(off[-1] + even[-1])
    planes = {k: np.zeros(total, dtype=np.uint8 if k == "mask" else np.float64) for k in ("v", "depth", "mask")}
    for f in range(F):
        for k in planes:
            planes[k][off[f]:off[f] + cnt[f]] = chunk[k][f]
    cap = max(int(cnt.max()), len(carry["y"]), 2) if cap is None else cap
    prev = None
    if carry["has_prev"] or carry["halted"]:
        prev = hp.FrameResult(*[carry[k] for k in hp.RESULT_FIELDS], 0, False)
    rec = hp.carry_record(cap, prev, np.stack([carry["y"] * 0, carry["y"], carry["z"]], 1), carry["index"])
    head = rec[:64].view(hp.CARRY_HEADER)
    head["has_prev"], head["halted"] = carry["has_prev"], carry["halted"]
    spec = [("feat_off", F, np.int64), ("feat_cnt", F, np.int32), ("v", total, np.float64), ("z", total, np.float64), ("prior", (F, 4), np.float64),
            ("mask", total, np.uint8), ("status", F, np.int32), ("n_selected", F, np.int32), ("n_inliers", F, np.int32)] + \
           [(k, F, np.float64) for k in tc.VALUES] + [("carry_in", len(rec), np.uint8)]
    d = ctx.block(spec)
    o = ctx.block([("frames", F, hp.TAIL_FRAME), ("error", 1, np.int64), ("carry_out", len(rec), np.uint8)])
    try:
        d.upload(dict({k: chunk[k] for k in ("status", "n_selected", "n_inliers", "prior") + tc.VALUES}, feat_off=off, feat_cnt=cnt, v=planes["v"],
                      z=planes["depth"], mask=planes["mask"], carry_in=rec))
        o.zero()
        b = _lib.Batch()
        b.n_frames, b.feat_off, b.feat_cnt, b.v, b.z, b.max_feat, b.total_feat = F, d["feat_off"].ptr, d["feat_cnt"].ptr, d["v"].ptr, d["z"].ptr, int(cnt.max()), total
        p = _lib.HeightPitchParams(hc.FOCUS, hc.CX, hc.CY, min_points, H, 0.005, 0.8, 0.01, 0, 0)
        outs = _lib.HeightPitchOutputs()
        for k in ("status", "n_selected", "n_inliers", "mask") + tc.VALUES:
            setattr(outs, k, d[k].ptr)
        _lib.check(ctx.lib.mvosr_height_pitch_tail_batch(ctx.handle, C.byref(b), C.byref(p), d["prior"].ptr, C.byref(outs), d["carry_in"].ptr,
                                                         o["carry_out"].ptr, cap, o["frames"].ptr, o["error"].ptr), "mvosr_height_pitch_tail_batch")
        frames, err, out = o["frames"].download(), int(o["error"].download()[0]), o["carry_out"].download()
    finally:
        d.free()
        o.free()
    h, y, z, index = hp.carry_fields(out, cap)
    return frames, err, dict({k: h[k] for k in ("has_prev", "halted", "n_inliers") + tc.VALUES}, y=y.copy(), z=z.copy(), index=index.copy())


def assert_tail(chunk, carry, cap=None):
    """The kernel's records, error word and carry-out are the restatement's, byte for byte -> the carry-out."""
    frames, err, out = run_tail(chunk, carry, cap)
    recs, error, want = tc.tail(chunk, carry)
    assert err == (-1 if error is None else (error[1] << 32) | error[0]), (err, error)
    for f, r in enumerate(recs or []):
        for k in tc.VALUES:
            assert np.float64(r[k]).tobytes() == frames[k][f].tobytes(), (f, k, r[k], frames[k][f])
        assert (r["n_inliers"], r["n_selected"], r["carried"]) == (frames["n_inliers"][f], frames["n_selected"][f], frames["carried"][f]), f
    assert (out["has_prev"], out["halted"]) == (want["has_prev"], want["halted"])
    if want["has_prev"]:
        for k in tc.VALUES + ("n_inliers",):
            assert np.float64(out[k]).tobytes() == np.float64(want[k]).tobytes(), k
    for k in ("y", "z", "index"):
        assert out[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    return want, recs


def test_tail_sums_in_numpys_order_at_every_count():
    chunk = tc.count_chunk()
    _, recs = assert_tail(chunk, tc.no_carry())
    for j, k in enumerate(tc.COUNTS):                                                # the expected value, spelled out: np.mean on the host
        y, z, _ = tc.inlier_yz(chunk["v"][2 * j], chunk["depth"][2 * j], chunk["mask"][2 * j])
        assert len(y) == k and recs[2 * j + 1]["height_t_mean"] == float(np.mean(z * chunk["prior"][2 * j + 1][2] + y * chunk["prior"][2 * j + 1][3]))
    # the same frames in two chunks, the carry handed on: a carried frame first in its chunk takes the carry-in's inliers
    first = {k: v[:5] for k, v in chunk.items()}
    rest = {k: v[5:] for k, v in chunk.items()}
    carry, _ = assert_tail(first, tc.no_carry(), cap=2048)
    assert carry["has_prev"] and len(carry["y"]) == tc.COUNTS[2]
    _, recs2 = assert_tail(rest, carry, cap=2048)
    assert recs2 == recs[5:]


def test_tail_inlier_placement_and_carry_in():
    rng = np.random.default_rng(5)
    src = tc.chunk_of([tc.crafted_frame(rng, 300, np.sort(rng.choice(300, 129, replace=False)))], rng)
    carry, _ = assert_tail(src, tc.no_carry())
    chunk = tc.placement_chunk()
    out, recs = assert_tail(chunk, carry)
    assert [r["carried"] for r in recs] == [1, 0, 1, 1, 0, 1, 0, 1]
    assert np.array_equal(out["index"], np.nonzero(chunk["mask"][6])[0]) and out["index"][0] == 3 and not np.any((out["index"] >= 64) & (out["index"] < 128))
    y, z, _ = tc.inlier_yz(chunk["v"][6], chunk["depth"][6], chunk["mask"][6])
    assert np.array_equal(out["y"], y) and np.array_equal(out["z"], z)               # the carry-out: the last fitted frame's, compacted


def test_tail_errors_and_halted_carry():
    rng = np.random.default_rng(6)
    fit = lambda: tc.crafted_frame(rng, 90, [2, 63, 64, 89])
    chunk = tc.chunk_of([tc.carried_frame(rng), fit()], rng)
    halted, _ = assert_tail(chunk, tc.no_carry())                                    # a carried frame with no previous
    assert halted["halted"] and not halted["has_prev"]
    assert_tail(chunk, halted)                                                       # ... and every later chunk passes the record on
    for status, n_selected in ((tc.ST_SINGULAR, 0), (tc.ST_MASK, 0), (tc.ST_EMPTY, 0), (tc.ST_RS_FEW, 12), (5, 0)):
        bad = tc.carried_frame(rng)
        bad.update(status=status, n_selected=n_selected)
        out, recs = assert_tail(tc.chunk_of([fit(), tc.carried_frame(rng), bad, fit()], rng), tc.no_carry())
        assert len(recs) == 2 and out["halted"] and out["has_prev"] and len(out["y"]) == 4


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------
def both_raise(exc, pts, ests, chunk=2, triples=None, before=None):
    res, ref = estimator(True, chunk), estimator(False)
    if before is not None:
        for est in (res, ref):
            est.process_batch(*before)
    for est in (ref, res):
        with pytest.raises(exc) as info:
            est.process_batch(pts, ests, triples=triples)
        if est is ref:
            message = str(info.value)
        else:
            assert str(info.value) == message
    same_state(res, ref)
    return res


def test_first_frame_with_too_few_points_raises_indexerror(golden):
    res = both_raise(IndexError, [hc.crafted()["one_row"].pts, golden["frames"][0]], [0.0, float(golden["priors"][0])])
    assert res.frame_count == 0 and res._prev is None and not res.results["n_inliers"]


def test_singular_frame_in_the_second_chunk_raises_linalgerror(golden):
    pts, est = singular_frame()
    c = hc.crafted()
    frames = [golden["frames"][0], c["three"].pts, pts, golden["frames"][1], c["one_row"].pts]
    res = both_raise(np.linalg.LinAlgError, frames, [float(golden["priors"][0]), 0.01, est, float(golden["priors"][1]), 0.02])
    assert res.frame_count == 2 and res._prev[0].carried


def test_two_point_frame_raises_valueerror(golden):
    res = both_raise(ValueError, [golden["frames"][0], golden["frames"][1], golden["frames"][2][:2]], [float(e) for e in golden["priors"][:3]])
    assert res.frame_count == 2 and res.declined_total == 1


def test_spent_samples_raise_valueerror(golden):
    spent = np.full((H, 3), -1, dtype=np.int32)
    res = both_raise(ValueError, [golden["frames"][1]], [float(golden["priors"][1])], triples=[spent],
                     before=([golden["frames"][0]], [float(golden["priors"][0])]))
    assert res.frame_count == 1


# ---- 6. a frame the device triangulation declines -----------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 2])
def test_declined_frame_takes_the_hosts_rows(golden, chunk):
    frames = [f.copy() for f in golden["frames"][:5]]
    frames[2][7, 0:2] = frames[2][3, 0:2]                                            # an exactly repeated pixel
    ests = [float(e) for e in golden["priors"][:5]]
    res, ref = estimator(True, chunk), estimator(False)
    assert res.process_batch(frames, ests) == ref.process_batch(frames, ests)
    same_state(res, ref)
    assert res.declined_total >= 1 and np.concatenate(res.last["dt_status"])[2] != 0
    assert not np.concatenate(res.last["dt_status"])[[0, 1, 3, 4]].any()             # the other four frames' rows never left the device:
    assert "rows" not in res.last and all(isinstance(v, (np.ndarray, list)) and len(v) <= 5 for v in res.last.values())   # self.last carries none


def flat_row_frame():
    """Six pixels on one image row, pixel 4 an exact copy of pixel 1: the repeated pixel makes the device triangulation decline the
    frame, and the host's Qhull then finds every point on one line ("Initial simplex is flat")."""
    pts = np.array([[100.0 + 10 * i, 200.0, 10.0 + i] for i in range(6)])
    pts[4, 0:2] = pts[1, 0:2]
    return pts


@pytest.mark.parametrize("place", [0, 1])
def test_scipy_raises_on_a_declined_frame(golden, staged, place):
    """The declined frame is the first (``place`` 0: no tail runs again) or the second (1: the tail runs again over one frame) of the
    second chunk of two, with two more chunks queued behind it: SciPy's exception leaves the call, and the object is left as the
    staged path is after the frames before the bad one."""
    from scipy.spatial import QhullError
    bad = 2 + place
    frames = [f for f in golden["frames"][:8]]
    frames[bad] = flat_row_frame()
    ests = [float(e) for e in golden["priors"][:8]]
    res, ref = estimator(True, 2), estimator(False)
    assert res.GPU_PIPELINE == 2
    before = res.ctx.alloc_stats()
    with pytest.raises(QhullError):
        res.process_batch(frames, ests)
    after = res.ctx.alloc_stats()
    print("alloc_stats before", before, "after", after, "dt_status", res.last["dt_status"], "errors", res.last["errors"])
    assert res.last["dt_status"][1][place] != 0                                      # the device did decline it (MVOSR_DT_DEGENERATE)
    assert res.declined_total == 1
    assert ref.process_batch(frames[:bad], ests[:bad]) == staged[1][:bad]
    same_state(res, ref)
    assert res.frame_count == bad and len(res.last["records"]) == bad
    # (the counters of alloc_stats only grow; what a call can leave behind is a live block)
    assert after["live_blocks"] == before["live_blocks"]
    more = (golden["frames"][8:10], [float(e) for e in golden["priors"][8:10]])
    assert res.process_batch(*more) == ref.process_batch(*more)
    same_state(res, ref)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(golden):
    from mvoscalerecovery_amd.height_pitch import HeightPitchEstimator
    with pytest.raises(ValueError, match="resident=True"):
        HeightPitchEstimator(triangulation="scipy", resident=True)
    est = estimator(True)
    with pytest.raises(ValueError, match="tris="):
        est.process_batch(golden["frames"][:1], golden["priors"][:1], tris=golden["rows"][:1])
    big = np.random.default_rng(0).uniform(1.0, 300.0, (6000, 3))
    message = None
    for e in (HeightPitchEstimator(max_iterations=H, seed=SEED), est):
        with pytest.raises(ValueError, match="bytes of LDS") as info:
            e.process_batch([golden["frames"][0], big], [0.0, 0.0])
        message = message or str(info.value)
        assert str(info.value) == message                                            # the staged path's message
    assert est.frame_count == 0 and est._prev is None and est.last is None           # ... before anything of the call ran
