"""-m gpu: flat_static_tri_kernel (mvosr_flat_static_tri_batch) and ``rescale.ScaleEstimator(model="static_tri",
model_resident=True)``.

The oracle is never the kernel under test: the given form is compared with the reference's own run (tests/golden/statictri.npz), the
fused form with the composition of the two entry points it stands in for on the same resident batch
(tests/static_resident_cases.py), the estimator with the reference's 60-frame sequence and with the staged estimator.  Every
comparison is by bytes (NaN to NaN).
"""
from __future__ import annotations

import numpy as np
import pytest

import flat_cases as fc
import static_resident_cases as sr
import statictri_cases as stc
from gpu_helpers import _check_error_mid_call_is_released, _declining, _rescale_frames

pytestmark = pytest.mark.gpu

ST_MODE, ST_MEDIAN, ST_RS_FEW = stc.ST_MODE, stc.ST_MEDIAN, stc.ST_RS_FEW


@pytest.fixture(scope="module")
def golden():
    return stc.golden()


@pytest.fixture(scope="module")
def crafted():
    c = stc.crafted()
    z = stc.golden()
    assert list(z["c_names"]) == list(c) and int(z["c_crc"]) == stc.checksum(list(c.values()))
    return c


@pytest.fixture(scope="module")
def random_lists():
    lists = stc.random_lists()
    assert int(stc.golden()["r_crc"]) == stc.checksum(lists)
    return lists


@pytest.fixture(scope="module")
def frames():
    fr = stc.sequence_frames()
    from mvoscalerecovery_amd import synth
    assert int(stc.golden()["s_crc"]) == synth.checksum(*[a for f in fr for a in f])
    return fr


@pytest.fixture(scope="module")
def staged_sequence(frames):
    """The staged estimator over the 60 frames: the scales, and the height level after every frame (computed once, shared)."""
    est = _estimator(model="static_tri")
    s, _ = est.scale_calculation_batch([a.copy() for a, _ in frames], [b.copy() for _, b in frames])
    return {"scales": s, "height_level": np.array(est.last["height_level"], dtype=np.float64), "final_level": est.height_level}


def _want(z, pre, i, h, min_count=0):
    """The reference's result for list i of the golden's family ``pre``, as the launch writes it."""
    if len(h) == 0 or len(h) <= min_count:
        return stc.static_tri_of(h, min_count=min_count)
    return {"scale_norm": z[pre + "_scale"][i], "raw_scale": np.float64(z[pre + "_scale"][i]) * np.float64(stc.ABS_REF),
            "status": int(z[pre + "_status"][i]), "n_used": len(h), "hist": z[pre + "_hist"][i]}


def _estimator(**kw):
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    kw.setdefault("delaunay_workers", 1)
    return ScaleEstimator(stc.ABS_REF, window_size=stc.WINDOW, **kw)


def _resident(chunk=None, **kw):
    est = _estimator(model="static_tri", model_resident=True, **kw)
    if chunk:
        est.GPU_CHUNK, est.GPU_MIN_CHUNK, est.GPU_RAMP = chunk, 1, False
    return est


# ---- 1. the given form against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [0, 12])
def test_given_form_crafted_lists_equal_the_reference(gpu, golden, crafted, min_count):
    lists = list(crafted.values())
    batch, guards = sr.run_given(gpu, lists, min_count=min_count, sentinel=0xA5)
    alone = sr.run_given(gpu, lists, min_count=min_count, alone=True)
    for i, (name, h) in enumerate(crafted.items()):
        want = _want(golden, "c", i, h, min_count)
        assert stc.same(batch[i], want), (name, batch[i], want)
        assert stc.same(alone[i], want), (name, alone[i], want)
    assert all(fc.all_bytes(g, 0xA5) for g in guards.values())                                # nothing behind the last list is written
    st = {name: batch[i]["status"] for i, name in enumerate(crafted)}
    assert st["empty"] == ST_RS_FEW and st["max2"] == ST_MEDIAN and st["max3"] == ST_MODE
    assert st["n12"] == (ST_RS_FEW if min_count else ST_MODE) and st["n13"] == ST_MODE


@pytest.mark.parametrize("min_count", [0, 12])
def test_given_form_random_lists_equal_the_reference(gpu, golden, random_lists, min_count):
    batch = sr.run_given(gpu, random_lists, min_count=min_count)
    alone = sr.run_given(gpu, random_lists, min_count=min_count, alone=True)
    for got in (batch, alone):
        bad = [i for i, h in enumerate(random_lists) if not stc.same(got[i], _want(golden, "r", i, h, min_count))]
        assert not bad, (bad[:10], got[bad[0]])
    st = np.array([g["status"] for g in batch])
    assert (st == ST_MEDIAN).sum() >= 20 and (st == ST_MODE).sum() >= 20


def test_given_form_refuses_invalid_heights_and_not_their_neighbours(gpu, crafted):
    bad = stc.refused()
    good = crafted["plateau2"]
    lists = [x for h in bad.values() for x in (h, good)]
    got = sr.run_given(gpu, lists, min_count=12)
    for i, name in enumerate(bad):
        r = got[2 * i]
        assert r["status"] == stc.ST_ERR_MASK and np.isnan(r["scale_norm"]) and np.isnan(r["raw_scale"]) and not r["hist"].any(), name
        assert r["n_used"] == len(bad[name])
        assert stc.same(got[2 * i + 1], stc.static_tri_of(good, min_count=12)) and got[2 * i + 1]["scale_norm"] == 0.45
    # rows that do not count (bit 0 clear) carry garbage and are not looked at
    rng = np.random.default_rng(5)
    h = np.concatenate([good, rng.choice([np.nan, -1.0, 0.0, np.inf], 17)])
    fl = np.concatenate([np.ones(len(good), np.uint8), np.zeros(17, np.uint8)])
    perm = rng.permutation(len(h))
    got = sr.run_given(gpu, [h[perm]], min_count=12, flags=[fl[perm]])[0]
    assert stc.same(got, stc.static_tri_of(good, min_count=12))
    # a frame without rows is the flat stage's refusal, whatever the model would say of an empty list
    none, ok = sr.run_given(gpu, [np.zeros(0), good], min_count=0, pad_empty=False)
    assert none["status"] == fc.ST_EMPTY and np.isnan(none["scale_norm"]) and np.isnan(none["raw_scale"]) and none["n_used"] == 0
    assert not none["hist"].any() and np.isnan(none["height_level"]) and none["n_kept"] == 0
    assert stc.same(ok, stc.static_tri_of(good))


def test_given_form_forty_thousand_entries_on_either_exit(gpu):
    rng = np.random.default_rng(40000)
    median = stc.from_counts(stc._counts(b2=2, b7=2, b11=2, b15=1), 71, tail=list(rng.uniform(1.95, 60.0, 39993)))
    median_low = np.concatenate([stc.from_counts(stc._counts(b2=2, b7=2), 72, tail=list(rng.uniform(1.95, 60.0, 19995))),
                                 stc.heights_of([stc.reachable(2.75, 3.0)[1]] * 20001)])      # an even count, the middle pair equal
    mode = np.float64(1.0) / np.abs(rng.normal(0.62, 0.11, 40000))
    assert len(median) == 40000 and len(median_low) == 40000
    want = [stc.static_tri_of(h, min_count=12) for h in (median, median_low, mode)]
    assert [w["status"] for w in want] == [ST_MEDIAN, ST_MEDIAN, ST_MODE] and want[0]["scale_norm"] > 1.9
    got = sr.run_given(gpu, [median, median_low, mode], min_count=12)
    assert all(stc.same(g, w) for g, w in zip(got, want)), (got, want)


# ---- 2. the fused form against the composition ------------------------------------------------------------------------------------
def _count_exits(tally, composed):
    for c in composed:
        st = int(c["status"])
        tally["mode"] += st == ST_MODE
        tally["median"] += st == ST_MEDIAN
        tally["few"] += st == ST_RS_FEW and int(c["n_used"]) > 0
        tally["empty_loose"] += st == ST_RS_FEW and int(c["n_used"]) == 0
    return tally


def test_fused_form_equals_the_composition_on_crafted_frames(gpu):
    tally = {"mode": 0, "median": 0, "few": 0, "empty_loose": 0}
    fam = dict(fc.select_families())
    fam.update(sr.model_frames())
    names = list(fam)
    for use_keep in (False, True):
        frames = [fam[n] if not use_keep else fam[n].with_keep(900 + i, 7 + 3 * i) for i, n in enumerate(names)]
        fused, composed = sr.run_pair(gpu, frames, use_keep=use_keep)
        assert not sr.differing(fused, composed), [(names[i], k) for i, k in sr.differing(fused, composed)]
        _count_exits(tally, composed)
        for n, c in zip(names, composed):
            assert int(c["status"]) == (fam[n].status or int(c["status"])), n                 # the flat stage's errors where the frames have them
    # the oracle's own statuses: every exit of the model is reached
    assert tally["mode"] >= 3 and tally["median"] >= 3 and tally["few"] >= 3 and tally["empty_loose"] >= 1, tally
    by = dict(zip(names, composed))
    assert int(by["loose12"]["status"]) == ST_RS_FEW and int(by["loose12"]["n_used"]) == 12
    assert int(by["loose13_cluster"]["status"]) == ST_MODE and int(by["loose13_spread"]["status"]) == ST_MEDIAN
    assert int(by["loose14_spread"]["status"]) == ST_MEDIAN and int(by["loose0"]["n_used"]) == 0
    assert int(by["singular"]["status"]) == fc.ST_SINGULAR and int(by["bad_ids"]["status"]) == fc.ST_MASK
    thr, _ = sr.run_pair(gpu, [fc.threshold_frame()], use_keep=False, min_count=0)
    thr12, thr12_c = sr.run_pair(gpu, [fc.threshold_frame()], use_keep=False)
    assert not sr.differing(thr12, thr12_c) and sr.frame_bytes(thr[0], sr.ROW_FIELDS) == sr.frame_bytes(thr12[0], sr.ROW_FIELDS)


def test_fused_form_equals_the_composition_on_row_counts_and_large_frames(gpu):
    rows = sr.row_count_frames()
    for use_keep in (False, True):
        fused, composed = sr.run_pair(gpu, list(rows.values()), use_keep=use_keep)
        assert not sr.differing(fused, composed), [(list(rows)[i], k) for i, k in sr.differing(fused, composed)]
        assert all(int(c["status"]) in (ST_MODE, ST_MEDIAN, ST_RS_FEW) for c in composed)
    tails = fc.tail_families(fc.max_points(gpu))
    assert len(tails["at_max_points"].xyz) == fc.max_points(gpu)
    for name, f in tails.items():                                                             # (one launch each: their sizes do not share a header)
        fused, composed = sr.run_pair(gpu, [f], use_keep=f.keep is not None)
        assert not sr.differing(fused, composed), (name, sr.differing(fused, composed))
        assert int(composed[0]["status"]) in (ST_MODE, ST_MEDIAN, ST_RS_FEW), name


def test_fused_form_equals_the_composition_on_a_resident_batch(gpu):
    """16 synthetic frames of 300 to 2000 features through the device path's own front — both triangulations and the vote's keep
    words from mvosr_graph_keep_batch, rows with explicit counts —, then both sides on that DeviceBatch, with keep and without."""
    from mvoscalerecovery_amd import stream
    rng = np.random.default_rng(16)
    sizes = [300, 2000] + [int(n) for n in rng.integers(300, 2001, 14)]
    fr = _rescale_frames(sizes, base_seed=1616)
    est = _estimator(ransac_seed=1)
    ctx = est.ctx
    st = est._chunk_dev_front([f[0] for f in fr], [f[1] for f in fr], 0)
    assert st["gpu"]
    try:
        pf, db = st["pf"], st["db"]
        b = db.struct()
        F, T, max_tri = pf.n_frames, 2 * int(pf.total_padded), 2 * int(db.max_feat)
        assert b.tri2_cnt is not None
        got = {}
        for keep in (True, False):
            keep_ptr = db.bufs["vote_counters"].ptr if keep else None
            rc = sr.launch_composition(ctx, b, keep_ptr, db.bufs["dt2_status"].ptr, F, T, max_tri, sentinel=0x5A)
            rf = sr.launch_fused(ctx, b, keep_ptr, db.bufs["dt2_status"].ptr, F, T, max_tri, sentinel=0x5A)
            for k in rf:                                                                      # whole arrays: gaps between the frames' rows and guards included
                assert rf[k].tobytes() == rc[k].tobytes(), (keep, k)
            got[keep] = rf
        assert np.isin(got[True]["status"][:F], (ST_MODE, ST_MEDIAN)).sum() >= 12 and (got[True]["n_used"][:F] > 12).sum() >= 12
        assert got[True]["tri_height"].tobytes() != got[False]["tri_height"].tobytes()       # (the keep words were read)
    finally:
        stream.free_blocks(st)


# ---- 3. refusals and their neighbours -----------------------------------------------------------------------------------------------
def test_refused_frames_and_their_neighbours(gpu):
    fam = fc.select_families()
    good = [fam["control"], sr.model_frames()["loose13_spread"], fam["k64"], sr.model_frames()["loose40_cluster"], fam["even_b"], fam["k3"]]
    big_feat = fc.disjoint("big_feat", [(1.6 + 0.001 * i, 0.0, int(i < 100)) for i in range(750)], 5, near=True)   # 2250 features, 100 rows
    big_tri = fc.disjoint("big_tri", [(1.6 + 0.01 * i, 0.0, 100) for i in range(22)], 6, near=True)             # 66 features, 2200 rows
    declined = fam["cluster200"]
    frames = [good[0], big_feat, good[1], big_tri, good[2], declined, good[3], fam["bad_ids"], good[4], fam["singular"], good[5]]
    max_feat = max(len(f.xyz) for f in frames if f is not big_feat)
    max_tri = max(len(f.tri) for f in frames if f is not big_tri)
    assert len(big_feat.xyz) > max_feat and len(big_tri.tri) > max_tri and len(big_feat.tri) <= max_tri and len(big_tri.xyz) <= max_feat
    dt = np.zeros(len(frames), np.int32)
    dt[5] = 3
    fused, composed, rf, rc = sr.run_pair(gpu, frames, use_keep=False, max_feat=max_feat, max_tri=max_tri, sentinel=0xA5, dt_status=dt)
    assert [int(f["status"]) for f in fused][1::2] == [fc.ST_MASK, fc.ST_MASK, fc.ST_EMPTY, fc.ST_MASK, fc.ST_SINGULAR]
    for i in (1, 3, 5, 7, 9):                                      # every refusal and error: no scale, no count, a zero histogram
        f = fused[i]
        assert np.isnan(f["scale_norm"]) and np.isnan(f["raw_scale"]) and int(f["n_used"]) == 0 and not f["hist"].any(), i
    for i in (1, 3, 5):                                            # refused before LDS is touched: the per-row outputs are not written
        f = fused[i]
        assert np.isnan(f["height_level"]) and int(f["n_kept"]) == 0, i
        assert fc.all_bytes(f["tri_height"], 0xA5) and fc.all_bytes(f["tri_flags"], 0xA5), i
    for i in (7, 9):                                               # an error inside the frame: the flat stage's outputs are written
        assert not fc.all_bytes(fused[i]["tri_flags"], 0xA5) and np.isfinite(fused[i]["height_level"]), i
    for k in rf:                                                   # ... all of it as the composition leaves it, guards included
        assert rf[k].tobytes() == rc[k].tobytes(), k
    F, T = len(frames), sum(len(f.tri) for f in frames)
    assert all(fc.all_bytes(rf[k][(T if k in sr.ROW_FIELDS else F):], 0xA5) for k in rf)
    # the good frames' bytes are those of a batch without the refused ones
    alone, _ = sr.run_pair(gpu, good, use_keep=False)
    assert [sr.frame_bytes(fused[i]) for i in range(0, len(frames), 2)] == [sr.frame_bytes(a) for a in alone]
    assert {int(a["status"]) for a in alone} == {ST_MODE, ST_MEDIAN, ST_RS_FEW}


def test_launcher_arguments(gpu):
    import ctypes as C
    from mvoscalerecovery_amd import _lib
    lib, h = gpu.lib, gpu.handle
    d = gpu.zeros(64, np.float64)
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.tri2_off, b.tri2, b.x, b.y, b.z, b.max_feat = 1, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, 8
    o = _lib.StaticTriOutputs(d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, None, None, None)
    call = lambda ctx=h, bb=b, oo=o, mc=12, hin=None, fin=None: lib.mvosr_flat_static_tri_batch(
        ctx, C.byref(bb) if bb is not None else None, None, -80.0, -85.0, 0.9, mc, 1.75, None, hin, fin, C.byref(oo) if oo is not None else None, 0)
    empty = _lib.Batch.from_buffer_copy(b)
    empty.n_frames = 0
    assert call(bb=empty) == 0                                       # nothing launched
    empty.n_frames = -4
    assert call(bb=empty) == 0
    assert call(ctx=None) == -2 and call(bb=None) == -2 and call(oo=None) == -2 and call(mc=-1) == -2
    assert call(hin=d.ptr) == -2 and call(fin=d.ptr) == -2           # one of the two given arrays alone
    for hole in ("scale_norm", "raw_scale", "height_level", "n_used", "n_kept", "status"):
        oo = _lib.StaticTriOutputs(d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, None, None, None)
        setattr(oo, hole, None)
        assert call(oo=oo) == -2, hole
    cap = fc.max_points(gpu)
    assert 0 < lib.mvosr_flat_static_tri_lds_bytes(cap, 2 * cap) <= gpu.lds_per_block
    assert lib.mvosr_flat_static_tri_lds_bytes(cap, 0) == lib.mvosr_flat_static_tri_lds_bytes(cap, 2 * cap)
    assert lib.mvosr_flat_static_tri_lds_bytes(0, 0) < lib.mvosr_flat_static_tri_lds_bytes(400, 800) < lib.mvosr_flat_static_tri_lds_bytes(401, 803)
    big = _lib.Batch.from_buffer_copy(b)
    big.max_feat = 20000                                             # beyond one workgroup's LDS: refused by its byte count, nothing launched
    with pytest.raises(_lib.MvosrLibraryError):
        _lib.check(call(bb=big), "mvosr_flat_static_tri_batch")
    d.free()


# ---- 4. the sequence ----------------------------------------------------------------------------------------------------------------
def _check_sequence(est, s, zeros, golden, staged_sequence):
    n = golden["s_n_heights"]
    assert s.tobytes() == golden["s_tri"].tobytes() and not np.asarray(zeros).any() and len(zeros) == len(s)
    assert np.array_equal(est.last["n_used"], n)
    assert np.array_equal(est.last["status"] == ST_RS_FEW, n <= 12) and (n <= 12).sum() >= 3
    assert np.isin(est.last["status"], (ST_MODE, ST_MEDIAN, ST_RS_FEW)).all()
    assert len(est.scale_queue) == 0 and est.scale == golden["s_tri"][-1]
    assert np.asarray(est.last["height_level"]).tobytes() == staged_sequence["height_level"].tobytes()
    assert np.float64(est.height_level).tobytes() == np.float64(staged_sequence["final_level"]).tobytes()
    assert sorted(est.last) == ["height_level", "n_kept", "n_used", "raw_scale", "scale_norm", "status"]
    assert est.last["raw_scale"].tobytes() == (est.last["scale_norm"] * np.float64(stc.ABS_REF)).tobytes()


@pytest.mark.parametrize("kw", [{"triangulation": "gpu"}, {"triangulation": "scipy", "sampling": "device"}], ids=["gpu", "scipy"])
def test_resident_static_tri_reproduces_the_sequence(gpu, golden, frames, staged_sequence, kw):
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    est = _resident(**kw)
    assert (est.triangulation, est.sampling, est.model) == (kw["triangulation"], "device", "static_tri")
    s, zeros = est.scale_calculation_batch([a.copy() for a in f3s], [a.copy() for a in f2s])
    _check_sequence(est, s, zeros, golden, staged_sequence)
    chunked = _resident(chunk=16, **kw)                              # four chunks, a pipeline
    s, zeros = chunked.scale_calculation_batch(f3s, f2s)
    _check_sequence(chunked, s, zeros, golden, staged_sequence)
    one = _resident(**kw)                                            # frame by frame
    got = [one.scale_calculation(a.copy(), b.copy()) for a, b in frames]
    assert np.array([g[0] for g in got], dtype=np.float64).tobytes() == golden["s_tri"].tobytes() and all(g[1] == 0 for g in got)
    assert len(one.scale_queue) == 0 and one.scale == golden["s_tri"][-1]
    assert np.float64(one.height_level).tobytes() == np.float64(staged_sequence["final_level"]).tobytes()
    with pytest.raises(ValueError, match="id_triples"):
        one.scale_calculation_batch(f3s[:2], f2s[:2], id_triples=[np.zeros((100, 3), np.int32)] * 2)


def test_resident_static_tri_stage_outputs(gpu, frames):
    sub = frames[:6]
    est = _resident()
    ref = _estimator(ransac_seed=3)
    est.scale_calculation_batch([a for a, _ in sub], [b for _, b in sub], stage=True)
    ref.scale_calculation_batch([a for a, _ in sub], [b for _, b in sub], stage=True)
    for k in ("valid", "tris2", "tri_flags"):                        # as on the RANSAC path: the same stages in front of the model
        assert len(est.last[k]) == len(sub) and all(np.array_equal(a, b) for a, b in zip(est.last[k], ref.last[k])), k
    assert np.array_equal(est.last["n_kept"], ref.last["n_kept"]) and est.last["height_level"].tobytes() == ref.last["height_level"].tobytes()
    assert [int(((f & 1) != 0).sum()) for f in est.last["tri_flags"]] == est.last["n_used"].tolist()


# ---- 5. declined frames -------------------------------------------------------------------------------------------------------------
def test_declined_frames_rerun_on_the_hosts_triangulations(gpu):
    base = _rescale_frames([150 + (i * 29) % 201 for i in range(200)], base_seed=91)
    at = [5, 63, 64, 197]                                            # the first chunk, both sides of a chunk boundary, the last chunk
    fr = _declining(base, at)
    f3s, f2s = [f[0] for f in fr], [f[1] for f in fr]
    staged = _estimator(model="static_tri", delaunay_workers=2)
    want, wz = staged.scale_calculation_batch(f3s, f2s)
    est = _resident(chunk=64, delaunay_workers=2)
    got, gz = est.scale_calculation_batch(f3s, f2s)
    assert got.tobytes() == want.tobytes() and gz.tobytes() == wz.tobytes()
    assert est.last_declined == len(at)
    for k in ("raw_scale", "scale_norm", "n_used", "status", "height_level"):
        assert np.asarray(est.last[k]).tobytes() == np.asarray(staged.last[k]).astype(np.asarray(est.last[k]).dtype).tobytes(), k
    assert est.scale == staged.scale and np.float64(est.height_level).tobytes() == np.float64(staged.height_level).tobytes()
    assert len(est.scale_queue) == 0


# ---- 6. the two halves ------------------------------------------------------------------------------------------------------------
def test_halves_compose_to_the_whole_run(gpu, golden, frames):
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    whole = _resident()
    s, z = whole.scale_calculation_batch(f3s, f2s)
    worker = _resident()
    a = worker.raw_scale_batch(f3s[:27], f2s[:27], frame_base=0)
    b = worker.raw_scale_batch(f3s[27:], f2s[27:], frame_base=27)
    assert worker.scale == 1 and worker.height_level is None and worker._frame_counter == 0          # no cross-frame state touched
    raw, status, level = (np.concatenate([a[i], b[i]]) for i in range(3))
    assert raw.tobytes() == whole.last["raw_scale"].tobytes() and np.array_equal(status, whole.last["status"])
    assert a[3] == {} and b[3] == {}
    tail = _resident()
    s2, z2 = tail.push_raw_scales(raw, status, level, {})
    assert s2.tobytes() == s.tobytes() == golden["s_tri"].tobytes() and z2.tobytes() == z.tobytes()
    assert tail.scale == whole.scale and len(tail.scale_queue) == 0 == len(whole.scale_queue)
    assert np.float64(tail.height_level).tobytes() == np.float64(whole.height_level).tobytes()
    assert tail._frame_counter == whole._frame_counter == len(frames)


# ---- 7. an error in the middle of a call -------------------------------------------------------------------------------------------
def _singular_at(frames, f, est):
    """``frames`` with frame ``f`` made singular: two survivors that share a row of the second triangulation moved onto the z axis
    (their x and y zeroed: with the third vertex the row's matrix has an exactly zero pivot; z and the pixels stay, so both
    triangulations and the vote — which read the pixels and z only — do not move)."""
    f3, f2 = frames[f][0].copy(), frames[f][1]
    est.scale_calculation_batch([f3], [f2], stage=True)
    valid, row = est.last["valid"][0], est.last["tris2"][0][0]
    lower = np.nonzero(f2[:, 1] > 185)[0]
    surv = lower[valid] if int(valid.sum()) > 10 else lower
    f3[surv[row[0]], :2] = 0.0
    f3[surv[row[1]], :2] = 0.0
    out = list(frames)
    out[f] = (f3, f2)
    return out


def test_singular_frame_mid_call(gpu, golden, frames, staged_sequence):
    fr = _singular_at(frames[:40], 25, _resident())
    f3s, f2s = [f[0] for f in fr], [f[1] for f in fr]
    with pytest.raises(np.linalg.LinAlgError):                       # (the precondition: the staged estimator raises at that frame)
        _estimator(model="static_tri").scale_calculation_batch(f3s[25:26], f2s[25:26])
    est = _resident(chunk=8)
    est.scale_calculation_batch(f3s[:3], f2s[:3])                    # (the estimator's blocks and caches exist from here on)
    fresh = _resident(chunk=8)
    fresh.scale_calculation_batch(f3s[:3], f2s[:3])
    before = est.ctx.alloc_stats()["live_blocks"]
    with pytest.raises(np.linalg.LinAlgError, match="frame 25"):
        est.scale_calculation_batch(f3s, f2s)
    # the frames before it have been carried, into scale and height_level
    carried = stc.carry(est.last["raw_scale"][:25], est.last["status"][:25], scale=golden["s_tri"][2])
    assert carried.tobytes() == golden["s_tri"][:25].tobytes()
    assert est.scale == golden["s_tri"][24] and len(est.scale_queue) == 0
    assert np.float64(est.height_level).tobytes() == staged_sequence["height_level"][24].tobytes()
    assert int(est.last["status"][25]) == fc.ST_SINGULAR and np.isnan(est.last["raw_scale"][25]) and int(est.last["n_used"][25]) == 0
    assert est.ctx.alloc_stats()["live_blocks"] == before            # the chunks' blocks are released
    # ... and the next call is a fresh estimator's next call
    got, _ = est.scale_calculation_batch(f3s[26:], f2s[26:])
    fresh.scale = est.scale
    want, _ = fresh.scale_calculation_batch(f3s[26:], f2s[26:])
    assert got.tobytes() == want.tobytes() == golden["s_tri"][26:40].tobytes()


def test_stream_error_mid_call_releases_chunks_and_reruns(gpu, monkeypatch):
    """The streamed call of the resident static_tri estimator, as the project checks it for the RANSAC model: a host step raising
    while the third of six chunks is collected, re-runs of the first two pending — nothing of the call stays alive on the estimator's
    contexts or in the Delaunay pool's slots, and the next call is unaffected."""
    fr = _declining(_rescale_frames([150 + (i * 29) % 200 for i in range(768)], base_seed=91), [5, 130, 700])

    def make():
        est = _resident(delaunay_workers=3)
        est.GPU_CHUNK, est.GPU_RAMP, est.GPU_MIN_CHUNK = 128, False, 1
        return est
    _check_error_mid_call_is_released(make, fr, lambda e: [e.ctx, e._redo_ctx], monkeypatch)


# ---- 8. without the keyword ---------------------------------------------------------------------------------------------------------
def test_without_the_keyword_nothing_moved(gpu, golden, frames):
    sub = frames[:12]
    f3s, f2s = [f[0] for f in sub], [f[1] for f in sub]
    outs = []
    for kw in ({"model": "static_tri"}, {"model": "static_tri", "model_resident": False}):
        est = _estimator(**kw)
        s, z = est.scale_calculation_batch(f3s, f2s)
        outs.append((s.tobytes(), z.tobytes(), sorted(est.last), est.triangulation, est.sampling, float(est.scale)))
        assert s.tobytes() == golden["s_tri"][:12].tobytes() and (est.triangulation, est.sampling) == ("scipy", "host")
    assert outs[0] == outs[1]
    outs = []
    for kw in ({}, {"model_resident": False}):
        est = _estimator(ransac_seed=31, **kw)
        s, e = est.scale_calculation_batch(f3s, f2s)
        outs.append((s.tobytes(), e.tobytes(), sorted(est.last), est.last["model"].tobytes(), est.last["best_ic"].tobytes(),
                     np.array(est.scale_queue).tobytes(), float(est.scale), est.triangulation, est.sampling))
        assert (e == 1).all() and sorted(est.last) == sorted(["raw_scale", "height_level", "model", "best_ic", "used", "n_kept", "status"])
    assert outs[0] == outs[1]
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    with pytest.raises(ValueError, match="staged path"):
        ScaleEstimator(stc.ABS_REF, stc.WINDOW, triangulation="gpu", model="static_tri")
