"""-m gpu: static_tri_kernel (mvosr_static_tri_batch) against the reference's own run (tests/golden/statictri.npz) and the plain
restatement (tests/statictri_cases.py), through the C ABI, the two methods and ``rescale.ScaleEstimator(model=...)``.  Every output
is compared by bytes (NaN to NaN): the road model is a function of the list alone."""
from __future__ import annotations

import numpy as np
import pytest

import flat_cases as fc
import statictri_cases as stc

pytestmark = pytest.mark.gpu


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


def _want(z, pre, i, h, min_count=0):
    """The reference's result for list i of the golden's family ``pre``, as the launch writes it."""
    if len(h) == 0 or len(h) <= min_count:
        return stc.static_tri_of(h, min_count=min_count)
    return {"scale_norm": z[pre + "_scale"][i], "raw_scale": np.float64(z[pre + "_scale"][i]) * np.float64(stc.ABS_REF),
            "status": int(z[pre + "_status"][i]), "n_used": len(h), "hist": z[pre + "_hist"][i]}


def _bytes(results):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for r in results for k in stc.FIELDS)


def _estimator(**kw):
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    return ScaleEstimator(stc.ABS_REF, window_size=stc.WINDOW, delaunay_workers=1, **kw)


# ---- the kernel through the C ABI ---------------------------------------------------------------------------------------------------
def test_every_crafted_list_alone_equals_the_reference(gpu, golden, crafted):
    for i, (name, h) in enumerate(crafted.items()):
        got = stc.run_lists(gpu, [h])[0]
        assert stc.same(got, _want(golden, "c", i, h)), (name, got)


def test_crafted_lists_in_one_ragged_batch_equal_the_reference(gpu, golden, crafted):
    lists = list(crafted.values())
    got, guards = stc.run_lists(gpu, lists, sentinel=0xA5)
    for i, (name, h) in enumerate(crafted.items()):
        assert stc.same(got[i], _want(golden, "c", i, h)), (name, got[i])
    assert all(fc.all_bytes(g, 0xA5) for g in guards.values())                                # nothing behind the last list is written
    # rescale.py:181's rule: 12 heights or fewer are not looked at
    got12 = stc.run_lists(gpu, lists, min_count=12)
    for i, (name, h) in enumerate(crafted.items()):
        assert stc.same(got12[i], _want(golden, "c", i, h, min_count=12)), (name, got12[i])
    assert got12[list(crafted).index("n12")]["status"] == stc.ST_RS_FEW and got12[list(crafted).index("n13")]["status"] == stc.ST_MODE
    assert got12[list(crafted).index("empty")]["status"] == stc.ST_RS_FEW == got[list(crafted).index("empty")]["status"]


def test_random_lists_in_one_launch_equal_the_reference(gpu, golden, random_lists):
    got = stc.run_lists(gpu, random_lists)
    bad = [i for i, h in enumerate(random_lists) if not stc.same(got[i], _want(golden, "r", i, h))]
    assert not bad, (bad[:10], got[bad[0]])
    st = np.array([g["status"] for g in got])
    assert (st == stc.ST_MEDIAN).sum() >= 20 and (st == stc.ST_MODE).sum() >= 20


def test_both_input_forms_give_the_same_bytes(gpu, crafted, random_lists):
    lists = list(crafted.values()) + random_lists[:120]
    packed = stc.run_lists(gpu, lists, min_count=12)
    want = _bytes(packed)
    assert _bytes(stc.run_lists(gpu, lists, min_count=12, with_cnt=True)) == want             # packed, the lengths in cnt
    for with_cnt in (False, True):                                                            # the row form: uncounted rows with garbage between
        rows, guards = stc.run_lists(gpu, lists, min_count=12, rows=77 + with_cnt, with_cnt=with_cnt, sentinel=0x5A)
        assert _bytes(rows) == want, with_cnt
        assert all(fc.all_bytes(g, 0x5A) for g in guards.values())
    assert _bytes(stc.run_lists(gpu, lists, min_count=12)) == want                            # a repeated launch is identical
    no_hist = stc.run_lists(gpu, lists, min_count=12, hist=False)                             # the histogram is optional
    assert all(g["status"] == p["status"] and stc.same(dict(g, hist=p["hist"]), p) for g, p in zip(no_hist, packed))
    assert not any(np.asarray(g["hist"]).any() for g in no_hist)


def test_invalid_heights_are_refused_and_their_neighbours_are_not(gpu, golden, crafted):
    bad = stc.refused()
    good = crafted["plateau2"]
    lists = [x for h in bad.values() for x in (h, good)]
    for rows in (None, 5):
        got = stc.run_lists(gpu, lists, rows=rows)
        for i, name in enumerate(bad):
            r = got[2 * i]
            assert r["status"] == stc.ST_ERR_MASK and np.isnan(r["scale_norm"]) and np.isnan(r["raw_scale"]) and not r["hist"].any(), name
            assert r["n_used"] == len(bad[name])
            assert stc.same(got[2 * i + 1], stc.static_tri_of(good)) and got[2 * i + 1]["scale_norm"] == 0.45


def test_forty_thousand_entries_on_either_exit(gpu):
    rng = np.random.default_rng(40000)
    median = stc.from_counts(stc._counts(b2=2, b7=2, b11=2, b15=1), 71, tail=list(rng.uniform(1.95, 60.0, 39993)))
    median_low = np.concatenate([stc.from_counts(stc._counts(b2=2, b7=2), 72, tail=list(rng.uniform(1.95, 60.0, 19995))),
                                 stc.heights_of([stc.reachable(2.75, 3.0)[1]] * 20001)])      # an even count, the middle pair equal
    mode = np.float64(1.0) / np.abs(rng.normal(0.62, 0.11, 40000))
    assert len(median) == 40000 and len(median_low) == 40000
    want = [stc.static_tri_of(h, min_count=12) for h in (median, median_low, mode)]
    assert [w["status"] for w in want] == [stc.ST_MEDIAN, stc.ST_MEDIAN, stc.ST_MODE] and want[0]["scale_norm"] > 1.9
    for rows in (None, 9):
        got = stc.run_lists(gpu, [median, median_low, mode], min_count=12, rows=rows)
        assert all(stc.same(g, w) for g, w in zip(got, want)), (rows, got, want)


def test_launcher_arguments(gpu):
    from mvoscalerecovery_amd import _lib
    lib, h = gpu.lib, gpu.handle
    d = gpu.zeros(4, np.float64)
    assert lib.mvosr_static_tri_batch(h, 0, d.ptr, None, d.ptr, None, 12, 1.75, d.ptr, d.ptr, d.ptr, None, d.ptr) == 0     # empty: nothing launched
    assert lib.mvosr_static_tri_batch(h, -3, d.ptr, None, d.ptr, None, 12, 1.75, d.ptr, d.ptr, d.ptr, None, d.ptr) == 0
    for hole in (0, 2, 4, 8, 9, 10, 12):                                                      # ctx, off, height, scale_norm, raw_scale, n_used, status
        args = [h, 1, d.ptr, None, d.ptr, None, 12, 1.75, d.ptr, d.ptr, d.ptr, None, d.ptr]
        args[hole] = None
        assert lib.mvosr_static_tri_batch(*args) == -2, hole
    with pytest.raises(_lib.MvosrLibraryError, match=r"failed \(-2\)"):
        _lib.check(lib.mvosr_static_tri_batch(h, 1, d.ptr, None, d.ptr, None, -1, 1.75, d.ptr, d.ptr, d.ptr, None, d.ptr), "mvosr_static_tri_batch")
    d.free()


# ---- the two methods ------------------------------------------------------------------------------------------------------------------
def test_road_model_calculation_static_tri_on_the_golden_lists(gpu, golden, crafted, random_lists):
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    est = ScaleEstimator(stc.ABS_REF, stc.WINDOW, triangulation="scipy", delaunay_workers=1)
    for i, (name, h) in enumerate(crafted.items()):
        s, zero, one = est.road_model_calculation_static_tri(h)
        assert (zero, one) == (0, 1) and stc.same(dict(_want(golden, "c", i, h), scale_norm=s), _want(golden, "c", i, h)), name
    assert np.isnan(est.road_model_calculation_static_tri(np.zeros(0))[0])                   # np.median([])
    assert est.road_model_calculation_static_tri(crafted["n12"])[0] == 0.7                   # no minimum count here (:294-310)
    for i in range(0, 60):
        assert np.float64(est.road_model_calculation_static_tri(random_lists[i])[0]).tobytes() == golden["r_scale"][i].tobytes()
    for name, h in stc.refused().items():
        with pytest.raises(ValueError, match="finite and positive"):
            est.road_model_calculation_static_tri(h)


def test_scale_calculation_static_tri_alone_and_batched(gpu, golden, crafted, random_lists):
    lists = [crafted["n13"], crafted["n12"], crafted["empty"], crafted["plateau2"], crafted["n12"]] + random_lists[:40]
    want_raw = [stc.static_tri_of(h, min_count=12) for h in lists]
    want = stc.carry([w["raw_scale"] for w in want_raw], [w["status"] for w in want_raw])
    one = _estimator(triangulation="scipy")
    got = []
    for h in lists:
        s, zero = one.scale_calculation_static_tri(h)
        assert zero == 0 and one.scale == s
        got.append(s)
    assert np.array(got, dtype=np.float64).tobytes() == want.tobytes()
    assert got[1] == got[0] == got[2] == 0.7 * stc.ABS_REF and got[4] == got[3] == 0.45 * stc.ABS_REF       # the carried lists
    batch = _estimator(triangulation="scipy")
    s, zeros = batch.scale_calculation_static_tri_batch(lists)
    assert s.tobytes() == want.tobytes() and not zeros.any() and len(zeros) == len(lists) and batch.scale == s[-1]
    assert len(one.scale_queue) == 0 == len(batch.scale_queue)                              # no window (rescale.py:179-187)
    fresh = _estimator(triangulation="scipy")
    assert fresh.scale_calculation_static_tri(crafted["n12"]) == (1, 0)                      # the initial scale (rescale.py:26)
    with pytest.raises(ValueError, match="finite and positive"):
        fresh.scale_calculation_static_tri(stc.refused()["nan"])


# ---- the estimator's keyword ------------------------------------------------------------------------------------------------------------
def test_model_static_tri_reproduces_the_sequence(gpu, golden, frames):
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    est = _estimator(model="static_tri")
    assert (est.triangulation, est.sampling) == ("scipy", "host")
    s, zeros = est.scale_calculation_batch([a.copy() for a in f3s], [a.copy() for a in f2s])
    assert s.tobytes() == golden["s_tri"].tobytes() and not zeros.any()
    assert "model" not in est.last and "best_ic" not in est.last and len(est.scale_queue) == 0          # no RANSAC, no window
    assert np.array_equal(est.last["n_used"], golden["s_n_heights"])
    assert np.array_equal(est.last["status"] == stc.ST_RS_FEW, golden["s_n_heights"] <= 12) and (golden["s_n_heights"] <= 12).sum() >= 3
    one = _estimator(model="static_tri", region="grow")                                      # the heights do not depend on the region
    got = [one.scale_calculation(a.copy(), b.copy()) for a, b in frames]
    assert np.array([g[0] for g in got], dtype=np.float64).tobytes() == golden["s_tri"].tobytes() and all(g[1] == 0 for g in got)
    assert "model" not in one.last and len(one.scale_queue) == 0 and one.scale == golden["s_tri"][-1]


def test_model_static_reproduces_the_sequence(gpu, golden, frames):
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    est = _estimator(model="static")
    s, ones = est.scale_calculation_batch([a.copy() for a in f3s], [a.copy() for a in f2s])
    assert s.tobytes() == golden["s_static"].tobytes() and (ones == 1).all()
    assert len(est.scale_queue) == 0
    assert len(est.sc.scale_queue) == stc.WINDOW and est.sc.camera_pitch == -0.5 * np.pi / 180          # the inner estimator's own state
    one = _estimator(model="static")
    got = [one.scale_calculation(a.copy(), b.copy()) for a, b in frames]
    assert np.array([g[0] for g in got], dtype=np.float64).tobytes() == golden["s_static"].tobytes() and all(g[1] == 1 for g in got)


def test_model_static_raises_where_the_reference_does(gpu):
    est = _estimator(model="static")
    with pytest.raises(AttributeError, match="height_level"):                                # an empty point list, no level ever set (:335)
        est.sc.scale_calculation_static_batch([np.zeros((0, 3))])
    assert len(est.sc.scale_queue) == 0


def test_default_model_is_the_estimator_without_the_keyword(gpu, frames):
    sub = frames[:5] + frames[7:9]
    outs = []
    for kw in ({}, {"model": "ransac"}):
        est = _estimator(triangulation="scipy", ransac_seed=31, **kw)
        s1, e1 = est.scale_calculation_batch([a.copy() for a, _ in sub], [b.copy() for _, b in sub])
        per = [est.scale_calculation(a.copy(), b.copy()) for a, b in sub[:3]]
        outs.append((s1.tobytes(), e1.tobytes(), np.array([p[0] for p in per]).tobytes(), [p[1] for p in per], sorted(est.last),
                     est.last["model"].tobytes(), est.last["best_ic"].tobytes(), np.array(est.scale_queue).tobytes(), float(est.scale),
                     est.triangulation, est.sampling))
        assert not hasattr(est, "sc")
    assert outs[0] == outs[1]
    dev = _estimator(ransac_seed=31, model="ransac")
    assert (dev.triangulation, dev.sampling) == ("gpu", "device")                             # the default still selects the device path
