"""-m gpu: depthcheck_kernel (mvosr_depth_check_batch) against the plain restatement (tests/depthcheck_cases.py) through the C ABI,
and ``ScaleEstimator.depth_check_batch`` / ``data_check`` against the reference's own run (tests/golden/depthcheck.npz).  Every
output is compared by bytes (NaN to NaN): the inputs are the same doubles, the counts are integers, every slope is the outcome of
IEEE operations taken one at a time and the file is built without contraction."""
from __future__ import annotations

import numpy as np
import pytest

import flat_cases as fc
import depthcheck_cases as dcc
import featdist_cases as fdc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crafted():
    c = dcc.crafted()
    assert int(dcc.golden()["c_crc"]) == dcc.checksum(c)
    return c


@pytest.fixture(scope="module")
def restated(crafted):
    return {name: dcc.depth_check_of(*case) for name, case in crafted.items()}


def _estimator(**kw):
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    return ScaleEstimator(fdc.ABS_REF, window_size=fdc.WINDOW, delaunay_workers=1, **kw)


def _show(got, want):
    return {k: (np.asarray(got[k]).tolist(), np.asarray(want[k]).tolist()) for k in ("n", "below", "above", "nan", "max", "status")}


# ---- the kernel through the C ABI ---------------------------------------------------------------------------------------------------
def test_every_crafted_frame_alone_equals_the_restatement(gpu, crafted, restated):
    for name, case in crafted.items():
        got, guards = dcc.run_frames(gpu, [case], sentinel=0xA5)
        assert dcc.same(got[0], restated[name]), (name, _show(got[0], restated[name]))
        assert all(fc.all_bytes(v, 0xA5) and v.size for v in guards.values()), name


def test_crafted_frames_in_one_ragged_batch_equal_the_restatement(gpu, crafted, restated):
    names = list(crafted)
    i = names.index("synthetic2100")
    names = names[:i + 1] + ["none_selected", "selected0"] + names[i + 1:]
    frames = [crafted[k] for k in names]
    j = names.index("plan%d" % (2 * dcc.plan()[1] + 1))
    empty = (np.zeros(0), np.zeros(0), np.zeros(0, np.uint8))    # a frame of no features between two full ones
    names, frames = names[:j + 1] + [None] + names[j + 1:], frames[:j + 1] + [empty] + frames[j + 1:]
    want = [restated[k] if k is not None else dcc.depth_check_of(*empty) for k in names]
    assert want[j + 1]["status"] == dcc.ST_NO_POINT
    got, guards = dcc.run_frames(gpu, frames, sentinel=0xA5)
    for k, g, w in zip(names, got, want):
        assert dcc.same(g, w), (k, _show(g, w))
    assert all(fc.all_bytes(v, 0xA5) and v.size for v in guards.values())
    again = dcc.run_frames(gpu, frames, with_cnt=False)          # off with one more entry, no gaps
    for k, g, w in zip(names, again, want):
        assert dcc.same(g, w), k


def test_golden_of_the_reference_on_the_crafted_frames(gpu, crafted):
    g = dcc.golden()
    names = [str(k) for k in g["c_names"]]
    got = dcc.run_frames(gpu, [crafted[k] for k in names])
    for i, (name, r) in enumerate(zip(names, got)):
        want = {k: g["c_" + k][i] for k in ("hist", "below", "above", "nan", "max", "n")}
        assert dcc.same(r, dict(want, status=0)), name


def test_refused_frames_leave_the_others_alone(gpu, crafted, restated):
    y, z, lv = crafted["plan%d" % (dcc.plan()[0] + 1)]
    bad = lv.copy()
    bad[-1] = 3                                                  # a level above 2, in the second row block
    tables = gpu.zeros((dcc.POPS, dcc.WORDS), np.int64)
    frames = [crafted["duplicate"], (y, z, bad), crafted["beyond"]]
    got = dcc.run_frames(gpu, frames, tables=tables)
    assert dcc.same(got[0], restated["duplicate"]) and dcc.same(got[2], restated["beyond"])
    assert dcc.same(got[1], dcc.depth_check_of(y, z, bad)) and got[1]["status"] == dcc.ST_ERR_MASK and not got[1]["n"].any()
    assert np.array_equal(tables.download(), dcc.table_of([restated["duplicate"], restated["beyond"]]))
    # a frame longer than the launch's max_feat is refused before it is read
    got = dcc.run_frames(gpu, [crafted["duplicate"], crafted["selected65"]], max_feat=10)
    assert dcc.same(got[0], restated["duplicate"]) and got[1]["status"] == dcc.ST_ERR_MASK and np.isnan(got[1]["max"]).all()
    tables.free()


def test_two_launches_add_to_one_table_and_a_repeat_is_identical(gpu, crafted, restated):
    first = ["plan%d" % (dcc.plan()[1] + 1), "depth_zero", "none_selected", "edge3"]
    second = ["synthetic2100", "population2_empty", "beyond"]
    tables = gpu.zeros((dcc.POPS, dcc.WORDS), np.int64)
    a = dcc.run_frames(gpu, [crafted[k] for k in first], tables=tables)
    assert np.array_equal(tables.download(), dcc.table_of(a))
    b = dcc.run_frames(gpu, [crafted[k] for k in second], tables=tables)
    assert np.array_equal(tables.download(), dcc.table_of(a + b))
    assert np.array_equal(tables.download(), dcc.table_of([restated[k] for k in first + second]))
    assert tables.download()[:, dcc.N_BINS + 2].tolist() == [1, 1, 1]             # depth_zero's NaN pair
    again = dcc.run_frames(gpu, [crafted[k] for k in second])
    for k, x, y in zip(second, b, again):
        assert all(np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes() for f in ("hist", "below", "above", "nan", "n")), k
        assert dcc.same_floats(x["max"], y["max"]) and x["status"] == y["status"]
    tables.free()


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def test_data_check_module(gpu, crafted, restated):
    from mvoscalerecovery_amd import data_check as D
    pts = lambda name: np.stack([np.zeros_like(crafted[name][0]), crafted[name][0], crafted[name][1]], axis=1)
    with pytest.raises(ValueError):
        D.depth_check(pts("none_selected"))
    with pytest.raises(ValueError):
        D.depth_check(np.zeros((0, 3)))
    one = D.depth_check(pts("plan%d" % (dcc.plan()[0] - 1)))
    r = restated["plan%d" % (dcc.plan()[0] - 1)]
    assert np.array_equal(one.hist, r["hist"][0]) and (one.below, one.above, one.nan, one.n) == tuple(int(r[k][0]) for k in ("below", "above", "nan", "n"))
    assert dcc.same_floats([one.max], [r["max"][0]]) and np.array_equal(one.bins, dcc.BINS)
    names = ["duplicate", "none_selected", "endpoint_lower", "selected64"]
    tables = D.new_tables()
    res = D.depth_check_batch([pts(k) for k in names], [crafted[k][2] for k in names], tables=tables)
    assert res.hist.shape == (4, 3, 59) and res.status.tolist() == [0, dcc.ST_NO_POINT, 0, 0]
    for i, k in enumerate(names):
        got = {f: getattr(res, f)[i] for f in D.FIELDS}
        assert dcc.same(got, restated[k]), k
    assert np.array_equal(tables.download(), res.tables()) and np.array_equal(res.tables(), dcc.table_of([restated[k] for k in names]))
    every = D.depth_check_batch([pts("endpoint_lower")])         # no levels: every point in every population
    assert every.n[0].tolist() == [3, 3, 3] and np.array_equal(every.hist[0, 2], restated["endpoint_lower"]["hist"][0])
    both = D.compare(pts("population2_empty"), pts("population2_empty")[crafted["population2_empty"][2] >= 1])
    r = restated["population2_empty"]
    assert np.array_equal(both.check_all.hist, r["hist"][0]) and np.array_equal(both.check_left.hist, r["hist"][1])
    assert both.check_left.n == 35 and np.array_equal(both.profile_left[0], D.road_profile(pts("population2_empty"))[0][1::2])
    tables.free()


def test_estimator_on_the_sequence_equals_the_references_run():
    from mvoscalerecovery_amd import synth
    g, gf = dcc.golden(), fdc.golden()
    frames = fdc.sequence_frames()
    assert int(gf["s_crc"]) == synth.checksum(*[a for fr in frames for a in fr])
    est = _estimator()
    res = est.depth_check_batch([f3.copy() for f3, _ in frames], [f2.copy() for _, f2 in frames])
    assert res.hist.shape == (60, 3, 59)
    for k in ("hist", "below", "above", "nan", "n"):
        assert np.array_equal(getattr(res, k), g["s_" + k]), k
    assert dcc.same_floats(res.max, g["s_max"])
    assert np.array_equal(res.status != 0, g["s_n"][:, 0] == 0)
    assert sorted(res.errors) == [i for i in range(60) if gf["s_end"][i] == 2]
    assert np.array_equal(est.depth_check_tables(), res.tables())
    assert np.array_equal(res.tables()[:, :59], g["s_hist"].sum(0)) and np.array_equal(res.tables()[:, 61], g["s_nan"].sum(0))
    quiet = est.depth_check_batch([frames[0][0]], [frames[0][1]], accumulate=False)
    assert np.array_equal(est.depth_check_tables(), res.tables()) and np.array_equal(quiet.hist[0], g["s_hist"][0])
    # frame by frame: the same bytes, the same tables, the staged pass's exceptions raised
    one = _estimator()
    for i, (f3, f2) in enumerate(frames):
        if i in res.errors:
            with pytest.raises(type(res.errors[i])):
                one.depth_check(f3.copy(), f2.copy())
            last = one.last_depth_check
        else:
            last = one.depth_check(f3.copy(), f2.copy())
        for k in ("hist", "below", "above", "nan", "n", "status"):
            assert np.array_equal(getattr(last, k)[0], getattr(res, k)[i]), (i, k)
        assert dcc.same_floats(last.max[0], res.max[i]), i
    assert np.array_equal(one.depth_check_tables(), res.tables())
    one.reset_depth_check()
    assert not one.depth_check_tables().any()
