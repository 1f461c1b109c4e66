"""-m gpu: featdist_kernel (mvosr_feature_distribution_batch) against the plain restatement (tests/featdist_cases.py) through the C
ABI, and ``ScaleEstimator.check_full_distribution`` and its companions against the reference's own run (tests/golden/featdist.npz).
Every output is compared by bytes (NaN to NaN): the inputs are the same doubles, the histograms are integers, mean / std / median
are stated in NumPy's own operation order and the file is built without contraction."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

import flat_cases as fc
import featdist_cases as fdc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return fdc.golden()


@pytest.fixture(scope="module")
def crafted():
    c = fdc.crafted()
    z = fdc.golden()
    assert list(z["l_names"]) == list(c) and int(z["l_crc"]) == fdc.checksum(c) and int(z["l_cap"]) == fdc.cap()
    return c


@pytest.fixture(scope="module")
def restated(crafted):
    return {name: fdc.featdist_of(*case) for name, case in crafted.items()}


@pytest.fixture(scope="module")
def sequence():
    from mvoscalerecovery_amd import synth
    frames, scales = fdc.sequence_frames(), fdc.sequence_scales()
    assert int(fdc.golden()["s_crc"]) == synth.checksum(*[a for fr in frames for a in fr])
    return frames, scales


def _estimator(**kw):
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    return ScaleEstimator(fdc.ABS_REF, window_size=fdc.WINDOW, delaunay_workers=1, **kw)


# ---- the kernel through the C ABI ---------------------------------------------------------------------------------------------------
def test_every_crafted_list_alone_equals_the_restatement(gpu, crafted, restated):
    for name, case in crafted.items():
        got = fdc.run_frames(gpu, [case])[0]
        assert fdc.same(got, restated[name]), (name, got["n"], got["stats"], restated[name]["stats"])


def test_crafted_lists_in_one_ragged_batch_equal_the_restatement(gpu, crafted, restated):
    names = list(crafted)
    i = names.index("len2000")
    names = names[:i] + ["len0"] + names[i:]                     # a frame of no features between two full ones
    got, guards = fdc.run_frames(gpu, [crafted[k] for k in names], sentinel=0xA5)
    for k, g in zip(names, got):
        assert fdc.same(g, restated[k]), k
    assert all(fc.all_bytes(v, 0xA5) and v.size for v in guards.values())
    again = fdc.run_frames(gpu, [crafted[k] for k in names], with_cnt=False)       # off with one more entry, no gaps
    for k, g in zip(names, again):
        assert fdc.same(g, restated[k]), k


def test_lengths_where_numpys_sum_changes_shape(crafted, restated, gpu):
    """Every length of the issue's list is there, all three populations full, and the sums are not the plain loop's."""
    assert {len(crafted["len%d" % n][0]) for n in fdc.LENGTHS + (fdc.cap(),)} == set(fdc.LENGTHS) | {fdc.cap()}
    differ = 0
    for n in (130, 136, 255, 256, 257, 1000, 1024, 2000, fdc.cap()):
        y = crafted["len%d" % n][0]
        got = fdc.run_frames(gpu, [crafted["len%d" % n]])[0]
        assert got["n"].tolist() == [n, n, n]
        differ += not fdc.same_floats(got["stats"][0][:2], fdc.stats_of(y, total=fdc.left_to_right_sum)[:2])
    assert differ >= 7


def test_edges(gpu, crafted, restated):
    for name in ("edges_all", "edges_finite", "closing_edges", "product_on_edge"):
        got = fdc.run_frames(gpu, [crafted[name]])[0]
        assert fdc.same(got, restated[name]), name
    y, lv, _ = crafted["edges_finite"]
    got = fdc.run_frames(gpu, [crafted["edges_finite"]])[0]
    for p in range(3):
        vals = y[lv >= p]
        for bins in (29, 49, 99, 169):
            assert np.array_equal(fdc.narrow(got["hist"][p], bins), np.histogram(vals, bins=np.array(range(0, bins + 1)) * 0.1)[0]), (p, bins)
    got = fdc.run_frames(gpu, [crafted["closing_edges"]])[0]
    assert got["hist"][2][fdc.N_BINS:].tolist() == [3, 3, 3]


def test_median(gpu, crafted, restated):
    for name in crafted:
        if name.startswith("median_") or name == "minus_zero":
            y = crafted[name][0]
            got = fdc.run_frames(gpu, [crafted[name]])[0]
            assert fdc.same(got, restated[name]), name
            assert fdc.same_floats(got["stats"][2][2], np.median(y)), name
    assert np.signbit(fdc.run_frames(gpu, [crafted["minus_zero"]])[0]["stats"][2][2]) == np.signbit(np.median(np.array([-0.0])))


def test_levels(gpu, crafted, restated):
    names = ["alternating", "level_3", "no_selection", "nothing_kept", "len257"]
    got = fdc.run_frames(gpu, [crafted[k] for k in names])
    for k, g in zip(names, got):
        assert fdc.same(g, restated[k]), k
    by = dict(zip(names, got))
    assert by["level_3"]["status"] == fdc.ST_ERR_MASK and not by["level_3"]["hist"].any() and np.isnan(by["level_3"]["stats"]).all()
    assert [by[k]["status"] for k in names if k != "level_3"] == [0, 0, 0, 0]               # ... for that frame only
    assert by["no_selection"]["n"][2] == 0 and np.isnan(by["no_selection"]["stats"][2]).all() and not by["no_selection"]["hist"][2].any()
    assert by["nothing_kept"]["n"].tolist() == [70, 0, 0] and by["len257"]["n"].tolist() == [257, 257, 257]
    # a frame longer than the launch's max_feat is refused before anything of it is read
    got = fdc.run_frames(gpu, [crafted["len257"], crafted["len9"]], max_feat=100)
    assert got[0]["status"] == fdc.ST_ERR_MASK and not got[0]["n"].any() and fdc.same(got[1], restated["len9"])


def test_launch_above_the_cap_is_refused(gpu):
    from mvoscalerecovery_amd import _lib
    with pytest.raises(_lib.MvosrLibraryError):
        fdc.run_frames(gpu, [(np.zeros(4), np.zeros(4, np.uint8), 1.0)], max_feat=fdc.cap() + 1)


def test_sequence_tables(gpu, crafted, restated):
    names = ["ragged1000", "alternating", "product_on_edge", "scale_small", "scale_negative", "len129", "level_3"]
    frames = [crafted[k] for k in names]
    seq = gpu.zeros((fdc.POPS, fdc.WORDS), np.int64)
    try:
        ones = [(y, lv, 1.0) for y, lv, _ in frames]
        got = fdc.run_frames(gpu, ones, seq=seq)
        raw = sum(g["hist"].astype(np.int64) for g in got)
        assert np.array_equal(seq.download(), raw) and raw.any()                           # scale 1: the sum of the raw histograms
        fdc.run_frames(gpu, ones, seq=seq)
        assert np.array_equal(seq.download(), 2 * raw)                                     # two launches accumulate
        seq.fill(0)
        got = fdc.run_frames(gpu, frames, seq=seq)
        want = sum(restated[k]["hist_scaled"].astype(np.int64) for k in names)
        assert np.array_equal(seq.download(), want) and not np.array_equal(want, raw)      # per-frame scales are applied
        assert restated["product_on_edge"]["hist_scaled"][2][fdc.N_BINS:].tolist() == [2, 2, 2]
        seq.fill(0)
        fdc.run_frames(gpu, [crafted["scale_nan"], crafted["scale_inf"]], seq=seq)
        table = seq.download()
        assert not table[:, 1:].any() and np.array_equal(table, restated["scale_inf"]["hist_scaled"].astype(np.int64))   # NaN adds nothing
    finally:
        seq.free()


# ---- the public surface -------------------------------------------------------------------------------------------------------------
def _modes_plain(modes):
    return [[float(v) for v in np.asarray(run, dtype=np.float64).reshape(-1)] for run in modes]


def _decode_modes(flat):
    runs, run = [], []
    for v in flat:
        if np.isnan(v):
            runs.append(run)
            run = []
        else:
            run.append(float(v))
    return runs + [run] if len(flat) else []


def _per_frame(est, golden, frames, scales):
    """check_full_distribution frame by frame, held to the golden after every frame -> the frames' results, stacked."""
    steps, cum = fdc.replay(golden, "s_", frames, scales)
    rows = []
    for i, ((f3, f2), s) in enumerate(zip(frames, scales)):
        a3, a2 = f3.copy(), f2.copy()
        error = ""
        try:
            est.check_full_distribution(a3, a2, s, None)
        except Exception as exc:                                  # noqa: BLE001 - compared with what the reference raised
            error = type(exc).__name__
        assert error == str(golden["s_error"][i]), i
        assert np.array_equal(a3, f3) and np.array_equal(a2, f2)                           # no remap (:563)
        last = est.last_distribution
        r, state = steps[i]
        got = {"n": last.n[0], "hist": last.words[0], "hist_scaled": last.words_scaled[0], "stats": np.stack([last.mean[0], last.std[0], last.median[0]], axis=1),
               "status": 0}
        assert fdc.same(got, r), i
        end = int(golden["s_end"][i])
        assert (end == 1) == (int(last.status[0]) == 1) and (end == 2) == (int(last.status[0]) in (2, 3, 4)), (i, last.status)
        low = f2[:, 1] > 185
        lv = golden["s_levels"][golden["s_levels_off"][i]:golden["s_levels_off"][i + 1]]
        assert np.array_equal(est.all_feature, f3[low])
        if lv.any():
            assert np.array_equal(est.correct_distance_feature, f3[low][lv >= 1])
        if (lv == 2).any():
            assert np.array_equal(est.flat_feature, f3[low][lv == 2])
        assert fdc.same_floats(getattr(est, "height_level", np.nan), golden["s_height_level"][i]), i
        assert [len(est.all_features), len(est.correct_distance_features), len(est.flat_features)] == golden["s_n_lists"][i].tolist()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d = est.plot_distribution("frame %d" % i, None)
            assert np.array_equal(d["all_hist"], golden["s_all49"][i]) and np.array_equal(d["correct_hist"], golden["s_cor49"][i]), i
            assert fdc.same_floats(d["selected"], 0.1 * golden["s_flat49"][i]) and fdc.same_floats(d["bins"], (np.array(range(0, 50)) * 0.1)[:-1])
            assert np.array_equal(d["all_points"][0], est.all_feature[:, 2]) and np.array_equal(d["selected_points"][1], -est.flat_feature[:, 1])
            assert fdc.same_floats(est.skewness_analysis(), golden["s_p1"][i]), i           # (stale after a frame that selects nothing)
            assert fdc.same_floats(est.check_skewness(est.flat_feature[:, 1], method='p2'), golden["s_p2"][i]), i
            assert fdc.same_floats(est.check_skewness(est.flat_feature[:, 1]), golden["s_p1"][i]), i
            m = golden["s_modes"][golden["s_modes_off"][i]:golden["s_modes_off"][i + 1]]
            assert _modes_plain(est.mode_analysis()) == _decode_modes(m), i
        rows.append((last.n[0], last.words[0], last.words_scaled[0], got["stats"], last.height_level[0], last.status[0], last.skew_p1[0], last.skew_p2[0]))
    for bins in (29, 49):
        assert np.array_equal(est.cumulative_histograms(bins), golden["s_cum%d" % bins]), bins
        lists = (est.all_features, est.correct_distance_features, est.flat_features)
        assert np.array_equal(est.cumulative_histograms(bins),
                              np.stack([np.histogram(np.array(l)[:, 1], bins=np.array(range(0, bins + 1)) * 0.1)[0] for l in lists]))
    assert np.array_equal(fdc.narrow(cum, 169), est.cumulative_histograms(169))
    return [np.stack(col) for col in zip(*rows)]


@pytest.mark.parametrize("kind", ["default", "scipy"])
def test_per_frame_and_batch_equal_each_other_and_the_reference(golden, sequence, kind):
    frames, scales = sequence
    kw = {} if kind == "default" else {"triangulation": "scipy"}
    one, many = _estimator(**kw), _estimator(**kw)
    per = _per_frame(one, golden, frames, scales)
    res = many.check_full_distribution_batch([f3.copy() for f3, _ in frames], [f2.copy() for _, f2 in frames], scales)
    assert len(res) == len(frames) and res.hist.shape == (len(frames), 3, 169)
    stats = np.stack([res.mean, res.std, res.median], axis=2)
    for a, b in zip(per, (res.n, res.words, res.words_scaled, stats, res.height_level, res.status, res.skew_p1, res.skew_p2)):
        assert fdc.same_floats(a, b) if np.asarray(a).dtype.kind == "f" else np.array_equal(a, b)
    assert sorted(res.errors) == [i for i in range(len(frames)) if golden["s_end"][i] == 2]
    assert [type(res.errors[i]).__name__ for i in sorted(res.errors)] == [str(golden["s_error"][i]) for i in sorted(res.errors)]
    steps, _ = fdc.replay(golden, "s_", frames, scales)
    for i in range(len(frames)):
        if steps[i][0]["n"][2] > 0:                              # a frame with a selection of its own
            assert fdc.same_floats([res.skew_p1[i, 2], res.skew_p2[i, 2]], [golden["s_p1"][i], golden["s_p2"][i]]), i
            m = golden["s_modes"][golden["s_modes_off"][i]:golden["s_modes_off"][i + 1]]
            assert _modes_plain(res.modes(i)) == _decode_modes(m), i
            assert fdc.same_floats(res.histogram(i, 2, 49, density=True), golden["s_flat49"][i]), i
        assert np.array_equal(res.histogram(i, 0, 49), golden["s_all49"][i]), i
    # the attributes after the call are those after the last frame
    for name in ("all_feature", "correct_distance_feature", "flat_feature"):
        assert np.array_equal(getattr(one, name), getattr(many, name)), name
    assert fdc.same_floats(one.height_level, many.height_level)
    for name in ("all_features", "correct_distance_features", "flat_features"):
        assert len(getattr(one, name)) == len(getattr(many, name)) and np.array_equal(np.array(getattr(one, name)), np.array(getattr(many, name))), name
    for bins in (29, 49, 169):
        assert np.array_equal(one.cumulative_histograms(bins), many.cumulative_histograms(bins))
    assert fdc.same_floats(one.skewness_analysis(), many.skewness_analysis())
    dens = many.cumulative_histograms(29, density=True)
    assert fdc.same_floats(dens[0], np.histogram(np.array(many.all_features)[:, 1], bins=np.array(range(0, 30)) * 0.1, density=True)[0])
    many.reset_distribution()
    assert not many.cumulative_histograms(169).any() and many.all_features == [] and many.flat_features == []


def test_crafted_frames_take_the_references_exits(golden):
    cf = fdc.crafted_frames()
    est = _estimator(triangulation="scipy")
    steps, cum = fdc.replay(golden, "f_", [(v[0], v[1]) for v in cf.values()], [v[2] for v in cf.values()])
    for i, (name, (f3, f2, s)) in enumerate(cf.items()):
        error = ""
        try:
            est.check_full_distribution(f3.copy(), f2.copy(), s, None)
        except Exception as exc:                                  # noqa: BLE001
            error = type(exc).__name__
        assert error == str(golden["f_error"][i]), name
        assert (int(est.last_distribution.status[0]) == 1) == (int(golden["f_end"][i]) == 1), name
        assert [len(est.all_features), len(est.correct_distance_features), len(est.flat_features)] == golden["f_n_lists"][i].tolist(), name
        assert fdc.same_floats(getattr(est, "height_level", np.nan), golden["f_height_level"][i]), name
        assert bool(golden["f_flat_ok"][i]) == (not isinstance(est.flat_feature, list)), name
        last = est.last_distribution
        assert np.array_equal(last.n[0], steps[i][0]["n"]) and np.array_equal(last.words[0], steps[i][0]["hist"]), name
    assert np.array_equal(est.cumulative_histograms(49), golden["f_cum49"])


def test_exceptions():
    est = _estimator(triangulation="scipy")
    with pytest.raises(TypeError):
        est.skewness_analysis()                                   # flat_feature is still [] (:501)
    with pytest.raises(TypeError):
        est.mode_analysis()
    with pytest.raises(TypeError):
        est.plot_distribution("none", None)                       # all_feature is still [] (:546)
    cap = est.engine.feature_distribution_max_features()
    assert cap == fdc.cap()
    n = cap + 8
    f2 = np.stack([np.linspace(10.0, 1200.0, n), np.linspace(190.0, 370.0, n)], axis=1)
    with pytest.raises(ValueError, match=str(cap)):
        est.check_full_distribution(np.ones((n, 3)), f2, 1.0, None)
    with pytest.raises(ValueError, match=str(cap)):
        est.check_skewness(np.ones(n))
    assert est.all_features == [] and isinstance(est.all_feature, list)
    with pytest.raises(UnboundLocalError):
        est.check_skewness(np.array([1.0, 2.0, 4.0]), method='p3')


def test_no_state_leaks_into_the_scale_path(sequence):
    frames, scales = sequence
    for kw in ({}, {"triangulation": "scipy"}):
        touched, clean = _estimator(**kw), _estimator(**kw)
        touched.check_full_distribution(frames[0][0].copy(), frames[0][1].copy(), scales[0], None)
        touched.check_full_distribution_batch([frames[1][0].copy()], [frames[1][1].copy()], scales[1:2])
        assert len(touched.scale_queue) == 0 and touched.last_raw_scale is None          # the scale queue is untouched
        for f3, f2 in frames[2:8]:
            a = touched.scale_calculation(f3.copy(), f2.copy())
            b = clean.scale_calculation(f3.copy(), f2.copy())
            assert fdc.same_floats(a, b)
        assert list(touched.scale_queue) == list(clean.scale_queue)
