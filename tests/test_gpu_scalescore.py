"""The scales' own score on the device: mvosr_scale_errors_batch and mvosr_window_median_cases (csrc/mvosr_scalescore.hip) through
the C ABI, evaluate.scale_errors / filter_scales, Scorer.score_gt_rescaled and RepeatedRuns.scale_scores.  Needs a real MI355X.

The comparator is the reference's own output in tests/golden/scalescores.npz (make_golden_scalescores.py): every float bit for
bit (any NaN where the reference has NaN), every integer exact.  The re-scaled ground truth goes through the scorer's kernels and
is held to their rule (tests/scores_cases.py): within 4 gaps, the gap being the fixture's |reference - extended precision|.
Every launch helper puts sentinel guards around its outputs.
"""
import json
import warnings

import numpy as np
import pytest

import scalescore_cases as ssc
import scores_cases as sc
from conftest import load_npz

pytestmark = pytest.mark.gpu
NAMES = list(ssc.SETS)
GLOBAL = 1                       # MVOSR_SCALE_ERRORS_GLOBAL
KEYS = ("mean", "max", "counts", "drift", "status")


@pytest.fixture(scope="module")
def golden():
    return load_npz("scalescores.npz")[0]


@pytest.fixture(scope="module")
def device(gpu):
    """Every set through mvosr_scale_errors_batch, once."""
    out = {}
    for name in NAMES:
        s = ssc.make_set(name)
        out[name] = dict(s, res=ssc.launch_errors(gpu, s["gt"], s["scales"]))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_scale_errors_equal_the_reference(gpu, golden, device, name):
    from mvoscalerecovery_amd import evaluate
    n, _, cases = ssc.SETS[name][:3]
    d, r = device[name], device[name]["res"]
    assert ssc.checksum(d) == int(golden[name + "_crc"])
    assert ssc.same(r["mean"], golden[name + "_mean"]) and ssc.same(r["max"], golden[name + "_max"]), (r["mean"], r["max"])
    assert np.array_equal(r["counts"], golden[name + "_counts"])                                       # integers: exact
    assert ssc.same(r["drift"], golden[name + "_drift"]), (r["drift"], golden[name + "_drift"])
    assert (r["status"] == (0 if n else 9)).all()                                                      # MVOSR_ST_ERR_EMPTY: no scale at all
    api = evaluate.scale_errors(d["gt"], d["scales"], ctx=gpu)
    assert api["n"] == n and api["exceed_counts"].dtype.kind == "i" and api["drift"].shape == (cases, 11)
    for k, g in (("mean", "mean"), ("max", "max"), ("drift", "drift"), ("within", "within")):
        assert ssc.same(api[k], golden["%s_%s" % (name, g)]), (name, k)
    assert np.array_equal(api["exceed_counts"], golden[name + "_counts"])
    one = evaluate.scale_errors(d["gt"], d["scales"][0], ctx=gpu)                                      # (n,) scales: no leading axis
    assert np.ndim(one["mean"]) == 0 and one["drift"].shape == (11,) and ssc.same(one["drift"], golden[name + "_drift"][0])


@pytest.mark.parametrize("name", [k for k in NAMES if ssc.SETS[k][5]])
def test_filter_equals_the_reference(gpu, golden, name):
    from mvoscalerecovery_amd import evaluate
    scales = ssc.make_set(name)["scales"]
    for w in ssc.SETS[name][5]:
        want = golden[name + "_filter%d" % w]
        assert ssc.same(ssc.launch_filter(gpu, scales, w), want), (name, w)
        assert ssc.same(evaluate.filter_scales(scales, w, ctx=gpu), want)
        assert ssc.same(evaluate.filter_scales(scales[-1], w, ctx=gpu), want[-1])
        left = evaluate.filter_scales(scales, w, ctx=gpu, on_device=True)
        assert left.shape == scales.shape and ssc.same(left.download(), want)
    for c in (0, scales.shape[0] - 1):                                                                 # one sequence alone: the same bytes
        assert ssc.launch_filter(gpu, scales[c:c + 1], 10).tobytes() == ssc.launch_filter(gpu, scales, 10)[c].tobytes()


def test_filter_beyond_one_block_equals_the_host_comparator(gpu):
    from mvoscalerecovery_amd import evaluate
    scales = ssc.make_set("n6000")["scales"]
    scales[1, 300] = np.nan
    got = ssc.launch_filter(gpu, scales, 7)
    assert ssc.same(got, np.array([evaluate.scale_filter(scales[c], 7) for c in range(2)]))


@pytest.mark.parametrize("name", [k for k in NAMES if ssc.SETS[k][0] <= ssc.LDS_ERRORS])
def test_lds_and_global_forms_agree(gpu, device, name):
    d = device[name]
    g = ssc.launch_errors(gpu, d["gt"], d["scales"], flags=GLOBAL)
    for k in KEYS:
        assert g[k].tobytes() == d["res"][k].tobytes(), (name, k)


@pytest.mark.parametrize("name", ["ten1000", "n21", "n6000", "nan"])
def test_one_launch_of_c_cases_equals_c_launches(gpu, device, name):
    d = device[name]
    for c in sorted({0, d["scales"].shape[0] // 2, d["scales"].shape[0] - 1}):
        one = ssc.launch_errors(gpu, d["gt"], d["scales"][c:c + 1])
        for k in KEYS:
            assert one[k][0].tobytes() == d["res"][k][c].tobytes(), (name, c, k)


def test_other_windows_steps_and_thresholds(gpu):
    """Not only the reference's lists: step 1 and 3, windows at the leaf sizes, one threshold, none."""
    s = ssc.make_set("n811")
    for windows, step, thr in (([7, 8, 9, 127, 128, 129, 257], 3, [0.25]), ([5, 64], 1, []), ([], 10, [0.1, 0.2])):
        want = ssc.errors_restated(s["gt"], s["scales"], windows, step, thr)
        for flags in (0, GLOBAL):
            got = ssc.launch_errors(gpu, s["gt"], s["scales"], windows, step, thr, flags)
            assert ssc.same(got["mean"], want["mean"]) and ssc.same(got["max"], want["max"])
            assert np.array_equal(got["counts"], want["counts"]) and ssc.same(got["drift"], want["drift"]), (windows, step, flags)


def test_same_bytes_every_run(gpu, device):
    for name in ("ten1000", "n6000"):
        d = device[name]
        again = ssc.launch_errors(gpu, d["gt"], d["scales"])
        for k in KEYS:
            assert again[k].tobytes() == d["res"][k].tobytes(), (name, k)
    s = device["ten1000"]["scales"]
    assert ssc.launch_filter(gpu, s, 10).tobytes() == ssc.launch_filter(gpu, s, 10).tobytes()


def test_gt_rescaled_against_change_scale_and_the_reference(gpu, golden):
    from mvoscalerecovery_amd import evaluate
    gaps = json.loads(str(golden["gtr_gaps"]))                                                         # measured by the fixture's maker
    gt = sc.make_sequence(ssc.GT_RESCALED)["gt"]
    scales = ssc.rescaled_scales()
    assert int(np.ascontiguousarray(scales).view(np.uint64).sum() & 0x7FFFFFFFFFFFFFFF) == int(golden["gtr_crc"])
    scorer = evaluate.Scorer(gt, ctx=gpu)
    got = scorer.score_gt_rescaled(scales)
    paths = np.array([evaluate.change_scale(gt, scales[c], ctx=gpu) for c in range(scales.shape[0])])
    want = scorer.score_paths(paths)
    assert set(got) == set(want) and got["tra"].shape == golden["gtr_tra"].shape
    for k in ("tra", "rot", "tra_mean", "rot_mean"):
        sc.within(got[k], want[k], gaps[k[:3]], "score_gt_rescaled vs change_scale + score_paths " + k)
        sc.within(got["trimmed"][k], want["trimmed"][k], gaps[k[:3]], "trimmed " + k)
    sc.within(got["tra"], golden["gtr_tra"], gaps["tra"], "score_gt_rescaled vs the reference tra")
    sc.within(got["rot"], golden["gtr_rot"], gaps["rot"], "score_gt_rescaled vs the reference rot")
    assert scorer.score_gt_rescaled(gpu.to_device(scales))["tra"].tobytes() == got["tra"].tobytes()    # scales already on the device
    assert scorer.score_gt_rescaled(scales)["rot"].tobytes() == got["rot"].tobytes()
    with pytest.raises(ValueError):
        scorer.score_gt_rescaled(scales[:, :-1])


def _runs_data():
    """A short main_offline dict whose motions carry 12 m steps, and a ground truth of its length."""
    from mvoscalerecovery_amd import synth
    seq = sc.make_sequence("n65")
    n = 60
    data = synth.synth_sequence_dict(n, base_seed=77, n_lo=300, n_hi=600, p_not_moving=0.05, p_too_few=0.05)
    motions = seq["motions"][:n].copy()
    motions[:, 3:12:4] *= 12.0
    data["motions"] = [m for m in motions]
    return data, seq["gt"][:n + 1]


def test_repeated_runs_scale_scores(gpu):
    from mvoscalerecovery_amd import evaluate
    from mvoscalerecovery_amd.rescale import RepeatedRuns
    data, gt = _runs_data()
    runs = RepeatedRuns(1.75, window_size=5, seed=11, cases=4, triangulation="gpu", delaunay_workers=0)
    runs.run(data)
    scales = runs.scales()
    assert scales.shape == (4, 60)
    speed_gt = np.concatenate([evaluate.calculate_speed(gt, ctx=gpu) / 12.0, [1.0, 1.0]])             # two more than the scales
    got = runs.scale_scores(speed_gt, poses_gt=gt, filter_window=5)
    assert set(got) == {"scales", "filtered", "gt_rescaled", "gt_rescaled_filtered", "trimmed"}
    filtered = np.array([evaluate.scale_filter(scales[c], 5) for c in range(4)])
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for key, rows in (("scales", scales), ("filtered", filtered)):
            host = [evaluate.evaluate_scale(speed_gt, rows[c]) for c in range(4)]                      # per case, on the host
            figs = got[key]
            assert ssc.same(figs["mean"], [h[0][0] for h in host]) and ssc.same(figs["max"], [h[0][1] for h in host]), key
            assert ssc.same(figs["within"], [h[0][2:] for h in host]) and ssc.same(figs["drift"], [h[1] for h in host]), key
            assert np.isfinite(figs["drift"][:, :3]).all() and np.isnan(figs["drift"][:, 3:]).all()   # 60 frames: windows 10, 20, 50
            trimmed = got["trimmed"][key]
            assert ssc.same(trimmed["mean"], evaluate.trimmed_mean(figs["mean"])) and ssc.same(trimmed["max"], evaluate.trimmed_mean(figs["max"]))
            assert ssc.same(trimmed["drift"], [evaluate.trimmed_mean(figs["drift"][:, k]) for k in range(11)])
            assert ssc.same(trimmed["within"], [evaluate.trimmed_mean(figs["within"][:, k]) for k in range(4)])
    scorer = evaluate.Scorer(gt, ctx=gpu)
    for key, rows in (("gt_rescaled", scales), ("gt_rescaled_filtered", filtered)):
        want = scorer.score_gt_rescaled(rows)
        assert all(got[key][k].tobytes() == want[k].tobytes() for k in ("tra", "rot", "tra_mean", "rot_mean")), key
    plain = runs.scale_scores(speed_gt)
    assert set(plain) == {"scales", "trimmed"} and plain["scales"]["drift"].tobytes() == got["scales"]["drift"].tobytes()
    with pytest.raises(ValueError):
        runs.scale_scores(speed_gt[:59])


def test_refusals_return_error_codes(gpu):
    lib, h = gpu.lib, gpu.handle
    buf = gpu.zeros(256, np.float64)
    p = buf.ptr
    w, t = np.array([10, 20], dtype=np.int32), np.array([0.1], dtype=np.float64)
    wp, tp = w.ctypes.data, t.ctypes.data
    call = lambda **kw: lib.mvosr_scale_errors_batch(*[{**dict(ctx=h, n_gt=8, gt=p, C=1, n=8, s=p, stride=8, W=2, w=wp, step=10, T=1, t=tp,
                                                               flags=0, stats=p, counts=p, drift=p, status=p), **kw}[k]
                                                       for k in ("ctx", "n_gt", "gt", "C", "n", "s", "stride", "W", "w", "step", "T", "t",
                                                                 "flags", "stats", "counts", "drift", "status")])
    assert call(n=9, stride=9) == -2                                                                   # more scales than ground truth
    assert call(C=0) == -2 and call(n=-1) == -2 and call(stride=7) == -2 and call(step=0) == -2
    assert call(W=17) == -2 and call(T=9) == -2 and call(gt=None) == -2 and call(stats=None) == -2 and call(w=None) == -2
    bad = np.array([10, 8193], dtype=np.int32)
    assert call(w=bad.ctypes.data) == -2 and call(C=65536) == -3
    assert lib.mvosr_window_median_cases(h, p, 1, 8, 8, 0, p, 8) == -2 and lib.mvosr_window_median_cases(h, p, 1, 8, 8, 65, p, 8) == -2
    assert lib.mvosr_window_median_cases(h, p, 0, 8, 8, 5, p, 8) == -2 and lib.mvosr_window_median_cases(h, p, 1, 8, 7, 5, p, 8) == -2
    assert lib.mvosr_window_median_cases(h, None, 1, 8, 8, 5, p, 8) == -2 and lib.mvosr_window_median_cases(h, p, 1, 0, 0, 5, p, 0) == 0
    assert (buf.download() == 0).all()                                                                 # nothing was launched
