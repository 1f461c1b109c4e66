"""GPU: mvosr_height_pitch_batch (height_pitch_kernel) and mvoscalerecovery_amd.height_pitch on crafted frames and on the reference's own
run of /root/reference/src/calculate_height_pitch.py (tests/golden/heightpitch.npz).

Crafted frames (tests/heightpitch_cases.py; at most 64 frames a launch, N <= 300, H <= 512): the np.longdouble reference decides every
integer output (tests/test_heightpitch_cases.py asserts it on the CPU), so n_selected, the point list, hyp_counts, best_ic, used,
n_inliers and the mask are demanded exactly, and every float within the reference's derived bound.
Golden leg: integers equal the script's; ransac_camera_heights to rtol 1e-9, the model to rtol 1e-8 / atol 1e-12; the four refined
lists within max(16 gap, 1e-12) of the script's, gap being what the generator measured between the float64 restatement and the script."""
import builtins

import numpy as np
import pytest

import heightpitch_cases as hc

pytestmark = pytest.mark.gpu

FLOATS = ("ransac_height", "refined_pitch", "refined_mean", "refined_std", "height_t_mean")
_REF = {}


def pos_for(f, H):
    pos = np.full((H, 3), -1, dtype=np.int32)
    if f.positions is not None:
        k = min(H, len(f.positions))
        pos[:k] = f.positions[:k]
    return pos


def ref_for(f, H, positions=None):
    key = (f.name, H, None if positions is None else positions.tobytes())
    if key not in _REF:
        _REF[key] = hc.reference(f.pts, f.rows, f.est, pos_for(f, H) if positions is None else positions)
        assert _REF[key]["decided"], f.name
    return _REF[key]


def run(frames, H=64, draw=None, max_feat=None):
    """One launch over `frames`.  draw: None — the frames' own positions; (seed, frame_base) — the device draws."""
    from mvoscalerecovery_amd.height_pitch import HeightPitchEstimator
    est = HeightPitchEstimator(max_iterations=H, seed=0 if draw is None else draw[0])
    return est.launch([f.pts for f in frames], [hc.prior_of(f.est) for f in frames], triples=None if draw is not None else [pos_for(f, H) for f in frames],
                      tris=[f.rows for f in frames], frame_base=0 if draw is None else draw[1], stage=True, max_feat=max_feat)


def unfitted(res, i, status, n_selected):
    assert int(res["status"][i]) == status and int(res["n_selected"][i]) == n_selected, (i, res["status"][i], res["n_selected"][i])
    assert all(np.isnan(res[k][i]) for k in FLOATS) and np.isnan(res["model"][i]).all() and np.isnan(res["refined_normal"][i]).all()
    assert int(res["best_ic"][i]) == 0 and int(res["n_inliers"][i]) == 0 and not res["mask"][i].any()


def check(res, i, f, ref, H):
    name = f.name
    if ref["status"] != 0:
        unfitted(res, i, ref["status"], ref["n_selected"])
        assert res["point_list"][i].tobytes() == ref["ids"].tobytes(), name
        return
    assert int(res["status"][i]) == 0 and int(res["n_selected"][i]) == ref["n_selected"], (name, res["status"][i], res["n_selected"][i])
    assert res["point_list"][i].tobytes() == ref["ids"].tobytes(), name
    assert np.array_equal(res["hyp_counts"][i], ref["hyp_counts"]), (name, np.nonzero(res["hyp_counts"][i] != ref["hyp_counts"])[0][:8])
    assert (int(res["best_ic"][i]), int(res["used"][i])) == (ref["best_ic"], ref["used"]), name
    assert int(res["n_inliers"][i]) == ref["n_inliers"] and np.array_equal(res["mask"][i], ref["mask"]), name
    assert np.all(np.abs(res["model"][i] - ref["model"]) <= ref["model_tol"]), (name, res["model"][i], ref["model"])
    assert abs(res["ransac_height"][i] - ref["ransac_height"]) <= ref["ransac_height_tol"] * abs(ref["ransac_height"]), name
    if ref["n_inliers"] >= 3:
        assert np.all(np.abs(res["refined_normal"][i] - ref["refined_normal"]) <= ref["refined_normal_tol"]), name
        for k in FLOATS[1:]:
            assert abs(res[k][i] - ref[k]) <= ref[k + "_tol"], (name, k, res[k][i], ref[k], ref[k + "_tol"])


def run_and_check(names, H=64):
    c = hc.crafted()
    frames = [c[n] for n in names]
    res = run(frames, H)
    for i, f in enumerate(frames):
        check(res, i, f, ref_for(f, H), H)
    return res


def test_empty_and_single_row_frames():
    c = hc.crafted()
    res = run([c["empty"], c["one_row"]])
    unfitted(res, 0, hc.ST_EMPTY, 0)
    unfitted(res, 1, hc.ST_RS_FEW, 3)
    assert res["point_list"][1].tolist() == c["one_row"].rows[0].tolist()


def test_min_points_boundary():
    res = run_and_check(["rows3", "rows4"])                               # 9 list points: carried; 12: fitted (:140)
    assert res["status"].tolist() == [hc.ST_RS_FEW, 0] and res["n_selected"].tolist() == [9, 12]


def test_wave_tails_and_point_list_across_wavefronts():
    run_and_check(["tail65", "tail129", "big300"])


def test_prior_window_edges():
    res = run_and_check(["prior-2", "prior+0", "prior+2", "prior+6"])
    assert res["n_selected"].tolist() == [18, 18, 18, 21]                 # one of each pair at 2 margins from an edge is kept


def test_negative_height_is_excluded():
    res = run_and_check(["neg_height"])
    assert int(res["n_selected"][0]) == 15


@pytest.mark.parametrize("H", hc.N_HYPS)
def test_hypothesis_counts(H):
    run_and_check(["tail129", "big300"], H)


def test_replay_edges():
    tie = run_and_check(["tie"], 3)
    assert int(tie["used"][0]) == 3 and int(tie["best_ic"][0]) == 3
    first = hc.planes_from(hc.back_project(hc.crafted()["tie"].pts), np.array([[0, 1, 2]]))[0]
    assert np.allclose(tie["model"][0], first if first[1] >= 0 else -first, rtol=1e-9)    # the FIRST of the equal counts
    res = run_and_check(["goal0", "never"])
    assert res["used"].tolist() == [1, 64]


def test_spent_samples():
    res = run_and_check(["spent"])
    assert not res["hyp_counts"][0][:6].any() and int(res["status"][0]) == 0


def test_inlier_placement():
    three = run_and_check(["three"], 8)
    assert int(three["n_inliers"][0]) == 3 and abs(three["refined_std"][0]) < 1e-12
    res = run_and_check(["wave0", "spread"])
    assert np.nonzero(res["mask"][0])[0][:3].tolist() == [3, 10, 40] and np.nonzero(res["mask"][1])[0][:3].tolist() == [1, 70, 260]


def test_refusals():
    c = hc.crafted()
    res = run([c["singular"], c["rows4"], c["badid"]])
    unfitted(res, 0, hc.ST_SINGULAR, 0)
    check(res, 1, c["rows4"], ref_for(c["rows4"], 64), 64)
    unfitted(res, 2, hc.ST_MASK, 0)
    res = run([c["rows4"], c["big300"], c["tail65"]], max_feat=len(c["tail65"].pts))     # feat_cnt > max_feat
    check(res, 0, c["rows4"], ref_for(c["rows4"], 64), 64)
    unfitted(res, 1, hc.ST_MASK, 0)
    check(res, 2, c["tail65"], ref_for(c["tail65"], 64), 64)


def test_ragged_batch_is_bytewise_the_single_frames():
    c = hc.crafted()
    frames = [c[n] for n in ("empty", "rows4", "empty", "tail65", "one_row", "big300", "empty")]
    a, b = run(frames), run(frames)
    keys = [k for k in a if k != "rows"]
    for i, f in enumerate(frames):
        alone = run([f])
        for k in keys:
            x, y, z = (np.ascontiguousarray(r[k][j]) for r, j in ((a, i), (b, i), (alone, 0)))
            assert x.tobytes() == y.tobytes() == z.tobytes(), (f.name, k)
        if f.name != "empty":
            check(a, i, f, ref_for(f, 64), 64)


def test_device_draw_is_the_documented_sequence():
    c = hc.crafted()
    frames = [c["tail129"], c["big300"]]
    seed, base, H = 77, 5, 64
    res = run(frames, H, draw=(seed, base))
    for i, f in enumerate(frames):
        M = ref_for(f, H)["n_selected"]
        pos = hc.draw_positions(seed, base + i, H, M)
        check(res, i, f, ref_for(f, H, pos), H)


# ---- the reference's own run ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return hc.load_golden()


def test_golden_sequence(golden):
    from mvoscalerecovery_amd.height_pitch import HeightPitchEstimator
    g = golden["seq"]
    est = HeightPitchEstimator(seed=0)
    res = est.launch(g["frames"], [hc.prior_of(e) for e in g["priors"]], triples=g["positions"], tris=g["rows"], stage=True)
    assert not res["status"].any()
    assert res["n_selected"].tolist() == g["suitable"].tolist()
    assert res["n_inliers"].tolist() == g["inlier_numbers"].astype(int).tolist()
    for i in range(len(g["frames"])):
        assert int(res["best_ic"][i]) == int(g["best_ic"][i]) and np.array_equal(res["mask"][i], g["mask"][i]), i
        np.testing.assert_allclose(res["model"][i], g["model"][i], rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(res["ransac_height"], g["ransac_camera_heights"], rtol=1e-9, atol=0)
    worst = {}
    for key, field in (("refined_camera_height_means", "refined_mean"), ("refined_camera_height_stds", "refined_std"),
                       ("refined_camera_height_t_means", "height_t_mean"), ("refined_pitchs", "refined_pitch")):
        tol = max(16 * g["meta"]["gaps"]["gap_" + field], 1e-12)
        worst[field] = (float(np.max(np.abs(res[field] - g[key]) / np.abs(g[key]))), tol)
        print("heightpitch golden %s: largest relative difference %.3e, allowed %.3e" % (field, *worst[field]))
    for field, (w, tol) in worst.items():
        assert w <= tol, (field, w, tol)


def _assert_lists(est, g):
    got = est.result_arrays()
    np.testing.assert_allclose(got[0], g["ransac_camera_heights"], rtol=1e-9, atol=0)
    assert got[5].tolist() == g["inlier_numbers"].astype(int).tolist()
    for k, (key, field) in zip((1, 2, 3, 4), (("refined_camera_height_means", "refined_mean"), ("refined_camera_height_stds", "refined_std"),
                                               ("refined_camera_height_t_means", "height_t_mean"), ("refined_pitchs", "refined_pitch"))):
        tol = max(16 * g["meta"]["gaps"]["gap_" + field], 1e-12)
        assert np.all(np.abs(got[k] - g[key]) <= tol * np.abs(g[key])), (key, got[k], g[key])


def test_estimator_carries_a_frame_with_too_few_points(golden, tmp_path):
    from mvoscalerecovery_amd import height_pitch as hp
    g = golden["carry"]
    est = hp.HeightPitchEstimator(seed=0)
    out = est.process_batch(g["frames"], g["priors"], triples=g["positions"], tris=g["rows"])
    assert [r.carried for r in out] == [False, True, False] and [r.n_selected for r in out] == g["suitable"].tolist()
    _assert_lists(est, g)
    # frame by frame, as the script's loop goes: the same lists
    one = hp.HeightPitchEstimator(seed=0)
    for i in range(3):
        one.process_batch([g["frames"][i]], [g["priors"][i]], triples=[g["positions"][i]], tris=[g["rows"][i]])
    assert all(np.array_equal(a, b) for a, b in zip(one.result_arrays(), est.result_arrays()))
    est.write_results(str(tmp_path))
    for name, arr in zip(hp.RESULT_FILES, est.result_arrays()):
        assert np.array_equal(np.loadtxt(tmp_path / name), arr.astype(np.float64)), name


def test_estimator_first_frame_with_too_few_points_raises(golden):
    from mvoscalerecovery_amd.height_pitch import HeightPitchEstimator
    g = golden["first"]
    with pytest.raises(getattr(builtins, g["meta"]["error"])):
        HeightPitchEstimator(seed=0).process(g["frames"][0], g["priors"][0])


def test_singular_frame_raises_linalgerror():
    from mvoscalerecovery_amd.height_pitch import HeightPitchEstimator
    f = hc.crafted()["singular"]
    with pytest.raises(np.linalg.LinAlgError):
        HeightPitchEstimator(seed=0).process_batch([f.pts], [f.est], tris=[f.rows])


def test_gpu_triangulation_selects_the_same_points(golden):
    from mvoscalerecovery_amd.height_pitch import HeightPitchEstimator
    g = golden["seq"]
    frames, priors = g["frames"][:3], [hc.prior_of(e) for e in g["priors"][:3]]
    a = HeightPitchEstimator(seed=3, triangulation="scipy").launch(frames, priors, stage=True)
    b = HeightPitchEstimator(seed=3, triangulation="gpu").launch(frames, priors, stage=True)
    assert a["n_selected"].tolist() == b["n_selected"].tolist() == g["suitable"][:3].tolist()
    for i in range(3):
        assert np.array_equal(a["rows"][i], g["rows"][i])
        assert np.array_equal(np.sort(a["point_list"][i]), np.sort(b["point_list"][i]))
