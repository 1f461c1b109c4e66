"""GPU: mvosr_height_pitch_eval_batch (height_pitch_eval_kernel<plane>, <line>) and mvoscalerecovery_amd.height_pitch.RansacEvaluation on
crafted scenes and on the reference's own runs of /root/reference/src/calculate_height_pitch_eval.py and
calculate_height_pitch_eval_line.py (tests/golden/hpeval.npz).

Crafted scenes (tests/hpeval_cases.py; at most a few frames a launch, N <= 100 features, H <= 513, C <= 10): the np.longdouble
reference decides every integer output, sign and flag (tests/test_hpeval_cases.py asserts it on the CPU), so n_selected, the point
list, hyp_counts, best_ic, used, n_inliers (repeats counted), the list mask and the degenerate flag are demanded exactly, and the
model, the RANSAC height, the sums and the refined values within the reference's derived bounds (hpeval_cases.within).
A list has three entries per kept row, so M is a multiple of 3: the register chunk of 512 x 8 entries is met at M = 4092 / 4095 /
4098 and the mask's words at M = 189 / 192 / 195 — the reachable neighbours of 4096 and of a multiple of 64.
Golden leg: integers and the RANSAC height on every (frame, case) pair, the integers exactly and the heights to rtol 1e-9; the four
refined lists within max(16 gap, 1e-12) of the scripts', gap being what the generator measured between the float64 restatement and
the script, on every fitted pair that is not flagged degenerate."""
import builtins

import numpy as np
import pytest

import heightpitch_cases as hc
import hpeval_cases as he

pytestmark = pytest.mark.gpu

DOUBLES = ("ransac_height", "refined_pitch", "refined_mean", "refined_std", "height_t_mean", "sum_y", "sum_z")


def sliced(s, C, H):
    """Scene s with its first C cases and H hypotheses (its reference is computed for exactly those positions)."""
    t = he.Scene.__new__(he.Scene)
    t.__dict__.update(s.__dict__)
    t.positions = np.ascontiguousarray(s.positions[:C, :H])
    t.name = "%s[%d,%d]" % (s.name, C, H)
    return t


def run(model, scenes, G=None, draw=None, max_feat=None):
    """One launch over `scenes` (the same C and H).  draw: None — the scenes' own positions; (seed, frame_base) — the device draws."""
    from mvoscalerecovery_amd.height_pitch import RansacEvaluation
    C, H = scenes[0].positions.shape[:2]
    assert all(s.positions.shape[:2] == (C, H) for s in scenes)
    ev = RansacEvaluation(model, H, cases=C, seed=0 if draw is None else draw[0], cases_per_group=G)
    mf = [s.max_feat for s in scenes if s.max_feat]
    return ev.launch([s.pts for s in scenes], [hc.prior_of(s.est) for s in scenes], samples=None if draw is not None else [s.positions for s in scenes],
                     tris=[s.rows for s in scenes], frame_base=0 if draw is None else draw[1], stage=True,
                     max_feat=max_feat if max_feat is not None else (max(mf) if mf else None))


def unfitted(res, i, status, n_selected):
    assert np.all(res["status"][i] == status) and int(res["n_selected"][i]) == n_selected, (i, res["status"][i], res["n_selected"][i])
    assert all(np.isnan(res[k][i]).all() for k in DOUBLES) and np.isnan(res["model"][i]).all() and np.isnan(res["refined_normal"][i]).all()
    assert not res["best_ic"][i].any() and not res["n_inliers"][i].any() and not res["list_mask"][i].any()


def device_case(res, i, c):
    d = {k: res[k][i][c] for k in DOUBLES + ("best_ic", "used", "n_inliers", "model", "refined_normal", "hyp_counts")}
    d.update(n_selected=int(res["n_selected"][i]), ids=res["point_list"][i], list_mask=res["list_mask"][i][c],
             degenerate=bool(res["status"][i][c] & he.ST_DEGENERATE))
    return d


def check(res, i, model, s, positions=None):
    """Frame i of a launch against scene s' references, case by case."""
    C = res["status"].shape[1]
    for c in range(C):
        ref = he.ref_for(model, s, c, None if positions is None else positions[c])
        assert ref["decided"], (s.name, c)
        if ref["status"] == he.ST_RS_FEW:
            unfitted(res, i, he.ST_RS_FEW, ref["n_selected"])
            assert res["point_list"][i].tobytes() == ref["ids"].tobytes(), s.name
            continue
        assert int(res["status"][i][c]) == ref["status"], (s.name, c, res["status"][i][c])
        he.within(device_case(res, i, c), ref, (model, s.name, c))


def run_and_check(model, names, G=None, C=None, H=None):
    cr = he.crafted()
    scenes = [cr[n] if C is None else sliced(cr[n], C, H) for n in names]
    res = run(model, scenes, G)
    for i, s in enumerate(scenes):
        check(res, i, model, s)
    return res


def same_bytes(a, b, i=None, j=None, what=""):
    for k in a:
        if k in ("rows", "kernel_ms"):
            continue
        x, y = (a[k] if i is None else a[k][i]), (b[k] if j is None else b[k][j])
        if isinstance(x, list):
            assert all(np.ascontiguousarray(p).tobytes() == np.ascontiguousarray(q).tobytes() for p, q in zip(x, y)), (what, k)
        else:
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, k)


@pytest.mark.parametrize("model", he.MODELS)
def test_min_points_boundary(model):
    res = run_and_check(model, ["few9", "min12"])                        # 9 list points: carried; 12: fitted (:159)
    assert res["n_selected"].tolist() == [9, 12] and np.all(res["status"][0] == he.ST_RS_FEW) and not (res["status"][1] & ~he.ST_DEGENERATE).any()


@pytest.mark.parametrize("model", he.MODELS)
@pytest.mark.parametrize("H", [1, 63, 64, 65])
def test_hypothesis_counts_inside_a_tile(model, H):
    run_and_check(model, ["mix60"], C=3, H=H)


@pytest.mark.parametrize("model", he.MODELS)
def test_one_full_tile(model):
    res = run_and_check(model, ["tile512"])
    assert res["used"].tolist() == [[512]]


@pytest.mark.parametrize("model", he.MODELS)
def test_replay_state_is_carried_across_tiles(model):
    res = run_and_check(model, ["goal_late", "best_first_tile", "best_second_tile"])     # H = 513
    assert np.all(res["used"] == 513)
    cr = he.crafted()
    first, second = he.ref_for(model, cr["best_first_tile"], 0), he.ref_for(model, cr["best_second_tile"], 0)
    assert int(res["best_ic"][1][0]) == first["hyp_counts"][3] > first["hyp_counts"][512] > 0
    assert int(res["best_ic"][2][0]) == second["hyp_counts"][512] > second["hyp_counts"][3] > 0
    assert np.all(res["best_ic"][0] > 0.8 * cr["goal_late"].M)                            # the stop at hypothesis 512, the second tile's first


@pytest.mark.parametrize("model", he.MODELS)
def test_single_hypothesis(model):
    res = run_and_check(model, ["h1"])
    assert np.all(res["used"] == 1)


@pytest.mark.parametrize("model", he.MODELS)
@pytest.mark.parametrize("name,C,groups", [("cases10", 10, (1, 2, 3, 10)), ("mix60", 3, (1, 2, 3)), ("tile512", 1, (1,))])
def test_results_do_not_depend_on_cases_per_group(model, name, C, groups):
    s = he.crafted()[name]
    base = run(model, [s], G=None)                                       # the launcher's default
    check(base, 0, model, s)
    for G in groups:                                                     # (10 by 3 and 3 by 2: a tail group)
        same_bytes(base, run(model, [s], G=G), what=(name, G))


@pytest.mark.parametrize("model", he.MODELS)
def test_mask_words(model):
    res = run_and_check(model, ["words189", "words192", "words195"])
    assert res["n_selected"].tolist() == [189, 192, 195]


@pytest.mark.parametrize("model", he.MODELS)
def test_register_chunk_of_4096_entries(model):
    res = run_and_check(model, ["chunk4092", "chunk4095", "chunk4098"])
    assert res["n_selected"].tolist() == [4092, 4095, 4098]


@pytest.mark.parametrize("model", he.MODELS)
def test_inliers_at_the_lists_ends(model):
    res = run_and_check(model, ["inliers_first", "inliers_last"])
    M = he.crafted()["inliers_last"].M
    assert np.nonzero(res["list_mask"][0][0])[0].tolist() == [0, 1, 2] and np.nonzero(res["list_mask"][1][0])[0].tolist() == [M - 3, M - 2, M - 1]
    assert res["n_inliers"].tolist() == [[3], [3]]


@pytest.mark.parametrize("model", he.MODELS)
def test_refinement_sample_over_two_wavefronts_segments(model):
    res = run_and_check(model, ["straddle"])
    assert np.nonzero(res["list_mask"][0][0])[0][:2].tolist() == [191, 192] and not res["status"].any()


@pytest.mark.parametrize("model", he.MODELS)
def test_degenerate_refinement_sample(model):
    res = run_and_check(model, ["degenerate"])
    assert np.all(res["status"][0] == he.ST_DEGENERATE)
    assert np.all(np.isfinite(res["ransac_height"])) and np.all(res["n_inliers"] > 3) and np.all(np.isfinite(res["sum_y"]))
    assert all(np.isnan(res[k]).all() for k in he.REFINED) and np.isnan(res["refined_normal"]).all()


@pytest.mark.parametrize("model", he.MODELS)
def test_spent_samples(model):
    res = run_and_check(model, ["spent"])
    assert not res["hyp_counts"][0][:, :6].any() and np.all(res["hyp_counts"][0][:, 6] > 0) and not (res["status"] & ~he.ST_DEGENERATE).any()


def test_line_models_of_both_signs():
    res = run_and_check("line", ["mix60", "neg"], C=3, H=64)
    assert np.all(res["ransac_height"][0] > 0) and np.all(res["ransac_height"][1] < 0)    # b < 0 flips (a, b) and h_bar: reproduced
    assert np.all(res["model"][:, :, 1] > 0) and np.all(res["model"][:, :, 2] == 0)
    plane = run_and_check("plane", ["neg"], C=3, H=64)
    assert np.all(plane["ransac_height"] > 0)


@pytest.mark.parametrize("model", he.MODELS)
def test_ragged_batch_is_bytewise_the_single_frames(model):
    cr = he.crafted()
    scenes = [sliced(cr[n], 2, 8) for n in ("empty", "min12", "empty", "cases10", "few9", "words192", "empty")]
    a, b = run(model, scenes), run(model, scenes)
    same_bytes(a, b, what="run to run")
    for i, s in enumerate(scenes):
        alone = run(model, [s])
        same_bytes(a, alone, i, 0, what=s.name)
        if not s.name.startswith("empty"):
            check(a, i, model, s)


@pytest.mark.parametrize("model", he.MODELS)
def test_device_draw_is_the_documented_sequence_and_splits_with_frame_base(model):
    cr = he.crafted()
    scenes = [sliced(cr[n], 3, 24) for n in ("mix60", "neg", "cases10")]
    seed, base = 77, 5
    whole = run(model, scenes, draw=(seed, base))
    for i, s in enumerate(scenes):
        pos = np.stack([he.draw_positions(model, seed, base + i, c, 24, s.M) for c in range(3)])
        check(whole, i, model, s, positions=pos)
    head, tail = run(model, scenes[:1], draw=(seed, base)), run(model, scenes[1:], draw=(seed, base + 1), G=2)
    same_bytes(whole, head, 0, 0, what="head")
    for i in (1, 2):
        same_bytes(whole, tail, i, i - 1, what="tail %d" % i)
    assert not np.array_equal(whole["hyp_counts"][0][0], whole["hyp_counts"][0][1])      # the cases draw differently


@pytest.mark.parametrize("model", he.MODELS)
def test_refusals(model):
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.height_pitch import RansacEvaluation
    cr = he.crafted()
    ok = sliced(cr["min12"], 2, 8)
    res = run(model, [cr["singular"], ok, cr["badid"], cr["empty"]], G=1)
    unfitted(res, 0, he.ST_SINGULAR, 0)
    check(res, 1, model, ok)
    unfitted(res, 2, he.ST_MASK, 0)
    unfitted(res, 3, he.ST_EMPTY, 0)
    big = sliced(cr["mix60"], 2, 8)
    res = run(model, [ok, big, ok], max_feat=len(ok.pts))                 # feat_cnt > max_feat
    check(res, 0, model, ok)
    unfitted(res, 1, he.ST_MASK, 0)
    check(res, 2, model, ok)
    with pytest.raises(ValueError):
        RansacEvaluation(model, 4097)
    with pytest.raises(ValueError):
        RansacEvaluation("circle", 10)
    ev = RansacEvaluation(model, 8, cases=2)
    ev.iterations = 4097                                                 # past the constructor: the C entry point refuses
    with pytest.raises(_lib.MvosrLibraryError):
        ev.launch([ok.pts], [hc.prior_of(0.0)], tris=[ok.rows])
    ev.iterations, ev.cases_per_group = 8, -1
    with pytest.raises(_lib.MvosrLibraryError):
        ev.launch([ok.pts], [hc.prior_of(0.0)], tris=[ok.rows])


# ---- the reference's own runs -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return he.load_golden()


def evaluate(model, g, **kw):
    from mvoscalerecovery_amd.height_pitch import RansacEvaluation
    ev = RansacEvaluation(model, g["meta"]["iterations"], cases=10, seed=0, **kw)
    out = ev.run(g["frames"], g["motion"][:, 3::4], samples=[None if p is None else p.astype(np.int32) for p in g["positions"]], tris=g["rows"])
    return ev, out


def expected_degenerate(model, g):
    K = he.K_of(model)
    deg, prev = np.zeros((10, len(g["frames"])), dtype=bool), None
    for i in range(len(g["frames"])):
        if g["mask"][i] is not None:
            ids = hc.select(hc.back_project(g["frames"][i]), g["rows"][i].astype(np.int64), g["priors"][i])[1]
            prev = np.array([he.degenerate(model, ids[g["mask"][i][c]]) for c in range(10)])
        if len(g["frames"][i]) and prev is not None:
            deg[:, i] = prev                                             # (a carried frame repeats its predecessor's inliers)
    return deg


def assert_run(model, g, ev, out):
    assert out["n_inliers"].astype(int).tolist() == g["n_inliers"].astype(int).tolist()
    np.testing.assert_allclose(out["ransac_height"], g["ransac_height"], rtol=1e-9, atol=0)       # every pair, none left out
    deg = expected_degenerate(model, g)
    assert np.array_equal(ev.degenerate, deg)
    fitted = np.array([len(d) > 0 for d in g["frames"]])[None, :] & np.ones((10, 1), bool)
    compare = fitted & ~deg
    assert compare.sum() >= (0.9 if model == "line" else 0.6) * fitted.sum()
    for k in he.REFINED:
        tol = max(16 * g["run"]["gaps"]["gap_" + k], 1e-12)
        worst = float(np.max(np.abs(out[k][compare] - g[k][compare]) / np.abs(g[k][compare])))
        print("hpeval golden %s %s: largest relative difference %.3e, allowed %.3e" % (model, k, worst, tol))
        assert worst <= tol, (k, worst, tol)
        assert np.isnan(out[k][fitted & deg]).all() and np.all(out[k][~fitted] == 0)


@pytest.mark.parametrize("model", he.MODELS)
def test_golden_sequence(golden, model, tmp_path):
    from mvoscalerecovery_amd import height_pitch as hp
    g = golden[model]["seq"]
    ev, out = evaluate(model, g)
    assert_run(model, g, ev, out)
    assert ev.last["n_selected"].tolist() == g["suitable"].tolist() and not ev.carried.any()
    for i in range(len(g["frames"])):                                    # the staged integers of the last launch's frames
        assert ev.last["best_ic"][i].tolist() == g["best_ic"][i].tolist(), i
        np.testing.assert_allclose(ev.last["model"][i], g["model"][i], rtol=1e-8, atol=1e-12)
    if model == "line":
        assert np.any(out["ransac_height"] < 0)
    # the sixty files under the scripts' own names
    m = golden["meta"]
    paths = ev.write_results(str(tmp_path), m["input_id"], m["input_date"])
    assert sorted(str(tmp_path / n) for n in g["run"]["files"]) == sorted(paths) and len(paths) == 60
    names = hp.eval_file_names(model, m["input_id"], m["input_date"], g["meta"]["iterations"])
    for c in range(10):
        for j, k in enumerate(hp.RESULT_FIELDS):
            assert np.array_equal(np.loadtxt(tmp_path / names[6 * c + j]), out[k][c], equal_nan=True)
    sp = ev.spread()
    assert set(sp) == set(hp.RESULT_FIELDS)
    np.testing.assert_allclose(sp["ransac_height"][0], out["ransac_height"].mean(0), rtol=1e-15)
    np.testing.assert_allclose(sp["ransac_height"][1], out["ransac_height"].std(0), rtol=1e-12)
    assert sp["refined_pitch"][0].shape == (len(g["frames"]),) and np.all(np.isfinite(sp["n_inliers"][1]))


@pytest.mark.parametrize("model", he.MODELS)
def test_staged_list_mask_is_the_scripts(golden, model):
    from mvoscalerecovery_amd.height_pitch import RansacEvaluation
    g = golden[model]["seq"]
    ev = RansacEvaluation(model, g["meta"]["iterations"], cases=10, seed=0)
    res = ev.launch(g["frames"][:3], [hc.prior_of(e) for e in g["priors"][:3]], samples=[p.astype(np.int32) for p in g["positions"][:3]],
                    tris=g["rows"][:3], stage=True)
    for i in range(3):
        assert np.array_equal(res["list_mask"][i], g["mask"][i]), i
        assert res["n_inliers"][i].tolist() == g["mask"][i].sum(1).tolist()


@pytest.mark.parametrize("model", he.MODELS)
def test_evaluation_carries_a_frame_with_too_few_points(golden, model):
    g = golden[model]["carry"]
    ev, out = evaluate(model, g)
    assert ev.carried.tolist() == [False, True, False]
    assert_run(model, g, ev, out)
    assert np.array_equal(out["ransac_height"][:, 1], out["ransac_height"][:, 0]) and np.array_equal(out["n_inliers"][:, 1], out["n_inliers"][:, 0])
    ok = ~ev.degenerate[:, 0]
    assert np.all(out["height_t_mean"][ok, 1] != out["height_t_mean"][ok, 0])             # the new prior
    # frame by frame batches: the same arrays
    ev1, out1 = evaluate(model, g, cases_per_group=3)
    ev1.run(g["frames"], g["motion"][:, 3::4], samples=[None if p is None else p.astype(np.int32) for p in g["positions"]], tris=g["rows"], batch=1)
    assert all(np.array_equal(ev1.results[k], out[k], equal_nan=True) for k in out)


@pytest.mark.parametrize("model", he.MODELS)
def test_evaluation_empty_dump_gives_zeros_and_keeps_the_state(golden, model):
    g = golden[model]["empty"]
    ev, out = evaluate(model, g)
    assert_run(model, g, ev, out)
    assert all(not out[k][:, 1].any() for k in out) and not ev.carried.any()


@pytest.mark.parametrize("model", he.MODELS)
def test_evaluation_first_frame_with_too_few_points_raises(golden, model):
    g = golden[model]["first"]
    with pytest.raises(getattr(builtins, g["run"]["error"])):
        evaluate(model, g)


def test_singular_frame_raises_linalgerror():
    from mvoscalerecovery_amd.height_pitch import RansacEvaluation
    s = he.crafted()["singular"]
    mot = hc.motions(3, 3)
    with pytest.raises(np.linalg.LinAlgError):
        RansacEvaluation("plane", 8, cases=2, seed=0).run([s.pts], mot[:, 3::4], tris=[s.rows])


def test_gpu_triangulation_selects_the_same_points(golden):
    from mvoscalerecovery_amd.height_pitch import RansacEvaluation
    g = golden["line"]["seq"]
    frames, priors = g["frames"][:2], [hc.prior_of(e) for e in g["priors"][:2]]
    a = RansacEvaluation("line", 20, cases=2, seed=3, triangulation="scipy").launch(frames, priors, stage=True)
    b = RansacEvaluation("line", 20, cases=2, seed=3, triangulation="gpu").launch(frames, priors, stage=True)
    assert a["n_selected"].tolist() == b["n_selected"].tolist() == g["suitable"][:2].tolist()
    for i in range(2):
        assert np.array_equal(np.sort(a["point_list"][i]), np.sort(b["point_list"][i]))
