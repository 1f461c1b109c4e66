"""GPU: mvosr_height_pitch_eval_budgets_batch (height_pitch_eval_budgets_kernel<plane>, <line>) and
mvoscalerecovery_amd.height_pitch.RansacBudgetSweep — the RANSAC evaluation at every iteration budget of a list from one launch.

The contract is bytewise: slot [f][c][k] of every output the entry point shares with mvosr_height_pitch_eval_batch holds what that
entry point writes at [f][c] with n_hyp = budgets[k] (tests/hpeval_budgets_cases.py: the budget lists).  So every test runs one
budgets launch and the single launches it stands in for and compares `tobytes`; on the crafted lists every slot is also held
against the np.longdouble reference of its budget (hpeval_cases.within: integers, `best`, status and the degenerate flag exactly,
doubles within the reference's own bounds) — the entry point has no list mask, so the mask handed to `within` is restated from the
slot's OWN model in float64 (the reference decides every entry, so a right model gives the reference's mask).
Crafted frames have at most 100 features (the chunk scenes 700) and a launch a few frames."""
import builtins

import numpy as np
import pytest

import heightpitch_cases as hc
import hpeval_budgets_cases as hb
import hpeval_cases as he
from test_gpu_hpeval import assert_run, sliced

pytestmark = pytest.mark.gpu


def cut(s, C=None, H=None):
    C, H = s.positions.shape[0] if C is None else C, s.positions.shape[1] if H is None else H
    return sliced(s, C, H)


def launch_args(scenes, budget, draw, max_feat):
    mf = [s.max_feat for s in scenes if s.max_feat]
    return dict(points3d_list=[s.pts for s in scenes], priors=[hc.prior_of(s.est) for s in scenes],
                samples=None if draw is not None else [s.positions[:, :budget] for s in scenes], tris=[s.rows for s in scenes],
                frame_base=0 if draw is None else draw[1], stage=True, max_feat=max_feat if max_feat is not None else (max(mf) if mf else None))


def sweep(model, scenes, budgets, G=None, draw=None, max_feat=None, stage=True):
    """One budgets launch over `scenes` (the same C).  draw: None — the scenes' own positions; (seed, frame_base) — the device draws."""
    from mvoscalerecovery_amd.height_pitch import RansacBudgetSweep
    C = scenes[0].positions.shape[0]
    assert all(s.positions.shape[0] == C and s.positions.shape[1] >= budgets[-1] for s in scenes)
    sw = RansacBudgetSweep(model, budgets, cases=C, seed=0 if draw is None else draw[0], cases_per_group=G)
    kw = launch_args(scenes, budgets[-1], draw, max_feat)
    kw["stage"] = stage
    return sw.launch(**kw)


def single(model, scenes, budget, G=None, draw=None, max_feat=None):
    """The launch of mvosr_height_pitch_eval_batch the slot of `budget` stands in for: the first `budget` samples."""
    from mvoscalerecovery_amd.height_pitch import RansacEvaluation
    ev = RansacEvaluation(model, budget, cases=scenes[0].positions.shape[0], seed=0 if draw is None else draw[0], cases_per_group=G)
    return ev.launch(**launch_args(scenes, budget, draw, max_feat))


def tb(x):
    return np.ascontiguousarray(x).tobytes()


def assert_slot_is_the_single_launch(sw, k, one, what="", frames=None, one_frames=None):
    """Slot k of frames `frames` of a budgets launch against frames `one_frames` of a single launch, byte for byte."""
    F = len(sw["n_selected"])
    frames = list(range(F)) if frames is None else frames
    one_frames = frames if one_frames is None else one_frames
    for i, j in zip(frames, one_frames):
        for key in hb.SHARED:
            assert tb(sw[key][i][:, k]) == tb(one[key][j]), (what, key, i, k, sw[key][i][:, k], one[key][j])
        assert int(sw["n_selected"][i]) == int(one["n_selected"][j]) and tb(sw["point_list"][i]) == tb(one["point_list"][j]), (what, i, k)


def assert_sweep_is_the_single_launches(model, scenes, budgets, sw=None, singles=None, **kw):
    sw = sweep(model, scenes, budgets, **kw) if sw is None else sw
    for k, b in enumerate(budgets):
        one = single(model, scenes, b, **kw) if singles is None or b not in singles else singles[b]
        if singles is not None:
            singles[b] = one
        assert_slot_is_the_single_launch(sw, k, one, what=(model, [s.name for s in scenes], b))
    assert tb(sw["hyp_counts"]) == tb(one["hyp_counts"])                             # the counts are the last budget's
    return sw


def same_launch(a, b, i=None, j=None, what=""):
    for k in a:
        if k in ("rows", "kernel_ms"):
            continue
        x, y = (a[k] if i is None else a[k][i]), (b[k] if j is None else b[k][j])
        if isinstance(x, list):
            assert all(tb(p) == tb(q) for p, q in zip(x, y)), (what, k)
        else:
            assert tb(x) == tb(y), (what, k)


def slot_unfitted(sw, i, status, n_selected, used=0):
    """Every slot of every case of frame i holds the refusal outputs of include/mvosr.h."""
    assert np.all(sw["status"][i] == status) and int(sw["n_selected"][i]) == n_selected, (i, sw["status"][i], sw["n_selected"][i])
    assert all(np.isnan(sw[k][i]).all() for k in hb.DOUBLES) and np.isnan(sw["model"][i]).all() and np.isnan(sw["refined_normal"][i]).all()
    assert not sw["best_ic"][i].any() and not sw["n_inliers"][i].any() and np.all(sw["best"][i] == -1) and np.all(sw["used"][i] == used)


def check_against_reference(sw, i, model, s, budgets):
    """Frame i of a budgets launch with scene s' own positions: every (case, budget) slot against its reference."""
    P = hc.back_project(s.pts)
    n = 0
    for c in range(sw["status"].shape[1]):
        for k, b in enumerate(budgets):
            ref = hb.ref_at(model, s, c, b)
            assert ref["decided"], (s.name, c, b)
            n += 1
            assert int(sw["n_selected"][i]) == ref["n_selected"] and tb(sw["point_list"][i]) == tb(ref["ids"]), (s.name, c, b)
            if ref["status"] == he.ST_RS_FEW:                                        # no model among the first b hypotheses
                assert int(sw["status"][i][c, k]) == he.ST_RS_FEW and int(sw["best"][i][c, k]) == -1 and int(sw["used"][i][c, k]) == b, (s.name, c, b)
                assert all(np.isnan(sw[q][i][c, k]) for q in hb.DOUBLES) and np.isnan(sw["model"][i][c, k]).all() and np.isnan(sw["refined_normal"][i][c, k]).all()
                assert int(sw["best_ic"][i][c, k]) == 0 and int(sw["n_inliers"][i][c, k]) == 0
                assert not sw["hyp_counts"][i][c, :b].any()
                continue
            assert int(sw["status"][i][c, k]) == ref["status"] and int(sw["best"][i][c, k]) == ref["best"], (s.name, c, b, sw["best"][i][c, k], ref["best"])
            d = {q: sw[q][i][c, k] for q in hb.DOUBLES + ("best_ic", "used", "n_inliers", "model", "refined_normal")}
            with np.errstate(invalid="ignore"):
                mask = he.residuals(model, P[ref["ids"]], d["model"]) < he.INLIER_THRESHOLD
            d.update(n_selected=int(sw["n_selected"][i]), ids=sw["point_list"][i], hyp_counts=sw["hyp_counts"][i][c, :b], list_mask=mask,
                     degenerate=bool(sw["status"][i][c, k] & he.ST_DEGENERATE))
            assert int(mask.sum()) == int(d["n_inliers"]), (s.name, c, b)
            he.within(d, ref, (model, s.name, c, b))
    return n


# ---- 6, 7: the crafted lists, against the existing kernel bytewise and against the reference ---------------------------------
COUNTED = {}


@pytest.mark.parametrize("model", he.MODELS)
@pytest.mark.parametrize("name", list(hb.BUDGETS))
def test_every_slot_is_the_single_launch_and_within_the_reference(model, name):
    s, budgets = he.crafted()[name], hb.BUDGETS[name]
    s = cut(s, H=budgets[-1])
    sw = assert_sweep_is_the_single_launches(model, [s], budgets)
    COUNTED[(model, name)] = check_against_reference(sw, 0, model, he.crafted()[name], budgets)
    if len(COUNTED) == 2 * len(hb.BUDGETS):
        assert sum(COUNTED.values()) == hb.N_COMBINATIONS                            # none left out


# ---- 8: where a checkpoint may fall: the ends of a replay step, of a tile, of two tiles ---------------------------------------
NINE = (63, 64, 65, 511, 512, 513, 1023, 1024, 1025)
SIXTEEN = (1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1100)


@pytest.mark.parametrize("model", he.MODELS)
def test_checkpoints_at_the_ends_of_replay_steps_and_tiles(model):
    cr = he.crafted()
    scenes = [cut(cr["mix60"], C=3), cut(cr["cases10"], C=3)]
    for s in scenes:                                                                 # (the draw ignores them: the device draws)
        s.positions = np.zeros((3, SIXTEEN[-1], 3), np.int32)
    draw, singles = (77, 9), {}
    sw = assert_sweep_is_the_single_launches(model, scenes, NINE, singles=singles, draw=draw)
    assert np.all(sw["used"] <= np.array(NINE)) and np.all(np.diff(sw["best_ic"], axis=2) >= 0)
    for b in (65, 1025):                                                             # a list of one budget is the single run
        assert_sweep_is_the_single_launches(model, scenes, (b,), singles=singles, draw=draw)
    sw16 = assert_sweep_is_the_single_launches(model, scenes, SIXTEEN, singles=singles, draw=draw)
    for k, b in enumerate(NINE):                                                     # ... and does not depend on the other budgets
        for key in hb.SHARED + ("best",):
            assert tb(sw[key][:, :, k]) == tb(sw16[key][:, :, SIXTEEN.index(b)]), (key, b)


# ---- 9: a stop inside a segment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", he.MODELS)
def test_goal_stop_inside_a_segment_freezes_the_later_checkpoints(model):
    budgets = (4, 64, 300, 1000)
    s = cut(he.crafted()["goal_late"])                                               # 90 % of the entries on one plane
    s.positions = np.zeros((2, budgets[-1], 3), np.int32)
    draw = (77, 0)
    sw = assert_sweep_is_the_single_launches(model, [s], budgets, draw=draw)
    used, best = sw["used"][0], sw["best"][0]                                        # (C, B)
    stopped = used < np.array(budgets)
    print("goal stop:", model, "used", used.tolist(), "best", best.tolist())
    assert stopped.any()                                                             # the stop was met
    for c in range(used.shape[0]):
        ks = np.nonzero(stopped[c])[0]
        if not len(ks):
            continue
        k0 = int(ks[0])
        assert stopped[c, k0:].all() and np.all(used[c, k0:] == used[c, k0])          # `used` repeats too
        for k in range(k0 + 1, len(budgets)):                                        # all later checkpoints: equal but for nothing
            for key in hb.SHARED + ("best",):
                assert tb(sw[key][0][c, k]) == tb(sw[key][0][c, k0]), (key, c, k)
    # without hyp_counts the tiles behind the stop are skipped: the same bytes
    lean = sweep(model, [s], budgets, draw=draw, stage=False)
    for key in hb.SHARED + ("best", "n_selected"):
        assert tb(lean[key]) == tb(sw[key]), key


@pytest.mark.parametrize("model", he.MODELS)
@pytest.mark.parametrize("stop_at", [350, 700])
def test_recorded_stop_between_checkpoints_in_either_tile(model, stop_at):
    """The device draw stops at once on this scene; here the stop is planted: every sample spent but a weak one at 7 and a sample of
    the dominant plane at `stop_at` — inside the segment (300, 600] of the first tile, or (600, 1000] of the second."""
    budgets = (4, 64, 300, 600, 1000)
    g = he.crafted()["goal_late"]
    s = cut(g)
    s.positions = np.full((2, budgets[-1], 3), -1, np.int32)
    s.positions[:, 7] = g.positions[:, 7]
    s.positions[:, stop_at] = g.positions[:, 512]
    sw = assert_sweep_is_the_single_launches(model, [s], budgets)
    want_used = [min(b, stop_at + 1) for b in budgets]
    want_best = [-1 if b <= 7 else (7 if b <= stop_at else stop_at) for b in budgets]
    assert sw["used"][0].tolist() == [want_used] * 2 and sw["best"][0].tolist() == [want_best] * 2
    lean = sweep(model, [s], budgets, stage=False)                                   # the tiles behind the stop skipped
    for key in hb.SHARED + ("best", "n_selected"):
        assert tb(lean[key]) == tb(sw[key]), key


# ---- 10: the register chunk and the mask's words ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", he.MODELS)
@pytest.mark.parametrize("names,budgets", [(("chunk4092", "chunk4095", "chunk4098"), (1, 4, 8)), (("words189", "words192", "words195"), (1, 16, 32))])
def test_register_chunk_and_mask_words(model, names, budgets):
    cr = he.crafted()
    sw = assert_sweep_is_the_single_launches(model, [cr[n] for n in names], budgets)
    assert sw["n_selected"].tolist() == [int(n[5:]) for n in names]
    assert not (sw["status"][:, :, -1] & ~he.ST_DEGENERATE).any()                    # every frame has a model at the last budget


# ---- 11: independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", he.MODELS)
def test_results_do_not_depend_on_cases_per_group(model):
    s, budgets = he.crafted()["cases10"], hb.BUDGETS["cases10"]
    base = sweep(model, [s], budgets)                                                # the launcher's default
    for G in (1, 3, 10):                                                             # (10 by 3: a tail group)
        same_launch(base, sweep(model, [s], budgets, G=G), what=G)


@pytest.mark.parametrize("model", he.MODELS)
def test_ragged_batch_is_bytewise_the_single_frames(model):
    cr, budgets = he.crafted(), (1, 3, 8)
    scenes = [sliced(cr[n], 2, 8) for n in ("empty", "min12", "empty", "cases10", "few9", "words192", "empty")]
    a = sweep(model, scenes, budgets)
    same_launch(a, sweep(model, scenes, budgets), what="run to run")
    for i, s in enumerate(scenes):
        same_launch(a, sweep(model, [s], budgets), i, 0, what=s.name)
    slot_unfitted(a, 0, he.ST_EMPTY, 0)
    slot_unfitted(a, 4, he.ST_RS_FEW, 9)
    assert not (a["status"][[1, 3, 5], :, -1] & ~he.ST_DEGENERATE).any()


@pytest.mark.parametrize("model", he.MODELS)
def test_a_sequence_split_with_frame_base_is_the_whole(model):
    cr, budgets = he.crafted(), (5, 24, 70, 600)
    scenes = [cut(cr[n], C=3) for n in ("mix60", "neg", "cases10")]
    for s in scenes:
        s.positions = np.zeros((3, budgets[-1], 3), np.int32)
    seed, base = 77, 5
    whole = sweep(model, scenes, budgets, draw=(seed, base))
    head, tail = sweep(model, scenes[:1], budgets, draw=(seed, base)), sweep(model, scenes[1:], budgets, draw=(seed, base + 1), G=2)
    same_launch(whole, head, 0, 0, what="head")
    for i in (1, 2):
        same_launch(whole, tail, i, i - 1, what="tail %d" % i)
    assert not np.array_equal(whole["hyp_counts"][0][0], whole["hyp_counts"][0][1])  # the cases draw differently
    assert not np.array_equal(whole["hyp_counts"][0], sweep(model, scenes[:1], budgets, draw=(seed, base + 1))["hyp_counts"][0])


@pytest.mark.parametrize("model", he.MODELS)
def test_a_slot_does_not_depend_on_the_other_budgets(model):
    s = he.crafted()["mix60"]
    a, b = sweep(model, [cut(s, H=64)], (8, 64)), sweep(model, [s], (8, 33, 64, 65))
    for ka, kb in ((0, 0), (1, 2)):
        for key in hb.SHARED + ("best",):
            assert tb(a[key][:, :, ka]) == tb(b[key][:, :, kb]), (key, ka)
    assert tb(a["hyp_counts"]) == tb(b["hyp_counts"][:, :, :64])


# ---- 12: refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", he.MODELS)
def test_refusals(model):
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.height_pitch import RansacBudgetSweep
    cr, budgets = he.crafted(), (1, 3, 8)
    ok = sliced(cr["min12"], 2, 8)
    alone = sweep(model, [ok], budgets)
    assert not (alone["status"][0][:, -1] & ~he.ST_DEGENERATE).any()
    refused = [("singular", he.ST_SINGULAR, 0), ("badid", he.ST_MASK, 0), ("empty", he.ST_EMPTY, 0), ("few9", he.ST_RS_FEW, 9)]
    scenes = [ok]
    for name, _, _ in refused:
        scenes += [sliced(cr[name], 2, 8), ok]
    for G in (None, 2):
        res = sweep(model, scenes, budgets, G=G)
        for q, (name, status, n_sel) in enumerate(refused):
            slot_unfitted(res, 1 + 2 * q, status, n_sel)
        for i in range(0, len(scenes), 2):                                           # the neighbours: the launch without the refused frames
            same_launch(res, alone, i, 0, what=("neighbour", i))
    big = sliced(cr["mix60"], 2, 8)
    res = sweep(model, [ok, big, ok], budgets, max_feat=len(ok.pts))                 # feat_cnt > max_feat: refused before LDS is touched
    slot_unfitted(res, 1, he.ST_MASK, 0)
    for i in (0, 2):
        same_launch(res, alone, i, 0, what=("max_feat", i))
    # a bad list: at the constructor, and by the C entry point past it
    for bad in ([], [5, 5], [5, 3], [0, 4], [1, 4097], list(range(1, 18))):
        with pytest.raises(ValueError):
            RansacBudgetSweep(model, bad)
    with pytest.raises(ValueError):
        RansacBudgetSweep("circle", [10])
    kw = dict(points3d_list=[ok.pts], priors=[hc.prior_of(0.0)], tris=[ok.rows])
    sw = RansacBudgetSweep(model, [2, 8], cases=2)
    for bad in ((8, 2), (4, 4), (0, 8), (8, 4097), tuple(range(1, 18))):             # (n_budgets = 17 among them)
        sw.budgets = bad
        with pytest.raises(_lib.MvosrLibraryError):
            sw.launch(**kw)
    sw.budgets, sw.cases_per_group = (2, 8), -1
    with pytest.raises(_lib.MvosrLibraryError):
        sw.launch(**kw)
    sw.cases_per_group = 0
    assert sw.launch(**kw)["used"].shape == (1, 2, 2)


# ---- 13: the scripts' own runs ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return he.load_golden()


GOLDEN_BUDGETS = {"seq": (1, 2, 5, 10, 20, 40), "carry": (1, 2, 5, 10, 20), "empty": (1, 2, 5, 10, 20)}


def golden_samples(g, budget=None):
    return [None if p is None else p.astype(np.int32)[:, :budget] for p in g["positions"]]


def run_sweep(model, g, budgets, **kw):
    from mvoscalerecovery_amd.height_pitch import RansacBudgetSweep
    batch = kw.pop("batch", 512)
    sw = RansacBudgetSweep(model, budgets, cases=10, seed=0, **kw)
    out = sw.run(g["frames"], g["motion"][:, 3::4], samples=golden_samples(g), tris=g["rows"], batch=batch)
    return sw, out


@pytest.mark.parametrize("model", he.MODELS)
@pytest.mark.parametrize("case", ["seq", "carry", "empty"])
def test_golden_runs_row_by_row(golden, model, case, tmp_path):
    from mvoscalerecovery_amd import height_pitch as hp
    g, budgets = golden[model][case], GOLDEN_BUDGETS[case]
    own = budgets.index(g["meta"]["iterations"])                                     # the list holds the scripts' own budget
    sw, out = run_sweep(model, g, budgets)
    assert set(out) == set(hp.RESULT_FIELDS) and all(v.shape == (len(budgets), 10, len(g["frames"])) for v in out.values())
    for k, b in enumerate(budgets):
        ev = hp.RansacEvaluation(model, b, cases=10, seed=0)
        one = ev.run(g["frames"], g["motion"][:, 3::4], samples=golden_samples(g, b), tris=g["rows"])
        for f in hp.RESULT_FIELDS:
            assert np.array_equal(out[f][k], one[f], equal_nan=True), (f, b)
        assert np.array_equal(sw.carried, ev.carried) and np.array_equal(sw.degenerate[k], ev.degenerate), b
        at = sw.results_at(b)
        assert all(np.array_equal(at[f], one[f], equal_nan=True) for f in at)
    fitted = np.array([len(d) > 0 for d in g["frames"]]) & ~sw.carried
    assert np.all(sw.used[:, :, ~fitted] == 0) and np.all(sw.best[:, :, ~fitted] == -1)
    assert np.all(sw.best[:, :, fitted] >= 0) and np.all(sw.used[:, :, fitted] > 0)   # every fitted pair has a model at every budget
    assert np.all(sw.used <= np.array(budgets)[:, None, None])
    if case == "seq":
        differ = int(np.sum(sw.best[budgets.index(20)] != sw.best[-1]))
        print("hpeval budgets golden %s: the best model at budget 20 differs from budget 40's on %d of %d pairs" % (model, differ, sw.best[-1].size))
        assert differ > 0                                                            # the checkpoints are really different
    # the row at the scripts' own budget is the scripts' run
    class Own:
        degenerate = sw.degenerate[own]
    assert_run(model, g, Own, {f: v[own] for f, v in out.items()})
    if case == "carry":
        assert sw.carried.tolist() == [False, True, False]
    # sixty files per budget under the scripts' names
    m = golden["meta"]
    paths = sw.write_results(str(tmp_path), m["input_id"], m["input_date"])
    assert len(paths) == 60 * len(budgets) == len(set(paths))
    assert sorted(str(tmp_path / n) for n in g["run"]["files"]) == sorted(paths[60 * own:60 * own + 60])
    for k, b in enumerate(budgets):
        names = hp.eval_file_names(model, m["input_id"], m["input_date"], b)
        assert [str(tmp_path / n) for n in names] == paths[60 * k:60 * k + 60]
        for c in range(10):
            for j, f in enumerate(hp.RESULT_FIELDS):
                assert np.array_equal(np.loadtxt(tmp_path / names[6 * c + j]), out[f][k][c], equal_nan=True)
    # frame by frame batches: the same arrays
    sw1, out1 = run_sweep(model, g, budgets, batch=1, cases_per_group=3)
    assert all(np.array_equal(out1[f], out[f], equal_nan=True) for f in out)
    assert np.array_equal(sw1.used, sw.used) and np.array_equal(sw1.best, sw.best) and np.array_equal(sw1.degenerate, sw.degenerate)


@pytest.mark.parametrize("model", he.MODELS)
def test_first_frame_with_too_few_points_raises(golden, model):
    g = golden[model]["first"]
    with pytest.raises(getattr(builtins, g["run"]["error"])):
        run_sweep(model, g, (1, 5, 20))


def test_singular_frame_raises_linalgerror_and_no_inlier_names_the_budget():
    from mvoscalerecovery_amd.height_pitch import RansacBudgetSweep
    cr = he.crafted()
    mot = hc.motions(3, 3)
    with pytest.raises(np.linalg.LinAlgError):
        RansacBudgetSweep("plane", (2, 8), cases=2, seed=0).run([cr["singular"].pts], mot[:, 3::4], tris=[cr["singular"].rows])
    # six spent samples first: a single run at budget 3 or 5 has no model, and says so; the sweep names the smallest such budget
    from mvoscalerecovery_amd.height_pitch import RansacEvaluation, frame_prior
    s = cr["spent"]
    still = np.tile([0.0, 0.0, 1.0], (3, 1))                                         # straight ahead: the prior is the scene's, 0
    assert frame_prior(0.0) == tuple(hc.prior_of(s.est)) and s.est == 0.0
    with pytest.raises(ValueError, match=r"frame 0: no sample of the RANSAC had an inlier$"):
        RansacEvaluation("plane", 5, cases=2, seed=0).run([s.pts], still, samples=[s.positions[:, :5]], tris=[s.rows])
    with pytest.raises(ValueError, match=r"frame 0: no sample of the RANSAC had an inlier at budget 3$"):
        RansacBudgetSweep("plane", (3, 5, 7, 12), cases=2, seed=0).run([s.pts], still, samples=[s.positions], tris=[s.rows])
    out = RansacBudgetSweep("plane", (7, 12), cases=2, seed=0).run([s.pts], still, samples=[s.positions], tris=[s.rows])
    assert np.all(np.isfinite(out["ransac_height"]))


# ---- 14: a property of a device-drawn run -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", he.MODELS)
def test_best_count_grows_and_used_is_the_budget_or_the_stop(golden, model):
    from mvoscalerecovery_amd.height_pitch import RansacBudgetSweep
    g, budgets = golden[model]["seq"], (3, 20, 100, 600, 1500)
    sw = RansacBudgetSweep(model, budgets, cases=10, seed=77)
    sw.run(g["frames"], g["motion"][:, 3::4], tris=g["rows"])
    r = sw.last
    assert not (r["status"][:, :, -1] & ~he.ST_DEGENERATE).any()
    assert np.all(np.diff(r["best_ic"], axis=2) >= 0) and np.all(np.diff(r["best"], axis=2) >= 0)
    bud = np.array(budgets)[None, None, :]
    last = r["used"][:, :, -1:]
    stopped_last = last < budgets[-1]
    want = np.where(stopped_last, np.minimum(bud, last), bud)
    assert np.array_equal(r["used"], want)
    print("hpeval budgets property %s: %d of %d (frame, case) pairs stopped before %d" % (model, int(stopped_last.sum()), stopped_last.size, budgets[-1]))
