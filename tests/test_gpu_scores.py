"""Scoring the repeated runs on the device: mvosr_paths_batch, mvosr_segment_table, mvosr_score_cases_batch, mvosr_pose2motion_batch
(csrc/mvosr_score.hip), evaluate.Scorer / calculate_speed / change_scale, offline.get_path_batch and RepeatedRuns.scores.  Needs a
real MI355X.

The comparator is the reference's own output in tests/golden/scores.npz (make_golden_scores.py) under the rule of
tests/scores_cases.py: integers exact, every float within 4 gaps, the gap being the fixture's |reference - extended precision| for
that quantity and sequence.  Every launch helper puts sentinel guards around its outputs.
"""
import json

import numpy as np
import pytest

import scores_cases as sc
from conftest import load_npz

pytestmark = pytest.mark.gpu
NAMES = list(sc.SEQUENCES)
WHOLE_PATHS = [k for k in NAMES if 1 < sc.SEQUENCES[k][0] <= sc.FULL_POSES_UP_TO]


@pytest.fixture(scope="module")
def golden():
    return load_npz("scores.npz")[0]


@pytest.fixture(scope="module")
def device(gpu):
    """Every sequence through the four launchers, once: paths, table, rows and means."""
    out = {}
    for name in NAMES:
        seq = sc.make_sequence(name)
        paths = sc.launch_paths(gpu, seq["motions"], seq["scales"])
        table = sc.launch_table(gpu, seq["gt"])
        out[name] = dict(seq, paths=paths, table=table, score=sc.launch_score(gpu, table, paths))
    return out


def gaps_of(golden, name):
    return json.loads(str(golden[name + "_gaps"]))


@pytest.mark.parametrize("name", NAMES)
def test_segment_table(golden, device, name):
    t = device[name]["table"]
    n, _, _, kind = sc.SEQUENCES[name]
    assert np.array_equal(t["last"], golden[name + "_last"]) and t["last"].dtype == np.int32          # integers: exact
    assert t["status"][0] == 0 and t["dist"][0] == 0.0
    has = t["last"] >= 0
    assert np.array_equal(np.isnan(t["gdelta"][:, :, :12]).all(axis=2), ~has)
    if kind == "exact":
        assert np.array_equal(t["dist"], 16.0 * np.arange(n + 1))
        assert t["last"][0, 3] == 26 and t["last"][0, 7] == 51                                         # dist[25] = 400 is not > 400
    elif n:
        sc.within(t["dist"], sc.distances(device[name]["gt"]), gaps_of(golden, name)["dist"], name + " dist")
        # (the restated sum is the reference's left-to-right sum of the same float64 norms; the table above is the check that binds)


@pytest.mark.parametrize("name", NAMES)
def test_paths(gpu, golden, device, name):
    d, g = device[name], gaps_of(golden, name)
    n, cases = sc.SEQUENCES[name][:2]
    assert d["paths"].shape == (cases, n + 1, 12)
    ident = np.eye(4)[:3].reshape(-1)
    assert all(np.array_equal(d["paths"][c, 0], ident) for c in range(cases))
    if n:
        pc, pr = sc.pose_cases(name), sc.pose_rows(name)
        sc.within(d["paths"][pc][:, pr], golden[name + "_poses"], g["poses"], name + " poses")
        sc.within(d["paths"][:, -1], golden[name + "_pose_end"], g["poses"], name + " last pose")
    # scales = NULL means ones; a per-case stride reads each case's own motions
    ones = sc.launch_paths(gpu, d["motions"], np.ones((2, n)))
    none = sc.launch_paths(gpu, d["motions"], None, cases=2)
    assert ones.tobytes() == none.tobytes()
    if n:
        scaled = np.broadcast_to(d["motions"], (cases, n, 12)).copy()
        scaled[:, :, 3:12:4] = scaled[:, :, 3:12:4] * d["scales"][:, :, None]
        own = sc.launch_paths(gpu, scaled, None, cases=cases, case_stride=n * 12)
        assert own.tobytes() == d["paths"].tobytes()                                                  # scaled first, rounded, then the chain


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_means(golden, device, name):
    d, g = device[name], gaps_of(golden, name)
    s, last = d["score"], d["table"]["last"]
    has = last >= 0
    cases = sc.SEQUENCES[name][1]
    assert (s["status"] == 0).all()
    assert np.array_equal(s["counts"], np.broadcast_to(has.sum(axis=0), (cases, 8)))                  # integers: exact
    assert np.isnan(s["r_seg"][:, ~has]).all() and np.isnan(s["t_seg"][:, ~has]).all()
    assert np.array_equal(np.isnan(s["means"]), np.broadcast_to(~has.any(axis=0), (cases, 2, 8)))
    if not has.any():
        return
    rc = golden[name + "_rows_cases"]
    sc.within(s["r_seg"][rc][:, has], golden[name + "_rows_r"], g["rows_r"], name + " r_err/len")
    sc.within(s["t_seg"][rc][:, has], golden[name + "_rows_t"], g["rows_t"], name + " t_err/len")
    columns = has.any(axis=0)
    assert np.array_equal(columns, golden[name + "_columns"])
    tra, rot = sc.scores_from_means(s["means"], columns)
    assert tra.shape == golden[name + "_tra"].shape                                                   # n65: seven columns
    sc.within(tra, golden[name + "_tra"], g["tra"], name + " tra")
    sc.within(rot, golden[name + "_rot"], g["rot"], name + " rot")
    # the means are the rows summed left to right over ascending first
    for k in np.nonzero(columns)[0]:
        rows = np.nonzero(has[:, k])[0]
        for q, seg in enumerate((s["r_seg"], s["t_seg"])):
            assert np.array_equal(np.cumsum(seg[:, rows, k], axis=1)[:, -1] / rows.size, s["means"][:, q, k])


@pytest.mark.parametrize("name", WHOLE_PATHS)
def test_pose2motion_speed_and_change_scale(gpu, golden, name):
    from mvoscalerecovery_amd import evaluate
    g = gaps_of(golden, name)
    seq = sc.make_sequence(name)
    ref_paths, gt_speed = golden[name + "_poses"], golden[name + "_gt_speed"]                         # whole paths at this length
    r = sc.launch_pose2motion(gpu, ref_paths)
    assert (r["status"] == 0).all()
    sc.within(r["motions"], golden[name + "_p2m"], g["p2m"], name + " pose2motion")
    assert np.array_equal(r["norms"], sc.norm3(r["motions"][..., 3:12:4]))
    speed = evaluate.calculate_speed(seq["gt"], ctx=gpu)
    if "gt_speed" in g:
        sc.within(speed, gt_speed, g["gt_speed"], name + " calculate_speed")
    else:
        assert np.array_equal(speed, gt_speed)                                                        # exact steps
    cs = evaluate.change_scale(ref_paths, gt_speed, ctx=gpu)
    sc.within(cs, golden[name + "_cs"], g["cs"], name + " change_scale")
    one = evaluate.change_scale(ref_paths[0], gt_speed, ctx=gpu)                                      # one path: the same bytes
    assert one.shape == ref_paths[0].shape and one.tobytes() == cs[0].tobytes()
    assert evaluate.calculate_speed(ref_paths, ctx=gpu).tobytes() == r["norms"].tobytes()
    with pytest.raises(ValueError):
        evaluate.change_scale(ref_paths, gt_speed[:-1], ctx=gpu)


def test_same_bytes_every_run_and_case_alone(gpu, device):
    d = device["n257"]
    again_paths = sc.launch_paths(gpu, d["motions"], d["scales"])
    again = sc.launch_score(gpu, d["table"], again_paths)
    assert again_paths.tobytes() == d["paths"].tobytes()
    for k in ("r_seg", "t_seg", "means", "counts", "status"):
        assert again[k].tobytes() == d["score"][k].tobytes(), k
    for c in (0, 4, 9):                                                                                # case c alone = case c of the ten
        p1 = sc.launch_paths(gpu, d["motions"], d["scales"][c:c + 1])
        s1 = sc.launch_score(gpu, d["table"], p1)
        assert p1[0].tobytes() == d["paths"][c].tobytes()
        for k in ("r_seg", "t_seg", "means", "counts"):
            assert s1[k][0].tobytes() == d["score"][k][c].tobytes(), (k, c)
    m = sc.launch_pose2motion(gpu, d["paths"])
    assert sc.launch_pose2motion(gpu, d["paths"][3])["motions"][0].tobytes() == m["motions"][3].tobytes()


def test_scorer_against_repeat_scores(gpu, golden, device):
    from mvoscalerecovery_amd import evaluate, offline
    d, g = device["n257"], gaps_of(golden, "n257")
    scorer = evaluate.Scorer(d["gt"], ctx=gpu)
    assert np.array_equal(scorer.last, golden["n257_last"]) and np.array_equal(scorer.columns, golden["n257_columns"])
    seg = scorer.segments
    assert seg["first"].dtype.kind == "i" and np.array_equal(seg["speed"], golden["n257_speed"])
    by_scales = scorer.score_scales(d["motions"], d["scales"])
    host_paths = [offline.get_path(d["motions"], d["scales"][c]) for c in range(10)]
    by_paths = scorer.score_paths(host_paths)
    host = evaluate.repeat_scores(d["gt"], host_paths)
    assert set(by_scales) == set(host) and set(by_scales["trimmed"]) == set(host["trimmed"])
    for a, b, what in ((by_scales, host, "score_scales vs repeat_scores"), (by_paths, host, "score_paths vs repeat_scores"),
                       (by_scales, by_paths, "score_scales vs score_paths")):
        for k in ("tra", "rot", "tra_mean", "rot_mean"):
            assert a[k].shape == b[k].shape
            sc.within(a[k], b[k], g[k[:3]], "%s %s" % (what, k))
            sc.within(a["trimmed"][k], b["trimmed"][k], g[k[:3]], "%s trimmed %s" % (what, k))
    # the device's own paths scored as paths: the same launches, the same bytes
    dev_paths = offline.get_path_batch(d["motions"], d["scales"], ctx=gpu)
    assert dev_paths.tobytes() == d["paths"].tobytes()
    again = scorer.score_paths(offline.get_path_batch(d["motions"], d["scales"], ctx=gpu, on_device=True))
    assert all(again[k].tobytes() == by_scales[k].tobytes() for k in ("tra", "rot", "tra_mean", "rot_mean"))
    # the rows, in the reference's order and types
    rows = scorer.errors(motions=d["motions"], scales=d["scales"][:2])
    ref0 = evaluate.calculate_sequence_error(d["gt"], host_paths[0])
    assert len(rows) == 2 and len(rows[0]) == len(ref0) == 180
    assert [(r[0], r[3], r[4]) for r in rows[0]] == [(r[0], r[3], r[4]) for r in ref0] and isinstance(rows[0][0][0], int)
    sc.within([r[1] for r in rows[0]], [r[1] for r in ref0], g["rows_r"], "errors() r_err/len")
    sc.within([r[2] for r in rows[0]], [r[2] for r in ref0], g["rows_t"], "errors() t_err/len")


def _runs_data():
    """A short main_offline dict whose motions carry 12 m steps, and a ground truth of its length."""
    from mvoscalerecovery_amd import synth
    seq = sc.make_sequence("n65")
    n = 60
    data = synth.synth_sequence_dict(n, base_seed=77, n_lo=300, n_hi=600, p_not_moving=0.05, p_too_few=0.05)
    motions = seq["motions"][:n].copy()
    motions[:, 3:12:4] *= 12.0
    data["motions"] = [m for m in motions]
    return data, motions, seq["gt"][:n + 1]


def _host_change_scale(path, speed):
    """script/change_scale.py:12-18 through the host comparators evaluate.pose2motion and offline.motion2pose."""
    from mvoscalerecovery_amd import evaluate, offline
    m = evaluate.pose2motion(path)
    t = m[:, 3:12:4]
    m[:, 3:12:4] = (speed * t.T / (np.sqrt(np.sum(t * t, 1)) + 0.00001)).T
    return offline.motion2pose(m)


def test_repeated_runs_scores(gpu):
    from mvoscalerecovery_amd import evaluate
    from mvoscalerecovery_amd.rescale import RepeatedRuns
    data, motions, gt = _runs_data()
    runs = RepeatedRuns(1.75, window_size=5, seed=11, cases=4, triangulation="gpu", delaunay_workers=0)
    runs.run(data)
    scales = runs.scales()
    assert scales.shape == (4, 60) and np.isfinite(scales).all() and (scales == 0).any() and (scales > 0).sum() > 100
    host_paths = runs.paths()
    host = evaluate.repeat_scores(gt, host_paths)                                                      # the reference's formulas, on the host
    last = sc.segment_table(sc.distances(gt))[0]
    columns = (last >= 0).any(axis=0)
    wide = sc.score_restated(gt, sc.paths_restated(motions, scales, dtype=np.longdouble), last, dtype=np.longdouble)[2]
    x_tra, x_rot = wide[:, 1, :][:, columns], wide[:, 0, :][:, columns] * 180 / np.longdouble(np.pi)
    gap = {"tra": float(np.abs(host["tra"] - x_tra).max()), "rot": float(np.abs(host["rot"] - x_rot).max())}   # reference vs extended
    speed_gt = evaluate.calculate_speed(gt, ctx=gpu)
    got = runs.scores(gt, speed_gt=speed_gt)
    assert columns.sum() >= 4 and got["tra"].shape == host["tra"].shape == (4, int(columns.sum()))
    for k in ("tra", "rot", "tra_mean", "rot_mean"):
        sc.within(got[k], host[k], gap[k[:3]], "RepeatedRuns.scores " + k)
        sc.within(got["trimmed"][k], host["trimmed"][k], gap[k[:3]], "RepeatedRuns.scores trimmed " + k)
    on_device = runs.paths(on_device=True)
    assert len(on_device) == 4 and all(np.allclose(a, b, rtol=0, atol=1e-9) for a, b in zip(on_device, host_paths))
    # re-scaled to the ground truth's speed: every case, the same keys; a path that moves at the true speed scores better
    rescaled = got["speed_scaled"]
    assert set(rescaled) == set(host) and rescaled["tra"].shape == got["tra"].shape
    host_scaled = evaluate.repeat_scores(gt, [_host_change_scale(p, speed_gt) for p in host_paths])   # the reference's formulas, on the host
    x_cs = sc.change_scale_restated(sc.paths_restated(motions, scales, dtype=np.longdouble), speed_gt, dtype=np.longdouble)
    x_means = sc.score_restated(gt, x_cs, last, dtype=np.longdouble)[2]
    for q, k in ((1, "tra"), (0, "rot")):
        unit = 180 / np.longdouble(np.pi) if k == "rot" else 1
        gap_cs = float(np.abs(host_scaled[k] - x_means[:, q, :][:, columns] * unit).max())             # reference vs extended
        sc.within(rescaled[k], host_scaled[k], gap_cs, "speed_scaled " + k)
    assert np.isfinite(rescaled["tra"]).all()
    assert runs.scores(gt)["tra"].tobytes() == got["tra"].tobytes() and "speed_scaled" not in runs.scores(gt)


def test_zero_rotation_block_raises(gpu, device):
    from mvoscalerecovery_amd import evaluate
    d = device["n130"]
    scorer = evaluate.Scorer(d["gt"], ctx=gpu)
    bad = d["paths"].copy()
    bad[1, 10, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = 0.0                                                     # case 1, the pose of first = 10
    with pytest.raises(np.linalg.LinAlgError):
        scorer.score_paths(bad)
    raw = sc.launch_score(gpu, device["n130"]["table"], bad)
    assert raw["status"].tolist() == [0, 7, 0]                                                        # MVOSR_ST_ERR_SINGULAR, that case only
    assert raw["means"][0].tobytes() == d["score"]["means"][0].tobytes()
    with pytest.raises(np.linalg.LinAlgError):
        evaluate.calculate_speed(bad, ctx=gpu)
    gt_bad = d["gt"].copy()
    gt_bad[0, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        evaluate.Scorer(gt_bad, ctx=gpu)
    with pytest.raises(IndexError):
        scorer.score_paths(d["paths"][:, :100])                                                       # shorter than a segment's last frame


def test_fewer_than_three_cases_raise(gpu, device):
    from mvoscalerecovery_amd import evaluate
    d = device["n130"]
    scorer = evaluate.Scorer(d["gt"], ctx=gpu)
    with pytest.raises(ValueError):
        scorer.score_scales(d["motions"], d["scales"][:2])
    assert scorer.score_scales(d["motions"], d["scales"])["tra"].shape == (3, 8)


def test_refusals_return_error_codes(gpu):
    lib, h = gpu.lib, gpu.handle
    buf = gpu.zeros(64, np.float64)
    p = buf.ptr
    assert lib.mvosr_paths_batch(h, 1, 0, p, 0, None, p) == -2                                         # C < 1
    assert lib.mvosr_paths_batch(h, 1, 1, None, 0, None, p) == -2 and lib.mvosr_paths_batch(h, 1, 1, p, 0, None, None) == -2
    assert lib.mvosr_paths_batch(h, -1, 1, p, 0, None, p) == -2 and lib.mvosr_paths_batch(h, 2, 2, p, 12, None, p) == -2
    assert lib.mvosr_segment_table(h, 0, p, p, p, p, p) == -2 and lib.mvosr_segment_table(h, 1, p, None, p, p, p) == -2
    assert lib.mvosr_score_cases_batch(h, 0, 1, p, 1, p, p, None, None, p, p, p) == -2
    assert lib.mvosr_score_cases_batch(h, 1, 1, p, 1, p, p, None, None, None, p, p) == -2
    assert lib.mvosr_score_cases_batch(h, 1, 1, p, 1, None, p, None, None, p, p, p) == -2
    assert lib.mvosr_pose2motion_batch(h, 0, 1, p, None, p, None, p) == -2 and lib.mvosr_pose2motion_batch(h, 1, 1, p, None, None, None, p) == -2
    assert lib.mvosr_pose2motion_batch(h, 1, 1, None, None, p, None, p) == -2
    assert (buf.download() == 0).all()                                                                 # nothing was launched
