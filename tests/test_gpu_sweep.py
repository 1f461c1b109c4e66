"""flat_selection_sweep_kernel (csrc/mvosr_rescale_sweep.hip) and rescale.ConstantSweep on the device.  Needs a real MI355X.

Everything here is integer or bit equality, no case left out of a comparison:

* crafted frames (tests/sweep_cases.py: 3-64 survivors, at most 128 rows, at most 8 frames a launch): for every setting the sweep
  launch's flag plane, level, count and status equal mvosr_flat_selection_batch's with that setting's constants on the
  host-compacted frame, and the flags, level and count of mvosr_flat_ransac_batch with them on the device form; n_sel = 1 and the
  maximum; keep words; dt_status; refusals with the flag rows untouched;
* one frame of ~1800 features / ~3600 rows (wavefront and histogram-pass boundaries);
* end to end on the golden sequence: ConstantSweep.run equals K separate RepeatedRuns(constants=...) runs in both device-sampling
  modes and over two calls; ScaleEstimator(constants=..., sampler=recorded) reproduces the patched reference's golden outputs;
  scores / scale_scores equal the per-config ones;
* the chunk pipeline: the sweep over four chunks with a declined frame in the first and the last equals the one-chunk run, and an
  error in the middle of a call of the sweep or of the repeated runs leaves no device block alive.
"""
import dataclasses

import numpy as np
import pytest

import flat_cases as fc
import sweep_cases as sw
from conftest import load_npz
from gpu_helpers import _declining

pytestmark = pytest.mark.gpu
SEEDS = [11, 2 ** 63 + 5, 977]
MODES = {"gpu": {"triangulation": "gpu"}, "scipy": {"triangulation": "scipy", "sampling": "device"}}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            _same_tree(a[k], b[k], path + "/" + str(k))
    else:
        assert _same(np.asarray(a, dtype=np.asarray(b).dtype), b), path


def _groups(fam, size=8):
    names = list(fam)
    return [names[i:i + size] for i in range(0, len(names), size)]


def _settings16():
    return sw.crafted_settings() + [(-78.0, -84.0, 0.9), (-80.0, -85.0, 0.0), (-89.9, -89.95, 1.0), (-70.0, -80.0, 1.1), (-85.0, -85.0, 0.95),
                                    (-80.0, -80.0, 1.0), (-82.5, -87.5, 0.7), (-75.0, -75.0, 0.9)]


def _check_setting(sweep, s, want, status=True):
    """One frame's sweep result for setting s against an existing entry point's."""
    assert _same(sweep["tri_flags"][s], want["tri_flags"])
    assert _same(sweep["height_level"][s], want["height_level"]) and int(sweep["n_kept"][s]) == want["n_kept"]
    if status:
        assert sweep["status"] == want["status"]


@pytest.fixture(scope="module")
def crafted(gpu):
    """name -> (frame, the same frame behind keep words), every second frame of the family behind extra dropped features."""
    fam = sw.crafted_frames()
    out = {}
    for i, (n, f) in enumerate(fam.items()):
        out[n] = (f, f if f.keep is not None else (f.with_keep(300 + i, 3) if len(f.xyz) <= 60 else f))
    return out


def test_sweep_equals_both_entry_points_on_crafted_frames(gpu, crafted):
    settings = sw.crafted_settings()
    seen = set()
    for names in _groups(crafted):
        frames, kframes = [crafted[n][0] for n in names], [crafted[n][1] for n in names]
        assert len(frames) <= 8
        by_keep, _ = sw.run_sweep(gpu, kframes, settings, use_keep=True)
        compact, _ = sw.run_sweep(gpu, frames, settings, use_keep=False)
        counts, _ = sw.run_sweep(gpu, kframes, settings, counts_form=True)
        for s, k in enumerate(settings):
            stage = sw.run_stage(gpu, frames, *k)
            dev = sw.run_dev(gpu, kframes, *k)
            for i, n in enumerate(names):
                for got in (by_keep[i], compact[i], counts[i]):
                    _check_setting(got, s, stage[i])
                    _check_setting(got, s, dev[i], status=False)
                    assert _same(got["tri_height"], stage[i]["tri_height"])
                assert stage[i]["status"] == frames[i].status
                seen.add((n, s, int(by_keep[i]["n_kept"][s]), bool(np.isnan(by_keep[i]["height_level"][s]))))
    # the cases the frames were crafted for did occur: settings that disagree on a frame, an empty loose set (NaN level), kept rows
    assert len({(n, k) for n, s, k, _ in seen if n == "between"}) > 1
    assert any(nan for n, s, k, nan in seen if n == "k0") and any(k > 0 for n, s, k, nan in seen)
    on_level = [k for n, s, k, _ in seen if n == "on_level" and settings[s] == (-80.0, -85.0, 1.0)]
    assert on_level == [1]                                           # three tight rows, the level on the middle one: only the top row is kept


def test_one_setting_and_the_maximum(gpu, crafted):
    settings = _settings16()
    assert len(settings) == gpu.lib.mvosr_flat_selection_sweep_max_settings() == 16
    names = _groups(crafted)[0]
    frames = [crafted[n][1] for n in names]
    full, _ = sw.run_sweep(gpu, frames, settings)
    for s, k in enumerate(settings):
        one, _ = sw.run_sweep(gpu, frames, [k])
        stage = sw.run_stage(gpu, [crafted[n][0] for n in names], *k)
        for i in range(len(frames)):
            assert _same(full[i]["tri_flags"][s], one[i]["tri_flags"][0]) and _same(full[i]["height_level"][s], one[i]["height_level"][0])
            assert full[i]["n_kept"][s] == one[i]["n_kept"][0] and full[i]["status"] == one[i]["status"]
            _check_setting(full[i], s, stage[i])
    from mvoscalerecovery_amd import _lib
    with pytest.raises(_lib.MvosrLibraryError):                    # one setting more than the maximum: refused, nothing launched
        sw.run_sweep(gpu, frames, settings + [settings[0]])


def test_skipped_and_refused_frames_leave_their_rows_untouched(gpu, crafted):
    settings = sw.crafted_settings()[:3]
    names = ["between", "k5", "keep_words", "equal_even", "near_thresholds0"]
    frames = [crafted[n][1] for n in names]
    plain, _ = sw.run_sweep(gpu, frames, settings)

    def check(res, raw, hit, status):
        for i, f in enumerate(frames):
            if i in hit:
                assert res[i]["status"] == status and np.isnan(res[i]["height_level"]).all() and not res[i]["n_kept"].any()
                assert fc.all_bytes(res[i]["tri_flags"], 0xAB) and fc.all_bytes(res[i]["tri_height"], 0xAB)
            else:
                assert res[i]["status"] == plain[i]["status"] and _same(res[i]["tri_flags"], plain[i]["tri_flags"])
                assert _same(res[i]["height_level"], plain[i]["height_level"]) and _same(res[i]["n_kept"], plain[i]["n_kept"])
    # dt_status != 0: skipped like a declined frame, as mvosr_flat_ransac_batch skips it
    dt = [0, 7, 0, 1, 0]
    res, raw = sw.run_sweep(gpu, frames, settings, dt_status=dt, sentinel=0xAB)
    check(res, raw, {1, 3}, fc.ST_EMPTY)
    dev = sw.run_dev(gpu, frames, *settings[0], dt_status=dt)
    assert [d["status"] for d in dev][1] == fc.ST_EMPTY == [d["status"] for d in dev][3]
    # more features than the header's max_feat, more rows than max_tri: refused before LDS is touched
    feats = sorted(len(f.xyz) for f in frames)
    res, raw = sw.run_sweep(gpu, frames, settings, max_feat=feats[2], sentinel=0xAB)
    over = {i for i, f in enumerate(frames) if len(f.xyz) > feats[2]}
    assert len(over) == 2
    check(res, raw, over, fc.ST_MASK)
    rows = sorted(len(f.tri) for f in frames)
    res, raw = sw.run_sweep(gpu, frames, settings, max_tri=rows[2], sentinel=0xAB)
    over = {i for i, f in enumerate(frames) if len(f.tri) > rows[2]}
    assert len(over) == 2
    check(res, raw, over, fc.ST_MASK)
    # the counts form: what lies between the frames' rows in a plane is never written
    res, raw = sw.run_sweep(gpu, frames, settings, counts_form=True, sentinel=0xAB)
    written = sum(len(f.tri) for f in frames)
    assert int((raw["tri_flags"] != 0xAB).sum()) == len(settings) * written and raw["tri_flags"].shape[1] > 2 * written
    for i in range(len(frames)):
        assert _same(res[i]["tri_flags"], plain[i]["tri_flags"])


def test_a_frame_across_wave_and_pass_boundaries(gpu):
    big = sw.big_frame()
    kbig = big.with_keep(5, 150)
    settings = _settings16()
    got, _ = sw.run_sweep(gpu, [kbig], settings)
    got_c, _ = sw.run_sweep(gpu, [kbig], settings, counts_form=True)
    assert len(big.tri) > 3 * 1024 and got[0]["status"] == 0
    kept = set()
    for s, k in enumerate(settings):
        stage = sw.run_stage(gpu, [big], *k)[0]
        _check_setting(got[0], s, stage)
        _check_setting(got_c[0], s, stage)
        kept.add(stage["n_kept"])
    assert _same(got[0]["tri_height"], stage["tri_height"]) and len(kept) > 8 and max(kept) > 500
    for s in (0, 7, 15):
        _check_setting(got[0], s, sw.run_dev(gpu, [kbig], *settings[s])[0], status=False)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _configs():
    from mvoscalerecovery_amd.rescale import RescaleConstants
    # the golden's settings, and three that bite where its sequence leaves a constant idle: lists shorter than min_points, a
    # selection and a tail constant moved together, and a loose threshold that moves a level
    return [RescaleConstants(**kw) for _, kw in sw.SETTINGS] + [RescaleConstants(ransac_min_points=600),
                                                               RescaleConstants(loose_deg=-75.0, slew=0.2), RescaleConstants(n_hyp=7, threshold=0.01)]


@pytest.fixture(scope="module")
def separate(gpu):
    """mode -> per config the result of RepeatedRuns(constants=config).run(data): the reference of the contract, computed once."""
    from mvoscalerecovery_amd.rescale import RepeatedRuns
    data = sw.golden_sequence()
    out = {}
    for mode, kw in MODES.items():
        out[mode] = []
        for k in _configs():
            rr = RepeatedRuns(sw.ABS_REF, window_size=sw.WINDOW, seeds=SEEDS, constants=k, delaunay_workers=0, **kw)
            out[mode].append((rr, rr.run(data)))
    return data, out


@pytest.mark.parametrize("mode", list(MODES))
def test_constant_sweep_equals_separate_repeated_runs(gpu, separate, mode):
    from mvoscalerecovery_amd.rescale import ConstantSweep
    data, ref = separate
    configs = _configs()
    sweep = ConstantSweep(sw.ABS_REF, configs, window_size=sw.WINDOW, seeds=SEEDS, delaunay_workers=0, **MODES[mode])
    got = sweep.run(data)
    assert got["scales"].shape == (len(configs), 3, len(data["move_flags"])) and got["raw_scale"].shape[:2] == (len(configs), 3)
    for k, (rr, want) in enumerate(ref[mode]):
        for key in ("scales", "error", "raw_scale", "status"):
            assert _same(got[key][k], want[key]), (mode, k, key)
        assert _same(got["kinds"], want["kinds"])
    # the launches that were made: one sweep launch for the 5 distinct selections, one fit per distinct (selection, RANSAC) pair
    # (and the same again for the frames both device triangulations declined, if any)
    assert sweep._sels[0] == (-80.0, -85.0, 0.9) and len(sweep._sels) == 5 and len(sweep._pairs) == 11
    assert sweep.launches == {"sweep": 1 + bool(sweep.estimator.last_declined), "cases": 11 * (1 + bool(sweep.estimator.last_declined))}
    few = got["status"][len(sw.SETTINGS)]                            # ransac_min_points = 600: some lists are shorter, some are not
    assert (few == fc.ST_RS_FEW).any() and (few == 0).any()
    assert not _same(got["scales"][0], got["scales"][len(sw.SETTINGS) + 1])
    # over two calls: the frame counter, every tail and the previous scale carry over
    cut = 11
    parts = [{k: v[:cut] for k, v in data.items()}, {k: v[cut:] for k, v in data.items()}]
    twice = ConstantSweep(sw.ABS_REF, configs, window_size=sw.WINDOW, seeds=SEEDS, delaunay_workers=0, **MODES[mode])
    both = [twice.run(p) for p in parts]
    assert _same(np.concatenate([b["scales"] for b in both], axis=2), got["scales"]) and _same(twice.scales(), got["scales"])
    assert _same(np.concatenate([b["raw_scale"] for b in both], axis=2), got["raw_scale"])


def test_estimator_with_constants_reproduces_the_patched_reference(gpu):
    """rescale.ScaleEstimator(constants=k) with the golden's recorded samples against the reference's rescale.py with k's literals
    (tests/golden/sweep.npz), as tests/golden/rescale.npz is reproduced: lists, inlier counts and iterations exact, continuous
    values within 1e-9 relative."""
    from mvoscalerecovery_amd import offline
    from mvoscalerecovery_amd.rescale import RescaleConstants, ScaleEstimator
    z, meta = load_npz("sweep.npz")
    data = sw.golden_sequence()
    assert meta["crc"] == sw.sequence_checksum(data)
    for i, (name, kw) in enumerate(sw.SETTINGS):
        est = ScaleEstimator(meta["abs_ref"], window_size=meta["window"], sampler=sw.recorded_sampler(z, i), constants=RescaleConstants(**kw),
                             delaunay_workers=0)
        assert est.triangulation == "scipy" and est.sampling == "host"
        calls = []
        real = est.scale_calculation

        def spy(f3, f2, img=None):
            out = real(f3, f2)
            pf2, fl = est.last["pf2"], est.last["tri_flags"]
            rec = {"ids": est.last["tris2"][0][(fl[:int(pf2.tri2_off[1])] & 4) != 0].reshape(-1), "height_level": est.height_level}
            if len(rec["ids"]) >= est.constants.ransac_min_points:
                rec.update(best_ic=int(est.last["best_ic"][0]), used=int(est.last["used"][0]))
            calls.append(rec)
            return out
        est.scale_calculation = spy
        out = offline.run_sequence(data, est)
        off = z["s%d_ids_off" % i]
        assert len(calls) == len(off) - 1
        for c, rec in enumerate(calls):
            assert np.array_equal(rec["ids"], z["s%d_ids" % i][off[c]:off[c + 1]]), (name, c)
            np.testing.assert_allclose(rec["height_level"], z["s%d_height_level" % i][c], rtol=1e-9)
        assert np.array_equal(["best_ic" in r for r in calls], z["s%d_ran" % i])
        assert np.array_equal([r["best_ic"] for r in calls if "best_ic" in r], z["s%d_best_ic" % i]), name
        assert np.array_equal([r["used"] for r in calls if "best_ic" in r], z["s%d_used" % i]), name
        np.testing.assert_allclose(out["scales"], z["s%d_scales" % i], rtol=1e-9)


def test_sweep_scores_equal_the_per_config_scores(gpu, separate):
    import scores_cases as sc
    from mvoscalerecovery_amd import evaluate
    from mvoscalerecovery_amd.rescale import ConstantSweep, RepeatedRuns
    data, _ = separate
    n = len(data["move_flags"])
    seq = sc.make_sequence("n65")
    motions = seq["motions"][:n].copy()
    motions[:, 3:12:4] *= 12.0                                       # 12 m steps: segments of 100 and 200 m exist
    data = dict(data, motions=[m for m in motions])
    gt = seq["gt"][:n + 1]
    configs = [_configs()[i] for i in (0, 2, 9, 11)]
    speed_gt = np.concatenate([evaluate.calculate_speed(gt, ctx=gpu) / 12.0, [1.0]])
    sweep = ConstantSweep(sw.ABS_REF, configs, window_size=sw.WINDOW, seeds=SEEDS, triangulation="gpu", delaunay_workers=0)
    sweep.run(data)
    got = sweep.scores(gt, speed_gt=speed_gt[:n])
    got_s = sweep.scale_scores(speed_gt, poses_gt=gt, filter_window=5)
    assert got["tra"].shape[:2] == (4, 3) and got["trimmed"]["tra_mean"].shape == (4,) and "speed_scaled" in got
    assert set(got_s) == {"scales", "filtered", "gt_rescaled", "gt_rescaled_filtered", "trimmed"} and got_s["scales"]["drift"].shape[:2] == (4, 3)
    for k, cfg in enumerate(configs):
        rr = RepeatedRuns(sw.ABS_REF, window_size=sw.WINDOW, seeds=SEEDS, constants=cfg, triangulation="gpu", delaunay_workers=0)
        rr.run(data)
        assert _same(rr.scales(), sweep.scales()[k])
        want = rr.scores(gt, speed_gt=speed_gt[:n])
        want_s = rr.scale_scores(speed_gt, poses_gt=gt, filter_window=5)
        take = lambda d: {key: (take(v) if isinstance(v, dict) else (v if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else np.asarray(v)[k]))
                          for key, v in d.items()}
        _same_tree(take(got), want, "scores[%d]" % k)
        _same_tree(take(got_s), want_s, "scale_scores[%d]" % k)
    best = sweep.best("tra_mean")
    assert best is configs[int(np.nanargmin(got["trimmed"]["tra_mean"]))]
    table = sweep.table("scale_mean")
    assert [row["config"] for row in table] == [0, 1, 2, 3] and table[2]["slew"] == 0.2
    assert table[1]["scale_mean"] == float(got_s["trimmed"]["scales"]["mean"][1]) and dataclasses.asdict(configs[3]).items() <= table[3].items()


@pytest.mark.parametrize("mode", list(MODES))
def test_a_frame_at_which_the_reference_raises(gpu, mode):
    """A frame with nothing below the vanishing row (rescale.py:124 raises on it): the sweep raises what RepeatedRuns raises, with
    every tail and the sample counter where RepeatedRuns leaves them — the frames before it pushed, the frame itself counted."""
    from mvoscalerecovery_amd.rescale import ConstantSweep, RepeatedRuns
    data = sw.golden_sequence()
    at = [i for i, f in enumerate(data["feature2ds"]) if len(f) > 100][7]
    f2 = np.array(data["feature2ds"][at], dtype=np.float64)
    f2[:, 1] = 10.0
    data["feature2ds"] = list(data["feature2ds"])
    data["feature2ds"][at] = f2
    configs = _configs()[:3]
    rr = RepeatedRuns(sw.ABS_REF, window_size=sw.WINDOW, seeds=SEEDS, constants=configs[2], delaunay_workers=0, **MODES[mode])
    with pytest.raises(Exception) as want:
        rr.run(data)
    sweep = ConstantSweep(sw.ABS_REF, configs, window_size=sw.WINDOW, seeds=SEEDS, delaunay_workers=0, **MODES[mode])
    with pytest.raises(type(want.value)) as got:
        sweep.run(data)
    assert str(got.value) == str(want.value)
    assert sweep.estimator._frame_counter == rr.estimator._frame_counter == 8 and sweep.scales().shape[2] == rr.scales().shape[1] == 0
    for c in range(3):
        assert sweep.tails[2][c].scale == rr.tails[c].scale and list(sweep.tails[2][c].scale_queue) == list(rr.tails[c].scale_queue)


# ---- the chunk pipeline: several chunks, declined frames, an error mid-call ------------------------------------------------------------
def _short_sequence(n, declined=()):
    """``n`` processed frames of 120-300 features, the frames ``declined`` replaced by ones both device triangulations decline."""
    from mvoscalerecovery_amd import synth
    data = synth.synth_sequence_dict(n, base_seed=67, n_lo=120, n_hi=300, p_not_moving=0.0, p_too_few=0.0)
    frames = _declining(list(zip(data["feature3ds"], data["feature2ds"])), declined)
    data["feature3ds"], data["feature2ds"] = [f[0] for f in frames], [f[1] for f in frames]
    return data


@pytest.mark.parametrize("mode", list(MODES))
def test_sweep_over_several_chunks_with_declined_frames(gpu, mode):
    """One chunk against chunks of 4 frames, a declined frame in the first chunk and one in the last: the same bits, the declined
    frames re-run once per chunk that holds one, and one set of launches per chunk and per re-run."""
    from mvoscalerecovery_amd.rescale import ConstantSweep, RescaleConstants
    F, step, declined = 14, 4, [1, 13]
    data = _short_sequence(F, declined)
    configs = [RescaleConstants(), RescaleConstants(loose_deg=-75.0)]
    runs = []
    for chunk in (None, step):
        sweep = ConstantSweep(sw.ABS_REF, configs, window_size=sw.WINDOW, seeds=SEEDS[:2], delaunay_workers=0, **MODES[mode])
        if chunk is not None:
            sweep.estimator.GPU_CHUNK = sweep.estimator.GPU_MIN_CHUNK = chunk
        runs.append((sweep, sweep.run(data)))
    (one, want), (chunked, got) = runs
    assert got["raw_scale"].shape == (2, 2, F) and len(chunked._sels) == 2 and len(chunked._pairs) == 2
    for key in ("scales", "error", "raw_scale", "status"):
        assert _same(got[key], want[key]), (mode, key)
    assert not _same(got["raw_scale"][0], got["raw_scale"][1])       # the selection constant bites on these frames
    if mode == "gpu":
        assert one.estimator.last_declined == chunked.estimator.last_declined == 2
        bounds = [(a, min(F, a + step)) for a in range(0, F, step)]
        launched = len(bounds) + len({k for k, (a, b) in enumerate(bounds) for f in declined if a <= f < b})
        assert (len(bounds), launched) == (4, 6)
    else:
        launched = 1                                                 # the host's triangulations: chunks of 2048 frames, nothing to re-run
    assert chunked.launches == {"sweep": launched, "cases": len(chunked._pairs) * launched}
    assert one.launches == {"sweep": 1 + (mode == "gpu"), "cases": 2 * (1 + (mode == "gpu"))}


@pytest.mark.parametrize("pipeline", ["repeats", "sweep"])
def test_error_mid_call_releases_every_block(gpu, pipeline, monkeypatch):
    """``_launch_cases`` raises on its third call, while a chunk is being started and the chunk before it is queued: the exception
    leaves the call, no device block of the call stays alive, and the estimator's next call equals a fresh estimator's."""
    from mvoscalerecovery_amd.rescale import ConstantSweep, RescaleConstants, ScaleEstimator
    data = _short_sequence(12)
    f3s, f2s = data["feature3ds"], data["feature2ds"]

    def make():
        if pipeline == "sweep":
            sweep = ConstantSweep(sw.ABS_REF, [RescaleConstants(), RescaleConstants(loose_deg=-75.0)], window_size=sw.WINDOW, seeds=SEEDS[:2],
                                  triangulation="gpu", delaunay_workers=0)
            est, call = sweep.estimator, lambda: sweep._raw_cases(f3s, f2s)
        else:
            est = ScaleEstimator(sw.ABS_REF, window_size=sw.WINDOW, ransac_seed=0, triangulation="gpu", delaunay_workers=0)
            call = lambda: est.raw_scale_cases_batch(f3s, f2s, SEEDS[:2])
        est.GPU_CHUNK = est.GPU_MIN_CHUNK = 4
        return est, call
    est, call = make()
    call()                                                           # (the estimator's context has its caches from here on)
    before = est.ctx.alloc_stats()["live_blocks"]
    real, calls = est._launch_cases, [0]

    def failing(*a, **k):
        calls[0] += 1
        if calls[0] == 3:
            raise RuntimeError("launch failed")
        return real(*a, **k)
    monkeypatch.setattr(est, "_launch_cases", failing)
    with pytest.raises(RuntimeError, match="launch failed"):
        call()
    monkeypatch.undo()
    assert calls[0] == 3 and est.ctx.alloc_stats()["live_blocks"] == before
    got, want = call(), make()[1]()
    assert set(got) == set(want) and sorted(got["host_errors"]) == sorted(want["host_errors"]) == []
    for key in want:
        if key != "host_errors":
            assert _same(got[key], want[key]), key
