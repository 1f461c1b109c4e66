"""The repeated runs on the device: mvosr_flat_ransac_cases_batch (csrc/mvosr_rescale_cases.hip), ScaleEstimator.raw_scale_cases_batch
and rescale.RepeatedRuns.  Needs a real MI355X.

The comparator is the parent's kernel: mvosr_flat_ransac_batch with rp->seed = the case's seed on the same resident batch
(tests/repeats_cases.py: run_pair), byte for byte; then oracle/rescale_oracle.py on the same lists (counts, best_ic, used exact;
models and scales to 1e-9, the existing device-vs-oracle tolerance), single estimators for RepeatedRuns, the reference's own ten
runs (tests/golden/rescale_repeats.npz) and the unseeded reference's distribution (tests/golden/rescale_distribution.npz).
"""
import numpy as np
import pytest

import flat_cases as fc
import repeats_cases as rc
from conftest import load_npz
from gpu_helpers import _declining, _ransac_triples, _rescale_frames

pytestmark = pytest.mark.gpu
SIZES = [400, 640, 900, 1300, 2000, 150, 2000, 777, 1024, 2000, 333, 1800, 120, 128, 110, 140]
SEEDS7 = [11, 2 ** 63 + 5, 3, 0, 2 ** 64 - 1, 123456789, 77]


@pytest.fixture(scope="module")
def synth_frames(gpu):
    """The sixteen synthetic frames as resident-batch frames: the features below the vanishing row, the vote's keep words and the
    second triangulation's rows, as the device-resident estimator's stage outputs give them."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    frames = _rescale_frames(SIZES)
    est = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=1, delaunay_workers=0)
    est.scale_calculation_batch([f[0] for f in frames], [f[1] for f in frames], stage=True)
    out = []
    for i, (f3, f2) in enumerate(frames):
        low = f2[:, 1] > est.vanish
        valid = np.asarray(est.last["valid"][i], bool)
        assert valid.shape[0] == int(low.sum())
        keep = np.where(valid, 1, -1 if int(valid.sum()) > 10 else 0).astype(np.int32)
        out.append(fc.Frame("synth%d" % i, f3[low], est.last["tris2"][i], keep=keep))
    return out


@pytest.fixture(scope="module")
def singles7(gpu, synth_frames):
    """The parent's kernel, once per seed, and the new call with one case per workgroup."""
    return rc.run_pair(gpu, synth_frames, SEEDS7, group=1, frame_base=40)


@pytest.mark.parametrize("group", [1, 3, 7, 0])
def test_case_equals_single_run_bit_for_bit(gpu, synth_frames, singles7, group):
    single, cases1 = singles7
    cases = cases1 if group == 1 else rc.run_pair(gpu, synth_frames, SEEDS7, group=group, frame_base=40, singles=False)[1]
    assert (np.array([s["status"] for s in single]) == 0).sum() >= 7 * 12          # the comparison is not between refusals
    rc.assert_cases_equal_singles(single, cases)
    for k in rc.SINGLE_KEYS + ("count_form",):
        assert rc.same(cases[k], cases1[k]), (k, group)                            # the result does not depend on G
    forms = set(cases["count_form"].tolist())
    assert forms <= {rc.FORM_PACKED, rc.FORM_GATHER}


def test_one_case(gpu, synth_frames, singles7):
    single, _ = singles7
    _, cases = rc.run_pair(gpu, synth_frames, SEEDS7[2:3], group=0, frame_base=40, singles=False)
    rc.assert_cases_equal_singles(single[2:3], cases)


def test_frame_ids_replace_the_counter(gpu, synth_frames, singles7):
    single, _ = singles7
    sel = [7, 2, 12]
    _, cases = rc.run_pair(gpu, [synth_frames[i] for i in sel], SEEDS7, group=3, frame_ids=[40 + i for i in sel], singles=False)
    for j, i in enumerate(sel):
        for c, s in enumerate(single):
            for k in rc.SINGLE_KEYS:
                assert rc.same(s[k][i], cases[k][j, c]), (k, i, c)


def test_against_the_oracle(gpu, synth_frames, singles7):
    from oracle import rescale_oracle as ro
    single, cases = singles7
    for f in (0, 5, 7, 12):
        fr = synth_frames[f]
        P = fr.survivors()
        ids = fc.point_list(fr, single[0]["tri_flags"][f])
        pts = P[ids]
        for c, seed in enumerate(SEEDS7[:3]):
            pos = ro.device_triples(seed, 40 + f, ids)
            counts = np.zeros(len(pos), np.int32)
            for h, t in enumerate(pos):
                v = ids[list(t)]
                if len(set(v.tolist())) == 3:
                    counts[h] = ro.count_inliers(ro.estimate_plane(pts[list(t)]), pts, ro.RANSAC_THRESHOLD)
            m, ic, used = ro.run_ransac(pts, pos, repeated_counts_zero=True)
            assert np.array_equal(cases["hyp_counts"][f, c], counts), (f, c)
            assert int(cases["best_ic"][f, c]) == ic and int(cases["used"][f, c]) == used, (f, c)
            m = m if m[1] >= 0 else -m
            np.testing.assert_allclose(cases["model"][f, c], m, rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(cases["raw_scale"][f, c], ro.scale_from_model(m, fc.ABS_REF), rtol=1e-9)


# ---- crafted frames ---------------------------------------------------------------------------------------------------------------
def test_crafted_few_exactly_twelve_declined_and_forms(gpu):
    frames = [rc.few_frame(), rc.exactly_min_frame(), rc.packed_frame(), rc.gather_frame(), rc.small_dense_frame(), rc.packed_frame()]
    dt = [0, 0, 0, 0, 0, 3]                                                          # the last frame's triangulation "declined"
    single, cases = rc.run_pair(gpu, frames, SEEDS7[:4], group=3, dt_status=dt)
    rc.assert_cases_equal_singles(single, cases)
    assert np.all(cases["status"][0] == fc.ST_RS_FEW) and int(single[0]["n_kept"][0]) == 3
    assert int(single[0]["n_kept"][1]) == 4 and np.all(cases["status"][1] == 0) and np.all(np.isfinite(cases["raw_scale"][1]))
    assert np.all(cases["status"][5] == fc.ST_EMPTY) and np.all(np.isnan(cases["raw_scale"][5])) and np.all(np.isnan(cases["model"][5]))
    assert np.all(cases["best_ic"][5] == 0) and np.all(cases["used"][5] == 0) and fc.all_bytes(cases["hyp_counts"][5], 0xFF)
    want = [rc.expected_form(f, single[0]["tri_flags"][i]) for i, f in enumerate(frames)]
    want[5] = rc.FORM_NONE
    assert cases["count_form"].tolist() == want
    assert {rc.FORM_NONE, rc.FORM_GATHER, rc.FORM_PACKED} == set(want)               # every form was exercised


def test_crafted_frame_over_max_feat_is_refused_neighbours_untouched(gpu):
    frames = [rc.small_dense_frame(), rc.packed_frame(), fc.road_frame("road100", 60, 40, 309)]
    single, cases = rc.run_pair(gpu, frames, SEEDS7[:3], group=2, max_feat=1000)
    rc.assert_cases_equal_singles(single, cases)
    assert np.all(cases["status"][1] == fc.ST_MASK) and np.all(np.isnan(cases["raw_scale"][1])) and np.all(np.isnan(cases["model"][1]))
    assert np.all(cases["best_ic"][1] == 0) and np.all(cases["used"][1] == 0) and fc.all_bytes(cases["hyp_counts"][1], 0xFF)
    assert int(cases["count_form"][1]) == rc.FORM_NONE
    assert np.all(cases["status"][[0, 2]] == 0)
    alone = rc.run_pair(gpu, [frames[0]], SEEDS7[:3], group=2, singles=False)[1]
    for k in rc.SINGLE_KEYS:
        assert rc.same(alone[k][0], cases[k][0]), k


def test_crafted_more_rows_than_max_tri_is_refused(gpu):
    frames = [rc.small_dense_frame(), rc.exactly_min_frame()]
    single, cases = rc.run_pair(gpu, frames, SEEDS7[:2], max_tri=20)                 # the first frame has 29 rows
    rc.assert_cases_equal_singles(single, cases)
    assert np.all(cases["status"][0] == fc.ST_MASK) and np.all(cases["status"][1] == 0)


def test_crafted_repeated_vertex_spends_its_iteration(gpu):
    f = fc.grid_frame()
    fl = rc.cpu_flags(f)
    H, Cn = 20, 3
    tr = rc.repeated_vertex_triples(f, fl, Cn, H)
    single, cases = rc.run_pair(gpu, [f], SEEDS7[:Cn], n_hyp=H, id_triples=tr[None], use_keep=False)
    rc.assert_cases_equal_singles(single, cases)
    assert np.all(cases["hyp_counts"][0, :, 0] == 0) and int(cases["hyp_counts"][0, 0, 1]) == 0
    assert np.all(cases["hyp_counts"][0, :, 2:].max(axis=1) > 0) and np.all(cases["used"][0] >= 2)


def test_crafted_singular_row(gpu):
    """The cases kernel does not recompute the heights: the frame's MVOSR_ST_ERR_SINGULAR is the flat selection's to report, and
    ScaleEstimator._collect_cases — what raw_scale_cases_batch returns — merges it.  The merged result equals the single runs."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    frames = [rc.singular_frame(), rc.small_dense_frame()]
    single, cases = rc.run_pair(gpu, frames, SEEDS7[:3], group=2)
    assert int(single[0]["status"][0]) == fc.ST_SINGULAR
    rc.assert_cases_equal_singles(single, cases, frames=[1])

    class Out:
        views = {k: None for k in ("raw_scale", "model", "best_ic", "used", "status", "count_form")}

        def __getitem__(self, k):
            return type("V", (), {"download": staticmethod(lambda: cases[k].copy())})
    res = ScaleEstimator._collect_cases({"status": single[0]["status"].copy()}, Out())
    for c, s in enumerate(single):
        for f in range(2):
            for k in ("raw_scale", "model", "best_ic", "used", "status"):
                assert rc.same(s[k][f], res["case_" + k][f, c]), (k, f, c)


# ---- RepeatedRuns against single estimators -----------------------------------------------------------------------------------------
def _sequence(n=96, seed=41):
    from mvoscalerecovery_amd import offline, synth
    data = synth.synth_sequence_dict(n, base_seed=seed, n_lo=120, n_hi=1500, p_not_moving=0.04, p_too_few=0.04)
    kinds = offline.plan_sequence(data)
    assert (kinds == 0).any() and (kinds == 2).any()
    proc = [i for i, k in enumerate(kinds) if k == 1]
    at = [proc[7], proc[len(proc) - 9]]
    fr = _declining([(np.asarray(data["feature3ds"][i]), np.asarray(data["feature2ds"][i])) for i in at], [0, 1])
    for i, (a3, a2) in zip(at, fr):
        data["feature3ds"][i], data["feature2ds"][i] = a3, a2
    return data, [proc.index(i) for i in at]


def _small_chunks(est):
    est.GPU_CHUNK = est.GPU_MIN_CHUNK = 20
    return est


@pytest.mark.parametrize("mode", [dict(triangulation="gpu"), dict(triangulation="scipy", sampling="device")], ids=["gpu", "scipy-device"])
def test_repeated_runs_equal_single_estimators(gpu, mode):
    from mvoscalerecovery_amd import offline
    from mvoscalerecovery_amd.rescale import RepeatedRuns, ScaleEstimator, case_seeds
    data, declined = _sequence()
    seeds = case_seeds(2024, 3)
    assert seeds == rc.case_seeds(2024, 3)                                           # the documented rule, restated in tests/repeats_cases.py
    rr = RepeatedRuns(1.75, window_size=5, seed=2024, cases=3, delaunay_workers=0, **mode)
    _small_chunks(rr.estimator)
    res = rr.run(data)
    assert res["scales"].shape == (3, 96) and np.array_equal(res["kinds"], offline.plan_sequence(data))
    if mode["triangulation"] == "gpu":
        assert rr.estimator.last_declined >= 2
    for c, s in enumerate(seeds):
        est = _small_chunks(ScaleEstimator(1.75, window_size=5, ransac_seed=s, delaunay_workers=0, **mode))
        one = offline.run_sequence_batched(data, est)
        assert np.array_equal(res["scales"][c], one["scales"]), c
        assert np.array_equal(res["error"][c], one["error"]), c
        assert np.array_equal(res["raw_scale"][c], est.last["raw_scale"], equal_nan=True), c
    assert not np.array_equal(res["scales"][0], res["scales"][1])                    # the cases are different runs
    # one run over the dict = two runs over its halves
    halves = [{k: v[:48] for k, v in data.items()}, {k: v[48:] for k, v in data.items()}]
    r2 = RepeatedRuns(1.75, window_size=5, seeds=seeds, delaunay_workers=0, **mode)
    _small_chunks(r2.estimator)
    both = np.concatenate([r2.run(halves[0])["scales"], r2.run(halves[1])["scales"]], axis=1)
    assert np.array_equal(both, res["scales"]) and np.array_equal(r2.scales(), res["scales"])
    sp = rr.spread()
    assert sp["scale_mean"].shape == (96,) and np.allclose(sp["scale_mean"], res["scales"].mean(axis=0))


# ---- the reference's own ten runs ---------------------------------------------------------------------------------------------------
def test_the_references_ten_runs(gpu):
    """tests/golden/rescale_repeats.npz (make_golden_repeats.py): /root/reference/src/rescale.py's ScaleEstimator run ten times over a
    40-frame dict, random.sample replaying _ransac_triples(seed_c, call, n).  The device path with the triples mapped to point ids
    reproduces all ten scales rows to rtol 1e-9, the tolerance of the existing main_offline golden test."""
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import RepeatedRuns
    z, meta = load_npz("rescale_repeats.npz")
    data = synth.synth_sequence_dict(meta["n_frames"], base_seed=meta["seed"], **meta["kw"])
    ids, ids_off, ran, seeds = z["ids"], z["ids_off"], z["ran"], [int(s) for s in z["seeds"]]
    Cn, Fp = len(seeds), len(ran)
    triples = np.zeros((Cn, Fp, 100, 3), np.int32)
    for c in range(Cn):
        call = -1
        for k in range(Fp):
            lst = ids[ids_off[k]:ids_off[k + 1]]
            if ran[k]:
                call += 1
                triples[c, k] = lst[_ransac_triples(seeds[c], call, len(lst))]
    rr = RepeatedRuns(meta["abs_ref"], window_size=meta["window"], seeds=seeds, triangulation="gpu", delaunay_workers=0)
    res = rr.run(data, id_triples=triples)
    assert res["scales"].shape == z["scales"].shape == (10, meta["n_frames"])
    np.testing.assert_allclose(res["scales"], z["scales"], rtol=1e-9, atol=0)


# ---- distribution ---------------------------------------------------------------------------------------------------------------------
def test_distribution_of_two_hundred_cases_in_one_call(gpu):
    """The existing criterion of test_rescale_device_distribution_matches_the_unseeded_reference — means within 3 standard errors,
    Kolmogorov-Smirnov p > 0.01 — on ONE raw_scale_cases_batch call with the 200 seeds 1000..1199."""
    from scipy import stats
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    z, meta = load_npz("rescale_distribution.npz")
    frames = [synth.synth_frame(fr["frame_idx"], fr["n"], base_seed=fr["seed"], upper_fraction=fr["upper_fraction"]) for fr in meta["frames"]]
    runs = int(meta["runs"])
    est = ScaleEstimator(meta["abs_ref"], window_size=5, triangulation="gpu", ransac_seed=0, delaunay_workers=0)
    r = est.raw_scale_cases_batch([f[0] for f in frames], [f[1] for f in frames], [1000 + s for s in range(runs)])
    dev = r["raw_scale"]
    assert dev.shape == (runs, len(frames)) and np.all(r["status"] == 0)
    for k in range(len(frames)):
        ref = z["f%d_raw_scales" % k]
        d = dev[:, k]
        se = np.sqrt(ref.var(ddof=1) / len(ref) + d.var(ddof=1) / len(d))
        assert abs(ref.mean() - d.mean()) <= 3 * se + 1e-12, (k, ref.mean(), d.mean(), se)
        assert stats.ks_2samp(ref, d).pvalue > 0.01, (k, stats.ks_2samp(ref, d))
