"""-m gpu: reliability_kernel (mvosr_reliability_batch) against tests/reliability_cases (the NumPy restatement of the reference's
find_reliability_by_graph) and the reference's own run (tests/golden/reliability.npz), through the C ABI, the stage method and
``ScaleEstimator(vote="reliability")``.  Reliabilities are compared as bytes (NaN to NaN), masks and statuses exactly: every
operation of the update is a single IEEE binary64 operation, so there is no tolerance."""
import numpy as np
import pytest

import flat_cases as fc
import reliability_cases as rc

pytestmark = pytest.mark.gpu

CRAFTED = sorted(rc.crafted_cases())
REFUSED = sorted(rc.refused_cases())


def _same_values(a, b):
    """Two arrays of doubles equal bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def _assert_case(got, want, what):
    assert got["status"] == want["status"], (what, got["status"])
    assert np.array_equal(got["keep"], want["keep"]), what
    if want["reliability"] is not None:
        assert _same_values(got["reliability"], want["reliability"]), what


def _bytes(r):
    return (np.ascontiguousarray(r["reliability"]).tobytes(), np.ascontiguousarray(r["keep"]).tobytes(), r["status"])


@pytest.fixture(scope="module")
def cases():
    c = dict(rc.crafted_cases())
    c.update(rc.refused_cases())
    return c


@pytest.fixture(scope="module")
def expected(cases):
    return {n: c.expected() for n, c in cases.items()}


def _run_by_pitch(gpu, cases):
    """All cases in ragged batches, one launch per camera pitch -> name -> result."""
    out = {}
    for pitch in sorted({c.pitch for c in cases.values()}):
        names = sorted(n for n, c in cases.items() if c.pitch == pitch)
        out.update(zip(names, rc.run_cases(gpu, [cases[n] for n in names])))
    return out


@pytest.fixture(scope="module")
def batch(gpu, cases):
    both = dict(cases)
    m = cases["mesh700"]
    both["mesh700_pitched"] = rc.Case("mesh700_pitched", m.tri, m.z, m.v, y=m.y, pitch=cases["pitched"].pitch)    # company for `pitched`
    return _run_by_pitch(gpu, both)


@pytest.fixture(scope="module")
def alone(gpu, cases):
    return {n: rc.run_cases(gpu, [c])[0] for n, c in cases.items()}


@pytest.mark.parametrize("name", CRAFTED + REFUSED)
def test_case_equals_the_restatement_alone_and_in_a_ragged_batch(name, expected, alone, batch):
    _assert_case(alone[name], expected[name], name)
    _assert_case(batch[name], expected[name], name + " (batch)")
    if expected[name]["reliability"] is not None:
        assert _bytes(alone[name]) == _bytes(batch[name]), name


def test_pitch_zero_gives_the_plain_values(batch, expected):
    assert not _same_values(batch["mesh700_pitched"]["reliability"], batch["mesh700"]["reliability"])      # the remap is applied ...
    assert _same_values(batch["mesh700"]["reliability"], expected["mesh700"]["reliability"])               # ... and is the identity at 0


def test_repeated_launch_is_identical(gpu, cases, batch):
    again = _run_by_pitch(gpu, cases)
    for n in cases:
        assert _bytes(again[n]) == _bytes(batch[n]), n


@pytest.mark.parametrize("limit", ["max_feat", "max_tri"])
def test_header_contract(gpu, cases, expected, limit):
    """A frame with more features than the header's max_feat, or more rows than max_tri = 2 max_feat, is refused before LDS is
    touched: MVOSR_ST_ERR_MASK, keep all -1, its reliabilities not written; the others are served; guards stay as they were."""
    if limit == "max_feat":
        names, over, kw = ["strip63", "strip65", "no_rows", "fan_low_hub5"], "strip65", {"max_feat": 66}      # strip65: 67 features
        cs = [cases[n] for n in names]
    else:
        rng = np.random.default_rng(5)
        z, v = rc._depth_rows(rng, 4)
        rows = np.array([[0, 1, 2], [1, 2, 3], [0, 2, 3]] * 3)                                                 # 9 rows > 2 * 4
        many = rc.Case("many_rows", rows, z, v)
        names, over, kw = ["one_triangle", "many_rows", "eight_rows"], "many_rows", {"max_feat": 4}
        cs = [cases["one_triangle"], many, rc.Case("eight_rows", rows[:8], z, v)]
    res, tails = rc.run_cases(gpu, cs, sentinel=0xA5, **kw)
    for k, t in tails.items():
        assert len(np.ravel(t)) >= 1 and fc.all_bytes(t, 0xA5), k
    for n, c, r in zip(names, cs, res):
        if n == over:
            assert r["status"] == rc.ST_MASK and (r["keep"] == -1).all() and len(r["keep"]) == c.n_feat, n
            assert fc.all_bytes(r["reliability"], 0xA5), n
        else:
            _assert_case(r, c.expected(), n)


def test_too_large_launches_are_refused(gpu):
    from mvoscalerecovery_amd import _lib
    c = rc.crafted_cases()["one_triangle"]
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvosr.h")) as fh:
        assert re.search(r"MVOSR_ERR_TOO_LARGE = -3\b", fh.read())
    for max_feat in (2400, 3000, 21846, 70000):       # beyond the 160 KB of LDS (twice); beyond 16-bit offers; beyond 16-bit ids
        with pytest.raises(_lib.MvosrLibraryError, match=r"mvosr_reliability_batch failed \(-3\)"):
            rc.run_cases(gpu, [c], max_feat=max_feat)
    assert rc.run_cases(gpu, [c], max_feat=2356)[0]["status"] == 0        # the largest header the 160 KB admit


# ---- the reference's own run -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vote_frames():
    z = rc.golden()
    out = []
    for k in range(int(z["n_vote"])):
        idx, n = (int(x) for x in z["v%d_spec" % k])
        f3, f2, rows = rc.synth_vote_frame(idx, n)
        out.append((f3, f2, rows, np.unpackbits(z["v%d_mask" % k])[:len(f3)].astype(bool), z["v%d_reliability" % k]))
    return out


def test_golden_frames_equal_the_reference_run(gpu, vote_frames):
    cs = [rc.Case("golden%d" % k, rows, f3[:, 2], f2[:, 1], y=f3[:, 1]) for k, (f3, f2, rows, _, _) in enumerate(vote_frames)]
    for r, (_, _, _, mask, rel) in zip(rc.run_cases(gpu, cs), vote_frames):
        assert r["status"] == 0 and r["reliability"].tobytes() == rel.tobytes()
        assert np.array_equal(r["keep"] == 0, mask)


def test_find_reliability_by_graph_equals_the_reference_masks(gpu, vote_frames, capsys):
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    est = ScaleEstimator(1.75, 5, triangulation="scipy", delaunay_workers=0, verbose=True)
    for f3, f2, rows, mask, rel in vote_frames:
        keep3 = f3.copy()
        got = est.find_reliability_by_graph(f3, f2, rows)
        assert got.dtype == bool and np.array_equal(got, mask) and np.array_equal(f3, keep3)
        assert est.last_reliability.tobytes() == rel.tobytes()
        lines = capsys.readouterr().out.strip().splitlines()[-3:]
        assert lines[0].startswith("reliability ") and lines[1] == "feature rejected  %d" % int((~mask).sum())
        assert lines[2] == "feature left      %d" % int(mask.sum())
    with pytest.raises(ValueError):
        est.find_reliability_by_graph(f3, f2, np.array([[0, 1, 1]]))


# ---- the estimator ---------------------------------------------------------------------------------------------------------------
def _estimator(**kw):
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    return ScaleEstimator(1.75, 5, triangulation="scipy", delaunay_workers=0, mutate_inputs=False, **kw)


@pytest.fixture(scope="module")
def sequence():
    from mvoscalerecovery_amd import synth
    frames = rc.sequence_frames()
    z = rc.golden()
    crc = 0
    for f3, f2 in frames:
        crc = synth.checksum(np.array([crc], dtype=np.int64), f3, f2)
    assert crc == int(z["seq_crc"]), "synthetic generator drifted from the fixture"
    return frames, z


def test_estimator_reproduces_the_sequence_frame_by_frame(gpu, sequence):
    frames, z = sequence
    est = _estimator(vote="reliability")
    for i, (f3, f2) in enumerate(frames):
        s, sd = est.scale_calculation(f3, f2)
        assert s == z["seq_scales"][i] and sd == z["seq_stds"][i], (i, s, z["seq_scales"][i])
        assert est.last_raw_scale[0] == z["seq_raw"][i] and int(est.last_status[0]) == int(z["seq_status"][i]), i
        assert int(est.last_counts[0][0]) == int(z["seq_kept"][i]), i
    assert est.flat_feature is not None and len(est.flat_feature) == len(est.flat_feature_2d) > 0


def test_estimator_reproduces_the_sequence_as_a_batch(gpu, sequence):
    frames, z = sequence
    est = _estimator(vote="reliability")
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    scales, stds = est.scale_calculation_batch(f3s, f2s)
    assert np.array_equal(scales, z["seq_scales"]) and np.array_equal(stds, z["seq_stds"])
    assert np.array_equal(est.last_raw_scale, z["seq_raw"]) and np.array_equal(est.last_status, z["seq_status"])
    # the two halves on their own (what a sharded driver calls), in two blocks
    est2 = _estimator(vote="reliability")
    parts = [est2.raw_scale_batch(f3s[a:b], f2s[a:b]) for a, b in ((0, 20), (20, 36))]
    assert not parts[0][3] and not parts[1][3]
    raw, status, level = (np.concatenate([p[k] for p in parts]) for k in range(3))
    s2, d2 = est2.push_raw_scales(raw, status, level)
    assert np.array_equal(s2, z["seq_scales"]) and np.array_equal(d2, z["seq_stds"])
    # the last frame's selected points, produced when they are read, equal the per-frame call's
    one = _estimator(vote="reliability")
    one.scale_calculation(f3s[-1], f2s[-1])
    assert np.array_equal(est.flat_feature, one.flat_feature) and np.array_equal(est.flat_feature_2d, one.flat_feature_2d)
    # ... and are what the stage methods select on that frame: the survivors' selection mapped back to the frame's features
    from mvoscalerecovery_amd import constants as K
    from scipy.spatial import Delaunay
    r3 = f3s[-1].copy()
    one.feature_remap(r3)
    low = f2s[-1][:, 1] > K.VANISH
    l3, l2 = r3[low], f2s[-1][low]
    mask = one.find_reliability_by_graph(l3, l2, Delaunay(l2).simplices)
    picked = one.feature_selection_by_tri(l3[mask], Delaunay(l2[mask]).simplices)
    assert 0 < len(picked) < int(mask.sum()) < len(mask)
    assert np.array_equal(est.flat_feature, l3[mask][picked]) and np.array_equal(est.flat_feature_2d, l2[mask][picked])
    # ... and differ from find_outliers' result on this sequence, or the keyword would test nothing
    base, _ = _estimator().scale_calculation_batch(f3s, f2s)
    assert int((np.asarray(base) != scales).sum()) >= 10


@pytest.mark.parametrize("idx", [276, 516])
def test_three_survivors_are_one_triangle(gpu, idx):
    """Six features of which the vote keeps exactly three: the reference triangulates them (:266, one row) and, with no steep
    triangle to set a level, takes the "no enough flat feature" branch (:277-279, :420-422) — not the three-FEATURE branch (:263)."""
    from oracle import scale_oracle as so
    from mvoscalerecovery_amd import synth
    f3, f2 = synth.synth_frame(idx, 6, base_seed=555, upper_fraction=0.0)
    r3, low = so.remap(f3), so.lower_mask(f2)
    mask = rc.sequential(so.delaunay(f2[low]), r3[low][:, 2], f2[low][:, 1], int(low.sum())) > rc.START
    assert int(low.sum()) == 6 and int(mask.sum()) == 3
    sel = so.tri_select(r3[low][mask], so.delaunay(f2[low][mask]))
    assert not sel.singular and sel.selected_ids.shape[0] == 0
    with np.errstate(all="ignore"):
        want = float(np.float64(1.75) / np.float64(sel.height_level))
    est = _estimator(vote="reliability")
    raw, status, level, errors = est.raw_scale_batch([f3, f3], [f2, f2])
    assert not errors and list(status) == [so.ST_NO_FLAT] * 2 and int(est.last_counts[0][0]) == 3
    assert _same_values(raw, [want, want]) and _same_values(level, [sel.height_level] * 2)
    if np.isfinite(want):
        s, sd = est.scale_calculation(f3, f2)
        assert s == want and sd == 100 and est.flat_feature is None


def test_feature_selection_takes_the_configured_vote(gpu, sequence):
    from mvoscalerecovery_amd import constants as K
    frames, _ = sequence
    f3, f2 = frames[3][0].copy(), frames[3][1]
    est, base = _estimator(vote="reliability"), _estimator()
    est.feature_remap(f3)
    sel = est.feature_selection(f3, f2)
    low = f2[:, 1] > K.VANISH
    from scipy.spatial import Delaunay
    mask = est.find_reliability_by_graph(f3[low], f2[low], Delaunay(f2[low]).simplices)
    picked = est.feature_selection_by_tri(f3[low][mask], Delaunay(f2[low][mask]).simplices)
    assert np.array_equal(sel, f3[low][mask][picked])
    assert not np.array_equal(mask, base.find_outliers(f3[low], f2[low], Delaunay(f2[low]).simplices))


def test_default_vote_is_byte_identical_to_no_keyword(gpu, sequence):
    frames, _ = sequence
    f3s, f2s = [f[0] for f in frames[:9]], [f[1] for f in frames[:9]]
    a, b = _estimator(vote="outliers"), _estimator()
    sa, sb = a.scale_calculation_batch(f3s, f2s), b.scale_calculation_batch(f3s, f2s)
    for x, y in zip(sa, sb):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert np.asarray(a.last_raw_scale).tobytes() == np.asarray(b.last_raw_scale).tobytes()
    assert np.asarray(a.last_status).tobytes() == np.asarray(b.last_status).tobytes()
    assert np.asarray(a.last_counts).tobytes() == np.asarray(b.last_counts).tobytes()
    assert list(a.scale_queue) == list(b.scale_queue) and a.height_level == b.height_level
    pa, pb = a.scale_calculation(f3s[0], f2s[0]), b.scale_calculation(f3s[0], f2s[0])
    assert pa == pb and np.array_equal(a.flat_feature, b.flat_feature)


def test_constructor_refuses_what_is_not_built(gpu):
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    with pytest.raises(ValueError, match="scipy"):
        ScaleEstimator(1.75, 5, triangulation="gpu", vote="reliability")
    with pytest.raises(ValueError, match="vote"):
        ScaleEstimator(1.75, 5, triangulation="scipy", vote="graph")
    est = _estimator(vote="reliability")
    with pytest.raises(ValueError, match="tri2s"):
        est.scale_calculation_batch([np.zeros((5, 3))], [np.zeros((5, 2))], tri1s=[np.zeros((0, 3), np.int32)], tri2s=[np.zeros((0, 3), np.int32)])


def test_metric_survivors_follow_the_vote(gpu, sequence):
    import depth_cases as dc
    from mvoscalerecovery_amd import constants as K
    from mvoscalerecovery_amd import reconstruct
    from scipy.spatial import Delaunay
    frames, _ = sequence
    f3s, f2s = [f[0] for f in frames[:2]], [f[1] for f in frames[:2]]
    est = _estimator(vote="reliability")
    _, l3, l2, rows, masks, _ = reconstruct._metric_survivors(est, f3s, f2s, dc.camera(1241, 376), np.ones(2))
    for f in range(2):
        r3 = f3s[f].copy()
        est.feature_remap(r3)
        low = f2s[f][:, 1] > K.VANISH
        want = est.find_reliability_by_graph(r3[low], f2s[f][low], Delaunay(f2s[f][low]).simplices)
        assert np.array_equal(masks[f], want) and np.array_equal(rows[f], Delaunay(l2[f][want]).simplices)
