"""The `rescale` variant's oracle (oracle/rescale_oracle.py) against goldens produced by running the
reference's own rescale.ScaleEstimator with random.sample replaying a recorded triple sequence
(tests/golden/make_golden.py: make_rescale)."""
import numpy as np

from conftest import load_npz
from oracle import rescale_oracle as ro


def ransac_triples(seed, call, n, h=100):
    rng = np.random.default_rng([seed, call])
    return np.stack([rng.choice(n, 3, replace=False) for _ in range(h)]).astype(np.int32)


def test_graph_demo_kat():
    """graph.py:156-165 self-demo (column [3,4,4,0,12,16,16,0], marginals [0.8, 0.3636.., 0.3636..])."""
    z, _ = load_npz("rescale.npz")
    tp = ro.triangle_potential()
    assert np.array_equal(tp, z["demo_tp"])
    idx = int(ro.edge_code(np.array([0.0, 1.0, 2.0]), np.array([2.0, 1.0, 1.0]), np.array([[0, 1, 2]]))[0])
    assert idx == int(z["demo_index"])
    assert tp[:, idx].tolist() == [3, 4, 4, 0, 12, 16, 16, 0]
    assert np.array_equal(ro.vertex_probabilities(tp)[idx], z["demo_prob"])


def test_rescale_sequence_golden():
    from mvoscalerecovery_amd import synth
    z, meta = load_npz("rescale.npz")
    call = {"k": -1}

    frame = {"i": 0}

    def sampler(n):
        call["k"] += 1
        if "f%d_list_triples" % frame["i"] in z.files:          # frame 26: every tenth triple names one vertex twice (the reference's
            return z["f%d_list_triples" % frame["i"]]           # random.sample draws such rank-deficient samples 0.5-2 % of the time)
        return ransac_triples(meta["ransac_seed"], call["k"], n)
    est = ro.OracleRescaleEstimator(meta["abs_ref"], window_size=meta["window"], sampler=sampler)
    for i, fr in enumerate(meta["frames"]):
        frame["i"] = i
        f3, f2 = synth.synth_frame(fr["frame_idx"], fr["n"], base_seed=fr["seed"], upper_fraction=fr["upper_fraction"])
        assert synth.checksum(f3, f2) == fr["crc"]
        s, sd = est.scale_calculation(f3, f2)
        assert np.array_equal(est.last["valid"], z["f%d_valid" % i]), i
        fs = est.last["flat"]
        assert np.array_equal(fs.ids, z["f%d_ids" % i]), i
        assert fs.height_level == float(z["f%d_height_level" % i])
        assert np.array_equal(fs.heights_loose, z["f%d_heights_loose" % i])
        if "f%d_model" % i in z.files:
            assert np.array_equal(est.last["model"], z["f%d_model" % i]), i
            assert est.last["best_ic"] == int(z["f%d_best_ic" % i])
            assert est.last["used"] == int(z["f%d_used" % i])
        assert s == float(z["f%d_scale" % i]) and sd == 1, i


def test_road_norm_helpers_golden():
    """Oracle restatements of the RANSAC consumers against what the reference itself returned with the same sample
    sequence (tests/golden/road_norm.json): road_model_calculation_ransac (scale_calculator.py:366-384) and the 2-D
    line variant get_pitch_line_ransac (estimate_road_norm.py:39-49,60-64)."""
    import json
    import os
    import numpy as np
    from oracle import rescale_oracle as ro
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "road_norm.json")))
    for c in g["planes"]:
        pts = np.array(c["pts"])
        h, pitch, inl = ro.road_model_ransac(pts, np.array(c["triples"]))
        assert abs(h - c["height"]) <= 1e-12 * abs(c["height"]) and abs(pitch - c["pitch"]) <= 1e-12
        assert int(inl.sum()) == c["n_inliers"]
    for c in g["lines"]:
        xy = np.array(c["xy"])
        m, ic, used = ro.run_ransac_line(xy, np.array(c["pairs"]), 0.01)
        assert ic == c["best_ic"] and used == c["used"]
        ref = np.array(c["model"])
        assert min(np.abs(m - ref).max(), np.abs(m + ref).max()) <= 1e-12          # SVD null vector: sign is arbitrary


def test_rescale_row_form_invariance_golden():
    """What makes the device triangulation usable for this estimator without a declared deviation: on the reference's own
    frames (tests/golden/rescale.npz) the vote's mask and flat_selection's kept triangles are the same whether the rows
    are SciPy's or brought to canonical form (vertex ids ascending, rows sorted) — graph.py:18-36,124-145 is symmetric in
    a row's vertices, rescale.py:75-96 keeps a set.  Only the ORDER of the point list (:101) follows the rows."""
    from mvoscalerecovery_amd import synth
    z, meta = load_npz("rescale.npz")
    est = ro.OracleRescaleEstimator(meta["abs_ref"], window_size=meta["window"], device_seed=5)
    for i, fr in enumerate(meta["frames"]):
        f3, f2 = synth.synth_frame(fr["frame_idx"], fr["n"], base_seed=fr["seed"], upper_fraction=fr["upper_fraction"])
        est.scale_calculation(f3, f2)
        assert np.array_equal(est.last["valid"], z["f%d_valid" % i]), i
        fs = est.last["flat"]
        assert np.array_equal(np.sort(fs.ids), np.sort(z["f%d_ids" % i])), i
        assert abs(fs.height_level - float(z["f%d_height_level" % i])) <= 1e-12 * abs(fs.height_level)
        assert np.array_equal(ro.canonical_rows(est.last["tri2"]), est.last["tri2"])


def test_sample_sequence_pinned_values():
    """The values every restatement of the sample sequence is held to (csrc/mvosr_ransac.hpp asserts the first two at compile time),
    and the pair draw and the evaluation runs' case key beside the triple draw."""
    assert ro.mix64(0) == 0xe220a8397b1dcdaf
    assert ro.mix64(1) == 0x910a2dec89025cc1
    assert ro.device_triples(7, 3, 12, 4).tolist() == [[6, 3, 11], [7, 9, 5], [10, 11, 1], [2, 11, 6]]
    assert np.array_equal(ro.key_draws(ro.frame_key(7, 3), 12, 4), ro.device_triples(7, 3, 12, 4))
    k = ro.eval_case_key(7, 3, 0)
    assert k != ro.frame_key(7, 3) and k != ro.eval_case_key(7, 3, 1)
    assert np.array_equal(ro.key_draws(k, 12, 50, 2), ro.key_draws(k, 12, 50)[:, :2])        # the pair: the triple's first two
    assert ro.device_triples(5, 0, 3, 20).min() == 0 and all(sorted(r) == [0, 1, 2] for r in ro.device_triples(5, 0, 3, 20).tolist())


def test_device_sample_sequence():
    """The counter-based sample sequence: three distinct positions below m, a function of (seed, frame counter,
    hypothesis) only, and close to uniform over positions."""
    a = ro.device_triples(7, 3, 50)
    assert a.shape == (100, 3) and a.min() >= 0 and a.max() < 50
    assert all(len(set(r)) == 3 for r in a.tolist())
    assert np.array_equal(a, ro.device_triples(7, 3, 50)) and not np.array_equal(a, ro.device_triples(7, 4, 50))
    assert not np.array_equal(a, ro.device_triples(8, 3, 50))
    small = ro.device_triples(1, 0, 12, n_hyp=2000)
    counts = np.bincount(small.reshape(-1), minlength=12)
    assert counts.min() > 400 and counts.max() < 600                      # 500 expected per position
    assert ro.mix64(0) == 0xE220A8397B1DCDAF                              # splitmix64's first output for state 0
    # a list that repeats its vertices (rescale.py:101): the positions are distinct, the VERTICES need not be — such a sample spends
    # its iteration as in the reference (ransac.py:8-21; rounds 4-5 drew it again: a declared deviation that is gone), at the rate
    # uniform positions give: P(two of three positions name one vertex) = 1 - (21/23)(18/22) = 0.253 for 8 vertices x 3
    ids = np.repeat(np.arange(8), 3)
    t = ro.device_triples(3, 9, ids, n_hyp=2000)
    assert all(len(set(r)) == 3 for r in t.tolist()) and len({tuple(r) for r in t.tolist()}) > 1200
    repeated = np.mean([len(set(ids[list(r)])) < 3 for r in t.tolist()])
    assert 0.22 < repeated < 0.29, repeated
    assert np.array_equal(t, ro.device_triples(3, 9, len(ids), n_hyp=2000))       # (the draw does not look at the ids)
    # ... and counts zero inliers in the restated loop, whatever plane rounding noise would have picked
    pts = np.random.default_rng(0).normal(size=(24, 3))
    pts[:, 1] = 1.0 + 1e-4 * pts[:, 1]
    pts = pts[np.repeat(np.arange(8), 3)]
    m, ic, used = ro.run_ransac(pts, [(0, 1, 5), (0, 5, 9)], repeated_counts_zero=True)
    m2, ic2, used2 = ro.run_ransac(pts, [(0, 5, 9)], repeated_counts_zero=True)
    assert np.array_equal(m, m2) and ic == ic2 and used == 2 and used2 == 1
