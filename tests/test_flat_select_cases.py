"""The crafted frames of tests/test_gpu_flat_select.py checked without a GPU, NumPy (float64 LAPACK) in the kernel's place: the family
set covers every exit of the median select, the constant of the height bound is what NumPy itself needs against mpmath, the rows
left out of the flag comparison stay within their caps, and the references agree with one another on the frames."""
import numpy as np
import pytest

import flat_cases as fc

NOMINAL_MAX_POINTS = 3400          # (160 KB of LDS: what ScaleEstimator._max_points() gives on an MI355X)


@pytest.fixture(scope="module")
def families():
    fam = dict(fc.select_families())
    fam.update(fc.tail_families(NOMINAL_MAX_POINTS))
    return {n: (f, fc.numpy_flat(f)) for n, f in fam.items()}


def test_family_set_covers_every_exit_of_the_select(families):
    plans = {n: fc.select_plan(hk[(fl & 1) != 0]) for n, (f, (hk, fl)) in families.items()}
    cov = fc.coverage(plans.values())
    assert not cov["missing"], cov
    assert {0, 1, 2, 3, 64, 65, 66} <= {p["k"] for p in plans.values()}
    # what each crafted case was tuned for, on NumPy's heights (the GPU test asserts the set only: the kernel's heights differ by ulps)
    assert (plans["control"]["exit"], plans["control"]["passes"], plans["control"]["cand"]) == ("direct", 1, 1)
    assert (plans["one_row_x100"]["exit"], plans["k1"]["exit"]) == ("range0", "range0")
    assert plans["cluster300"]["exit"] == "direct" and plans["cluster300"]["passes"] >= 5
    assert plans["cluster200"]["exit"] == "direct" and plans["cluster200"]["passes"] >= 5 and plans["cluster200"]["cand"] >= 2
    assert plans["shift0"]["exit"] == "pattern" and plans["shift0"]["passes"] >= 5
    assert (plans["direct64"]["exit"], plans["direct64"]["passes"], plans["direct64"]["cand"]) == ("direct", 1, 64)
    assert (plans["direct63"]["exit"], plans["direct63"]["cand"]) == ("direct", 63)
    assert plans["direct65"]["passes"] == 2                               # 65 candidates: another pass
    assert plans["direct_tie"]["exit"] == "direct" and plans["direct_tie"]["tie"] and plans["direct_tie"]["cand"] >= 4


def test_even_count_cases_are_what_their_notes_say(families):
    """(a) the copies of the lower middle end exactly at rank khi, (a3) one further, (b) the upper middle is another value, (c) the
    copies end at klo — counted on NumPy's heights (bit-identical for a repeated row)."""
    want = {"even_a": 1, "even_a3": 2, "even_b": 0, "even_c": 0}
    for name, extra in want.items():
        hk, fl = families[name][1]
        s = np.sort(hk[(fl & 1) != 0])
        k = len(s)
        assert k % 2 == 0
        klo, khi = (k - 1) // 2, k // 2
        le = int((s <= s[klo]).sum())
        assert le - khi == extra, (name, le, khi)
        assert (s[khi] == s[klo]) == (extra > 0)
    hk, fl = families["even_c"][1]
    s = np.sort(hk[(fl & 1) != 0])
    assert s[(len(s) - 1) // 2] == s[(len(s) - 1) // 2 - 1]                 # (c): the lower middle IS repeated


def test_height_constant_and_left_out_rows(families):
    """NumPy's solve against mpmath over every family: the largest error in units of kappa 2^-53 is what C_HEIGHT was taken from (a
    factor 4 on it), the flags agree with the mpmath verdict wherever the bound decides, and the undecided rows stay within 2 % of a
    family (50 % of the threshold family, with both sides of both thresholds left)."""
    worst = 0.0
    for name, (f, (hk, fl)) in families.items():
        h, pitch, kappa = fc.mp_rows(f)
        ok = ~f.skip
        ratio = np.abs(hk[ok].astype(np.longdouble) - h[ok]) / np.abs(h[ok]) / (kappa[ok] * fc.U53)
        worst = max(worst, float(ratio.max()))
        bits, dec0, dec1 = fc.flag_reference(pitch[ok], kappa[ok])
        assert np.array_equal((fl[ok] & 1)[dec0], (bits & 1)[dec0]) and np.array_equal((fl[ok] & 2)[dec1], (bits & 2)[dec1]), name
        cap = 0.5 if name == "thresholds" else 0.02
        assert (~dec0).mean() <= cap and (~dec1).mean() <= cap, (name, int((~dec0).sum()), int((~dec1).sum()))
        if name == "thresholds":
            assert (~dec0).any() and (~dec1).any()                          # the bisected rows ARE inside the bound
            assert {0, 1} <= set((bits & 1)[dec0].tolist()) and {0, 2} <= set((bits & 2)[dec1].tolist())
            s80, s85 = np.sin(np.deg2rad(fc.LOOSE_DEG)), np.sin(np.deg2rad(fc.TIGHT_DEG))
            mu = np.sin(np.deg2rad(pitch[ok]))
            assert (np.abs(mu - s80) <= 1e-12).sum() >= 3 and (np.abs(mu - s85) <= 1e-12).sum() >= 3       # the kernel's asin branch
    assert worst <= fc.C_HEIGHT_MEASURED, worst
    assert fc.C_HEIGHT >= 4 * fc.C_HEIGHT_MEASURED


def test_bad_and_singular_rows_are_what_the_kernel_will_see(families):
    for name in ("singular", "bad_and_singular"):
        f = families[name][0]
        for row in f.tri[f.skip & ~f.bad]:
            assert np.linalg.matrix_rank(f.xyz[row]) < 3
    f = families["bad_ids"][0]
    assert ((f.tri[f.bad] < 0) | (f.tri[f.bad] >= len(f.xyz))).any(1).all()


def test_tail_frames_layouts_and_pinned_counts(families):
    """The counting layout the source's conditions give each tail frame (NumPy's kept rows), and on the planar frames the two
    np.longdouble count bounds coincide for the drawn hypotheses."""
    from oracle import rescale_oracle as ro
    lay = {}
    for name, (f, (hk, fl)) in families.items():
        _, kept = fc.expected_discrete(hk, fl, 0.9)
        L = f.tri[kept].reshape(-1)
        if f.status or len(L) < fc.MIN_POINTS:
            continue
        lay[name] = fc.count_layout(len(L), len(f.survivors()), len(f.tri), len(np.unique(L)))
        if name in ("grid", "road_small", "fan_dedup", "fan_packed", "keep_few"):
            tr = L[ro.device_triples(5, 0, L, 129)]
            lo, hi = fc.count_bounds(f.survivors(), L, tr)
            assert np.array_equal(lo, hi), name
            m, tol = fc.plane_ld(f.survivors(), tr[int(np.argmax(lo))])
            assert tol < 1e-9 and abs(float(np.sum(m * m)) - 1.0) < 1e-15
    assert (lay["road_packed"], lay["road_dedup"], lay["control"], lay["grid"]) == ("packed", "dedup", "list", "dedup")
    assert (lay["fan_dedup"], lay["fan_packed"], lay["at_max_points"]) == ("dedup", "packed", "packed")
    f = families["keep_over_4096"][0]
    assert len(f.xyz) > 4096 and (f.keep >= 0).sum() == 500 and {-1, 0, 1} <= set(f.keep.tolist())
    assert set(families["keep_few"][0].keep.tolist()) == {-1, 1}


def test_replay_rule():
    assert fc.replay([0, 0, 0], 30) == (-1, 0, 3)
    assert fc.replay([3, 5, 5, 4], 30) == (1, 5, 4)
    assert fc.replay([3, 25, 29], 30) == (1, 25, 2)                          # 25 > 0.8 * 30: stop
    assert fc.replay([24, 24, 25, 30], 30) == (2, 25, 3)                     # 24 is not above the goal, 25 is


def test_graph_cases_cover_what_the_vote_test_needs():
    from oracle import rescale_oracle as ro
    cases = fc.graph_cases()
    codes, nvs = set(), {}
    for c in cases:
        codes |= set(ro.edge_code(c["v"], c["z"], c["tri"]).tolist())
        nvs[c["name"]] = int(ro.graph_inliers(c["v"], c["z"], c["tri"])[0].sum())
    assert codes == set(range(8))
    assert nvs["exactly_10"] == 10 and nvs["exactly_11"] == 11 and nvs["random"] <= 10 < max(nvs.values())
    c = [c for c in cases if c["name"] == "ties_and_minus_zero"][0]
    prods = [(c["v"][r[i]] - c["v"][r[j]]) * (c["z"][r[i]] - c["z"][r[j]]) for r in c["tri"] for i, j in ((0, 1), (1, 2), (0, 2))]
    assert any(p == 0 and np.signbit(p) for p in prods) and any(p == 0 and not np.signbit(p) for p in prods)
    assert np.bincount(c["tri"].reshape(-1), minlength=len(c["v"])).min() == 0
