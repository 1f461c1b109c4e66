"""The crafted frames of tests/test_gpu_triangle_batch.py checked without a GPU, NumPy float64 (oracle.triangle_batch_oracle) in the
kernel's place: no row of a family is undecided under the mpmath reference (but in `threshold_band`), no kept row sits within the
derived bound of a clip edge, the rows from 4096 on decide all three outputs of `many_rows`, and NumPy agrees with mpmath within
the derived height bound — the share of it that NumPy uses is printed and has not grown."""
import warnings

import numpy as np
import pytest

import tribatch_cases as tc


@pytest.fixture(scope="module")
def fam():
    return tc.families()


def _live(fam):
    return {n: f for n, f in fam.items() if len(f.tri)}


def test_rows_decided_and_clear_of_the_clip(fam):
    for name, f in _live(fam).items():
        r = tc.reference(f)
        if f.band:
            continue
        assert r["undecided"] == 0, (name, r)
        if f.expect is not None:
            hk = tc.kept_rows(f)
            hk = hk[~np.isnan(hk)]
            assert len(hk) == f.expect[0][0] == r["kept_lo"] and (hk == hk[0]).all(), name      # one bit pattern: sd == 0 exactly
            assert len({tuple(t) for t in f.tri[~np.isnan(tc.kept_rows(f))].tolist()}) == 1
        else:
            assert r["clip_clear"], (name, r)
    assert tc.reference(fam["none_kept"])["kept_hi"] == 0
    c = tc.reference(fam["control"])
    assert (c["kept_lo"], c["cnt2"]) == (425, 420) and len(fam["control"].feats) == 300 and len(fam["control"].tri) == 600


def test_many_rows_is_decided_by_its_recomputed_rows(fam):
    """The rows t >= 4096 hold kept rows of >= 10 distinct heights, the one clipped outlier and steep rows; leaving them out of any
    ONE sweep changes counts[0], counts[1] or the height by far more than its bound; the moved copy is the same multiset of rows with
    all of those below 4096."""
    a, b = fam["many_rows"], fam["many_rows_moved"]
    assert len(a.tri) == 4096 + 512 + 37 and len(a.feats) == 300
    hk = tc.kept_rows(a)
    s = tc.mp_rows(a)[0]
    tail = np.arange(len(a.tri)) >= tc.KEEP
    r = tc.reference(a)
    lo, hi = r["mean"] - 3 * r["sd"], r["mean"] + 3 * r["sd"]
    kt = hk[tail & ~np.isnan(hk)]
    assert len(np.unique(kt)) >= 10 and ((kt > hi) | (kt < lo)).sum() == 1 and (s[tail] < 0.95).any()
    assert not ((hk[~tail & ~np.isnan(hk)] > hi) | (hk[~tail & ~np.isnan(hk)] < lo)).any()      # the only clipped row is in the tail
    full = tc.sweeps(hk, tail, 0)
    assert (full[0], full[1]) == (r["kept_lo"], r["cnt2"]) and r["cnt2"] == r["kept_lo"] - 1
    for sweep in (1, 2, 3):
        cut = tc.sweeps(hk, tail, sweep)
        moved = cut[0] != full[0] or cut[1] != full[1] or abs(cut[2] - full[2]) > 100 * tc.height_tol(full[1]) * full[2]
        assert moved, (sweep, cut, full)
        print("sweep %d without its recompute loop: counts (%d, %d) height %.6f  (right: (%d, %d) %.6f)" % ((sweep,) + tuple(map(float, cut)) + tuple(map(float, full))))
    assert sorted(map(tuple, a.tri.tolist())) == sorted(map(tuple, b.tri.tolist())) and np.array_equal(a.feats, b.feats)
    hb = tc.kept_rows(b)
    assert not ((hb[tc.KEEP:] > hi) | (hb[tc.KEEP:] < lo)).any() and len(np.unique(hb[tc.KEEP:][~np.isnan(hb[tc.KEEP:])])) > 10


def test_threshold_band_has_both_sides_of_both_thresholds(fam):
    r = tc.reference(fam["threshold_band"])
    assert min(r["s_sides"]) >= 5 and min(r["h_sides"]) >= 4, r
    assert r["kept_lo"] >= 5 and r["kept_hi"] - r["kept_lo"] == r["undecided"] <= 4, r


def test_numpy_against_mpmath(fam):
    """oracle.triangle_batch_oracle.camera_height (float64 LAPACK) on every family with a reference: counts equal (within the
    bounds for the band), height within (cnt2 + 8) u of the mpmath mean over the same rows."""
    from oracle.triangle_batch_oracle import camera_height
    worst = 0.0
    for name, f in _live(fam).items():
        if f.skip.any():
            continue
        r = tc.reference(f)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            h, n_kept, n_clip = camera_height(f.feats, f.tri, tc.FOCUS, tc.CX, tc.CY)
        assert r["kept_lo"] <= n_kept <= r["kept_hi"], (name, n_kept, r)
        if f.band:
            continue
        if f.expect is not None:
            assert (n_kept, n_clip) == f.expect[0] and np.isnan(h), (name, n_kept, n_clip, h)
            continue
        assert n_clip == r["cnt2"], (name, n_clip, r)
        if r["cnt2"] == 0:
            assert np.isnan(h), name
            continue
        rel = float(abs(np.longdouble(h) - r["height"]) / r["height"])
        share = rel / tc.height_tol(r["cnt2"])
        print("%-16s counts (%d, %d)  |h_numpy - h_mpmath| / bound: %.4f" % (name, n_kept, n_clip, share))
        assert share <= 1.0, (name, share)
        worst = max(worst, share)
    print("largest share of the height bound NumPy uses: %.4f" % worst)
    assert worst <= tc.HEIGHT_SHARE_MEASURED


def test_bad_and_singular_rows_are_what_the_kernel_will_see(fam):
    f = fam["singular"]
    a, b, c = f.tri[f.skip][0]
    assert np.array_equal(f.feats[a], f.feats[b]) and a != b and f.status == tc.ST_SINGULAR
    f = fam["bad_id"]
    n = len(f.feats)
    assert {int(f.tri[f.skip].max()), int(f.tri[f.skip].min())} == {n, -1} and f.status == tc.ST_MASK
    f = fam["bad_and_singular"]
    assert f.tri[f.skip].max() == len(f.feats) and np.array_equal(f.feats[0], f.feats[len(f.feats) - 1]) and f.status == tc.ST_MASK
    names = list(fam)
    assert names[0].startswith("empty") and names[-1].startswith("empty") and any(n.startswith("empty") for n in names[1:-1])
    assert all(len(fam[n].feats) == 0 and len(fam[n].tri) == 0 for n in names if n.startswith("empty"))
