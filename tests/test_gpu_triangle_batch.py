"""triangle_batch_kernel (csrc/mvosr_rescale.hip) on crafted frames through mvosr_triangle_batch with a hand-built batch header:
the rows from 4096 on that every sweep recomputes, the statuses _SINGULAR, _MASK and _EMPTY, frames with none, one and two equal
kept rows (0 / 0, sd == 0, both clip comparisons strict), rows on both sides of both keep thresholds, and a frame larger than the
header's max_feat.  Needs a real MI355X.

Reference: mpmath at 60 digits per row, the rest in np.longdouble (tests/tribatch_cases.py).  counts exact wherever no row is
undecided (s further than C_HEIGHT kappa_inf(A) 2^-53 relative from 0.98 — flat_cases.C_HEIGHT, the same plane_normal — and no kept
height within the derived bound of mean -+ 3 sd: asserted on the CPU for every family but `threshold_band`, which is held to count
bounds only); height within (cnt2 + 8) 2^-53 relative of the mpmath mean over the same rows — three roundings per Y, two for the
row's sum, 2 u for the third, cnt2 - 1 for a sum of cnt2 positive terms in any order, one for the division, one spare.  NumPy
float64 uses 0.003 of that bound on the CPU (tests/test_tribatch_cases.py)."""
import numpy as np
import pytest

import tribatch_cases as tc

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a["counts"] == b["counts"] and a["status"] == b["status"] and np.float64(a["height"]).tobytes() == np.float64(b["height"]).tobytes()


@pytest.fixture(scope="module")
def fam():
    return tc.families()


@pytest.fixture(scope="module")
def batch(gpu, fam):
    """name -> outputs, every family in ONE launch (the empty frames first, in the middle and last)."""
    return dict(zip(fam, tc.run_tri(gpu, list(fam.values()))))


def _check(name, f, o):
    assert o["status"] == f.status, (name, o)
    if f.status == tc.ST_EMPTY:
        assert o["counts"] == (0, 0) and np.isnan(o["height"]), (name, o)
        return
    if f.status == tc.ST_SINGULAR:
        return                                                    # (the singular row's own s is inf / inf or 0 / 0: nothing is asserted on it)
    r = tc.reference(f)
    assert r["kept_lo"] <= o["counts"][0] <= r["kept_hi"], (name, o, r)
    if f.band:
        assert 0 <= o["counts"][1] <= o["counts"][0]
        return
    if f.expect is not None:
        assert o["counts"] == f.expect[0] and np.isnan(o["height"]), (name, o)
        return
    assert o["counts"] == (r["kept_lo"], r["cnt2"]), (name, o, r["kept_lo"], r["cnt2"])
    if r["cnt2"] == 0:
        assert np.isnan(o["height"]), (name, o)
        return
    rel = float(abs(np.longdouble(o["height"]) - r["height"]) / r["height"])
    print("%-16s counts %s  |h_kernel - h_mpmath| / bound: %.4f" % (name, o["counts"], rel / tc.height_tol(r["cnt2"])))
    assert rel <= tc.height_tol(r["cnt2"]), (name, o["height"], float(r["height"]), rel, tc.height_tol(r["cnt2"]))


def test_every_family_in_one_batch(batch, fam):
    """height, counts and status of every family against the mpmath reference (a row with a bad id is left out of the frame's
    statistics, the rows around it count as usual)."""
    for name, f in fam.items():
        _check(name, f, batch[name])
    assert batch["none_kept"]["counts"] == (0, 0) and batch["none_kept"]["status"] == 0
    assert batch["one_kept"]["counts"] == (1, 0) and batch["two_equal"]["counts"] == (2, 0)
    assert batch["bad_and_singular"]["status"] == tc.ST_MASK


def test_recomputed_rows(batch, fam):
    """`many_rows`: the rows t >= 4096 carry ten of the kept heights, the clipped outlier and steep rows (what each sweep's
    recompute loop decides: tests/test_tribatch_cases.py); the copy with those rows below 4096 gives identical counts and a height
    within the two sums' bound of the first's."""
    a, b = batch["many_rows"], batch["many_rows_moved"]
    r = tc.reference(fam["many_rows"])
    assert a["counts"] == b["counts"] == (r["kept_lo"], r["cnt2"]) and r["cnt2"] == r["kept_lo"] - 1
    assert abs(a["height"] - b["height"]) <= 2 * r["cnt2"] * tc.U53 * abs(a["height"]), (a, b)


def test_batch_equals_frames_alone_and_itself(gpu, batch, fam):
    again = tc.run_tri(gpu, list(fam.values()))
    for (name, f), o2 in zip(fam.items(), again):
        assert _same(batch[name], o2), (name, "two launches differ", batch[name], o2)
        alone = tc.run_tri(gpu, [f])[0]
        assert _same(batch[name], alone), (name, "batch != alone", batch[name], alone)


def test_frame_larger_than_the_header(gpu, fam):
    """max_feat sizes the launch's LDS: a frame with more features than it states is refused — MVOSR_ST_ERR_MASK, NaN height,
    counts (0, 0) — and the frames around it are processed as usual."""
    names = ("one_kept", "control", "two_equal", "empty_middle", "none_kept")
    frames = [fam[n] for n in names]
    small = max(len(f.feats) for f in frames if f.name != "control")
    assert small < len(fam["control"].feats)
    out = tc.run_tri(gpu, frames, max_feat=small)
    assert out[1]["status"] == tc.ST_MASK and out[1]["counts"] == (0, 0) and np.isnan(out[1]["height"]), out[1]
    for i in (0, 2, 3, 4):
        _check(names[i], frames[i], out[i])
        assert _same(out[i], tc.run_tri(gpu, [frames[i]])[0]), names[i]


def test_camera_heights_equals_the_direct_call(gpu, batch, fam):
    """triangle_batch.camera_heights(tris=...) passes the rows through: `control` equals the direct call."""
    from mvoscalerecovery_amd import triangle_batch
    f = fam["control"]
    h, counts, status = triangle_batch.camera_heights([f.feats], tris=[f.tri])
    o = batch["control"]
    assert np.float64(h[0]).tobytes() == np.float64(o["height"]).tobytes() and tuple(int(c) for c in counts[0]) == o["counts"] and status[0] == o["status"]
