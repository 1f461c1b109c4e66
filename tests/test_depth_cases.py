"""CPU: tests/depth_cases.py against the reference's recorded run (tests/golden/depth_*.npz, made by
tests/golden/make_golden_depth.py), and the reference itself against every condition the GPU tests impose — so a GPU
failure cannot be the fixture's fault."""
import numpy as np
import pytest

import depth_cases as dc

FIXTURES = ("depth_small", "depth_full", "depth_ties")


@pytest.fixture(scope="module", params=FIXTURES)
def fixture_frames(request):
    return request.param, dc.load_fixture(request.param)          # (load_fixture checks the CRC of the regenerated inputs)


def test_rule_reproduces_the_reference(fixture_frames):
    name, frames = fixture_frames
    for i, fr in enumerate(frames):
        cam = fr["cam"]
        tri, claims = dc.locate(fr["f2"], fr["rows"], cam.width, cam.height)
        ref = fr["tri"]
        assert np.array_equal(tri >= 0, ref >= 0), (name, i, "coverage")                       # 0 pixels excluded
        ties = claims > 1
        assert np.array_equal(tri[~ties], ref[~ties]), (name, i, "ids off ties")
        assert dc.all_contained(fr["f2"], fr["rows"], tri, ties), (name, i, "the rule's pick on tie pixels")
        assert dc.all_contained(fr["f2"], fr["rows"], ref, ties), (name, i, "the reference's pick on tie pixels")
        if name == "depth_ties":
            assert ties.sum() > 1000                                                             # the fixture is there for them
        # depths: float64 restatement within the bound of the exact value, on the rule's own triangles
        factor = dc.bound_factor(fr["ref_err_units"])
        datas = dc.model64(fr["f3"], fr["rows"])
        yy, xx, d_true, unit = dc.truth(fr["f3"], fr["rows"], tri, cam)
        units = dc.err_units(dc.depth64(datas, tri, cam)[yy, xx], d_true, unit)
        assert units.max() <= factor, (name, i, units.max(), factor)


def test_reference_meets_the_conditions_of_the_gpu_tests(fixture_frames):
    name, frames = fixture_frames
    for i, fr in enumerate(frames):
        cam = fr["cam"]
        assert 0.0 < fr["ref_err_units"] < 1.0, (name, i, fr["ref_err_units"])                 # measured 0.19 - 0.39
        # the stored depths are within ref_err_units of the exact value of the reference's own triangle: ties "truth" to its formula
        yy, xx, d_true, unit = dc.truth(fr["f3"], fr["rows"], fr["tri"], cam)
        s = fr["stride"]
        sy, sx, d_ref = dc.stored_depths(fr)
        assert np.array_equal(sy, yy[::s]) and len(d_ref) == len(sy)
        units = dc.err_units(d_ref, d_true[::s], unit[::s])
        assert units.max() <= fr["ref_err_units"], (name, i, units.max())
        # The reference's datas.  The device's datas are compared with the EXACT planes (depth_cases.model_true), never with these,
        # so no GPU condition rests on them; they are checked for what an explicit inverse can promise: each of the three entries
        # of a row of A^-1 is off by up to one unit 2**-52 * cond2(A), their sum n by up to three, the normalisation adds
        # rounding of its own — 4 units.  (Measured: up to 2.46 units in height, 1.76 in the normal — depth_small frames 5 and 2;
        # the errors of n and of height cancel in the depth, which stays below 0.39 units.  So the reference's datas do NOT meet
        # the max(1, 4 * ref_err_units) = 1.0 - 1.5 units the device's datas are held to in test_gpu_depth.py.)
        assert dc.model_within(fr["datas"], fr["f3"], fr["rows"], 4.0).all(), (name, i)
        assert fr["datas"].shape == (len(fr["rows"]), 4) and (fr["datas"][:, 1] >= 0).all()


def test_locate_edge_cases():
    f2 = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [4.0, 4.0]])
    rows = np.array([[0, 1, 2], [3, 2, 1]])
    tri, claims = dc.locate(f2, rows, 6, 5)
    assert (tri[:, 5] == -1).all() and (tri[:5, :5] >= 0).all()                                # the square, closed
    diag = [(y, 4 - y) for y in range(5)]
    assert all(claims[y, x] == 2 and tri[y, x] == 0 for y, x in diag)                           # shared edge: both claim, the lowest row wins
    assert claims.sum() == 25 + 5
    # a flat row and a row outside the image claim nothing
    tri2, claims2 = dc.locate(np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [-9.0, -9.0], [-5.0, -9.0], [-9.0, -5.0]]),
                              np.array([[0, 1, 2], [3, 4, 5]]), 4, 4)
    assert (tri2 == -1).all() and claims2.sum() == 0
    assert dc.contains_exact(f2, rows[0], 2, 2) and not dc.contains_exact(f2, rows[0], 3, 2)
