"""CPU: the NumPy restatement of the point-cloud contract (tests/cloud_cases.py) against the reference's recorded run
(tests/golden/depth_*.npz: coverage, and the depths of every ``stride``-th covered pixel in the order the reference appended
them) and on a hand-made image.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import cloud_cases as cc
import depth_cases as dc


@pytest.fixture(scope="module")
def golden_frames():
    """(name, frame, restated depth image) for the frames of the three depth fixtures — computed once."""
    out = []
    for name in ("depth_small", "depth_full", "depth_ties"):
        for i, fr in enumerate(dc.load_fixture(name)):
            out.append(("%s[%d]" % (name, i), fr, dc.depth64(fr["datas"], fr["tri"], fr["cam"])))
    return out


def test_golden_counts_order_and_depths(golden_frames):
    for label, fr, depth in golden_frames:
        cam, tri = fr["cam"], fr["tri"]
        pts, cols = cc.cloud(depth, tri, cam)
        assert cols is None and pts.dtype == np.float64
        assert len(pts) == int((tri >= 0).sum()), label                      # one point per covered pixel
        sy, sx, d_ref = dc.stored_depths(fr)
        z = pts[::fr["stride"], 2]
        assert np.array_equal(z, depth[sy, sx]), (label, "raster order: the reference's append order")
        # ... and those z are the reference's recorded depths within the fixture's own bound
        yy, xx, d_true, unit = dc.truth(fr["f3"], fr["rows"], tri, cam)
        s = fr["stride"]
        factor = dc.bound_factor(fr["ref_err_units"])
        assert dc.err_units(z, d_true[::s], unit[::s]).max() <= factor, label
        assert dc.err_units(d_ref, d_true[::s], unit[::s]).max() <= factor, label
        # x and y: the ray times z, each product rounded once
        px = (xx.astype(np.float64) - cam.cx) / cam.fx
        py = (yy.astype(np.float64) - cam.cy) / cam.fy
        assert np.array_equal(pts[:, 0], px * pts[:, 2]) and np.array_equal(pts[:, 1], py * pts[:, 2]), label
        assert np.array_equal(pts[:, 2], depth[yy, xx]), label
        # float32 is the float64 value rounded once
        p32, _ = cc.cloud(depth, tri, cam, dtype=np.float32)
        assert p32.dtype == np.float32 and np.array_equal(p32, pts.astype(np.float32)), label
        # without ids the depth image alone gives the same cloud here (no covered pixel of depth 0)
        assert (depth[tri >= 0] != 0).all() and cc.same_bytes(cc.cloud(depth, None, cam)[0], pts), label


def test_hand_made_image():
    d, tri = cc.hand_image()
    cam = SimpleNamespace(width=7, height=5, fx=2.0, fy=4.0, cx=3.0, cy=2.0)
    # ids: every id >= 0, zeros included, raster order
    pts, _ = cc.cloud(d, tri, cam)
    yy, xx = np.nonzero(tri >= 0)
    assert len(pts) == 22 and np.array_equal(pts[:, 2], d[yy, xx], equal_nan=True)
    assert np.array_equal(pts[0], [(0 - 3.0) / 2.0 * 1.0, (0 - 2.0) / 4.0 * 1.0, 1.0])
    k = int(np.nonzero((yy == 2) & (xx == 0))[0][0])
    assert np.signbit(pts[k, 2]) and pts[k, 2] == 0.0                        # the covered -0.0 stays -0.0
    assert np.isnan(pts[2]).all()                                            # NaN depth: a NaN point, kept without a range
    # no ids: depth != 0 — the two zero-depth covered pixels are lost, NaN stays
    p0, _ = cc.cloud(d, None, cam)
    assert len(p0) == 20 and np.isnan(p0[:, 2]).sum() == 1
    # range: closed interval on depth * scale; NaN fails; inf fails a finite far
    pr, _ = cc.cloud(d, tri, cam, depth_range=(2.0, 12.0))
    assert pr[:, 2].tolist() == [2.0, 5.0, 7.0, 3.0, 4.0, 6.0, 8.0, 9.0, 10.0, 11.0, 12.0]
    pr, _ = cc.cloud(d, tri, cam, depth_range=(-np.inf, np.inf))
    assert len(pr) == 21 and not np.isnan(pr[:, 2]).any() and np.isinf(pr[:, 2]).sum() == 2
    pr, _ = cc.cloud(d, tri, cam, depth_range=(0.0, 0.0))
    assert len(pr) == 2 and (pr[:, 2] == 0).all()                           # -0.0 >= 0.0: the zeros are in [0, 0]
    # scale: applied before the range test, one multiplication
    ps, _ = cc.cloud(d, tri, cam, scale=0.5, depth_range=(2.0, 12.0))
    assert ps[:, 2].tolist() == [2.5, 3.5, 2.0, 3.0, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5]
    # stride: rows 0, 3 and columns 0, 3, 6 at stride 3
    p3, _ = cc.cloud(d, tri, cam, stride=3)
    assert p3[:, 2].tolist()[:1] == [1.0] and np.isnan(p3[1, 2]) and p3[2:, 2].tolist() == [7.0, 10.0, 0.5]
    p4, _ = cc.cloud(d, tri, cam, stride=4)                                  # rows 0, 4 and columns 0, 4
    assert p4[:, 2].tolist() == [1.0, 5.0]
    # colours: BGR -> RGB, / 255.0, float32 = astype
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    _, col = cc.cloud(d, tri, cam, image=img)
    assert np.array_equal(col, img[yy, xx, ::-1] / 255.0) and col[0].tolist() == [2 / 255.0, 1 / 255.0, 0.0]
    _, c32 = cc.cloud(d, tri, cam, image=img, dtype=np.float32)
    assert c32.dtype == np.float32 and np.array_equal(c32, col.astype(np.float32))
    # the batch form
    pts2, cols2, off = cc.clouds(np.stack([d, d]), np.stack([tri, np.full_like(tri, -1)]), cam, images=np.stack([img, img]))
    assert off.tolist() == [0, 22, 22] and cc.same_bytes(pts2, pts) and cc.same_bytes(cols2, col)


def test_crafted_batches_are_what_they_say():
    for w, h in ((7, 5), (64, 4), (65, 63), (311, 95)):
        names, depth, tri, images, scales = cc.crafted_batch(w, h)
        assert len(set(names)) == len(names) == len(depth) and names[-1] == "hostile"
        n = w * h
        cnt = dict(zip(names, (tri.reshape(len(names), -1) >= 0).sum(1)))
        assert cnt["all"] == n and cnt["none"] == 0 and cnt["first"] == 1 and cnt["last"] == 1 and cnt["row"] == w
        assert cnt["upto_wave-1"] == min(63, n) and cnt["upto_segment+1"] == min(4097, n)
        assert ("tail" in cnt) == (n % cc.SEGMENT != 0)
        assert np.array_equal((tri >= 0)[:-1], (depth != 0)[:-1])            # the two coverage rules agree off the hostile frame
        assert np.isnan(depth[-1]).any() and (depth[-1] == 0).any() and (tri[-1] >= 0).all()
