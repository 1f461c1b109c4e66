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


# ---- large images, many frames, strides: the inputs of the GPU tests are what they are meant to be -------------------------

def test_divmod_small_restatement_over_its_whole_range():
    """cl_span / cloud_fill_kernel / depth_raster_kernel: divmod_small(i, d, 1.0f / d) — the float32 estimate and its two
    corrections equal divmod(i, d) for EVERY i in [0, 2^22), the range the launchers keep it in (kClMaxSide = 2^21 plus a
    segment), at the divisors of the tests (widths, strides) and at the range's top."""
    i = np.arange(1 << 22, dtype=np.int64)
    for d in (1, 2, 3, 5, 7, 63, 64, 65, 311, 1241, 4095, 4096, 4097, 5121, 8200, 20472, (1 << 21) - 1, 1 << 21):
        q, r = cc.divmod_small(i, d)
        assert np.array_equal(q, i // d) and np.array_equal(r, i % d), d
    for d in (8199, 8201, 2 ** 31 - 1):                                          # the other strides; float32 cannot represent the last: 2^31 - 1 -> 2^31
        assert d in cc.STRIDES
        q, r = cc.divmod_small(i, d)
        assert np.array_equal(q, i // d) and np.array_equal(r, i % d), d
    assert np.float32(2 ** 31 - 1) == np.float32(2 ** 31) and np.float32(8201) == 8201


def test_large_batch_cuts_land_where_they_are_meant_to():
    """The cuts of the many-segment and thin / wide images: an edge one pixel before / at / after a segment boundary, and
    inside a row or at a row end as the size's note says.  (Masks only: no frame of 2 M pixels is drawn here.)"""
    S = cc.SEGMENT
    for label, (w, h, cuts) in list(cc.MANY_SEGMENTS.items()) + list(cc.THIN_WIDE.items()):
        n = w * h
        nseg = -(-n // S)
        names = cc.large_names(cuts, teeth=label == "2097152x1")
        assert names[:2] == ["all", "checker"] and len(names) == len(set(names)) == 2 + 6 * len(cuts) + (6 if "teeth_0+0" in names else 0)
        assert cc.large_mask("all", w, h).all() and cc.large_mask("checker", w, h).sum() in (n // 2, (n + 1) // 2)
        for c in cuts:
            assert 0 < c < n, (label, c)
            at_boundary = c % S == 0
            assert at_boundary or (c + 1) % S == 0, (label, c)                   # a boundary, or the last pixel before one
            for delta in (-1, 0, 1):
                e = c + delta
                up, fr = cc.large_mask("upto_%d%+d" % (c, delta), w, h), cc.large_mask("from_%d%+d" % (c, delta), w, h)
                assert up.sum() == e and up[:e].all() and not up[e:].any(), (label, c, delta)
                assert np.array_equal(fr, ~up), (label, c, delta)
                # the segments' counts: full ones, then e % S pixels in the segment of the edge, then empty ones
                per = np.add.reduceat(up.astype(np.int64), np.arange(0, n, S))
                assert len(per) == nseg and (per[:e // S] == S).all() and (per[e // S + 1:] == 0).all() and (e % S == 0 or per[e // S] == e % S)
            if at_boundary:                                                      # one pixel before / at / after: the edge is in the segment before, between two, in the one after
                assert (c - 1) // S == c // S - 1 and (c + 1) // S == c // S
        bounds = {c for c in cuts if c % S == 0}
        if label in ("1x5000", "5000x1", "4097x3"):
            assert bounds == set(range(S, n, S)), (label, "every boundary the image reaches")
    # the sizes are what the table says
    assert [-(-w * h // S) for w, h, _ in cc.MANY_SEGMENTS.values()] == [256, 258, 515]
    w, h, cuts = cc.MANY_SEGMENTS["4096x256"]
    assert all(c % w in (0, w - 1) for c in cuts)                                # every segment is one row: a cut is a row end too
    w, h, cuts = cc.MANY_SEGMENTS["4100x257"]
    assert all(c % w > 0 and (c % w) + S > w for c in cuts)                      # the segment that begins at the cut straddles a row end
    w, h, cuts = cc.MANY_SEGMENTS["8200x257"]
    assert w > 2 * S and [c // S for c in cuts] == [256, 512, 513]               # the scan's second and third round begin at 256 and 512
    assert any((c % w) + S <= w for c in cuts) and any((c % w) + S > w for c in cuts)    # a segment inside one row, and one across a row end
    w, h, cuts = cc.THIN_WIDE["2097152x1"]
    assert w == cc.MAX_SIDE and -(-w // S) == 512 and [c // S for c in cuts] == [256, 511]
    for delta in (-1, 0, 1):                                                     # teeth / gaps: an edge at EVERY boundary + delta
        t, g = cc.large_mask("teeth_0%+d" % delta, w, h), cc.large_mask("gaps_0%+d" % delta, w, h)
        assert np.array_equal(t, ~g)
        edges = np.nonzero(t[1:] != t[:-1])[0] + 1
        want = np.arange(0, w + S, S) + delta                                    # (the image's two ends shifted into it count as well)
        assert np.array_equal(edges, want[(want > 0) & (want < w)]), delta
    # a small batch is drawn as crafted_batch draws it, and a part of it holds the values of the whole
    names, depth, tri, images, scales = cc.large_batch(311, 95, [S], seed=3)
    assert names == cc.large_names([S]) and depth.shape == (8, 95, 311) and images.shape == (8, 95, 311, 3) and scales.shape == (8,)
    assert (tri[0] == 5).all() and np.isnan(depth[0]).any() and (depth[0] == 0).any()                    # "all" holds the hostile pattern
    assert np.array_equal((tri >= 0)[1:], (depth != 0)[1:]) and (depth[1:][tri[1:] >= 0] >= 0.5).all()
    for f, k in enumerate(names):
        assert np.array_equal((tri[f] >= 0).reshape(-1), cc.large_mask(k, 311, 95)), k
    part = cc.large_batch(311, 95, [S], seed=3, frames=names[3:5])
    assert part[0] == names[3:5] and all(cc.same_bytes(a, b[3:5]) for a, b in zip(part[1:], (depth, tri, images, scales)))


def test_stride_cases_counts():
    """The restatement on the stride cases: from max(width, height) upward only pixel (0, 0) is on the grid, so a frame's count
    is 1 when it covers that pixel and 0 otherwise; below, the grid's size bounds it and the fully covered frame reaches it."""
    from mvoscalerecovery_amd.reconstruct import grid_points
    for w, h in cc.STRIDE_SIZES:
        cam = SimpleNamespace(width=w, height=h, fx=0.6 * w, fy=0.6 * w, cx=0.5 * w, cy=0.5 * h)
        names, depth, tri, images, scales = cc.large_batch(w, h, [cc.SEGMENT])
        covers_origin = tri[:, 0, 0] >= 0
        assert covers_origin.any() and not covers_origin.all()
        for s in cc.STRIDES:
            off = cc.clouds(depth, tri, cam, stride=s)[2]
            cnt = np.diff(off)
            assert (cnt <= grid_points(w, h, s)).all() and cnt[0] == grid_points(w, h, s), (w, h, s)     # "all" (ids): the whole grid
            if s >= max(w, h):
                assert grid_points(w, h, s) == 1 and np.array_equal(cnt, covers_origin.astype(np.int64)), (w, h, s)
            else:
                assert grid_points(w, h, s) > 1
        assert [s >= max(w, h) for s in cc.STRIDES] == ([False] * 4 + [True] * 3 if w == 8200 else [False] + [True] * 6)


def test_many_frames_batches_are_what_they_say():
    for F in (257, 513):
        seen = {}
        for turn in range(3):
            kinds = cc.special_kinds(F, turn)
            assert sorted(kinds) == [f for f in (255, 256, 257, 511, 512) if f < F]
            depth, tri, images, scales = cc.many_frames(7, 5, F, kinds, seed=turn)
            cnt = (tri.reshape(F, -1) >= 0).sum(1)
            assert np.array_equal(tri >= 0, depth != 0)
            for f, kind in kinds.items():
                assert cnt[f] == {"empty": 0, "full": 35, "single": 1}[kind], (F, turn, f)
                seen.setdefault(f, set()).add(kind)
            others = np.delete(cnt, sorted(kinds))
            assert others.min() >= 0 and 10 < others.mean() < 25                 # random coverage elsewhere
        assert all(v == {"empty", "full", "single"} for v in seen.values())      # every one of them each kind in turn
