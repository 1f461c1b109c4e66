"""GPU: mvosr_dense_depth_batch / mvosr_triangle_model_batch and mvoscalerecovery_amd.reconstruct against the reference's
recorded run (tests/golden/depth_*.npz) and the CPU restatement (tests/depth_cases.py).

Every image comparison is over ALL pixels (0 excluded): coverage identical, ids identical off tie pixels, the device's
triangle an exact closed container on tie pixels; depths within max(1, 4 * ref_err_units) * unit * |truth| of the exact
value (depth_cases: the only tolerance), ``datas`` within the same multiple of 2**-52 * cond2(A).  Nothing here provokes a
fault: every hostile case is one the kernels answer with a status."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cloud_cases as cc
import depth_cases as dc

pytestmark = pytest.mark.gpu

ST_SINGULAR, ST_MASK, ST_EMPTY = 7, 8, 9
SENTINEL = 0x5A


def check_image(fr, depth, tri_id, datas, covered, rows=None, factor=None, label=""):
    """One frame of device output against the rule, the reference's image (when the fixture has it) and the exact depths.
    Returns the device's largest depth error in units."""
    cam = fr["cam"]
    rows = fr["rows"] if rows is None else rows
    factor = dc.bound_factor(fr["ref_err_units"]) if factor is None else factor
    want, claims = dc.locate(fr["f2"], rows, cam.width, cam.height)
    ties = claims > 1
    assert np.array_equal(tri_id >= 0, want >= 0), (label, "coverage vs the rule")
    assert np.array_equal(tri_id, want), (label, "ids vs the rule (lowest claiming row)")
    if "tri" in fr and rows is fr["rows"]:
        assert np.array_equal(tri_id >= 0, fr["tri"] >= 0), (label, "coverage vs the reference")
        assert np.array_equal(tri_id[~ties], fr["tri"][~ties]), (label, "ids vs the reference off ties")
    assert dc.all_contained(fr["f2"], rows, tri_id, ties), (label, "container check on tie pixels")
    assert int(covered) == int((want >= 0).sum()), (label, "covered")
    assert (depth[tri_id < 0] == 0.0).all(), (label, "uncovered pixels are 0")
    yy, xx, d_true, unit = dc.truth(fr["f3"], rows, tri_id, cam)
    units = dc.err_units(depth[yy, xx], d_true, unit)
    print("%s: %d covered, %d tie pixels, device depth error %.3f units (bound %.2f)" % (label, len(yy), int(ties.sum()), units.max(), factor))
    assert units.max() <= factor, (label, units.max(), factor)
    ok = dc.model_within(datas, fr["f3"], rows, factor)
    eh, en, _, _, _ = dc.model_errors(datas, fr["f3"], rows)
    print("%s: datas error %.3f (height) %.3f (normal) units" % (label, eh.max(), en.max()))
    assert ok.all(), (label, "datas", eh.max(), en.max(), factor)
    return float(units.max())


def launch(ctx, cam, f3s, f2s, rows, keeps=None, first=0, n=0, ids=True, which=1):
    """mvosr_dense_depth_batch through ctypes on a packed batch; every output pre-filled with SENTINEL bytes."""
    from mvoscalerecovery_amd import _lib, packing
    from mvoscalerecovery_amd.engine import DeviceBatch
    from mvoscalerecovery_amd.reconstruct import pack_all
    F, H, W = len(f3s), cam.height, cam.width
    pf = pack_all([np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in f3s], [np.asarray(b, dtype=np.float64).reshape(-1, 2) for b in f2s])
    off, flat = packing._pack_tris([np.ascontiguousarray(r, dtype=np.int32).reshape(-1, 3) for r in rows])
    if which == 1:
        pf.tri1_off, pf.tri1 = off, flat
        db = DeviceBatch(ctx, pf, with_tri2=False)
    else:
        pf.tri1_off, pf.tri1 = packing._pack_tris([np.zeros((0, 3), np.int32)] * F)
        pf.tri2_off, pf.tri2 = off, flat
        db = DeviceBatch(ctx, pf, with_tri2=True)
    d_u = ctx.to_device(pf.u)
    d_keep = None
    if keeps is not None:
        kp = np.zeros(len(pf.u), dtype=np.int32)
        for f in range(F):
            kp[pf.frame_slice(f)] = np.where(keeps[f], 0, -1)
        d_keep = ctx.to_device(kp)
    bufs = {"depth": ctx.empty((F, H, W), np.float64), "tri_id": ctx.empty((F, H, W), np.int32),
            "tri_model": ctx.empty((max(int(off[-1]), 1), 4), np.float64), "covered": ctx.empty(F, np.int32), "status": ctx.empty(F, np.int32)}
    for b in bufs.values():
        b.fill(SENTINEL)
    o = _lib.DepthOutputs(bufs["depth"].ptr, bufs["tri_id"].ptr if ids else None, bufs["tri_model"].ptr, bufs["covered"].ptr, bufs["status"].ptr)
    c = _lib.Camera(W, H, cam.fx, cam.fy, cam.cx, cam.cy)
    bs = db.struct()
    rc = ctx.lib.mvosr_dense_depth_batch(ctx.handle, C.byref(bs), which, d_u.ptr, d_keep.ptr if d_keep is not None else None, C.byref(c),
                                         C.byref(o), first, n)
    ctx.sync()
    out = {k: b.download() for k, b in bufs.items()}
    out["rc"], out["tri_off"] = rc, off
    for b in list(bufs.values()) + [d_u] + ([d_keep] if d_keep is not None else []):
        b.free()
    db.free()
    return out


def sentinel_like(a):
    return np.frombuffer(bytes([SENTINEL]) * a.nbytes, dtype=a.dtype).reshape(a.shape)


# ---- 1. the three fixtures ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["depth_small", "depth_full", "depth_ties"])
def test_fixtures_through_depth_maps(gpu, name):
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    worst = 0.0
    for i, fr in enumerate(dc.load_fixture(name)):
        rec = Reconstruct(fr["cam"], ctx=gpu)
        res = rec.depth_maps([fr["f3"]], [fr["f2"]], tris=[fr["rows"]], ids=True)
        assert res.status[0] == 0
        worst = max(worst, check_image(fr, res.depth[0], res.tri_id[0], res.datas[0], res.covered[0], label="%s[%d]" % (name, i)))
        # the stored reference depths, pixel by pixel (both within their bounds of the same exact value)
        sy, sx, d_ref = dc.stored_depths(fr)
        same = res.tri_id[0][sy, sx] == fr["tri"][sy, sx]
        _, _, d_true, unit = dc.truth(fr["f3"], fr["rows"], fr["tri"], fr["cam"])
        s = fr["stride"]
        gap = np.abs(res.depth[0][sy, sx] - d_ref)[same]
        lim = ((dc.bound_factor(fr["ref_err_units"]) + fr["ref_err_units"]) * unit[::s] * np.abs(d_true[::s]).astype(np.float64))[same]
        assert (gap <= lim).all(), (name, i, "device vs the reference's stored depths")
        # the keep path: all features, the fixture's survivor mask, rows numbered over the survivors — the same image bit for bit
        res_k = rec.depth_maps([fr["f3_all"]], [fr["f2_all"]], tris=[fr["rows"]], keeps=[fr["keep"]], ids=True)
        assert np.array_equal(res_k.depth, res.depth) and np.array_equal(res_k.tri_id, res.tri_id) and np.array_equal(res_k.datas[0], res.datas[0])
        # the reference's two methods
        if i == 0:
            assert np.array_equal(rec.triangle_model(fr["f3"], fr["rows"]), res.datas[0])
            one = rec.depth_generate(fr["f3"], fr["f2"], fr["rows"])
            assert np.array_equal(one.depth, res.depth[0]) and np.array_equal(one.tri_id, res.tri_id[0])
            assert one.points.shape == (int(res.covered[0]), 3) and np.array_equal(one.points[:, 2], res.depth[0][res.tri_id[0] >= 0])
    print("%s: device's largest depth error %.3f units" % (name, worst))


# ---- 2. batch == per-frame == sub-range; sentinels; determinism -----------------------------------------------------------

def ragged_batch():
    frames = [fr for fr in dc.load_fixture("depth_small") if (fr["cam"].width, fr["cam"].height) == (310, 94)]
    cam = frames[0]["cam"]
    f3s, f2s, rows = [fr["f3"] for fr in frames], [fr["f2"] for fr in frames], [fr["rows"] for fr in frames]
    f3s.insert(2, np.zeros((0, 3)))
    f2s.insert(2, np.zeros((0, 2)))
    rows.insert(2, np.zeros((0, 3), np.int32))                       # an empty frame
    f3s.append(np.array([[-1.0, 1.0, 5.0], [1.0, 1.2, 6.0], [0.0, 0.4, 9.0]]))
    f2s.append(np.array([[20.0, 80.0], [200.0, 85.0], [110.0, 30.0]]))
    rows.append(np.array([[0, 1, 2]], np.int32))                     # a three-point frame
    return cam, f3s, f2s, rows


def test_batch_equals_per_frame_equals_subranges(gpu):
    cam, f3s, f2s, rows = ragged_batch()
    F = len(f3s)
    full = launch(gpu, cam, f3s, f2s, rows)
    again = launch(gpu, cam, f3s, f2s, rows)
    assert full["rc"] == 0
    for k in ("depth", "tri_id", "tri_model", "covered", "status"):
        assert np.array_equal(full[k], again[k]), ("two launches bit-identical", k)
    assert full["status"].tolist() == [0, 0, ST_EMPTY, 0, 0, 0]
    assert (full["depth"][2] == 0).all() and (full["tri_id"][2] == -1).all() and full["covered"][2] == 0
    assert full["covered"][5] == (full["tri_id"][5] == 0).sum() > 1000
    for f in range(F):                                               # per-frame calls
        one = launch(gpu, cam, [f3s[f]], [f2s[f]], [rows[f]])
        assert np.array_equal(one["depth"][0], full["depth"][f]) and np.array_equal(one["tri_id"][0], full["tri_id"][f]), f
        assert one["status"][0] == full["status"][f] and one["covered"][0] == full["covered"][f]
        a, b = int(full["tri_off"][f]), int(full["tri_off"][f + 1])
        assert np.array_equal(one["tri_model"][:b - a], full["tri_model"][a:b])
    for first, n in ((1, 2), (3, 3), (0, 1), (5, 1)):                # sub-ranges: the other frames keep the sentinel
        sub = launch(gpu, cam, f3s, f2s, rows, first=first, n=n)
        assert sub["rc"] == 0
        inside = np.zeros(F, bool)
        inside[first:first + n] = True
        for k in ("depth", "tri_id", "covered", "status"):
            assert np.array_equal(sub[k][inside], full[k][inside]), (first, n, k)
            assert np.array_equal(sub[k][~inside], sentinel_like(sub[k][~inside])), (first, n, k, "untouched frames")
        a, b = int(full["tri_off"][first]), int(full["tri_off"][first + n])
        assert np.array_equal(sub["tri_model"][a:b], full["tri_model"][a:b])
        rest = np.ones(len(sub["tri_model"]), bool)
        rest[a:b] = False
        assert np.array_equal(sub["tri_model"][rest], sentinel_like(sub["tri_model"][rest]))
    no_ids = launch(gpu, cam, f3s, f2s, rows, ids=False)             # without the id image: same depths, ids untouched
    assert np.array_equal(no_ids["depth"], full["depth"]) and np.array_equal(no_ids["tri_id"], sentinel_like(no_ids["tri_id"]))
    as_tri2 = launch(gpu, cam, f3s, f2s, rows, which=2)              # the same rows as the batch's second triangulation
    assert as_tri2["rc"] == 0 and np.array_equal(as_tri2["depth"], full["depth"]) and np.array_equal(as_tri2["tri_id"], full["tri_id"])


# ---- 3. rows invariance ---------------------------------------------------------------------------------------------------

def test_rows_invariance(gpu):
    from mvoscalerecovery_amd import packing
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    for name in ("depth_full", "depth_small"):
        for i, fr in enumerate(dc.load_fixture(name)[:3]):
            rec = Reconstruct(fr["cam"], ctx=gpu)
            a = rec.depth_maps([fr["f3"]], [fr["f2"]], tris=[fr["rows"]], ids=True)
            b = rec.depth_maps([fr["f3"]], [fr["f2"]], tris=[packing.canonical_rows(fr["rows"])], ids=True)
            c = rec.depth_maps([fr["f3"]], [fr["f2"]], triangulation="gpu", ids=True)
            s = rec.depth_maps([fr["f3"]], [fr["f2"]], triangulation="scipy", ids=True)
            assert np.array_equal(s.rows[0], fr["rows"]) and np.array_equal(s.depth, a.depth)
            assert np.array_equal(c.rows[0], b.rows[0]), "the device triangulation's rows are the canonical rows of SciPy's set"
            factor = dc.bound_factor(fr["ref_err_units"])
            yy, xx, d_true, unit = dc.truth(fr["f3"], fr["rows"], a.tri_id[0], fr["cam"])
            for other in (b, c):
                assert np.array_equal(other.tri_id[0] >= 0, a.tri_id[0] >= 0), "coverage"
                ta = np.sort(a.rows[0][a.tri_id[0][yy, xx]], axis=1)
                tb = np.sort(other.rows[0][other.tri_id[0][yy, xx]], axis=1)
                differ = (ta != tb).any(1)                                    # only pixels on a shared edge may name the other triangle
                _, claims = dc.locate(fr["f2"], fr["rows"], fr["cam"].width, fr["cam"].height)
                assert not differ[claims[yy, xx] == 1].any(), "ids as triangle sets"
                gap = np.abs(other.depth[0][yy, xx] - a.depth[0][yy, xx])[~differ]
                lim = (2 * factor * unit * np.abs(d_true).astype(np.float64))[~differ]
                assert (gap <= lim).all(), (name, i, "depths within twice the bound of each other")


# ---- 4. the many-rows path ------------------------------------------------------------------------------------------------

def test_dense_frame_many_rows(gpu):
    """The 20 000-feature frame of dense.npz (its seed, the reference's recorded vote and second triangulation: 33 623 rows —
    more ids than a one-workgroup LDS table of the frame could hold) against depth_cases: coverage and ids exact, depth bound at
    its strictest (factor 1: the formula's floor)."""
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd import constants as K
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    z = np.load(os.path.join(dc.GOLDEN, "dense.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    f3, f2 = synth.synth_frame(meta["frame_idx"], meta["n"], base_seed=meta["seed"])
    assert synth.checksum(f3, f2) == meta["crc"]
    low = f2[:, 1] > K.VANISH
    valid = z["valid"].astype(bool)
    fr = {"cam": dc.camera(1241, 376), "f3": np.ascontiguousarray(f3[low][valid]), "f2": np.ascontiguousarray(f2[low][valid]),
          "rows": z["tri2"].astype(np.int32), "ref_err_units": 0.0}
    assert len(fr["rows"]) > 16384
    res = Reconstruct(fr["cam"], ctx=gpu).depth_maps([fr["f3"]], [fr["f2"]], tris=[fr["rows"]], ids=True)
    assert res.status[0] == 0
    check_image(fr, res.depth[0], res.tri_id[0], res.datas[0], res.covered[0], factor=1.0, label="dense")


# ---- 5. hostile input -----------------------------------------------------------------------------------------------------

def test_hostile_input(gpu):
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    cam, f3s, f2s, rows = ragged_batch()
    good = launch(gpu, cam, f3s, f2s, rows)
    # a vertex id out of range in frame 1: MVOSR_ST_ERR_MASK there, the neighbours as before
    bad_rows = [r.copy() for r in rows]
    bad_rows[1][7, 1] = len(f3s[1])
    bad_rows[1][9, 0] = -3
    out = launch(gpu, cam, f3s, f2s, bad_rows)
    assert out["rc"] == 0 and out["status"].tolist() == [0, ST_MASK, ST_EMPTY, 0, 0, 0]
    for f in (0, 2, 3, 4, 5):
        assert np.array_equal(out["depth"][f], good["depth"][f]) and np.array_equal(out["tri_id"][f], good["tri_id"][f])
    assert not np.isin(out["tri_id"][1], (7, 9)).any()                               # the bad rows claim nothing
    # more rows than a triangulation of the frame's points can have: refused as a whole
    too_many = [r.copy() for r in rows]
    too_many[5] = np.tile(rows[5], (7, 1))
    out = launch(gpu, cam, f3s, f2s, too_many)
    assert out["status"][5] == ST_MASK and (out["tri_id"][5] == -1).all() and np.array_equal(out["depth"][0], good["depth"][0])
    rec = Reconstruct(cam, ctx=gpu)
    with pytest.raises(ValueError):
        rec.depth_maps(f3s, f2s, tris=bad_rows)
    # a singular row (three features on a plane through the origin): status, LinAlgError from Python
    f3_sing = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    f2_sing = np.array([[10.0, 10.0], [60.0, 12.0], [30.0, 50.0], [70.0, 60.0]])
    r_sing = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    out = launch(gpu, cam, [f3_sing], [f2_sing], [r_sing])
    assert out["status"].tolist() == [ST_SINGULAR]
    with pytest.raises(np.linalg.LinAlgError):
        rec.triangle_model(f3_sing, r_sing)
    with pytest.raises(np.linalg.LinAlgError):
        rec.depth_generate(f3_sing, f2_sing, r_sing)
    # features far outside the image, NaN and infinite pixels: boxes are clipped, rows without a finite area claim nothing
    f2_far = f2s[0].copy()
    f2_far[::7] *= 1e6
    f2_far[3] = [-1e300, 1e300]
    f2_far[5] = [np.nan, 40.0]
    f2_far[11] = [np.inf, -np.inf]
    out = launch(gpu, cam, [f3s[0]], [f2_far], [rows[0]])
    want, _ = dc.locate(f2_far, rows[0], cam.width, cam.height)
    assert out["rc"] == 0 and np.array_equal(out["tri_id"][0], want)
    # width = 1, height = 1, and a one-pixel image
    for w, h in ((1, 94), (310, 1), (1, 1), (3, 2)):
        c = dc.camera(w, h, cam.fx, cam.fy, cam.cx, cam.cy)
        shift = f2s[0] - np.array([100.0, 40.0]) * (w == 1 or h == 1)
        out = launch(gpu, c, [f3s[0], f3s[1]], [shift, f2s[1]], [rows[0], rows[1]])
        for f, p in enumerate((shift, f2s[1])):
            want, _ = dc.locate(p, rows[f], w, h)
            assert np.array_equal(out["tri_id"][f], want), (w, h, f)
            assert (out["depth"][f][want < 0] == 0).all()
            assert out["covered"][f] == (want >= 0).sum()
    # bad arguments: MVOSR_ERR_ARG, nothing launched
    lib, ERR_ARG = gpu.lib, -2
    b, o = _lib.Batch(), _lib.DepthOutputs()
    cam_s = _lib.Camera(310, 94, 1.0, 1.0, 0.0, 0.0)
    dummy = gpu.zeros(64, np.float64)
    for k in ("feat_off", "feat_cnt", "x", "y", "z", "v", "tri1_off", "tri1", "tri2_off", "tri2"):
        setattr(b, k, dummy.ptr)
    b.n_frames, b.total_feat = 1, 16
    o.depth = o.status = dummy.ptr
    call = lambda which=1, u=dummy.ptr, cam_=cam_s, o_=o, first=0, n=0: lib.mvosr_dense_depth_batch(
        gpu.handle, C.byref(b), which, u, None, C.byref(cam_), C.byref(o_), first, n)
    assert call(which=0) == ERR_ARG and call(which=3) == ERR_ARG
    assert call(u=None) == ERR_ARG
    assert call(cam_=_lib.Camera(0, 94, 1.0, 1.0, 0.0, 0.0)) == ERR_ARG and call(cam_=_lib.Camera(310, -1, 1.0, 1.0, 0.0, 0.0)) == ERR_ARG
    o2 = _lib.DepthOutputs()
    o2.status = dummy.ptr
    assert call(o_=o2) == ERR_ARG                                    # null depth
    assert call(first=1, n=1) == ERR_ARG and call(first=-1, n=1) == ERR_ARG
    assert lib.mvosr_triangle_model_batch(gpu.handle, C.byref(b), 1, None, None, dummy.ptr) == ERR_ARG
    assert lib.mvosr_triangle_model_batch(gpu.handle, C.byref(b), 5, None, dummy.ptr, dummy.ptr) == ERR_ARG
    dummy.free()


# ---- 5b. wide images: every band plan, the tile beyond 40 KB, the widest image and one pixel more -----------------------------

def reference_units(fr):
    """The REFERENCE's largest depth error on a strip frame, in units: its arithmetic in float64 (depth64 over model64) against
    the longdouble truth, on the CPU.  The bound of the device's depths comes from this, never from the device."""
    cam = fr["cam"]
    tri, _ = dc.locate(fr["f2"], fr["rows"], cam.width, cam.height)
    d = dc.depth64(dc.model64(fr["f3"], fr["rows"]), tri, cam)
    yy, xx, d_true, unit = dc.truth(fr["f3"], fr["rows"], tri, cam)
    return float(dc.err_units(d[yy, xx], d_true, unit).max())


def strip_batch(w, h):
    """A wide-image batch: a float-pixel frame, an empty frame, an integer-pixel frame."""
    a, b = dc.strip_pair(w, h)
    empty = dict(cam=a["cam"], f3=np.zeros((0, 3)), f2=np.zeros((0, 2)), rows=np.zeros((0, 3), np.int32))
    return [a, empty, b]


def launch_frames(gpu, frames, **kw):
    return launch(gpu, frames[0]["cam"], [fr["f3"] for fr in frames], [fr["f2"] for fr in frames], [fr["rows"] for fr in frames], **kw)


def strip_shape_params():
    return [pytest.param(i, id="%sx%d" % ("Wmax" if i == 7 else w, h)) for i, (w, h, _) in enumerate(dc.strip_shapes(0))]


@pytest.mark.parametrize("index", strip_shape_params())
def test_wide_images(gpu, index):
    """mvosr_dense_depth_batch: ``band_rows = clamp((10240 / width) & ~1, 2, 16)`` — 14 rows (641, 682), 2 rows inside 40 KB
    (2561, 5120), and the clamp to 2 rows beyond (5121, 8193, Wmax): the first launches of depth_raster_kernel with a dynamic
    LDS request above kDpTileWords, up to ``max_lds_per_block - 64`` at Wmax.  depth_raster_kernel: ``y_hi = min(y_lo +
    band_rows, height) - 1`` with a last band of one row (682 x 15, 310 x 17) and of two of fourteen (641 x 30); the sweep's
    divmod_small(e, W) with W above 10240."""
    wmax = dc.max_width(gpu.lds_per_block)
    w, h, band = dc.strip_shapes(wmax)[index]
    assert band == dc.band_rows(w) and 4 * band * w + 64 <= gpu.lds_per_block
    frames = strip_batch(w, h)
    out = launch_frames(gpu, frames)
    assert out["rc"] == 0 and out["status"].tolist() == [0, ST_EMPTY, 0]
    assert (out["depth"][1] == 0).all() and (out["tri_id"][1] == -1).all() and out["covered"][1] == 0
    for f in (0, 2):
        fr = frames[f]
        u = reference_units(fr)
        a, b = int(out["tri_off"][f]), int(out["tri_off"][f + 1])
        got = check_image(fr, out["depth"][f], out["tri_id"][f], out["tri_model"][a:b], out["covered"][f], factor=dc.bound_factor(u),
                          label="%dx%d[%d] (%d band rows, LDS %d B)" % (w, h, f, band, 4 * band * w))
        print("%dx%d[%d]: reference %.3f units, factor %.2f, device %.3f units" % (w, h, f, u, dc.bound_factor(u), got))


def test_one_pixel_wider_than_the_lds_is_refused(gpu):
    """mvosr_dense_depth_batch: ``lds + 64 > max_lds_per_block`` — Wmax + 1 is MVOSR_ERR_TOO_LARGE and nothing is launched: every
    output keeps its sentinel.  (The frames are those of the Wmax test: nothing depends on the answer.)"""
    wmax = dc.max_width(gpu.lds_per_block)
    frames = strip_batch(wmax, 3)
    cam = dc.camera(wmax + 1, 3, *[getattr(frames[0]["cam"], k) for k in ("fx", "fy", "cx", "cy")])
    out = launch(gpu, cam, [fr["f3"] for fr in frames], [fr["f2"] for fr in frames], [fr["rows"] for fr in frames])
    assert out["rc"] == -3 and b"dense_depth" in gpu.lib.mvosr_last_error()          # MVOSR_ERR_TOO_LARGE
    for k in ("depth", "tri_id", "tri_model", "covered", "status"):
        assert np.array_equal(out[k].view(np.uint8), sentinel_like(out[k]).view(np.uint8)), k


def test_first_width_above_the_tile(gpu):
    """5121 x 5, the first width whose two-row band is more than kDpTileWords: the batch against per-frame calls and sub-ranges
    (``first_frame``, ``n_launch``), as the batch's second triangulation, and without the id image — the sweep's ``par`` path
    where a band's first pixel is not 16-byte aligned (an odd width: every other band) — all byte-identical to the batch;
    then both stages together: point_clouds against the restatement on the device's own images."""
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    w, h = 5121, 5
    frames = strip_batch(w, h)
    F = len(frames)
    full = launch_frames(gpu, frames)
    assert full["rc"] == 0 and full["status"].tolist() == [0, ST_EMPTY, 0] and (full["covered"][[0, 2]] > w * h // 2).all()
    for f in range(F):
        one = launch_frames(gpu, [frames[f]])
        assert one["rc"] == 0 and cc.same_bytes(one["depth"][0], full["depth"][f]) and cc.same_bytes(one["tri_id"][0], full["tri_id"][f]), f
        assert one["status"][0] == full["status"][f] and one["covered"][0] == full["covered"][f]
        a, b = int(full["tri_off"][f]), int(full["tri_off"][f + 1])
        assert cc.same_bytes(one["tri_model"][:b - a], full["tri_model"][a:b])
    for first, n in ((0, 1), (1, 2), (2, 1)):
        sub = launch_frames(gpu, frames, first=first, n=n)
        inside = np.zeros(F, bool)
        inside[first:first + n] = True
        assert sub["rc"] == 0
        for k in ("depth", "tri_id", "covered", "status"):
            assert cc.same_bytes(sub[k][inside], full[k][inside]), (first, n, k)
            assert np.array_equal(sub[k][~inside], sentinel_like(sub[k][~inside])), (first, n, k, "untouched frames")
    as_tri2 = launch_frames(gpu, frames, which=2)
    assert as_tri2["rc"] == 0
    for k in ("depth", "tri_id", "tri_model", "covered", "status"):
        assert cc.same_bytes(as_tri2[k], full[k]), ("which = 2", k)
    no_ids = launch_frames(gpu, frames, ids=False)
    assert no_ids["rc"] == 0 and cc.same_bytes(no_ids["depth"], full["depth"]) and cc.same_bytes(no_ids["covered"], full["covered"])
    assert np.array_equal(no_ids["tri_id"], sentinel_like(no_ids["tri_id"]))
    # the two stages together
    pair = [frames[0], frames[2]]
    cam = pair[0]["cam"]
    rec = Reconstruct(cam, ctx=gpu)
    f3s, f2s, rows = [fr["f3"] for fr in pair], [fr["f2"] for fr in pair], [fr["rows"] for fr in pair]
    dm = rec.depth_maps(f3s, f2s, tris=rows, ids=True)
    assert cc.same_bytes(dm.depth, full["depth"][[0, 2]]) and cc.same_bytes(dm.tri_id, full["tri_id"][[0, 2]])
    for stride in (1, 3):
        res = rec.point_clouds(f3s, f2s, tris=rows, stride=stride)
        pts, _, off = cc.clouds(dm.depth, dm.tri_id, cam, stride=stride)
        assert np.array_equal(res.offsets, off) and cc.same_bytes(res.points, pts) and len(pts) > 0, stride
        if stride == 1:
            assert np.array_equal(np.diff(off), dm.covered)


# ---- 6. metric depth next to the scale -------------------------------------------------------------------------------------

def test_metric_depth_batch(gpu, stages):
    from mvoscalerecovery_amd import constants as K
    from mvoscalerecovery_amd.reconstruct import Reconstruct, metric_depth_batch
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    frames = stages[:6]
    f3s, f2s = [g["f3"] for g in frames], [g["f2"] for g in frames]
    abs_ref = frames[0]["abs_ref"]
    cam = dc.camera(1241, 376)
    mk = lambda: ScaleEstimator(abs_ref, window_size=5, device=0, mutate_inputs=False, triangulation="scipy")
    est, twin = mk(), mk()
    want_scales, _ = twin.scale_calculation_batch([a.copy() for a in f3s], [b.copy() for b in f2s])
    keep3 = [a.copy() for a in f3s]
    res, scales = metric_depth_batch(est, f3s, f2s, cam)
    assert all(np.array_equal(a, b) for a, b in zip(keep3, f3s)), "the caller's arrays are not touched"
    assert np.array_equal(scales, np.asarray(want_scales))
    assert float(scales[0]) == float(frames[0]["scale_first_call"])             # the golden scale of the first frame (a window of one)
    assert list(est.scale_queue) == list(twin.scale_queue)                      # the state scale_calculation_batch alone leaves
    low = [b[:, 1] > K.VANISH for b in f2s]
    s3 = [np.ascontiguousarray(a[m][g["valid"].astype(bool)]) for a, m, g in zip(f3s, low, frames)]
    s2 = [np.ascontiguousarray(b[m][g["valid"].astype(bool)]) for b, m, g in zip(f2s, low, frames)]
    plain = Reconstruct(cam, ctx=gpu).depth_maps(s3, s2, tris=[g["tri2"] for g in frames])
    assert np.array_equal(res.depth, plain.depth * np.asarray(want_scales)[:, None, None])     # same kernel, one multiplication
    assert np.array_equal(res.covered, plain.covered) and (res.covered > 100000).all()
    given, sc2 = metric_depth_batch(est, f3s, f2s, cam, scales=np.full(6, 2.0))
    assert np.array_equal(given.depth, plain.depth * 2.0) and list(est.scale_queue) == list(twin.scale_queue)


# ---- 7. steady state allocates nothing --------------------------------------------------------------------------------------

def test_second_call_allocates_nothing(gpu):
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    cam, f3s, f2s, rows = ragged_batch()
    rec = Reconstruct(cam, ctx=gpu)
    first = rec.depth_maps(f3s, f2s, tris=rows, ids=True)
    a0 = gpu.alloc_stats()
    second = rec.depth_maps(f3s, f2s, tris=rows, ids=True)
    a1 = gpu.alloc_stats()
    assert a1["hip_malloc"] == a0["hip_malloc"] and a1["host_malloc"] == a0["host_malloc"], (a0, a1)
    assert np.array_equal(first.depth, second.depth) and np.array_equal(first.tri_id, second.tri_id)
    dev = rec.depth_maps(f3s, f2s, tris=rows, on_device=True)
    assert dev.depth is None and len(dev.chunks) == 1
    first_frame, n, d_depth, d_ids = dev.chunks[0]
    assert (first_frame, n) == (0, len(f3s)) and d_ids is None and np.array_equal(d_depth.download(), first.depth)
    d_depth.free()
    small = rec.depth_maps(f3s, f2s, tris=rows, budget_bytes=2 * cam.width * cam.height * 8)      # three chunks of two frames
    assert np.array_equal(small.depth, first.depth) and np.array_equal(small.status, first.status)
