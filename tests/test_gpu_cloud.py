"""GPU: mvosr_point_cloud_batch and the point-cloud side of mvoscalerecovery_amd.reconstruct against the NumPy restatement
(tests/cloud_cases.py) applied to the DEVICE'S OWN depth and id images.  Every comparison is ``==`` on the bytes, over every
point: there is no tolerance in this file.  Nothing here provokes a fault: a capacity that is too small is answered with the
overflow word."""
import ctypes as C
import itertools

import numpy as np
import pytest

import cloud_cases as cc
import depth_cases as dc

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
SIZES = [(7, 5), (64, 4), (65, 63), (311, 95)]


def crafted_camera(w, h):
    return dc.camera(w, h, 0.58 * w, 0.61 * w, 0.49 * w, 0.52 * h)


def assert_cloud(res, want, label):
    pts, cols, off = want
    assert np.array_equal(res.offsets, off), (label, "frame_off", res.offsets.tolist(), off.tolist())
    assert cc.same_bytes(res.points, pts), (label, "points")
    if cols is None:
        assert res.colors is None, label
    else:
        assert cc.same_bytes(res.colors, cols), (label, "colours")


# ---- 1. crafted images through cloud_from_depth -----------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_crafted_images(gpu, size):
    """One batch of crafted frames per size, resident on the device once; every combination of ids, stride, range, scales,
    precision and colours."""
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    w, h = size
    cam = crafted_camera(w, h)
    names, depth, tri, images, scales = cc.crafted_batch(w, h)
    rec = Reconstruct(cam, ctx=gpu)
    d_depth, d_tri, d_img, d_sc = gpu.to_device(depth), gpu.to_device(tri), gpu.to_device(images), gpu.to_device(scales)
    try:
        assert np.array_equal(d_depth.download().view(np.uint64), depth.view(np.uint64))
        n = 0
        for ids, stride, rng, sc, dtype, col in itertools.product((True, False), (1, 3, 4), (None, (-1.0, 60.0)), (False, True),
                                                                  (np.float64, np.float32), (False, True)):
            res = rec.cloud_from_depth(d_depth, d_tri if ids else None, images=d_img if col else None, scales=d_sc if sc else None,
                                       depth_range=rng, stride=stride, dtype=dtype)
            want = cc.clouds(depth, tri if ids else None, cam, images if col else None, scales if sc else None, rng, stride, dtype)
            assert_cloud(res, want, (size, ids, stride, rng, sc, np.dtype(dtype).name, col))
            assert np.array_equal(res.covered, np.diff(want[2]))
            n += 1
        # the frames say what they should (no ids, stride 1, no range: depth != 0)
        res = rec.cloud_from_depth(d_depth)
        cnt = dict(zip(names, np.diff(res.offsets)))
        assert cnt["all"] == w * h and cnt["none"] == 0 and cnt["first"] == 1 and cnt["last"] == 1
        assert cnt["hostile"] == int((depth[-1] != 0).sum()) < w * h                  # NaN and inf kept, both zeros dropped
        with_ids = rec.cloud_from_depth(d_depth, d_tri)
        assert np.diff(with_ids.offsets)[-1] == w * h                                  # ... and kept by the id rule
        # host arrays take the same way
        host = rec.cloud_from_depth(depth, tri, images=list(images), scales=scales, depth_range=(0.0, np.inf), stride=3, dtype=np.float32)
        assert_cloud(host, cc.clouds(depth, tri, cam, images, scales, (0.0, np.inf), 3, np.float32), (size, "host arrays"))
        print("%dx%d: %d frames, %d combinations" % (w, h, len(names), n))
    finally:
        for b in (d_depth, d_tri, d_img, d_sc):
            b.free()


# ---- 2. sentinels, capacity, overflow ---------------------------------------------------------------------------------------

def raw_call(ctx, cam, depth, tri, images, scales, capacity, dtype=np.float64, stride=1, rng=None, room=64):
    """mvosr_point_cloud_batch through ctypes; points / colours / frame_off / overflow pre-filled with SENTINEL bytes, the point
    buffers ``room`` rows longer than ``capacity``."""
    call = raw_prepare(ctx, cam, depth, tri, images, scales, capacity, dtype, stride, rng, room)
    raw_launch(ctx, call)
    ctx.sync()
    return raw_collect(ctx, call)


def raw_prepare(ctx, cam, depth, tri, images, scales, capacity, dtype=np.float64, stride=1, rng=None, room=64, ins=None):
    """The buffers and argument structs of one ``raw_call``: inputs uploaded (or another call's ``ins``, shared), outputs
    pre-filled.  Uploading waits for the stream, so calls that are to be queued back to back are all prepared first."""
    from mvoscalerecovery_amd import _lib
    F = len(depth)
    own = ins is None
    if own:
        ins = [ctx.to_device(depth), ctx.to_device(tri) if tri is not None else None, ctx.to_device(images) if images is not None else None,
               ctx.to_device(scales) if scales is not None else None]
    outs = {"points": ctx.empty((capacity + room, 3), dtype), "colors": ctx.empty((capacity + room, 3), dtype),
            "frame_off": ctx.empty(F + 2, np.int64), "overflow": ctx.empty(2, np.int32)}
    for b in outs.values():
        b.fill(SENTINEL)
    i = _lib.CloudInputs(*[b.ptr if b is not None else None for b in ins], F)
    p = _lib.CloudParams(rng[0] if rng else 0.0, rng[1] if rng else 0.0, stride, (1 if rng else 0) | (2 if np.dtype(dtype) == np.float32 else 0))
    o = _lib.CloudOutputs(outs["points"].ptr, outs["colors"].ptr if ins[2] is not None else None, outs["frame_off"].ptr, outs["overflow"].ptr,
                          capacity)
    c = _lib.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    return {"ins": ins, "own": own, "outs": outs, "args": (i, c, p, o), "rc": None}


def raw_launch(ctx, call):
    """Queue a prepared call on the context's stream; nothing is waited for."""
    i, c, p, o = call["args"]
    call["rc"] = ctx.lib.mvosr_point_cloud_batch(ctx.handle, C.byref(i), C.byref(c), C.byref(p), C.byref(o))


def raw_collect(ctx, call):
    """Download a launched call's outputs (the download waits for the stream) and free its buffers."""
    got = {k: b.download() for k, b in call["outs"].items()}
    got["rc"] = call["rc"]
    for b in list(call["outs"].values()) + ([b for b in call["ins"] if b is not None] if call["own"] else []):
        b.free()
    return got


def sentinel_like(a):
    return np.frombuffer(bytes([SENTINEL]) * a.nbytes, dtype=a.dtype).reshape(a.shape)


def test_sentinels_capacity_and_overflow(gpu):
    w, h = 311, 95
    cam = crafted_camera(w, h)
    names, depth, tri, images, scales = cc.crafted_batch(w, h)
    for dtype in (np.float64, np.float32):
        pts, cols, off = cc.clouds(depth, tri, cam, images, scales, None, 1, dtype)
        K = int(off[-1])
        # exact capacity: everything, overflow 0, nothing past frame_off[F]
        got = raw_call(gpu, cam, depth, tri, images, scales, K, dtype)
        assert got["rc"] == 0 and got["overflow"][0] == 0 and np.array_equal(got["frame_off"][:-1], off)
        assert cc.same_bytes(got["points"][:K], pts) and cc.same_bytes(got["colors"][:K], cols)
        for k in ("points", "colors"):
            assert np.array_equal(got[k][K:].view(np.uint8), sentinel_like(got[k][K:]).view(np.uint8)), (k, "past frame_off[F]")
        assert got["frame_off"][-1] == sentinel_like(got["frame_off"])[-1] and got["overflow"][1] == sentinel_like(got["overflow"])[1]
        # room to spare: the rows between frame_off[F] and the capacity keep the sentinel too
        got = raw_call(gpu, cam, depth, tri, images, scales, K + 1000, dtype)
        assert got["overflow"][0] == 0 and cc.same_bytes(got["points"][:K], pts)
        assert np.array_equal(got["points"][K:].view(np.uint8), sentinel_like(got["points"][K:]).view(np.uint8))
        # too small (cut inside a frame, inside a wavefront's run): the first `capacity` rows, nothing beyond, the TRUE counts, overflow 1
        for cap in (K - 1, K // 2 + 7, 1):
            got = raw_call(gpu, cam, depth, tri, images, scales, cap, dtype)
            assert got["rc"] == 0 and got["overflow"][0] == 1 and np.array_equal(got["frame_off"][:-1], off), cap
            assert cc.same_bytes(got["points"][:cap], pts[:cap]) and cc.same_bytes(got["colors"][:cap], cols[:cap]), cap
            for k in ("points", "colors"):
                assert np.array_equal(got[k][cap:].view(np.uint8), sentinel_like(got[k][cap:]).view(np.uint8)), (k, cap, "past the capacity")
    # capacity 0: a counting call — frame_off and the overflow word only
    got = raw_call(gpu, cam, depth, tri, None, None, 0, stride=3, rng=(1.0, 50.0))
    want = cc.clouds(depth, tri, cam, None, None, (1.0, 50.0), 3)[2]
    assert got["rc"] == 0 and np.array_equal(got["frame_off"][:-1], want) and got["overflow"][0] == (1 if want[-1] else 0)
    assert np.array_equal(got["points"].view(np.uint8), sentinel_like(got["points"]).view(np.uint8))
    # Python: a capacity that is too small raises with the size needed; the right one then fits
    from mvoscalerecovery_amd.reconstruct import CloudCapacityError, Reconstruct
    rec = Reconstruct(cam, ctx=gpu)
    with pytest.raises(CloudCapacityError) as exc:
        rec.cloud_from_depth(depth, tri, capacity=10)
    assert exc.value.needed == int((tri >= 0).sum())
    res = rec.cloud_from_depth(depth, tri, capacity=exc.value.needed)
    assert_cloud(res, cc.clouds(depth, tri, cam), "retry with the needed capacity")


# ---- 3. golden frames through point_clouds ----------------------------------------------------------------------------------

def groups_by_camera(frames):
    out = {}
    for fr in frames:
        out.setdefault((fr["cam"].width, fr["cam"].height), []).append(fr)
    return out


def frame_images(frames, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (fr["cam"].height, fr["cam"].width, 3), dtype=np.uint8) for fr in frames]


def test_depth_small_batch_chunks_per_frame_and_host(gpu):
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    frames = dc.load_fixture("depth_small")
    sizes = groups_by_camera(frames)
    assert len(frames) == 6 and (311, 95) in sizes and (312, 96) in sizes
    for (w, h), group in sizes.items():
        cam = group[0]["cam"]
        rec = Reconstruct(cam, ctx=gpu)
        f3s, f2s, rows = [g["f3"] for g in group], [g["f2"] for g in group], [g["rows"] for g in group]
        imgs = frame_images(group, w)
        dm = rec.depth_maps(f3s, f2s, tris=rows, ids=True)                         # the device's own images
        want = cc.clouds(dm.depth, dm.tri_id, cam, np.stack(imgs))
        full = rec.point_clouds(f3s, f2s, tris=rows, images=imgs)
        assert_cloud(full, want, ((w, h), "one batch"))
        assert np.array_equal(full.covered, dm.covered) and np.array_equal(np.diff(full.offsets), dm.covered) and (full.status == 0).all()
        small = rec.point_clouds(f3s, f2s, tris=rows, images=imgs, budget_bytes=1)   # a frame per chunk
        assert_cloud(small, want, ((w, h), "split by the budget"))
        for f, g in enumerate(group):
            one = rec.point_clouds([g["f3"]], [g["f2"]], tris=[g["rows"]], images=[imgs[f]])
            p, c = full.frame(f)
            assert cc.same_bytes(one.points, p) and cc.same_bytes(one.colors, c), ((w, h), f, "per-frame call")
            host = rec.depth_generate(g["f3"], g["f2"], g["rows"])                 # the host route, unchanged
            assert cc.same_bytes(host.points, p), ((w, h), f, "depth_generate's points")
        plain = rec.point_clouds(f3s, f2s, tris=rows)
        assert plain.colors is None and cc.same_bytes(plain.points, full.points)


@pytest.mark.parametrize("name", ["depth_full", "depth_ties"])
def test_full_width_and_integer_pixels(gpu, name):
    """depth_full: one 1241 x 376 frame — the real, odd width (a segment begins mid-row almost everywhere); depth_ties: integer
    pixel coordinates."""
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    for (w, h), group in groups_by_camera(dc.load_fixture(name)).items():
        cam = group[0]["cam"]
        rec = Reconstruct(cam, ctx=gpu)
        f3s, f2s, rows = [g["f3"] for g in group], [g["f2"] for g in group], [g["rows"] for g in group]
        imgs = frame_images(group, h)
        dm = rec.depth_maps(f3s, f2s, tris=rows, ids=True)
        scales = np.linspace(0.7, 1.9, len(group))
        for kw in (dict(), dict(images=imgs, scales=scales, depth_range=(2.0, 40.0), stride=4, dtype=np.float32),
                   dict(stride=3, scales=scales)):
            res = rec.point_clouds(f3s, f2s, tris=rows, **kw)
            want = cc.clouds(dm.depth, dm.tri_id, cam, np.stack(imgs) if "images" in kw else None, kw.get("scales"), kw.get("depth_range"),
                             kw.get("stride", 1), kw.get("dtype", np.float64))
            assert_cloud(res, want, (name, (w, h), sorted(kw)))
            assert len(res.points) > 0
    if name == "depth_full":
        assert (w, h) == (1241, 376)


# ---- 4. keeps and the device triangulation ----------------------------------------------------------------------------------

def test_keeps_and_gpu_triangulation(gpu):
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    group = groups_by_camera(dc.load_fixture("depth_small"))[(310, 94)][:3]
    cam = group[0]["cam"]
    rec = Reconstruct(cam, ctx=gpu)
    rows = [g["rows"] for g in group]
    base = rec.point_clouds([g["f3"] for g in group], [g["f2"] for g in group], tris=rows)
    kept = rec.point_clouds([g["f3_all"] for g in group], [g["f2_all"] for g in group], tris=rows, keeps=[g["keep"] for g in group])
    assert_cloud(kept, (base.points, None, base.offsets), "keeps: the survivors' cloud")
    dm = rec.depth_maps([g["f3"] for g in group], [g["f2"] for g in group], triangulation="gpu", ids=True)
    dev = rec.point_clouds([g["f3"] for g in group], [g["f2"] for g in group], triangulation="gpu", stride=2)
    assert_cloud(dev, cc.clouds(dm.depth, dm.tri_id, cam, stride=2), "triangulation='gpu'")


# ---- 5. determinism, on_device ------------------------------------------------------------------------------------------------

def test_determinism_and_on_device(gpu):
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    group = groups_by_camera(dc.load_fixture("depth_small"))[(310, 94)]
    cam = group[0]["cam"]
    rec = Reconstruct(cam, ctx=gpu)
    f3s, f2s, rows = [g["f3"] for g in group], [g["f2"] for g in group], [g["rows"] for g in group]
    imgs = frame_images(group, 5)
    kw = dict(tris=rows, images=imgs, scales=np.linspace(0.5, 2.0, len(group)), depth_range=(1.0, 60.0))
    a = rec.point_clouds(f3s, f2s, **kw)
    b = rec.point_clouds(f3s, f2s, **kw)
    assert_cloud(b, (a.points, a.colors, a.offsets), "the same call twice")
    per = 310 * 94 * 12 + 3 * 310 * 94 + 48 * 310 * 94
    dev = rec.point_clouds(f3s, f2s, on_device=True, budget_bytes=2 * per, **kw)
    assert dev.points is None and dev.colors is None and len(dev.chunks) == -(-len(group) // 2)
    assert np.array_equal(dev.offsets, a.offsets) and np.array_equal(dev.covered, a.covered)
    at = 0
    for first, n, d_pts, d_col, off in dev.chunks:
        assert off[0] == 0 and np.array_equal(off, a.offsets[first:first + n + 1] - a.offsets[first])
        k = int(off[-1])
        assert d_pts.shape[0] >= k and cc.same_bytes(d_pts.download()[:k], a.points[at:at + k])
        assert cc.same_bytes(d_col.download()[:k], a.colors[at:at + k])
        at += k
        d_pts.free()
        d_col.free()
        assert d_pts.ptr is None
    assert at == len(a.points)


# ---- 6. metric clouds next to the scale -----------------------------------------------------------------------------------------

def test_metric_point_clouds(gpu, stages):
    from mvoscalerecovery_amd import constants as K
    from mvoscalerecovery_amd.reconstruct import Reconstruct, metric_point_clouds
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    frames = stages[:3]
    f3s, f2s = [g["f3"] for g in frames], [g["f2"] for g in frames]
    cam = dc.camera(1241, 376)
    mk = lambda: ScaleEstimator(frames[0]["abs_ref"], window_size=5, device=0, mutate_inputs=False, triangulation="scipy")
    est, twin = mk(), mk()
    want_scales, _ = twin.scale_calculation_batch([a.copy() for a in f3s], [b.copy() for b in f2s])
    imgs = [np.random.default_rng(f).integers(0, 256, (376, 1241, 3), dtype=np.uint8) for f in range(3)]
    res, scales = metric_point_clouds(est, f3s, f2s, cam, images=imgs, depth_range=(0.0, 80.0), stride=2)
    assert np.array_equal(scales, np.asarray(want_scales))
    assert list(est.scale_queue) == list(twin.scale_queue) and est.scale == twin.scale      # the state scale_calculation_batch alone leaves
    low = [b[:, 1] > K.VANISH for b in f2s]
    s3 = [np.ascontiguousarray(a[m][g["valid"].astype(bool)]) for a, m, g in zip(f3s, low, frames)]
    s2 = [np.ascontiguousarray(b[m][g["valid"].astype(bool)]) for b, m, g in zip(f2s, low, frames)]
    plain = Reconstruct(cam, ctx=gpu).depth_maps(s3, s2, tris=[g["tri2"] for g in frames], ids=True)     # the UNSCALED device images
    assert_cloud(res, cc.clouds(plain.depth, plain.tri_id, cam, np.stack(imgs), scales, (0.0, 80.0), 2), "metric_point_clouds")
    assert len(res.points) > 30000 and np.array_equal(res.covered, plain.covered)
    given, sc2 = metric_point_clouds(est, f3s, f2s, cam, scales=np.full(3, 2.0), stride=8, dtype=np.float32)
    assert_cloud(given, cc.clouds(plain.depth, plain.tri_id, cam, None, np.full(3, 2.0), None, 8, np.float32), "given scales")
    assert list(est.scale_queue) == list(twin.scale_queue)


# ---- 7. steady state allocates nothing -------------------------------------------------------------------------------------------

def test_second_call_allocates_nothing(gpu):
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    group = groups_by_camera(dc.load_fixture("depth_small"))[(310, 94)]
    cam = group[0]["cam"]
    rec = Reconstruct(cam, ctx=gpu)
    f3s, f2s, rows = [g["f3"] for g in group], [g["f2"] for g in group], [g["rows"] for g in group]
    kw = dict(tris=rows, images=frame_images(group, 9), scales=np.full(len(group), 1.5), stride=2)
    first = rec.point_clouds(f3s, f2s, **kw)
    a0 = gpu.alloc_stats()
    second = rec.point_clouds(f3s, f2s, **kw)
    a1 = gpu.alloc_stats()
    assert a1["hip_malloc"] == a0["hip_malloc"] and a1["host_malloc"] == a0["host_malloc"], (a0, a1)
    assert_cloud(second, (first.points, first.colors, first.offsets), "second call")


# ---- 8. large images, many frames, queued calls, thin and wide images, strides, the size limit ----------------------------------

F64, F32 = np.float64, np.float32
# (ids, range, scales, dtype, colours, stride): between them every option on and off; a batch of a large image takes one, in turn
OPTIONS = [(True, None, False, F64, True, 1), (False, (-1.0, 60.0), True, F32, False, 1), (True, (-1.0, 60.0), False, F32, True, 1),
           (False, None, True, F64, False, 1), (True, None, True, F64, False, 3)]
LIGHT = [o for o in OPTIONS if o[3] is F32 and not o[4]] + [(True, None, False, F32, False, 1), (False, None, False, F32, False, 3)]


def run_large(gpu, w, h, cuts, per_batch, options, teeth=False):
    """The frames of ``cc.large_batch`` through cloud_from_depth, ``per_batch`` of them resident at a time, each batch with the
    next of ``options``: frame_off, points and colours against ``cc.clouds``.  Returns the number of batches."""
    from mvoscalerecovery_amd.reconstruct import Reconstruct
    cam = crafted_camera(w, h)
    rec = Reconstruct(cam, ctx=gpu)
    names = cc.large_names(cuts, teeth)
    seen = set()
    for b, at in enumerate(range(0, len(names), per_batch)):
        part, depth, tri, images, scales = cc.large_batch(w, h, cuts, frames=names[at:at + per_batch], teeth=teeth)
        ids, rng, sc, dtype, col, stride = options[b % len(options)]
        seen.add(options[b % len(options)])
        res = rec.cloud_from_depth(depth, tri if ids else None, images=images if col else None, scales=scales if sc else None,
                                   depth_range=rng, stride=stride, dtype=dtype)
        want = cc.clouds(depth, tri if ids else None, cam, images if col else None, scales if sc else None, rng, stride, dtype)
        assert_cloud(res, want, ((w, h), part, ids, rng, sc, np.dtype(dtype).name, col, stride))
        if ids and rng is None and stride == 1:
            assert np.array_equal(np.diff(res.offsets), [cc.large_mask(k, w, h).sum() for k in part]), part
    assert len(seen) == len(options), "fewer batches than option combinations"
    return b + 1


@pytest.mark.parametrize("case", list(cc.MANY_SEGMENTS))
def test_many_segments(gpu, case):
    """cloud_scan_kernel: ``for (i0 < nseg; i0 += kClBlock)`` takes a second (4100 x 257: 258 segments) and a third (8200 x 257:
    515) trip, so ``base += all`` carries something other than 0 and cl_block_excl<int> writes its LDS slot again behind the
    second __syncthreads; 4096 x 256 is the last size without a second trip (exactly 256 segments).  cl_segment / cl_span /
    cloud_fill_kernel: a width of at least kClSeg — a segment is one row (4096), lies inside a row or crosses exactly one row
    end (4100, 8200), where ``dr`` of divmod_small(col0 + j, width) is only ever 0 or 1."""
    w, h, cuts = cc.MANY_SEGMENTS[case]
    n = run_large(gpu, w, h, cuts, 2 if w == 8200 else 3, LIGHT if w == 8200 else OPTIONS)
    print("%s: %d segments, %d frames in %d batches" % (case, -(-w * h // cc.SEGMENT), len(cc.large_names(cuts)), n))


@pytest.mark.parametrize("case", list(cc.THIN_WIDE))
def test_thin_and_wide(gpu, case):
    """cl_span / cloud_fill_kernel: width 1 (``dr`` of divmod_small runs to 4095: every pixel of a segment is a row of its own),
    height 1 (``dr`` is always 0, ``col`` runs to the width), 4097 x 3 (a segment crosses a row end, three times at another
    column), and 2^21 x 1: kClMaxSide, the top of divmod_small's range (col0 + j reaches 2^21 - 1) — the last 4096 columns are
    compared value by value as well."""
    w, h, cuts = cc.THIN_WIDE[case]
    wide = w == cc.MAX_SIDE
    n = run_large(gpu, w, h, cuts, 2 if wide else 1, LIGHT if wide else OPTIONS, teeth=wide)
    print("%s: %d segments, %d batches" % (case, -(-w * h // cc.SEGMENT), n))
    if wide:
        from mvoscalerecovery_amd.reconstruct import Reconstruct
        cam = crafted_camera(w, h)
        name = "from_%d+0" % cuts[-1]                                              # exactly the last segment: columns 2^21 - 4096 ... 2^21 - 1
        _, depth, tri, _, _ = cc.large_batch(w, h, cuts, frames=[name], teeth=True)
        res = Reconstruct(cam, ctx=gpu).cloud_from_depth(depth, tri)
        col = np.arange(w - cc.SEGMENT, w)
        d = depth[0, 0, col]
        assert res.offsets.tolist() == [0, cc.SEGMENT] and (d > 0).all()
        assert np.array_equal(res.points[:, 2], d) and np.array_equal(res.points[:, 0], (col.astype(np.float64) - cam.cx) / cam.fx * d)
        assert np.array_equal(res.points[:, 1], np.full(cc.SEGMENT, (0.0 - cam.cy) / cam.fy) * d)


def check_raw(got, want, F, K, dtype, colours, label):
    """A raw call's outputs against the restatement: all F + 1 offsets, the first ``min(K, capacity)`` rows, every tail."""
    pts, cols, off = want
    assert got["rc"] == 0, label
    assert np.array_equal(got["frame_off"][:F + 1], off), (label, "frame_off")
    assert got["frame_off"][F + 1] == sentinel_like(got["frame_off"])[F + 1] and got["overflow"][1] == sentinel_like(got["overflow"])[1], label
    assert cc.same_bytes(got["points"][:K], pts[:K]), (label, "points")
    assert np.array_equal(got["points"][K:].view(np.uint8), sentinel_like(got["points"][K:]).view(np.uint8)), (label, "points' tail")
    if colours:
        assert cc.same_bytes(got["colors"][:K], cols[:K]), (label, "colours")
    assert np.array_equal(got["colors"][K if colours else 0:].view(np.uint8), sentinel_like(got["colors"][K if colours else 0:]).view(np.uint8)), label


@pytest.mark.parametrize("turn", [0, 1, 2])
@pytest.mark.parametrize("size,F", [((7, 5), 257), ((7, 5), 513), ((65, 63), 513), ((311, 95), 513)], ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "F%d" % v)
def test_many_frames(gpu, size, F, turn):
    """cloud_scan_kernel, the last workgroup to arrive: ``for (i0 < n_frames; i0 += kClBlock)`` takes a second (F = 257) and a
    third (F = 513) trip, ``run += all`` carries something other than 0, cl_block_excl<long long> writes its slot again.  The
    frames on either side of a round — 255, 256, 257, 511, 512 — are empty, full and single-pixel in turn."""
    w, h = size
    cam = crafted_camera(w, h)
    depth, tri, images, scales = cc.many_frames(w, h, F, cc.special_kinds(F, turn), seed=turn)
    ids, rng, sc, dtype, col, _ = OPTIONS[turn]
    a = (tri if ids else None, images if col else None, scales if sc else None)
    want = cc.clouds(depth, a[0], cam, a[1], a[2], rng, 1, dtype)
    K = int(want[2][-1])
    assert K > 0 and len(want[2]) == F + 1
    got = raw_call(gpu, cam, depth, *a, K, dtype, rng=rng)
    check_raw(got, want, F, K, dtype, col, (size, F, turn))
    assert got["overflow"][0] == 0
    got = raw_call(gpu, cam, depth, *a, K - 1, dtype, rng=rng)                     # one row short: the true counts, overflow 1
    check_raw(got, want, F, K - 1, dtype, col, (size, F, turn, "one row short"))
    assert got["overflow"][0] == 1
    print("%dx%d F=%d turn %d: %d points" % (w, h, F, turn, K))


def test_back_to_back(gpu):
    """cloud_count_kernel / cloud_scan_kernel: ``*a.arrive`` — the arrival counter lives in the context's workspace at an offset
    that depends on the call's frame and segment counts; three calls of two sizes queued with nothing waited for in between
    share the workspace, and each must find its counter at 0 and its segment counts its own."""
    F = 513
    big, small = crafted_camera(311, 95), crafted_camera(65, 63)
    depth, tri, images, scales = cc.many_frames(311, 95, F, cc.special_kinds(F, 1), seed=5)
    d3, t3, i3, s3 = cc.many_frames(65, 63, 3, {1: "empty"}, seed=6)
    want = cc.clouds(depth, tri, big, None, scales, None, 1, np.float32)
    want3 = cc.clouds(d3, t3, small, i3, None, (1.0, 50.0), 3, np.float64)
    K, K3 = int(want[2][-1]), int(want3[2][-1])
    first = raw_prepare(gpu, big, depth, tri, None, scales, K, np.float32)
    middle = raw_prepare(gpu, small, d3, t3, i3, None, K3, np.float64, stride=3, rng=(1.0, 50.0))
    third = raw_prepare(gpu, big, depth, tri, None, scales, K, np.float32, ins=first["ins"])
    gpu.sync()
    for call in (first, middle, third):                                            # queued: no sync, no copy in between
        raw_launch(gpu, call)
    got3, got2, got1 = raw_collect(gpu, third), raw_collect(gpu, middle), raw_collect(gpu, first)
    check_raw(got1, want, F, K, np.float32, False, "first")
    check_raw(got3, want, F, K, np.float32, False, "third")
    check_raw(got2, want3, 3, K3, np.float64, True, "middle")
    assert got1["overflow"][0] == got2["overflow"][0] == got3["overflow"][0] == 0
    for k in ("points", "colors", "frame_off", "overflow"):
        assert cc.same_bytes(got1[k], got3[k]), (k, "first and third call")


@pytest.mark.parametrize("size", cc.STRIDE_SIZES, ids=lambda s: "%dx%d" % s)
def test_large_strides(gpu, size):
    """cl_span: divmod_small(row, stride) and divmod_small(col, stride) with a stride larger than a side (the quotient is
    always 0), next to the segment size (4096, 4097), next to the width (8199, 8200, 8201) and one that float cannot
    represent (2^31 - 1: ``rS`` is 2^-31).  From max(width, height) upward only pixel (0, 0) is on the grid."""
    from mvoscalerecovery_amd.reconstruct import Reconstruct, grid_points
    w, h = size
    cam = crafted_camera(w, h)
    names, depth, tri, images, scales = cc.large_batch(w, h, [cc.SEGMENT])
    rec = Reconstruct(cam, ctx=gpu)
    bufs = [gpu.to_device(a) for a in (depth, tri, images, scales)]
    d_depth, d_tri, d_img, d_sc = bufs
    try:
        for k, stride in enumerate(cc.STRIDES):
            for ids, rng, sc, dtype, col, _ in (OPTIONS[k % 2], OPTIONS[2 + k % 2]):
                res = rec.cloud_from_depth(d_depth, d_tri if ids else None, images=d_img if col else None, scales=d_sc if sc else None,
                                           depth_range=rng, stride=stride, dtype=dtype)
                want = cc.clouds(depth, tri if ids else None, cam, images if col else None, scales if sc else None, rng, stride, dtype)
                assert_cloud(res, want, (size, stride, ids, rng, sc, np.dtype(dtype).name, col))
                cnt = np.diff(res.offsets)
                if stride >= max(w, h):
                    assert set(cnt.tolist()) <= {0, 1}, (size, stride, cnt.tolist())
            full = np.diff(rec.cloud_from_depth(d_depth, d_tri, stride=stride).offsets)     # ids, no range: the grid pixels a frame covers
            assert full[0] == grid_points(w, h, stride)
            if stride >= max(w, h):
                assert np.array_equal(full, (tri[:, 0, 0] >= 0).astype(np.int64)) and 0 < full.sum() < len(names), (size, stride)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("size", [(cc.MAX_SIDE + 1, 1), (1, cc.MAX_SIDE + 1)], ids=lambda s: "%dx%d" % s)
def test_side_beyond_the_limit_is_refused(gpu, size):
    """mvosr_point_cloud_batch: ``cam->width > kClMaxSide || cam->height > kClMaxSide`` — one pixel beyond divmod_small's range
    is MVOSR_ERR_TOO_LARGE and nothing is launched: every output keeps its sentinel.  (The inputs are allocated at their
    full size.)"""
    w, h = size
    cam = crafted_camera(w, h)
    depth, tri = np.ones((1, h, w)), np.zeros((1, h, w), np.int32)
    got = raw_call(gpu, cam, depth, tri, None, None, 64)
    assert got["rc"] == -3                                                         # MVOSR_ERR_TOO_LARGE
    assert b"point_cloud" in gpu.lib.mvosr_last_error()
    for k in ("points", "colors", "frame_off", "overflow"):
        assert np.array_equal(got[k].view(np.uint8), sentinel_like(got[k]).view(np.uint8)), k
