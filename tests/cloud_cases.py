"""CPU side of the point-cloud tests (as ``depth_cases.py`` is for the depth tests): the contract of
``mvosr_point_cloud_batch`` restated in NumPy with the reference's operations (/root/reference/src/reconstruct.py:32, :35 the
rays, :108 the point, :110 the colour; every operation rounded on its own), and the crafted images of
``tests/test_gpu_cloud.py``.  Every comparison with it is bit for bit: there is no tolerance here."""
from __future__ import annotations

import numpy as np

SEGMENT = 4096          # pixels per workgroup of the cloud kernels (kClSeg)
SPAN = 1024             # consecutive pixels of one wavefront (kClSpan)
WAVE = 64
MAX_SIDE = 1 << 21      # the largest width or height the launcher takes (kClMaxSide): divmod_small's range is [0, 2^22)
HOSTILE = np.array([np.nan, np.inf, -np.inf, -3.5, -0.0, 0.0, 7.25, 1e-300, 1e300, 42.0])


def divmod_small(i, d):
    """``divmod_small`` of the device code (mvosr_device.hpp) on an int array ``i`` in [0, 2^22) and a divisor ``d`` >= 1: the
    quotient's estimate is the float32 product ``float32(i) * (float32(1) / float32(d))`` truncated, then one correction each
    way in integers.  Returns ``(q, r)``."""
    i = np.asarray(i, dtype=np.int64)
    rd = np.float32(1.0) / np.float32(d)
    q = (i.astype(np.float32) * rd).astype(np.int64)              # (both factors float32: the product is rounded to float32)
    q = q - (q * d > i)
    q = q + ((q + 1) * d <= i)
    return q, i - q * d


def cloud(depth, tri_id, cam, image=None, scale=None, depth_range=None, stride=1, dtype=np.float64):
    """One frame.  ``depth`` (H,W) float64; ``tri_id`` (H,W) int32 or None; ``image`` (H,W,3) uint8 BGR or None; ``scale`` a
    float or None; ``depth_range`` (near, far) or None.  Returns ``(points (K,3), colors (K,3) or None)`` in raster order."""
    depth = np.asarray(depth, dtype=np.float64)
    H, W = depth.shape
    assert (H, W) == (cam.height, cam.width)
    with np.errstate(all="ignore"):
        q = (np.asarray(tri_id) >= 0) if tri_id is not None else (depth != 0.0)          # covered (NaN != 0: covered)
        grid = np.zeros((H, W), dtype=bool)
        grid[::stride, ::stride] = True                                                 # row % stride == 0 and col % stride == 0
        q = q & grid
        dm = depth if scale is None else depth * np.float64(scale)                      # ONE multiplication
        if depth_range is not None:
            q = q & (dm >= depth_range[0]) & (dm <= depth_range[1])                     # NaN fails
        yy, xx = np.nonzero(q)                                                          # raster order: row outer
        d = dm[yy, xx]
        px = (xx.astype(np.float64) - cam.cx) / cam.fx                                  # :32
        py = (yy.astype(np.float64) - cam.cy) / cam.fy                                  # :35
        pts = np.stack([px * d, py * d, d], axis=1)                                     # :108
        cols = None if image is None else np.asarray(image)[yy, xx, ::-1] / 255.0       # :110
        return pts.astype(dtype), None if cols is None else cols.astype(dtype)


def clouds(depth, tri_id, cam, images=None, scales=None, depth_range=None, stride=1, dtype=np.float64):
    """A batch: ``(points, colors, offsets)`` — the frames' clouds back to back."""
    got = [cloud(depth[f], None if tri_id is None else tri_id[f], cam, None if images is None else images[f],
                 None if scales is None else scales[f], depth_range, stride, dtype) for f in range(len(depth))]
    off = np.concatenate([[0], np.cumsum([len(p) for p, _ in got])]).astype(np.int64)
    pts = np.concatenate([p for p, _ in got]) if got else np.zeros((0, 3), dtype)
    cols = None if images is None else np.concatenate([c for _, c in got])
    return pts, cols, off


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- crafted coverage ------------------------------------------------------------------------------------------------------

def coverage_masks(width, height):
    """Named boolean (H,W) coverage patterns of one image size: all, none, first / last pixel only, checkerboard, one full row,
    coverage that ends one pixel before / at / after every wavefront, span and segment boundary the image reaches (flat
    raster index), and — when the pixel count is no multiple of the segment — the tail of the last segment only."""
    n = width * height
    flat = lambda m: m.reshape(height, width)
    masks = {"all": np.ones(n, bool), "none": np.zeros(n, bool)}
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0], last[-1] = True, True
    masks["first"], masks["last"] = first, last
    yy, xx = np.divmod(np.arange(n), width)
    masks["checker"] = (yy + xx) % 2 == 0
    masks["row"] = yy == height // 2
    for name, b in (("wave", WAVE), ("span", SPAN), ("segment", SEGMENT)):
        for delta in (-1, 0, 1):
            e = min(max(b + delta, 1), n)
            m = np.zeros(n, bool)
            m[:e] = True
            masks["upto_%s%+d" % (name, delta)] = m
            m2 = np.zeros(n, bool)
            m2[min(e, n - 1):] = True
            masks["from_%s%+d" % (name, delta)] = m2
    if n % SEGMENT:
        m = np.zeros(n, bool)
        m[(n // SEGMENT) * SEGMENT:] = True
        masks["tail"] = m
    return {k: flat(v) for k, v in masks.items()}


def crafted_batch(width, height, seed=0, hostile=True):
    """One batch of crafted frames at ``width`` x ``height``: ``(names, depth (F,H,W), tri_id (F,H,W), images (F,H,W,3), scales (F,))``.
    Depths are positive random values where covered and 0 elsewhere — so that the id rule and the depth rule agree —; with
    ``hostile`` a last frame ("hostile") is fully covered and holds NaN, +-inf, negative values, -0.0 and +0.0 (there the two
    rules differ: the ids keep the zeros) in a repeating pattern."""
    rng = np.random.default_rng(seed + 1000 * width + height)
    masks = coverage_masks(width, height)
    names = list(masks)
    F = len(names) + (1 if hostile else 0)
    depth = np.zeros((F, height, width))
    tri = np.full((F, height, width), -1, dtype=np.int32)
    for f, k in enumerate(names):
        m = masks[k]
        depth[f][m] = rng.uniform(0.5, 80.0, int(m.sum()))
        tri[f][m] = rng.integers(0, 4000, int(m.sum()))
    if hostile:
        depth[-1] = HOSTILE[(np.arange(width * height) * 7 % len(HOSTILE))].reshape(height, width)
        tri[-1] = 5
        names.append("hostile")
    images = rng.integers(0, 256, (F, height, width, 3), dtype=np.uint8)
    scales = rng.uniform(0.2, 3.0, F)
    return names, depth, tri, images, scales


def large_names(cuts, teeth=False):
    """The frames of ``large_batch`` in order: all, checker, and per cut and delta in (-1, 0, +1) an ``upto`` and a ``from``;
    with ``teeth`` six more that put an edge at EVERY segment boundary + delta at once (where the boundaries are too many for a
    frame each): ``teeth`` covers the segments of even number, ``gaps`` those of odd number, each shifted by delta."""
    names = ["all", "checker"]
    for c in cuts:
        for delta in (-1, 0, 1):
            names += ["upto_%d%+d" % (c, delta), "from_%d%+d" % (c, delta)]
    if teeth:
        for delta in (-1, 0, 1):
            names += ["teeth_0%+d" % delta, "gaps_0%+d" % delta]
    return names


def large_mask(name, width, height):
    """The flat (n,) coverage of one frame of ``large_batch``: ``upto_C+D`` covers the raster indices [0, C+D), ``from_C+D``
    covers [C+D, n) (the edge clipped to [0, n]: either may be empty)."""
    n = width * height
    if name == "all":
        return np.ones(n, bool)
    if name == "checker":
        yy, xx = np.divmod(np.arange(n), width)
        return (yy + xx) % 2 == 0
    kind, edge = name.split("_")
    if kind in ("teeth", "gaps"):
        return ((np.arange(n) - int(edge[-2:])) // SEGMENT) % 2 == (0 if kind == "teeth" else 1)
    e = min(max(int(edge[:-2]) + int(edge[-2:]), 0), n)
    m = np.zeros(n, bool)
    if kind == "upto":
        m[:e] = True
    else:
        m[e:] = True
    return m


def large_batch(width, height, cuts, seed=0, frames=None, teeth=False):
    """Crafted frames for LARGE images — a handful, not the 20-odd full masks of ``coverage_masks`` —: ``(names, depth (F,H,W),
    tri_id (F,H,W), images (F,H,W,3), scales (F,))`` as ``crafted_batch`` returns them.  ``cuts``: flat raster indices (segment
    boundaries, row ends).  Depths and ids are drawn as in ``crafted_batch``; the frame "all" is fully covered and holds the
    hostile value pattern.  ``frames``: build only these of ``large_names(cuts)`` — every frame is drawn from a generator of its
    own, so a part of the batch holds the same values as the whole, and a test can keep a few frames resident at a time."""
    every = large_names(cuts, teeth)
    names = every if frames is None else list(frames)
    assert set(names) <= set(every)
    F, n = len(names), width * height
    depth = np.zeros((F, height, width))
    tri = np.full((F, height, width), -1, dtype=np.int32)
    images = np.empty((F, height, width, 3), dtype=np.uint8)
    scales = np.empty(F)
    for f, k in enumerate(names):
        rng = np.random.default_rng([seed, width, height, every.index(k)])
        m = large_mask(k, width, height).reshape(height, width)
        if k == "all":
            depth[f] = HOSTILE[(np.arange(n) * 7 % len(HOSTILE))].reshape(height, width)
            tri[f] = 5
        else:
            depth[f][m] = rng.uniform(0.5, 80.0, int(m.sum()))
            tri[f][m] = rng.integers(0, 4000, int(m.sum()))
        images[f] = rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
        scales[f] = rng.uniform(0.2, 3.0)
    return names, depth, tri, images, scales


def many_frames(width, height, n_frames, kinds, seed=0):
    """``n_frames`` small frames with random coverage (about half the pixels) — ``(depth, tri_id, images, scales)`` —, except
    the frames of ``kinds`` = {frame: "empty" | "full" | "single"}: no pixel, every pixel, one pixel (its place moves with the
    frame).  Depths are 0 exactly where a pixel is not covered, so the id rule and the depth rule agree."""
    rng = np.random.default_rng([seed, width, height, n_frames])
    m = rng.random((n_frames, height, width)) < 0.5
    for f, kind in kinds.items():
        m[f] = kind == "full"
        if kind == "single":
            m[f].reshape(-1)[(7 * f) % (width * height)] = True
    depth = np.where(m, rng.uniform(0.5, 80.0, m.shape), 0.0)
    tri = np.where(m, rng.integers(0, 4000, m.shape), -1).astype(np.int32)
    images = rng.integers(0, 256, (n_frames, height, width, 3), dtype=np.uint8)
    scales = rng.uniform(0.2, 3.0, n_frames)
    return depth, tri, images, scales


def special_kinds(n_frames, turn):
    """The frames on either side of the scan's rounds of 256 — 255, 256, 257, 511, 512, those the batch has — as empty, full
    and single-pixel frames: frame number ``k`` of the list is kind ``(k + turn) % 3``, so over ``turn`` = 0, 1, 2 every one of
    them is each kind once."""
    frames = [f for f in (255, 256, 257, 511, 512) if f < n_frames]
    return {f: ("empty", "full", "single")[(k + turn) % 3] for k, f in enumerate(frames)}


def boundaries(width, height, which=None):
    """The segment boundaries inside a ``width`` x ``height`` image (flat raster indices), or those numbered ``which``."""
    n = width * height
    return [k * SEGMENT for k in (which if which is not None else range(1, (n - 1) // SEGMENT + 1))]


# (width, height, cuts) of the large-image tests: many segments ...
MANY_SEGMENTS = {
    "4096x256": (4096, 256, [255 * SEGMENT, 256 * SEGMENT - 1]),                    # 256 segments, each one image row
    "4100x257": (4100, 257, [255 * SEGMENT, 256 * SEGMENT, 257 * SEGMENT]),         # 258 segments that straddle the row ends
    "8200x257": (8200, 257, [256 * SEGMENT, 512 * SEGMENT, 513 * SEGMENT]),         # 515 segments, a row is more than two
}
# ... and thin or wide ones: every boundary the image reaches; the widest image has 511, too many for six frames each: its
# `teeth` and `gaps` frames carry an edge at every one of them +-1, and two boundaries (after the scan's first round, the last) have their own frames
THIN_WIDE = {
    "1x5000": (1, 5000, boundaries(1, 5000)),
    "5000x1": (5000, 1, boundaries(5000, 1)),
    "4097x3": (4097, 3, boundaries(4097, 3)),
    "2097152x1": (MAX_SIDE, 1, boundaries(MAX_SIDE, 1, (256, 511))),
}
STRIDE_SIZES = [(8200, 9), (311, 95)]
STRIDES = [7, 4096, 4097, 8199, 8200, 8201, 2 ** 31 - 1]


def hand_image():
    """The 7x5 hand-made image of test_cloud_cases: ``(cam-less depth (5,7), tri_id (5,7))`` with NaN, +-inf, -0.0, a covered pixel
    of depth 0 and uncovered pixels."""
    d = np.array([[1.0, 2.0, 0.0, np.nan, 5.0, 0.0, 7.0],
                  [0.0, np.inf, 3.0, 0.0, -np.inf, 4.0, 0.0],
                  [-0.0, 6.0, 0.0, -2.0, 0.0, 8.0, 9.0],
                  [10.0, 0.0, 11.0, 0.0, 12.0, 0.0, 0.5],
                  [0.0, 13.0, 0.0, 14.0, 0.0, 15.0, 0.0]])
    tri = np.where(d != 0.0, 3, -1).astype(np.int32)
    tri[2, 0] = 1          # covered, depth -0.0
    tri[4, 6] = 2          # covered, depth +0.0
    return d, tri
