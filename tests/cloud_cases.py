"""CPU side of the point-cloud tests (as ``depth_cases.py`` is for the depth tests): the contract of
``mvosr_point_cloud_batch`` restated in NumPy with the reference's operations (/root/reference/src/reconstruct.py:32, :35 the
rays, :108 the point, :110 the colour; every operation rounded on its own), and the crafted images of
``tests/test_gpu_cloud.py``.  Every comparison with it is bit for bit: there is no tolerance here."""
from __future__ import annotations

import numpy as np

SEGMENT = 4096          # pixels per workgroup of the cloud kernels (kClSeg)
SPAN = 1024             # consecutive pixels of one wavefront (kClSpan)
WAVE = 64


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
        vals = np.array([np.nan, np.inf, -np.inf, -3.5, -0.0, 0.0, 7.25, 1e-300, 1e300, 42.0])
        depth[-1] = vals[(np.arange(width * height) * 7 % len(vals))].reshape(height, width)
        tri[-1] = 5
        names.append("hostile")
    images = rng.integers(0, 256, (F, height, width, 3), dtype=np.uint8)
    scales = rng.uniform(0.2, 3.0, F)
    return names, depth, tri, images, scales


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
