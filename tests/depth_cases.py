"""CPU side of the dense-depth tests (as ``flat_cases.py`` is for the flat-selection tests): the point-location rule of
``mvosr_dense_depth_batch`` restated in NumPy, the triangle planes and depths in float64 with the reference's operation
order (/root/reference/src/reconstruct.py:70-90, :104) and in ``np.longdouble`` (Cramer's rule on the longdouble copies
of the inputs: "truth"), the condition-scaled error unit, and the exact closed-container check for tie pixels.

The only tolerance of the depth tests:

    |d - truth| <= max(1, 4 * ref_err_units) * unit * |truth|,      unit = 2**-52 * cond2(A_t) * kappa_p
    kappa_p = (|nx px| + |ny py| + |nz|) / |nx px + ny py + nz|     (the cancellation in the denominator)

``ref_err_units`` is the reference's own largest error in those units over a fixture, stored in the fixture."""
from __future__ import annotations

import os
import zlib
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
FX, CX, CY = 718.856, 607.1928, 185.2157          # the KITTI camera the synthetic frames are drawn for (synth.py)


def camera(width, height, fx=FX, fy=FX, cx=CX, cy=CY):
    return SimpleNamespace(width=int(width), height=int(height), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy))


def scaled_camera(width, height):
    """The 1241-wide camera scaled to ``width`` (intrinsics and pixels by width / 1241), ``height`` rows."""
    s = width / 1241.0
    return camera(width, height, FX * s, FX * s, CX * s, CY * s), s


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c & 0xFFFFFFFF


def synth_features(n, seed, scale=1.0, integer_pixels=False, cam=None):
    """The features a fixture frame starts from (regenerated, never stored): ``synth.synth_frame`` below the camera
    (y > 0, reconstruct.py:171), pixels scaled; ``integer_pixels``: pixels rounded, duplicates dropped, x and y recomputed
    from the rounded pixels — every edge function is then exact and pixels ON edges abound."""
    from mvoscalerecovery_amd import synth
    f3, f2 = synth.synth_frame(0, n, base_seed=seed, upper_fraction=0.1)
    f2 = f2 * scale
    if integer_pixels:
        f2 = np.round(f2)
        _, ui = np.unique(f2, axis=0, return_index=True)
        ui.sort()
        f2, f3 = f2[ui], f3[ui].copy()
        f3[:, 0] = (f2[:, 0] - cam.cx) * f3[:, 2] / cam.fx
        f3[:, 1] = (f2[:, 1] - cam.cy) * f3[:, 2] / cam.fy
    low = f3[:, 1] > 0
    return np.ascontiguousarray(f3[low]), np.ascontiguousarray(f2[low])


def strip_frame(width, height, n, seed, integer_pixels=False):
    """A frame for an image of ANY shape — a scaled KITTI frame would leave a strip of 5 000 x 5 pixels nearly empty —: ``n``
    pixels drawn uniformly over [0, width) x [0, height), depths z in [4, 60], x = (u - cx) z / fx and y = (v - cy) z / fy with
    the 1241-wide camera scaled to ``width``, rows from SciPy's Delaunay triangulation of the pixels.  ``integer_pixels``: the
    pixels rounded, duplicates dropped (x and y from the rounded pixels) — pixels ON edges abound, as in depth_ties.
    Returns the dict of a fixture frame without the recorded parts: cam, f3, f2, rows."""
    from scipy.spatial import Delaunay
    cam, _ = scaled_camera(width, height)
    rng = np.random.default_rng([seed, width, height, n])
    f2 = np.stack([rng.uniform(0.0, width, n), rng.uniform(0.0, height, n)], axis=1)
    z = rng.uniform(4.0, 60.0, n)
    if integer_pixels:
        f2 = np.round(f2)
        _, ui = np.unique(f2, axis=0, return_index=True)
        ui.sort()
        f2, z = f2[ui], z[ui]
    f3 = np.stack([(f2[:, 0] - cam.cx) * z / cam.fx, (f2[:, 1] - cam.cy) * z / cam.fy, z], axis=1)
    rows = Delaunay(f2).simplices.astype(np.int32)
    return dict(cam=cam, f3=np.ascontiguousarray(f3), f2=np.ascontiguousarray(f2), rows=np.ascontiguousarray(rows))


def band_rows(width):
    """The band plan of mvosr_dense_depth_batch, restated: an even number of image rows whose ids fit 10240 words (40 KB) of
    LDS, at most 16, at least 2 however wide the image — the request then grows with the width."""
    return min(max((10240 // width) & ~1, 2), 16)


LDS_160K = 160 * 1024                      # the LDS a workgroup can ask for on the MI355X (mvosr_ctx_device_info)


def max_width(lds_per_block):
    """The widest image the rasteriser takes: two rows of ids plus 64 B within the device's LDS per workgroup."""
    return (lds_per_block - 64) // 8


def strip_shapes(wmax):
    """(width, height, band rows) of the wide-image tests: every value the band plan takes, heights that end in a band of one
    or two rows, the tile at exactly 40 KB, the first request above it, and the widest image the device takes."""
    return [(641, 30, 14), (682, 15, 14), (310, 17, 16), (2561, 5, 2), (5120, 5, 2), (5121, 5, 2), (8193, 4, 2), (wmax, 3, 2)]


def strip_pair(width, height):
    """The two frames of a wide-image test — float pixels, integer pixels —: about one feature per 40 pixels (at least 120,
    so that the small shapes are covered too), seeds fixed."""
    n = max(120, width * height // 40)
    return strip_frame(width, height, n, 1), strip_frame(width, height, n, 2, integer_pixels=True)


# ---- point location ------------------------------------------------------------------------------------------------------

def _sorted_vertices(f2, rows):
    r = np.sort(np.asarray(rows, dtype=np.int64).reshape(-1, 3), axis=1)
    return f2[r[:, 0]], f2[r[:, 1]], f2[r[:, 2]]


def locate(f2, rows, width, height):
    """The rule: a pixel belongs to a row when its three edge functions times the row's orientation sign are >= 0, every edge
    evaluated from its lower to its higher vertex id (negated for the triangle that sees it the other way); the lowest
    claiming row wins.  Returns ``(tri (H,W) int32, -1 = none; claims (H,W) int32)``."""
    f2 = np.asarray(f2, dtype=np.float64)
    A, B, Cc = _sorted_vertices(f2, rows)
    none = np.iinfo(np.int32).max
    tri = np.full((height, width), none, dtype=np.int32)
    claims = np.zeros((height, width), dtype=np.int32)
    with np.errstate(all="ignore"):
        area = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (B[:, 1] - A[:, 1]) * (Cc[:, 0] - A[:, 0])
        us, vs = np.stack([A[:, 0], B[:, 0], Cc[:, 0]], 1), np.stack([A[:, 1], B[:, 1], Cc[:, 1]], 1)
        bx0, bx1 = np.maximum(np.ceil(us.min(1)), 0.0), np.minimum(np.floor(us.max(1)), width - 1.0)
        by0, by1 = np.maximum(np.ceil(vs.min(1)), 0.0), np.minimum(np.floor(vs.max(1)), height - 1.0)
    live = ((area > 0) | (area < 0)) & (bx0 <= bx1) & (by0 <= by1)
    for k in np.nonzero(live)[0]:
        x0, x1, y0, y1 = int(bx0[k]), int(bx1[k]), int(by0[k]), int(by1[k])
        px, py = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.float64), np.arange(y0, y1 + 1, dtype=np.float64))
        a, b, c = A[k], B[k], Cc[k]
        s = 1.0 if area[k] > 0 else -1.0
        e01 = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
        e12 = (c[0] - b[0]) * (py - b[1]) - (c[1] - b[1]) * (px - b[0])
        e02 = (c[0] - a[0]) * (py - a[1]) - (c[1] - a[1]) * (px - a[0])
        ins = (s * e01 >= 0) & (s * e12 >= 0) & (s * e02 <= 0)
        yy, xx = np.nonzero(ins)
        yy += y0
        xx += x0
        claims[yy, xx] += 1
        tri[yy, xx] = np.minimum(tri[yy, xx], k)
    tri[tri == none] = -1
    return tri, claims


def contains_exact(f2, row, px, py):
    """Is pixel (px, py) in the CLOSED triangle ``row``?  Exact rational arithmetic on the float64 inputs."""
    P = [(Fraction(float(f2[i, 0])), Fraction(float(f2[i, 1]))) for i in row]
    x, y = Fraction(int(px)), Fraction(int(py))

    def e(a, b):
        return (b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0])
    area = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[1][1] - P[0][1]) * (P[2][0] - P[0][0])
    s = 1 if area > 0 else -1
    return area != 0 and s * e(P[0], P[1]) >= 0 and s * e(P[1], P[2]) >= 0 and s * e(P[2], P[0]) >= 0


def all_contained(f2, rows, tri, mask):
    """Every pixel of ``mask`` lies in the closed triangle ``tri`` names for it (exactly)."""
    rows = np.asarray(rows)
    return all(tri[y, x] >= 0 and contains_exact(f2, rows[tri[y, x]], x, y) for y, x in np.argwhere(mask))


# ---- planes and depths ---------------------------------------------------------------------------------------------------

def model64(f3, rows):
    """``Reconstruct.triangle_model`` in float64, vectorised: explicit inverse, n = A^-1 . 1, height = 1/|n|, the sign rule."""
    A = np.asarray(f3, dtype=np.float64)[np.asarray(rows, dtype=np.int64).reshape(-1, 3)]
    n = (np.linalg.inv(A) @ np.ones((3, 1)))[:, :, 0]
    s = np.sqrt((n * n).sum(1))
    h = 1.0 / s
    n = n / s[:, None]
    flip = n[:, 1] < 0
    n[flip] = -n[flip]
    h[flip] = -h[flip]
    return np.concatenate([n, h[:, None]], axis=1)


def normals_true(f3, rows):
    """n = A^-1 . 1 by Cramer's rule in longdouble (unnormalised)."""
    A = np.asarray(f3, dtype=np.float64)[np.asarray(rows, dtype=np.int64).reshape(-1, 3)].astype(np.longdouble)
    a, b, c = A[:, 0], A[:, 1], A[:, 2]

    def cr(p, q):
        return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)
    det = (a * cr(b, c)).sum(1)
    return (cr(b, c) + cr(c, a) + cr(a, b)) / det[:, None]


def model_true(f3, rows):
    n = normals_true(f3, rows)
    s = np.sqrt((n * n).sum(1))
    h = 1 / s
    n = n / s[:, None]
    flip = n[:, 1] < 0
    n[flip] = -n[flip]
    h[flip] = -h[flip]
    return np.concatenate([n, h[:, None]], axis=1)


def cond2(f3, rows):
    return np.linalg.cond(np.asarray(f3, dtype=np.float64)[np.asarray(rows, dtype=np.int64).reshape(-1, 3)])


def depth64(datas, tri, cam):
    """``depth_generate``'s arithmetic (:31-36, :104) in float64 on a located image; 0 where ``tri`` is -1."""
    H, W = tri.shape
    yy, xx = np.nonzero(tri >= 0)
    k = tri[yy, xx]
    px = (xx.astype(np.float64) - cam.cx) / cam.fx
    py = (yy.astype(np.float64) - cam.cy) / cam.fy
    d = np.zeros((H, W))
    with np.errstate(all="ignore"):
        d[yy, xx] = datas[k, 3] / ((datas[k, 0] * px + datas[k, 1] * py) + datas[k, 2])
    return d


def truth(f3, rows, tri, cam):
    """Per covered pixel of ``tri`` (raster order): the exact depth 1 / (n . p) in longdouble and the error unit
    ``2**-52 * cond2(A_t) * kappa_p`` (float64).  Returns ``(yy, xx, d_true, unit)``."""
    yy, xx = np.nonzero(tri >= 0)
    k = tri[yy, xx]
    L = np.longdouble
    n = normals_true(f3, rows)
    px = (xx.astype(L) - L(cam.cx)) / L(cam.fx)
    py = (yy.astype(L) - L(cam.cy)) / L(cam.fy)
    t0, t1, t2 = n[k, 0] * px, n[k, 1] * py, n[k, 2]
    den = t0 + t1 + t2
    kappa = ((np.abs(t0) + np.abs(t1) + np.abs(t2)) / np.abs(den)).astype(np.float64)
    return yy, xx, 1 / den, EPS * cond2(f3, rows)[k] * kappa


def err_units(d, d_true, unit):
    """|d - truth| / (|truth| * unit) per pixel (float64)."""
    return (np.abs(d.astype(np.longdouble) - d_true) / (np.abs(d_true) * unit)).astype(np.float64)


def bound_factor(ref_err_units):
    return max(1.0, 4.0 * float(ref_err_units))


def model_errors(datas, f3, rows):
    """Per row: (relative error of height, largest absolute error of the unit normal) in units of 2**-52 * cond2(A); a row
    whose |ny| is below its own bound may carry the opposite overall sign (the sign rule flips on rounding there)."""
    t = model_true(f3, rows)
    u = EPS * cond2(f3, rows)
    d = np.asarray(datas, dtype=np.longdouble)
    eh = np.abs(d[:, 3] - t[:, 3]) / np.abs(t[:, 3])
    en = np.abs(d[:, :3] - t[:, :3]).max(1)
    eh2 = np.abs(-d[:, 3] - t[:, 3]) / np.abs(t[:, 3])
    en2 = np.abs(-d[:, :3] - t[:, :3]).max(1)
    return (eh / u).astype(np.float64), (en / u).astype(np.float64), (eh2 / u).astype(np.float64), (en2 / u).astype(np.float64), \
        (np.abs(t[:, 1]) / u).astype(np.float64)


def model_within(datas, f3, rows, factor):
    eh, en, eh2, en2, ny_units = model_errors(datas, f3, rows)
    ok = (eh <= factor) & (en <= factor)
    ok |= (ny_units <= factor) & (eh2 <= factor) & (en2 <= factor)
    return ok


# ---- fixtures ------------------------------------------------------------------------------------------------------------

def load_fixture(name):
    """``tests/golden/<name>.npz`` as a list of per-frame dicts with the inputs regenerated (and their CRC checked)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    frames = []
    for i in range(int(z["n_frames"])):
        g = lambda k: z["f%d_%s" % (i, k)]
        w, h, n, seed, integer = (int(v) for v in g("spec"))
        cam, s = scaled_camera(w, h)
        f3, f2 = synth_features(n, seed, s, bool(integer), cam)
        assert crc(f3, f2) == int(g("crc")), "fixture %s frame %d: regenerated inputs differ from the recorded ones" % (name, i)
        keep = np.unpackbits(g("keep"))[:len(f3)].astype(bool)
        fr = dict(cam=cam, f3_all=f3, f2_all=f2, keep=keep, f3=np.ascontiguousarray(f3[keep]), f2=np.ascontiguousarray(f2[keep]),
                  rows=g("rows").astype(np.int32), datas=g("datas"), tri=g("tri").astype(np.int32), stride=int(g("stride")),
                  depths=g("depths"), ref_err_units=float(g("ref_err_units")))
        frames.append(fr)
    return frames


def stored_depths(fr):
    """(yy, xx, d_ref) of the pixels whose reference depth the fixture stores: every ``stride``-th covered pixel in raster order."""
    yy, xx = np.nonzero(fr["tri"] >= 0)
    return yy[::fr["stride"]], xx[::fr["stride"]], fr["depths"]
