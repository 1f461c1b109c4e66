"""CPU: the dense-depth entry points in the binding, the header and the library; the new structs' layouts against a C
compile; ``reconstruct``'s argument validation and chunk planning on plain arrays (no GPU)."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvosr_triangle_model_batch", "mvosr_dense_depth_batch")


def test_symbols_header_and_abi():
    from mvoscalerecovery_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvosr.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert _lib.ABI_VERSION == 13 and "#define MVOSR_ABI_VERSION 13" in header
    lib = _lib.load()                                   # every symbol resolved, ABI of the library == the binding's
    assert lib.mvosr_abi_version() == 13
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, exported), name


def test_depth_structs_match_the_header(tmp_path):
    from mvoscalerecovery_amd import _lib
    structs = {"mvosr_camera": _lib.Camera, "mvosr_depth_outputs": _lib.DepthOutputs}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvosr.h"', 'int main(void) {']
    for st, cls in structs.items():
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for n, _ in cls._fields_:
            src.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, n, st, n))
    src.append('return 0; }')
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in structs.items():
        assert int(got[st]) == C.sizeof(cls), st
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)
    assert C.sizeof(_lib.Camera) == 40 and C.sizeof(_lib.DepthOutputs) == 40


def test_bad_arguments_are_refused_before_any_gpu_work():
    """Null context / batch, which_tri outside 1..2: MVOSR_ERR_ARG (-2) and a message, without a device."""
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    b, cam, o = _lib.Batch(), _lib.Camera(4, 4, 1.0, 1.0, 0.0, 0.0), _lib.DepthOutputs()
    assert lib.mvosr_dense_depth_batch(None, C.byref(b), 1, None, None, C.byref(cam), C.byref(o), 0, 0) == -2
    assert b"dense_depth" in lib.mvosr_last_error()
    assert lib.mvosr_triangle_model_batch(None, C.byref(b), 2, None, None, None) == -2
    assert b"triangle_model" in lib.mvosr_last_error()


def test_strip_frames_are_fit_for_the_wide_image_tests():
    """The inputs of test_gpu_depth's wide-image tests, by the restatement alone: every frame covers at least half its image,
    a triangle crosses every boundary between two bands (band height by the launcher's formula, restated here), no row is
    singular, and the reference-order float64 depths are finite."""
    import depth_cases as dc
    wmax = dc.max_width(dc.LDS_160K)
    assert wmax == 20472
    for w, h, band in dc.strip_shapes(wmax):
        rows_per_band = (10240 // w) & ~1                                          # mvosr_dense_depth_batch's band plan
        rows_per_band = 2 if rows_per_band < 2 else (16 if rows_per_band > 16 else rows_per_band)
        assert rows_per_band == band == dc.band_rows(w), (w, h)
        assert (4 * band * w <= 40960) == (w <= 5120)                              # the tile leaves 40 KB only by the clamp to two rows
        assert 4 * band * w + 64 <= dc.LDS_160K
        for fr in dc.strip_pair(w, h):
            f2, rows, cam = fr["f2"], fr["rows"], fr["cam"]
            assert (cam.width, cam.height) == (w, h) and len(rows) > 0 and len(rows) < 2 * len(f2)
            tri, claims = dc.locate(f2, rows, w, h)
            assert (tri >= 0).sum() >= 0.5 * w * h, (w, h, "coverage", float((tri >= 0).mean()))
            v = f2[rows][:, :, 1]
            y0, y1 = np.maximum(np.ceil(v.min(1)), 0), np.minimum(np.floor(v.max(1)), h - 1)
            for b in range(band, h, band):                                         # image rows b - 1 and b lie in two bands
                assert ((y0 <= b - 1) & (y1 >= b)).any(), (w, h, "no triangle crosses the band boundary at row", b)
            datas = dc.model64(fr["f3"], rows)                                     # (np.linalg.inv raises on a singular row)
            assert np.isfinite(datas).all(), (w, h)
            d = dc.depth64(datas, tri, cam)
            assert np.isfinite(d).all() and (d[tri >= 0] != 0).all(), (w, h)
        a, b = dc.strip_pair(w, h)
        assert (b["f2"] == np.round(b["f2"])).all() and len(np.unique(b["f2"], axis=0)) == len(b["f2"])
        assert not (a["f2"] == np.round(a["f2"])).all()
    assert [h % band for _, h, band in dc.strip_shapes(wmax)[:3]] == [2, 1, 1]     # the last band: 2 rows, 1 row, 1 row
    assert 4 * dc.band_rows(wmax + 1) * (wmax + 1) + 64 > dc.LDS_160K              # one pixel wider is refused


def test_plan_chunks():
    from mvoscalerecovery_amd import reconstruct as rc
    per = 1241 * 376 * 8
    assert rc.plan_chunks(0, 1241, 376) == []
    assert rc.plan_chunks(5, 1241, 376, budget_bytes=per * 2) == [(0, 2), (2, 2), (4, 1)]
    assert rc.plan_chunks(5, 1241, 376, ids=True, budget_bytes=per * 2) == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1)]      # 12 B per pixel
    assert rc.plan_chunks(3, 1241, 376, budget_bytes=1) == [(0, 1), (1, 1), (2, 1)]                                  # at least a frame
    chunks = rc.plan_chunks(1000, 1241, 376)                                                                           # the default: 2 GiB
    assert chunks[0] == (0, (2 << 30) // per) and sum(n for _, n in chunks) == 1000
    assert all(a + n == b for (a, n), (b, _) in zip(chunks, chunks[1:]))
    with pytest.raises(ValueError):
        rc.plan_chunks(3, 10, 10, budget_bytes=0)


def test_argument_validation():
    from mvoscalerecovery_amd import reconstruct as rc
    cam = SimpleNamespace(width=8, height=6, fx=2.0, fy=2.0, cx=4.0, cy=3.0)
    assert rc.check_camera(cam) == (8, 6, 2.0, 2.0, 4.0, 3.0)
    for bad in (SimpleNamespace(width=0, height=6, fx=1, fy=1, cx=0, cy=0), SimpleNamespace(width=8, height=2.5, fx=1, fy=1, cx=0, cy=0)):
        with pytest.raises(ValueError):
            rc.check_camera(bad)
    with pytest.raises(TypeError):
        rc.check_camera(SimpleNamespace(width=8, height=6))
    f3, f2 = np.zeros((5, 3)), np.zeros((5, 2))
    a, b, t, k = rc.check_frames([f3], [f2], [np.array([[0, 1, 2]], dtype=np.int64)], [np.ones(5, bool)])
    assert t[0].dtype == np.int32 and k[0].dtype == np.bool_ and a[0].shape == (5, 3)
    for args in (([f3], [f2, f2]), ([f3], [np.zeros((4, 2))]), ([np.zeros((5, 2))], [f2]), ([f3], [f2], [np.zeros((1, 3))]),
                 ([f3], [f2], [np.zeros((2, 2), int)]), ([f3], [f2], None, [np.ones(4, bool)]), ([f3], [f2], None, [np.ones(5, int)]),
                 ([f3], [f2], [], None)):
        with pytest.raises(ValueError):
            rc.check_frames(*args)
    # the packer keeps EVERY feature (rows index the caller's arrays), NaN and -inf pixel rows included
    g3, g2 = np.arange(15.0).reshape(5, 3), np.array([[1.0, 2.0], [3.0, np.nan], [5.0, -np.inf], [7.0, 8.0], [9.0, 1.0]])
    pf = rc.pack_all([g3, np.zeros((0, 3)), g3[:3]], [g2, np.zeros((0, 2)), g2[:3]])
    assert pf.feat_cnt.tolist() == [5, 0, 3] and pf.max_feat == 5 and (pf.feat_off % 2 == 0).all() and pf.total_padded >= 8
    assert np.array_equal(pf.u[pf.frame_slice(0)], g2[:, 0]) and np.array_equal(pf.v[pf.frame_slice(0)], g2[:, 1], equal_nan=True)
    assert np.array_equal(pf.z[pf.frame_slice(2)], g3[:3, 2]) and np.array_equal(pf.x[pf.frame_slice(0)], g3[:, 0])
    r = rc.Reconstruct(cam)                      # (no device is touched until something is launched)
    with pytest.raises(ValueError):
        r.depth_maps([f3], [f2], triangulation="qhull")
    with pytest.raises(np.linalg.LinAlgError):
        rc.raise_for_depth_status(rc.ST_ERR_SINGULAR, 3)
    with pytest.raises(ValueError):
        rc.raise_for_depth_status(rc.ST_ERR_MASK)
    rc.raise_for_depth_status(0)
    rc.raise_for_depth_status(rc.ST_ERR_EMPTY)
