"""CPU: mvosr_region_grow_batch in the binding, the header and the library; the two new structs' layouts against a C compile;
``GraphGrow`` and ``ScaleEstimator(region=...)`` validate their arguments without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "mvosr_region_grow_batch"


def test_symbol_header_and_abi():
    from mvoscalerecovery_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvosr.h")).read()
    assert NEW in _lib.SYMBOLS and re.search(r"\bint %s\(" % NEW, header)
    assert _lib.ABI_VERSION == 13 and "#define MVOSR_ABI_VERSION 13" in header          # an additive change
    lib = _lib.load()
    assert lib.mvosr_abi_version() == 13
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s\b" % NEW, exported)


def test_grow_structs_match_the_header(tmp_path):
    from mvoscalerecovery_amd import _lib
    structs = {"mvosr_grow_params": _lib.GrowParams, "mvosr_grow_outputs": _lib.GrowOutputs}
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
    assert C.sizeof(_lib.GrowParams) == 32 and C.sizeof(_lib.GrowOutputs) == 80


def test_null_arguments_are_refused_before_any_gpu_work():
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    b, gp, o = _lib.Batch(), _lib.GrowParams(8.0, -85.0, -80.0, 0.4), _lib.GrowOutputs()
    assert lib.mvosr_region_grow_batch(None, C.byref(b), None, None, C.byref(gp), C.byref(o), 0) == -2
    assert b"region_grow" in lib.mvosr_last_error()


def test_graph_grow_validates_without_a_device():
    from mvoscalerecovery_amd.graph import GraphGrow
    g = GraphGrow()                                                   # (no device is touched until something is launched)
    assert g.threshold_angle == 8.0 and g.threshold_height == 0.2 and g.last == {}
    assert GraphGrow(threshold_angle=5).threshold_angle == 5.0
    for bad in ("8", None, float("nan"), True):
        with pytest.raises(ValueError):
            GraphGrow(threshold_angle=bad)
    tri, h, a = np.array([[0, 1, 2], [1, 2, 3]]), np.array([1.7, 1.6]), np.array([-88.0, -87.0])
    for args in ((tri[:, :2], h, a), (tri.astype(float), h, a), (tri, h[:1], a), (tri, h, a[:1]), (np.zeros((0, 3), int), h[:0], a[:0]),
                 (np.array([[0, 1, -2]]), h[:1], a[:1]), (np.array([[0, 1, 70000]]), h[:1], a[:1])):
        with pytest.raises(ValueError, match="frame 0"):
            g.process(*args)
    with pytest.raises(ValueError, match="frame 1"):
        g.process_batch([tri, tri[:, :2]], [h, h], [a, a])
    with pytest.raises(ValueError):
        g.process_batch([tri], [h, h], [a])
    assert g.process_batch([], [], []) == []


def test_region_keyword_validates_without_a_device():
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    with pytest.raises(ValueError, match="region"):
        ScaleEstimator(1.75, 5, region="graph", delaunay_workers=0)
    for kw in ({"sampling": "device"}, {"triangulation": "gpu"}, {"triangulation": "scipy", "sampling": "device"}):
        with pytest.raises(ValueError, match="region='grow'"):
            ScaleEstimator(1.75, 5, region="grow", delaunay_workers=0, **kw)
