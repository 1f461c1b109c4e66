#!/usr/bin/env python3
"""Diagnostic: how many lists reach the road model's skewness decision, and how many of them the guard band sends to
NumPy's exact summation order, over one bench.py run in this process.  Needs a library built with
-DMVOSR_ROAD_EXACT_COUNT (never the shipped build):
    bash profiles/ab_build.sh cnt -DMVOSR_ROAD_EXACT_COUNT
    MVOSR_LIB_PATH=profiles/ab/libmvosr_cnt.so python profiles/road_exact_count.py [bench.py args]
Prints decisions, exact by the earlier two-pass band alone, exact by the band in use (a build without the third counter
reports it as 0)."""
import ctypes as C
import os
import runpy
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.argv = [os.path.join(R, "bench.py"), "--no-cpu-baseline", "--no-e2e"] + sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
except SystemExit as e:
    if e.code not in (None, 0):
        raise
from mvoscalerecovery_amd import _lib                 # (the library bench.py loaded: same path, same handle)
lib = C.CDLL(_lib.LIB_PATH)
out = (C.c_ulonglong * 3)()
assert lib.mvosr_debug_road_exact_count(out, 0) == 0
n, old, new = out[0], out[1], out[2]
print("road decisions %d  exact (two-pass band) %d = %.3g  exact (band in use) %d = %.3g" % (n, old, old / max(n, 1), new, new / max(n, 1)))
