#!/usr/bin/env python3
"""Diagnostic: how many frames of a step the lean road-model kernel leaves on its cold list (and how many the step leaves
on the redo list), read from the context's workspace after the last step of one bench.py run in this process:
    python profiles/road_cold_count.py [bench.py args]
The lists are addressed by the batch's frame count; the workspace records the largest one it has seen, so the figures
hold for a run whose steps all have the same number of frames (bench.py's)."""
import ctypes as C
import os
import runpy
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from mvoscalerecovery_amd import _lib                 # noqa: E402


class CtxHead(C.Structure):
    """The head of `struct mvosr_ctx` (csrc/mvosr_host.hpp) up to the int workspace: nsel [F], redo list [1 + F], cold list [1 + F]."""
    _fields_ = [("device", C.c_int), ("own_stream", C.c_void_p), ("stream", C.c_void_p), ("n_cu", C.c_int),
                ("max_lds_per_block", C.c_int), ("name", C.c_char * 128), ("ws_ysel", C.c_void_p), ("ws_ysel_len", C.c_size_t),
                ("ws_nsel", C.c_void_p), ("ws_nsel_len", C.c_size_t)]


def report(ctx):
    head = CtxHead.from_address(ctx.handle.value)
    if not head.ws_nsel or head.n_cu != ctx.n_cu:
        return
    F = int(head.ws_nsel_len)
    ctx.sync()
    words = np.empty(2 * (F + 1), dtype=np.int32)
    _lib.check(ctx.lib.mvosr_memcpy_d2h(ctx.handle, C.c_void_p(words.ctypes.data), C.c_void_p(head.ws_nsel + 4 * F), C.c_size_t(words.nbytes)), "d2h")
    print("road lists after the last step: frames %d  redo list %d  cold list %d = %.3g of the frames" % (F, words[0], words[F + 1], words[F + 1] / max(F, 1)),
          file=sys.stderr)


created = []
_init = _lib.Context.__init__


def init(self, *a, **k):
    _init(self, *a, **k)
    created.append(self)


_lib.Context.__init__ = init                          # (bench.py's own context: kept alive, read once the run is over)
sys.argv = [os.path.join(R, "bench.py"), "--no-cpu-baseline", "--no-e2e"] + sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
except SystemExit as e:
    if e.code not in (None, 0):
        raise
for ctx in created:
    if getattr(ctx, "handle", None):
        report(ctx)
