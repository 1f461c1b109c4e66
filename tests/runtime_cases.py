"""Drivers of tests/test_gpu_runtime.py (import-only, as ``flat_cases.py`` is): the memory, stream and event part of the C ABI
(include/mvosr.h) through ctypes, the ordering rounds of the caching allocators, and the kernels' launchers cut in three —
prepare, launch, collect — so that several launches can be queued on one context with no synchronisation between them.

The ordering rounds do not depend on luck.  Behind the work in flight they place an event ``E`` (mvosr_event_record; for work
of the upload stream mvosr_upload_fence first, which puts the compute stream behind it) and report, per round,
  in flight:  ``E`` was NOT done immediately before the call under test — the window existed;
  contract:   ``E`` WAS done at the moment the call under test handed the block to its next user;
  data:       after a final synchronisation every destination holds the bytes its own source had when the copy was queued.
Nothing here reads or writes outside a block the test owns: a runtime that breaks the contract shows as wrong BYTES."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

OK, ERR_ARG = 0, -2
FILL = 0x5A
MARK_NOW, MARK_IDLE, MARK_UPLOAD = 1, 2, 3
BIG = 64 << 20          # bytes of the large buffers: the size at which a copy outlasts the host's next few calls (LABNOTES 14)


class Runtime:
    """mvosr_malloc ... mvosr_event_query on one ``_lib.Context``; a call that is expected to succeed is asserted to."""

    def __init__(self, ctx):
        self.ctx, self.lib, self.h = ctx, ctx.lib, ctx.handle

    def error(self):
        return (self.lib.mvosr_last_error() or b"").decode()

    def _ok(self, rc, what):
        assert rc == OK, (what, rc, self.error())

    def _alloc(self, fn, n, what):
        p = C.c_void_p()
        self._ok(fn(self.h, n, C.byref(p)), what)
        assert p.value
        return p.value

    def malloc(self, n):
        return self._alloc(self.lib.mvosr_malloc, n, "mvosr_malloc")

    def host_alloc(self, n):
        return self._alloc(self.lib.mvosr_host_alloc, n, "mvosr_host_alloc")

    def free(self, p):
        self._ok(self.lib.mvosr_free(self.h, p), "mvosr_free")

    def host_free(self, p):
        self._ok(self.lib.mvosr_host_free(self.h, p), "mvosr_host_free")

    def mark(self, p, m):
        self._ok(self.lib.mvosr_block_mark(self.h, p, m), "mvosr_block_mark")

    def h2d(self, d, arr):                       # synchronous, from any host array
        arr = np.ascontiguousarray(arr)
        self._ok(self.lib.mvosr_memcpy_h2d(self.h, d, arr.ctypes.data, arr.nbytes), "mvosr_memcpy_h2d")

    def d2h(self, d, n):                         # synchronous
        out = np.empty(n, np.uint8)
        self._ok(self.lib.mvosr_memcpy_d2h(self.h, out.ctypes.data, d, n), "mvosr_memcpy_d2h")
        return out

    def h2d_async(self, d, s, n):
        self._ok(self.lib.mvosr_memcpy_h2d_async(self.h, d, s, n), "mvosr_memcpy_h2d_async")

    def d2h_async(self, h, d, n):
        self._ok(self.lib.mvosr_memcpy_d2h_async(self.h, h, d, n), "mvosr_memcpy_d2h_async")

    def d2h_kernel(self, h, d, n):
        self._ok(self.lib.mvosr_memcpy_d2h_kernel(self.h, h, d, n), "mvosr_memcpy_d2h_kernel")

    def memset(self, d, byte, n):
        self._ok(self.lib.mvosr_memset(self.h, d, byte, n), "mvosr_memset")

    def fence(self):
        self._ok(self.lib.mvosr_upload_fence(self.h), "mvosr_upload_fence")

    def sync(self):
        self._ok(self.lib.mvosr_ctx_sync(self.h), "mvosr_ctx_sync")

    def trim(self):
        self._ok(self.lib.mvosr_ctx_trim(self.h), "mvosr_ctx_trim")

    def event(self):
        """A new event recorded on the context's current stream."""
        ev = C.c_void_p()
        self._ok(self.lib.mvosr_event_create(self.h, C.byref(ev)), "mvosr_event_create")
        self._ok(self.lib.mvosr_event_record(self.h, ev), "mvosr_event_record")
        return ev

    def done(self, ev):
        d = C.c_int(-1)
        self._ok(self.lib.mvosr_event_query(self.h, ev, C.byref(d)), "mvosr_event_query")
        assert d.value in (0, 1)
        return bool(d.value)

    def wait(self, ev):
        self._ok(self.lib.mvosr_event_sync(self.h, ev), "mvosr_event_sync")

    def drop(self, ev):
        self._ok(self.lib.mvosr_event_destroy(self.h, ev), "mvosr_event_destroy")

    def stats(self):
        return self.ctx.alloc_stats()


def host_view(p, n):
    """``n`` bytes of host memory at address ``p`` as a writable uint8 array."""
    return np.frombuffer((C.c_uint8 * n).from_address(p), dtype=np.uint8)


@functools.lru_cache(maxsize=2)
def patterns(n, count, seed=0):
    """``count`` byte patterns of ``n`` bytes (a multiple of 8) that differ from each other in EVERY byte: one random block,
    xor-ed with a byte of its own per pattern."""
    base = np.frombuffer(np.random.default_rng(seed).bytes(n), dtype=np.uint64)
    return [(base ^ np.uint64(0x0101010101010101 * (1 + 37 * k % 255))).view(np.uint8) for k in range(count)]


# ---- item 2: staging buffers ----------------------------------------------------------------------------------------------
STAGING_STYLES = ("free", "mark_upload", "mark_now", "idle_withdrawn", "free_before_event")


def staging_rounds(rt, n, pats, style):
    """Per round k: mvosr_host_alloc(n), fill with pats[k] at once, mvosr_memcpy_h2d_async into a device target of its own,
    the event behind the copy, release in ``style`` —
      free: mvosr_host_free alone;  mark_upload / mark_now: that mark, then free;
      idle_withdrawn: MVOSR_MARK_IDLE, then mark 0, then free (a withdrawn mark: the block is an unmarked one again);
      free_before_event: as ``free``, but released BEFORE the fence and the event are placed (the fence itself puts the compute
      stream behind the copy, so only this order shows whether the release looked at the upload stream).
    Returns the observations; asserts nothing about ordering itself (the caller does, after everything has been waited for)."""
    rounds = len(pats)
    targets = [rt.malloc(n) for _ in range(rounds)]
    for d in targets:
        rt.memset(d, FILL, n)
    rt.sync()
    before = rt.stats()
    events, source_of, reuses, in_flight, pointers = [], {}, [], [], []
    for k in range(rounds):
        if k:
            in_flight.append(not rt.done(events[-1]))            # immediately before the call under test
        s = rt.host_alloc(n)
        reuses += [(k, j, rt.done(events[j])) for j in source_of.get(s, ())]        # the contract, at the moment of the hand-over
        host_view(s, n)[:] = pats[k]
        rt.h2d_async(targets[k], s, n)
        if style == "free_before_event":
            rt.host_free(s)
        rt.fence()
        events.append(rt.event())
        if style == "mark_upload":
            rt.mark(s, MARK_UPLOAD)
        elif style == "mark_now":
            rt.mark(s, MARK_NOW)
        elif style == "idle_withdrawn":
            rt.mark(s, MARK_IDLE)
            rt.mark(s, 0)
        if style != "free_before_event":
            rt.host_free(s)
        source_of.setdefault(s, []).append(k)
        pointers.append(s)
    rt.fence()
    rt.sync()
    after = rt.stats()
    wrong = [k for k in range(rounds) if not np.array_equal(rt.d2h(targets[k], n), pats[k])]
    for ev in events:
        rt.drop(ev)
    for d in targets:
        rt.free(d)
    return {"in_flight": in_flight, "reuses": reuses, "wrong": wrong, "host_malloc": after["host_malloc"] - before["host_malloc"],
            "distinct": len(set(pointers))}


# ---- items 3 and 7: device blocks -----------------------------------------------------------------------------------------
def device_round(rt, n, p1, p2, reader, release, switch=None):
    """mvosr_malloc(n), synchronous upload of p1, ``reader`` ("kernel": mvosr_memcpy_d2h_kernel, "async":
    mvosr_memcpy_d2h_async) into a page-locked H1, the event, [MVOSR_MARK_NOW when ``release`` == "mark_now"], [``switch()``:
    item 7 changes the context's stream here, with the reader in flight on the old one], release, mvosr_malloc(n) again and AT
    ONCE mvosr_memcpy_h2d_async of p2 (its last quarter first) into whatever came back — no fence: the upload stream is not ordered behind the
    reader's stream, only the allocator's wait keeps p2 out of the reader's way."""
    d = rt.malloc(n)
    rt.h2d(d, p1)
    h1, s2 = rt.host_alloc(n), rt.host_alloc(n)
    host_view(h1, n)[:] = FILL
    host_view(s2, n)[:] = p2
    rt.sync()
    (rt.d2h_kernel if reader == "kernel" else rt.d2h_async)(h1, d, n)
    ev = rt.event()                             # (before the mark: the mark's own event is then behind it, as a release's is)
    if release == "mark_now":
        rt.mark(d, MARK_NOW)
    if switch is not None:
        switch()
    in_flight = not rt.done(ev)                 # immediately before the calls under test
    rt.free(d)
    d2 = rt.malloc(n)
    done = rt.done(ev)                          # the contract, at the moment of the hand-over
    q = n // 4 * 3                              # the LAST quarter first: the reader gets there last, so an upload that was let in
    rt.h2d_async(d2 + q, s2 + q, n - q)         # early overwrites bytes the reader has yet to read (both sweep the block front to back)
    rt.h2d_async(d2, s2, q)
    rt.wait(ev)
    rt.fence()
    rt.sync()
    res = {"in_flight": in_flight, "done": done, "same_block": d2 == d,
           "h1_ok": bool(np.array_equal(host_view(h1, n), p1)), "d2_ok": bool(np.array_equal(rt.d2h(d2, n), p2))}
    rt.drop(ev)
    rt.host_free(h1)
    rt.host_free(s2)
    rt.free(d2)
    return res


def device_rounds(rt, n, reader, release, rounds=3, switch=None, seed=0):
    """``rounds`` rounds of ``device_round`` on a context whose caches are empty at the start, so that the released block is the
    only one the second request can be served from."""
    rt.trim()
    pats = patterns(n, 2 * rounds, seed)
    return [device_round(rt, n, pats[2 * r], pats[2 * r + 1], reader, release, switch) for r in range(rounds)]


def check_device_rounds(res, label):
    print("%s: in flight before the release in %d of %d rounds" % (label, sum(r["in_flight"] for r in res), len(res)))
    assert all(r["same_block"] for r in res), (label, "the second request was not served from the released block", res)
    assert all(r["done"] for r in res), (label, "block handed out while its reader was in flight", res)
    assert all(r["h1_ok"] for r in res), (label, "the reader's destination does not hold the first pattern", res)
    assert all(r["d2_ok"] for r in res), (label, "the block does not hold the second pattern", res)
    assert any(r["in_flight"] for r in res), (label, "the reader was never in flight at the release: the buffer is too small", res)


# ---- item 6: launches without a synchronisation between them --------------------------------------------------------------
def same_results(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).shape == np.asarray(b[k]).shape
                                    and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


class CloudCall:
    """mvosr_point_cloud_batch on a crafted batch (the ``raw_call`` of tests/test_gpu_cloud.py, cut in three): inputs uploaded and
    outputs pre-filled with FILL bytes by the constructor, ``launch`` queues the kernels and returns, ``collect`` downloads."""

    def __init__(self, ctx, cam, depth, tri, images, scales, capacity, room=64):
        from mvoscalerecovery_amd import _lib
        self.ctx, F = ctx, len(depth)
        self.ins = [ctx.to_device(depth), ctx.to_device(tri), ctx.to_device(images), ctx.to_device(scales)]
        self.outs = {"points": ctx.empty((capacity + room, 3), np.float64), "colors": ctx.empty((capacity + room, 3), np.float64),
                     "frame_off": ctx.empty(F + 2, np.int64), "overflow": ctx.empty(2, np.int32)}
        for b in self.outs.values():
            b.fill(FILL)
        self.i = _lib.CloudInputs(*[b.ptr for b in self.ins], F)
        self.p = _lib.CloudParams(0.0, 0.0, 1, 0)
        self.o = _lib.CloudOutputs(self.outs["points"].ptr, self.outs["colors"].ptr, self.outs["frame_off"].ptr, self.outs["overflow"].ptr, capacity)
        self.c = _lib.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)

    def launch(self):
        rc = self.ctx.lib.mvosr_point_cloud_batch(self.ctx.handle, C.byref(self.i), C.byref(self.c), C.byref(self.p), C.byref(self.o))
        assert rc == OK, (rc, self.ctx.lib.mvosr_last_error())

    def collect(self):
        got = {k: b.download() for k, b in self.outs.items()}
        for b in list(self.outs.values()) + self.ins:
            b.free()
        return got


class DepthCall:
    """mvosr_dense_depth_batch on a packed batch (the ``launch`` of tests/test_gpu_depth.py, cut in three)."""

    def __init__(self, ctx, cam, f3s, f2s, rows):
        from mvoscalerecovery_amd import _lib, packing
        from mvoscalerecovery_amd.engine import DeviceBatch
        from mvoscalerecovery_amd.reconstruct import pack_all
        self.ctx = ctx
        F, H, W = len(f3s), cam.height, cam.width
        pf = pack_all([np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in f3s], [np.asarray(b, dtype=np.float64).reshape(-1, 2) for b in f2s])
        off, flat = packing._pack_tris([np.ascontiguousarray(r, dtype=np.int32).reshape(-1, 3) for r in rows])
        pf.tri1_off, pf.tri1 = off, flat
        self.db = DeviceBatch(ctx, pf, with_tri2=False)
        self.d_u = ctx.to_device(pf.u)
        self.bufs = {"depth": ctx.empty((F, H, W), np.float64), "tri_id": ctx.empty((F, H, W), np.int32),
                     "tri_model": ctx.empty((max(int(off[-1]), 1), 4), np.float64), "covered": ctx.empty(F, np.int32), "status": ctx.empty(F, np.int32)}
        for b in self.bufs.values():
            b.fill(FILL)
        self.o = _lib.DepthOutputs(self.bufs["depth"].ptr, self.bufs["tri_id"].ptr, self.bufs["tri_model"].ptr, self.bufs["covered"].ptr,
                                   self.bufs["status"].ptr)
        self.c = _lib.Camera(W, H, cam.fx, cam.fy, cam.cx, cam.cy)
        self.bs = self.db.struct()

    def launch(self):
        rc = self.ctx.lib.mvosr_dense_depth_batch(self.ctx.handle, C.byref(self.bs), 1, self.d_u.ptr, None, C.byref(self.c), C.byref(self.o), 0, 0)
        assert rc == OK, (rc, self.ctx.lib.mvosr_last_error())

    def collect(self):
        got = {k: b.download() for k, b in self.bufs.items()}
        for b in list(self.bufs.values()) + [self.d_u]:
            b.free()
        self.db.free()
        return got


class ScaleCall:
    """mvosr_scale_batch on packed frames with the oracle's triangulations (as tests/test_gpu_kernels.py launches it)."""

    def __init__(self, ctx, frames, ores, abs_ref=1.75):
        from gpu_helpers import _pack
        from mvoscalerecovery_amd.engine import DeviceBatch, DeviceOutputs, ScaleEngine
        self.ctx = ctx
        pf = _pack(frames, [r.tri1 for r in ores], [r.tri2 for r in ores], [r.valid for r in ores])
        self.eng = ScaleEngine(abs_ref, ctx=ctx)
        self.db = DeviceBatch(ctx, pf)
        self.out = DeviceOutputs(ctx, self.db, counts=True)

    def launch(self):
        self.eng.scale_batch(self.db, self.out)

    def collect(self):
        got = {k: self.out.get(k) for k in ("status", "raw_scale", "height", "height_level", "counts")}
        self.out.free()
        self.db.free()
        return got


def run_alone(call):
    """One call with a synchronisation before and after it."""
    call.ctx.sync()
    call.launch()
    call.ctx.sync()
    return call.collect()


def run_queued(ctx, calls):
    """Every call of ``calls`` queued on ``ctx`` back to back: one synchronisation before the first, one after the last."""
    ctx.sync()
    for c in calls:
        c.launch()
    ctx.sync()
    return [c.collect() for c in calls]


# ---- item 7: an adopted stream, run by a child process (see test_gpu_runtime.test_stream_adoption) -------------------------
def stream_adoption(n=BIG):
    """Adopt a torch stream; item 3's rounds on it; then the rounds again with the context's own stream restored (NULL) while the
    adopted stream still has the reader in flight, the block released after the switch.  Prints the in-flight shares."""
    import torch
    from mvoscalerecovery_amd import _lib
    torch.cuda.set_device(0)
    ctx = _lib.Context(0)
    rt = Runtime(ctx)
    stream = torch.cuda.Stream(device=0)
    adopt = lambda: ctx.set_stream(stream.cuda_stream)
    adopt()
    try:
        for reader, release in (("kernel", "free"), ("kernel", "mark_now"), ("async", "free")):
            check_device_rounds(device_rounds(rt, n, reader, release), "adopted stream, %s reader, %s" % (reader, release))
        for reader in ("kernel", "async"):
            res = []
            for r in range(3):
                adopt()
                res += device_rounds(rt, n, reader, "free", rounds=1, switch=lambda: ctx.set_stream(None), seed=r)
            check_device_rounds(res, "own stream restored under the %s reader" % reader)
        # and from one adopted stream to another
        other = torch.cuda.Stream(device=0)
        res = []
        for r in range(3):
            adopt()
            res += device_rounds(rt, n, "kernel", "free", rounds=1, switch=lambda: ctx.set_stream(other.cuda_stream), seed=10 + r)
        check_device_rounds(res, "a second adopted stream under the kernel reader")
        ctx.set_stream(None)
    finally:
        torch.cuda.synchronize()
        ctx.close()
    print("stream adoption ok")
