"""GPU: the context runtime underneath every kernel (csrc/mvosr_capi.hip through ctypes) — the copy kernel against bytes, and the
guarantee the caching allocators exist to give (include/mvosr.h: "a freed block may still be in use by work queued on the
context's streams: its next user waits for that work"), the upload fence, the allocators' bookkeeping, the shared grow-only
workspaces under launches that are not synchronised against each other, and a change of streams under work in flight.

The ordering tests follow tests/runtime_cases.py: an event behind the work in flight, "not done" observed immediately before
the call under test (the window existed), "done" at the moment the block is handed on, and bytes compared at the end.  Every
comparison is ``==`` on bytes; there is no tolerance in this file.  Nothing here provokes a fault: a runtime that breaks its
contract shows as wrong bytes in buffers the test owns.  What each test catches is recorded in LABNOTES 14."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_cases as cc
import depth_cases as dc
import runtime_cases as rc_
from runtime_cases import BIG, ERR_ARG, FILL, OK, Runtime, host_view

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = [0, 1, 15, 16, 17, 255, 4095, 4096, 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 * (1 << 20) + 5]   # one trip of the grid: 2^20 bytes
OFFSETS = (0, 1, 8, 16)


@pytest.fixture
def fresh():
    """A context of the test's own (empty caches, empty workspaces), closed afterwards."""
    from mvoscalerecovery_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


# ---- 1. the copy kernel against bytes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def copy_blocks(gpu):
    """A device block of random bytes and a page-locked destination, both as long as the largest case with its offsets and guards."""
    rt = Runtime(gpu)
    n = max(SIZES) + max(OFFSETS)
    src = np.frombuffer(np.random.default_rng(5).bytes(n), dtype=np.uint8)
    d = rt.malloc(n)
    rt.h2d(d, src)
    total = GUARD + n + GUARD
    h = rt.host_alloc(total)
    yield rt, src, d, h, total
    rt.sync()
    rt.free(d)
    rt.host_free(h)


@pytest.mark.parametrize("size", SIZES)
def test_copy_kernel_bytes_and_guards(copy_blocks, size):
    """mvosr_memcpy_d2h_kernel at every pairing of source and destination offsets {0, 1, 8, 16}: 16-byte vectors only where both
    ends are 16-aligned, a byte tail behind them, bytes alone otherwise ((8, 8) included).  The destination range equals the
    source bytes and every other byte of the buffer — 64 guard bytes before and after, at least — keeps 0x5A."""
    rt, src, d, h, total = copy_blocks
    assert d % 256 == 0 and h % 256 == 0
    buf = host_view(h, total)
    for so, do in itertools.product(OFFSETS, OFFSETS):
        buf[:] = FILL
        rt.d2h_kernel(h + GUARD + do, d + so, size)
        ev = rt.event()
        rt.wait(ev)
        rt.drop(ev)
        a = GUARD + do
        assert np.array_equal(buf[a:a + size], src[so:so + size]), (size, so, do, "copied range")
        assert (buf[:a] == FILL).all() and (buf[a + size:] == FILL).all(), (size, so, do, "bytes outside the range")


def test_copy_null_arguments(gpu):
    """Size 0: MVOSR_OK and nothing written, also with null pointers; bytes > 0 with a null end: MVOSR_ERR_ARG — for the copy
    kernel and both asynchronous copies."""
    rt = Runtime(gpu)
    d, h = rt.malloc(4096), rt.host_alloc(4096)
    rt.memset(d, 0x33, 4096)
    rt.sync()
    host_view(h, 4096)[:] = FILL
    lib, ctx = gpu.lib, gpu.handle
    try:
        for name, dst, src in (("mvosr_memcpy_d2h_kernel", h, d), ("mvosr_memcpy_d2h_async", h, d), ("mvosr_memcpy_h2d_async", d, h)):
            fn = getattr(lib, name)
            assert fn(ctx, dst, src, 0) == OK and fn(ctx, None, None, 0) == OK and fn(ctx, dst, None, 0) == OK, name
            assert fn(ctx, None, src, 16) == ERR_ARG and "null" in rt.error(), name
            assert fn(ctx, dst, None, 16) == ERR_ARG and "null" in rt.error(), name
            assert fn(None, dst, src, 16) == ERR_ARG, name
        rt.fence()
        rt.sync()
        assert (host_view(h, 4096) == FILL).all() and (rt.d2h(d, 4096) == 0x33).all()
    finally:
        rt.free(d)
        rt.host_free(h)


# ---- 2. staging buffers: the next user waits for the upload ---------------------------------------------------------------------
@pytest.mark.parametrize("style", rc_.STAGING_STYLES)
def test_staging_buffer_waits_for_its_upload(fresh, style):
    """Six rounds of alloc / fill / asynchronous upload / event / release per release style (runtime_cases.staging_rounds).  A
    pointer that was the source of copy j comes back only once E_j is done; every target ends with its own pattern; page-locked
    memory grows by two blocks at the most ("once: from then on two rotate"), which then rotate."""
    rt = Runtime(fresh)
    res = rc_.staging_rounds(rt, BIG, rc_.patterns(BIG, 6), style)
    print("%s: %d MiB, copy in flight before the next request in %d of %d rounds; %d re-uses, %d blocks allocated, %d distinct pointers"
          % (style, BIG >> 20, sum(res["in_flight"]), len(res["in_flight"]), len(res["reuses"]), res["host_malloc"], res["distinct"]))
    assert not [r for r in res["reuses"] if not r[2]], ("a staging buffer handed out while it was the source of a copy in flight (round, copy, done)", res["reuses"])
    assert res["wrong"] == [], ("targets that do not hold their own pattern", res["wrong"])
    assert res["host_malloc"] <= 2 and res["distinct"] <= 2, res
    assert res["reuses"], "no block was ever re-used: the rounds tested nothing"
    assert any(res["in_flight"]), "no copy was in flight when the next buffer was asked for: the buffer is too small"


# ---- 3. device blocks: the next user waits for the download ---------------------------------------------------------------------
@pytest.mark.parametrize("reader,release", [("kernel", "free"), ("kernel", "mark_now"), ("async", "free"), ("async", "mark_now")])
def test_device_block_waits_for_its_reader(fresh, reader, release):
    """runtime_cases.device_round: the block is read by the copy kernel (or a queued download), released, asked for again and
    overwritten at once by an upload that nothing but the allocator's wait orders behind the reader."""
    res = rc_.device_rounds(Runtime(fresh), BIG, reader, release)
    rc_.check_device_rounds(res, "%d MiB, %s reader, %s" % (BIG >> 20, reader, release))


# ---- 4. the fence ---------------------------------------------------------------------------------------------------------------
def test_fence_orders_the_compute_stream_behind_uploads(fresh):
    """Upload, mvosr_upload_fence, copy kernel out of the same block: the kernel reads what was uploaded, for one large copy and
    for 32 copies of 4 KiB behind one fence (queued behind another large upload, so that they are still waiting at the fence)."""
    rt = Runtime(fresh)
    small, count = 4096, 32
    pat = rc_.patterns(BIG, 3, seed=4)
    d, d_other, d_small = rt.malloc(BIG), rt.malloc(BIG), rt.malloc(small * count)
    s, s_other, s_small = rt.host_alloc(BIG), rt.host_alloc(BIG), rt.host_alloc(small * count)
    h, h_small = rt.host_alloc(BIG), rt.host_alloc(small * count)
    host_view(s, BIG)[:] = pat[0]
    host_view(s_other, BIG)[:] = pat[1]
    host_view(s_small, small * count)[:] = pat[2][:small * count]
    for p, n in ((d, BIG), (d_other, BIG), (d_small, small * count)):
        rt.memset(p, FILL, n)
    host_view(h, BIG)[:] = 0
    host_view(h_small, small * count)[:] = 0
    rt.sync()
    # one large copy
    rt.h2d_async(d, s, BIG)
    rt.fence()
    rt.d2h_kernel(h, d, BIG)
    ev = rt.event()
    rt.wait(ev)
    rt.drop(ev)
    large_ok = np.array_equal(host_view(h, BIG), pat[0])
    # 32 small ones behind one fence
    rt.h2d_async(d_other, s_other, BIG)
    for i in range(count):
        rt.h2d_async(d_small + i * small, s_small + i * small, small)
    rt.fence()
    rt.d2h_kernel(h_small, d_small, small * count)
    ev = rt.event()
    rt.wait(ev)
    rt.drop(ev)
    small_ok = [i for i in range(count) if not np.array_equal(host_view(h_small, small * count)[i * small:(i + 1) * small], pat[2][i * small:(i + 1) * small])]
    rt.fence()
    rt.sync()
    other_ok = np.array_equal(rt.d2h(d_other, BIG), pat[1])
    for p in (d, d_other, d_small):
        rt.free(p)
    for p in (s, s_other, s_small, h, h_small):
        rt.host_free(p)
    assert large_ok, "the copy kernel behind the fence did not read the uploaded bytes"
    assert small_ok == [], ("4 KiB copies the kernel behind the fence did not see", small_ok)
    assert other_ok


# ---- 5. bookkeeping -------------------------------------------------------------------------------------------------------------
def test_allocator_bookkeeping(fresh):
    rt = Runtime(fresh)
    lib, h = fresh.lib, fresh.handle
    start = rt.stats()
    assert start["live_blocks"] == 0 and start["cached_device_bytes"] == 0 and start["cached_host_bytes"] == 0
    # live blocks; double free, foreign pointers, NULL
    d, p = rt.malloc(1000), rt.host_alloc(1000)
    assert rt.stats()["live_blocks"] == 2
    rt.free(d)
    rt.host_free(p)
    assert rt.stats()["live_blocks"] == 0
    for fn, ptr in ((lib.mvosr_free, d), (lib.mvosr_host_free, p), (lib.mvosr_free, p), (lib.mvosr_host_free, d),
                    (lib.mvosr_free, 0x1000), (lib.mvosr_host_free, 0x1000)):
        assert fn(h, ptr) == ERR_ARG and ("%x" % ptr) in rt.error().lower(), (ptr, rt.error())      # (twice / the other allocator's / nobody's)
    assert lib.mvosr_free(h, None) == OK and lib.mvosr_host_free(h, None) == OK
    # marks
    assert lib.mvosr_block_mark(h, 0x1000, rc_.MARK_NOW) == ERR_ARG and "1000" in rt.error()
    assert lib.mvosr_block_mark(h, d, rc_.MARK_NOW) == ERR_ARG                                      # (a cached block is not a live one)
    assert lib.mvosr_block_mark(h, None, rc_.MARK_NOW) == ERR_ARG
    q = rt.malloc(1000)
    assert lib.mvosr_block_mark(h, q, 7) == ERR_ARG and "7" in rt.error()
    for m in (rc_.MARK_NOW, rc_.MARK_IDLE, rc_.MARK_UPLOAD, 0):
        assert lib.mvosr_block_mark(h, q, m) == OK, m
    # a request of the same size after a free: the same pointer, a cache hit, no hipMalloc
    assert q == d
    s0 = rt.stats()
    rt.free(q)
    q2 = rt.malloc(1000)
    s1 = rt.stats()
    assert q2 == q and s1["cache_hits"] == s0["cache_hits"] + 1 and s1["hip_malloc"] == s0["hip_malloc"]
    # never to a larger request (1000 B is a 1024-byte block)
    rt.free(q2)
    big = rt.malloc(1025)
    s2 = rt.stats()
    assert big != q2 and s2["hip_malloc"] == s1["hip_malloc"] + 1 and s2["cache_hits"] == s1["cache_hits"]
    # ... nor to a much smaller one ("<= want + want/4"): a cached 2 MiB block does not serve 1 MiB, for device and host
    for alloc, free, key in ((rt.malloc, rt.free, "hip_malloc"), (rt.host_alloc, rt.host_free, "host_malloc")):
        two = alloc(2 << 20)
        free(two)
        rt.sync()                              # (the release's event is done: a page-locked block that is busy is not waited for but doubled)
        a = rt.stats()
        one = alloc(1 << 20)
        b = rt.stats()
        assert one != two and b[key] == a[key] + 1 and b["cache_hits"] == a["cache_hits"], key
        again = alloc(2 << 20)
        assert again == two and rt.stats()["cache_hits"] == b["cache_hits"] + 1, key
        free(one)
        free(again)
    # trim: the cached blocks go back to the runtime, live blocks keep their contents
    pat = rc_.patterns(1 << 20, 1, seed=9)[0]
    keep = rt.malloc(1 << 20)
    rt.h2d(keep, pat)
    before = rt.stats()
    assert before["cached_device_bytes"] > 0 and before["cached_host_bytes"] > 0 and before["live_blocks"] == 2      # keep, big
    rt.trim()
    after = rt.stats()
    assert after["cached_device_bytes"] == 0 and after["cached_host_bytes"] == 0 and after["live_blocks"] == 2
    assert after["hip_free"] > before["hip_free"] and after["host_free"] > before["host_free"]
    assert np.array_equal(rt.d2h(keep, 1 << 20), pat)
    rt.free(keep)
    rt.free(big)
    assert rt.stats()["live_blocks"] == start["live_blocks"]


# ---- 6. one workspace, several tenants, no synchronisation between the calls ----------------------------------------------------
def test_shared_workspace_cloud_and_depth_queued(gpu, fresh):
    """mvosr_point_cloud_batch on 64x8 frames, on 310x94 frames (the context's byte workspace is freed and reallocated) and on
    the small ones again, mvosr_dense_depth_batch — another layout of the same workspace — in between, all queued on a fresh
    context with no synchronisation between the calls: every result is byte-identical to the same call alone on the session
    context with a synchronisation around it, and the clouds equal the CPU restatement."""
    crafted_camera = lambda w, hgt: dc.camera(w, hgt, 0.58 * w, 0.61 * w, 0.49 * w, 0.52 * hgt)       # (tests/test_gpu_cloud.py's)
    batches = {}
    for key, (w, hgt) in (("small", (64, 8)), ("large", (310, 94))):
        cam = crafted_camera(w, hgt)
        _, depth, tri, images, scales = cc.crafted_batch(w, hgt, hostile=False)
        want = cc.clouds(depth, tri, cam, images, scales)
        batches[key] = (cam, depth, tri, images, scales, int(want[2][-1]), want)
    frames = [fr for fr in dc.load_fixture("depth_small") if (fr["cam"].width, fr["cam"].height) == (310, 94)]
    assert len(frames) >= 2
    dargs = (frames[0]["cam"], [fr["f3"] for fr in frames], [fr["f2"] for fr in frames], [fr["rows"] for fr in frames])
    cloud = lambda ctx, key: rc_.CloudCall(ctx, *batches[key][:6])
    depth_call = lambda ctx: rc_.DepthCall(ctx, *dargs)
    alone = {"small": rc_.run_alone(cloud(gpu, "small")), "large": rc_.run_alone(cloud(gpu, "large")), "depth": rc_.run_alone(depth_call(gpu))}
    for key in ("small", "large"):
        pts, cols, off = batches[key][6]
        K = int(off[-1])
        got = alone[key]
        assert got["overflow"][0] == 0 and np.array_equal(got["frame_off"][:-1], off), key
        assert cc.same_bytes(got["points"][:K], pts) and cc.same_bytes(got["colors"][:K], cols), key
        assert (got["points"][K:].view(np.uint8) == FILL).all() and (got["colors"][K:].view(np.uint8) == FILL).all(), key
    assert (alone["depth"]["status"] == 0).all() and (alone["depth"]["covered"] > 0).all()
    order = ["small", "large", "depth", "small", "depth", "large", "small"]
    got = rc_.run_queued(fresh, [depth_call(fresh) if k == "depth" else cloud(fresh, k) for k in order])
    for i, k in enumerate(order):
        assert rc_.same_results(got[i], alone[k]), (i, k, "queued call differs from the call alone")


def test_shared_workspace_scale_batches_queued(gpu, fresh):
    """mvosr_scale_batch: a 3-frame batch, a 40-frame batch of larger frames — both arrays of the scale kernels' workspace grow,
    the redo list and the size classes' header with them — and the 3-frame batch again, queued with no synchronisation between
    the calls; status and raw scale against the oracle, every output byte-identical to the call alone."""
    from gpu_helpers import _oracle_frames
    from mvoscalerecovery_amd import synth
    sets = {"few": [synth.synth_frame(i, n, base_seed=99) for i, n in enumerate((300, 700, 350))],
            "many": [synth.synth_frame(i, 900 + 13 * i, base_seed=41) for i in range(40)]}
    ores = {k: _oracle_frames(v) for k, v in sets.items()}
    call = lambda ctx, k: rc_.ScaleCall(ctx, sets[k], ores[k])
    alone = {k: rc_.run_alone(call(gpu, k)) for k in sets}
    order = ["few", "many", "few", "many", "few"]
    got = rc_.run_queued(fresh, [call(fresh, k) for k in order])
    for i, k in enumerate(order):
        for f, r in enumerate(ores[k]):
            want = r.raw_scale
            assert got[i]["status"][f] == r.status and (got[i]["raw_scale"][f] == want or (np.isnan(want) and np.isnan(got[i]["raw_scale"][f]))), (i, k, f)
        assert rc_.same_results(got[i], alone[k]), (i, k, "queued call differs from the call alone")


# ---- 7. stream adoption ---------------------------------------------------------------------------------------------------------
def test_stream_adoption_keeps_the_allocator_contract(gpu):
    """runtime_cases.stream_adoption in a child process (torch and its stream, as tests/test_gpu_multirank.py adopts one): item 3
    on an adopted stream, then the context's own stream restored — and a second stream adopted — while the first still has the
    reader in flight; a block released after the switch must still wait for that reader."""
    from conftest import ROOT
    code = "import sys; sys.path[:0] = [%r, %r]; import runtime_cases; runtime_cases.stream_adoption()" % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "stream adoption ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
