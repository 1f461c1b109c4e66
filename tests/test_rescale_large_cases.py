"""CPU: the large-frame kernels' plan header (csrc/mvosr_rescale_large_plan.hpp) compiled with g++ into a stand-alone program; the
two entry points declared and bound; the chunk routing of ScaleEstimator(large_frames=True) as a pure function; the keyword's
handling where no device is needed."""
import os
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>
#include "mvosr_rescale_large_plan.hpp"
using namespace mvosr;

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
struct Region { const char *name; size_t off, bytes, align; unsigned live; };
static size_t audit(const char *plan, const std::vector<Region> &r) {
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % r[i].align == 0, "%s.%s at %zu needs %zu", plan, r[i].name, r[i].off, r[i].align);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j) {
            if (!(r[i].live & r[j].live) || !r[i].bytes || !r[j].bytes) continue;
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s.%s overlaps %s", plan, r[i].name, r[j].name);
        }
    }
    return end;
}
#define SAME32(f) CHECK((size_t)p.f == q.f, "32-bit and size_t plans differ at " #f)

static void plans() {
    // the flat plan: a function of n_hyp alone (there is no frame size to pass), every region live together
    for (long long h : {1ll, 7ll, 100ll, 511ll, 512ll}) {
        const FlatLargePlan<size_t> q = flat_large_plan<size_t>((size_t)h);
        const FlatLargePlan<uint32_t> p = flat_large_plan<uint32_t>((uint32_t)h);
        SAME32(ext); SAME32(misc); SAME32(hist); SAME32(mods); SAME32(cnts); SAME32(total);
        const size_t end = audit("flat_large", {{"ext", q.ext, 4 * 8, 8, 1u}, {"misc", q.misc, 4u * FM_N, 4, 1u},
                                                {"hist", q.hist, 4u * kFlatBins, 8, 1u},          // (later uint64[64]: 8-aligned)
                                                {"mods", q.mods, (size_t)kPlaneBytes * (size_t)h, 32, 1u}, {"cnts", q.cnts, 4u * (size_t)h, 4, 1u}});
        CHECK(end <= q.total, "flat_large: n_hyp %lld", h);
        CHECK(8u * 64 <= 4u * kFlatBins, "the direct list fits the histogram");
    }
    CHECK(flat_large_plan<size_t>(512).total <= 160u * 1024, "n_hyp = 512 fits 160 KiB: %zu", flat_large_plan<size_t>(512).total);
    CHECK(kLargeWaves <= 16 && FM_CW + kLargeWaves <= FM_N && FM_WSUM + kLargeWaves <= FM_CW, "misc slots per wavefront");
    // the vote's plan: a function of the tile; the tile never grows past kGraphLargeMaxTile whatever the header's max_feat
    size_t largest = 0;
    for (long long mf : {0ll, 1ll, 63ll, 64ll, 65ll, 300ll, 3400ll, 8191ll, 8192ll, 8193ll, 20000ll, 32000ll, 1000000ll, 2000000000ll})
        for (long long asked : {0ll, -1ll, 1ll, 64ll, 100ll, 8192ll, 8193ll, 1000000ll}) {
            const long long t = graph_large_tile<long long>(asked, mf);
            CHECK(t >= 1 && t <= kGraphLargeMaxTile, "tile %lld (asked %lld, max_feat %lld)", t, asked, mf);
            CHECK(asked <= 0 || asked > kGraphLargeMaxTile || t == asked, "a caller's tile within the cap is taken as it is");
            const GraphLargePlan<size_t> q = graph_large_plan<size_t>((size_t)t);
            const GraphLargePlan<uint32_t> p = graph_large_plan<uint32_t>((uint32_t)t);
            SAME32(total_cnt); SAME32(good_cnt); SAME32(flag); SAME32(total);
            const size_t end = audit("graph_large", {{"total", q.total_cnt, 4u * (size_t)t, 4, 1u}, {"good", q.good_cnt, 4u * (size_t)t, 4, 1u},
                                                     {"flag", q.flag, 8, 4, 1u}});
            CHECK(end <= q.total, "graph_large: tile %lld", t);
            if (q.total > largest) largest = q.total;
        }
    CHECK(largest == graph_large_plan<size_t>(kGraphLargeMaxTile).total && largest <= 160u * 1024, "the vote's LDS is bounded: %zu", largest);
    // the workspace: regions disjoint and aligned, absent ones empty, the total a function of the batch
    for (int planes = 0; planes < 2; ++planes) for (int hh = 0; hh < 2; ++hh) for (int ff = 0; ff < 2; ++ff)
        for (size_t F : {(size_t)1, (size_t)3, (size_t)512}) for (size_t tf : {(size_t)0, (size_t)7, (size_t)40000}) for (size_t mt : {(size_t)1, (size_t)13, (size_t)80000}) {
            const FlatLargeWs w = flat_large_ws(F, tf, mt, planes, hh, ff);
            const size_t plane = planes ? 8 * ((tf + 1) & ~(size_t)1) : 0, rows = F * mt;
            const size_t end = audit("ws", {{"x", w.x, plane, 8, 1u}, {"y", w.y, plane, 8, 1u}, {"z", w.z, plane, 8, 1u},
                                            {"heights", w.heights, hh ? 8 * rows : 0, 8, 1u}, {"list", w.list, 12 * rows, 4, 1u},
                                            {"flags", w.flags, ff ? rows : 0, 1, 1u}});
            CHECK(end <= w.total, "ws F %zu total_feat %zu max_tri %zu", F, tf, mt);
        }
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "flat")) { printf("%zu\n", flat_large_plan<size_t>((size_t)atoll(argv[2])).total); return 0; }
    if (argc == 4 && !strcmp(argv[1], "graph")) {
        printf("%zu\n", graph_large_plan<size_t>((size_t)graph_large_tile<long long>(atoll(argv[2]), atoll(argv[3]))).total);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "plans")) plans();
    else return 2;
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rescale_large_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_plans_are_aligned_disjoint_and_bounded(plan_exe):
    assert _run(plan_exe, "plans").strip() == "0 failed"


def test_lds_does_not_grow_with_the_frame(plan_exe):
    """The flat kernel's request depends on n_hyp alone — the plan takes no frame size —, the vote's on the tile, which stops at
    8192 vertices whatever max_feat says: 20 000- and 2 000 000 000-feature headers ask for the same bytes."""
    flat = [int(_run(plan_exe, "flat", str(h))) for h in (1, 100, 512)]
    assert flat == sorted(flat) and flat[-1] <= 160 * 1024
    assert abs((flat[-1] - flat[0]) - 36 * 511) < 16                   # a plane and a count per hypothesis (and the total's rounding to 16)
    g = [int(_run(plan_exe, "graph", "0", str(mf))) for mf in (8192, 20000, 32000, 2000000000)]
    assert len(set(g)) == 1 and g[0] <= 160 * 1024
    assert int(_run(plan_exe, "graph", "64", "20000")) < int(_run(plan_exe, "graph", "100", "20000")) < g[0]


def test_entry_points_are_declared_and_bound():
    from mvoscalerecovery_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvosr.h")).read()
    lib = _lib.load()
    for name in ("mvosr_graph_keep_large_batch", "mvosr_flat_ransac_large_batch"):
        assert "int %s(mvosr_ctx *ctx, const mvosr_batch *b," % name in header
        assert hasattr(lib, name)
    # the large flat entry point takes mvosr_flat_ransac_batch's parameter list; the vote's has the tile behind the resident one's
    assert getattr(lib, "mvosr_flat_ransac_large_batch").argtypes == getattr(lib, "mvosr_flat_ransac_batch").argtypes
    assert getattr(lib, "mvosr_graph_keep_large_batch").argtypes[:-1] == getattr(lib, "mvosr_graph_keep_batch").argtypes
    assert _lib.ABI_VERSION == 13 and "#define MVOSR_ABI_VERSION 13" in header            # additive: the number stays
    src = open(os.path.join(CSRC, "Makefile")).read()
    assert "mvosr_rescale_large.hip" in src and "mvosr_rescale_large_plan.hpp" in src


def test_null_arguments_are_refused_before_any_device_work():
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    assert lib.mvosr_graph_keep_large_batch(None, None, 0, 10, None, None, None, None, 0) != 0
    assert lib.mvosr_flat_ransac_large_batch(None, None, None, None, None, None, None, None, 0) != 0


# ---- routing -------------------------------------------------------------------------------------------------------------------
def test_chunk_routing_is_by_the_chunks_largest_frame():
    from mvoscalerecovery_amd.rescale import chunk_goes_large
    cap = 3400
    assert not chunk_goes_large([], cap)
    assert not chunk_goes_large([1, 3400, 20], cap)                   # the limit itself is resident
    assert chunk_goes_large([1, 3401, 20], cap)                       # one frame beyond it: the whole chunk
    assert chunk_goes_large([np.int32(20000)], cap)


def test_stream_is_cut_into_size_classes():
    from mvoscalerecovery_amd.rescale import size_class_runs
    cap, limit = 3400, 32000
    assert size_class_runs([], cap, limit) == ([], None)
    assert size_class_runs([600] * 5, cap, limit) == ([(0, 5, False)], None)
    assert size_class_runs([600, 3400, 3401, 20000, 700, 32000, 5], cap, limit) == ([(0, 2, False), (2, 4, True), (4, 5, False), (5, 6, True), (6, 7, False)], None)
    # the call ends before the first frame beyond the opt-in limit, whatever follows it
    runs, stop = size_class_runs([600, 5000, 32001, 600, 40000], cap, limit)
    assert (runs, stop) == ([(0, 1, False), (1, 2, True)], 2)
    assert size_class_runs([32001, 5], cap, limit) == ([], 0)
    # every frame is in exactly one run, in order, and a run's class is its frames'
    rng = np.random.default_rng(4)
    sizes = rng.choice([100, 3400, 3401, 9000], 200)
    runs, stop = size_class_runs(sizes, cap, limit)
    assert stop is None and [a for a, _, _ in runs] == [0] + [b for _, b, _ in runs[:-1]] and runs[-1][1] == 200
    for a, b, large in runs:
        assert np.all((sizes[a:b] > cap) == large)
    assert all(x[2] != y[2] for x, y in zip(runs, runs[1:]))          # maximal: neighbours differ


def test_host_chunks_of_large_runs_are_cut_by_points():
    from mvoscalerecovery_amd.rescale import host_chunks
    assert host_chunks([], 2048) == [] and host_chunks([], 2048, 10) == []
    assert host_chunks([2000] * 5000, 2048) == [(0, 2048), (2048, 4096), (4096, 5000)]          # without a cap: the step alone
    assert host_chunks([20000] * 5000, 2048) == [(0, 2048), (2048, 4096), (4096, 5000)]
    chunks = host_chunks([20000] * 5000, 2048, 10_000_000)
    assert chunks[0] == (0, 500) and chunks[-1][1] == 5000 and all(b - a <= 500 for a, b in chunks)
    assert [a for a, _ in chunks[1:]] == [b for _, b in chunks[:-1]]
    # one large frame among small ones: frames x largest frame stays within twice the points; a frame beyond the cap goes alone
    sizes = [100] * 300 + [30000] + [100] * 300
    for a, b in host_chunks(sizes, 2048, 1_000_000):
        assert sum(sizes[a:b]) <= 1_000_000 and (b - a) * max(sizes[a:b]) <= 2_000_000
    assert host_chunks([50, 5000, 50], 2048, 1000) == [(0, 1), (1, 2), (2, 3)]


def test_large_frames_keyword_needs_no_device_to_be_refused():
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    for bad in (1, 0, "yes", None):
        with pytest.raises(TypeError, match="large_frames"):
            ScaleEstimator(1.75, large_frames=bad)
    for kw in ({"sampling": "host"}, {"triangulation": "scipy"}, {"sampler": lambda n: None}, {"triangulation": "scipy", "sampling": "host"}):
        with pytest.raises(ValueError, match="large_frames=True belongs to the device-resident path"):
            ScaleEstimator(1.75, large_frames=True, **kw)
    import inspect
    assert inspect.signature(ScaleEstimator.__init__).parameters["large_frames"].default is False


def test_limits_with_and_without_the_opt_in(monkeypatch):
    """_max_points() keeps its meaning; the opt-in limit is the triangulators'; the error names whichever applies."""
    from mvoscalerecovery_amd import packing
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    monkeypatch.setattr(packing, "delaunay_gpu_max_points", lambda: 32000)
    ctx = types.SimpleNamespace(lds_per_block=163840, lib=types.SimpleNamespace(mvosr_delaunay_lds_points=lambda: 4744))
    for large in (False, True):
        est = types.SimpleNamespace(N_HYP=100, ctx=ctx, large_frames=large)
        est._max_points = lambda: ScaleEstimator._max_points(est)
        est._large_max_points = lambda: ScaleEstimator._large_max_points(est)
        est._frame_limit = lambda: ScaleEstimator._frame_limit(est)
        assert est._max_points() == (163840 - 14000 - 3600) // 43 == 3400
        assert est._frame_limit() == (32000 if large else 3400)
        old = str(ScaleEstimator._oversized_error(est, 3, 5000))
        assert "frame 3 has 5000 features" in old and "at most 3400 per frame (one workgroup's LDS)" in old
        new = str(ScaleEstimator._oversized_error(est, 3, 40000, 32000))
        assert "frame 3 has 40000 features" in new and "at most 32000 per frame with large_frames=True" in new
