"""CPU: what surrounds flat_static_tri_kernel (csrc/mvosr_rescale_static.hip) and needs no device.

* the C ABI: include/mvosr.h declares the struct and both functions, _lib.SYMBOLS binds them with matching arity, the ABI version
  has not moved, the Makefile builds the file;
* the LDS plan (csrc/mvosr_rescale_static_plan.hpp), compiled with g++ into a stand-alone program as tests/test_rescale_plan.py does:
  it grows with its sizes, every offset is aligned, regions that are live together do not overlap, an accepted frame lies inside
  the request, every frame mvosr_flat_ransac_batch's request admits is admitted, and the frame limit of rescale.py fits 160 KiB;
* every constructor rule of ``ScaleEstimator(model_resident=...)`` with the device and the worker pool out of reach, and that the
  constructor without the keyword resolves as before;
* ``RepeatedRuns`` and ``ConstantSweep`` refuse a model that is not the RANSAC plane.
"""
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mvosr.h")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _header():
    with open(HEADER) as f:
        return f.read()


def _declaration(name):
    m = re.search(r"^(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, _header(), re.M | re.S)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_header_declares_the_struct_and_both_functions():
    h = _header()
    assert re.search(r"#define\s+MVOSR_ABI_VERSION\s+13\b", h)
    m = re.search(r"typedef struct mvosr_static_tri_outputs\s*\{(.*?)\}\s*mvosr_static_tri_outputs;", h, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == ["scale_norm", "raw_scale", "height_level", "n_used", "n_kept", "status", "hist", "tri_height", "tri_flags"]
    args = _declaration("mvosr_flat_static_tri_batch")
    assert len(args) == 13 and args[0] == "mvosr_ctx *ctx" and args[-1] == "int64_t max_tri"
    assert "const mvosr_static_tri_outputs *o" in args and "const double *tri_height_in" in args and "const uint8_t *tri_flags_in" in args
    assert _declaration("mvosr_flat_static_tri_lds_bytes") == ["int max_feat", "int64_t max_tri"]


def test_lib_binds_them_with_matching_arity():
    import ctypes as C
    from mvoscalerecovery_amd import _lib
    assert _lib.ABI_VERSION == 13
    res, args = _lib.SYMBOLS["mvosr_flat_static_tri_batch"]
    assert res is C.c_int and len(args) == len(_declaration("mvosr_flat_static_tri_batch"))
    assert args[1] is C.POINTER(_lib.Batch) and args[11] is C.POINTER(_lib.StaticTriOutputs) and args[12] is C.c_int64
    assert [a for a in args[3:8]] == [C.c_double, C.c_double, C.c_double, C.c_int32, C.c_double]
    res, args = _lib.SYMBOLS["mvosr_flat_static_tri_lds_bytes"]
    assert res is C.c_size_t and args == [C.c_int, C.c_int64]
    assert [n for n, _ in _lib.StaticTriOutputs._fields_] == ["scale_norm", "raw_scale", "height_level", "n_used", "n_kept", "status",
                                                              "hist", "tri_height", "tri_flags"]
    assert all(t is C.c_void_p for _, t in _lib.StaticTriOutputs._fields_)


def test_makefile_builds_the_new_file():
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "mvosr_rescale_static.hip" in srcs and "mvosr_rescale_static_plan.hpp" in hdrs
    assert "-ffp-contract=off" in mk
    assert os.path.exists(os.path.join(CSRC, "mvosr_rescale_static.hip"))


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mvosr_rescale_plan.hpp"
#include "mvosr_rescale_static_plan.hpp"
using namespace mvosr;

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
#define SAME32(f) CHECK((size_t)p.f == q.f, "32-bit and size_t plans differ at " #f)

struct Region { const char *name; size_t off, bytes, align; unsigned live; };

// phase 1: the planes are read, heights and flags written; phase 2: the median search (histogram, then the candidate list);
// phase 4: the road model's sweep and the decision.  Returns the largest end.
static size_t static_end(long long n, long long tn) {
    const StaticPlan<uint32_t> p = static_plan<uint32_t>((uint32_t)n, (uint32_t)tn);
    const StaticPlan<size_t> q = static_plan<size_t>((size_t)n, (size_t)tn);
    SAME32(heights); SAME32(flags); SAME32(ext); SAME32(misc); SAME32(model); SAME32(work); SAME32(total); SAME32(work_bytes);
    SAME32(x); SAME32(y); SAME32(z); SAME32(hist);
    const size_t plane = 8u * (size_t)n;
    std::vector<Region> r = {
        {"heights", q.heights, 8u * (size_t)tn, 8, 7u}, {"flags", q.flags, (size_t)tn, 1, 7u}, {"ext", q.ext, 32, 8, 7u},
        {"misc", q.misc, 4u * FM_N, 4, 7u}, {"model", q.model, 4u * 32, 4, 7u},
        {"x", q.x, plane, 8, 1u}, {"y", q.y, plane, 8, 1u}, {"z", q.z, plane, 8, 1u},
        {"hist", q.hist, 4u * kFlatBins, 8, 2u}, {"list", q.hist, 8u * kFlatDirect, 8, 2u}};
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % r[i].align == 0, "%s at %zu needs %zu (n %lld tn %lld)", r[i].name, r[i].off, r[i].align, n, tn);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j) {
            if (!(r[i].live & r[j].live) || !r[i].bytes || !r[j].bytes) continue;
            if (!strcmp(r[i].name, "list") && !strcmp(r[j].name, "hist")) continue;      // (the list takes the histogram's room on purpose)
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s overlaps %s (n %lld tn %lld)", r[i].name, r[j].name, n, tn);
        }
    }
    for (size_t i = 5; i < r.size(); ++i)
        CHECK(r[i].off >= q.work && r[i].off + r[i].bytes <= q.work + q.work_bytes, "%s leaves the work area (n %lld tn %lld)", r[i].name, n, tn);
    // every offset the plan names is a multiple of 16
    for (size_t o : {q.heights, q.flags, q.ext, q.misc, q.model, q.work, q.x, q.hist, q.total})
        CHECK(o % 16 == 0, "offset %zu is no multiple of 16 (n %lld tn %lld)", o, n, tn);
    CHECK(q.y % 8 == 0 && q.z % 8 == 0, "planes");
    CHECK(FM_CW + kStaticWaves <= FM_N && FM_WSUM + kStaticWaves <= FM_CW && kStaticModelBins <= 32 && kFlatDirect * 8 <= kFlatBins * 4, "slots");
    return end;
}

static void properties() {
    const int NF = 71, NT = 141;
    std::vector<size_t> end((size_t)NF * NT), total((size_t)NF * NT);
    for (int n = 0; n < NF; ++n)
        for (int tn = 0; tn < NT; ++tn) {
            end[(size_t)n * NT + tn] = static_end(n, tn);
            total[(size_t)n * NT + tn] = static_plan<size_t>(n, tn).total;
            CHECK(end[(size_t)n * NT + tn] <= total[(size_t)n * NT + tn], "plan (%d, %d) ends behind its total", n, tn);
        }
    // the plan grows with its sizes, offset by offset ...
    for (int n = 0; n + 1 < NF; ++n)
        for (int tn = 0; tn + 1 < NT; ++tn) {
            const StaticPlan<size_t> a = static_plan<size_t>(n, tn), b = static_plan<size_t>(n + 1, tn), c = static_plan<size_t>(n, tn + 1);
            for (const StaticPlan<size_t> &g : {b, c})
                CHECK(g.heights >= a.heights && g.flags >= a.flags && g.ext >= a.ext && g.misc >= a.misc && g.model >= a.model && g.work >= a.work &&
                      g.x >= a.x && g.y >= a.y && g.z >= a.z && g.hist >= a.hist && g.total >= a.total && g.work_bytes >= a.work_bytes,
                      "not monotone at (%d, %d)", n, tn);
        }
    // ... so a frame the kernel accepts lies inside what every header that admits it asked for
    for (int mf = 0; mf < NF; ++mf)
        for (int mt = 0; mt < NT; ++mt)
            for (int n = 0; n <= mf; ++n)
                for (int tn = 0; tn <= mt; ++tn)
                    if (end[(size_t)n * NT + tn] > total[(size_t)mf * NT + mt])
                        CHECK(false, "frame (%d, %d) ends at %zu, header (%d, %d) asked for %zu", n, tn, end[(size_t)n * NT + tn], mf, mt, total[(size_t)mf * NT + mt]);
    for (long long n : {255ll, 256ll, 341ll, 342ll, 2000ll, 2001ll, 3480ll, 8000ll, 65535ll})
        for (long long tn : {1ll, n, 2 * n - 5, 2 * n}) {
            CHECK(static_end(n, tn) <= static_plan<size_t>(n, tn).total, "plan (%lld, %lld)", n, tn);
        }
    // the launch accepts every frame mvosr_flat_ransac_batch accepts: from the size at which the planes outgrow the histogram
    // (342 features) it asks for less LDS than that one does with a single hypothesis, and below it for less than 64 KiB
    for (long long n = 0; n <= 4200; n += 7)
        for (long long tn : {1ll, n, 2 * n}) {
            const size_t mine = static_plan<size_t>(n, tn).total, theirs = flat_plan<size_t>(true, n, tn, 1).total;
            CHECK(n >= 342 ? mine <= theirs : mine <= 65536, "(%lld, %lld): %zu against %zu", n, tn, mine, theirs);
        }
    // the given form: nothing row-sized
    CHECK(static_plan<size_t>(0, 0).total == 32 + 4u * FM_N + 128 + 4u * kFlatBins, "the plan at (0, 0): %zu", static_plan<size_t>(0, 0).total);
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "static")) { printf("%zu\n", static_plan<size_t>(atoll(argv[2]), atoll(argv[3])).total); return 0; }
    if (argc == 2 && !strcmp(argv[1], "properties")) properties();
    else return 2;
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("static_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)     # (plain C++: no HIP)
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_plan_grows_is_aligned_and_its_live_regions_are_disjoint(plan_exe):
    assert _run(plan_exe, "properties").strip() == "0 failed"


@pytest.mark.parametrize("lds_per_block", [65536, 163840])
def test_the_frame_limit_fits_the_lds(plan_exe, lds_per_block, monkeypatch):
    from mvoscalerecovery_amd import packing
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    huge = 1 << 30                                                    # (the two Delaunay caps out of the way: the LDS term decides)
    monkeypatch.setattr(packing, "delaunay_gpu_max_points", lambda: huge)
    est = types.SimpleNamespace(N_HYP=ScaleEstimator.N_HYP,
                                ctx=types.SimpleNamespace(lds_per_block=lds_per_block, lib=types.SimpleNamespace(mvosr_delaunay_lds_points=lambda: huge)))
    cap = ScaleEstimator._max_points(est)
    assert 0 < cap < huge
    assert int(_run(plan_exe, "static", str(cap), str(2 * cap))) <= lds_per_block
    if lds_per_block == 163840:
        assert int(_run(plan_exe, "static", str(cap), str(2 * cap))) <= 160 * 1024


# ---- the constructor -----------------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """ScaleEngine and the worker pool raise: a refusal that passes here needs neither."""
    from mvoscalerecovery_amd import packing, rescale

    def fail(*a, **k):
        raise _Reached("the constructor asked for a device or the pool")
    monkeypatch.setattr(rescale, "ScaleEngine", fail)
    monkeypatch.setattr(packing, "start_pool", fail)
    monkeypatch.delenv("MVOSR_TRIANGULATION", raising=False)
    return rescale


def _accepted(rescale, **kw):
    """The constructor's resolved (triangulation, sampling, model, model_resident): it ran up to the point where it asks for the
    pool or the device (stopped there), every refusal behind it."""
    seen = {}

    class Probe(rescale.ScaleEstimator):
        def __setattr__(self, k, v):
            seen[k] = v
            object.__setattr__(self, k, v)
    with pytest.raises(_Reached):
        Probe(1.75, 5, **kw)
    return seen["triangulation"], seen["sampling"], seen["model"], seen["model_resident"]


def test_model_resident_is_a_bool(no_device):
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(TypeError, match="model_resident"):
            no_device.ScaleEstimator(1.75, 5, model="static_tri", model_resident=bad)


@pytest.mark.parametrize("kw", [{}, {"model": "ransac"}, {"model": "static"}, {"model": "static", "triangulation": "gpu"}])
def test_model_resident_belongs_to_static_tri(no_device, kw):
    with pytest.raises(ValueError, match="model_resident=True belongs to model='static_tri'"):
        no_device.ScaleEstimator(1.75, 5, model_resident=True, **kw)


def test_model_resident_refuses_grow_large_frames_and_host_sampling(no_device):
    E = no_device.ScaleEstimator
    with pytest.raises(ValueError, match="model_resident=True belongs to .*region='threshold'"):
        E(1.75, 5, model="static_tri", model_resident=True, region="grow")
    with pytest.raises(ValueError, match="model_resident=True belongs to .*large_frames=True keeps the staged path"):
        E(1.75, 5, model="static_tri", model_resident=True, large_frames=True)
    with pytest.raises(ValueError, match="model_resident=True belongs to the device-resident path"):
        E(1.75, 5, model="static_tri", model_resident=True, sampling="host")
    with pytest.raises(ValueError, match="model_resident=True belongs to the device-resident path"):
        E(1.75, 5, model="static_tri", model_resident=True, sampler=lambda m: None)
    with pytest.raises(ValueError, match="model_resident=True belongs to the device-resident path"):
        E(1.75, 5, model="static_tri", model_resident=True, triangulation="scipy")           # (resolves to host sampling, as for RANSAC)
    with pytest.raises(ValueError, match="triangulation must be"):
        E(1.75, 5, model="static_tri", model_resident=True, triangulation="cpu")


def test_model_resident_resolves_as_the_ransac_model(no_device, monkeypatch):
    assert _accepted(no_device, model="static_tri", model_resident=True) == ("gpu", "device", "static_tri", True)
    assert _accepted(no_device, model="static_tri", model_resident=True, triangulation="gpu") == ("gpu", "device", "static_tri", True)
    assert _accepted(no_device, model="static_tri", model_resident=True, triangulation="scipy", sampling="device") == \
        ("scipy", "device", "static_tri", True)
    assert _accepted(no_device, model="static_tri", model_resident=True, sampling="device") == ("gpu", "device", "static_tri", True)
    monkeypatch.setenv("MVOSR_TRIANGULATION", "scipy")
    assert _accepted(no_device, model="static_tri", model_resident=True, sampling="device") == ("scipy", "device", "static_tri", True)
    with pytest.raises(ValueError, match="model_resident=True belongs to the device-resident path"):
        no_device.ScaleEstimator(1.75, 5, model="static_tri", model_resident=True)           # (scipy -> host sampling, as for RANSAC)


def test_without_the_keyword_the_constructor_resolves_as_before(no_device, monkeypatch):
    assert _accepted(no_device) == ("gpu", "device", "ransac", False)
    assert _accepted(no_device, model_resident=False) == ("gpu", "device", "ransac", False)
    assert _accepted(no_device, triangulation="scipy") == ("scipy", "host", "ransac", False)
    assert _accepted(no_device, triangulation="scipy", sampling="device") == ("scipy", "device", "ransac", False)
    assert _accepted(no_device, sampler=lambda m: None) == ("scipy", "host", "ransac", False)
    assert _accepted(no_device, model="static_tri") == ("scipy", "host", "static_tri", False)
    assert _accepted(no_device, model="static_tri", model_resident=False, large_frames=True) == ("scipy", "host", "static_tri", False)
    assert _accepted(no_device, model="static") == ("scipy", "host", "static", False)
    assert _accepted(no_device, region="grow") == ("scipy", "host", "ransac", False)
    for kw in ({"model": "static_tri", "triangulation": "gpu"}, {"model": "static_tri", "sampling": "device"},
               {"model": "static_tri", "triangulation": "gpu", "model_resident": False}):
        with pytest.raises(ValueError, match="runs on the staged path"):
            no_device.ScaleEstimator(1.75, 5, **kw)
    with pytest.raises(ValueError, match="large_frames=True belongs to the device-resident path"):
        no_device.ScaleEstimator(1.75, 5, triangulation="scipy", large_frames=True)
    monkeypatch.setenv("MVOSR_TRIANGULATION", "scipy")
    assert _accepted(no_device) == ("scipy", "host", "ransac", False)


def test_repeated_runs_and_the_sweep_refuse_another_model(no_device):
    R = no_device
    for kw in ({"model": "static_tri", "model_resident": True}, {"model": "static_tri"}, {"model": "static"}):
        with pytest.raises(ValueError, match="RepeatedRuns repeats the RANSAC model"):
            R.RepeatedRuns(1.75, cases=2, seed=1, **kw)
        with pytest.raises(ValueError, match="ConstantSweep sweeps the RANSAC model"):
            R.ConstantSweep(1.75, [R.RescaleConstants()], cases=2, seed=1, **kw)
    with pytest.raises(_Reached):                                     # (the RANSAC model goes on to ask for its device)
        R.RepeatedRuns(1.75, cases=2, seed=1)
    with pytest.raises(_Reached):
        R.RepeatedRuns(1.75, cases=2, seed=1, model="ransac")
    # an estimator of another model handed in by a subclass is refused as well
    class Other(R.RepeatedRuns):
        @staticmethod
        def _make_estimator(absolute_reference, window_size, kw):
            return types.SimpleNamespace(model="static_tri", sampling="device", ctx=None)
    with pytest.raises(ValueError, match="RepeatedRuns repeats the RANSAC model, not model='static_tri'"):
        Other(1.75, cases=2, seed=1)
