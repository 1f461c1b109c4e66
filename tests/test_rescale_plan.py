"""CPU: the LDS plans of the rescale-variant kernels (csrc/mvosr_rescale_plan.hpp), compiled with g++ into a stand-alone program.

* every plan's ``total`` is the byte count the launchers asked for before the plans existed (the formulas below restate those
  launchers, slack included): the MVOSR_ERR_TOO_LARGE thresholds have not moved;
* a frame the kernels accept (n <= max_feat, tn <= max_tri) lies inside what its launch requested, late aliases at their largest
  admissible extent included; regions that are live together do not overlap; every offset has its type's alignment; the kernels'
  32-bit plans are the launchers' size_t plans;
* the cap rescale.py puts on a frame's points keeps flat_plan within the device's LDS.
"""
import os
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mvosr_rescale_plan.hpp"
using namespace mvosr;

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- what the launchers requested before the plans (48 = FM_N, 2048 = kFlatBins, 36 = a plane + its count, 8 = kRsWaves,
// 32 + 256 = GM_N + kGrowBins)
static size_t even(long long n) { return (size_t)((n + 1) & ~1ll); }
static size_t old_graph(long long mf) { return 16u * even(mf) + 4u * ((size_t)mf + 4) + 16; }
static size_t old_flat_dev(long long mf, long long mt, long long h) {
    return 8u * (size_t)mt + 32 + 4u * 48 + 24u * even(mf) + 4u * 2048 + (size_t)mt + 32 + 36u * (size_t)h + 16;
}
static size_t old_flat_stage(long long mf, long long mt) {
    size_t lds = 24u * even(mf);
    if (lds < 4u * 2048) lds = 4u * 2048;
    return lds + 9u * (size_t)mt + 32 + 4u * 48 + 16;
}
static size_t old_tribatch(long long mf) { return 24u * even(mf) + 8u * 3 * 2 * 8 + 32; }
static size_t old_ransac(long long h) { return 36u * (size_t)h + 16; }
static size_t old_grow_work(bool pts, long long mf, long long mt) {
    const size_t table = (12u * (size_t)mt + 4u * ((size_t)mf + 2) + 7u) & ~(size_t)7;
    const size_t planes = pts ? 24u * even(mf) : 0u;
    return table > planes ? table : planes;
}
static size_t old_grow(bool pts, long long mf, long long mt) {
    return 16u * (size_t)mt + 64u + old_grow_work(pts, mf, mt) + 4u * (32 + 256) + ((6u * (size_t)mt + 15u) & ~(size_t)15);
}

static const int kSmallFeat = 70, kSmallTri = 140;
static const long long kHyps[4] = {1, 7, 100, 512};

static std::vector<long long> feats() {
    std::vector<long long> v;
    for (int i = 0; i <= kSmallFeat; ++i) v.push_back(i);
    for (long long x : {255ll, 256ll, 2000ll, 2001ll, 8000ll, 65535ll}) v.push_back(x);
    return v;
}
static std::vector<long long> tris(long long mf) {
    std::vector<long long> v;
    for (int i = 0; i <= kSmallTri; ++i) v.push_back(i);
    for (long long x : {2 * mf, 21845ll, 65534ll}) v.push_back(x);
    return v;
}

static void totals() {
    for (long long h : kHyps) CHECK(ransac_plan<size_t>(h).total == old_ransac(h), "n_hyp %lld", h);
    for (long long mf : feats()) {
        CHECK(graph_plan<size_t>(mf).total == old_graph(mf), "max_feat %lld", mf);
        CHECK(tribatch_plan<size_t>(mf).total == old_tribatch(mf), "max_feat %lld", mf);
        for (long long mt : tris(mf)) {
            CHECK(flat_plan<size_t>(false, mf, mt, 0).total == old_flat_stage(mf, mt), "max_feat %lld max_tri %lld", mf, mt);
            for (long long h : kHyps)
                CHECK(flat_plan<size_t>(true, mf, mt, h).total == old_flat_dev(mf, mt, h), "max_feat %lld max_tri %lld n_hyp %lld", mf, mt, h);
            const long long gt = mt < 1 ? 1 : mt;                   // mvosr_region_grow_batch raises max_tri to at least 1
            for (int pts = 0; pts < 2; ++pts)
                CHECK(grow_plan<size_t>(pts, mf, gt).total == old_grow(pts, mf, gt), "pts %d max_feat %lld max_tri %lld", pts, mf, gt);
        }
    }
}

// ---- a plan's regions: where, how long, the alignment the type needs, and the phases (bits) in which they are live
struct Region { const char *name; size_t off, bytes, align; unsigned live; };
// every region aligned, no two that are live together overlapping; returns the largest end
static size_t audit(const char *plan, const std::vector<Region> &r, long long n, long long tn, long long h) {
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % r[i].align == 0, "%s.%s at %zu needs %zu (n %lld tn %lld n_hyp %lld)", plan, r[i].name, r[i].off, r[i].align, n, tn, h);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j) {
            if (!(r[i].live & r[j].live) || !r[i].bytes || !r[j].bytes) continue;
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s.%s overlaps %s (n %lld tn %lld n_hyp %lld)",
                  plan, r[i].name, r[j].name, n, tn, h);
        }
    }
    return end;
}
#define SAME32(f) CHECK((size_t)p.f == q.f, "32-bit and size_t plans differ at " #f)

// flat_selection_kernel: phase 1 up to the selection, phase 2 (dev) the RANSAC tail with the list and the distinct vertices,
// phase 4 (dev) the tail with the packed vertices; stage form: phase 1 the normals, phase 2 the median search
static size_t flat_end(bool dev, long long n, long long tn, long long h, int block) {
    const FlatPlan<uint32_t> p = flat_plan<uint32_t>(dev, n, tn, h);
    const FlatPlan<size_t> q = flat_plan<size_t>(dev, n, tn, h);
    SAME32(heights); SAME32(ext); SAME32(misc); SAME32(x); SAME32(y); SAME32(z); SAME32(hist); SAME32(flags); SAME32(mods); SAME32(cnts);
    SAME32(total); SAME32(heights_bytes); SAME32(hist_bytes); SAME32(list); SAME32(w2); SAME32(packed);
    const size_t plane = 8u * (size_t)n;
    std::vector<Region> r = {
        {"heights", q.heights, 8u * (size_t)tn, 8, 1u}, {"ext", q.ext, 32, 8, 7u}, {"misc", q.misc, 4u * FM_N, 4, 7u},
        {"flags", q.flags, (size_t)tn, 1, 7u}};
    CHECK(q.heights_bytes == 8u * (size_t)tn && q.hist_bytes == 4u * kFlatBins, "region sizes");
    if (!dev) {
        r.push_back({"x", q.x, plane, 8, 1u}); r.push_back({"y", q.y, plane, 8, 1u}); r.push_back({"z", q.z, plane, 8, 1u});
        r.push_back({"hist", q.hist, q.hist_bytes, 8, 2u});
        r[0].live = 3u;                                             // (the heights are compared after the search)
        return audit("flat(stage)", r, n, tn, 0);
    }
    r.push_back({"x", q.x, plane, 8, 7u}); r.push_back({"y", q.y, plane, 8, 7u}); r.push_back({"z", q.z, plane, 8, 7u});
    r.push_back({"hist", q.hist, q.hist_bytes, 8, 1u});
    r.push_back({"mods", q.mods, (size_t)kPlaneBytes * (size_t)h, 16, 7u}); r.push_back({"cnts", q.cnts, 4u * (size_t)h, 4, 7u});
    // the point list at its longest: every row kept
    const size_t M = 3u * (size_t)tn;
    r.push_back({"list", q.list, 2u * M, 2, 2u});
    CHECK(q.list + 2u * M <= q.heights + q.heights_bytes, "list leaves the heights' room (tn %lld)", tn);
    // the distinct vertices behind the longest list the kernel's `dedup` admits, with the multiplicities over the histogram
    for (long long K = tn; K >= 0; --K) {
        const size_t m = 3u * (size_t)K, me = (m + 1) & ~(size_t)1;
        if (!(2 * me + 2 * (size_t)n <= q.heights_bytes && n <= 2 * kFlatBins - 2)) continue;
        r.back().bytes = 2u * m;
        r.push_back({"distinct", q.list + 2u * me, 2u * (size_t)n, 2, 2u});
        r.push_back({"w2", q.w2, 4u * ((size_t)(n + 1) / 2 + 1), 4, 6u});
        CHECK(q.list + 2u * me + 2u * (size_t)n <= q.heights + q.heights_bytes, "distinct vertices leave the heights' room");
        CHECK(4u * ((size_t)(n + 1) / 2 + 1) <= q.hist_bytes, "multiplicities leave the histogram's room");
        // ... and the packed vertices at the largest count the kernel's `packed` admits
        long long items = n < 2 * block ? n : 2 * block;
        while (items > 0 && !(28 * (size_t)items + 8 <= q.heights_bytes)) --items;
        if (items > 0) {
            const size_t a = 8u * (size_t)items;
            r.push_back({"px", q.packed, a, 8, 4u}); r.push_back({"py", q.packed + a, a, 8, 4u}); r.push_back({"pz", q.packed + 2 * a, a, 8, 4u});
            r.push_back({"pw", q.packed + 3 * a, 4u * (size_t)items, 4, 4u});
            CHECK(q.packed + 3 * a + 4u * (size_t)items <= q.heights + q.heights_bytes, "packed vertices leave the heights' room");
        }
        break;
    }
    return audit("flat(dev)", r, n, tn, h);
}

static size_t graph_end(long long n) {
    const GraphPlan<uint32_t> p = graph_plan<uint32_t>(n);
    const GraphPlan<size_t> q = graph_plan<size_t>(n);
    SAME32(p); SAME32(cnt); SAME32(flag); SAME32(total);
    return audit("graph", {{"p", q.p, 16u * (size_t)n, 16, 1u}, {"cnt", q.cnt, 4u * (size_t)n, 4, 1u}, {"flag", q.flag, 8, 4, 1u}}, n, 0, 0);
}
static size_t tribatch_end(long long n) {
    const TriBatchPlan<uint32_t> p = tribatch_plan<uint32_t>(n);
    const TriBatchPlan<size_t> q = tribatch_plan<size_t>(n);
    SAME32(x); SAME32(y); SAME32(z); SAME32(red); SAME32(flag); SAME32(total);
    const size_t plane = 8u * (size_t)n;
    return audit("tribatch", {{"x", q.x, plane, 8, 1u}, {"y", q.y, plane, 8, 1u}, {"z", q.z, plane, 8, 1u},
                              {"red", q.red, 8u * 3 * 2 * kRsWaves, 8, 1u}, {"flag", q.flag, 8, 4, 1u}}, n, 0, 0);
}
// region_grow_kernel carves at the header's sizes: phase 1 the vertex planes (pts), 2 the table, 4 the labels
static size_t grow_end(bool pts, long long mf, long long mt) {
    const GrowPlan<uint32_t> p = grow_plan<uint32_t>(pts, mf, mt);
    const GrowPlan<size_t> q = grow_plan<size_t>(pts, mf, mt);
    SAME32(hinv); SAME32(ang); SAME32(ext); SAME32(work); SAME32(misc); SAME32(hist); SAME32(nb); SAME32(total); SAME32(work_bytes);
    SAME32(x); SAME32(y); SAME32(z); SAME32(r16); SAME32(inc); SAME32(start); SAME32(label);
    const size_t T = (size_t)mt, plane = 8u * (size_t)mf;
    std::vector<Region> r = {
        {"hinv", q.hinv, 8u * T, 8, 7u}, {"ang", q.ang, 8u * T, 8, 7u}, {"ext", q.ext, 64, 8, 7u}, {"misc", q.misc, 4u * GM_N, 4, 7u},
        {"hist", q.hist, 4u * kGrowBins, 4, 7u}, {"nb", q.nb, 6u * T, 2, 7u},
        {"r16", q.r16, 6u * T, 2, 2u}, {"inc", q.inc, 6u * T, 2, 2u}, {"start", q.start, 4u * ((size_t)mf + 1), 4, 2u},
        {"label", q.label, 8u * T, 4, 4u}};
    if (pts) { r.push_back({"x", q.x, plane, 8, 1u}); r.push_back({"y", q.y, plane, 8, 1u}); r.push_back({"z", q.z, plane, 8, 1u}); }
    for (size_t i = 6; i < r.size(); ++i)
        CHECK(r[i].off >= q.work && r[i].off + r[i].bytes <= q.work + q.work_bytes, "grow.%s leaves the work area (max_feat %lld max_tri %lld)", r[i].name, mf, mt);
    return audit(pts ? "grow(pts)" : "grow", r, mf, mt, 0);
}

static void containment() {
    const int NF = kSmallFeat + 1, NT = kSmallTri + 1;
    std::vector<size_t> end((size_t)NF * NT), total((size_t)NF * NT);
    // per-frame plans: a frame's largest end against the request of every header that admits the frame
    for (int form = 0; form < 5; ++form) {                           // stage, then the device-resident form at each n_hyp
        const bool dev = form > 0;
        const long long h = dev ? kHyps[form - 1] : 0;
        for (int n = 0; n < NF; ++n)
            for (int tn = 0; tn < NT; ++tn) {
                end[(size_t)n * NT + tn] = flat_end(dev, n, tn, h, dev ? 1024 : 512);
                total[(size_t)n * NT + tn] = flat_plan<size_t>(dev, n, tn, h).total;
            }
        for (int mf = 0; mf < NF; ++mf)
            for (int mt = 0; mt < NT; ++mt)
                for (int n = 0; n <= mf; ++n)
                    for (int tn = 0; tn <= mt; ++tn)
                        if (end[(size_t)n * NT + tn] > total[(size_t)mf * NT + mt]) {
                            CHECK(false, "flat form %d: frame (%d, %d) ends at %zu, header (%d, %d) asked for %zu", form, n, tn,
                                  end[(size_t)n * NT + tn], mf, mt, total[(size_t)mf * NT + mt]);
                        }
    }
    for (int mf = 0; mf < NF; ++mf)
        for (int n = 0; n <= mf; ++n) {
            CHECK(graph_end(n) <= graph_plan<size_t>(mf).total, "graph: frame %d, header %d", n, mf);
            CHECK(tribatch_end(n) <= tribatch_plan<size_t>(mf).total, "tribatch: frame %d, header %d", n, mf);
        }
    // carved at the header's sizes: the plan's own end against its total
    for (int pts = 0; pts < 2; ++pts)
        for (int mf = 0; mf < NF; ++mf)
            for (int mt = 1; mt < NT; ++mt)
                CHECK(grow_end(pts, mf, mt) <= grow_plan<size_t>(pts, mf, mt).total, "grow: pts %d header (%d, %d)", pts, mf, mt);
    for (long long h = 1; h <= 512; ++h) {
        const RansacPlan<size_t> q = ransac_plan<size_t>(h);
        const RansacPlan<uint32_t> p = ransac_plan<uint32_t>(h);
        SAME32(mods); SAME32(cnts); SAME32(total);
        CHECK(audit("ransac", {{"mods", q.mods, (size_t)kPlaneBytes * (size_t)h, 16, 1u}, {"cnts", q.cnts, 4u * (size_t)h, 4, 1u}}, 0, 0, h) <= q.total,
              "ransac: n_hyp %lld", h);
    }
    // the largest frame whose multiplicities `dedup` puts over the histogram
    CHECK(4u * ((size_t)(2 * kFlatBins - 2 + 1) / 2 + 1) <= flat_plan<size_t>(true, 2 * kFlatBins - 2, 1, 1).hist_bytes, "w2 at the dedup cap");
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "flat")) {                     // flat <max_feat> <n_hyp>: the device-resident request at max_tri = 2 max_feat
        const long long mf = atoll(argv[2]);
        printf("%zu\n", flat_plan<size_t>(true, mf, 2 * mf, atoll(argv[3])).total);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "totals")) totals();
    else if (argc == 2 && !strcmp(argv[1], "containment")) containment();
    else return 2;
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rescale_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_totals_are_the_launchers_old_formulas(plan_exe):
    assert _run(plan_exe, "totals").strip() == "0 failed"


def test_accepted_frames_lie_inside_the_request_aligned_and_disjoint(plan_exe):
    assert _run(plan_exe, "containment").strip() == "0 failed"


@pytest.mark.parametrize("lds_per_block", [65536, 163840])
def test_python_cap_keeps_flat_plan_within_the_lds(plan_exe, lds_per_block, monkeypatch):
    from mvoscalerecovery_amd import packing
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    huge = 1 << 30                                                    # (the two Delaunay caps out of the way: the LDS term decides)
    monkeypatch.setattr(packing, "delaunay_gpu_max_points", lambda: huge)
    est = types.SimpleNamespace(N_HYP=ScaleEstimator.N_HYP,
                                ctx=types.SimpleNamespace(lds_per_block=lds_per_block, lib=types.SimpleNamespace(mvosr_delaunay_lds_points=lambda: huge)))
    cap = ScaleEstimator._max_points(est)
    assert 0 < cap < huge
    assert int(_run(plan_exe, "flat", str(cap), str(ScaleEstimator.N_HYP))) <= lds_per_block
