"""CPU: the LDS plans of the scale kernels (csrc/mvosr_scale_plan.hpp), compiled with g++ into a stand-alone program.

* every plan's ``total`` is the byte count the launchers asked for before the header existed (the three formulas below restate
  them): mvosr_lds_bytes, mvosr_max_lds_features, pick_waves' 8/16 crossover and the tiled kernel's eligibility have not moved;
* every region has its type's alignment, regions that are live together do not overlap, the selected bit-set (and the words the
  LDS-resident kernels' tail may read) lies inside the vote counters' room;
* a frame the kernels accept (n <= max_feat) lies inside what its launch requested;
* the residencies DESIGN states (three LDS-resident workgroups of 2000 features, two tiled ones, per 160 KB) hold;
* the per-wave slot arrays of misc[] end inside every plan's misc.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
#include "mvosr_scale_plan.hpp"
using namespace mvosr;

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- what the launchers requested before the plan header (704 = the 176-int histogram, 96 = 6 reduction slots of 2 doubles
// per wavefront, 128 / 256 = 32 / 64 ints of misc, 1536 = 3 tiles of 512 vertices, 1024 / 576 = the pending lists' capacities)
static size_t a16(size_t v) { return (v + 15u) & ~(size_t)15; }
static size_t even(long long n) { return (size_t)((n + 1) & ~1ll); }
static size_t old_lds(long long n, int w) { return a16(24u * even(n) + 2u * even(n) + 16) + 704 + 96u * (size_t)w + 128; }
static size_t old_dense(long long n, int w) { return a16(2u * even(n) + 16) + a16(4u * (((size_t)n + 31) / 32)) + 96u * (size_t)w + 128; }
static size_t old_tiled(long long n, int w) {
    const size_t ntiles = ((size_t)n + 511) / 512;
    const size_t pend_v = a16(45u * 1536), pend_h = pend_v + 4u * 1024, toff = a16(pend_h + 12u * 576);
    return a16(toff + 8u * (ntiles + 2)) + 96u * (size_t)w + 256;
}

static const int kWavesList[4] = {1, 4, 8, 16};
static std::vector<long long> feats() {
    std::vector<long long> v;
    for (int i = 0; i <= 70; ++i) v.push_back(i);
    for (long long x : {255ll, 256ll, 320ll, 321ll, 1024ll, 1152ll, 2000ll, 2001ll, 2048ll, 3000ll}) v.push_back(x);
    for (long long x = 6000; x <= 6200; ++x) v.push_back(x);          // around mvosr_max_lds_features
    for (long long x : {8000ll, 20000ll, 65535ll}) v.push_back(x);
    return v;
}

static void totals() {
    for (long long n : feats())
        for (int w : kWavesList) {
            CHECK(lds_plan((int)n, w).total == old_lds(n, w), "lds n %lld waves %d", n, w);
            CHECK(dense_plan((int)n, w).total == old_dense(n, w), "dense n %lld waves %d", n, w);
            CHECK(tiled_plan((int)n, w).total == old_tiled(n, w), "tiled n %lld waves %d", n, w);
        }
    CHECK(3u * (size_t)lds_plan(2000, 8).total <= 160u * 1024, "three LDS-resident workgroups per CU at 2000 features");
    CHECK(2u * (size_t)tiled_plan(20000, 8).total <= 160u * 1024, "two tiled workgroups per CU");
}

// ---- a plan's regions: where, how long, the alignment the type needs, and the phases (bits) in which they are live
struct Region { const char *name; size_t off, bytes, align; unsigned live; };
// every region aligned, no two that are live together overlapping; returns the largest end
static size_t audit(const char *plan, const std::vector<Region> &r, long long n, int w) {
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % r[i].align == 0, "%s.%s at %zu needs %zu (n %lld waves %d)", plan, r[i].name, r[i].off, r[i].align, n, w);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j) {
            if (!(r[i].live & r[j].live) || !r[i].bytes || !r[j].bytes) continue;
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s.%s overlaps %s (n %lld waves %d)",
                  plan, r[i].name, r[j].name, n, w);
        }
    }
    return end;
}
static size_t red_bytes(int w) { return 8u * (size_t)(kRedSlots * 2 * w); }
static void misc_slots(const char *plan, size_t misc, size_t ints, size_t total) {
    CHECK((size_t)M_WCNT + kMaxWaves <= ints && (size_t)M_WCNT2 + kMaxWaves <= ints, "%s: a per-wave slot array leaves misc", plan);
    CHECK(misc + 4u * ints <= total, "%s: misc leaves the plan", plan);
}

// phase 1 the vote (counters), phase 2 the selection and the tail (the bit-set over the counters)
static size_t lds_end(long long n, int w) {
    const LdsPlan p = lds_plan((int)n, w);
    const size_t nn = (size_t)n, words = (nn + 31) / 32, room = p.reserved - p.c;
    CHECK(4u * words <= room, "lds: the bit-set leaves the counters' room (n %lld)", n);
    CHECK(4u * (words > 1 ? words : 1) <= room, "lds: the tail's reads leave the counters' room (n %lld)", n);
    CHECK(p.reserved + kReservedBytes == p.red, "lds: the reserved region");
    misc_slots("lds", p.misc, kMiscInts, p.total);
    return audit("lds", {{"p", p.p, 16u * even(n), 16, 3u}, {"y", p.y, 8u * even(n), 16, 3u},       // (staged two features per store)
                         {"c", p.c, 4u * ((nn + 1) / 2), 4, 1u}, {"sel", p.c, 4u * (words > 1 ? words : 1), 4, 2u},
                         {"red", p.red, red_bytes(w), 8, 3u}, {"misc", p.misc, 4u * kMiscInts, 4, 3u}}, n, w);
}
static size_t dense_end(long long n, int w) {
    const DensePlan p = dense_plan((int)n, w);
    const size_t nn = (size_t)n;
    misc_slots("dense", p.misc, kMiscInts, p.total);
    return audit("dense", {{"c", p.c, 4u * ((nn + 1) / 2), 4, 1u}, {"sel", p.sel, 4u * ((nn + 31) / 32), 4, 1u},
                           {"red", p.red, red_bytes(w), 8, 1u}, {"misc", p.misc, 4u * kMiscInts, 4, 1u}}, n, w);
}
// carved at the header's max_feat; a frame of n features puts its tile index, 2 (ntiles(n) + 1) ints, at toff
static size_t tiled_end(long long n, long long mf, int w) {
    const TiledPlan p = tiled_plan((int)mf, w);
    const size_t RW = (size_t)kRing * kTileW, ntiles = ((size_t)n + kTileW - 1) / kTileW;
    CHECK((size_t)M_PENDV < kTiledMiscInts && (size_t)M_PENDH < kTiledMiscInts, "tiled: a pending counter leaves misc");
    misc_slots("tiled", p.misc, kTiledMiscInts, p.total);
    return audit("tiled", {{"ringA", p.ringA, 16u * RW, 16, 1u}, {"ringB", p.ringB, 16u * RW, 16, 1u}, {"ringH", p.ringH, 8u * RW, 8, 1u},
                           {"ringC", p.ringC, 4u * RW, 4, 1u}, {"used", p.used, RW, 1, 1u}, {"pendV", p.pendV, 4u * kPendCap, 4, 1u},
                           {"pendH", p.pendH, 8u * kPendCapH, 8, 1u}, {"pendHv", p.pendH + 8u * kPendCapH, 4u * kPendCapH, 4, 1u},
                           {"toff", p.toff, 8u * (ntiles + 1), 4, 1u}, {"red", p.red, red_bytes(w), 8, 1u},
                           {"misc", p.misc, 4u * kTiledMiscInts, 4, 1u}}, n, w);
}

static void containment() {
    const std::vector<long long> f = feats();                        // (ascending)
    for (int w : kWavesList) {
        std::vector<size_t> le(f.size()), de(f.size());
        for (size_t i = 0; i < f.size(); ++i) { le[i] = lds_end(f[i], w); de[i] = dense_end(f[i], w); }
        for (size_t m = 0; m < f.size(); ++m) {
            const size_t lt = lds_plan((int)f[m], w).total, dt = dense_plan((int)f[m], w).total, tt = tiled_plan((int)f[m], w).total;
            for (size_t i = 0; i <= m; ++i) {
                CHECK(le[i] <= lt, "lds: frame %lld ends at %zu, header %lld asked for %zu (waves %d)", f[i], le[i], f[m], lt, w);
                CHECK(de[i] <= dt, "dense: frame %lld ends at %zu, header %lld asked for %zu (waves %d)", f[i], de[i], f[m], dt, w);
                CHECK(tiled_end(f[i], f[m], w) <= tt, "tiled: frame %lld, header %lld (waves %d)", f[i], f[m], w);
            }
        }
    }
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "totals")) totals();
    else if (argc == 2 && !strcmp(argv[1], "containment")) containment();
    else return 2;
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("scale_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_totals_are_the_old_formulas_and_the_stated_residencies_hold(plan_exe):
    assert _run(plan_exe, "totals").strip() == "0 failed"


def test_accepted_frames_lie_inside_the_request_aligned_and_disjoint(plan_exe):
    assert _run(plan_exe, "containment").strip() == "0 failed"
