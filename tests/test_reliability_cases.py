"""CPU: the restatement of find_reliability_by_graph (tests/reliability_cases.py) against the reference's own run
(tests/golden/reliability.npz, and the reference itself where it is present), the crafted cases, the LDS plan of
reliability_kernel (csrc/mvosr_reliability_plan.hpp, compiled with g++ into a stand-alone program) and the C ABI's new entry."""
import os
import re
import subprocess

import numpy as np
import pytest

import reliability_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")
CRAFTED = sorted(rc.crafted_cases())


@pytest.fixture(scope="module")
def cases():
    return rc.crafted_cases()


@pytest.fixture(scope="module")
def vote_frames():
    """The golden's vote frames with their inputs regenerated: (f3, f2, rows, mask, reliability)."""
    from mvoscalerecovery_amd import synth
    z = rc.golden()
    out = []
    for k in range(int(z["n_vote"])):
        idx, n = (int(x) for x in z["v%d_spec" % k])
        assert synth.checksum(*synth.synth_frame(idx, n)) == int(z["v%d_crc" % k]), "synthetic generator drifted from the fixture"
        f3, f2, rows = rc.synth_vote_frame(idx, n)
        out.append((f3, f2, rows, np.unpackbits(z["v%d_mask" % k])[:len(f3)].astype(bool), z["v%d_reliability" % k]))
    return out


# ---- the restatement against the reference ---------------------------------------------------------------------------------------
def test_golden_covers_the_named_sizes(vote_frames):
    z = rc.golden()
    assert [int(z["v%d_spec" % k][1]) for k in range(int(z["n_vote"]))] == list(rc.GOLDEN_SIZES)
    assert len(z["seq_raw"]) == len(z["seq_scales"]) == len(z["seq_status"]) == 36
    for f3, _, _, mask, rel in vote_frames:
        assert len(rel) == len(mask) == len(f3) and np.array_equal(mask, rel > rc.START)


@pytest.mark.parametrize("k", range(len(rc.GOLDEN_SIZES)))
def test_both_forms_equal_the_reference_run_bit_for_bit(k, vote_frames):
    f3, f2, rows, mask, rel = vote_frames[k]
    seq = rc.sequential(rows, f3[:, 2], f2[:, 1], len(f3))
    sch, rounds, widest = rc.scheduled(rows, f3[:, 2], f2[:, 1], len(f3))
    assert seq.tobytes() == rel.tobytes()
    assert sch.tobytes() == rel.tobytes()
    assert np.array_equal(seq > rc.START, mask)
    assert 3 <= rounds < len(rows) and widest >= 1


@pytest.mark.reference
@pytest.mark.parametrize("k", range(len(rc.GOLDEN_SIZES)))
def test_both_forms_equal_the_reference_itself(k, vote_frames):
    from oracle import ref_harness
    if not ref_harness.reference_available():
        pytest.skip("reference not present")
    sc = ref_harness.load_reference()
    est = sc.ScaleEstimator(1.75, 5)
    f3, f2, rows, _, _ = vote_frames[k]
    with ref_harness.quiet():
        mask = est.find_reliability_by_graph(f3, f2, rows)
    graph = est.triangle2graph(rows)
    E = rc.edges_in_order(rows, len(f3))
    assert [(i, j) for i in range(len(graph)) for j in graph[i]] == [(int(i), int(j)) for i, j, _ in E]      # the order itself
    assert np.array_equal(mask, rc.sequential(rows, f3[:, 2], f2[:, 1], len(f3)) > rc.START)
    assert np.array_equal(mask, rc.scheduled(rows, f3[:, 2], f2[:, 1], len(f3))[0] > rc.START)


# ---- the crafted cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CRAFTED)
def test_expected_is_self_consistent(name, cases):
    c = cases[name]
    want = c.expected()
    assert want["status"] == 0 and not c.refused()
    r = want["reliability"]
    sch, rounds, _ = rc.scheduled(c.tri, c.remapped_z(), c.v, c.n_feat)
    assert sch.tobytes() == r.tobytes() or np.array_equal(sch, r, equal_nan=True)
    assert np.array_equal(want["keep"] == 0, r > rc.START) and set(np.unique(want["keep"]).tolist()) <= {0, -1}
    named = np.zeros(c.n_feat, bool)
    named[c.tri.reshape(-1)] = True
    assert (r[~named] == rc.START).all() and (want["keep"][~named] == -1).all()              # nobody names it: exactly 0.8, rejected
    # the order by brute force: a plain dictionary walk of triangle2graph's rule
    graph = {}
    for row in c.tri:
        s = sorted(int(x) for x in row)
        for a, b in ((s[0], s[1]), (s[0], s[2]), (s[1], s[2])):
            if b not in graph.setdefault(a, []):
                graph[a].append(b)
    assert [(i, j) for i in sorted(graph) for j in graph[i]] == [(int(i), int(j)) for i, j, _ in rc.edges_in_order(c.tri, c.n_feat)]
    assert len(c.tri) <= 2 * c.n_feat


def test_refused_cases_are_refused():
    for name, c in rc.refused_cases().items():
        want = c.expected()
        assert c.refused() and want["status"] == rc.ST_MASK and (want["keep"] == -1).all() and want["reliability"] is None, name


def test_crafted_cases_hold_what_they_claim(cases):
    r = cases["unnamed_vertices"].expected()
    assert (r["reliability"][[3, 5, 6]] == rc.START).all() and (r["keep"][[3, 5, 6]] == -1).all()
    assert rc.scheduled(cases["strip1500"].tri, cases["strip1500"].z, cases["strip1500"].v, 1502)[1:] == (3001, 1)      # one edge per round
    assert rc.scheduled(cases["strip1500_shuffled"].tri, cases["strip1500"].z, cases["strip1500"].v, 1502)[1] < 100
    E = rc.edges_in_order(cases["edge_on_three_rows"].tri, 43)
    assert E[0].tolist() == [0, 1, 0]                                                        # (0, 1): its first row is row 0
    r = cases["saturated_nan"].expected()["reliability"]
    assert r[60] == 0.0 and np.isnan(r[61]) and np.isnan(r[62]) and int(np.isnan(r).sum()) == 2
    c = cases["underflow"]
    i, j = rc.edges_in_order(c.tri, c.n_feat)[:, :2].T
    signs = np.sign(c.v[i] - c.v[j]) * np.sign(c.z[i] - c.z[j])
    assert (signs > 0).any() and not rc._abnormal(c.z, c.v, i, j).any()                     # the signs would say abnormal: the product says 0
    c = cases["nonfinite_depth"]
    assert np.isfinite(c.expected()["reliability"]).all()                                    # a NaN product is a normal edge
    c = cases["pitched"]
    assert c.pitch != 0.0 and not np.array_equal(c.remapped_z(), c.z)
    plain = rc.Case("plain", c.tri, c.z, c.v, y=c.y).expected()
    assert not np.array_equal(plain["reliability"], c.expected()["reliability"])
    assert np.array_equal(rc.Case("plain", c.tri, c.z, c.v, y=c.y).remapped_z(), c.z)          # pitch 0: the plain values


def test_the_order_sensitive_case_discriminates(cases):
    c = cases[rc.ORDER_CASE]
    ours, other = c.expected(), c.expected(block_order="ascending_j")
    assert not np.array_equal(rc.edges_in_order(c.tri, 7)[:, :2], rc.edges_in_order(c.tri, 7, "ascending_j")[:, :2])
    assert not np.array_equal(ours["keep"], other["keep"])
    assert ours["keep"][6] == 0 and other["keep"][6] == -1


# ---- the LDS plan ----------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
#include "mvosr_reliability_plan.hpp"
using namespace mvosr;

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
#define SAME32(f) CHECK((size_t)p.f == q.f, "32-bit and size_t plans differ at " #f " (%lld, %lld)", mf, mt)

// where, how many bytes a frame of (n, tn) uses, the alignment the type needs, the phases (bits) in which it is live
struct Region { const char *name; size_t off, bytes, align; unsigned live; };

// the plan at the header's (mf, mt), used by a frame of (n, tn) the kernel accepts: returns the largest end
static size_t frame_end(long long mf, long long mt, long long n, long long tn) {
    const ReliabilityPlan<uint32_t> p = reliability_plan<uint32_t>((uint32_t)mf, (uint32_t)mt);
    const ReliabilityPlan<size_t> q = reliability_plan<size_t>((size_t)mf, (size_t)mt);
    SAME32(work); SAME32(st); SAME32(it); SAME32(r16); SAME32(inc); SAME32(first); SAME32(abn); SAME32(misc); SAME32(total);
    SAME32(work_bytes); SAME32(bits_bytes); SAME32(z); SAME32(v); SAME32(rel); SAME32(lstart); SAME32(ptr);
    const size_t N = (size_t)n, T = (size_t)tn, words = 4u * ((3u * T + 31) / 32);
    // phase 1: the build (z', v alive); phase 2: the lists and the rounds (the late aliases alive)
    const std::vector<Region> r = {
        {"z", q.z, 8u * N, 8, 1u}, {"v", q.v, 8u * N, 8, 1u},
        {"rel", q.rel, 8u * N, 8, 2u}, {"lstart", q.lstart, 4u * (N + 1), 4, 2u}, {"ptr", q.ptr, 4u * N, 4, 2u},
        {"st", q.st, 4u * (N + 1), 4, 3u}, {"it", q.it, 6u * T, 2, 3u}, {"r16", q.r16, 6u * T, 2, 3u}, {"inc", q.inc, 12u * T, 2, 2u},
        {"first", q.first, words, 4, 3u}, {"abn", q.abn, words, 4, 3u}, {"misc", q.misc, 4u * RM_N, 4, 3u}};
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % r[i].align == 0, "%s at %zu needs %zu (header %lld, %lld)", r[i].name, r[i].off, r[i].align, mf, mt);
        if (i < 5) CHECK(r[i].off >= q.work && r[i].off + r[i].bytes <= q.work + q.work_bytes, "%s leaves the work area (header %lld, %lld)", r[i].name, mf, mt);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j) {
            if (!(r[i].live & r[j].live) || !r[i].bytes || !r[j].bytes) continue;
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s overlaps %s (header %lld, %lld, frame %lld, %lld)",
                  r[i].name, r[j].name, mf, mt, n, tn);
        }
    }
    CHECK(words <= q.bits_bytes, "bit words");
    return end;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "total")) {                    // total <max_feat>: the request at max_tri = 2 max_feat
        long long mf = 0;
        sscanf(argv[2], "%lld", &mf);
        printf("%zu\n", reliability_plan<size_t>((size_t)mf, (size_t)(mf < 1 ? 1 : 2 * mf)).total);
        return 0;
    }
    if (argc != 2 || strcmp(argv[1], "check")) return 2;
    // the launcher's headers: max_tri = 2 max_feat, at least 1; every frame such a header admits
    for (long long mf = 0; mf <= 70; ++mf) {
        const long long mt = mf < 1 ? 1 : 2 * mf;
        const size_t total = reliability_plan<size_t>((size_t)mf, (size_t)mt).total;
        for (long long n = 0; n <= mf; ++n)
            for (long long tn = 1; tn <= mt; ++tn)
                CHECK(frame_end(mf, mt, n, tn) <= total, "frame (%lld, %lld) leaves the request of header (%lld, %lld)", n, tn, mf, mt);
    }
    for (long long mf : {255ll, 256ll, 1999ll, 2000ll, 2001ll, 2356ll, 10922ll}) {
        const long long mt = 2 * mf;
        const size_t total = reliability_plan<size_t>((size_t)mf, (size_t)mt).total;
        for (long long n : {0ll, 1ll, mf - 1, mf})
            for (long long tn : {1ll, mt - 1, mt})
                CHECK(frame_end(mf, mt, n, tn) <= total, "frame (%lld, %lld) leaves the request of header (%lld, %lld)", n, tn, mf, mt);
    }
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("reliability_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_plan_is_aligned_disjoint_and_inside_the_request(plan_exe):
    r = subprocess.run([plan_exe, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failed", r.stdout + r.stderr


def test_plan_totals_at_the_documented_sizes(plan_exe):
    total = lambda mf: int(subprocess.run([plan_exe, "total", str(mf)], capture_output=True, text=True, check=True).stdout)
    assert total(2000) == 16 * 2000 + 16 + 4 * 2002 + 24 * 4000 + 8 * 375 + 64 <= 163840        # the header's formula: 136 KB
    assert round(total(2000) / 1024) == 136
    assert total(2356) <= 163840 < total(2400)                                                    # the largest frames the 160 KB admit


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_bound():
    from mvoscalerecovery_amd import _lib
    with open(os.path.join(ROOT, "include", "mvosr.h")) as fh:
        header = fh.read()
    m = re.search(r"int mvosr_reliability_batch\(([^;]*)\);", header)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["ctx", "p", "b", "reliability_out", "keep_out", "status_out"]
    assert len(_lib.SYMBOLS["mvosr_reliability_batch"][1]) == 6
    assert _lib.ABI_VERSION == 13 and re.search(r"#define MVOSR_ABI_VERSION 13\b", header)
