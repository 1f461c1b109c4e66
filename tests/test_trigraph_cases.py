"""CPU: the restatement of feature_selection_by_tri_graph (tests/trigraph_cases.py) against the reference's own run
(tests/golden/trigraph.npz, and the reference itself where it is present), the crafted cases, the LDS plan of tri_graph_kernel
(csrc/mvosr_trigraph_plan.hpp, compiled with g++ into a stand-alone program), the C ABI's new entry and the estimator's keyword."""
import os
import re
import subprocess

import numpy as np
import pytest

import trigraph_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")
CRAFTED = sorted(tc.crafted_cases())


@pytest.fixture(scope="module")
def cases():
    return tc.crafted_cases()


@pytest.fixture(scope="module")
def frames():
    """The golden's frames with their inputs regenerated: (f3, rows, golden arrays by name)."""
    from mvoscalerecovery_amd import synth
    z = tc.golden()
    out = []
    for k in range(int(z["n_frames"])):
        idx, n = (int(x) for x in z["f%d_spec" % k])
        assert synth.checksum(*synth.synth_frame(idx, n)) == int(z["f%d_crc" % k]), "synthetic generator drifted from the fixture"
        f3, _, rows = tc.synth_survivors(idx, n)
        out.append((f3, rows, {name[len("f%d_" % k):]: z[name] for name in z.files if name.startswith("f%d_" % k)}))
    return out


# ---- the restatement against the reference ---------------------------------------------------------------------------------------
def test_golden_covers_the_named_sizes(frames):
    z = tc.golden()
    assert [int(z["f%d_spec" % k][1]) for k in range(int(z["n_frames"]))] == list(tc.GOLDEN_SIZES)
    assert len(z["seq_raw"]) == len(z["seq_scales"]) == len(z["seq_status"]) == 36
    assert 0 < float(z["p_atol"]) < 1e-5
    for f3, rows, g in frames:
        assert len(g["p_road"]) == len(g["pitch"]) == len(g["heights"]) == len(g["neighbors"]) == len(rows)
        assert np.array_equal(g["ids"], np.unique(rows[g["p_road"] > 0.5].reshape(-1)))
        # what makes the from-points comparison meaningful
        assert np.abs(g["pitch"] + 80).min() > 1e-5 and np.abs(g["p_road"][g["pitch"] < -80] - 0.5).min() > 1e-5


@pytest.mark.parametrize("k", range(len(tc.GOLDEN_SIZES)))
def test_both_forms_equal_the_reference_run_bit_for_bit(k, frames):
    f3, rows, g = frames[k]
    graph = tc.region_graph(rows)
    assert [[int(u) for u in row if u >= 0] for row in g["neighbors"]] == graph                 # the reference's lists, in its order
    assert np.array_equal(tc.neighbors_table(rows), g["neighbors"])                             # the closed form the device builds
    seq = tc.sequential(graph, g["heights"], g["pitch"])
    sch, rounds, widest = tc.scheduled(graph, g["heights"], g["pitch"])
    assert seq.tobytes() == g["p_road"].tobytes()
    assert sch.tobytes() == g["p_road"].tobytes()
    assert rounds == int(g["rounds"]) and 12 <= rounds <= 17 and widest >= 1
    assert tc.height_level(g["heights"], g["pitch"]).tobytes() == g["level"].tobytes()
    if k == 0:                                                                                  # the association is what is pinned
        for form in ("left_to_right", "chained_fma", "pairwise"):
            assert tc.sequential(graph, g["heights"], g["pitch"], form=form).tobytes() != g["p_road"].tobytes(), form


@pytest.mark.reference
@pytest.mark.parametrize("k", range(len(tc.GOLDEN_SIZES) - 1))
def test_restatement_equals_the_reference_itself(k, frames):
    from oracle import ref_harness
    if not ref_harness.reference_available():
        pytest.skip("reference not present")
    est = ref_harness.load_reference().ScaleEstimator(1.75, 5)
    f3, rows, g = frames[k]
    with ref_harness.quiet():
        ids = est.feature_selection_by_tri_graph(f3, rows)
        graph = est.triangle2region_graph(rows)
    assert [[int(u) for u in lst] for lst in graph] == tc.region_graph(rows)
    p = tc.sequential(tc.region_graph(rows), g["heights"], g["pitch"])
    assert np.array_equal(ids, np.unique(rows[p > 0.5].reshape(-1))) and np.array_equal(ids, g["ids"])
    assert np.float64(est.height_level).tobytes() == g["level"].tobytes()


# ---- the crafted cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CRAFTED)
def test_expected_is_self_consistent(name, cases):
    c = cases[name]
    want = c.expected()
    assert want["status"] == 0 and not c.refused() and len(c.tri) <= 2 * c.n_feat
    graph = tc.region_graph(c.tri)
    assert [[int(u) for u in row if u >= 0] for row in want["neighbors"]] == graph
    assert all(len(g) <= 3 for g in graph)
    seq = tc.sequential(graph, c.heights, c.pitch)
    nan = np.isnan(seq)
    assert np.array_equal(nan, np.isnan(want["p_road"])) and seq[~nan].tobytes() == want["p_road"][~nan].tobytes()       # scheduled = sequential
    flat = c.pitch < tc.THR
    assert want["n_flat"] == int(flat.sum()) and (want["p_road"][~flat].tobytes() == want["p_initial"][~flat].tobytes())
    assert want["n_rounds"] <= max(want["n_flat"], 0) and (want["n_rounds"] > 0) == bool(flat.any())
    named = np.zeros(c.n_feat, bool)
    named[c.tri[want["valid"] != 0].reshape(-1)] = True
    assert np.array_equal(want["selected"] != 0, named)


def test_refused_cases_are_refused():
    for name, c in tc.refused_cases().items():
        want = c.expected()
        assert c.refused() and want["status"] == tc.ST_MASK and not want["valid"].any() and not want["selected"].any(), name
    assert tc.Case("no_rows", np.zeros((0, 3)), [], [], n_feat=5).expected()["status"] == tc.ST_EMPTY


def test_crafted_cases_hold_what_they_claim(cases):
    r = cases["one_row"].expected()
    assert r["p_road"][0] == r["p_initial"][0] == (-70 - -85.0) / 20 - 0.2 and r["valid"][0] == 1 and r["n_rounds"] == 1
    assert cases["strip1500"].expected()["n_rounds"] == 1500                                   # one row per round
    assert cases["strip1500_shuffled"].expected()["n_rounds"] < 100
    a, b = cases["strip1500"].expected(), cases["strip1500_shuffled"].expected()
    assert a["n_flat"] == b["n_flat"] == 1500
    c = cases["threshold_steps"]
    d = c.heights[[1, 2, 3, 5, 6, 7]] - c.heights[0]
    assert [tc.compare(c.heights[i], c.heights[0]) for i in (1, 2, 3, 5, 6, 7)] == [1 if x > 0.1 else -1 if x < -0.1 else 0 for x in d]
    assert sorted(set(tc.compare(c.heights[i], c.heights[0]) for i in (1, 2, 3))) == [0, 1]    # +0.1 and its two neighbours straddle the test
    assert sorted(set(tc.compare(c.heights[i], c.heights[0]) for i in (5, 6, 7))) == [-1, 0]
    r = cases["no_flat_row"].expected()
    assert r["n_flat"] == 0 and r["n_rounds"] == 0 and not r["valid"].any() and np.isfinite(r["height_level"])
    r = cases["only_flat_rows"].expected()
    assert np.isnan(r["height_level"]) and r["n_flat"] == len(cases["only_flat_rows"].tri) and r["valid"].any()
    c = cases["nan_inputs"]
    r = c.expected()
    assert not r["valid"][np.isnan(c.pitch)].any() and np.isnan(r["p_initial"][np.isnan(c.pitch)]).all()
    r = cases["two_components"].expected()
    assert not r["selected"][10:20].any()


def test_the_two_flip_cases_discriminate(cases):
    c = cases[tc.ORDER_CASE]
    assert tc.region_graph(c.tri)[2] == [1, 0]                                                   # list order is not ascending order
    ours, other = c.expected(), c.expected(order="ascending")
    assert ours["valid"][2] == 1 and other["valid"][2] == 0 and int((ours["valid"] != other["valid"]).sum()) == 1
    c = cases[tc.HIGHER_CASE]
    graph = tc.region_graph(c.tri)
    assert 6 in graph[1] and c.pitch[1] < tc.THR and c.pitch[6] < tc.THR                        # row 1 reads flat row 6 before 6's turn
    ours, other = c.expected(), c.expected(higher="final")
    assert ours["valid"][1] == 1 and other["valid"][1] == 0
    assert min(abs(ours["p_road"][1] - 0.5), abs(tc.sequential(graph, c.heights, c.pitch, higher="final")[1] - 0.5)) > 0.01


def test_fma_is_exact():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    assert tc.fma(a, b, -1.0) == -2.0 ** -60 and a * b - 1.0 == 0.0                             # the product's low bits survive
    assert np.isnan(tc.fma(np.nan, 1.0, 1.0)) and tc.fma(np.inf, 1.0, 1.0) == np.inf


# ---- the LDS plan ----------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
#include "mvosr_trigraph_plan.hpp"
using namespace mvosr;

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
#define SAME32(f) CHECK((size_t)p.f == q.f, "32-bit and size_t plans differ at " #f " (%lld, %lld)", mf, mt)

// where, how many bytes a frame of (n, tn) uses, the alignment the type needs, the phases (bits) in which it is live
struct Region { const char *name; size_t off, bytes, align; unsigned live; bool in_work; };

static size_t frame_end(bool pts, long long mf, long long mt, long long n, long long tn) {
    const TriGraphPlan<uint32_t> p = trigraph_plan<uint32_t>(pts, (uint32_t)mf, (uint32_t)mt);
    const TriGraphPlan<size_t> q = trigraph_plan<size_t>(pts, (size_t)mf, (size_t)mt);
    SAME32(work); SAME32(h); SAME32(p0); SAME32(nb); SAME32(lvl); SAME32(flag); SAME32(sel); SAME32(misc); SAME32(total); SAME32(work_bytes);
    SAME32(x); SAME32(y); SAME32(z); SAME32(st); SAME32(it); SAME32(r16); SAME32(hs); SAME32(leaf); SAME32(p1);
    const size_t N = (size_t)n, T = (size_t)tn;
    // phases: 1 the values (vertex planes), 2 the table and the neighbours, 4 height_level, 8 the rounds and the outputs
    const std::vector<Region> r = {
        {"x", q.x, pts ? 8u * N : 0, 8, 1u, true}, {"y", q.y, pts ? 8u * N : 0, 8, 1u, true}, {"z", q.z, pts ? 8u * N : 0, 8, 1u, true},
        {"st", q.st, 4u * (N + 1), 4, 2u, true}, {"it", q.it, 6u * T, 2, 2u, true}, {"r16", q.r16, 6u * T, 2, 2u, true},
        {"hs", q.hs, 8u * T, 8, 4u, true}, {"leaf", q.leaf, 8u * TL_N, 8, 4u, true}, {"p1", q.p1, 8u * T, 8, 8u, true},
        {"h", q.h, 8u * T, 8, 15u, false}, {"p0", q.p0, 8u * T, 8, 15u, false}, {"nb", q.nb, 6u * T, 2, 15u, false},
        {"lvl", q.lvl, 2u * T, 2, 15u, false}, {"flag", q.flag, T, 1, 15u, false}, {"sel", q.sel, 4u * ((N + 31) / 32), 4, 15u, false},
        {"misc", q.misc, 4u * TM_N, 4, 15u, false}};
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        if (!r[i].bytes) continue;
        CHECK(r[i].off % r[i].align == 0, "%s at %zu needs %zu (header %lld, %lld)", r[i].name, r[i].off, r[i].align, mf, mt);
        if (r[i].in_work) CHECK(r[i].off >= q.work && r[i].off + r[i].bytes <= q.work + q.work_bytes, "%s leaves the work area (header %lld, %lld)", r[i].name, mf, mt);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j) {
            if (!(r[i].live & r[j].live) || !r[j].bytes) continue;
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s overlaps %s (header %lld, %lld, frame %lld, %lld)",
                  r[i].name, r[j].name, mf, mt, n, tn);
        }
    }
    CHECK(TL_SLOT >= 8192 / 64 && TL_VAL > TL_SLOT && TL_STACK >= TL_VAL + 9 && 8 * TL_TABLE >= 8 * TL_STACK + 4 * 24 && 8 * TL_N >= 8 * TL_TABLE + 4 * (8192 / 64), "leaf region");
    CHECK(TM_WSUM + kRsWaves <= TM_LEAVES && TM_LEAVES < TM_N && TM_CNT + 3 <= TM_WSUM, "misc slots");
    return end;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "total")) {                    // total <pts> <max_feat>: the request at max_tri = 2 max_feat
        long long pts = 0, mf = 0;
        sscanf(argv[2], "%lld", &pts);
        sscanf(argv[3], "%lld", &mf);
        printf("%zu\n", trigraph_plan<size_t>(pts != 0, (size_t)mf, (size_t)(mf < 1 ? 1 : 2 * mf)).total);
        return 0;
    }
    if (argc != 2 || strcmp(argv[1], "check")) return 2;
    for (int pts = 0; pts < 2; ++pts) {
        for (long long mf = 0; mf <= 70; ++mf) {
            const long long mt = mf < 1 ? 1 : 2 * mf;
            const size_t total = trigraph_plan<size_t>(pts, (size_t)mf, (size_t)mt).total;
            for (long long n = 0; n <= mf; ++n)
                for (long long tn = 1; tn <= mt; ++tn)
                    CHECK(frame_end(pts, mf, mt, n, tn) <= total, "frame (%lld, %lld) leaves the request of header (%lld, %lld)", n, tn, mf, mt);
        }
        for (long long mf : {255ll, 256ll, 1999ll, 2000ll, 2001ll, 2095ll, 32767ll}) {
            const long long mt = 2 * mf;
            const size_t total = trigraph_plan<size_t>(pts, (size_t)mf, (size_t)mt).total;
            for (long long n : {0ll, 1ll, mf - 1, mf})
                for (long long tn : {1ll, mt - 1, mt})
                    CHECK(frame_end(pts, mf, mt, n, tn) <= total, "frame (%lld, %lld) leaves the request of header (%lld, %lld)", n, tn, mf, mt);
        }
    }
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("trigraph_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_plan_is_aligned_disjoint_and_inside_the_request(plan_exe):
    r = subprocess.run([plan_exe, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failed", r.stdout + r.stderr


def test_plan_totals_at_the_documented_sizes(plan_exe):
    total = lambda pts, mf: int(subprocess.run([plan_exe, "total", str(pts), str(mf)], capture_output=True, text=True, check=True).stdout)
    # the header's formula at 2 000 features: the table is the largest tenant of the work area in both forms
    want = (4 * 2002 + 12 * 4000 + 8) + 16 * 4000 + 6 * 4000 + 2 * 4000 + 4000 + 4 * 63 + 4 + 80
    assert total(0, 2000) == total(1, 2000) == want <= tc.LDS_LIMIT
    assert round(total(1, 2000) / 1024) == 153
    assert total(1, 2095) <= tc.LDS_LIMIT < total(1, 2096)                                       # the largest frames the 160 KB admit
    assert total(0, 2095) <= tc.LDS_LIMIT < total(0, 2096)


# ---- the C ABI and the estimator's keyword ---------------------------------------------------------------------------------------
def test_symbol_is_declared_and_bound():
    from mvoscalerecovery_amd import _lib
    with open(os.path.join(ROOT, "include", "mvosr.h")) as fh:
        header = fh.read()
    m = re.search(r"int mvosr_tri_graph_batch\(([^;]*)\);", header)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["ctx", "p", "b", "tri_height_in", "tri_pitch_in", "o"]
    assert len(_lib.SYMBOLS["mvosr_tri_graph_batch"][1]) == 6
    fields = re.search(r"typedef struct mvosr_trigraph_outputs \{(.*?)\} mvosr_trigraph_outputs;", header, re.S).group(1)
    names = [n for line in fields.splitlines() if ";" in line for n in re.findall(r"\*(\w+)", line.split(";")[0])]
    assert names == [k for k, _ in _lib.TriGraphOutputs._fields_]
    assert _lib.ABI_VERSION == 13 and re.search(r"#define MVOSR_ABI_VERSION 13\b", header)


def test_estimator_keyword_is_validated():
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    with pytest.raises(ValueError, match="scipy"):
        ScaleEstimator(1.75, 5, triangulation="gpu", selection="tri_graph")
    with pytest.raises(ValueError, match="scipy"):
        ScaleEstimator(1.75, 5, selection="tri_graph")                                           # the default triangulation is the device's
    with pytest.raises(ValueError, match="selection"):
        ScaleEstimator(1.75, 5, triangulation="scipy", selection="graph")
