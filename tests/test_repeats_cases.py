"""CPU: the repeated runs without a device — the LDS plan of flat_ransac_cases_kernel (csrc/mvosr_rescale_cases_plan.hpp) compiled
with g++ into a stand-alone program, the ctypes mirror of mvosr_rescale_cases_outputs against the header, the trimmed score of
evaluate.py, RepeatedRuns' assembly and file names with a stub in place of the device call, and the design of the crafted frames
of tests/repeats_cases.py.
"""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import flat_cases as fc
import repeats_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mvosr_rescale_cases_plan.hpp"
using namespace mvosr;

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
#define SAME32(f) CHECK((size_t)p.f == q.f, "32-bit and size_t plans differ at " #f)

struct Region { const char *name; size_t off, bytes, align; unsigned live; };

// phases (bits): 1 the form is built (w, dv), 2 the gather form's cases, 4 the packed form's cases.  Returns the largest end.
static size_t frame_end(long long n, long long tn, long long h) {
    const CasesPlan<uint32_t> p = cases_plan<uint32_t>(n, tn, h);
    const CasesPlan<size_t> q = cases_plan<size_t>(n, tn, h);
    SAME32(x); SAME32(y); SAME32(z); SAME32(list); SAME32(aux); SAME32(mods); SAME32(cnts); SAME32(misc); SAME32(total);
    SAME32(aux_bytes); SAME32(w); SAME32(dv); SAME32(px);
    const size_t plane = 8u * (size_t)n;
    const size_t items = (size_t)(n < kCasesPackMax ? n : kCasesPackMax);      // the packed form at its largest admissible extent
    std::vector<Region> r = {
        {"x", q.x, plane, 8, 7u}, {"y", q.y, plane, 8, 7u}, {"z", q.z, plane, 8, 7u},
        {"list", q.list, 6u * (size_t)tn, 2, 7u},                              // every row kept
        {"mods", q.mods, (size_t)kCasesPlaneBytes * (size_t)h, 16, 7u}, {"cnts", q.cnts, 4u * (size_t)h, 4, 7u},
        {"misc", q.misc, 4u * CM_N, 4, 7u},
        {"w", q.w, 4u * (size_t)n, 4, 3u}, {"dv", q.dv, 2u * (size_t)n, 2, 3u},
        {"px", q.px, 8u * items, 8, 4u}, {"py", q.px + 8u * items, 8u * items, 8, 4u}, {"pz", q.px + 16u * items, 8u * items, 8, 4u},
        {"pw", q.px + 24u * items, 4u * items, 4, 4u}};
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % r[i].align == 0, "%s at %zu needs %zu (n %lld tn %lld n_hyp %lld)", r[i].name, r[i].off, r[i].align, n, tn, h);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j) {
            if (!(r[i].live & r[j].live) || !r[i].bytes || !r[j].bytes) continue;
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s overlaps %s (n %lld tn %lld n_hyp %lld)",
                  r[i].name, r[j].name, n, tn, h);
        }
    }
    for (size_t i = 7; i < r.size(); ++i)
        CHECK(r[i].off >= q.aux && r[i].off + r[i].bytes <= q.aux + q.aux_bytes, "%s leaves aux (n %lld)", r[i].name, n);
    CHECK(end <= q.total, "the plan's own end %zu beyond its total %zu (n %lld tn %lld n_hyp %lld)", end, q.total, n, tn, h);
    return end;
}

static void containment() {
    const long long hyps[4] = {1, 7, 100, 512};
    const int NF = 71, NT = 141;
    std::vector<size_t> end((size_t)NF * NT), total((size_t)NF * NT);
    for (long long h : hyps) {
        for (int n = 0; n < NF; ++n)
            for (int tn = 0; tn < NT; ++tn) {
                end[(size_t)n * NT + tn] = frame_end(n, tn, h);
                total[(size_t)n * NT + tn] = cases_plan<size_t>(n, tn, h).total;
            }
        for (int mf = 0; mf < NF; ++mf)
            for (int mt = 0; mt < NT; ++mt)
                for (int n = 0; n <= mf; ++n)
                    for (int tn = 0; tn <= mt; ++tn)
                        if (end[(size_t)n * NT + tn] > total[(size_t)mf * NT + mt])
                            CHECK(false, "frame (%d, %d) ends at %zu, header (%d, %d) asked for %zu (n_hyp %lld)", n, tn,
                                  end[(size_t)n * NT + tn], mf, mt, total[(size_t)mf * NT + mt], h);
        // the large frames: alone, one smaller, and under a header one larger in either size
        for (long long n : {255ll, 256ll, 1023ll, 1024ll, 1025ll, 2000ll, 2001ll})
            for (long long tn : {1ll, n, 2 * n - 5, 2 * n}) {
                const size_t e = frame_end(n, tn, h);
                for (long long mf : {n, n + 1, 2 * n})
                    for (long long mt : {tn, tn + 1, 2 * mf})
                        if (mt >= tn) CHECK(e <= cases_plan<size_t>(mf, mt, h).total, "frame (%lld, %lld) under header (%lld, %lld)", n, tn, mf, mt);
            }
    }
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "total")) {                    // total <max_feat> <n_hyp>: the request at max_tri = 2 max_feat
        const long long mf = atoll(argv[2]);
        printf("%zu\n", cases_plan<size_t>(mf, 2 * mf, atoll(argv[3])).total);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "containment")) containment();
    else return 2;
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("cases_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_accepted_frames_lie_inside_the_request_aligned_and_disjoint(plan_exe):
    assert _run(plan_exe, "containment").strip() == "0 failed"


def test_total_at_the_point_cap_fits_the_devices_lds(plan_exe, monkeypatch):
    """ScaleEstimator._max_points() on a device with the MI355X's 160 KB of LDS per workgroup: the cases kernel's request at that
    cap fits too (the cap is flat_selection_kernel's; a 64 KB device would refuse the launch with MVOSR_ERR_TOO_LARGE instead)."""
    from mvoscalerecovery_amd import packing
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    huge = 1 << 30
    monkeypatch.setattr(packing, "delaunay_gpu_max_points", lambda: huge)
    est = types.SimpleNamespace(N_HYP=ScaleEstimator.N_HYP,
                                ctx=types.SimpleNamespace(lds_per_block=163840, lib=types.SimpleNamespace(mvosr_delaunay_lds_points=lambda: huge)))
    cap = ScaleEstimator._max_points(est)
    assert 3000 < cap < huge
    assert int(_run(plan_exe, "total", str(cap), str(ScaleEstimator.N_HYP))) <= 163840
    # one workgroup per CU at 2000 features, as the DESIGN section says
    assert 163840 // 2 < int(_run(plan_exe, "total", "2000", "100")) <= 163840


def test_ctypes_struct_matches_the_header(tmp_path):
    from mvoscalerecovery_amd import _lib
    cls, st = _lib.RescaleCasesOutputs, "mvosr_rescale_cases_outputs"
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvosr.h"', 'int main(void) {', 'printf("%s %%zu\\n", sizeof(%s));' % (st, st)]
    for n, _ in cls._fields_:
        src.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, n, st, n))
    src += ['printf("abi %d\\n", MVOSR_ABI_VERSION);',
            'printf("forms %d %d %d\\n", MVOSR_CASES_FORM_NONE, MVOSR_CASES_FORM_GATHER, MVOSR_CASES_FORM_PACKED);', 'return 0; }']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(line.split(None, 1) for line in lines)
    assert int(got["abi"]) == _lib.ABI_VERSION == 13
    assert got["forms"].split() == [str(v) for v in (_lib.CASES_FORM_NONE, _lib.CASES_FORM_GATHER, _lib.CASES_FORM_PACKED)]
    assert [int(v) for v in got["forms"].split()] == [rc.FORM_NONE, rc.FORM_GATHER, rc.FORM_PACKED]
    assert int(got[st]) == C.sizeof(cls)
    for n, _ in cls._fields_:
        assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, n


# ---- evaluate.py ------------------------------------------------------------------------------------------------------------------
def test_trimmed_mean():
    from mvoscalerecovery_amd.evaluate import trimmed_mean
    assert trimmed_mean([5.0, 1.0, 3.0, 9.0]) == 4.0                                 # 1 and 9 dropped
    assert trimmed_mean([2.0, 2.0, 2.0]) == 2.0
    assert trimmed_mean(np.array([10, 0, 1, 2, 3, 4, 5, 6, 7, 100])) == np.mean([1, 2, 3, 4, 5, 6, 7, 10])
    v = np.random.default_rng(3).normal(size=10)
    assert trimmed_mean(v) == np.mean(np.sort(v)[1:-1])                              # score_calculation.py:21-22
    for bad in ([], [1.0], [1.0, 2.0]):
        with pytest.raises(ValueError):
            trimmed_mean(bad)


def test_repeat_scores_equal_the_per_case_calls():
    from mvoscalerecovery_amd import evaluate, offline
    rng = np.random.default_rng(17)
    n = 900
    motions = np.tile(np.eye(3, 4).reshape(-1), (n, 1))
    motions[:, 3] = rng.normal(0, 0.02, n)
    motions[:, 11] = 1.0 + rng.normal(0, 0.05, n)
    gt = offline.get_path(motions, np.ones(n))
    paths = [offline.get_path(motions, 1.0 + rng.normal(0, 0.05 + 0.01 * c, n)) for c in range(10)]
    r = evaluate.repeat_scores(gt, paths)
    assert r["tra"].shape == r["rot"].shape == (10, 8)
    for c, p in enumerate(paths):
        rot, tra, _ = evaluate.calculate_ave_errors(evaluate.calculate_sequence_error(gt, p))
        assert np.array_equal(r["tra"][c], np.asarray(tra)) and np.array_equal(r["rot"][c], np.asarray(rot))
        assert r["tra_mean"][c] == np.mean(tra) and r["rot_mean"][c] == np.mean(rot)       # evaluate_vo.py:107
    assert r["trimmed"]["tra_mean"] == np.mean(np.sort(r["tra_mean"])[1:-1])
    assert r["trimmed"]["rot_mean"] == np.mean(np.sort(r["rot_mean"])[1:-1])
    assert np.array_equal(r["trimmed"]["tra"], [np.mean(np.sort(r["tra"][:, k])[1:-1]) for k in range(8)])
    with pytest.raises(ValueError):
        evaluate.repeat_scores(gt, paths[:2])


# ---- RepeatedRuns with a stub in place of the device call ------------------------------------------------------------------------
class _StubEstimator:
    """raw_scale_cases_batch without a device: case c of processed frame k gets 1 + 0.01 c + 0.001 k; frame 3 has no fit."""
    sampling = "device"

    def __init__(self):
        self._frame_counter = 0
        self.calls = []
        self.ctx = None

    def raw_scale_cases_batch(self, f3, f2, seeds, id_triples=None):
        F, Cn = len(f3), len(seeds)
        k0 = self._frame_counter
        self.calls.append((F, list(seeds), k0))
        raw = 1.0 + 0.01 * np.arange(Cn)[:, None] + 0.001 * (k0 + np.arange(F))[None, :]
        status = np.zeros((Cn, F), np.int32)
        for k in range(F):
            if k0 + k == 3:
                raw[:, k], status[:, k] = np.nan, fc.ST_RS_FEW
        return {"raw_scale": raw, "status": status, "height_level": np.ones(F), "host_errors": {}}


class _PyTail:
    """The tail recurrence in Python (rescale.py:169-178): stands in for mvosr_slew_median_host."""

    def __init__(self, window):
        self.window, self.scale, self.queue, self._frame_counter, self.prev = window, 1, [], 0, (0, 100)

    def push(self, raw, status, level, host_errors):
        out = []
        for r, s in zip(raw, status):
            if s == 0:
                self.scale = self.scale + 0.3 if r - self.scale > 0.3 else (self.scale - 0.3 if r - self.scale < -0.3 else r)
            self.queue = (self.queue + [self.scale])[-self.window:]
            out.append(np.median(self.queue))
        self._frame_counter += len(raw)
        return np.array(out), np.ones(len(raw))


def _stubbed(monkeypatch, cases=4, **kw):
    from mvoscalerecovery_amd import rescale
    stub = _StubEstimator()
    monkeypatch.setattr(rescale.RepeatedRuns, "_make_estimator", staticmethod(lambda a, w, k: stub))
    monkeypatch.setattr(rescale, "_CaseTail", lambda ctx, window: _PyTail(window))
    return rescale.RepeatedRuns(1.75, window_size=5, cases=cases, **kw), stub


def _toy_dict(n=14):
    rng = np.random.default_rng(5)
    sizes = [150, 150, 40, 150, 0, 150, 150, 150, 60, 150, 150, 0, 150, 150][:n]       # 0: not moving; <= 100: too few
    motions = [np.concatenate([np.eye(3), rng.normal(0, 0.1, (3, 1)) + [[0], [0], [1]]], axis=1).reshape(-1) for _ in sizes]
    return {"motions": motions, "move_flags": [s > 0 for s in sizes], "feature3ds": [np.zeros((s, 3)) for s in sizes],
            "feature2ds": [np.zeros((s, 2)) for s in sizes]}


def test_repeated_runs_sequence_assembly(monkeypatch):
    from mvoscalerecovery_amd import offline, rescale
    rr, stub = _stubbed(monkeypatch, seed=9)
    assert rr.seeds == rc.case_seeds(9, 4) == rescale.case_seeds(9, 4) and len(set(rr.seeds)) == 4
    data = _toy_dict()
    res = rr.run(data)
    kinds = offline.plan_sequence(data)
    assert np.array_equal(res["kinds"], kinds) and (kinds == 0).sum() == 2 and (kinds == 2).sum() == 2
    assert res["scales"].shape == (4, 14) and res["error"].shape == (4, 15)
    for c in range(4):
        tail = _PyTail(5)
        filt, std = tail.push(res["raw_scale"][c], res["status"][c], None, {})
        s, e = offline.assemble_outputs(kinds, list(filt), list(std))
        assert np.array_equal(res["scales"][c], s[1:]) and np.array_equal(res["error"][c], e)
        assert np.all(res["scales"][c][kinds == 0] == 0)                             # not moving: scale 0
        assert res["scales"][c][2] == res["scales"][c][1] and res["scales"][c][8] == res["scales"][c][7]   # too few: the previous scale
    assert stub.calls == [(10, rr.seeds, 0)] and stub._frame_counter == 10
    # a second run continues: counter, tails and the previous scale carry over
    rr2, stub2 = _stubbed(monkeypatch, seeds=rr.seeds)
    cut = 8                                                                          # the second part begins with a too-few frame
    parts = [{k: v[:cut] for k, v in data.items()}, {k: v[cut:] for k, v in data.items()}]
    both = np.concatenate([rr2.run(p)["scales"] for p in parts], axis=1)
    assert np.array_equal(both, res["scales"]) and np.array_equal(rr2.scales(), res["scales"])
    assert [c[2] for c in stub2.calls] == [0, 6]
    sp = rr.spread()
    assert np.allclose(sp["scale_std"], res["scales"].std(axis=0)) and sp["raw_mean"].shape == (10,) and np.isnan(sp["raw_mean"][3])


def test_repeated_runs_file_names_and_paths(monkeypatch, tmp_path):
    from mvoscalerecovery_amd import offline
    rr, _ = _stubbed(monkeypatch, cases=3, seeds=[1, 2, 3])
    data = _toy_dict()
    res = rr.run(data)
    names = rr.write_results(str(tmp_path) + "/seq_", "tag")
    assert sorted(os.listdir(tmp_path)) == sorted(["seq_scales.txttag%d" % c for c in range(3)] + ["seq_path.txttag%d" % c for c in range(3)])
    assert sorted(os.path.basename(n) for n in names) == sorted(os.listdir(tmp_path))
    paths = rr.paths()
    for c in range(3):
        assert np.array_equal(np.loadtxt(str(tmp_path / ("seq_scales.txttag%d" % c))), res["scales"][c])       # main_offline.py:90
        want = offline.get_path(np.array(data["motions"]), res["scales"][c])
        assert np.array_equal(paths[c], want) and want.shape == (15, 12)
        assert np.allclose(np.loadtxt(str(tmp_path / ("seq_path.txttag%d" % c))), want, rtol=0, atol=0)       # :92-93


def test_repeated_runs_seeds(monkeypatch):
    rr, _ = _stubbed(monkeypatch, cases=10)
    assert len(rr.seeds) == 10 and len(set(rr.seeds)) == 10 and all(0 <= s < 2 ** 64 for s in rr.seeds)    # from the OS
    rr, _ = _stubbed(monkeypatch, seeds=[2 ** 64 + 5, 7])
    assert rr.seeds == [5, 7] and rr.cases == 2
    assert rc.case_seeds(0, 2)[0] == rc.mix64(0) and rc.case_seeds(5, 12)[:10] == rc.case_seeds(5, 10)


# ---- the crafted frames' design ---------------------------------------------------------------------------------------------------
def test_crafted_frames_are_what_they_claim():
    def design(f):
        fl = rc.cpu_flags(f)
        ids = fc.point_list(f, fl)
        return len(ids), len(np.unique(ids)), rc.expected_form(f, fl), fl
    m, d, form, _ = design(rc.few_frame())
    assert m == 9 and form == rc.FORM_NONE and m < fc.MIN_POINTS
    m, d, form, _ = design(rc.exactly_min_frame())
    assert m == 12 == fc.MIN_POINTS and d == 12 and form == rc.FORM_PACKED
    m, d, form, _ = design(rc.packed_frame())
    assert 500 < d <= rc.PACK_MAX and form == rc.FORM_PACKED and len(rc.packed_frame().xyz) == 2000
    m, d, form, _ = design(rc.gather_frame())
    assert d > rc.PACK_MAX + 100 and form == rc.FORM_GATHER                        # more than 1000 distinct kept vertices
    f = rc.small_dense_frame()
    m, d, form, fl = design(f)
    assert m > 2 * len(f.xyz) and (fl & 4).astype(bool).mean() > 0.8 and form == rc.FORM_PACKED   # nearly every row kept
    f = rc.singular_frame()
    row = f.tri[np.nonzero(f.skip)[0][0]]
    assert row[0] == row[1] and abs(np.linalg.det(f.xyz[row])) == 0.0 and f.status == fc.ST_SINGULAR
    g = fc.grid_frame()
    tr = rc.repeated_vertex_triples(g, rc.cpu_flags(g), 3, 20)
    assert tr.shape == (3, 20, 3) and np.all(tr[:, 0, 0] == tr[:, 0, 1]) and len(set(tr[0, 1].tolist())) == 1
    assert all(len(set(t.tolist())) == 3 for t in tr[:, 2:].reshape(-1, 3)) and tr.max() < len(g.xyz)
