"""CPU: the budget sweep of the RANSAC evaluation (csrc/mvosr_hpeval_budgets.hip, height_pitch.RansacBudgetSweep) — plumbing and
references, no device.

* the LDS plan (csrc/mvosr_hpeval_budgets_plan.hpp), compiled with g++ into a stand-alone program: regions that live together are
  disjoint and aligned to 16, the total is what the library's ..._lds_bytes returns, the 32-bit plan is the size_t plan, and the
  total exceeds hpeval_plan's by the snapshots alone — it does not grow with the last budget beyond one tile;
* the header, the binding and the built library name the same functions, and the binding's structs have the header's layout;
* check_budgets on good and bad lists;
* table, smallest_budget, spread and results_at on planted results (NaN refined values, an all-carried frame, an empty dump);
* the checkpoints' semantics: the np.longdouble reference DECIDES every one of the 324 (scene, model, case, budget) combinations
  that tests/test_gpu_hpeval_budgets.py demands exactly — 50 of them without a model yet —, and a replay cut at the budgets and at
  the tiles' ends, its state carried, is the uncut replay of each budget's hypotheses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import flat_cases as fc
import hpeval_budgets_cases as hb
import hpeval_cases as he
from conftest import ROOT

CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")

# ---- the LDS plan ----------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "mvosr_hpeval_budgets_plan.hpp"
using namespace mvosr;
static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
struct Region { const char *name; size_t off, bytes; };
static size_t frame_end(long long n, long long tn, long long h, long long nb) {
    const HpEvalBudgetsPlan<uint32_t> p = hpeval_budgets_plan<uint32_t>((uint32_t)n, (uint32_t)tn, (uint32_t)h, (uint32_t)nb);
    const HpEvalBudgetsPlan<size_t> q = hpeval_budgets_plan<size_t>((size_t)n, (size_t)tn, (size_t)h, (size_t)nb);
    const HpEvalPlan<size_t> e = hpeval_plan<size_t>((size_t)n, (size_t)tn, (size_t)h);
    CHECK(p.frame.x == q.frame.x && p.frame.y == q.frame.y && p.frame.z == q.frame.z && p.frame.list == q.frame.list && p.frame.mods == q.frame.mods &&
          p.frame.cnts == q.frame.cnts && p.frame.words == q.frame.words && p.frame.misc == q.frame.misc && p.frame.red == q.frame.red &&
          p.frame.total == q.frame.total && p.snap == q.snap && p.total == q.total, "32-bit and size_t plans differ (%lld %lld %lld %lld)", n, tn, h, nb);
    CHECK(q.frame.x == e.x && q.frame.y == e.y && q.frame.z == e.z && q.frame.list == e.list && q.frame.mods == e.mods && q.frame.cnts == e.cnts &&
          q.frame.words == e.words && q.frame.misc == e.misc && q.frame.red == e.red && q.frame.total == e.total, "the frame's part is not hpeval_plan");
    CHECK(q.total == e.total + (size_t)kHpeSnapBytes * (size_t)nb, "the request exceeds hpeval_plan's by more than the snapshots (%lld %lld %lld %lld)", n, tn, h, nb);
    const size_t tile = (size_t)(h < kHpMaxHyp ? h : kHpMaxHyp);
    const std::vector<Region> r = {{"x", q.frame.x, 8u * (size_t)n}, {"y", q.frame.y, 8u * (size_t)n}, {"z", q.frame.z, 8u * (size_t)n},
        {"list", q.frame.list, 6u * (size_t)tn}, {"mods", q.frame.mods, (size_t)kHpPlaneBytes * tile}, {"cnts", q.frame.cnts, 4u * tile},
        {"words", q.frame.words, 8u * ((3u * (size_t)tn + 63) / 64)}, {"misc", q.frame.misc, 4u * HE_N}, {"red", q.frame.red, 8u * HER_N},
        {"snap", q.snap, sizeof(HpeSnapshot) * (size_t)nb}};
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % 16 == 0, "%s at %zu (%lld %lld %lld %lld)", r[i].name, r[i].off, n, tn, h, nb);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j)
            CHECK(!r[i].bytes || !r[j].bytes || r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s overlaps %s (%lld %lld %lld %lld)",
                  r[i].name, r[j].name, n, tn, h, nb);
    }
    CHECK(end <= q.total, "plan ends at %zu, total %zu", end, q.total);
    return end;
}
int main(int argc, char **argv) {
    static_assert(sizeof(HpeSnapshot) == 48 && kHpeSnapBytes == 48 && kHpeMaxBudgets == 16, "48 bytes per checkpoint, at most 16");
    static_assert(HB_NEXT != HE_DONE && HB_NEXT != HE_DEGEN && HB_NEXT >= HM_I0 + 3 && HB_NEXT < HM_CW, "slots");
    if (argc == 4) {
        const long long mf = atoll(argv[1]);
        printf("%zu %zu\n", hpeval_budgets_plan<size_t>(mf, mf ? 2 * mf : 1, atoll(argv[2]), atoll(argv[3])).total, hpeval_plan<size_t>(mf, mf ? 2 * mf : 1, atoll(argv[2])).total);
        return 0;
    }
    const long long hyps[6] = {1, 65, 500, 512, 513, 4096}, nbs[3] = {1, 7, 16};
    for (long long nb : nbs)
        for (long long h : hyps)
            for (long long mf = 0; mf <= 40; ++mf) {
                const long long mt = mf ? 2 * mf : 1;                   // what the launcher asks for
                const size_t total = hpeval_budgets_plan<size_t>(mf, mt, h, nb).total;
                for (long long n = 0; n <= mf; ++n)
                    for (long long tn = 0; tn <= mt; ++tn)
                        CHECK(frame_end(n, tn, h, nb) <= total, "frame (%lld, %lld) leaves the request of header %lld, last budget %lld", n, tn, mf, h);
            }
    for (long long mf : {255ll, 256ll, 2000ll, 2001ll, 10922ll}) { frame_end(mf, 2 * mf, 500, 16); frame_end(mf, 2 * mf, 4096, 16); }
    // one tile is all the hypotheses ever take
    CHECK(hpeval_budgets_plan<size_t>(2000, 4000, 512, 7).total == hpeval_budgets_plan<size_t>(2000, 4000, 4096, 7).total, "the request grows beyond a tile");
    CHECK(hpeval_budgets_plan<size_t>(2000, 4000, 511, 7).total < hpeval_budgets_plan<size_t>(2000, 4000, 512, 7).total, "the request does not grow up to a tile");
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("hpeval_budgets_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_plan_regions_are_aligned_and_disjoint_and_add_the_snapshots_only(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failed", r.stdout + r.stderr


def test_lds_request_is_the_plans_total(plan_exe):
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    for mf, h, nb in ((0, 1, 1), (3, 64, 2), (300, 513, 6), (2000, 2000, 7), (2000, 4096, 16)):
        want, base = (int(x) for x in subprocess.run([plan_exe, str(mf), str(h), str(nb)], capture_output=True, text=True, check=True).stdout.split())
        for model in (_lib.HP_MODEL_PLANE, _lib.HP_MODEL_LINE):
            assert int(lib.mvosr_height_pitch_eval_budgets_lds_bytes(mf, h, nb, model)) == want
            assert want - int(lib.mvosr_height_pitch_eval_lds_bytes(mf, h, model)) == want - base == 48 * nb
    assert lib.mvosr_height_pitch_eval_budgets_lds_bytes(2000, 4096, 16, 0) <= 96 * 1024


# ---- header, binding, library ------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(tmp_path):
    from mvoscalerecovery_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvosr.h")).read()
    assert re.search(r"\bint mvosr_height_pitch_eval_budgets_batch\(", header) and re.search(r"\bsize_t mvosr_height_pitch_eval_budgets_lds_bytes\(", header)
    assert len(_lib.SYMBOLS["mvosr_height_pitch_eval_budgets_batch"][1]) == 8 and len(_lib.SYMBOLS["mvosr_height_pitch_eval_budgets_lds_bytes"][1]) == 4
    assert re.search(r"#define MVOSR_ABI_VERSION 13\b", header) and _lib.ABI_VERSION == 13   # the change is additive
    lib = _lib.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    for sym in ("mvosr_height_pitch_eval_budgets_batch", "mvosr_height_pitch_eval_budgets_lds_bytes"):
        assert re.search(r"\bT %s\b" % sym, exported), sym
    structs = {"mvosr_height_pitch_eval_budgets_outputs": _lib.HeightPitchEvalBudgetsOutputs, "mvosr_height_pitch_eval_params": _lib.HeightPitchEvalParams}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvosr.h"', 'int main(void) {']
    for st, cls in structs.items():
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for n, _ in cls._fields_:
            src.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, n, st, n))
    src.append('return 0; }')
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in structs.items():
        assert int(got[st]) == C.sizeof(cls), st
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)
    assert "list_mask" not in dict(_lib.HeightPitchEvalBudgetsOutputs._fields_) and "best" in dict(_lib.HeightPitchEvalBudgetsOutputs._fields_)


# ---- check_budgets -----------------------------------------------------------------------------------------------------------
def test_check_budgets():
    from mvoscalerecovery_amd.height_pitch import check_budgets
    assert check_budgets([25, 50, 100]) == (25, 50, 100) and check_budgets((1,)) == (1,) and check_budgets(np.array([1, 4096])) == (1, 4096)
    assert check_budgets(range(1, 17)) == tuple(range(1, 17))
    for bad in ([], range(1, 18), [5, 5], [5, 3], [0, 1], [-1], [1, 4097], [4097], [1.5, 2], None, 7):
        with pytest.raises(ValueError):
            check_budgets(bad)


# ---- the study's figures on planted results -----------------------------------------------------------------------------------
def planted():
    """3 budgets, 4 cases, 5 frames: frame 1 an empty dump, frame 3 carried by every case; the spread of ransac_height halves with
    every budget; refined values NaN for case 2 of frame 2 (a degenerate pair) and for every case of frame 4."""
    from mvoscalerecovery_amd import height_pitch as hp
    sw = hp.RansacBudgetSweep.__new__(hp.RansacBudgetSweep)
    sw.model, sw.cases, sw.budgets = "plane", 4, (10, 20, 40)
    B, Cn, n = 3, 4, 5
    dev = np.array([-3.0, -1.0, 1.0, 3.0])                                          # population std sqrt(5)
    res = {k: np.zeros((B, Cn, n)) for k in hp.RESULT_FIELDS}
    for k, scale in enumerate((0.4, 0.2, 0.1)):
        for i, w in ((0, 1.0), (2, 2.0), (4, 3.0)):
            for f in hp.RESULT_FIELDS:
                res[f][k, :, i] = 1.7 + scale * w * dev
        for f in hp.RESULT_FIELDS:
            res[f][k, :, 3] = res[f][k, :, 2]                                        # the carried frame repeats its predecessor
    for f in he.REFINED:
        res[f][:, 2, 2] = np.nan
        res[f][:, 2, 3] = np.nan
        res[f][:, :, 4] = np.nan
    sw.results = res
    sw.carried = np.array([False, False, False, True, False])
    sw.degenerate = np.isnan(res["refined_mean"])
    used = np.zeros((B, Cn, n), np.int32)
    for k, b in enumerate(sw.budgets):
        used[k][:, [0, 2, 4]] = b
    used[1:, 0, 0] = 15                                                              # one pair stopped at 15: before budgets 20 and 40
    used[2, 1, 4] = 33
    sw.used, sw.best = used, np.where(used > 0, 3, -1).astype(np.int32)
    return sw


def test_table_spread_and_smallest_budget_on_planted_results():
    sw = planted()
    s5 = np.sqrt(5.0)
    t = sw.table()
    assert [r["budget"] for r in t] == [10, 20, 40]
    for r, scale in zip(t, (0.4, 0.2, 0.1)):                                         # the fitted frames are 0, 2, 4: weights 1, 2, 3
        assert r["mean_std"] == pytest.approx(scale * s5 * 2.0, rel=1e-12) and r["max_std"] == pytest.approx(scale * s5 * 3.0, rel=1e-12)
    assert [r["mean_used"] for r in t] == [10.0, pytest.approx((11 * 20 + 15) / 12), pytest.approx((10 * 40 + 15 + 33) / 12)]
    assert [r["stopped_share"] for r in t] == [0.0, pytest.approx(1 / 12), pytest.approx(2 / 12)]
    # refined values: the degenerate pair is left out of frame 2's figure, frame 4 (all NaN) out of the means over the frames
    tr = sw.table("refined_mean")
    three = np.std(np.array([-3.0, -1.0, 3.0]))
    assert tr[0]["mean_std"] == pytest.approx(0.4 * (s5 + 2.0 * three) / 2, rel=1e-12) and tr[0]["max_std"] == pytest.approx(0.4 * 2.0 * three, rel=1e-12)
    assert np.isfinite([r["mean_std"] for r in tr]).all()
    sp = sw.spread()
    assert set(sp) == set(sw.results) and sp["ransac_height"][0].shape == (3, 5) and sp["ransac_height"][1].shape == (3, 5)
    np.testing.assert_allclose(sp["ransac_height"][0][:, [0, 2, 3, 4]], 1.7, rtol=1e-12)
    assert not sp["ransac_height"][1][:, 1].any() and np.isnan(sp["refined_pitch"][1][:, 4]).all()
    np.testing.assert_allclose(sp["refined_std"][1][:, 2], np.array([0.4, 0.2, 0.1]) * 2.0 * three, rtol=1e-12)
    # the mean spreads are 0.8, 0.4, 0.2 (x sqrt 5): only the last lies within 10 % of the last, the last two within 100 % (and a rounding)
    assert sw.smallest_budget() == 40 and sw.smallest_budget(within=0.99) == 40 and sw.smallest_budget(within=1.01) == 20
    assert sw.smallest_budget(within=2.99) == 20 and sw.smallest_budget(within=3.01) == 10
    assert sw.smallest_budget("refined_mean", within=1.01) == 20
    at = sw.results_at(20)
    assert set(at) == set(sw.results) and all(np.array_equal(at[k], sw.results[k][1], equal_nan=True) for k in at)
    with pytest.raises(ValueError):
        sw.results_at(30)
    sw.results = None
    for call in (sw.table, sw.spread, sw.smallest_budget, lambda: sw.results_at(20), lambda: sw.write_results(".", "00", "x")):
        with pytest.raises(RuntimeError):
            call()


# ---- the checkpoints ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", he.MODELS)
def test_reference_decides_every_checkpoint_and_the_cut_replay_is_the_uncut(model):
    cr = he.crafted()
    n = 0
    for name, budgets in hb.BUDGETS.items():
        s = cr[name]
        assert budgets[-1] <= s.positions.shape[1] and list(budgets) == sorted(set(budgets)), name
        for c in range(s.positions.shape[0]):
            full = hb.ref_at(model, s, c, budgets[-1])
            cut = hb.cut_replay(full["hyp_counts"], s.M, budgets)
            bests = []
            for k, b in enumerate(budgets):
                ref = hb.ref_at(model, s, c, b)
                assert ref["decided"], (name, c, b)                                  # none may be left out
                n += 1
                assert np.array_equal(ref["hyp_counts"], full["hyp_counts"][:b]), (name, c, b)    # the run at b is the first b hypotheses
                assert (ref["best"], ref["best_ic"], ref["used"]) == fc.replay(full["hyp_counts"][:b], s.M, he.GOAL) == cut[k], (name, c, b, cut[k])
                assert (ref["status"] == he.ST_RS_FEW) == (ref["best"] < 0) and (ref["best"] >= 0 or ref["used"] == b), (name, c, b)
                bests.append(ref["best"])
            assert bests == sorted(bests), (name, c, bests)                          # the best's number only grows with the budget
    assert n == hb.N_COMBINATIONS // 2


def test_the_lists_hold_what_they_are_for():
    """50 checkpoints without a model; checkpoints of one case with different best models; a goal stop between checkpoints."""
    cr = he.crafted()
    few = 0
    for model in he.MODELS:
        for name, budgets in hb.BUDGETS.items():
            s = cr[name]
            few += sum(hb.ref_at(model, s, c, b)["status"] == he.ST_RS_FEW for c in range(s.positions.shape[0]) for b in budgets)
        g = [hb.ref_at(model, cr["goal_late"], 0, b) for b in hb.BUDGETS["goal_late"]]
        assert [r["best"] for r in g] == [-1, -1, 7, 7, 7, 7, 7, 512] and [r["used"] for r in g] == list(hb.BUDGETS["goal_late"])
        b2 = [hb.ref_at(model, cr["best_second_tile"], 0, b)["best"] for b in hb.BUDGETS["best_second_tile"]]
        assert b2 == [-1, -1, 3, 3, 3, 512]                                          # the best moves in the second tile
        b1 = [hb.ref_at(model, cr["best_first_tile"], 0, b)["best"] for b in hb.BUDGETS["best_first_tile"]]
        assert b1 == [-1, -1, 3, 3, 3, 3]
        sp = [hb.ref_at(model, cr["spent"], 0, b)["best"] for b in hb.BUDGETS["spent"]]
        assert sp[:6] == [-1] * 6 and sp[6] == 6                                     # six spent samples, then a model
        dg = [hb.ref_at(model, cr["degenerate"], 0, b) for b in hb.BUDGETS["degenerate"]]
        assert dg[0]["status"] == he.ST_DEGENERATE
        many = {tuple(hb.ref_at(model, cr["cases10"], c, b)["best"] for b in hb.BUDGETS["cases10"]) for c in range(10)}
        assert len(many) > 1 and any(len(set(m)) > 2 for m in many)                  # several distinct best models within a case
    assert few == hb.N_RS_FEW
    # a stop inside a segment: the state freezes, `used` repeats
    counts = np.array([0, 2, 0, 9, 1, 9, 10, 3])
    assert hb.cut_replay(counts, 10, (2, 3, 5, 8)) == [(1, 2, 2), (1, 2, 3), (3, 9, 4), (3, 9, 4)]
    assert hb.cut_replay(counts, 12, (2, 3, 5, 8)) == [(1, 2, 2), (1, 2, 3), (3, 9, 5), (6, 10, 7)]
