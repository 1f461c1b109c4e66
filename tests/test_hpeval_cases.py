"""CPU: the RANSAC evaluation's references and plumbing (tests/hpeval_cases.py).

* the NumPy restatement of /root/reference/src/calculate_height_pitch_eval.py and calculate_height_pitch_eval_line.py replays the
  scripts' own runs (tests/golden/hpeval.npz, written by tests/golden/make_golden_hpeval.py): every integer of every (frame, case)
  pair exactly, the RANSAC height to rtol 1e-9, the model to rtol 1e-8 / atol 1e-12; the four refined lists within max(16 gap, 1e-12)
  of the gaps the generator measured, on every fitted pair that is not flagged degenerate; the carry, the empty dump and the
  first-frame exception included, and the type of the exception that ends each script;
* the np.longdouble reference DECIDES every integer, sign and flag of every crafted scene for both models, and the float64
  restatement lies within its bounds; the scenes have the shapes tests/test_gpu_hpeval.py relies on;
* the documented draw sequence;
* the LDS plan (csrc/mvosr_hpeval_plan.hpp), compiled with g++ into a stand-alone program: an accepted frame lies inside the request,
  every region aligned to 16, no two overlapping, the request growing with every size but not with n_hyp beyond a tile; the
  binding's structs have the header's layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heightpitch_cases as hc
import hpeval_cases as he
from conftest import ROOT

CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")


@pytest.fixture(scope="module")
def golden():
    return he.load_golden()


def replay(model, g):
    """-> per case the list of per-frame dicts (None for an empty dump)"""
    out = []
    n_cases = g["positions"][[i for i, p in enumerate(g["positions"]) if p is not None][0]].shape[0]
    for c in range(n_cases):
        prev, rs = None, []
        for i, d in enumerate(g["frames"]):
            if not len(d):
                rs.append(None)
                continue
            pos = g["positions"][i][c] if g["positions"][i] is not None else None
            prev = he.restate(model, d, g["rows"][i], g["priors"][i], pos, prev)
            rs.append(prev)
        out.append(rs)
    return out


@pytest.mark.parametrize("model", he.MODELS)
@pytest.mark.parametrize("case", ["seq", "carry", "empty"])
def test_restatement_replays_the_scripts_runs(golden, model, case):
    g = golden[model][case]
    assert g["run"]["error"] == ("TypeError" if model == "plane" else None)          # the plane script's last line, after its sixty files
    rss = replay(model, g)
    compared = fitted = 0
    for c, rs in enumerate(rss):
        for i, r in enumerate(rs):
            if r is None:
                assert all(g[k][c, i] == 0 for k in he.FIELDS)                       # the empty dump: six zeros
                continue
            assert r["n_selected"] == g["suitable"][i] and r["n_inliers"] == int(g["n_inliers"][c, i]), (c, i)
            np.testing.assert_allclose(r["ransac_height"], g["ransac_height"][c, i], rtol=1e-9, atol=0)
            if not r["carried"]:
                assert r["best_ic"] == int(g["best_ic"][i][c]) and np.array_equal(r["list_mask"], g["mask"][i][c]), (c, i)
                np.testing.assert_allclose(r["model"], g["model"][i][c], rtol=1e-8, atol=1e-12)
            fitted += 1
            if r["degenerate"]:
                continue
            compared += 1
            for k in he.REFINED:
                tol = max(16 * g["run"]["gaps"]["gap_" + k], 1e-12)
                assert abs(r[k] - g[k][c, i]) <= tol * abs(g[k][c, i]), (k, c, i, r[k], g[k][c, i], tol)
    assert (fitted, compared) == (g["run"]["fitted_pairs"], g["run"]["compared_pairs"])
    assert compared >= (0.9 if model == "line" else 0.6) * fitted
    if case == "carry":
        for rs in rss:
            assert [r["carried"] for r in rs] == [False, True, False]
            assert rs[1]["ransac_height"] == rs[0]["ransac_height"] and rs[1]["n_inliers"] == rs[0]["n_inliers"]
            assert rs[1]["height_t_mean_script"] != rs[0]["height_t_mean_script"]    # (the new prior, :223)
    if case == "seq" and model == "line":
        assert np.any(g["ransac_height"] < 0)                                        # the line's sign rule reads b: reproduced, not repaired


@pytest.mark.parametrize("model", he.MODELS)
def test_first_frame_with_too_few_points_raises_what_the_scripts_raise(golden, model):
    g = golden[model]["first"]
    assert g["run"]["error"] == "IndexError" and not g["run"]["files"]
    with pytest.raises(IndexError):
        he.restate(model, g["frames"][0], g["rows"][0], g["priors"][0], None, None)


@pytest.mark.parametrize("model", he.MODELS)
def test_the_sixty_file_names(golden, model):
    from mvoscalerecovery_amd import height_pitch as hp
    m = golden["meta"]
    for case in ("seq", "carry", "empty"):
        run = golden[model][case]["run"]
        names = hp.eval_file_names(model, m["input_id"], m["input_date"], golden[model][case]["meta"]["iterations"], m["n_cases"])
        assert len(names) == 60 and sorted(names) == run["files"] and not run["stray"]
    assert any(n.endswith(".txt.txt") for n in names) and all("result_heights_plane_ransac_" in n for n in names[0::6])


def test_reference_decides_the_pinned_frames(golden):
    for model in he.MODELS:
        g = golden[model]["seq"]
        for i, c in ((0, 0), (7, 9)):
            ref = he.reference(model, g["frames"][i], g["rows"][i], g["priors"][i], g["positions"][i][c])
            assert ref["decided"], (model, i, c)
            assert ref["n_selected"] == g["suitable"][i] and ref["n_inliers"] == int(g["n_inliers"][c, i])
            assert ref["best_ic"] == int(g["best_ic"][i][c]) and np.array_equal(ref["list_mask"], g["mask"][i][c])
            he.within(he.restate(model, g["frames"][i], g["rows"][i], g["priors"][i], g["positions"][i][c]), ref, (model, i, c))


@pytest.mark.parametrize("model", he.MODELS)
def test_reference_decides_every_crafted_scene(model):
    cases = he.crafted()
    K = he.K_of(model)
    ref = {}
    for name, s in cases.items():
        if name in he.NO_REF:
            continue
        for c in range(s.positions.shape[0]):
            r = he.ref_for(model, s, c)
            assert r["decided"], (name, c)
            if r["n_selected"] >= he.MIN_POINTS:
                he.within(he.restate(model, s.pts, s.rows, s.est, s.positions[c]), r, (name, c))
        ref[name] = he.ref_for(model, s, 0)
    assert cases["min12"].M == 12 and ref["min12"]["status"] == 0 and cases["few9"].M == 9 and ref["few9"]["status"] == he.ST_RS_FEW    # :159
    assert [cases["words%d" % m].M for m in (189, 192, 195)] == [189, 192, 195]
    assert [cases["chunk%d" % m].M for m in (4092, 4095, 4098)] == [4092, 4095, 4098]      # (a list has 3 entries per row)
    assert ref["goal_late"]["used"] == 513 and 0 < ref["goal_late"]["best_ic"] > 0.8 * cases["goal_late"].M
    assert he.ref_for(model, cases["goal_late"], 0)["hyp_counts"][7] > 0
    assert ref["best_first_tile"]["best"] == 3 and ref["best_first_tile"]["used"] == 513 and ref["best_first_tile"]["hyp_counts"][512] > 0
    assert ref["best_second_tile"]["best"] == 512 and ref["best_second_tile"]["hyp_counts"][3] > 0
    assert ref["h1"]["used"] == 1 and ref["tile512"]["used"] == 512
    M = cases["inliers_last"].M
    assert np.nonzero(ref["inliers_last"]["list_mask"])[0].tolist() == [M - 3, M - 2, M - 1]
    assert np.nonzero(ref["inliers_first"]["list_mask"])[0].tolist() == [0, 1, 2]
    first = np.nonzero(ref["straddle"]["list_mask"])[0][:K]
    assert first[0] == 191 and first[1] == 192 and len(cases["straddle"].rows) <= 512       # row 63 is wavefront 0's last, row 64 wavefront 1's first
    assert not ref["straddle"]["degenerate"] and ref["degenerate"]["degenerate"] and ref["degenerate"]["status"] == he.ST_DEGENERATE
    assert ref["degenerate"]["n_inliers"] > K
    assert not ref["spent"]["hyp_counts"][:6].any() and ref["spent"]["hyp_counts"][6] > 0
    assert (ref["neg"]["ransac_height"] < 0) == (model == "line") and ref["neg"]["model"][1] > 0 and ref["mix60"]["ransac_height"] > 0
    some = [he.ref_for(model, cases["cases10"], c) for c in range(10)]
    assert len({r["best"] for r in some}) > 1                                               # the cases differ
    with pytest.raises(np.linalg.LinAlgError):
        s = cases["singular"]
        hc.select(hc.back_project(s.pts), s.rows.astype(np.int64), s.est)


def test_line_restatement_is_the_oracles_svd_line():
    """The closed-form line against the null vector estimate_line asks an SVD for, on a crafted scene's list."""
    s = he.crafted()["mix60"]
    P = hc.back_project(s.pts)
    v = he.vertex_samples("line", s.ids, s.positions[0])
    m = he.models_from("line", P, v)
    for vv, mm in zip(v[:20], m[:20]):
        if np.isnan(mm[0]):
            continue
        A = np.ones((2, 3))
        A[:, :2] = P[vv][:, 1:3]
        sv = np.linalg.svd(A)[-1][-1, :]
        sv = sv if sv[np.argmax(np.abs(sv))] * mm[[0, 1, 3]][np.argmax(np.abs(sv))] > 0 else -sv
        np.testing.assert_allclose(mm[[0, 1, 3]], sv, rtol=0, atol=1e-9)


def test_device_draw_restatement():
    tri = he.draw_positions("plane", 77, 5, 2, 500, 36)
    assert tri.min() >= 0 and tri.max() < 36
    assert np.all((tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2]))
    pair = he.draw_positions("line", 77, 5, 2, 500, 36)
    assert np.array_equal(pair[:, :2], tri[:, :2]) and np.all(pair[:, 2] == -1) and np.all(pair[:, 0] != pair[:, 1])
    assert not np.array_equal(tri, he.draw_positions("plane", 77, 5, 3, 500, 36))          # another case, another sequence
    assert not np.array_equal(tri, he.draw_positions("plane", 77, 6, 2, 500, 36))
    assert not np.array_equal(tri, hc.draw_positions(77, 5, 500, 36))                       # (not the single-run estimator's either)
    assert len(np.unique(tri)) == 36
    # a prefix property the tiles rely on: hypothesis h does not depend on n_hyp
    assert np.array_equal(he.draw_positions("plane", 77, 5, 2, 600, 36)[:500], tri)


# ---- the LDS plan ----------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "mvosr_hpeval_plan.hpp"
using namespace mvosr;
static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
struct Region { const char *name; size_t off, bytes; };
static size_t frame_end(long long n, long long tn, long long h) {
    const HpEvalPlan<uint32_t> p = hpeval_plan<uint32_t>((uint32_t)n, (uint32_t)tn, (uint32_t)h);
    const HpEvalPlan<size_t> q = hpeval_plan<size_t>((size_t)n, (size_t)tn, (size_t)h);
    CHECK(p.x == q.x && p.y == q.y && p.z == q.z && p.list == q.list && p.mods == q.mods && p.cnts == q.cnts && p.words == q.words &&
          p.misc == q.misc && p.red == q.red && p.total == q.total, "32-bit and size_t plans differ (%lld %lld %lld)", n, tn, h);
    const size_t tile = (size_t)(h < kHpMaxHyp ? h : kHpMaxHyp);
    const std::vector<Region> r = {{"x", q.x, 8u * (size_t)n}, {"y", q.y, 8u * (size_t)n}, {"z", q.z, 8u * (size_t)n}, {"list", q.list, 6u * (size_t)tn},
        {"mods", q.mods, (size_t)kHpPlaneBytes * tile}, {"cnts", q.cnts, 4u * tile}, {"words", q.words, 8u * ((3u * (size_t)tn + 63) / 64)},
        {"misc", q.misc, 4u * HE_N}, {"red", q.red, 8u * HER_N}};
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % 16 == 0, "%s at %zu (%lld %lld %lld)", r[i].name, r[i].off, n, tn, h);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j)
            CHECK(!r[i].bytes || !r[j].bytes || r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s overlaps %s (%lld %lld %lld)",
                  r[i].name, r[j].name, n, tn, h);
    }
    CHECK(end <= q.total, "plan ends at %zu, total %zu", end, q.total);
    return end;
}
int main(int argc, char **argv) {
    static_assert(HM_CW + kHpWaves <= HE_N && HM_I0 + 3 <= HE_DONE && HE_DEGEN < HM_CW && HER_MODEL + 4 <= HER_N &&
                  HER_YZ == HER_SUM + 2 * kHpWaves && HER_DEV == HER_YZ + 2 * kHpWaves && HER_MODEL == HER_DEV + 2 * kHpWaves, "slots");
    static_assert(kHpeMaxHyp % kHpMaxHyp == 0, "tiles");
    if (argc == 3) { const long long mf = atoll(argv[1]); printf("%zu\n", hpeval_plan<size_t>(mf, mf ? 2 * mf : 1, atoll(argv[2])).total); return 0; }
    const long long hyps[6] = {1, 65, 500, 512, 513, 4096};
    for (long long h : hyps)
        for (long long mf = 0; mf <= 70; ++mf) {
            const long long mt = mf ? 2 * mf : 1;                       // what the launcher asks for
            const size_t total = hpeval_plan<size_t>(mf, mt, h).total;
            for (long long n = 0; n <= mf; ++n)
                for (long long tn = 0; tn <= mt; ++tn)
                    CHECK(frame_end(n, tn, h) <= total, "frame (%lld, %lld) leaves the request of header %lld, n_hyp %lld", n, tn, mf, h);
        }
    for (long long mf : {255ll, 256ll, 2000ll, 2001ll, 10922ll}) { frame_end(mf, 2 * mf, 500); frame_end(mf, 2 * mf, 4096); }
    // one tile is all the hypotheses ever take
    CHECK(hpeval_plan<size_t>(2000, 4000, 512).total == hpeval_plan<size_t>(2000, 4000, 4096).total, "the request grows beyond a tile");
    CHECK(hpeval_plan<size_t>(2000, 4000, 511).total < hpeval_plan<size_t>(2000, 4000, 512).total, "the request does not grow up to a tile");
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("hpeval_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_accepted_frames_lie_inside_the_request_aligned_and_disjoint(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failed", r.stdout + r.stderr


def test_lds_request_is_the_plans_total_and_fits_a_cu(plan_exe):
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    for mf, h in ((0, 1), (3, 64), (300, 513), (2000, 500), (2000, 4096)):
        want = int(subprocess.run([plan_exe, str(mf), str(h)], capture_output=True, text=True, check=True).stdout)
        for model in (_lib.HP_MODEL_PLANE, _lib.HP_MODEL_LINE):
            assert int(lib.mvosr_height_pitch_eval_lds_bytes(mf, h, model)) == want
    assert lib.mvosr_height_pitch_eval_lds_bytes(2000, 500, 0) == 92080                # DESIGN 3.15's figure
    assert lib.mvosr_height_pitch_eval_lds_bytes(2000, 4096, 0) <= 96 * 1024


def test_binding_matches_the_header(tmp_path):
    from mvoscalerecovery_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvosr.h")).read()
    assert re.search(r"\bint mvosr_height_pitch_eval_batch\(", header) and len(_lib.SYMBOLS["mvosr_height_pitch_eval_batch"][1]) == 6
    assert re.search(r"#define MVOSR_ABI_VERSION 13\b", header) and _lib.ABI_VERSION == 13   # the change is additive
    assert re.search(r"#define MVOSR_ST_HP_REFINE_DEGENERATE 0x100\b", header) and _lib.ST_HP_REFINE_DEGENERATE == he.ST_DEGENERATE == 0x100
    structs = {"mvosr_height_pitch_eval_params": _lib.HeightPitchEvalParams, "mvosr_height_pitch_eval_outputs": _lib.HeightPitchEvalOutputs}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvosr.h"', 'int main(void) {',
           'printf("plane %d\\nline %d\\n", (int)MVOSR_HP_MODEL_PLANE, (int)MVOSR_HP_MODEL_LINE);']
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
    assert (int(got["plane"]), int(got["line"])) == (_lib.HP_MODEL_PLANE, _lib.HP_MODEL_LINE)
    for st, cls in structs.items():
        assert int(got[st]) == C.sizeof(cls), st
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)
