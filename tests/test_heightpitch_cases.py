"""CPU: the height-and-pitch estimator's references and plumbing (tests/heightpitch_cases.py).

* the NumPy restatement of /root/reference/src/calculate_height_pitch.py replays the script's own run (tests/golden/heightpitch.npz,
  written by tests/golden/make_golden_heightpitch.py): integers exactly, heights to rtol 1e-9, the model to rtol 1e-8 / atol 1e-12, the
  four refined lists within max(16 gap, 1e-12) of the gaps the generator measured; the carry and the first-frame exception included;
* the np.longdouble reference DECIDES every integer of every pinned and crafted frame, and the float64 restatement lies within
  its bounds;
* `estimated_pitches` is the script's get_pitch, bit for bit;
* the LDS plan (csrc/mvosr_heightpitch_plan.hpp), compiled with g++ into a stand-alone program: an accepted frame lies inside the
  request, every region aligned, no two overlapping; the binding's structs have the header's layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heightpitch_cases as hc
from conftest import ROOT

CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")
LISTS = (("refined_camera_height_means", "refined_mean"), ("refined_camera_height_stds", "refined_std"),
         ("refined_camera_height_t_means", "height_t_mean"), ("refined_pitchs", "refined_pitch"))


@pytest.fixture(scope="module")
def golden():
    return hc.load_golden()


def _replay(g):
    prev, out = None, []
    for i in range(g["meta"]["n_results"]):
        prev = hc.restate(g["frames"][i], g["rows"][i], g["priors"][i], g["positions"][i], prev)
        out.append(prev)
    return out


@pytest.mark.parametrize("case", ["seq", "carry"])
def test_restatement_replays_the_scripts_run(golden, case):
    g = golden[case]
    rs = _replay(g)
    assert len(rs) == len(g["frames"]) and g["meta"]["error"] is None
    assert [r["n_selected"] for r in rs] == g["suitable"].tolist()
    assert [r["n_inliers"] for r in rs] == g["inlier_numbers"].astype(int).tolist()
    np.testing.assert_allclose([r["ransac_height"] for r in rs], g["ransac_camera_heights"], rtol=1e-9, atol=0)
    for i, r in enumerate(rs):
        if g["positions"][i] is None:
            assert r["carried"] and r["n_selected"] < hc.MIN_POINTS
            continue
        assert r["best_ic"] == int(g["best_ic"][i]) and np.array_equal(r["mask"], g["mask"][i])
        np.testing.assert_allclose(r["model"], g["model"][i], rtol=1e-8, atol=1e-12)
    for key, field in LISTS:
        tol = max(16 * g["meta"]["gaps"]["gap_" + field], 1e-12)
        got = np.array([r[field] for r in rs])
        assert np.all(np.abs(got - g[key]) <= tol * np.abs(g[key])), (key, np.max(np.abs(got - g[key]) / np.abs(g[key])), tol)
    if case == "carry":
        assert [r["carried"] for r in rs] == [False, True, False]
        assert rs[1]["ransac_height"] == rs[0]["ransac_height"] and rs[1]["refined_pitch"] == rs[0]["refined_pitch"]
        assert rs[1]["height_t_mean"] != rs[0]["height_t_mean"]                       # (the new prior, :202)


def test_first_frame_with_too_few_points_raises_what_the_script_raises(golden):
    g = golden["first"]
    assert g["meta"]["error"] == "IndexError" and g["meta"]["n_results"] == 0 and len(g["suitable"]) == 1 and g["suitable"][0] < hc.MIN_POINTS
    with pytest.raises(IndexError):
        hc.restate(g["frames"][0], g["rows"][0], g["priors"][0], None, None)


def test_estimated_pitches_are_get_pitch_bit_for_bit(golden):
    from mvoscalerecovery_amd import estimate_road_norm, height_pitch
    motions = hc.motions
    for case, g in golden.items():
        mot = motions(g["meta"]["motion_seed"], len(g["frames"]) + 2)
        assert hc.crc(mot) == g["meta"]["motion_crc"]
        ts = mot[:, 3::4]
        n = len(g["priors"])
        got = height_pitch.estimated_pitches(ts, 1, n)
        assert np.array_equal(got, g["priors"]), case
        assert got[-1] == estimate_road_norm.get_pitch(ts[0:n + 1, 0:3])
    assert height_pitch.frame_prior(0.01) == hc.prior_of(0.01)
    with pytest.raises(IndexError):
        height_pitch.estimated_pitches(np.zeros((3, 3)), 1, 3)


def _within(r, ref, name):
    """the float64 restatement against the long-double reference and its bounds"""
    assert r["n_selected"] == ref["n_selected"] and np.array_equal(r["ids"], ref["ids"]), name
    if ref["status"] != 0:
        return
    assert np.array_equal(r["hyp_counts"], ref["hyp_counts"]), name
    assert (r["best"], r["best_ic"], r["used"]) == (ref["best"], ref["best_ic"], ref["used"]), name
    assert np.array_equal(r["mask"], ref["mask"]) and r["n_inliers"] == ref["n_inliers"], name
    assert np.all(np.abs(r["model"] - ref["model"]) <= ref["model_tol"]), name
    assert abs(r["ransac_height"] - ref["ransac_height"]) <= ref["ransac_height_tol"] * abs(ref["ransac_height"]), name
    for k in ("refined_pitch", "refined_mean", "refined_std", "height_t_mean"):
        assert abs(r[k] - ref[k]) <= ref[k + "_tol"], (name, k, r[k], ref[k], ref[k + "_tol"])
    assert np.all(np.abs(r["refined_normal"] - ref["refined_normal"]) <= ref["refined_normal_tol"]), name


def test_reference_decides_the_pinned_frames(golden):
    g = golden["seq"]
    for i in (0, 5, 11):                                                  # (the smallest, a middle and the largest frame: 60 s for all twelve)
        ref = hc.reference(g["frames"][i], g["rows"][i], g["priors"][i], g["positions"][i])
        assert ref["decided"], i
        assert ref["n_selected"] == g["suitable"][i] and ref["n_inliers"] == int(g["inlier_numbers"][i])
        assert ref["best_ic"] == int(g["best_ic"][i]) and np.array_equal(ref["mask"], g["mask"][i])
        _within(hc.restate(g["frames"][i], g["rows"][i], g["priors"][i], g["positions"][i]), ref, i)
        assert abs(ref["refined_pitch"] - g["refined_pitchs"][i]) <= ref["refined_pitch_tol"] + 16 * g["meta"]["gaps"]["gap_refined_pitch"]


SKIP_REF = ("empty", "singular", "badid")


def test_reference_decides_every_crafted_frame():
    cases = hc.crafted()
    for name, f in cases.items():
        if name in SKIP_REF:
            continue
        ref = hc.reference(f.pts, f.rows, f.est, f.positions)
        assert ref["decided"], name
        if ref["n_selected"] >= hc.MIN_POINTS:
            _within(hc.restate(f.pts, f.rows, f.est, f.positions), ref, name)
    ref = {k: hc.reference(cases[k].pts, cases[k].rows, cases[k].est, cases[k].positions) for k in cases if k not in SKIP_REF}
    assert ref["one_row"]["n_selected"] == 3 and ref["rows3"]["n_selected"] == 9 and ref["rows4"]["n_selected"] == 12      # :140
    assert ref["rows3"]["status"] == hc.ST_RS_FEW and ref["rows4"]["status"] == 0
    assert len(cases["tail65"].pts) == 65 and len(cases["tail129"].pts) == 129 and len(cases["big300"].pts) == 300
    kept = np.nonzero(ref["big300"]["keep"])[0]
    assert kept.min() < 64 <= kept.max() and len(cases["big300"].rows) % 64                                                # kept rows on both sides of a wavefront's segment
    assert ref["neg_height"]["n_selected"] == 15
    q = ref["neg_height"]["rows_q"]
    assert np.sum((q["height"] < 0) & (q["pitch"] < -85.5)) == 2                          # in the window, excluded by height > 0 (:112)
    for deg, n_edge in ((-2, 2), (0, 2), (2, 2), (6, 4)):
        f, r = cases["prior%+d" % deg], ref["prior%+d" % deg]
        lo, hi = hc.prior_of(f.est)[:2]
        q = r["rows_q"]
        near = np.minimum(np.abs(q["pitch"] - lo), np.abs(q["pitch"] - hi)) < 1e-6
        assert near.sum() == n_edge and r["keep"][near].sum() == n_edge // 2, (deg, near.sum())
        assert r["n_selected"] == 3 * (5 + n_edge // 2)
    assert ref["tie"]["hyp_counts"].tolist() == [3, 3, 3] and ref["tie"]["best"] == 0 and ref["tie"]["used"] == 3
    assert ref["goal0"]["used"] == 1 and ref["goal0"]["best_ic"] == 18
    assert ref["never"]["used"] == len(cases["never"].positions)
    assert ref["spent"]["n_selected"] == 21 and not ref["spent"]["hyp_counts"][:6].any() and ref["spent"]["best"] >= 6
    assert ref["three"]["n_inliers"] == 3
    assert np.nonzero(ref["wave0"]["mask"])[0][:3].tolist() == [3, 10, 40] and np.nonzero(ref["spread"]["mask"])[0][:3].tolist() == [1, 70, 260]
    with pytest.raises(np.linalg.LinAlgError):
        f = cases["singular"]
        hc.select(hc.back_project(f.pts), f.rows.astype(np.int64), f.est)


def test_device_draw_restatement():
    pos = hc.draw_positions(77, 5, 500, 36)
    assert pos.min() >= 0 and pos.max() < 36
    assert np.all((pos[:, 0] != pos[:, 1]) & (pos[:, 0] != pos[:, 2]) & (pos[:, 1] != pos[:, 2]))
    assert not np.array_equal(pos, hc.draw_positions(77, 6, 500, 36)) and np.array_equal(pos, hc.draw_positions(77, 5, 500, 36))
    assert len(np.unique(pos)) == 36


def test_asin_bound_near_one():
    assert hc.asin_bound(1.0, 1e-12) == pytest.approx(np.sqrt(2e-12), rel=1e-3)           # asin'(x) is unbounded at 1: the bound is not delta
    assert hc.asin_bound(0.5, 1e-12) == pytest.approx(2e-12 / np.sqrt(0.75), rel=1e-6)


# ---- the LDS plan ----------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <vector>
#include "mvosr_heightpitch_plan.hpp"
using namespace mvosr;
static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
struct Region { const char *name; size_t off, bytes; };
static size_t frame_end(long long n, long long tn, long long h) {
    const HeightPitchPlan<uint32_t> p = heightpitch_plan<uint32_t>((uint32_t)n, (uint32_t)tn, (uint32_t)h);
    const HeightPitchPlan<size_t> q = heightpitch_plan<size_t>((size_t)n, (size_t)tn, (size_t)h);
    CHECK(p.x == q.x && p.y == q.y && p.z == q.z && p.list == q.list && p.mods == q.mods && p.cnts == q.cnts && p.words == q.words &&
          p.misc == q.misc && p.red == q.red && p.total == q.total, "32-bit and size_t plans differ (%lld %lld %lld)", n, tn, h);
    const std::vector<Region> r = {{"x", q.x, 8u * (size_t)n}, {"y", q.y, 8u * (size_t)n}, {"z", q.z, 8u * (size_t)n}, {"list", q.list, 6u * (size_t)tn},
        {"mods", q.mods, (size_t)kHpPlaneBytes * (size_t)h}, {"cnts", q.cnts, 4u * (size_t)h}, {"words", q.words, 8u * (((size_t)n + 63) / 64)},
        {"misc", q.misc, 4u * HM_N}, {"red", q.red, 8u * HR_N}};
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
    static_assert(HM_CW + kHpWaves <= HM_N && HM_I0 + 3 <= HM_CW && HR_NHAT + 3 <= HR_N && HR_DEV + 2 * kHpWaves <= HR_MODEL, "slots");
    if (argc == 3) { const long long mf = atoll(argv[1]); printf("%zu\n", heightpitch_plan<size_t>(mf, mf ? 2 * mf : 1, atoll(argv[2])).total); return 0; }
    const long long hyps[4] = {1, 65, 500, 512};
    for (long long h : hyps)
        for (long long mf = 0; mf <= 70; ++mf) {
            const long long mt = mf ? 2 * mf : 1;                       // what the launcher asks for
            const size_t total = heightpitch_plan<size_t>(mf, mt, h).total;
            for (long long n = 0; n <= mf; ++n)
                for (long long tn = 0; tn <= mt; ++tn)
                    CHECK(frame_end(n, tn, h) <= total, "frame (%lld, %lld) leaves the request of header %lld, n_hyp %lld", n, tn, mf, h);
        }
    for (long long mf : {255ll, 256ll, 2000ll, 2001ll, 10922ll}) frame_end(mf, 2 * mf, 500);
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("heightpitch_plan")
    src = d / "plan_check.cpp"
    src.write_text("#include <stdlib.h>\n" + PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_accepted_frames_lie_inside_the_request_aligned_and_disjoint(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failed", r.stdout + r.stderr


def test_lds_request_is_the_plans_total_and_fits_a_cu(plan_exe):
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    for mf, h in ((0, 1), (3, 64), (300, 512), (2000, 500)):
        want = int(subprocess.run([plan_exe, str(mf), str(h)], capture_output=True, text=True, check=True).stdout)
        assert int(lib.mvosr_height_pitch_lds_bytes(mf, h)) == want
    assert lib.mvosr_height_pitch_lds_bytes(2000, 500) <= 96 * 1024            # one workgroup per CU, with room


def test_binding_matches_the_header(tmp_path):
    from mvoscalerecovery_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvosr.h")).read()
    assert re.search(r"\bint mvosr_height_pitch_batch\(", header) and len(_lib.SYMBOLS["mvosr_height_pitch_batch"][1]) == 6
    structs = {"mvosr_height_pitch_params": _lib.HeightPitchParams, "mvosr_height_pitch_outputs": _lib.HeightPitchOutputs}
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
