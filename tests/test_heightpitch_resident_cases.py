"""CPU: the device-resident path of HeightPitchEstimator — the tail's entry in the header and the binding, the LDS plan and the carry
record's layout (csrc/mvosr_heightpitch_tail_plan.hpp, compiled with g++ into a stand-alone program), and the NumPy restatement of the
tail (tests/heightpitch_tail_cases.py) against the reference's own run of the carry case (tests/golden/heightpitch.npz)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heightpitch_cases as hc
import heightpitch_tail_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")
LDS_PER_CU = 160 * 1024


def test_binding_matches_the_header(tmp_path):
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd import height_pitch as hp
    header = open(os.path.join(ROOT, "include", "mvosr.h")).read()
    assert re.search(r"\bint mvosr_height_pitch_tail_batch\(", header) and len(_lib.SYMBOLS["mvosr_height_pitch_tail_batch"][1]) == 10
    assert re.search(r"\bsize_t mvosr_height_pitch_tail_lds_bytes\(int max_feat\);", header)
    assert re.search(r"#define MVOSR_ABI_VERSION 13\b", header) and _lib.ABI_VERSION == 13   # the change is additive
    structs = {"mvosr_height_pitch_tail_frame": _lib.HeightPitchTailFrame, "mvosr_height_pitch_carry": _lib.HeightPitchCarry}
    kinds = ("SINGULAR", "MASK", "EMPTY", "NO_MODEL", "NO_PREVIOUS", "STATUS", "UPSTREAM")
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvosr.h"', 'int main(void) {']
    src += ['printf("%s %%d\\n", (int)MVOSR_HPT_ERR_%s);' % (k, k) for k in kinds]
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
    for k in kinds:
        assert int(got[k]) == getattr(_lib, "HPT_ERR_" + k) == getattr(tc, "ERR_" + k), k
    for (st, cls), dt in zip(structs.items(), (hp.TAIL_FRAME, hp.CARRY_HEADER)):
        assert int(got[st]) == C.sizeof(cls) == dt.itemsize, st
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset == dt.fields[n][1], (st, n)


# ---- the LDS plan and the carry record ----------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mvosr_heightpitch_plan.hpp"
#include "mvosr_heightpitch_tail_plan.hpp"
using namespace mvosr;
static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
struct Region { const char *name; size_t off, bytes, align; };
static size_t audit(const char *plan, const std::vector<Region> &r, long long n) {
    size_t end = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].off % r[i].align == 0, "%s.%s at %zu needs %zu (n %lld)", plan, r[i].name, r[i].off, r[i].align, n);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (size_t j = 0; j < i; ++j)
            CHECK(!r[i].bytes || !r[j].bytes || r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s.%s overlaps %s (n %lld)",
                  plan, r[i].name, r[j].name, n);
    }
    return end;
}
// every region of the tail's kernels is live from the load to the last sum: none may overlap
static size_t tail_end(long long n) {
    const HpTailPlan<uint32_t> p = hptail_plan<uint32_t>((uint32_t)n);
    const HpTailPlan<size_t> q = hptail_plan<size_t>((size_t)n);
    CHECK(p.terms == q.terms && p.node == q.node && p.misc == q.misc && p.total == q.total, "32-bit and size_t plans differ (%lld)", n);
    const size_t end = audit("tail", {{"terms", q.terms, 8u * (size_t)n, 16}, {"node", q.node, 8u * (kHptNodes + 2), 16}, {"misc", q.misc, 4u * HTM_N, 16}}, n);
    CHECK(end <= q.total, "tail plan ends at %zu, total %zu", end, q.total);
    return end;
}
static void carry(long long cap) {
    const HpCarryPlan<uint32_t> p = hpcarry_plan<uint32_t>((uint32_t)cap);
    const HpCarryPlan<size_t> q = hpcarry_plan<size_t>((size_t)cap);
    CHECK(p.y == q.y && p.z == q.z && p.index == q.index && p.total == q.total, "32-bit and size_t records differ (%lld)", cap);
    const size_t end = audit("carry", {{"header", 0, (size_t)kHptCarryHeader, 8}, {"y", q.y, 8u * (size_t)cap, 8}, {"z", q.z, 8u * (size_t)cap, 8},
                                       {"index", q.index, 4u * (size_t)cap, 4}}, cap);
    CHECK(end <= q.total && q.total % 16 == 0, "carry record ends at %zu, total %zu", end, q.total);
}
int main(int argc, char **argv) {
    static_assert(HTM_CW + kHptWaves <= HTM_FIT && HTM_FIT + kHptWaves <= HTM_ERR && HTM_ERR + 2 * kHptWaves <= HTM_N && HTM_ERR % 2 == 0, "slots");
    static_assert(kHptBlock == 64 * kHptWaves && kHptNodes <= kHptBlock, "one thread a node");
    if (argc == 3 && !strcmp(argv[1], "tail")) { printf("%zu\n", hptail_plan<size_t>(atoll(argv[2])).total); return 0; }
    if (argc == 3 && !strcmp(argv[1], "carry")) { printf("%zu\n", hpcarry_plan<size_t>(atoll(argv[2])).total); return 0; }
    if (argc == 3 && !strcmp(argv[1], "largest")) {                  // the largest frame height_pitch_kernel's plan admits in `lds` bytes, at one hypothesis
        long long n = 0;
        while (heightpitch_plan<size_t>(n + 1, 2 * (n + 1), 1).total <= (size_t)atoll(argv[2])) ++n;
        printf("%lld\n", n);
        return 0;
    }
    // a list the kernels accept (n <= carry_cap) lies inside what the launch requested at carry_cap
    for (long long cap = 0; cap <= 300; ++cap) {
        carry(cap);
        const size_t total = hptail_plan<size_t>(cap).total;
        for (long long n = 0; n <= cap; ++n) CHECK(tail_end(n) <= total, "list %lld leaves the request of capacity %lld", n, cap);
    }
    for (long long cap : {2000ll, 2001ll, 4535ll, 8191ll, 8192ll}) { carry(cap); tail_end(cap); }
    CHECK(hptail_plan<size_t>(0).misc + 4u * HTM_N <= hptail_plan<size_t>(0).total, "the resolve kernel's slots");
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("hptail_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def test_accepted_lists_lie_inside_the_request_aligned_and_disjoint(plan_exe):
    assert _run(plan_exe) == "0 failed"


def test_requests_are_the_plans_totals_and_fit_a_cu(plan_exe):
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    for n in (0, 1, 3, 300, 2000, 2001, 8192):
        assert int(lib.mvosr_height_pitch_tail_lds_bytes(n)) == int(_run(plan_exe, "tail", str(n)))
        assert int(lib.mvosr_height_pitch_carry_bytes(n)) == int(_run(plan_exe, "carry", str(n)))
    # the largest frame mvosr_height_pitch_lds_bytes admits on the device is the tail's largest list: it fits, with room
    largest = int(_run(plan_exe, "largest", str(LDS_PER_CU)))
    assert int(lib.mvosr_height_pitch_lds_bytes(largest, 1)) <= LDS_PER_CU < int(lib.mvosr_height_pitch_lds_bytes(largest + 1, 1))
    assert largest <= 8192 and int(lib.mvosr_height_pitch_tail_lds_bytes(largest)) <= LDS_PER_CU // 4


def test_carry_record_round_trip():
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd import height_pitch as hp
    rng = np.random.default_rng(0)
    inl = rng.standard_normal((7, 3))
    prev = hp.FrameResult(1.0, 2.0, 3.0, 4.0, 5.0, 7, 30, False)
    for cap in (7, 8, 301):
        rec = hp.carry_record(cap, prev, inl, np.arange(7))
        assert len(rec) == int(_lib.load().mvosr_height_pitch_carry_bytes(cap))
        h, y, z, index = hp.carry_fields(rec, cap)
        assert [h[k] for k in hp.RESULT_FIELDS] == [1.0, 2.0, 3.0, 4.0, 5.0, 7] and (h["has_prev"], h["count"], h["halted"]) == (1, 7, 0)
        assert np.array_equal(y, inl[:, 1]) and np.array_equal(z, inl[:, 2]) and index.tolist() == list(range(7))
    h = hp.carry_fields(hp.carry_record(10), 10)[0]
    assert (h["has_prev"], h["count"]) == (0, 0)


def test_pack_planes_is_pack_frames_layout():
    from mvoscalerecovery_amd import height_pitch as hp
    rng = np.random.default_rng(1)
    for sizes in ((5, 0, 2, 7, 1), (4,), (0, 0), (3, 3, 0)):
        pts = [rng.standard_normal((n, 3)) for n in sizes]
        rows = [np.zeros((0, 3), np.int32)] * len(pts)
        _, arrays, off, _, planes, _ = hp._pack_frames(pts, rows, np.zeros((len(pts), 4)))
        got, goff, gcnt = hp._pack_planes(pts)
        assert np.array_equal(got, planes) and np.array_equal(goff, off) and np.array_equal(gcnt, arrays["feat_cnt"]), sizes


def test_resident_needs_the_device_triangulation():
    from mvoscalerecovery_amd import height_pitch as hp
    with pytest.raises(ValueError, match="resident=True belongs to triangulation='gpu'"):
        hp.HeightPitchEstimator.__init__(object.__new__(hp.HeightPitchEstimator), triangulation="scipy", resident=True)


# ---- the restatement against the reference's own run --------------------------------------------------------------------------
def _chunk_from_restate(g, idx):
    """The script's float64 restatement of the golden frames `idx` as the kernel's outputs."""
    frames = []
    for i in idx:
        pts = g["frames"][i]
        try:
            r = hc.restate(pts, g["rows"][i], float(g["priors"][i]), g["positions"][i] if g["positions"][i] is not None else np.zeros((0, 3)))
        except IndexError:
            r = {"carried": True, "n_selected": int(g["suitable"][i])}
        f = {"v": pts[:, 1], "depth": pts[:, 2], "n_selected": r["n_selected"]}
        if r["carried"]:
            f.update(status=tc.ST_RS_FEW, mask=np.zeros(len(pts), bool), n_inliers=0, **{k: float("nan") for k in tc.VALUES})
        else:
            f.update(status=0, mask=r["mask"], n_inliers=r["n_inliers"], **{k: float(r[k]) for k in tc.VALUES})
        frames.append(f)
    c = {k: np.array([f[k] for f in frames]) for k in ("status", "n_selected", "n_inliers") + tc.VALUES}
    c.update({k: [f[k] for f in frames] for k in ("v", "depth", "mask")}, prior=np.array([hc.prior_of(float(g["priors"][i])) for i in idx]))
    return c


def test_restatement_replays_the_scripts_carry():
    g = hc.load_golden()["carry"]
    chunk = _chunk_from_restate(g, range(3))
    keys = {"ransac_height": "ransac_camera_heights", "refined_mean": "refined_camera_height_means", "refined_std": "refined_camera_height_stds",
            "height_t_mean": "refined_camera_height_t_means", "refined_pitch": "refined_pitchs"}
    def check(recs):
        assert [r["carried"] for r in recs] == [0, 1, 0] and [r["n_selected"] for r in recs] == g["suitable"].tolist()
        assert [r["n_inliers"] for r in recs] == g["inlier_numbers"].astype(int).tolist()
        for k in tc.COPIED:
            assert recs[1][k] == recs[0][k], k                                       # :163-165: everything repeats
        assert recs[1]["height_t_mean"] != recs[0]["height_t_mean"]                  # ... but :202-203 see the new prior
        for field, key in keys.items():
            tol = 1e-9 if field == "ransac_height" else max(16 * g["meta"]["gaps"]["gap_" + field], 1e-12)
            for i, r in enumerate(recs):
                assert abs(r[field] - g[key][i]) <= tol * abs(g[key][i]), (field, i, r[field], g[key][i])
    recs, error, out = tc.tail(chunk, tc.no_carry())
    assert error is None and not out["halted"]
    check(recs)
    # frame by frame, the carry handed on: the same records, the same carry-out
    carry, single = tc.no_carry(), []
    for i in range(3):
        one = {k: (v[i:i + 1]) for k, v in chunk.items()}
        r, error, carry = tc.tail(one, carry)
        assert error is None
        single += r
    check(single)
    assert single == recs and all(np.array_equal(carry[k], out[k]) for k in ("y", "z", "index"))
    y, z, idx = tc.inlier_yz(chunk["v"][2], chunk["depth"][2], chunk["mask"][2])
    assert np.array_equal(out["y"], y) and np.array_equal(out["z"], z) and np.array_equal(out["index"], idx)


def test_restatement_errors_in_the_host_loops_order():
    g = hc.load_golden()["carry"]
    chunk = _chunk_from_restate(g, [1, 0])                                           # a first frame with too few points (:167)
    recs, error, out = tc.tail(chunk, tc.no_carry())
    assert recs == [] and error == (0, tc.ERR_NO_PREVIOUS) and out["halted"] and not out["has_prev"]
    assert tc.tail(chunk, out) == (None, (0, tc.ERR_UPSTREAM), out)
    chunk = _chunk_from_restate(g, [0, 1, 1, 2])
    for status, n_selected, kind in ((tc.ST_SINGULAR, 0, tc.ERR_SINGULAR), (tc.ST_MASK, 0, tc.ERR_MASK), (tc.ST_EMPTY, 0, tc.ERR_EMPTY),
                                     (tc.ST_RS_FEW, 12, tc.ERR_NO_MODEL), (5, 0, tc.ERR_STATUS)):
        bad = dict(chunk, status=chunk["status"].copy(), n_selected=chunk["n_selected"].copy())
        bad["status"][2], bad["n_selected"][2] = status, n_selected
        recs, error, out = tc.tail(bad, tc.no_carry())
        assert len(recs) == 2 and recs[1]["carried"] and error == (2, kind) and out["halted"] and out["has_prev"]
        assert np.array_equal(out["index"], np.nonzero(chunk["mask"][0])[0]) and out["height_t_mean"] == recs[1]["height_t_mean"]
