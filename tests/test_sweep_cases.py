"""CPU: the constants of rescale.RescaleConstants and the sweep's infrastructure.

* tests/sweep_cases.py's NumPy estimator with constants reproduces tests/golden/sweep.npz — the reference's own rescale.py with
  one setting's literals substituted, run through main_offline.py's loop (tests/golden/make_golden_sweep.py) — for every setting:
  the point lists, the fits' inlier counts and iterations exactly, levels and scales to 1e-9.  (On this sequence `min_points30`
  changes nothing — its shortest list has 387 entries — and `loose-75` moves levels and lists but no scale, the slew limiter
  being active; the device tests add settings that bite there.)
* the crafted frames of tests/test_gpu_sweep.py are what they claim.
* flat_selection_sweep_kernel's LDS plan (csrc/mvosr_rescale_sweep_plan.hpp), compiled with g++: alignment, no overlap of regions
  live together, carved <= requested, the maximum of n_sel, and the Python cap on a frame's points.
* RescaleConstants, ConstantSweep.grid, and ConstantSweep's bookkeeping with a stub in place of the device.
"""
import dataclasses
import json
import os
import subprocess
import types

import numpy as np
import pytest

import flat_cases as fc
import sweep_cases as sw
from conftest import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvoscalerecovery_amd", "csrc")


# ---- the golden ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    z, meta = load_npz("sweep.npz")
    return z, meta, sw.golden_sequence()


def test_golden_inputs_and_settings(golden):
    from mvoscalerecovery_amd import rescale
    z, meta, data = golden
    assert meta["crc"] == sw.sequence_checksum(data) and meta["sequence"] == sw.SEQUENCE and meta["sample_seed"] == sw.SAMPLE_SEED
    assert meta["settings"] == [[name, sw.setting(i)] for i, (name, _) in enumerate(sw.SETTINGS)]
    assert sw.DEFAULTS == dataclasses.asdict(rescale.RescaleConstants())
    moved = [kw for _, kw in sw.SETTINGS]
    for want in ({}, {"loose_deg": -75.0}, {"tight_deg": -88.0}, {"height_factor": 0.8}, {"height_factor": 1.0}, {"threshold": 0.003},
                 {"threshold": 0.01}, {"n_hyp": 30}, {"ransac_min_points": 30}, {"slew": 0.2}):
        assert want in moved
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sweep.npz")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "rescale.npz"))
    for i in range(len(sw.SETTINGS)):                               # the recorded samples are the generator's sequence
        t = z["s%d_triples" % i]
        lens = np.diff(z["s%d_ids_off" % i])[z["s%d_ran" % i]]
        assert t.shape == (len(lens), sw.setting(i)["n_hyp"], 3)
        for call in (0, len(lens) - 1):
            assert np.array_equal(t[call], sw.sample_triples(sw.SAMPLE_SEED, call, int(lens[call]), t.shape[1]))


@pytest.mark.parametrize("i", range(len(sw.SETTINGS)), ids=[n for n, _ in sw.SETTINGS])
def test_numpy_estimator_with_constants_reproduces_the_patched_reference(golden, i):
    from mvoscalerecovery_amd import offline
    z, meta, data = golden
    est = sw.SweepOracle(meta["abs_ref"], meta["window"], sw.SETTINGS[i][1], sw.recorded_sampler(z, i))
    out = offline.run_sequence(data, est)
    off = z["s%d_ids_off" % i]
    assert len(est.calls) == len(off) - 1
    for c, rec in enumerate(est.calls):
        assert np.array_equal(rec["ids"], z["s%d_ids" % i][off[c]:off[c + 1]]), c
        np.testing.assert_allclose(rec["height_level"], z["s%d_height_level" % i][c], rtol=1e-9)
    assert np.array_equal(["best_ic" in r for r in est.calls], z["s%d_ran" % i])
    assert np.array_equal([r["best_ic"] for r in est.calls if "best_ic" in r], z["s%d_best_ic" % i])
    assert np.array_equal([r["used"] for r in est.calls if "best_ic" in r], z["s%d_used" % i])
    np.testing.assert_allclose(out["scales"], z["s%d_scales" % i], rtol=1e-9)


def test_golden_settings_move_what_they_should(golden):
    z = golden[0]
    name = {n: i for i, (n, _) in enumerate(sw.SETTINGS)}
    same = lambda key, a: np.array_equal(z["s%d_%s" % (name[a], key)], z["s0_" + key])
    assert not same("height_level", "loose-75") and not same("ids", "loose-75")
    assert same("height_level", "tight-88") and not same("ids", "tight-88") and not same("scales", "tight-88")
    for n in ("factor0.8", "factor1.0"):
        assert not same("height_level", n) and not same("ids", n) and not same("scales", n)
    for n in ("threshold0.003", "threshold0.01"):
        assert same("ids", n) and not same("best_ic", n) and not same("scales", n)
    assert same("ids", "n_hyp30") and z["s%d_used" % name["n_hyp30"]].max() == 30 and z["s0_used"].max() > 30 and not same("scales", "n_hyp30")
    assert same("ids", "slew0.2") and same("best_ic", "slew0.2") and not same("scales", "slew0.2")


# ---- the crafted frames' design -----------------------------------------------------------------------------------------------------
def _pitch(frame):
    hk, _ = fc.numpy_flat(frame)
    P, tri = frame.survivors(), frame.tri[~frame.skip]
    n = np.linalg.solve(P[tri], np.ones((len(tri), 3, 1)))[:, :, 0]
    return np.arcsin(-n[:, 1] / np.sqrt(np.sum(n * n, 1))) * 180.0 / np.pi, hk[~frame.skip]


def test_crafted_frames_are_what_they_claim():
    fam, settings = sw.crafted_frames(), sw.crafted_settings()
    assert len(settings) == 8 and any(lo < ti for lo, ti, _ in settings)                 # one inverted
    for f in fam.values():
        assert 3 <= len(f.survivors()) and len(f.tri) <= 128 and len(f.survivors()) <= 64
    pitch, _ = _pitch(fam["between"])
    assert np.any((pitch < -75.0) & (pitch > -80.0)) and np.any((pitch < -85.0) & (pitch > -88.0))
    for k in (0, 1, 2, 5, 6):
        pitch, _ = _pitch(fam["k%d" % k])
        assert int((pitch < -80.0).sum()) == k == int((pitch < -75.0).sum())
    for name, k in (("equal_even", 4), ("equal_odd", 5)):
        pitch, h = _pitch(fam[name])
        hs = np.sort(h[pitch < -80.0])
        assert len(hs) == k and hs[(k - 1) // 2] == hs[k // 2] == hs[k // 2 - 1]
    _, loose_h, level, flags = sw.flat_selection(fam["on_level"].survivors(), fam["on_level"].tri, -80.0, -85.0, 1.0)
    # (factor 1.0 and an odd k: the level IS the middle row's height, whatever the arithmetic; that row is not kept, > being strict)
    assert (flags & 2).all() and len(loose_h) == 3 and level == np.sort(loose_h)[1] and int(((flags & 4) != 0).sum()) == 1
    kw = fam["keep_words"].keep
    assert set(np.unique(kw).tolist()) == {-1, 0, 1} and len(kw) <= 64
    assert fam["bad_id"].status == fc.ST_MASK and fam["singular"].status == fc.ST_SINGULAR
    row = fam["singular"].tri[np.nonzero(fam["singular"].skip)[0][0]]
    assert abs(np.linalg.det(fam["singular"].xyz[row])) == 0.0
    # rows within 1e-12 of sin(threshold) on either side, for every threshold of the settings
    mu = []
    for f in (fam[k] for k in fam if k.startswith("near_thresholds")):
        n = np.linalg.solve(f.xyz[f.tri], np.ones((len(f.tri), 3, 1)))[:, :, 0]
        mu.append(-n[:, 1] / np.sqrt(np.sum(n * n, 1)))
    mu = np.concatenate(mu)
    for deg in sorted({s[0] for s in settings} | {s[1] for s in settings}):
        d = mu - np.sin(deg * np.pi / 180.0)
        assert np.any((d > 0) & (d <= 1e-12)) and np.any((d < 0) & (d >= -1e-12)) and np.any((np.abs(d) > 1e-12) & (np.abs(d) < 1e-8)), deg
    big = sw.big_frame()
    assert 1700 <= len(big.xyz) <= 2000 and 3300 <= len(big.tri) <= 4000 and len(big.tri) > 2 * 1024       # more than two trips of the workgroup


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include "mvosr_rescale_sweep_plan.hpp"
using namespace mvosr;

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
struct Region { const char *name; size_t off, bytes, align; unsigned live; };
#define SAME32(f) CHECK((size_t)p.f == q.f, "32-bit and size_t plans differ at " #f)

// phase 1 (bit 0): the planes are read, the heights and the bits written; phase 2 (bit 1): a histogram per wavefront
static size_t sweep_end(long long n, long long tn, long long s) {
    const SweepPlan<uint32_t> p = sweep_plan<uint32_t>(n, tn, s);
    const SweepPlan<size_t> q = sweep_plan<size_t>(n, tn, s);
    SAME32(heights); SAME32(bits); SAME32(misc); SAME32(thr); SAME32(work); SAME32(total); SAME32(work_bytes); SAME32(x); SAME32(y); SAME32(z); SAME32(hist);
    const size_t plane = 8u * (size_t)n;
    const Region r[] = {{"heights", q.heights, 8u * (size_t)tn, 8, 3u}, {"bits", q.bits, 4u * (size_t)tn, 4, 3u}, {"misc", q.misc, 4u * SM_N, 4, 3u},
                        {"thr", q.thr, 16u * (size_t)s, 8, 3u}, {"x", q.x, plane, 8, 1u}, {"y", q.y, plane, 8, 1u}, {"z", q.z, plane, 8, 1u},
                        {"hist", q.hist, 4u * (size_t)kSweepBins * kSweepWaves, 4, 2u}};
    const int R = sizeof(r) / sizeof(r[0]);
    size_t end = 0;
    for (int i = 0; i < R; ++i) {
        CHECK(r[i].off % r[i].align == 0, "%s at %zu needs %zu (n %lld tn %lld s %lld)", r[i].name, r[i].off, r[i].align, n, tn, s);
        if (r[i].off + r[i].bytes > end) end = r[i].off + r[i].bytes;
        for (int j = 0; j < i; ++j) {
            if (!(r[i].live & r[j].live) || !r[i].bytes || !r[j].bytes) continue;
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off, "%s overlaps %s (n %lld tn %lld s %lld)", r[i].name, r[j].name, n, tn, s);
        }
    }
    CHECK(q.x >= q.work && q.z + plane <= q.work + q.work_bytes && q.hist + 4u * kSweepBins * kSweepWaves <= q.work + q.work_bytes, "work area (n %lld)", n);
    CHECK(end <= q.total, "plan ends at %zu behind its total %zu (n %lld tn %lld s %lld)", end, q.total, n, tn, s);
    return end;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "total")) {                    // total <max_feat> <n_sel>: the request at max_tri = 2 max_feat
        const long long mf = atoll(argv[2]);
        printf("%zu\n", sweep_plan<size_t>(mf, 2 * mf, atoll(argv[3])).total);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "constants")) { printf("%d %d %d\n", kSweepMaxSel, kSweepWaves, kSweepBins); return 0; }
    if (argc != 2 || strcmp(argv[1], "containment")) return 2;
    CHECK(2 * kSweepMaxSel <= 32, "two bits per setting in a 32-bit word");
    CHECK(kSweepMaxSel <= 64 && SM_CW + kSweepWaves <= SM_N, "one lane per setting's thresholds, a misc slot per wavefront");
    // a frame the kernel accepts (n <= max_feat, tn <= max_tri) lies inside what the header's sizes requested
    const int NF = 70, NT = 150;
    for (long long s = 1; s <= kSweepMaxSel; s += (s < 3 ? 1 : 5))
        for (int mf = 0; mf < NF; mf += 3)
            for (int mt = 0; mt < NT; mt += 7) {
                const size_t total = sweep_plan<size_t>(mf, mt, s).total;
                for (int n = 0; n <= mf; ++n)
                    for (int tn = 0; tn <= mt; ++tn) CHECK(sweep_end(n, tn, s) <= total, "frame (%d, %d) in header (%d, %d)", n, tn, mf, mt);
            }
    for (long long n : {255ll, 256ll, 682ll, 683ll, 684ll, 2000ll, 2001ll, 3400ll, 65535ll})
        for (long long tn : {1ll, 2 * n - 5, 2 * n, 21845ll, 65534ll})
            for (long long s : {1ll, 7ll, (long long)kSweepMaxSel}) sweep_end(n, tn, s);
    printf("%ld failed\n", fails);
    return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("sweep_plan")
    src = d / "plan_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_plan_accepted_frames_lie_inside_the_request_aligned_and_disjoint(plan_exe):
    assert _run(plan_exe, "containment").strip() == "0 failed"


def test_plan_constants_and_the_library_agree(plan_exe):
    from mvoscalerecovery_amd import _lib
    max_sel, waves, bins = map(int, _run(plan_exe, "constants").split())
    assert (max_sel, waves, bins) == (16, 16, 256)                                        # the named maximum of n_sel, pinned
    lib = _lib.load()
    assert lib.mvosr_flat_selection_sweep_max_settings() == max_sel
    for mf, mt, s in ((0, 0, 1), (64, 128, 8), (2000, 0, 16), (2000, 3700, 4), (3400, 6800, 16)):
        want = int(_run(plan_exe, "total", str(mf), str(s))) if mt in (0, 2 * mf) else None
        got = lib.mvosr_flat_selection_sweep_lds_bytes(mf, mt, s)
        assert want is None or got == want
        assert got >= 12 * (mt or 2 * mf) + 24 * mf
    header = open(os.path.join(ROOT, "include", "mvosr.h")).read()
    for name in ("mvosr_flat_selection_sweep_batch", "mvosr_flat_selection_sweep_lds_bytes", "mvosr_flat_selection_sweep_max_settings"):
        assert name in header and hasattr(lib, name)
    assert _lib.ABI_VERSION == 13 and "#define MVOSR_ABI_VERSION 13" in header            # additive, as the earlier additions: the number stays


@pytest.mark.parametrize("lds_per_block", [65536, 163840])
def test_python_cap_keeps_the_sweep_plan_within_the_lds(plan_exe, lds_per_block, monkeypatch):
    from mvoscalerecovery_amd import packing, rescale
    huge = 1 << 30
    monkeypatch.setattr(packing, "delaunay_gpu_max_points", lambda: huge)
    for n_hyp in (1, 100, 512):
        est = types.SimpleNamespace(N_HYP=n_hyp, ctx=types.SimpleNamespace(lds_per_block=lds_per_block,
                                                                            lib=types.SimpleNamespace(mvosr_delaunay_lds_points=lambda: huge)))
        cap = rescale._SweepEstimator._max_points(est)
        assert 0 < cap <= rescale.ScaleEstimator._max_points(est)
        assert int(_run(plan_exe, "total", str(cap), "16")) <= lds_per_block


# ---- RescaleConstants, the grid, the bookkeeping ---------------------------------------------------------------------------------------
def test_rescale_constants_defaults_and_ranges():
    from mvoscalerecovery_amd import rescale
    k = rescale.RescaleConstants()
    assert (k.loose_deg, k.tight_deg, k.height_factor) == (-80.0, -85.0, 0.9) == k.selection()
    assert k.ransac() == (rescale.RANSAC_MIN_POINTS, rescale.RANSAC_ITERATIONS, rescale.RANSAC_THRESHOLD, rescale.RANSAC_GOAL) == (12, 100, 0.005, 0.8)
    assert k.slew == rescale.SLEW == 0.3
    assert rescale.RescaleConstants(loose_deg=-80, n_hyp=np.int64(100)) == k and hash(rescale.RescaleConstants()) == hash(k)
    with pytest.raises(dataclasses.FrozenInstanceError):
        k.slew = 0.2
    for bad in ({"loose_deg": -91}, {"tight_deg": 95.0}, {"loose_deg": float("nan")}, {"height_factor": -0.1}, {"ransac_min_points": 2},
                {"n_hyp": 0}, {"n_hyp": 513}, {"n_hyp": 30.5}, {"threshold": 0.0}, {"goal_fraction": -1.0}, {"slew": 0.0}, {"slew": float("inf")},
                {"threshold": "0.005"}):
        with pytest.raises(ValueError):
            rescale.RescaleConstants(**bad)
    assert rescale.RescaleConstants(loose_deg=-86.0, tight_deg=-82.0).selection() == (-86.0, -82.0, 0.9)          # inverted is legal
    with pytest.raises(TypeError):
        rescale.ScaleEstimator(1.75, constants={"slew": 0.2})


def test_grid_is_a_product():
    from mvoscalerecovery_amd import rescale
    g = rescale.ConstantSweep.grid(loose_deg=[-80, -75], n_hyp=[100, 30], slew=0.2)
    assert [(k.loose_deg, k.n_hyp, k.slew) for k in g] == [(-80.0, 100, 0.2), (-80.0, 30, 0.2), (-75.0, 100, 0.2), (-75.0, 30, 0.2)]
    assert all(k.tight_deg == -85.0 for k in g)
    with pytest.raises(TypeError):
        rescale.ConstantSweep.grid(good_bits=[1])


class _StubSweepEstimator:
    """In place of the inner estimator: no device; the library's host functions only."""
    sampling, triangulation = "device", "scipy"

    def __init__(self, *a, constants=None, **kw):
        from mvoscalerecovery_amd import _lib
        self._frame_counter, self.constants = 0, constants
        self.ctx = types.SimpleNamespace(lib=_lib.load())


def test_constant_sweep_shares_launches_and_carries_tails(monkeypatch, tmp_path):
    """With stubbed per-frame results: which configs share a selection and a (selection, RANSAC) pair, that slew and window cost
    nothing but a tail, that row [k, c] is the tail of RepeatedRuns fed the same raw scales, continuation, and the file names."""
    from mvoscalerecovery_amd import offline, rescale
    from test_repeats_cases import _toy_dict
    monkeypatch.setattr(rescale, "_SweepEstimator", _StubSweepEstimator)
    K = rescale.RescaleConstants
    configs = [K(), K(slew=0.2), K(n_hyp=30), K(loose_deg=-75.0), K(loose_deg=-75.0, threshold=0.01), K(height_factor=1.0, slew=0.1)]
    sweep = rescale.ConstantSweep(1.75, configs, window_size=5, cases=3, seed=9)
    assert sweep.seeds == rescale.case_seeds(9, 3) and sweep.max_settings == 16
    assert sweep._sels == [(-80.0, -85.0, 0.9), (-75.0, -85.0, 0.9), (-80.0, -85.0, 1.0)]
    assert sweep._pair_of == [0, 0, 1, 2, 3, 4] and [p[0] for p in sweep._pairs] == [0, 0, 1, 1, 2]
    assert [k.n_hyp for k in sweep._pair_constants] == [100, 30, 100, 100, 100] and sweep._pair_constants[3].threshold == 0.01
    data = _toy_dict()
    kinds = offline.plan_sequence(data)
    rng = np.random.default_rng(3)

    def fake_raw(f3, f2):
        F, k0 = len(f3), sweep.estimator._frame_counter
        raw = 1.0 + rng.uniform(0.0, 2.0, (5, 3, 64))[:, :, k0:k0 + F]
        status = np.zeros((5, 3, F), np.int32)
        if k0 == 0:
            raw[:, :, 3], status[:, :, 3] = np.nan, fc.ST_RS_FEW
        return {"raw_scale": raw, "status": status, "height_level": np.ones((3, F)), "n_kept": np.ones((3, F), np.int32),
                "frame_status": np.zeros(F, np.int32), "host_errors": {}}
    monkeypatch.setattr(sweep, "_raw_cases", fake_raw)
    cut = 8
    parts = [{k: v[:cut] for k, v in data.items()}, {k: v[cut:] for k, v in data.items()}]
    outs = [sweep.run(p) for p in parts]
    scales, raw = sweep.scales(), np.concatenate([o["raw_scale"] for o in outs], axis=2)
    assert scales.shape == (6, 3, 14) and raw.shape == (6, 3, 10) and outs[0]["error"].shape == (6, 3, cut + 1)
    assert np.array_equal(raw[0], raw[1], equal_nan=True) and not np.array_equal(raw[0], raw[2], equal_nan=True)   # slew shares the raw scales, n_hyp does not
    assert not np.array_equal(scales[0], scales[1])
    for k, cfg in enumerate(configs):                                # the reference's recurrence on the same raw scales (rescale.py:169-178)
        for c in range(3):
            s, q, want = 1, [], []
            for r in raw[k, c]:
                if not np.isnan(r):
                    s = s + cfg.slew if r - s > cfg.slew else (s - cfg.slew if r - s < -cfg.slew else r)
                q = (q + [s])[-5:]
                want.append(np.median(q))
            full, _ = offline.assemble_outputs(kinds, want, [1] * len(want))
            assert np.array_equal(scales[k, c], full[1:]), (k, c)
    names = sweep.write_results(str(tmp_path) + "/seq_", "t")
    assert sorted(os.path.basename(n) for n in names) == sorted(os.listdir(tmp_path)) and len(names) == 2 * 6 * 3
    assert np.array_equal(np.loadtxt(str(tmp_path / "seq_scales.txttk4_2")), scales[4, 2])
    with pytest.raises(ValueError):
        sweep.table("tra_mean")                                      # no scores yet
    sweep.last_scores = {"trimmed": {"tra_mean": np.array([3.0, 2.0, np.nan, 1.5, 2.5, 1.5]), "rot_mean": np.arange(6.0)}}
    assert sweep.best("tra_mean") is configs[3] and sweep.best("rot_mean") is configs[0]
    table = sweep.table("tra_mean")
    assert [row["config"] for row in table] == list(range(6)) and table[1]["slew"] == 0.2 and table[3]["tra_mean"] == 1.5
    with pytest.raises(ValueError):
        sweep.best("speed")
    with pytest.raises(ValueError):
        rescale.ConstantSweep(1.75, [], cases=3)
    with pytest.raises(TypeError):
        rescale.ConstantSweep(1.75, configs, cases=3, constants=K())
