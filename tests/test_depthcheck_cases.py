"""CPU: the restatement of mvosr_depth_check_batch (tests/depthcheck_cases.py) against the reference's own run
(tests/golden/depthcheck.npz); the plan header's binning against np.histogram through a stand-alone program; the C ABI's new entry
and struct; ``data_check``'s host side; the crafted frames' own premises."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depthcheck_cases as dcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference/script/data_check.py"


@pytest.fixture(scope="module")
def golden():
    return dcc.golden()


@pytest.fixture(scope="module")
def crafted():
    return dcc.crafted()


@pytest.fixture(scope="module")
def restated(crafted):
    return {name: dcc.depth_check_of(*case) for name, case in crafted.items()}


def _golden_frame(golden, pre, i):
    return {k: golden[pre + k][i] for k in ("hist", "below", "above", "nan", "max", "n")}


# ---- the restatement against the reference's run -----------------------------------------------------------------------------------
def test_restatement_equals_the_reference_on_the_crafted_frames(golden, crafted, restated):
    assert int(golden["c_crc"]) == dcc.checksum(crafted), "the crafted frames drifted from the fixture"
    names = [str(k) for k in golden["c_names"]]
    assert names == [k for k, (y, _, lv) in crafted.items() if np.count_nonzero(np.asarray(y) > 0) and not np.any(lv > 2)]
    assert len(names) >= len(crafted) - 2
    for i, name in enumerate(names):
        want = dict(_golden_frame(golden, "c_", i), status=0)
        assert dcc.same(restated[name], want), name
        assert np.array_equal(golden["c_raised"][i], golden["c_n"][i] == 0), name


def test_restatement_equals_the_reference_on_the_sequence(golden):
    from mvoscalerecovery_amd import synth
    seq = dcc.sequence_points()
    assert int(golden["s_crc"]) == synth.checksum(*[np.ascontiguousarray(a) for fr in seq for a in fr])
    assert len(seq) == 60 and golden["s_hist"].shape == (60, 3, dcc.N_BINS)
    for i, fr in enumerate(seq):
        r = dcc.depth_check_of(*fr)
        assert dcc.same(r, dict(_golden_frame(golden, "s_", i), status=r["status"])), i
        assert r["status"] == (0 if golden["s_n"][i, 0] else dcc.ST_NO_POINT)
    n0 = golden["s_n"][:, 0]
    sizes = np.array([len(fr[0]) for fr in seq])
    share = golden["s_hist"][:, 0].sum(1)[sizes > 3] / (n0[sizes > 3] ** 2)
    assert share.min() >= 0.5 and np.count_nonzero(golden["s_hist"][:, 0].sum(0)) == dcc.N_BINS


@pytest.mark.reference
def test_the_reference_itself_where_it_is_present(golden, crafted):
    if not os.path.isfile(REFERENCE):
        pytest.skip("reference not present")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_depthcheck", os.path.join(ROOT, "tests", "golden", "make_golden_depthcheck.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    mod = gen.load_reference()
    for i, name in enumerate(str(k) for k in golden["c_names"]):
        y, z, lv = crafted[name]
        if len(y) > 600:
            continue
        for p in range(3):
            r = gen.reference_depth_check(mod, np.asarray(y, dtype=np.float64)[lv >= p], np.asarray(z, dtype=np.float64)[lv >= p])
            assert np.array_equal(r["hist"], golden["c_hist"][i, p]) and dcc.same_floats([r["max"]], [golden["c_max"][i, p]]), (name, p)
            assert (r["below"], r["above"], r["nan"], r["n"]) == tuple(int(golden["c_" + k][i, p]) for k in ("below", "above", "nan", "n"))


# ---- the plan header's binning on the host -------------------------------------------------------------------------------------------
BIN_PROGRAM = r"""
#include "mvosr_depthcheck_plan.hpp"
#include <cstdio>
#include <cstring>
using namespace mvosr;
int main() {
    unsigned long long bits;
    while (std::scanf("%llx", &bits) == 1) {
        double q;
        std::memcpy(&q, &bits, 8);
        std::printf("%d\n", depthcheck_slot(q));
    }
    std::printf("plan %d %d %d %d %d %d\n", kDcBins, kDcSlots, kDcRows, kDcTile, kDcCopies, kDcLdsBytes);
    const DepthCheckGrid a = depthcheck_grid(512, 2000, 256), b = depthcheck_grid(1, 2000, 256), c = depthcheck_grid(1, 20000, 256), d = depthcheck_grid(3, 0, 256);
    std::printf("grid %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)a.row_blocks, (long long)a.j_split, (long long)b.row_blocks, (long long)b.j_split,
                (long long)c.row_blocks, (long long)c.j_split, (long long)d.row_blocks, (long long)d.j_split);
    return 0;
}
"""


def test_plan_header_bins_like_numpy(tmp_path):
    src, exe = tmp_path / "bins.cpp", tmp_path / "bins"
    src.write_text(BIN_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "mvoscalerecovery_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    e = dcc.BINS.astype(np.float64)
    rng = np.random.default_rng(59)
    vals = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [0.0, -0.0, np.inf, -np.inf, np.nan],
                           [np.finfo(np.float64).max, -np.finfo(np.float64).max, np.finfo(np.float64).tiny, -np.finfo(np.float64).tiny,
                            5e-324, -5e-324],
                           rng.uniform(-2100.0, 1050.0, 8000), rng.standard_cauchy(2000) * 300.0])
    assert vals.size >= 10000 + 3 * 60
    text = "\n".join("%x" % b for b in vals.view(np.uint64)) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = np.array([int(v) for v in out[:vals.size]])
    finite = ~np.isnan(vals)
    want = np.full(vals.size, dcc.N_BINS + 2)
    want[finite & (vals < e[0])] = dcc.N_BINS
    want[finite & (vals > e[-1])] = dcc.N_BINS + 1
    inside = finite & (vals >= e[0]) & (vals <= e[-1])
    for k in np.nonzero(inside)[0]:                              # np.histogram on one value at a time: the bin it counts it in
        want[k] = int(np.argmax(np.histogram(vals[k:k + 1], dcc.BINS)[0]))
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    counts = np.bincount(got[inside], minlength=dcc.N_BINS)
    assert np.array_equal(counts, np.histogram(vals[inside], dcc.BINS)[0])
    assert got[list(vals).index(950.0)] == 58 and got[60 * 3 + 1] == 40 and got[60 * 3] == 40       # the closing edge; -0.0 and 0.0
    rows, tile = dcc.plan()
    plan = [int(v) for v in out[vals.size].split()[1:]]
    assert plan[:4] == [dcc.N_BINS, dcc.WORDS, rows, tile] and plan[5] == tile * 20 + 3 * dcc.WORDS * plan[4] * 4 + 16 <= 40 * 1024
    grid = [int(v) for v in out[vals.size + 1].split()[1:]]
    assert grid[0] == 8 and grid[1] == 1                         # 512 frames fill the device by themselves
    assert grid[2] == 8 and grid[3] == 4                         # one frame of 2000: every tile its own workgroup
    assert grid[4] == 79 and 79 * grid[5] >= 1024 and grid[5] <= 40    # one frame of 20 000 spans over a thousand workgroups
    assert grid[6] == 0 and grid[7] == 1


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported():
    from mvoscalerecovery_amd import _lib
    assert "mvosr_depth_check_batch" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "mvosr.h")) as fh:
        header = fh.read()
    m = re.search(r"int mvosr_depth_check_batch\(([^;]*)\);", header)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["ctx", "n_frames", "off", "cnt", "y", "z", "level", "params", "outputs", "tables"]
    assert len(_lib.SYMBOLS["mvosr_depth_check_batch"][1]) == 10
    assert _lib.ABI_VERSION == 13 and re.search(r"#define MVOSR_ABI_VERSION 13\b", header)            # additive: the number stays
    assert re.search(r"#define MVOSR_DC_BINS %d\b" % dcc.N_BINS, header) and _lib.DC_BINS == dcc.N_BINS
    assert re.search(r"#define MVOSR_DC_TABLE_WORDS %d\b" % dcc.WORDS, header) and _lib.DC_TABLE_WORDS == dcc.WORDS
    assert re.search(r"#define MVOSR_ST_DC_NO_POINT %d\b" % dcc.ST_NO_POINT, header) and _lib.ST_DC_NO_POINT == dcc.ST_NO_POINT
    used = [int(v) for v in re.findall(r"MVOSR_ST_[A-Z_]+ = (\d+)", header)]
    assert dcc.ST_NO_POINT not in used and len(used) >= 12      # a status word the header did not use
    with open(os.path.join(ROOT, "mvoscalerecovery_amd", "csrc", "Makefile")) as fh:
        mk = fh.read()
    assert "mvosr_depthcheck.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    assert "mvosr_depthcheck_plan.hpp" in re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1)
    lib = _lib.load()
    assert lib.mvosr_abi_version() == 13
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mvosr_depth_check_batch\b", exported)


def test_structs_match_the_header(tmp_path):
    from mvoscalerecovery_amd import _lib
    structs = {"mvosr_depth_check_params": _lib.DepthCheckParams, "mvosr_depth_check_outputs": _lib.DepthCheckOutputs}
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
    assert C.sizeof(_lib.DepthCheckParams) == 8 and C.sizeof(_lib.DepthCheckOutputs) == 56


def test_bad_arguments_are_refused_before_any_gpu_work():
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    p, o = _lib.DepthCheckParams(4, 0), _lib.DepthCheckOutputs()
    assert lib.mvosr_depth_check_batch(None, 1, None, None, None, None, None, C.byref(p), C.byref(o), None) == -2
    assert b"depth_check" in lib.mvosr_last_error()


# ---- data_check's host side ---------------------------------------------------------------------------------------------------------
def test_argument_validation():
    from mvoscalerecovery_amd import data_check as D
    pts = np.arange(12.0).reshape(4, 3)
    a, lv = D.check_points([pts, pts[:2]])
    assert [l.tolist() for l in lv] == [[2, 2, 2, 2], [2, 2]] and a[0].dtype == np.float64
    a, lv = D.check_points([pts], [[0, 1, 2, 1]])
    assert lv[0].dtype == np.uint8 and lv[0].tolist() == [0, 1, 2, 1]
    for bad in ([np.zeros(5)], [np.zeros((5, 2))], [np.zeros((2, 3, 3))]):
        with pytest.raises(ValueError):
            D.check_points(bad)
    for levels in ([[0, 1, 2]], [[0, 1, 2, 1], [0]], [[0, 1, 2, 3]], [[0, 1, 2, -1]], [np.zeros((4, 1), int)]):
        with pytest.raises(ValueError):
            D.check_points([pts], levels)
    assert np.array_equal(D.BINS, np.array(range(-40, 20)) * 50) and D.BINS.size == 60
    e = D.concatenate([])
    assert e.hist.shape == (0, 3, 59) and e.status.shape == (0,) and e.errors == {}


def test_profiles_and_cloud_on_plain_arrays():
    from mvoscalerecovery_amd import data_check as D
    pts = np.array([[1.0, 0.5, 10.0], [2.0, 0.0, 11.0], [3.0, 1.9, 12.0], [4.0, 2.0, 13.0], [5.0, 9.9, 14.0], [6.0, 10.0, 15.0],
                    [7.0, -1.0, 16.0], [8.0, np.nan, 17.0]])
    z, h = D.road_profile(pts)
    assert z.tolist() == [10.0, 12.0, 13.0, 14.0] and h.tolist() == [-0.5, -1.9, -2.0, -9.9]
    z, h = D.road_profile(pts, y_max=2.0)
    assert z.tolist() == [10.0, 12.0]
    x, z, h = D.road_cloud(pts)
    assert x.tolist() == [1.0, 3.0] and z.tolist() == [10.0, 12.0] and h.tolist() == [-0.5, -1.9]
    assert D.road_cloud(pts, y_max=11.0)[0].tolist() == [1.0, 3.0, 4.0, 5.0, 6.0]


def test_batch_record_and_tables_on_plain_arrays(restated):
    from mvoscalerecovery_amd import data_check as D
    names = ["selected2", "none_selected", "beyond"]
    rs = [restated[k] for k in names]
    res = D.DepthCheckBatch(*(np.stack([np.asarray(r[k]) for r in rs]) for k in D.FIELDS), {})
    assert np.array_equal(res.tables(), dcc.table_of(rs)) and res.tables().shape == (3, 62)
    one = res.frame(2, 1)
    assert one.n == int(rs[2]["n"][1]) and np.array_equal(one.hist, rs[2]["hist"][1]) and one.bins is D.BINS
    assert one.hist.sum() + one.below + one.above + one.nan == one.n ** 2
    assert callable(D.compare) and callable(D.depth_check) and callable(D.depth_check_batch)


def test_estimator_entry_points_exist():
    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator
    for name in ("depth_check_batch", "depth_check", "depth_check_tables", "reset_depth_check"):
        assert callable(getattr(ScaleEstimator, name, None)), name


# ---- the crafted frames' premises -------------------------------------------------------------------------------------------------------
def test_crafted_frames_hold_what_they_are_named_for(crafted, restated):
    rows, tile = dcc.plan()
    sel = lambda name: int(np.count_nonzero(crafted[name][0] > 0))
    assert [sel("selected%d" % n) for n in (0, 1, 2, 63, 64, 65)] == [0, 1, 2, 63, 64, 65]
    assert all(len(crafted["selected%d" % n][0]) == n + 5 for n in (0, 1, 2, 63, 64, 65))
    for n in (rows - 1, rows, rows + 1, tile - 1, tile, tile + 1, 2 * tile + 1):
        assert sel("plan%d" % n) == n and restated["plan%d" % n]["n"][0] == n
    assert sel("synthetic2100") == 2100 and len(crafted["synthetic2100"][0]) == 2137
    for r in restated.values():
        assert np.array_equal(r["hist"].sum(1) + r["below"] + r["above"] + r["nan"], r["n"] ** 2)
    # the edges: the forward pair sits on the edge, to the bit
    for k, e in enumerate(dcc.EDGE_VALUES):
        y, z, _ = crafted["edge%d" % k]
        assert (y[0], z[0]) == dcc.EDGE_FIRST and dcc.slope((y[0], z[0]), (y[1], z[1])) == e
        back = dcc.slope((y[1], z[1]), (y[0], z[0]))
        assert back != e and abs(back - e) < 1.0
        h = restated["edge%d" % k]["hist"][2]
        want = np.zeros(59, np.int64)
        want[40] += 2                                            # the diagonal
        want[min(int((e + 2000) // 50), 58)] += 1
        outside = back < dcc.BINS[0] or back > dcc.BINS[-1]     # (the reverse pair of the last edge may lie just above it)
        if not outside:
            want[int(np.searchsorted(dcc.BINS, back, side="right")) - 1] += 1
        assert np.array_equal(h, want), (e, back)
        r = restated["edge%d" % k]
        assert int(r["below"][2] + r["above"][2]) == int(outside) and r["nan"][2] == 0
    # equal depths: +0.0 and -0.0 off the diagonal, both counted in the bin of 0
    y, z, _ = crafted["equal_depths"]
    a, b = dcc.slope((y[0], z[0]), (y[1], z[1])), dcc.slope((y[1], z[1]), (y[0], z[0]))
    assert a == 0 and b == 0 and np.signbit(a) != np.signbit(b) and restated["equal_depths"]["hist"][0][40] == 5
    assert restated["equal_depths"]["max"][0] > 0
    r = restated["duplicate"]
    assert r["hist"][0][40] >= 9 and r["n"].tolist() == [4, 4, 3]          # the three copies among themselves: 9 zero slopes
    r = restated["depth_zero"]
    assert r["nan"].tolist() == [1, 1, 1] and np.isnan(r["max"]).all() and r["hist"][0][40] >= 2 + 4
    r = restated["depth_negative"]
    assert r["status"] == 0 and r["n"].tolist() == [4, 3, 2] and not np.isnan(r["max"]).any()
    r = restated["unselected"]
    assert r["n"].tolist() == [3, 2, 1] and r["status"] == 0
    r = restated["none_selected"]
    assert r["status"] == dcc.ST_NO_POINT and not r["hist"].any() and np.isnan(r["max"]).all() and not r["n"].any()
    assert restated["selected0"]["status"] == dcc.ST_NO_POINT
    r = restated["beyond"]
    assert r["below"][0] > 0 and r["above"][0] > 0
    r = restated["population2_empty"]
    assert r["n"].tolist() == [70, 35, 0] and np.isnan(r["max"][2]) and not r["hist"][2].any() and r["status"] == 0
    r = restated["population1_is_0"]
    assert np.array_equal(r["hist"][0], r["hist"][1]) and r["n"][0] == r["n"][1] > r["n"][2] > 0
    r = restated["endpoint_lower"]
    assert r["n"].tolist() == [3, 2, 1] and r["hist"].sum(1).tolist() == [9, 4, 1]
    # the largest frame lands in many bins, and the populations differ
    r = restated["synthetic2100"]
    assert np.count_nonzero(r["hist"][0]) == 59 and r["n"][0] > r["n"][1] > r["n"][2] > 0
