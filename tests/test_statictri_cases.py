"""CPU: the restatement of road_model_calculation_static_tri (tests/statictri_cases.py) against the reference's own run
(tests/golden/statictri.npz): the crafted lists, the 600 random lists and the 60-frame sequence with its carried frames; the C ABI's
new entry; the estimator's ``model`` keyword, refused without a device."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import statictri_cases as stc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope="module")
def bound():
    """Everything here is about mvosr_static_tri_batch: without the entry there is nothing to state."""
    from mvoscalerecovery_amd import _lib
    assert "mvosr_static_tri_batch" in _lib.SYMBOLS
    return _lib


@pytest.fixture(scope="module")
def golden():
    return stc.golden()


@pytest.fixture(scope="module")
def crafted():
    return stc.crafted()


def _same_as_golden(z, pre, i, h):
    want = {"scale_norm": z[pre + "_scale"][i], "raw_scale": np.float64(z[pre + "_scale"][i]) * np.float64(stc.ABS_REF),
            "status": int(z[pre + "_status"][i]), "n_used": len(h), "hist": z[pre + "_hist"][i]}
    return stc.same(stc.static_tri_of(h), want)


# ---- (a) the crafted lists ---------------------------------------------------------------------------------------------------------
def test_crafted_lists_are_the_goldens(golden, crafted):
    assert list(golden["c_names"]) == list(crafted)
    assert int(golden["c_crc"]) == stc.checksum(list(crafted.values())), "the crafted lists drifted from the fixture"


def test_restatement_equals_the_reference_on_every_crafted_list(golden, crafted):
    for i, (name, h) in enumerate(crafted.items()):
        if len(h) == 0:
            assert np.isnan(golden["c_scale"][i]) and stc.static_tri_of(h)["status"] == stc.ST_RS_FEW      # np.median([]) is NaN
            continue
        assert _same_as_golden(golden, "c", i, h), name


def test_crafted_lists_take_the_exits_they_are_named_for(golden, crafted):
    r = {name: stc.static_tri_of(h) for name, h in crafted.items()}
    scale = lambda name: float(r[name]["scale_norm"])
    assert r["all_ones"]["status"] == stc.ST_MEDIAN and not r["all_ones"]["hist"].any()
    assert r["max2"]["status"] == stc.ST_MEDIAN and r["max2"]["hist"].max() == 2 and r["max3"]["status"] == stc.ST_MODE
    for name in ("median_odd", "median_even", "median_above", "median_above_even", "median_repeats"):
        assert r[name]["status"] == stc.ST_MEDIAN, name
    assert len(crafted["median_odd"]) % 2 == 1 and len(crafted["median_even"]) % 2 == 0
    s = np.sort(1.0 / crafted["median_even"])
    assert s[7] != s[8] and scale("median_even") == (s[7] + s[8]) / 2                       # the two middle values are unequal
    assert scale("median_above") > 1.9 and scale("median_above_even") > 1.9                 # most values lie outside the bins
    assert scale("plateau2") == 0.45 and scale("plateau3") == 0.8
    assert scale("max_bin0") == 0.1 and scale("max_bin0_1") == 0.15 and scale("max_bin18") == 1.9
    assert scale("first_run_not_max") == 0.4                                                # not the run that holds the maximum (1.1)
    assert (scale("rel32"), scale("rel33"), scale("rel34")) == (1.1, 0.3, 0.3)              # 0.33 * 100 rounds to 33.0
    assert scale("runs_k_k2") == 0.5 and scale("local_max_2") == 0.3 and scale("local_max_2_low") == 0.9
    assert r["n13"]["status"] == stc.ST_MODE and stc.static_tri_of(crafted["n12"], min_count=12)["status"] == stc.ST_RS_FEW
    assert stc.static_tri_of(crafted["n13"], min_count=12)["status"] == stc.ST_MODE


def test_edge_values_land_where_the_builder_says():
    ev = stc.edge_values()
    assert {k for k, _, _, _ in ev} == set(range(1, 20))
    for k, side, h, hi in ev:
        assert np.float64(1.0) / h == hi and (hi < stc.EDGES[k], hi == stc.EDGES[k], hi > stc.EDGES[k]) == (side < 0, side == 0, side > 0)
        want = (k - 1 if side < 0 else k) if k < 19 else (18 if side <= 0 else -1)
        assert stc.bin_of(float(hi)) == want, (k, side)
    assert stc.EDGES[3] == 0.30000000000000004 and all(int(e * 10) == k for k, e in enumerate(stc.EDGES))
    assert np.array_equal(np.array(stc.EDGES), np.array(range(0, 20)) * 0.1)


def test_invalid_heights_are_refused_in_the_restatement():
    for name, h in stc.refused().items():
        r = stc.static_tri_of(h)
        assert r["status"] == stc.ST_ERR_MASK and np.isnan(r["scale_norm"]) and not r["hist"].any(), name


# ---- (b) the random lists ----------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_on_the_random_lists(golden):
    lists = stc.random_lists()
    assert len(lists) == stc.N_RANDOM == len(golden["r_scale"]) and int(golden["r_crc"]) == stc.checksum(lists)
    st = golden["r_status"]
    assert int((st == stc.ST_MODE).sum()) >= 20 and int((st == stc.ST_MEDIAN).sum()) >= 20
    bad = [i for i, h in enumerate(lists) if not _same_as_golden(golden, "r", i, h)]
    assert not bad, bad[:10]


# ---- (c) the sequence --------------------------------------------------------------------------------------------------------------
def test_carry_rule_reproduces_the_sequence(golden):
    n = golden["s_n_heights"]
    assert len(n) == stc.N_SEQUENCE and int((n <= 12).sum()) >= 3
    tri = golden["s_tri"]
    few = np.nonzero(n <= 12)[0]
    assert few[0] > 0 and all(tri[f] == tri[f - 1] for f in few)                            # a short frame returns the scale as it stands
    # every other frame is a mode or a median of inverse heights times the reference height
    norm = tri / stc.ABS_REF
    status = np.where(n <= 12, stc.ST_RS_FEW, stc.ST_MODE)
    assert stc.carry(np.where(n <= 12, np.nan, tri), status).tobytes() == tri.tobytes()
    assert np.all(norm > 0.5) and np.all(norm < 2.5)
    assert np.isfinite(golden["s_static"]).all() and len(golden["s_static"]) == stc.N_SEQUENCE


# ---- the C ABI and the estimator's keyword -------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_bound(bound):
    with open(os.path.join(ROOT, "include", "mvosr.h")) as fh:
        header = fh.read()
    m = re.search(r"int mvosr_static_tri_batch\(([^;]*)\);", header)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["ctx", "n_lists", "off", "cnt", "height", "flags", "min_count", "absolute_reference", "scale_norm", "raw_scale", "n_used",
         "hist", "status"]
    assert len(bound.SYMBOLS["mvosr_static_tri_batch"][1]) == 13
    assert bound.ABI_VERSION == 13 and re.search(r"#define MVOSR_ABI_VERSION 13\b", header)
    with open(os.path.join(ROOT, "mvoscalerecovery_amd", "csrc", "Makefile")) as fh:
        assert "mvosr_statictri.hip" in re.search(r"^SRCS\s*=(.*)$", fh.read(), re.M).group(1)


def test_model_keyword_is_refused_before_any_device(monkeypatch):
    from mvoscalerecovery_amd import rescale

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(rescale, "ScaleEngine", no_device)
    monkeypatch.setattr(rescale.packing, "start_pool", no_device)
    for model in ("static_tri", "static"):
        with pytest.raises(ValueError, match="staged path"):
            rescale.ScaleEstimator(1.75, 5, triangulation="gpu", model=model)
        with pytest.raises(ValueError, match="staged path"):
            rescale.ScaleEstimator(1.75, 5, sampling="device", model=model)
        with pytest.raises(ValueError, match="staged path"):
            rescale.ScaleEstimator(1.75, 5, triangulation="scipy", sampling="device", model=model)
    with pytest.raises(ValueError, match="model must be"):
        rescale.ScaleEstimator(1.75, 5, model="tri")
    with pytest.raises(ValueError, match="model must be"):
        rescale.ScaleEstimator(1.75, 5, triangulation="scipy", model=None)
