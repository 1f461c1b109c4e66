"""CPU checks of the scale-score cases (tests/scalescore_cases.py) against the reference's outputs in tests/golden/scalescores.npz:
the crafted sets still come out of their seeds byte for byte; the host comparators (evaluate.evaluate_scale, patch, scale_filter)
equal the reference exactly; the NumPy restatement of the kernels' summation order equals it exactly — the proof that the order is
right before any GPU sees it —; bad arguments are refused before any device work; the new exports are declared and bound under
the same ABI number.  No GPU."""
import os
import re
import warnings

import numpy as np
import pytest

import scalescore_cases as ssc
from conftest import ROOT, load_npz

NAMES = list(ssc.SETS)


@pytest.fixture(scope="module")
def golden():
    return load_npz("scalescores.npz")[0]


@pytest.fixture(scope="module")
def sets(golden):
    out = {}
    for name in NAMES:
        out[name] = s = ssc.make_set(name)
        assert ssc.checksum(s) == int(golden[name + "_crc"]), "the generator drifted from the fixture: " + name
    return out


@pytest.mark.parametrize("name", NAMES)
def test_host_comparators_equal_the_reference(golden, sets, name):
    from mvoscalerecovery_amd import evaluate
    n, _, cases, _, _, filt = ssc.SETS[name]
    gt, scales = sets[name]["gt"], sets[name]["scales"]
    for c in range(cases):
        if golden[name + "_raises"]:
            with pytest.raises(ValueError):
                evaluate.evaluate_scale(gt, scales[c])
            continue
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            head, drift = evaluate.evaluate_scale(gt, scales[c])
        assert ssc.same(head[0], golden[name + "_mean"][c]) and ssc.same(head[1], golden[name + "_max"][c])
        assert ssc.same(head[2:], golden[name + "_within"][c]) and ssc.same(drift, golden[name + "_drift"][c])
    for w in filt:
        got = np.array([evaluate.scale_filter(scales[c], w) for c in range(cases)])
        assert ssc.same(got, golden[name + "_filter%d" % w]), (name, w)


@pytest.mark.parametrize("name", NAMES)
def test_restated_summation_order_equals_the_reference(golden, sets, name):
    n = ssc.SETS[name][0]
    r = ssc.errors_restated(sets[name]["gt"], sets[name]["scales"])
    assert ssc.same(r["mean"], golden[name + "_mean"]) and ssc.same(r["max"], golden[name + "_max"])
    assert np.array_equal(r["counts"], golden[name + "_counts"])
    assert ssc.same(r["drift"], golden[name + "_drift"])
    if n:
        assert ssc.same(1 - r["counts"] / n, golden[name + "_within"])                  # the shares, from the integers


def test_the_sets_cover_what_they_were_made_for(golden):
    seg = lambda name, w: len(range(0, ssc.SETS[name][0] - w, ssc.STEP))
    assert np.isnan(golden["n10_drift"]).all() and seg("n11", 10) == 1 and seg("n21", 10) == 2 and seg("n21", 20) == 1
    assert np.isfinite(golden["n11_drift"][:, 0]).all() and np.isnan(golden["n11_drift"][:, 1:]).all()
    assert seg("n801", 800) == 1 and seg("n811", 800) == 2 and seg("n137", 100) == 4
    assert ssc.SETS["n6000"][0] > ssc.LDS_ERRORS and seg("n83000", 10) > 8192
    assert np.isnan(golden["nan_mean"][1]) and np.isnan(golden["nan_max"][1]) and np.isfinite(golden["nan_mean"][[0, 2]]).all()
    assert np.isnan(golden["nan_drift"][1, :5]).all() and np.isfinite(golden["nan_within"]).all()
    assert np.isinf(golden["inf_mean"]).all() and np.isnan(golden["inf_drift"][2, 0]) and np.isinf(golden["inf_drift"][0, 0])
    assert (golden["cancel_drift"][:2, :5] == 0).all() and (golden["cancel_mean"] == 0.25).all()   # mixed signs cancel in every window
    assert {ssc.SETS[k][2] for k in NAMES} >= {1, 10, 11}
    # the running median: the first entry the value itself, a NaN in the window gives NaN, window 1 is the identity
    s = ssc.make_set("nan")["scales"]
    f = golden["nan_filter10"]
    assert np.array_equal(f[:, 0], s[:, 0]) and np.isnan(f[1, 123:133]).all() and np.isfinite(f[1, 133:]).all()
    assert ssc.same(golden["n21_filter1"], ssc.make_set("n21")["scales"])


def test_arguments_are_checked_before_any_device_work():
    from mvoscalerecovery_amd import evaluate
    with pytest.raises(ValueError, match="broadcast"):
        evaluate.scale_errors(np.ones(5), np.ones((2, 6)))                              # a longer re: the reference's subtraction fails
    with pytest.raises(ValueError):
        evaluate.scale_errors(np.ones(5), np.ones((2, 5)), windows=[0])
    with pytest.raises(ValueError):
        evaluate.scale_errors(np.ones(5), np.ones((2, 5)), windows=list(range(1, 18)))
    with pytest.raises(ValueError):
        evaluate.scale_errors(np.ones(5), np.ones((2, 5)), step=0)
    with pytest.raises(ValueError):
        evaluate.scale_errors(np.ones(5), np.ones((2, 2, 5)))
    with pytest.raises(ValueError):
        evaluate.filter_scales(np.ones(5), window=65)
    with pytest.raises(ValueError):
        evaluate.filter_scales(np.ones(5), window=0)
    scorer = evaluate.Scorer.__new__(evaluate.Scorer)                                    # (the table itself needs the device)
    scorer.ctx, scorer.n_poses = None, 11
    with pytest.raises(ValueError, match="10 motions"):
        scorer.score_gt_rescaled(np.ones((3, 9)))


def test_header_and_binding():
    from mvoscalerecovery_amd import _lib, evaluate
    with open(os.path.join(ROOT, "include", "mvosr.h")) as fh:
        header = fh.read()
    for name, n_args in (("mvosr_scale_errors_batch", 17), ("mvosr_window_median_cases", 8)):
        assert re.search(r"\b%s\(" % name, header) and len(_lib.SYMBOLS[name][1]) == n_args, name
    assert "#define MVOSR_ABI_VERSION 13" in header and _lib.ABI_VERSION == 13
    assert "#define MVOSR_SCALE_MAX_WINDOWS %d" % _lib.SCALE_MAX_WINDOWS in header
    assert "#define MVOSR_SCALE_MAX_THRESHOLDS %d" % _lib.SCALE_MAX_THRESHOLDS in header
    assert "#define MVOSR_SCALE_ERRORS_GLOBAL %d" % _lib.SCALE_ERRORS_GLOBAL in header
    with open(os.path.join(ROOT, "mvoscalerecovery_amd", "csrc", "mvosr_scalescore_plan.hpp")) as fh:
        plan = fh.read()
    assert "kSsLdsErrors = %d;" % _lib.SCALE_LDS_ERRORS in plan and "kSsLdsSegments = %d;" % _lib.SCALE_LDS_SEGMENTS in plan
    assert "kSsMaxWindow = %d;" % _lib.SCALE_MAX_WINDOW in plan and ssc.LDS_ERRORS == _lib.SCALE_LDS_ERRORS
    assert evaluate.SCALE_WINDOWS == ssc.WINDOWS and evaluate.SCALE_THRESHOLDS == ssc.THRESHOLDS and evaluate.SCALE_STEP == ssc.STEP
    lib = _lib.load()
    assert lib.mvosr_abi_version() == 13 and hasattr(lib, "mvosr_scale_errors_batch") and hasattr(lib, "mvosr_window_median_cases")


@pytest.mark.reference
@pytest.mark.skipif(not os.path.isdir("/root/reference/script"), reason="needs /root/reference")
def test_live_script_equals_the_comparators_on_fresh_seeds():
    import contextlib
    import importlib.util
    import io
    import matplotlib
    matplotlib.use("Agg")
    from mvoscalerecovery_amd import evaluate
    spec = importlib.util.spec_from_file_location("ref_evaluate_scale", "/root/reference/script/evaluate_scale.py")
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    rng = np.random.RandomState(int.from_bytes(os.urandom(4), "little"))
    for n in (37, 400, 1203):
        gt = 0.8 + 0.4 * rng.rand(n + 5)
        re_ = gt[:n] + 0.25 * rng.randn(n)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            es.evaluate_scale(gt, re_)
        head_line, list_line = buf.getvalue().strip().split("\n")
        head, drift = evaluate.evaluate_scale(gt, re_)
        assert ssc.same([float(x) for x in head_line.split()], head)
        assert ssc.same([np.mean(es.patch(gt[:n] - re_, w, 10)) for w in ssc.WINDOWS], drift)
        r = ssc.errors_restated(gt, re_[None])
        assert ssc.same(r["mean"][0], head[0]) and ssc.same(r["drift"][0], drift)
        assert ssc.same(es.filter(re_, 10), evaluate.scale_filter(re_, 10))
