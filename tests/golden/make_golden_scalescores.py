#!/usr/bin/env python3
"""Generates tests/golden/scalescores.npz: the reference's own scoring of scales — /root/reference/script/evaluate_scale.py:
evaluate_scale run as it stands with its printed figures parsed back (a double's shortest repr round-trips), patch and filter
called directly — over the crafted sets of tests/scalescore_cases.py; and, for Scorer.score_gt_rescaled, the ground truth of one
sequence of tests/scores_cases.py re-scaled by script/change_scale.py to each case's scales and scored by evaluate_vo.py, with the
gap |reference - extended precision| per quantity (the rule of make_golden_scores.py).

Per set (data only): the inputs' checksum; mean, max, within (the four printed shares), counts (the integers behind them, by the
reference's own expression), drift (eleven windows), raises (1 where the reference raises: np.max of no scale at all); per kept
window the filtered sequences.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_scalescores.py"""
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
REF_SCRIPT = "/root/reference/script"
sys.path.insert(0, REF_SCRIPT)

import matplotlib                                             # noqa: E402
matplotlib.use("Agg")
import evaluate_scale as es                                   # noqa: E402  (the reference's)
import evaluate_vo as ev                                      # noqa: E402  (the reference's)

import make_golden_scores as mgs                              # noqa: E402  (reference_change_scale)
import scalescore_cases as ssc                                # noqa: E402
import scores_cases as sc                                     # noqa: E402

LD = np.longdouble
FLOAT = re.compile(r"[-+]?(?:nan|inf|\d+\.?\d*(?:[eE][-+]?\d+)?)")


def printed(gt, re_):
    """What evaluate_scale prints: six figures, then the list of eleven (np.float64(...) wrappers of newer NumPy dropped)."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        es.evaluate_scale(gt, re_)
    head, tail = buf.getvalue().strip().split("\n")
    head = [float(x) for x in head.split()]
    tail = [float(x) for x in FLOAT.findall(tail.replace("np.float64", ""))]
    assert len(head) == 6 and len(tail) == len(ssc.WINDOWS), (head, tail)
    return np.array(head), np.array(tail)


def one_set(name):
    n, n_gt, cases, seed, kind, filt = ssc.SETS[name]
    s = ssc.make_set(name)
    gt, scales = s["gt"], s["scales"]
    out = {"crc": np.int64(ssc.checksum(s))}
    mean, mx, within, counts, drift, raises = [], [], [], [], [], 0
    for c in range(cases):
        re_ = scales[c]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            direct = np.array([np.mean(es.patch(gt[:n] - re_, w, 10)) for w in ssc.WINDOWS])
            a = np.abs(gt[:n] - re_)
            counts.append([int(np.sum(a > t)) for t in ssc.THRESHOLDS])
        try:
            head, tail = printed(gt, re_)
        except ValueError:                                    # np.max of an empty array: the reference prints nothing
            assert n == 0
            raises = 1
            head, tail = np.full(6, np.nan), direct
        assert ssc.same(tail, direct), (name, c, "the printed drift is patch's")
        mean.append(head[0]); mx.append(head[1]); within.append(head[2:]); drift.append(tail)
    out.update(mean=np.array(mean), max=np.array(mx), within=np.array(within).reshape(cases, 4), counts=np.array(counts, dtype=np.int64),
               drift=np.array(drift), raises=np.int64(raises))
    for w in filt:
        out["filter%d" % w] = np.array([es.filter(scales[c], w) for c in range(cases)])
    print("%-8s n %6d C %2d mean %.6g max %.6g finite drifts %d" % (name, n, cases, out["mean"][0], out["max"][0],
                                                                  int(np.isfinite(out["drift"][0]).sum())))
    return out


def gt_rescaled(tmp):
    """tesh.sh:6-8 for every case of one sequence: change_scale.py on the ground truth with the case's scales as the speed file,
    evaluate_vo's errors of the result against the ground truth; and the same in np.longdouble."""
    name = ssc.GT_RESCALED
    gt = sc.make_sequence(name)["gt"]
    scales = ssc.rescaled_scales()
    cases = scales.shape[0]
    tra, rot = [], []
    for c in range(cases):
        path = mgs.reference_change_scale(gt, scales[c], tmp, "g%d" % c)
        r, t, _ = ev.calculate_ave_errors(ev.calculate_sequence_error(gt, path))
        tra.append(np.asarray(t, dtype=np.float64))
        rot.append(np.asarray(r, dtype=np.float64))
    tra, rot = np.array(tra), np.array(rot)
    last = sc.segment_table(sc.distances(gt, dtype=LD))[0]
    columns = (last >= 0).any(axis=0)
    x_paths = np.concatenate([sc.change_scale_restated(gt, scales[c], dtype=LD) for c in range(cases)])
    x_means = sc.score_restated(gt, x_paths, last, dtype=LD)[2]
    x_tra, x_rot = x_means[:, 1, :][:, columns], x_means[:, 0, :][:, columns] * 180 / LD(np.pi)
    gaps = {"tra": mgs.gap_of(tra, x_tra, "tra"), "rot": mgs.gap_of(rot, x_rot, "rot")}
    print("gt_rescaled %s C %d columns %d gaps %s" % (name, cases, int(columns.sum()), {k: "%.2e" % v for k, v in gaps.items()}))
    return {"gtr_tra": tra, "gtr_rot": rot, "gtr_gaps": np.array(json.dumps(gaps)),
            "gtr_crc": np.int64(int(np.ascontiguousarray(scales).view(np.uint64).sum() & 0x7FFFFFFFFFFFFFFF))}


def main():
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not extended precision here"
    arrays = {}
    for name in ssc.SETS:
        for k, v in one_set(name).items():
            arrays["%s_%s" % (name, k)] = v
    with tempfile.TemporaryDirectory(prefix="scalescores") as tmp:
        assert "." not in tmp, "change_scale.py derives its output name by splitting the path at dots"
        arrays.update(gt_rescaled(tmp))
    # the issue's probes
    assert np.isnan(arrays["n10_drift"]).all() and np.isfinite(arrays["n11_drift"][:, 0]).all() and np.isnan(arrays["n11_drift"][:, 1:]).all()
    assert np.isnan(arrays["nan_mean"][1]) and np.isnan(arrays["nan_max"][1]) and np.isfinite(arrays["nan_within"]).all()
    assert np.isfinite(arrays["n801_drift"]).all() and arrays["n0_raises"] == 1
    arrays["meta"] = np.array(json.dumps({"numpy": np.__version__, "sets": {k: list(v[:5]) for k, v in ssc.SETS.items()}}))
    path = os.path.join(HERE, "scalescores.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("scalescores.npz", size, "bytes")
    assert size < 400 * 1024


if __name__ == "__main__":
    main()
