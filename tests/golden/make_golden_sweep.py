#!/usr/bin/env python3
"""Generate tests/golden/sweep.npz: what the constants of rescale.RescaleConstants MEAN, pinned to the reference's own code.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_sweep.py

For every setting of tests/sweep_cases.py's SETTINGS the text of /root/reference/src/rescale.py is read at run time, the literals
of that setting are substituted (each pattern must occur exactly as often as stated, else the generator stops), and the result is
executed as the module `rescale` that /root/reference/src/main_offline.py imports (main_offline.py:20) — the reference's own loop,
run as __main__ on a short synthetic sequence with `random.sample` replaying a recorded sample sequence, as make_golden.py's
`make_rescale_main_offline` does.  A setting on which the patched reference raises stops the generator: change SEQUENCE's seed in
tests/sweep_cases.py, not the comparison.

The fixture holds DATA only: the sequence's parameters and the checksum of its arrays, the sample seed and the recorded samples,
and per setting the scales file the loop wrote, the ids and the level flat_selection returned per call, and the inlier count and
iterations of every fit.  No source text is stored.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import runpy
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.ref_harness import REFERENCE_SRC, load_reference  # noqa: E402
from mvoscalerecovery_amd import offline  # noqa: E402
import sweep_cases as sw  # noqa: E402

warnings.simplefilter("ignore")


def patched_source(k):
    """rescale.py's text with the literals of setting ``k`` (a dict of all eight constants; goal_fraction is not in that file)."""
    src = open(os.path.join(REFERENCE_SRC, "rescale.py")).read()
    subs = [("pitch_deg<-80", "pitch_deg<%r" % k["loose_deg"], 1), ("pitch_deg>=-80", "pitch_deg>=%r" % k["loose_deg"], 1),
            ("pitch_deg<-85", "pitch_deg<%r" % k["tight_deg"], 1), ("0.9*(np.median(", "%r*(np.median(" % k["height_factor"], 1),
            ("point_selected.shape[0]>=12", "point_selected.shape[0]>=%d" % k["ransac_min_points"], 1),
            ("get_pitch_ransac(a_array,100,0.005)", "get_pitch_ransac(a_array,%d,%r)" % (k["n_hyp"], k["threshold"]), 1),
            ("scale - self.scale >0.3", "scale - self.scale >%r" % k["slew"], 1), ("self.scale += 0.3", "self.scale += %r" % k["slew"], 1),
            ("scale - self.scale<-0.3", "scale - self.scale<-%r" % k["slew"], 1), ("self.scale -= 0.3", "self.scale -= %r" % k["slew"], 1)]
    for old, new, count in subs:
        assert src.count(old) == count, "rescale.py: %r occurs %d times, expected %d" % (old, src.count(old), count)
        src = src.replace(old, new)
    return src


def run_setting(data, k):
    """main_offline.py as __main__ on ``data`` with the patched estimator -> (scales, per-call records, recorded samples)."""
    import importlib
    load_reference()                                     # (the stub cv2, np.float, and the reference on sys.path)
    ransac_mod = importlib.import_module("thirdparty.Ransac.ransac")
    import estimate_road_norm
    mod = types.ModuleType("rescale")
    mod.__file__ = "<rescale.py with one setting's literals>"
    exec(compile(patched_source(k), mod.__file__, "exec"), mod.__dict__)
    state = {"call": -1, "triples": None, "pos": 0, "calls": [], "samples": []}

    def fake_sample(d, n):
        t = state["triples"][state["pos"]]
        state["pos"] += 1
        return [d[int(i)] for i in t]

    real_run = ransac_mod.run_ransac

    def run_spy(d, *a, **kw):
        state["call"] += 1
        state["triples"] = sw.sample_triples(sw.SAMPLE_SEED, state["call"], len(list(d)), k["n_hyp"])
        state["samples"].append(state["triples"])
        state["pos"] = 0
        m, ic = real_run(d, *a, **kw)
        state["calls"][-1].update(best_ic=int(ic), used=state["pos"])
        return m, ic

    real_flat = mod.ScaleEstimator.flat_selection

    def flat_spy(self, feature3d, triangle_ids):
        out = real_flat(self, feature3d, triangle_ids)
        state["calls"].append({"ids": np.asarray(out[0], dtype=np.int32).reshape(-1), "height_level": float(self.height_level)})
        return out

    class _Cv2Stub(types.ModuleType):
        def __getattr__(self, attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return 0
    old = {name: sys.modules.get(name) for name in ("cv2", "rescale")}
    sys.modules["cv2"], sys.modules["rescale"] = _Cv2Stub("cv2"), mod
    real_sample = ransac_mod.random.sample
    ransac_mod.random.sample = fake_sample
    estimate_road_norm.run_ransac = run_spy
    mod.ScaleEstimator.flat_selection = flat_spy
    old_argv, old_cwd = sys.argv, os.getcwd()
    try:
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "evaluate_result"))
            os.makedirs(os.path.join(tmp, "result"))
            path = os.path.join(tmp, "result", "synth_result.npy.golden.npy")
            offline.save_sequence_dict(path, data)
            sys.argv = ["main_offline.py", path, ".golden"]
            os.chdir(tmp)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    runpy.run_path(os.path.join(REFERENCE_SRC, "main_offline.py"), run_name="__main__")
            finally:
                os.chdir(old_cwd)
                sys.argv = old_argv
            scales = np.loadtxt(os.path.join(tmp, "evaluate_result", "synth_result_scales.txt.golden"))
    finally:
        ransac_mod.random.sample = real_sample
        estimate_road_norm.run_ransac = real_run
        for name, m in old.items():
            if m is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = m
    return scales, state["calls"], state["samples"]


def main():
    data = sw.golden_sequence()
    kinds = offline.plan_sequence(data)
    assert (kinds == 0).any() and (kinds == 2).any() and (kinds == 1).sum() >= 18, "the sequence must pass through both of the loop's gates"
    out = {}
    for i, (name, _) in enumerate(sw.SETTINGS):
        k = sw.setting(i)
        scales, calls, samples = run_setting(data, k)
        assert len(calls) == int((kinds == 1).sum()) and len(scales) == len(kinds)
        ids = [c["ids"] for c in calls]
        assert max((int(x.max()) for x in ids if len(x)), default=0) < 32768
        out["s%d_scales" % i] = scales
        out["s%d_ids" % i] = np.concatenate(ids).astype(np.int16)
        out["s%d_ids_off" % i] = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int32)
        out["s%d_height_level" % i] = np.array([c["height_level"] for c in calls], dtype=np.float64)
        out["s%d_ran" % i] = np.array(["best_ic" in c for c in calls], dtype=bool)
        out["s%d_best_ic" % i] = np.array([c["best_ic"] for c in calls if "best_ic" in c], dtype=np.int32)
        out["s%d_used" % i] = np.array([c["used"] for c in calls if "best_ic" in c], dtype=np.int32)
        out["s%d_triples" % i] = np.stack(samples).astype(np.int16) if samples else np.zeros((0, k["n_hyp"], 3), np.int16)
        print("%-16s fits %2d of %2d calls, list lengths %d..%d, last scale %.6f" %
              (name, int(out["s%d_ran" % i].sum()), len(calls), min(map(len, ids)), max(map(len, ids)), scales[-1]))
    out["meta"] = np.array(json.dumps({"settings": [[n, sw.setting(i)] for i, (n, _) in enumerate(sw.SETTINGS)], "sequence": sw.SEQUENCE,
                                       "crc": sw.sequence_checksum(data), "sample_seed": sw.SAMPLE_SEED, "abs_ref": sw.ABS_REF,
                                       "window": sw.WINDOW, "scipy": __import__("scipy").__version__}))
    np.savez_compressed(os.path.join(HERE, "sweep.npz"), **out)
    print("sweep.npz", os.path.getsize(os.path.join(HERE, "sweep.npz")), "bytes")


if __name__ == "__main__":
    main()
