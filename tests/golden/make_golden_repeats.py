#!/usr/bin/env python3
"""Generates tests/golden/rescale_repeats.npz: the reference's own rescale.ScaleEstimator (/root/reference/src/rescale.py, the estimator
main_offline.py:20 imports) run TEN times over one synthetic 40-frame dict — what /root/reference/test_off_line.sh:4-16 does with ten
processes of main_offline.py.  The reference seeds its RANSAC from OS entropy (thirdparty/Ransac/ransac.py:6); here random.sample
replays make_golden.ransac_triples(seed_c, call, n) for case c, so that every run is reproducible and the runs differ.

Kept (data only): the ten scales rows (main_offline's scales file per case), per estimator call the ids flat_selection returned (the
list the triples index — the same in every case, which is asserted), whether the RANSAC ran, and the ten seeds.

Self-check: case 0 through /root/reference/src/main_offline.py ITSELF (runpy, make_golden.make_rescale_main_offline) equals row 0.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_repeats.py"""
import importlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                                      # noqa: E402  (puts the repository root on sys.path)
from mvoscalerecovery_amd import offline, synth               # noqa: E402

N_FRAMES, SEED, CASES = 40, 4711, 10
KW = {"n_lo": 300, "n_hi": 700, "p_not_moving": 0.06, "p_too_few": 0.06}
SEEDS = [9000 + 37 * c for c in range(CASES)]


def run_case(data, seed):
    """One run of the reference's estimator over the dict with main_offline's loop (offline.run_sequence restates :57-88; the
    self-check below runs the script itself): (scales row, ids per estimator call, ran per call)."""
    rescale = importlib.import_module("rescale")
    ransac_mod = importlib.import_module("thirdparty.Ransac.ransac")
    import estimate_road_norm
    state = {"call": -1, "triples": None, "pos": 0, "ids": [], "ran": []}

    def fake_sample(d, k):
        t = state["triples"][state["pos"]]
        state["pos"] += 1
        return [d[int(i)] for i in t]

    real_run, real_sample, real_flat = ransac_mod.run_ransac, ransac_mod.random.sample, rescale.ScaleEstimator.flat_selection

    def run_spy(d, *a, **k):
        state["call"] += 1
        state["triples"] = mg.ransac_triples(seed, state["call"], len(list(d)))
        state["pos"] = 0
        state["ran"][-1] = True
        return real_run(d, *a, **k)

    def flat_spy(self, feature3d, triangle_ids):
        out = real_flat(self, feature3d, triangle_ids)
        state["ids"].append(np.asarray(out[0], dtype=np.int32).reshape(-1))
        state["ran"].append(False)
        return out

    ransac_mod.random.sample = fake_sample
    estimate_road_norm.run_ransac = run_spy
    rescale.ScaleEstimator.flat_selection = flat_spy
    try:
        with mg.quiet():
            est = rescale.ScaleEstimator(absolute_reference=mg.ABS_REF, window_size=5)            # main_offline.py:38
            res = offline.run_sequence(data, est)
    finally:
        ransac_mod.random.sample = real_sample
        estimate_road_norm.run_ransac = real_run
        rescale.ScaleEstimator.flat_selection = real_flat
    return res["scales"], state["ids"], np.asarray(state["ran"], dtype=bool)


def main():
    sc = mg.load_reference()
    data = synth.synth_sequence_dict(N_FRAMES, base_seed=SEED, **KW)
    kinds = offline.plan_sequence(data)
    assert (kinds == 0).any() and (kinds == 2).any(), "the dict needs a not-moving and a too-few frame"
    rows, ids0, ran0 = [], None, None
    for c, seed in enumerate(SEEDS):
        scales, ids, ran = run_case(data, seed)
        if ids0 is None:
            ids0, ran0 = ids, ran
        assert len(ids) == len(ids0) and all(np.array_equal(a, b) for a, b in zip(ids, ids0)) and np.array_equal(ran, ran0), \
            "the deterministic stages differ between cases"
        rows.append(scales)
        print("case", c, "seed", seed, "mean scale", float(np.mean(scales[scales != 0])))
    rows = np.array(rows)
    assert rows.shape == (CASES, N_FRAMES) and len({r.tobytes() for r in rows}) == CASES, "the cases must differ"
    assert ran0.any() and len(ids0) == int((kinds == 1).sum())
    # self-check: main_offline.py itself on case 0
    old_here = mg.HERE
    with tempfile.TemporaryDirectory() as tmp:
        mg.HERE = tmp
        try:
            mg.make_rescale_main_offline(sc, N_FRAMES, SEED, "check", ransac_seed=SEEDS[0], **KW)
        finally:
            mg.HERE = old_here
        z = np.load(os.path.join(tmp, "check.npz"))
        assert np.array_equal(z["scales"], rows[0]), "main_offline.py's own run of case 0 differs from the row"
        assert np.array_equal(z["ids"], np.concatenate(ids0)) and np.array_equal(z["ran"], ran0)
    ids_off = np.concatenate([[0], np.cumsum([len(x) for x in ids0])]).astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "rescale_repeats.npz"), scales=rows, ids=np.concatenate(ids0), ids_off=ids_off, ran=ran0,
                        seeds=np.asarray(SEEDS, dtype=np.int64),
                        meta=np.array(json.dumps({"n_frames": N_FRAMES, "seed": SEED, "kw": KW, "abs_ref": mg.ABS_REF, "window": 5,
                                                  "cases": CASES, "scipy": __import__("scipy").__version__})))
    print("rescale_repeats", rows.shape, "estimator calls", len(ids0), "ransac calls", int(ran0.sum()))


if __name__ == "__main__":
    main()
