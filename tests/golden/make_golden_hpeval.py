"""Generates tests/golden/hpeval.npz from the reference's own runs of src/calculate_height_pitch_eval.py ("plane") and
src/calculate_height_pitch_eval_line.py ("line").

Both are Python-2 programs over text dumps; they are executed AS THEY LIE in /root/reference, with the stubbing of
make_golden_heightpitch.py: the source is read at run time, its print statements are given parentheses in memory, cv2 is stubbed,
np.float is shimmed, and the script runs in a scratch directory laid out as it expects (result/kitti_<id>/kitti_<id>_feature_<date>/,
eval_ransac/, eval_ransac_line/).  random.sample is spied (the size-3 and size-2 draws recorded as list positions, per case and
frame), as are get_pitch (the priors), get_pitch_ransac / get_pitch_line_ransac (model, best count) and the first get_inliers of
each frame (the LIST mask).  The sixty files a run writes are read back.  Nothing of the reference's text is stored: the fixture
holds seeds, checksums, positions, recorded numbers, file names and the type of the exception that ends each script.

A run is repeated (the scripts seed from OS entropy) until the float64 restatement replays its integers and no decision lies in a
rounding band (hpeval_cases.check_margins).  Refined floats are compared on the fitted (frame, case) pairs that are not flagged
degenerate; the generator asserts that those are at least 90 % (line) / 60 % (plane) of the fitted pairs.

Run from the repository root on a machine that has /root/reference:  python tests/golden/make_golden_hpeval.py"""
import contextlib
import io
import json
import os
import random
import re
import sys
import tempfile
import types
import warnings

import numpy as np
from scipy.spatial import Delaunay

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REF_SRC = "/root/reference/src"
SCRIPTS = {"plane": "calculate_height_pitch_eval.py", "line": "calculate_height_pitch_eval_line.py"}
OUT_DIRS = {"plane": "eval_ransac", "line": "eval_ransac_line"}
INPUT_ID, INPUT_DATE, CASES = "07", "0405", 10
MIN_COMPARED = {"line": 0.9, "plane": 0.6}

import heightpitch_cases as hc                                # noqa: E402
import hpeval_cases as he                                     # noqa: E402


def run_script(model, dumps, mot, iterations):
    """-> dict: files {relative name: array}, priors, per (case, fitted frame) the recorded positions / model / best count / list
    mask / list length, and the type name of the exception that ended the run (None: it ran to its end)."""
    name = SCRIPTS[model]
    src = open(os.path.join(REF_SRC, name)).read()
    src = re.sub(r"^(\s*)print (?!\()(.*)$", r"\1print(\2)", src, flags=re.M)
    K = he.K_of(model)
    rec = {"priors": [], "fits": [], "cur": None, "want_mask": False}
    real_sample = random.sample

    def sample(pop, k):
        idx = real_sample(range(len(pop)), k)
        if k == K and rec["cur"] is not None:
            rec["cur"].append(idx)
        return [pop[i] for i in idx]

    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda *a, **k: np.zeros((1, 1))
    old_cv2, old_argv, old_cwd, old_path = sys.modules.get("cv2"), sys.argv, os.getcwd(), list(sys.path)
    had_float = hasattr(np, "float")
    for mod in [k for k in sys.modules if k == "estimate_road_norm" or k.startswith("thirdparty")]:
        del sys.modules[mod]
    err, files = None, {}
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "result", "kitti_" + INPUT_ID)
        feat = os.path.join(base, "kitti_%s_feature_%s" % (INPUT_ID, INPUT_DATE))
        os.makedirs(feat)
        for d in OUT_DIRS.values():
            os.makedirs(os.path.join(tmp, d))
        for i, d in enumerate(dumps):
            np.savetxt(os.path.join(feat, "%d.txt" % (i + 1)), d, fmt="%.18e")
        for kind in ("motion", "pose"):
            np.savetxt(os.path.join(base, "kitti_%s_%s_%s.txt" % (INPUT_ID, kind, INPUT_DATE)), mot, fmt="%.18e")
        sys.modules["cv2"] = cv2
        sys.path.insert(0, REF_SRC)
        if not had_float:
            np.float = float
        random.sample = sample
        sys.argv = [name, INPUT_ID, INPUT_DATE, str(len(dumps) + 1), str(iterations)]
        os.chdir(tmp)
        ns = {"__name__": "__main__"}
        try:
            import estimate_road_norm as ern
            gp, gi = ern.get_pitch, ern.get_inliers
            fit_name = "get_pitch_line_ransac" if model == "line" else "get_pitch_ransac"
            gr = getattr(ern, fit_name)

            def get_pitch(ts):
                rec["priors"].append(float(gp(ts)))
                return rec["priors"][-1]

            def fit(pts, it, thr):
                rec["cur"] = []
                m, b = gr(pts, it, thr)
                rec["fits"].append({"frame": len(rec["priors"]) - 1, "positions": np.array(rec["cur"], dtype=np.int32).reshape(-1, K),
                                    "model": np.array(m, dtype=np.float64), "best_ic": int(b), "M": int(pts.shape[0])})
                rec["cur"], rec["want_mask"] = None, True
                return m, b

            def get_inliers(m, data, thr):
                out = gi(m, data, thr)
                if rec["want_mask"]:                            # the first call after a fit: over the list
                    rec["fits"][-1]["mask"] = np.array(out, dtype=bool)
                    rec["want_mask"] = False
                return out
            ern.get_pitch, ern.get_inliers = get_pitch, get_inliers
            setattr(ern, fit_name, fit)
            with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                try:
                    exec(compile(src, os.path.join(REF_SRC, name), "exec"), ns)
                except Exception as e:                          # noqa: BLE001 — what the script itself raises is the datum
                    err = type(e).__name__
        finally:
            os.chdir(old_cwd)
            sys.argv, sys.path[:] = old_argv, old_path
            random.sample = real_sample
            if not had_float:
                del np.float
            if old_cv2 is not None:
                sys.modules["cv2"] = old_cv2
            else:
                sys.modules.pop("cv2", None)
            sys.modules.pop("estimate_road_norm", None)
        for fn in sorted(os.listdir(os.path.join(tmp, OUT_DIRS[model]))):
            files[os.path.join(OUT_DIRS[model], fn)] = np.atleast_1d(np.loadtxt(os.path.join(tmp, OUT_DIRS[model], fn)))
        stray = [fn for fn in os.listdir(tmp) if fn not in ("result",) + tuple(OUT_DIRS.values())]
    return {"files": files, "priors": np.array(rec["priors"]), "fits": rec["fits"], "error": err, "stray": stray}


def make_case(case, specs, mot_seed, iterations, store, meta):
    from mvoscalerecovery_amd import height_pitch as hp
    specs = [list(s) for s in specs]
    cm = {"motion_seed": mot_seed, "iterations": iterations}
    n = len(specs)
    nonempty = [i for i, s in enumerate(specs) if s[0] != "empty"]
    for model in he.MODELS:
        for attempt in range(12):
            dumps = [he.dump_of(s) for s in specs]
            mot = hc.motions(mot_seed, n + 2)
            rows = [Delaunay(d[:, 0:2]).simplices.astype(np.int32) if len(d) else np.zeros((0, 3), np.int32) for d in dumps]
            got = run_script(model, dumps, mot, iterations)
            names = hp.eval_file_names(model, INPUT_ID, INPUT_DATE, iterations, CASES)
            complete = sorted(got["files"]) == sorted(names)
            # the spy's records in call order: case-major, the non-empty frames in order
            priors = np.full(n, np.nan)
            fits = {}
            for k, p in enumerate(got["priors"]):
                priors[nonempty[k % len(nonempty)]] = p
            for f in got["fits"]:
                fits[(f["frame"] // len(nonempty), nonempty[f["frame"] % len(nonempty)])] = f
            ok, compared, fitted, results = True, 0, 0, None
            gaps = {"gap_" + k: 0.0 for k in he.REFINED}
            if complete:
                results = {k: np.stack([got["files"][names[c * 6 + j]] for c in range(CASES)]) for j, k in enumerate(he.FIELDS)}
                suitable = np.zeros(n, np.int32)
                for c in range(CASES):
                    prev = None
                    for i in range(n):
                        if specs[i][0] == "empty":
                            ok &= all(results[k][c, i] == 0 for k in he.FIELDS)
                            continue
                        f = fits.get((c, i))
                        pos = f["positions"] if f else np.zeros((1, 3), np.int32)
                        if not he.check_margins(model, dumps[i], rows[i], priors[i], pos):
                            print(case, model, "case", c, "frame", i, "has a decision inside a rounding band: again")
                            ok = False
                            break
                        r = he.restate(model, dumps[i], rows[i], priors[i], pos, prev)
                        prev = r
                        suitable[i] = r["n_selected"]
                        if (f is None) != r["carried"] or (f and (f["M"] != r["n_selected"] or f["best_ic"] != r["best_ic"] or
                                                                  not np.array_equal(f["mask"], r["list_mask"]))):
                            print(case, model, "case", c, "frame", i, "restatement and script disagree on an integer: again")
                            ok = False
                            break
                        if r["n_inliers"] != int(results["n_inliers"][c, i]):
                            ok = False
                            break
                        assert np.isclose(r["ransac_height"], results["ransac_height"][c, i], rtol=1e-9, atol=0), (case, model, c, i)
                        fitted += 1
                        if r["degenerate"]:
                            continue
                        compared += 1
                        for k in he.REFINED:
                            want = results[k][c, i]
                            gaps["gap_" + k] = max(gaps["gap_" + k], float(abs(r[k] - want) / abs(want)))
                    if not ok:
                        break
            if ok:
                break
        else:
            raise SystemExit("no admissible run of %s / %s" % (case, model))
        if fitted:
            assert compared >= MIN_COMPARED[model] * fitted, (case, model, compared, fitted)
        pre = "%s_%s_" % (model, case)
        if results is not None:
            for k in he.FIELDS:
                store[pre + k] = results[k]
            store[pre + "suitable"] = suitable
        for i in range(n):
            fs = [fits.get((c, i)) for c in range(CASES)]
            if not complete or any(f is None for f in fs):
                continue
            pos = np.full((CASES, iterations, 3), -1, np.int16)
            for c, f in enumerate(fs):
                pos[c, :len(f["positions"]), :f["positions"].shape[1]] = f["positions"]
            mods = np.stack([he.four(model, f["model"]) for f in fs])
            store[pre + "positions%d" % i] = pos
            store[pre + "model%d" % i] = np.where(mods[:, 1:2] >= 0, mods, -mods)
            store[pre + "best_ic%d" % i] = np.array([f["best_ic"] for f in fs], np.int32)
            store[pre + "mask%d" % i] = np.stack([f["mask"] for f in fs])
        cm[model] = {"error": got["error"], "files": sorted(got["files"]), "stray": sorted(got["stray"]), "gaps": gaps, "fitted_pairs": fitted,
                     "compared_pairs": compared}
        print(case, model, "error", got["error"], "files", len(got["files"]), "fitted", fitted, "compared", compared, gaps)
    cm["frames"] = [dict(spec=s, crc=hc.crc(d)) for s, d in zip(specs, dumps)]
    cm["motion_crc"] = hc.crc(mot)
    store[case + "_priors"] = priors
    for i, t in enumerate(rows):
        if len(t):
            store[case + "_rows%d" % i] = t.astype(np.int16)
    meta["cases"][case] = cm


def main():
    store, meta = {}, {"cases": {}, "input_id": INPUT_ID, "input_date": INPUT_DATE, "n_cases": CASES}
    sizes = [210 + 60 * i for i in range(8)]                                         # 210 .. 630 features
    make_case("seq", [("synth", 800 + i, n, 13579) for i, n in enumerate(sizes)], 21, 40, store, meta)
    make_case("carry", [("synth", 830, 330, 13579), ("wall", 41, 260), ("synth", 831, 390, 13579)], 22, 20, store, meta)
    make_case("empty", [("synth", 840, 300, 13579), ("empty",), ("synth", 841, 360, 13579)], 23, 20, store, meta)
    make_case("first", [("wall", 42, 240), ("synth", 850, 300, 13579)], 24, 20, store, meta)
    c = meta["cases"]
    for case in ("seq", "carry", "empty"):
        assert c[case]["plane"]["error"] == "TypeError" and c[case]["line"]["error"] is None, case    # the plane script's last line
        assert len(c[case]["plane"]["files"]) == 60 and len(c[case]["line"]["files"]) == 60
    assert c["first"]["plane"]["error"] == c["first"]["line"]["error"] == "IndexError" and not c["first"]["plane"]["files"]
    path = os.path.join(HERE, "hpeval.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **store)
    print("wrote hpeval.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
