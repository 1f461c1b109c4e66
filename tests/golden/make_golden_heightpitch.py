"""Generates tests/golden/heightpitch.npz from the reference's own run of src/calculate_height_pitch.py.

The script is a Python-2 program over text dumps.  It is executed AS IT LIES in /root/reference (as make_golden.py's
make_triangle_batch does with triangle_batch.py): its source is read at run time, its print statements are given parentheses in
memory, cv2.imread is stubbed, np.float is shimmed, and it runs in a scratch directory on dumps written from synthetic frames
until the first missing dump ends its loop — its six result lists are then in the exec namespace.  random.sample is spied (the
size-3 draws recorded as list positions, drawn by the same generator in the same state), as are get_pitch (the priors),
get_pitch_ransac (model, best count) and get_inliers (the mask).  Nothing of the reference's text is stored: the fixture holds
seeds, checksums and recorded numbers.

Run from the repository root on a machine that has /root/reference:  python tests/golden/make_golden_heightpitch.py"""
import contextlib
import io
import json
import os
import random
import re
import sys
import tempfile
import types

import numpy as np
from scipy.spatial import Delaunay

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REF_SRC = "/root/reference/src"

from mvoscalerecovery_amd import synth                      # noqa: E402
import flat_cases as fc                                       # noqa: E402
import heightpitch_cases as hc                                # noqa: E402

U53 = 2.0 ** -53


def run_script(dumps, mot):
    """-> dict: the six lists, priors, suitable-point counts, per fitted frame the recorded positions / model / best count / mask,
    and the type name of the exception that ended the run (None: the missing dump)."""
    src = open(os.path.join(REF_SRC, "calculate_height_pitch.py")).read()
    src = re.sub(r"^(\s*)print (?!\()(.*)$", r"\1print(\2)", src, flags=re.M)
    rec = {"positions": [], "priors": [], "models": [], "masks": [], "cur": None}
    real_sample = random.sample

    def sample(pop, k):
        idx = real_sample(range(len(pop)), k)
        if k == 3:
            rec["cur"].append(idx)
        return [pop[i] for i in idx]

    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda *a, **k: np.zeros((1, 1))
    old_cv2, old_argv, old_cwd, old_path = sys.modules.get("cv2"), sys.argv, os.getcwd(), list(sys.path)
    had_float = hasattr(np, "float")
    for name in [k for k in sys.modules if k == "estimate_road_norm" or k.startswith("thirdparty")]:
        del sys.modules[name]
    err = None
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "feat"))
        with open(os.path.join(tmp, "list.txt"), "w") as fh:
            fh.write("header\n" + "".join("img%d.png\n" % i for i in range(len(dumps) + 2)))
        for i, d in enumerate(dumps):
            np.savetxt(os.path.join(tmp, "feat", "%d.txt" % (i + 1)), d, fmt="%.18e")
        np.savetxt(os.path.join(tmp, "motion.txt"), mot, fmt="%.18e")
        sys.modules["cv2"] = cv2
        sys.path.insert(0, REF_SRC)
        if not had_float:
            np.float = float
        random.sample = sample
        sys.argv = ["calculate_height_pitch.py", os.path.join(tmp, "list.txt"), os.path.join(tmp, "feat") + "/",
                    os.path.join(tmp, "motion.txt"), os.path.join(tmp, "motion.txt")]
        os.chdir(tmp)
        buf = io.StringIO()
        ns = {"__name__": "__main__"}
        try:
            import estimate_road_norm as ern
            gp, gr, gi = ern.get_pitch, ern.get_pitch_ransac, ern.get_inliers

            def get_pitch(ts):
                rec["priors"].append(float(gp(ts)))
                return rec["priors"][-1]

            def get_pitch_ransac(pts, it, thr):
                rec["cur"] = []
                m, b = gr(pts, it, thr)
                rec["positions"].append(np.array(rec["cur"], dtype=np.int32))
                rec["models"].append((np.array(m, dtype=np.float64), int(b)))
                return m, b

            def get_inliers(m, data, thr):
                rec["cur"] = []                                 # (the line RANSAC's pairs are not recorded anyway)
                out = gi(m, data, thr)
                rec["masks"].append(np.array(out, dtype=bool))
                return out
            ern.get_pitch, ern.get_pitch_ransac, ern.get_inliers = get_pitch, get_pitch_ransac, get_inliers
            with contextlib.redirect_stdout(buf):
                try:
                    exec(compile(src, os.path.join(REF_SRC, "calculate_height_pitch.py"), "exec"), ns)
                except (OSError, IOError):
                    pass                                        # the first missing dump ends the script's while loop
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
    out = {k: np.array(ns.get(k, []), dtype=np.float64) for k in
           ("ransac_camera_heights", "refined_camera_height_means", "refined_camera_height_stds", "refined_camera_height_t_means",
            "refined_pitchs", "inlier_numbers")}
    out["suitable"] = np.array([int(x) for x in re.findall(r"suitable point : ?(\d+)", buf.getvalue())], dtype=np.int32)
    out.update(priors=np.array(rec["priors"]), positions=rec["positions"], models=rec["models"], masks=rec["masks"], error=err)
    return out


def check_margins(pts, rows, est, positions):
    """True when no decision of the frame lies inside a rounding band: every row's pitch further than flat_cases.pitch_margin_deg
    from both window edges, every residual further than test_gpu_ransac.py's mask band from its threshold."""
    P = hc.back_project(pts)
    sure, maybe, q = hc.keep_bounds(P, rows, est)
    if not np.array_equal(sure, maybe):
        return False
    ids = np.asarray(rows)[sure].reshape(-1)
    if len(ids) < hc.MIN_POINTS:
        return True
    m = hc.planes_from(P, hc.vertex_triples(ids, positions))
    Q = P[ids]
    for mm in m:
        if np.isnan(mm[0]):
            continue
        band = 2 * 4.1 * U53 * (np.abs(Q) @ np.abs(mm[:3]) + abs(mm[3]))
        if np.any(np.abs(hc.residuals(Q, mm) - hc.THRESHOLD) <= band):
            return False
    cnt = np.array([np.sum(hc.residuals(Q, mm) < hc.THRESHOLD) for mm in np.nan_to_num(m, nan=1e300)])
    best = fc.replay(cnt, len(ids), hc.GOAL)[0]
    band = 2 * 4.1 * U53 * (np.abs(P) @ np.abs(m[best][:3]) + abs(m[best][3]))
    return not np.any(np.abs(hc.residuals(P, m[best]) - hc.INLIER_THRESHOLD) <= band)


def make_case(name, specs, mot_seed, store):
    """specs: list of ("synth", frame_idx, n, base_seed) / ("wall", seed, n).  Re-runs (the script draws from OS entropy) until the
    float64 restatement replays the script's integers and no decision lies in a band; re-draws a frame's seed where one does."""
    specs = [list(s) for s in specs]
    for attempt in range(20):
        dumps = []
        for s in specs:
            if s[0] == "synth":
                f3, f2 = synth.synth_frame(s[1], s[2], base_seed=s[3])
                dumps.append(np.stack([f2[:, 0], f2[:, 1], f3[:, 2]], 1))
            else:
                dumps.append(hc.wall_frame(s[1], s[2]))
        mot = hc.motions(mot_seed, len(dumps) + 2)
        got = run_script(dumps, mot)
        rows = [Delaunay(d[:, 0:2]).simplices.astype(np.int32) for d in dumps]       # :69-70 (the same call: the same rows)
        n_done = len(got["ransac_camera_heights"])
        fitted = [i for i in range(len(got["suitable"])) if got["suitable"][i] >= hc.MIN_POINTS]
        pos = {f: got["positions"][k] for k, f in enumerate(fitted)}
        ok, prev, rs = True, None, []
        for i in range(len(got["suitable"])):
            if not check_margins(dumps[i], rows[i], got["priors"][i], pos.get(i, np.zeros((1, 3), np.int32))):
                print(name, "frame", i, "has a decision inside a rounding band: new seed")
                specs[i][-1 if specs[i][0] == "synth" else 1] += 1000
                ok = False
                break
            if i >= n_done:
                break
            r = hc.restate(dumps[i], rows[i], got["priors"][i], pos.get(i), prev)
            prev = r
            rs.append(r)
            if r["n_selected"] != got["suitable"][i] or r["n_inliers"] != int(got["inlier_numbers"][i]):
                print(name, "frame", i, "restatement and script disagree on an integer (a rank-deficient sample?): again")
                ok = False
                break
            if i in pos:
                k = fitted.index(i)
                if r["best_ic"] != got["models"][k][1] or not np.array_equal(r["mask"], got["masks"][k]):
                    print(name, "frame", i, "best count or mask differ: again")
                    ok = False
                    break
        if ok:
            break
    else:
        raise SystemExit("no admissible run of " + name)
    gaps = {}
    for key, field in (("refined_camera_height_means", "refined_mean"), ("refined_camera_height_stds", "refined_std"),
                       ("refined_camera_height_t_means", "height_t_mean"), ("refined_pitchs", "refined_pitch")):
        mine = np.array([r[field] for r in rs])
        gaps["gap_" + field] = float(np.max(np.abs(mine - got[key][:len(rs)]) / np.abs(got[key][:len(rs)]))) if len(rs) else 0.0
    if len(rs):
        h = np.array([r["ransac_height"] for r in rs])
        assert np.allclose(h, got["ransac_camera_heights"], rtol=1e-9, atol=0), name
    pre = name + "_"
    for key in ("ransac_camera_heights", "refined_camera_height_means", "refined_camera_height_stds", "refined_camera_height_t_means",
                "refined_pitchs", "inlier_numbers", "suitable", "priors"):
        store[pre + key] = got[key]
    for i, t in enumerate(rows):
        store[pre + "rows%d" % i] = t
    for k, f in enumerate(fitted):
        store[pre + "positions%d" % f] = got["positions"][k]
        m = got["models"][k][0]
        store[pre + "model%d" % f] = m if m[1] >= 0 else -m
        store[pre + "best_ic%d" % f] = np.int32(got["models"][k][1])
        store[pre + "mask%d" % f] = got["masks"][k]
    meta = {"frames": [dict(kind=s[0], args=s[1:], crc=hc.crc(d)) for s, d in zip(specs, dumps)], "motion_seed": mot_seed,
            "motion_crc": hc.crc(mot), "n_results": n_done, "error": got["error"], "gaps": gaps}
    print(name, "frames", len(dumps), "results", n_done, "error", got["error"], "suitable", got["suitable"].tolist(), gaps)
    return meta


def main():
    store, meta = {}, {}
    sizes = [210 + 60 * i for i in range(12)]                                        # 210 .. 870 features
    meta["seq"] = make_case("seq", [("synth", 700 + i, n, 24680) for i, n in enumerate(sizes)], 11, store)
    meta["first"] = make_case("first", [("wall", 31, 240), ("synth", 720, 300, 24680)], 12, store)
    meta["carry"] = make_case("carry", [("synth", 730, 330, 24680), ("wall", 32, 260), ("synth", 731, 390, 24680)], 13, store)
    assert meta["seq"]["error"] is None and meta["seq"]["n_results"] == 12
    assert meta["first"]["error"] is not None and meta["first"]["n_results"] == 0
    assert meta["carry"]["error"] is None and meta["carry"]["n_results"] == 3
    np.savez_compressed(os.path.join(HERE, "heightpitch.npz"), meta=np.array(json.dumps(meta)), **store)
    print("wrote heightpitch.npz", os.path.getsize(os.path.join(HERE, "heightpitch.npz")), "bytes")


if __name__ == "__main__":
    main()
