#!/usr/bin/env python3
"""Generates tests/golden/scores.npz: the reference's own scoring of repeated runs — /root/reference/script/evaluate_vo.py
(calculate_sequence_error, calculate_ave_errors), script/transformation.py (motion2pose, pose2motion; get_path of
src/main_offline.py:114-119 is its motion2pose after the in-place scaling restated here), script/change_scale.py run as a
script on temporary files and calculate_speed.py's three lines — over the crafted sequences of tests/scores_cases.py.

Per sequence (data only): the inputs' checksum; the reference's segment table, speeds, rows (r_err/len, t_err/len per case),
per-length means, paths (cases 0 and C - 1: whole up to 300 frames, every 64th row beyond; the last pose of every case),
pose2motion / calculate_speed / change_scale outputs; and per quantity gap = max |reference - extended|, extended being the same
formulas (general affine inverse by the adjugate) in np.longdouble from the same float64 inputs.

Asserted here (conditions on the data, not measurements of the code under test): np.longdouble has at least 63 mantissa bits;
every gap is positive; in every noisy sequence each decisive dist comparison clears its threshold by at least 1e-6 m, so that a
last-bit difference in dist cannot move a segment end; the extended table equals the reference's.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_scores.py"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_SCRIPT = "/root/reference/script"
sys.path.insert(0, REF_SCRIPT)

import matplotlib                                             # noqa: E402
matplotlib.use("Agg")
import evaluate_vo as ev                                      # noqa: E402  (the reference's)
import transformation as tf                                   # noqa: E402  (the reference's)

import scores_cases as sc                                     # noqa: E402

LD = np.longdouble
MIN_MARGIN = 1e-6


def reference_get_path(motions, scales):
    """src/main_offline.py:114-119 (importing that file needs cv2): each translation times its scale — one multiplication, as
    offline.get_path has it —, then the reference's motion2pose (main_offline.py:100-111 is transformation.py:10-21)."""
    m = np.array(motions, dtype=np.float64, copy=True)
    m[:, 3:12:4] = m[:, 3:12:4] * np.asarray(scales, dtype=np.float64)[:, None]
    return tf.motion2pose(m)


def reference_change_scale(path, speed, tmp, tag):
    """script/change_scale.py itself on text files (np.savetxt's default format round-trips a double)."""
    src = os.path.join(tmp, "kitti_path.txt." + tag)
    spd = os.path.join(tmp, "speed_file")
    np.savetxt(src, path)
    np.savetxt(spd, speed)
    subprocess.run([sys.executable, os.path.join(REF_SCRIPT, "change_scale.py"), src, spd, tag], check=True, cwd=tmp)
    return np.loadtxt(os.path.join(tmp, "kitti_path_gt.txt" + tag)).reshape(-1, 12)


def gap_of(ref, ext, what):
    ref, ext = np.asarray(ref, dtype=LD), np.asarray(ext, dtype=LD)
    assert ref.shape == ext.shape, (what, ref.shape, ext.shape)
    if ref.size == 0 or np.isnan(ref).all():
        return 0.0
    g = float(np.nanmax(np.abs(ref - ext)))
    assert g > 0, (what, "gap must be positive")
    return g


def one_sequence(name, tmp):
    n, cases, seed, kind = sc.SEQUENCES[name]
    seq = sc.make_sequence(name)
    motions, scales, gt = seq["motions"], seq["scales"], seq["gt"]
    out = {"crc": np.int64(sc.checksum(seq))}
    # -- the reference
    paths = np.array([reference_get_path(motions, scales[c]) for c in range(cases)]).reshape(cases, n + 1, 12)
    dist = np.array(ev.trajectory_distances(gt), dtype=np.float64)
    last = np.full(((n + 1 + sc.STEP - 1) // sc.STEP, 8), -1, dtype=np.int32)
    for f, first in enumerate(range(0, n + 1, sc.STEP)):
        for k, length in enumerate(sc.LENGTHS):
            last[f, k] = ev.last_frame_from_segment_length(list(dist), first, int(length))
    rows_r, rows_t, tra, rot, meta_rows = [], [], [], [], None
    for c in range(cases):
        errors = ev.calculate_sequence_error(gt, paths[c])
        r, t, _ = ev.calculate_ave_errors(errors)
        e = np.array(errors, dtype=np.float64).reshape(-1, 5)
        rows_r.append(e[:, 1])
        rows_t.append(e[:, 2])
        tra.append(np.asarray(t, dtype=np.float64))
        rot.append(np.asarray(r, dtype=np.float64))
        meta_rows = e[:, [0, 3, 4]]
    rows_r, rows_t, tra, rot = np.array(rows_r), np.array(rows_t), np.array(tra), np.array(rot)
    f_idx, l_idx = np.nonzero(last >= 0)
    assert np.array_equal(meta_rows[:, 0], f_idx * sc.STEP) and np.array_equal(meta_rows[:, 1], sc.LENGTHS[l_idx]), "row order"
    columns = (last >= 0).any(axis=0)
    assert tra.shape == (cases, int(columns.sum()))
    # -- extended precision, from the same float64 inputs
    x_paths = sc.paths_restated(motions, scales, dtype=LD)
    x_dist = sc.distances(gt, dtype=LD)
    x_last, margin = sc.segment_table(x_dist)
    assert np.array_equal(x_last, last), "the extended table differs from the reference's"
    if kind != "exact" and margin.size:
        assert margin.min() >= MIN_MARGIN, (name, "a dist comparison is closer than 1e-6 m to its threshold", float(margin.min()))
    x_r, x_t, x_means = sc.score_restated(gt, x_paths, last, dtype=LD)
    x_tra, x_rot = x_means[:, 1, :][:, columns], x_means[:, 0, :][:, columns] * 180 / LD(np.pi)
    has = last >= 0
    gaps = {"poses": gap_of(paths, x_paths, "poses") if n else 0.0, "dist": gap_of(dist, x_dist, "dist") if kind != "exact" and n else 0.0}
    if has.any():
        gaps.update(rows_r=gap_of(rows_r, x_r[:, has], "rows_r"), rows_t=gap_of(rows_t, x_t[:, has], "rows_t"),
                    tra=gap_of(tra, x_tra, "tra"), rot=gap_of(rot, x_rot, "rot"))
    pc, pr = sc.pose_cases(name), sc.pose_rows(name)
    keep_rows = [0, cases - 1] if n > sc.FULL_POSES_UP_TO else list(range(cases))
    out.update(last=last, speed=meta_rows[:, 2], rows_cases=np.asarray(sorted(set(keep_rows)), dtype=np.int64),
               rows_r=rows_r[sorted(set(keep_rows))], rows_t=rows_t[sorted(set(keep_rows))], tra=tra, rot=rot,
               columns=columns, poses=paths[pc][:, pr], pose_end=paths[:, -1], margin=np.float64(margin.min() if margin.size else np.inf))
    # -- pose2motion, calculate_speed, change_scale: on the reference's own float64 paths (whole ones are kept up to 300 frames)
    if 1 < n <= sc.FULL_POSES_UP_TO:                         # (one step from the identity is exact: no gap to measure)
        gt_speed = sc_speed(tf.pose2motion(gt))
        x_m, x_norms = sc.pose2motion_restated(gt, dtype=LD)
        if kind == "exact":
            assert np.array_equal(gt_speed, np.full(n, 16.0)), "exact steps: every operation of the reference's is exact"
        else:
            gaps["gt_speed"] = gap_of(gt_speed, x_norms[0], "gt_speed")
        p2m = np.array([tf.pose2motion(paths[c]) for c in pc])
        gaps["p2m"] = gap_of(p2m, sc.pose2motion_restated(paths[pc], dtype=LD)[0], "p2m")
        cs = np.array([reference_change_scale(paths[c], gt_speed, tmp, "t%d" % c) for c in pc])
        gaps["cs"] = gap_of(cs, sc.change_scale_restated(paths[pc], gt_speed, dtype=LD), "cs")
        out.update(gt_speed=gt_speed, p2m=p2m, cs=cs)
    out["gaps"] = np.array(json.dumps(gaps))
    print("%-8s n %4d C %2d rows %4d columns %d margin %.3g gaps %s" % (name, n, cases, rows_r.shape[1], int(columns.sum()),
                                                                        float(out["margin"]), {k: "%.2e" % v for k, v in gaps.items()}))
    return out


def sc_speed(motion):
    """What script/calculate_speed.py:8-11 saves for the motions its pose2motion gave (the script itself runs on sys.argv at import)."""
    t = motion[:, 3:12:4]
    return np.sqrt(np.sum(t * t, 1))


def main():
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not extended precision here"
    arrays = {}
    with tempfile.TemporaryDirectory(prefix="scores") as tmp:
        assert "." not in tmp, "change_scale.py derives its output name by splitting the path at dots"
        for name in sc.SEQUENCES:
            for k, v in one_sequence(name, tmp).items():
                arrays["%s_%s" % (name, k)] = v
    # the exact-step sequence pins the strict comparison
    last = arrays["exact60_last"]
    assert last[0, 3] == 26 and last[0, 7] == 51, "dist[25] = 400 is not > 400"
    assert arrays["n65_tra"].shape[1] == 7 and arrays["n9_rows_r"].shape[1] == 1 and arrays["n257_tra"].shape[1] == 8
    assert arrays["n1_rows_r"].shape[1] == 0 and arrays["n0_rows_r"].shape[1] == 0
    arrays["meta"] = np.array(json.dumps({"numpy": np.__version__, "sequences": {k: list(v) for k, v in sc.SEQUENCES.items()}}))
    path = os.path.join(HERE, "scores.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("scores.npz", size, "bytes")
    assert size < 400 * 1024


if __name__ == "__main__":
    main()
