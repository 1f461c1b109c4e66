"""The device's pose arithmetic on the host: csrc/mvosr_score_math.hpp is plain C++, so g++ builds the very operations the
kernels of csrc/mvosr_score.hip run (-ffp-contract=off, like the library) and the segment errors and per-length means of every
crafted sequence are checked against the reference's outputs (tests/golden/scores.npz) under the rule of tests/scores_cases.py —
four gaps — without a GPU.  What differs on the device: its acos and its launch geometry, which tests/test_gpu_scores.py covers."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import scores_cases as sc
from conftest import ROOT, load_npz

SOURCE = r"""
#include "mvosr_score_math.hpp"
using namespace mvosr;
extern "C" void score_host(int n_cases, int rows, const double *paths, int n_first, const int *last, const double *gt,
                           double *r_seg, double *t_seg, double *means) {
    for (int c = 0; c < n_cases; ++c) {
        const double *P = paths + (long)c * rows * 12;
        for (int li = 0; li < 8; ++li) {
            double sr = 0.0, st = 0.0;
            int count = 0;
            for (int f = 0; f < n_first; ++f) {
                const int s = f * 8 + li, l = last[s];
                double r = NAN, t = NAN;
                if (l >= 0) {
                    bool zero;
                    const PoseDD g = ground_delta(pose_load(gt + f * 10 * 12), pose_load(gt + l * 12));
                    segment_error(pose_load(P + f * 10 * 12), pose_load(P + l * 12), g, 100.0 * (li + 1), &r, &t, &zero);
                    sr = sr + r; st = st + t; ++count;
                }
                r_seg[(long)c * n_first * 8 + s] = r;
                t_seg[(long)c * n_first * 8 + s] = t;
            }
            means[c * 16 + li] = count ? sr / count : NAN;
            means[c * 16 + 8 + li] = count ? st / count : NAN;
        }
    }
}
extern "C" void pose2motion_host(int n, const double *poses, double *motions) {
    for (int i = 0; i < n; ++i) {
        const Pose m = pose_mul(pose_inverse(pose_load(poses + i * 12)), pose_load(poses + (i + 1) * 12));
        for (int k = 0; k < 12; ++k) motions[i * 12 + k] = m.m[k];
    }
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_math")
    src, so = d / "score_host.cpp", d / "score_host.so"
    src.write_text(SOURCE)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mvoscalerecovery_amd", "csrc"),
                    str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    P = C.c_void_p
    lib.score_host.argtypes = [C.c_int, C.c_int, P, C.c_int, P, P, P, P, P]
    lib.pose2motion_host.argtypes = [C.c_int, P, P]
    return lib


@pytest.mark.parametrize("name", [k for k in sc.SEQUENCES if sc.SEQUENCES[k][0] >= 9])
def test_segment_errors_and_means_within_the_rule(host, name):
    z, _ = load_npz("scores.npz")
    g = json.loads(str(z[name + "_gaps"]))
    n, cases = sc.SEQUENCES[name][:2]
    seq = sc.make_sequence(name)
    last = np.ascontiguousarray(z[name + "_last"])
    has = last >= 0
    paths = np.ascontiguousarray(sc.paths_restated(seq["motions"], seq["scales"]))          # the kernel's chain order
    gt = np.ascontiguousarray(seq["gt"])
    F = last.shape[0]
    r, t, means = np.empty((cases, F, 8)), np.empty((cases, F, 8)), np.empty((cases, 2, 8))
    host.score_host(cases, n + 1, paths.ctypes.data, F, last.ctypes.data, gt.ctypes.data, r.ctypes.data, t.ctypes.data, means.ctypes.data)
    rc = z[name + "_rows_cases"]
    sc.within(r[rc][:, has], z[name + "_rows_r"], g["rows_r"], name + " r_err/len")
    sc.within(t[rc][:, has], z[name + "_rows_t"], g["rows_t"], name + " t_err/len")
    tra, rot = sc.scores_from_means(means, has.any(axis=0))
    sc.within(tra, z[name + "_tra"], g["tra"], name + " tra")
    sc.within(rot, z[name + "_rot"], g["rot"], name + " rot")
    assert np.isnan(r[:, ~has]).all()


def test_plain_product_and_inverse_equal_the_restatement(host):
    """pose_mul and pose_inverse in plain doubles are, operation for operation, tests/scores_cases.py's mul and inv."""
    z, _ = load_npz("scores.npz")
    poses = np.ascontiguousarray(z["n130_poses"][0])
    out = np.empty((poses.shape[0] - 1, 12))
    host.pose2motion_host(out.shape[0], poses.ctypes.data, out.ctypes.data)
    assert out.tobytes() == sc.pose2motion_restated(poses)[0][0].tobytes()
