"""CPU checks of the scoring cases (tests/scores_cases.py) against the reference's outputs in tests/golden/scores.npz: the crafted
sequences still come out of their seeds byte for byte; the vectorised NumPy restatement reproduces the reference's tables exactly
and its floats within one gap; the kernels' operation orders, restated for any float type, stay within the rule's four; the
conditions the sequences were designed for hold; the new exports are declared and bound and refuse bad arguments.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import scores_cases as sc
from conftest import ROOT, load_npz

NAMES = list(sc.SEQUENCES)


@pytest.fixture(scope="module")
def golden():
    z, _ = load_npz("scores.npz")
    return z


@pytest.fixture(scope="module")
def restated():
    """Every sequence through the restatement, once."""
    out = {}
    for name in NAMES:
        seq = sc.make_sequence(name)
        dist = sc.distances(seq["gt"])
        last, margin = sc.segment_table(dist)
        out[name] = dict(seq, dist=dist, last=last, margin=margin)
        for form, paths_of, score_of in (("np", sc.paths_numpy, sc.score_numpy), ("k", sc.paths_restated, sc.score_restated)):
            paths = paths_of(seq["motions"], seq["scales"])
            r, t, means = score_of(seq["gt"], paths, last)
            out[name][form] = dict(paths=paths, r_seg=r, t_seg=t, means=means)
    return out


def gaps_of(golden, name):
    return json.loads(str(golden[name + "_gaps"]))


@pytest.mark.parametrize("name", NAMES)
def test_inputs_come_out_of_their_seeds(golden, restated, name):
    assert sc.checksum(restated[name]) == int(golden[name + "_crc"])


@pytest.mark.parametrize("name", NAMES)
def test_restated_tables_equal_the_references(golden, restated, name):
    r = restated[name]
    assert np.array_equal(r["last"], golden[name + "_last"])
    has = r["last"] >= 0
    assert np.array_equal(has.any(axis=0), golden[name + "_columns"])
    f, li = np.nonzero(has)
    speed = sc.LENGTHS[li] / (0.1 * (r["last"][f, li] - f * sc.STEP + 1).astype(np.float64))
    assert np.array_equal(speed, golden[name + "_speed"])


@pytest.mark.parametrize("form,gaps", [("np", 1.0), ("k", sc.GAPS)])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_within_one_gap(golden, restated, name, form, gaps):
    """The vectorised restatement of the reference's formulation ("np": np.linalg.inv and matmul on stacks) within ONE gap of the
    reference's values; the kernels' operation orders ("k": adjugate inverse, k-ascending products, in float64) within the rule's
    four, like the device."""
    r, g = dict(restated[name], **restated[name][form]), gaps_of(golden, name)
    n, cases = sc.SEQUENCES[name][:2]
    pc, pr = sc.pose_cases(name), sc.pose_rows(name)
    if n:
        sc.within(r["paths"][pc][:, pr], golden[name + "_poses"], g["poses"], name + " poses", gaps=gaps)
        sc.within(r["paths"][:, -1], golden[name + "_pose_end"], g["poses"], name + " last pose", gaps=gaps)
    has = r["last"] >= 0
    if has.any():
        rc = golden[name + "_rows_cases"]
        sc.within(r["r_seg"][rc][:, has], golden[name + "_rows_r"], g["rows_r"], name + " r_err/len", gaps=gaps)
        sc.within(r["t_seg"][rc][:, has], golden[name + "_rows_t"], g["rows_t"], name + " t_err/len", gaps=gaps)
        tra, rot = sc.scores_from_means(r["means"], has.any(axis=0))
        sc.within(tra, golden[name + "_tra"], g["tra"], name + " tra", gaps=gaps)
        sc.within(rot, golden[name + "_rot"], g["rot"], name + " rot", gaps=gaps)
    if name + "_p2m" in golden.files:
        ref_paths = golden[name + "_poses"]                               # (whole paths at this length)
        m = sc.pose2motion_numpy(ref_paths) if form == "np" else sc.pose2motion_restated(ref_paths)[0]
        sc.within(m, golden[name + "_p2m"], g["p2m"], name + " pose2motion", gaps=gaps)
        norms = sc.pose2motion_restated(r["gt"])[1] if form == "k" else sc.norm3(sc.pose2motion_numpy(r["gt"])[None][..., 3:12:4])
        if form == "k":
            cs = sc.change_scale_restated(ref_paths, golden[name + "_gt_speed"])
            sc.within(cs, golden[name + "_cs"], g["cs"], name + " change_scale", gaps=gaps)
        if "gt_speed" in g:
            sc.within(norms[0], golden[name + "_gt_speed"], g["gt_speed"], name + " calculate_speed", gaps=gaps)
        else:
            assert np.array_equal(norms[0], golden[name + "_gt_speed"])


def test_design_conditions(golden, restated):
    """What the sequences were built for — conditions on the data, asserted by the generator too."""
    rows = {name: int((restated[name]["last"] >= 0).sum()) for name in NAMES}
    assert rows["n257"] == 180 and rows["n130"] == 78 and rows["n65"] == 25 and rows["n9"] == 1 and rows["n1"] == 0 and rows["n0"] == 0
    assert int(golden["n65_columns"].sum()) == 7 and golden["n65_tra"].shape == (3, 7) and golden["n257_tra"].shape == (10, 8)
    last = restated["n257"]["last"]
    assert (last[-5:, -1] == -1).all() and (last[0] >= 0).all()                   # late firsts lack the long lengths
    # exact steps of 16 m: dist is exact, dist[25] = 400 is not > 400
    ex = restated["exact60"]
    assert np.array_equal(ex["dist"], 16.0 * np.arange(61)) and ex["last"][0, 3] == 26 and ex["last"][0, 7] == 51
    for name in NAMES:
        n, cases, _, kind = sc.SEQUENCES[name]
        if kind != "exact" and restated[name]["margin"].size:
            assert restated[name]["margin"].min() >= 1e-6, name                    # a last-bit difference in dist moves no segment end
        for k, v in gaps_of(golden, name).items():
            assert v > 0 or n == 0 or (k == "dist" and kind == "exact"), (name, k)
        if n > 30:
            assert (restated[name]["scales"] == 0).any(), name                     # not-moving frames
    assert {sc.SEQUENCES[k][1] for k in NAMES} == {1, 3, 10}
    # ground truth and result rotate about 1e-3 rad apart per step; in same130 not at all
    for name, lo, hi in (("n257", 2e-4, 2e-3), ("same130", 0.0, 0.0)):
        r = restated[name]
        step_gt = sc.pose2motion_restated(r["gt"])[0][0].reshape(-1, 3, 4)[:, :, :3]
        step_re = r["motions"].reshape(-1, 3, 4)[:, :, :3]
        tr = np.einsum("nij,nij->n", step_gt, step_re)
        ang = np.arccos(np.clip(0.5 * (tr - 1), -1, 1))
        if hi == 0.0:
            assert np.abs(step_gt - step_re).max() < 1e-12
        else:
            assert lo < np.median(ang) < hi, np.median(ang)
    assert 1e-11 < gaps_of(golden, "same130")["rows_r"] < 1e-9                    # arccos's rounding noise, per metre


def test_header_and_binding():
    from mvoscalerecovery_amd import _lib
    with open(os.path.join(ROOT, "include", "mvosr.h")) as fh:
        header = fh.read()
    for name, n_args in (("mvosr_paths_batch", 7), ("mvosr_segment_table", 7), ("mvosr_score_cases_batch", 12),
                         ("mvosr_pose2motion_batch", 8), ("mvosr_score_firsts", 1)):
        assert re.search(r"\b%s\(" % name, header) and len(_lib.SYMBOLS[name][1]) == n_args, name
    assert "#define MVOSR_SCORE_LENGTHS %d" % _lib.SCORE_LENGTHS in header and "#define MVOSR_SCORE_STEP %d" % _lib.SCORE_STEP in header
    lib = _lib.load()
    assert [lib.mvosr_score_firsts(n) for n in (0, 1, 10, 11, 4542)] == [0, 1, 1, 2, 455]


def test_host_entry_points_refuse_without_launching():
    """Null pointers and C < 1 are refused before any device work (no GPU here: a launch would fail differently)."""
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    one = 0x1000
    assert lib.mvosr_paths_batch(None, 1, 1, one, 0, None, one) == -2
    assert lib.mvosr_segment_table(None, 1, one, one, one, one, one) == -2
    assert lib.mvosr_score_cases_batch(None, 1, 1, one, 0, None, None, None, None, one, one, one) == -2
    assert lib.mvosr_pose2motion_batch(None, 1, 1, one, None, one, None, one) == -2
    assert b"null" in lib.mvosr_last_error()


def test_python_surface_exists():
    from mvoscalerecovery_amd import evaluate, offline
    from mvoscalerecovery_amd.rescale import RepeatedRuns
    assert callable(offline.get_path_batch) and callable(evaluate.calculate_speed) and callable(evaluate.change_scale)
    assert all(hasattr(evaluate.Scorer, k) for k in ("score_scales", "score_paths", "errors"))
    assert callable(RepeatedRuns.scores)
    tra = np.arange(6.0).reshape(2, 3)
    with pytest.raises(ValueError):
        evaluate._reduce_scores(tra, tra)                                           # fewer than three cases
