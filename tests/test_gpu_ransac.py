"""ransac_plane_kernel (plane and line) and plane_inliers_kernel (csrc/mvosr_rescale.hip) on crafted clouds, through the C entry
points with hand-built buffers: the chunk loop and its partly filled tail (M up to 8230), ragged batches with frames of no points,
the replay rule at its edges (tie, count equal to the goal, first count above it, goal never reached), spent samples (an index
repeated or out of range, a NaN coordinate), the sign rule, threshold 0.  Needs a real MI355X.

Inlier counts between np.longdouble bounds (flat_cases.count_bounds; ransac_cases.line_count_bounds for the line, eps derived above
ransac_cases._line_terms) — equal in every pinned family, so the counts are exact there —, then ransac.py's rule replayed on the
kernel's OWN counts for best_ic / used / the best hypothesis, whose model must lie within flat_cases.plane_ld's (ransac_cases.line_ld's)
derived tolerance of the np.longdouble model after the sign rule.  The float64 restatement of the kernel's expressions uses 0.04 /
0.07 of those tolerances on the CPU (tests/test_ransac_cases.py).  The mask: the np.longdouble verdict wherever
| |r| - threshold | > 2 * 4.1 u (sum |p_i n_i| + |d|).  Clouds, references and launchers: tests/ransac_cases.py."""
import numpy as np
import pytest

import ransac_cases as rc

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_frame(a, b):
    return _same(a["counts"], b["counts"]) and _same(a["model"], b["model"]) and a["best_ic"] == b["best_ic"] and a["used"] == b["used"]


@pytest.fixture(scope="module")
def cases():
    return rc.cases()


@pytest.fixture(scope="module")
def runs(gpu, cases):
    """(name, line) -> the outputs of the case launched alone with its own table."""
    return {(n, line): rc.run_ransac(gpu, [c], line)[0] for n, c in cases.items() for line in (False, True)}


def _check(c, line, o, tag):
    lo, hi = rc.bounds(c, line)
    cnt = o["counts"].astype(np.int64)
    assert np.all((lo <= cnt) & (cnt <= hi)), (tag, np.nonzero((cnt < lo) | (cnt > hi))[0][:8], cnt[:8], lo[:8], hi[:8])
    spent, _ = rc._spent(c, line)
    assert not cnt[spent].any(), (tag, "a spent sample counts nothing")
    if c.zero:
        assert not cnt.any(), (tag, "threshold 0: nothing counts")
    if c.expect is not None and not line:
        k = c.expect >= 0
        assert np.array_equal(cnt[k], c.expect[k]), (tag, cnt[k][:8], c.expect[k][:8])
    best, best_ic, used = rc.replay(cnt, c.M, c.goal)
    assert (o["best_ic"], o["used"]) == (best_ic, used), (tag, o["best_ic"], o["used"], best_ic, used)
    m = o["model"]
    if best < 0:
        assert np.isnan(m).all(), (tag, m)
    else:
        ref, tol = rc.model_ld(c, best, line)
        err = float(np.abs(m.astype(np.longdouble) - ref).max())
        assert err <= tol, (tag, best, m, ref, err, tol)
        assert m[1] >= 0, (tag, m)
        if line:
            assert m[2] == 0.0, (tag, m)
    return best


def test_counts_replay_and_model(runs, cases):
    """Every case, plane and line, launched alone: counts within the bounds (exact where they coincide: every pinned family),
    best_ic / used from the replay of the kernel's own counts, the model within the derived tolerance of the np.longdouble one."""
    for (name, line), o in runs.items():
        _check(cases[name], line, o, (name, "line" if line else "plane"))


def test_replay_rule_at_its_edges(runs, cases):
    """The tables of ransac_cases.replay_cases, from the kernel's outputs alone: the first of two tied best counts wins (its
    plane, not the other's), a count equal to the goal does not stop the loop, the first count above it does and later larger
    counts are ignored, and a goal never reached consumes every hypothesis."""
    seen = set()
    for (name, line), o in runs.items():
        kind, c = name.rsplit("_", 1)[0], cases[name]
        if line or kind not in ("tie", "goal_equal", "goal_stop", "later_larger", "never"):
            continue
        seen.add(kind)
        level = lambda h: c.pts[c.samples[h, 0], 1]
        if kind == "tie":
            assert (o["best_ic"], o["used"]) == (int(c.expect[1]), c.H)
            assert abs(-o["model"][3] / o["model"][1] - level(1)) < 1e-9 and level(1) != level(2)
        elif kind == "goal_equal" and c.M != 10:
            assert float(o["best_ic"]) == float(c.M) * c.goal and o["used"] == c.H
        elif kind == "goal_equal":
            assert (o["best_ic"], o["used"]) == (10, 4)
        elif kind == "goal_stop":
            assert (o["best_ic"], o["used"]) == (int(c.expect[3]), 4)
        elif kind == "later_larger":
            assert (o["best_ic"], o["used"]) == (int(c.expect[1]), 2) and o["counts"][2:].max() > o["best_ic"]
            assert abs(-o["model"][3] / o["model"][1] - level(1)) < 1e-9
        else:
            assert (o["best_ic"], o["used"]) == (int(c.expect[2]), c.H)
    assert len(seen) == 5


def test_replay_rule_across_blocks_of_64(runs, cases):
    """The tables of 130 hypotheses (ransac_cases.replay_cases, `wide_*`), plane and line: the kernel replays 64 counts at a time, so
    the first count above the goal is placed at the last lane of a block, the first two of the next and the last lane of the ragged
    block, ties straddle an edge and lie two blocks apart, larger counts follow a stop, and a count equal to the goal stands alone.
    Counts as constructed, best_ic / used as the sequential restatement of ransac.py:9-22 gives them, the model the best row's level."""
    seen = 0
    for (name, line), o in runs.items():
        if not name.startswith("wide_"):
            continue
        seen += 1
        c = cases[name]
        assert np.array_equal(o["counts"].astype(np.int64), c.expect), (name, line)
        best, best_ic, used = rc.replay(c.expect, c.M, c.goal)
        assert (best, best_ic, used) == rc.wide_expected(c)
        assert (o["best_ic"], o["used"]) == (best_ic, used), (name, line, o["best_ic"], o["used"], best_ic, used)
        assert abs(-o["model"][3] / o["model"][1] - c.pts[c.samples[best, 0], 1]) < 1e-9, (name, line, o["model"])
    assert seen == 2 * (len(rc.WIDE_STOPS) + 4)


def test_degenerate_and_guarded_samples(runs, cases):
    """Every hypothesis spent: best_ic 0, NaN model, used == H (M = 1, M = 2 in 3-D, the all-degenerate table); indices M, -1 and
    2^31 - 1 among valid samples count nothing and the valid ones around them count as usual (checked against the bounds in
    test_counts_replay_and_model); the line variant does not read the third column (garbage there, and for `index_guard` the
    out-of-range values of column 2 replaced: those hypotheses are valid again)."""
    for name in ("road_1", "road_2", "all_degenerate"):
        o, c = runs[name, False], cases[name]
        assert o["best_ic"] == 0 and o["used"] == c.H and np.isnan(o["model"]).all() and not o["counts"].any(), name
    o = runs["road_1", True]
    assert o["best_ic"] == 0 and o["used"] == cases["road_1"].H and np.isnan(o["model"]).all()
    c = cases["index_guard"]
    sp, spl = rc._spent(c, False)[0], rc._spent(c, True)[0]
    assert sp.sum() >= 22 and spl.sum() < sp.sum()
    assert runs["index_guard", True]["counts"][sp & ~spl].all()
    # the sign rule at n_y == 0 (b == 0): kept as sampled — the two orientations are each other's negative
    for line in (False, True):
        a, b = runs["sign_zero_a", line]["model"], runs["sign_zero_b", line]["model"]
        assert a[1] == 0 and b[1] == 0 and a[0] * b[0] < 0 and a[3] * b[3] < 0, (line, a, b)


def _batch_frames(cases):
    """Every case that shares the launch's threshold and goal (all but `threshold_zero` and the goal-0.25 tables), its table
    resized to BATCH_H, with a frame of no points first, in the middle and last."""
    fr = [c.resized(rc.BATCH_H) for c in cases.values() if c.threshold == rc.THRESHOLD and c.goal == rc.GOAL]
    k = len(fr) // 2
    return [None] + fr[:k] + [None] + fr[k:] + [None]


@pytest.mark.parametrize("line", (False, True), ids=("plane", "line"))
def test_ragged_batch(gpu, cases, runs, line):
    """One batch of every family, the frames scrambled in the point planes with odd gaps of garbage between them and M == 0
    frames first, in the middle and last: equal to each frame launched alone bit for bit, two launches bit-identical, the frames
    of no points with a NaN model, best_ic = used = 0 and counts all zero (the buffer is pre-filled with 0xFF bytes)."""
    frames = _batch_frames(cases)
    assert len(frames) >= 40 and {f.M for f in frames if f is not None} >= set(rc.POINT_COUNTS)
    b1 = rc.run_ransac(gpu, frames, line, rc.BATCH_H, ragged=True)
    b2 = rc.run_ransac(gpu, frames, line, rc.BATCH_H, ragged=True)
    for i, f in enumerate(frames):
        assert _same_frame(b1[i], b2[i]), (i, "two launches differ")
        if f is None:
            o = b1[i]
            assert np.isnan(o["model"]).all() and o["best_ic"] == 0 and o["used"] == 0 and not o["counts"].any(), (i, o)
            continue
        alone = rc.run_ransac(gpu, [f], line, rc.BATCH_H)[0]
        assert _same_frame(b1[i], alone), (f.name, "batch != alone")
        own = runs[f.name, line]["counts"]
        assert np.array_equal(b1[i]["counts"], np.resize(own, rc.BATCH_H)), f.name
        _check(f, line, b1[i], (f.name, "batch", line))


def test_counts_output_is_optional(gpu, cases, runs):
    for name in ("road_513", "road_4097", "goal_stop_100"):
        for line in (False, True):
            o = rc.run_ransac(gpu, [cases[name]], line, want_counts=False)[0]
            r = runs[name, line]
            assert _same(o["model"], r["model"]) and (o["best_ic"], o["used"]) == (r["best_ic"], r["used"])
            assert (o["counts"] == -1).all()                                 # (the launcher's buffer, never handed over)


def test_wrappers_equal_the_direct_calls(gpu, cases, runs):
    """estimate_road_norm.get_pitch_ransac / get_pitch_line_ransac with the table given against the direct calls."""
    from mvoscalerecovery_amd import estimate_road_norm as ern
    for name in ("road_513", "grid", "sign_neg"):
        c = cases[name]
        m, ic = ern.get_pitch_ransac(c.pts, c.H, c.threshold, triples=c.samples)
        assert _same(m, runs[name, False]["model"]) and ic == runs[name, False]["best_ic"], name
        m, ic = ern.get_pitch_line_ransac(c.pts[:, :2], c.H, c.threshold, pairs=c.samples[:, :2])
        r = runs[name, True]
        assert _same(m, r["model"][[0, 1, 3]]) and ic == r["best_ic"], name


# ---- plane_inliers_kernel -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def masks():
    return {n: rc.mask_case(n) + rc.mask_reference(*rc.mask_case(n)) for n in rc.MASK_SIZES}


def test_mask_against_longdouble(gpu, masks):
    """mask[i] equals the np.longdouble verdict wherever it is decided; the bytes are 0 or 1; the bytes behind mask[n - 1] are
    untouched."""
    for n, (pts, model, verdict, decided) in masks.items():
        mask, guard = rc.run_mask(gpu, pts, model)
        assert set(np.unique(mask).tolist()) <= {0, 1}, n
        assert (guard == 0xA5).all(), n
        assert np.array_equal(mask[decided].astype(bool), verdict[decided]), (n, np.nonzero(mask.astype(bool) != verdict)[0][:8])
        assert (~decided).mean() <= 0.01


def test_mask_edges(gpu, masks):
    pts, model, verdict, _ = masks[257]
    assert verdict.any()
    mask, guard = rc.run_mask(gpu, pts, np.array([model[0], np.nan, model[2], model[3]]))
    assert not mask.any() and (guard == 0xA5).all()                           # a NaN model: nothing is an inlier
    mask, _ = rc.run_mask(gpu, pts, model, threshold=0.0)
    assert not mask.any()                                                     # threshold 0: |r| < 0 never holds
    on = np.nonzero(verdict)[0][:6]
    p2 = pts.copy()
    for k, i in enumerate(on):
        p2[i, k % 3] = np.nan
    mask, _ = rc.run_mask(gpu, p2, model)
    assert not mask[on].any() and np.array_equal(np.delete(mask, on), np.delete(rc.run_mask(gpu, pts, model)[0], on))
    mask, guard = rc.run_mask(gpu, pts, model, n=0)                           # n == 0: OK, nothing touched
    assert len(mask) == 0 and (guard == 0xA5).all()


def test_get_inliers_equals_the_direct_call(gpu, masks):
    from mvoscalerecovery_amd import estimate_road_norm as ern
    for n in (257, 100003):
        pts, model, _, _ = masks[n]
        got = ern.get_inliers(model, pts, rc.MASK_THRESHOLD)
        assert got.dtype == bool and np.array_equal(got, rc.run_mask(gpu, pts, model)[0].astype(bool))
