"""The crafted clouds of tests/test_gpu_ransac.py checked without a GPU: every family stays within its share of undecided
hypotheses under the np.longdouble reference alone, the counts the constructions promise are what the bounds give, M * 0.8 is the
integer the goal families assume, and the three references — the bounds, the float64 restatement of the kernel's expressions and
the oracle's SVD models (oracle.rescale_oracle.run_ransac / run_ransac_line) — agree with one another."""
import numpy as np
import pytest

import ransac_cases as rc


@pytest.fixture(scope="module")
def cases():
    return rc.cases()


def test_goal_products_and_level_sizes():
    for M in rc.GOAL_M:
        assert (float(M) * rc.GOAL).is_integer(), M
        a, b, c, r1, r2 = rc.SIZES[M]
        assert a + b + c + r1 + r2 == M and float(a + b) == float(M) * rc.GOAL and r1 == r2
        cnt = rc.level_counts(rc.SIZES[M])
        assert cnt[:3] == [a + b, a + b + c, b + c] and cnt[3:] == [r1, r2]
    assert not (64 * rc.GOAL).is_integer() and not (4096 * rc.GOAL).is_integer()


def test_sizes_cover_the_boundaries(cases):
    ms = {c.M for c in cases.values()}
    assert set(rc.POINT_COUNTS) <= ms and 8193 + 37 in ms
    assert set(rc.N_HYPS) <= {c.H for c in cases.values()}
    assert max(c.M for c in cases.values()) == 8230 and cases["road_8230"].H == 512


def test_undecided_share_and_promised_counts(cases):
    """Per family at most 2 % of the hypotheses may have lo != hi, none in a pinned one — plane and line; where the construction
    promises a count, both bounds equal it."""
    for name, c in cases.items():
        for line in (False, True):
            lo, hi = rc.bounds(c, line)
            und = int((lo != hi).sum())
            assert und <= (0 if c.pinned else 0.02 * c.H), (name, line, und, c.H)
        lo, hi = rc.bounds(c, False)
        if c.expect is not None:
            k = c.expect >= 0
            assert np.array_equal(lo[k], c.expect[k]) and np.array_equal(hi[k], c.expect[k]), (name, lo[k][:8], c.expect[k][:8])
        if c.zero:
            assert not lo.any() and not hi.any()


def test_tail_decides_the_best(cases):
    """M > 4096: the best hypothesis is B's only through the points of the last, partly filled chunk — without them A (the
    first hypothesis) stays the best; and every B hypothesis counts every point of the tail."""
    for M in (4097, 8230):
        c = cases["road_%d" % M]
        lo, _ = rc.bounds(c)
        best, ic, _ = rc.replay(lo, c.M, c.goal)
        n_tail = (M - 1) % rc.CHUNK + 1
        cut = rc.Case("cut", c.pts[:M - n_tail], c.samples, pinned=True)
        _, cnt = rc.numpy_model(cut)                                          # (a sample from the tail is out of range now: count 0)
        best_cut, ic_cut, _ = rc.replay(cnt, cut.M, c.goal)
        assert best != best_cut and ic == ic_cut + n_tail, (M, best, best_cut, ic, ic_cut)
        assert abs(c.pts[c.samples[best], 1] - 2.5).max() == 0 and abs(c.pts[c.samples[best_cut], 1] - 1.7).max() == 0


def test_replay_tables_are_what_their_notes_say(cases):
    want = {"tie": lambda c: (1, c.expect[1], c.H), "goal_equal": None, "goal_stop": lambda c: (3, c.expect[3], 4),
            "later_larger": lambda c: (1, c.expect[1], 2), "never": lambda c: (2, c.expect[2], c.H)}
    seen = set()
    for name, c in cases.items():
        kind = name.rsplit("_", 1)[0]
        if kind not in want:
            continue
        seen.add(kind)
        got = rc.replay(c.expect, c.M, c.goal)
        if kind == "goal_equal":
            goal = float(c.M) * c.goal
            first = int(np.argmax(c.expect == goal))
            assert c.expect[first] == goal                                   # a count EQUAL to the goal is in the table ...
            if c.M == 10:
                assert got == (3, 10, 4)                                       # ... does not stop the loop; the first count above it does
            else:
                assert got == (first, int(goal), c.H)
        else:
            assert got == want[kind](c), (name, got)
        if kind == "tie":
            assert c.expect[1] == c.expect[2] == c.expect.max() and c.pts[c.samples[1, 0], 1] != c.pts[c.samples[2, 0], 1]
        if kind == "later_larger":
            assert c.expect[2:].max() > c.expect[1] > float(c.M) * c.goal
    assert seen == set(want)


def test_wide_replay_tables_are_what_their_notes_say(cases):
    """The tables of 130 hypotheses (the replay runs 64 at a time): the module's sequential restatement of ransac.py:9-22 gives what
    the construction promises, the promised counts are what both bounds give for the plane AND the line (a spent row is spent for
    both), and the designs hold: where the first count above the goal lies, which rows tie, what lies behind a stop."""
    wide = {n: c for n, c in cases.items() if n.startswith("wide_")}
    assert len(wide) == len(rc.WIDE_STOPS) + 4 and rc.SIZES[rc.WIDE_M] == min((s for s in rc.SIZES.items() if all(s[1])), key=lambda s: s[0])[1]
    for name, c in wide.items():
        assert c.H == rc.WIDE_H == 2 * 64 + 2 and c.M == rc.WIDE_M and c.pinned
        want = rc.wide_expected(c)
        assert rc.replay(c.expect, c.M, c.goal) == want, (name, rc.replay(c.expect, c.M, c.goal), want)
        for line in (False, True):
            lo, hi = rc.bounds(c, line)
            assert np.array_equal(lo, c.expect) and np.array_equal(hi, c.expect), (name, line)
            assert np.array_equal(rc._spent(c, line)[0], c.expect == 0), (name, line)
        goal = float(c.M) * c.goal
        over = np.nonzero(c.expect > goal)[0]
        kind = name[len("wide_"):].rsplit("_", 1)[0]
        if kind.startswith("stop"):
            assert over[0] == want[0] and c.expect[:want[0]].max() < c.expect[want[0]]
        else:
            assert len(over) == 0
        if kind.startswith("stop") and kind != "stop_then_larger":
            assert c.expect[0] == goal and want[0] in rc.WIDE_STOPS                 # (a count equal to the goal before it: no stop there)
        if kind == "stop_then_larger":
            assert c.expect[63] > c.expect[62] and c.expect[64:128].max() > c.expect[62] and c.expect[128:].max() > c.expect[62]
        if kind in ("tie_adjacent", "tie_apart"):
            i, j = np.nonzero(c.expect)[0]
            assert (i, j) == ((63, 64) if kind == "tie_adjacent" else (64, 128)) and c.expect[i] == c.expect[j]
            assert c.pts[c.samples[i, 0], 1] != c.pts[c.samples[j, 0], 1]         # two levels: the model tells which one won
        if kind == "goal_exact":
            assert c.expect[0] == goal and not c.expect[1:].any()


def test_float64_restatement_within_the_bounds(cases):
    """The kernel's expressions in float64 NumPy: counts between lo and hi, the model of every hypothesis that can have one within
    the derived tolerance of the np.longdouble one (and NaN for the spent ones); prints the share of the tolerance it uses."""
    for line in (False, True):
        worst = 0.0
        for name, c in cases.items():
            m, cnt = rc.numpy_model(c, line)
            lo, hi = rc.bounds(c, line)
            assert np.all((lo <= cnt) & (cnt <= hi)), (name, line, np.nonzero((cnt < lo) | (cnt > hi))[0][:8])
            spent, _ = rc._spent(c, line)
            assert np.isnan(m[spent]).all()
            for h in np.nonzero(~spent)[0][:64]:
                ref, tol = rc.model_ld(c, h, line)
                err = float(np.abs(rc.sign_rule(m[h]).astype(np.longdouble) - ref).max())
                assert err <= tol, (name, line, h, err, tol)
                worst = max(worst, err / tol)
                if line:
                    assert m[h, 2] == 0.0
        kind = "line" if line else "plane"
        print("largest |m_float64 - m_longdouble| / tolerance, %s: %.3f" % (kind, worst))
        assert worst <= rc.MODEL_SHARE_MEASURED[kind]


def test_sign_cases_are_what_their_notes_say(cases):
    m = {n: rc.numpy_model(cases[n])[0][0] for n in ("sign_pos", "sign_neg", "sign_zero_a", "sign_zero_b")}
    assert m["sign_pos"][1] > 0 and m["sign_neg"][1] < 0
    assert m["sign_zero_a"][1] == 0 and m["sign_zero_b"][1] == 0 and m["sign_zero_a"][0] * m["sign_zero_b"][0] < 0
    ml = {n: rc.numpy_model(cases[n], True)[0][0] for n in ("sign_line_pos", "sign_line_neg", "sign_zero_a", "sign_zero_b")}
    assert ml["sign_line_pos"][1] > 0 and ml["sign_line_neg"][1] < 0
    assert ml["sign_zero_a"][1] == 0 and ml["sign_zero_b"][1] == 0 and ml["sign_zero_a"][0] * ml["sign_zero_b"][0] < 0


def test_oracle_svd_models_agree(cases):
    """oracle.rescale_oracle.run_ransac / run_ransac_line (SVD null vectors) on the same tables: best count and hypotheses used
    equal the replay of the bounds (which coincide), the model that of the replay's best hypothesis to 1e-9 (what the suite asks
    of the SVD models elsewhere).  Left out: tables the oracle has no rule for (NaN coordinates, indices out of range, threshold 0
    — and for the line oracle a repeated pair, whose rank-1 SVD is arbitrary)."""
    from oracle import rescale_oracle as ro
    n = 0
    for name, c in cases.items():
        if c.zero or np.isnan(c.pts).any() or name == "index_guard":
            continue
        for line in (False, True):
            spent, _ = rc._spent(c, line)
            lo, hi = rc.bounds(c, line)
            if (lo != hi).any() or (line and spent.any()):
                continue
            if line:
                m, ic, used = ro.run_ransac_line(c.pts[:, :2], c.samples[:, :2], c.threshold, c.goal)
            else:
                m, ic, used = ro.run_ransac(c.pts, c.samples, c.threshold, c.goal, repeated_counts_zero=True)
            best, best_ic, want_used = rc.replay(lo, c.M, c.goal)
            assert (ic, used) == (best_ic, want_used), (name, line, ic, used, best_ic, want_used)
            assert (m is None) == (best < 0)
            if best >= 0:
                ref, _ = rc.model_ld(c, best, line)
                m4 = np.array([m[0], m[1], 0.0, m[2]]) if line else np.asarray(m)
                r64 = ref.astype(np.float64)                                   # (the SVD's null vector has an arbitrary sign)
                assert min(np.abs(m4 - r64).max(), np.abs(m4 + r64).max()) <= 1e-9, (name, line, m4, ref)
            n += 1
    assert n >= 40


def test_mask_cases_undecided_share():
    """At most 1 % of a mask case's points are within eps of the threshold, both verdicts occur, and float64 NumPy gives the
    np.longdouble verdict wherever it is decided."""
    for n in rc.MASK_SIZES:
        pts, model = rc.mask_case(n)
        verdict, decided = rc.mask_reference(pts, model)
        assert (~decided).mean() <= 0.01, (n, int((~decided).sum()))
        if n > 1:
            assert verdict.any() and not verdict.all()
        got = np.abs(((pts[:, 0] * model[0] + pts[:, 1] * model[1]) + pts[:, 2] * model[2]) + model[3]) < rc.MASK_THRESHOLD
        assert np.array_equal(got[decided], verdict[decided])
