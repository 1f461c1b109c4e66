"""The headline kernels on the crafted frames of tests/scale_cases.py: the packed 16-bit vote counters at the ends of their range,
the survivors' compaction through every (WAVES, SC) instantiation and the dense two-sweep kernel, the division-free pitch test on
both sides of its band, `h > level` at equality, the per-thread flag words at bit 63, and which frames the HOT kernel hands to
the exact pass.  Every comparison is equality with the oracle (or, for a row's pitch, with the np.longdouble truth on the rows
the decidability rule of scale_cases.py keeps); the over-limit inputs are ones the kernels refuse with MVOSR_ST_ERR_MASK."""
import numpy as np
import pytest

import scale_cases as sc
from oracle import scale_oracle as so

pytestmark = pytest.mark.gpu

NOMINAL_MAX_LDS = 6208
N_PLAN = len(sc.compaction_plan(NOMINAL_MAX_LDS))


def _K():
    from mvoscalerecovery_amd import constants as K
    return K


def _want_status(c):
    return c.status if c.status is not None else c.oracle().status


def _same(got, want):
    return (np.isnan(got) and np.isnan(want)) or got == want


def _check_hot(c, res, f, tag, tri_valid=True):
    """What a launch without stage outputs reports, against the oracle: status, raw scale, height and the counts (`tri_valid`: the
    tiled kernel marks vertices by height keys and does not count the rows above the level)."""
    K, r = _K(), c.oracle()
    assert res["status"][f] == _want_status(c), (tag, c.name, res["status"][f], _want_status(c))
    if c.status is not None:
        return
    assert _same(res["raw_scale"][f], r.raw_scale) and _same(res["height"][f], r.height), (tag, c.name, res["raw_scale"][f], r.raw_scale)
    assert res["counts"][f, K.CNT_VALID] == int(r.valid.sum()), (tag, c.name)
    if r.status != so.ST_ERR_SINGULAR:
        assert res["counts"][f, K.CNT_TRI_PITCH] == int(r.sel.valid_pitch.sum()), (tag, c.name)
        assert not tri_valid or res["counts"][f, K.CNT_TRI_VALID] == int(r.sel.tri_valid.sum()), (tag, c.name)
        assert res["counts"][f, K.CNT_SELECTED] == len(r.sel.selected_ids), (tag, c.name)


def _check_exact(c, res, pf, f, tag):
    """Stage outputs: counters, mask, selected set, height_level bitwise, counts, histograms, raw scale and status."""
    if c.status is not None or c.oracle().status == so.ST_ERR_SINGULAR:       # (refused / raised: the status, and the vote before it)
        assert res["status"][f] == _want_status(c), (tag, c.name, res["status"][f])
        if c.status is None:
            assert np.array_equal(res["vote_counters"][pf.frame_slice(f)], c.oracle().counters), (tag, c.name)
        return
    K, r, sl = _K(), c.oracle(), pf.frame_slice(f)
    nv = int(r.valid.sum())
    assert res["status"][f] == r.status, (tag, c.name, res["status"][f], r.status)
    assert np.array_equal(res["vote_counters"][sl], r.counters), (tag, c.name)
    assert res["counts"][f, K.CNT_VALID] == nv, (tag, c.name)
    assert np.array_equal(np.nonzero(res["selected"][sl][:nv])[0], r.sel.selected_ids), (tag, c.name)
    assert res["counts"][f, K.CNT_TRI_PITCH] == int(r.sel.valid_pitch.sum()), (tag, c.name)
    assert res["counts"][f, K.CNT_TRI_VALID] == int(r.sel.tri_valid.sum()), (tag, c.name)
    assert res["counts"][f, K.CNT_SELECTED] == len(r.sel.selected_ids), (tag, c.name)
    for name, want in (("height_level", r.height_level), ("height", r.height), ("raw_scale", r.raw_scale)):        # bitwise
        assert _same(res[name][f], want), (tag, c.name, name, res[name][f], want)
    if r.road is not None and "hist" in res:
        assert np.array_equal(res["hist"][f, 0], r.road.hist_raw) and np.array_equal(res["hist"][f, 1], r.road.hist), (tag, c.name)
        assert res["counts"][f, K.CNT_KEPT] == r.road.n_kept and res["counts"][f, K.CNT_MODES] == r.road.n_modes, (tag, c.name)
        assert res["counts"][f, K.CNT_MODE_LEFT] == r.road.mode_left and res["counts"][f, K.CNT_MODE_RIGHT] == r.road.mode_right, (tag, c.name)


def _check_full(c, res, pf, f, tag):
    """Per-triangle outputs: heights bitwise, and the pitch decision against the truth on the decided rows.  Returns their number."""
    assert res["status"][f] == _want_status(c), (tag, c.name, res["status"][f], _want_status(c))
    if c.status is not None:
        return 0
    r = c.oracle()
    rows = slice(int(pf.tri2_off[f]), int(pf.tri2_off[f + 1]))
    assert np.array_equal(res["tri_heights"][rows], r.sel.heights), (tag, c.name)
    if r.status == so.ST_ERR_SINGULAR:
        return 0
    dec, flat = sc.decided_rows(c)
    with np.errstate(invalid="ignore"):
        got = res["tri_pitch_deg"][rows] < sc.THR_DEG
    assert np.array_equal(got[dec], flat[dec]), (tag, c.name, np.nonzero(got[dec] != flat[dec])[0][:5])
    assert _same(res["raw_scale"][f], r.raw_scale), (tag, c.name)
    if dec.all():                                                # (FULL is EXACT plus the per-triangle outputs: the same stage outputs)
        _check_exact(c, res, pf, f, tag)
    return int(dec.sum())


# ---------------------------------------------------------------------------------------------------------------- vote family
@pytest.fixture(scope="module")
def votes():
    cases = sc.vote_cases()
    out = {}
    for vote in ("reference", "fixed"):
        mine = [c for c in cases if c.vote == vote]
        refused = [c for c in mine if c.status is not None]
        assert len(refused) == 1
        mine.remove(refused[0])
        mine.insert(len(mine) // 2, refused[0])                # (the refused frame has neighbours on both sides)
        out[vote] = mine
    return out


@pytest.mark.parametrize("vote", ["reference", "fixed"])
def test_vote_counters_through_the_vote_kernel(gpu, votes, vote):
    K, cases = _K(), votes[vote]
    for waves in (1, 4, 8, 16):
        pf, st, cnt, counts = sc.run_vote(gpu, cases, waves=waves, vote=vote)
        for f, c in enumerate(cases):
            if c.status is not None:                            # 32 766 rows: refused, and only this frame
                assert st[f] == K.ST_ERR_MASK, (waves, c.name)
                continue
            want = c.votes()
            assert st[f] == 0 and np.array_equal(cnt[pf.frame_slice(f)], want), (waves, c.name, np.nonzero(cnt[pf.frame_slice(f)] != want)[0][:8])
            assert counts[f, K.CNT_VALID] == int((want >= 0).sum()), (waves, c.name)
    print("vote family (%s): %d frames x 4 instantiations of outlier_vote_kernel, every counter compared" % (vote, len(cases)))


@pytest.mark.parametrize("vote", ["reference", "fixed"])
def test_vote_counters_through_the_scale_kernels(gpu, votes, vote):
    K, cases = _K(), votes[vote]
    for waves in (1, 4, 8, 16):
        pf, res = sc.run_scale(gpu, cases, kind="exact", waves=waves, vote=vote)
        for f, c in enumerate(cases):
            assert res["status"][f] == _want_status(c), (waves, c.name, res["status"][f])
            if c.status is None:
                want = c.votes()
                assert np.array_equal(res["vote_counters"][pf.frame_slice(f)], want), (waves, c.name)
                assert res["counts"][f, K.CNT_VALID] == int((want >= 0).sum()), (waves, c.name)
                assert _same(res["raw_scale"][f], c.oracle().raw_scale), (waves, c.name)
    print("vote family (%s): %d frames x 4 instantiations of scale_frames_kernel (EXACT)" % (vote, len(cases)))


# ---------------------------------------------------------------------------------------------------------- compaction family
@pytest.mark.parametrize("k", range(N_PLAN))
def test_compaction_through_every_instantiation(gpu, k):
    from mvoscalerecovery_amd import _lib
    max_lds = int(_lib.load().mvosr_max_lds_features())
    n, waves, inst = sc.compaction_plan(max_lds)[k]
    cases = sc.compaction_cases(n, waves, inst and inst[1])
    for c in cases:
        assert np.array_equal(c.oracle().valid, c.info["keep"]), c.name
    tag = "n=%d %s" % (n, "dense two-sweep" if inst is None else "<%d,%d>" % inst)
    pf, res = sc.run_scale(gpu, cases, kind="full", waves=waves)
    for f, c in enumerate(cases):
        _check_full(c, res, pf, f, tag + " FULL")
    pf, res = sc.run_scale(gpu, cases, kind="exact", waves=waves)
    for f, c in enumerate(cases):
        _check_exact(c, res, pf, f, tag + " EXACT")
    pf, res = sc.run_scale(gpu, cases, kind="hot", waves=waves)
    for f, c in enumerate(cases):
        _check_hot(c, res, f, tag + " HOT")
    print("compaction family: %s, %d masks x FULL / EXACT / HOT, %d rows of tri2" % (tag, len(cases), sum(len(c.tri2) for c in cases)))


# ----------------------------------------------------------------------------------------------------------- selection family
@pytest.fixture(scope="module")
def selection():
    cases = sc.selection_cases()
    return cases, [sc.only_decided(c) for c in cases]


@pytest.mark.parametrize("waves", [1, 4, 8, 16])
def test_selection_through_the_lds_kernels(gpu, selection, waves):
    cases, decided = selection
    tag = "waves=%d" % waves
    pf, res = sc.run_scale(gpu, cases, kind="full", waves=waves)
    n_rows = sum(_check_full(c, res, pf, f, tag + " FULL") for f, c in enumerate(cases))
    pf, res = sc.run_scale(gpu, decided, kind="exact", waves=waves)
    for f, c in enumerate(decided):
        _check_exact(c, res, pf, f, tag + " EXACT")
    pf, res = sc.run_scale(gpu, decided, kind="hot", waves=waves)
    for f, c in enumerate(decided):
        _check_hot(c, res, f, tag + " HOT")
    for c, r in zip(decided, res["status"]):
        if c.info["family"] == "singular":
            assert r == so.ST_ERR_SINGULAR
    print("selection family: %s, %d frames x FULL / EXACT / HOT, %d decided rows of %d" % (tag, len(cases), n_rows, sum(len(c.tri2) for c in cases)))


def test_selection_through_the_dense_kernels(gpu, selection):
    """tri2 numbered over the features: the dense feature-numbered kernel (HOT + exact pass, EXACT, FULL) and the tiled kernel."""
    cases, decided = selection
    pf, res = sc.run_scale(gpu, cases, kind="full", layout="features")
    assert pf.tri2_ids == 1
    n_rows = 0
    for f, c in enumerate(cases):
        order = pf.tri2_order[int(pf.tri2_off[f]):int(pf.tri2_off[f + 1])]
        assert np.array_equal(order, np.arange(len(order)))          # (rows kept in place: per-row outputs line up with the oracle's)
        n_rows += _check_full(c, res, pf, f, "dense FULL")
    pf, res = sc.run_scale(gpu, decided, kind="exact", layout="features")
    for f, c in enumerate(decided):
        _check_exact(c, res, pf, f, "dense EXACT")
    pf, res = sc.run_scale(gpu, decided, kind="hot", layout="features")
    for f, c in enumerate(decided):
        _check_hot(c, res, f, "dense HOT")
    pf, res = sc.run_scale(gpu, decided, kind="hot", layout="tiled")
    for f, c in enumerate(decided):
        _check_hot(c, res, f, "tiled", tri_valid=False)
    print("selection family: dense feature-numbered FULL / EXACT / HOT and tiled, %d frames, %d decided rows" % (len(cases), n_rows))


@pytest.mark.parametrize("waves", [1, 4])
def test_flag_words_at_their_last_bit(gpu, waves):
    """64 B rows with flat rows at bits 0 and 63 of the first and the last thread: equal to the oracle through the instantiation
    whose limit it is and through the larger ones; one row more is refused by that instantiation."""
    K = _K()
    at_limit, over = sc.flag_bits_case(waves), sc.flag_bits_case(waves, extra_rows=1)
    assert len(at_limit.tri2) == 64 * 64 * waves and over.status == K.ST_ERR_MASK
    n_inst = 0
    for w, cases in ((waves, [at_limit, over, at_limit]), (8, [at_limit]), (16, [at_limit])):
        pf, res = sc.run_scale(gpu, cases, kind="full", waves=w)
        for f, c in enumerate(cases):
            _check_full(c, res, pf, f, "waves=%d FULL" % w)
        pf, res = sc.run_scale(gpu, cases, kind="exact", waves=w)
        for f, c in enumerate(cases):
            _check_exact(c, res, pf, f, "waves=%d EXACT" % w)
        pf, res = sc.run_scale(gpu, cases, kind="hot", waves=w)
        for f, c in enumerate(cases):
            _check_hot(c, res, f, "waves=%d HOT" % w)
        n_inst += 1
    for kind in ("exact", "hot"):                                   # (128 flag bits per thread: no limit near these sizes)
        pf, res = sc.run_scale(gpu, [at_limit], kind=kind, layout="features")
        (_check_exact(at_limit, res, pf, 0, "dense") if kind == "exact" else _check_hot(at_limit, res, 0, "dense"))
    print("flag_bits (waves=%d): %d rows, %d LDS instantiations x FULL / EXACT / HOT + dense; +1 row refused" % (waves, len(at_limit.tri2), n_inst))


# ---------------------------------------------------------------------------------------------------------------- redo family
def test_which_frames_the_hot_kernel_hands_to_the_exact_pass(gpu):
    from mvoscalerecovery_amd import _lib
    pairs = sc.redo_cases()
    cases, expect = [c for c, _ in pairs], np.array([e for _, e in pairs])
    assert (~expect).sum() >= 49 and expect.sum() == 4
    for waves in (0, 4, 8, 16):
        pf, res = sc.run_scale(gpu, cases, kind="hot", waves=waves, hot_only=True)
        redo = res["status"] == _lib.ST_REDO
        assert np.array_equal(redo, expect), (waves, [c.name for c, g, w in zip(cases, redo, expect) if g != w])
        for f, c in enumerate(cases):
            if not expect[f]:
                _check_hot(c, res, f, "hot_only waves=%d" % waves)
        pf, res = sc.run_scale(gpu, cases, kind="hot", waves=waves)          # the same batch with its exact pass: the oracle, frame by frame
        for f, c in enumerate(cases):
            _check_hot(c, res, f, "waves=%d" % waves)
    print("redo family: %d ordinary frames not handed over, 4 reason frames handed over, 1 all-outside threshold frame not; x 4 wave settings"
          % int((~expect).sum() - 1))
