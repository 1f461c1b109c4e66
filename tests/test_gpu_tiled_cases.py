"""scale_frames_tiled_kernel on the crafted multi-tile frames of tests/tiled_cases.py: the three-tile ring and its wrapped slots,
far rows and the two pending lists at their caps, the 64-bit height key and the guard band at the level, the per-wavefront candidate
lists up to 65 chunks, tri2 checked against the vote, a vote counter at the end of its range across two tiles, and a mixed batch.
Every frame goes through run_scale(kind="hot", layout="tiled"); with hot_only exactly the frames a case was built to hand over come
back MVOSR_ST_REDO, and those frames also go through the two-sweep kernel on the tile layout (kind="exact").  Every comparison with
the oracle is equality; the only constant is the kernel's own kLevelGuard, which the band cases sit a factor 10 and 100 to either
side of."""
import numpy as np
import pytest

import scale_cases as sc
import tiled_cases as tc
from oracle import scale_oracle as so
from test_gpu_scale_cases import _K, _check_exact, _check_hot, _same

pytestmark = pytest.mark.gpu

PER_FRAME = ("status", "raw_scale", "height", "height_level", "counts")


def _redo():
    from mvoscalerecovery_amd import _lib
    return _lib.ST_REDO


def _identical(a, b, frames, tag):
    for k in PER_FRAME:
        assert np.array_equal(a[k][frames], b[k][frames], equal_nan=True), (tag, k)


def _run_family(gpu, cases, tag, vote="reference", far_tables=(True, False), hist=False, mutate=None, refused=()):
    """hot_only: exactly the recorded frames are handed over, every other frame equals the oracle (the tiled kernel's own result: a
    full call also redoes the frames of the batch's exact mask); with the exact pass every frame does; the same with and without
    the packer's far table, bit for bit; the handed-over frames through the two-sweep kernel on
    the tile layout.  `refused`: frames that `mutate` made wrong (MVOSR_ST_ERR_MASK, checked by the caller).  Returns the results
    of the run with the exact pass."""
    want = np.array([c.info.get("redo") is not None for c in cases])
    live = np.array([f not in refused for f in range(len(cases))])
    runs = []
    for far_table in far_tables:
        t = "%s far_table=%s" % (tag, far_table)
        pf, only = sc.run_scale(gpu, cases, kind="hot", layout="tiled", vote=vote, hot_only=True, far_table=far_table, hist=hist, mutate=mutate)
        handed = only["status"] == _redo()
        assert np.array_equal(handed[live], want[live]), (t, [(c.name, bool(g)) for c, g, w in zip(cases, handed, want) if g != w])
        pf, res = sc.run_scale(gpu, cases, kind="hot", layout="tiled", vote=vote, far_table=far_table, hist=hist, mutate=mutate)
        for f, c in enumerate(cases):
            if live[f]:
                if not want[f]:
                    _check_hot(c, only, f, t + " hot_only", tri_valid=False)
                _check_hot(c, res, f, t, tri_valid=False)
        runs.append((only, res))
    if len(runs) == 2:
        _identical(runs[0][1], runs[1][1], np.ones(len(cases), bool), tag + ": with against without the far table")
        _identical(runs[0][0], runs[1][0], live & ~want, tag + ": hot_only, with against without the far table")
    over = [c for f, c in enumerate(cases) if want[f] and live[f]]
    if over:
        pf, ex = sc.run_scale(gpu, over, kind="exact", layout="tiled", vote=vote)
        for f, c in enumerate(over):
            _check_exact(c, ex, pf, f, tag + " two-sweep EXACT")
    return runs[0][1]


# ------------------------------------------------------------------------------------------------------------- 1. walk and ring
def test_walk_and_ring(gpu):
    cases = tc.walk_cases()
    assert [c.n for c in cases] == list(tc.WALK_SIZES)
    _run_family(gpu, cases, "walk")
    _run_family(gpu, tc.walk_cases_fixed(), "walk (fixed vote)", vote="fixed")
    print("walk family: n = %s, %d extreme rows and %d one further (far) per triangulation, far rows of tri1 in all: %d"
          % (list(tc.WALK_SIZES), sum(len(c.info["extreme"]) for c in cases), sum(len(c.info["one_further"]) for c in cases), sum(c.info["far1"] for c in cases)))


# --------------------------------------------------------------------------------------- 2. far rows and the pending lists
def test_far_rows_and_the_pending_lists(gpu):
    far, caps = tc.far_cases(), tc.cap_cases()
    ref = [c for c in far if c.vote == "reference"]
    batch = ref[:2] + caps[:2] + ref[2:] + caps[2:]                      # (the frames over the cap have neighbours on both sides)
    res = _run_family(gpu, batch, "far")
    by = {c.name: f for f, c in enumerate(batch)}
    assert res["status"][by["far_singular"]] == so.ST_ERR_SINGULAR
    assert [c.info["redo"] for c in caps] == [None, "overflow", None, "overflow"]          # (what _run_family held the hot_only run against)
    fixed = [c for c in far if c.vote == "fixed"]
    _run_family(gpu, fixed, "far (fixed vote)", vote="fixed")
    print("far family: %d + %d frames; cap frames 341 / 342 far rows of tri1 and 192 / 193 of tri2: handed over 342 and 193 only" % (len(batch), len(fixed)))


# -------------------------------------------------------------------------------------------------------- 3. keys and the band
def test_keys_and_the_band(gpu):
    K, cases = _K(), tc.keys_cases()
    res = _run_family(gpu, cases, "keys")
    by = {c.name: f for f, c in enumerate(cases)}
    assert res["counts"][by["keys/negative"], K.CNT_SELECTED] == 3 and res["status"][by["keys/negative"]] == so.ST_MEDIAN
    assert res["status"][by["keys/nothing_selected"]] == so.ST_NO_FLAT and res["status"][by["keys/no_steep"]] == so.ST_NO_FLAT
    assert res["status"][by["keys/lone_bins"]] == so.ST_LEVEL and _same(res["raw_scale"][by["keys/lone_bins"]], sc.ABS_REF / sc.LEVEL)
    for rel in tc.BAND_OUTSIDE:                                           # not handed over, and the decision is right
        f = by["keys/band/%+g" % rel]
        assert res["counts"][f, K.CNT_SELECTED] == (6 if rel > 0 else 3), rel
    print("keys family: %d frames, handed over: %s" % (len(cases), [c.name for c in cases if c.info["redo"]]))


# ----------------------------------------------------------------------------------------------------------- 4. candidate lists
def _check_lists(cases, res, tag):
    K = _K()
    for f, c in enumerate(cases):
        r = c.oracle()
        assert np.array_equal(res["hist"][f, 0], r.road.hist_raw), (tag, c.name, np.nonzero(res["hist"][f, 0] != r.road.hist_raw)[0][:8])
        assert res["counts"][f, K.CNT_SELECTED] == len(r.sel.selected_ids) and res["counts"][f, K.CNT_KEPT] == r.road.n_kept, (tag, c.name)
        assert res["counts"][f, K.CNT_MODES] == r.road.n_modes, (tag, c.name)
        assert _same(res["height"][f], r.height) and _same(res["raw_scale"][f], r.raw_scale), (tag, c.name)


@pytest.mark.parametrize("which", ["small", "large"])
def test_candidate_lists(gpu, which):
    cases = tc.list_cases_small() if which == "small" else tc.list_cases_large()
    for hot_only in (True, False):
        pf, res = sc.run_scale(gpu, cases, kind="hot", layout="tiled", hot_only=hot_only, hist=True)
        assert not (res["status"] == _redo()).any()
        for f, c in enumerate(cases):
            _check_hot(c, res, f, "lists hot_only=%s" % hot_only, tri_valid=False)
        _check_lists(cases, res, "lists hot_only=%s" % hot_only)
    print("candidate lists (%s): n = %s; longest list per frame %s entries" % (which, sorted({c.n for c in cases}), sorted({max(c.info["wave_cands"]) for c in cases})))


# ------------------------------------------------------------------------------------------------------ 5. tri2 against the vote
def _name_a_dropped_feature(c, far):
    """mutate(pf) for frame 1 of a batch: one vertex of a stored tri2 row (near: the row of the smallest vertices; far: the first far
    row) becomes a feature the vote dropped, in a place that leaves the row where the tile index has it."""
    keep = c.info["keep"]

    def mutate(pf):
        a = int(pf.tri2_off[1])
        offs = pf.tile2_off[int(pf.tile_base[1]):int(pf.tile_base[2])]
        r = a + (int(offs[-1]) if far else 0)
        row = pf.tri2[r].copy()
        lo, hi = int(row.min()), int(row.max())
        dropped = np.nonzero(~keep)[0]
        if far:                                                          # the middle vertex: anywhere between the other two
            at, cand = int(np.argsort(row)[1]), dropped[(dropped > lo) & (dropped < hi)]
        else:                                                            # the largest vertex: further along the tile of the smallest
            at, cand = int(np.argmax(row)), dropped[(dropped > lo) & (dropped < (lo // tc.W + 1) * tc.W)]
        assert len(cand) and tc.is_far([row])[0] == far
        pf.tri2[r, at] = cand[-1]
        assert tc.is_far([pf.tri2[r]])[0] == far and pf.tri2[r].min() == lo
    return mutate


@pytest.mark.parametrize("far", [False, True])
def test_tri2_against_the_vote(gpu, far):
    c = tc.walk_case(1537)
    assert c.info["far2"] == 2 and not c.info["keep"].all()
    cases = [c, c, c]
    res = _run_family(gpu, cases, "used flag", mutate=_name_a_dropped_feature(c, far), refused=(1,))
    assert res["status"].tolist() == [c.oracle().status, so.ST_ERR_MASK, c.oracle().status]


# ------------------------------------------------------------------------------------------------- 6. vote range across tiles
def test_vote_range_across_tiles(gpu):
    K = _K()
    for vote in ("reference", "fixed"):
        cases = [c for c in tc.fan_strip_cases() if c.vote == vote]
        assert len(cases) == 2
        res = _run_family(gpu, cases, "fan strip " + vote, vote=vote)
        for f, c in enumerate(cases):
            cnt = c.votes()
            assert res["counts"][f, K.CNT_VALID] == int((cnt >= 0).sum()) and (cnt[c.info["centre"]] >= 0) == (c.info["centre_count"] > 0), c.name


# ---------------------------------------------------------------------------------------------------------------- 7. mixed batch
def test_mixed_batch(gpu):
    walk = tc.walk_case(1537)
    cases = [tc.tiny_case(0), tc.walk_case(3073), tc.tiny_case(3), tc.cap_votes_case(342), tc.tiny_case(4), walk, tc.walk_case(300),
             sc.control_cases(count=1)[0]]
    assert all(tc.order_free(c) for c in cases)
    mutate1 = _name_a_dropped_feature(walk, far=False)

    def shifted(k):
        def mutate(pf):
            # (_name_a_dropped_feature works on frame 1: present frame k as frame 1)
            view = type("V", (), {})()
            view.tri2, view.tri2_off = pf.tri2, np.array([0, pf.tri2_off[k], pf.tri2_off[k + 1]])
            view.tile2_off, view.tile_base = pf.tile2_off, np.array([0, pf.tile_base[k], pf.tile_base[k + 1]])
            mutate1(view)
        return mutate
    runs = [sc.run_scale(gpu, cases, kind="hot", layout="tiled", mutate=shifted(5))[1] for _ in range(2)]
    _identical(runs[0], runs[1], np.ones(len(cases), bool), "mixed batch, twice")
    res = runs[0]
    assert res["status"].tolist() == [so.ST_ERR_EMPTY, cases[1].oracle().status, so.ST_TOO_FEW, cases[3].oracle().status,
                                      so.ST_NO_FLAT, so.ST_ERR_MASK, cases[6].oracle().status, cases[7].oracle().status]
    for f, c in enumerate(cases):
        one = sc.run_scale(gpu, [c], kind="hot", layout="tiled", mutate=shifted(0) if f == 5 else None)[1]
        for k in PER_FRAME:
            assert np.array_equal(res[k][f], one[k][0], equal_nan=True), (c.name, k, res[k][f], one[k][0])
        if f in (1, 3, 4, 6, 7):
            _check_hot(c, res, f, "mixed batch", tri_valid=False)
    print("mixed batch: frames of %s features; statuses %s" % ([c.n for c in cases], res["status"].tolist()))
