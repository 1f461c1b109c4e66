"""The crafted frames of tests/test_gpu_scale_cases.py checked without a GPU: every case has the property its name claims (on the
oracle and on the np.longdouble truth), every CPU stand-in of a subtly wrong kernel differs from the oracle on at least one case,
the rows left out of the pitch comparison stay within their caps, and the constant of the decidability rule is what NumPy itself
needs against the truth."""
import numpy as np
import pytest

import scale_cases as sc
from oracle import scale_oracle as so

NOMINAL_MAX_LDS = 6208             # (160 KB of LDS: what mvosr_max_lds_features() gives on an MI355X)


@pytest.fixture(scope="module")
def votes():
    return sc.vote_cases()


@pytest.fixture(scope="module")
def selection():
    return sc.selection_cases() + [sc.flag_bits_case(1), sc.flag_bits_case(4)]


@pytest.fixture(scope="module")
def compaction():
    return [(n, inst, sc.compaction_cases(n, waves, inst and inst[1])) for n, waves, inst in sc.compaction_plan(NOMINAL_MAX_LDS)]


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18


# ---------------------------------------------------------------------------------------------------------------- vote family
def test_fans_drive_one_counter_to_the_ends_of_its_range(votes):
    fans = [c for c in votes if "centre" in c.info and len(c.tri1) == sc.MAX_VOTE_ROWS]
    assert len(fans) == 12 and {(c.info["centre"] & 1, c.info["centre_count"] > 0, c.vote) for c in fans} == \
        {(p, s, v) for p in (0, 1) for s in (False, True) for v in ("reference", "fixed")}
    for c in fans:
        cnt = c.votes()
        assert (c.tri1 == c.info["centre"]).any(axis=1).all(), c.name                      # every row holds the centre
        assert cnt[c.info["centre"]] == c.info["centre_count"] and c.info["centre_count"] in (32766, -32764), c.name
        assert abs(cnt[c.info["partner"]]) <= 4 and c.info["partner"] == c.info["centre"] ^ 1, c.name        # the word's other half
        assert cnt[-sc.N_SPARE:].tolist() == [1] * sc.N_SPARE, c.name                      # unreferenced
        assert int((cnt >= 0).sum()) >= 4 and c.tri2.max() < int((cnt >= 0).sum())
    pairs = [c for c in votes if "up" in c.info]
    assert len(pairs) == 6
    for c in pairs:                   # both halves of word 0, hard, in opposite directions
        cnt = c.votes()
        assert {c.info["up"], c.info["down"]} == {0, 1}
        assert cnt[c.info["up"]] == 32766 and cnt[c.info["down"]] == -32764, c.name


def test_the_packed_counters_hold_every_vote_case_and_the_mutants_do_not(votes):
    """The no-borrow claim, on the CPU model of the packed counters: biased halves give the oracle's counts on every case with at
    most 32 765 rows; unbiased halves, or a read-back against 0x7FFF, do not."""
    seen = {"unbiased": 0, "bias_7fff": 0}
    for c in votes:
        cnt = c.votes()
        if len(c.tri1) <= sc.MAX_VOTE_ROWS:
            assert np.array_equal(sc.packed_votes(c.f2[:, 1], c.f3[:, 2], c.tri1, c.vote), cnt), c.name
            seen["unbiased"] += not np.array_equal(sc.mutant_votes_unbiased(c), cnt)
            seen["bias_7fff"] += not np.array_equal(sc.mutant_votes_bias_7fff(c), cnt)
        else:                          # one row more: the centre's half would reach 0xFFFF — the frame the kernels refuse
            assert c.status == so.ST_ERR_MASK and cnt[c.info["centre"]] == 32767
    assert seen["unbiased"] > 0 and seen["bias_7fff"] > 0, seen
    # the borrow itself: vertex 0 (low half) at -32 764 takes one from vertex 1's half
    c = next(c for c in votes if c.name.startswith("opposite/up1/reference"))
    assert sc.mutant_votes_unbiased(c)[1] == c.votes()[1] - 1


def test_edge_counts(votes):
    cases = [c for c in votes if c.name.startswith("edge_counts")]
    assert [c.vote for c in cases] == ["reference", "fixed"]
    for c in cases:
        cnt = c.votes()
        assert np.array_equal(cnt, c.info["want"]), c.name
        assert cnt[0] == 0 and cnt[3] == -1 and np.array_equal(so.votes_valid(cnt), c.info["want"] >= 0)
        v, z = c.f2[:, 1], c.f3[:, 2]
        with np.errstate(invalid="ignore"):
            prod = [(v[a] - v[b]) * (z[a] - z[b]) for a, b in ((8, 9), (9, 10), (13, 12), (12, 11), (14, 15))]
        assert prod[0] == 0 and np.signbit(prod[0]) and prod[2] == 0 and not np.signbit(prod[2]) and np.isnan(prod[4])     # -0.0, +0.0, NaN
        assert np.isfinite(c.f3[np.nonzero(cnt >= 0)[0][c.tri2]]).all()


# ---------------------------------------------------------------------------------------------------------- compaction family
def test_compaction_frames_vote_exactly_their_masks(compaction):
    n_frames, instantiations = 0, set()
    for n, inst, cases in compaction:
        instantiations.add(inst)
        for c in cases:
            keep = c.info["keep"]
            assert c.n == n and np.array_equal(c.oracle().valid, keep), c.name
            assert np.array_equal(so.outlier_votes(c.f2[:, 1], c.f3[:, 2], c.tri1, "fixed") >= 0, keep), c.name
            nv = int(keep.sum())
            y = c.f3[keep, 1]
            assert len(np.unique(y)) == nv and (nv < 3 or len(np.unique(c.tri2)) == nv), c.name        # distinct y', everyone in a row
            assert len(c.tri1) <= sc.MAX_VOTE_ROWS
            dec, flat = sc.decided_rows(c)
            if c.oracle().status != so.ST_ERR_SINGULAR:
                assert dec.all() and np.array_equal(c.oracle().sel.valid_pitch, flat), c.name          # no row within rounding of -80 deg
            n_frames += 1
    assert instantiations == set(sc.INSTANTIATIONS) | {None}
    assert n_frames >= 17 * 6


def test_compaction_masks_are_what_their_names_say(compaction):
    for n, inst, cases in compaction:
        m = {c.name.split("/")[-1]: c.info["keep"] for c in cases}
        assert m["all"].all() and m["only0"].sum() == 1 and m["only0"][0]
        assert np.nonzero(m["last+3front"])[0].tolist() == [0, 1, 2, n - 1]
        assert np.array_equal(np.nonzero(m["every2nd"])[0], np.arange(0, n, 2)) and np.array_equal(np.nonzero(m["every64th"])[0], np.arange(0, n, 64))
        assert np.nonzero(m["last_subchunk"])[0][0] % 64 == 0 and m["last_subchunk"][-1] and 1 <= m["last_subchunk"].sum() <= 64
        if inst is None or inst[0] == 1:
            continue
        per = inst[1] * sc.WAVE
        slices = [m[k] for k in ("slice_first_dropped", "slice_middle_dropped", "slice_last_dropped")]
        assert not slices[0][:per].any() and slices[0][per:].all()
        assert not slices[2][per * ((n - 1) // per):].any() and slices[2][:per * ((n - 1) // per)].all()
        for s in slices:
            w = np.nonzero(~s)[0][0] // per
            assert np.array_equal(np.nonzero(~s)[0], np.arange(w * per, min(n, (w + 1) * per)))


def test_compaction_layout_and_its_mutant(compaction):
    """The stable compaction puts survivor j at slot j; bases that skip an empty wave slice do not, and the heights show it."""
    differs = 0
    for n, inst, cases in compaction:
        if inst is None:
            continue
        for c in cases:
            keep = c.info["keep"]
            good = sc.compacted_layout(keep, *inst)
            assert np.array_equal(good, np.nonzero(keep)[0]), c.name
            bad = sc.compacted_layout(keep, *inst, skip_empty=True)
            if not np.array_equal(bad, good):
                assert "slice" in c.name
                assert not np.array_equal(sc.layout_heights(c, bad), c.oracle().sel.heights, equal_nan=True), c.name
                differs += 1
    assert differs >= 6


# ----------------------------------------------------------------------------------------------------------- selection family
def test_threshold_rows_sit_where_their_delta_says(selection):
    th = [c for c in selection if c.info.get("family") == "threshold"]
    assert [c.info["delta"] for c in th] == list(sc.THRESHOLD_OUTSIDE + sc.THRESHOLD_INSIDE)
    for c in th:
        p = np.asarray(sc.pitch_true(c) - sc.THR_DEG, dtype=np.float64)
        side = c.info["side"]
        assert (side == 1).sum() >= 40 and (side == -1).sum() >= 40
        assert np.array_equal(p < 0, side == 1), c.name
        assert np.all(np.abs(np.abs(p) / c.info["delta"] - 1) < 1e-3), c.name                 # the true pitch is -80 -+ delta
        r = np.abs(np.asarray(sc.band_ratio(c), dtype=np.float64))
        assert (r.max() <= 2.5e-10) if c.info["inside"] else (r.min() >= 4e-9), (c.name, r.min(), r.max())
        flat, steep = sc.fast_pitch_test(c)                                                   # ... and the fast test sees it that way
        if c.info["inside"]:
            assert not flat.any() and not steep.any()
        else:
            assert np.array_equal(flat, side == 1) and np.array_equal(steep, side == -1)
        h = c.oracle().sel.heights
        assert 0.5 < h.min() and h.max() < 2.0


def test_near_origin_rows_leave_the_fast_test(selection):
    c = next(c for c in selection if c.name == "near_origin")
    flat, steep = sc.fast_pitch_test(c)
    assert not flat.any() and not steep.any()                        # |det| <= 1e-9 mag on every row
    p = np.asarray(sc.pitch_true(c), dtype=np.float64)
    assert np.all(np.abs(np.where(c.info["side"] == 1, p + 89.0, p + 70.0)) < 1e-6)
    assert np.array_equal(c.oracle().sel.valid_pitch, c.info["side"] == 1)


def test_singular_rows_raise_in_numpy(selection):
    for m in sc.SINGULAR_MATRICES:
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.inv(np.array(m, dtype=np.float64))
    cases = [c for c in selection if c.info.get("family") == "singular"]
    assert len(cases) == 3 and all(c.oracle().status == so.ST_ERR_SINGULAR and c.oracle().valid.all() for c in cases)


def test_level_equal_sits_on_the_level(selection):
    c = next(c for c in selection if c.name == "level_equal")
    s = c.oracle().sel
    assert s.height_level == sc.LEVEL and np.all(s.heights[:4] == sc.LEVEL) and not s.valid_pitch[:4].any()
    assert s.valid_pitch[4:].all() and s.heights[4] == sc.LEVEL and s.heights[5] == np.nextafter(sc.LEVEL, 2.0)
    assert s.tri_valid[4:].tolist() == c.info["want_selected"] == [False, True]
    for order in ([0, 1, 2, 3], [3, 1, 0, 2]):                      # the mean is L in any summation order
        assert np.mean(s.heights[order]) == sc.LEVEL and sum(s.heights[order]) / 4 == sc.LEVEL
    assert not np.array_equal(sc.mutant_select_ge(c), s.tri_valid)   # `>=` at the level takes the row of height exactly L as well


def test_flag_bits_frames(selection):
    for waves in (1, 4):
        c = next(c for c in selection if c.name == "flag_bits/w%d" % waves)
        B = 64 * waves
        s = c.oracle().sel
        assert len(c.tri2) == 64 * B and c.n <= 300 and c.oracle().valid.all()
        assert np.nonzero(s.valid_pitch)[0].tolist() == [0, B - 1, 63 * B, 64 * B - 1] == c.info["flat_at"].tolist()
        assert s.tri_valid[c.info["flat_at"]].all() and len(s.selected_ids) == 12
        assert np.array_equal(sc.flag_words(s.valid_pitch, B), s.valid_pitch)
        assert not np.array_equal(sc.flag_words(s.valid_pitch, B, shift_mask=31), s.valid_pitch)       # bit 63 lands on row 31 B + tid
        more = sc.flag_bits_case(waves, extra_rows=1)
        assert len(more.tri2) == 64 * B + 1 and more.status == so.ST_ERR_MASK


def test_sel_words_and_nan_row(selection):
    c = next(c for c in selection if c.name == "sel_words")
    assert c.oracle().sel.selected_ids.tolist() == c.info["want_selected"] == [0, 31, 32, 63, 64, c.n - 1]
    c = next(c for c in selection if c.name == "nan_row")
    s, k = c.oracle().sel, c.info["nan_at"]
    assert np.isnan(s.pitch_deg[k]) and not s.valid_pitch[k] and not c.oracle().sel.singular
    assert np.isfinite(np.delete(s.pitch_deg, k)).all() and np.isfinite(s.height_level)
    dec, flat = sc.decided_rows(c)
    assert dec[k] and not flat[k]


def test_pitch_mutants_are_visible(selection):
    """A fast test without its band decides the rows inside the band itself (no hand-over to the reference's formulation); a band
    around 85 deg calls the flat rows between -80 and -85 deg steep."""
    inside = [c for c in selection if c.info.get("inside")]
    for c in inside:
        flat, steep = sc.mutant_pitch_no_band(c)
        assert (flat | steep).all()
    c = next(c for c in selection if c.name == "threshold/0.001")
    flat, steep = sc.mutant_pitch_band_at_85(c)
    assert not np.array_equal(flat, c.oracle().sel.valid_pitch) and steep.all()


def test_decidability_constant_and_caps(selection):
    """C_PITCH is at least four times NumPy's own worst pitch error (in units of 2^-52 cond_2(A) 180/pi) against the longdouble
    truth; NumPy agrees with the truth on every decided row; at most 10 % of the threshold rows and 2 % of any other family are
    left undecided, and every (band side, pitch side) class keeps at least 8 decided rows."""
    worst, left, total, classes = 0.0, {}, {}, {}
    for c in selection:
        fam = c.info["family"]
        if fam == "singular":
            continue
        units = sc.numpy_pitch_error_units(c)
        worst = max(worst, float(np.nanmax(units)))
        dec, flat = sc.decided_rows(c)
        assert np.array_equal(c.oracle().sel.valid_pitch[dec], flat[dec]), c.name
        left[fam] = left.get(fam, 0) + int((~dec).sum())
        total[fam] = total.get(fam, 0) + len(dec)
        if fam == "threshold":
            for sgn in (1, -1):
                key = (c.info["inside"], sgn)
                classes[key] = classes.get(key, 0) + int((dec & (c.info["side"] == sgn)).sum())
            assert len(sc.only_decided(c).tri2) == int(dec.sum())
    print("C_PITCH: measured %.3f (recorded %.2f), constant %.2f; undecided rows %s of %s" % (worst, sc.C_PITCH_MEASURED, sc.C_PITCH, left, total))
    assert worst <= sc.C_PITCH_MEASURED and sc.C_PITCH >= 4 * worst
    assert left["threshold"] <= 0.10 * total["threshold"]
    assert all(left[f] <= 0.02 * total[f] for f in total if f != "threshold"), (left, total)
    assert len(classes) == 4 and min(classes.values()) >= 8, classes


# ---------------------------------------------------------------------------------------------------------------- redo family
def test_redo_family():
    controls = sc.control_cases()
    assert len(controls) == 64 and all(300 <= c.info["n_synth"] <= 700 for c in controls)
    cases = sc.redo_cases()
    kept = [c for c, redo in cases if c.info.get("family") == "control"]
    assert len(kept) >= 48 and all(sc.control_ok(c) for c in kept)
    for c in kept:
        sel, status, gap, pitch = sc.control_margins(c)
        assert sel and status != so.ST_LEVEL and gap >= 1e-9 and pitch >= 1e-5, c.name
    reasons = {c.name: (c, redo) for c, redo in cases if c.info.get("family") != "control"}
    c, redo = reasons["threshold/1e-08"] if "threshold/1e-08" in reasons else reasons["threshold/1e-08/decided"]
    flat, steep = sc.fast_pitch_test(c)
    assert redo and not (flat | steep).any()                                      # rows inside the pitch band
    c, redo = reasons["level_equal"]
    s = c.oracle().sel
    assert redo and np.min(np.abs(s.heights[s.valid_pitch] - s.height_level)) == 0.0       # a flat height within the level guard
    c, redo = reasons["nothing_selected"]
    s = c.oracle().sel
    assert redo and c.oracle().status == so.ST_NO_FLAT and s.valid_pitch.any() and np.all(s.heights[s.valid_pitch] < s.height_level - 0.3)
    c, redo = reasons["lone_bins"]
    r = c.oracle()
    assert redo and r.status == so.ST_LEVEL and r.road.n_kept == 0 and r.road.hist_raw.max() == 1 and r.raw_scale == sc.ABS_REF / sc.LEVEL
    c, redo = reasons["threshold/1e-05"]                                          # every row outside the band, wide margins otherwise
    flat, steep = sc.fast_pitch_test(c)
    sel, status, gap, pitch = sc.control_margins(c)
    assert not redo and (flat | steep).all() and sel and status != so.ST_LEVEL and gap >= 1e-9 and pitch >= 5e-6
