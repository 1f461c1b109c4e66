"""CPU side of tests/scale_rowflags_cases.py: every crafted frame is what its docstring says, the CPU twin of the lean
bookkeeping reproduces the oracle on every frame, and each mutant of it differs from the oracle on at least one frame — the
frames tests/test_gpu_scale_rowflags.py runs through the kernels can see those mistakes."""
import numpy as np
import pytest

import scale_cases as sc
import scale_rowflags_cases as rf
from oracle import scale_oracle as so

BITS_PLAN = [(64, 1, 0), (64, 1, 1), (256, 1, 0), (256, 1, 1), (512, 1, 0), (512, 1, 1), (1024, 2, 0)]
LEAN_PLAN = [p for p in BITS_PLAN if p[1] == 1]          # (the lean form has one 64-bit word per thread: no twin of 128 rows)


@pytest.fixture(scope="module")
def bits():
    return [rf.rowflag_bits_case(b, fw, short) for b, fw, short in BITS_PLAN]


@pytest.fixture(scope="module")
def others():
    out = [rf.steep_count_case(k) for k in ("none", "one", "all", "nan")]
    out += [rf.rare_row_case(what, where, 256) for what in ("singular", "band") for where in rf.RARE_POSITIONS]
    return out


def _agrees(c, block, mutant=None):
    """Does lean_book (with `mutant`) give what the oracle gives for frame c: the flat rows, the two counts and the flags?"""
    flat, steep, _, singular = rf.oracle_rows(c)
    b = rf.book_of(c, block, mutant)
    if singular:                                                  # (the oracle raises: only the flag is compared)
        return b["singular"]
    fast_flat, fast_steep = sc.fast_pitch_test(c)
    want_undecided = not (fast_flat | fast_steep).all()          # (a row in the band, or one with a NaN)
    return (np.array_equal(b["seen"], flat) and b["n_pitch"] == int(flat.sum()) and b["n_steep"] == int(steep.sum())
            and not b["singular"] and b["undecided"] == want_undecided)


def test_flag_frames_are_what_they_say(bits):
    for c, (block, fw, short) in zip(bits, BITS_PLAN):
        s = c.oracle().sel
        assert 64 <= c.n <= 128 and len(c.tri2) == 64 * fw * block - short and c.oracle().valid.all(), c.name
        assert np.array_equal(s.valid_pitch, c.info["flat"]) and c.oracle().status != so.ST_ERR_SINGULAR, c.name
        words = rf.lane_words(block, fw, 41)
        cols = [k for k in rf.SPECIAL_BITS if k < 64 * fw]
        for k in cols:                                            # every special bit is set in some lanes and clear in others
            assert 0 < words[:, k].sum() < block, (c.name, k)
        assert all(not np.array_equal(words[:, a], words[:, b]) for a in cols for b in cols if a < b), c.name
        # every marker row is flat, above the level, and the only row that holds its triangle
        for j, (kk, l) in enumerate(rf.marker_rows(block, fw)):
            t = kk * block + l
            assert s.tri_valid[t] and (c.tri2 == 3 * j).any(1).sum() == 1, (c.name, kk, l)
        assert s.valid_pitch[-1] and 0 < s.tri_valid.sum() < s.valid_pitch.sum(), c.name
        assert len(s.selected_ids) == 3 * (c.info["n_markers"] + rf.N_ABOVE), c.name


def test_the_twin_reproduces_the_oracle(bits, others):
    for c, (block, fw, _) in zip(bits, BITS_PLAN):
        if fw == 1:
            assert _agrees(c, block), c.name
    for c in others:
        for block in (64, 256, 512):
            assert _agrees(c, block), (c.name, block)


def test_every_mutant_is_seen(bits, others):
    seen = dict.fromkeys(rf.MUTANTS, 0)
    for m in rf.MUTANTS[:4]:
        for c, (block, fw, _) in zip(bits, BITS_PLAN):
            if fw == 1:
                seen[m] += not _agrees(c, block, m)
        for c in others:
            seen[m] += not _agrees(c, 256, m)
    assert seen["half0_only"] >= len(LEAN_PLAN) and seen["npitch_low_half"] >= len(LEAN_PLAN), seen
    assert seen["inband_is_steep"] >= 4 and seen["rare_last_row"] >= 2, seen
    # which frames see what: the flat in-band rows and the NaN rows see the steep count's mutant; the rare row in front of its thread's other rows sees
    # the flags' (a row that is its thread's last or only one cannot)
    nan = next(c for c in others if c.name == "steep_count/nan")
    assert not _agrees(nan, 256, "inband_is_steep")
    assert all(not _agrees(rf.rare_row_case("band", where, 256), 256, "inband_is_steep") for where in rf.RARE_POSITIONS)
    for what in ("singular", "band"):
        got = {where: _agrees(rf.rare_row_case(what, where, 256), 256, "rare_last_row") for where in rf.RARE_POSITIONS}
        assert got == {"first": False, "last": True, "only": True}, (what, got)
    # 0/1-multiply masking: seen by the twin on a row that is not steep and whose height is inf (no frame can carry one through
    # the oracle: test_the_overflow_frame_is_not_decidable)
    flat, steep, h = np.array([False, True, False]), np.array([True, False, True]), np.array([1.5, np.inf, 2.5])
    assert rf.lean_book(flat, steep, h, 64)["hsum"] == 4.0
    assert np.isnan(rf.lean_book(flat, steep, h, 64, mutant="mask_by_multiply")["hsum"])


def test_steep_count_frames(others):
    by = {c.info["kind"]: c for c in others if c.info.get("family") == "steep_count"}
    r = by["none"].oracle()
    assert np.isnan(r.height_level) and r.status == so.ST_NO_FLAT and r.sel.valid_pitch.all()
    r = by["one"].oracle()
    assert (r.sel.pitch_deg >= sc.THR_DEG).sum() == 1 and r.height_level == r.sel.heights[len(by["one"].tri2) // 2]
    r = by["all"].oracle()
    assert not r.sel.valid_pitch.any() and np.isfinite(r.height_level) and r.status == so.ST_NO_FLAT
    r = by["nan"].oracle()
    k = by["nan"].info["nan_at"]
    assert np.isnan(r.sel.pitch_deg[k]).all() and np.isfinite(np.delete(r.sel.pitch_deg, k)).all() and np.isfinite(r.height_level)
    bad, good = rf.refused_among_steep_case()
    at = bad.info["bad_at"]
    assert bad.status == so.ST_ERR_MASK and bad.tri2[at].max() == bad.n and np.array_equal(np.delete(bad.tri2, at, 0), good.tri2)
    steep = good.oracle().sel.pitch_deg >= sc.THR_DEG
    assert steep[at - 2:at + 2].all() and np.isfinite(good.oracle().height_level)


def test_rare_frames(others):
    for c in (c for c in others if c.info.get("family") == "rare"):
        T, B = len(c.tri2), c.info["block"]
        flat, steep = sc.fast_pitch_test(c)
        left = np.nonzero(~(flat | steep))[0]
        if "singular_at" in c.info:
            assert c.oracle().status == so.ST_ERR_SINGULAR and left.tolist() == c.info["singular_at"], c.name
        else:
            at = c.info["band_at"]
            dec, is_flat = sc.decided_rows(c)
            assert left.tolist() == [at] and dec.all() and is_flat[at] and c.oracle().sel.valid_pitch[at], c.name
            assert abs(float(sc.band_ratio(c)[at])) < sc.BAND and c.oracle().status != so.ST_ERR_SINGULAR, c.name
        where = c.name.split("/")[2]
        at = left[0]
        mine = np.arange(at % B, T, B)                               # the rows of the thread that has the rare one
        assert {"first": at == mine[0] and len(mine) == 3, "last": at == T - 1 == mine[-1] and len(mine) == 3,
                "only": mine.tolist() == [at] and at == B - 1}[where], c.name


def test_the_overflow_frame_is_not_decidable():
    """Dropped from the GPU cases: a flat triangle whose 3 h overflows has a plane normal of 1.7e-308, which the oracle's LU
    cannot resolve — NumPy calls the row steep, and the oracle's own level is inf."""
    c = rf.overflow_case()
    s = c.oracle().sel
    assert np.isinf(s.heights[-1]) and sc.fast_pitch_test(c)[0][-1]
    assert not s.valid_pitch[-1] and not np.isfinite(s.height_level)

