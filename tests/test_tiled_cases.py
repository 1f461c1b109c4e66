"""The crafted frames of tests/test_gpu_tiled_cases.py checked without a GPU: the packer puts every feature at the tile position the
case was built for and marks exactly the recorded rows as far; the per-wavefront candidate counts follow from the oracle's flat rows
and the retire rule; the oracle's status is the one the case was built for; the band and skew conditions hold; the NumPy model of
the tiled kernel's selection rule (tiled_cases.model) equals the oracle on every case and hands over exactly the recorded frames;
and every mutant of that model differs from the oracle on at least one case."""
import numpy as np
import pytest

import scale_cases as sc
import tiled_cases as tc
from oracle import scale_oracle as so


@pytest.fixture(scope="module")
def families():
    return {"walk": tc.walk_cases(), "walk_fixed": tc.walk_cases_fixed(), "far": tc.far_cases(), "cap": tc.cap_cases(), "keys": tc.keys_cases(),
            "lists": tc.list_cases_small() + tc.list_cases_large(), "fan": tc.fan_strip_cases()}


@pytest.fixture(scope="module")
def everything(families):
    return [c for cs in families.values() for c in cs]


@pytest.fixture(scope="module")
def models(everything):
    return {c.name: tc.model(c) for c in everything}


def _pack(cases):
    from mvoscalerecovery_amd import packing
    pf = packing.pack_features([c.f3 for c in cases], [c.f2 for c in cases], vanish=sc.VANISH)
    packing.attach_tri1(pf, [c.tri1 for c in cases])
    packing.apply_tile_order(pf)
    packing.attach_tri2(pf, [c.tri2 for c in cases], [np.asarray(c.oracle().valid) for c in cases], feature_ids=True)
    return pf


def _rowset(rows):
    return sorted(map(tuple, np.asarray(rows).tolist()))


def test_the_packer_sees_the_tiles_and_far_rows_the_cases_were_built_for(everything):
    from mvoscalerecovery_amd import packing
    n_far = [0, 0]
    for c in everything:
        pf = _pack([c])
        assert np.array_equal(pf.extra["perm"][0], np.arange(c.n)), c.name                    # feature i is tile position i
        ntiles = (c.n + tc.W - 1) // tc.W
        assert pf.tile_w == tc.W and len(pf.tile1_off) == ntiles + 1 == len(pf.tile2_off) and pf.tile_far_off[-1] == 9 * (c.info["far1"] + c.info["far2"])
        for which, rows, stored, offs in ((0, c.tri1.astype(np.int64), pf.tri1, pf.tile1_off), (1, tc.feature_rows(c), pf.tri2, pf.tile2_off)):
            far = tc.is_far(rows)
            n_near = len(rows) - int(far.sum())
            assert int(far.sum()) == c.info["far%d" % (which + 1)] and offs[-1] == n_near, (c.name, which)
            assert _rowset(stored[n_near:len(rows)]) == _rowset(rows[far]), (c.name, which)        # exactly the recorded rows, vertex order kept
            lo = np.sort(rows[~far].min(axis=1))
            assert np.array_equal(offs[:-1], np.searchsorted(lo, np.arange(ntiles) * tc.W)), (c.name, which)
            assert np.array_equal(stored[:n_near].min(axis=1), lo), (c.name, which)
            _, again = packing._tile_sort(rows.astype(np.int32), c.n)
            assert np.array_equal(again, offs), (c.name, which)
            n_far[which] += int(far.sum())
        tiles = set()
        for rows in (c.tri1.astype(np.int64), tc.feature_rows(c)):
            tiles |= set((rows[tc.is_far(rows)].reshape(-1) // tc.W).tolist())
        assert sorted(tiles) == c.info["far_tiles"], c.name
    print("far rows over all cases: %d of tri1, %d of tri2" % tuple(n_far))


def test_walk_cases(families):
    assert [c.n for c in families["walk"]] == list(tc.WALK_SIZES) and [c.vote for c in families["walk_fixed"]] == ["fixed"] * 3
    for c in families["walk"] + families["walk_fixed"]:
        keep, n = c.info["keep"], c.n
        assert np.array_equal(c.oracle().valid, keep) and np.array_equal(so.outlier_votes(c.f2[:, 1], c.f3[:, 2], c.tri1, "fixed") >= 0, keep), c.name
        for b in range(tc.W, n, tc.W):                                    # dropped on both sides of every boundary
            assert not keep[b - 3:b - 1].any() and keep[b - 1] and keep[b] and not keep[b + 1:b + 3].any(), (c.name, b)
        last = keep[(n - 1) // tc.W * tc.W:]
        assert len(last) < 12 or not last.all(), c.name
        rows = tc.feature_rows(c)
        have = set(_rowset(rows))
        for lo, mid, hi in c.info["extreme"]:                             # last feature of tile k .. last feature of tile k + 1: near, the slot wraps for k >= 1
            assert lo % tc.W == tc.W - 1 and hi == lo + tc.W and (lo, mid, hi) in have and not tc.is_far([[lo, mid, hi]])[0]
            assert any((np.sort(c.tri1, axis=1) == [lo, mid, hi]).all(axis=1))
        for lo, mid, hi in c.info["one_further"]:
            assert lo % tc.W == tc.W - 1 and hi == lo + tc.W + 1 and (lo, mid, hi) in have and tc.is_far([[lo, mid, hi]])[0]
        for key, further in (("extreme", 0), ("one_further", 1)):          # k = 0, a middle k and the last k that the frame allows
            ks = [lo // tc.W for lo, _, _ in c.info[key]]
            last = max(ks) if ks else -1
            assert (last + 3) * tc.W - 1 + further > n - 1 and ks == sorted({k for k in (0, last // 2, last) if 0 <= k <= last}), (c.name, key, ks)
        assert c.info["far2"] == len(c.info["one_further"]) and c.info["far1"] >= c.info["far2"]
        nv = int(keep.sum())
        assert len(np.unique(c.f3[keep, 1])) == nv and len(np.unique(c.tri2)) == nv                  # distinct y', every survivor in a row
        dec, flat = sc.decided_rows(c)                                    # (rows in the case's order; the fixed mode's oracle sorts them)
        vp = c.oracle().sel.valid_pitch
        assert dec.all() and (np.array_equal(vp, flat) if c.vote == "reference" else vp.sum() == flat.sum()), c.name
    assert max(k for c in families["walk"] for k in [max([0] + [lo // tc.W for lo, _, _ in c.info["extreme"]])]) >= 4


def test_far_and_cap_cases(families):
    by = {c.name: c for c in families["far"] + families["cap"]}
    for vote in ("reference", "fixed"):
        c = by["far_votes/" + vote]
        cnt = c.votes()
        near = so.outlier_votes(c.f2[:, 1], c.f3[:, 2], c.tri1[~tc.is_far(c.tri1)], vote)
        assert (near[[100, 101, 600]] == [0, 0, -2]).all() and (cnt[[100, 101, 600]] == [-1, -1, 0]).all()    # decided by the far rows alone
        assert c.info["far_tiles"] == [0, 1, 2, 4] and c.n >= 2049
    assert by["far_flat"].info["far_tiles"] == [0, 2, 4] and by["far_flat"].info["far2"] == 1
    c = by["far_steep"]
    s = c.oracle().sel
    far = tc.is_far(tc.feature_rows(c))
    assert far.sum() == 1 and not s.valid_pitch[far][0] and np.mean(s.heights[~s.valid_pitch & ~far]) == 1.0 and s.height_level == 1.5
    assert 1.0 < 1.25 < 1.5                                               # (the near candidate's height lies between the two levels)
    assert by["far_singular"].oracle().status == so.ST_ERR_SINGULAR and by["far_singular"].info["far2"] == 1
    assert [(c.info["far1"], c.info["far2"], c.info["over"]) for c in families["cap"]] == [(341, 0, False), (342, 0, True), (0, 192, False), (0, 193, True)]
    assert 3 * 341 <= tc.PEND_CAP < 3 * 342 and 3 * 192 <= tc.PEND_CAP_H < 3 * 193
    for c in families["far"] + families["cap"]:
        if c.oracle().status != so.ST_ERR_SINGULAR:
            assert sc.decided_rows(c)[0].all(), c.name


def test_keys_cases(families, models):
    by = {c.name: c for c in families["keys"]}
    want = {"keys/negative": so.ST_MEDIAN, "keys/no_steep": so.ST_NO_FLAT, "keys/nothing_selected": so.ST_NO_FLAT, "keys/lone_bins": so.ST_LEVEL}
    for name, st in want.items():
        assert by[name].oracle().status == st, name
    assert np.isnan(by["keys/no_steep"].oracle().height_level) and np.isnan(by["keys/no_steep"].oracle().raw_scale)
    for name, c in by.items():
        m = models[name]
        if "rel" in c.info:                                               # the band: 1e-12 from the kernel, the cases a factor 10 / 100 to either side
            rel, margin = c.info["rel"], tc.band_margin(c, m)
            assert m["level3"] == 3 * tc.L0 and abs(margin - abs(rel)) <= 0.02 * abs(rel), (name, margin)
            assert (margin <= tc.LEVEL_GUARD / 9) if c.info["redo"] else (margin >= 99 * tc.LEVEL_GUARD), (name, margin)
            sel = c.oracle().sel
            assert sel.tri_valid[4] == (rel > 0) and sel.tri_valid[5], name               # the decision itself, from the oracle
        assert sc.decided_rows(c)[0].all(), name
    h = by["keys/steep_negative"].oracle().sel
    assert (h.heights[~h.valid_pitch] < 0).all()
    h = by["keys/steep_both_signs"].oracle().sel
    assert (h.heights[~h.valid_pitch] < 0).any() and (h.heights[~h.valid_pitch] > 0).any()


def test_list_cases(families):
    sizes = sorted({c.n for c in families["lists"]})
    assert sizes == sorted(tc.list_sizes() + list(tc.LIST_LARGE)) and {(n // 64) % 8 for n in tc.list_sizes()} == set(range(8))
    assert {n % 64 for n in tc.list_sizes()} == {0, 1, 63} and all(8 <= n // 64 <= 31 for n in tc.list_sizes())
    patterns = {}
    for c in families["lists"]:
        n, cls = c.n, c.info["cls"]
        r = c.oracle()
        assert sum(c.info["wave_cands"]) == n                             # every feature is a candidate
        nfull, rem = n // 64, n % 64
        want = [64 * len(range(w, nfull, tc.DW)) + (rem if nfull % tc.DW == w else 0) for w in range(tc.DW)]
        assert c.info["wave_cands"] == want, c.name
        sel = np.zeros(n, bool)
        sel[r.sel.selected_ids] = True
        i = np.nonzero(cls == 1)[0]
        assert sel[i].all() and not sel[cls == 0].any() and sel[cls == 2].sum() == 3
        assert np.array_equal(np.floor(c.f3[i, 1] * 10).astype(int), (i // 64) % 160 + 5)               # the bin rule
        hist = np.bincount((i // 64) % 160 + 5, minlength=169)
        hist[6] += 3
        assert np.array_equal(r.road.hist_raw, hist), c.name
        patterns.setdefault(c.name.split("/")[-1], []).append(n)
        assert sc.decided_rows(c)[0].all(), c.name
    assert set(patterns) == set(tc.LIST_PATTERNS) and all(len(v) >= 24 + 4 for v in patterns.values())
    chunks = {n: max(-(-k // 64) for k in c.info["wave_cands"]) for c in families["lists"] for n in [c.n] if n in tc.LIST_LARGE}
    assert chunks == {32256: 63, 32768: 64, 32769: 65, 33280: 65}
    c = next(c for c in families["lists"] if c.name == "lists/n32256/wave5_none")
    assert not np.isin(c.oracle().sel.selected_ids // 64 % 8, [5]).any()


def test_fan_strips(families):
    assert len(families["fan"]) == 4
    for c in families["fan"]:
        rows = c.tri1.astype(np.int64)
        assert len(rows) == sc.MAX_VOTE_ROWS and (rows[:, 0] == tc.FAN_CENTRE).all() and tc.FAN_CENTRE == 3 * tc.W - 1 and c.n == tc.N_FAN
        assert c.info["far1"] == 0 and set((rows // tc.W).reshape(-1).tolist()) == {2, 3}                # every row is tile 2's; slots wrap
        assert c.votes()[tc.FAN_CENTRE] == c.info["centre_count"] and c.info["centre_count"] in (32766, -32764)


def test_status_band_and_skew_conditions(everything, models):
    for c in everything:
        m = models[c.name]
        assert tc.order_free(c), c.name
        assert tc.model_redo(c, m) == c.info["redo"], (c.name, tc.model_redo(c, m), c.info["redo"])
        if c.info["redo"] is None and c.oracle().status != so.ST_ERR_SINGULAR:
            assert tc.band_margin(c, m) >= 99 * tc.LEVEL_GUARD, (c.name, tc.band_margin(c, m))
            assert c.oracle().status in (so.ST_MODE, so.ST_RIGHT, so.ST_MEDIAN, so.ST_ERR_LEFT, so.ST_ERR_RIGHT), c.name
        assert c.info["wave_cands"] is None or m["overflow"] or c.info["wave_cands"] == np.bincount((np.nonzero(m["cand"])[0] // 64) % tc.DW, minlength=tc.DW).tolist(), c.name


def test_the_model_equals_the_oracle_and_every_mutant_is_seen(everything, models):
    for c in everything:
        assert tc.model_equals_oracle(c, models[c.name]), c.name
    seen = {tag: [c.name for c in everything if not tc.model_equals_oracle(c, tc.model(c, **kw))] for tag, kw in tc.MUTANTS.items()}
    for tag in tc.MUTANTS:
        print("mutant %-55s seen by %d cases: %s" % (tag, len(seen[tag]), ", ".join(seen[tag][:6])))
    assert all(seen[tag] for tag in tc.MUTANTS), [tag for tag in tc.MUTANTS if not seen[tag]]
    # each where it was built to be seen
    assert "keys/negative" in seen["key compared as sign-magnitude"] and "keys/at_level" in seen[">= at the level"]
    assert "far_votes/reference" in seen["far votes dropped"] and "far_votes/fixed" in seen["far votes dropped"]
    assert "far_flat" in seen["far heights dropped"] and "far_steep" in seen["far steep rows left out of the level"]
    cut = seen["selbits cut at 64 chunks"]                                 # only lists of more than 64 chunks, and every such frame with a selected entry there
    assert {"lists/n32769/all"} | {"lists/n33280/" + p for p in tc.LIST_PATTERNS} <= set(cut) and all(name.split("/")[1] in ("n32769", "n33280") for name in cut)
    assert "cap_votes/342" in seen["pending cap: a row that starts at entry 1023 fits"] and "cap_heights/192" in seen["pending cap: 575 height entries applied"]
    partial = seen["partial group credited to wavefront (nfull - 1) % 8"]
    assert partial and all(int(name.split("/")[1][1:]) % 64 for name in partial)


def test_tiny_frames():
    assert [tc.tiny_case(n).oracle().status for n in (0, 3, 4)] == [so.ST_TOO_FEW, so.ST_TOO_FEW, so.ST_NO_FLAT]
