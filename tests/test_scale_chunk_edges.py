"""CPU twin of tests/test_gpu_scale_chunk_edges.py: the family of tests/scale_chunk_cases.py really holds every boundary the
GPU test is about — the row counts, the feature counts, where the flat rows sit, the ids out of range — so that a change of the
helper cannot hollow the GPU test without this file failing."""
import numpy as np
import pytest

import scale_cases as sc
import scale_chunk_cases as cc
from oracle import scale_oracle as so


@pytest.fixture(scope="module")
def families():
    return {w: cc.family(w) for w in cc.WAVES}


@pytest.mark.parametrize("waves", cc.WAVES)
def test_row_counts_cover_the_chunk_boundaries(families, waves):
    B = cc.block(waves)
    want = {1, 2 * B - 1, 2 * B, 2 * B + 1, 4 * B, 4 * B + 1}
    assert set(cc.row_counts(waves)) == want and cc.chunk(waves) == 2 * B
    got = {(len(c.tri1), len(c.tri2)) for c in families[waves] if c.name.startswith("counts/")}
    assert got == {(a, b) for a in want for b in want}                     # independently: the whole cross product
    for c in families[waves]:
        if c.name.startswith("counts/"):
            nv = int(c.oracle().valid.sum())
            assert c.tri1.min() >= 0 and c.tri1.max() < c.n and c.tri2.min() >= 0 and c.tri2.max() < nv, c.name
            assert len(c.tri2) <= 64 * B and len(c.tri1) <= sc.MAX_VOTE_ROWS, c.name
            assert c.oracle().status != so.ST_ERR_SINGULAR, c.name
    # rows of a real triangulation, in its order: a count within the triangulation is its first rows
    c = next(c for c in families[waves] if c.info.get("t1n") == 1)
    assert np.array_equal(c.tri1, so.delaunay(c.f2)[:1])


@pytest.mark.parametrize("waves", cc.WAVES)
def test_feature_counts_cover_the_staging_edges(families, waves):
    B, cap = cc.block(waves), cc.capacity(waves)
    ns = sorted(c.n for c in families[waves] if c.name.startswith("features/"))
    assert ns == sorted({4, 2 * B - 1, 2 * B, 2 * B + 1, cap - 1, cap})
    half = lambda n: (n + 1) // 2                                           # pairs of features: one lane, one load each
    assert half(2 * B - 1) == B and half(2 * B) == B and half(2 * B + 1) == B + 1
    assert any(n % 2 for n in ns) and cap == (512 if waves == 1 else 256 * waves)
    assert max(c.n for c in families[waves]) == cap                        # the batch runs through the <W, 4> (<1, 8>) instantiation
    for c in families[waves]:
        if c.name.startswith("features/") and c.n > 4:
            assert len(c.tri1) > c.n and len(c.tri2) > int(c.oracle().valid.sum()) // 2, c.name     # the frame's own triangulations


@pytest.mark.parametrize("waves", cc.WAVES)
def test_flat_rows_sit_where_the_names_say(families, waves):
    B = cc.block(waves)
    flat = {c.name.split("/")[-1]: c for c in families[waves] if c.info.get("family") == "flat_rows"}
    assert set(flat) == {"last_trip", "last_partial_trip", "last_lane", "trips_0_and_2_of_4"}
    for name, c in flat.items():
        got = np.nonzero(c.oracle().sel.valid_pitch)[0]
        assert np.array_equal(got, np.sort(c.info["flat_at"])), name      # the oracle finds exactly the planted rows flat
        assert c.oracle().sel.tri_valid[got].all() and c.oracle().status != so.ST_ERR_SINGULAR, name   # ... and above the level
        assert int(c.oracle().valid.sum()) == c.n, name
    trips = lambda c: -(-len(c.tri2) // (2 * B))
    trip, lane = cc.flat_trips(flat["last_trip"])
    assert trips(flat["last_trip"]) == 3 and set(trip) == {2}
    trip, lane = cc.flat_trips(flat["last_partial_trip"])
    assert len(flat["last_partial_trip"].tri2) == 4 * B + 1 and list(trip) == [2] and list(lane) == [0]
    trip, lane = cc.flat_trips(flat["last_lane"])
    assert set(lane) == {B - 1} and set(trip) == set(range(trips(flat["last_lane"])))
    trip, lane = cc.flat_trips(flat["trips_0_and_2_of_4"])
    assert trips(flat["trips_0_and_2_of_4"]) == 4 and set(trip) == {0, 2}


@pytest.mark.parametrize("waves", cc.WAVES)
def test_refused_frames_have_one_id_out_of_range_in_the_last_partial_chunk(families, waves):
    B = cc.block(waves)
    bad = [c for c in families[waves] if c.status is not None]
    assert [c.info["which"] for c in bad] == [1, 2] and all(c.status == so.ST_ERR_MASK for c in bad)
    pos = [families[waves].index(c) for c in bad]
    assert 0 < pos[0] and pos[1] < len(families[waves]) - 1                # neighbours on both sides
    for c in bad:
        rows, limit = (c.tri1, c.n) if c.info["which"] == 1 else (c.tri2, c.info["n_valid"])
        other, other_limit = (c.tri2, c.info["n_valid"]) if c.info["which"] == 1 else (c.tri1, c.n)
        assert len(rows) == 4 * B + 1 and len(rows) % (2 * B) == 1         # the last chunk holds one row
        out = np.argwhere((rows < 0) | (rows >= limit))
        assert len(out) == 1 and out[0][0] == len(rows) - 1 and rows[-1].max() == limit
        assert other.min() >= 0 and other.max() < other_limit
        assert c.info["n_valid"] == int(c.oracle().valid.sum())


@pytest.mark.parametrize("waves", cc.WAVES[1:])
def test_wide_family_needs_the_eight_subchunk_instantiation(waves):
    B = cc.block(waves)
    cases = cc.wide_family(waves)
    assert max(c.n for c in cases) == cc.capacity(waves) + 1 <= 2 * cc.capacity(waves)
    assert (cc.capacity(waves) + 2) // 2 > 2 * B                           # its staging loop makes a second trip
    assert {(len(c.tri1), len(c.tri2)) for c in cases} >= {(2 * B, 2 * B), (4 * B + 1, 2 * B + 1)}
    assert sum(c.info.get("family") == "flat_rows" for c in cases) == 4
