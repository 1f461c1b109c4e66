"""The LDS-resident scale kernels at the edges of their streamed loops (tests/scale_chunk_cases.py): row counts of either
triangulation around one and two chunks of 2 B rows, feature counts around the staging loop's second half-load and at the
instantiation's capacity, flat rows only in the last trip / only in the last lane / in none of some trips, an id out of range in
the last partial chunk of either triangulation, and a survivor count that is not the one the second triangulation was built on.

The product (HOT) launch is compared with the oracle by test_gpu_scale_cases.py's own hot check (status, raw scale and height
bitwise, the counts), its height_level within 1e-13 of the oracle's (the product path sums 3 h in the workgroup's order); the
same frames through the EXACT variant by that file's exact check (every stage output bitwise), and the two launches' raw scales
bit for bit."""
import numpy as np
import pytest

import scale_cases as sc
import scale_chunk_cases as cc
import test_gpu_scale_cases as base
from oracle import scale_oracle as so

pytestmark = pytest.mark.gpu

LEVEL_TOL = 1e-13


@pytest.fixture(scope="module")
def families():
    return {w: cc.family(w) for w in cc.WAVES}


def _check_level(c, res, f, tag):
    if c.status is not None or c.oracle().status == so.ST_ERR_SINGULAR:
        return 0.0
    want, got = c.oracle().height_level, res["height_level"][f]
    if np.isnan(want):
        assert np.isnan(got), (tag, c.name)
        return 0.0
    err = abs(got - want) / max(abs(want), float(np.mean(np.abs(c.oracle().sel.heights))))
    assert err <= LEVEL_TOL, (tag, c.name, got, want, err)
    return err


def _check_batch(gpu, cases, waves, tag, mutate=None, refused=()):
    """HOT and EXACT launches of one batch against the oracle; frames in `refused` must come back MVOSR_ST_ERR_MASK."""
    K = base._K()
    pf, hot = sc.run_scale(gpu, cases, kind="hot", waves=waves, mutate=mutate)
    pf, exact = sc.run_scale(gpu, cases, kind="exact", waves=waves, mutate=mutate)
    worst = 0.0
    for f, c in enumerate(cases):
        if f in refused:
            assert hot["status"][f] == K.ST_ERR_MASK and exact["status"][f] == K.ST_ERR_MASK, (tag, c.name, hot["status"][f], exact["status"][f])
            continue
        base._check_hot(c, hot, f, tag + " HOT")
        worst = max(worst, _check_level(c, hot, f, tag + " HOT"))
        base._check_exact(c, exact, pf, f, tag + " EXACT")
        assert hot["status"][f] == exact["status"][f] and base._same(hot["raw_scale"][f], exact["raw_scale"][f]), (tag, c.name)
    return worst


@pytest.mark.parametrize("waves", cc.WAVES)
def test_chunk_edges_against_the_oracle(gpu, families, waves):
    cases = families[waves]
    worst = _check_batch(gpu, cases, waves, "waves=%d" % waves)
    n_bad = sum(c.status is not None for c in cases)
    assert n_bad == 2
    print("chunk edges (waves=%d): %d frames x HOT / EXACT, %d refused for an id out of range; largest level error %.2e (bound %g)"
          % (waves, len(cases), n_bad, worst, LEVEL_TOL))


@pytest.mark.parametrize("waves", cc.WAVES[1:])
def test_chunk_edges_through_the_wide_instantiation(gpu, waves):
    cases = cc.wide_family(waves)
    assert max(c.n for c in cases) == cc.capacity(waves) + 1
    worst = _check_batch(gpu, cases, waves, "wide waves=%d" % waves)
    print("chunk edges (<%d,8>): %d frames x HOT / EXACT; largest level error %.2e" % (waves, len(cases), worst))


@pytest.mark.parametrize("waves", cc.WAVES)
def test_survivor_count_that_tri2_was_not_built_on(gpu, families, waves):
    """n2_expected off by one (either way) refuses those frames and only those; without n2_expected the batch runs as it is."""
    cases = [c for c in families[waves] if c.status is None][::5]
    up, down = 1, len(cases) - 2

    def off_by_one(pf):
        pf.n2_expected = pf.n2_expected.copy()
        pf.n2_expected[up] += 1
        pf.n2_expected[down] -= 1

    def no_expectation(pf):
        pf.n2_expected = None

    _check_batch(gpu, cases, waves, "n2+-1 waves=%d" % waves, mutate=off_by_one, refused=(up, down))
    _check_batch(gpu, cases, waves, "n2 null waves=%d" % waves, mutate=no_expectation)
    print("n2_expected (waves=%d): %d frames, two refused when it is off by one, none without it" % (waves, len(cases)))
