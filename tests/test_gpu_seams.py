"""The compaction's step 1 and the tail of the LDS-resident scale kernels on the crafted frames of tests/seam_cases.py: every
selected set (none, all, the first / last three survivors, the first and last index of every wave's slice, bits 0 and 31 of
every word, large stale counters behind the bit-set) at every size of the plan, through the instantiation that takes it, in HOT
mode and in EXACT mode with the selected bytes; the compaction masks at the capacity, one below it and at ragged sizes through
the scale kernels and outlier_vote_kernel; a mixed batch, the same frames through the size-class launches, and a second launch
that must repeat the first byte for byte.  Every comparison with the oracle is equality."""
import numpy as np
import pytest

import scale_cases as sc
import seam_cases as sm
from oracle import scale_oracle as so

pytestmark = pytest.mark.gpu

CLASS_MIN_FRAMES = 2048            # kClassMinFrames


def _K():
    from mvoscalerecovery_amd import constants as K
    return K


def _same(got, want):
    return (np.isnan(got) and np.isnan(want)) or got == want


def _check(c, res, pf, f, tag, level=True):
    """status, raw scale, height, (height_level,) the counts — and, where the launch has them, the counters and selected bytes."""
    K, r = _K(), c.oracle()
    nv = int(np.asarray(r.valid).sum())
    sl = pf.frame_slice(f)
    assert res["status"][f] == r.status, (tag, c.name, res["status"][f], r.status)
    for name, want in (("raw_scale", r.raw_scale), ("height", r.height)) + ((("height_level", r.height_level),) if level else ()):
        assert _same(res[name][f], want), (tag, c.name, name, res[name][f], want)
    assert res["counts"][f, K.CNT_VALID] == nv, (tag, c.name)
    assert res["counts"][f, K.CNT_TRI_PITCH] == int(r.sel.valid_pitch.sum()), (tag, c.name)
    assert res["counts"][f, K.CNT_TRI_VALID] == int(r.sel.tri_valid.sum()), (tag, c.name)
    assert res["counts"][f, K.CNT_SELECTED] == len(r.sel.selected_ids), (tag, c.name, res["counts"][f, K.CNT_SELECTED], len(r.sel.selected_ids))
    if "selected" in res:
        assert np.array_equal(np.nonzero(res["selected"][sl][:nv])[0], r.sel.selected_ids), (tag, c.name)
        assert np.array_equal(res["vote_counters"][sl], r.counters), (tag, c.name)
        if r.road is not None and "hist" in res:
            assert np.array_equal(res["hist"][f, 0], r.road.hist_raw) and np.array_equal(res["hist"][f, 1], r.road.hist), (tag, c.name)
            assert res["counts"][f, K.CNT_KEPT] == r.road.n_kept, (tag, c.name)


def _exact_level(c):
    """Is the frame's level the same double in any summation order?  (the seam frames: walls of height exactly LEVEL, or one steep row)"""
    return c.info.get("family") in ("seam", "level_equal")


def _run_both(gpu, cases, waves, tag):
    from mvoscalerecovery_amd import _lib
    pf, res = sc.run_scale(gpu, cases, kind="hot", waves=waves, hot_only=True)
    for f, c in enumerate(cases):                                # the product kernel alone: who is handed to the exact pass
        nothing = len(c.oracle().sel.selected_ids) == 0
        handed = nothing or c.info.get("family") == "level_equal"
        if c.info.get("family") in ("seam", "level_equal"):
            assert (res["status"][f] == _lib.ST_REDO) == handed, (tag, c.name, res["status"][f])
    pf, res = sc.run_scale(gpu, cases, kind="hot", waves=waves)
    for f, c in enumerate(cases):
        _check(c, res, pf, f, tag + " HOT", level=_exact_level(c))
    pf, res = sc.run_scale(gpu, cases, kind="exact", waves=waves)
    for f, c in enumerate(cases):
        _check(c, res, pf, f, tag + " EXACT")


@pytest.fixture(scope="module")
def frames():
    return {(n, waves): sm.seam_cases(n, waves) for n, waves, _ in sm.PLAN}


@pytest.mark.parametrize("k", range(len(sm.PLAN)))
def test_selected_sets_through_every_instantiation(gpu, frames, k):
    n, waves, inst = sm.PLAN[k]
    cases = frames[(n, waves)] + [sm.handed_over_case()]
    _run_both(gpu, cases, waves, "n=%d <%d,%d>" % ((n,) + inst))
    print("seams: n=%d through <%d,%d>: %d selected sets + the handed-over frame, HOT alone / HOT / EXACT" % ((n,) + inst + (len(cases) - 1,)))


@pytest.mark.parametrize("k", range(len(sm.COMPACT_PLAN)))
def test_keep_masks_through_scale_and_vote_kernels(gpu, k):
    K = _K()
    n, waves, inst = sm.COMPACT_PLAN[k]
    cases = sc.compaction_cases(n, waves, inst[1])
    for c in cases:
        assert np.array_equal(c.oracle().valid, c.info["keep"]), c.name
    tag = "n=%d <%d,%d>" % ((n,) + inst)
    _run_both(gpu, cases, waves, tag)
    pf, st, cnt, counts = sc.run_vote(gpu, cases, waves=waves)
    for f, c in enumerate(cases):
        want = c.oracle().counters
        assert st[f] == 0 and np.array_equal(cnt[pf.frame_slice(f)], want), (tag, c.name)
        assert counts[f, K.CNT_VALID] == int((want >= 0).sum()), (tag, c.name)
    print("seams: %s, %d keep masks through scale_frames_kernel (HOT, EXACT) and outlier_vote_kernel" % (tag, len(cases)))


def _meaningful(cases, pf, res):
    out = [res[k] for k in ("status", "raw_scale", "height", "height_level", "counts") if k in res]
    if "selected" in res:
        out.append(res["vote_counters"])
        out += [res["selected"][pf.frame_slice(f)][:int(np.asarray(c.oracle().valid).sum())] for f, c in enumerate(cases)]
    return out


def test_mixed_batch_and_its_repeat(gpu):
    cases = sm.mixed_batch()
    assert len({c.n for c in cases}) >= 5
    _run_both(gpu, cases, 0, "mixed")
    for kind in ("hot", "exact"):
        pf, a = sc.run_scale(gpu, cases, kind=kind)
        pf, b = sc.run_scale(gpu, cases, kind=kind)
        for x, y in zip(_meaningful(cases, pf, a), _meaningful(cases, pf, b)):
            assert x.tobytes() == y.tobytes(), kind
    print("seams: a mixed batch of %d frames; two launches byte-identical (HOT and EXACT)" % len(cases))


def test_size_class_launches(gpu):
    """The same frames with enough small ones for one launch per size class (the LIST instantiations)."""
    big, small = sm.mixed_batch(), sm.small_batch()
    cases = big + [small[i % len(small)] for i in range(CLASS_MIN_FRAMES)]
    assert len(cases) >= CLASS_MIN_FRAMES and min(c.n for c in cases) <= 320 < 1152 < max(c.n for c in cases)
    pf, res = sc.run_scale(gpu, cases, kind="hot")
    for f, c in enumerate(cases):
        _check(c, res, pf, f, "by class", level=_exact_level(c))
    pf, again = sc.run_scale(gpu, cases, kind="hot")
    for x, y in zip(_meaningful(cases, pf, res), _meaningful(cases, pf, again)):
        assert x.tobytes() == y.tobytes()
    print("seams: %d frames in three size classes, equal to the oracle; two launches byte-identical" % len(cases))
