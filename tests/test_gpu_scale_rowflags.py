"""The scale kernels' per-thread bookkeeping of the first selection sweep on the crafted frames of tests/scale_rowflags_cases.py:
flag words whose bits 0, 31, 32 and 63 (the dense kernel: also 64, 95, 96, 127) differ from lane to lane, at exactly 64 B rows
and one row less; frames with no, one and only steep rows, rows that are neither, and a refused frame among steep rows; a
single singular or in-band row as its thread's first, last and only row.  Every launch is compared with the oracle by
test_gpu_scale_cases.py's checks (HOT: status, raw scale and height bitwise, the counts, and test_gpu_scale_chunk_edges.py's bound
on height_level; EXACT: every stage output bitwise).  The product's 4- and 8-wavefront HOT kernels take the lean form of the
bookkeeping (LeanRowBook), every other kernel the per-row form: both are run."""
import numpy as np
import pytest

import scale_cases as sc
import scale_rowflags_cases as rf
import test_gpu_scale_cases as base
import test_gpu_scale_chunk_edges as edges
from oracle import scale_oracle as so

pytestmark = pytest.mark.gpu


def _hot_and_exact(gpu, cases, waves, tag, layout="survivors"):
    pf, hot = sc.run_scale(gpu, cases, kind="hot", waves=waves, layout=layout)
    pf, exact = sc.run_scale(gpu, cases, kind="exact", waves=waves, layout=layout)
    for f, c in enumerate(cases):
        base._check_hot(c, hot, f, tag + " HOT")
        edges._check_level(c, hot, f, tag + " HOT")
        base._check_exact(c, exact, pf, f, tag + " EXACT")
    return hot, exact


@pytest.mark.parametrize("waves", [1, 4, 8])
def test_flag_words_bit_by_bit(gpu, waves):
    """64 B and 64 B - 1 rows through the instantiation whose limit that is: the selected set (one marker triangle per special
    bit), n_pitch and n_tri_valid."""
    block = 64 * waves
    cases = [rf.rowflag_bits_case(block), rf.rowflag_bits_case(block, short=1)]
    hot, exact = _hot_and_exact(gpu, cases, waves, "waves=%d" % waves)
    K = base._K()
    for f, c in enumerate(cases):                                # (spelled out: the counts are what the frames are about; the
        s = c.oracle().sel                                       # selected set is compared by the exact check)
        for res in (hot, exact):
            assert res["counts"][f, K.CNT_TRI_PITCH] == int(s.valid_pitch.sum()) and res["counts"][f, K.CNT_TRI_VALID] == int(s.tri_valid.sum())
            assert res["counts"][f, K.CNT_SELECTED] == 3 * (c.info["n_markers"] + rf.N_ABOVE), c.name
    print("flag words (waves=%d): %d and %d rows x HOT / EXACT" % (waves, len(cases[0].tri2), len(cases[1].tri2)))


def test_flag_words_of_the_dense_kernel(gpu):
    """128 B rows, B = 1024, tri2 numbered over the features: both 64-bit flag words of the dense feature-numbered kernel (the
    per-row form of the books)."""
    c = rf.rowflag_bits_case(1024, fw=2)
    assert len(c.tri2) == 128 * 1024
    _hot_and_exact(gpu, [c], 0, "dense", layout="features")
    print("flag words (dense): %d rows x HOT / EXACT" % len(c.tri2))


@pytest.mark.parametrize("waves", [1, 4, 8, 16])
def test_steep_count(gpu, waves):
    """No steep row (the level is NaN), one, only steep rows, rows that are neither; and a refused frame, whose level is still
    written: the mean over its steep rows without the row that is out of range."""
    cases = [rf.steep_count_case(k) for k in ("none", "one", "all", "nan")]
    bad, good = rf.refused_among_steep_case()
    cases[2:2] = [bad]                                           # (neighbours on both sides)
    hot, exact = _hot_and_exact(gpu, cases, waves, "waves=%d" % waves)
    want = good.oracle().height_level
    assert hot["status"][2] == exact["status"][2] == so.ST_ERR_MASK
    assert exact["height_level"][2] == want, (waves, exact["height_level"][2], want)
    assert abs(hot["height_level"][2] - want) <= edges.LEVEL_TOL * float(np.mean(np.abs(good.oracle().sel.heights))), (waves, hot["height_level"][2], want)
    print("steep count (waves=%d): %d frames x HOT / EXACT, one refused with its level written" % (waves, len(cases)))


@pytest.mark.parametrize("waves", [1, 4, 8])
def test_a_single_rare_row(gpu, waves):
    """One singular row: MVOSR_ST_ERR_SINGULAR.  One row inside the pitch test's band: the HOT kernel leaves the frame to the
    exact pass, which finishes it as the EXACT variant does.  Wherever the row sits among its thread's rows."""
    from mvoscalerecovery_amd import _lib
    block = 64 * waves
    sing = [rf.rare_row_case("singular", where, block) for where in rf.RARE_POSITIONS]
    band = [rf.rare_row_case("band", where, block) for where in rf.RARE_POSITIONS]
    cases = sing + band
    hot, exact = _hot_and_exact(gpu, cases, waves, "waves=%d" % waves)
    assert (hot["status"][:3] == so.ST_ERR_SINGULAR).all() and (exact["status"][:3] == so.ST_ERR_SINGULAR).all()
    for f in range(3, 6):
        assert hot["status"][f] == exact["status"][f] and base._same(hot["raw_scale"][f], exact["raw_scale"][f]), cases[f].name
    pf, only = sc.run_scale(gpu, cases, kind="hot", waves=waves, hot_only=True)
    assert (only["status"][3:] == _lib.ST_REDO).all() and (only["status"][:3] == so.ST_ERR_SINGULAR).all(), (waves, only["status"])
    print("rare rows (waves=%d): 3 singular frames refused, 3 in-band frames handed to the exact pass and finished as EXACT" % waves)

