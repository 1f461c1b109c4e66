"""CPU half of the seam tests: the NumPy twin of tests/seam_cases.py against plain statements of the tail's rules, the mutants it
must expose, and the crafted frames against the oracle (the selected set is the prescribed one, every frame is clear of the HOT kernel's
guard band except the one built to be handed over).  tests/test_gpu_seams.py runs the same frames on the device."""
import numpy as np
import pytest

import scale_cases as sc
import seam_cases as sm
from oracle import scale_oracle as so


def _counters(n, seed):
    """Counters of all-surviving features as a vote leaves them: 1 + rows, a few large."""
    rng = np.random.default_rng([7, n, seed])
    c = rng.integers(1, 8, n)
    c[rng.integers(0, n, 5)] = 30000
    return c


def _tail_inputs():
    """(tag, n, waves, sc, ids): every selected set of every planned size, with nvalid = n."""
    for n, waves, (W, S) in sm.PLAN:
        for tag, ids in sm.selected_sets(n, waves).items():
            yield "n%d/<%d,%d>/%s" % (n, W, S, tag), n, W, S, np.array(sorted(ids), dtype=np.int64)


def test_plan_reaches_every_instantiation_of_the_issue():
    assert {inst for _, _, inst in sm.PLAN} == {(1, 8), (4, 4), (4, 8), (8, 4), (8, 8), (16, 4)}
    for n, waves, (W, S) in sm.PLAN + sm.COMPACT_PLAN:
        assert W == waves and n <= W * S * 64 and (S == 8 or W == 1 or n <= W * 4 * 64)
        assert S == (8 if W == 1 or n > W * 4 * 64 else 4)                        # the dispatch's choice of SC
    # slices: a size whose last waves are empty, and nvalid on both sides of a slice edge
    assert any(sm.tail_partition(n, w)[1][-1] >= n for n, w, _ in sm.PLAN if w > 1)
    sizes = {n for n, _, _ in sm.PLAN}
    assert {63 + 1, 65, 511, 512, 513, 2047, 2048, 2049} <= sizes


def test_partition_covers_the_survivors_once():
    for nvalid in list(range(1, 200)) + [511, 512, 513, 1999, 2047, 2048, 2049, 4095, 4096]:
        for waves in (1, 4, 8, 16):
            per, begin, end = sm.tail_partition(nvalid, waves)
            assert per == -(-nvalid // (64 * waves)) * 64 and per % 64 == 0
            owner = np.full(nvalid, -1)
            for w in range(waves):
                assert begin[w] % 32 == 0                                        # a slice starts on a word boundary
                assert (owner[begin[w]:end[w]] == -1).all()
                owner[begin[w]:end[w]] = w
            assert (owner >= 0).all() and (np.diff(owner) >= 0).all()


def test_tail_twin_equals_flatnonzero_and_cumsum():
    checked = 0
    for tag, n, W, S, ids in _tail_inputs():
        words = sm.lds_words(n, _counters(n, 1), ids, W * S * 2)
        nsel, dense, bases = sm.tail_twin(words, n, W, S)
        sel = np.zeros(n, bool)
        sel[ids] = True
        assert nsel == int(sel.sum()), tag
        assert np.array_equal(dense, np.flatnonzero(sel)), tag                   # the dense list: the selected survivors, in order
        per, begin, end = sm.tail_partition(n, W)
        before = np.concatenate([[0], np.cumsum(sel)])
        assert np.array_equal(bases, before[np.minimum(begin, n)]), tag          # a wave's base: the selected points in front of its slice
        checked += 1
    # survivors fewer than features: the zeroed words reach (n + 31) / 32, the live ones (nvalid + 31) / 32
    for n, nvalid, W, S in ((2000, 1500, 8, 4), (2048, 33, 8, 4), (320, 64, 1, 8), (1024, 1000, 4, 4)):
        ids = np.unique([0, 31, 32, nvalid - 1])
        words = sm.lds_words(n, _counters(n, 2), ids, W * S * 2)
        nsel, dense, _ = sm.tail_twin(words, nvalid, W, S)
        assert nsel == len(ids) and np.array_equal(dense, ids)
        checked += 1
    print("tail twin: %d (size, instantiation, selected set) combinations equal np.flatnonzero / np.cumsum" % checked)


def test_each_mutant_is_caught_by_a_case():
    caught = {"stale": [], "own_word": []}
    for tag, n, W, S, ids in _tail_inputs():
        words = sm.lds_words(n, _counters(n, 1), ids, W * S * 2)
        good = sm.tail_twin(words, n, W, S)
        for mutant in ("stale", "own_word"):
            bad = sm.tail_twin(words, n, W, S, mutant=mutant)
            if bad[0] != good[0] or not np.array_equal(bad[1], good[1]):
                caught[mutant].append(tag)
    for mutant, tags in caught.items():
        print("mutant %-8s caught by %3d cases, e.g. %s" % (mutant, len(tags), ", ".join(tags[:4])))
        assert tags, mutant
    # what the cases are for: the unmasked stale word needs a frame short of the capacity, the base a selected point in a wave's
    # first word
    assert not any(t.startswith("n2048/<8,4>") for t in caught["stale"])          # (n = capacity: no word past the bit-set)
    assert any("slice_edges" in t for t in caught["own_word"]) and not any("/none" in t for t in caught["own_word"])


@pytest.fixture(scope="module")
def frames():
    return {(n, waves): sm.seam_cases(n, waves) for n, waves, _ in sm.PLAN}


def test_frames_select_exactly_the_prescribed_set(frames):
    total = 0
    for (n, waves), cases in frames.items():
        for c in cases:
            r = c.oracle()
            want = c.info["want_selected"]
            assert np.asarray(r.valid).all() and c.n == n, c.name
            assert np.array_equal(r.sel.selected_ids, want), (c.name, len(r.sel.selected_ids), len(want))
            assert r.status == (so.ST_NO_FLAT if len(want) == 0 else r.status) and r.status != so.ST_ERR_SINGULAR, (c.name, r.status)
            if len(want):                                        # clear of the guard band and of the pitch band: not handed over
                _, status, gap, pitch = sc.control_margins(c)
                assert gap >= 1e-3 and pitch >= 1.0 and status != so.ST_LEVEL, (c.name, status, gap, pitch)
            total += 1
    print("seam frames: %d frames, the oracle's selected set is the prescribed one" % total)


def test_twin_on_the_oracle_words_gives_the_oracle_selection(frames):
    """The frames through the twin with the oracle's own counters in the stale words (the 'stale' frames put large ones there)."""
    for n, waves, (W, S) in sm.PLAN:
        for c in frames[(n, waves)]:
            words, nvalid = sm.oracle_words(c, W, S)
            nsel, dense, _ = sm.tail_twin(words, nvalid, W, S)
            assert nsel == len(c.info["want_selected"]) and np.array_equal(dense, c.info["want_selected"]), c.name
            if n + 31 < W * S * 64:
                assert sm.tail_twin(words, nvalid, W, S, mutant="stale")[0] > nsel, c.name


def test_stale_frames_leave_large_counters_behind_the_bit_set():
    c = sm.seam_cases(1153, 8)[-1]
    counters = c.oracle().counters
    first = 2 * ((c.n + 31) // 32)
    assert counters[first:first + 8].min() >= 200 and np.asarray(c.oracle().valid).all()
    assert sc.only_decided(sm.handed_over_case()).info["family"] == "level_equal"
