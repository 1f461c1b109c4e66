"""The sequence-tail cases of tests/seqtail_cases.py on the CPU: the two restatements of the median agree, mvosr_slew_median_host
equals the recurrence, the blocked layout is sharding.shard_sizes', the cases hold what their names say — and a kernel that is
wrong in one of the ways the cases are built for would not pass them, shown on the references: a recurrence with >=, a median
that reads one element of padding, a block index that gives the head blocks base_len elements."""
import numpy as np
import pytest

import seqtail_cases as sc


@pytest.fixture(scope="module")
def median_cases():
    return sc.median_cases()


@pytest.fixture(scope="module")
def blocked_cases():
    return sc.blocked_cases()


@pytest.fixture(scope="module")
def slew_cases():
    return sc.slew_cases()


def test_median_restatements_agree(median_cases, blocked_cases):
    for c in median_cases + blocked_cases:
        a, b = sc.median_deque(c["seq"], c["window"], c["queue"]), sc.median_sorted(c["seq"], c["window"], c["queue"])
        assert (sc.same_values if c.get("by_value") else sc.same)(a, b), c["name"]


def test_median_cases_cover_what_the_issue_lists(median_cases):
    seen = {(c["window"], len(c["queue"]), len(c["seq"])) for c in median_cases}
    for w in sc.WINDOWS:
        for nq in {0, 1, w - 1, w}:
            for n in sc.LENGTHS:
                assert (w, nq, n) in seen, (w, nq, n)
        assert {c["kind"] for c in median_cases if c["window"] == w} >= set(sc.SEQ_KINDS) | {"zeros"}, w
        assert any(c["nan_in_queue"] for c in median_cases if c["window"] == w)
    for c in median_cases:
        zero = bool(np.any(c["seq"] == 0.0) or np.any(c["queue"] == 0.0))
        assert zero == c["by_value"], c["name"]                       # zeros in the one kind that is compared by value, nowhere else
        ref = sc.median_deque(c["seq"], c["window"], c["queue"])
        w, n = c["window"], len(c["seq"])
        if c["kind"] == "one_nan" and not c["nan_in_queue"]:
            at = n // 2                                                # NaN at exactly `window` consecutive outputs and nowhere else
            want = np.zeros(n, bool)
            want[at:at + w] = True
            assert np.array_equal(np.isnan(ref), want), c["name"]
        if c["nan_in_queue"]:
            # the queue's NaN, element nq // 2 of the queue, is in the window until len(queue) - nq // 2 + i + 1 > window
            nq = len(c["queue"])
            want = np.arange(n) + 1 + (nq - nq // 2) <= w
            assert np.array_equal(np.isnan(ref), want), c["name"]
        if c["kind"] == "inf_middles" and w % 2 == 0 and n > 3 * w:
            full = np.arange(n) + 1 + len(c["queue"]) >= 2 * w         # (the window is full and the queue has left it)
            inf_only = np.arange(n) < 2 * n // 3
            assert np.all(np.isnan(ref[full & inf_only])), c["name"]   # +inf and -inf as the two middle elements: NaN
        if c["kind"] == "overflow" and w % 2 == 0 and n > 3 * w:
            assert np.isinf(ref[n // 2 - 1]) and np.isinf(ref[-1]) and ref[n // 2 - 1] > 0 > ref[-1], c["name"]
        if c["kind"] == "denormal":
            assert np.all(np.abs(ref) < 2.3e-308) and np.all(ref != 0.0)


def test_blocked_layout_is_the_sharding_layout(blocked_cases):
    from mvoscalerecovery_amd import sharding
    combos = set()
    for c in blocked_cases:
        n, nb = len(c["seq"]), c["n_blocks"]
        assert c["sizes"] == sharding.shard_sizes(n, nb) and sum(c["sizes"]) == n
        assert c["sizes"] == [n // nb + (1 if r < n % nb else 0) for r in range(nb)]
        assert sc.same(sc.concat_blocks(c["buf"], c["sizes"], c["stride"]), c["seq"]), c["name"]
        assert c["stride"] >= max(c["sizes"]) and c["padded"] == (c["stride"] > max(max(c["sizes"]), 1))
        got = np.array([sc.seq_at(c["buf"], n, nb, c["stride"], i) for i in range(n)])
        assert sc.same(got, c["seq"]), c["name"]                      # the kernel's index arithmetic, restated
        combos.add((nb, "lt" if n < nb else "eq" if n == nb else n % nb))
    for nb in sc.N_BLOCKS:
        assert {(nb, 0), (nb, 1), (nb, nb - 1), (nb, "lt"), (nb, "eq")} <= combos, nb
    assert any(c["n_blocks"] == 64 and c["window"] == 64 and c["sizes"] == [5] * 64 for c in blocked_cases)   # a window over 13 blocks
    assert any(len(c["queue"]) and c["padded"] for c in blocked_cases)


def test_a_median_that_reads_padding_differs(blocked_cases):
    """Every padded case with a short block that another non-empty block follows (two or more blocks of base_len >= 1 elements
    behind the head blocks): reading each block as long as the longest takes one element of padding — NaN or 1e300 — into the
    sequence in front of that block, and the medians differ."""
    hit = 0
    for c in blocked_cases:
        if not c["padded"] or c["extra"] == 0 or c["base_len"] == 0 or c["n_blocks"] - c["extra"] < 2:
            continue
        wrong = sc.concat_blocks_reading_padding(c["buf"], c["sizes"], c["stride"])[:len(c["seq"])]
        assert not sc.same(sc.median_deque(wrong, c["window"], c["queue"]), sc.median_deque(c["seq"], c["window"], c["queue"])), c["name"]
        hit += 1
    assert hit >= 16                                                   # (n % n_blocks == 1 with 3, 7, 8, 64 blocks, both windows, both paddings)


def test_a_block_index_with_short_head_blocks_differs(blocked_cases):
    """Every case with extra > 0: an index that gives the head blocks base_len elements reads other elements — or none: with
    base_len 0 it divides by zero, and where the stride is the longest block it can run past the end of the buffer."""
    hit = 0
    for c in blocked_cases:
        if c["extra"] == 0:
            continue
        n, nb = len(c["seq"]), c["n_blocks"]
        try:
            wrong = np.array([sc.seq_at(c["buf"], n, nb, c["stride"], i, head_len_is_base=True) for i in range(n)])
        except ZeroDivisionError:
            assert c["base_len"] == 0
            hit += 1
            continue
        except IndexError:
            hit += 1
            continue
        assert not sc.same(wrong, c["seq"]), c["name"]
        assert not sc.same(sc.median_deque(wrong, c["window"], c["queue"]), sc.median_deque(c["seq"], c["window"], c["queue"])), c["name"]
        hit += 1
    assert hit >= 20


def test_slew_host_equals_the_recurrence(slew_cases):
    assert {len(c["raw"]) for c in slew_cases} >= set(sc.SLEW_LENGTHS)
    for c in slew_cases:
        p, f = sc.slew_reference(c)
        hp, hf, s_out = sc.run_slew_host(c)
        assert sc.same(hp, p) and sc.same(hf, f), c["name"]
        assert sc.same([s_out], [p[-1]]), c["name"]
        assert sc.same(f, sc.median_sorted(p, c["window"], c["queue"])), c["name"]


def test_slew_cases_hold_what_their_names_say(slew_cases):
    by = {c["name"]: c for c in slew_cases}
    # the ramp: a thousand rounded additions are not one multiplication
    c = by["ramp"]
    p, _ = sc.slew_reference(c)
    k = np.arange(1, 1001)
    assert np.all(np.diff(p[:1000]) > 0) and np.all(np.diff(p[1000:]) < 0)
    assert np.any(p[:1000] != c["scale_in"] + k * sc.SLEW) and p[1999] != c["scale_in"]
    s = c["scale_in"]
    for i in range(1000):
        s += sc.SLEW
        assert p[i] == s
    # the exact-limit pairs: met with the running scale exactly s, the value taken — and a recurrence with >= differs there
    c = by["exact_limit"]
    p, _ = sc.slew_reference(c)
    wrong, _ = sc.slew_reference(c, at_limit_moves=True)
    assert len(c["exact_at"]) == 2 * len(sc.EXACT_UP) and {a % 64 for a in c["exact_at"]} >= {0, 63}
    for j, at in enumerate(c["exact_at"]):
        before = c["scale_in"] if at == 0 else p[at - 1]
        assert abs(c["raw"][at] - before) == sc.SLEW and p[at] == c["raw"][at], (j, at)
        assert wrong[at] != p[at] and wrong[at] in (before + sc.SLEW, before - sc.SLEW), (j, at)
    assert not sc.same(p, wrong)
    # NaN: not applied, it never reaches the scale; applied, it is the scale until the next applied finite frame
    p, _ = sc.slew_reference(by["nan_not_applied"])
    assert not np.any(np.isnan(p)) and np.any(np.isnan(by["nan_not_applied"]["raw"]))
    c = by["nan_applied"]
    p, f = sc.slew_reference(c)
    assert np.array_equal(np.isnan(p), np.isnan(c["raw"])) and np.isnan(p).sum() == 5
    after = [i + 1 for i in np.nonzero(np.isnan(p))[0] if not np.isnan(c["raw"][i + 1])]
    assert len(after) == 4 and all(p[i] == c["raw"][i] for i in after)              # the finite frame after a NaN takes its own value
    p, _ = sc.slew_reference(by["block_of_zeros"])
    assert np.all(p[64:128] == p[63])
    p, _ = sc.slew_reference(by["apply_2_and_minus1"])
    moved = np.nonzero(np.diff(np.concatenate([[by["apply_2_and_minus1"]["scale_in"]], p])))[0]
    assert {int(v) for v in by["apply_2_and_minus1"]["apply"][moved]} == {2, -1}
    assert np.isnan(sc.slew_reference(by["scale_in_nan_not_applied"])[0]).all()
    p, _ = sc.slew_reference(by["scale_in_nan"])
    assert p[0] == by["scale_in_nan"]["raw"][0]
    p, _ = sc.slew_reference(by["inf_raw"])
    assert np.all(np.isfinite(p)) and p[3] == p[2] + sc.SLEW and p[10] == p[9] - sc.SLEW
