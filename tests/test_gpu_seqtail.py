"""The sequence tail on the device against tests/seqtail_cases.py: mvosr_window_median, mvosr_window_median_blocked and
mvosr_slew_median through the C entry points.  What a case must give is defined exactly — medians, and a recurrence of rounded
double additions — so every comparison is equality, byte for byte with NaN at the same positions (the signed-zero case by
value); every output buffer carries one guard element behind its end."""
import numpy as np
import pytest

import seqtail_cases as sc

pytestmark = pytest.mark.gpu


def test_window_median_contiguous_cases(gpu):
    for c in sc.median_cases():
        want = sc.median_deque(c["seq"], c["window"], c["queue"])
        rc, got, guard = sc.run_median(gpu, c["seq"], c["window"], c["queue"])
        assert rc == 0 and guard, c["name"]
        assert (sc.same_values if c["by_value"] else sc.same)(got, want), c["name"]


def test_window_median_blocked_cases(gpu):
    """Each blocked result equals the reference and the contiguous call on the concatenated sequence."""
    for c in sc.blocked_cases():
        want = sc.median_deque(c["seq"], c["window"], c["queue"])
        rc, got, guard = sc.run_median(gpu, c["seq"], c["window"], c["queue"], blocks=(c["buf"], c["n_blocks"], c["stride"]))
        assert rc == 0 and guard, c["name"]
        assert sc.same(got, want), c["name"]
        rc, flat, guard = sc.run_median(gpu, sc.concat_blocks(c["buf"], c["sizes"], c["stride"]), c["window"], c["queue"])
        assert rc == 0 and guard and sc.same(got, flat), c["name"]


def test_window_median_launcher_refusals(gpu):
    """MVOSR_ERR_ARG and nothing launched: the output keeps its fill."""
    seq = 1.0 + np.arange(23, dtype=np.float64)
    buf, sizes, stride = sc.build_blocks(seq, 4)
    assert sizes == [6, 6, 6, 5] and stride == 6

    def refused(window, queue, blocks):
        rc, got, guard = sc.run_median(gpu, seq, window, queue, blocks=blocks)
        return rc == sc.ERR_ARG and guard and sc.all_sentinel(got)

    assert refused(5, (), (buf, 4, 5))                               # stride shorter than the longest block
    for blocks in (None, (buf, 4, 6)):
        assert refused(0, (), blocks) and refused(65, (), blocks)
        assert refused(5, np.ones(6), blocks)                        # n_queue > window
        assert refused(64, np.ones(65), blocks)
    assert refused(5, (), (buf, 0, 6))                               # n_blocks 0
    # n % n_blocks == 0: every block has base_len elements, a stride of base_len - 1 is refused and one of base_len is not
    b20 = sc.build_blocks(seq[:20], 4)[0]
    rc, got, guard = sc.run_median(gpu, seq[:20], 5, (), blocks=(b20, 4, 4))
    assert rc == sc.ERR_ARG and guard and sc.all_sentinel(got)
    rc, got, guard = sc.run_median(gpu, seq[:20], 5, (), blocks=(b20, 4, 5))
    assert rc == 0 and guard and sc.same(got, sc.median_deque(seq[:20], 5))


def test_slew_median_cases(gpu):
    """Device, host function and Python recurrence agree byte for byte on `pushed` and `filtered`."""
    for c in sc.slew_cases():
        want_p, want_f = sc.slew_reference(c)
        p, f, guards = sc.run_slew(gpu, c)
        assert guards, c["name"]
        assert sc.same(p, want_p), (c["name"], np.nonzero(~(p == want_p) & ~(np.isnan(p) & np.isnan(want_p)))[0][:5])
        assert sc.same(f, want_f), c["name"]
        hp, hf, _ = sc.run_slew_host(c)
        assert sc.same(p, hp) and sc.same(f, hf), c["name"]
