"""The margin of the road kernel's interior test (kSingleMargin in csrc/mvosr_kernels.hip), checked on the kernel's own
edge doubles with NumPy: a value of bin b that keeps the margin c from both edges of its bin is dropped by remove_single
exactly when bin b itself has count 1 — whatever its neighbours' counts, and for the closed interval of the first single
bin as for the half-open one of the others."""
import itertools
import os
import re
from fractions import Fraction

import numpy as np

from gpu_helpers import _oracle

C_MARGIN = 2.0 ** -40                          # kSingleMargin
N_BINS = 169


def _edge_mismatch():
    """max over k = 0..169 of |fl(edge(k+1) - 0.1) - edge(k)|, exactly (edges: the doubles (double)k * 0.1)."""
    e = np.arange(0, N_BINS + 2, dtype=np.float64) * 0.1
    lo = e[1:] - 0.1
    return max(abs(Fraction(float(lo[k])) - Fraction(float(e[k]))) for k in range(N_BINS + 1))


def test_margin_is_the_kernels():
    src = os.path.join(os.path.dirname(__file__), "..", "mvoscalerecovery_amd", "csrc", "mvosr_kernels.hip")
    m = re.search(r"constexpr double kSingleMargin = (0x1p-\d+);", open(src).read())
    assert m and float.fromhex(m.group(1)) == C_MARGIN


def test_margin_against_edge_mismatch():
    so = _oracle()
    assert np.array_equal(so.BIN_EDGES, np.arange(0, N_BINS + 1, dtype=np.float64) * 0.1)      # the kernel's bin_edge(k)
    delta = _edge_mismatch()
    assert delta == Fraction(2.0 ** -48)
    assert Fraction(C_MARGIN) >= 16 * delta


def _values(rng, lo, hi):
    a, b = lo + C_MARGIN, hi - C_MARGIN
    return np.concatenate([[a, np.nextafter(a, hi), b, np.nextafter(b, lo)], rng.uniform(np.nextafter(a, hi), np.nextafter(b, lo), 16)])


def test_interior_value_drops_with_its_own_bin_only():
    so = _oracle()
    e = so.BIN_EDGES
    rng = np.random.default_rng(20261020)
    n_checked = 0
    for b in range(N_BINS):
        y = _values(rng, e[b], e[b + 1])
        assert np.all(np.searchsorted(e, y, side="right") - 1 == b)                         # np.histogram's bin
        inside = (y - e[b] > C_MARGIN) & (e[b + 1] - y > C_MARGIN)                          # the kernel's test
        assert inside[1] and inside[3] and inside[4:].all()
        # left / own / right single in every combination; each once with the pattern's lowest single as the list's first
        # single bin (closed interval) and once with an earlier single far to the left (all of the pattern half-open)
        for left, own, right, earlier in itertools.product((False, True), repeat=4):
            if (left and b == 0) or (right and b == N_BINS - 1) or (earlier and b < 3):
                continue
            hist = np.full(N_BINS, 5)
            if left:
                hist[b - 1] = 1
            if own:
                hist[b] = 1
            if right:
                hist[b + 1] = 1
            if earlier:
                hist[b - 3] = 1
            drop = so.single_bin_drop_mask(y, hist)
            assert np.array_equal(drop, np.full(y.shape, own)), (b, left, own, right, earlier, drop)
            n_checked += 1
    assert n_checked > 8 * N_BINS
