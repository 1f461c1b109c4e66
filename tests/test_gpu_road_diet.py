"""The road-model kernel's lean path after its diet: the interior test in front of remove_single's interval test, the tail's
divisions and roots taken one per lane, whole groups of rows without the partial-row bookkeeping.  Every list goes through
`road_model_batch` twice without the statistics output (the lean kernel, its cold list behind it) and once with it (the
full variant); all three are compared with the oracle with `==`."""
import numpy as np
import pytest

import scale_cases as sc
from gpu_helpers import _assert_frame_equal, _oracle
from test_gpu_road_hot import TIERS, _lists_of, _median_case, _ordinary
from test_gpu_road_onepass import _cluster_list, _run

N_BINS = 169


def _ulps(x, k):
    """x moved k doubles up (k < 0: down)."""
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def _compare(gpu, lists, want_cold=None):
    so = _oracle()
    F = len(lists)
    hl = 0.5 + 0.001 * np.arange(F)
    lean = _run(gpu, lists, hl, False)
    _, cold = _lists_of(gpu, F)
    lean2 = _run(gpu, lists, hl, False)
    full = _run(gpu, lists, hl, True)
    for k in ("status", "height", "raw_scale", "counts"):
        assert np.array_equal(lean[k], lean2[k], equal_nan=True), k                            # run-to-run identity
    for k in ("status", "height", "counts"):
        assert np.array_equal(lean[k], full[k], equal_nan=True), (k, np.flatnonzero(lean["status"] != full["status"]))
    for i, y in enumerate(lists):
        rm = so.road_model(np.asarray(y, dtype=np.float64), hl[i])
        assert lean["status"][i] == rm.status, (i, len(y), lean["status"][i], rm.status)
        assert lean["counts"][i, 4] == rm.n_kept and lean["counts"][i, 5] == rm.n_modes, (i, len(y), lean["counts"][i], rm.n_kept, rm.n_modes)
        if rm.status in (so.ST_MODE, so.ST_RIGHT, so.ST_MEDIAN, so.ST_LEVEL):
            assert lean["height"][i] == rm.height, (i, len(y), lean["height"][i], rm.height)
            assert lean["raw_scale"][i] == 1.75 / rm.height, i
        else:
            assert np.isnan(lean["height"][i]), i
    if want_cold is not None:
        assert sorted(int(f) for f in cold) == sorted(want_cold), (sorted(cold), sorted(want_cold))


def _edge_ulp_lists():
    """A populous bin b with single bins beside it, values on and next to the shared edges.  Left single: its lone value at
    its own lower edge + u ulps ("low"), or the double just below edge(b) ("top", the upper end of its interval).  Right
    single: its lone value at edge(b+1) + u ulps — u = 0 is the shared edge itself.  Each once as the list's first single
    bin and once behind an earlier single three bins further left (where there is room for one)."""
    so = _oracle()
    e = so.BIN_EDGES
    rng = np.random.default_rng(20261020)
    lists = []
    for b in (0, 1, 84, 167, 168):
        for left, right in (("low", None), (None, "low"), ("low", "low"), ("top", None), ("top", "low")):
            if (left and b == 0) or (right and b == N_BINS - 1):
                continue
            for u in range(9):
                for earlier in (False, True):
                    if earlier and b < 4:
                        continue
                    v = list(rng.uniform(e[b] + 0.01, e[b + 1] - 0.01, 29))
                    v += [float(e[b]), _ulps(e[b], 1), _ulps(e[b], 2)]
                    v += [_ulps(e[b + 1], -j) for j in range(1, 9)]                  # edge(b+1) minus 1..8 ulps: bin b's
                    if left == "low":
                        v.append(_ulps(e[b - 1], u))
                    elif left == "top":
                        v.append(_ulps(e[b], -1))
                    elif b > 0:
                        v += [_ulps(e[b], -1), float(e[b - 1]) + 0.05, float(e[b - 1]) + 0.06]   # (bin b-1 holds three: not single)
                    if right:
                        v.append(_ulps(e[b + 1], u))
                    if earlier:
                        v.append(float(e[b - 4]) + 0.05)
                    v = np.array(v)
                    rng.shuffle(v)
                    hist = np.histogram(v, bins=e)[0]
                    assert hist[b] >= 40 and (not left or hist[b - 1] == 1) and (not right or hist[b + 1] == 1)   # (the construction)
                    lists.append(v)
    return lists


@pytest.mark.gpu
def test_road_diet_edge_ulps(gpu):
    _compare(gpu, _edge_ulp_lists())


def _heavy_lists():
    so = _oracle()
    e = so.BIN_EDGES
    rng = np.random.default_rng(7)
    b = 14
    lists = []
    for t in TIERS:
        n = 64 * t
        for side in (+1, -1):
            lone = float(e[b + side]) + 0.05
            for near_edge in (False, True):
                v = rng.uniform(e[b] + 0.001, e[b + 1] - 0.001, n)
                if near_edge:
                    # a tenth of the values within 2 ulps of the edge shared with the single bin, on bin b's side of it (edge(b)
                    # itself is bin b's and lies in the left single's interval (lo, edge(b)]: dropped)
                    idx = rng.choice(n, n // 10, replace=False)
                    k = rng.integers(1, 3, idx.size) if side > 0 else rng.integers(0, 3, idx.size)
                    v[idx] = [_ulps(e[b + 1], -int(j)) if side > 0 else _ulps(e[b], int(j)) for j in k]
                v[rng.integers(1, n)] = lone
                assert np.histogram(v, bins=e)[0][b + side] == 1
                lists.append(v)
    return lists


@pytest.mark.gpu
def test_road_diet_heavy_suspects(gpu):
    """Every value a suspect (one bin, a single next to it): no row of any lane is skipped, and none but the lone value is
    dropped — except the values ON the left single's upper edge."""
    so = _oracle()
    lists = _heavy_lists()
    n_plain = [len(y) - so.road_model(y, 0.5).n_kept for y in lists[0::2]]
    assert n_plain == [1] * len(n_plain)
    assert any(len(y) - so.road_model(y, 0.5).n_kept > 1 for y in lists[1::2])
    _compare(gpu, lists, want_cold=[])


@pytest.mark.gpu
def test_road_diet_group_boundaries(gpu):
    """Lengths around every row group's end; the list's last 70 values mix 0.0, 16.9, values outside [0, 16.9] and ordinary
    ones, so that the partial row and the group that holds it see data that is not binned."""
    rng = np.random.default_rng(11)
    lists = []
    for g in range(25):
        for d in (-1, 0, 1):
            n = 64 * g + d
            if not 1 <= n <= 1536:
                continue
            y = _ordinary(rng, n)
            m = min(n, 70)
            tail = rng.choice(np.array([0.0, 16.9, -0.3, 17.5, np.nan]), m, p=[0.15, 0.15, 0.15, 0.15, 0.4])
            y[n - m:] = np.where(np.isnan(tail), y[n - m:], tail)
            lists.append(y)
    _compare(gpu, lists)


def _band(so, y, thr=0.3):
    """(margin, bound) of the kernel's band test, from one-pass sums evaluated by NumPy (its own order: the last bits differ
    from the kernel's, which is why the caller accepts only decisions that are far from even)."""
    drop = so.single_bin_drop_mask(y, so.histogram_170(y))
    rm = so.road_model(y, 0.5)
    mode10 = (rm.mode_left + rm.mode_right) / 2 / 10.0
    N, n, sh = len(y), int((~drop).sum()), y[0]
    d = y - sh
    S1, S2, Q = d[~drop].sum(), (d[~drop] ** 2).sum(), (d ** 2).sum()
    m1 = S1 / n
    mean, var = sh + m1, S2 / n - m1 * m1
    with np.errstate(all="ignore"):
        sd = np.sqrt(var)
        g = 2.0 ** -52 * (2.0 * ((N + 63) // 64) + 64.0 + N / 8192.0)
        a2 = Q / n
        r, rho = np.sqrt(a2), np.sqrt(N / n)
        Mg = abs(sh) + r
        rms = np.sqrt(mean * mean + var)
        margin = abs((mean - mode10) - thr * sd)
        bound = (1e-11 * (rms + sd) + 1e-22 * rms * rms / sd
                 + g * ((Mg + rho * r) + abs(mode10) + (1.0 + thr) * sd + (1.0 + thr) * (a2 * (6.0 + 2.0 * rho) + g * Mg * Mg) / sd))
    return margin, bound


@pytest.mark.gpu
def test_road_diet_statistics_rounds(gpu):
    """Narrow clusters far from the shift: the band decides between the lean kernel's own statistics and the cold list.
    The full variant with the statistics output always sums in NumPy's order, so which lists it WOULD send there without
    is worked out here from the same formula; the cold list read back must hold exactly those."""
    so = _oracle()
    lists, want, s = [], [], 0
    for first, edge_bin in ((0.0, 165), (0.05, 120), (16.85, 5)):
        for w in (1e-8, 1e-6, 1e-3):
            for kappa in (-0.02, -0.002, 0.002, 0.02):
                y = _cluster_list(first, edge_bin, 1300, w, kappa, 3000 + s)
                margin, bound = _band(so, y)
                even = not (np.isnan(margin) or np.isnan(bound) or margin > 10.0 * bound or margin < 0.1 * bound)
                assert not even, (len(lists), margin, bound)                                   # (the construction)
                if not margin > bound:
                    want.append(len(lists))
                lists.append(y)
                s += 1
    assert 0 < len(want) < len(lists)
    _compare(gpu, lists, want_cold=want)


@pytest.mark.gpu
def test_road_diet_wide_and_list(gpu):
    """Beyond the register tier: 1 700 values (the lean kernel's cold list, the LIST pass) and 5 200 (a workgroup per
    frame), each with a single bin next to the mode bin and edge-ulp values behind the first 1 536 values."""
    so = _oracle()
    e = so.BIN_EDGES
    rng = np.random.default_rng(13)
    b = 14
    lists = []
    for n in (1700, 5200):
        for side in (+1, -1):
            y = np.clip(1.45 + 0.02 * rng.standard_normal(n), e[b] + 1e-6, e[b + 1] - 1e-6)     # the mode bin
            y[1::3] = _ordinary(rng, n)[1::3]
            y = np.where((y >= e[b + side]) & (y < e[b + side + 1]), 1.45, y)                     # (nothing else in the single's bin)
            y[5] = e[b + side] + 0.05                                                            # the lone value
            tail = np.arange(1600, n, 7)
            k = rng.integers(0, 4, tail.size)
            y[tail] = [_ulps(e[b + 1], -1 - int(j)) if side > 0 else _ulps(e[b], int(j)) for j in k]
            assert np.histogram(y, bins=e)[0][b + side] == 1
            lists.append(y)
    _compare(gpu, lists[:2], want_cold=[0, 1])
    _compare(gpu, lists[2:])


@pytest.mark.gpu
def test_road_diet_fused(gpu):
    """The fused HOT path: three control frames and one whose road model is the median (cold list), frame by frame."""
    so = _oracle()
    controls = [c for c in sc.control_cases(count=8) if sc.control_ok(c)][:3]
    cases = controls[:2] + [_median_case(), controls[2]]
    pf, res = sc.run_scale(gpu, cases, kind="hot")
    _, cold = _lists_of(gpu, len(cases))
    assert list(cold) == [2]
    _, res2 = sc.run_scale(gpu, cases, kind="hot")
    for k in ("status", "raw_scale", "height", "height_level", "counts"):
        assert np.array_equal(res[k], res2[k], equal_nan=True), k
    for f, c in enumerate(cases):
        _assert_frame_equal(so, c.oracle(), res, pf, f, check_stage=False)
