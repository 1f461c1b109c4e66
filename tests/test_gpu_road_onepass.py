"""The road-model kernel's one-pass statistics (shifted sums, dropped values subtracted) against the oracle: lists built to
sit inside or at the edge of the guard band that sends a list to NumPy's exact order, lengths across the 64-value rows
and the register tiers, suspect-heavy lists, and run-to-run identity."""
import numpy as np
import pytest

from gpu_helpers import _oracle


def _cluster_list(first, edge_bin, n, w, kappa, seed):
    """`first`, then n-1 values in a cluster of width ~w around the bin edge edge_bin*0.1: more of them just below the edge
    than above, so the bin below is the single mode and mode/10 IS the edge; skew = (mean - edge)/std ~ 0.3 + kappa."""
    rng = np.random.default_rng(seed)
    edge = edge_bin * 0.1
    n1 = (n - 1) // 2 + 3
    a = rng.uniform(0.1, 1.0, n1)
    u = rng.uniform(0.1, 1.0, n - 1 - n1)
    lo, hi = 0.0, 100.0
    for _ in range(200):                                                # scale of the upper part for the skew asked for
        c = 0.5 * (lo + hi)
        z = np.concatenate([-a, c * u])
        if z.mean() / z.std() < 0.3 + kappa:
            lo = c
        else:
            hi = c
    z = np.concatenate([-a, lo * u])
    rng.shuffle(z)
    return np.concatenate([[first], edge + w * z])


def _near_threshold_list(so, edge_bin, n, seed):
    """A cluster of width 0.03 whose skew (NumPy's, through the oracle) is moved as close to 0.3 as one value's
    neighbouring doubles allow."""
    y = _cluster_list(0.0, edge_bin, n + 1, 0.03, 0.0, seed)[1:]
    best = None
    for k in range(-300, 301):
        z = y.copy()
        z[0] = y[0] + k * np.spacing(y[0])
        sk = so.road_model(z, 0.5).skew
        if best is None or abs(sk - 0.3) < abs(best[0] - 0.3):
            best = (sk, z)
    return best[1]


def _lists():
    rng = np.random.default_rng(20261016)
    out = []
    out.append(np.full(42, 0.3))                                         # NumPy: mean 0.30000000000000004, std 5.6e-17
    for v in (0.05, 1.0, 1.55, 7.3, 16.85):
        out.append(np.full(300, v))                                      # constant
        out.append(v + 1e-13 * rng.standard_normal(700))                 # nearly constant
    # the shift (first value) far from the mean: values at both ends of [0, 16.9]
    for first, body in ((0.0, 16.5), (16.9, 0.4), (16.89, 1.25)):
        y = body + 0.05 * rng.standard_normal(900)
        y[0] = first
        out.append(np.clip(y, 0.0, 16.9))
    # skew within ~1e-13 of 0.3 (inside both bands: decided in NumPy's order)
    so = _oracle()
    for eb, n, seed in ((165, 1000, 1), (120, 1000, 2), (33, 700, 3), (14, 300, 4)):
        out.append(_near_threshold_list(so, eb, n, seed))
    # lengths across the row boundaries and the register tiers (and beyond the deepest one)
    for n in (1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281,
              1535, 1536, 1537, 2047, 3000, 5000):
        out.append(np.clip(1.4 + 0.3 * rng.standard_normal(n), 0.0, 16.9))
    # suspect-heavy: many count-1 bins (a value alone in its bin, its neighbours full)
    for n in (200, 600, 1300):
        y = np.clip(2.0 + 0.2 * rng.standard_normal(n), 0.0, 16.9)
        y[: n // 10] = 0.1 * rng.integers(0, 169, n // 10) + 0.05 + 1e-3 * rng.standard_normal(n // 10)
        out.append(np.clip(y, 0.0, 16.9))
        z = (np.arange(n) % 169) * 0.1                                   # values ON the bin edges, one or more per bin
        z[::7] += 0.1 - 2.0 ** -50
        out.append(np.clip(z, 0.0, 16.9))
    return out


def _run(gpu, lists, hl, stats):
    from mvoscalerecovery_amd import packing
    from mvoscalerecovery_amd.engine import DeviceBatch, DeviceOutputs, ScaleEngine
    F = len(lists)
    cnt = np.array([len(y) for y in lists], dtype=np.int32)
    padded = (cnt.astype(np.int64) + 1) & ~np.int64(1)
    off = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    y = np.zeros(int(padded.sum()), dtype=np.float64)
    for i, v in enumerate(lists):
        y[off[i]:off[i] + cnt[i]] = v
    pf = packing.PackedFrames(F, off, cnt, y.copy(), y, y.copy(), y.copy(), y.copy(), [None] * F, max_feat=int(cnt.max()))
    eng = ScaleEngine(1.75, ctx=gpu)
    db = DeviceBatch(gpu, pf, with_tri2=False)
    out = DeviceOutputs(gpu, db, counts=True, hist=stats)
    eng.road_model_batch(db, out, hl)
    res = {k: out.get(k) for k in out.bufs}
    out.free()
    db.free()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [False, True])
def test_road_onepass_against_oracle(gpu, stats):
    so = _oracle()
    lists = _lists()
    hl = 0.5 + 0.001 * np.arange(len(lists))
    res = _run(gpu, lists, hl, stats)
    res2 = _run(gpu, lists, hl, stats)
    for k in ("status", "height", "counts"):
        assert np.array_equal(res[k], res2[k], equal_nan=True), k                 # run-to-run identity
    st, h, counts = res["status"], res["height"], res["counts"]
    for i, y in enumerate(lists):
        rm = so.road_model(np.asarray(y, dtype=np.float64), hl[i])
        assert st[i] == rm.status, (i, len(y), st[i], rm.status)
        assert counts[i, 4] == rm.n_kept and counts[i, 5] == rm.n_modes, (i, counts[i], rm.n_kept, rm.n_modes)
        if rm.status in (so.ST_MODE, so.ST_RIGHT, so.ST_MEDIAN, so.ST_LEVEL):
            assert h[i] == rm.height, (i, len(y), h[i], rm.height)
        if stats and rm.status in (so.ST_MODE, so.ST_RIGHT):
            assert np.array_equal(res["stats"][i, :3], [rm.mean, rm.std, rm.skew], equal_nan=True), i


@pytest.mark.gpu
def test_road_onepass_wide(gpu):
    """Lists beyond four wavefronts' register tiers take the wide variant (a workgroup per frame)."""
    so = _oracle()
    rng = np.random.default_rng(7)
    lists = [np.clip(1.4 + 0.3 * rng.standard_normal(n), 0.0, 16.9) for n in (5200, 6000, 9000)]
    lists.append(np.full(6000, 0.3))
    hl = np.full(len(lists), 0.7)
    res = _run(gpu, lists, hl, False)
    for i, y in enumerate(lists):
        rm = so.road_model(y, hl[i])
        assert res["status"][i] == rm.status and res["height"][i] == rm.height, (i, res["status"][i], rm.status)
        assert res["counts"][i, 4] == rm.n_kept, i


@pytest.mark.gpu
def test_road_onepass_band_edge(gpu):
    """Lists where the one-pass sums are least accurate, decided WITHOUT the statistics output (the fast decision): the
    shift is a dropped single at one end of [0, 16.9], the kept values a cluster of width 1e-8 .. 1e-4 around a bin edge
    at the other end, skew 0.3 +- 0.002 / 0.02.  (y - sh)^2 ~ 270 against a variance down to 1e-17: the one-pass variance
    is rounding noise, and the earlier two-pass band alone lets some of these lists through to the fast path with the
    wrong side of 0.3; the one-pass term of the band sends them to NumPy's order."""
    so = _oracle()
    lists, s = [], 0
    for first, edge_bin in ((0.0, 165), (0.05, 120), (16.85, 5)):
        for n in (300, 1300):
            for w in (1e-8, 3e-8, 1e-7, 3e-7, 1e-6, 1e-5, 1e-4):
                for kappa in (-0.02, -0.002, 0.002, 0.02):
                    lists.append(_cluster_list(first, edge_bin, n, w, kappa, 1000 + s))
                    s += 1
    hl = np.full(len(lists), 0.5)
    res = _run(gpu, lists, hl, False)
    n_right = 0
    for i, y in enumerate(lists):
        rm = so.road_model(y, hl[i])
        assert rm.status in (so.ST_MODE, so.ST_RIGHT) and abs(rm.skew - 0.3) < 0.03, (i, rm.status, rm.skew)    # (the construction)
        assert res["status"][i] == rm.status and res["height"][i] == rm.height, (i, len(y), res["status"][i], rm.status, rm.skew)
        assert res["counts"][i, 4] == rm.n_kept == len(y) - 1, i
        n_right += rm.status == so.ST_RIGHT
    assert 0 < n_right < len(lists)
