"""The road model's lean (HOT) variant and its cold list.  Without the statistics / histogram outputs `road_model_batch`
runs the lean kernel, which leaves a frame that needs the packed list (median, NumPy-order sums) or is longer than its
deepest register tier on the cold list; the full LIST pass behind it finishes those.  Every case is compared with the
oracle with `==` and run twice; the cold list itself is read back from the context's workspace."""
import ctypes as C

import numpy as np
import pytest

import scale_cases as sc
from gpu_helpers import _assert_frame_equal, _oracle
from test_gpu_road_onepass import _cluster_list, _run

RC_HOT = 24                                    # kRoadRCHot: rows of 64 values in the lean variant's deepest tier
TIERS = (4, 8, 12, 16, 20, RC_HOT)             # its tiers


class _CtxHead(C.Structure):
    """The head of `struct mvosr_ctx` (csrc/mvosr_host.hpp) up to the int workspace."""
    _fields_ = [("device", C.c_int), ("own_stream", C.c_void_p), ("stream", C.c_void_p), ("n_cu", C.c_int),
                ("max_lds_per_block", C.c_int), ("name", C.c_char * 128), ("ws_ysel", C.c_void_p), ("ws_ysel_len", C.c_size_t),
                ("ws_nsel", C.c_void_p), ("ws_nsel_len", C.c_size_t)]


def _lists_of(ctx, n_frames):
    """(redo list, cold list) of the last call on a batch of n_frames: the workspace's int block is nsel [F], the redo
    list [1 + F], the cold list [1 + F]; [0] = count."""
    ctx.sync()
    head = _CtxHead.from_address(ctx.handle.value)
    assert head.n_cu == ctx.n_cu and head.ws_nsel and head.ws_nsel_len >= n_frames         # (the mirror fits the struct)
    words = np.empty(2 * (n_frames + 1), dtype=np.int32)
    rc = ctx.lib.mvosr_memcpy_d2h(ctx.handle, C.c_void_p(words.ctypes.data), C.c_void_p(head.ws_nsel + 4 * n_frames), C.c_size_t(words.nbytes))
    assert rc == 0
    redo, cold = words[:n_frames + 1], words[n_frames + 1:]
    assert 0 <= cold[0] <= n_frames
    return redo[1:1 + redo[0]].copy(), cold[1:1 + cold[0]].copy()


def _ordinary(rng, n):
    return np.clip(1.4 + 0.3 * rng.standard_normal(n), 0.0, 16.9)


def _cold_lists(rng):
    """Lists the lean variant cannot finish: constant ones (the one-pass std is exactly 0, the band not a number: NumPy's
    order), lists without modes (no bin above 2: the median of the kept values), lists beyond the deepest tier."""
    out = [np.full(300, 7.3), np.full(700, 1.55), np.full(42, 0.3)]
    out += [np.array([2.05, 2.07]), np.repeat(0.1 * np.arange(5, 60) + 0.05, 2), np.array([0.31, 0.32, 5.01, 5.02, 9.0])]
    out += [_ordinary(rng, n) for n in (RC_HOT * 64 + 1, 1700, 3000)]
    return out


def _hot_lists(rng):
    """Lists it finishes: ordinary ones up to the deepest tier, an empty one (NO_FLAT), one whose values are all lone (LEVEL),
    and a nearly constant one in the middle of its bin (mean - mode/10 = 0.05 against a band of 1e-22 * rms^2 / std = 2e-9)."""
    return ([_ordinary(rng, n) for n in (63, 200, 700, 1100, RC_HOT * 64)] + [np.zeros(0), np.array([0.05, 0.35, 0.65])] +
            [1.55 + 1e-13 * rng.standard_normal(700)])


def _check(gpu, lists, n_cold=None):
    so = _oracle()
    F = len(lists)
    hl = 0.5 + 0.001 * np.arange(F)
    res = _run(gpu, lists, hl, False)
    _, cold = _lists_of(gpu, F)
    res2 = _run(gpu, lists, hl, False)
    _, cold2 = _lists_of(gpu, F)
    for k in ("status", "height", "raw_scale", "counts"):
        assert np.array_equal(res[k], res2[k], equal_nan=True), k
    assert sorted(cold) == sorted(cold2) and len(set(cold)) == len(cold)
    for i, y in enumerate(lists):
        if len(y) == 0:
            # an empty selection never reaches the oracle's road_model: frame_raw_scale answers ref / level (:277-279, :420-422)
            assert res["status"][i] == so.ST_NO_FLAT and np.isnan(res["height"][i]) and res["raw_scale"][i] == 1.75 / hl[i], i
            continue
        rm = so.road_model(np.asarray(y, dtype=np.float64), hl[i])
        assert res["status"][i] == rm.status, (i, len(y), res["status"][i], rm.status)
        assert res["counts"][i, 4] == rm.n_kept and res["counts"][i, 5] == rm.n_modes, (i, res["counts"][i], rm.n_kept, rm.n_modes)
        if rm.status in (so.ST_MODE, so.ST_RIGHT, so.ST_MEDIAN, so.ST_LEVEL):
            assert res["height"][i] == rm.height, (i, len(y), res["height"][i], rm.height)
        else:
            assert np.isnan(res["height"][i]), i
    if n_cold is not None:
        assert len(cold) == n_cold, (sorted(cold), n_cold)
    return set(int(f) for f in cold)


@pytest.mark.gpu
def test_road_hot_all_cold(gpu):
    lists = _cold_lists(np.random.default_rng(1))
    assert _check(gpu, lists, n_cold=len(lists)) == set(range(len(lists)))


@pytest.mark.gpu
def test_road_hot_none_cold(gpu):
    _check(gpu, _hot_lists(np.random.default_rng(2)), n_cold=0)


@pytest.mark.gpu
def test_road_hot_mixed_shuffled(gpu):
    rng = np.random.default_rng(3)
    cold, hot = _cold_lists(rng), _hot_lists(rng)
    tagged = [(y, True) for y in cold] + [(y, False) for y in hot]
    order = rng.permutation(len(tagged))
    lists = [tagged[i][0] for i in order]
    want = set(k for k, i in enumerate(order) if tagged[i][1])
    assert _check(gpu, lists, n_cold=len(cold)) == want


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames", [1, 3, 4, 5, 257])
def test_road_hot_batch_sizes(gpu, n_frames):
    """A workgroup holds four frames and the LIST pass strides over 256 of them: batches around both, empty lists among them."""
    rng = np.random.default_rng(100 + n_frames)
    pool = [(y, True) for y in _cold_lists(rng)[:6]] + [(y, False) for y in _hot_lists(rng)[:3] + [np.zeros(0)]]
    picks = [pool[(3 * i + n_frames) % len(pool)] for i in range(n_frames)]
    if n_frames >= 3:
        picks[1] = (np.zeros(0), False)
    _check(gpu, [y for y, _ in picks], n_cold=sum(c for _, c in picks))
    if n_frames == 257:
        _check(gpu, [pool[i % 6][0] for i in range(n_frames)], n_cold=n_frames)   # every frame on the list, beyond one stride


@pytest.mark.gpu
def test_road_hot_tier_boundaries(gpu):
    rng = np.random.default_rng(4)
    lengths = [64 * t + d for t in TIERS for d in (-1, 0, 1)]
    lists = [_ordinary(rng, n) for n in lengths]
    cold = _check(gpu, lists, n_cold=1)
    assert cold == {lengths.index(RC_HOT * 64 + 1)}


@pytest.mark.gpu
def test_road_hot_band_boundary(gpu):
    """test_road_onepass_band_edge's lists, narrow clusters (inside the band: cold) next to wide ones (outside: decided by
    the lean variant).  The band's leading term is g * (1 + thr) * 8 * a2 / std with g = 2^-52 * (2 * 21 + 64) = 2.4e-14 and
    a2 = mean (y - shift)^2 = 140 .. 270, about 5e-11 / std; the margin is |skew - 0.3| * std, and std is about half the
    width.  Width 1e-8: the band is 1e-2, the margin at most 1e-10 (cold).  Width 1e-3 with |skew - 0.3| = 0.02: the band
    is 1e-7, the margin 1e-5 (hot)."""
    lists, wide, s = [], [], 0
    for first, edge_bin in ((0.0, 165), (0.05, 120), (16.85, 5)):
        for w in (1e-8, 1e-6, 1e-3):
            for kappa in (-0.02, -0.002, 0.002, 0.02):
                lists.append(_cluster_list(first, edge_bin, 1300, w, kappa, 2000 + s))
                wide.append(w == 1e-3 and abs(kappa) == 0.02)
                s += 1
    cold = _check(gpu, lists)
    assert 0 < len(cold) < len(lists)
    for i, w in enumerate(lists):
        if wide[i]:
            assert i not in cold, i
    assert all(i in cold for i in range(len(lists)) if i % 12 < 4)            # the 1e-8 clusters


def _median_case():
    """lone_bins_case with two of the wide triangle's y' in one bin: remove_single drops the third, two values are kept, no
    bin is above 2 — the median (ST_MEDIAN), which the lean variant leaves to the cold list."""
    tris = [sc.wall_tri(2.0 + k, sc.LEVEL) for k in range(4)]
    tris.append(np.array([[-6.0, 2.05, 8.0], [6.0, 2.07, 9.0], [0.5, 2.65, 20.0]]))
    return sc.tri_frame("median", np.array(tris), family="median")


@pytest.mark.gpu
def test_road_hot_fused(gpu):
    """scale_batch in HOT mode: one batch with a frame that ends on the fallback level (redo list), one whose road model
    is cold (cold list) and ordinary ones; each equals the oracle, and the batch equals its frames run one by one."""
    so = _oracle()
    controls = [c for c in sc.control_cases(count=8) if sc.control_ok(c)][:3]
    level, median = sc.lone_bins_case(), _median_case()
    assert level.oracle().status == so.ST_LEVEL and median.oracle().status == so.ST_MEDIAN        # (the construction)
    cases = [controls[0], level, controls[1], median, controls[2]]
    pf, res = sc.run_scale(gpu, cases, kind="hot")
    redo, cold = _lists_of(gpu, len(cases))
    assert 1 in redo and 3 not in redo and list(cold) == [3]       # (the HOT scale kernel may list ordinary frames of its own)
    _, res2 = sc.run_scale(gpu, cases, kind="hot")
    keys = ("status", "raw_scale", "height", "height_level", "counts")
    for k in keys:
        assert np.array_equal(res[k], res2[k], equal_nan=True), k
    for f, c in enumerate(cases):
        _assert_frame_equal(so, c.oracle(), res, pf, f, check_stage=False)
        _, one = sc.run_scale(gpu, [c], kind="hot")
        for k in ("status", "raw_scale", "height"):           # (height_level: the product mode's sum depends on the batch's variant)
            assert np.array_equal(one[k][0], res[k][f], equal_nan=True), (c.name, k)
        assert np.array_equal(one["counts"][0, 3:6], res["counts"][f, 3:6]), c.name            # selected, kept, modes
