"""The batch-header contract on hand-built buffers: mvosr_batch.max_feat (and max_tri / max_pts) size a launch's LDS while the
per-frame counts live in device memory, so a C-ABI caller can state a header smaller than a frame.  Every per-frame kernel must
refuse such a frame before it touches LDS, with the outputs include/mvosr.h states, and leave the frames around it alone.

Per entry point, with the offending frame in the middle of three to five small frames, larger than the header by one and, in a
second case, by a lot:
  1. the offending frame has exactly the refusal outputs of mvosr.h;
  2. every other frame is bit-identical to the same frame launched alone under a true header, and equals its CPU reference;
  3. nothing outside the frames' slices was written: the outputs are pre-filled with a sentinel byte and end in a guard element.
A kernel without its guard does not stop at the offending frame: it processes it (past the end of its LDS), so the frame's status
is 0 where MVOSR_ST_ERR_MASK is asserted, its tallies / counters / level are the computed ones where zero / -1 / NaN are asserted,
and its per-triangle rows are written where the sentinel is asserted; a stage launcher that did not hand max_tri to the kernel
would refuse every frame, neighbours included; a graph vote without the row bound returns status 0 and a centre tally of
3 * 21846 mod 2^16 = 2 for the fan just outside the bound.  Each guard is therefore pinned by the assertions on the refused frame.
Integer tallies and status words are compared exactly.  (The flat selection's heights are the one continuous quantity: they go
through tests/flat_cases.py's references and the bound derived there, as in tests/test_gpu_flat_select.py.)"""
import ctypes as C

import numpy as np
import pytest

import flat_cases as fc

pytestmark = pytest.mark.gpu
SENT = 0x5A
ST_MASK = fc.ST_MASK
GRAPH_MAX_ROWS = 21845                      # MVOSR_GRAPH_MAX_ROWS: 3 * 21845 = 65535, the largest 16-bit tally


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_dict(a, b):
    return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)


def _guards_intact(tails):
    return all(len(np.ravel(t)) >= 1 and fc.all_bytes(t, SENT) for t in tails.values())


def _headers(sizes, mid):
    """(header larger-by-one, header smaller by a lot): the offending frame's size - 1, and the largest of the others."""
    others = max(s for i, s in enumerate(sizes) if i != mid)
    assert sizes[mid] - 1 >= others and sizes[mid] - others >= 20
    return sizes[mid] - 1, others


# ---- the graph vote -------------------------------------------------------------------------------------------------------------
def _graph_case(name, n, seed):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0, 100, (n, 2))
    return {"name": name, "v": uv[:, 1].copy(), "z": rng.uniform(1, 50, n), "tri": Delaunay(uv).simplices.astype(np.int32), "declined": False}


def _fan_case(name, rows, n_ring=120, centre_times=1, seed=7):
    """A fan: the centre vertex 0 is in every row (`centre_times` times: a row may name a vertex up to three times), the ring
    vertices go round as often as the row count asks."""
    rng = np.random.default_rng(seed)
    i = np.arange(rows)
    a, b = 1 + i % n_ring, 1 + (i + 1) % n_ring
    tri = np.stack([np.zeros(rows, np.int64), a if centre_times < 2 else np.zeros(rows, np.int64), b if centre_times < 3 else np.zeros(rows, np.int64)], 1)
    return {"name": name, "v": rng.uniform(0, 100, n_ring + 1), "z": rng.uniform(1, 50, n_ring + 1), "tri": tri.astype(np.int32), "declined": False}


def _check_graph_frame(c, g, min_valid=10):
    from oracle import rescale_oracle as ro
    valid, good, total = ro.graph_inliers(c["v"], c["z"], c["tri"])
    assert np.array_equal(g["total"], total) and np.array_equal(g["good"], good), c["name"]
    nv = int(valid.sum())
    assert g["n_valid"] == nv and np.array_equal(g["keep"], np.where(valid, 1, -1 if nv > min_valid else 0)), c["name"]
    assert g["status"] == 0 and g["status_inliers"] == 0, c["name"]
    return total


def _check_graph_refused(c, g):
    n = len(c["v"])
    assert g["status"] == ST_MASK and g["status_inliers"] == ST_MASK, c["name"]
    assert _same(g["total"], np.zeros(n, np.int32)) and _same(g["good"], np.zeros(n, np.int32)), c["name"]       # stage form
    assert _same(g["keep"], np.full(n, -1, np.int32)) and g["n_valid"] == 0, c["name"]                            # keep form


def test_graph_vote_frame_larger_than_the_header(gpu):
    """mvosr_graph_inliers_batch and mvosr_graph_keep_batch: total / good zero, keep -1, n_valid 0, MVOSR_ST_ERR_MASK."""
    sizes, mid = (61, 54, 127, 23, 70), 2
    cases = [_graph_case("g%d" % i, n, 300 + i) for i, n in enumerate(sizes)]
    solo = [fc.run_graph(gpu, [c], sentinel=SENT) for c in cases]
    for header in _headers(sizes, mid):
        got, tails = fc.run_graph(gpu, cases, max_feat=header, sentinel=SENT)
        assert _guards_intact(tails), header
        for i, c in enumerate(cases):
            if i == mid:
                _check_graph_refused(c, got[i])
                continue
            assert _same_dict(got[i], solo[i][0][0]) and _guards_intact(solo[i][1]), (header, c["name"])
            _check_graph_frame(c, got[i])
    _check_graph_frame(cases[mid], solo[mid][0][0])                  # (the offending frame is an ordinary one under a true header)


def test_graph_vote_tally_range(gpu):
    """The two 16-bit tallies of a vertex: with MVOSR_GRAPH_MAX_ROWS rows they hold the oracle's values — 21845 for a fan's
    centre, 65535 (every bit of the field) for a vertex named three times by every row — and with one row more the frame is
    refused instead of carrying `total` into `good`.  Between two ordinary frames, which are untouched."""
    small = [_graph_case("left", 40, 311), _graph_case("right", 33, 312)]
    solo = [fc.run_graph(gpu, [c], sentinel=SENT)[0][0] for c in small]
    for times in (1, 3):
        inside = _fan_case("fan_inside_x%d" % times, GRAPH_MAX_ROWS, centre_times=times)
        outside = _fan_case("fan_outside_x%d" % times, GRAPH_MAX_ROWS + 1, centre_times=times)
        for fan, refused in ((inside, False), (outside, True)):
            cases = [small[0], fan, small[1]]
            got, tails = fc.run_graph(gpu, cases, sentinel=SENT)
            assert _guards_intact(tails), fan["name"]
            if refused:
                _check_graph_refused(fan, got[1])
            else:
                total = _check_graph_frame(fan, got[1])
                assert total[0] == times * GRAPH_MAX_ROWS and (times < 3 or total[0] == 0xFFFF)
            for i, j in ((0, 0), (2, 1)):
                assert _same_dict(got[i], solo[j]), (fan["name"], i)
                _check_graph_frame(small[j], got[i])


def test_graph_vote_frame_beyond_one_trip_of_the_block(gpu):
    """More than 512 features and more than 512 rows: the strided loops of the 512-thread block run more than once."""
    c = _graph_case("wide", 700, 320)
    assert len(c["v"]) > 512 and len(c["tri"]) > 512
    got, tails = fc.run_graph(gpu, [_graph_case("l", 30, 321), c, _graph_case("r", 45, 322)], sentinel=SENT)
    assert _guards_intact(tails)
    total = _check_graph_frame(c, got[1])
    assert total.sum() == 3 * len(c["tri"])


# ---- flat_selection, both forms -------------------------------------------------------------------------------------------------
def _flat_frame(name, n_tri, seed, reps=1):
    """n_tri flat triangles with three vertices of their own (3 n_tri features), loose, tight and steep ones, each row `reps` times."""
    rng = np.random.default_rng(seed)
    specs = [(float(rng.uniform(1.5, 1.9)), (0.0, 0.0, 0.0, 7.0, 20.0)[i % 5], reps) for i in range(n_tri)]
    return fc.disjoint(name, specs, seed, near=True)


def _check_flat_frame(f, o, dev):
    """Heights and flag bits against the 60-digit rows (flat_cases' bound), the discrete part exactly from the kernel's own heights."""
    h, pitch, kappa = fc.mp_rows(f)
    bits, dec0, dec1 = fc.flag_reference(pitch, kappa)
    rel = np.abs(o["tri_height"].astype(np.longdouble) - h) / np.abs(h)
    assert np.all(rel <= fc.height_bound(kappa)), f.name
    assert np.array_equal((o["tri_flags"] & 1)[dec0], (bits & 1)[dec0]) and np.array_equal((o["tri_flags"] & 2)[dec1], (bits & 2)[dec1]), f.name
    level, kept = fc.expected_discrete(o["tri_height"], o["tri_flags"], 0.9)
    assert _same(np.float64(o["height_level"]), np.float64(level)) and np.array_equal((o["tri_flags"] & 4) != 0, kept), f.name
    assert o["n_kept"] == int(kept.sum()) and o["status"] in ((0, fc.ST_RS_FEW) if dev else (0,)), (f.name, o["status"])


def _check_flat_refused(f, o, dev):
    assert o["status"] == ST_MASK and np.isnan(o["height_level"]) and o["n_kept"] == 0, (f.name, o["status"])
    assert fc.all_bytes(o["tri_height"], SENT) and fc.all_bytes(o["tri_flags"], SENT), f.name      # per-triangle outputs: not written
    if dev:
        assert np.isnan(o["raw_scale"]) and np.isnan(o["model"]).all() and o["best_ic"] == 0 and o["used"] == 0, f.name
        assert fc.all_bytes(o["hyp_counts"], SENT), f.name


def _flat_contract(gpu, frames, mid, dev, headers):
    """headers: (max_feat, max_tri) overrides, None for the true value."""
    ids = [40 + i for i in range(len(frames))]
    if dev:
        run = lambda fr, fid, **kw: fc.run_dev(gpu, fr, use_keep=True, frame_ids=fid, sentinel=SENT, **kw)
    else:
        run = lambda fr, fid, **kw: fc.run_stage(gpu, fr, sentinel=SENT, **kw)
    solo = [run([f], [ids[i]]) for i, f in enumerate(frames)]
    for max_feat, max_tri in headers:
        got, tails = run(frames, ids, max_feat=max_feat, max_tri=max_tri)
        assert _guards_intact(tails), (max_feat, max_tri)
        for i, f in enumerate(frames):
            if i == mid:
                _check_flat_refused(f, got[i], dev)
                continue
            assert _same_dict(got[i], solo[i][0][0]) and _guards_intact(solo[i][1]), (max_feat, max_tri, f.name)
            _check_flat_frame(f, got[i], dev)
    _check_flat_frame(frames[mid], solo[mid][0][0], dev)


def _feature_frames(dev):
    sizes, mid = (54, 126, 75, 21), 1
    frames = [_flat_frame("hc_feat_%d_%d" % (dev, i), n // 3, 400 + i) for i, n in enumerate(sizes)]
    if dev:                                                          # (the header counts the features BEFORE keep)
        frames = [f.with_keep(410 + i, 6, mode="mixed") for i, f in enumerate(frames)]
        sizes = tuple(n + 6 for n in sizes)
    assert tuple(len(f.xyz) for f in frames) == sizes
    return frames, mid, [(h, None) for h in _headers(sizes, mid)]


def _row_frames(dev):
    """The offending frame has no more features than its neighbours but every row three times: rows against max_tri."""
    frames = [_flat_frame("hc_rows_%d_0" % dev, 25, 420), _flat_frame("hc_rows_%d_1" % dev, 20, 421, reps=3), _flat_frame("hc_rows_%d_2" % dev, 31, 422)]
    rows = tuple(len(f.tri) for f in frames)
    assert rows == (25, 60, 31) and max(len(f.xyz) for f in frames) == 93
    return frames, 1, [(None, h) for h in _headers(rows, 1)]


def test_flat_selection_features_against_the_header(gpu):
    frames, mid, headers = _feature_frames(False)
    _flat_contract(gpu, frames, mid, False, headers)


def test_flat_selection_rows_against_max_tri(gpu):
    """The stage form's launcher hands max_tri to the kernel: 9 max_tri bytes of LDS hold the heights and flags."""
    frames, mid, headers = _row_frames(False)
    _flat_contract(gpu, frames, mid, False, headers)


def test_flat_ransac_features_against_the_header(gpu):
    frames, mid, headers = _feature_frames(True)
    _flat_contract(gpu, frames, mid, True, headers)


def test_flat_ransac_rows_against_max_tri(gpu):
    frames, mid, headers = _row_frames(True)
    _flat_contract(gpu, frames, mid, True, headers)


# ---- the outlier vote alone -----------------------------------------------------------------------------------------------------
def _vote_sets(sizes, seed):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    sets = []
    for n in sizes:
        uv = rng.uniform(0, 1, (n, 2)) * [1241.0, 376.0]
        sets.append({"uv": uv, "z": rng.uniform(2.0, 60.0, n), "tri": Delaunay(uv).simplices.astype(np.int32)})
    return sets


def _run_vote(gpu, sets, max_feat=None):
    """mvosr_outlier_vote_batch over the engine's packed batch with outputs of this test's own: status, counts and vote_counters,
    pre-filled with SENT and one guard element longer.  -> (pf, status, counts, counters) with the guards still attached."""
    from mvoscalerecovery_amd import _lib, packing
    from mvoscalerecovery_amd.engine import DeviceBatch, ScaleEngine
    f3s = [np.stack([np.zeros(len(s["z"])), np.zeros(len(s["z"])), s["z"]], axis=1) for s in sets]
    pf = packing.pack_features(f3s, [s["uv"] for s in sets], vanish=-1.0)
    packing.attach_tri1(pf, [s["tri"] for s in sets])
    eng = ScaleEngine(1.75, ctx=gpu, camera_pitch=0.0)
    db = DeviceBatch(gpu, pf, with_tri2=False)
    st = db.struct()
    if max_feat is not None:
        st.max_feat = int(max_feat)
        for k in range(4):
            st.size_hint[k] = 0
    F, N = pf.n_frames, pf.total_padded
    bufs = [gpu.empty(F + 1, np.int32).fill(SENT), gpu.empty((F + 1, _lib.N_COUNTS), np.int32).fill(SENT), gpu.empty(N + 1, np.int32).fill(SENT)]
    o = _lib.Outputs(None, None, None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, None, None, None, None, None)
    _lib.check(gpu.lib.mvosr_outlier_vote_batch(gpu.handle, C.byref(eng.params), C.byref(st), C.byref(o), 0), "mvosr_outlier_vote_batch")
    gpu.sync()
    res = [b.download() for b in bufs]
    for b in bufs:
        b.free()
    db.free()
    return pf, res[0], res[1], res[2]


def _vote_contract(gpu, sets, mid, headers):
    from mvoscalerecovery_amd import constants as K
    from oracle import scale_oracle as so
    want = [so.outlier_votes(s["uv"][:, 1], s["z"], s["tri"]) for s in sets]
    solo = []
    for i, s in enumerate(sets):
        if i != mid:
            pf1, st1, cn1, vc1 = _run_vote(gpu, [s])
            solo.append((st1[0], cn1[0], vc1[pf1.frame_slice(0)]))
        else:
            solo.append(None)
    for header in headers:
        pf, status, counts, counters = _run_vote(gpu, sets, max_feat=header)
        written = np.zeros(len(counters), bool)
        for i, s in enumerate(sets):
            sl = pf.frame_slice(i)
            written[sl] = True
            if i == mid:
                assert status[i] == ST_MASK and counts[i, K.CNT_VALID] == 0, header
                assert _same(counters[sl], np.full(len(s["z"]), -1, np.int32)), header       # nobody survives: no stale word reads as a survivor
                continue
            assert status[i] == solo[i][0] == 0, (header, i)
            assert _same(counts[i], solo[i][1]) and _same(counters[sl], solo[i][2]), (header, i)
            assert np.array_equal(counters[sl], want[i]) and counts[i, K.CNT_VALID] == int((want[i] >= 0).sum()), (header, i)
        # nothing else: the padding between the frames, the guard elements, the counts the vote does not form
        assert fc.all_bytes(counters[~written], SENT) and fc.all_bytes(status[-1:], SENT) and fc.all_bytes(counts[-1], SENT), header
        other = [k for k in range(counts.shape[1]) if k != K.CNT_VALID]
        assert fc.all_bytes(counts[:-1, other], SENT), header


def test_outlier_vote_lds_variant_frame_larger_than_the_header(gpu):
    sizes, mid = (57, 33, 129, 80), 2
    assert max(sizes) <= int(gpu.lib.mvosr_max_lds_features())
    _vote_contract(gpu, _vote_sets(sizes, 500), mid, _headers(sizes, mid))


def test_outlier_vote_dense_variant_frame_larger_than_the_header(gpu):
    """The dense kernel runs where the HEADER is beyond the LDS-resident variant's capacity: the header is that capacity + 1 and,
    in the second case, + 40; the offending frame has one feature more than the larger of the two, its neighbours are small."""
    cap = int(gpu.lib.mvosr_max_lds_features())
    sizes, mid = (64, cap + 42, 101), 1
    _vote_contract(gpu, _vote_sets(sizes, 510), mid, (cap + 41, cap + 1))


# ---- the device triangulations --------------------------------------------------------------------------------------------------
def _run_delaunay(gpu, sets, qhull, max_pts=None):
    """-> (rows per frame as far as tri_cnt says, the frame's whole row slice, tri_cnt, status, guards intact)"""
    from mvoscalerecovery_amd import _lib
    cnt = np.array([len(s) for s in sets], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    uv = np.concatenate(sets)
    F, T = len(sets), int(2 * cnt.sum())
    d = [gpu.to_device(np.ascontiguousarray(uv[:, 0])), gpu.to_device(np.ascontiguousarray(uv[:, 1])), gpu.to_device(off), gpu.to_device(cnt),
         gpu.to_device(2 * off)]
    tri, tc, st = gpu.empty((T + 1, 3), np.int32).fill(SENT), gpu.empty(F + 1, np.int32).fill(SENT), gpu.empty(F + 1, np.int32).fill(SENT)
    m = int(cnt.max() if max_pts is None else max_pts)
    if qhull:
        _lib.check(gpu.lib.mvosr_delaunay_qhull_batch(gpu.handle, F, d[2].ptr, d[3].ptr, d[0].ptr, d[1].ptr, None, m, d[4].ptr, tri.ptr, tc.ptr,
                                                      None, st.ptr, None), "mvosr_delaunay_qhull_batch")
    else:
        _lib.check(gpu.lib.mvosr_delaunay_batch(gpu.handle, F, d[2].ptr, d[3].ptr, d[0].ptr, d[1].ptr, None, m, d[4].ptr, tri.ptr, tc.ptr,
                                                None, st.ptr), "mvosr_delaunay_batch")
    gpu.sync()
    t, n, s = tri.download(), tc.download(), st.download()
    for b in d + [tri, tc, st]:
        b.free()
    slices = [t[2 * off[f]:2 * off[f] + 2 * cnt[f]] for f in range(F)]
    rows = [slices[f][:max(int(n[f]), 0)] for f in range(F)]
    return rows, slices, n[:F], s[:F], fc.all_bytes(t[T:], SENT) and fc.all_bytes(n[F:], SENT) and fc.all_bytes(s[F:], SENT)


@pytest.mark.parametrize("qhull", [False, True], ids=["delaunay", "qhull"])
def test_triangulation_frame_larger_than_max_pts(gpu, qhull):
    """mvosr_delaunay_batch and mvosr_delaunay_qhull_batch: a frame above max_pts is declined — status & 0xFF ==
    MVOSR_DT_DEGENERATE, tri_cnt 0, no row written — and its neighbours have the rows they get alone (SciPy's: in canonical form
    from the first, themselves from the second)."""
    from scipy.spatial import Delaunay
    from mvoscalerecovery_amd import packing
    sizes, mid = (48, 97, 131, 26, 60), 2
    rng = np.random.default_rng(600)
    sets = [np.ascontiguousarray(rng.uniform(0, 1, (n, 2)) * [1241.0, 376.0]) for n in sizes]
    solo = [_run_delaunay(gpu, [q], qhull) for q in sets]
    for header in _headers(sizes, mid):
        rows, slices, tcnt, status, guards = _run_delaunay(gpu, sets, qhull, max_pts=header)
        assert guards, header
        for f, q in enumerate(sets):
            if f == mid:
                assert (status[f] & 0xFF) == 1 and tcnt[f] == 0 and fc.all_bytes(slices[f], SENT), (header, status[f], tcnt[f])
                continue
            assert status[f] == 0 == solo[f][3][0] and tcnt[f] == solo[f][2][0] and solo[f][4], (header, f, status[f])
            assert _same(rows[f], solo[f][0][0]), (header, f)
            want = Delaunay(q).simplices
            assert np.array_equal(rows[f], want if qhull else packing.canonical_rows(want)), (header, f)
    assert solo[mid][3][0] == 0 and solo[mid][2][0] == len(Delaunay(sets[mid]).simplices)
