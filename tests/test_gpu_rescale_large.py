"""The rescale variant's large-frame kernels (csrc/mvosr_rescale_large.hip) and ScaleEstimator(large_frames=True).  Needs a real
MI355X:  python -m pytest tests -m gpu

Below the resident limit the comparator is the resident entry point, byte for byte, over whole sentinel-filled arrays
(tests/large_cases.py); beyond it, oracle/rescale_oracle.py with the device's sample sequence."""
import numpy as np
import pytest

import flat_cases as fc
import large_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def max_points(gpu):
    return fc.max_points(gpu)


@pytest.fixture(scope="module")
def families(max_points):
    fam = dict(fc.select_families())
    fam.update(fc.tail_families(max_points))
    fam.update(lc.flat_frames())
    assert len(fam["at_max_points"].xyz) == max_points            # the largest frame both entry points take
    return fam


def _resident_batches(frames, lds_per_block, n_hyp=100):
    """`frames` in order, cut into batches the RESIDENT entry point takes: its LDS request grows with the batch's largest feature
    count and largest row count (flat_plan of csrc/mvosr_rescale_plan.hpp, bounded from above as _max_points() bounds it)."""
    out, cur, mf, mt = [], [], 0, 0
    for f in frames:
        nf, nt = max(mf, len(f.xyz)), max(mt, len(f.tri))
        if cur and 24 * (nf + 2) + 9 * nt + 14000 + 36 * n_hyp > lds_per_block:
            out.append(cur)
            cur, nf, nt = [], len(f.xyz), len(f.tri)
        cur.append(f)
        mf, mt = nf, nt
    return out + [cur]


def _pair(gpu, frames, **kw):
    a, toff = lc.run_flat(gpu, frames, "resident", **kw)
    b, _ = lc.run_flat(gpu, frames, "large", **kw)
    return a, b, toff


# ---- large against resident, byte for byte ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_keep", [True, False])
def test_flat_large_equals_resident_on_crafted_families(gpu, families, use_keep):
    """Every crafted family of flat_cases (select: one-bin starts, repeated patterns, direct ranking, both parities, thresholds,
    bad ids, singular rows; tail: packed / dedup / list layouts, keep words, the frame of exactly _max_points() features) and the
    refusals of large_cases, in as few batches as the resident entry point's LDS takes: every byte of every output — tri_height, tri_flags and hyp_counts included, guards and
    unwritten rows included — equals the resident entry point's."""
    seen = set()
    for frames in _resident_batches(list(families.values()), gpu.lds_per_block):
        a, b, toff = _pair(gpu, frames, use_keep=use_keep)
        assert lc.same_bytes(a, b) == [], [f.name for f in frames]
        seen |= set(int(s) for s in a["status"][:len(frames)])
        # without the optional outputs (heights and flags in the workspace): the required ones are the same bytes, the others untouched
        c, _ = lc.run_flat(gpu, frames, "large", use_keep=use_keep, optional=False)
        assert lc.same_bytes(a, c, lc.FLAT_FIELDS[:7]) == []
        assert all(fc.all_bytes(c[k], lc.SENTINEL) for k in lc.FLAT_FIELDS[7:])
    assert {0, fc.ST_SINGULAR, fc.ST_MASK, fc.ST_EMPTY, fc.ST_RS_FEW} <= seen                          # (the set covers every status)


@pytest.mark.parametrize("n_hyp", [1, 100, 512])
def test_flat_large_batch_positions_and_sample_inputs(gpu, families, n_hyp):
    """One frame alone, and as first, middle and last of a batch — with and without keep words, with frame_ids, with id_triples:
    resident bytes, and the frame's own results do not depend on its place."""
    A = fc.road_frame("A", 260, 300, 171).with_keep(172, 90)
    B, Cc = families["k3"], families["grid"]
    batch = [A, B, A, Cc, A]
    ids = [40, 7, 40, 9, 40]
    for use_keep in (True, False):
        a, b, toff = _pair(gpu, batch, n_hyp=n_hyp, use_keep=use_keep, frame_ids=ids, seed=77)
        assert lc.same_bytes(a, b) == []
        one, _, toff1 = _pair(gpu, [A], n_hyp=n_hyp, use_keep=use_keep, frame_base=40, seed=77)
        assert lc.same_bytes(one, _) == []
        for i in (0, 2, 4):
            for k in ("raw_scale", "height_level", "model", "best_ic", "used", "n_kept", "status", "hyp_counts"):
                assert np.array_equal(b[k][i], one[k][0], equal_nan=True), (k, i)
            assert np.array_equal(b["tri_flags"][toff[i]:toff[i + 1]], one["tri_flags"][:toff1[1]])
            assert np.array_equal(b["tri_height"][toff[i]:toff[i + 1]], one["tri_height"][:toff1[1]])
    rng = np.random.default_rng(n_hyp)
    triples = [rng.integers(-2, len(f.survivors()) + 2, (n_hyp, 3)) for f in batch]        # (ids out of range are clamped alike)
    a, b, _ = _pair(gpu, batch, n_hyp=n_hyp, id_triples=triples)
    assert lc.same_bytes(a, b) == []
    assert n_hyp < 100 or int(a["status"][0]) == 0                 # (one random triple seldom is a plane with an inlier)


def test_flat_large_refusals_and_recycled_workspace(gpu, families):
    """A header that states less than a frame holds (max_feat, max_tri) and a declined dt_status: the resident refusals, nothing
    else written.  A second launch after a larger batch has dirtied the workspace gives the same bytes."""
    frames = [families["road_small"], families["road_packed"], families["k64"], families["grid"]]
    for kw in ({"max_feat": 100}, {"max_tri": 150}, {"dt_status": [0, 5, 0, 5]}):
        a, b, _ = _pair(gpu, frames, **kw)
        assert lc.same_bytes(a, b) == [], kw
        assert {fc.ST_MASK, fc.ST_EMPTY} & set(int(s) for s in b["status"][:4])
    first, _ = lc.run_flat(gpu, frames, "large", optional=False)
    lc.run_flat(gpu, [families["at_max_points"], families["road_dedup"]] * 2, "large", optional=False)
    again, _ = lc.run_flat(gpu, frames, "large", optional=False)
    assert lc.same_bytes(first, again) == []


def test_flat_large_abi_contract(gpu, families):
    """n_frames <= 0 launches nothing; n_hyp outside 1..512 is an argument error; under a workspace limit the call returns
    MVOSR_ERR_ALLOC (its own context: the shared one's workspace may already be large enough)."""
    import ctypes as C
    from mvoscalerecovery_amd import _lib
    b = _lib.Batch()
    b.n_frames = 0
    dummy = gpu.zeros(8, np.float64)
    for name in ("x", "y", "z", "v", "feat_off", "feat_cnt", "tri1_off", "tri1", "tri2_off", "tri2"):
        setattr(b, name, dummy.ptr)
    ro = _lib.RescaleOutputs(*([dummy.ptr] * 7 + [None] * 3))
    rp = _lib.RescaleParams(0, 10, -80.0, -85.0, 0.9, 12, 100, 0.005, 0.8, 1.75, 1, 0)
    assert gpu.lib.mvosr_flat_ransac_large_batch(gpu.handle, C.byref(b), None, C.byref(rp), None, None, None, C.byref(ro), 0) == 0
    assert gpu.lib.mvosr_graph_keep_large_batch(gpu.handle, C.byref(b), 0, 10, None, dummy.ptr, None, None, 0) == 0
    rp.n_hyp = 513
    assert gpu.lib.mvosr_flat_ransac_large_batch(gpu.handle, C.byref(b), None, C.byref(rp), None, None, None, C.byref(ro), 0) != 0
    dummy.free()
    ctx = _lib.Context(0)
    try:
        ctx.workspace_limit(4096)
        with pytest.raises(_lib.MvosrAllocError):
            lc.run_flat(ctx, [families["road_packed"]], "large")
        ctx.workspace_limit(0)
        a, _ = lc.run_flat(ctx, [families["road_packed"]], "large")
        assert int(a["status"][0]) == 0
    finally:
        ctx.close() if hasattr(ctx, "close") else None


def test_graph_keep_large_equals_resident_whatever_the_tile(gpu):
    """flat_cases.graph_cases() — ten-or-fewer survivors, a declined triangulation, ties and -0.0 — with a bad id, a frame without
    rows, one without features and a 300-feature Delaunay frame, as one batch: keep, n_valid and status are the resident entry
    point's bytes for the library's tile and for 64, 100, n - 1, n, n + 1 (n = 300: one to five sweeps)."""
    cases = lc.graph_cases()
    want, off = lc.run_keep(gpu, cases, large=False)
    n = len(cases[-1]["v"])
    assert n == 300
    for tile in (0, 64, 100, n - 1, n, n + 1):
        got, _ = lc.run_keep(gpu, cases, large=True, tile=tile)
        assert lc.same_bytes(want, got) == [], tile
    for i, c in enumerate(cases):                                   # ... and the oracle's, where the frame is whole
        if c["declined"] or c["name"] in ("bad_id", "no_features"):
            continue
        keep, nv = lc.keep_oracle(c)
        assert np.array_equal(want["keep"][off[i]:off[i + 1]], keep) and int(want["n_valid"][i]) == nv, c["name"]
    # the header's max_feat below a frame: refused like the resident one
    a, _ = lc.run_keep(gpu, cases, large=False, max_feat=100)
    b, _ = lc.run_keep(gpu, cases, large=True, max_feat=100, tile=64)
    assert lc.same_bytes(a, b) == []


# ---- beyond the resident limit: the oracle ---------------------------------------------------------------------------------------
def test_large_kernels_one_frame_past_the_limit(gpu, max_points):
    """_max_points() + 1 features: the vote against the oracle's words, flat_selection + RANSAC against the oracle the way
    gpu_helpers compares (point list, inlier count, consumed hypotheses exact; heights, level, plane, scale to 1e-9)."""
    frame = fc.road_frame("past", 700, max_points + 1 - 700, 266)
    assert len(frame.xyz) == max_points + 1
    want = lc.oracle_flat(frame, seed=5, frame_counter=3)
    assert want["status"] == 0 and want["M"] >= 12                  # (checked on the CPU before the device runs)
    r, toff = lc.run_flat(gpu, [frame], "large", frame_base=3, seed=5)
    lc.check_flat_against_oracle(r, toff, 0, frame, want)
    case = lc.delaunay_graph_case("past", max_points + 1, 267)
    keep, nv = lc.keep_oracle(case)
    got, off = lc.run_keep(gpu, [case], large=True)
    assert np.array_equal(got["keep"][:off[1]], keep) and int(got["n_valid"][0]) == nv and int(got["status"][0]) == 0


def test_large_kernels_wide_list_and_many_rows(gpu):
    """An all-road 110 x 110 grid: 23 762 rows (more than MVOSR_GRAPH_MAX_ROWS), nearly every one kept, a point list of 70 935 entries
    — the smallest shape at which a 16-bit id, list position or tally goes wrong.  Two tiles in the vote (12 100 > 8192)."""
    frame = lc.big_grid()
    assert len(frame.tri) > 21845
    want = lc.oracle_flat(frame, seed=9, frame_counter=0)
    assert want["status"] == 0 and want["M"] > 65535
    r, toff = lc.run_flat(gpu, [frame], "large", seed=9, use_keep=False)
    lc.check_flat_against_oracle(r, toff, 0, frame, want)
    assert int(r["best_ic"][0]) > 65535                             # (the count itself is wider than 16 bits)
    rng = np.random.default_rng(3)
    case = lc.graph_case("grid", frame.xyz[:, 2] * 30.0 + rng.normal(0, 1.0, len(frame.xyz)), frame.xyz[:, 2] + rng.normal(0, 0.3, len(frame.xyz)),
                         np.concatenate([frame.tri, frame.tri[:4000]]))
    keep, nv = lc.keep_oracle(case)
    for tile in (0, 5000):
        got, off = lc.run_keep(gpu, [case], large=True, tile=tile)
        assert np.array_equal(got["keep"][:off[1]], keep) and int(got["n_valid"][0]) == nv, tile


# ---- the estimator ---------------------------------------------------------------------------------------------------------------
MODES = ({"triangulation": "gpu"}, {"triangulation": "scipy", "sampling": "device"})


@pytest.fixture(scope="module")
def c5_frame():
    """One 20 000-feature synth frame (BASELINE config C5's shape) and the oracle's run of it, made once: status 0, M >= 12."""
    from mvoscalerecovery_amd import synth
    frames = [synth.synth_frame(3, 20000, base_seed=4242)]
    want, snap, ref = lc.oracle_estimator_run(frames, window=5, seed=77)
    assert snap[0]["model"] is not None and len(snap[0]["ids"]) >= 12          # (on the CPU, before the device runs)
    return frames, want, snap, ref


@pytest.mark.parametrize("mode", MODES, ids=["gpu", "scipy-device"])
def test_estimator_takes_a_20000_feature_frame(gpu, c5_frame, max_points, mode):
    """ScaleEstimator(large_frames=True) end to end on a 20 000-feature frame against the oracle: vote mask, point list, inlier count
    and consumed hypotheses exact; level, plane and scale to 1e-9 — with both triangulations on the device, and with SciPy's."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    frames, want, snap, ref = c5_frame
    assert int(np.count_nonzero(frames[0][1][:, 1] > 185)) > max_points
    est = ScaleEstimator(fc.ABS_REF, window_size=5, ransac_seed=77, delaunay_workers=0, large_frames=True, **mode)
    lc.check_estimator_against_oracle(est, frames, want, snap, ref)
    assert est.last_declined == 0


@pytest.fixture(scope="module")
def ragged():
    from mvoscalerecovery_amd import synth
    sizes = [600, 4200, 700, 3900, 500, 800, 5200, 650, 900]
    return sizes, [synth.synth_frame(i, n, base_seed=909) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("mode", MODES, ids=["gpu", "scipy-device"])
def test_estimator_ragged_batch_four_ways(gpu, ragged, max_points, mode):
    """Frames above the resident limit scattered in a batch: one call, two calls, per-frame calls and two-frame chunks give the same
    scales, queue, running scale, sample counter and per-frame results; the small frames' raw results are those of
    large_frames=False at the same sample counters."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    sizes, frames = ragged
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    below = [int(np.count_nonzero(f2[:, 1] > 185)) for f2 in f2s]
    big = [i for i, n in enumerate(below) if n > max_points]
    assert len(big) == 3 and 0 not in big
    new = lambda **kw: ScaleEstimator(fc.ABS_REF, window_size=5, ransac_seed=31, delaunay_workers=0, **kw, **mode)
    one = new(large_frames=True)
    s_one, _ = one.scale_calculation_batch(f3s, f2s)
    assert np.all(np.isfinite(s_one)) and np.all(one.last["status"][big] == 0)
    two = new(large_frames=True)
    s_two = np.concatenate([two.scale_calculation_batch(f3s[:4], f2s[:4])[0], two.scale_calculation_batch(f3s[4:], f2s[4:])[0]])
    per = new(large_frames=True)
    s_per = np.array([per.scale_calculation(f3, f2)[0] for f3, f2 in frames])
    small = new(large_frames=True)
    small.GPU_CHUNK = small.GPU_MIN_CHUNK = 2
    s_small, _ = small.scale_calculation_batch(f3s, f2s)
    for est, s in ((two, s_two), (per, s_per), (small, s_small)):
        assert np.array_equal(s, s_one)
        assert list(est.scale_queue) == list(one.scale_queue) and est.scale == one.scale and est._frame_counter == one._frame_counter == len(frames)
    for k in ("raw_scale", "model", "best_ic", "used", "n_kept", "status", "height_level"):
        assert np.array_equal(small.last[k], one.last[k], equal_nan=True), k
        assert np.array_equal(per.last[k][0], one.last[k][-1], equal_nan=True), k
    old = new()
    for i in range(len(frames)):
        if i in big:
            continue
        raw, status, level, _ = old.raw_scale_batch([f3s[i]], [f2s[i]], frame_base=i)
        assert raw[0] == one.last["raw_scale"][i] and status[0] == one.last["status"][i] and level[0] == one.last["height_level"][i], i
    # the default estimator still refuses the first large frame, with the message it has always had
    with pytest.raises(ValueError, match="frame %d has %d features.*one workgroup's LDS" % (big[0], below[big[0]])):
        old.scale_calculation_batch(f3s, f2s)


@pytest.mark.parametrize("mode", MODES, ids=["gpu", "scipy-device"])
def test_estimator_refuses_beyond_the_opt_in_limit(gpu, mode):
    """A frame beyond mvosr_delaunay_max_points() under large_frames=True: the ValueError names the frame and the new limit, the
    frames before it have gone through the slew limiter, the window and the sample counter, and the estimator carries on — the
    state tests/test_gpu_rescale.py describes for the old limit."""
    from mvoscalerecovery_amd import packing, synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    limit = packing.delaunay_gpu_max_points()
    frames = [synth.synth_frame(i, 600, base_seed=77) for i in range(6)]
    frames.insert(3, synth.synth_frame(99, limit + 3000, base_seed=77))
    n_big = int(np.count_nonzero(frames[3][1][:, 1] > 185))
    assert n_big > limit
    new = lambda: ScaleEstimator(fc.ABS_REF, window_size=5, ransac_seed=3, delaunay_workers=0, large_frames=True, **mode)
    est = new()
    assert est._large_max_points() == limit == est._frame_limit() > est._max_points()
    with pytest.raises(ValueError, match="frame 3 has %d features.*at most %d per frame with large_frames=True" % (n_big, limit)):
        est.scale_calculation_batch([f[0] for f in frames], [f[1] for f in frames])
    ref = new()
    ref.scale_calculation_batch([f[0] for f in frames[:3]], [f[1] for f in frames[:3]])
    assert list(est.scale_queue) == list(ref.scale_queue) and est.scale == ref.scale and len(est.scale_queue) == 3
    assert est._frame_counter == 4                                        # (the refused frame took its turn)
    with pytest.raises(ValueError, match="frame 0 has %d features" % n_big):
        est.scale_calculation_batch([frames[3][0]], [frames[3][1]])
    s, _ = est.scale_calculation_batch([f[0] for f in frames[4:]], [f[1] for f in frames[4:]])
    assert np.all(np.isfinite(s))


def test_estimator_large_frames_steady_state_allocates_nothing(gpu, ragged):
    """No hipMalloc / hipHostMalloc between the second and the third identical call with large frames in it."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    _, frames = ragged
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    est = ScaleEstimator(fc.ABS_REF, window_size=5, ransac_seed=1, delaunay_workers=0, triangulation="gpu", large_frames=True)
    est.scale_calculation_batch(f3s, f2s)
    est.scale_calculation_batch(f3s, f2s)
    before = gpu.alloc_stats()
    est.scale_calculation_batch(f3s, f2s)
    after = gpu.alloc_stats()
    assert after["hip_malloc"] == before["hip_malloc"] and after["host_malloc"] == before["host_malloc"], (before, after)


# ---- model="static_tri" on large frames, and what keeps the old limit ---------------------------------------------------------
def test_static_tri_takes_large_frames(gpu, max_points):
    """model="static_tri" with large_frames=True on a batch with a frame above _max_points(): the vote's masks and the number of
    loose heights are the oracle's, exactly; the mode (or median) of the inverse heights — statictri_cases.static_tri_of on the
    oracle's loose heights — to 1e-9, on seeds for which that figure does not move when the heights move by 1e-9 (checked on the
    CPU first).  The small frames of the batch, which ride through the large-frame kernels, give the bits of large_frames=False;
    without the keyword the large frame fails as before; beyond the opt-in limit: the ValueError that names it."""
    import statictri_cases as stc
    from mvoscalerecovery_amd import _lib, packing, synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    from oracle import rescale_oracle as ro
    frames = [synth.synth_frame(i, n, base_seed=515) for i, n in enumerate([700, 6000, 900])]
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    assert int(np.count_nonzero(f2s[1][:, 1] > 185)) > max_points
    ref = ro.OracleRescaleEstimator(fc.ABS_REF, window_size=5, sampler=lambda n: None)
    rng = np.random.default_rng(1)
    want, masks = [], []
    for f3, f2 in frames:
        _, loose = ref.feature_selection(np.asarray(f3, np.float64), np.asarray(f2, np.float64))
        w = stc.static_tri_of(loose, min_count=12, absolute_reference=fc.ABS_REF)
        assert w["status"] not in (stc.ST_RS_FEW, stc.ST_ERR_MASK) and w["n_used"] > 12
        for _ in range(3):
            moved = stc.static_tri_of(loose * rng.uniform(1 - 1e-9, 1 + 1e-9, len(loose)), min_count=12, absolute_reference=fc.ABS_REF)
            assert moved["status"] == w["status"] and abs(moved["raw_scale"] - w["raw_scale"]) <= 2e-9 * w["raw_scale"]
        want.append(w)
        masks.append(ref.last["valid"].copy())
    new = lambda **kw: ScaleEstimator(fc.ABS_REF, window_size=5, delaunay_workers=0, model="static_tri", **kw)
    est = new(large_frames=True)
    s, zeros = est.scale_calculation_batch(f3s, f2s)
    assert not zeros.any() and len(est.scale_queue) == 0
    for i, w in enumerate(want):
        assert np.array_equal(est.last["valid"][i], masks[i]), i
        assert int(est.last["n_used"][i]) == w["n_used"] and int(est.last["status"][i]) == w["status"], i
        assert abs(est.last["raw_scale"][i] - w["raw_scale"]) <= 1e-9 * w["raw_scale"], i
        assert abs(s[i] - w["raw_scale"]) <= 1e-9 * w["raw_scale"], i
    old = new()
    for i in (0, 2):
        old.scale_calculation_batch([f3s[i]], [f2s[i]])
        for k in ("raw_scale", "scale_norm", "n_used", "status", "height_level"):
            assert old.last[k][0] == est.last[k][i], (k, i)
    with pytest.raises(_lib.MvosrLibraryError):
        new().scale_calculation_batch(f3s, f2s)
    limit = packing.delaunay_gpu_max_points()
    big = synth.synth_frame(9, limit + 3000, base_seed=515)
    with pytest.raises(ValueError, match="frame 1 has .* features.*at most %d per frame with large_frames=True" % limit):
        new(large_frames=True).scale_calculation_batch([f3s[0], big[0]], [f2s[0], big[1]])


def test_what_keeps_the_old_limit_under_large_frames(gpu):
    """RepeatedRuns and ConstantSweep meet a 5000-feature frame, model="static" and region="grow" a 9000-feature one, with
    large_frames=True exactly as without it: the same exception type, the same message."""
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ConstantSweep, RepeatedRuns, ScaleEstimator
    frames = [synth.synth_frame(0, 600, base_seed=77), synth.synth_frame(99, 5000, base_seed=77)]
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]

    def outcome(call):
        with pytest.raises(Exception) as exc:
            call()
        return type(exc.value), str(exc.value)
    for kw in ({}, {"large_frames": True}):
        rr = RepeatedRuns(fc.ABS_REF, window_size=5, cases=2, seed=7, triangulation="gpu", delaunay_workers=0, **kw)
        t, msg = outcome(lambda: rr.estimator.raw_scale_cases_batch(f3s, f2s, rr.seeds))
        assert t is ValueError and "frame 1 has 5000 features" in msg and "one workgroup's LDS" in msg and "large_frames" not in msg
        sw = ConstantSweep(fc.ABS_REF, ConstantSweep.grid(), window_size=5, cases=2, seed=7, triangulation="gpu", delaunay_workers=0, **kw)
        t, msg = outcome(lambda: sw._raw_cases(f3s, f2s))
        assert t is ValueError and "frame 1 has 5000 features" in msg and "one workgroup's LDS" in msg and "large_frames" not in msg
    # (the staged path's own LDS limit lies higher: its vote kernel holds 20 bytes a feature — 9000 features do not fit 160 KiB)
    g3s, g2s = [f3s[0], synth.synth_frame(98, 9000, base_seed=77)[0]], [f2s[0], synth.synth_frame(98, 9000, base_seed=77)[1]]
    for staged in ({"model": "static"}, {"region": "grow"}):
        a = outcome(lambda: ScaleEstimator(fc.ABS_REF, window_size=5, delaunay_workers=0, **staged).scale_calculation_batch(g3s, g2s))
        b = outcome(lambda: ScaleEstimator(fc.ABS_REF, window_size=5, delaunay_workers=0, large_frames=True, **staged).scale_calculation_batch(g3s, g2s))
        assert a == b, staged
