"""GPU: RansacEvaluation / RansacBudgetSweep(triangulation="gpu", resident=True) — the device-resident path — against the
unchanged staged ``triangulation="gpu"`` run byte for byte, and mvosr_height_pitch_eval_tail_batch alone through the C ABI against
the restatement of tests/hpeval_carry_cases.py, byte for byte.

Every object here runs at most 64 hypotheses on frames of a few hundred features.  The frames with fewer than 12 list points are the
crafted `three` (9 list points under a Delaunay triangulation of its pixels) and `one_row` (3), and the singular frame is the crafted
`singular` with its repeated point moved to a pixel of its own at depth 0, as in tests/test_gpu_heightpitch_resident.py: the resident
path triangulates on the device, so a crafted frame's own rows do not enter."""
import ctypes as C

import numpy as np
import pytest

import heightpitch_cases as hc
import hpeval_carry_cases as cc
import hpeval_cases as he

pytestmark = pytest.mark.gpu

H, SEED, CASES, BUDGETS = 64, 3, 10, (4, 20, 64)


def same_bytes(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


# ---- 1. the tail alone, through the C ABI ---------------------------------------------------------------------------------------
def run_tail(chunk, carry, used_best=True):
    """mvosr_height_pitch_eval_tail_batch on a hand-made chunk -> dict of everything it wrote (the outputs start as 0xAB bytes)."""
    from mvoscalerecovery_amd import _lib
    from mvoscalerecovery_amd import height_pitch as hp
    ctx = _lib.default_context(0)
    F, Cn, B = chunk["status"].shape
    ints = ("status", "n_inliers") + (("used", "best") if used_best else ())
    doubles = cc.VALUES + ("sum_y", "sum_z")
    nbytes = hp.eval_carry_bytes(Cn, B)
    d = ctx.block([("n_selected", F, np.int32), ("prior", (F, 4), np.float64)] + [(k, (F, Cn, B), np.int32) for k in ints] +
                  [(k, (F, Cn, B), np.float64) for k in doubles] + [("carry_in", len(carry), np.uint8)])
    o = ctx.block([(k, (B, Cn, F), np.float64) for k in cc.FIELDS] + [("degenerate", (B, Cn, F), np.uint8)] +
                  ([("used", (B, Cn, F), np.int32), ("best", (B, Cn, F), np.int32)] if used_best else []) +
                  [("carried", F, np.uint8), ("frame_class", F, np.int32), ("source", F, np.int32), ("error", 1, np.int64),
                   ("carry_out", nbytes, np.uint8)])
    try:
        d.upload(dict({k: chunk[k] for k in ("n_selected", "prior") + ints + doubles}, carry_in=carry))
        _lib.check(ctx.lib.mvosr_memset(ctx.handle, o.ptr, 0xAB, o.nbytes), "memset")
        ti, to = _lib.HeightPitchEvalTailInputs(), _lib.HeightPitchEvalTailOutputs()
        for k, _ in ti._fields_:
            setattr(ti, k, d[k].ptr if k in d else None)
        for k, _ in to._fields_:
            setattr(to, k, o[k].ptr if k in o else None)
        _lib.check(ctx.lib.mvosr_height_pitch_eval_tail_batch(ctx.handle, F, Cn, B, cc.MIN_POINTS, C.byref(ti), d["prior"].ptr, d["carry_in"].ptr,
                                                              o["carry_out"].ptr, C.byref(to)), "mvosr_height_pitch_eval_tail_batch")
        return {k: v.download() for k, v in o.views.items()}
    finally:
        d.free()
        o.free()


def assert_tail(chunk, carry, used_best=True):
    """The kernels' outputs, error word and carry-out are the restatement's, byte for byte -> the restatement's result."""
    got, want = run_tail(chunk, carry, used_best), cc.tail(chunk, carry, used_best=used_best)
    assert int(got["error"][0]) == want["error"], (int(got["error"][0]), want["error"])
    assert same_bytes(got["carry_out"], want["carry_out"])
    per_element = cc.FIELDS + ("degenerate",) + (("used", "best") if used_best else ())
    n = want["end"]
    if not want["upstream"]:
        for k in ("frame_class", "source", "carried"):
            assert same_bytes(got[k], want[k]), k
        for k in per_element:
            assert same_bytes(got[k][:, :, :n], want[k]), k
    for k in per_element + (("frame_class", "source", "carried") if want["upstream"] else ()):
        rest = got[k][..., n:] if not want["upstream"] else got[k]                   # frames from the error on: not written
        assert np.all(np.ascontiguousarray(rest).view(np.uint8) == 0xAB), k
    return want


@pytest.mark.parametrize("Cn,B", [(1, 1), (9, 7), (16, 4), (13, 5), (10, 16)], ids=lambda v: str(v))
@pytest.mark.parametrize("F", [1, 255, 256, 257, 513])
def test_tail_at_the_round_and_wavefront_edges(F, Cn, B):
    from mvoscalerecovery_amd import height_pitch as hp
    kinds = cc.kinds_for(F)
    assert F < 257 or (kinds[255], kinds[256]) == ("carry", "carry")                 # the last frame of a round, the first of the next
    first = assert_tail(cc.chunk_of(kinds, Cn, B, seed=F + Cn), hp.eval_carry_record(Cn, B))
    assert first["error"] == -1 and first["end"] == F
    # a chunk whose every frame is carried: the source is the carry-in's
    every = assert_tail(cc.chunk_of(["carry"] * min(F, 70), Cn, B, seed=1), first["carry_out"], used_best=F != 255)
    assert every["error"] == -1 and np.all(every["source"] == -1) and np.all(every["carried"] == 1)
    if kinds[F - 1] == "fit":
        assert same_bytes(every["ransac_height"][:, :, 0], first["ransac_height"][:, :, F - 1])


def test_tail_chunk_boundaries_and_degenerate_sources():
    from mvoscalerecovery_amd import height_pitch as hp
    seq = ["fit", "carry", "carry", "carry", "deg", "carry", "fit", "deg", "carry", "carry", "fit"]
    Cn, B = 3, 2
    chunk = cc.chunk_of(seq, Cn, B, seed=3)
    whole = assert_tail(chunk, hp.eval_carry_record(Cn, B))
    assert whole["source"].tolist() == [0, 0, 0, 0, 4, 4, 6, 7, 7, 7, 10]
    assert np.isnan(whole["height_t_mean"][0, 0, 5]) and np.isfinite(whole["height_t_mean"][1, 0, 5])   # degenerate at one budget only
    assert whole["degenerate"][0, 0, 5] == 1 and whole["ransac_height"][0, 0, 5] == chunk["ransac_height"][4, 0, 0]
    for c in range(1, len(seq)):                                                     # between source and carried frame too
        a = assert_tail(cc.cut(chunk, 0, c), hp.eval_carry_record(Cn, B))
        b = assert_tail(cc.cut(chunk, c, len(seq)), a["carry_out"])
        for k in cc.FIELDS + ("degenerate", "used", "best"):
            assert same_bytes(np.concatenate([a[k], b[k]], axis=2), whole[k]), (c, k)
        assert same_bytes(b["carry_out"], whole["carry_out"])


@pytest.mark.parametrize("kind,code", [("singular", cc.ERR_SINGULAR), ("mask", cc.ERR_MASK), ("empty", cc.ERR_EMPTY), (("nomodel", 0), cc.ERR_NO_MODEL),
                                       (("nomodel", 2), cc.ERR_NO_MODEL), ("status", cc.ERR_STATUS)], ids=lambda v: str(v))
def test_tail_error_kinds_and_the_halted_carry(kind, code):
    from mvoscalerecovery_amd import height_pitch as hp
    Cn, B = 13, 5
    kinds = ["fit", "carry"] * 130 + ["fit", kind, "fit", "carry"]                   # the error in the second round of the resolve step
    r = assert_tail(cc.chunk_of(kinds, Cn, B, seed=4), hp.eval_carry_record(Cn, B))
    assert hp.eval_tail_error(r["error"]) == (code, kind[1] if isinstance(kind, tuple) else 0, 261) and r["end"] == 261
    head, _ = hp.eval_carry_fields(r["carry_out"])
    assert (head["has_prev"], head["halted"]) == (1, 1)
    nxt = assert_tail(cc.chunk_of(["fit", "carry"], Cn, B, seed=5), r["carry_out"], used_best=False)      # a halted carry-in
    assert hp.eval_tail_error(nxt["error"])[0] == cc.ERR_UPSTREAM and same_bytes(nxt["carry_out"], r["carry_out"])


def test_tail_no_previous():
    from mvoscalerecovery_amd import height_pitch as hp
    Cn, B = 2, 3
    r = assert_tail(cc.chunk_of(["carry", "fit"], Cn, B, seed=7), hp.eval_carry_record(Cn, B))           # at frame 0
    assert hp.eval_tail_error(r["error"]) == (cc.ERR_NO_PREVIOUS, 0, 0)
    assert same_bytes(r["carry_out"], hp.eval_carry_record(Cn, B, None, halted=True))
    r = assert_tail(cc.chunk_of(["fit", "carry"], Cn, B, seed=7), hp.eval_carry_record(Cn, B))           # the same kinds the other way round: fine
    assert r["error"] == -1
    r = assert_tail(cc.chunk_of(["carry"] * 300, Cn, B, seed=8), hp.eval_carry_record(Cn, B), used_best=False)
    assert hp.eval_tail_error(r["error"]) == (cc.ERR_NO_PREVIOUS, 0, 0)
    r = assert_tail(cc.chunk_of(["fit"], Cn, B, seed=9), hp.eval_carry_record(Cn + 1, B))                # a record of another size
    assert hp.eval_tail_error(r["error"])[0] == cc.ERR_UPSTREAM


# ---- 2. both objects, both models, against the staged run -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return he.load_golden()


def make(kind, model, resident, **kw):
    from mvoscalerecovery_amd import height_pitch as hp
    if kind == "sweep":
        return hp.RansacBudgetSweep(model, BUDGETS, cases=CASES, seed=SEED, triangulation="gpu", resident=resident, **kw)
    return hp.RansacEvaluation(model, 32, cases=CASES, seed=SEED, triangulation="gpu", resident=resident, **kw)


def recorded_samples(model, frames):
    """List positions per frame for the lists a staged ``launch(stage=True)`` of the device triangulation builds."""
    from mvoscalerecovery_amd import height_pitch as hp
    ev = make("eval", model, False)
    rng = np.random.default_rng(12)
    out = []
    for p in frames:
        if not len(p):
            out.append(None)
            continue
        M = len(ev.launch([p], [hp.frame_prior(0.0)], stage=True)["point_list"][0])
        out.append(rng.integers(0, max(M, 1), (CASES, H, 3)).astype(np.int32))
    return out


def same_runs(res, ref, kind):
    assert set(res.results) == set(ref.results)
    for k in ref.results:
        assert same_bytes(res.results[k], ref.results[k]), k
    assert same_bytes(res.carried, ref.carried) and same_bytes(res.degenerate, ref.degenerate)
    if kind == "sweep":
        assert same_bytes(res.used, ref.used) and same_bytes(res.best, ref.best)


_STAGED = {}


def staged_run(golden, kind, model, case, draw):
    """The staged ``triangulation="gpu"`` run of a golden case, computed once and left unchanged."""
    key = (kind, model, case, draw)
    if key not in _STAGED:
        g = golden[model][case]
        samples = recorded_samples(model, g["frames"]) if draw == "recorded" else None
        ref = make(kind, model, False)
        ref.run(g["frames"], g["motion"][:, 3::4], samples=samples)
        _STAGED[key] = (ref, samples)
    return _STAGED[key]


@pytest.mark.parametrize("draw", ["device", "recorded"])
@pytest.mark.parametrize("batch", [512, 5, 1])
@pytest.mark.parametrize("model", he.MODELS)
@pytest.mark.parametrize("kind", ["eval", "sweep"])
def test_equals_the_staged_run_bytewise(golden, kind, model, batch, draw, tmp_path):
    for case in ("seq", "empty"):
        g = golden[model][case]
        ref, samples = staged_run(golden, kind, model, case, draw)
        res = make(kind, model, True)
        out = res.run(g["frames"], g["motion"][:, 3::4], samples=samples, batch=batch)
        assert out is res.results
        same_runs(res, ref, kind)
        assert res.declined_total == 0 and set(res.last) == {"dt_status", "errors"}
        assert sum(len(s) for s in res.last["dt_status"]) == sum(len(f) > 0 for f in g["frames"]) and all(e == -1 for e in res.last["errors"])
        if case == "empty":                                                          # six zeros, nothing carried
            assert not res.carried[1] and all(not v[..., 1].any() for v in res.results.values())
        if case == "seq" and batch == 5:
            assert [len(s) for s in res.last["dt_status"]] == [5, 3]
            a = res.write_results(str(tmp_path / "res"), "05", "x")
            b = ref.write_results(str(tmp_path / "ref"), "05", "x")
            assert len(a) == len(b) == 60 * (len(BUDGETS) if kind == "sweep" else 1)
            for pa, pb in zip(a, b):
                assert open(pa, "rb").read() == open(pb, "rb").read(), pa
            if kind == "sweep":                                                      # the untouched readers work on this path's results
                assert res.table() == ref.table() and res.smallest_budget() == ref.smallest_budget()
                assert all(same_bytes(x, y) for k in res.results for x, y in zip(res.spread()[k], ref.spread()[k]))
                assert same_bytes(res.results_at(20)["n_inliers"], ref.results_at(20)["n_inliers"])


# ---- 3. the sequence rules, end to end ------------------------------------------------------------------------------------------------
def singular_frame():
    s = hc.crafted()["singular"]
    pts = s.pts.copy()
    pts[18] = [pts[0, 0] + 3.0, pts[0, 1] + 2.0, 0.0]
    return pts


def both_raise(exc, kind, frames, motion, batch=2):
    """Both paths raise ``exc`` with the staged run's message, and leave ``results`` what it was."""
    res, ref = make(kind, "plane", True), make(kind, "plane", False)
    message = None
    for ev in (ref, res):
        before = ev.results = {"kept": np.zeros(1)}
        with pytest.raises(exc) as info:
            ev.run(frames, motion, batch=batch)
        message = message or str(info.value)
        assert str(info.value) == message and ev.results is before
    return res


@pytest.mark.parametrize("kind", ["eval", "sweep"])
def test_sequence_rules_end_to_end(golden, kind):
    c, g = hc.crafted(), golden["plane"]["seq"]
    fit, three, one_row, empty = g["frames"], c["three"].pts, c["one_row"].pts, np.zeros((0, 3))
    frames = [fit[0], three, one_row, fit[1], empty, three, fit[2]]
    motion = hc.motions(5, len(frames) + 2)[:, 3::4]
    res, ref = make(kind, "plane", True), make(kind, "plane", False)
    res.run(frames, motion, batch=2)
    ref.run(frames, motion, batch=2)
    same_runs(res, ref, kind)
    assert res.carried.tolist() == [False, True, True, False, False, True, False] and res.declined_total == 0
    assert [len(s) for s in res.last["dt_status"]] == [2, 2, 2]                      # the empty dump falls between chunks
    # a carried frame: the source's five values, its own height under the prior
    h = res.results["ransac_height"]
    assert same_bytes(h[..., 1], h[..., 0]) and same_bytes(h[..., 5], h[..., 3]) and not h[..., 4].any()
    ht = res.results["height_t_mean"]
    assert not same_bytes(ht[..., 1], ht[..., 2]) and not same_bytes(ht[..., 1], ht[..., 0])
    # the exceptions: the staged run's types and messages
    both_raise(IndexError, kind, [one_row, fit[0]], motion)
    both_raise(np.linalg.LinAlgError, kind, [fit[0], three, singular_frame(), fit[1], one_row], motion)
    r = both_raise(ValueError, kind, [fit[0], fit[1], fit[2][:1]], motion)
    assert r.declined_total == 1


# ---- 4. a frame the device triangulation declines -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["eval", "sweep"])
def test_declined_frame_takes_the_hosts_rows(golden, kind):
    g = golden["plane"]["seq"]
    frames = [f.copy() for f in g["frames"]]
    frames[3][7, 0:2] = frames[3][3, 0:2]                                            # an exactly repeated pixel, in the second chunk of four
    frames[4] = hc.crafted()["three"].pts                                            # the frame behind it is carried: its source is the declined frame
    res, ref = make(kind, "plane", True), make(kind, "plane", False)
    res.run(frames, g["motion"][:, 3::4], batch=2)
    ref.run(frames, g["motion"][:, 3::4], batch=2)
    same_runs(res, ref, kind)                                                        # ... so the later chunks' tails ran again
    assert res.carried.tolist() == [False] * 4 + [True] + [False] * 3
    status = np.concatenate(res.last["dt_status"])
    assert res.declined_total == 1 and status[3] != 0 and not status[[0, 1, 2, 4, 5, 6, 7]].any()
    assert all(isinstance(v, list) and len(v) == 4 for v in res.last.values())       # status and error words, no lists, no masks


@pytest.mark.parametrize("place", [0, 1])
@pytest.mark.parametrize("kind", ["eval", "sweep"])
def test_scipy_raises_on_a_declined_frame(golden, kind, place):
    """Six pixels on one image row, pixel 4 an exact copy of pixel 1 — the device triangulation declines the frame and the host's Qhull
    finds every point on one line —, as the first (``place`` 0: no tail runs again) or the second (1: the tail runs again over one frame)
    dump of the second chunk of two, two more chunks queued behind it: SciPy's exception leaves the run, ``results`` is what it was."""
    from scipy.spatial import QhullError
    g = golden["plane"]["seq"]
    frames = [f for f in g["frames"]]
    bad = np.array([[100.0 + 10 * i, 200.0, 10.0 + i] for i in range(6)])
    bad[4, 0:2] = bad[1, 0:2]
    frames[2 + place] = bad
    res = make(kind, "plane", True)
    assert res.GPU_PIPELINE == 2 and len(frames) == 8
    kept = res.results = {"kept": np.zeros(1)}
    before = res.ctx.alloc_stats()
    with pytest.raises(QhullError):
        res.run(frames, g["motion"][:, 3::4], batch=2)
    after = res.ctx.alloc_stats()
    print("alloc_stats before", before, "after", after, "dt_status", res.last["dt_status"], "errors", res.last["errors"])
    assert res.last["dt_status"][1][place] != 0                                      # the device did decline it (MVOSR_DT_DEGENERATE)
    assert res.declined_total == 1 and res.results is kept
    # (the counters of alloc_stats only grow; what a run can leave behind is a live block)
    assert after["live_blocks"] == before["live_blocks"]


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["eval", "sweep"])
def test_refusals(golden, kind):
    g = golden["plane"]["seq"]
    motion = g["motion"][:, 3::4]
    res = make(kind, "plane", True)
    with pytest.raises(ValueError, match="tris="):
        res.run(g["frames"][:2], motion, tris=g["rows"][:2])
    res.run(g["frames"][:2], motion)
    last, results = res.last, res.results
    big = np.random.default_rng(0).uniform(1.0, 300.0, (6000, 3))
    message = None
    for ev in (make(kind, "plane", False), res):
        with pytest.raises(ValueError, match="bytes of LDS") as info:
            ev.run([g["frames"][0], big], motion)
        message = message or str(info.value)
        assert str(info.value) == message                                            # the staged launch's message
    assert res.last is last and res.results is results and res.declined_total == 0   # ... before anything of the call ran
    from mvoscalerecovery_amd import height_pitch as hp
    assert "resident" not in vars(make(kind, "plane", False)) and hp.RansacEvaluation.GPU_PIPELINE == hp.HeightPitchEstimator.GPU_PIPELINE
