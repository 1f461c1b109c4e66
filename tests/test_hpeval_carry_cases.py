"""CPU: the restatement of mvosr_height_pitch_eval_tail_batch's contract (tests/hpeval_carry_cases.py) against the host's own rules —
a loop over ``height_pitch._eval_frame_rules`` as ``RansacBudgetSweep.run`` runs it —, chunked at every boundary against the
unchunked run, the carry record's round trip, the values an fma would change, and the ``resident=True`` refusal that needs no device
(DESIGN.md §3.27).  No GPU."""
import math

import numpy as np
import pytest

import hpeval_carry_cases as cc

C_B = ((1, 1), (3, 2), (2, 5))


def host_loop(chunk, budgets_named=True):
    """``RansacBudgetSweep.run``'s loop over a hand-made launch result, frame by frame and budget by budget -> (values (B, C, n),
    carried, degenerate, used, best, frames done, the exception or None)."""
    from mvoscalerecovery_amd import height_pitch as hp
    F, Cn, B = chunk["status"].shape
    budgets = tuple(10 * (k + 1) for k in range(B))
    out = {k: np.zeros((B, Cn, F)) for k in hp.RESULT_FIELDS}
    carried, deg = np.zeros(F, bool), np.zeros((B, Cn, F), bool)
    used, best = np.zeros((B, Cn, F), np.int32), np.full((B, Cn, F), -1, np.int32)
    prev = [None] * B
    ests = [float(e) for e in chunk["est"]]
    for f in range(F):
        row = {}
        try:
            for k, budget in enumerate(budgets):
                row[k] = hp._eval_frame_rules(f, ests[f], chunk["status"][f][:, k], int(chunk["n_selected"][f]),
                                              lambda name: chunk[name][f][:, k], prev[k], budget if budgets_named else None)
        except Exception as exc:                                                     # (results[:f] stand; frame f is not final)
            return out, carried, deg, used, best, f, exc
        for k in range(B):
            prev[k], carried[f] = row[k]
            for name in hp.RESULT_FIELDS:
                out[name][k, :, f] = prev[k][name]
            deg[k, :, f] = prev[k]["degenerate"]
        if not carried[f]:
            used[:, :, f], best[:, :, f] = chunk["used"][f].T, chunk["best"][f].T
    return out, carried, deg, used, best, F, None


def run_chunked(chunk, cuts):
    """The restatement over the chunk cut at ``cuts``, the carry handed on -> the per-chunk results."""
    from mvoscalerecovery_amd import height_pitch as hp
    F, Cn, B = chunk["status"].shape
    carry, parts, a = hp.eval_carry_record(Cn, B), [], 0
    for b in list(cuts) + [F]:
        r = cc.tail(cc.cut(chunk, a, b), carry)
        parts.append((a, b, r))
        carry, a = r["carry_out"], b
    return parts


def joined(parts, F, Cn, B):
    """The chunks' final frames as one call's arrays, up to the first chunk with an error."""
    out = {k: np.zeros((B, Cn, F)) for k in cc.FIELDS}
    carried, deg = np.zeros(F, bool), np.zeros((B, Cn, F), bool)
    used, best = np.zeros((B, Cn, F), np.int32), np.full((B, Cn, F), -1, np.int32)
    for a, b, r in parts:
        n = r["end"]
        if n:
            for k in cc.FIELDS:
                out[k][:, :, a:a + n] = r[k]
            deg[:, :, a:a + n], used[:, :, a:a + n], best[:, :, a:a + n] = r["degenerate"] != 0, r["used"], r["best"]
            carried[a:a + n] = r["carried"][:n] != 0
        if r["error"] >= 0:
            return out, carried, deg, used, best, a + n, r["error"]
    return out, carried, deg, used, best, F, -1


def same_bytes(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


SEQUENCE = ["fit", "carry", "carry", "carry", "deg", "carry", "fit", "deg", "carry", "carry", "fit"]


@pytest.mark.parametrize("Cn,B", C_B)
def test_restatement_is_the_hosts_loop_at_every_chunking(Cn, B):
    chunk = cc.chunk_of(SEQUENCE, Cn, B, seed=3)
    F = len(SEQUENCE)
    want = host_loop(chunk)
    assert want[6] is None and want[1].tolist() == [k == "carry" for k in SEQUENCE]
    whole = joined(run_chunked(chunk, []), F, Cn, B)
    for cuts in [[c] for c in range(1, F)] + [list(range(1, F))]:
        got = joined(run_chunked(chunk, cuts), F, Cn, B)
        for x, y, z in zip(got[:5], want[:5], whole[:5]):
            if isinstance(x, dict):
                assert all(same_bytes(x[k], y[k]) and same_bytes(x[k], z[k]) for k in x), cuts
            else:
                assert same_bytes(x, y) and same_bytes(x, z), cuts
        assert got[5:] == (F, -1)
    # a degenerate source: NaN height_t_mean, the other five copied
    assert np.isnan(whole[0]["height_t_mean"][0, 0, 5]) and whole[2][0, 0, 5] and whole[0]["ransac_height"][0, 0, 5] == chunk["ransac_height"][4, 0, 0]
    if B > 1:                                                                        # ... degenerate at one budget and not at another
        assert not whole[2][1, 0, 5] and np.isfinite(whole[0]["height_t_mean"][1, 0, 5])


ERRORS = [("singular", np.linalg.LinAlgError, cc.ERR_SINGULAR), ("mask", ValueError, cc.ERR_MASK), ("empty", ValueError, cc.ERR_EMPTY),
          (("nomodel", 0), ValueError, cc.ERR_NO_MODEL), (("nomodel", 1), ValueError, cc.ERR_NO_MODEL)]


@pytest.mark.parametrize("kind,exc,code", ERRORS, ids=lambda v: str(v) if not isinstance(v, type) else v.__name__)
def test_every_error_kind_is_the_hosts_exception(kind, exc, code):
    from mvoscalerecovery_amd import height_pitch as hp
    Cn, B = 3, 3
    kinds = ["fit", "carry", "fit" if kind == ("nomodel", 1) else "deg", kind, "fit", "carry"]   # (no-model at a later index: the frames before are clean)
    chunk = cc.chunk_of(kinds, Cn, B, seed=5)
    want = host_loop(chunk)
    assert isinstance(want[6], exc) and want[5] == 3
    for cuts in ([], [2], [3], [4], [1, 2, 3, 4, 5]):
        got = joined(run_chunked(chunk, cuts), len(kinds), Cn, B)
        k, bud, frame = hp.eval_tail_error(got[6])
        assert (k, got[5]) == (code, 3), cuts
        assert frame == 3 - max([0] + [c for c in cuts if c <= 3])                   # (the word names the chunk's frame)
        for x, y in zip(got[:5], want[:5]):
            if isinstance(x, dict):
                assert all(same_bytes(x[n][:, :, :3], y[n][:, :, :3]) for n in x)
            else:
                assert same_bytes(x[..., :3], y[..., :3])
        if code == cc.ERR_NO_MODEL:
            assert str(want[6]) == "frame 3: no sample of the RANSAC had an inlier at budget %d" % (10 * (bud + 1)) and bud == kind[1]
        # every chunk behind the error passes the halted record on and reports the upstream kind
        parts = run_chunked(chunk, cuts)
        at = [i for i, (_, _, r) in enumerate(parts) if r["error"] >= 0][0]
        for _, _, r in parts[at + 1:]:
            assert hp.eval_tail_error(r["error"])[0] == cc.ERR_UPSTREAM and r["end"] == 0
            assert hp.eval_carry_fields(r["carry_out"])[0]["halted"] == 1


def test_no_previous_and_unknown_status():
    from mvoscalerecovery_amd import height_pitch as hp
    chunk = cc.chunk_of(["carry", "fit"], 2, 2, seed=7)
    want = host_loop(chunk)
    assert isinstance(want[6], IndexError) and want[5] == 0
    assert str(want[6]) == "too many indices for array: array is 1-dimensional, but 2 were indexed"
    r = cc.tail(chunk, hp.eval_carry_record(2, 2))
    assert hp.eval_tail_error(r["error"]) == (cc.ERR_NO_PREVIOUS, 0, 0) and r["end"] == 0
    head, _ = hp.eval_carry_fields(r["carry_out"])
    assert head["halted"] == 1 and head["has_prev"] == 0
    # after a chunk of fitted frames the same chunk is fine: the source is the carry-in's
    first = cc.tail(cc.chunk_of(["fit", "deg"], 2, 2, seed=8), hp.eval_carry_record(2, 2))
    r = cc.tail(chunk, first["carry_out"])
    assert r["error"] == -1 and r["source"].tolist() == [-1, 1] and r["carried"].tolist() == [1, 0]
    # a status word the rules do not know
    r = cc.tail(cc.chunk_of(["fit", "status", "fit"], 2, 2, seed=9), hp.eval_carry_record(2, 2))
    assert hp.eval_tail_error(r["error"]) == (cc.ERR_STATUS, 0, 1) and r["end"] == 1
    # a carry record written for other numbers of cases and budgets halts the chunk
    r = cc.tail(chunk, hp.eval_carry_record(3, 2))
    assert hp.eval_tail_error(r["error"])[0] == cc.ERR_UPSTREAM and same_bytes(r["carry_out"], hp.eval_carry_record(2, 2, None, halted=True))


def test_carry_record_round_trips():
    from mvoscalerecovery_amd import height_pitch as hp
    rng = np.random.default_rng(2)
    for Cn, B in C_B + ((13, 5), (10, 16)):
        assert hp.eval_carry_bytes(Cn, B) % 16 == 0 and hp.eval_carry_bytes(Cn, B) >= 16 + 65 * Cn * B
        state = {k: rng.normal(size=(Cn, B)) for k in hp.EVAL_CARRY_VALUES}
        state["degenerate"] = rng.random((Cn, B)) < 0.5
        rec = hp.eval_carry_record(Cn, B, state, halted=True)
        assert rec.dtype == np.uint8 and len(rec) == hp.eval_carry_bytes(Cn, B)
        head, back = hp.eval_carry_fields(rec)
        assert (head["has_prev"], head["halted"], head["n_cases"], head["n_budgets"]) == (1, 1, Cn, B)
        assert all(same_bytes(back[k], state[k]) for k in state)
        assert same_bytes(hp.eval_carry_record(Cn, B, back, halted=True), rec)
        empty = hp.eval_carry_record(Cn, B)
        assert not empty[:8].any() and not empty[16:].any() and empty[8:16].view(np.int32).tolist() == [Cn, B]
    assert hp.eval_tail_error(-1) == (0, 0, -1) and hp.eval_tail_error(cc.error_word(4, 3, 513)) == (4, 3, 513)


def test_an_fma_would_change_the_pools_values():
    ests, pool = cc.fma_pool()
    assert len(pool) >= 64
    for sy, sz, n in pool:
        for e in ests:
            s, c = math.sin(e), math.cos(e)
            two = cc.two_products(sy, sz, s, c, n)
            assert two == (float(np.float64(sz) * np.float64(s) + np.float64(sy) * np.float64(c)) / n)
            assert two not in cc.fused(sy, sz, s, c, n)
    # and the restatement's carried value is the host rule's expression, bit for bit
    from mvoscalerecovery_amd import height_pitch as hp
    chunk = cc.chunk_of(["fit", "carry"], 4, 3, seed=1)
    r = cc.tail(chunk, hp.eval_carry_record(4, 3))
    want = (chunk["sum_z"][0] * chunk["prior"][1][2] + chunk["sum_y"][0] * chunk["prior"][1][3]) / chunk["n_inliers"][0].astype(np.float64)
    assert same_bytes(r["height_t_mean"][:, :, 1], want.T)


# ---- the public surface, without a device ----------------------------------------------------------------------------------------
def test_resident_belongs_to_the_device_triangulation():
    from mvoscalerecovery_amd import height_pitch as hp
    message = None
    for make in (lambda: hp.RansacEvaluation("plane", 8, resident=True), lambda: hp.RansacBudgetSweep("line", (4, 8), resident=True),
                 lambda: hp.RansacEvaluation("plane", 8, triangulation="scipy", resident=True)):
        with pytest.raises(ValueError, match="resident=True belongs to triangulation='gpu'") as info:
            make()
        message = message or str(info.value)
        assert str(info.value) == message == hp.RESIDENT_ERROR
    with pytest.raises(ValueError) as info:                                          # the estimator's text
        hp.HeightPitchEstimator(resident=True)
    assert str(info.value) == message
    assert hp.RansacEvaluation.resident is False and hp.RansacBudgetSweep.resident is False


@pytest.mark.parametrize("budget", [None, 20])
def test_error_kinds_map_to_the_scripts_exceptions(budget):
    """``hp_resident.frame_error`` — the resident paths' one mapping — gives, kind by kind, the type and text ``_eval_frame_rules``
    raises for the corresponding status word, spelled out here once more; kind 0 is no error."""
    from mvoscalerecovery_amd import _lib, height_pitch as hp
    from mvoscalerecovery_amd.hp_resident import frame_error
    at = "" if budget is None else " at budget 20"
    index_text = "too many indices for array: array is 1-dimensional, but 2 were indexed"
    cases = [(_lib.HPT_ERR_SINGULAR, hp.ST_ERR_SINGULAR, 0, np.linalg.LinAlgError, "Singular matrix"),
             (_lib.HPT_ERR_MASK, hp.ST_ERR_MASK, 0, ValueError, "frame 7: a triangle names a vertex outside the frame"),
             (_lib.HPT_ERR_EMPTY, hp.ST_ERR_EMPTY, 0, ValueError, "frame 7: no features or no triangles"),
             (_lib.HPT_ERR_NO_MODEL, hp.ST_RS_FEW, hp.MIN_POINTS, ValueError, "frame 7: no sample of the RANSAC had an inlier" + at),
             (_lib.HPT_ERR_NO_PREVIOUS, hp.ST_RS_FEW, hp.MIN_POINTS - 1, IndexError, index_text)]
    for kind, status, n_sel, exc, text in cases:
        got = frame_error(kind, 7, budget)
        assert type(got) is exc and str(got) == text, kind
        with pytest.raises(exc) as info:
            hp._eval_frame_rules(7, 0.0, np.array([0, status, 0]), n_sel, None, None, budget)
        assert type(info.value) is exc and str(info.value) == text, kind
    got = frame_error(_lib.HPT_ERR_STATUS, 7, budget)
    assert type(got) is RuntimeError and str(got) == "frame 7: the tail stopped with error 6"
    assert frame_error(0, 7, budget) is None
