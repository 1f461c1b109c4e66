"""CPU: the chunk pipeline of the repeated runs and the constant sweep without a device — the order in which ``stream.run`` starts and
collects the chunks of ``stream.fixed_plan``, what it frees when a step raises, the re-run of a chunk's declined frames scattered
into the chunk's results (``ScaleEstimator._rerun_declined``) and the merge of a refused frame into its cases
(``ScaleEstimator._merge_refused``).  Every expected value is written out here.
"""
import types

import numpy as np
import pytest

from mvoscalerecovery_amd import constants as K
from mvoscalerecovery_amd import stream
from mvoscalerecovery_amd.rescale import ScaleEstimator


def _recorded_run(F, step, depth, fail=None):
    """``stream.run`` over ``fixed_plan(F, step)`` with steps that only record: ``(events, freed chunk numbers, what run returned)``.
    ``fail``: ``("start" | "collect", chunk)`` raises there."""
    events, freed = [], []

    def start(a, b, tables, k):
        assert tables is None
        if fail == ("start", k):
            raise RuntimeError("start %d" % k)
        events.append(("start", a, b))
        return {"k": k}

    def collect(st, a, b, last):
        if fail == ("collect", st["k"]):
            raise RuntimeError("collect %d" % st["k"])
        events.append(("collect", a, b, last))
        return {"k": st["k"]}
    run = lambda: stream.run(stream.fixed_plan(F, step), start, collect, depth, lambda st: freed.append(st["k"]), [], lambda: None)
    if fail is None:
        return events, freed, run()
    with pytest.raises(RuntimeError, match="^%s %d$" % fail):
        run()
    return events, freed, None


def test_fixed_plan():
    assert list(stream.fixed_plan(0, 2)) == []
    assert list(stream.fixed_plan(4, 2)) == [(0, 2, None), (2, 4, None)]
    assert list(stream.fixed_plan(5, 2)) == [(0, 2, None), (2, 4, None), (4, 5, None)]


def test_chunk_order_one_ahead():
    events, freed, (bounds, states, results) = _recorded_run(5, 2, 1)
    assert events == [("start", 0, 2), ("start", 2, 4), ("collect", 0, 2, False), ("start", 4, 5), ("collect", 2, 4, False),
                      ("collect", 4, 5, True)]
    assert bounds == [(0, 2), (2, 4), (4, 5)] and [r["k"] for r in results] == [0, 1, 2] == [s["k"] for s in states] and freed == []


def test_chunk_order_depth_zero_alternates():
    events, freed, _ = _recorded_run(5, 2, 0)
    # (nothing is queued behind a chunk that is collected the moment it is started: ``last`` is not looked at here)
    assert [e[:3] for e in events] == [("start", 0, 2), ("collect", 0, 2), ("start", 2, 4), ("collect", 2, 4), ("start", 4, 5), ("collect", 4, 5)]
    assert freed == []


def test_collect_raises_every_state_is_freed():
    # chunk 1's collection raises: chunk 0 is collected, chunk 1 is being collected, chunk 2 is still queued
    events, freed, _ = _recorded_run(6, 2, 1, fail=("collect", 1))
    assert events == [("start", 0, 2), ("start", 2, 4), ("collect", 0, 2, False), ("start", 4, 6)]
    assert set(freed) == {0, 1, 2}


def test_start_raises_the_queued_chunk_is_freed():
    events, freed, _ = _recorded_run(6, 2, 1, fail=("start", 2))
    assert events == [("start", 0, 2), ("start", 2, 4), ("collect", 0, 2, False)]
    assert 1 in freed and 2 not in freed


def test_rerun_of_declined_frames_is_scattered():
    e = ValueError("frame 4")
    res = {"a": np.arange(6.0), "b": np.arange(18, dtype=np.int32).reshape(6, 3), "c": np.arange(36.0).reshape(6, 2, 3)}
    sub = {"a": np.array([-1.0, -2.0]), "b": np.array([[-1, -2, -3], [-4, -5, -6]], dtype=np.int32),
           "c": -np.arange(1.0, 13.0).reshape(2, 2, 3), "host_errors": {1: e}}
    s1, s2 = np.array([0, 3, 0, 0, 0, 0]), np.array([0, 0, 0, 0, 1, 0])
    f3s, f2s = ["p0", "p1", "p2", "p3", "p4", "p5"], ["q0", "q1", "q2", "q3", "q4", "q5"]
    calls = []

    def host_chunk(g3, g2, redo):
        calls.append((g3, g2, redo.tolist()))
        return sub
    me = types.SimpleNamespace(last_declined=5)
    out = ScaleEstimator._rerun_declined(me, res, s1, s2, f3s, f2s, host_chunk)
    assert out is res and me.last_declined == 7 and calls == [(["p1", "p4"], ["q1", "q4"], [1, 4])]
    assert res["a"].tolist() == [0.0, -1.0, 2.0, 3.0, -2.0, 5.0]
    assert res["b"].tolist() == [[0, 1, 2], [-1, -2, -3], [6, 7, 8], [9, 10, 11], [-4, -5, -6], [15, 16, 17]] and res["b"].dtype == np.int32
    want_c = np.arange(36.0).reshape(6, 2, 3)
    want_c[1] = [[-1.0, -2.0, -3.0], [-4.0, -5.0, -6.0]]
    want_c[4] = [[-7.0, -8.0, -9.0], [-10.0, -11.0, -12.0]]
    assert np.array_equal(res["c"], want_c)
    assert res["host_errors"] == {4: e}
    # nothing declined: the host chunk is not run
    res2 = {"a": np.arange(3.0)}
    ScaleEstimator._rerun_declined(me, res2, np.zeros(3, np.int32), np.zeros(3, np.int32), f3s[:3], f2s[:3], host_chunk)
    assert res2["a"].tolist() == [0.0, 1.0, 2.0] and res2["host_errors"] == {} and me.last_declined == 7 and len(calls) == 1


def _status():
    return np.array([0, K.ST_ERR_SINGULAR, K.ST_RS_FEW, K.ST_ERR_EMPTY, 0], dtype=np.int32)


def test_refused_frames_merge_into_the_cases_of_the_repeated_runs():
    F, Cn = 5, 2
    assert (K.ST_ERR_SINGULAR, K.ST_ERR_MASK, K.ST_ERR_EMPTY, K.ST_RS_FEW) == (7, 8, 9, 11)
    raw = np.arange(1.0, 11.0).reshape(F, Cn)
    model = np.arange(1.0, 41.0).reshape(F, Cn, 4)
    best, used = np.arange(1, 11, dtype=np.int32).reshape(F, Cn), np.arange(11, 21, dtype=np.int32).reshape(F, Cn)
    status = np.array([[0, 11], [0, 0], [11, 11], [0, 11], [0, 0]], dtype=np.int32)
    form = np.array([1, 2, 1, 2, 1], dtype=np.int32)
    ScaleEstimator._merge_refused(_status(), nan=(raw, model), zero=(best, used, form), take=(status,))
    nan = np.nan
    assert np.array_equal(raw, [[1.0, 2.0], [nan, nan], [5.0, 6.0], [nan, nan], [9.0, 10.0]], equal_nan=True)
    want_model = np.arange(1.0, 41.0).reshape(F, Cn, 4)
    want_model[1], want_model[3] = nan, nan
    assert np.array_equal(model, want_model, equal_nan=True) and np.isnan(model).sum() == 16
    assert best.tolist() == [[1, 2], [0, 0], [5, 6], [0, 0], [9, 10]] and used.tolist() == [[11, 12], [0, 0], [15, 16], [0, 0], [19, 20]]
    assert status.tolist() == [[0, 11], [7, 7], [11, 11], [9, 9], [0, 0]] and form.tolist() == [1, 0, 1, 0, 1]


def test_refused_frames_merge_into_the_cases_of_the_sweep():
    F, P, Cn = 5, 3, 2
    raw = np.arange(1.0, 31.0).reshape(F, P, Cn)
    status = np.zeros((F, P, Cn), dtype=np.int32)
    status[2] = 11
    status[0, 1, 1] = 11
    ScaleEstimator._merge_refused(_status(), nan=(raw,), take=(status,))
    want = np.arange(1.0, 31.0).reshape(F, P, Cn)
    want[1], want[3] = np.nan, np.nan
    assert np.array_equal(raw, want, equal_nan=True) and np.isnan(raw).sum() == 12
    assert status.tolist() == [[[0, 0], [0, 11], [0, 0]], [[7, 7]] * 3, [[11, 11]] * 3, [[9, 9]] * 3, [[0, 0]] * 3]


def test_collect_cases_refuses_through_the_merge():
    """``_collect_cases`` keeps its contract: the outputs' views downloaded as ``case_*``, refused frames merged."""
    arrays = {"raw_scale": np.array([[1.0, 2.0], [3.0, 4.0]]), "model": np.ones((2, 2, 4)), "best_ic": np.array([[5, 6], [7, 8]], dtype=np.int32),
              "used": np.array([[1, 1], [2, 2]], dtype=np.int32), "status": np.zeros((2, 2), dtype=np.int32), "count_form": np.array([1, 2], dtype=np.int32)}

    class Out:
        views = dict.fromkeys(arrays)

        def __getitem__(self, k):
            return types.SimpleNamespace(download=lambda: arrays[k].copy())
    res = ScaleEstimator._collect_cases({"status": np.array([K.ST_ERR_MASK, 0], dtype=np.int32)}, Out())
    assert set(res) == {"status"} | {"case_" + k for k in arrays}
    assert np.isnan(res["case_raw_scale"][0]).all() and res["case_raw_scale"][1].tolist() == [3.0, 4.0]
    assert np.isnan(res["case_model"][0]).all() and (res["case_model"][1] == 1.0).all()
    assert res["case_best_ic"].tolist() == [[0, 0], [7, 8]] and res["case_used"].tolist() == [[0, 0], [2, 2]]
    assert res["case_status"].tolist() == [[8, 8], [0, 0]] and res["case_count_form"].tolist() == [0, 2]
