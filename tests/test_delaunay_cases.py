"""tests/delaunay_cases.py on the CPU: the exact verifier against hand-damaged rows, the class table of the crafted cases, and
mvosr_qhull_rows_host (csrc/mvosr_qhull_host.c) on every case — SciPy's rows (set, order, rotation) or declined, never declined where
it must accept, always declined where SciPy's rows are not the Delaunay triangulation, and the same decision and reason as the
restatement in oracle/qhull_rows.py.  No GPU needed."""
import collections

import numpy as np
import pytest

import delaunay_cases as dc
from mvoscalerecovery_amd import packing


# ------------------------------------------------------------------------------------------------------------- the verifier

def _general(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, 1241, n), rng.uniform(186, 376, n)], axis=1)


def test_verifier_passes_scipy_rows_in_general_position():
    for seed, n in ((1, 5), (2, 40), (3, 300), (4, 777)):
        p = _general(seed, n)
        d = dc.defects(p, dc.scipy_rows(p))
        assert d["clean"] and d["structure"] == [] and d["non_delaunay"] == 0 and d["ties"] == 0, (n, d)
        assert d["clean"] == dc.defects(p, packing.canonical_rows(dc.scipy_rows(p)))["clean"]       # (any order, any rotation)


def test_verifier_reports_every_kind_of_damage():
    p = _general(7, 200)
    rows = dc.scipy_rows(p)
    # a flipped diagonal: rows (a, b, c), (b, a, d) over the interior edge a b become (a, d, c), (b, c, d)
    edges = collections.defaultdict(list)
    for r, t in enumerate(rows.tolist()):
        for k in range(3):
            edges[frozenset((t[k], t[(k + 1) % 3]))].append((r, t[(k + 2) % 3]))
    flipped = 0
    for e, owners in edges.items():
        if len(owners) != 2:
            continue
        (r1, c), (r2, d) = owners
        a, b = tuple(e)
        P = dc.exact_ints(p)
        if dc._orient(P[c], P[d], P[a]) * dc._orient(P[c], P[d], P[b]) >= 0:
            continue                                                  # (not a convex quadrilateral: no flip)
        bad = rows.copy()
        bad[r1], bad[r2] = (a, d, c), (b, c, d)
        got = dc.defects(p, bad)
        assert got["structure"] == [] and got["non_delaunay"] >= 1 and not got["clean"], (e, got)
        flipped += 1
        if flipped == 25:
            break
    assert flipped == 25
    got = dc.defects(p, np.delete(rows, 17, axis=0))                  # a dropped row
    assert got["structure"] and not got["clean"]
    got = dc.defects(p, np.concatenate([rows, rows[5:6]]))            # a duplicated row
    assert got["structure"] and not got["clean"]
    wrong = rows.copy()                                               # a row with a wrong id
    wrong[30, 1] = (wrong[30, 1] + 57) % len(p)
    got = dc.defects(p, wrong)
    assert not got["clean"] and (got["structure"] or got["non_delaunay"])
    wrong = rows.copy()
    wrong[30, 1] = len(p)                                             # ... and one out of range
    assert dc.defects(p, wrong)["structure"]
    # exact ties: the four corners of an integer rectangle, either diagonal
    q = np.concatenate([_general(8, 60) * [0.3, 0.3] + [700, 200], [[100.0, 200.0], [140.0, 200.0], [140.0, 230.0], [100.0, 230.0]]])
    got = dc.defects(q, dc.scipy_rows(q))
    assert got["structure"] == [] and got["ties"] == 1 and not got["clean"], got
    # exactly collinear sites on the hull are boundary vertices, as in Qhull's 'Qt' rows
    line = np.concatenate([_general(9, 80), np.stack([np.arange(0.0, 1000.0, 125.0), np.full(8, 100.0)], axis=1)])
    assert dc.defects(line, dc.scipy_rows(line))["clean"]


def test_margins():
    sq = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 3.0], [0.0, 3.0 + 3e-7], [2.0, -5.0], [9.0, 1.5], [2.0, 9.0], [-6.0, 1.0]])
    rows = dc.scipy_rows(sq)
    g = dc.cot_gap(sq, rows, np.arange(4))
    assert 1e-9 < g < 1e-6, g                                          # a corner 3e-7 px off the circle of the other three
    assert dc.cot_gap(sq, rows, np.arange(0)) == np.inf
    assert dc.collinear_margin(np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [5.0, 0.0]]), np.arange(4)) == 0.0
    assert dc.collinear_margin(np.array([[0.0, 0.0], [1.0, 1.0], [1.0, 1.0], [5.0, 0.0]]), np.arange(4)) == 0.0
    m = dc.collinear_margin(np.array([[0.0, 0.0], [10.0, 0.0], [5.0, 1e-6], [3.0, 7.0]]), np.arange(4))
    assert 1e-7 < m < 1e-6, m


# ---------------------------------------------------------------------------------------------------------------- the table

def test_case_list_and_classes():
    cases, table = dc.all_cases(), dc.table()
    assert len(cases) == len(table) == len({c.name for c in cases})
    assert all(120 <= len(c.points) <= 340 for c in cases), sorted({len(c.points) for c in cases})
    assert all(max(len(c.points) for c in cases[i:i + 16]) >= 256 for i in range(0, len(cases), 16))
    again = dc.ring(4.0, 12, 1e-7, 1, 130)
    assert np.array_equal(again.points, dc.ring(4.0, 12, 1e-7, 1, 130).points)            # seeded, deterministic
    rings = [e for e in table if e.case.family == "ring" and not e.case.params.get("rect")]
    assert sum(e.case.params["seed"] in (0, 1) for e in rings) == len(dc.RING_R) * len(dc.RING_K) * len(dc.EPS_LADDER) * 2
    assert len(rings) == len(dc.RING_R) * len(dc.RING_K) * len(dc.EPS_LADDER) * 2 + len(dc.RING_EXTRA) * len(dc.RING_EXTRA_SEEDS)
    for R in (40.0, 4.0):
        assert any(e.cls == dc.MUST_ACCEPT and e.cls_replay == dc.MUST_ACCEPT for e in rings if e.case.params["R"] == R), R
    rect0 = [e for e in table if e.case.params.get("rect") and e.case.params["eps"] == 0.0]
    assert rect0 and all(e.defects["ties"] == 1 and e.cls == dc.SCIPY_NOT_DELAUNAY for e in rect0)
    hubs = [e for e in table if e.case.family == "hub"]
    assert len(hubs) == 2 * len(dc.HUB_K)
    for e in hubs:
        k, pts = e.case.params["k"], e.points
        hub_id = 0 if e.case.params["first_id"] else len(pts) - 1
        assert (e.scipy == hub_id).any(axis=1).sum() == k, e.case                         # the star degree IS k
        owned = ((e.scipy.min(axis=1)) == hub_id).sum()
        assert owned == (k if e.case.params["first_id"] else 0), e.case
        assert e.cls_replay == dc.MUST_ACCEPT, (e.case, e.defects, e.cot_gap, e.col, e.host_reason)
        assert e.beyond_limits == (k > 60 or (e.case.params["first_id"] and k > 32))
        assert e.cls == (dc.FREE if e.beyond_limits else dc.MUST_ACCEPT), e.case
    outside = [e for e in table if e.cls == dc.SCIPY_NOT_DELAUNAY and e.cot_gap > 1e-8]
    assert len(outside) >= 20, len(outside)                          # SciPy is not Delaunay AND the kernel's relative band does not see it
    for fam in ("hull_line", "segment", "twins", "unmask"):
        assert any(e.case.family == fam for e in table)
    by = collections.Counter((e.case.family, e.cls) for e in table)
    print("\nclasses (delaunay_kernel):", dict(by), "\nSciPy not Delaunay with cot_gap > 1e-8:", len(outside))


# ----------------------------------------------------------------------------------------------------------- the host replay

def test_host_replay_on_every_case():
    """Declined, or SciPy's rows in set, order and rotation; never declined in must_accept (by construction of the class: pinned
    here for the families); ALWAYS declined where SciPy's rows hold a non-Delaunay edge."""
    acc = collections.Counter()
    for e in dc.table():
        if e.host_rows is not None:
            assert e.host_rows.dtype == np.int32 and np.array_equal(e.host_rows, e.scipy), e.case
        else:
            assert e.host_reason > 0, e.case
        if e.defects["non_delaunay"] > 0:
            assert e.host_rows is None, (e.case, e.defects)
        if e.host_rows is not None:
            assert e.defects["structure"] == [] and e.defects["non_delaunay"] == 0, (e.case, e.defects)
        acc[(e.case.family, "accepted" if e.host_rows is not None else "declined")] += 1
    print("\nhost replay:", dict(acc))
    # what the replay takes today at the large radii (everything from eps = 1e-7 up at R = 40)
    for e in dc.table():
        p = e.case.params
        if e.case.family == "ring" and not p.get("rect") and p["R"] == 40.0 and p["eps"] >= 1e-7:
            assert e.host_rows is not None, (e.case, e.host_reason)


def test_host_replay_and_oracle_take_the_same_decisions():
    from oracle.qhull_rows import Declined, QhullDelaunay2D
    for e in dc.table():
        try:
            want, why = QhullDelaunay2D(e.points).simplices(), None
        except Declined as exc:
            want, why = None, str(exc)
        assert (want is None) == (e.host_rows is None), (e.case, e.host_reason, why)
        if want is None:
            assert dc.HOST_REASON_TEXT[e.host_reason] == why, (e.case, e.host_reason, why)
        else:
            assert np.array_equal(want, e.host_rows), e.case
