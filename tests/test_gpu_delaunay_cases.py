"""The crafted cases of tests/delaunay_cases.py (sets that sit on the decline bands; classes computed on the CPU, in exact arithmetic)
through qhull_rows_kernel and delaunay_kernel, by packing.delaunay_gpu and the C ABI: SciPy's rows or DECLINED, never declined in
``must_accept``; delaunay_kernel's accepted rows pass the exact verifier and it declines every case in which SciPy's rows are not the
Delaunay triangulation; every instantiation the launcher picks gives the same rows.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import collections

import numpy as np
import pytest

import delaunay_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def case_table():
    """The class table (SciPy, the exact verifier, the margins and the host replay on every case: CPU work, done once per process) is
    built HERE, so that its seconds are this fixture's set-up and not the first test's."""
    import time
    t0 = time.perf_counter()
    table = dc.table()
    print("\nclass table of %d cases: %.1f s on the CPU" % (len(table), time.perf_counter() - t0))
    return table


def _table():
    return dc.table()


def _points():
    return [e.points for e in _table()]


def _canon(e):
    from mvoscalerecovery_amd import packing
    if not hasattr(e, "canon"):
        e.canon = packing.canonical_rows(e.scipy)
    return e.canon


def _run(gpu, sets, keeps=None, rows="canonical"):
    """packing.delaunay_gpu: (rows or None per set, status words, row counts)."""
    from mvoscalerecovery_amd import packing
    got = packing.delaunay_gpu(gpu, sets, keeps, rows=rows)
    st = np.array(packing.delaunay_gpu.last_status).copy()
    return got, st, np.array([0 if t is None else len(t) for t in got])


def _report(name, table, got, want_of):
    by = collections.defaultdict(lambda: [0, 0, 0])
    for e, t in zip(table, got):
        c = by[e.case.family]
        c[0 if t is not None else 1] += 1
        c[2] += int(t is not None and np.array_equal(t, want_of(e)))
    print("\n%s, per family (accepted, declined, rows equal to SciPy's):" % name, {k: tuple(v) for k, v in by.items()})


def _big(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, 1241, n), rng.uniform(186, 376, n)], axis=1)


# -------------------------------------------------------------------------------------------------------- qhull_rows_kernel

def _check_qhull(table, got, st, label):
    for e, t, s in zip(table, got, st):
        why = int(s) >> 8
        assert (t is None) == (int(s) != 0), (label, e.case, s)
        if t is not None:
            assert t.shape == e.scipy.shape and np.array_equal(t, e.scipy), (label, e.case)          # set, ORDER and ROTATION
        assert e.cls_replay != dc.MUST_ACCEPT or t is not None, (label, e.case, why)
        # one contract, two statements of it: the device replay decides what the host replay decides, for the same reason
        assert (t is None) == (e.host_rows is None), (label, e.case, "device", why, "host", e.host_reason)
        assert dc.DEVICE_REASON_KIND[why] == dc.HOST_REASON_KIND[e.host_reason], (label, e.case, "device", why, "host", e.host_reason)


def test_qhull_rows_kernel_on_the_crafted_cases(gpu):
    """mvosr_delaunay_qhull_batch on every case in one batch: declined, or SciPy's rows; never declined in must_accept; the decision
    and the reason are the host replay's (mvosr_qhull_rows_host), case by case.  The reason lists of the two files are numbered
    differently and the device has one name for every guard band: compared by the kind of decision (delaunay_cases.*_REASON_KIND)."""
    table = _table()
    got, st, _ = _run(gpu, _points(), rows="qhull")
    _report("qhull_rows_kernel", table, got, lambda e: e.scipy)
    _check_qhull(table, got, st, "16-bit facet ids")


def test_qhull_rows_kernel_wide_facet_ids_on_the_crafted_cases(gpu):
    """The launcher instantiates qhull_rows_kernel by the batch's max_pts: 32-bit facet ids above 8 000 points per frame.  The
    whole case list in a batch with one 8 200-site frame: the same rows, decisions and reasons."""
    from scipy.spatial import Delaunay
    table = _table()
    big = _big(31, 8200)
    got, st, _ = _run(gpu, [e.points for e in table] + [big], rows="qhull")
    assert got[-1] is not None and np.array_equal(got[-1], Delaunay(big).simplices)
    _check_qhull(table, got[:-1], st[:-1], "32-bit facet ids")


# ----------------------------------------------------------------------------------------------------------- delaunay_kernel

def _check_delaunay(entries, got, st, label, verify=True):
    """The class rules of delaunay_kernel on one launch's results."""
    for e, t, s in zip(entries, got, st):
        why = int(s) >> 8
        assert (t is None) == (int(s) != 0), (label, e.case, s)
        if t is not None:
            want = _canon(e)
            same = t.shape == want.shape and np.array_equal(t, want)
            if verify:
                # the SciPy-independent check, in exact arithmetic (rows equal to SciPy's canonical rows ARE that set of rows: its verdict)
                d = e.defects if same else dc.defects(e.points, t)
                assert d["clean"], (label, e.case, {k: d[k] for k in ("non_delaunay", "ties")}, d["structure"][:3], "cot_gap %.3g" % e.cot_gap)
            assert same, (label, e.case)
        assert e.cls != dc.MUST_ACCEPT or t is not None, (label, e.case, "declined, reason bits", why)
        assert e.cls != dc.SCIPY_NOT_DELAUNAY or t is None, (label, e.case, "accepted where SciPy's rows are not Delaunay; cot_gap %.3g" % e.cot_gap)
        if e.case.family == "hub":
            k, first = e.case.params["k"], e.case.params["first_id"]
            if e.beyond_limits:             # a star of more than kDtWaveDeg sites, or more than kDtWaveRows rows owned by the hub
                assert t is None and why & (dc.DT_WHY_DEGREE | dc.DT_WHY_ROWS), (label, e.case, why)
                if k <= dc.DT_WAVE_DEG:
                    assert why & dc.DT_WHY_ROWS and not why & dc.DT_WHY_DEGREE, (label, e.case, why)
                if not first:
                    assert why & dc.DT_WHY_DEGREE and not why & dc.DT_WHY_ROWS, (label, e.case, why)
            else:
                assert t is not None, (label, e.case, why)


def _same_results(a, b, label):
    (got_a, st_a, n_a), (got_b, st_b, n_b) = a, b
    assert np.array_equal(n_a, n_b), label
    assert np.array_equal(st_a & 0xFF, st_b & 0xFF), label
    for k, (x, y) in enumerate(zip(got_a, got_b)):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), (label, k)


@pytest.fixture(scope="module")
def eight_waves(gpu):
    """(c): the case list plus one 2 300-site frame in a launch of fewer than 512 frames — eight wavefronts per frame."""
    from scipy.spatial import Delaunay
    from mvoscalerecovery_amd import packing
    big = _big(32, 2300)
    table = _table()
    assert 128 < len(table) + 1 < 512
    got, st, cnt = _run(gpu, _points() + [big])
    assert got[-1] is not None and np.array_equal(got[-1], packing.canonical_rows(Delaunay(big).simplices))
    return got[:-1], st[:-1], cnt[:-1]


def test_delaunay_kernel_on_the_crafted_cases(gpu, eight_waves):
    """mvosr_delaunay_batch on every case: declined, or canonical_rows(SciPy) exactly; accepted rows pass the exact verifier;
    must_accept is never declined; a case whose SciPy rows are not the Delaunay triangulation is ALWAYS declined (a triangulator
    that returns the unique Delaunay set cannot equal SciPy there); hubs up to kDtWaveDeg / kDtWaveRows equal SciPy with either id
    placement and decline with DT_WHY_DEGREE / DT_WHY_ROWS beyond."""
    table = _table()
    got, st, _ = eight_waves
    _report("delaunay_kernel (eight wavefronts)", table, got, _canon)
    why = collections.Counter((e.case.family, int(s) >> 8) for e, s in zip(table, st) if s)
    print("declines by (family, reason bits):", dict(why))
    wrong = [(e.case.name, "%.2g" % e.cot_gap) for e, t in zip(table, got) if e.cls == dc.SCIPY_NOT_DELAUNAY and t is not None]
    print("accepted although SciPy's rows are not Delaunay: %d of %d" % (len(wrong), sum(e.cls == dc.SCIPY_NOT_DELAUNAY for e in table)), wrong)
    _check_delaunay(table, got, st, "eight wavefronts")


def test_delaunay_kernel_small_frame_ladder_on_the_crafted_cases(gpu, eight_waves):
    """(a): the list repeated to 512 frames and more — the launcher's ladder, two wavefronts per frame at these sizes: both copies
    give the rows, counts and status codes of the eight-wavefront launch, and obey the class rules."""
    table = _table()
    reps = -(-512 // len(table))
    got, st, cnt = _run(gpu, _points() * reps)
    assert len(got) >= 512 and max(len(p) for p in _points()) <= 500
    F = len(table)
    for r in range(reps):
        _same_results((got[r * F:(r + 1) * F], st[r * F:(r + 1) * F], cnt[r * F:(r + 1) * F]), eight_waves, "ladder copy %d" % r)
    _check_delaunay(table, got[:F], st[:F], "two wavefronts")


def test_delaunay_kernel_parts_variant_on_the_crafted_cases(gpu, eight_waves, monkeypatch):
    """(b): slices of 16 frames (each holds a frame of 256 sites and more) — several workgroups per frame, the PARTS variant — and
    the same slices as one workgroup per frame (MVOSR_DT_PARTS=0): the rows, counts and status codes of the eight-wavefront launch."""
    table, pts = _table(), _points()
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("MVOSR_DT_PARTS", raising=False)
        else:
            monkeypatch.setenv("MVOSR_DT_PARTS", env)
        got, st, cnt = [], [], []
        for lo in range(0, len(pts), 16):
            assert max(len(p) for p in pts[lo:lo + 16]) >= 256
            g, s, c = _run(gpu, pts[lo:lo + 16])
            got += g; st.append(s); cnt.append(c)
        st, cnt = np.concatenate(st), np.concatenate(cnt)
        _same_results((got, st, cnt), eight_waves, "slices of 16, MVOSR_DT_PARTS=%s" % env)
        _check_delaunay(table, got, st, "slices of 16, MVOSR_DT_PARTS=%s" % env, verify=env is None)
    monkeypatch.delenv("MVOSR_DT_PARTS", raising=False)


def test_delaunay_kernel_global_variant_on_three_rings(gpu):
    """(d): three ring cases — far outside every band; SciPy not Delaunay although no candidate pair is near the relative band; an
    exact tie — each embedded in a frame of mvosr_delaunay_lds_points() + 300 sites: the GLOBAL variant, same class rules."""
    n = int(gpu.lib.mvosr_delaunay_lds_points()) + 300
    entries = []
    for j, base in enumerate((dc.ring(4.0, 12, 1e-3, 0), dc.ring(0.05, 12, 1e-5, 1), dc.rect(0.0, 0))):
        rng = np.random.default_rng([99, j])
        crafted = base.points[base.crafted]
        centre = crafted.mean(axis=0)
        radius = float(np.hypot(*(crafted - centre).T).max())
        bg = dc._background(rng, n - len(crafted), centre, radius + 20.0)
        e = dc.classify(dc._assemble(rng, "ring", base.name + " in %d sites" % n, bg, crafted, **base.params))
        entries.append(e)
    assert [e.cls for e in entries] == [dc.MUST_ACCEPT, dc.SCIPY_NOT_DELAUNAY, dc.SCIPY_NOT_DELAUNAY], [(e.cls, e.defects, e.cot_gap) for e in entries]
    got, st, _ = _run(gpu, [e.points for e in entries])
    print("\ndelaunay_kernel (global-memory variant): statuses", [hex(int(s)) for s in st], "cot_gap", ["%.2g" % e.cot_gap for e in entries])
    _check_delaunay(entries, got, st, "global-memory variant")


def test_seeded_second_triangulation_on_the_unmask_cases(gpu):
    """The ``unmask`` cases — a first triangulation made harmless by one extra site, and a vote that takes that site out — through
    mvosr_delaunay_batch_seeded and mvosr_delaunay_batch_ex (info words, carried stars): the status and rows of the unseeded call on
    the survivors, under the class rules of the survivors' set; as five frames and repeated to 512 and more (the ladder)."""
    from mvoscalerecovery_amd import _lib
    entries = [e for e in _table() if e.case.family == "unmask"]
    assert len(entries) == 5
    lib = gpu.lib
    for reps in (1, 103):
        ent = entries * reps
        sets = [e.case.points for e in ent]
        F = len(sets)
        cnt = np.array([len(p) for p in sets], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
        uv = np.concatenate(sets)
        keep = np.concatenate([e.case.keep for e in ent]).astype(np.int32)
        d_u, d_v = gpu.to_device(np.ascontiguousarray(uv[:, 0])), gpu.to_device(np.ascontiguousarray(uv[:, 1]))
        d_off, d_cnt, d_toff, d_keep = gpu.to_device(off), gpu.to_device(cnt), gpu.to_device(2 * off), gpu.to_device(keep)
        rows, n_max = int(2 * cnt.sum()), int(cnt.max())
        tri1, tri1b, tri2, tri3, tri4 = (gpu.empty((rows, 3), np.int32) for _ in range(5))
        c1, c1b, c2, c3, c4, s1, s1b, s2, s3, s4, used = (gpu.zeros(F, np.int32) for _ in range(11))
        info = gpu.zeros(int(cnt.sum()), np.uint32)
        _lib.check(lib.mvosr_delaunay_batch(gpu.handle, F, d_off.ptr, d_cnt.ptr, d_u.ptr, d_v.ptr, None, n_max, d_toff.ptr,
                                            tri1.ptr, c1.ptr, None, s1.ptr), "first")
        _lib.check(lib.mvosr_delaunay_batch_seeded(gpu.handle, F, d_off.ptr, d_cnt.ptr, d_u.ptr, d_v.ptr, d_keep.ptr, n_max, d_toff.ptr,
                                                   tri2.ptr, c2.ptr, used.ptr, s2.ptr, d_toff.ptr, tri1.ptr, c1.ptr), "seeded")
        _lib.check(lib.mvosr_delaunay_batch(gpu.handle, F, d_off.ptr, d_cnt.ptr, d_u.ptr, d_v.ptr, d_keep.ptr, n_max, d_toff.ptr,
                                            tri3.ptr, c3.ptr, None, s3.ptr), "unseeded")
        _lib.check(lib.mvosr_delaunay_batch_ex(gpu.handle, F, d_off.ptr, d_cnt.ptr, d_u.ptr, d_v.ptr, None, n_max, d_toff.ptr,
                                               tri1b.ptr, c1b.ptr, None, s1b.ptr, None, None, None, None, info.ptr), "first + info")
        _lib.check(lib.mvosr_delaunay_batch_ex(gpu.handle, F, d_off.ptr, d_cnt.ptr, d_u.ptr, d_v.ptr, d_keep.ptr, n_max, d_toff.ptr,
                                               tri4.ptr, c4.ptr, None, s4.ptr, d_toff.ptr, tri1b.ptr, c1b.ptr, info.ptr, None), "seeded + carried stars")
        gpu.sync()
        t1, t1b, t2, t3, t4 = (x.download() for x in (tri1, tri1b, tri2, tri3, tri4))
        n1, n1b, n2, n3, n4 = (x.download() for x in (c1, c1b, c2, c3, c4))
        h1, h1b, h2, h3, h4, nu = (x.download() for x in (s1, s1b, s2, s3, s4, used))
        for b in (d_u, d_v, d_off, d_cnt, d_toff, d_keep, tri1, tri1b, tri2, tri3, tri4, c1, c1b, c2, c3, c4, s1, s1b, s2, s3, s4, used, info):
            b.free()
        assert np.array_equal(n1, n1b) and np.array_equal(h1, h1b)
        got = []
        for f, e in enumerate(ent):
            a = int(2 * off[f])
            assert np.array_equal(t1[a:a + n1[f]], t1b[a:a + n1b[f]]), (reps, f)
            full = e.case.points
            if h1[f] == 0:                                    # the first triangulation: every site, the extra one included
                want = dc.scipy_rows(full)
                from mvoscalerecovery_amd import packing
                assert np.array_equal(t1[a:a + n1[f]], packing.canonical_rows(want)), (reps, e.case)
            if e.case.params["of"] in ("ring", "rect", "wide"):
                assert h1[f] == 0, (reps, e.case, h1[f] >> 8)                     # made harmless by the site in the middle
            assert nu[f] == len(e.points), (reps, e.case)
            # (the code; the reason bits above it say which of a declined frame's failing tests fired, and a seeded walk meets them in another order)
            assert h2[f] & 0xFF == h3[f] & 0xFF == h4[f] & 0xFF and n2[f] == n3[f] == n4[f], (reps, e.case, h2[f], h3[f], h4[f])
            assert np.array_equal(t2[a:a + n2[f]], t3[a:a + n3[f]]) and np.array_equal(t4[a:a + n4[f]], t3[a:a + n3[f]]), (reps, e.case)
            got.append(np.ascontiguousarray(t3[a:a + n3[f]]) if h3[f] == 0 else None)
        if reps == 1:
            print("\nunmask (seeded = unseeded = carried stars): statuses", [hex(int(s)) for s in h3], [e.cls for e in ent])
        _check_delaunay(ent, got, h3, "unmask x %d" % reps, verify=reps == 1)
