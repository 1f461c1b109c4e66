"""-m gpu: region_grow_kernel (mvosr_region_grow_batch) in both forms against tests/grow_cases.numpy_grow, the reference's own
run (tests/golden/grow.npz) through ``graph.GraphGrow``, and ``rescale.ScaleEstimator(region="grow")``."""
import numpy as np
import pytest

import flat_cases as fc
import grow_cases as gc

pytestmark = pytest.mark.gpu

GIVEN = sorted(gc.given_cases())
REFUSED = sorted(gc.refused_cases())
FIELDS = ("region", "label", "neighbors", "n_region", "n_flat", "status", "level", "threshold_height")


def _bytes(r, keys=FIELDS):
    return {k: np.ascontiguousarray(r[k]).tobytes() for k in keys}


def _same_bits(a, b):
    """Two doubles equal bit for bit, any NaN equal to any NaN."""
    a, b = np.float64(a), np.float64(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def _assert_discrete(got, want, what):
    assert int(got["status"]) == want["status"], what
    assert np.array_equal(got["region"] != 0, want["region"]), what
    assert set(np.unique(got["region"]).tolist()) <= {0, 1}, what
    assert np.array_equal(got["label"], want["label"]), what
    assert int(got["n_region"]) == want["n_region"] and int(got["n_flat"]) == want["n_flat"], what
    assert _same_bits(got["level"], want["level"]), (what, got["level"], want["level"])
    assert _same_bits(got["threshold_height"], want["threshold_height"]), (what, got["threshold_height"], want["threshold_height"])
    assert np.array_equal(np.sort(got["neighbors"], 1), np.sort(want["neighbors"], 1)), what       # per row, as sets


@pytest.fixture(scope="module")
def cases():
    c = dict(gc.given_cases())
    c.update(gc.refused_cases())
    return c


@pytest.fixture(scope="module")
def batch(gpu, cases):
    names = sorted(cases)
    return dict(zip(names, gc.run_given(gpu, [cases[n] for n in names])))


@pytest.fixture(scope="module")
def alone(gpu, cases):
    return {n: gc.run_given(gpu, [c])[0] for n, c in cases.items()}


@pytest.mark.parametrize("name", GIVEN + REFUSED)
def test_given_form_equals_numpy(name, cases, alone, batch):
    want = cases[name].expected()
    _assert_discrete(alone[name], want, name)
    assert _bytes(alone[name]) == _bytes(batch[name]), name                    # alone and inside the ragged batch


def test_given_form_repeated_launch_is_identical(gpu, cases, batch):
    names = sorted(cases)
    again = gc.run_given(gpu, [cases[n] for n in names])
    for n, r in zip(names, again):
        assert _bytes(r) == _bytes(batch[n]), n


def test_shuffled_rows_map_the_region_through_the_permutation(gpu, cases, alone):
    c = cases["holes"]
    want = c.expected()
    sizes = np.bincount(want["label"])
    seeded = np.unique(want["label"][(c.ang < gc.SEED_DEG) & (1 / c.h < want["level"])])
    top = np.sort(sizes[seeded])[::-1]
    assert len(top) >= 2 and top[0] > top[1], "the case must be free of ties"
    shuffled, perm = c.permuted(5)
    got = gc.run_given(gpu, [shuffled])[0]
    assert np.array_equal(got["region"], alone["holes"]["region"][perm])
    assert int(got["n_region"]) == int(alone["holes"]["n_region"]) > 1
    _assert_discrete(got, shuffled.expected(), "holes+shuffled")


@pytest.mark.parametrize("limit", ["max_tri", "max_feat"])
def test_refused_frames_leave_their_rows_untouched(gpu, cases, limit):
    """The header contract: a frame beyond max_feat or max_tri, and a frame without rows, get their per-frame values and
    nothing else; guard elements behind every output stay as they were."""
    names = ["strip63", "strip65", "no_rows", "ramp7"]
    cs = [cases[n] for n in names]
    kw = {"max_tri": 64} if limit == "max_tri" else {"max_feat": 66}            # strip65: 65 rows over 67 vertices
    res, tails = gc.run_given(gpu, cs, sentinel=0xA5, **kw)
    for k, t in tails.items():
        assert len(np.ravel(t)) >= 1 and fc.all_bytes(t, 0xA5), k
    for n, c, r in zip(names, cs, res):
        if n in ("strip65", "no_rows"):
            assert int(r["status"]) == (gc.ST_MASK if n == "strip65" else gc.ST_EMPTY), n
            assert np.isnan(r["level"]) and np.isnan(r["threshold_height"]) and int(r["n_region"]) == 0 and int(r["n_flat"]) == 0, n
            for k in ("region", "label", "neighbors"):
                assert fc.all_bytes(r[k], 0xA5), (n, k)
        else:
            _assert_discrete(r, c.expected(), n)


# ---- the from-points form ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def families():
    fam = dict(fc.select_families())
    fam["grid"] = fc.grid_frame()
    fam["road_small"] = fc.road_frame("road_small", 20, 0, 63, n_in=2, n_out=2)
    return fam


@pytest.fixture(scope="module")
def family_runs(gpu, families):
    names = sorted(families)
    frames = [families[n] for n in names]
    return dict(zip(names, zip(gc.run_points(gpu, frames), fc.run_stage(gpu, frames))))


@pytest.fixture(scope="module")
def real():
    out = {}
    for n in (300, 2000):
        xyz, rows, d = gc.synth_rows(0, n)
        out[n] = (fc.Frame("synth%d" % n, xyz, rows), d)
    return out


@pytest.fixture(scope="module")
def real_runs(gpu, real):
    frames = [real[n][0] for n in (300, 2000)]
    return dict(zip((300, 2000), zip(gc.run_points(gpu, frames), fc.run_stage(gpu, frames))))


def _assert_points_discrete(fr, got, what):
    if int(got["status"]) == gc.ST_SINGULAR or fr.status == gc.ST_SINGULAR:
        assert int(got["status"]) == fr.status == gc.ST_SINGULAR, what
        assert not got["region"].any() and int(got["n_region"]) == 0 and int(got["n_flat"]) == 0 and np.isnan(got["level"]), what
        return
    want = gc.numpy_grow(fr.tri, got["tri_height"], got["tri_angle"], n_feat=len(fr.survivors()))     # on the kernel's own values
    assert want["status"] == fr.status or (fr.status == 0 and want["status"] == gc.ST_MASK), what     # (repeated rows: an edge on > 2 rows)
    _assert_discrete(got, want, what)


@pytest.mark.parametrize("name", sorted(list(fc.select_families()) + ["grid", "road_small"]))
def test_from_points_on_the_flat_families(name, families, family_runs):
    fr = families[name]
    got, stage = family_runs[name]
    _assert_continuous(fr, got, stage, name)
    _assert_points_discrete(fr, got, name)


def _assert_continuous(fr, got, stage, name):
    assert got["tri_height"].tobytes() == stage["tri_height"].tobytes(), name              # flat_selection's own heights
    _, pitch, kappa = fc.mp_rows(fr)
    ok = ~fr.skip
    L = np.longdouble
    deg = L(180) / (np.arctan(L(1)) * 4)
    mu = np.sin(pitch[ok].astype(L) / deg)
    eps = 2.0 * fc.height_bound(kappa[ok])
    lo = np.arcsin(np.maximum(mu - eps, L(-1))) * deg - L(1e-12)
    hi = np.arcsin(np.minimum(mu + eps, L(1))) * deg + L(1e-12)
    ang = got["tri_angle"][ok].astype(L)
    assert ((ang >= lo) & (ang <= hi)).all(), (name, float(np.max(np.maximum(lo - ang, ang - hi))))
    assert np.isnan(got["tri_angle"][fr.bad]).all() and np.isnan(got["tri_height"][fr.bad]).all()
    bits, dec0, dec1 = fc.flag_reference(pitch[ok], kappa[ok])
    a = got["tri_angle"][ok]
    fl = stage["tri_flags"][ok]
    assert np.array_equal((a < gc.LEVEL_DEG)[dec0], (fl[dec0] & 1) != 0) and np.array_equal((a < gc.SEED_DEG)[dec1], (fl[dec1] & 2) != 0), name
    assert np.array_equal((a < gc.LEVEL_DEG)[dec0], (bits[dec0] & 1) != 0) and np.array_equal((a < gc.SEED_DEG)[dec1], (bits[dec1] & 2) != 0), name


@pytest.mark.parametrize("n", [300, 2000])
def test_from_points_on_real_triangulations(n, real, real_runs):
    fr, d = real[n]
    got, stage = real_runs[n]
    _assert_continuous(fr, got, stage, "synth%d" % n)
    _assert_points_discrete(fr, got, "synth%d" % n)
    assert int(got["status"]) == 0 and int(got["n_region"]) > len(fr.tri) // 10
    assert np.array_equal(np.sort(got["neighbors"], 1), np.sort(d.neighbors, 1))           # SciPy's own adjacency, per row as sets
    assert (got["neighbors"] >= 0).sum(1).max() == 3


def test_from_points_refuses_oversized_frames_untouched(gpu, real):
    fr = real[300][0]
    small = fc.grid_frame()
    res, tails = gc.run_points(gpu, [small, fr, small], max_feat=len(small.xyz), max_tri=len(small.tri), sentinel=0x5A)
    for k, t in tails.items():
        assert fc.all_bytes(t, 0x5A), k
    assert int(res[1]["status"]) == gc.ST_MASK and np.isnan(res[1]["level"]) and int(res[1]["n_region"]) == 0
    for k in ("region", "label", "neighbors", "tri_height", "tri_angle"):
        assert fc.all_bytes(res[1][k], 0x5A), k
    assert _bytes(res[0]) == _bytes(res[2]) and int(res[0]["status"]) == 0


# ---- the class and the estimator -----------------------------------------------------------------------------------------------
def test_graph_grow_equals_the_reference_run(gpu):
    from mvoscalerecovery_amd.graph import GraphGrow
    frames = gc.golden_frames()
    g = GraphGrow(ctx=gpu)
    for d in frames:
        rows = g.process(d["rows"], d["heights"], d["angles"])
        assert isinstance(rows, list) and rows == d["region"].tolist()
        assert g.threshold_height == float(d["threshold_height"])                      # graph.py:93
        assert int(g.last["n_flat"][0]) > 0 and len(g.last["label"][0]) == len(d["rows"])
    many = g.process_batch([d["rows"] for d in frames], [d["heights"] for d in frames], [d["angles"] for d in frames])
    assert many == [d["region"].tolist() for d in frames]
    d = frames[0]
    assert g.process(d["rows"], d["heights"], np.full(len(d["rows"]), -70.0)) == []   # nothing flat: graph.py:95-96
    with pytest.raises(ValueError, match="frame 1"):
        g.process_batch([d["rows"], np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]])], [d["heights"], np.ones(3)], [d["angles"], np.full(3, -88.0)])


def test_estimator_with_region_grow(gpu):
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    frames = [synth.synth_frame(i, 300, base_seed=1234) for i in range(3)]
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    kw = dict(triangulation="scipy", sampling="host", ransac_seed=1, delaunay_workers=0)
    est = ScaleEstimator(1.75, 5, region="grow", **kw)
    sel = est.feature_selection_batch(f3s, f2s)
    grow, pf2 = est.last["grow"], est.last["pf2"]
    for f in range(3):
        low3 = f3s[f][f2s[f][:, 1] > 185]
        valid = est.last["valid"][f]
        if valid.sum() > 10:
            low3 = low3[valid]
        t0, t1 = int(pf2.tri2_off[f]), int(pf2.tri2_off[f + 1])
        tri = est.last["tris2"][f]
        want = gc.numpy_grow(tri, grow["tri_height"][t0:t1], grow["tri_angle"][t0:t1], n_feat=len(low3))
        assert want["status"] == 0 and want["n_region"] > 50
        assert np.array_equal(sel[f][0], low3[tri[want["region"]].reshape(-1)]), f
    s, _ = est.scale_calculation_batch(f3s, f2s)
    assert np.isfinite(s).all()
    # the default selection is what it was: the keyword's default and its absence
    a = ScaleEstimator(1.75, 5, region="threshold", **kw)
    b = ScaleEstimator(1.75, 5, **kw)
    for x, y in zip(a.feature_selection_batch(f3s, f2s), b.feature_selection_batch(f3s, f2s)):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    sa, sb = a.scale_calculation_batch(f3s, f2s), b.scale_calculation_batch(f3s, f2s)
    assert np.asarray(sa[0]).tobytes() == np.asarray(sb[0]).tobytes()
