"""flat_selection_kernel (csrc/mvosr_rescale.hip) on crafted frames: the median select's four exits, the even-count middle, the
strict keep rule, the three counting layouts of the RANSAC tail and the wavefront replay of ransac.py's rule — both
instantiations (mvosr_flat_selection_batch, mvosr_flat_ransac_batch), height_factor 0.9 and 1.0.  Needs a real MI355X.

Continuous part against mpmath (60 digits): tri_height within C_HEIGHT * kappa_inf(A) * 2^-53 relative.  Measured over every family
here, NumPy's float64 linalg.solve against mpmath reaches 0.93 of kappa * 2^-53 (tests/test_flat_select_cases.py measures it again);
C_HEIGHT = 4 * 0.93, rounded up = 3.75 (the kernel's pivot order and (a + b) + c sums are not LAPACK's).  Flags against the mpmath
pitch for every row further from -80 / -85 than that bound carried to degrees.  Discrete part exact, from the kernel's own heights.
The tail's inlier counts between np.longdouble bounds (flat_cases.count_bounds: eps derived there), then ransac.py's rule replayed
on the kernel's own counts.  Frames, references and launchers: tests/flat_cases.py.
"""
import numpy as np
import pytest

import flat_cases as fc

pytestmark = pytest.mark.gpu
HFS = (0.9, 1.0)
SEED = 5
PINNED = ("grid", "road_small", "road_dedup", "fan_dedup", "fan_packed", "keep_few", "keep_over_4096")   # planar frames: both count bounds coincide


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def frames(gpu):
    sel = fc.select_families()
    tail = fc.tail_families(fc.max_points(gpu))
    assert not set(sel) & set(tail)
    return sel, tail


@pytest.fixture(scope="module")
def runs(gpu, frames):
    """(name, hf) -> {"frame", "kframe", "stage", "dev", "devk", "fc"}: the stage form, the device-resident form without keep
    and with keep words (the same survivors behind -1 / 0 / 1), and the frame's counter in the sample sequence.  The select
    families go through as ONE batch per launch (neighbours of every kind in LDS before and after), the tail frames alone."""
    sel, tail = frames
    out = {}
    names = list(sel)
    kfr = {n: (sel[n].with_keep(100 + i, 37) if sel[n].keep is None else sel[n]) for i, n in enumerate(names)}
    for hf in HFS:
        st = fc.run_stage(gpu, [sel[n] for n in names], hf)
        dv = fc.run_dev(gpu, [sel[n] for n in names], hf, use_keep=False, seed=SEED)
        dk = fc.run_dev(gpu, [kfr[n] for n in names], hf, use_keep=True, seed=SEED)
        for i, n in enumerate(names):
            out[n, hf] = {"frame": sel[n], "kframe": kfr[n], "stage": st[i], "dev": dv[i], "devk": dk[i], "fc": i}
    for j, (n, f) in enumerate(tail.items()):
        kf = f if f.keep is not None else f.with_keep(200 + j, 150)
        for hf in HFS:
            out[n, hf] = {"frame": f, "kframe": kf, "stage": fc.run_stage(gpu, [f], hf)[0], "fc": 40 + j,
                          "dev": fc.run_dev(gpu, [f], hf, use_keep=False, seed=SEED, frame_base=40 + j)[0],
                          "devk": fc.run_dev(gpu, [kf], hf, use_keep=True, seed=SEED, frame_base=40 + j)[0]}
    return out


def test_heights_and_flags_against_mpmath(runs):
    """tri_height within C_HEIGHT kappa 2^-53 of the 60-digit solve, flag bits 0/1 equal to its verdict away from the thresholds;
    at most 2 % of a family's rows left out (50 % of the threshold family, both sides of both thresholds remaining)."""
    worst = 0.0
    for (name, hf), r in runs.items():
        f = r["frame"]
        h, pitch, kappa = fc.mp_rows(f)
        ok = ~f.skip
        bits, dec0, dec1 = fc.flag_reference(pitch[ok], kappa[ok])
        for form in ("stage", "dev", "devk"):
            hk, fl = r[form]["tri_height"][ok], r[form]["tri_flags"][ok]
            rel = np.abs(hk.astype(np.longdouble) - h[ok]) / np.abs(h[ok])
            ratio = (rel / (kappa[ok] * fc.U53)).astype(np.float64)
            worst = max(worst, float(ratio.max()))
            assert np.all(rel <= fc.height_bound(kappa[ok])), (name, hf, form, float(ratio.max()), int(np.argmax(ratio)))
            assert np.array_equal((fl & 1)[dec0], (bits & 1)[dec0]), (name, hf, form, "bit0")
            assert np.array_equal((fl & 2)[dec1], (bits & 2)[dec1]), (name, hf, form, "bit1")
        cap = 0.5 if name == "thresholds" else 0.02
        assert (~dec0).mean() <= cap and (~dec1).mean() <= cap, (name, (~dec0).sum(), (~dec1).sum())
        if name == "thresholds":
            assert {0, 1} <= set((bits & 1)[dec0].tolist()) and {0, 2} <= set((bits & 2)[dec1].tolist())
    print("largest |h_kernel - h_mpmath| / (|h| kappa 2^-53): %.3f (bound %.2f)" % (worst, fc.C_HEIGHT))


def test_select_coverage_from_the_kernels_heights(runs, frames):
    """Over the family set the select takes every exit, >= 2 and >= 5 passes, the direct ranking with 1, 2..63 and 64 candidates and
    with a tie on the rank — judged by select_plan on the kernel's OWN loose heights (they may differ from NumPy's by ulps)."""
    plans = {}
    for n in list(frames[0]) + list(frames[1]):
        s = runs[n, 0.9]["stage"]
        plans[n] = fc.select_plan(s["tri_height"][(s["tri_flags"] & 1) != 0])
        print("%-18s k %4d  %-7s passes %d  candidates %d%s" % (n, plans[n]["k"], plans[n]["exit"], plans[n]["passes"], plans[n]["cand"],
                                                                "  tie" if plans[n]["tie"] else ""))
    cov = fc.coverage(plans.values())
    assert not cov["missing"], cov
    ks = {p["k"] for p in plans.values()}
    assert {0, 1, 2, 3, 64, 65, 66} <= ks, sorted(ks)


def _check_discrete(name, hf, f, o, dev):
    hk, fl = o["tri_height"], o["tri_flags"]
    level, kept = fc.expected_discrete(hk, fl, hf)
    assert _same(np.float64(o["height_level"]), np.float64(level)), (name, hf, o["height_level"], level)
    assert np.array_equal((fl & 4) != 0, kept), (name, hf, np.nonzero(((fl & 4) != 0) != kept)[0][:8])
    assert o["n_kept"] == int(kept.sum()), (name, hf)
    assert not (fl & ~np.uint8(7)).any()
    assert np.isnan(hk[f.bad]).all() and not fl[f.bad].any(), (name, "rows with a bad id: height NaN, flags 0")
    if f.status:
        assert o["status"] == f.status, (name, hf, o["status"])
    else:
        assert o["status"] in ((0, fc.ST_RS_FEW) if dev else (0,)), (name, hf, o["status"])
    return level, kept


def test_level_and_kept_rows_exact(runs):
    """height_level == height_factor * np.median(own loose heights) bit for bit (NaN iff none is loose), kept == tight and
    height > level for every row, n_kept, status; and the strict '>': with height_factor 1.0 and an odd count of loose rows a tight
    row whose height EQUALS the level exists and is not kept."""
    on_level = set()
    for (name, hf), r in runs.items():
        for form in ("stage", "dev", "devk"):
            o = r[form]
            level, kept = _check_discrete(name, hf, r["frame"], o, form != "stage")
            loose = (o["tri_flags"] & 1) != 0
            assert np.isnan(level) == (not loose.any())
            if hf == 1.0 and loose.sum() % 2 == 1:
                eq = ((o["tri_flags"] & 2) != 0) & (o["tri_height"] == level)
                if eq.any():
                    assert not ((o["tri_flags"] & 4) != 0)[eq].any(), (name, form, "a height equal to the level is not above it")
                    on_level.add((name, form))
    for name in ("direct_tie", "direct63", "direct65", "k65", "k1"):           # odd counts whose median row is tight
        assert {(name, "stage"), (name, "dev"), (name, "devk")} <= on_level, (name, sorted(on_level))


def test_two_forms_agree_bit_for_bit(runs):
    for (name, hf), r in runs.items():
        for form in ("dev", "devk"):
            for k in ("tri_height", "tri_flags", "height_level", "n_kept"):
                assert _same(r["stage"][k], r[form][k]), (name, hf, form, k)
        for k in ("status", "hyp_counts", "best_ic", "used", "model", "raw_scale"):            # keep words change nothing but the load
            assert _same(r["dev"][k], r["devk"][k]), (name, hf, k)


def test_a_frame_alone_first_last_and_in_the_middle(gpu, runs, frames):
    """Alone, first, in the middle and last in a batch of different frames: the same outputs whatever else the launch holds
    (stale misc / ext / hist of a neighbour would show)."""
    sel = frames[0]
    others = [sel[n] for n in ("cluster200", "shift0", "k0", "one_row_x100")]
    for name in ("direct64", "direct_tie", "even_a", "even_c", "cluster300", "k1", "bad_ids", "singular"):
        f = sel[name]
        for pos, batch in [(0, [f])] + [(p, others[:p] + [f] + others[p:]) for p in range(len(others) + 1)]:
            st = fc.run_stage(gpu, batch, 1.0)[pos]
            dv = fc.run_dev(gpu, batch, 1.0, use_keep=False, seed=SEED, frame_ids=[900 + i if i != pos else runs[name, 1.0]["fc"]
                                                                                 for i in range(len(batch))])[pos]
            for k, v in runs[name, 1.0]["stage"].items():
                assert _same(st[k], v), (name, pos, "stage", k)
            for k, v in runs[name, 1.0]["dev"].items():
                assert _same(dv[k], v), (name, pos, "dev", k)


# ---- the tail ---------------------------------------------------------------------------------------------------------------
def _check_tail(name, f, o, triples_of, n_hyp, min_points=fc.MIN_POINTS, pinned=False):
    """`o`: one frame's outputs of the device-resident form; triples_of(list ids) -> (n_hyp, 3) vertex ids of the hypotheses."""
    P = f.survivors()
    L = fc.point_list(f, o["tri_flags"])
    M = len(L)
    assert M == 3 * o["n_kept"]
    nan4 = np.isnan(o["model"]).all()
    if f.status or M < min_points:
        assert o["status"] == (f.status or fc.ST_RS_FEW), (name, o["status"])
        assert nan4 and np.isnan(o["raw_scale"]) and o["best_ic"] == 0 and o["used"] == 0, name
        return None
    tr = np.asarray(triples_of(L)).reshape(n_hyp, 3)
    cnt = o["hyp_counts"]
    lo, hi = fc.count_bounds(P, L, tr)
    assert np.all((lo <= cnt) & (cnt <= hi)), (name, np.nonzero((cnt < lo) | (cnt > hi))[0][:8], cnt[:8], lo[:8], hi[:8])
    if pinned:
        assert np.array_equal(lo, hi), (name, "the crafted frame pins every count", np.nonzero(lo != hi)[0][:8])
    best, best_ic, used = fc.replay(cnt, M)
    assert (o["best_ic"], o["used"]) == (best_ic, used), (name, o["best_ic"], o["used"], best_ic, used)
    if best < 0:
        assert o["status"] == fc.ST_RS_FEW and nan4 and np.isnan(o["raw_scale"]), name
        return cnt
    assert o["status"] == 0, (name, o["status"])
    m, tol = fc.plane_ld(P, tr[best])
    tol = max(tol, 1e-12)
    got = o["model"].astype(np.longdouble)
    assert got[1] >= 0 and abs(float(np.sqrt(np.sum(got * got))) - 1.0) <= 1e-14, (name, o["model"])
    assert np.all(np.abs(got - m) <= tol), (name, best, o["model"], m.astype(np.float64), tol)
    raw = np.longdouble(fc.ABS_REF) * np.sqrt(np.sum(m[:3] ** 2)) / -m[3]
    rtol = tol / float(abs(m[3])) + tol / float(np.sqrt(np.sum(m[:3] ** 2))) + 1e-14
    assert abs(np.longdouble(o["raw_scale"]) - raw) <= rtol * abs(raw), (name, o["raw_scale"], float(raw))
    return cnt


def _drawn(seed, frame_counter, n_hyp):
    from oracle import rescale_oracle as ro
    return lambda L: L[ro.device_triples(seed, frame_counter, L, n_hyp)]


def test_tail_counts_and_replay_on_every_frame(runs):
    """Every frame's drawn hypotheses (oracle.rescale_oracle.device_triples for the seed and the frame's counter): counts between the
    np.longdouble bounds (pinned where the frame is planar), ransac.py's rule replayed on the kernel's counts, the model and
    raw_scale against the best hypothesis' plane.  The three counting layouts are all taken — by the source's conditions on the
    kernel's own kept rows."""
    layouts = {}
    for (name, hf), r in runs.items():
        f = r["frame"]
        for form, fr in (("dev", f), ("devk", r["kframe"])):
            o = r[form]
            _check_tail(name, fr, o, _drawn(SEED, r["fc"], 100), 100, pinned=name in PINNED)
        L = fc.point_list(f, r["dev"]["tri_flags"])
        if not f.status and len(L) >= fc.MIN_POINTS:
            layouts[name, hf] = fc.count_layout(len(L), len(f.survivors()), len(f.tri), len(np.unique(L)))
    for k in sorted(layouts):
        print("%-18s hf %.1f  %s" % (k[0], k[1], layouts[k]))
    assert set(layouts.values()) == {"list", "dedup", "packed"}, layouts
    assert layouts["road_packed", 0.9] == "packed" and layouts["road_dedup", 0.9] == "dedup" and layouts["control", 0.9] == "list"
    assert layouts["fan_dedup", 0.9] == "dedup" and layouts["fan_packed", 0.9] == "packed" and layouts["at_max_points", 0.9] == "packed"
    for name in ("fan_dedup", "fan_packed"):                            # the 16-bit multiplicity: one vertex on >= 300 kept rows
        L = fc.point_list(runs[name, 0.9]["frame"], runs[name, 0.9]["dev"]["tri_flags"])
        assert np.bincount(L).max() >= 300


def test_n_hyp_values_prefixes_and_frame_ids(gpu, frames):
    """n_hyp 1 .. 512 on one frame per layout: the same checks, counts that are prefixes of one another, and frame_ids[f] in the
    place of frame_base + f."""
    sel, tail = frames
    for name, f in (("grid", tail["grid"]), ("road_packed", tail["road_packed"]), ("k66", sel["k66"])):
        longest = None
        for H in sorted(fc.N_HYPS, reverse=True):
            a = fc.run_dev(gpu, [f], 0.9, n_hyp=H, use_keep=False, seed=SEED, frame_base=77)[0]
            b = fc.run_dev(gpu, [f, f], 0.9, n_hyp=H, use_keep=False, seed=SEED, frame_base=3, frame_ids=[77, 78])
            cnt = _check_tail(name, f, a, _drawn(SEED, 77, H), H, pinned=name in PINNED)
            _check_tail(name, f, b[1], _drawn(SEED, 78, H), H, pinned=name in PINNED)
            for k in a:
                assert _same(a[k], b[0][k]), (name, H, k)
            longest = cnt if longest is None else longest
            assert np.array_equal(cnt, longest[:H]), (name, H)


def _scenarios(f, L, H, pool_seed=81):
    """id_triples for the grid frame with list L: name -> (H, 3).  From a pool of vertex triples with pinned counts: `good` (count
    above the goal: three on-plane vertices), `bad` (below the goal, at least one lifted vertex), `zero` (one vertex twice)."""
    rng = np.random.default_rng(pool_seed)
    P, n = f.survivors(), len(f.survivors())
    on = np.setdiff1d(np.arange(n), f.off_plane)
    pool = np.array([[rng.choice(on), rng.choice(on), rng.choice(f.off_plane)] for _ in range(400)])
    pool = pool[(pool[:, 0] != pool[:, 1])]
    lo, hi = fc.count_bounds(P, L, pool)
    goal = len(L) * fc.GOAL
    sure = (lo == hi) & (hi < goal) & (lo > 0)
    pool, cnt = pool[sure], lo[sure]
    good = np.array([[on[0], on[5], on[17]], [on[3], on[40], on[21]]])
    glo, ghi = fc.count_bounds(P, L, good)
    assert np.all(glo == ghi) and np.all(glo > goal)
    # the largest count that two different planes of the pool share: the scenario's maximum, everything else below it
    top = None
    for v in np.unique(cnt)[::-1]:
        idx = np.nonzero(cnt == v)[0]
        pl = [fc.plane_ld(P, pool[i])[0] for i in idx]
        pair = [(i, j) for a, i in enumerate(idx) for b, j in enumerate(idx) if a < b and float(np.max(np.abs(pl[a] - pl[b]))) > 1e-6]
        if pair and (cnt < v).sum() >= 8:
            top = (v, pair[0])
            break
    assert top is not None
    low = pool[cnt < top[0]]
    filler = lambda k, src=None: (pool if src is None else src)[rng.integers(0, len(pool if src is None else src), k)]
    zero = np.array([[on[2], on[2], on[9]], [on[4], on[8], on[4]], [on[6], on[6], on[6]]])
    sc = {}
    for pos in sorted({0, 63, 64, 65, 128, H - 1}):
        if pos < H:
            t = filler(H)
            t[pos] = good[0]
            if pos + 1 < H:
                t[pos + 1:] = good[1]                       # (what follows the stop is never looked at, however good)
            if pos >= 3:
                t[1], t[2] = zero[0], zero[1]
            sc["stop_at_%d" % pos] = (t, pos + 1)
    sc["never"] = (filler(H), H)
    if H > 70:
        t = filler(H, low)
        t[5], t[70] = pool[top[1][0]], pool[top[1][1]]
        t[0], t[64] = zero[0], zero[2]
        sc["tie_across_rounds"] = (t, H)
    sc["all_zero"] = (zero[rng.integers(0, 3, H)], H)
    return sc


def test_id_triples_early_stop_ties_and_repeated_vertices(gpu, frames, runs):
    """With id_triples: the first count above the goal at hypothesis 0, 63, 64, 65, 128, the last one, and never; two hypotheses
    tying for the largest count in different 64-rounds (the earlier one is the model); triples that name one vertex twice (count 0,
    never the best); every hypothesis at zero (MVOSR_ST_RS_FEW)."""
    f = frames[1]["grid"]
    L = fc.point_list(f, runs["grid", 0.9]["dev"]["tri_flags"])
    seen = set()
    for H in fc.N_HYPS:
        sc = _scenarios(f, L, H)
        names = list(sc)
        outs = fc.run_dev(gpu, [f] * len(names), 0.9, n_hyp=H, use_keep=False, id_triples=[sc[n][0] for n in names], seed=SEED)
        for n, o in zip(names, outs):
            tr, used = sc[n]
            cnt = _check_tail("grid/%s/H%d" % (n, H), f, o, lambda _l, tr=tr: tr, H, pinned=True)
            assert o["used"] == used, (n, H, o["used"], used)
            rep = (tr[:, 0] == tr[:, 1]) | (tr[:, 0] == tr[:, 2]) | (tr[:, 1] == tr[:, 2])
            assert not cnt[rep].any()
            if n == "tie_across_rounds":
                assert cnt[5] == cnt[70] == cnt.max() == o["best_ic"]
                m5, tol = fc.plane_ld(f.survivors(), tr[5])
                assert np.all(np.abs(o["model"].astype(np.longdouble) - m5) <= max(tol, 1e-12)), "the first of two equal counts stays the best"
            if n == "all_zero":
                assert o["status"] == fc.ST_RS_FEW and o["best_ic"] == 0 and o["used"] == H
            seen.add(n)
    assert {"stop_at_0", "stop_at_63", "stop_at_64", "stop_at_65", "stop_at_128", "stop_at_511", "never", "tie_across_rounds", "all_zero"} <= seen


def test_too_few_list_entries(gpu):
    """MVOSR_ST_RS_FEW when the list is shorter than ransac_min_points: 9 and 12 entries against 12, 12 against 13."""
    four = fc.disjoint("four_kept", [(1.7, 0.0, 1)] * 4 + [(1.0, 0.0, 1)] * 3, 91)      # level 0.9 * 1.7: four rows kept
    three = fc.disjoint("three_kept", [(1.7, 0.0, 1)] * 3 + [(1.0, 0.0, 1)] * 2, 92)
    for f, mp, few in ((four, 12, False), (four, 13, True), (three, 12, True)):
        o = fc.run_dev(gpu, [f], 0.9, use_keep=False, seed=SEED, min_points=mp)[0]
        assert 3 * o["n_kept"] == (12 if f is four else 9)
        _check_discrete(f.name, 0.9, f, o, True)
        _check_tail(f.name, f, o, _drawn(SEED, 0, 100), 100, min_points=mp)
        assert (o["status"] == fc.ST_RS_FEW) == few, (f.name, mp, o["status"])


# ---- the vote's keep words ----------------------------------------------------------------------------------------------------
def test_graph_keep_words_on_crafted_frames(gpu):
    """mvosr_graph_keep_batch against oracle.rescale_oracle.graph_inliers and mvosr_graph_inliers_batch: equal v or z (products
    exactly 0, and -0.0 by underflow), all eight edge codes, a vertex on no row, exactly min_valid and min_valid + 1 passing
    features, a declined first triangulation."""
    from oracle import rescale_oracle as ro
    cases = fc.graph_cases()
    codes = set()
    for c in cases:
        codes |= set(ro.edge_code(c["v"], c["z"], c["tri"]).tolist())
    assert codes == set(range(8))
    got = fc.run_graph(gpu, cases, min_valid=10)
    kinds = set()
    for c, g in zip(cases, got):
        valid, good, total = ro.graph_inliers(c["v"], c["z"], c["tri"])
        assert np.array_equal(g["total"], total) and np.array_equal(g["good"], good), c["name"]
        if c["declined"]:
            assert (g["keep"] == -1).all() and g["n_valid"] == 0, c["name"]
            kinds.add("declined")
            continue
        nv = int(valid.sum())
        assert g["n_valid"] == nv, (c["name"], g["n_valid"], nv)
        want = np.where(valid, 1, -1 if nv > 10 else 0)
        assert np.array_equal(g["keep"], want), (c["name"], np.nonzero(g["keep"] != want)[0][:8])
        kinds.add("fail=-1" if nv > 10 else "fail=0")
        if (total == 0).any():
            assert not valid[total == 0].any()
            kinds.add("0/0")
        if c["name"].startswith("exactly"):
            kinds.add("nv=%d" % nv)
    assert {"declined", "fail=-1", "fail=0", "0/0", "nv=10", "nv=11"} <= kinds, kinds
