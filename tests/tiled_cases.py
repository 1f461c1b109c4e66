"""Crafted multi-tile frames for scale_frames_tiled_kernel (csrc/mvosr_kernels.hip) — shared by
tests/test_tiled_cases.py (CPU) and tests/test_gpu_tiled_cases.py.  Test infrastructure.

A frame is a scale_cases.Case whose image column is the feature index (the pixel rows span less), so that packing.apply_tile_order
leaves feature i at tile position i and a row's place in the walk — the tile of its smallest vertex, or the far list — is what the
builder wrote.  Selection-side frames have every feature on pixel row scale_cases.V_ROW (nobody is flagged); vote-side frames use the
anti-diagonal of scale_cases.compaction_case at half its pitch.  y' are multiples of a power of two wherever a height has to land
somewhere exactly: the kernel's 3h = (y0 + y1) + y2 and its level are then exact, and so are the oracle's h and level.

`info` of every case: far1 / far2 (far rows per triangulation), far_tiles (the tiles their vertices lie in), wave_cands (candidates
per wavefront: group g of 64 features is retired by wavefront g mod 8), redo (why the HOT kernel hands the frame over, or None).
Every case is order-free (`order_free`, asserted where it is built): the tiled layout gives the road model its list in
wavefront-list order, and a status that hangs on the last bits of the skew would depend on that order.

`model` is a NumPy restatement of the kernel's selection rule with switches for the ways it could be subtly wrong.
"""
import numpy as np

import scale_cases as sc
from oracle import scale_oracle as so

W = 512                            # kTileW
DW = 8                             # kTiledWaves
PEND_CAP, PEND_CAP_H = 1024, 576   # kPendCap, kPendCapH (entries: three per far row)
LEVEL_GUARD = 1e-12                # kLevelGuard
WALK_SIZES = (511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2049, 3073)
LIST_G = (8, 17, 26, 11, 20, 29, 14, 23)       # g mod 8 = 0 .. 7
LIST_R = (0, 1, 63)
LIST_LARGE = (32256, 32768, 32769, 33280)
LIST_PATTERNS = ("all", "every_other_group", "wave5_none")
L0 = 1.5                           # the level of most selection-side frames
HIGH = 2.0625                      # a flat height well above it (three vertices in one histogram bin)


# ============================================================================================================================
# what a case contains
# ============================================================================================================================
def is_far(rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return rows.max(axis=1) >= (rows.min(axis=1) // W + 2) * W            # packing._tile_sort's rule, restated


def feature_rows(c):
    """tri2 numbered over the frame's features, in the oracle's row order (the fixed vote mode puts the rows in canonical form)."""
    r = c.oracle()
    return np.nonzero(np.asarray(r.valid))[0][np.asarray(r.tri2, dtype=np.int64).reshape(-1, 3)]


def wave_candidates(c):
    """Candidates (features with a flat row of finite height) per wavefront, from the oracle's valid_pitch rows."""
    s = c.oracle().sel
    cand = np.zeros(c.n, dtype=bool)
    cand[feature_rows(c)[s.valid_pitch & ~np.isnan(s.heights)].reshape(-1)] = True
    return np.bincount((np.nonzero(cand)[0] // 64) % DW, minlength=DW)


def order_free(c):
    """The oracle's status is decided without the skew, or the skew is at least 0.01 from its threshold."""
    r = c.oracle()
    if r.road is None or r.road.status not in (so.ST_MODE, so.ST_RIGHT):
        return True
    return abs(r.road.skew - so.SKEW_THRESHOLD) >= 0.01


def _finish(c, redo=None):
    f1, f2 = is_far(c.tri1), is_far(feature_rows(c))
    far_v = np.concatenate([c.tri1[f1].reshape(-1), feature_rows(c)[f2].reshape(-1)])
    singular = c.oracle().status == so.ST_ERR_SINGULAR
    c.info.update(far1=int(f1.sum()), far2=int(f2.sum()), far_tiles=sorted(set((far_v // W).tolist())),
                  wave_cands=None if singular else wave_candidates(c).tolist(), redo=redo)
    assert order_free(c), (c.name, c.oracle().road.skew)
    return c


# ============================================================================================================================
# the builder
# ============================================================================================================================
class Strip:
    """n features at tile positions 0 .. n-1.  Selection side: every pixel row V_ROW, (x, z) on a circle such that three consecutive
    features are the corners of an equilateral triangle.  Vote side: (v, z') = (t, Z0 - t) with t = 200 + i / 2, nobody flagged
    except the pairs made by `drop_pair`."""

    def __init__(self, n, vote_side=False):
        i = np.arange(n, dtype=np.float64)
        ang = (2.0 * np.pi / 3.0 + 1.0 / 1024.0) * i
        self.n, self.vote_side = n, vote_side
        self.x, self.y = 400.0 * np.cos(ang), np.full(n, 0.25)
        if vote_side:
            self.v, self.z = 200.0 + i / 2, 10000.0 - (200.0 + i / 2)
        else:
            self.v, self.z = np.full(n, sc.V_ROW), 1000.0 + 400.0 * np.sin(ang)
        self.rows1, self.rows2, self._placed = [], [], 0

    def place(self, ids):
        """Give three features that are not neighbours the corners of an equilateral triangle (vote side: x alone; z is the vote's)."""
        a = 2.0 * np.pi * np.arange(3) / 3.0 + 0.37 * self._placed
        self._placed += 1
        self.x[list(ids)] = 400.0 * np.cos(a)
        if not self.vote_side:
            self.z[list(ids)] = 1000.0 + 400.0 * np.sin(a)

    def flat(self, ids, ys=None, place=True):
        """A tri2 row on the plane y = const (pitch -90 deg) when the three y' are equal, and within a degree of it otherwise."""
        if place:
            self.place(ids)
        if ys is not None:
            self.y[list(ids)] = ys
        self.rows2.append(list(ids))

    def wall(self, ids, H, d=1.0):
        """A steep tri2 row on the plane x = const (pitch 0) of height exactly H: y' = (H - d, H, H + d)."""
        k = len(self.rows2)
        self.x[list(ids)] = 3.0 + k / 64.0
        if not self.vote_side:
            self.z[list(ids)] = (5.0 + k, 6.0 + k, 5.0 + k)
        self.y[list(ids)] = (H - d, H, H + d)
        self.rows2.append(list(ids))

    def drop_pair(self, d1, d2):
        """Move d2 next to d1: (dv)(dz') = 1/64 > 0 for this pair alone, so that a row (k, d1, d2) flags d1 and d2 and not k."""
        assert self.vote_side
        self.v[d2], self.z[d2] = self.v[d1] + 0.125, self.z[d1] + 0.125

    def case(self, name, vote="reference", redo=None, **info):
        n = self.n
        rows1 = np.array(self.rows1 if self.rows1 else [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(n // 3)], dtype=np.int64)
        valid = so.outlier_votes(self.v, self.z, rows1, vote) >= 0
        rows2 = np.array(self.rows2, dtype=np.int64)
        assert valid[rows2].all(), name
        f3 = np.column_stack([self.x, self.y, self.z])
        f2 = np.column_stack([np.arange(n, dtype=np.float64), self.v])
        return _finish(sc.Case(name, f3, f2, rows1, (np.cumsum(valid) - 1)[rows2], vote, **info), redo)


def _survivor_strip_rows(s, rng, vote):
    """Vote side: y' distinct multiples of 2^-15 as in compaction_case, tri2 = rows (j, j+1, j+2) over the survivors."""
    n = s.n
    s.y = 1.5 + rng.permutation(n) / 32768.0 + np.where(rng.random(n) < 0.3, rng.integers(1, 5, n) / 2.0, 0.0)
    keep = np.nonzero(so.outlier_votes(s.v, s.z, np.array(s.rows1), vote) >= 0)[0]
    s.rows2 = [[keep[j], keep[j + 1], keep[j + 2]] for j in range(len(keep) - 2)]


# ============================================================================================================================
# 1. walk and ring
# ============================================================================================================================
def walk_mask(n):
    """Survivors: everyone but two features on either side of every tile boundary (the boundary's own two neighbours stay: the
    extreme rows stand on them) and two in the middle of the last tile."""
    keep = np.ones(n, dtype=bool)
    for b in range(W, n, W):
        for d in (b - 3, b - 2, b + 1, b + 2):
            if d < n:
                keep[d] = False
    s = (n - 1) // W * W
    if n - s >= 12:
        keep[s + (n - s) // 2], keep[s + (n - s) // 2 + 1] = False, False
    return keep


def _extreme_ks(n, one_further):
    """k = 0, a middle k and the last k for which the row (last feature of tile k, ., (k+2) 512 - 1 [+ 1]) exists."""
    last = (n - int(one_further)) // W - 2                                # (k + 2) W - 1 + one_further <= n - 1
    return sorted({k for k in (0, last // 2, last) if 0 <= k <= last})


def walk_case(n, vote="reference"):
    keep = walk_mask(n)
    base = sc.compaction_case("walk/n%d%s" % (n, "" if vote == "reference" else "/" + vote), keep, seed=7)
    f3, f2 = base.f3.copy(), base.f2.copy()
    f2[:, 1], f3[:, 2] = f2[:, 1] / 2, f3[:, 2] / 2                       # (half the pitch: the image column spans more than the rows)
    cum = np.cumsum(keep) - 1
    extra = []
    for further in (False, True):
        for k in _extreme_ks(n, further):
            lo, hi = k * W + W - 1, (k + 2) * W - 1 + int(further)
            mids = (k + 1) * W + 64 + np.arange(384)
            mids = mids[keep[mids]]
            area = np.abs((f3[mids, 0] - f3[lo, 0]) * (f3[hi, 2] - f3[lo, 2]) - (f3[hi, 0] - f3[lo, 0]) * (f3[mids, 2] - f3[lo, 2]))
            extra.append((lo, int(mids[np.argmax(area)]), hi, further))
    rows = np.array([e[:3] for e in extra], dtype=np.int64).reshape(-1, 3)
    assert keep[rows].all()
    tri1 = np.concatenate([base.tri1, rows])
    tri2 = np.concatenate([base.tri2, cum[rows]])
    c = sc.Case(base.name, f3, f2, tri1, tri2, vote, keep=keep, extreme=[e[:3] for e in extra if not e[3]], one_further=[e[:3] for e in extra if e[3]])
    return _finish(c)


def walk_cases():
    return [walk_case(n) for n in WALK_SIZES]


WALK_SIZES_FIXED = (1025, 1537, 3073)


def walk_cases_fixed():
    """Three of the sizes in the order-invariant vote mode (the masks hold in both modes)."""
    return [walk_case(n, "fixed") for n in WALK_SIZES_FIXED]


# ============================================================================================================================
# 2. far rows and the pending lists (2560 features: tiles 0 .. 4)
# ============================================================================================================================
N_FAR = 2560


def far_votes_case(vote):
    """100, 101: one near row takes them to 0, one far row (its third vertex in the last tile) to -1 — dropped through the pending
    list alone.  600, 601: three near rows take them to -2; two far rows (vertices in tiles 2 and 4) bring 600 back to 0 — kept
    through the pending list alone."""
    s = Strip(N_FAR, vote_side=True)
    s.drop_pair(100, 101)
    s.drop_pair(600, 601)
    s.rows1 = [[50, 100, 101], [2100, 100, 101], [550, 600, 601], [560, 600, 601], [570, 600, 601], [600, 1100, 2200], [600, 1200, 2300]]
    s.rows1 += [[k, k + 1, k + 2] for k in range(700, 2400, 9)]
    _survivor_strip_rows(s, np.random.default_rng(41), vote)
    c = s.case("far_votes/" + vote, vote, dropped=[100, 101, 601], through_pending={100: -1, 101: -1, 600: 0})
    cnt = c.votes()
    assert cnt[100] == -1 and cnt[101] == -1 and cnt[600] == 0 and cnt[601] == -2 and np.nonzero(cnt < 0)[0].tolist() == [100, 101, 601]
    return c


def _sel_far_base(n=N_FAR):
    """Four near walls at level L0 and one near flat row above it."""
    s = Strip(n)
    for k in range(4):
        s.wall([300 + 3 * k, 301 + 3 * k, 302 + 3 * k], L0)
    s.flat([510, 511, 512], (HIGH,) * 3, place=False)
    return s


def far_flat_case():
    """(10, 1030, 2550): the only flat triangle at its three vertices, above the level."""
    s = _sel_far_base()
    s.flat([10, 1030, 2550], (2.5625,) * 3)
    c = s.case("far_flat", want_selected=[10, 510, 511, 512, 1030, 2550])
    assert c.oracle().sel.selected_ids.tolist() == c.info["want_selected"]
    return c


def far_steep_case():
    """Near walls at 1.0 (three of them) and a far wall at 3.0: the level is 1.5 with it and 1.0 without; a near candidate at 1.25."""
    s = Strip(N_FAR)
    for k in range(3):
        s.wall([300 + 3 * k, 301 + 3 * k, 302 + 3 * k], 1.0)
    s.wall([20, 1040, 2540], 3.0)
    s.flat([510, 511, 512], (HIGH,) * 3, place=False)
    s.flat([1022, 1023, 1024], (1.25,) * 3, place=False)
    c = s.case("far_steep", want_selected=[510, 511, 512])
    assert c.oracle().height_level == 1.5 and c.oracle().sel.selected_ids.tolist() == c.info["want_selected"]
    return c


def far_singular_case():
    s = _sel_far_base()
    ids = [30, 1050, 2530]
    s.rows2.append(ids)
    m = np.array(sc.SINGULAR_MATRICES[1], dtype=np.float64)
    s.x[ids], s.y[ids], s.z[ids] = m[:, 0], m[:, 1], m[:, 2]
    c = s.case("far_singular")
    assert c.oracle().status == so.ST_ERR_SINGULAR
    return c


def cap_votes_case(n_far):
    """n_far far rows of tri1, each of which takes its own pair (2j, 2j+1) from 0 to -1."""
    s = Strip(N_FAR, vote_side=True)
    for j in range(n_far):
        s.drop_pair(2 * j, 2 * j + 1)
        s.rows1 += [[700 + j, 2 * j, 2 * j + 1], [2100 + j, 2 * j, 2 * j + 1]]
    _survivor_strip_rows(s, np.random.default_rng(43), "reference")
    over = 3 * n_far > PEND_CAP
    c = s.case("cap_votes/%d" % n_far, redo="overflow" if over else None, over=over)
    assert np.array_equal(np.nonzero(~c.oracle().valid)[0], np.arange(2 * n_far)) and c.info["far1"] == n_far
    return c


def cap_heights_case(n_far):
    """n_far far rows of tri2 (j, 1024 + j, 2100 + j), each the only flat triangle at its three vertices, all above the level."""
    s = Strip(N_FAR)
    for k in range(4):
        s.wall([1500 + 3 * k, 1501 + 3 * k, 1502 + 3 * k], L0)
    for j in range(n_far):
        s.flat([j, 1024 + j, 2100 + j], (2.0 + (j % 32) / 16.0 + 1.0 / 64.0,) * 3)
    over = 3 * n_far > PEND_CAP_H
    c = s.case("cap_heights/%d" % n_far, redo="overflow" if over else None, over=over)
    assert len(c.oracle().sel.selected_ids) == 3 * n_far and c.info["far2"] == n_far
    return c


def cap_cases():
    return [cap_votes_case(341), cap_votes_case(342), cap_heights_case(192), cap_heights_case(193)]


def far_cases():
    return [far_votes_case("reference"), far_votes_case("fixed"), far_flat_case(), far_steep_case(), far_singular_case()]


# ============================================================================================================================
# 3. keys and the band (1600 features; rows straddle the boundaries of tiles 0|1, 1|2 and 2|3)
# ============================================================================================================================
N_KEYS = 1600
ANCHORS = (510, 1022, 1534)
U44 = 2.0 ** -44


def _ids(k):
    a = ANCHORS[k % 3] + 3 * (k // 3)
    return [a, a + 1, a + 2]


def _keys_frame(name, walls, flats, redo=None, **info):
    """walls: heights; flats: (y0, y1, y2) — rows k = 0, 1, .. on the anchors in turn."""
    s = Strip(N_KEYS)
    k = 0
    for H in walls:
        s.wall(_ids(k), H)
        k += 1
    for ys in flats:
        s.flat(_ids(k), ys, place=False)
        k += 1
    return s.case(name, redo=redo, **info)


def _tilted(s, ids, zs, xs):
    """Features on the plane y = 1 - z / 8 (normal (0, 1, 1/8): pitch -82.9 deg, a flat row) — its heights are negative beyond z = 8."""
    for i, z, x in zip(ids, zs, xs):
        s.x[i], s.z[i], s.y[i] = x, z, 1.0 - z / 8.0


def negative_keys_case():
    """511 is on two flat rows, of heights -3 and -1 (3h = -9 and -3); the level is -2.  Its largest flat height is -1: selected.  A
    key that orders negative heights by magnitude keeps -3."""
    s = Strip(N_KEYS)
    for k in range(4):
        s.wall(_ids(3 * k + 1), -2.0)
    _tilted(s, [511, 512, 513, 600, 601], [24.0, 36.0, 36.0, 12.0, 12.0], [0.0, -10.0, 10.0, -10.0, 10.0])
    s.rows2 += [[511, 512, 513], [511, 600, 601]]
    c = s.case("keys/negative", want_selected=[511, 600, 601])
    r = c.oracle()
    assert r.height_level == -2.0 and sorted(r.sel.heights[r.sel.valid_pitch].tolist()) == [-3.0, -1.0] and r.sel.selected_ids.tolist() == [511, 600, 601]
    return c


def zero_keys_case(level):
    """511 (y' = -0.0) is on two flat rows whose heights are both +0.0, (-0.0 + 1) + -1 and (-0.0 + 0.5) + -0.5.  (A height of -0.0 needs
    three y' of -0.0: a plane through the camera centre, which is singular — it cannot be a flat row.)"""
    s = Strip(N_KEYS)
    for k in range(4):
        s.wall(_ids(3 * k + 1), level)
    _tilted(s, [511, 512, 513, 600, 601], [8.0, 0.0, 16.0, 4.0, 12.0], [0.0, -10.0, 4.0, -10.0, 4.0])
    s.y[511] = -0.0
    s.rows2 += [[511, 512, 513], [511, 600, 601]]
    s.flat(_ids(2), (HIGH,) * 3, place=False)
    c = s.case("keys/zero/level%g" % level)
    r = c.oracle()
    assert np.signbit(c.f3[511, 1]) and r.sel.valid_pitch[4:6].all() and (r.sel.heights[4:6] == 0.0).all()
    assert (511 in r.sel.selected_ids.tolist()) == (level < 0)
    return c


def band_delta(rel):
    """The multiple of 2^-44 nearest to rel x 3 L0: what one y' of a flat row at the level is moved by."""
    return round(abs(rel) * 3 * L0 / U44) * U44 * np.sign(rel)


BAND_INSIDE, BAND_OUTSIDE = (1e-13, -1e-13), (1e-10, -1e-10)


def keys_cases():
    walls = [L0] * 4
    out = [negative_keys_case(), zero_keys_case(-2.0), zero_keys_case(1.0),
           _keys_frame("keys/steep_negative", [-2.0] * 4, [(HIGH,) * 3, (2.5625,) * 3]),
           _keys_frame("keys/steep_both_signs", [-1.0, -1.0, 2.0, 2.0], [(HIGH,) * 3, (2.5625,) * 3], redo="mixed"),
           _keys_frame("keys/no_steep", [], [(HIGH,) * 3, (2.5625,) * 3], redo="nan"),
           _keys_frame("keys/at_level", walls, [(L0,) * 3, (HIGH,) * 3], redo="band", rel=0.0)]
    for rel in BAND_INSIDE + BAND_OUTSIDE:
        out.append(_keys_frame("keys/band/%+g" % rel, walls, [(L0, L0, L0 + band_delta(rel)), (HIGH,) * 3],
                               redo="band" if rel in BAND_INSIDE else None, rel=rel))
    out.append(_keys_frame("keys/nothing_selected", walls, [(1.0,) * 3, (1.125,) * 3], redo="none"))
    out.append(lone_bins_strip_case())
    return out


def lone_bins_strip_case():
    """scale_cases.lone_bins_case() in a strip of 1537 features: its flat triangle on 1534, 1535, 1536 (tiles 2 and 3: the ring wraps)."""
    lb = sc.lone_bins_case()
    s = Strip(1537)
    for k, a in enumerate((510, 1022, 100, 800, 1534)):
        ids = [a, a + 1, a + 2]
        s.x[ids], s.y[ids], s.z[ids] = lb.f3[3 * k:3 * k + 3].T
        s.rows2.append(ids)
    c = s.case("keys/lone_bins", redo="level")
    assert c.oracle().status == so.ST_LEVEL
    return c


# ============================================================================================================================
# 4. candidate lists
# ============================================================================================================================
LIST_LEVEL, LIST_D = 0.375, 0.125
EXTRA0 = 192                       # nine extra features (group 3: wavefront 3) carry the three walls


def list_classes(n, pattern):
    """Per feature: 1 selected, 0 a candidate below the level, 2 one of the nine wall features."""
    g = np.arange(n) // 64
    if pattern == "all":
        cls = np.ones(n, dtype=np.int64)
    elif pattern == "every_other_group":
        cls = (g % 2 == 0).astype(np.int64)
    else:
        cls = (g % DW != 5).astype(np.int64)
    if 0 < n % 64 < 3:                                                  # (a group of one or two cannot hold a row of its own)
        cls[64 * (n // 64):] = cls[64 * (n // 64) - 1]
    cls[EXTRA0:EXTRA0 + 9] = 2
    return cls


def list_case(n, pattern):
    """Every feature is a candidate.  Selected feature i has y' in histogram bin (i // 64) % 160 + 5; the others lie below the level.
    Walls (y' = L - d, L - d, L + 2d: height exactly L) stand on nine extra features, which three flat rows across the walls make
    candidates as well: six below the level, three above."""
    cls = list_classes(n, pattern)
    s = Strip(n)
    i = np.arange(n)
    b = (i // 64) % 160 + 5
    s.y = np.where(cls == 1, (np.ceil(0.1 * b * 1024.0) + 1 + i % 64) / 1024.0, 0.25 + (i % 64) / 1024.0)
    ex = EXTRA0 + np.arange(9).reshape(3, 3)
    for w, zs in enumerate(((5.0, 16.0, 9.0), (13.0, 20.0, 31.0), (11.0, 40.0, 17.0))):      # (no three of a role on one line)
        s.x[ex[w]], s.z[ex[w]] = 3.0 + w, zs
        s.y[ex[w]] = (LIST_LEVEL - LIST_D, LIST_LEVEL - LIST_D, LIST_LEVEL + 2 * LIST_D)
        s.rows2.append(ex[w].tolist())
    for r in range(3):
        s.rows2.append(ex[:, r].tolist())
    run = cls + 3 * (np.arange(n) // (64 * 160))                         # (no row across a wrap of the bins: 16 in y' would tilt it past the camera)
    edges = np.nonzero(np.diff(run))[0] + 1
    for a, e in zip(np.concatenate([[0], edges]), np.concatenate([edges, [n]])):
        if cls[a] == 2:
            continue
        assert e - a >= 3
        s.rows2 += [[k, k + 1, k + 2] for k in range(a, e - 2, 3)]
        if (e - a) % 3:
            s.rows2.append([e - 3, e - 2, e - 1])
    s.rows1 = [[k, k + 1, k + 2] for k in range(0, n - 2, 64)]
    c = s.case("lists/n%d/%s" % (n, pattern), cls=cls)
    r = c.oracle()
    want = np.nonzero((cls == 1) | ((cls == 2) & (c.f3[:, 1] > LIST_LEVEL)))[0]
    assert r.height_level == LIST_LEVEL and np.array_equal(r.sel.selected_ids, want), c.name
    assert sum(c.info["wave_cands"]) == n
    return c


def list_sizes():
    return [64 * g + r for g in LIST_G for r in LIST_R]


def list_cases_small():
    return [list_case(n, LIST_PATTERNS[(k + j) % 3]) for k, n in enumerate(list_sizes()) for j in range(3)]


def list_cases_large():
    return [list_case(n, p) for n in LIST_LARGE for p in LIST_PATTERNS]


# ============================================================================================================================
# 6. vote range across tiles
# ============================================================================================================================
N_FAN, FAN_CENTRE = 2100, 3 * W - 1


def fan_strip_case(plus, vote, seed=3):
    """scale_cases.fan_case's construction in a strip of 2100 features: 32 765 rows through the last feature of tile 2, whose 256 ring
    vertices lie in tiles 2 and 3 (ring slots that wrap to the ring's start)."""
    rng = np.random.default_rng([seed, int(plus)])
    n, centre, partner = N_FAN, FAN_CENTRE, FAN_CENTRE ^ 1
    ring = np.array([i for i in range(centre - 129, centre + 129) if i not in (centre, partner)])
    assert len(ring) == sc.N_RING
    sgn = rng.uniform(1.0, 90.0, sc.N_RING) * rng.choice([-1.0, 1.0], sc.N_RING)
    v, z = np.full(n, 300.0), np.full(n, 10.0)
    v[ring] = 300.0 + sgn
    z[ring] = 10.0 + (-1.0 if plus else 1.0) * np.sign(sgn) * rng.uniform(0.5, 4.0, sc.N_RING)
    rest = np.setdiff1d(np.arange(n), np.concatenate([ring, [centre, partner]]))
    v[rest], z[rest] = 250.0 + (rest % 97), 3.0 + (rest % 89) / 8.0                      # (unreferenced: counter 1)
    k = np.arange(sc.MAX_VOTE_ROWS)
    rows = np.stack([np.full(len(k), centre), ring[k % sc.N_RING], ring[(k + 1) % sc.N_RING]], 1)
    rows[[5, 1000, 20000], 2] = partner
    f3 = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(1, 2, n), z])
    f2 = np.column_stack([np.arange(n, dtype=np.float64), v])
    nv = int((so.outlier_votes(v, z, rows, vote) >= 0).sum())
    tri2 = np.array([[nv - 4, nv - 3, nv - 2], [nv - 3, nv - 2, nv - 1]])
    c = sc.Case("fan_strip/%s/%s" % ("plus" if plus else "minus", vote), f3, f2, rows, tri2, vote, centre=centre,
                centre_count=(1 + len(k)) if plus else (1 - len(k)))
    assert c.votes()[centre] == c.info["centre_count"] and c.oracle().status == so.ST_NO_FLAT
    return _finish(c, redo="none")


def fan_strip_cases():
    return [fan_strip_case(plus, vote) for vote in ("reference", "fixed") for plus in (True, False)]


# ============================================================================================================================
# 7. small frames of the mixed batch
# ============================================================================================================================
def tiny_case(n):
    """0, 3 or 4 features on the plane y = 2 (at 4: two flat rows, no steep one)."""
    pts = np.array([[-6.0, 2.0, 8.0], [6.0, 2.0, 9.0], [0.5, 2.0, 20.0], [3.0, 2.0, 30.0]])[:n]
    f2 = np.column_stack([np.arange(n, dtype=np.float64), np.full(n, sc.V_ROW)])
    rows = np.array([[0, 1, 2], [1, 2, 3]][:max(n - 2, 0)], dtype=np.int64).reshape(-1, 3)
    return sc.Case("tiny/%d" % n, pts, f2, rows, rows if n > 3 else np.zeros((0, 3)))


# ============================================================================================================================
# the kernel's selection rule in NumPy, with switches
# ============================================================================================================================
def _key64(h, sign_magnitude=False):
    b = np.ascontiguousarray(h, dtype=np.float64).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    if sign_magnitude:                                                   # the sign bit flipped and nothing else: negatives order by magnitude
        return b ^ top
    return np.where(b >> np.uint64(63) != 0, ~b, b | top)


def _unkey64(k, sign_magnitude=False):
    top = np.uint64(1) << np.uint64(63)
    if sign_magnitude:
        return (k ^ top).view(np.float64)
    return np.where(k >> np.uint64(63) != 0, k & ~top, ~k).view(np.float64)


def model(c, far_votes=True, far_heights=True, far_steep=True, sign_magnitude=False, ge=False, partial_to_previous=False,
          selbits_cut=False, pend_first_index=False, pend_apply_short=False):
    """What scale_frames_tiled_kernel computes for the frame, from the oracle's flat / steep classification of the rows: the vote with
    the far rows' contributions through the pending list, per vertex the largest flat 3h through the 64-bit key, the level as the mean
    of the steep 3h, one comparison per candidate, the candidates parked in per-wavefront lists and read back.  Returns
    {valid, overflow, selected_y (sorted; what reaches the road model), nsel}.  The switches are the mutants of test_tiled_cases.py."""
    n = c.n
    v, z = c.f2[:, 1], c.f3[:, 2]
    tri1 = c.tri1.astype(np.int64)
    far1 = is_far(tri1) if len(tri1) else np.zeros(0, dtype=bool)
    flags = sc._vote_flags(v, z, tri1, c.vote)
    ids = np.concatenate([tri1[~far1].reshape(-1), tri1[far1].reshape(-1)])             # near rows in the walk, then the pending entries
    add = np.where(np.concatenate([flags[~far1].reshape(-1), flags[far1].reshape(-1)]), -1, 1)
    n_near, n_pend = 3 * int((~far1).sum()), 3 * int(far1.sum())
    overflow = n_pend > (PEND_CAP + 2 if pend_first_index else PEND_CAP)                # (mutant: a row whose FIRST entry is inside "fits")
    applied = min(n_pend, PEND_CAP) if far_votes else 0
    cnt = np.ones(n, dtype=np.int64)
    np.add.at(cnt, ids[:n_near + applied], add[:n_near + applied])
    valid = cnt >= 0
    # tri2: the oracle's rows and their classification (the pitch test is not what this model is about)
    s = c.oracle().sel
    rows = feature_rows(c)
    y = c.f3[:, 1]
    h3 = (y[rows[:, 0]] + y[rows[:, 1]]) + y[rows[:, 2]]
    far2 = is_far(rows)
    with np.errstate(invalid="ignore"):
        flat = s.valid_pitch & (h3 == h3)
        steep = ~s.valid_pitch & ~np.isnan(s.pitch_deg)
    n_pend_h = 3 * int(far2.sum())
    overflow |= n_pend_h > PEND_CAP_H
    use_steep = steep & (far_steep | ~far2)
    with np.errstate(all="ignore"):
        hl = np.sum(h3[use_steep]) / np.float64(use_steep.sum())
    key = np.zeros(n, dtype=np.uint64)
    near_flat = flat & ~far2
    np.maximum.at(key, rows[near_flat].reshape(-1), np.repeat(_key64(h3[near_flat], sign_magnitude), 3))
    if far_heights:
        fr = rows[far2].reshape(-1)
        fk = np.repeat(np.where(flat[far2], _key64(h3[far2], sign_magnitude), np.uint64(0)), 3)
        take = min(len(fr), PEND_CAP_H - 1 if pend_apply_short else PEND_CAP_H)
        np.maximum.at(key, fr[:take], fk[:take])
    cand = key != 0
    hm = _unkey64(key, sign_magnitude)
    with np.errstate(invalid="ignore"):
        sel = cand & ((hm >= hl) if ge else (hm > hl))
    # the lists: wavefront w appends the candidates of the groups g = w (mod 8) at its base; the tail reads its own list back
    nfull, rem = n >> 6, n & 63
    cap = np.array([64 * len(range(w, nfull, DW)) for w in range(DW)])
    if rem:
        cap[((nfull - 1) if partial_to_previous else nfull) % DW] += rem
    base = np.concatenate([[0], np.cumsum(cap)[:-1]])
    plane_y, plane_s = np.full(n + 64, np.nan), np.zeros(n + 64, dtype=bool)
    wave = (np.arange(n) // 64) % DW
    lists = []
    for w in range(DW):                                                  # (later wavefronts write over an overlap)
        mine = np.nonzero(cand & (wave == w))[0]
        plane_y[base[w]:base[w] + len(mine)], plane_s[base[w]:base[w] + len(mine)] = y[mine], sel[mine]
        lists.append(len(mine))
    out_y = []
    for w in range(DW):
        ly, ls = plane_y[base[w]:base[w] + lists[w]], plane_s[base[w]:base[w] + lists[w]]
        if selbits_cut:
            ls = ls & (np.arange(lists[w]) < 64 * 64)
        out_y.append(ly[ls])
    out_y = np.sort(np.concatenate(out_y))
    return dict(valid=valid, overflow=bool(overflow), selected_y=out_y, nsel=int(sel.sum()), level3=float(hl),
                hmax3=hm, cand=cand, mixed=bool((h3[use_steep] < 0).any() and (h3[use_steep] > 0).any()))


MUTANTS = {"far votes dropped": dict(far_votes=False), "far heights dropped": dict(far_heights=False),
           "far steep rows left out of the level": dict(far_steep=False), "key compared as sign-magnitude": dict(sign_magnitude=True),
           ">= at the level": dict(ge=True), "partial group credited to wavefront (nfull - 1) % 8": dict(partial_to_previous=True),
           "selbits cut at 64 chunks": dict(selbits_cut=True), "pending cap: a row that starts at entry 1023 fits": dict(pend_first_index=True),
           "pending cap: 575 height entries applied": dict(pend_apply_short=True)}


def model_redo(c, m):
    """Why the kernel hands the frame over, from the model's numbers (None: it does not).  The road model's own hand-over (a frame
    that ends on the level) is the oracle's ST_LEVEL."""
    if m["overflow"]:
        return "overflow"
    if c.oracle().status == so.ST_ERR_SINGULAR or not np.array_equal(m["valid"], c.oracle().valid):
        return None
    if m["level3"] != m["level3"]:
        return "nan"
    if m["mixed"]:
        return "mixed"
    with np.errstate(invalid="ignore"):
        if (m["cand"] & (np.abs(m["hmax3"] - m["level3"]) <= LEVEL_GUARD * abs(m["level3"]))).any():
            return "band"
    if m["nsel"] == 0:
        return "none"
    return "level" if c.oracle().status == so.ST_LEVEL else None


def model_equals_oracle(c, m):
    """The model's survivors and what it hands the road model, against the oracle (frames that overflow are the exact pass's)."""
    r = c.oracle()
    if m["overflow"]:
        return True
    if not np.array_equal(m["valid"], r.valid):
        return False
    if r.status == so.ST_ERR_SINGULAR:
        return True
    want = np.sort(c.f3[np.asarray(r.valid)][r.sel.selected_ids, 1])
    return m["nsel"] == len(want) and np.array_equal(m["selected_y"], want)


def band_margin(c, m):
    """min |3h_max - 3 level| / |3 level| over the candidates."""
    with np.errstate(all="ignore"):
        return float(np.min(np.abs(m["hmax3"][m["cand"]] - m["level3"])) / abs(m["level3"])) if m["cand"].any() else np.inf
