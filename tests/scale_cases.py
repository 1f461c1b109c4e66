"""Crafted frames and references for the headline kernels — scale_frames_kernel<WAVES, SC, MODE>, its dense siblings and
outlier_vote_kernel (csrc/mvosr_kernels.hip) — shared by tests/test_scale_cases.py (CPU) and tests/test_gpu_scale_cases.py.
Test infrastructure.

Both triangulations are INPUTS of mvosr_scale_batch / mvosr_outlier_vote_batch, and the oracle's stage functions take any rows,
so a frame here is (f3, f2, tri1, tri2) with connectivity no triangulation would give: fans of 32 765 rows through one vertex,
first triangulations that vote exactly a prescribed survivor mask, disjoint triangles whose pitch sits a chosen distance from
the -80 deg threshold.  Every frame is processed with camera_pitch = 0 on both sides (y.1 - z.0 is the input's own double: the
remap contributes no rounding) and packed with a vanishing row below every pixel row.

Expected values come from oracle.scale_oracle (`outlier_votes`, `tri_select`, `road_model`, `frame_raw_scale`) and, for the pitch
of a row, from Cramer's rule in np.longdouble (`pitch_true`).  The `mutant_*` functions are CPU stand-ins for a subtly wrong kernel:
tests/test_scale_cases.py asserts that each differs from the oracle on at least one case, i.e. that the cases can see it.
"""
import numpy as np

import flat_cases as fc
from oracle import scale_oracle as so

ABS_REF = 1.75
ORACLE_KW = dict(camera_pitch=0.0, vanish=-1.0)
VANISH = -1.0
V_ROW = 500.0                      # the one pixel row of every feature of a selection frame: every vote product is +-0, nobody is flagged
MAX_VOTE_ROWS = 32765              # kMaxVoteRows
COUNTER_BIAS = 0x8000              # kCounterBias
THR_DEG = -80.0
S2 = np.sin(np.deg2rad(80.0)) ** 2
BAND = 1e-9                        # s2_lo / s2_hi = sin^2(80 deg) (1 -+ 1e-9); half-width in degrees: 1e-9 / (2 cot 80 deg) = 1.6e-7
U52 = 2.0 ** -52
WAVE = 64
INSTANTIATIONS = ((1, 8), (4, 4), (4, 8), (8, 4), (8, 8), (16, 4), (16, 8))
# Largest |pitch_numpy - pitch_longdouble| / (2^-52 cond_2(A) 180/pi) over every regular row of the selection family, NumPy's
# float64 inv against Cramer's rule in longdouble (test_scale_cases.py measures it again and asserts that it has not grown).  The
# kernel's pivot order and its FMAs are not LAPACK's: a factor 4 on the measured maximum, rounded up (the precedent of
# flat_cases.C_HEIGHT).  A pitch decision is compared only on rows farther from -80 deg than C_PITCH 2^-52 cond_2(A) 180/pi.
C_PITCH_MEASURED = 3.46
C_PITCH = 14.0


class Case:
    """One frame: f3 (n,3), f2 (n,2), tri1 rows over the features, tri2 rows over the survivors of the vote.  `vote`: the vote mode
    it was built for.  `status`: set where the kernels must refuse the frame whatever the oracle says (MVOSR_ST_ERR_MASK)."""

    def __init__(self, name, f3, f2, tri1, tri2, vote="reference", status=None, **info):
        self.name, self.vote, self.status, self.info = name, vote, status, info
        self.f3 = np.ascontiguousarray(f3, dtype=np.float64).reshape(-1, 3)
        self.f2 = np.ascontiguousarray(f2, dtype=np.float64).reshape(-1, 2)
        self.tri1 = np.ascontiguousarray(tri1, dtype=np.int32).reshape(-1, 3)
        self.tri2 = np.ascontiguousarray(tri2, dtype=np.int32).reshape(-1, 3)
        self._ores = None

    @property
    def n(self):
        return self.f3.shape[0]

    def oracle(self):
        """The oracle's frame (cached; never modified)."""
        if self._ores is None:
            self._ores = so.frame_raw_scale(self.f3, self.f2, ABS_REF, self.tri1, self.tri2, check_triangle=self.vote, **ORACLE_KW)
        return self._ores

    def votes(self):
        return so.outlier_votes(self.f2[:, 1], self.f3[:, 2], self.tri1, self.vote)

    def rows_xyz(self):
        """(T2,3,3): the vertices of tri2's rows (tri2 numbers the survivors of the vote)."""
        return self.f3[np.asarray(self.oracle().valid)][self.tri2.astype(np.int64)]


# ============================================================================================================================
# vote family
# ============================================================================================================================
def _vote_flags(v, z, tri, vote):
    """(T,3) True = the row votes against the vertex (oracle.scale_oracle.outlier_votes, :105-119)."""
    v0, v1, v2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    d0, d1, d2 = z[tri[:, 0]], z[tri[:, 1]], z[tri[:, 2]]
    with np.errstate(invalid="ignore"):
        a, b, c = (v0 - v1) * (d0 - d1) > 0, (v0 - v2) * (d0 - d2) > 0, (v1 - v2) * (d1 - d2) > 0
    return np.stack([a | b, a | c, b | c], 1) if vote == "fixed" else np.stack([a | b, a | b | c, c], 1)


def packed_votes(v, z, tri, vote, init=COUNTER_BIAS + 1, decode_bias=COUNTER_BIAS, signed=False):
    """The LDS-resident kernels' counters on the CPU: two 16-bit halves per 32-bit word, every half starts at `init`, a vote is
    ONE wrap-around add of (+1 or 0xFFFFFFFF) << 16 (id & 1) to the word; read back as half - decode_bias (`signed`: as int16)."""
    n = v.shape[0]
    tri = np.asarray(tri, dtype=np.int64)
    flag = _vote_flags(v, z, tri, vote).reshape(-1)
    ids = tri.reshape(-1)
    words = np.full((n + 1) // 2, (init << 16) | init, dtype=np.uint64)
    add = (np.where(flag, np.uint64(0xFFFFFFFF), np.uint64(1)) << (np.uint64(16) * (ids & 1).astype(np.uint64))) & np.uint64(0xFFFFFFFF)
    np.add.at(words, ids >> 1, add)
    words &= np.uint64(0xFFFFFFFF)
    halves = np.stack([words & np.uint64(0xFFFF), words >> np.uint64(16)], 1).reshape(-1)[:n].astype(np.int64)
    if signed:
        halves = np.where(halves >= 0x8000, halves - 0x10000, halves)
    return halves - decode_bias


def mutant_votes_unbiased(c):
    """Halves that start at 1 and are read as int16: a -1 on a half at 0 borrows from the other half of the word."""
    return packed_votes(c.f2[:, 1], c.f3[:, 2], c.tri1, c.vote, init=1, decode_bias=0, signed=True)


def mutant_votes_bias_7fff(c):
    """Counters set up with kCounterBias + 1 but read back against 0x7FFF."""
    return packed_votes(c.f2[:, 1], c.f3[:, 2], c.tri1, c.vote, decode_bias=0x7FFF)


N_RING, N_SPARE = 256, 4


def _finish_vote_case(name, v, z, rows, vote, shuffle, seed, **info):
    """x and y at random, the pixel column, and a tri2 over the LAST survivors (the unreferenced spare vertices: counter 1)."""
    rng = np.random.default_rng([seed, 77])
    n = v.shape[0]
    rows = np.asarray(rows, dtype=np.int64)
    if shuffle:                      # the vertices of every row rotated, the rows permuted: the fixed vote does not depend on either
        rows = np.stack([np.roll(r, k) for r, k in zip(rows, rng.integers(3, size=len(rows)))])[rng.permutation(len(rows))]
    f3 = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(1, 2, n), z])
    f2 = np.column_stack([np.arange(n, dtype=np.float64), v])
    nv = int((so.outlier_votes(v, z, rows, vote) >= 0).sum())
    tri2 = np.array([[nv - 4, nv - 3, nv - 2], [nv - 3, nv - 2, nv - 1]])
    return Case(name, f3, f2, rows, tri2, vote, status=so.ST_ERR_MASK if len(rows) > MAX_VOTE_ROWS else None, **info)


def fan_case(name, centre, plus, vote, n_rows=MAX_VOTE_ROWS, shuffle=False, seed=3):
    """Every row holds vertex `centre` (first in the row): it is never (plus) or always flagged.  The other half of its counter word
    belongs to `centre ^ 1`, which three rows hold; 256 ring vertices with mixed votes; four unreferenced vertices at the end."""
    rng = np.random.default_rng([seed, centre, int(plus)])
    n = 2 + N_RING + N_SPARE
    partner = centre ^ 1
    ring = np.array([i for i in range(2 + N_RING) if i not in (centre, partner)])
    s = rng.uniform(1.0, 90.0, N_RING) * rng.choice([-1.0, 1.0], N_RING)
    v, z = np.full(n, 300.0), np.full(n, 10.0)
    v[ring] = 300.0 + s
    z[ring] = 10.0 + (-1.0 if plus else 1.0) * np.sign(s) * rng.uniform(0.5, 4.0, N_RING)     # plus: (v - vc)(z - zc) < 0 for every ring vertex
    v[-N_SPARE:], z[-N_SPARE:] = 250.0 + np.arange(N_SPARE), 3.0 + np.arange(N_SPARE)
    k = np.arange(n_rows)
    rows = np.stack([np.full(n_rows, centre), ring[k % N_RING], ring[(k + 1) % N_RING]], 1)
    rows[[5, 1000, 20000], 2] = partner                       # (at the centre's own pixel row and depth: its pair with the centre gives 0)
    return _finish_vote_case(name, v, z, rows, vote, shuffle, seed, centre=centre, partner=partner,
                             centre_count=(1 + n_rows) if plus else (1 - n_rows))


def opposite_case(name, up, vote, shuffle=False, seed=5):
    """Vertices 0 and 1 share a counter word and are both in every row: `up` is never flagged (+32 765), the other always."""
    rng = np.random.default_rng([seed, up])
    n = 2 + N_RING + N_SPARE
    down = up ^ 1
    ring = 2 + np.arange(N_RING)
    v, z = np.full(n, 300.0), np.full(n, 10.0)
    z[down] = 5.0
    v[ring], z[ring] = rng.uniform(301.0, 390.0, N_RING), rng.uniform(5.5, 9.5, N_RING)
    v[-N_SPARE:], z[-N_SPARE:] = 250.0 + np.arange(N_SPARE), 3.0 + np.arange(N_SPARE)
    k = np.arange(MAX_VOTE_ROWS)
    rows = np.stack([np.full(len(k), up), np.full(len(k), down), ring[k % N_RING]], 1)
    return _finish_vote_case(name, v, z, rows, vote, shuffle, seed, up=up, down=down)


def edge_counts_case(vote):
    """Counters at the keep / drop boundary and products that are +0, -0 and NaN.  Expected (both vote modes):
    0, 1 flagged by one row -> 0 (kept); 3, 4 flagged by two rows -> -1 (dropped); 2 -> 2; 5 -> 3; 6, 7, 17 unreferenced -> 1;
    8..16 in one row whose products are +-0 or NaN -> 2."""
    nan = float("nan")
    v = np.array([100, 200, 300, 100, 200, 300, 50, 60, 150, 150, 150, 110, 120, 130, 140, 160, 170, 70], dtype=np.float64)
    z = np.array([10, 20, 5, 10, 20, 5, 1, 2, 7, 8, 9, 4, 4, 4, nan, 6, 5, 3], dtype=np.float64)
    rows = np.array([[2, 0, 1], [5, 3, 4], [5, 3, 4], [8, 9, 10], [13, 12, 11], [14, 15, 16]])
    want = np.array([0, 0, 2, -1, -1, 3, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1])
    rng = np.random.default_rng(9)
    n = len(v)
    f3 = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(1, 2, n), z])
    f2 = np.column_stack([np.arange(n, dtype=np.float64), v])
    return Case("edge_counts/" + vote, f3, f2, rows, [[0, 1, 2], [1, 2, 5]], vote, want=want)      # (survivors 0,1,2,5,6,7: all finite)


def vote_cases():
    """Every vote frame, in both vote modes; in `fixed` mode also with the rows rotated and permuted."""
    out = []
    for vote, shuffles in (("reference", (False,)), ("fixed", (False, True))):
        for sh in shuffles:
            tag = "%s%s" % (vote, "+shuffled" if sh else "")
            for centre in (0, 1):
                for plus in (True, False):
                    out.append(fan_case("fan_%s/centre%d/%s" % ("plus" if plus else "minus", centre, tag), centre, plus, vote, shuffle=sh))
            for up in (0, 1):
                out.append(opposite_case("opposite/up%d/%s" % (up, tag), up, vote, shuffle=sh))
        out.append(edge_counts_case(vote))
        out.append(fan_case("fan_plus/32766rows/" + vote, 0, True, vote, n_rows=MAX_VOTE_ROWS + 1))
    return out


# ============================================================================================================================
# compaction family
# ============================================================================================================================
def compaction_case(name, keep, seed=1):
    """A frame whose vote (either mode) keeps exactly `keep`.  Every feature sits on the anti-diagonal (v, z) = (t, Z0 - t) with
    its own integer t — any two of them give (dv)(dz) < 0, no flag — except that a dropped feature d2 is moved next to its partner
    d1: (t1 + 1/4, Z0 - t1 + 1/4), so that (dv)(dz) = 1/16 > 0 for that pair alone (against everyone else (de)^2 - (dt)^2 < 0).  A row
    (k, d1, d2) with k kept flags d1 and d2 and not k; two such rows drop both.  tri2: rows (j, j+1, j+2) over the survivors, whose
    y' are all distinct — a survivor written to the wrong place changes a triangle height."""
    keep = np.asarray(keep, dtype=bool)
    n = keep.shape[0]
    rng = np.random.default_rng([seed, n, int(keep.sum())])
    K, D = np.nonzero(keep)[0], np.nonzero(~keep)[0]
    assert len(K) >= 1
    t, e = 200.0 + np.arange(n), np.zeros(n)
    rows = []
    kk = lambda i: K[i % len(K)]
    if len(D) == 1:                  # one dropped feature: its partner is a kept one, lifted back by three rows of its own
        assert len(K) >= 4
        d, k2 = D[0], K[0]
        t[k2], e[k2] = t[d], 0.25
        rows += [[K[1], d, k2]] * 2 + [[k2, K[1], K[2]], [k2, K[2], K[3]], [k2, K[3], K[1]]]
    else:
        for i in range(0, len(D) - 1, 2):
            d1, d2 = D[i], D[i + 1]
            t[d2], e[d2] = t[d1], 0.25
            rows += [[kk(i), d1, d2]] * 2
        if len(D) % 2:               # the odd one out sits on the other side of the last pair's d1
            d3, d1 = D[-1], D[-3]
            t[d3], e[d3] = t[d1], -0.25
            rows += [[kk(len(D)), d3, d1]] * 2
    for i in range(0, len(K) - 2, 7):                         # rows among kept features: +1 each
        rows.append([K[i], K[i + 1], K[i + 2]])
    if not rows:
        rows.append([K[0], K[0], K[0]])
    rows = np.array(rows, dtype=np.int64)[rng.permutation(len(rows))]
    v, z = t + e, 20000.0 - t + e
    # y': distinct multiples of 2^-15 (exact), mostly within 0.2 of 1.5 (flat-ish rows), three in ten lifted by 0.5 .. 2 (steep rows)
    y = 1.5 + rng.permutation(n) / 32768.0 + np.where(rng.random(n) < 0.3, rng.integers(1, 5, n) / 2.0, 0.0)
    f3 = np.column_stack([rng.uniform(-8, 8, n), y, z])
    f2 = np.column_stack([np.arange(n, dtype=np.float64), v])
    nv = len(K)
    tri2 = np.stack([np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)], 1) if nv >= 3 else np.array([[0, 0, nv - 1]])
    return Case(name, f3, f2, rows, tri2, keep=keep)


def compaction_masks(n, waves, sc):
    """name -> survivor mask for a frame of n features run by the (waves, sc) instantiation."""
    i = np.arange(n)
    m = {"all": np.ones(n, bool), "only0": i == 0, "last+3front": (i < 3) | (i == n - 1), "every2nd": i % 2 == 0, "every64th": i % 64 == 0,
         "last_subchunk": i >= 64 * ((n - 1) // 64)}
    per = sc * WAVE
    last_wave = (n - 1) // per
    if last_wave >= 1:               # (one wave slice only: dropping it leaves nobody)
        for tag, w in (("first", 0), ("middle", last_wave // 2), ("last", last_wave)):
            m["slice_%s_dropped" % tag] = ~((i >= w * per) & (i < (w + 1) * per))
    return m


def compaction_plan(max_lds):
    """(n, waves override, (WAVES, SC) or None for the dense two-sweep kernel): the sizes the issue names, through the instantiation
    the dispatch picks for them, and every instantiation at least once."""
    plan = [(319, 1, (1, 8)), (320, 1, (1, 8)), (321, 1, (1, 8)), (321, 4, (4, 4)),
            (1023, 4, (4, 4)), (1024, 4, (4, 4)), (1025, 4, (4, 8)), (1025, 8, (8, 4)),
            (2047, 8, (8, 4)), (2048, 8, (8, 4)), (2049, 8, (8, 8)), (2049, 16, (16, 4)),
            (4095, 16, (16, 4)), (4096, 16, (16, 4)), (4097, 16, (16, 8)),
            (max_lds, 16, (16, 8)), (max_lds + 1, 16, None)]
    return plan


def compaction_cases(n, waves, sc):
    return [compaction_case("compact/n%d/%s" % (n, tag), m) for tag, m in compaction_masks(n, waves, sc or 8).items()]


def compacted_layout(keep, waves, sc, skip_empty=False):
    """Which feature the compaction leaves at every survivor slot (-1: nothing written): wave w owns [w sc 64, (w+1) sc 64) and
    writes its survivors from base = the counts of the waves before it.  `skip_empty`: the mutant whose running base stops at the
    first wave slice without survivors."""
    keep = np.asarray(keep, dtype=bool)
    per = sc * WAVE
    cnt = [int(keep[w * per:(w + 1) * per].sum()) for w in range(waves)]
    slot = np.full(int(keep.sum()), -1, dtype=np.int64)
    for w in range(waves):
        base = 0
        for i in range(w):
            if skip_empty and cnt[i] == 0:
                break
            base += cnt[i]
        ids = np.nonzero(keep[w * per:(w + 1) * per])[0] + w * per
        slot[base:base + len(ids)] = ids
    return slot


def layout_heights(c, slot):
    """tri2's heights when survivor slot j holds feature slot[j] (NaN where nothing was written)."""
    y = np.where(slot >= 0, c.f3[np.maximum(slot, 0), 1], np.nan)
    return np.mean(y[c.tri2], 1)


# ============================================================================================================================
# selection family: disjoint small triangles
# ============================================================================================================================
def _rot_y(p, az):
    c, s = np.cos(az), np.sin(az)
    return np.column_stack([p[:, 0] * c + p[:, 2] * s, p[:, 1], -p[:, 0] * s + p[:, 2] * c])


def tri_frame(name, tris, rows=None, **info):
    """Triangle i has the features 3i, 3i+1, 3i+2; every feature on pixel row V_ROW; tri1 = those triples (every counter 2)."""
    pts = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    own = np.arange(n).reshape(-1, 3)
    f2 = np.column_stack([np.arange(n, dtype=np.float64), np.full(n, V_ROW)])
    return Case(name, pts, f2, own, own if rows is None else rows, **info)


def wall_tri(x, L, e=0.0, z=5.0):
    """A steep triangle (the plane x = const, pitch 0) of height L + e: y = (L - 1 + e, L + e, L + 1 + e)."""
    return np.array([[x, L - 1 + e, z], [x, L + e, z + 1.0], [x, L + 1 + e, z]])


THRESHOLD_OUTSIDE = (1e-3, 1e-5, 1e-6)
THRESHOLD_INSIDE = (2e-8, 1e-8, 3e-9)
THRESHOLD_PER_SIDE = 48


def threshold_cases(seed=21):
    """One frame per delta: 48 triangles with true pitch -80 - delta (flat side) and 48 with -80 + delta, heights about 1.7, at
    random azimuths.  info: delta, inside (the fast test's band), side (+1 flat, -1 steep, per row)."""
    out = []
    for delta in THRESHOLD_OUTSIDE + THRESHOLD_INSIDE:
        rng = np.random.default_rng([seed, int(round(delta * 1e10))])
        tris, side = [], []
        for sgn in (1, -1):
            for _ in range(THRESHOLD_PER_SIDE):
                p = fc.flat_tri(rng, rng.uniform(1.5, 1.9), 10.0 - sgn * delta, near=True)        # pitch = -(90 - tilt)
                tris.append(_rot_y(p, rng.uniform(0.0, 2.0 * np.pi)))
                side.append(sgn)
        order = rng.permutation(len(tris))
        out.append(tri_frame("threshold/%g" % delta, np.array(tris)[order], family="threshold", delta=delta,
                             inside=delta in THRESHOLD_INSIDE, side=np.array(side)[order]))
    return out


def near_origin_case(seed=22):
    """Planes that almost pass through the camera centre (height 1e-10, coordinates of order 10), at -70 and -89 deg: the fast
    test's determinant is lost to cancellation (|det| <= 1e-9 mag) and the reference's formulation decides."""
    rng = np.random.default_rng(seed)
    tris, side = [], []
    for tilt, sgn in ((20.0, -1), (1.0, 1)):
        for _ in range(32):
            tris.append(_rot_y(fc.flat_tri(rng, 1e-10, tilt), rng.uniform(-0.3, 0.3)))
            side.append(sgn)
    order = rng.permutation(len(tris))
    return tri_frame("near_origin", np.array(tris)[order], family="near_origin", side=np.array(side)[order])


SINGULAR_MATRICES = ([[1, 0, 0], [0, 1, 0], [1, 1, 0]], [[2, 4, 8], [1, 2, 4], [4, 8, 16]], [[4, 2, 1], [4, 2, 1], [1, 8, 2]])


def _ordinary_tris(rng, count):
    """Flat (heights 1.8 .. 2.2) and steep (tilted 25 .. 60 deg, or walls) triangles far from the threshold."""
    tris = []
    for i in range(count):
        if i % 3 == 0:
            tris.append(fc.flat_tri(rng, rng.uniform(1.8, 2.2), rng.uniform(1.0, 4.0), near=True))
        elif i % 3 == 1:
            tris.append(fc.flat_tri(rng, rng.uniform(1.8, 2.2), rng.uniform(25.0, 60.0), near=True))
        else:
            tris.append(wall_tri(rng.uniform(2.0, 6.0), 1.5, rng.integers(-16, 17) / 64.0))
    return tris


def singular_cases(seed=23):
    """Rows that are exactly singular in small integers with power-of-two pivots: every LU meets an exact zero."""
    out = []
    for k, m in enumerate(SINGULAR_MATRICES):
        rng = np.random.default_rng([seed, k])
        tris = _ordinary_tris(rng, 12)
        tris.insert(5, np.array(m, dtype=np.float64))
        out.append(tri_frame("singular/%d" % k, np.array(tris), family="singular"))
    return out


LEVEL = 1.5


def level_equal_case(seed=24, flats=((LEVEL, False), (np.nextafter(LEVEL, 2.0), True)), name="level_equal"):
    """Four walls y = (L-1, L, L+1): their heights, and the mean of those, are exactly L in any summation order.  One flat triangle
    of height exactly L (h > level is false) and one a single ulp above (true)."""
    rng = np.random.default_rng(seed)
    tris = [wall_tri(2.0 + k, LEVEL) for k in range(4)]
    for h, _ in flats:
        tris.append(fc.flat_tri(rng, h, near=True))
    return tri_frame(name, np.array(tris), family="level_equal", want_selected=[sel for _, sel in flats])


N_WALLS = 90


def flag_bits_case(waves, extra_rows=0, seed=25):
    """tri2 of exactly 64 B rows (B = 64 waves threads, one flag bit per row and thread): 90 walls over and over, and flat
    triangles well above the level at rows 0, B-1, 63 B and 64 B - 1 only — bits 0 and 63 of the first and of the last thread."""
    rng = np.random.default_rng([seed, waves])
    B = WAVE * waves
    T = 64 * B + extra_rows
    tris = [fc.flat_tri(rng, 2.5 + 0.01 * k, near=True) for k in range(4)]
    tris += [wall_tri(2.0 + 0.05 * k, LEVEL, rng.integers(-16, 17) / 64.0) for k in range(N_WALLS)]
    own = np.arange(3 * len(tris)).reshape(-1, 3)
    rows = own[4 + np.arange(T) % N_WALLS]
    flat_at = np.array([0, B - 1, 63 * B, 64 * B - 1])
    rows[flat_at] = own[:4]
    return tri_frame("flag_bits/w%d%s" % (waves, "+%d" % extra_rows if extra_rows else ""), np.array(tris), rows, family="flag_bits",
                     status=so.ST_ERR_MASK if extra_rows else None, flat_at=flat_at, block=B)


def sel_words_case(seed=26, nv=100):
    """Flat triangles above the level on the survivors {0, 31, 32} and {63, 64, nv-1}: both ends of the selected bit-set's words."""
    rng = np.random.default_rng(seed)
    flat_ids = [[0, 31, 32], [63, 64, nv - 1]]
    pts = np.zeros((nv, 3))
    rest = [i for i in range(nv) if i not in flat_ids[0] + flat_ids[1]]
    rows = []
    for k, ids in enumerate(flat_ids):
        pts[ids] = fc.flat_tri(rng, 2.5 + 0.25 * k, near=True)
        rows.append(ids)
    for k in range(len(rest) // 3):
        ids = rest[3 * k:3 * k + 3]
        pts[ids] = wall_tri(2.0 + 0.05 * k, LEVEL, rng.integers(-16, 17) / 64.0)
        rows.insert(len(rows) // 2, ids)
    pts[rest[3 * (len(rest) // 3):]] = [1.0, 1.0, 1.0]                  # (the feature no row holds)
    f2 = np.column_stack([np.arange(nv, dtype=np.float64), np.full(nv, V_ROW)])
    return Case("sel_words", pts, f2, rows, rows, family="sel_words", want_selected=sorted(flat_ids[0] + flat_ids[1]))


def nan_row_case(seed=27):
    """60 ordinary triangles and one whose first vertex has x = NaN: its pitch is NaN, the row is neither flat nor steep."""
    rng = np.random.default_rng(seed)
    tris = _ordinary_tris(rng, 60)
    bad = fc.flat_tri(rng, 2.0, near=True)
    bad[0, 0] = np.nan
    tris.insert(17, bad)
    return tri_frame("nan_row", np.array(tris), family="nan_row", nan_at=17)


def selection_cases():
    """The frames every scale kernel can run (the flag_bits frames, which need a waves override, come from flag_bits_case)."""
    return threshold_cases() + [near_origin_case()] + singular_cases() + [level_equal_case(), sel_words_case(), nan_row_case()]


# ---- the longdouble truth and the decidability rule -------------------------------------------------------------------------
def _ld_rows(c):
    return c.rows_xyz().astype(np.longdouble)


def pitch_true(c):
    """Pitch of every tri2 row in degrees, Cramer's rule in np.longdouble on the stored doubles (depth_cases.normals_true's form)."""
    A = _ld_rows(c)
    a, b, cc = A[:, 0], A[:, 1], A[:, 2]

    def cr(p, q):
        return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)
    with np.errstate(all="ignore"):
        det = (a * cr(b, cc)).sum(1)
        nrm = (cr(b, cc) + cr(cc, a) + cr(a, b)) / det[:, None]
        return np.arcsin(-nrm[:, 1] / np.sqrt((nrm * nrm).sum(1))) * (np.longdouble(180.0) / np.pi)


def band_ratio(c):
    """c_y^2 / |c|^2 / sin^2(80 deg) - 1 per row, c = (p1 - p0) x (p2 - p0), in np.longdouble: what the fast test's band is about."""
    A = _ld_rows(c)
    e1, e2 = A[:, 1] - A[:, 0], A[:, 2] - A[:, 0]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    s2 = np.sin(np.longdouble(80.0) * np.pi / np.longdouble(180.0)) ** 2
    return cy * cy / (cx * cx + cy * cy + cz * cz) / s2 - 1


def cond2(c):
    with np.errstate(all="ignore"):
        A = c.rows_xyz()
        ok = np.isfinite(A).all(axis=(1, 2))
        k = np.full(len(A), np.inf)
        k[ok] = np.linalg.cond(A[ok])
        return k


def pitch_margin_deg(c, const=C_PITCH):
    return const * U52 * cond2(c) * 180.0 / np.pi


def decided_rows(c):
    """(decided, flat_true): rows whose longdouble pitch is farther from -80 deg than the margin — on those NumPy, the kernel's LU
    and the fast test must all agree with the truth — plus the rows whose pitch is NaN (neither flat nor steep, whatever rounds)."""
    p = pitch_true(c)
    with np.errstate(invalid="ignore"):
        far = np.abs(p - THR_DEG) > pitch_margin_deg(c)
        return np.asarray(far | np.isnan(p)), np.asarray(p < THR_DEG)


def numpy_pitch_error_units(c):
    """|pitch_numpy - pitch_true| / (2^-52 cond_2(A) 180/pi) per row (NaN rows and singular frames excluded by the caller)."""
    got = c.oracle().sel.pitch_deg
    return np.asarray(np.abs(got - pitch_true(c)), dtype=np.float64) / (U52 * cond2(c) * 180.0 / np.pi)


def only_decided(c):
    """The same frame with the undecided rows taken out of tri2 (the features stay): what the HOT and EXACT runs, which report
    counts and not rows, are compared on."""
    dec, _ = decided_rows(c)
    if dec.all():
        return c
    info = dict(c.info)
    for k in ("side",):
        if k in info:
            info[k] = info[k][dec]
    return Case(c.name + "/decided", c.f3, c.f2, c.tri1, c.tri2[dec], c.vote, c.status, **info)


# ---- CPU stand-ins of the fast test and the flag words ----------------------------------------------------------------------
def fast_pitch_test(c, s2_lo=S2 * (1 - BAND), s2_hi=S2 * (1 + BAND), safe_rel=1e-9):
    """classify_triangle's division-free test in float64 (without its FMAs: a few ulps, far below the band): (flat, steep); a row
    that is neither goes to the reference's formulation."""
    A = c.rows_xyz()
    with np.errstate(all="ignore"):
        e1, e2 = A[:, 1] - A[:, 0], A[:, 2] - A[:, 0]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        tx, ty, tz = A[:, 0, 0] * cx, A[:, 0, 1] * cy, A[:, 0, 2] * cz
        det, mag = (tx + ty) + tz, (np.abs(tx) + np.abs(ty)) + np.abs(tz)
        c2, q2, sy = cz * cz + (cy * cy + cx * cx), cy * cy, cy * det
        safe = np.abs(det) > safe_rel * mag
        flat = safe & (sy > 0) & (q2 > s2_hi * c2)
        steep = safe & ((sy <= 0) | (q2 < s2_lo * c2))
    return flat, steep


def mutant_pitch_no_band(c):
    return fast_pitch_test(c, S2, S2)


def mutant_pitch_band_at_85(c):
    s2 = np.sin(np.deg2rad(85.0)) ** 2
    return fast_pitch_test(c, s2 * (1 - BAND), s2 * (1 + BAND))


def flag_words(flat, block, shift_mask=63):
    """Which rows the second sweep takes for flat: thread tid keeps bit (kk & shift_mask) of one word for its kk-th row,
    row = kk block + tid.  shift_mask = 31 is the mutant."""
    flat = np.asarray(flat, dtype=bool)
    T = len(flat)
    kk, tid = np.arange(T) // block, np.arange(T) % block
    words = np.zeros((block, shift_mask + 1), dtype=bool)
    words[tid[flat], kk[flat] & shift_mask] = True
    return words[tid, kk & shift_mask]


def mutant_select_ge(c):
    """tri_valid with `>=` at the level."""
    s = c.oracle().sel
    with np.errstate(invalid="ignore"):
        return s.valid_pitch & (s.heights >= s.height_level)


# ============================================================================================================================
# redo family: which frames the HOT kernel hands to the exact pass
# ============================================================================================================================
def control_margins(c):
    """The oracle's margins of an ordinary frame: (something selected, status, min |h - level| / mean |h| over the flat rows,
    min |pitch + 80| in degrees)."""
    r = c.oracle()
    s = r.sel
    flat = s.valid_pitch
    level_gap = np.min(np.abs(s.heights[flat] - s.height_level)) / np.mean(np.abs(s.heights)) if flat.any() else np.inf
    return len(s.selected_ids) > 0, r.status, float(level_gap), float(np.min(np.abs(s.pitch_deg - THR_DEG)))


def control_ok(c):
    sel, status, gap, pitch = control_margins(c)
    return sel and status != so.ST_LEVEL and gap >= 1e-9 and pitch >= 1e-5


def control_cases(count=64, seed=4711):
    """Ordinary frames: synth.synth_frame with 300 - 700 features (those below the vanishing row), SciPy's triangulations."""
    from mvoscalerecovery_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(300, 701))
        f3, f2 = synth.synth_frame(i, n, base_seed=seed, upper_fraction=0.1)
        low = f2[:, 1] > so.VANISH
        r = so.frame_raw_scale(f3[low], f2[low], ABS_REF, **ORACLE_KW)
        c = Case("control/%d" % i, f3[low], f2[low], r.tri1, r.tri2, family="control", n_synth=n)
        c._ores = r
        out.append(c)
    return out


def nothing_selected_case():
    """Walls at level 1.5 and flat triangles well below it: no row is selected (:277-279)."""
    return level_equal_case(seed=31, flats=((1.0, False), (1.1, False)), name="nothing_selected")


def lone_bins_case(seed=32):
    """One wide flat triangle above the level whose three y' lie in three different histogram bins: remove_single drops all three
    and the road model falls back on the level (ST_LEVEL, :334-335)."""
    tris = [wall_tri(2.0 + k, LEVEL) for k in range(4)]
    tris.append(np.array([[-6.0, 2.05, 8.0], [6.0, 2.35, 9.0], [0.5, 2.65, 20.0]]))
    return tri_frame("lone_bins", np.array(tris), family="lone_bins")


def redo_cases():
    """(case, expected): True = the HOT kernel must leave it for the exact pass, False = it must not."""
    th = {c.info["delta"]: c for c in threshold_cases()}
    out = [(c, False) for c in control_cases() if control_ok(c)]
    out += [(only_decided(th[1e-8]), True), (level_equal_case(), True), (nothing_selected_case(), True), (lone_bins_case(), True),
            (th[1e-5], False)]
    return out


# ============================================================================================================================
# on the device
# ============================================================================================================================
def run_scale(ctx, cases, kind="hot", waves=0, vote="reference", layout="survivors", hot_only=False, hist=None, mutate=None, far_table=True):
    """mvosr_scale_batch on `cases` as one batch.  kind: "hot" (the product kernel + its exact pass), "exact" (stage outputs),
    "full" (per-triangle outputs).  layout: "survivors", "features" (tri2 numbered over the features: the dense kernels),
    "tiled".  hist: ask for the histogram / statistics outputs (default: with "exact"; they do not change the mode).  mutate(pf):
    called on the packed batch before it is uploaded.  far_table=False: the tiled layout without the packer's table of far
    vertices (tile_far / tile_far_off cleared).  Returns (PackedFrames, {name: host array})."""
    from mvoscalerecovery_amd import packing
    from mvoscalerecovery_amd.engine import DeviceBatch, DeviceOutputs, ScaleEngine
    pf = packing.pack_features([c.f3 for c in cases], [c.f2 for c in cases], vanish=VANISH)
    packing.attach_tri1(pf, [c.tri1 for c in cases])
    masks = [np.asarray(c.oracle().valid) for c in cases]
    if layout == "tiled":
        packing.apply_tile_order(pf)
        masks = [m if pf.extra["perm"][f] is None else m[pf.extra["perm"][f]] for f, m in enumerate(masks)]
    packing.attach_tri2(pf, [c.tri2 for c in cases], masks, feature_ids=layout != "survivors")
    if layout == "tiled":
        assert pf.tile_w == packing.TILE_W
    if mutate is not None:
        mutate(pf)
    eng = ScaleEngine(ABS_REF, ctx=ctx, camera_pitch=0.0, check_triangle=vote)
    db = DeviceBatch(ctx, pf)
    if not far_table:
        st = db.struct()
        st.tile_far, st.tile_far_off = None, None
    out = DeviceOutputs(ctx, db, counts=True, stage=kind in ("exact", "full"), per_triangle=kind == "full",
                        hist=kind == "exact" if hist is None else hist)
    eng.scale_batch(db, out, waves=waves, hot_only=hot_only)
    ctx.sync()
    res = {k: out.get(k) for k in out.bufs}
    out.free()
    db.free()
    return pf, res


def run_vote(ctx, cases, waves=0, vote="reference"):
    """mvosr_outlier_vote_batch on `cases` as one batch: (PackedFrames, status, vote_counters)."""
    from mvoscalerecovery_amd import packing
    from mvoscalerecovery_amd.engine import DeviceBatch, DeviceOutputs, ScaleEngine
    pf = packing.pack_features([c.f3 for c in cases], [c.f2 for c in cases], vanish=VANISH)
    packing.attach_tri1(pf, [c.tri1 for c in cases])
    eng = ScaleEngine(ABS_REF, ctx=ctx, camera_pitch=0.0, check_triangle=vote)
    db = DeviceBatch(ctx, pf, with_tri2=False)
    out = DeviceOutputs(ctx, db, counts=True, stage=True)
    eng.outlier_vote_batch(db, out, waves=waves)
    ctx.sync()
    st, cnt, counts = out.get("status"), out.get("vote_counters"), out.get("counts")
    out.free()
    db.free()
    return pf, st, cnt, counts
