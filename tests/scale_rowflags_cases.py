"""Crafted frames for the per-thread bookkeeping of phase_select's first sweep (csrc/mvosr_kernels.hip: RowBook, LeanRowBook) —
the flag words, the steep count, the rare flags and the sums — shared by tests/test_scale_rowflags_cases.py (CPU) and
tests/test_gpu_scale_rowflags.py.  Test infrastructure.

The frames are scale_cases.Case frames of disjoint small triangles (tri_frame): every feature on one pixel row, so nobody is
voted out and tri2's ids are the features' own.  Expected values come from oracle.scale_oracle through Case.oracle().

`lean_book` is a CPU twin of the lean form's bookkeeping (LeanRowBook: the product's HOT kernels, at most 64 rows per thread),
thread by thread: the low 32-bit half filed at the end of the 16th trip of kTC = 2 rows, the high one behind the sweep, the steep count as "my rows less the flat ones less the rare neither ones", the rare flags accumulated over
all of a thread's rows, the sums with a select to +0.0.  Its `mutant` argument switches in one subtly wrong rule at a time;
tests/test_scale_rowflags_cases.py asserts that every mutant differs from the oracle on at least one case.
What scale_cases.py and scale_chunk_cases.py already pin down (64 B rows with flat rows at bits 0 and 63 of the first and last
thread, row counts around one and two chunks, an id out of range in the last partial chunk) is not repeated here."""
import numpy as np

import flat_cases as fc
import scale_cases as sc
from oracle import scale_oracle as so

KTC = 2                                   # kTC: rows per thread and trip
SPECIAL_BITS = (0, 31, 32, 63, 64, 95, 96, 127)
N_ABOVE, N_BELOW, N_WALL = 2, 4, 16       # ordinary flat triangles above / below the level, walls around it
MUTANTS = ("half0_only", "npitch_low_half", "inband_is_steep", "rare_last_row", "mask_by_multiply")


# ============================================================================================================================
# flag words
# ============================================================================================================================
def lane_words(block, fw, seed):
    """(block, 64 fw) bool: bit kk of lane l's flag words.  A quarter of the bits at random; the special bits (0, 31, 32, 63 and,
    fw = 2, 64, 95, 96, 127) of lane l are bits 0 .. 5 of l and the xor of two neighbouring ones, so that every one of them is set
    in some lanes and clear in others and no two of them agree in all lanes."""
    rng = np.random.default_rng([seed, block, fw])
    bits = rng.random((block, 64 * fw)) < 0.25
    lanes = np.arange(block)
    for j, kk in enumerate(b for b in SPECIAL_BITS if b < 64 * fw):
        bits[:, kk] = (lanes >> j) & 1 if j < 6 else ((lanes >> (j - 6)) ^ (lanes >> (j - 5))) & 1
    return bits


def marker_rows(block, fw):
    """(kk, lane) of the rows that each hold a flat triangle of their own, above the level: the selected set has that triangle's
    three vertices iff that one bit is kept."""
    m = [(0, block - 1), (31, 0), (32, block - 1), (63, 0)]
    if fw == 2:
        m += [(64, block - 1), (95, 0), (96, block - 1), (127, 0)]
    return m


def rowflag_bits_case(block, fw=1, short=0, seed=41):
    """tri2 of 64 fw block - short rows (fw = 2: the dense kernels' two 64-bit words per thread); row kk block + l is flat iff bit
    kk of lane l's word is set.  The marker rows are flat
    and hold a flat triangle nobody else holds; the last row is flat; the other flat rows hold one of N_ABOVE triangles above the
    level or N_BELOW below it, the other rows a wall."""
    rng = np.random.default_rng([seed, block, fw, short])
    T = 64 * fw * block - short
    bits = lane_words(block, fw, seed)
    markers = marker_rows(block, fw)
    for kk, l in markers:
        bits[l, kk] = True
    last = T - 1
    bits[last % block, last // block] = True
    tris = [fc.flat_tri(rng, 3.0 + 0.125 * k, near=True) for k in range(len(markers))]
    tris += [fc.flat_tri(rng, 2.5 + 0.125 * k, near=True) for k in range(N_ABOVE)]
    tris += [fc.flat_tri(rng, 1.0 + 0.0625 * k, near=True) for k in range(N_BELOW)]
    tris += [sc.wall_tri(2.0 + 0.05 * k, sc.LEVEL, rng.integers(-16, 17) / 64.0) for k in range(N_WALL)]
    own = np.arange(3 * len(tris)).reshape(-1, 3)
    t = np.arange(T)
    flat = bits[t % block, t // block]
    n_m = len(markers)
    pick = np.where(flat, n_m + rng.integers(0, N_ABOVE + N_BELOW, T), n_m + N_ABOVE + N_BELOW + rng.integers(0, N_WALL, T))
    for j, (kk, l) in enumerate(markers):
        pick[kk * block + l] = j
    return sc.tri_frame("rowflag_bits/b%d/fw%d%s" % (block, fw, "-%d" % short if short else ""), np.array(tris), own[pick],
                        family="rowflag_bits", block=block, fw=fw, flat=flat, n_markers=n_m)


# ============================================================================================================================
# the CPU twin of the lean bookkeeping
# ============================================================================================================================
def lean_book(flat, steep, heights, block, singular=None, undecided=None, mutant=None):
    """LeanRowBook over T <= 64 block rows (row t belongs to thread t % block, as its row t // block), given every row's
    decision.  Returns dict(seen: the rows the second sweep takes for flat, n_pitch, n_steep, hsum, singular, undecided) — the
    counts and the sum over all threads (the sum in float64, thread by thread in row order, then over the threads: the order is
    not the kernel's, which only matters for the last bits).  Mutants: "half0_only" (the bit placed by kk & 31, always in the
    low half), "npitch_low_half", "inband_is_steep" (a row that went to the reference's formulation and did not come back
    steep — flat inside the band, or neither — is counted steep all the same: only the out-of-range rows are taken off),
    "rare_last_row", "mask_by_multiply"."""
    assert mutant is None or mutant in MUTANTS
    flat, steep = np.asarray(flat, dtype=bool), np.asarray(steep, dtype=bool)
    T = len(flat)
    assert T <= 64 * block
    z = np.zeros(T, dtype=bool)
    singular = z if singular is None else np.asarray(singular, dtype=bool)
    undecided = z if undecided is None else np.asarray(undecided, dtype=bool)
    lanes = np.arange(block)
    lo, hi, cur = (np.zeros(block, dtype=np.uint64) for _ in range(3))
    neither, inband = np.zeros(block, dtype=np.int64), np.zeros(block, dtype=np.int64)
    f_sing, f_und = np.zeros(block, dtype=bool), np.zeros(block, dtype=bool)
    hsum = np.zeros(block)
    trips = range(0, (T + block - 1) // block, KTC)

    def rows_of(kk):
        t = kk * block + lanes
        ok = t < T
        return np.where(ok, t, 0), ok

    with np.errstate(all="ignore"):
        for kk0 in trips:
            for kk in range(kk0, kk0 + KTC):
                t, ok = rows_of(kk)
                cur |= (ok & flat[t]).astype(np.uint64) << np.uint64(kk & 31)
                neither += ok & ~flat[t] & ~steep[t]
                inband += ok & undecided[t] & ~steep[t]
                if mutant == "rare_last_row":                # the flags of the row at hand replace the thread's, they are not or-ed in
                    f_sing, f_und = np.where(ok, singular[t], f_sing), np.where(ok, undecided[t], f_und)
                else:
                    f_sing, f_und = f_sing | (ok & singular[t]), f_und | (ok & undecided[t])
                h = np.where(ok, heights[t], 0.0)
                if mutant == "mask_by_multiply":
                    hsum += h * (ok & steep[t])                  # inf * 0 = NaN
                else:
                    hsum += np.where(ok & steep[t], h, 0.0)
            if kk0 + KTC == 32:                                  # end_trip
                lo, cur = lo | cur, np.zeros(block, dtype=np.uint64)
        if T > 32 * block and mutant != "half0_only":           # close
            hi = cur
        else:
            lo = lo | cur
        pop = lambda w: np.array([bin(int(x)).count("1") for x in w], dtype=np.int64)
        npitch = pop(lo) if mutant == "npitch_low_half" else pop(lo) + pop(hi)
        my_rows = (T + block - 1 - lanes) // block
        nsteep = my_rows - npitch - neither + (inband if mutant == "inband_is_steep" else 0)
        seen = np.zeros(T, dtype=bool)
        cur = lo.copy()
        for kk0 in trips:
            for kk in range(kk0, kk0 + KTC):
                t, ok = rows_of(kk)
                seen[t[ok]] = ((cur >> np.uint64(kk & 31)) & np.uint64(1)).astype(bool)[ok]
            if kk0 + KTC == 32:                                  # end_mark_trip
                cur = hi.copy()
        return dict(seen=seen, n_pitch=int(npitch.sum()), n_steep=int(nsteep.sum()), hsum=float(hsum.sum()),
                    singular=bool(f_sing.any()), undecided=bool(f_und.any()))


def oracle_rows(c):
    """(flat, steep, heights, singular) per row of tri2 as the oracle has them (a singular frame: no decisions, one flag)."""
    s = c.oracle().sel
    with np.errstate(invalid="ignore"):
        return s.valid_pitch, s.pitch_deg >= sc.THR_DEG, s.heights, s.singular


def book_of(c, block, mutant=None):
    """lean_book on the oracle's decisions for frame c; `undecided`: the rows the fast test leaves to the reference's formulation."""
    flat, steep, h, _ = oracle_rows(c)
    f_fast, s_fast = sc.fast_pitch_test(c)
    und = ~(f_fast | s_fast)
    sing = np.zeros(len(flat), dtype=bool)
    if "singular_at" in c.info:
        sing[c.info["singular_at"]] = True
    return lean_book(flat, steep, h, block, singular=sing, undecided=und, mutant=mutant)


# ============================================================================================================================
# steep count
# ============================================================================================================================
def steep_count_case(kind, seed=43, n_rows=300):
    """kind: "none" (flat rows only: the level is the mean of nothing, NaN), "one" (one wall among flat rows), "all" (walls only:
    nothing flat), "nan" (walls, flat rows and one row whose pitch is NaN: neither flat nor steep)."""
    rng = np.random.default_rng([seed, len(kind)])
    flats = [fc.flat_tri(rng, 2.0 + 0.125 * k, near=True) for k in range(4)] + [fc.flat_tri(rng, 1.0 + 0.125 * k, near=True) for k in range(2)]
    walls = [sc.wall_tri(2.0 + 0.05 * k, sc.LEVEL, rng.integers(-16, 17) / 64.0) for k in range(12)]
    info = {}
    if kind == "none":
        tris, pick = flats, rng.integers(0, len(flats), n_rows)
    elif kind == "one":
        tris, pick = flats + walls[:1], rng.integers(0, len(flats), n_rows)
        pick[n_rows // 2] = len(flats)
    elif kind == "all":
        tris, pick = walls, rng.integers(0, len(walls), n_rows)
    else:
        bad = fc.flat_tri(rng, 2.0, near=True)
        bad[0, 0] = np.nan
        tris, pick = flats + walls + [bad], rng.integers(0, len(flats) + len(walls), n_rows)
        info["nan_at"] = [0, n_rows // 3, n_rows - 1]
        pick[info["nan_at"]] = len(tris) - 1
    own = np.arange(3 * len(tris)).reshape(-1, 3)
    return sc.tri_frame("steep_count/" + kind, np.array(tris), own[pick], family="steep_count", kind=kind, **info)


def refused_among_steep_case(seed=44, n_rows=300):
    """(refused, good): walls and a few flat rows, and in `refused` one row — walls before and behind it — with an id one past
    the range.  The kernels refuse it (MVOSR_ST_ERR_MASK) and still write its level: the mean over the steep rows without that
    row, i.e. the level of `good`, the same frame without the row."""
    rng = np.random.default_rng(seed)
    tris = [fc.flat_tri(rng, 2.5 + 0.125 * k, near=True) for k in range(3)]
    tris += [sc.wall_tri(2.0 + 0.05 * k, sc.LEVEL, rng.integers(-16, 17) / 64.0) for k in range(12)]
    own = np.arange(3 * len(tris)).reshape(-1, 3)
    pick = 3 + rng.integers(0, 12, n_rows)
    pick[::17] = rng.integers(0, 3, len(pick[::17]))
    at = n_rows // 2 + 1
    pick[at - 2:at + 3] = 3 + np.arange(5)                     # (walls on both sides)
    rows = own[pick]
    good = sc.tri_frame("refused_among_steep/good", np.array(tris), np.delete(rows, at, 0), family="steep_count")
    rows = rows.copy()
    rows[at, 1] = 3 * len(tris)
    bad = sc.tri_frame("refused_among_steep", np.array(tris), rows, family="steep_count", status=so.ST_ERR_MASK, bad_at=at)
    bad._ores = good.oracle()
    return bad, good


# ============================================================================================================================
# rare flags
# ============================================================================================================================
RARE_POSITIONS = ("first", "last", "only")


def rare_row_case(what, where, block, seed=45):
    """Ordinary flat and steep rows and ONE rare row: `what` = "singular" (an exactly singular matrix) or "band" (a flat triangle
    1e-8 deg inside the fast test's band: the reference's formulation decides it).  `where`: "first" = row 0, thread 0's first of
    three rows; "last" = the frame's last row, the last of its thread's three; "only" = row block - 1 of block + 10 rows, the
    last thread's only row."""
    rng = np.random.default_rng([seed, block, RARE_POSITIONS.index(where), len(what)])
    T = block + 10 if where == "only" else 2 * block + 10
    at = {"first": 0, "last": T - 1, "only": block - 1}[where]
    tris = sc._ordinary_tris(rng, 24)
    if what == "singular":
        tris.append(np.array(sc.SINGULAR_MATRICES[1], dtype=np.float64))
    else:
        tris.append(sc._rot_y(fc.flat_tri(rng, 2.0, 10.0 - 1e-8, near=True), rng.uniform(0.0, 2.0 * np.pi)))
    own = np.arange(3 * len(tris)).reshape(-1, 3)
    pick = rng.integers(0, 24, T)
    pick[at] = 24
    info = {"singular_at": [at]} if what == "singular" else {"band_at": at}
    return sc.tri_frame("rare/%s/%s/b%d" % (what, where, block), np.array(tris), own[pick], family="rare", block=block, **info)


# ============================================================================================================================
# sums
# ============================================================================================================================
def overflow_case(seed=46):
    """A flat triangle at y = 6e307 (three times its height is inf) beside finite walls.  NOT a usable frame: see
    test_scale_rowflags_cases.py::test_the_overflow_frame_is_not_decidable — the oracle's LU cannot resolve a normal of
    1.7e-308, calls the row steep and its level is inf."""
    rng = np.random.default_rng(seed)
    big = fc.flat_tri(rng, 6e307, near=True)
    tris = [sc.wall_tri(2.0 + 0.05 * k, sc.LEVEL, rng.integers(-16, 17) / 64.0) for k in range(8)] + [big]
    return sc.tri_frame("overflow", np.array(tris), family="sums")

