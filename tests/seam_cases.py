"""Crafted frames and a NumPy twin for the seams of the LDS-resident scale kernels (csrc/mvosr_kernels.hip) that are built of LDS
round trips and not of arithmetic: the tail (frame_tail, SC > 0), which counts and packs the selected survivors, and step 1 of the
survivors' compaction (phase_vote), for which the frames here are scale_cases' keep masks at the sizes where lanes fall past the
frame's end.  Shared by tests/test_seam_cases.py (CPU) and tests/test_gpu_seams.py.  Test infrastructure.

The twin restates the tail's rule as the kernel has it, on the same words:

  The selected bit-set lives where the vote counters were.  Words [0, (n + 31) / 32) were zeroed behind the compaction (n: the
  frame's features), the bits of selected SURVIVORS (ids < nvalid) were set, and every word from (n + 31) / 32 on still holds two
  biased 16-bit counters (or, past the counters, anything).  Every wave reads all WAVES SC 2 words of the instantiation's
  capacity, keeps those with index < (nvalid + 31) / 32, and takes nsel = their popcount and its own base = the popcount of the
  words in front of its slice [w per, min(nvalid, (w + 1) per)), per = ceil(nvalid / B) 64.  Point j of the slice goes to
  base + (selected points of the slice in front of j).

It is checked against one-line statements (np.flatnonzero / np.cumsum) in test_seam_cases.py, and each `mutant` argument is a
subtly wrong kernel that at least one case there must expose.

Frames.  Every feature sits on pixel row V_ROW (all vote products are +-0: nobody is flagged, nvalid = n) unless the frame comes
from scale_cases.compaction_case.  The selected set is prescribed through tri2: the selected vertices lie on one gently tilted
road plane y = Y_FLAT + TILT x, so that ANY three of them are a flat row whose height is above the level; everybody else stands in
walls of height exactly LEVEL.  A selected set is a union of rows, i.e. it has at least three members: "only index 0" and "only
the last index" are the three first / last survivors.  When every survivor is selected no wall is left to give a level: two
vertices are then lowered to Y_LOW under a third (a steep row of lower mean height) and tied to the plane by far vertices."""
import numpy as np

import scale_cases as sc
from oracle import scale_oracle as so

WAVE = 64
POISON = 0xDEADBEEF                 # what the twin puts where the kernel must not look (past the counters)
Y_FLAT, TILT, Y_LOW = 2.55, 0.004, 2.3
# (n, waves_per_frame, (WAVES, SC)): the sizes of the issue through the instantiation that takes them
PLAN = ((64, 1, (1, 8)), (65, 1, (1, 8)), (128, 1, (1, 8)), (320, 1, (1, 8)),
        (321, 4, (4, 4)), (511, 4, (4, 4)), (512, 4, (4, 4)), (513, 4, (4, 4)), (1024, 4, (4, 4)),
        (1025, 4, (4, 8)), (1152, 4, (4, 8)),
        (1153, 8, (8, 4)), (2047, 8, (8, 4)), (2048, 8, (8, 4)),
        (2049, 8, (8, 8)),
        (2048, 16, (16, 4)), (2049, 16, (16, 4)))
# compaction masks (scale_cases.compaction_masks): n = capacity, capacity - 1, and an n that is no multiple of 64 and leaves
# lanes past the frame's end in several waves
COMPACT_PLAN = ((512, 1, (1, 8)), (511, 1, (1, 8)), (300, 1, (1, 8)),
                (1024, 4, (4, 4)), (1023, 4, (4, 4)), (700, 4, (4, 4)),
                (2048, 8, (8, 4)), (2047, 8, (8, 4)), (1500, 8, (8, 4)),
                (4096, 16, (16, 4)), (4095, 16, (16, 4)), (3000, 16, (16, 4)))


# ============================================================================================================================
# the twin
# ============================================================================================================================
def popcount(words):
    words = np.asarray(words, dtype=np.uint64)
    return np.array([bin(int(w)).count("1") for w in words.reshape(-1)], dtype=np.int64).reshape(words.shape)


def tail_partition(nvalid, waves):
    """(per, begin[w], end[w]): the waves' slices of the survivors (end < begin never: an empty slice has end == min(begin, nvalid))."""
    B = waves * WAVE
    per = -(-nvalid // B) * WAVE
    begin = np.arange(waves) * per
    end = np.maximum(np.minimum(nvalid, begin + per), np.minimum(begin, nvalid))
    return per, begin, end


def lds_words(n, counters, selected_ids, capacity_words):
    """The bit-set's region as the tail finds it: `capacity_words` 32-bit words."""
    words = np.full(max(capacity_words, (n + 1) // 2), POISON, dtype=np.uint64)
    half = np.zeros(2 * ((n + 1) // 2), dtype=np.uint64)
    half[:n] = (np.asarray(counters, dtype=np.int64) + sc.COUNTER_BIAS).astype(np.uint64)
    if n % 2:
        half[n] = sc.COUNTER_BIAS + 1                      # (the pad feature's half: staged like any other, never voted on)
    words[:(n + 1) // 2] = half[0::2] | (half[1::2] << np.uint64(16))
    words[:(n + 31) // 32] = 0
    for j in np.asarray(selected_ids, dtype=np.int64):
        words[j >> 5] |= np.uint64(1) << np.uint64(j & 31)
    return words[:capacity_words]


def tail_twin(words, nvalid, waves, sc_, mutant=None):
    """frame_tail<WAVES, MODE, SC> on the words: (nsel, dense list of survivor ids in the order of the stores, base[w]).
    mutant: "stale" (no mask by word index), "own_word" (the base takes the wave's own first word too)."""
    cap_words = waves * sc_ * 2
    assert len(words) == cap_words
    per, begin, end = tail_partition(nvalid, waves)
    assert per <= sc_ * WAVE
    nwords = (nvalid + 31) >> 5
    wi = np.arange(cap_words)
    pc = popcount(words)
    live = np.ones(cap_words, bool) if mutant == "stale" else wi < nwords
    nsel = int(pc[live].sum())
    dense = np.full(max(nsel, 0) + 4 * cap_words * 32, -1, dtype=np.int64)      # (room for a mutant's wild base)
    bases = []
    for w in range(waves):
        front = begin[w] >> 5
        base = int(pc[live & (wi <= front if mutant == "own_word" else wi < front)].sum())
        bases.append(base)
        for k in range(sc_):
            j = begin[w] + k * WAVE + np.arange(WAVE)
            jc = np.minimum(j, max(nvalid - 1, 0))
            bit = ((words[jc >> 5] >> (jc & 31).astype(np.uint64)) & np.uint64(1)).astype(bool)
            sel = (j < end[w]) & bit
            dense[base + np.cumsum(sel)[sel] - 1] = j[sel]
            base += int(sel.sum())
    return nsel, dense[:max(nsel, 0)], np.array(bases)


# ============================================================================================================================
# frames with a prescribed selected set
# ============================================================================================================================
def _road_points(m, rng):
    """m points on the road plane, three to a small well-shaped triangle, the triangles on a grid."""
    p = np.arange(m)
    r, t = p // 3, p % 3
    off = np.array([[0.0, 0.0], [0.7, 0.1], [0.2, 0.8]])
    x = -4.0 + (r % 9) + off[t, 0] + rng.uniform(0.0, 0.04, m)
    z = 6.0 + 2.0 * (r // 9) + off[t, 1] + rng.uniform(0.0, 0.04, m)
    return np.column_stack([x, Y_FLAT + TILT * x, z])


def _rows_over(ids):
    """Rows of three over `ids` in order; a remainder is covered by one more row over the last three."""
    ids = np.asarray(ids, dtype=np.int64)
    rows = [ids[3 * r:3 * r + 3] for r in range(len(ids) // 3)]
    if len(ids) % 3:
        rows.append(ids[-3:])
    return rows


def selected_frame(name, n, ids, stale_rows=0, seed=41):
    """A frame of n features, all survivors, whose selected set is exactly `ids` (a sorted union of triples, or empty).
    stale_rows: that many extra tri1 rows on the features whose counters share the words just past the bit-set's zeroed part."""
    ids = np.array(sorted(set(int(i) for i in ids)), dtype=np.int64)
    assert len(ids) == 0 or (len(ids) >= 3 and ids[0] >= 0 and ids[-1] < n)
    rng = np.random.default_rng([seed, n, len(ids)])
    rest = np.setdiff1d(np.arange(n), ids)
    pts = np.ones((n, 3))
    rows = []
    if len(rest) >= 3:
        flat = ids
        if len(ids) == 0:                                        # flat rows BELOW the level: counted, not selected
            low = rest[:6]
            rest = rest[6:]
            p = _road_points(len(low), rng)
            p[:, 1] -= 1.5
            pts[low] = p
            rows += _rows_over(low)
        pts[flat] = _road_points(len(flat), rng)
        rows += _rows_over(flat)
        for k in range(len(rest) // 3):                          # walls: heights exactly LEVEL, in any summation order
            w = rest[3 * k:3 * k + 3]
            pts[w] = sc.wall_tri(2.0 + 0.01 * (k % 400), sc.LEVEL, z=5.0 + (k // 400))
            rows.insert(len(rows) // 2, w)
    else:
        assert len(rest) == 0 and n >= 32
        flat, (c2, c1) = ids[:-2], ids[-2:]
        pts[flat] = _road_points(len(flat), rng)
        a = pts[flat[0]]
        pts[c1] = [a[0] - 0.25, Y_LOW, a[2] + 0.01]
        pts[c2] = [a[0] + 0.25, Y_LOW, a[2] + 0.01]
        rows += _rows_over(flat)
        rows.insert(1, np.array([c1, c2, flat[0]]))              # steep, mean height below every flat row's: the level
        rows.append(np.array([c1, flat[24], flat[26]]))          # flat rows that select c1 and c2 (far vertices: a tilt of 2 deg)
        rows.insert(3, np.array([c2, flat[21], flat[23]]))
    f2 = np.column_stack([np.arange(n, dtype=np.float64), np.full(n, sc.V_ROW)])
    tri1 = [np.arange(n - n % 3).reshape(-1, 3)]
    if stale_rows:
        f0 = min(2 * ((n + 31) // 32), n - 8)
        tri1.append(np.tile(np.array([[f0, f0 + 1, f0 + 2], [f0 + 3, f0 + 4, f0 + 5], [f0 + 5, f0 + 6, f0 + 7]]), (stale_rows // 3, 1)))
    c = sc.Case(name, pts, f2, np.concatenate(tri1), np.array(rows), family="seam", want_selected=ids, n_features=n)
    return c


def selected_sets(n, waves):
    """name -> selected ids for a frame of n survivors run with `waves` wavefronts."""
    per, begin, end = tail_partition(n, waves)
    full = [w for w in range(waves) if end[w] > begin[w]]
    edges = sorted({int(begin[w]) for w in full} | {int(end[w]) - 1 for w in full})
    while len(edges) < 3:                                       # (one wave, tiny frame)
        edges = sorted(set(edges) | {len(edges)})
    bits = [j for j in range(n) if j % 32 in (0, 31)]
    return {"none": [], "all": range(n), "front3": [0, 1, 2], "back3": [n - 3, n - 2, n - 1],
            "slice_edges": edges, "bit0_bit31": bits}


def seam_cases(n, waves):
    out = [selected_frame("seam/n%d/w%d/%s" % (n, waves, tag), n, ids) for tag, ids in selected_sets(n, waves).items()]
    out.append(selected_frame("seam/n%d/w%d/stale" % (n, waves), n, selected_sets(n, waves)["slice_edges"], stale_rows=600))
    return out


def handed_over_case():
    """A flat row exactly on the level: the HOT kernel leaves the frame to the exact pass (scale_cases.level_equal_case)."""
    return sc.level_equal_case()


def mixed_batch():
    """One launch's worth: every selected set at a size of the <8,4> class, compaction masks, and the frame that is handed over."""
    out = seam_cases(1153, 8)[:4] + seam_cases(2047, 8)[3:] + seam_cases(321, 8)[2:5]
    out += sc.compaction_cases(1500, 8, 4)[:4]
    out.insert(5, handed_over_case())
    return out


def small_batch():
    """Frames of the 1-wave class (n <= 320), for the ragged path's second class."""
    return seam_cases(65, 1)[1:4] + seam_cases(320, 1)[2:6]


def oracle_words(c, waves, sc_):
    """The words the tail of instantiation (waves, sc) finds for case c, from the oracle's counters and selected set."""
    r = c.oracle()
    return lds_words(c.n, r.counters, r.sel.selected_ids, waves * sc_ * 2), int(np.asarray(r.valid).sum())
