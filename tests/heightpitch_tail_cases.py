"""The estimator's frame-to-frame carry (csrc/mvosr_heightpitch_tail.hip, mvosr_height_pitch_tail_batch) restated in NumPy, and the
crafted chunks tests/test_gpu_heightpitch_resident.py hands the kernel through the C ABI — shared with
tests/test_heightpitch_resident_cases.py (CPU).  Test infrastructure.

* `tail`: the body of HeightPitchEstimator.process_batch's loop (calculate_height_pitch.py:140, :163-167, :202-203) for one chunk:
  per-frame records, the error word, the carry-out — from the chunk's kernel outputs as plain arrays.  np.mean is the reference for
  the one value a carried frame computes.
* `crafted_chunk`: hand-made outputs, masks and planes — no triangulation, no RANSAC.
"""
import numpy as np

FOCUS, CY, MIN_POINTS = 718.856, 185.2157, 12
ST_SINGULAR, ST_MASK, ST_EMPTY, ST_RS_FEW = 7, 8, 9, 11
ERR_SINGULAR, ERR_MASK, ERR_EMPTY, ERR_NO_MODEL, ERR_NO_PREVIOUS, ERR_STATUS, ERR_UPSTREAM = 1, 2, 3, 4, 5, 6, 7
VALUES = ("ransac_height", "refined_mean", "refined_std", "height_t_mean", "refined_pitch")
COPIED = ("ransac_height", "refined_mean", "refined_std", "refined_pitch", "n_inliers")


def no_carry():
    return {"has_prev": 0, "halted": 0, "n_inliers": 0, "y": np.zeros(0), "z": np.zeros(0), "index": np.zeros(0, np.int32),
            **{k: 0.0 for k in VALUES}}


def inlier_yz(v, depth, mask, focus=FOCUS, cy=CY):
    """back_project's Y and Z of the masked features, in feature order (:68, :66)."""
    idx = np.nonzero(mask)[0].astype(np.int32)
    d = np.asarray(depth, dtype=np.float64)[idx]
    return d * (np.asarray(v, dtype=np.float64)[idx] - cy) / focus, d, idx


def tail(chunk, carry, min_points=MIN_POINTS, max_feat=None, focus=FOCUS, cy=CY):
    """chunk: dict of per-frame arrays status, n_selected, n_inliers and VALUES, lists v, depth, mask (one array per frame) and
    prior (F, 4).  carry: dict as `no_carry`.  -> (records: list of dicts, error: (frame, kind) or None, carry-out)."""
    F = len(chunk["status"])
    if carry["halted"]:
        return None, (0, ERR_UPSTREAM), dict(carry)
    max_feat = max([len(x) for x in chunk["v"]] + [0]) if max_feat is None else max_feat
    cur = dict(carry)                                                                # the state after the last frame
    recs, error = [], None
    for f in range(F):
        st, ns, n = int(chunk["status"][f]), int(chunk["n_selected"][f]), len(chunk["v"][f])
        kind = 0
        if st == ST_SINGULAR:
            kind = ERR_SINGULAR
        elif st == ST_MASK:
            kind = ERR_MASK
        elif st == ST_EMPTY:
            kind = ERR_EMPTY
        elif st == ST_RS_FEW and ns >= min_points:
            kind = ERR_NO_MODEL
        elif st == ST_RS_FEW and not cur["has_prev"]:
            kind = ERR_NO_PREVIOUS
        elif st not in (0, ST_RS_FEW) or (st == 0 and not 0 < n <= max_feat):
            kind = ERR_STATUS
        if kind:
            error = (f, kind)
            break
        if st == 0:
            y, z, idx = inlier_yz(chunk["v"][f], chunk["depth"][f], chunk["mask"][f], focus, cy)
            r = {k: float(chunk[k][f]) for k in VALUES}
            r.update(n_inliers=int(chunk["n_inliers"][f]), n_selected=ns, carried=0)
            cur = dict(r, has_prev=1, halted=0, y=y, z=z, index=idx)
        else:
            s, c = chunk["prior"][f][2], chunk["prior"][f][3]
            with np.errstate(all="ignore"):
                h_t = float(np.mean(cur["z"] * s + cur["y"] * c))                   # :202-203 under the new prior
            r = {k: cur[k] for k in COPIED}
            r.update(height_t_mean=h_t, n_selected=ns, carried=1)
            cur = dict(cur, height_t_mean=h_t)
        recs.append(r)
    cur["halted"] = int(error is not None)
    return recs, error, cur


# ---- crafted chunks ---------------------------------------------------------------------------------------------------------
def crafted_frame(rng, n, inliers):
    """A fitted frame of n features whose mask is set at `inliers`; the planes are seeded noise."""
    mask = np.zeros(n, dtype=bool)
    mask[np.asarray(inliers, dtype=np.int64)] = True
    return {"v": rng.uniform(0.0, 376.0, n), "depth": rng.uniform(4.0, 60.0, n), "mask": mask, "status": 0, "n_selected": 3 * n,
            "n_inliers": int(mask.sum()), **{k: float(rng.uniform(0.5, 2.5)) for k in VALUES}}


def carried_frame(rng, n=5, n_selected=9):
    return {"v": rng.uniform(0.0, 376.0, n), "depth": rng.uniform(4.0, 60.0, n), "mask": np.zeros(n, dtype=bool), "status": ST_RS_FEW,
            "n_selected": n_selected, "n_inliers": 0, **{k: float("nan") for k in VALUES}}


def chunk_of(frames, rng):
    """The frames as `tail`'s chunk, with seeded priors (sin and cos of an angle near the script's)."""
    est = rng.uniform(-0.1, 0.1, len(frames))
    prior = np.stack([est * 57.3 - 95, est * 57.3 - 85, np.sin(est), np.cos(est)], 1)
    c = {k: np.array([f[k] for f in frames]) for k in ("status", "n_selected", "n_inliers") + VALUES}
    c.update({k: [f[k] for f in frames] for k in ("v", "depth", "mask")}, prior=prior)
    return c


# inlier counts at which np.add.reduce takes another path: the plain loop, the eight accumulators, their remainder, the first
# split (its half rounded down to a multiple of 8) and deeper recursion
COUNTS = (1, 7, 8, 9, 127, 128, 129, 136, 1000)


def count_chunk(seed=11):
    """Per count a fitted source (n not a multiple of 64, inliers spread over the frame) followed by a carried frame."""
    rng = np.random.default_rng(seed)
    frames = []
    for k in COUNTS:
        n = max(2 * k + 37, 70)
        n += (n % 64 == 0)
        frames += [crafted_frame(rng, n, np.sort(rng.choice(n, k, replace=False))), carried_frame(rng)]
    return chunk_of(frames, rng)


def placement_chunk(seed=12):
    """First inlier at feature 63 and at 64; an all-zero mask word in the middle; two carries in a row; a carried frame first."""
    rng = np.random.default_rng(seed)
    a = crafted_frame(rng, 203, [63, 64, 65, 130, 202])
    b = crafted_frame(rng, 203, [64, 100, 127, 128, 201])
    hole = crafted_frame(rng, 331, list(range(3, 64, 5)) + list(range(128, 331, 3)))     # features 64..127: no inlier
    return chunk_of([carried_frame(rng), a, carried_frame(rng), carried_frame(rng), b, carried_frame(rng), hole, carried_frame(rng)], rng)
