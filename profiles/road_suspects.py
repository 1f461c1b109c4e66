#!/usr/bin/env python3
"""How much work remove_single's suspects are for the road-model kernel, counted on the CPU with the oracle:

    python profiles/road_suspects.py [--frames 1024] [--workload c2|kitti] [--features 2000] [--quiet]

The lists are the bench's: frame i of the pool is synth.synth_frame(i, n, base_seed=2024), its list the y' of the flat
selection (oracle frame_raw_scale, flat_feature[:, 1]) in list order; value j belongs to lane j mod 64 of the frame's
wavefront.  Per list it prints
    the length, the single bins (count 1), the SUSPECTS (values whose own bin or a neighbour of it is single) and the
    largest number of them in one lane (the trips of the wavefront's suspects loop), the values that sit IN a single bin
    and their largest number in one lane, and the suspects that fail the interior test (closer than kSingleMargin to an
    edge of their bin: the ones that still take the three-interval test);
then the averages, and how many lists kept all values but one per single bin.  Needs no GPU."""
import argparse
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from mvoscalerecovery_amd import synth            # noqa: E402
from oracle import scale_oracle as so             # noqa: E402

MARGIN = 2.0 ** -40                                # kSingleMargin (csrc/mvosr_kernels.hip)
N_BINS = 169


def count(y):
    e = so.BIN_EDGES
    hist = so.histogram_170(y)
    single = hist == 1
    near = single.copy()
    near[1:] |= single[:-1]
    near[:-1] |= single[1:]
    inr = (y >= 0.0) & (y <= e[N_BINS])
    b = np.clip(np.searchsorted(e, y, side="right") - 1, 0, N_BINS - 1)      # np.histogram's bin (the last one closed)
    sus = inr & near[b]
    own = inr & single[b]
    lane = np.arange(len(y)) % 64
    interior = (y - e[b] > MARGIN) & (e[b + 1] - y > MARGIN)
    dropped = int(so.single_bin_drop_mask(y, hist).sum())
    return dict(n=len(y), single=int(single.sum()), sus=int(sus.sum()), sus_lane=int(np.bincount(lane[sus], minlength=64).max()),
                own=int(own.sum()), own_lane=int(np.bincount(lane[own], minlength=64).max()), edge=int((sus & ~interior).sum()),
                dropped=dropped)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024, help="frames of the pool")
    ap.add_argument("--workload", choices=("c2", "kitti"), default="c2")
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--quiet", action="store_true", help="the summary only")
    args = ap.parse_args()
    if args.workload == "kitti":
        sizes = [int(v) for v in np.random.default_rng(4541).integers(300, 1501, args.frames)]       # bench.py frame_sizes
    else:
        sizes = [args.features] * args.frames
    rows = []
    if not args.quiet:
        print("frame  length single suspects /lane  in-single /lane  at-edge dropped")
    for i, n in enumerate(sizes):
        f3, f2 = synth.synth_frame(i, n, base_seed=2024)
        res = so.frame_raw_scale(f3, f2, 1.75)
        if res.flat_feature is None or len(res.flat_feature) == 0:
            continue
        c = count(np.ascontiguousarray(res.flat_feature[:, 1], dtype=np.float64))
        rows.append(c)
        if not args.quiet:
            print("%5d %7d %6d %8d %5d %10d %5d %8d %7d" % (i, c["n"], c["single"], c["sus"], c["sus_lane"], c["own"], c["own_lane"], c["edge"], c["dropped"]))
    k = len(rows)
    avg = {key: sum(r[key] for r in rows) / k for key in rows[0]}
    print("%d lists (%s): length %.0f  single bins %.2f  suspects %.1f (largest per lane %.2f)  in a single bin %.2f (per lane %.2f)"
          % (k, args.workload, avg["n"], avg["single"], avg["sus"], avg["sus_lane"], avg["own"], avg["own_lane"]))
    print("suspects that fail the interior test: %d of %d in all lists; lists with 8 or more trips: %d; lists whose dropped values are "
          "exactly their single bins' lone ones: %d of %d"
          % (sum(r["edge"] for r in rows), sum(r["sus"] for r in rows), sum(r["sus_lane"] >= 8 for r in rows),
             sum(r["dropped"] == r["single"] for r in rows), k))


if __name__ == "__main__":
    main()
