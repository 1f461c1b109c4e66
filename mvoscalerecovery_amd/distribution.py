"""Host side of the feature-distribution analysis (/root/reference/src/scale_calculator.py:428-599).

The device kernel (csrc/mvosr_featdist.hip, mvosr_feature_distribution_batch) leaves, per frame and population, integers and three
floats: the 169-bin histogram of y with the counts on edges 29, 49 and 99, and mean / std / median.  What the reference derives
from them is a few scalar operations each — the narrower histograms, the density, the two skews, the modes — and stays here, in
NumPy, operation for operation as the reference evaluates it.  Nothing here touches the points themselves.
"""
from __future__ import annotations

import numpy as np

N_BINS = 169
HIST_WORDS = 172                                    # MVOSR_FD_HIST_WORDS
EDGES = np.array(range(0, N_BINS + 1)) * 0.1        # :492; the edge arrays of :506, :514, :528 are prefixes of it
CLOSING_SLOT = {29: 169, 49: 170, 99: 171}          # bins of a narrower histogram -> the word that counts y == its closing edge
POPULATIONS = ("all", "correct_distance", "flat")

# status of a frame in a batch result (the kernel's own MVOSR_ST_ERR_MASK, 8, passes through)
DIST_OK = 0                # reached :599 with a selection
DIST_EARLY = 1             # returned at :586: three features or fewer below the vanishing row
DIST_RAISED_TRI1 = 2       # the first triangulation raised (:572)
DIST_RAISED_TRI2 = 3       # the second triangulation raised (:583)
DIST_RAISED_SELECTION = 4  # feature_selection_by_tri raised (:588)
DIST_NO_SELECTION = 5      # reached :599, nothing selected (:590)


def narrow_histogram(words, bins):
    """np.histogram(y, np.array(range(0, bins + 1)) * 0.1) from the kernel's 172 words: the first ``bins`` counts, and the values
    exactly on the closing edge — bin ``bins`` of the wide histogram — in the last one (np.histogram's last bin is closed)."""
    words = np.asarray(words)
    if bins == N_BINS:
        return words[..., :N_BINS].astype(np.int64)
    if bins not in CLOSING_SLOT:
        raise ValueError("bins must be one of 29, 49, 99, 169")
    h = words[..., :bins].astype(np.int64)
    h[..., -1] += words[..., CLOSING_SLOT[bins]]
    return h


def density_of(counts, bins):
    """np.histogram(..., density=True): counts / np.diff(edges) / counts.sum()."""
    counts = np.asarray(counts)
    with np.errstate(all="ignore"):
        return counts / np.array(np.diff(EDGES[:bins + 1]), float) / counts.sum()


def p1_mode(words):
    """check_skewness's own mode (:492-495): single counts zeroed, the mean of the upper edges of the bins that hold the maximum."""
    dis = narrow_histogram(words, N_BINS)
    dis[dis == 1] = 0
    return np.mean(EDGES[1:][dis == np.max(dis)])


def skews(mean, std, median, mode):
    """(p1, p2) of :489 and :496."""
    with np.errstate(all="ignore"):
        return (mean - mode) / std, 3 * (mean - median) / std


def check_mode(dis_data, bins, verbose=False):
    """scale_calculator.py:446-483: the runs of flagged bins, as lists of their upper edges ([[array]] for a single flagged bin,
    as the reference builds it)."""
    d = np.array(dis_data)
    top = np.max(d)
    if top <= 2:
        return []
    flagged = np.zeros(d.shape[0], dtype=bool)
    flagged[0] = d[0] == top
    flagged[-1] = d[-1] == top
    inner = d[1:-1]
    flagged[1:-1] = (inner >= d[0:-2]) & (inner >= d[2:]) & (inner >= 0.33 * top) & (inner >= 2)
    uppers = bins[1:][flagged]
    if verbose:
        print(uppers)
    if np.sum(flagged) == 1:
        return [[uppers]]
    runs, run = [], []
    for upper in uppers:
        if run and not (upper - run[-1] < 0.11):
            runs.append(run)
            run = []
        run.append(upper)
    if run:
        runs.append(run)
    return runs


def check_reverse_mode(dis_data):
    """scale_calculator.py:428-443: the bins that are local minima (a bin level with both neighbours is none)."""
    d = np.array(dis_data)
    low = np.min(d)
    flag = np.zeros(d.shape[0], dtype=bool)
    flag[0] = d[0] == low
    flag[-1] = d[-1] == low
    inner = d[1:-1]
    flag[1:-1] = (inner <= d[0:-2]) & (inner <= d[2:]) & ~((inner == d[2:]) & (inner == d[0:-2]))
    return flag


def check_distance(feature3d, focus, verbose=False):
    """scale_calculator.py:49-54: features for which f |X| or f |Y| exceeds z (z + 1)."""
    zz = feature3d[:, 2] * (feature3d[:, 2] + 1)
    flag = ((zz - np.abs(focus * feature3d[:, 0])) < 0) | ((zz - np.abs(focus * feature3d[:, 1])) < 0)
    if verbose:
        print(np.sum(flag), flag.shape)
    return flag


class FeatureDistribution:
    """What ``check_full_distribution_batch`` returns: per frame and population (0 every feature below the vanishing row, 1 kept by
    the vote, 2 selected as road) ``n``, ``hist`` (169 bins of y), ``mean`` / ``std`` / ``median`` / ``skew_p1`` / ``skew_p2``; per
    frame ``height_level``, ``status`` (DIST_*) and, where the per-frame call would raise, the exception in ``errors``."""

    def __init__(self, n, words, words_scaled, stats, height_level, status, errors):
        self.n = np.asarray(n, dtype=np.int32)
        self.words = np.asarray(words, dtype=np.int32)
        self.words_scaled = np.asarray(words_scaled, dtype=np.int32)
        self.hist = self.words[..., :N_BINS]
        self.mean, self.std, self.median = stats[..., 0], stats[..., 1], stats[..., 2]
        self.height_level = np.asarray(height_level, dtype=np.float64)
        self.status = np.asarray(status, dtype=np.int32)
        self.errors = dict(errors)
        self.skew_p1 = np.full(self.n.shape, np.nan)
        for f, p in zip(*np.nonzero(self.n > 0)):
            self.skew_p1[f, p] = skews(self.mean[f, p], self.std[f, p], self.median[f, p], p1_mode(self.words[f, p]))[0]
        self.skew_p2 = skews(self.mean, self.std, self.median, 0.0)[1]

    def __len__(self):
        return len(self.status)

    def histogram(self, frame, population, bins=49, density=False, scaled=False):
        """np.histogram of the population's y (``scaled``: y * scale) over ``np.array(range(0, bins + 1)) * 0.1``."""
        h = narrow_histogram((self.words_scaled if scaled else self.words)[frame, population], bins)
        return density_of(h, bins) if density else h

    def modes(self, frame):
        """``mode_analysis`` of that frame (:505-507): check_mode over the density of the selected features' 99-bin histogram."""
        return check_mode(self.histogram(frame, 2, 99, density=True), EDGES[:100])
