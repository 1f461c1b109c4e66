"""Crafted sequences and references for the sequence tail — window_median_kernel in its contiguous and its blocked form
(csrc/mvosr_kernels.hip) and slew_kernel (csrc/mvosr_rescale.hip) — shared by tests/test_seqtail_cases.py (CPU: the references
against one another, mvosr_slew_median_host, and what a wrong kernel would give) and tests/test_gpu_seqtail.py (the C entry
points on the device).  Test infrastructure.

References: the reference's own operations in Python floats — a `deque` with `np.median` under np.errstate(all="ignore")
(rescale.py:175-178, scale_calculator.py:396-400) and the if / elif / else recurrence of rescale.py:169-177 — and the median
restated independently as a sort, then the middle element or (a + b) / 2.  Both operations are DEFINED in double precision (a
median picks elements, the mean of two is one rounded addition and an exact halving, the recurrence is a chain of rounded
additions), so there is nothing to compute at a higher precision and no tolerance: every comparison is equality, doubles byte
for byte with NaN at the same positions (`same`).  The one case that holds zeros is compared by value (`same_values`): the
mean of +0 and -0 and the order of the two under a sort are the only places where equal values have two encodings.
"""
import ctypes as C
from collections import deque

import numpy as np

SLEW = 0.3                                            # rescale.py:169-172
WINDOWS = (1, 2, 3, 4, 5, 63, 64)
LENGTHS = (1, 255, 256, 257, 513)                     # window_median_kernel runs 256 threads per block
SLEW_LENGTHS = (1, 63, 64, 65, 127, 128, 129)         # slew_kernel walks 64 frames per trip
N_BLOCKS = (2, 3, 7, 8, 64)
ERR_ARG = -2                                          # MVOSR_ERR_ARG


# ---- comparisons --------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Equal byte for byte, NaN at the same positions (a NaN's payload is not part of any definition here)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def same_values(a, b):
    """Equal by value (+0 == -0), NaN at the same positions: the signed-zero case only."""
    return bool(np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True))


# ---- references ---------------------------------------------------------------------------------------------------------------
def median_deque(seq, window, queue=()):
    """The reference's own operations: append, popleft beyond `window`, np.median of the deque."""
    q = deque(float(x) for x in queue)
    out = np.empty(len(seq), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i, s in enumerate(seq):
            q.append(float(s))
            if len(q) > window:
                q.popleft()
            out[i] = np.median(q)
    return out


def median_sorted(seq, window, queue=()):
    """The same, restated: output i is over the last `window` elements of queue + seq[:i + 1], sorted — NaN if one of them is
    NaN, else the middle element or the two middle elements' (a + b) / 2."""
    full = [float(x) for x in queue] + [float(x) for x in seq]
    nq = len(full) - len(seq)
    out = np.empty(len(seq), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(len(seq)):
            w = full[max(0, nq + i + 1 - window):nq + i + 1]
            if any(x != x for x in w):
                out[i] = np.nan
                continue
            w = sorted(w)
            m = len(w)
            out[i] = w[m // 2] if m % 2 else (w[m // 2 - 1] + w[m // 2]) / 2.0
    return out


def slew_recurrence(raw, apply, slew, scale_in, at_limit_moves=False):
    """rescale.py:169-177 in Python floats: the values pushed.  at_limit_moves: the WRONG recurrence with >= / <= (a difference
    exactly at the limit takes the step instead of the value) — what the exact-limit cases must tell apart."""
    s = float(scale_in)
    out = np.empty(len(raw), dtype=np.float64)
    for i in range(len(raw)):
        if apply[i] != 0:                              # rescale.py:152 — only a frame with a RANSAC plane moves the scale
            r = float(raw[i])
            d = r - s
            if (d >= slew) if at_limit_moves else (d > slew):
                s += slew
            elif (d <= -slew) if at_limit_moves else (d < -slew):
                s -= slew
            else:
                s = r
        out[i] = s
    return out


# ---- the blocked layout -------------------------------------------------------------------------------------------------------
def build_blocks(seq, n_blocks, stride=None, pad=np.nan):
    """The gathered buffer of `seq` over `n_blocks` ranks: block r, sharding.shard_sizes' share, starts at r * stride; the rest
    is `pad`.  stride None: the longest block.  -> (buffer, sizes, stride)"""
    from mvoscalerecovery_amd import sharding
    sizes = sharding.shard_sizes(len(seq), n_blocks)
    stride = max(max(sizes), 1) if stride is None else int(stride)
    buf = np.full(n_blocks * stride, pad, dtype=np.float64)
    at = 0
    for r, m in enumerate(sizes):
        buf[r * stride:r * stride + m] = seq[at:at + m]
        at += m
    return buf, sizes, stride


def concat_blocks(buf, sizes, stride):
    return np.concatenate([buf[r * stride:r * stride + m] for r, m in enumerate(sizes)]) if len(sizes) else np.zeros(0)


def concat_blocks_reading_padding(buf, sizes, stride):
    """WRONG on purpose: every block read as long as the longest one — one element of padding after a shorter block."""
    longest = max(sizes)
    return np.concatenate([buf[r * stride:r * stride + min(longest, stride)] for r in range(len(sizes))])


def seq_at(buf, n, n_blocks, stride, i, head_len_is_base=False):
    """median_seq_at of mvosr_kernels.hip restated: element i of the sequence in the gathered buffer.  head_len_is_base: the
    WRONG index that gives the first n % n_blocks blocks n / n_blocks elements as well."""
    base, extra = divmod(n, n_blocks)
    hl = base if head_len_is_base else base + 1
    head = extra * hl
    if i < head:
        r, j = divmod(i, hl)
    else:
        k = i - head
        r = extra + k // base
        j = k - (r - extra) * base
    return buf[r * stride + j]


# ---- window-median cases ------------------------------------------------------------------------------------------------------
def _seq(kind, n, window, rng):
    """n values without a zero (`zeros` apart)."""
    i = np.arange(n, dtype=np.float64)
    if kind == "equal":
        return np.full(n, 1.75)
    if kind == "alternating":
        return np.where(np.arange(n) % 2 == 0, 1.25, 2.5)
    if kind == "ascending":
        return 1.0 + i * 2.0 ** -20
    if kind == "descending":
        return 3.0 - i * 2.0 ** -20
    if kind == "inf_middles":
        # a full even window over the alternation holds as many -inf as +inf: they are its two middle elements, their mean is
        # NaN (NumPy's too); an odd window's median is one of the two
        s = np.where(np.arange(n) % 2 == 0, np.inf, -np.inf)
        s[2 * n // 3:] = rng.uniform(0.5, 3.0, n - 2 * n // 3)
        return s
    if kind == "overflow":
        # the two middle values' sum is beyond the largest double: (a + b) / 2 is inf, not their mean — NumPy's np.mean as well
        s = np.where(np.arange(n) % 2 == 0, 1.5e308, 1.7e308)
        s[n // 2:] = -s[n // 2:]
        return s
    if kind == "denormal":
        return rng.integers(1, 1000, n).astype(np.float64) * 5e-324     # (positive: an odd sum's half rounds to even, never to zero)
    if kind == "one_nan":
        s = rng.uniform(0.5, 3.0, n)
        s[n // 2] = np.nan
        return s
    if kind == "random":
        return rng.uniform(0.5, 3.0, n)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0]), n)
    raise ValueError(kind)


SEQ_KINDS = ("equal", "alternating", "ascending", "descending", "inf_middles", "overflow", "denormal", "one_nan", "random")


def _queue_lengths(window):
    return sorted({0, 1, window - 1, window})            # (the full queue loses its oldest element at the first push)


def median_cases():
    """Contiguous cases: every window with every kind of sequence (the queue length going round), every window with every
    queue length and every n (the kind going round), a NaN in the carried-in queue, and the signed zeros."""
    rng = np.random.default_rng(20)
    cases = []

    def add(kind, n, window, nq, nan_in_queue=False):
        seq = _seq(kind, n, window, rng)
        q = rng.uniform(0.5, 3.0, nq) if kind != "zeros" else rng.choice(np.array([0.0, -0.0, 2.0]), nq)
        if kind == "denormal":
            q = rng.integers(1, 1000, nq).astype(np.float64) * 5e-324
        if nan_in_queue:
            q[nq // 2] = np.nan
        cases.append({"name": "%s-n%d-w%d-q%d%s" % (kind, n, window, nq, "-nanq" if nan_in_queue else ""), "kind": kind, "seq": seq,
                      "window": window, "queue": q, "by_value": kind == "zeros", "nan_in_queue": nan_in_queue})

    k = 0
    for w in WINDOWS:
        for kind in SEQ_KINDS:
            ql = _queue_lengths(w)
            add(kind, 257, w, ql[k % len(ql)])
            k += 1
    for w in WINDOWS:
        for nq in _queue_lengths(w):
            for n in LENGTHS:
                add(SEQ_KINDS[k % len(SEQ_KINDS)], n, w, nq)
                k += 1
    for w in WINDOWS:
        for nq in _queue_lengths(w):
            if nq:
                add("random", 70, w, nq, nan_in_queue=True)
    for w in WINDOWS:
        add("zeros", 257, w, min(w, 3))
    return cases


def blocked_cases():
    """Blocked cases: n_blocks x (n % n_blocks of 0, 1, n_blocks - 1; n < n_blocks: base_len 0 and empty trailing blocks;
    n == n_blocks) x (stride = longest block; longer, padded with NaN; longer, padded with 1e300), windows 5 and 64 — blocks of
    five or six elements, so that a window of 64 spans thirteen blocks — with and without a carried-in queue.  Distinct values:
    any wrong index shows."""
    rng = np.random.default_rng(21)
    cases, k = [], 0
    for nb in N_BLOCKS:
        for n in sorted({5 * nb, 5 * nb + 1, 5 * nb + nb - 1, nb - 1, nb}):
            for window in (5, 64):
                for extra_stride, pad in ((0, np.nan), (3, np.nan), (1, 1e300)):
                    seq = 1.0 + rng.permutation(n).astype(np.float64) * 2.0 ** -10
                    q = rng.uniform(1.0, 1.4, (0, 3, window)[k % 3])
                    k += 1
                    sizes_max = -(-n // nb)
                    buf, sizes, stride = build_blocks(seq, nb, max(sizes_max, 1) + extra_stride, pad)
                    cases.append({"name": "nb%d-n%d-w%d-s+%d-%s-q%d" % (nb, n, window, extra_stride, "nan" if pad != pad else "1e300", len(q)),
                                  "seq": seq, "window": window, "queue": q, "n_blocks": nb, "buf": buf, "sizes": sizes, "stride": stride,
                                  "padded": extra_stride > 0, "extra": n % nb, "base_len": n // nb})
    return cases


# ---- slew cases ---------------------------------------------------------------------------------------------------------------
def exact_limit_pairs(slew=SLEW, want=6):
    """Pairs (s, raw) with fl(raw - s) == slew exactly and fl(s + slew) != raw: the reference's `>` takes raw, a `>=` would take
    s + slew, and the two differ.  Such a pair needs the sum rounded on a finer grid than the difference (both round the same
    exact quantity): raw just below 0.25 (ulp 2^-55) while raw - s is in [0.25, 0.5) (ulp 2^-54), s ~ -0.05 (ulp 2^-57).  A
    deterministic walk over s in steps of its ulp, raw among the neighbours of fl(s + slew)."""
    pairs = []
    for k in range(1, 1 << 14):
        s = -0.05 - k * 2.0 ** -57
        up = s + slew
        for raw in (float(np.nextafter(up, np.inf)), float(np.nextafter(up, -np.inf))):
            if raw - s == slew and s + slew != raw:
                pairs.append((s, raw))
        if len(pairs) >= want:
            break
    return pairs[:want]


EXACT_UP = exact_limit_pairs()
EXACT_DOWN = [(-s, -raw) for s, raw in EXACT_UP]        # the mirror: fl(raw - s) == -slew, fl(s - slew) != raw
assert len(EXACT_UP) >= 4, "no exact-limit pairs found"
assert all(r - s == SLEW and s + SLEW != r for s, r in EXACT_UP) and all(r - s == -SLEW and s - SLEW != r for s, r in EXACT_DOWN)


def _exact_limit_sequence():
    """Every pair met with the running scale exactly s: a frame within the limit sets the scale to its own value (0.1 on the way,
    then s), the next frame is the pair's raw.  The first pair sits on frame 0 (scale_in = s), the padding puts others on lanes 63
    and 64."""
    raw, at = [], []
    pairs = [p for ud in zip(EXACT_UP, EXACT_DOWN) for p in ud]
    scale_in = pairs[0][0]
    for j, (s, r) in enumerate(pairs):
        if j:
            raw += [0.1 if s < 0 else -0.1, s]
            while j in (3, 4) and len(raw) % 64 != (63 if j == 3 else 0):
                raw.insert(len(raw) - 1, s)               # (within the limit of 0.1: the scale is s from here on)
        at.append(len(raw))
        raw.append(r)
    raw = np.array(raw)
    return raw, np.ones(len(raw), np.int32), scale_in, at


def slew_cases():
    rng = np.random.default_rng(22)
    cases = []

    def add(name, raw, apply, scale_in=1.5, window=5, queue=(1.25, 1.5), **kw):
        c = {"name": name, "raw": np.ascontiguousarray(raw, dtype=np.float64), "apply": np.ascontiguousarray(apply, dtype=np.int32),
             "scale_in": float(scale_in), "window": int(window), "queue": np.array(queue, dtype=np.float64), "slew": SLEW}
        c.update(kw)
        assert len(c["raw"]) == len(c["apply"])
        cases.append(c)

    def mixed(n):
        raw = rng.uniform(0.5, 3.5, n)
        raw[rng.random(n) < 0.15] += 5.0
        raw[rng.random(n) < 0.15] -= 5.0
        return raw

    for n in SLEW_LENGTHS:
        add("mixed-n%d" % n, mixed(n), (rng.random(n) > 0.2).astype(np.int32), queue=rng.uniform(1.0, 2.0, n % 3))
    # a thousand steps up, a thousand down: the additions round one after another (not scale_in + k * slew)
    add("ramp", np.concatenate([np.full(1000, 1e6), np.full(1000, -1e6)]), np.ones(2000, np.int32), ramp=True)
    raw, apply, s_in, at = _exact_limit_sequence()
    add("exact_limit", raw, apply, scale_in=s_in, exact_at=at)
    # apply patterns
    raw, apply = mixed(129), (rng.random(129) > 0.3).astype(np.int32)
    raw[apply == 0] = np.nan
    add("nan_not_applied", raw, apply, no_nan_pushed=True)
    raw, apply = mixed(129), np.ones(129, np.int32)
    for i in (0, 40, 63, 64, 100):
        raw[i] = np.nan
    add("nan_applied", raw, apply)                        # (the recurrence defines what follows: both comparisons fail, the scale IS the NaN, the next finite frame replaces it)
    raw, apply = mixed(192), np.ones(192, np.int32)
    apply[64:128] = 0
    add("block_of_zeros", raw, apply)
    for name, lanes in (("lane0_only", (0, 64, 128)), ("lane63_only", (63, 127, 191))):
        apply = np.zeros(192, np.int32)
        apply[list(lanes)] = 1
        add(name, mixed(192), apply)
    add("apply_2_and_minus1", mixed(129), rng.choice(np.array([0, 2, -1], np.int32), 129))
    add("scale_in_nan", mixed(65), np.ones(65, np.int32), scale_in=np.nan)
    add("scale_in_nan_not_applied", mixed(65), np.zeros(65, np.int32), scale_in=np.nan)
    raw = mixed(129)
    raw[[3, 64, 70]], raw[[10, 63, 90]] = np.inf, -np.inf
    add("inf_raw", raw, np.ones(129, np.int32))
    add("queue_empty", mixed(65), np.ones(65, np.int32), queue=())
    add("queue_full", mixed(65), np.ones(65, np.int32), queue=(1.0, 1.5, 1.25, 1.75, 1.4))
    add("window_64", mixed(129), np.ones(129, np.int32), window=64, queue=rng.uniform(1.0, 2.0, 63))
    return cases


def slew_reference(c, at_limit_moves=False):
    """(pushed, filtered) of a slew case: the recurrence, then the deque's medians."""
    pushed = slew_recurrence(c["raw"], c["apply"], c["slew"], c["scale_in"], at_limit_moves)
    return pushed, median_deque(pushed, c["window"], c["queue"])


# ---- launchers ----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A
_SENT64 = np.frombuffer(bytes([SENTINEL] * 8), dtype=np.float64)[0]


def _addr(q):
    from mvoscalerecovery_amd import _lib
    return _lib.addr(q) if q.size else None


def run_median(ctx, seq, window, queue=(), blocks=None):
    """mvosr_window_median (blocks None) or mvosr_window_median_blocked (blocks = (buffer, n_blocks, stride)) -> (rc, the n
    outputs, guard_intact).  The output buffer holds one element more than n and is pre-filled with SENTINEL bytes."""
    n = len(seq)
    q = np.ascontiguousarray(np.asarray(queue, dtype=np.float64))
    data = np.ascontiguousarray(seq if blocks is None else blocks[0], dtype=np.float64)
    src = ctx.to_device(data) if data.size else ctx.empty(1, np.float64)
    out = ctx.empty(n + 1, np.float64).fill(SENTINEL)
    if blocks is None:
        rc = ctx.lib.mvosr_window_median(ctx.handle, src.ptr, n, int(window), _addr(q), int(q.size), out.ptr)
    else:
        rc = ctx.lib.mvosr_window_median_blocked(ctx.handle, src.ptr, n, int(blocks[1]), int(blocks[2]), int(window), _addr(q), int(q.size), out.ptr)
    ctx.sync()
    got = out.download()
    src.free()
    out.free()
    return int(rc), got[:n], bool(got[n:].view(np.uint64)[0] == _SENT64.view(np.uint64))


def all_sentinel(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == SENTINEL))


def run_slew(ctx, c):
    """mvosr_slew_median on a slew case -> (pushed, filtered, guards_intact)."""
    from mvoscalerecovery_amd import _lib
    n = len(c["raw"])
    io = [ctx.to_device(c["raw"]), ctx.to_device(c["apply"]), ctx.empty(n + 1, np.float64).fill(SENTINEL), ctx.empty(n + 1, np.float64).fill(SENTINEL)]
    q = c["queue"]
    _lib.check(ctx.lib.mvosr_slew_median(ctx.handle, io[0].ptr, io[1].ptr, n, C.c_double(c["slew"]), C.c_double(c["scale_in"]), c["window"],
                                         _addr(q), int(q.size), io[2].ptr, io[3].ptr), "mvosr_slew_median")
    ctx.sync()
    p, f = io[2].download(), io[3].download()
    for b in io:
        b.free()
    return p[:n], f[:n], all_sentinel(p[n:]) and all_sentinel(f[n:])


def run_slew_host(c):
    """mvosr_slew_median_host (no GPU) on a slew case -> (pushed, filtered, scale_out)."""
    from mvoscalerecovery_amd import _lib
    lib = _lib.load()
    n = len(c["raw"])
    p, f, s_out, q = np.empty(n), np.empty(n), np.zeros(1), c["queue"]
    _lib.check(lib.mvosr_slew_median_host(_lib.addr(c["raw"]), _lib.addr(c["apply"]), n, C.c_double(c["slew"]), C.c_double(c["scale_in"]),
                                          c["window"], _addr(q), int(q.size), _lib.addr(p), _lib.addr(f), _lib.addr(s_out)),
               "mvosr_slew_median_host")
    return p, f, float(s_out[0])
