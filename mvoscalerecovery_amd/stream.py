"""The streamed-chunk path both estimators share (scale_calculator.ScaleEstimator, rescale.ScaleEstimator): a batch goes through the
device in chunks, each packed, uploaded and launched while the chunks before it run, and collected a few chunks later.

``plan`` cuts a call into chunks (``fixed_plan``: into equal ones), ``run`` keeps them in flight, and ``Rerun`` records carry the frames a chunk's device triangulation
declined through the host's triangulations while later chunks run (``advance``), to be finished after the call's last chunk
(``finish_all``).  What differs between the estimators comes in as values and callables."""
import contextlib
import os
import time

import numpy as np

# Shared-memory slots of the Delaunay worker pool (packing.delaunay_submit).  A submission's points and rows live in its slot's
# segments until its handle is ready: submissions in flight at the same time must use distinct slots.
CHUNK_SLOTS = 4
SLOT_CHUNK = 0              # host-path chunk k: first triangulations in SLOT_CHUNK + k % CHUNK_SLOTS (0-3) ...
SLOT_CHUNK_TRI2 = 4         # ... second triangulations in SLOT_CHUNK_TRI2 + k % CHUNK_SLOTS (4-7)
SLOT_DEFER = 8              # re-run record i of a call (i < GPU_REDO_MAX_DEFERRED <= 8): first triangulations in SLOT_DEFER + i (8-15) ...
SLOT_DEFER_TRI2 = 16        # ... second triangulations in SLOT_DEFER_TRI2 + i (16-23)
SLOT_EARLY = 24             # the call's last chunk: the frames its first triangulation declined, found early (24) ...
SLOT_EARLY_TRI2 = 25        # ... their second triangulations (25)


class StreamKnobs:
    """The streamed path's knobs, shared by both estimators (class attributes: tests and profiles override them per instance)."""
    GPU_CHUNK = 8192            # frames per chunk, at most (a call of F frames uses chunks of F/4, GPU_MIN_CHUNK at least: the pipeline needs a few)
    GPU_MIN_CHUNK = 512         # ... and at least (tests lower it to put chunk boundaries everywhere)
    GPU_RESIDENT = 512          # frames the GPU works on at once (two 8-wavefront workgroups per CU): chunks are multiples of it
    GPU_CHUNK_POINTS = 10000000 # ... and features per chunk (40 B each in staging memory, ~180 B each on the device)
    GPU_RAMP = True             # short first chunks (see chunk_size)
    GPU_RAMP_FRACTIONS = (1 / 6, 1 / 3, 1 / 2, 2 / 3, 5 / 6)   # their sizes, as fractions of a full chunk: with 2000-feature frames one, two,
                                # three, four and five whole rounds of the triangulation kernel's resident frames (768) before the
                                # six-round chunks.  (The shape barely matters any more — every ramp tried gave 520-530 k
                                # frames/s —: the pipeline's stages are balanced, PCIe at 6.5 ms per chunk against the GPU's 7.2.)
    GPU_PIPELINE = 2            # chunks queued on the device behind the one being collected (with the short first chunks 1 -> 2 is +3 % at 32 768 frames, +6 % at 16 384; 3: the same)
    GPU_SIDE_DOWNLOADS = os.environ.get("MVOSR_SIDE_DOWNLOADS", "1") != "0"   # a chunk's results reach page-locked memory through a copy KERNEL — not through a
                                # hipMemcpyAsync parked on a copy engine behind the chunk's kernels (False / MVOSR_SIDE_DOWNLOADS=0: as before round 6's second half; LABNOTES 10.14)
    GPU_REDO_EARLY = True       # a deferred re-run's steps are taken while later chunks run (advance) ...
    GPU_REDO_EARLY_MAX = 16     # ... for chunks with at most so many frames to redo (more: the one merged re-run at the call's end)
    GPU_REDO_MAX_DEFERRED = 8   # re-run records a call holds at most (each keeps device blocks and a pair of pool slots)

    def _resident_frames(self, max_pts):
        """Frames the triangulation kernel works on at a time (mvosr_delaunay_frames_per_cu x CUs)."""
        ctx = self.engine.ctx
        return max(self.GPU_RESIDENT, int(ctx.lib.mvosr_delaunay_frames_per_cu(int(max_pts))) * int(ctx.n_cu))

    def _redo_context(self):
        """A context of its own (stream, workspace, caches) for the re-runs that advance while later chunks run: on the estimator's
        stream their few launches would sit BEHIND the chunks already queued — two chunks, 8 ms each — at every step."""
        if getattr(self, "_redo_ctx", None) is None:
            from . import _lib
            self._redo_ctx = _lib.Context(self.engine.ctx.device)
        return self._redo_ctx


def chunk_size(F, chunk, min_chunk, points, head_sizes, fractions=(), full=None):
    """(frames per chunk, sizes of the short first chunks) for a call of ``F`` frames.  A chunk is ``min(chunk, max(min_chunk,
    ceil(F / 4)))`` frames — ``full`` when given —: larger chunks leave fewer launch tails, but a call that is ONE chunk packs,
    uploads and computes one after the other.  Then the points cap as it will bite (``points`` over the mean of ``head_sizes``,
    the first frames' sizes): the short first chunks are fractions of THAT chunk.  The first chunks are short (``fractions`` of a
    chunk) for a call of three chunks of 2048 frames or more: the GPU starts after the pack + upload of a sixth of a chunk instead
    of a whole one, and the host, which prepares a frame in less time than the GPU spends on it, is ahead from then on."""
    C = min(chunk, max(min_chunk, -(-F // 4))) if full is None else full
    C = int(max(min_chunk, min(C, points // max(1, sum(head_sizes) // max(1, len(head_sizes))))))
    ramp = [int(C * x) for x in fractions] if C >= 2048 and F >= 3 * C else []
    return C, ramp


def plan(F, tables_of, C, ramp, points, resident, stop=None):
    """Yields ``(a, b, tables)`` for each chunk of frames ``a:b`` of a call of ``F``.  A chunk's sizes are looked at when its turn
    comes (one pass over a whole call's frames before the first chunk was 5 ms at 32 768 frames, with an idle GPU): ``tables_of(a, b)``
    returns the packer's tables of those frames (or None) and their sizes.  A chunk is ``ramp[k]`` frames (``C`` past the ramp),
    cut to ``points`` features, halved while frames x largest frame is above twice that (the triangulation's workspace: one
    20 000-point frame among thousands of small ones must not turn into a 20 GB request) and rounded down to whole rounds of
    ``resident(largest frame)`` frames, except for the call's last chunk.  ``stop(a, sizes)``: a frame index at which the call ends
    (before a frame the device path does not take), or None."""
    a, k = 0, 0
    while a < F:
        b = min(F, a + (ramp[k] if k < len(ramp) else C))
        tb, lens = tables_of(a, b)
        if stop is not None and (end := stop(a, lens)) is not None:
            F, stop = end, None
            if a >= F:
                return
            b, lens = min(b, F), lens[:F - a]
        b = min(b, a + max(int(np.searchsorted(np.cumsum(lens), points, side="right")), 1))
        while b - a > 1 and (b - a) * int(lens[:b - a].max()) > 2 * points:
            b = a + max(1, (b - a) // 2)
        # (whole rounds of resident frames: the triangulation kernels then have no partly filled last round — 32 768 frames of
        # 2000 features in chunks of 5000: 349-388 k frames/s, of 4096: 379-408 k)
        res = resident(int(lens[:b - a].max()))
        if b < F and b - a >= 2 * res:
            b = a + ((b - a) // res) * res
        yield a, b, (tuple(t[:b - a] for t in tb) if tb is not None else None)
        a, k = b, k + 1


def fixed_plan(F, step):
    """``plan`` without a look at the frames: chunks of ``step`` frames, no packer's tables."""
    for a in range(0, F, step):
        yield a, min(F, a + step), None


def tables_of(feature3ds, feature2ds, **kw):
    """``tables_of`` for ``plan``: the C packer's pointer tables (engine.frame_tables; ``kw`` goes to it) and the frames' sizes from
    them — one C loop over the lists, where a Python loop was 7 ms per 32 768 frames — or from the lists where they do not pack in place."""
    from .engine import frame_tables

    def of(a, b):
        tb = frame_tables(feature3ds[a:b], feature2ds[a:b], **kw)
        if tb is not None:
            return tb, tb[2].astype(np.int64)
        return None, np.fromiter((len(x) for x in feature3ds[a:b]), dtype=np.int64, count=b - a)
    return of


def run(plan, start, collect, depth, free, records, finish):
    """The chunks of ``plan`` through the device: ``start(a, b, tables, k)`` packs, uploads and launches chunk ``k`` and returns its
    state; ``depth`` chunks stay queued behind the one whose results ``collect(state, a, b, last)`` waits for — this process packs
    and uploads the next chunk meanwhile.  ``finish()`` after the last collection (the call's deferred re-runs).  Returns the
    chunks' bounds, states and results.  When anything raises, every chunk state is ``free``-d and every record of ``records``
    released before the exception leaves: no device block of the call stays alive and no pool job still writes into its slot."""
    bounds, states, results, queue = [], [], [], []
    try:
        for k, (a, b, tables) in enumerate(plan):
            bounds.append((a, b))
            queue.append((start(a, b, tables, k), a, b))
            while len(queue) > depth:
                st, pa, pb = queue.pop(0)
                states.append(st)
                results.append(collect(st, pa, pb, False))
        while queue:
            st, pa, pb = queue.pop(0)
            states.append(st)
            results.append(collect(st, pa, pb, not queue))
        finish()
    except BaseException:
        for st in states + [q[0] for q in queue]:
            free(st)
        for r in records:
            r.free()
        del records[:]
        raise
    return bounds, states, results


def concat(bounds, results, fields, errors):
    """The chunks' results as one call's: each of ``fields`` concatenated, and the host errors (``errors``) keyed by frame of the call."""
    return ([np.concatenate([r[f] for r in results]) for f in fields],
            {a + f: e for (a, _), r in zip(bounds, results) for f, e in r[errors].items()})


def scatter(res, frames, sub, fields, errors, first=0):
    """A re-run's results ``sub[first:first + len(frames)]`` into a chunk's results ``res`` at the chunk's ``frames``."""
    n = len(frames)
    for k in fields:
        res[k][frames] = sub[k][first:first + n]
    res[errors].update({int(f): sub[errors][first + i] for i, f in enumerate(frames) if first + i in sub[errors]})


def free_blocks(st):
    """Free the device blocks a chunk's or a re-run's state holds (a second call finds nothing), and the re-run record started early
    for the chunk, if any."""
    if st is None:
        return
    for k in ("out", "dbatch", "db", "flags", "aux", "vote_out", "side"):
        if st.get(k) is not None:
            for blk in st[k] if isinstance(st[k], list) else [st[k]]:
                blk.free()
            st[k] = None
    if st.get("early") is not None:
        st.pop("early").free()


def wait_out(*handles):
    """Until the pool jobs of ``handles`` (None: none) no longer write into their slots."""
    for h in handles:
        if h is not None:
            with contextlib.suppress(Exception):
                h.get()


class Rerun:
    """A chunk's frames to redo through the host's triangulations.  ``res``: the chunk's results (the re-run's values are scattered
    into them); ``redo``: the frames' positions in the chunk.  ``chain``: the re-run's steps as ``(ready, step)`` pairs, ``step(wait)``
    taken once ``ready()`` (``wait``: forced by ``finish_all``), and ``collect()`` its results; ``begun``: ``finish_all`` finishes
    the chain rather than merging the record into the call's one re-run.  ``free()`` releases the record's device blocks and waits
    out its pool handles.  Other keywords: whatever the estimator keeps with it."""

    def __init__(self, res, redo, free, **data):
        self.res, self.redo, self.free = res, redo, free
        self.chain, self.step, self.collect, self.begun = [], 0, None, False
        self.__dict__.update(data)


def advance(records):
    """Each record one step further where that step would not wait."""
    for r in records:
        if r.step < len(r.chain) and r.chain[r.step][0]():
            r.chain[r.step][1](False)
            r.step += 1


def advance_while(records, outstanding):
    """While ``outstanding()`` (a chunk's results are waited for), the records' steps are taken the moment their inputs are there:
    the thread looks in on them every 0.2 ms instead of sleeping until the chunk's results arrive."""
    while any(r.step < len(r.chain) for r in records) and outstanding():
        advance(records)
        time.sleep(2e-4)


def finish_all(records, merge, fields, errors, then=None):
    """Every record's re-run done and scattered into its chunk's results: the begun chains' remaining steps forced in stage order
    across records (every launch before any result is waited for), then their results; the other records' frames in ONE re-run,
    ``merge(rest)``.  ``then(record)``: each record's own epilogue, in order.  The records are dropped from ``records``."""
    advance(records)
    begun = [r for r in records if r.begun]
    for s in range(max((len(r.chain) for r in begun), default=0)):
        for r in begun:
            if r.step == s < len(r.chain):
                r.chain[s][1](True)
                r.step += 1
    for r in begun:
        scatter(r.res, r.redo, r.collect(), fields, errors)
    rest = [r for r in records if not r.begun]
    if rest:
        merge(rest)
    if then is not None:
        for r in records:
            then(r)
    del records[:]
