"""Parity of the HIP path (through the C ABI) against the CPU oracle and the committed golden vectors of the reference —
the `rescale` estimator (the one /root/reference/src/main.py:20 imports) and its kernels.  Needs a real MI355X:  python -m pytest tests -m gpu

Constructions say which path they mean: ``triangulation="scipy"`` is the host-SciPy baseline every device path is compared with; a
construction without the keyword IS the shipped default (triangulation "gpu" with the reference's vote)."""
import os

import numpy as np
import pytest

from conftest import load_json, load_npz
from gpu_helpers import _check_error_mid_call_is_released, _check_rescale_device_against_oracle, _declining, _ransac_triples, _rescale_frames

pytestmark = pytest.mark.gpu


def test_rescale_variant_golden(gpu):
    """mvoscalerecovery_amd.rescale.ScaleEstimator against the reference's rescale.ScaleEstimator run
    with the same RANSAC sample triples (tests/golden/rescale.npz): vote masks, kept-triangle vertex
    lists, inlier counts exact; continuous values (heights from an LU solve vs LAPACK's inverse, the
    plane from a cross product vs an SVD null vector) within 1e-9 relative; north-star bound 1e-4."""
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    z, meta = load_npz("rescale.npz")
    call = {"k": -1}

    def sampler(n):
        call["k"] += 1
        return _ransac_triples(meta["ransac_seed"], call["k"], n)
    est = ScaleEstimator(meta["abs_ref"], window_size=meta["window"], sampler=sampler)
    for i, fr in enumerate(meta["frames"]):
        f3, f2 = synth.synth_frame(fr["frame_idx"], fr["n"], base_seed=fr["seed"], upper_fraction=fr["upper_fraction"])
        s, sd = est.scale_calculation(f3, f2)
        assert np.array_equal(est.last["valid"][0], z["f%d_valid" % i]), i
        pf2, fl = est.last["pf2"], est.last["tri_flags"]
        ids = est.last["tris2"][0][(fl[:int(pf2.tri2_off[1])] & 4) != 0].reshape(-1)
        assert np.array_equal(ids, z["f%d_ids" % i]), i
        np.testing.assert_allclose(est.height_level, float(z["f%d_height_level" % i]), rtol=1e-9)
        if "f%d_model" % i in z.files:
            m_ref = z["f%d_model" % i]
            m_ref = m_ref if m_ref[1] >= 0 else -m_ref
            np.testing.assert_allclose(est.last["model"][0], m_ref, rtol=1e-8, atol=1e-12)
            assert int(est.last["best_ic"][0]) == int(z["f%d_best_ic" % i]), i
            assert int(est.last["used"][0]) == int(z["f%d_used" % i]), i
        assert sd == 1
        assert abs(s - float(z["f%d_scale" % i])) <= 1e-9 * abs(float(z["f%d_scale" % i])), (i, s)


def test_rescale_variant_batch_equals_per_frame(gpu):
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    frames = [synth.synth_frame(i, 500 + 40 * i, base_seed=1357, upper_fraction=0.1) for i in range(8)]
    a = ScaleEstimator(1.75, window_size=5, ransac_seed=11, triangulation="scipy")
    b = ScaleEstimator(1.75, window_size=5, ransac_seed=11, triangulation="scipy")
    seq = [a.scale_calculation(f3, f2)[0] for f3, f2 in frames]
    bat, _ = b.scale_calculation_batch([f[0] for f in frames], [f[1] for f in frames])
    assert seq == list(bat)
    assert list(a.scale_queue) == list(b.scale_queue)


@pytest.mark.parametrize("batch", [True, False])
def test_rescale_device_resident_vs_oracle(gpu, batch):
    """rescale.ScaleEstimator(triangulation="gpu") — Delaunay, vote, Delaunay, flat_selection + RANSAC, slew limiter and
    window median all on the device — against the oracle's restatement of /root/reference/src/rescale.py:113-178 with the
    same counter-based sample sequence and SciPy's triangulations in canonical row form: masks, point lists, inlier
    counts and consumed hypotheses exact; heights / planes / scales to 1e-9 (LU vs LAPACK's inverse, cross product vs SVD)."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    from oracle import rescale_oracle as ro
    frames = _rescale_frames([400, 640, 900, 1300, 2000, 150, 2000, 777, 1024, 2000, 333, 1800, 120, 128, 110, 140])   # (small frames: point lists that repeat few vertices often)
    est = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=1234)
    ref = ro.OracleRescaleEstimator(1.75, window_size=5, device_seed=1234)
    _check_rescale_device_against_oracle(est, ref, frames, batch)
    assert est.last_declined == 0


def test_rescale_gpu_equals_scipy_device_sampling(gpu):
    """triangulation="gpu" and triangulation="scipy" with sampling="device" are the same function: bit-identical scales,
    planes and counts over a ragged batch that spans several chunks of the streaming path, batch == per-frame."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    rng = np.random.default_rng(3)
    frames = _rescale_frames([int(n) for n in rng.integers(120, 1500, 96)], base_seed=77)
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    a = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=99)
    a.GPU_CHUNK = 20                                                  # several chunks, a pipeline
    sa, _ = a.scale_calculation_batch(f3s, f2s)
    b = ScaleEstimator(1.75, window_size=5, triangulation="scipy", sampling="device", ransac_seed=99)
    sb, _ = b.scale_calculation_batch(f3s, f2s)
    assert np.array_equal(sa, sb)
    for k in ("model", "best_ic", "used", "n_kept", "status", "height_level", "raw_scale"):
        assert np.array_equal(a.last[k], b.last[k], equal_nan=True), k
    c = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=99)
    sc = [c.scale_calculation(f3, f2)[0] for f3, f2 in frames[:24]]
    assert sc == list(sa[:24])
    # two calls == one call (the window state, the running scale and the sample counter carry over)
    d = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=99)
    s1, _ = d.scale_calculation_batch(f3s[:40], f2s[:40])
    s2, _ = d.scale_calculation_batch(f3s[40:], f2s[40:])
    assert np.array_equal(np.concatenate([s1, s2]), sa)
    assert list(d.scale_queue) == list(a.scale_queue) and d.scale == a.scale


def test_rescale_device_resident_reference_golden(gpu):
    """The device-resident path against the REFERENCE's own run (tests/golden/rescale.npz: rescale.ScaleEstimator with
    random.sample replaying recorded triples).  The recorded triples are list positions in SciPy's row order; mapped to
    the point ids they picked (id_triples) they replay the same hypotheses on the device's canonical rows: vote masks
    equal, kept-vertex multisets equal, inlier counts and consumed hypotheses equal, level / plane / scale to 1e-9."""
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    z, meta = load_npz("rescale.npz")
    est = ScaleEstimator(meta["abs_ref"], window_size=meta["window"], triangulation="gpu", ransac_seed=0)
    est.stage_outputs = True
    call = -1
    for i, fr in enumerate(meta["frames"]):
        f3, f2 = synth.synth_frame(fr["frame_idx"], fr["n"], base_seed=fr["seed"], upper_fraction=fr["upper_fraction"])
        ids_ref = z["f%d_ids" % i]
        tr = None
        if len(ids_ref) >= 12:
            call += 1
            lt = z["f%d_list_triples" % i] if "f%d_list_triples" % i in z.files else _ransac_triples(meta["ransac_seed"], call, len(ids_ref))
            tr = [ids_ref[lt].astype(np.int32)]        # (frame 26: every tenth triple names one vertex twice — counted as zero inliers here,
        s, sd = est.scale_calculation_batch([f3], [f2], id_triples=tr, stage=True)      # as rounding noise by the reference: same best plane)
        assert np.array_equal(est.last["valid"][0], z["f%d_valid" % i]), i
        ids = est.last["tris2"][0][(est.last["tri_flags"][0] & 4) != 0].reshape(-1)
        assert np.array_equal(np.sort(ids), np.sort(ids_ref)), i
        np.testing.assert_allclose(est.last["height_level"][0], float(z["f%d_height_level" % i]), rtol=1e-9)
        if "f%d_model" % i in z.files:
            m_ref = z["f%d_model" % i]
            m_ref = m_ref if m_ref[1] >= 0 else -m_ref
            np.testing.assert_allclose(est.last["model"][0], m_ref, rtol=1e-7, atol=1e-11)
            assert int(est.last["best_ic"][0]) == int(z["f%d_best_ic" % i]), i
            assert int(est.last["used"][0]) == int(z["f%d_used" % i]), i
        assert abs(s[0] - float(z["f%d_scale" % i])) <= 1e-9 * abs(float(z["f%d_scale" % i])), (i, s)


def test_rescale_device_resident_steady_state_allocates_nothing(gpu):
    """A steady-state call of the device-resident path takes every buffer from the context's caches: no hipMalloc /
    hipHostMalloc between the second and the third call over the same shapes."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    frames = _rescale_frames([900] * 64, base_seed=5)
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    est = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=1)
    est.scale_calculation_batch(f3s, f2s)
    est.scale_calculation_batch(f3s, f2s)
    before = gpu.alloc_stats()
    est.scale_calculation_batch(f3s, f2s)
    after = gpu.alloc_stats()
    assert after["hip_malloc"] == before["hip_malloc"] and after["host_malloc"] == before["host_malloc"], (before, after)


def test_slew_median_kernel(gpu):
    """mvosr_slew_median against the reference's recurrence (rescale.py:169-178) written out in Python: jumps beyond
    +-0.3, frames without a plane, a carried-in queue, lengths around the 64-frame blocks of the kernel."""
    import ctypes as C
    from collections import deque
    from mvoscalerecovery_amd import _lib
    rng = np.random.default_rng(8)
    for n in (1, 5, 63, 64, 65, 1000):
        raw = rng.uniform(0.5, 3.5, n)
        raw[rng.random(n) < 0.1] += 5.0
        apply = (rng.random(n) > 0.2).astype(np.int32)
        raw[apply == 0] = np.nan
        q_in, s_in, window = [1.25, 1.5], 1.5, 5
        scale, q, want_p, want_f = s_in, deque(q_in), [], []
        for i in range(n):
            if apply[i]:
                if raw[i] - scale > 0.3:
                    scale += 0.3
                elif raw[i] - scale < -0.3:
                    scale -= 0.3
                else:
                    scale = raw[i]
            q.append(scale)
            if len(q) > window:
                q.popleft()
            want_p.append(scale)
            want_f.append(np.median(q))
        io = gpu.block([("raw", n, np.float64), ("apply", n, np.int32), ("pushed", n, np.float64), ("filtered", n, np.float64)])
        io.upload({"raw": raw, "apply": apply})
        qa = np.array(q_in)
        _lib.check(gpu.lib.mvosr_slew_median(gpu.handle, io["raw"].ptr, io["apply"].ptr, n, 0.3, s_in, window, _lib.addr(qa), 2,
                                             io["pushed"].ptr, io["filtered"].ptr))
        assert io["pushed"].download().tolist() == want_p and io["filtered"].download().tolist() == want_f, n
        io.free()


def test_rescale_sharded_sequence_driver_two_ranks_one_gpu(gpu, tmp_path):
    """The estimator the reference's main_offline.py imports behind the sharded driver: two ranks (gloo, sharing this GPU)
    each run the device-resident per-frame half on their block of the 200-frame sequence, ONE all-gather reassembles the raw
    scales, every rank applies the slew limiter and window median — the same scales, bit for bit, as the single-process
    batched run and as the per-frame loop (the sample sequence is keyed by a frame's position in the sequence)."""
    import subprocess
    import sys
    import textwrap
    from conftest import ROOT
    from mvoscalerecovery_amd import offline, synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    data = synth.synth_sequence_dict(200, base_seed=41, n_lo=300, n_hi=1500)
    one = offline.run_sequence_batched(data, ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=8))
    loop = offline.run_sequence(data, ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=8))
    np.testing.assert_array_equal(one["scales"], loop["scales"])
    solo = offline.run_sequence_sharded(data, ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=8))
    np.testing.assert_array_equal(solo["scales"], one["scales"])
    np.save(tmp_path / "want.npy", one["scales"])
    script = tmp_path / "worker.py"
    script.write_text(textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %(root)r)
        import numpy as np
        import torch.distributed as dist
        from mvoscalerecovery_amd import offline, sharding, synth
        from mvoscalerecovery_amd.rescale import ScaleEstimator
        rank, local, world = sharding.init_distributed("gloo")
        data = synth.synth_sequence_dict(200, base_seed=41, n_lo=300, n_hi=1500)
        res = offline.run_sequence_sharded(data, ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=8))
        assert np.array_equal(res["scales"], np.load(%(want)r)), "rank %%d differs" %% rank
        dist.barrier()
        dist.destroy_process_group()
        print("rank", rank, "ok")
    """) % {"root": ROOT, "want": str(tmp_path / "want.npy")})
    port = 29500 + os.getpid() % 150
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), MVOSR_SHARE_GPU="1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for rank, p in enumerate(procs):
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
        assert p.returncode == 0, out
        assert "rank %d ok" % rank in out


def test_rescale_oversized_frame_is_refused_up_front(gpu):
    """one 5000-feature frame inside a normal batch of the device-resident rescale path: a ValueError that names the
    frame and the limit — not a library error from mvosr_flat_ransac_batch —, raised like every other error of a run: the frames
    BEFORE it have gone through the slew limiter, the window and the sample counter (what the reference's per-frame loop leaves
    behind), nothing queued is dropped, and the estimator carries on."""
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    frames = [synth.synth_frame(i, 600, base_seed=77) for i in range(6)]
    frames.insert(3, synth.synth_frame(99, 5000, base_seed=77))
    for kw in ({"triangulation": "gpu"}, {"triangulation": "scipy", "sampling": "device"}):
        est = ScaleEstimator(1.75, window_size=5, ransac_seed=3, delaunay_workers=0, **kw)
        with pytest.raises(ValueError, match="frame 3 has 5000 features"):
            est.scale_calculation_batch([f[0] for f in frames], [f[1] for f in frames])
        ref = ScaleEstimator(1.75, window_size=5, ransac_seed=3, delaunay_workers=0, **kw)
        s3, _ = ref.scale_calculation_batch([f[0] for f in frames[:3]], [f[1] for f in frames[:3]])
        assert list(est.scale_queue) == list(ref.scale_queue) and est.scale == ref.scale and len(est.scale_queue) == 3, kw
        assert est._frame_counter == 4                                        # (the refused frame took its turn)
        with pytest.raises(ValueError, match="frame 0 has 5000 features"):       # ... also as the first frame of a call
            est.scale_calculation_batch([frames[3][0]], [frames[3][1]])
        s, _ = est.scale_calculation_batch([f[0] for f in frames[4:]], [f[1] for f in frames[4:]])      # the estimator is still usable
        assert np.all(np.isfinite(s))
    # a frame with 5000 features of which few lie below the vanishing row is an ordinary frame
    f3, f2 = synth.synth_frame(5, 5000, base_seed=77, upper_fraction=0.8)
    est = ScaleEstimator(1.75, window_size=5, ransac_seed=3, delaunay_workers=0, triangulation="gpu")
    s, _ = est.scale_calculation_batch([f3], [f2])
    assert np.all(np.isfinite(s))


def test_rescale_any_window_size(gpu):
    """The reference takes any window (/root/reference/src/rescale.py:23,175-178); the C loop's ring buffer holds 64: larger windows
    (and 0: np.median of an empty deque) walk the same recurrence in Python — against the oracle."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    from oracle import rescale_oracle as ro
    frames = _rescale_frames([700] * 12, base_seed=31)
    for w in (1, 64, 65, 100):
        est = ScaleEstimator(1.75, window_size=w, ransac_seed=5, delaunay_workers=0, triangulation="gpu")
        ref = ro.OracleRescaleEstimator(1.75, window_size=w, device_seed=5)
        s, _ = est.scale_calculation_batch([f[0] for f in frames], [f[1] for f in frames])
        want = [ref.scale_calculation(f3, f2)[0] for f3, f2 in frames]
        np.testing.assert_allclose(s, want, rtol=1e-9)
    est = ScaleEstimator(1.75, window_size=0, ransac_seed=5, delaunay_workers=0, triangulation="gpu")
    s, _ = est.scale_calculation_batch([f[0] for f in frames[:3]], [f[1] for f in frames[:3]])
    assert np.all(np.isnan(s)) and len(est.scale_queue) == 0


def test_rescale_main_offline_reference_golden_device_resident(gpu):
    """/root/reference/src/main_offline.py ITSELF with the estimator it really imports (rescale.ScaleEstimator,
    random.sample replaying recorded triples) on the 200-frame dict (tests/golden/seq200_rescale_main_offline.npz) against
    offline.run_sequence_batched with rescale.ScaleEstimator(triangulation="gpu") and the same triples mapped to point ids: the
    scales file to 1e-9 — move_flag skips, the N > 100 gate, "repeat the previous scale", slew limiter and window median included."""
    from mvoscalerecovery_amd import offline, synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    z, meta = load_npz("seq200_rescale_main_offline.npz")
    data = synth.synth_sequence_dict(meta["n_frames"], base_seed=meta["seed"], **meta["kw"])
    ids, ids_off, ran = z["ids"], z["ids_off"], z["ran"]
    triples, call = [], -1
    for k in range(len(ran)):
        lst = ids[ids_off[k]:ids_off[k + 1]]
        if ran[k]:
            call += 1
            triples.append(lst[_ransac_triples(meta["ransac_seed"], call, len(lst))].astype(np.int32))
        else:
            triples.append(np.zeros((100, 3), np.int32))
    est = ScaleEstimator(meta["abs_ref"], window_size=meta["window"], triangulation="gpu", ransac_seed=0)
    res = offline.run_sequence_batched(data, est, id_triples=triples)
    assert res["scales"].shape == z["scales"].shape
    np.testing.assert_allclose(res["scales"], z["scales"], rtol=1e-9, atol=0)
    loop = offline.run_sequence(data, ScaleEstimator(meta["abs_ref"], window_size=meta["window"], triangulation="gpu", ransac_seed=0))
    assert loop["scales"].shape == z["scales"].shape and np.all((loop["scales"] == 0) == (z["scales"] == 0))    # same skips with its own draws


def test_rescale_device_distribution_matches_the_unseeded_reference(gpu):
    """VERDICT r4 item 2d / ADVICE r4: the reference's RANSAC is unseeded, so parity is statistical.  Six 400-600-feature frames; the
    reference's raw scales over 200 unseeded runs each (tests/golden/rescale_distribution.npz) against the device path over 200
    seeds: means within 3 standard errors, two-sample Kolmogorov-Smirnov p > 0.01 — the sampler spends an iteration on a triple naming one vertex
    twice (zero inliers), as the reference does (ransac.py:8-21): no declared deviation left in this estimator."""
    from scipy import stats
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    z, meta = load_npz("rescale_distribution.npz")
    frames = [synth.synth_frame(fr["frame_idx"], fr["n"], base_seed=fr["seed"], upper_fraction=fr["upper_fraction"]) for fr in meta["frames"]]
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    runs = int(meta["runs"])
    dev = np.zeros((runs, len(frames)))
    for seed in range(runs):
        est = ScaleEstimator(meta["abs_ref"], window_size=5, triangulation="gpu", ransac_seed=1000 + seed)
        est.scale_calculation_batch(f3s, f2s)
        dev[seed] = est.last["raw_scale"]
    for k in range(len(frames)):
        ref = z["f%d_raw_scales" % k]
        d = dev[:, k]
        se = np.sqrt(ref.var(ddof=1) / len(ref) + d.var(ddof=1) / len(d))
        assert abs(ref.mean() - d.mean()) <= 3 * se + 1e-12, (k, ref.mean(), d.mean(), se)
        assert stats.ks_2samp(ref, d).pvalue > 0.01, (k, stats.ks_2samp(ref, d))


def test_rescale_default_construction_is_device_resident(gpu, monkeypatch):
    """rescale.ScaleEstimator(absolute_reference, window_size) as /root/reference/src/main.py:20,55 constructs it: the
    device-resident path (both triangulations, the vote, flat selection and RANSAC on the device; the counter-based sampler);
    MVOSR_TRIANGULATION=scipy, a host sampler or sampling="host" give the host path as before."""
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    monkeypatch.setenv("MVOSR_TRIANGULATION", "scipy")
    assert ScaleEstimator(1.75, window_size=5, delaunay_workers=0).triangulation == "scipy"
    monkeypatch.delenv("MVOSR_TRIANGULATION")
    est = ScaleEstimator(1.75, window_size=5, delaunay_workers=0, ransac_seed=7)
    assert (est.triangulation, est.sampling) == ("gpu", "device")
    assert ScaleEstimator(1.75, window_size=5, delaunay_workers=0, sampling="host").triangulation == "scipy"
    assert ScaleEstimator(1.75, window_size=5, delaunay_workers=0, sampler=lambda n, k: list(range(k))).triangulation == "scipy"
    explicit = ScaleEstimator(1.75, window_size=5, delaunay_workers=0, ransac_seed=7, triangulation="gpu")
    for i in range(8):
        f3, f2 = synth.synth_frame(i, 600 + 150 * i, base_seed=515)
        assert est.scale_calculation(f3, f2) == explicit.scale_calculation(f3, f2), i


def test_rescale_deferred_reruns_started_early(gpu):
    """Round 6: the few frames a chunk's device triangulation declines have their host re-run STARTED when the chunk is collected and
    advanced while the call's later chunks run (``_advance_deferred``: first triangulations on the pool -> vote launched -> keep words
    back -> second triangulations -> flat_selection + RANSAC launched), instead of one merged re-run at the call's end.  Same scales,
    planes and counts as the merged re-run and as triangulation="scipy" with the device's sampler; the early route is really taken."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    F = 1900
    frames = _rescale_frames([150 + (i * 29) % 200 for i in range(F)], base_seed=91)
    declined = [5, 600, 601, 1200, F - 3]
    for f in declined:                                # quarter-pixel grid and a repeated pixel: the device triangulation declines
        a3, a2 = frames[f][0].copy(), np.ascontiguousarray(np.round(frames[f][1] * 4) / 4)
        low = np.nonzero(a2[:, 1] > 200.0)[0]                 # (two sites well below the vanishing row: the repeated site is among the triangulated ones)
        a2[low[1]], a3[low[1]] = a2[low[0]], a3[low[0]]
        frames[f] = (a3, a2)
    f3s, f2s = [f[0] for f in frames], [f[1] for f in frames]
    b = ScaleEstimator(1.75, window_size=5, triangulation="scipy", sampling="device", ransac_seed=99)
    sb, _ = b.scale_calculation_batch(f3s, f2s)
    for early in (True, False):
        a = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=99, delaunay_workers=3 if early else 0)
        a.GPU_REDO_EARLY = early
        sa, _ = a.scale_calculation_batch(f3s, f2s)
        assert np.array_equal(sa, sb), early
        for k in ("model", "best_ic", "used", "n_kept", "status", "height_level", "raw_scale"):
            assert np.array_equal(a.last[k], b.last[k], equal_nan=True), (k, early)
        assert a.last_declined >= len(declined) - 1, a.last_declined
        assert (getattr(a, "redo_early_started", 0) >= 3) == early, getattr(a, "redo_early_started", 0)
        # (the LAST chunk's declined frame: found by the early read of the first triangulation's status)
        assert getattr(a, "redo_early_status_hits", 0) == (1 if early else 0)


def test_rescale_stream_error_mid_call_releases_chunks_and_reruns(gpu, monkeypatch):
    """rescale's streamed call: a host step raising while its third of six chunks is collected, re-runs of the first two pending —
    nothing of the call stays alive on the estimator's contexts or in the Delaunay pool's slots, and the next call is unaffected."""
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    frames = _declining(_rescale_frames([150 + (i * 29) % 200 for i in range(768)], base_seed=91), [5, 130, 700])

    def make():
        est = ScaleEstimator(1.75, window_size=5, triangulation="gpu", ransac_seed=99, delaunay_workers=3)
        est.GPU_CHUNK, est.GPU_RAMP, est.GPU_MIN_CHUNK = 128, False, 1
        return est
    _check_error_mid_call_is_released(make, frames, lambda e: [e.ctx, e._redo_ctx], monkeypatch)
