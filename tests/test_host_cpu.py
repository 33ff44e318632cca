"""CPU tests (no GPU): the C-ABI library loads and exports every symbol the header declares, the host
logic (prologue, frame plan, struct packing) matches the reference-generated fixtures, the product path
fails loudly without a GPU, and the N>1 path (instant sharding + in-place all-gather + halo ranges) is
exercised with world_size=2 over gloo using the oracle-backed stand-in backend of tests/fake_backend.py."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden


def test_library_exports_every_header_symbol():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd.hip import ABI_VERSION, SYMBOLS, load_library
    lib = load_library()
    common = open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "eaqhm_common.h")).read()
    assert ABI_VERSION == int(re.search(r"^#define\s+EAQHM_ABI_VERSION\s+(\d+)", common, re.M).group(1))
    header = open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"\b(eaqhm_[a-z_0-9]+)\s*\(", header))
    declared.discard("eaqhm_ctx")
    bound = {n for n, _, _ in SYMBOLS}
    assert declared == bound, (declared ^ bound)
    for name in declared:
        assert getattr(lib, name) is not None


def test_no_cpu_fallback():
    """Without a GPU the product raises; it never routes through the oracle."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import eaqhm_amd
    with pytest.raises(eaqhm_amd.HipUnavailable):
        eaqhm_amd.iqhmLS_complexamps(np.zeros(5), np.ones(1), np.ones(5), 16000)
    g = load_golden("sa19_female_default.npz")
    with pytest.raises(eaqhm_amd.HipUnavailable):
        eaqhm_amd.eaQHMAnalysisAndSynthesis(os.path.join(GOLDEN, "SA19.WAV"), "female", printPrompts=False,
                                            pitch_track=g["swipe_track"])
    with pytest.raises(eaqhm_amd.HipUnavailable):      # the batch entry fails the same way
        eaqhm_amd.eaQHMAnalysisAndSynthesisBatch([os.path.join(GOLDEN, "SA19.WAV")], "female",
                                                 pitch_tracks=[g["swipe_track"]])
    with pytest.raises(ValueError):                    # ... after its own argument checks
        eaqhm_amd.eaQHMAnalysisAndSynthesisBatch(["a.wav", "b.wav"], ["female"])
    pkg = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, fn)).read().replace("no CPU", ""), fn


def test_prologue_and_plan_sa19(sa19_golden):
    from eaqhm_amd import prologue
    from eaqhm_amd.engine import FramePlan
    g = sa19_golden
    fs, s = prologue.read_signal(os.path.join(GOLDEN, "SA19.WAV"))
    assert fs == 16000 and len(s) == 63488
    assert prologue.pitch_limits("female") == (160, 300) and prologue.pitch_limits((90, 400)) == (90, 400)
    assert prologue.pitch_limits("x") == (70, 500) and prologue.pitch_limits("male") == (70, 180)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    assert fstep == int(g["frame_step"])
    assert np.array_equal([f.isSpeech for f in frames], g["vuv_isSpeech"])
    assert np.array_equal([f.isVoiced for f in frames], g["vuv_isVoiced"])
    grid = prologue.resample_track(g["swipe_track"], np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    assert np.abs(grid - g["f0s_5ms"]).max() == 0
    u = load_golden("unit_vectors.npz")
    assert np.abs(prologue.resample_track(u["gl_v"], u["gl_t"]) - u["gl_out"]).max() == 0
    prologue.apply_full_waveform(frames, len(s), 480)
    plan = FramePlan(len(s), fs, grid, frames, fstep, 15, 3, 32, 0)
    assert (plan.Kmax, plan.No_ti, plan.n_frames) == (59, 4233, 4169)
    assert np.array_equal(plan.ti[plan.analysed], g["ti_a0"]) and np.abs(plan.frame_f0 - g["f0_a0"]).max() == 0
    assert np.array_equal(2 * plan.frame_wl + 1, g["ls_shapes_iqhm"][:, 0])
    assert np.array_equal(2 * plan.frame_K + 1, g["ls_shapes_iqhm"][:, 1])
    assert plan.f0_stale == g["stale_f0"][0, 1]


def test_voiced_only_target_and_flags():
    from eaqhm_amd import prologue
    from eaqhm_amd.engine import FramePlan
    g = load_golden("sa19_female_voicedonly_adpt1.npz")
    fs, s = prologue.read_signal(os.path.join(GOLDEN, "SA19.WAV"))
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    plan = FramePlan(len(s), fs, g["f0s_5ms"], frames, fstep, 15, 3, 32, 0)
    assert np.array_equal(plan.in_bounds, g["det_isSpeech"]) and np.array_equal(plan.analysed, g["det_isVoiced"])
    import eaqhm_oracle as O
    ti5 = np.array([f.ti for f in frames])
    ref = O.voiced_only_target(s, ti5, g["vuv_isSpeech"], g["vuv_isVoiced"], fstep)
    assert np.array_equal(prologue.voiced_only_target(s, frames, fstep), ref)


def test_struct_packing_quirks(sa19_golden):
    from eaqhm_amd.functions import _slot_arrays
    from eaqhm_amd.structs import Deterministic, Frame
    d = Deterministic(ti=np.int64(5), isSpeech=True, isVoiced=True)
    assert d.ak == [] and d.a0 == [] and d.frange == [] and d.pk == [] and not hasattr(d, "amplitudes")
    assert "isVoiced" in str(d) and str(Frame(1, True, 0.5)).startswith("{")
    vals = np.array([[1.5, 0, 2.5, 0, 0, 3.5, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 9.0, 0, 0, 0]])
    (arr, empty, one), = _slot_arrays(vals != 0, vals)
    assert len(empty) == 0 and empty.dtype == object and len(one) == 4 and one[3][0] == 9.0 and one[0] == 0
    q = load_golden("unit_vectors.npz")["abi_dtype"]
    assert str(arr.dtype) == q[0] and str(arr.shape) == q[1] and type(arr[1]).__name__ == q[2]
    assert str(np.shape(arr[0])) == q[3] and arr[2][0] == 2.5 and arr[1] == 0


def test_pack_results_fast_and_equal_to_the_cell_loop():
    """functions.py:404-411 for a minute of speech: 64,000 instants x 59 slots, ~2 M active cells.  The
    result must equal what the literal per-cell restatement of misc.py:65-93 builds (checked on a sample of instants)
    (the per-cell Python loop of round 2 took 15.6 s for this on the GPU box's host; `bench.py` reports what the vectorised
    packing takes there: `host_stages_s.pack_results`, 1.0 s)."""
    import time
    from types import SimpleNamespace
    from eaqhm_amd.functions import pack_results
    rng = np.random.default_rng(5)
    T, K = 64000, 59
    am = rng.uniform(0.01, 1, (T, K)) * (rng.uniform(size=(T, K)) < 0.55)
    am[:, 40:] *= rng.uniform(size=(T, 1)) < 0.3
    analysed = np.ones(T, dtype=bool)
    analysed[:32] = analysed[-32:] = False
    analysed[1000:1010] = False
    in_bounds = np.ones(T, dtype=bool)
    in_bounds[:32] = in_bounds[-32:] = False
    am[5000] = 0                                  # a voiced instant without any accepted harmonic
    fin = dict(am=am, fm=am * 1000, pk=am - 0.5, a0=rng.standard_normal(T))
    plan = SimpleNamespace(ti=np.arange(1, 15 * T, 15), No_ti=T, analysed=analysed, in_bounds=in_bounds)
    t0 = time.time()
    det = pack_results(plan, fin)
    took = time.time() - t0
    assert len(det) == T
    # (No timing assertion: this VM's page faults make 6 M object allocations slow and its load varies — 3-4 s here,
    # against 4.5-9 s for the per-cell loop; bench.py measures the real thing on the GPU box's host: 1.0 s vs 15.6 s.)
    print("pack_results: %.2f s for %d instants" % (took, T))
    for i in (0, 31, 32, 999, 1005, 5000, 5001, 40000, T - 33, T - 1):
        d = det[i]
        assert type(d.ti) is np.int64 and d.ti == 15 * i
        assert d.isSpeech == bool(in_bounds[i]) and d.isVoiced == bool(analysed[i])
        if not analysed[i]:
            assert d.a0 == [] and d.ak == [] and not hasattr(d, "amplitudes")
            continue
        assert type(d.a0) is np.float64 and d.a0 == fin["a0"][i] and d.ak == []
        nz = np.flatnonzero(am[i])
        for arr, src in ((d.amplitudes, am), (d.frange, fin["fm"]), (d.pk, fin["pk"])):
            ref = np.zeros(int(nz[-1]) + 1 if len(nz) else 0, dtype=object)       # misc.py:89-93
            for k in nz:
                ref[k] = np.array([src[i, k]])
            assert arr.dtype == object and len(arr) == len(ref)
            for x, y in zip(arr, ref):
                assert type(x) is type(y) and (x == y if isinstance(y, int) else (x.shape == (1,) and x[0] == y[0]))


def test_sharding_ranges():
    from eaqhm_amd.engine import Sharding
    for world in (1, 2, 3, 8):
        for T in (7, 16, 4233):
            got = [Sharding(r, world).instants(T) for r in range(world)]
            assert got[0][0] == 0 and got[-1][1] == T
            assert all(a[1] == b[0] for a, b in zip(got, got[1:]))
            assert max(h - l for l, h in got) <= -(-T // world)


def test_cost_balanced_sharding():
    """ranges balanced by the sum of F(N, Kc), not by the number of instants."""
    from eaqhm_amd.engine import Sharding, ls_cost
    T = 4000
    cost = np.where(np.arange(T) < 2000, ls_cost(241, 53), ls_cost(301, 97))     # high pitch, then low pitch: 4.6x
    cost[:32] = 0
    cost[-32:] = 0                                                               # instants that are not analysed
    for world in (2, 4, 8):
        b = Sharding(0, world).balance(T, cost)
        assert b[0] == 0 and b[-1] == T and all(x <= y for x, y in zip(b, b[1:]))
        shares = np.array([cost[b[r]:b[r + 1]].sum() for r in range(world)])
        assert shares.max() / shares.mean() < 1.01
        counts = np.diff(b)
        assert counts.max() / counts.min() > 2.0
        assert [Sharding(r, world).balance(T, cost) for r in range(world)] == [b] * world    # same on every rank
    assert Sharding(0, 4).balance(10, np.zeros(10)) == [0, 3, 6, 9, 10]          # nothing to balance: equal counts


def test_cli_needs_the_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import eaqhm_amd
    from eaqhm_amd import cli
    with pytest.raises(eaqhm_amd.HipUnavailable):
        cli.main([os.path.join(GOLDEN, "SA19.WAV"), "--gender", "female", "--max-adpt", "0", "--no-write"])


def test_sharding_is_stateless_and_checks_its_ranges():
    """One Sharding may serve several engines (run_interleaved): the ranges live on the engine, and a collective that is
    handed ranges of another buffer refuses instead of exchanging the wrong rows."""
    import torch
    from eaqhm_amd.engine import Sharding
    sh = Sharding(0, 2, group=object())          # (never reaches a collective: the check comes first)
    assert not hasattr(sh, "bounds")
    b = sh.balance(10, np.arange(10.0))
    assert b == sh.balance(10, np.arange(10.0)) and b[0] == 0 and b[-1] == 10
    with pytest.raises(ValueError):
        sh.share_rows(torch.zeros(12, 3), b, 4)
    with pytest.raises(ValueError):
        sh.all_gather_rows(torch.zeros(10, 3), [0, 5])


def test_srer_from_limbs_semantics():
    """One SRER formula for every world size (engine.srer_from_limbs) with NumPy's semantics in the degenerate cases
    the reference passes through silently (functions.py:388, :394: nan compares False, inf <= inf breaks)."""
    from eaqhm_amd.engine import srer_from_limbs
    rng = np.random.default_rng(1)
    d = rng.standard_normal(5000) * 1e-3
    tot = sum(int(v) for v in np.trunc(d * 2.0 ** 60).astype(object))
    tot2 = sum(int(v) for v in np.trunc(d * d * 2.0 ** 64).astype(object))

    def limbs(v):
        return [v & 0xffffffff, (v >> 32) & 0xffffffff, v >> 64]
    L = limbs(tot) + limbs(tot2) + [0, 0]
    want = 20 * np.log10(0.1 / np.std(d))
    assert abs(srer_from_limbs(L, len(d), 0.1) - want) < 1e-9
    # the sum of two ranks' limbs is the limbs of the sum: split the samples anywhere
    h = 1234
    def part(x):
        return limbs(sum(int(v) for v in np.trunc(x * 2.0 ** 60).astype(object))) + \
               limbs(sum(int(v) for v in np.trunc(x * x * 2.0 ** 64).astype(object))) + [0, 0]
    two = [a + b for a, b in zip(part(d[:h]), part(d[h:]))]
    assert srer_from_limbs(two, len(d), 0.1) == srer_from_limbs(L, len(d), 0.1)
    assert np.isnan(srer_from_limbs(L[:6] + [1, 0], len(d), 0.1))            # a non-finite sample
    assert srer_from_limbs([0] * 8, 100, 0.1) == np.inf                       # perfect reconstruction
    assert srer_from_limbs(L, len(d), 0.0) == -np.inf                         # silent target
    assert np.isnan(srer_from_limbs([0] * 8, 100, 0.0))
    assert not (np.float64(np.nan) <= np.float64(1.0)) and np.float64(np.inf) <= np.float64(np.inf)


def test_auto_track_budget_rule():
    """track_budget_bytes="auto" (the drop-in's default): resident while the dense tracks take less than 40 % of the
    free device memory, else a budget between 256 MiB and 4 GiB; without a device (CPU stand-in) resident."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fake_backend import OracleBackend
    from eaqhm_amd import prologue
    from eaqhm_amd.engine import DeviceAnalysis, FramePlan, auto_track_budget
    from eaqhm_amd.synth import synth_speech_int16
    GiB = 2 ** 30
    assert auto_track_budget(54 * GiB, 280 * GiB) is None                  # 60 min @16 kHz on an empty MI355X: resident
    assert auto_track_budget(217 * GiB, 280 * GiB) == 4 * GiB              # 4 h @16 kHz: streamed, capped
    assert auto_track_budget(3 * GiB, 4 * GiB) == int(0.15 * 4 * GiB)      # a crowded device
    assert auto_track_budget(900 * 2 ** 20, GiB) == 256 * 2 ** 20          # never below 256 MiB
    assert auto_track_budget(10 * GiB, None) is None                       # nothing known about the device
    torch.set_num_threads(2)
    fs = 16000
    s = synth_speech_int16(0.3, fs) / 32768.0
    t = np.arange(0, len(s) / fs, 0.001)
    grid = prologue.resample_track(np.column_stack([t, _pitch_profile(t, "true")]),
                                   np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    prologue.apply_full_waveform(frames, len(s), 480)
    plan = FramePlan(len(s), fs, grid, frames, fstep, 15, 3, 32, 0)
    eng = DeviceAnalysis(s, s, plan, 100, 1, ctx=OracleBackend(), track_budget_bytes="auto")
    assert not eng.streaming and len(eng.blocks) == 1
    with pytest.raises(ValueError):
        DeviceAnalysis(s, s, plan, 100, 1, ctx=OracleBackend(), track_budget_bytes="all of it")


def test_time_block_streaming_matches_resident_run_host_logic():
    """SURVEY §8f row 4 (long files): with a track budget the frames are worked off in time blocks whose dense tracks
    are regenerated from the records; the host logic (block plan, windows, seeding flags, stop rule) with the oracle
    stand-in must reproduce the resident run exactly, and hold no more track cells than the budget allows."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fake_backend import OracleBackend
    from eaqhm_amd import prologue
    from eaqhm_amd.engine import DeviceAnalysis, FramePlan
    from eaqhm_amd.synth import synth_speech_int16
    torch.set_num_threads(2)
    fs = 16000
    x = synth_speech_int16(0.72, fs).copy()
    x[5200:6100] = 0                                  # digital silence: empty-row seeding inside one block's halo
    s = x / 32768.0
    t = np.arange(0, len(s) / fs, 0.001)
    grid = prologue.resample_track(np.column_stack([t, _pitch_profile(t, "true")]),
                                   np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    prologue.apply_full_waveform(frames, len(s), 480)
    plan = FramePlan(len(s), fs, grid, frames, fstep, 15, 3, 32, 0)
    res = DeviceAnalysis(s, s, plan, 100, 2, ctx=OracleBackend())
    res.run()
    budget = DeviceAnalysis.TRACK_BYTES_PER_CELL * plan.Kmax * 1500
    blk = DeviceAnalysis(s, s, plan, 100, 2, ctx=OracleBackend(), track_budget_bytes=budget)
    assert len(blk.blocks) >= 4 and blk.track_bytes() <= budget < res.track_bytes()
    assert blk.blocks[0][0] == 0 and blk.blocks[-1][1] == blk.nf
    assert all(a[1] == b[0] for a, b in zip(blk.blocks, blk.blocks[1:]))
    c = plan.frame_c
    for fa, fb, lo, hi in blk.blocks:                # every window of the block (+ the sample before) is resident
        assert lo <= c[fa] - plan.frame_wl[fa] - 1 or lo == 0
        assert c[fb - 1] + plan.frame_wl[fb - 1] < hi and (hi - lo) <= 1500
    blk.run()
    assert [float(v) for v in blk.SRER] == [float(v) for v in res.SRER]
    a, b = res.final_arrays(), blk.final_arrays()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        DeviceAnalysis(s, s, plan, 100, 2, ctx=OracleBackend(), track_budget_bytes=1000)


def test_bench_self_launch_returns_a_failed_rank_promptly():
    """`python bench.py --gpus 2` without a launcher starts the ranks itself; when a rank fails (here: no GPU in this
    container) the parent must return its exit code at once instead of waiting for the others."""
    import subprocess
    import time
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the ranks would run")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, timeout=120)
    assert r.returncode != 0 and time.time() - t0 < 60
    assert b"needs an MI355X" in r.stderr and r.stdout.strip() == b""


def test_bench_dump_outputs_stay_within_budget(tmp_path, monkeypatch):
    """`bench.py --dump-outputs`: float64 files of at most DUMP_BYTES in all; arrays too large for the budget keep the
    same seeded rows (am / fm / pk of one instant stay together), small ones are written whole."""
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(1)
    am = rng.standard_normal((8000, 59))
    arrays = dict(a0=np.arange(8000.0), am=am, fm=2 * am, s_recon=rng.standard_normal(300000),
                  SRER=np.arange(5, dtype=np.float32))
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "whole" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, v), k
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 10 ** 6)
    bench.dump_outputs(str(tmp_path / "sample"), arrays)
    files = sorted((tmp_path / "sample").iterdir())
    assert sum(f.stat().st_size for f in files) <= 4 * 10 ** 6
    got = {f.stem: np.load(f) for f in files}
    assert set(got) == set(arrays) and all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["a0"], arrays["a0"]) and np.array_equal(got["SRER"], arrays["SRER"])
    n = len(got["am"])
    assert 0 < n < 8000 and np.array_equal(got["fm"], 2 * got["am"])
    assert np.array_equal(got["am"], am[np.sort(np.random.default_rng(0).choice(8000, n, replace=False))])
    assert 0 < len(got["s_recon"]) < 300000


def _pitch_profile(t, profile):
    f0 = 220.0 + 40.0 * np.sin(2 * np.pi * 0.31 * t) + 10.0 * np.sin(2 * np.pi * 1.7 * t)
    if profile == "step":      # a pitch track that drops to 0.7 of the true pitch half way: the second half's frames
        f0 = np.where(t < 0.5 * t[-1], f0, 0.7 * f0)    # have ~1.4x the harmonics and longer windows (~3x the cost)
    return f0


# ----------------------------------------------------------------------------- world_size = 2 over gloo
def _sharded_worker(rank, world, port, out_path, profile="true", dur=0.62):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fake_backend import OracleBackend
    from eaqhm_amd import prologue
    from eaqhm_amd.engine import DeviceAnalysis, FramePlan, Sharding
    from eaqhm_amd.synth import synth_speech_int16
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from threadpoolctl import threadpool_limits
    threadpool_limits(limits=2)          # two ranks share the CI container's 8 cores
    fs = 16000
    s = synth_speech_int16(max(dur, 0.3), fs)[:int(dur * fs)] / 32768.0
    t = np.arange(0, len(s) / fs, 0.001)
    f0 = _pitch_profile(t, profile)
    grid = prologue.resample_track(np.column_stack([t, f0]), np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    prologue.apply_full_waveform(frames, len(s), 480)
    plan = FramePlan(len(s), fs, grid, frames, fstep, 15, 3, 32, 0)
    eng = DeviceAnalysis(s, s, plan, 100, 2, shard=Sharding(rank, world, dist.group.WORLD), ctx=OracleBackend())
    eng.run()
    fin = eng.final_arrays()
    if rank == 0:
        np.savez(out_path, SRER=np.array(eng.SRER), n_frames_rank0=eng.n_ls_frames, bounds=np.array(eng.bounds),
                 **fin)
    dist.destroy_process_group()


@pytest.mark.slow
@pytest.mark.parametrize("world,profile", [(2, "true"), (4, "true"), (2, "step")])
def test_two_rank_gloo_matches_single_process(tmp_path, world, profile):
    """world 4 has interior ranks (two neighbours each) for the boundary-row exchange; the "step" pitch profile makes
    the second half of the file ~3x as expensive per frame, so the cost-balanced ranges differ clearly in length."""
    import torch.multiprocessing as mp
    import eaqhm_oracle as O
    from eaqhm_amd import prologue
    from eaqhm_amd.synth import synth_speech_int16
    out = str(tmp_path / "rank0.npz")
    mp.spawn(_sharded_worker, args=(world, 29000 + os.getpid() % 2000 + world + 10 * len(profile), out, profile),
             nprocs=world, join=True)
    got = np.load(out)
    fs = 16000
    s = synth_speech_int16(0.62, fs) / 32768.0
    t = np.arange(0, len(s) / fs, 0.001)
    f0 = _pitch_profile(t, profile)
    b = got["bounds"]
    if profile == "step":
        assert (b[1] - b[0]) > 1.3 * (b[2] - b[1]), "ranges not cost-balanced: %r" % (b,)
    grid = prologue.resample_track(np.column_stack([t, f0]), np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    ref = O.analyse(s, fs, grid, np.array([f.ti for f in frames]), np.array([float(f.isSpeech) for f in frames]),
                    np.array([float(f.isVoiced) for f in frames]), fstep, f0min=100, maxAdpt=2)
    assert len(got["SRER"]) == len(ref["SRER"])
    assert np.abs(got["SRER"] - np.array(ref["SRER"])).max() < 1e-9
    # (the same NumPy code on both sides; the mis-scaled pitch of "step" gives badly conditioned systems, where the
    # ranks' 2 BLAS threads and this process's 8 already round differently: profiles/r02_parity/conditioning_f0scale.txt)
    lo = 1.0 if profile == "true" else 1e3
    assert np.abs(got["s_recon"] - ref["s_recon"]).max() < 1e-11 * lo
    assert np.abs(got["am"] - ref["am"]).max() < 1e-12 * lo and np.abs(got["fm"] - ref["fm"]).max() < 1e-7 * lo
    assert np.abs(got["pk"] - ref["pk"]).max() < 1e-9 * lo and np.abs(got["a0"] - ref["a0"]).max() < 1e-12 * lo
    assert 0 < int(got["n_frames_rank0"]) < ref["n_ls_frames"]      # rank 0 analysed only its share


@pytest.mark.slow
def test_more_ranks_than_work_gloo(tmp_path):
    """Four ranks on a file with a handful of analysed frames: ranges shorter than the boundary margin (the exchange falls
    back to whole rows) and ranks that may own no frame at all — same result as the single-process oracle."""
    import torch.multiprocessing as mp
    import eaqhm_oracle as O
    from eaqhm_amd import prologue
    from eaqhm_amd.synth import synth_speech_int16
    out, dur, fs = str(tmp_path / "rank0.npz"), 0.075, 16000
    mp.spawn(_sharded_worker, args=(4, 31000 + os.getpid() % 2000, out, "true", dur), nprocs=4, join=True)
    got = np.load(out)
    s = synth_speech_int16(0.3, fs)[:int(dur * fs)] / 32768.0
    t = np.arange(0, len(s) / fs, 0.001)
    grid = prologue.resample_track(np.column_stack([t, _pitch_profile(t, "true")]),
                                   np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    ref = O.analyse(s, fs, grid, np.array([f.ti for f in frames]), np.array([float(f.isSpeech) for f in frames]),
                    np.array([float(f.isVoiced) for f in frames]), fstep, f0min=100, maxAdpt=2)
    assert 0 < ref["n_ls_frames"] // len(ref["SRER"]) < 40          # a handful of frames for four ranks
    assert len(got["SRER"]) == len(ref["SRER"])
    assert np.abs(got["SRER"] - np.array(ref["SRER"])).max() < 1e-9
    assert np.abs(got["s_recon"] - ref["s_recon"]).max() < 1e-11
    assert np.array_equal(got["am"] != 0, ref["am"] != 0) and np.abs(got["am"] - ref["am"]).max() < 1e-12


def test_swipe_matches_reference_tracks(sa19_golden, sa19_signal):
    """Host SWIPE' restatement (swipe.py) against the tracks the reference's SWIPE.py produced."""
    from eaqhm_amd.swipe import swipep
    fs, s = sa19_signal
    tr = swipep(s, fs, [160, 300])
    ref = sa19_golden["swipe_track"]
    assert tr.shape == ref.shape and np.abs(tr[:, 0] - ref[:, 0]).max() == 0
    assert np.abs(tr[:, 1] - ref[:, 1]).max() < 1e-9 and np.abs(tr[:, 2] - ref[:, 2]).max() < 1e-12
    g = load_golden("synth16k_2s_adpt3.npz")
    tr = swipep(g["wav_int16"] / 32768.0, 16000, [160, 300])
    assert np.abs(tr[:, 1] - g["swipe_track"][:, 1]).max() < 1e-9


def test_swipe_on_tiled_signal_matches_prep_fixture():
    """SA19 tiled x2 (the bench workload family): SWIPE' + 5 ms resampling against the fixture grid."""
    from scipy.io import wavfile
    from eaqhm_amd import prologue
    from eaqhm_amd.swipe import swipep
    fs, x = wavfile.read(os.path.join(GOLDEN, "SA19.WAV"))
    s = np.tile(x, 2) / 32768.0
    grid = prologue.resample_track(swipep(s, fs, [160, 300]), np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    ref = load_golden("prep_fixtures.npz")["sa19x2_f0s_5ms"]
    assert grid.shape[0] == ref.shape[0] and np.abs(grid[:, 1] - ref[:, 1]).max() < 1e-9


def test_bench_workloads_are_complete():
    """bench.py's named workloads (BASELINE.json configs 2-5) find their committed pitch fixtures, and the default one
    has the frame geometry DESIGN.md quotes (63,936 LS frames per adaptation, Kmax 59, 8-12 tile rows)."""
    sys.path.insert(0, ROOT)
    import bench
    from eaqhm_amd.engine import FramePlan, ls_cost
    for wl in ("synth16k_60s", "synth48k_60s"):
        fs, track = bench.load_track(wl)
        assert track.shape[1] >= 2 and track.shape[0] == 12000 and np.all(track[:, 1] > 150)
    fs, s, grid, frames, fstep = bench.load_workload("synth16k_60s")
    plan = FramePlan(len(s), fs, grid, frames, fstep, 15, 3, 32, 0)
    assert (plan.L, plan.n_frames, plan.Kmax) == (960000, 63936, 59)
    nt = (2 * (2 * plan.frame_K + 1) + 1 + 15) // 16
    assert nt.min() >= 7 and nt.max() == 12
    flops = float(ls_cost(2 * plan.frame_wl.astype(np.int64) + 1, 2 * plan.frame_K.astype(np.int64) + 1).sum())
    assert abs(flops - 1.306e12) / 1.306e12 < 0.01            # adaptation-0 geometry (bench sums the actual n_active per launch)
    fs, s, track = bench.load_signal("sa19x10")
    assert len(s) == 634880
