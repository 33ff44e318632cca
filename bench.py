#!/usr/bin/env python3
"""bench.py — analysis frames/s of the eaQHM hot path on N MI355X (one process per GPU).

    python bench.py [--workload W] --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Called as plain `python bench.py --gpus N` with N > 1 (no WORLD_SIZE in the environment) it starts the N ranks
itself, as fresh child processes, before anything touches a GPU; rank 0 prints the one JSON line.

A "step" is one complete run of the adaptation loop (functions.py:163-402) over the workload: adaptation
0..maxAdpt or until the reference's stop rule fires.  Inputs (signal, pitch grid, frame tables) are resident in HBM
before the timed region; result packing into Python structs is outside it.  `ms_per_step` is the
wall time of one timed step.

A plain run sets up, warms up, times the K steps and prints the headline (frames/s, ms_per_step, the run's SRER).
`--dump-outputs DIR` then also writes what the last timed step computed — the arrays a caller of the analysis
receives: a0, am, fm, pk, s_recon and SRER — as DIR/<name>.npy in float64 (at most 64 MB: see dump_outputs).
`--full` adds everything else, as separate figures of the same line: HIP events around every launch of the timed
steps and the roofline from them, the SRER of the reference's own run where a fixture has it, what lies outside the
timed region timed once in `host_stages_s` (SWIPE', VUV + frame plan, upload, collecting the final arrays, packing the
Deterministic structs) together with the end-to-end rate a caller of eaQHMAnalysisAndSynthesis sees, and the CPU
baseline.

`roofline.frac` (--full) is the rate of the adaptation >= 1 launches (the kernel that executes the complex algorithm
F(N, Kc) counts); the figure over all launches, which credits adaptation 0 with flops its closed-form real algorithm
does not execute, is kept as `frac_all_launches_F_credit`.

Workloads (BASELINE.json configs):
    synth16k_60s  (default) synthetic 60 s speech @16 kHz, `female`, maxAdpt=5 — configs[3], the workload
                  `north_star` quotes the frames/s metric on; 63,936 LS frames per adaptation
    synth48k_60s  the same generator at 48 kHz — configs[4]; 191,936 large frames per adaptation
    sa19          SA19.WAV — configs[1];  sa19x10 — configs[2]
With N > 1 the SAME signal is sharded over the ranks by analysis instants (strong scaling, as config 4 is written).
Pitch grids come from committed fixtures produced by the reference's own SWIPE' (tests/golden), because the
reference cannot travel to the GPU box.

Prints ONE JSON line (rank 0).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

PEAK_FP64_TFLOPS = 78.6   # MI355X FP64 (vector = matrix) spec: half the 157.3 TF FP32 vector peak
                          # of MI355X_MICROARCH.md's chip table
WORKLOADS = ("synth16k_60s", "synth48k_60s", "sa19", "sa19x10")


def ls_flops(N, Kc):
    """Algorithmic FP64 flops of one frame's least squares."""
    from eaqhm_amd.engine import ls_cost
    return ls_cost(N, Kc)


def load_signal(workload):
    """(fs, float signal, 5 ms pitch grid or 1 ms track)."""
    from scipy.io import wavfile
    from eaqhm_amd.synth import synth_speech_int16
    if workload.startswith("sa19"):
        reps = int(workload[5:]) if len(workload) > 4 else 1
        fs, x = wavfile.read(os.path.join(GOLDEN, "SA19.WAV"))
        x = np.tile(x, reps)
        if reps == 1:
            track = np.load(os.path.join(GOLDEN, "sa19_female_default.npz"))["swipe_track"]
        else:
            track = np.load(os.path.join(GOLDEN, "prep_fixtures.npz"))["sa19x%d_f0s_5ms" % reps]
        return fs, x / 32768.0, track
    fs, track = load_track(workload)
    return fs, synth_speech_int16(60.0, fs) / 32768.0, track


def load_track(workload):
    """(fs, 5 ms pitch grid the reference's SWIPE' + getLinear produced for the synthetic workload)."""
    if workload == "synth16k_60s":
        return 16000, np.load(os.path.join(GOLDEN, "prep_fixtures.npz"))["synth16k_60s_f0s_5ms"]
    if workload == "synth48k_60s":
        return 48000, np.load(os.path.join(GOLDEN, "prep_synth48k_60s.npz"))["synth48k_60s_f0s_5ms"]
    raise SystemExit("unknown workload %s (choose from %s)" % (workload, ", ".join(WORKLOADS)))


def load_workload(workload):
    from eaqhm_amd import prologue
    fs, s, track = load_signal(workload)
    grid = prologue.resample_track(track, np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    prologue.apply_full_waveform(frames, len(s), 32 * 15)
    return fs, s, grid, frames, fstep


def source_hash():
    """sha256 over the kernel sources (csrc/*.hip, csrc/*.h, include/*.h): what a profile must have been taken with to
    describe the library this bench runs (tools/summarize_pmc.py stamps the same hash into pmc_hbm_traffic.json)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    base = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc")
    for fn in sorted(glob.glob(os.path.join(base, "*.hip")) + glob.glob(os.path.join(base, "*.h")) +
                     glob.glob(os.path.join(ROOT, "include", "*.h"))):
        h.update(os.path.basename(fn).encode())
        h.update(open(fn, "rb").read())
    return h.hexdigest()[:16]


def reference_srer(workload):
    """SRER list of the REFERENCE for this workload where one exists (fixtures made by tests/golden/make_golden.py, which
    imports the reference in the build container; sa19x10: BASELINE.md)."""
    if workload == "synth16k_60s":
        return [float(v) for v in np.load(os.path.join(GOLDEN, "synth16k_60s_adpt5.npz"))["SRER"]], \
            "tests/golden/synth16k_60s_adpt5.npz (the reference itself on this workload, maxAdpt=5)"
    if workload == "sa19":
        return [float(v) for v in np.load(os.path.join(GOLDEN, "sa19_female_default.npz"))["SRER"]], \
            "tests/golden/sa19_female_default.npz (= the reference's README screenshot)"
    if workload == "sa19x10":
        return [17.866028549428748, 24.213570062975556, 23.958838476216723], "BASELINE.md (reference run of the survey)"
    return None, None


def host_stages(workload, eng, plan, s, fs):
    """What SURVEY §8d keeps outside the metric, timed once on this host: SWIPE' on the workload's signal, VUV + frame
    plan, upload (engine construction), collecting the final arrays, packing the result structs (functions.py:86-146,
    :404-411)."""
    import torch
    from eaqhm_amd import prologue
    from eaqhm_amd.engine import DeviceAnalysis, FramePlan
    from eaqhm_amd.functions import pack_results
    from eaqhm_amd.swipe import swipep
    out = {}
    t0 = time.perf_counter()
    track = swipep(s, fs, [160, 300])
    out["swipe"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    grid = prologue.resample_track(track, np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    prologue.apply_full_waveform(frames, len(s), 32 * 15)
    plan2 = FramePlan(len(s), fs, grid, frames, fstep, 15, 3, 32, 0)
    out["vuv_and_plan"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    eng2 = DeviceAnalysis(s, s, plan2, 160, 0, device_index=eng.ctx.device.index)
    torch.cuda.synchronize()
    out["upload"] = time.perf_counter() - t0
    del eng2
    t0 = time.perf_counter()
    fin = eng.final_arrays()
    out["final_arrays"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    det = pack_results(plan, fin)
    out["pack_results"] = time.perf_counter() - t0
    out["structs"] = len(det)
    return out


def cpu_baseline(workload):
    """The oracle (NumPy port of the reference's path) on a bounded excerpt of the same workload, on this host's
    cores: once with one BLAS thread and once with the GPU box's CPU share per GPU."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import eaqhm_oracle as O
    from threadpoolctl import threadpool_limits
    from eaqhm_amd.synth import synth_speech_int16
    if workload.startswith("sa19"):          # SA19.WAV itself, adaptations 0-1
        fs, s, track = load_signal("sa19")
        sample = "SA19.WAV, adaptations 0-1"
        max_adpt = 1
    else:                                    # the workload's generator run for a shorter signal (same seed, same law,
        fs, track = load_track(workload)     # same margins), pitch grid = the head of the workload's
        dur, max_adpt = (2.5, 1) if fs == 16000 else (0.35, 0)     # 48 kHz: ~25 frames/s on a CPU
        s = synth_speech_int16(dur, fs) / 32768.0
        sample = "%.2f s of the workload's synthetic signal, adaptations 0-%d" % (dur, max_adpt)
    grid = O.get_linear(track, np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    ti5, sp, vo, fstep = O.voiced_unvoiced_frames(s, fs, "female")
    host = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = min(host, 16)       # the GPU box's CPU share per GPU; beyond it the small BLAS calls only contend
    runs = {}
    for threads in (1, cores):
        with threadpool_limits(limits=threads):
            t0 = time.time()
            r = O.analyse(s, fs, grid, ti5, sp, vo, fstep, f0min=160, maxAdpt=max_adpt)
            dt = time.time() - t0
        runs[threads] = (r["n_ls_frames"] / dt, dt, r)
    best = max(runs, key=lambda k: runs[k][0])
    return {"value": runs[best][0], "unit": "frames/s", "cores": best, "kind": "port",
            "frames_per_s_1_thread": runs[1][0], "frames_per_s_%d_threads" % cores: runs[cores][0], "host_cores": host,
            "threads_tried": [1, cores],
            "threads_note": "SURVEY 8d asks for 1 thread and all cores; all %d host cores were measured in round 2 at 47 "
                            "frames/s (the LS matrices are 100-200 wide: BLAS threads only contend), so the second leg "
                            "uses the box's per-GPU CPU share (%d)" % (host, cores),
            "sample": "%s (%d LS frames; %.1f s at 1 BLAS thread, %.1f s at %d), oracle/eaqhm_oracle.py"
                      % (sample, runs[1][2]["n_ls_frames"], runs[1][1], runs[cores][1], cores),
            "srer_db": [float(v) for v in runs[best][2]["SRER"]]}


def launch_figures(eng, plan, n_adpt):
    """--full: per-rank figures from the events of the timed region (LS launches on the launch stream)."""
    import torch
    torch.cuda.synchronize()
    ls_ms = [e0.elapsed_time(e1) for (a, st, e0, e1) in eng.timeline if st == "ls"]
    post_ms = [e0.elapsed_time(e1) for (a, st, e0, e1) in eng.timeline if st == "post"]
    gather_ms = [e0.elapsed_time(e1) for (a, st, e0, e1) in eng.timeline if st == "gather"]
    N = 2 * plan.frame_wl[eng.f_lo:eng.f_hi].astype(np.int64) + 1
    n_act = [plan.frame_K[eng.f_lo:eng.f_hi].astype(np.int64)]          # adaptation 0: K harmonics
    for nc in eng.ncol_hist[:max(n_adpt - 1, 0)]:                         # adaptations >= 1: active slots per frame
        n_act.append(nc.cpu().numpy().astype(np.int64))
    flops_per_launch = [float(ls_flops(N, 2 * n + 1).sum()) for n in n_act]
    # algorithmic bytes per launch: 8N signal window + 16 N n_active track windows (a >= 1) +
    # 32 Kc amplitudes and slopes out
    bytes_per_launch = [float(np.sum(8 * N) + (np.sum(16 * N * n) if a > 0 else 0) + np.sum(32 * (2 * n + 1)))
                        for a, n in enumerate(n_act)]
    return {"ls_ms": ls_ms, "post_ms": post_ms, "gather_ms": gather_ms, "flops_per_launch": flops_per_launch,
            "bytes_per_launch": bytes_per_launch, "flops_step": sum(flops_per_launch)}


def roofline_figures(lf, eng, plan, fs, workload, world, allr):
    """--full: the roofline of the dominant kernel from launch_figures() of all ranks (`allr`: one row per rank)."""
    ls_ms, post_ms, gather_ms = lf["ls_ms"], lf["post_ms"], lf["gather_ms"]
    flops_per_launch, bytes_per_launch, flops_step = lf["flops_per_launch"], lf["bytes_per_launch"], lf["flops_step"]
    # roofline of the dominant kernel: algorithmic flops of ALL ranks' launches / (sum of their durations / ranks),
    # i.e. per-GPU achieved rate averaged over the ranks
    ls_total_s = float(allr[:, 2].sum())
    achieved = float(allr[:, 3].sum()) / ls_total_s / 1e12 if ls_total_s > 0 else 0.0
    kernel = "eaqhm_ls_tile_kernel" if fs <= 16000 else "eaqhm_ls_mfma_kernel"
    # Adaptation 0 is solved by a cheaper algorithm than the one F(N, Kc) counts (closed-form Gramian, two real systems of
    # half the order), so its launch "achieves" more algorithmic flops per second than the matrix pipe does work: the
    # rate of the adaptation >= 1 launches alone (rank 0) is reported next to the overall one
    ls_a = [a for (a, st, e0, e1) in eng.timeline if st == "ls"]
    t_ge1 = sum(t for a, t in zip(ls_a, ls_ms) if a >= 1) / 1e3
    f_ge1 = sum(flops_per_launch[a] for a in ls_a if a >= 1 and a < len(flops_per_launch))
    frac_ge1 = (f_ge1 / t_ge1 / 1e12 / PEAK_FP64_TFLOPS) if t_ge1 > 0 else None
    ms0 = [t for a, t in zip(ls_a, ls_ms) if a == 0]
    # HBM traffic of that kernel: not measurable from inside this process; taken from the committed rocprofv3 PMC
    # passes of this same command and workload (profiles/r03_<workload>/pmc_hbm_traffic.json), N = 1 only
    # (the PMC passes of tools/profile_round.sh; used only if they were taken with exactly these kernel sources)
    traffic, traffic_src = None, None
    pmc = os.path.join(ROOT, "profiles", "r03_%s" % workload, "pmc_hbm_traffic.json")
    src = source_hash()
    if world == 1 and os.path.exists(pmc):
        j = json.load(open(pmc))
        traffic_src = {"file": os.path.relpath(pmc, ROOT), "profile_source_hash": j.get("source_hash"),
                       "tree_source_hash": src}
        if j.get("source_hash") == src:
            traffic = j.get(kernel, {}).get("hbm_bytes_per_launch_fetch_doubled")
        else:
            traffic_src["stale"] = "kernel sources changed since the counter passes: traffic withheld"
    achieved_all = achieved
    if frac_ge1 is not None:
        achieved = frac_ge1 * PEAK_FP64_TFLOPS
    roofline = {"bound": "mfma", "kernel": kernel, "achieved": achieved, "peak": PEAK_FP64_TFLOPS,
                "unit": "TFLOP/s", "frac": achieved / PEAK_FP64_TFLOPS,
                "frac_definition": "algorithmic flops F(N,Kc) of the adaptation >= 1 launches / their HIP-event time "
                                   "(rank 0); all launches incl. the cheaper closed-form adaptation 0: frac_all_launches_F_credit",
                "frac_all_launches_F_credit": achieved_all / PEAK_FP64_TFLOPS, "traffic": traffic,
                "traffic_unit": "HBM bytes per launch (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE)",
                "traffic_source": traffic_src,
                "algorithmic_bytes_per_launch": float(np.mean(bytes_per_launch)),
                "algorithmic_bytes_launch0": bytes_per_launch[0],
                "flops_per_launch_mean": flops_step / max(len(flops_per_launch), 1),
                "launch_ms_mean": float(np.mean(ls_ms)) if ls_ms else None,
                "launch_ms_adaptation0": float(np.mean(ms0)) if ms0 else None,
                "frac_adaptation_ge1_launches": frac_ge1,
                "source_hash": src,
                "launches_timed": len(ls_ms),
                "post_stage_ms_mean": float(np.mean(post_ms)) if post_ms else None,
                # the bandwidth-type stage (spline + interpolation + synthesis + SRER, functions.py:337-388):
                # algorithmic bytes = records read (1+3 Kmax) 8 No_ti + tracks and reconstruction written (1+2 Kmax) 8 L
                "post_stage_hbm": (lambda b, t: {"bound": "hbm", "algorithmic_bytes": b, "achieved_GBps": b / t / 1e6,
                                                 "peak_GBps": 8000.0, "frac": b / t / 1e6 / 8000.0})(
                    float((1 + 3 * plan.Kmax) * 8 * plan.No_ti + (1 + 2 * plan.Kmax) * 8 * (eng.t_hi - eng.t_lo)),
                    float(np.mean(post_ms))) if post_ms else None,
                "all_gather_ms_mean": float(np.mean(gather_ms)) if gather_ms else None,
                "ls_ms_mean_per_rank": [float(v) for v in allr[:, 4]],
                "ls_frames_per_rank": [int(v) for v in allr[:, 5]],
                "ls_imbalance_max_over_mean": float(allr[:, 4].max() / allr[:, 4].mean()) if allr[:, 4].mean() > 0 else None}
    return roofline


DUMP_BYTES = 64 * 10 ** 6     # --dump-outputs writes at most this many bytes in all


def dump_outputs(outdir, arrays):
    """`arrays` as outdir/<name>.npy in float64.  The arrays of more than 1 MiB share what the small ones leave of
    DUMP_BYTES; where they do not fit, each keeps the same fraction of its rows (elements of a 1-D array): a fixed
    sample, numpy.random.default_rng(0).choice without replacement, kept in order — the same rows for the same length,
    so am / fm / pk keep the same instants."""
    os.makedirs(outdir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    big = [k for k, a in arrays.items() if a.nbytes > 2 ** 20]
    room = DUMP_BYTES - 1024 * len(arrays) - sum(a.nbytes for k, a in arrays.items() if k not in big)   # .npy headers
    need = sum(arrays[k].nbytes for k in big)
    frac = min(1.0, room / need) if need else 1.0
    for k, a in arrays.items():
        if k in big and frac < 1.0:
            n = a.shape[0]
            a = a[np.sort(np.random.default_rng(0).choice(n, int(n * frac), replace=False))]
        np.save(os.path.join(outdir, k + ".npy"), a)


def self_launch(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as child processes (nothing in this process
    has touched a GPU yet) and pass rank 0's JSON line through.  The children are polled: the first one that fails takes
    its siblings down (they would otherwise sit in a collective until the RCCL timeout) and its exit code is returned.
    A rendezvous port that turns out to be taken (bind-then-close is a race against other jobs) gets two more tries."""
    import socket
    rc = 1
    for attempt in range(3):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        procs = []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                          stdout=None if r == 0 else subprocess.DEVNULL,
                                          stderr=subprocess.PIPE if r == 0 else None))
        rc, err0 = 0, b""
        live = list(procs)
        while live and rc == 0:
            time.sleep(0.2)
            for p in list(live):
                code = p.poll()
                if code is None:
                    continue
                live.remove(p)
                if code != 0:
                    rc = code
        if rc != 0:
            for p in live:               # exact PIDs this process started
                p.terminate()
            for p in live:
                try:
                    p.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    p.kill()
        err0 = procs[0].stderr.read() if procs[0].stderr else b""
        sys.stderr.buffer.write(err0)
        if rc == 0 or b"EADDRINUSE" not in err0 and b"Address already in use" not in err0:
            return rc
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-adpt", type=int, default=5)
    ap.add_argument("--workload", default="synth16k_60s", choices=WORKLOADS)
    ap.add_argument("--full", action="store_true",
                    help="also the roofline (HIP events in the timed steps), the SRER of the reference, the host "
                         "stages and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-host-stages", action="store_true",
                    help="with --full: skip the one-off timing of SWIPE' / VUV / packing")
    ap.add_argument("--track-budget-mb", type=float, default=0.0,
                    help="time-block streaming of the dense tracks under this budget (0: resident) — SURVEY 8f row 4")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float64, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))

    # stdout carries exactly ONE JSON line: everything else (RCCL prints a version banner to stdout) goes to stderr
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    # EAQHM_BENCH_REHEARSAL=1: every rank on GPU 0, collectives staged through the host over gloo — lets a one-GPU box
    # walk through the complete N-rank code path of this file (RCCL itself excepted); its numbers mean nothing
    rehearsal = os.environ.get("EAQHM_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local = 0
    torch.cuda.set_device(local)
    use_dist = world > 1 or os.environ.get("EAQHM_FORCE_DIST") == "1"   # the latter: 1-rank rehearsal of the RCCL path
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))

    from eaqhm_amd.engine import DeviceAnalysis, FramePlan, Sharding
    fs, s, grid, frames, fstep = load_workload(args.workload)
    plan = FramePlan(len(s), fs, grid, frames, fstep, 15, 3, 32, 0)
    if rehearsal and use_dist:
        class HostStaged(Sharding):
            def _all_gather_into(self, out, part):
                host = out.cpu()
                dist.all_gather_into_tensor(host, part.cpu().clone(), group=self.group)
                out.copy_(host)

            def all_reduce_sum(self, t):
                host = t.cpu()
                dist.all_reduce(host, group=self.group)
                t.copy_(host)
        shard = HostStaged(rank, world, dist.group.WORLD)
    else:
        shard = Sharding(rank, world, dist.group.WORLD if use_dist else None)
    eng = DeviceAnalysis(s, s, plan, 160, args.max_adpt, device_index=local, shard=shard,
                         track_budget_bytes=int(args.track_budget_mb * 2 ** 20) if args.track_budget_mb > 0 else None)

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        eng.reset()
        eng.run()
    eng.profile = args.full          # --full: HIP events around every LS launch, on the launch stream
    barrier()
    t0 = time.perf_counter()
    frames_done = 0
    n_adpt = 0
    for _ in range(args.steps):
        eng.reset(keep_timeline=True)
        n_adpt = eng.run()
        frames_done += eng.n_ls_frames
    barrier()
    dt = time.perf_counter() - t0

    if args.dump_outputs:        # every rank takes part (the final arrays are merged over the ranks); rank 0 writes
        fin = eng.final_arrays()
        if rank == 0:
            dump_outputs(args.dump_outputs, dict(fin, SRER=np.array(eng.SRER, dtype=np.float64)))

    mine = [dt, float(frames_done)]
    if args.full:
        lf = launch_figures(eng, plan, n_adpt)
        mine += [sum(lf["ls_ms"]) / 1e3, lf["flops_step"] * args.steps,
                 float(np.mean(lf["ls_ms"])) if lf["ls_ms"] else 0.0, float(eng.nf)]
    if use_dist:
        allr = [None] * world
        dist.all_gather_object(allr, mine)      # (any backend; a few floats per rank, after the timed region)
        allr = np.array(allr, dtype=np.float64)
    else:
        allr = np.array([mine], dtype=np.float64)
    dt = float(allr[:, 0].max())
    frames_total = float(allr[:, 1].sum())
    srer = [float(v) for v in eng.SRER]
    out = {"metric": "analysis_frames_per_sec", "value": frames_total / dt, "unit": "frames/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
           "data": ("synthetic speech-like signal (eaqhm_amd/synth.py, SURVEY §8d config 4 recipe)"
                    if args.workload.startswith("synth") else "SA19.WAV (the reference's sample recording)")
                   + "; pitch grid = fixture from the reference's SWIPE'",
           "config": {"workload": "%s_female_maxAdpt%d" % (args.workload, args.max_adpt), "samples": int(plan.L),
                      "fs": int(fs), "ls_frames_per_adaptation": int(plan.n_frames), "adaptations_executed": n_adpt,
                      "Kmax": int(plan.Kmax), "track_bytes": int(eng.track_bytes()), "time_blocks": len(eng.blocks),
                      "parallelism": "instants sharded x%d by LS cost; boundary records all-gathered per adaptation"
                                     % world},
           "final_srer_db": max(srer), "srer_db": srer}
    if args.full:
        out["roofline"] = roofline_figures(lf, eng, plan, fs, args.workload, world, allr)
    ref, ref_src = reference_srer(args.workload) if args.full else (None, None)
    if ref is not None and args.max_adpt == 5:
        out["srer_ref_db"] = ref
        out["srer_ref_source"] = ref_src
        out["final_srer_ref_db"] = max(ref)
        out["srer_abs_diff_db"] = ([abs(a - b) for a, b in zip(srer, ref)] if len(ref) == len(srer) else None)
        out["final_srer_abs_diff_db"] = abs(max(srer) - max(ref))
    if args.full and rank == 0 and world == 1 and not args.no_host_stages:
        hs = host_stages(args.workload, eng, plan, s, fs)
        loop_s = dt / args.steps
        out["host_stages_s"] = hs
        total = hs["swipe"] + hs["vuv_and_plan"] + hs["upload"] + loop_s + hs["final_arrays"] + hs["pack_results"]
        out["end_to_end"] = {"seconds": total, "frames_per_sec": frames_total / args.steps / total,
                             "note": "one call of eaQHMAnalysisAndSynthesis on this file: SWIPE' + VUV/plan + upload + "
                                     "adaptation loop + final arrays + struct packing (wav decoding excluded)"}
    if rehearsal:
        out["rehearsal"] = "all ranks on one GPU, collectives staged through the host: code-path check only"
    if args.full:
        out["cpu_baseline"] = (cpu_baseline(args.workload) if rank == 0 and world == 1 and not args.no_cpu_baseline
                               else None)
    sys.stdout.flush()
    os.dup2(real_stdout, 1)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
