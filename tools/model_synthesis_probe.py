"""Resynthesis from the model: device time of eaqhm_modify_prep (prep + scan) and eaqhm_modify_synth against
eaqhm_eval_synth on the same records, output samples per second, and unpack_model against pack_results on the host.

    python tools/model_synthesis_probe.py [--workloads synth16k_60s,synth48k_60s] [--reps 5] [--contours] [--formant]
                                          [--noise] [--noise-formant] [--noise-modulation] [--shape] [--formant-warp]
                                          [--cepstrum] [--align] [--build] [--noise-cepstrum] [--swipe] [--viterbi] [--onsets]
                                          [--out FILE]

Models: one analysis run of the 60 s synthetic workloads (female, maxAdpt=5 at 16 kHz, 1 at 48 kHz).  Settings: rho in
{0.5, 1, 2} x beta in {1, 1.25}.  --contours adds the contour path (eaqhm_modify_prep with gain and
eaqhm_modify_synth with the curve group): unit contours, rho a 0.5 Hz sinusoid 0.7-1.4 with beta = 1, rho = 1 with
beta ramping 0.85 -> 1.2, and both varying; eval_ms_per_msample normalises the eval time by the output length.
--formant adds the formant scale (eaqhm_modify_prep with alpha) at rho = 1: alpha in {0.85, 1.2} x
beta in {1, 1.25} on the scalar map, and alpha ramping 0.85 -> 1.2 on the contour map;
ratio_to_scalar compares each with the scalar path at the same beta (envelope on).  --noise adds the stochastic
component on the workload's own residual: eaqhm_noise_analyse, and eaqhm_noise_synth at rho in
{0.5, 1, 2} beside the deterministic prep + eval of the same session at the same rho (beta = 1); every time there is
the median of three windows of 20 launches, with the max - min of the three.  --noise-formant adds the formant warp of
the noise model on the same residual's model: eaqhm_noise_warp and eaqhm_noise_envelope (a 129-point
grid) at alpha in {0.85, 1.2} and a ramp between them, beside eaqhm_noise_synth of the warped model at rho = 1 in the
same session, with the same windows.  --noise-modulation adds the pitch-synchronous modulation of the noise (DESIGN.md
§10.2): eaqhm_noise_modulation (2 harmonics) next to eaqhm_noise_analyse, and eaqhm_noise_synth with the mod group next to
the plain one at rho in {0.5, 1, 2}, with the same windows.  --shape adds the shape-invariant phase
mode: eaqhm_modify_synth with the shape group next to without at rho in {0.5, 1, 2} x beta in {1, 1.25}
and on the four contour settings, each the median of three
windows of 20 launches with the max - min of the existing kernel's three (the margin).  --formant-warp adds the
piecewise-linear formant warp: eaqhm_modify_prep without the envelope + eaqhm_modify_amp_warp
next to eaqhm_modify_prep with alpha at the same beta, and eaqhm_noise_warp_map next to eaqhm_noise_warp on the
workload's residual, with the same windows and margin.  --cepstrum adds the discrete-cepstrum envelope (DESIGN.md
§9.5): eaqhm_model_cepstrum at the default order, and eaqhm_modify_prep without the envelope + eaqhm_modify_amp_cepstrum
next to eaqhm_modify_prep with the envelope at the same beta, with the same windows and margin.  --align adds the time
alignment: the model's cepstrum against a copy of itself stretched by warp_rows with a sinusoidal tempo
0.8-1.25, band 2 s: eaqhm_cepstrum_cost, and eaqhm_dtw's forward pass (with its launch count) and backtrack apart
(EAQHM_OPT_DTW_PHASES), each the median of three windows with their max - min, and the NumPy model's time for the same
band on a 5 s excerpt on the host.  --noise-cepstrum adds the noise model to and from cepstral rows on
the workload's residual model: eaqhm_noise_cepstrum (Q = 63) and eaqhm_noise_from_cepstrum next to eaqhm_noise_warp at
alpha = 1.2, with the same windows and the warp's max - min as the margin.  --mlpg times the delta rows and the
trajectory solve on random rows, once as one run and once as 200 runs, next to
scipy.linalg.solveh_banded on the host.  --gv times the global-variance ascent (eaqhm_gv_ascend, 30
sweeps) from the solve's trajectory on the same kind of rows, as one run and as 200, next to eaqhm_mlpg_solve in the same
session and to the same iteration in NumPy on the host's band, with the largest difference between the two results.
--cepstrum-warp times every entry point of the warped cepstrum (include/eaqhm_cepwarp.h) next to its
sibling on the linear axis, same session, same model, same rows' shapes, at the default order and at order 24 with
a = cepstrum_warp(fs): the ratio to the sibling with the sibling's max - min beside it.
--kmeans times the two steps of a Lloyd round of the k-means codebook (eaqhm_kmeans_assign and
eaqhm_kmeans_update) at N = 10^6 with (D, K) = (36, 8) and (100, 32) next to torch (cdist + argmin, index_add_) and to one
EM round (eaqhm_gmm_estep + eaqhm_gmm_mstep) at the same sizes, then the whole kmeans call with its rounds, and the mean
log-likelihood of gmm_fit after 20 rounds from the axis start and from the k-means start on a seeded clustered set.
--nn times the nearest-row search of the non-parallel training (eaqhm_nn_rows) on random rows at
nA = nB = 60 000 with D = 24 and 48 and at nA = 2 000, nB = 60 000 (the split path) next to torch (cdist + argmin) on the
same device, with the fraction of the FP64 matrix peak at 2 nA nB D flops.
--swipe times the device SWIPE'  on the 60 s synthetic signals of --workloads at the workloads' own plim
([160, 300]) and at [70, 500]: each of the three kernels per window size, the whole swipep_device call from a host array
to the host result as wall time with a cold and with a cached plan, and swipe.swipep in the same process (one run after
one warm-up), with the number of instants whose pitch differs.
--viterbi times the continuous pitch track on the same signals and limits: the forward pass (without and
with the unvoiced state, also per step in cycles), the backtrack and the refinement, and the whole swipep_viterbi call with
a cached plan next to swipep_device and to swipe.swipep in the same process.
--formant-tracks times the formant tracks on the all-pole models of the same signals
(formant.signal_allpole: 12 000 frames, p = 18 and 50): eaqhm_allpole_roots, eaqhm_formant_candidates, the forward pass
at N = 3 and 4 (also per step) and the backtrack, next to a numpy.roots loop over the same frames on the host.
--onsets times the transient onset detector on the same signals at its defaults: eaqhm_onset_bands (also
per frame), eaqhm_onset_flux and eaqhm_onset_peaks, and the whole onset_strength + onsets call as wall time.
EAQHM_LIB selects another build of
the library.  Device times are warmed HIP-event windows around synchronised launches; per-kernel
times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/model_synthesis_probe.py` run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def analyse(workload):
    import eaqhm_amd
    from eaqhm_amd.functions import pack_arrays, pack_results
    from eaqhm_amd.synth import synth_speech_int16
    from scipy.io import wavfile
    import tempfile
    fs, fix, key, adpt = {"synth16k_60s": (16000, "prep_fixtures.npz", "synth16k_60s_f0s_5ms", 5),
                          "synth48k_60s": (48000, "prep_synth48k_60s.npz", "synth48k_60s_f0s_5ms", 1)}[workload]
    grid = np.load(os.path.join(GOLDEN, fix))[key]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, workload + ".wav")
        x = synth_speech_int16(60.0, fs)
        wavfile.write(path, fs, x)
        s_recon, _, _, _, eng = eaqhm_amd.eaQHMAnalysisAndSynthesis(path, "female", maxAdpt=adpt, printPrompts=False,
                                                                    pitch_track=grid, _return_engine=True)
    fin = eng.final_arrays()
    t = time.perf_counter()
    det = pack_results(eng.plan, fin)
    t_pack = time.perf_counter() - t
    return fs, len(s_recon), det, pack_arrays(eng.plan, fin), t_pack, x / 32768.0 - s_recon


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def prepare(torch, det, fs, L, reps):
    """Device state of one model: records, codes and moments, the prep outputs, and the time of eaqhm_eval_synth on the
    same records (synthesis + SRER, no track output: what the analysis's last pass runs)."""
    from eaqhm_amd.functions import _ctx
    from eaqhm_amd.model import unpack_model
    t = time.perf_counter()
    m = unpack_model(det)
    t_unpack = time.perf_counter() - t
    c = _ctx(0)
    dev = c.device
    rec_h = m["records"]
    n, K, D = rec_h.shape[0], m["Kmax"], m["step"]
    rec = torch.as_tensor(rec_h, device=dev)
    code = torch.empty(n * K, dtype=torch.uint8, device=dev)
    mom = torch.empty(n * (K + 1), dtype=torch.float64, device=dev)
    amp, R, ph0 = (torch.empty(n * K, dtype=torch.float64, device=dev) for _ in range(3))
    c.spline_solve(rec, n, K, D, code, mom)
    target = torch.zeros(L, dtype=torch.float64, device=dev)
    s_hat = torch.empty(L, dtype=torch.float64, device=dev)
    ph_knot = torch.empty(n * K, dtype=torch.float64, device=dev)
    partials = torch.empty(c.eval_partials_len(0, L, D), dtype=torch.int64, device=dev)
    sums = torch.empty(16, dtype=torch.float64, device=dev)
    t_eval = timed(torch, lambda: c.eval_synth(rec, code, mom, n, K, D, fs, L, 0, L, 0, L, target, 1.0, None, None, 0, 0,
                                               ph_knot, s_hat, partials, sums), reps)
    return dict(c=c, rec=rec, code=code, mom=mom, amp=amp, R=R, ph0=ph0, n=n, K=K, D=D, fs=fs, L=L, t_eval=t_eval,
                t_unpack=t_unpack)


def probe(workload, reps, contours=False, formant=False, noise=False, shape=False, noise_formant=False,
          noise_modulation=False, formant_warp=False, cepstrum=False, align=False, build=False, noise_cepstrum=False,
          cepstrum_warp=False):
    import torch
    fs, L, det, arrays, t_pack, residual = analyse(workload)
    st = prepare(torch, det, fs, L, reps)
    c, rec, code, mom, amp, R, ph0 = (st[k] for k in ("c", "rec", "code", "mom", "amp", "R", "ph0"))
    n, K, D, t_eval, t_unpack = st["n"], st["K"], st["D"], st["t_eval"], st["t_unpack"]
    dev = c.device
    rows = []
    for beta in (1.0, 1.25):
        beta_d = torch.full((n,), beta, dtype=torch.float64, device=dev)
        t_prep = timed(torch, lambda: c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, None, True, amp, R, ph0),
                       reps)
        for rho in (0.5, 1.0, 2.0):
            Lo = int(np.rint(rho * L))
            out = torch.empty(Lo, dtype=torch.float64, device=dev)
            t_syn = timed(torch, lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, rho, beta, Lo, 0, Lo,
                                                        out), reps)
            rows.append(dict(rho=rho, beta=beta, prep_scan_ms=round(t_prep, 3), eval_ms=round(t_syn, 3),
                             total_ms=round(t_prep + t_syn, 3), out_samples=Lo,
                             eval_ms_per_msample=round(t_syn / (Lo / 1e6), 4),
                             msamples_per_s=round(Lo / ((t_prep + t_syn) * 1e-3) / 1e6, 1),
                             ratio_to_eval_synth=round((t_prep + t_syn) / t_eval, 3)))
    res = dict(workload=workload, fs=fs, L=L, No_ti=n, Kmax=K, eval_synth_ms=round(t_eval, 3),
               pack_results_s=round(t_pack, 3), unpack_model_s=round(t_unpack, 3), settings=rows)
    if contours:
        res["contours"] = probe_contours(torch, c, rec, code, mom, amp, R, ph0, n, K, D, fs, L, t_eval, reps)
    if formant:
        res["formant"] = formant_rows(torch, st, reps)
    if noise:
        res["noise"] = noise_rows(torch, st, residual)
    if shape:
        res["shape"] = shape_rows(torch, st)
    if noise_formant:
        import eaqhm_amd
        res["noise_formant"] = noise_formant_rows(torch, eaqhm_amd.eaQHMNoiseAnalysis(residual, np.zeros(L), fs))
    if noise_modulation:
        res["noise_modulation"] = noise_modulation_rows(torch, st, residual)
    if formant_warp:
        import eaqhm_amd
        res["formant_warp"] = formant_warp_rows(torch, st, eaqhm_amd.eaQHMNoiseAnalysis(residual, np.zeros(L), fs))
    if cepstrum:
        res["cepstrum"] = cepstrum_rows(torch, st)
    if align:
        res["align"] = align_rows(torch, st)
    if build:
        res["build"] = build_rows(torch, st)
    if noise_cepstrum:
        import eaqhm_amd
        res["noise_cepstrum"] = noise_cepstrum_rows(torch, eaqhm_amd.eaQHMNoiseAnalysis(residual, np.zeros(L), fs))
    if cepstrum_warp:
        import eaqhm_amd
        res["cepstrum_warp"] = cepwarp_rows(torch, st, eaqhm_amd.eaQHMNoiseAnalysis(residual, np.zeros(L), fs))
    return res


FP64_MATRIX_PEAK = 78.6e12   # MI355X, FLOP/s


def gmm_rows(torch, reps=20, runs=3, sizes=(65536, 1000000), shapes=((18, 18, 8), (50, 50, 32))):
    """One E-step, one M-step and one regression of the joint-density mixture on random rows, next to
    the same step written with torch matmuls on the same device (a comparison, not a bar).  Each time: median of `runs`
    warmed windows of `reps` launches, and max - min of the windows.  Fractions of the FP64 matrix peak: the E-step at
    its useful half N M D^2 (the lower triangle of W), the M-step at 2 N M D^2, the regression at 2 N M dx dy."""
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    rows = []
    for N in sizes:
        for dx, dy, M in shapes:
            D = dx + dy
            g = torch.Generator(device=dev).manual_seed(N + D + M)
            rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=g)   # noqa: E731
            Z = rnd(N, D)
            mu = rnd(M, D)
            W = torch.tril(0.1 * rnd(M, D, D), -1) + torch.eye(D, dtype=torch.float64, device=dev)
            k = torch.full((M,), -np.log(M) - 0.5 * D * np.log(2 * np.pi), dtype=torch.float64, device=dev)
            gamma = torch.empty((N, M), dtype=torch.float64, device=dev)
            ll = torch.empty(N, dtype=torch.float64, device=dev)
            work = torch.empty(c.gmm_work_len(N, D, M), dtype=torch.float64, device=dev)
            S0 = torch.empty(M, dtype=torch.float64, device=dev)
            S1 = torch.empty((M, D), dtype=torch.float64, device=dev)
            S2 = torch.empty((M, D, D), dtype=torch.float64, device=dev)
            A, b = rnd(M, dy, dx) / np.sqrt(dx), rnd(M, dy)
            X = Z[:, :dx].contiguous()
            Y = torch.empty((N, dy), dtype=torch.float64, device=dev)

            def t_estep():
                lp = torch.stack([k[m] - 0.5 * (((Z - mu[m]) @ W[m].T) ** 2).sum(dim=1) for m in range(M)], dim=1)
                l = torch.logsumexp(lp, dim=1)
                return torch.exp(lp - l[:, None]), l

            def t_mstep():
                return gamma.sum(dim=0), gamma.T @ Z, torch.stack([(Z * gamma[:, m:m + 1]).T @ Z for m in range(M)])

            def t_regress():
                T = (X @ A.reshape(M * dy, dx).T).reshape(N, M, dy) + b[None]
                return (gamma[:, :, None] * T).sum(dim=1)

            e = med(lambda: c.gmm_estep(Z, N, D, M, mu, W, k, gamma, ll))
            m_ = med(lambda: c.gmm_mstep(Z, gamma, N, D, M, work, S0, S1, S2))
            r = med(lambda: c.gmm_regress(X, gamma, A, b, N, dx, dy, M, Y))
            te, tm, tr = med(t_estep), med(t_mstep), med(t_regress)
            frac = lambda flops, ms: round(flops / (ms * 1e-3) / FP64_MATRIX_PEAK, 4)   # noqa: E731
            rows.append(dict(N=N, dx=dx, dy=dy, M=M,
                             estep_ms=e[0], estep_spread_ms=e[1], estep_torch_ms=te[0], estep_torch_spread_ms=te[1],
                             estep_peak_fraction=frac(float(N) * M * D * D, e[0]),
                             mstep_ms=m_[0], mstep_spread_ms=m_[1], mstep_torch_ms=tm[0], mstep_torch_spread_ms=tm[1],
                             mstep_peak_fraction=frac(2.0 * N * M * D * D, m_[0]),
                             regress_ms=r[0], regress_spread_ms=r[1], regress_torch_ms=tr[0],
                             regress_torch_spread_ms=tr[1], regress_peak_fraction=frac(2.0 * N * M * dx * dy, r[0])))
            print(json.dumps(rows[-1]), flush=True)
            del Z, gamma, work, X, Y
            torch.cuda.empty_cache()
    return rows


def kmeans_clustered(N, D, K, seed):
    """Seeded rows float64[N, D] around K centres 4 standard deviations of the noise apart on average, shuffled."""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((K, D)) / np.sqrt(2.0)
    return centres[rng.integers(0, K, size=N)] + rng.standard_normal((N, D))


def kmeans_rows(torch, reps=20, runs=3, N=1000000, shapes=((36, 8), (100, 32))):
    """One assignment and one update of the k-means codebook on seeded clustered rows, next to torch on
    the same device (cdist + argmin; index_add_, one warmed call: a comparison, not a bar) and to one EM round of the mixture
    (eaqhm_gmm_estep + eaqhm_gmm_mstep, M = K) at the same sizes.  Each time: median of `runs` warmed windows of `reps`
    launches, and max - min of the windows.  The update is timed on the labels of the assignment (shuffled rows: the
    running cluster changes at almost every row) and on sorted labels (it never changes inside a chunk).  Then the whole
    kmeans call from host rows, once warmed, with its Lloyd rounds; and gmm_fit after 20 rounds (tol = 0) from both
    starts on a clustered set of 20 000 x 16, 8 components."""
    import eaqhm_amd
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    rows = []
    for D, K in shapes:
        Zh = kmeans_clustered(N, D, K, 1000 + D)
        Z = torch.as_tensor(Zh - Zh.mean(axis=0), device=dev)
        C = Z[:: N // K][:K].contiguous()
        g = (C * C).sum(dim=1)
        labels = torch.zeros(N, dtype=torch.int32, device=dev)
        changed = torch.empty(-(-N // 64), dtype=torch.int32, device=dev)
        work = torch.empty(c.kmeans_work_len(N, D, K), dtype=torch.float64, device=dev)
        count = torch.empty(K, dtype=torch.int64, device=dev)
        S1 = torch.empty((K, D), dtype=torch.float64, device=dev)
        Q = torch.empty((K, D), dtype=torch.float64, device=dev)
        a = med(lambda: c.kmeans_assign(Z, N, D, D, C, g, K, labels, changed))
        u = med(lambda: c.kmeans_update(Z, N, D, D, labels, K, work, count, S1, Q))
        sorted_labels = torch.sort(labels)[0].contiguous()
        us = med(lambda: c.kmeans_update(Z, N, D, D, sorted_labels, K, work, count, S1, Q))
        ll = labels.long()

        def t_update():
            return (torch.bincount(ll, minlength=K), torch.zeros_like(S1).index_add_(0, ll, Z),
                    torch.zeros_like(Q).index_add_(0, ll, Z * Z))

        ta = med(lambda: torch.cdist(Z, C).argmin(dim=1))
        tu = (round(timed(torch, t_update, 1), 1), None)    # one warmed call: float64 index_add_ onto K rows takes seconds
        mu = C.clone()
        W = torch.eye(D, dtype=torch.float64, device=dev).repeat(K, 1, 1)
        kk = torch.full((K,), -np.log(K) - 0.5 * D * np.log(2 * np.pi), dtype=torch.float64, device=dev)
        gamma = torch.empty((N, K), dtype=torch.float64, device=dev)
        lln = torch.empty(N, dtype=torch.float64, device=dev)
        gwork = torch.empty(c.gmm_work_len(N, D, K), dtype=torch.float64, device=dev)
        S0, S2 = torch.empty(K, dtype=torch.float64, device=dev), torch.empty((K, D, D), dtype=torch.float64, device=dev)
        e = med(lambda: c.gmm_estep(Z, N, D, K, mu, W, kk, gamma, lln))
        m_ = med(lambda: c.gmm_mstep(Z, gamma, N, D, K, gwork, S0, S1, S2))
        del gamma, gwork, work, Z
        torch.cuda.empty_cache()
        whole = []
        for _ in range(2):                              # the second call is the warmed one
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eaqhm_amd.kmeans(Zh, K)
            whole.append(round((time.perf_counter() - t0) * 1e3, 1))
        rows.append(dict(N=N, D=D, K=K, assign_ms=a[0], assign_spread_ms=a[1], assign_torch_ms=ta[0],
                         assign_torch_spread_ms=ta[1], update_ms=u[0], update_spread_ms=u[1], update_sorted_ms=us[0],
                         update_sorted_spread_ms=us[1], update_torch_ms=tu[0], update_torch_spread_ms=tu[1],
                         estep_ms=e[0], estep_spread_ms=e[1], mstep_ms=m_[0], mstep_spread_ms=m_[1],
                         assign_gb_per_s=round(N * D * 8 / (a[0] * 1e-3) / 1e9, 1),
                         update_gb_per_s=round(N * D * 8 / (u[0] * 1e-3) / 1e9, 1),
                         kmeans_call_ms=whole, kmeans_rounds=int(out["rounds"]),
                         kmeans_smallest_cluster=int(out["counts"].min())))
        print(json.dumps(rows[-1]), flush=True)
        del Zh
    Zq = kmeans_clustered(20000, 16, 8, 77)
    fits = {}
    for name, init in (("axis", None), ("kmeans", "kmeans")):
        try:
            fits[name] = float(eaqhm_amd.gmm_fit(Zq, 8, iters=20, tol=0.0, init=init)["loglik"][-1])
        except np.linalg.LinAlgError as err:
            fits[name] = str(err)
    rows.append(dict(quality_set="kmeans_clustered(20000, 16, 8, seed 77)", rounds=20, mean_loglik=fits))
    print(json.dumps(rows[-1]), flush=True)
    return rows


def nn_rows(torch, reps=20, runs=3, shapes=((60000, 60000, 24), (60000, 60000, 48), (2000, 60000, 24))):
    """eaqhm_nn_rows (the norms, the search and the merge together) on seeded normal rows, next to torch on
    the same device (cdist + argmin, windows of 5: a comparison, not a bar).  Each time: median of `runs` warmed windows of
    `reps` launches, and max - min of the windows; the fraction of the FP64 matrix peak counts 2 nA nB D flops."""
    from eaqhm_amd import nonparallel
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    dev = c.device

    def med(fn, n=reps):
        ts = sorted(timed(torch, fn, n) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    rows = []
    for nA, nB, D in shapes:
        rng = np.random.default_rng(nA + nB + D)
        A = torch.as_tensor(rng.standard_normal((nA, D)), device=dev)
        B = torch.as_tensor(rng.standard_normal((nB, D)), device=dev)
        work = torch.empty(c.nn_work_len(nA, nB, D), dtype=torch.float64, device=dev)
        index = torch.empty(nA, dtype=torch.int64, device=dev)
        dist2 = torch.empty(nA, dtype=torch.float64, device=dev)
        t = med(lambda: c.nn_rows(A, nA, D, B, nB, D, D, work, index, dist2))
        tt = med(lambda: torch.cdist(A, B).argmin(dim=1), 5)
        same = float((torch.cdist(A, B).argmin(dim=1) == index).double().mean().item())
        rows.append(dict(nA=nA, nB=nB, D=D, splits=nonparallel.nn_splits(nA, nB), nn_rows_ms=t[0], nn_rows_spread_ms=t[1],
                         peak_fraction=round(2.0 * nA * nB * D / (t[0] * 1e-3) / FP64_MATRIX_PEAK, 4),
                         torch_cdist_argmin_ms=tt[0], torch_spread_ms=tt[1], same_index_as_torch=same))
    return rows


def swipe_rows(torch, workloads, reps=20, runs=3):
    """The device SWIPE'  on the 60 s synthetic signals: per kernel and window size the median of `runs`
    warmed HIP-event windows of `reps` launches with their max - min; the whole pitch.swipep_device call (host array in,
    host track out) as wall time, cold (no plan, no device copy of it) and with the plan cached (median of five); and
    swipe.swipep on this host in this process, one run after one warm-up."""
    from eaqhm_amd import pitch
    from eaqhm_amd.functions import _ctx
    from eaqhm_amd.swipe import swipep
    from eaqhm_amd.synth import synth_speech_int16
    c = _ctx(0)
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - t0

    rows = []
    for wl in workloads:
        fs = {"synth16k_60s": 16000, "synth48k_60s": 48000}[wl]
        x = synth_speech_int16(60.0, fs) / 32768.0
        for plim in ((160, 300), (70, 500)):
            for cache in (pitch._PLANS, pitch._KERNELS, pitch._DEVICE_PLANS):
                cache.clear()
            got, cold = wall(lambda: pitch.swipep_device(x, fs, plim))
            cached = sorted(wall(lambda: pitch.swipep_device(x, fs, plim))[1] for _ in range(5))
            _, t_plan = wall(lambda: (pitch._PLANS.clear(), pitch._KERNELS.clear(), pitch.swipe_plan(len(x), fs, plim)))
            swipep(x, fs, list(plim))
            ref, host = wall(lambda: swipep(x, fs, list(plim)))
            plan = pitch.swipe_plan(len(x), float(fs), plim)
            on = pitch._device_plan(plan, torch, dev)
            x_d = torch.as_tensor(x, device=dev)
            nE, T, npc = len(plan["fERBs"]), len(plan["t"]), len(plan["pc"])
            kernels, wins = [], []
            for w, w_d in zip(plan["windows"], on["windows"]):
                L = torch.empty((w["nframes"], nE), dtype=torch.float64, device=dev)
                Si = torch.empty((w["ncand"], w["nframes"]), dtype=torch.float64, device=dev)
                tl = med(lambda: c.swipe_loudness(x_d, len(x), w["w"], w["hop"], w["pad"], w["nframes"], w_d["window"], fs,
                                                  w["sumw2"], w_d["lo"], w_d["xlo"], w_d["df"], nE, L, nE))
                tsc = med(lambda: c.swipe_scores(w_d["K"], w["ncand"], nE, L, w["nframes"], nE, nE, Si))
                kernels.append(dict(w=w["w"], nframes=w["nframes"], ncand=w["ncand"], loudness_ms=tl[0],
                                    loudness_spread_ms=tl[1], scores_ms=tsc[0], scores_spread_ms=tsc[1]))
                wins.append((Si, w["j0"], w["ncand"], w["nframes"], w_d["mu"], w_d["tshift"]))
            ps = torch.empty((2, T), dtype=torch.float64, device=dev)
            tp = med(lambda: c.swipe_pick(wins, on["t"], T, npc, plan["pc"][0], on["ntc"], on["nftc"], on["ptab"], on["nf"],
                                          plan["nfmax"], ps[0], ps[1], None))
            rows.append(dict(workload=wl, plim=list(plim), samples=len(x), instants=T, candidates=npc, erb_points=nE,
                             kernels=kernels, pick_ms=tp[0], pick_spread_ms=tp[1],
                             device_call_cold_s=round(cold, 4), device_call_cached_s=round(cached[2], 4),
                             device_call_cached_min_max_s=[round(cached[0], 4), round(cached[-1], 4)],
                             host_plan_s=round(t_plan, 4), host_swipep_s=round(host, 4),
                             host_over_device_cached=round(host / cached[2], 2),
                             pitch_differs=int((got[:, 1] != ref[:, 1]).sum()),
                             strength_max_abs_diff=float(np.abs(got[:, 2] - ref[:, 2]).max())))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def viterbi_rows(torch, workloads, reps=20, runs=3):
    """The continuous pitch track on the 60 s synthetic signals at [160, 300] and [70, 500]: the forward
    pass, the backtrack (both launches) and the refinement as the median of `runs` warmed HIP-event windows of `reps`
    launches with their max - min, without and with the unvoiced state; the forward pass per step in ns and in cycles of
    the device's clock; the whole pitch.swipep_viterbi call (host array in, host track out) with the plan cached (median
    of five) next to pitch.swipep_device and to swipe.swipep on this host in the same process (one run after one
    warm-up); and what the path changes: steps of more than 8 candidates, raw and along the path."""
    from eaqhm_amd import pitch
    from eaqhm_amd.functions import _ctx
    from eaqhm_amd.swipe import swipep
    from eaqhm_amd.synth import synth_speech_int16
    c = _ctx(0)
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - t0

    rows = []
    for wl in workloads:
        fs = {"synth16k_60s": 16000, "synth48k_60s": 48000}[wl]
        x = synth_speech_int16(60.0, fs) / 32768.0
        for plim in ((160, 300), (70, 500)):
            pitch.swipep_viterbi(x, fs, plim)                                   # the plan, its device copy, the code objects
            got, _ = wall(lambda: pitch.swipep_viterbi(x, fs, plim, return_path=True))
            cached = sorted(wall(lambda: pitch.swipep_viterbi(x, fs, plim))[1] for _ in range(5))
            cached_uv = sorted(wall(lambda: pitch.swipep_viterbi(x, fs, plim, unvoiced=0.2))[1] for _ in range(5))
            device = sorted(wall(lambda: pitch.swipep_device(x, fs, plim))[1] for _ in range(5))
            swipep(x, fs, list(plim))
            ref, host = wall(lambda: swipep(x, fs, list(plim)))
            plan = pitch.swipe_plan(len(x), float(fs), plim)
            on, S = pitch._strengths_on_device(x, plan, torch, dev=dev, c=c)
            T, npc = len(plan["t"]), len(plan["pc"])
            cost = pitch.viterbi_costs(npc)
            cost_d = torch.as_tensor(cost, device=dev)
            ntiles = -(-T // pitch.VITERBI_TILE)
            bp = torch.empty((T, npc + 1), dtype=torch.int16, device=dev)
            tm = torch.empty((ntiles, npc + 1), dtype=torch.int16, device=dev)
            last = torch.empty(npc + 1, dtype=torch.float64, device=dev)
            q = torch.empty(T, dtype=torch.int32, device=dev)
            ps = torch.empty((2, T), dtype=torch.float64, device=dev)
            pc_d = torch.as_tensor(np.ascontiguousarray(plan["pc"]), device=dev)
            W = len(cost) - 1
            tf = med(lambda: c.viterbi_forward(S, npc, T, cost_d, W, None, bp, tm, last))
            tfu = med(lambda: c.viterbi_forward(S, npc, T, cost_d, W, (0.2, 1.0), bp, tm, last))
            tb = med(lambda: c.viterbi_backtrack(bp, tm, last, npc, T, q))
            tr = med(lambda: c.viterbi_refine(S, q, npc, T, pc_d, on["ntc"], on["nftc"], on["ptab"], on["nf"],
                                              plan["nfmax"], ps[0], ps[1]))
            raw = S.argmax(dim=0).cpu().numpy()
            path = got[1]
            big = lambda v: int((np.abs(np.diff(v.astype(np.int64))) > 8).sum())  # noqa: E731
            rows.append(dict(workload=wl, plim=list(plim), instants=T, candidates=npc, W=W, clock_khz=c.clock_khz,
                             forward_ms=tf[0], forward_spread_ms=tf[1], forward_unvoiced_ms=tfu[0],
                             forward_unvoiced_spread_ms=tfu[1], backtrack_ms=tb[0], backtrack_spread_ms=tb[1],
                             refine_ms=tr[0], refine_spread_ms=tr[1],
                             forward_ns_per_step=round(tf[0] * 1e6 / T, 1),
                             forward_cycles_per_step=round(tf[0] * 1e-3 / T * c.clock_khz * 1e3, 0),
                             forward_unvoiced_cycles_per_step=round(tfu[0] * 1e-3 / T * c.clock_khz * 1e3, 0),
                             viterbi_call_cached_s=round(cached[2], 4),
                             viterbi_call_cached_min_max_s=[round(cached[0], 4), round(cached[-1], 4)],
                             viterbi_unvoiced_call_cached_s=round(cached_uv[2], 4),
                             device_call_cached_s=round(device[2], 4), host_swipep_s=round(host, 4),
                             host_over_viterbi_cached=round(host / cached[2], 2),
                             big_steps_raw=big(raw), big_steps_path=big(path),
                             pitch_differs_from_swipep=int((got[0][:, 1] != ref[:, 1]).sum())))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def formant_track_rows(torch, workloads, reps=20, runs=3):
    """Formant tracks on the all-pole models of the 60 s synthetic signals (formant.signal_allpole at the
    noise model's defaults: 12 000 frames, p = 18 at 16 kHz and 50 at 48 kHz): eaqhm_allpole_roots,
    eaqhm_formant_candidates, eaqhm_formant_forward (N = 3 and 4) and eaqhm_formant_backtrack as the median of `runs`
    warmed HIP-event windows of `reps` launches with their max - min; the forward pass per step in ns; the steps the
    iteration took; and a numpy.roots loop over the same frames on this host, one run."""
    from eaqhm_amd import formant
    from eaqhm_amd.functions import _ctx
    from eaqhm_amd.synth import synth_speech_int16
    c = _ctx(0)
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    rows = []
    for wl in workloads:
        fs = {"synth16k_60s": 16000, "synth48k_60s": 48000}[wl]
        x = synth_speech_int16(60.0, fs) / 32768.0
        model = formant.signal_allpole(x, fs)
        Nf, p = model["refl"].shape
        refl = torch.as_tensor(model["refl"], device=dev)
        roots = torch.empty((Nf, p, 2), dtype=torch.float64, device=dev)
        iters = torch.empty(Nf, dtype=torch.int32, device=dev)
        f = torch.empty((Nf, 8), dtype=torch.float64, device=dev)
        b = torch.empty((Nf, 8), dtype=torch.float64, device=dev)
        count = torch.empty(Nf, dtype=torch.int32, device=dev)
        tr = med(lambda: c.allpole_roots(refl, Nf, p, roots, iters))
        tc = med(lambda: c.formant_candidates(roots, iters, Nf, p, fs, 50.0, min(5500.0, fs / 2), 1000.0, f, b, count))
        it = iters.cpu().numpy()
        cand = dict(f=f.cpu().numpy(), b=b.cpu().numpy(), count=count.cpu().numpy())
        row = dict(workload=wl, frames=Nf, order=p, roots_ms=tr[0], roots_spread_ms=tr[1], candidates_ms=tc[0],
                   candidates_spread_ms=tc[1], steps_mean=round(float(it.mean()), 2), steps_max=int(it.max()),
                   unfinished=int((it == formant.FORMANT_ITMAX + 1).sum()),
                   candidates_mean=round(float(cand["count"].mean()), 2))
        for N in (3, 4):
            L, lf = formant.formant_cost_tables(cand, N, (550, 1650, 2750, 3850))
            st = formant.formant_states(N)
            L_d, lf_d, st_d = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (L, lf, np.array(st)))
            bp = torch.empty((Nf, len(st)), dtype=torch.int16, device=dev)
            last = torch.empty(len(st), dtype=torch.float64, device=dev)
            q = torch.empty(Nf, dtype=torch.int32, device=dev)
            total = torch.empty(1, dtype=torch.float64, device=dev)
            tf = med(lambda: c.formant_forward(L_d, lf_d, count, st_d, N, Nf, 1.0, 2.0, bp, last))
            tb = med(lambda: c.formant_backtrack(bp, last, N, Nf, q, total))
            row.update({"forward_N%d_ms" % N: tf[0], "forward_N%d_spread_ms" % N: tf[1],
                        "forward_N%d_ns_per_step" % N: round(tf[0] * 1e6 / Nf, 1),
                        "backtrack_N%d_ms" % N: tb[0], "backtrack_N%d_spread_ms" % N: tb[1]})
        t0 = time.perf_counter()
        for k in model["refl"]:
            a = np.array([1.0])
            for ki in k:
                a = np.concatenate((a, [0.0])) + ki * np.concatenate(([0.0], a[::-1]))
            np.roots(a)
        row["host_numpy_roots_s"] = round(time.perf_counter() - t0, 3)
        row["host_over_device_roots"] = round(row["host_numpy_roots_s"] * 1e3 / tr[0], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def onset_rows(torch, workloads, reps=20, runs=3):
    """The transient onset detector on the 60 s synthetic signals at its defaults (12 000 frames; window
    256 at 16 kHz, 512 at 48 kHz; 24 bands): eaqhm_onset_bands, eaqhm_onset_flux and eaqhm_onset_peaks as the median of
    `runs` warmed HIP-event windows of `reps` launches with their max - min; the bands kernel per frame in ns; and the
    whole onset_strength + onsets call (host array in, host result out) as wall time, the median of five."""
    from eaqhm_amd import transient
    from eaqhm_amd.functions import _ctx
    from eaqhm_amd.synth import synth_speech_int16
    c = _ctx(0)
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    rows = []
    for wl in workloads:
        fs = {"synth16k_60s": 16000, "synth48k_60s": 48000}[wl]
        s = synth_speech_int16(60.0, fs) / 32768.0
        x, fs_, hop, win, k, lag, floor = transient.check_onset_arguments(s, fs)
        n, w, B = len(x), len(win), len(k) - 1
        Nf = (n - 1) // hop + 1
        lo, hi = transient.whole_frames(n, hop, w)
        x_d, win_d = torch.as_tensor(x, device=dev), torch.as_tensor(win, device=dev)
        L = torch.empty((Nf, B), dtype=torch.float64, device=dev)
        d = torch.empty(Nf, dtype=torch.float64, device=dev)
        flag = torch.empty(Nf, dtype=torch.uint8, device=dev)
        inv = 1.0 / float(win.sum()) ** 2
        tb = med(lambda: c.onset_bands(x_d, n, w, hop, Nf, win_d, inv, k, B, floor, L, B))
        tf = med(lambda: c.onset_flux(L, Nf, B, B, lag, lo, hi, d))
        tp = med(lambda: c.onset_peaks(d, Nf, 3, 3, 20, 6, 0.5, flag))
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            on = transient.onsets(transient.onset_strength(s, fs))
            walls.append(time.perf_counter() - t0)
        row = dict(workload=wl, frames=Nf, window=w, hop=hop, bands=B, bands_ms=tb[0], bands_spread_ms=tb[1],
                   bands_ns_per_frame=round(tb[0] * 1e6 / Nf, 1), flux_ms=tf[0], flux_spread_ms=tf[1], peaks_ms=tp[0],
                   peaks_spread_ms=tp[1], whole_call_ms=round(sorted(walls)[2] * 1e3, 3), onsets=len(on["frames"]),
                   flagged=int(flag.sum().item()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def host_band(P, r, span):
    """(ab [2 span + 1, T, dy], q [T, dy]): the lower band of R = diag(P^s) + W^T diag(P^D) W in solveh_banded's layout
    (ab[k, i] = R[i + k, i]) and q = r^s + W^T r^D for one run of T rows, every column at once.  NumPy on the host."""
    T, dy = P.shape[0], P.shape[1] // 2
    L, u = span, np.arange(T)
    w = np.arange(1, L + 1) / (2.0 * sum(k * k for k in range(1, L + 1)))
    A = np.zeros((T, 2 * L + 1))                         # A[u, c - u + L] = W[u, c]
    for tau in range(1, L + 1):
        np.add.at(A, (u, np.minimum(u + tau, T - 1) - u + L), w[tau - 1])
        np.add.at(A, (u, np.maximum(u - tau, 0) - u + L), -w[tau - 1])
    ab = np.zeros((2 * L + 1, T, dy))
    ab[0] = P[:, :dy]
    q = r[:, :dy].copy()
    for e in range(2 * L + 1):                           # row u of W touches column i = u + e - L
        i = u + e - L
        ok = (i >= 0) & (i < T)
        q[i[ok]] += A[ok, e, None] * r[ok, dy:]
        for f in range(e, 2 * L + 1):                    # ... and column i + k, k = f - e
            ok2 = ok & (i + f - e < T)
            np.add.at(ab[f - e], i[ok2], (A[ok2, e] * A[ok2, f])[:, None] * P[ok2, dy:])
    return ab, q


def mlpg_rows(torch, n=60000, dys=24, span=2, reps=5, runs=3):
    """eaqhm_ceps_delta on n rows of dys + 1 columns and eaqhm_mlpg_solve on n rows of dys static columns (DESIGN.md
    §12.1), once with all rows in one run and once cut into 200 equal runs.  Each time: median of `runs` warmed windows of
    `reps` launches, and max - min of the windows.  Beside them scipy.linalg.solveh_banded on the host for the same dys
    systems per run, from the band the host forms with NumPy (forming not timed): a comparison, not a bar."""
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    g = torch.Generator(device=dev).manual_seed(n + dys + span)
    C = torch.randn(n, dys + 1, dtype=torch.float64, device=dev, generator=g)
    D = torch.empty_like(C)
    P = torch.exp(torch.randn(n, 2 * dys, dtype=torch.float64, device=dev, generator=g))
    P[:, dys:] *= 100.0
    r = torch.randn(n, 2 * dys, dtype=torch.float64, device=dev, generator=g) * P
    work = torch.empty(c.mlpg_work_len(n, dys, span), dtype=torch.float64, device=dev)
    Y = torch.empty((n, dys), dtype=torch.float64, device=dev)
    d = med(lambda: c.ceps_delta(C, n, dys + 1, span, D))
    rows = []
    for n_runs in (1, 200):
        T = n // n_runs
        start = torch.arange(n_runs, dtype=torch.int64, device=dev) * T
        length = torch.full((n_runs,), T, dtype=torch.int64, device=dev)
        t = med(lambda: c.mlpg_solve(P, r, n, dys, span, start, length, n_runs, work, Y))
        row = dict(n=n, dys=dys, span=span, n_runs=n_runs, delta_ms=d[0], delta_spread_ms=d[1], solve_ms=t[0],
                   solve_spread_ms=t[1])
        try:
            from scipy.linalg import solveh_banded
            Ph, rh = P.cpu().numpy(), r.cpu().numpy()
            bands = []
            for k in range(n_runs):                      # one contiguous band and right-hand side per system
                ab, q = host_band(Ph[k * T:(k + 1) * T], rh[k * T:(k + 1) * T], span)
                bands.append((np.ascontiguousarray(ab.transpose(2, 0, 1)), np.ascontiguousarray(q.T)))
            t0 = time.perf_counter()
            for ab, q in bands:
                for j in range(dys):
                    solveh_banded(ab[j], q[j], lower=True)
            row["host_solveh_banded_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        except ImportError:
            row["host_solveh_banded_ms"] = None
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def mlpg_em_rows(torch, n=60000, dxs=24, dys=24, span=2, components=(8, 32), reps=20, runs=3):
    """eaqhm_mlpg_estep on n rows of 2 dxs source and dys static target columns, all rows in one run and
    cut into 200 equal runs, for each number of components.  Beside it, on the same rows in the same session, its two
    siblings eaqhm_gmm_estep (the marginal E-step on the 2 dxs source columns) and eaqhm_gmm_regress (2 dys columns), and
    one whole refinement iteration: the E-step, P = gamma @ py, the regression and eaqhm_mlpg_solve.  Each time: median of
    `runs` warmed windows of `reps` launches, and max - min of the windows.  The siblings are the comparison, not a bar."""
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    dev = c.device
    dx, dy = 2 * dxs, 2 * dys

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    rows = []
    for M in components:
        g = torch.Generator(device=dev).manual_seed(n + dx + dys + M)
        rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=g)   # noqa: E731
        X, Y = rnd(n, dx), rnd(n, dys)
        prior = torch.softmax(rnd(n, M), dim=1)
        A, bq = rnd(M, dy, dx) * (0.5 / np.sqrt(dx)), 0.5 * rnd(M, dy)
        py = torch.exp(0.5 * rnd(M, dy))
        kc = 0.5 * torch.log(py).sum(dim=1) - dys * np.log(2 * np.pi)
        pyA, pyb = (py[:, :, None] * A).contiguous(), (py * bq).contiguous()
        mu = rnd(M, dx)
        W = torch.tril(0.1 * rnd(M, dx, dx), -1) + torch.eye(dx, dtype=torch.float64, device=dev)
        kx = torch.full((M,), -np.log(M) - 0.5 * dx * np.log(2 * np.pi), dtype=torch.float64, device=dev)
        gamma = torch.empty((n, M), dtype=torch.float64, device=dev)
        g0 = torch.empty((n, M), dtype=torch.float64, device=dev)
        ll = torch.empty(n, dtype=torch.float64, device=dev)
        r = torch.empty((n, dy), dtype=torch.float64, device=dev)
        work = torch.empty(c.mlpg_work_len(n, dys, span), dtype=torch.float64, device=dev)
        marginal = med(lambda: c.gmm_estep(X, n, dx, M, mu, W, kx, g0, ll))
        for n_runs in (1, 200):
            T = n // n_runs
            start = torch.arange(n_runs, dtype=torch.int64, device=dev) * T
            length = torch.full((n_runs,), T, dtype=torch.int64, device=dev)

            def estep():
                c.mlpg_estep(X, prior, A, bq, py, kc, Y, n, dx, dys, M, span, start, length, n_runs, gamma, ll)

            def iteration():
                estep()
                P = (gamma @ py).contiguous()
                c.gmm_regress(X, gamma, pyA, pyb, n, dx, dy, M, r)
                c.mlpg_solve(P, r, n, dys, span, start, length, n_runs, work, Y)
            e = med(estep)
            reg = med(lambda: c.gmm_regress(X, gamma, pyA, pyb, n, dx, dy, M, r))
            Y0 = Y.clone()
            it = med(iteration)
            Y.copy_(Y0)
            flops = 2.0 * n * M * dx * dy
            rows.append(dict(n=n, dx=dx, dys=dys, span=span, M=M, n_runs=n_runs, estep_ms=e[0], estep_spread_ms=e[1],
                             estep_peak_fraction=round(flops / (e[0] * 1e-3) / FP64_MATRIX_PEAK, 4),
                             gmm_estep_ms=marginal[0], gmm_estep_spread_ms=marginal[1], gmm_regress_ms=reg[0],
                             gmm_regress_spread_ms=reg[1], iteration_ms=it[0], iteration_spread_ms=it[1]))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def host_gv(bands, n, span, mean, prec, iters, y):
    """The ascent of DESIGN.md §12.2 in NumPy on the host's bands [(start, ab [2 span + 1, T, dy], q [T, dy])], every
    column at once; y float64[n, dy] is y_ML, every row in a run."""
    q = np.vstack([b[2] for b in bands])
    diag = np.vstack([b[1][0] for b in bands])
    omega = 1.0 / (2 * n)

    def Ry(y):
        out = np.empty_like(y)
        for s, ab, _ in bands:
            T = ab.shape[1]
            v, o = y[s:s + T], out[s:s + T]
            o[:] = ab[0] * v
            for k in range(1, min(2 * span, T - 1) + 1):
                o[k:] += ab[k, :T - k] * v[:-k]
                o[:-k] += ab[k, :T - k] * v[k:]
        return out
    m = y.mean(axis=0)
    v = ((y - m) ** 2).mean(axis=0)
    y = m + np.sqrt(mean / v) * (y - m)
    for _ in range(iters):
        m = y.mean(axis=0)
        v = ((y - m) ** 2).mean(axis=0)
        g = omega * (q - Ry(y)) - prec * (v - mean) * (2.0 / n) * (y - m)
        h = (4 * span + 1) * omega * diag + prec * (2.0 / n) * (np.abs(v - mean) + 2 * v)
        y = y + g / h
    return y


def gv_rows(torch, n=60000, dys=24, span=2, iters=30, reps=20, runs=3):
    """eaqhm_gv_ascend (`iters` sweeps, no trace) on n rows of dys static columns from eaqhm_mlpg_solve's trajectory
    (DESIGN.md §12.2), once with all rows in one run and once cut into 200 equal runs: median of `runs` warmed windows of
    `reps` calls and max - min of the windows (each call starts from a fresh copy of y_ML; the copy is timed apart and
    taken off).  Beside it eaqhm_mlpg_solve on the same rows in the same session, and the same iteration in NumPy on the
    band the host forms (forming not timed), with the largest difference between the two results: comparisons, not bars."""
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return ts[len(ts) // 2], ts[-1] - ts[0]

    g = torch.Generator(device=dev).manual_seed(n + dys + span)
    P = torch.exp(torch.randn(n, 2 * dys, dtype=torch.float64, device=dev, generator=g))
    P[:, dys:] *= 100.0
    r = torch.randn(n, 2 * dys, dtype=torch.float64, device=dev, generator=g) * P
    work = torch.empty(c.mlpg_work_len(n, dys, span), dtype=torch.float64, device=dev)
    gwork = torch.empty(c.gv_work_len(n, dys, span), dtype=torch.float64, device=dev)
    Yml = torch.empty((n, dys), dtype=torch.float64, device=dev)
    Y = torch.empty_like(Yml)
    rows = []
    for n_runs in (1, 200):
        T = n // n_runs
        start = torch.arange(n_runs, dtype=torch.int64, device=dev) * T
        length = torch.full((n_runs,), T, dtype=torch.int64, device=dev)
        solve = med(lambda: c.mlpg_solve(P, r, n, dys, span, start, length, n_runs, work, Yml))
        mean = 2.0 * Yml.var(dim=0, unbiased=False)              # twice the trajectory's own variance, spread 0.15
        prec = 1.0 / (0.15 * mean) ** 2

        def ascend():
            Y.copy_(Yml)
            c.gv_ascend(P, r, n, dys, span, start, length, n_runs, mean, prec, iters, gwork, Y, None)
        copy = med(lambda: Y.copy_(Yml))
        t = med(ascend)
        row = dict(n=n, dys=dys, span=span, iters=iters, n_runs=n_runs, launches=2 * iters + 4 + (iters + 1) % 2,   # without a trace: the copy home only after an even number of sweeps
                   
                   ascend_ms=round(t[0] - copy[0], 4), ascend_spread_ms=round(t[1], 4), copy_ms=round(copy[0], 4),
                   solve_ms=round(solve[0], 4), solve_spread_ms=round(solve[1], 4))
        Ph, rh = P.cpu().numpy(), r.cpu().numpy()
        bands = [(k * T,) + host_band(Ph[k * T:(k + 1) * T], rh[k * T:(k + 1) * T], span) for k in range(n_runs)]
        # host_band's ab[k, i] = R[i + k, i]: what host_gv reads as ab[k, :T - k]
        t0 = time.perf_counter()
        ref = host_gv(bands, n, span, mean.cpu().numpy(), prec.cpu().numpy(), iters, Yml.cpu().numpy())
        row["host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        row["max_abs_difference_from_host"] = float(np.abs(Y.cpu().numpy() - ref).max())
        row["max_abs_result"] = float(np.abs(ref).max())
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def noise_cepstrum_rows(torch, nz, Q=63, reps=20, runs=3):
    """The noise model `nz` to cepstral rows and back, same session: eaqhm_noise_cepstrum at order Q
    and eaqhm_noise_from_cepstrum on its rows at the model's own LPC order, next to eaqhm_noise_warp at alpha = 1.2 on
    the same model (base_ms), which shares the way back's lag sums and recursion and is the comparison, not a bar.
    Each time: median of `runs` warmed windows of `reps` launches; margin_ms = max - min of the warp's windows."""
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    dev = c.device
    p, Nf = nz["order"], len(nz["sigma"])

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    sigma, refl = (torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in (nz["sigma"], nz["refl"]))
    sigma_o, refl_o = torch.empty_like(sigma), torch.empty_like(refl)
    alpha_d = torch.full((Nf,), 1.2, dtype=torch.float64, device=dev)
    ceps = torch.empty((Nf, Q + 1), dtype=torch.float64, device=dev)
    base = med(lambda: c.noise_warp(sigma, refl, Nf, p, alpha_d, sigma_o, refl_o))
    fwd = med(lambda: c.noise_cepstrum(sigma, refl, Nf, p, Q, ceps))
    back = med(lambda: c.noise_from_cepstrum(ceps, Nf, Q, p, sigma_o, refl_o))
    return [dict(setting="Q%d" % Q, hop=nz["hop"], order=p, frames=Nf, silent=int((nz["sigma"] == 0).sum()),
                 base_ms=base[0], margin_ms=base[1], cepstrum_ms=fwd[0], cepstrum_spread_ms=fwd[1],
                 from_cepstrum_ms=back[0], from_cepstrum_spread_ms=back[1],
                 from_cepstrum_to_warp=round(back[0] / base[0], 3), cepstrum_to_warp=round(fwd[0] / base[0], 3))]


def cepwarp_rows(torch, st, nz, reps=20, runs=3, grid=120):
    """Every *_warped entry point next to its sibling, same session, same model: the fit, the knot
    amplitudes at beta = 1.25, the envelope and the phase on a `grid`-point grid up to fs/2, the model build and the noise
    frames from cepstral rows, at the default order min(63, 2 + round(fs / 1000)) and at order 24, a = cepstrum_warp(fs).
    The warped kernels read rows fitted on the warped axis, the siblings rows fitted on the linear one (the noise rows are
    noise_cepstrum's, cut to the order, and those moved by cepstrum_rewarp).  Each time: median of `runs` warmed windows
    of `reps` launches; margin_ms = max - min of the sibling's windows; ratio = warped / sibling."""
    from eaqhm_amd.model import _records_f0, cepstrum_rewarp, cepstrum_warp, check_model_build_arguments, noise_cepstrum
    c, rec, amp = (st[k] for k in ("c", "rec", "amp"))
    n, K, D, fs = st["n"], st["K"], st["D"], st["fs"]
    dev = c.device
    a = cepstrum_warp(fs)

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return ts[len(ts) // 2], ts[-1] - ts[0]

    def row(setting, P, base, new, **more):
        return dict(setting=setting, order=P, cep_warp=round(a, 6), base_ms=round(base[0], 4), margin_ms=round(base[1], 4),
                    new_ms=round(new[0], 4), new_spread_ms=round(new[1], 4), ratio=round(new[0] / base[0], 4), **more)

    rows = []
    rec_h = rec.cpu().numpy()
    f_grid = torch.as_tensor(np.linspace(0.0, fs / 2.0, grid), device=dev)
    beta_d = torch.full((n,), 1.25, dtype=torch.float64, device=dev)
    noise_rows = noise_cepstrum(nz, 63)
    Nf, p = len(noise_rows), nz["order"]
    sigma_o = torch.empty(Nf, dtype=torch.float64, device=dev)
    refl_o = torch.empty((Nf, p), dtype=torch.float64, device=dev)
    for P in sorted({min(63, 2 + int(round(fs / 1000.0))), 24}):
        lin = torch.empty((n, P + 1), dtype=torch.float64, device=dev)
        wrp = torch.empty((n, P + 1), dtype=torch.float64, device=dev)
        rows.append(row("fit_P%d" % P, P, med(lambda: c.model_cepstrum(rec, n, K, fs, P, 5e-4, lin)),
                        med(lambda: c.model_cepstrum_warped(rec, n, K, fs, P, 5e-4, wrp, a)), instants=n,
                        nan_rows=int(torch.isnan(wrp).any(dim=1).sum().item())))
        rows.append(row("amp_P%d" % P, P, med(lambda: c.modify_amp_cepstrum(rec, n, K, fs, beta_d, lin, P, amp)),
                        med(lambda: c.modify_amp_cepstrum_warped(rec, n, K, fs, beta_d, wrp, P, amp, a)), cells=n * K))
        out = torch.empty((n, grid), dtype=torch.float64, device=dev)
        rows.append(row("envelope_P%d" % P, P, med(lambda: c.cepstrum_envelope(lin, n, P, fs, f_grid, grid, out)),
                        med(lambda: c.cepstrum_envelope_warped(wrp, n, P, fs, f_grid, grid, out, a)), cells=n * grid))
        rows.append(row("phase_P%d" % P, P, med(lambda: c.cepstrum_phase(lin, n, P, fs, f_grid, grid, out)),
                        med(lambda: c.cepstrum_phase_warped(wrp, n, P, fs, f_grid, grid, out, a)), cells=n * grid))
        b = check_model_build_arguments(_records_f0(rec_h, K), lin.cpu().numpy(), fs, D,
                                        voiced=(rec_h[:, :K] != 0).any(axis=1))
        Kb = b["Kmax"]
        f_d, th_d, a0_d = (torch.as_tensor(np.ascontiguousarray(b[k]), device=dev) for k in ("f0", "theta", "a0"))
        v_d = torch.as_tensor(b["voiced"].astype(np.uint8), device=dev)
        built = torch.empty((n, 3 * Kb + 1), dtype=torch.float64, device=dev)
        rows.append(row("build_P%d" % P, P,
                        med(lambda: c.model_build(f_d, th_d, v_d, lin, P, a0_d, n, fs, Kb, b["Kcap"], False, built)),
                        med(lambda: c.model_build_warped(f_d, th_d, v_d, wrp, P, a0_d, n, fs, Kb, b["Kcap"], False, built,
                                                         a)), Kmax_built=Kb, cells=int(b["counts"].sum())))
        nl = torch.as_tensor(np.ascontiguousarray(noise_rows[:, :P + 1]), device=dev)
        nw = torch.as_tensor(cepstrum_rewarp(noise_rows, 0.0, a, P), device=dev)
        rows.append(row("noise_from_cepstrum_Q%d" % P, P,
                        med(lambda: c.noise_from_cepstrum(nl, Nf, P, p, sigma_o, refl_o)),
                        med(lambda: c.noise_from_cepstrum_warped(nw, Nf, P, p, sigma_o, refl_o, a)), frames=Nf, lpc_order=p))
    return rows


def build_rows(torch, st, reps=20, runs=3):
    """The model from parameters, same session: eaqhm_model_build on the model's own f0, voicing and
    cepstrum (default order; new_ms), next to eaqhm_modify_amp_cepstrum at beta = 1 on the same model (base_ms), which
    does the same work per cell (one Clenshaw sum and one exp) and is the comparison, not a bar.  Each time: median of
    `runs` warmed windows of `reps` launches; margin_ms = max - min of the existing kernel's windows."""
    from eaqhm_amd.model import _records_f0, check_model_build_arguments
    c, rec, amp = (st[k] for k in ("c", "rec", "amp"))
    n, K, D, fs = st["n"], st["K"], st["D"], st["fs"]
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return ts[len(ts) // 2], ts[-1] - ts[0]

    P = min(63, 2 + int(round(fs / 1000.0)))
    ceps = torch.empty((n, P + 1), dtype=torch.float64, device=dev)
    c.model_cepstrum(rec, n, K, fs, P, 5e-4, ceps)
    rec_h = rec.cpu().numpy()
    a = check_model_build_arguments(_records_f0(rec_h, K), ceps.cpu().numpy(), fs, D,
                                    voiced=(rec_h[:, :K] != 0).any(axis=1))
    Kb = a["Kmax"]
    f_d, th_d, a0_d = (torch.as_tensor(np.ascontiguousarray(a[k]), device=dev) for k in ("f0", "theta", "a0"))
    v_d = torch.as_tensor(a["voiced"].astype(np.uint8), device=dev)
    out = torch.empty((n, 3 * Kb + 1), dtype=torch.float64, device=dev)
    beta_d = torch.ones(n, dtype=torch.float64, device=dev)
    base = med(lambda: c.modify_amp_cepstrum(rec, n, K, fs, beta_d, ceps, P, amp))
    new = med(lambda: c.model_build(f_d, th_d, v_d, ceps, P, a0_d, n, fs, Kb, a["Kcap"], False, out))
    cells = int(a["counts"].sum())
    return [dict(setting="build_P%d" % P, order=P, instants=n, Kmax_model=K, Kmax_built=Kb, active_cells_built=cells,
                 active_cells_model=int(np.count_nonzero(rec_h[:, :K])), bytes_written=n * (3 * Kb + 1) * 8,
                 base_ms=round(base[0], 4), margin_ms=round(base[1], 4), new_ms=round(new[0], 4),
                 new_spread_ms=round(new[1], 4), new_gb_per_s=round(n * (3 * Kb + 1) * 8 / (new[0] * 1e-3) / 1e9, 1))]


def align_rows(torch, st, band_s=2.0, excerpt_s=5.0, runs=3):
    """The time alignment of the model's cepstrum (default order) against a copy of itself stretched
    by warp_rows with a 0.25 Hz sinusoidal tempo between 0.8 and 1.25, band `band_s` seconds.  One launch sequence per
    window (the forward pass is thousands of launches), median of `runs` windows and their max - min: the cost kernel,
    eaqhm_dtw's forward pass and its backtrack (EAQHM_OPT_DTW_PHASES).  numpy_model_s: tests/model_align_ref.py on the
    first `excerpt_s` seconds with the same band, on the host."""
    from eaqhm_amd.model import band_min_radius, warp_rows
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import model_align_ref as AR
    c, rec, n, K, D, fs = (st[k] for k in ("c", "rec", "n", "K", "D", "fs"))
    dev = c.device
    P = min(63, 2 + int(round(fs / 1000.0)))
    ceps = torch.empty((n, P + 1), dtype=torch.float64, device=dev)
    c.model_cepstrum(rec, n, K, fs, P, 5e-4, ceps)
    CA = ceps.cpu().numpy()
    tempo = np.exp(np.log(1.25 / 0.8) / 2 * np.sin(2 * np.pi * 0.25 * np.arange(2 * n) * D / fs))   # 0.8 .. 1.25
    idx = np.concatenate(([0.0], np.cumsum(1.0 / tempo)))
    CB = warp_rows(CA, idx[idx <= n - 1])
    nA, nB = len(CA), len(CB)
    r = max(int(band_s * fs / D), band_min_radius(nA, nB))
    W = 2 * r + 1
    A_d, B_d = torch.as_tensor(CA, device=dev), torch.as_tensor(CB, device=dev)
    band = torch.empty((nA, W), dtype=torch.float64, device=dev)
    ptr = torch.empty((nA, W), dtype=torch.uint8, device=dev)
    path = torch.empty((nA + nB - 1, 2), dtype=torch.int32, device=dev)
    plen = torch.zeros(1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)

    def med(fn, before=None):
        ts = []
        for _ in range(runs + 1):              # the first window warms
            if before:
                before()
            torch.cuda.synchronize()
            ts.append(timed_once(torch, fn))
        ts = sorted(ts[1:])
        return round(ts[len(ts) // 2], 3), round(ts[-1] - ts[0], 3)

    cost = lambda: c.cepstrum_cost(A_d, nA, B_d, nB, P, 0.0, 4.0, r, band)
    t_cost = med(cost)
    c.set_option(3, 1)
    t_fwd = med(lambda: c.dtw(band, nA, nB, r, ptr, path, plen, total), before=cost)
    c.set_option(3, 2)
    t_back = med(lambda: c.dtw(band, nA, nB, r, ptr, path, plen, total))
    c.set_option(3, 0)
    L = int(plen.item())
    m = min(nA, int(excerpt_s * fs / D))
    mb = int(np.searchsorted(idx, m))
    t = time.perf_counter()
    dense = AR.cost(CA[:m], CB[:mb])
    re = max(min(r, AR.full_radius(m, mb)), AR.min_radius(m, mb))
    AR.align(dense, re)
    t_np = time.perf_counter() - t
    return dict(order=P, nA=nA, nB=nB, band_s=band_s, r=r, cells=nA * W, cost_ms=t_cost[0], cost_spread_ms=t_cost[1],
                forward_ms=t_fwd[0], forward_spread_ms=t_fwd[1],
                forward_launches_at_most=(nA + 63) // 64 + (nB + 63) // 64 - 1, backtrack_ms=t_back[0],
                backtrack_spread_ms=t_back[1], path_len=L, total=float(total.item()),
                numpy_model_s=round(t_np, 2), numpy_model_rows=(m, mb), numpy_model_r=re)


def timed_once(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def cepstrum_rows(torch, st, reps=20, runs=3):
    """The discrete-cepstrum envelope, same session, same model.  fit rows: eaqhm_model_cepstrum at
    the default order min(63, 2 + round(fs / 1000)) and at 63, lam = 5e-4 (new_ms only: there is no existing
    counterpart).  prep rows: eaqhm_modify_prep without the envelope followed by eaqhm_modify_amp_cepstrum (new_ms)
    against eaqhm_modify_prep with the envelope (base_ms) at beta in {1.25, 1} (at beta = 1 the existing path copies the
    amplitudes), and with alpha = 1.2 on both sides.  Each time: median of `runs` windows of `reps` launches;
    margin_ms = max - min of the existing path's windows."""
    c, rec, code, mom, amp, R, ph0 = (st[k] for k in ("c", "rec", "code", "mom", "amp", "R", "ph0"))
    n, K, D, fs = st["n"], st["K"], st["D"], st["fs"]
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return ts[len(ts) // 2], ts[-1] - ts[0]

    rows = []
    P0 = min(63, 2 + int(round(fs / 1000.0)))
    for P in sorted({P0, 63}):
        ceps = torch.empty((n, P + 1), dtype=torch.float64, device=dev)
        t = med(lambda: c.model_cepstrum(rec, n, K, fs, P, 5e-4, ceps))
        rows.append(dict(setting="fit_P%d" % P, new_ms=round(t[0], 4), new_spread_ms=round(t[1], 4), order=P,
                         instants=n, us_per_instant=round(1e3 * t[0] / n, 5),
                         nan_rows=int(torch.isnan(ceps).any(dim=1).sum().item())))
    ceps = torch.empty((n, P0 + 1), dtype=torch.float64, device=dev)
    c.model_cepstrum(rec, n, K, fs, P0, 5e-4, ceps)
    for beta, alpha in ((1.25, None), (1.0, None), (1.25, 1.2)):
        beta_d = torch.full((n,), beta, dtype=torch.float64, device=dev)
        alpha_d = None if alpha is None else torch.full((n,), alpha, dtype=torch.float64, device=dev)

        def cepstrum_path():
            c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, None, False, amp, R, ph0)
            c.modify_amp_cepstrum(rec, n, K, fs, beta_d, ceps, P0, amp, alpha=alpha_d)

        base = med(lambda: c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, alpha_d, True, amp, R, ph0))
        new = med(cepstrum_path)
        rows.append(dict(setting="prep_beta%g%s" % (beta, "" if alpha is None else "_alpha%g" % alpha),
                         base_ms=round(base[0], 4), margin_ms=round(base[1], 4), new_ms=round(new[0], 4),
                         new_spread_ms=round(new[1], 4), new_minus_base_ms=round(new[0] - base[0], 4),
                         ratio=round(new[0] / base[0], 4), order=P0))
    return rows


def formant_warp_rows(torch, st, nz, reps=20, runs=3):
    """The piecewise-linear formant warp next to the formant scale, same session, same model.
    Deterministic rows: eaqhm_modify_prep without the envelope followed by eaqhm_modify_amp_warp (new_ms) against
    eaqhm_modify_prep with alpha (base_ms) at beta in {1, 1.25}: the VTLN maps 0.85 and 1.2 against alpha = 0.85 and
    1.2, and a 16-breakpoint map against alpha = 1.2.  Noise rows: eaqhm_noise_warp_map against eaqhm_noise_warp on
    the model `nz`.  Each time: median of `runs` windows of `reps` launches; margin_ms = max - min of the existing
    path's windows."""
    from eaqhm_amd.model import formant_warp_vtln
    c, rec, code, mom, amp, R, ph0 = (st[k] for k in ("c", "rec", "code", "mom", "amp", "R", "ph0"))
    n, K, D, fs = st["n"], st["K"], st["D"], st["fs"]
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return ts[len(ts) // 2], ts[-1] - ts[0]

    def row(setting, base, new, **more):
        return dict(setting=setting, base_ms=round(base[0], 4), margin_ms=round(base[1], 4), new_ms=round(new[0], 4),
                    new_spread_ms=round(new[1], 4), new_minus_base_ms=round(new[0] - base[0], 4),
                    ratio=round(new[0] / base[0], 4), **more)

    nyq = fs / 2.0
    x16 = nyq * np.arange(1, 17) / 16.0
    cases = [("vtln0.85", 0.85) + formant_warp_vtln(fs, 0.85), ("vtln1.2", 1.2) + formant_warp_vtln(fs, 1.2),
             ("b16", 1.2, x16, x16 * (1.0 + 0.15 * np.sin(np.pi * np.arange(1, 17) / 16.0)))]
    rows = []
    for beta in (1.0, 1.25):
        beta_d = torch.full((n,), beta, dtype=torch.float64, device=dev)
        for name, alpha, x, y in cases:
            alpha_d = torch.full((n,), alpha, dtype=torch.float64, device=dev)
            x_d = torch.as_tensor(x, device=dev)
            y_d = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(y, (n, len(x)))), device=dev)

            def warp_path():
                c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, None, False, amp, R, ph0)
                c.modify_amp_warp(rec, n, K, fs, beta_d, x_d, y_d, len(x), amp)

            base = med(lambda: c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, alpha_d, True, amp, R, ph0))
            rows.append(row("prep_%s_beta%g" % (name, beta), base, med(warp_path), breakpoints=len(x)))
    H, p, Nf = nz["hop"], nz["order"], len(nz["sigma"])
    sigma, refl = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (nz["sigma"], nz["refl"]))
    sigma_w, refl_w = torch.empty_like(sigma), torch.empty_like(refl)
    for name, alpha, x, y in cases:
        alpha_d = torch.full((Nf,), alpha, dtype=torch.float64, device=dev)
        x_d = torch.as_tensor(x / fs, device=dev)
        y_d = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(y / fs, (Nf, len(x)))), device=dev)
        base = med(lambda: c.noise_warp(sigma, refl, Nf, p, alpha_d, sigma_w, refl_w))
        new = med(lambda: c.noise_warp_map(sigma, refl, Nf, p, x_d, y_d, len(x), sigma_w, refl_w))
        rows.append(row("noise_%s" % name, base, new, breakpoints=len(x), hop=H, order=p, frames=Nf))
    return rows


def noise_modulation_rows(torch, st, residual, harmonics=2, reps=20, runs=3):
    """The pitch-synchronous modulation of the noise on `residual` with the model of `st`: device time
    of eaqhm_noise_modulation next to eaqhm_noise_analyse, and of eaqhm_noise_synth with the mod group next to without
    at rho in {0.5, 1, 2} (beta = 1) with the analysed coefficients.  Each time: median of `runs` windows of `reps`
    launches, and their max - min."""
    from eaqhm_amd.model import (_fundamental_at, _records_f0, _records_phase, _scalar_path,
                                 check_noise_analysis_arguments, noise_time_map)
    c, K, D, fs, L, n = (st[k] for k in ("c", "K", "D", "fs", "L", "n"))
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    rec = st["rec"].cpu().numpy()
    model = dict(records=rec, Kmax=K, step=D, ti=np.arange(n, dtype=np.int64) * D)
    f0 = _records_f0(rec, K)
    e, _, H, p = check_noise_analysis_arguments(residual, np.zeros(len(residual)), fs)
    Nf = (L - 1) // H + 1
    e_d, th_d, f0_d, v_d = (torch.as_tensor(np.ascontiguousarray(x), device=dev)
                            for x in (e, _records_phase(rec, K, f0, D, fs), f0,
                                      (rec[:, :K] != 0).any(axis=1).astype(np.uint8)))
    sigma = torch.empty(Nf, dtype=torch.float64, device=dev)
    refl = torch.empty((Nf, p), dtype=torch.float64, device=dev)
    mod = torch.empty((Nf, 2 * harmonics), dtype=torch.float64, device=dev)
    t_an, s_an = med(lambda: c.noise_analyse(e_d, L, H, p, sigma, refl))
    t_mo, s_mo = med(lambda: c.noise_modulation(e_d, L, H, th_d, f0_d, v_d, n, 0.0, float(D), fs, harmonics, mod))
    rows = [dict(setting="analysis", hop=H, order=p, frames=Nf, harmonics=harmonics, analyse_ms=t_an,
                 analyse_spread_ms=s_an, modulation_ms=t_mo, modulation_spread_ms=s_mo,
                 modulation_to_analyse=round(t_mo / t_an, 3),
                 mean_abs_c1=round(float(torch.hypot(mod[:, 0], mod[:, 1]).mean()), 4))]
    for rho in (0.5, 1.0, 2.0):
        Lo = int(np.rint(rho * L))
        tau = noise_time_map(H, Lo, rho)
        theta, nu = _fundamental_at(model, fs, tau, f0, *_scalar_path(n, rho, 1.0))
        tau_d, theta_d, nu_d = (torch.as_tensor(x, device=dev) for x in (tau, theta, nu))
        out = torch.empty(Lo, dtype=torch.float64, device=dev)
        t_ns, s_ns = med(lambda: c.noise_synth(sigma, refl, Nf, H, p, tau_d, len(tau), 0, Lo, 0, Lo, out))
        t_nm, s_nm = med(lambda: c.noise_synth(sigma, refl, Nf, H, p, tau_d, len(tau), 0, Lo, 0, Lo, out,
                                               mod=(mod, harmonics, theta_d, nu_d)))
        rows.append(dict(setting="rho%g" % rho, out_frames=len(tau), noise_synth_ms=t_ns, noise_synth_spread_ms=s_ns,
                         noise_synth_mod_ms=t_nm, noise_synth_mod_spread_ms=s_nm,
                         mod_minus_plain_ms=round(t_nm - t_ns, 4), mod_to_plain=round(t_nm / t_ns, 3)))
    return rows


def noise_formant_rows(torch, nz, reps=20, runs=3, grid=129):
    """The formant warp of a noise model `nz` (from eaQHMNoiseAnalysis): device time of eaqhm_noise_warp and of
    eaqhm_noise_envelope on `grid` frequencies in [0, fs/2] at alpha 0.85, 1.2 and a ramp 0.85 -> 1.2 over the frames,
    beside eaqhm_noise_synth of the warped model at rho = 1.  Each time: median of `runs` windows of `reps` launches,
    and their max - min."""
    from eaqhm_amd.functions import _ctx
    from eaqhm_amd.model import noise_time_map
    c = _ctx(0)
    dev = c.device
    H, p, L = nz["hop"], nz["order"], nz["length"]
    Nf = len(nz["sigma"])

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    sigma, refl, tau = (torch.as_tensor(np.ascontiguousarray(x), device=dev)
                        for x in (nz["sigma"], nz["refl"], noise_time_map(H, L, 1.0)))
    sigma_w, refl_w = torch.empty_like(sigma), torch.empty_like(refl)
    fnorm = torch.as_tensor(np.linspace(0.0, 0.5, grid), device=dev)
    env = torch.empty((Nf, grid), dtype=torch.float64, device=dev)
    out = torch.empty(L, dtype=torch.float64, device=dev)
    rows = []
    for setting, alpha in (("alpha0.85", np.full(Nf, 0.85)), ("alpha1.2", np.full(Nf, 1.2)),
                           ("alpha_ramp", np.linspace(0.85, 1.2, Nf))):
        alpha_d = torch.as_tensor(alpha, device=dev)
        t_w, s_w = med(lambda: c.noise_warp(sigma, refl, Nf, p, alpha_d, sigma_w, refl_w))
        t_e, s_e = med(lambda: c.noise_envelope(sigma, refl, Nf, p, alpha_d, fnorm, grid, env))
        t_ns, s_ns = med(lambda: c.noise_synth(sigma_w, refl_w, Nf, H, p, tau, len(tau), 0, L, 0, L, out))
        rows.append(dict(setting=setting, hop=H, order=p, frames=Nf, warp_ms=t_w, warp_spread_ms=s_w, envelope_ms=t_e,
                         envelope_spread_ms=s_e, envelope_grid=grid, noise_synth_ms=t_ns, noise_synth_spread_ms=s_ns,
                         warp_to_noise_synth=round(t_w / t_ns, 3)))
    return rows


def noise_rows(torch, st, residual, reps=20, runs=3):
    """The stochastic component on `residual` (the workload's s - s_recon, default hop and order): device time of
    eaqhm_noise_analyse, and of eaqhm_noise_synth (lattice + cross-fade) at rho in {0.5, 1, 2} beside the deterministic
    eaqhm_modify_prep + eaqhm_modify_synth at the same rho and beta = 1.  Each time: median of `runs` windows of `reps`
    launches, and their max - min."""
    from eaqhm_amd.model import check_noise_analysis_arguments, noise_time_map
    c, rec, code, mom, amp, R, ph0 = (st[k] for k in ("c", "rec", "code", "mom", "amp", "R", "ph0"))
    n, K, D, fs, L = st["n"], st["K"], st["D"], st["fs"], st["L"]
    dev = c.device

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return round(ts[len(ts) // 2], 4), round(ts[-1] - ts[0], 4)

    e, _, H, p = check_noise_analysis_arguments(residual, np.zeros(len(residual)), fs)
    Nf = (L - 1) // H + 1
    e_d = torch.as_tensor(e, device=dev)
    sigma = torch.empty(Nf, dtype=torch.float64, device=dev)
    refl = torch.empty((Nf, p), dtype=torch.float64, device=dev)
    t_an, s_an = med(lambda: c.noise_analyse(e_d, L, H, p, sigma, refl))
    one_d = torch.ones(n, dtype=torch.float64, device=dev)
    t_prep, _ = med(lambda: c.modify_prep(rec, code, mom, n, K, D, fs, one_d, None, None, True, amp, R, ph0))
    rows = [dict(setting="analysis", hop=H, order=p, frames=Nf, analyse_ms=t_an, analyse_spread_ms=s_an)]
    for rho in (0.5, 1.0, 2.0):
        Lo = int(np.rint(rho * L))
        tau = torch.as_tensor(noise_time_map(H, Lo, rho), device=dev)
        out = torch.empty(Lo, dtype=torch.float64, device=dev)
        t_ns, s_ns = med(lambda: c.noise_synth(sigma, refl, Nf, H, p, tau, len(tau), 0, Lo, 0, Lo, out))
        t_det, s_det = med(lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, rho, 1.0, Lo, 0, Lo, out))
        rows.append(dict(setting="rho%g" % rho, out_frames=len(tau), noise_synth_ms=t_ns, noise_synth_spread_ms=s_ns,
                         det_eval_ms=t_det, det_eval_spread_ms=s_det, det_total_ms=round(t_prep + t_det, 4),
                         noise_to_det_eval=round(t_ns / t_det, 3)))
    return rows


def shape_rows(torch, st, reps=20, runs=3):
    """The shape-invariant phase mode: device time of the shape eval kernels next to the existing ones,
    same session, same prepared model.  Each time: median of `runs` windows of `reps` launches; margin_ms = max - min of
    the existing kernel's windows."""
    from eaqhm_amd.model import _records_f0, contour_time_map, fundamental_advance
    c, rec, code, mom, amp, R, ph0 = (st[k] for k in ("c", "rec", "code", "mom", "amp", "R", "ph0"))
    n, K, D, fs, L = st["n"], st["K"], st["D"], st["fs"], st["L"]
    dev = c.device
    f0 = _records_f0(rec.cpu().numpy(), K)
    f0_d = torch.as_tensor(f0, device=dev)

    def med(fn):
        ts = sorted(timed(torch, fn, reps) for _ in range(runs))
        return ts[len(ts) // 2], ts[-1] - ts[0]

    def row(setting, Lo, base, new):
        return dict(setting=setting, out_samples=Lo, eval_ms=round(base[0], 4), margin_ms=round(base[1], 4),
                    shape_eval_ms=round(new[0], 4), shape_spread_ms=round(new[1], 4),
                    shape_minus_eval_ms=round(new[0] - base[0], 4), ratio=round(new[0] / base[0], 4))

    rows = []
    for beta in (1.0, 1.25):
        beta_d = torch.full((n,), beta, dtype=torch.float64, device=dev)
        c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, None, True, amp, R, ph0)
        for rho in (0.5, 1.0, 2.0):
            Lo = int(np.rint(rho * L))
            out = torch.empty(Lo, dtype=torch.float64, device=dev)
            S_d = torch.as_tensor(fundamental_advance(f0, np.full(n - 1, beta * rho), D, fs), device=dev)
            base = med(lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, rho, beta, Lo, 0, Lo, out))
            new = med(lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, rho, beta, Lo, 0, Lo, out,
                                             shape=(f0_d, S_d)))
            rows.append(row("rho%g_beta%g" % (rho, beta), Lo, base, new))
    t = np.arange(n) * D / fs
    one = np.ones(n)
    sinus = 1.05 + 0.35 * np.sin(2 * np.pi * 0.5 * t)
    ramp = np.interp(t, [0.0, t[-1]], [0.85, 1.2])
    for label, rho, beta in (("unit", one, one), ("rho_sinus", sinus, one), ("beta_ramp", one, ramp),
                             ("both", sinus, ramp)):
        tm = contour_time_map(rho, beta, D, L)
        Lo = tm["L_out"]
        beta_d, gain_d, C_d, rate_d = (torch.as_tensor(np.ascontiguousarray(x), device=dev)
                                       for x in (beta, tm["gain"], tm["C"], tm["rate"]))
        S_d = torch.as_tensor(fundamental_advance(f0, tm["gain"], D, fs), device=dev)
        out = torch.empty(Lo, dtype=torch.float64, device=dev)
        c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, gain_d, None, True, amp, R, ph0)
        curve = (C_d, rate_d, gain_d, tm["rate_min"])
        base = med(lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, 0.0, 0.0, Lo, 0, Lo, out, curve))
        c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, None, True, amp, R, ph0)   # the shape mode's prep
        new = med(lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, 0.0, 0.0, Lo, 0, Lo, out, curve,
                                         (f0_d, S_d)))
        rows.append(row("contour_" + label, Lo, base, new))
    return rows


def formant_rows(torch, st, reps):
    """rho = 1: the scalar path (alpha = 1, envelope on) and the formant path at alpha in {0.85, 1.2} for beta in
    {1, 1.25}, and an alpha ramp 0.85 -> 1.2 through the contour kernels (rho = beta = 1)."""
    from eaqhm_amd.model import contour_time_map
    c, rec, code, mom, amp, R, ph0 = (st[k] for k in ("c", "rec", "code", "mom", "amp", "R", "ph0"))
    n, K, D, fs, L, t_eval = st["n"], st["K"], st["D"], st["fs"], st["L"], st["t_eval"]
    dev = c.device
    out = torch.empty(L, dtype=torch.float64, device=dev)
    rows = []

    def row(setting, t_prep, t_syn, t_scalar):
        total = t_prep + t_syn
        return dict(setting=setting, prep_scan_ms=round(t_prep, 3), eval_ms=round(t_syn, 3), total_ms=round(total, 3),
                    ratio_to_eval_synth=round(total / t_eval, 3), ratio_to_scalar=round(total / t_scalar, 3))

    for beta in (1.0, 1.25):
        beta_d = torch.full((n,), beta, dtype=torch.float64, device=dev)
        t_sp = timed(torch, lambda: c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, None, True, amp, R, ph0),
                     reps)
        t_syn = timed(torch, lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, 1.0, beta, L, 0, L, out),
                      reps)
        t_scalar = t_sp + t_syn
        rows.append(row("scalar_beta%g" % beta, t_sp, t_syn, t_scalar))
        for alpha in (0.85, 1.2):
            alpha_d = torch.full((n,), alpha, dtype=torch.float64, device=dev)
            t_fp = timed(torch, lambda: c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None, alpha_d, True, amp, R,
                                                      ph0), reps)
            t_fs = timed(torch, lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, 1.0, beta, L, 0, L,
                                                       out), reps)
            rows.append(row("alpha%g_beta%g" % (alpha, beta), t_fp, t_fs, t_scalar))
    t = np.arange(n) * D / fs
    one = np.ones(n)
    ramp = np.interp(t, [0.0, t[-1]], [0.85, 1.2])
    tm = contour_time_map(one, one, D, L)
    one_d, gain_d, C_d, rate_d, alpha_d = (torch.as_tensor(np.ascontiguousarray(x), device=dev)
                                           for x in (one, tm["gain"], tm["C"], tm["rate"], ramp))
    outc = torch.empty(tm["L_out"], dtype=torch.float64, device=dev)
    t_fp = timed(torch, lambda: c.modify_prep(rec, code, mom, n, K, D, fs, one_d, gain_d, alpha_d, True, amp, R, ph0),
                 reps)
    t_fs = timed(torch, lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, 0.0, 0.0, tm["L_out"], 0,
                                               tm["L_out"], outc, (C_d, rate_d, gain_d, tm["rate_min"])), reps)
    rows.append(row("alpha_ramp_contour", t_fp, t_fs, rows[0]["total_ms"]))
    return rows


def probe_contours(torch, c, rec, code, mom, amp, R, ph0, n, K, D, fs, L, t_eval, reps):
    from eaqhm_amd.model import contour_time_map
    dev = c.device
    t = np.arange(n) * D / fs
    one = np.ones(n)
    sinus = 1.05 + 0.35 * np.sin(2 * np.pi * 0.5 * t)
    ramp = np.interp(t, [0.0, t[-1]], [0.85, 1.2])
    rows = []
    for label, rho, beta in (("unit", one, one), ("rho_sinus", sinus, one), ("beta_ramp", one, ramp),
                             ("both", sinus, ramp)):
        tm = contour_time_map(rho, beta, D, L)
        Lo = tm["L_out"]
        beta_d, gain_d, C_d, rate_d = (torch.as_tensor(np.ascontiguousarray(x), device=dev)
                                       for x in (beta, tm["gain"], tm["C"], tm["rate"]))
        out = torch.empty(Lo, dtype=torch.float64, device=dev)
        t_prep = timed(torch, lambda: c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, gain_d, None, True, amp, R,
                                                    ph0), reps)
        t_syn = timed(torch, lambda: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, 0.0, 0.0, Lo, 0, Lo, out,
                                                    (C_d, rate_d, gain_d, tm["rate_min"])), reps)
        rows.append(dict(contour=label, prep_scan_ms=round(t_prep, 3), eval_ms=round(t_syn, 3),
                         total_ms=round(t_prep + t_syn, 3), out_samples=Lo,
                         eval_ms_per_msample=round(t_syn / (Lo / 1e6), 4),
                         msamples_per_s=round(Lo / ((t_prep + t_syn) * 1e-3) / 1e6, 1),
                         ratio_to_eval_synth=round((t_prep + t_syn) / t_eval, 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synth16k_60s,synth48k_60s")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--contours", action="store_true", help="also time the contour kernels")
    ap.add_argument("--formant", action="store_true", help="also time the formant prep kernels")
    ap.add_argument("--noise", action="store_true", help="also time the noise analysis and synthesis kernels")
    ap.add_argument("--noise-formant", action="store_true", help="also time the noise warp and envelope kernels")
    ap.add_argument("--noise-modulation", action="store_true",
                    help="also time the modulation analysis and the modulated noise synthesis")
    ap.add_argument("--shape", action="store_true", help="also time the shape-invariant phase kernels")
    ap.add_argument("--formant-warp", action="store_true",
                    help="also time the piecewise-linear formant warp next to the formant scale")
    ap.add_argument("--cepstrum", action="store_true",
                    help="also time the cepstral fit and the amplitudes read off it against the prep with the envelope")
    ap.add_argument("--align", action="store_true",
                    help="also time the alignment kernels on the model against a time-stretched copy of itself")
    ap.add_argument("--build", action="store_true",
                    help="also time eaqhm_model_build next to eaqhm_modify_amp_cepstrum (the model from parameters)")
    ap.add_argument("--noise-cepstrum", action="store_true",
                    help="also time eaqhm_noise_cepstrum and eaqhm_noise_from_cepstrum next to eaqhm_noise_warp")
    ap.add_argument("--cepstrum-warp", action="store_true",
                    help="also time every *_warped entry point of the warped cepstrum next to its sibling")
    ap.add_argument("--gmm", action="store_true",
                    help="time eaqhm_gmm_estep, eaqhm_gmm_mstep and eaqhm_gmm_regress next to torch matmuls (random rows; "
                         "needs no workload: pass --workloads '')")
    ap.add_argument("--mlpg", action="store_true",
                    help="time eaqhm_ceps_delta and eaqhm_mlpg_solve next to scipy.linalg.solveh_banded on the host (random "
                         "rows; needs no workload: pass --workloads '')")
    ap.add_argument("--gv", action="store_true",
                    help="time eaqhm_gv_ascend next to eaqhm_mlpg_solve and the same iteration in NumPy on the host (random "
                         "rows; needs no workload: pass --workloads '')")
    ap.add_argument("--kmeans", action="store_true",
                    help="time eaqhm_kmeans_assign and eaqhm_kmeans_update next to torch and to one EM round, the whole "
                         "kmeans call and the fit from both starts (seeded rows; needs no workload: pass --workloads '')")
    ap.add_argument("--mlpg-em", action="store_true",
                    help="time eaqhm_mlpg_estep next to eaqhm_gmm_estep and eaqhm_gmm_regress, and one refinement iteration "
                         "(random rows; needs no workload: pass --workloads '')")
    ap.add_argument("--nn", action="store_true",
                    help="time eaqhm_nn_rows next to torch cdist + argmin (random rows; needs no workload: pass "
                         "--workloads '')")
    ap.add_argument("--swipe", action="store_true",
                    help="time the device SWIPE' kernels and the whole swipep_device call next to swipe.swipep on the "
                         "60 s signals of --workloads (nothing else runs)")
    ap.add_argument("--viterbi", action="store_true",
                    help="time the forward, backtrack and refine kernels of the continuous pitch track and the whole "
                         "swipep_viterbi call next to swipep_device and swipe.swipep on the 60 s signals of --workloads "
                         "(nothing else runs)")
    ap.add_argument("--formant-tracks", action="store_true",
                    help="time the roots, candidates, forward and backtrack kernels of the formant tracks next to a "
                         "numpy.roots loop on the all-pole models of the 60 s signals of --workloads (nothing else runs)")
    ap.add_argument("--onsets", action="store_true",
                    help="time the bands, flux and peaks kernels of the transient onset detector and the whole "
                         "onset_strength + onsets call on the 60 s signals of --workloads (nothing else runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.onsets:
        import torch
        res_onsets = [dict(onsets=onset_rows(torch, a.workloads.split(",")))]
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res_onsets, f, indent=1)
        return 0
    if a.formant_tracks:
        import torch
        res_formant = [dict(formant_tracks=formant_track_rows(torch, a.workloads.split(",")))]
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res_formant, f, indent=1)
        return 0
    if a.viterbi:
        import torch
        res_viterbi = [dict(viterbi=viterbi_rows(torch, a.workloads.split(",")))]
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res_viterbi, f, indent=1)
        return 0
    if a.swipe:
        import torch
        res_swipe = [dict(swipe=swipe_rows(torch, a.workloads.split(",")))]
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res_swipe, f, indent=1)
        return 0
    if a.nn:
        import torch
        res_nn = dict(nn=nn_rows(torch))
        if not a.workloads and not (a.kmeans or a.gv or a.mlpg or a.gmm or a.mlpg_em):
            print(json.dumps(res_nn))
            if a.out:
                with open(a.out, "w") as f:
                    json.dump([res_nn], f, indent=1)
            return 0
    if a.kmeans:
        import torch
        res_kmeans = dict(kmeans=kmeans_rows(torch))
        if not a.workloads and not a.gmm and not a.mlpg and not a.gv and not a.mlpg_em:
            if a.out:
                with open(a.out, "w") as f:
                    json.dump([res_kmeans], f, indent=1)
            return 0
    if a.gv:
        import torch
        res_gv = dict(gv=gv_rows(torch))
        if not a.workloads and not a.gmm and not a.mlpg and not a.mlpg_em:
            if a.out:
                with open(a.out, "w") as f:
                    json.dump([res_gv], f, indent=1)
            return 0
    if a.mlpg:
        import torch
        res_mlpg = dict(mlpg=mlpg_rows(torch))
        if not a.workloads and not a.gmm and not a.mlpg_em:
            if a.out:
                with open(a.out, "w") as f:
                    json.dump([res_mlpg], f, indent=1)
            return 0
    if a.gmm:
        import torch
        res_gmm = dict(gmm=gmm_rows(torch))
        if not a.workloads and not a.mlpg_em:
            if a.out:
                with open(a.out, "w") as f:
                    json.dump([res_gmm], f, indent=1)
            return 0
    if a.mlpg_em:
        import torch
        res_em = dict(mlpg_em=mlpg_em_rows(torch))
        if not a.workloads:
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(([res_gmm] if a.gmm else []) + ([res_mlpg] if a.mlpg else []) + ([res_gv] if a.gv else [])
                              + ([res_kmeans] if a.kmeans else []) + [res_em], f, indent=1)
            return 0
    res = [probe(w, a.reps, a.contours, a.formant, a.noise, a.shape, a.noise_formant,
                 a.noise_modulation, a.formant_warp, a.cepstrum, a.align, a.build, a.noise_cepstrum, a.cepstrum_warp)
           for w in a.workloads.split(",")]
    if a.gmm:
        res.append(res_gmm)
    if a.mlpg:
        res.append(res_mlpg)
    if a.gv:
        res.append(res_gv)
    if a.kmeans:
        res.append(res_kmeans)
    if a.mlpg_em:
        res.append(res_em)
    if a.nn:
        res.append(res_nn)
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
