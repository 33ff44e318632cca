"""Case tables and input builders of the direct tests of the noise kernels (csrc/eaqhm_noise.hip): the
analysis, the lattice filter and cross-fade, the formant warp and envelope readout (scale and map), the
pitch-synchronous modulation and the modulated cross-fade, at every hop, order and count edge of the kernels.  Plain
NumPy / SciPy, no torch: tests/test_noise_direct_cases_cpu.py shows with the models alone that the cases can judge a
kernel, tests/test_gpu_noise_direct.py runs them on the device.

A case is a dict with a `name` and the inputs of one call.  `*_models(case)` runs the NumPy model of the call in float64
(the definition) and in np.longdouble; the largest deviation between the two is the case's yardstick, from which the
GPU test takes its bar (100 x, DESIGN.md §10's rule).  The models of a case are computed once per process."""
import numpy as np
from scipy.signal import lfilter

import formant_warp_ref as FW
import noise_cepstrum_ref as NC
import noise_model_ref as N
import noise_modulation_ref as R
import noise_warp_ref as W

FS = 16000.0
SEED = 77                      # of the white excitation in every synthesis case

# (hop, order): windows of 4, 8, 16, 60 samples (shorter than a wave), 64, 68 (not a multiple of 64), the largest
# order, orders 32 / 33, the largest hop (133 120 bytes of LDS in the analysis kernel) with the smallest and largest order
SHAPES = [(1, 1), (1, 3), (2, 7), (4, 15), (15, 59), (16, 63), (17, 63), (64, 32), (64, 33), (256, 63), (1024, 1),
          (1024, 63)]
LENGTH_SHAPES = [(2, 7), (16, 63), (1024, 63)]     # these also run at every short length


def _unique(seq):
    out = []
    for x in seq:
        if x not in out:
            out.append(x)
    return out


def residual(L, seed, silent=None, level=0.02):
    """A coloured residual of L samples: the AR(4) noise of noise_model_ref.ar_fixture (poles 0.97 e^{+-0.5i},
    0.9 e^{+-2i}) times `level`, exactly zero on [silent[0], silent[1])."""
    rng = np.random.default_rng([seed, L])
    a = np.poly([0.97 * np.exp(0.5j), 0.97 * np.exp(-0.5j), 0.9 * np.exp(2.0j), 0.9 * np.exp(-2.0j)]).real
    e = level * lfilter([1.0], a, rng.normal(size=L))
    if silent is not None:
        e[silent[0]:silent[1]] = 0.0
    return e


def silent_stretch(H):
    """[2.5 H, 7.5 H): the whole window of frame 5 (frames 4 and 5 at H = 1) and parts of its neighbours'."""
    return 2 * H + H // 2, 7 * H + H // 2


def expected_silent(H, L, stretch):
    """bool[Nf]: frames whose whole window [mH - 2H, mH + 2H), as far as it lies inside the signal, lies in `stretch`."""
    Nf = (L - 1) // H + 1
    lo, hi = stretch if stretch is not None else (0, 0)
    out = np.zeros(Nf, dtype=bool)
    for m in range(Nf):
        a, b = max(0, m * H - 2 * H), min(L, m * H + 2 * H)
        out[m] = lo <= a and b <= hi
    return out


# ---- analysis
def short_lengths(H):
    """Frame counts 1, 1, 2, 3, 4, 5, 10: below, at and above the four waves of a block."""
    return _unique([1, H, H + 1, 2 * H + 1, 3 * H + 1, 4 * H + 1, 10 * H])


def analysis_cases():
    """Every shape at L = 9H + 1 with the silent stretch; LENGTH_SHAPES also at the short lengths, without one."""
    cases = []
    for H, p in SHAPES:
        L = 9 * H + 1
        st = silent_stretch(H)
        cases.append(dict(name="H%d_p%d_L%d" % (H, p, L), H=H, p=p, L=L, stretch=st, e=residual(L, 1000 * H + p, st)))
        if (H, p) in LENGTH_SHAPES:
            for L in short_lengths(H):
                cases.append(dict(name="H%d_p%d_L%d" % (H, p, L), H=H, p=p, L=L, stretch=None,
                                  e=residual(L, 1000 * H + p)))
    return cases


_CACHE = {}


def _once(kind, case, make):
    key = (kind, case["name"])
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _pair(ref, ref_l, scale=1.0):
    return float(np.abs(ref - ref_l).max() / scale) if np.size(ref) else 0.0


def analysis_models(case):
    """dict(sigma, refl, stop, sigma_l, refl_l, stop_l, smax, dev_k, dev_s): sigma relative to the largest sigma."""
    def make():
        sg, k, stop = N.analyse(case["e"], case["H"], case["p"])
        sg_l, k_l, stop_l = N.analyse(case["e"], case["H"], case["p"], np.longdouble)
        smax = float(sg.max())
        return dict(sigma=sg, refl=k, stop=stop, sigma_l=sg_l, refl_l=k_l, stop_l=stop_l, smax=smax,
                    dev_k=_pair(k, k_l), dev_s=_pair(sg, sg_l, smax))
    return _once("analysis", case, make)


# ---- synthesis
def noise_model(sigma, refl, H):
    """The dict layout of eaQHMNoiseAnalysis around (sigma, refl)."""
    return NC.noise_model(sigma, refl, hop=H, fs=FS)


def synthesis_model(H, p):
    """(sigma[10], refl[10, p]): pole frames inside r = 0.9, frame 1 silent (the short outputs blend into it)."""
    sigma, refl, _ = NC.pole_frames(10, p, 0.9, seed=H, silent=(1,))
    return sigma, refl


def output_lengths(H):
    """Nq = 1, 1, 2, 64, 65 around the filter kernel's 64 lanes; the two large hops at Nq = 1 and 3."""
    return _unique([1, H, H + 1, 63 * H + 1, 64 * H + 1] if H <= 64 else [H, 2 * H + 1])


def time_maps(H, L_out):
    """(name, tau[Nq]): rho 1, 0.37 (most frames past the model's last one, held) and 2.9, and tau = 0; maps that
    coincide (Nq = 1) are listed once.  Up to hop 64 also "far", rho = 1 moved 10^6 frames past the model's end: with
    both blended frames the last one, only there does a blend fraction that is not capped at 1 show, as the rounding
    of (1 - fr) x + fr x (the models of the two large hops cost seconds per call and keep to the four maps)."""
    Nq = (L_out - 1) // H + 1
    maps = [("rho%g" % rho, N.time_map(H, L_out, rho)) for rho in (1.0, 0.37, 2.9)] + [("tau0", np.zeros(Nq))]
    if H <= 64:
        maps.append(("far", N.time_map(H, L_out, 1.0) + 1e6 * H))
    out = []
    for name, tau in maps:
        if not any(np.array_equal(tau, t) for _, t in out):
            out.append((name, tau))
    return out


def synthesis_cases(shapes=None):
    cases = []
    for H, p in (SHAPES if shapes is None else shapes):
        sigma, refl = synthesis_model(H, p)
        for L_out in output_lengths(H):
            for name, tau in time_maps(H, L_out):
                cases.append(dict(name="H%d_p%d_Lout%d_%s" % (H, p, L_out, name), H=H, p=p, L_out=L_out, tau=tau,
                                  Nq=len(tau), sigma=sigma, refl=refl))
    return cases


def synthesis_models(case):
    """dict(out, out_l, top, dev): relative to the output's maximum."""
    def make():
        args = (case["sigma"], case["refl"], case["H"], case["tau"], case["L_out"], SEED)
        ref, ref_l = N.synth(*args), N.synth(*args, np.longdouble)
        top = float(np.abs(ref).max())
        return dict(out=ref, out_l=ref_l, top=top, dev=_pair(ref, ref_l, top))
    return _once("synthesis", case, make)


# ---- warp and envelope
WARP_ORDERS = [1, 2, 31, 32, 62, 63]
WARP_COUNTS = [1, 3, 4, 5, 7, 8, 9, 37]     # around the 4 waves of an envelope block and the 8 of a warp block
ENVELOPE_SIZES = [1, 63, 64, 65]
MAP_SIZES = [2, 16]


def warp_pairs():
    """(p, Nf): every count at the largest and smallest order, the other orders at 9 frames."""
    return [(63, c) for c in WARP_COUNTS] + [(1, c) for c in WARP_COUNTS] + [(p, 9) for p in (2, 31, 32, 62)]


def warp_model(p, Nf):
    """(sigma[Nf], refl[Nf, p]) with silent frames first, in the middle and last (first and last at 4 frames, the first
    at 3, none in a model of one frame: every model keeps a frame that `alphas`' ramp warps)."""
    silent = (0, Nf // 2, Nf - 1) if Nf >= 5 else (0, Nf - 1) if Nf == 4 else (0,) if Nf == 3 else ()
    sigma, refl, _ = NC.pole_frames(Nf, p, 0.9, seed=3, silent=silent)
    return sigma, refl


def alphas(Nf):
    """(name, alpha[Nf]): three constants and a ramp 0.7 .. 1.6 with exact 1.0 at frames 1, 4, 7, .."""
    mixed = np.linspace(0.7, 1.6, Nf)
    mixed[1::3] = 1.0
    return [("0.5", np.full(Nf, 0.5)), ("0.999", np.full(Nf, 0.999)), ("2", np.full(Nf, 2.0)), ("mixed", mixed)]


def warp_cases():
    cases = []
    for p, Nf in warp_pairs():
        sigma, refl = warp_model(p, Nf)
        for name, alpha in alphas(Nf):
            cases.append(dict(name="p%d_Nf%d_alpha%s" % (p, Nf, name), p=p, Nf=Nf, alpha=alpha, sigma=sigma, refl=refl))
    return cases


def warp_models(case):
    """dict(sigma, refl, stop, sigma_l, refl_l, stop_l, smax, dev_k, dev_s) of the scale warp."""
    def make():
        sg, k, stop = W.warp(case["sigma"], case["refl"], case["alpha"])
        sg_l, k_l, stop_l = W.warp(case["sigma"], case["refl"], case["alpha"], np.longdouble)
        smax = float(case["sigma"].max())
        return dict(sigma=sg, refl=k, stop=stop, sigma_l=sg_l, refl_l=k_l, stop_l=stop_l, smax=smax,
                    dev_k=_pair(k, k_l), dev_s=_pair(sg, sg_l, smax))
    return _once("warp", case, make)


def envelope_freqs(F):
    """F frequencies in Hz from 0 to fs/2, both included; fs/2 alone for F = 1."""
    return np.array([FS / 2]) if F == 1 else np.linspace(0.0, FS / 2, F)


def envelope_cases():
    return [dict(c, name="%s_F%d" % (c["name"], F), F=F, freqs=envelope_freqs(F)) for c in warp_cases()
            for F in ENVELOPE_SIZES]


def _finite_dev(ref, ref_l):
    fin = np.isfinite(ref)
    return float(np.abs(ref[fin] - ref_l[fin]).max()) if fin.any() else 0.0


def envelope_models(case):
    """dict(out, out_l, dev): the deviation over the finite entries (rows of silent frames are -inf)."""
    def make():
        args = (case["sigma"], case["refl"], case["alpha"], case["freqs"] / FS)
        ref, ref_l = W.envelope(*args), W.envelope(*args, np.longdouble)
        return dict(out=ref, out_l=ref_l, dev=_finite_dev(ref, ref_l))
    return _once("envelope", case, make)


def warp_map(Nf, B):
    """(f_in[B], f_out[Nf, B]) in Hz with row Nf // 3 the identity (f_in bit for bit).  B = 2: a knee at 0.7 fs/2 moved
    by 0.8 .. 1.16 over the rows and (fs/2, fs/2); B = 16: breakpoints every fs/32 moved by -15 .. +12 % in mid-band."""
    nyq = FS / 2
    u = np.linspace(-1.0, 0.8, Nf)[:, None] if Nf > 1 else np.array([[1.0]])      # no row but Nf // 3 is the identity
    if B == 2:
        x = np.array([0.7 * nyq, nyq])
        y = np.concatenate(((1.0 + 0.2 * u) * x[0], np.full((Nf, 1), nyq)), axis=1)
    else:
        j = np.arange(1, B + 1)
        x = nyq * j / B
        y = x * (1.0 + 0.15 * u * np.sin(np.pi * j / B))
        y[:, -1] = nyq
    y[Nf // 3] = x
    return x, np.ascontiguousarray(y)


def map_cases():
    """Warp and envelope under the piecewise-linear map: B in {2, 16} at p in {1, 63}, 9 frames."""
    cases = []
    for p in (1, 63):
        sigma, refl = warp_model(p, 9)
        for B in MAP_SIZES:
            x, y = warp_map(9, B)
            cases.append(dict(name="p%d_Nf9_B%d" % (p, B), p=p, Nf=9, B=B, x=x, y=y, identity=3, sigma=sigma, refl=refl))
    return cases


def map_models(case):
    """The scale warp's dict for the map (formant_warp_ref.noise_warp)."""
    def make():
        args = (case["sigma"], case["refl"], case["x"] / FS, case["y"] / FS)
        sg, k, stop = FW.noise_warp(*args)
        sg_l, k_l, stop_l = FW.noise_warp(*args, np.longdouble)
        smax = float(case["sigma"].max())
        return dict(sigma=sg, refl=k, stop=stop, sigma_l=sg_l, refl_l=k_l, stop_l=stop_l, smax=smax,
                    dev_k=_pair(k, k_l), dev_s=_pair(sg, sg_l, smax))
    return _once("map", case, make)


def map_envelope_models(case, F):
    def make():
        args = (case["sigma"], case["refl"], case["x"] / FS, case["y"] / FS, envelope_freqs(F) / FS)
        ref, ref_l = FW.noise_envelope(*args), FW.noise_envelope(*args, np.longdouble)
        return dict(out=ref, out_l=ref_l, dev=_finite_dev(ref, ref_l))
    return _once("map_envelope_F%d" % F, case, make)


# ---- modulation
MOD_HOPS = [1, 15, 17, 64, 1024]
MOD_HARMONICS = [1, 8]
MOD_COUNTS = [1, 3, 4, 5, 10]


def modulation_inputs(H, count):
    """dict(e, L, theta, f0, voiced, ti0, D, n) for `count` frames at hop H: instants D = 0.8 H apart from ti0 = -0.7 D
    (no frame centre and no sample half-way between two instants), random phases, f0 in 100 .. 300 Hz; unvoiced are
    the first and the last instant and, from 3 frames on, the instant nearest to the last frame.  Frame 0's nearest
    instant (1) is voiced.  Ten frames carry the analysis cases' silent stretch."""
    L = (count - 1) * H + 1
    D = 0.8 * H
    ti0 = -0.7 * D
    n = int(np.ceil(((count - 1) * H - ti0) / D)) + 2
    rng = np.random.default_rng([H, count])
    voiced = np.ones(n, dtype=bool)
    voiced[0] = voiced[-1] = False
    if count >= 3:
        voiced[R.nearest((count - 1) * H, ti0, D, n)] = False
    return dict(e=residual(L, 7000 + H, silent_stretch(H) if count == 10 else None), L=L, theta=rng.uniform(0, 1, n),
                f0=rng.uniform(100.0, 300.0, n), voiced=voiced, ti0=ti0, D=D, n=n)


def modulation_cases():
    cases = []
    for H in MOD_HOPS:
        for count in MOD_COUNTS:
            inp = modulation_inputs(H, count)
            for M in MOD_HARMONICS:
                cases.append(dict(inp, name="H%d_Nf%d_M%d" % (H, count, M), H=H, Nf=count, M=M))
    return cases


def modulation_models(case):
    """dict(mod, mod_l, dev)."""
    def make():
        args = (case["e"], case["H"], case["M"], case["theta"], case["f0"], case["voiced"], case["ti0"], case["D"], FS)
        ref, ref_l = R.analyse(*args), R.analyse(*args, np.longdouble)
        return dict(mod=ref, mod_l=ref_l, dev=_pair(ref, ref_l))
    return _once("modulation", case, make)


# ---- modulated cross-fade
CROSSFADE_SHAPES = [(2, 7), (16, 63), (64, 33)]
CROSSFADE_COUNTS = [1, 64, 65]


def crossfade_cases():
    """The synthesis model of the shape with hand-built coefficients (|c| up to 0.3 / M, zero on the silent frame),
    theta in [0, 1) and nu in 0.005 .. 0.03 cycles per sample per output frame, under the time map rho = 2.9."""
    cases = []
    for H, p in CROSSFADE_SHAPES:
        sigma, refl = synthesis_model(H, p)
        for Nq in CROSSFADE_COUNTS:
            L_out = H if Nq == 1 else (Nq - 1) * H + 1
            tau = N.time_map(H, L_out, 2.9)
            for M in MOD_HARMONICS:
                rng = np.random.default_rng([H, Nq, M])
                mod = rng.uniform(-0.3 / M, 0.3 / M, (len(sigma), 2 * M))
                mod[sigma == 0] = 0.0
                cases.append(dict(name="H%d_p%d_Nq%d_M%d" % (H, p, Nq, M), H=H, p=p, L_out=L_out, tau=tau, Nq=Nq, M=M,
                                  sigma=sigma, refl=refl, mod=mod, theta=rng.uniform(0, 1, Nq),
                                  nu=rng.uniform(0.005, 0.03, Nq)))
    return cases


def crossfade_models(case):
    """dict(out, out_l, top, dev): relative to the output's maximum."""
    def make():
        args = (case["sigma"], case["refl"], case["H"], case["tau"], case["L_out"], SEED, case["mod"], case["theta"],
                case["nu"])
        ref, ref_l = R.synth_mod(*args), R.synth_mod(*args, np.longdouble)
        top = float(np.abs(ref).max())
        return dict(out=ref, out_l=ref_l, top=top, dev=_pair(ref, ref_l, top))
    return _once("crossfade", case, make)


# ---- the stop path of the analysis
STOP_SHAPE = (16, 8)
STOP_AT = 70                   # samples 70 and 71: inside the windows of frames 3, 4, 5, 6 and of no other


def stop_path_inputs():
    """dict(clean, huge, nan, covered): a residual of 10 frames at STOP_SHAPE, the same with samples 70 and 71 at
    1e200 (r[0] and r[1] overflow: k_1 = -inf / inf is not below 1 in magnitude, the recursion stops at stage 1 with
    E = inf) and with sample 70 NaN (r[0] > 0 is false: a silent frame); covered = bool[Nf], the frames whose window
    holds the samples."""
    H, _ = STOP_SHAPE
    L = 9 * H + 1
    clean = residual(L, 99)
    huge, nan = clean.copy(), clean.copy()
    huge[STOP_AT:STOP_AT + 2] = 1e200
    nan[STOP_AT] = np.nan
    m = np.arange((L - 1) // H + 1)
    covered = (m * H - 2 * H <= STOP_AT) & (STOP_AT + 1 < m * H + 2 * H)
    return dict(clean=clean, huge=huge, nan=nan, covered=covered)
