"""The cases of tests/noise_direct_cases.py are fit to judge the noise kernels (csrc/eaqhm_noise.hip), shown with the
NumPy models alone: every case has a non-zero yardstick (the deviation between the model in float64 and in
np.longdouble, from which tests/test_gpu_noise_direct.py takes its bars), no frame of any case stops its
Levinson-Durbin recursion early in either precision (so the GPU test excludes nothing), the silent frames are the ones
the construction says, and each of eleven deliberate errors, written here as variants of the models, moves at least one
case by more than 100 x that case's yardstick.

What the yardsticks came to here (float64 vs longdouble): analysis k 8.4e-18 .. 2.1e-14 and sigma / max sigma
1.4e-17 .. 1.5e-14; synthesis 9.1e-18 .. 1.2e-15 of the output's maximum; scale warp k' 9.3e-18 .. 2.2e-10; envelope
3.3e-16 .. 1.5e-12; modulation 3.1e-17 .. 1.0e-14; modulated cross-fade 6.9e-17 .. 9.5e-16.  max |k'| after the warp
is 0.986."""
import numpy as np
import pytest

import noise_direct_cases as C
import noise_model_ref as N
import noise_modulation_ref as R


@pytest.fixture(scope="module", autouse=True)
def _quiet():
    with np.errstate(all="ignore"):
        yield


# ---- the yardsticks are non-zero, nothing stops, the silent frames are the constructed ones
def test_case_tables_hold_every_shape_length_and_count():
    an = C.analysis_cases()
    assert len({c["name"] for c in an}) == len(an)
    assert {(c["H"], c["p"]) for c in an} == set(C.SHAPES) and len(C.SHAPES) == 12
    for H, p in C.SHAPES:
        Ls = sorted(c["L"] for c in an if (c["H"], c["p"]) == (H, p))
        want = {9 * H + 1} | ({1, H, H + 1, 2 * H + 1, 3 * H + 1, 4 * H + 1, 10 * H} if (H, p) in C.LENGTH_SHAPES else set())
        assert Ls == sorted(want), (H, p)
    assert sorted({(c["L"] - 1) // c["H"] + 1 for c in an if (c["H"], c["p"]) == (1024, 63)}) == [1, 2, 3, 4, 5, 10]
    sy = C.synthesis_cases()
    assert len({c["name"] for c in sy}) == len(sy)
    for H, p in C.SHAPES:
        nq = sorted({c["Nq"] for c in sy if (c["H"], c["p"]) == (H, p)})
        assert nq == ([1, 2, 64, 65] if H <= 64 else [1, 3]), (H, p)
        names = {c["name"].rsplit("_", 1)[1] for c in sy if (c["H"], c["p"]) == (H, p) and c["Nq"] > 1}
        assert names == {"rho1", "rho0.37", "rho2.9", "tau0"} | ({"far"} if H <= 64 else set())
    held = [c for c in sy if c["name"].endswith("rho0.37") and c["Nq"] >= 64]
    assert held and all(np.mean(c["tau"] / c["H"] > 9) > 0.9 for c in held)        # past the model's last frame
    assert all(len(c["sigma"]) == 10 and np.count_nonzero(c["sigma"] == 0) == 1 for c in sy)
    wp = C.warp_pairs()
    assert {p for p, _ in wp} == set(C.WARP_ORDERS) and {n for p, n in wp if p in (1, 63)} == set(C.WARP_COUNTS)
    assert all(n == 9 for p, n in wp if p not in (1, 63))
    for c in C.warp_cases():
        if c["name"].endswith("mixed") and c["Nf"] >= 3:
            unit = c["alpha"] == 1.0
            assert (unit & (c["sigma"] > 0)).any() and (~unit & (c["sigma"] > 0)).any(), c["name"]
        if c["Nf"] >= 5:
            assert c["sigma"][0] == c["sigma"][c["Nf"] // 2] == c["sigma"][-1] == 0
    for c in C.map_cases():
        assert np.array_equal(c["y"][c["identity"]], c["x"]) and c["sigma"][c["identity"]] > 0
        assert sum(np.array_equal(row, c["x"]) for row in c["y"]) == 1
    for F in C.ENVELOPE_SIZES:
        f = C.envelope_freqs(F)
        assert len(f) == F and f[-1] == C.FS / 2 and (F == 1 or f[0] == 0.0)
    mo = C.modulation_cases()
    assert {(c["H"], c["M"], c["Nf"]) for c in mo} == {(H, M, n) for H in C.MOD_HOPS for M in C.MOD_HARMONICS
                                                        for n in C.MOD_COUNTS}
    assert all(not c["voiced"][0] and not c["voiced"][-1] and c["voiced"].any() for c in mo)
    xf = C.crossfade_cases()
    assert {(c["H"], c["p"], c["Nq"], c["M"]) for c in xf} == {(H, p, n, M) for H, p in C.CROSSFADE_SHAPES
                                                               for n in C.CROSSFADE_COUNTS for M in C.MOD_HARMONICS}


def test_analysis_yardsticks_stops_and_silent_frames():
    devs_k, devs_s = [], []
    for c in C.analysis_cases():
        m = C.analysis_models(c)
        assert not m["stop"].any() and not m["stop_l"].any(), c["name"]
        silent = C.expected_silent(c["H"], c["L"], c["stretch"])
        assert np.array_equal(m["sigma"] == 0, silent) and np.array_equal(m["sigma_l"] == 0, silent), c["name"]
        if c["stretch"] is not None:       # one whole window at least, and two that the stretch cuts through
            lo, hi = c["stretch"]
            cut = [mm for mm in range(len(silent)) if not silent[mm]
                   and max(0, mm * c["H"] - 2 * c["H"]) < hi and min(c["L"], mm * c["H"] + 2 * c["H"]) > lo]
            assert silent.any() and len(cut) >= 2, c["name"]
            assert np.all(m["refl"][silent] == 0)
        assert m["dev_s"] > 0, c["name"]
        if c["L"] == 1:
            # the one exception: every lag but r[0] is exactly zero, so every k is exactly zero in any arithmetic
            assert np.all(m["refl"] == 0) and np.all(m["refl_l"] == 0) and m["dev_k"] == 0
        else:
            assert m["dev_k"] > 0, c["name"]
            devs_k.append(m["dev_k"])
        devs_s.append(m["dev_s"])
    print("analysis yardsticks: k %.3g .. %.3g, sigma %.3g .. %.3g" % (min(devs_k), max(devs_k), min(devs_s), max(devs_s)))


@pytest.mark.slow
def test_synthesis_yardsticks():
    devs = []
    for c in C.synthesis_cases():
        m = C.synthesis_models(c)
        assert m["top"] > 0 and m["dev"] > 0, c["name"]
        devs.append(m["dev"])
    for c in C.crossfade_cases():
        m = C.crossfade_models(c)
        assert m["top"] > 0 and m["dev"] > 0, c["name"]
        plain = N.synth(c["sigma"], c["refl"], c["H"], c["tau"], c["L_out"], C.SEED)
        assert np.abs(m["out"] - plain).max() > 1e-3 * m["top"], c["name"]       # the modulation moves the signal
    print("synthesis yardsticks: %.3g .. %.3g" % (min(devs), max(devs)))


@pytest.mark.slow
def test_warp_envelope_and_map_yardsticks_and_stops():
    devs, kmax = [], 0.0
    for c in C.warp_cases():
        m = C.warp_models(c)
        assert not m["stop"].any() and not m["stop_l"].any(), c["name"]
        assert m["dev_k"] > 0 and m["dev_s"] > 0, c["name"]
        unit = (c["alpha"] == 1.0) | (c["sigma"] == 0)
        assert np.array_equal(m["refl"][c["alpha"] == 1.0], c["refl"][c["alpha"] == 1.0])
        gone = (c["sigma"] == 0) & (c["alpha"] != 1.0)       # a silent frame under a unit alpha keeps its k
        assert np.all(m["sigma"][c["sigma"] == 0] == 0) and np.all(m["refl"][gone] == 0)
        assert np.all(m["sigma"][~unit] != c["sigma"][~unit]), c["name"]
        devs.append(m["dev_k"])
        kmax = max(kmax, float(np.abs(m["refl"]).max()))
    for c in C.map_cases():
        m = C.map_models(c)
        assert not m["stop"].any() and not m["stop_l"].any(), c["name"]
        assert m["dev_k"] > 0 and m["dev_s"] > 0, c["name"]
        assert np.array_equal(m["refl"][c["identity"]], c["refl"][c["identity"]])
        for F in C.ENVELOPE_SIZES:
            assert C.map_envelope_models(c, F)["dev"] > 0, (c["name"], F)
    for c in C.envelope_cases():
        m = C.envelope_models(c)
        assert m["dev"] > 0, c["name"]
        assert np.array_equal(np.isfinite(m["out"]).all(axis=1), c["sigma"] > 0)
    print("warp yardsticks: k' %.3g .. %.3g, max |k'| %.4f" % (min(devs), max(devs), kmax))
    assert kmax < 1


def test_modulation_yardsticks_and_zero_rows():
    for c in C.modulation_cases():
        m = C.modulation_models(c)
        assert m["dev"] > 0, c["name"]
        zero = np.all(m["mod"] == 0, axis=1)
        assert np.array_equal(zero, np.all(m["mod_l"] == 0, axis=1)), c["name"]
        unvoiced = ~c["voiced"][R.nearest(np.arange(c["Nf"]) * c["H"], c["ti0"], c["D"], c["n"])]
        silent = C.expected_silent(c["H"], c["L"], C.silent_stretch(c["H"]) if c["Nf"] == 10 else None)
        assert np.array_equal(zero, unvoiced | silent), c["name"]
        assert not zero[0] and (c["Nf"] < 3 or zero[-1]), c["name"]
        if c["Nf"] == 10:
            assert (silent & ~unvoiced).any(), c["name"]


def test_stop_path_inputs_in_the_model():
    """What no finite input reaches: two overflowing samples stop the recursion at stage 1 in exactly the frames that
    hold them (all k zero, sigma = +inf); a NaN makes those frames silent; the other frames are the clean call's."""
    H, p = C.STOP_SHAPE
    s = C.stop_path_inputs()
    cov = s["covered"]
    assert np.flatnonzero(cov).tolist() == [3, 4, 5, 6]
    sg0, k0, stop0 = N.analyse(s["clean"], H, p)
    assert not stop0.any() and np.all(sg0 > 0)
    sg, k, stop = N.analyse(s["huge"], H, p)
    assert np.array_equal(stop, np.where(cov, 1, 0)) and np.array_equal(N.stop_stage(sg, k), stop)
    assert np.all(np.isposinf(sg[cov])) and np.all(k[cov] == 0)
    assert np.array_equal(sg[~cov], sg0[~cov]) and np.array_equal(k[~cov], k0[~cov])
    sg, k, stop = N.analyse(s["nan"], H, p)
    assert not stop.any() and np.all(sg[cov] == 0) and np.all(k[cov] == 0)
    assert np.array_equal(sg[~cov], sg0[~cov]) and np.array_equal(k[~cov], k0[~cov])


# ---- the deliberate errors
def _analyse_variant(e, H, p, half=0.5, shift=0, drop_last=False, inflate=True):
    """noise_model_ref.analyse with switches: the window's half-sample offset, the frame start mH - 2H + shift, the
    highest lag, the inflation of r[0]."""
    e = np.asarray(e, dtype=np.float64)
    L, W = len(e), 4 * H
    w = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(W) + half) / W)
    Nf = (L - 1) // H + 1
    pad = np.concatenate((np.zeros(2 * H), e, np.zeros(3 * H + 1)))
    sigma, refl = np.zeros(Nf), np.zeros((Nf, p))
    sw2 = (w * w).sum()
    for m in range(Nf):
        x = w * pad[m * H + shift: m * H + shift + W]
        r = np.array([np.dot(x[l:], x[:W - l]) for l in range(p + 1)])
        if not r[0] > 0:
            continue
        if inflate:
            r[0] = r[0] * (1 + 1e-9)
        a = np.zeros(p + 1)
        a[0] = 1
        E = r[0]
        for i in range(1, p + (0 if drop_last else 1)):
            k = -(r[i] + np.dot(a[1:i], r[i - 1:0:-1])) / E
            assert abs(k) < 1
            a[1:i] = a[1:i] + k * a[i - 1:0:-1]
            a[i] = k
            E = E * (1 - k * k)
            refl[m, i - 1] = k
        sigma[m] = np.sqrt(E / sw2)
    return sigma, refl


def _synth_variant(sigma, refl, H, tau, L_out, seed, hold=True, cap=True, shift=0, extra_fade=False, warm=True):
    """noise_model_ref.synth with switches: frames past the model's last one held or zero, the blend fraction capped at
    1 or not, the excitation index n + shift, the fade-in of a frame Nq added or not, the 2H warm-up samples of the
    lattice run or skipped."""
    Nq = (L_out - 1) // H + 1
    if extra_fade:
        tau = np.concatenate((tau, tau[-1:]))
    nq, p, Nf = len(tau), np.shape(refl)[1], len(sigma)
    mu = np.asarray(tau, dtype=np.float64) / H
    m0 = np.minimum(np.floor(mu).astype(np.int64), Nf - 1)
    m1 = np.minimum(m0 + 1, Nf - 1)
    fr = mu - m0
    if cap:
        fr = np.minimum(fr, 1.0)
    sg = (1 - fr) * sigma[m0] + fr * sigma[m1]
    k = (1 - fr)[:, None] * refl[m0] + fr[:, None] * refl[m1]
    if not hold:
        sg = np.where(mu > Nf - 1, 0.0, sg)
        k = np.where((mu > Nf - 1)[:, None], 0.0, k)
    v = N.synthesis_window(H)
    b = np.zeros((p + 1, nq))
    y = np.zeros((2 * H, nq))
    qH = np.arange(nq, dtype=np.int64) * H
    for t in range(0 if warm else 2 * H, 4 * H):
        f = sg * N.white(seed, qH - 3 * H + t + shift)
        for i in range(p, 0, -1):
            f = f - k[:, i - 1] * b[i - 1]
            b[i] = b[i - 1] + k[:, i - 1] * f
        b[0] = f
        if t >= 2 * H:
            y[t - 2 * H] = f
    out = np.zeros(L_out)
    for q in range(nq):
        n = q * H - H + np.arange(2 * H)
        ok = (n >= 0) & (n < L_out)
        out[n[ok]] += (v * y[:, q])[ok]
    assert nq == Nq + int(extra_fade)
    return out


def _modulation_variant(c, floor=False, harmonic_shift=False):
    """noise_modulation_ref.analyse with switches: the instant by floor instead of nearest, harmonic j where j + 1
    belongs (coefficient 1 then reads e^0)."""
    e, H, M, D, ti0, n = c["e"], c["H"], c["M"], c["D"], c["ti0"], c["n"]

    def instant(x):
        r = (np.asarray(x, dtype=np.float64) - ti0) / D
        return np.clip(np.floor(r) if floor else np.rint(r), 0, n - 1).astype(np.int64)

    L, W = len(e), 4 * H
    v = np.arange(W)
    w = 0.5 - 0.5 * np.cos(np.pi * ((2 * v + 1) / float(W)))
    pad = np.concatenate((np.zeros(2 * H), e, np.zeros(3 * H)))
    mod = np.zeros((c["Nf"], 2 * M))
    for m in range(c["Nf"]):
        if not c["voiced"][instant(m * H)]:
            continue
        x = w * pad[m * H: m * H + W]
        u = x * x
        P = R._wave_sum(u)
        if not P > 0:
            continue
        pos = (m * H - 2 * H + v).astype(np.float64)
        i = instant(pos)
        cs, sn = R.harmonics_of(c["theta"][i] + c["f0"][i] * (pos - (ti0 + i * D)) / C.FS, M + 1)
        if harmonic_shift:
            cs, sn = np.concatenate((np.ones((1, W)), cs[:-1])), np.concatenate((np.zeros((1, W)), sn[:-1]))
        mod[m, 0::2] = R._wave_sum(u * cs[:M]) / P
        mod[m, 1::2] = -R._wave_sum(u * sn[:M]) / P
    return mod


def _worst(rows):
    """rows of (case name, difference, yardstick): the largest difference in units of 100 yardsticks and its case."""
    ratio, name = max((d / (100 * y), nm) for nm, d, y in rows if y > 0)
    return ratio, name


def test_variants_without_an_error_are_the_models():
    for c in C.analysis_cases():
        m = C.analysis_models(c)
        sg, k = _analyse_variant(c["e"], c["H"], c["p"])
        assert np.array_equal(sg, m["sigma"]) and np.array_equal(k, m["refl"]), c["name"]
    for c in C.synthesis_cases(C.SHAPES[:6]):
        got = _synth_variant(c["sigma"], c["refl"], c["H"], c["tau"], c["L_out"], C.SEED)
        assert np.array_equal(got, C.synthesis_models(c)["out"]), c["name"]
    for c in C.modulation_cases():
        assert np.array_equal(_modulation_variant(c), C.modulation_models(c)["mod"]), c["name"]


ANALYSIS_ERRORS = {"window without the half-sample offset": dict(half=0.0), "frame start at mH - 2H + 1": dict(shift=1),
                   "highest lag dropped": dict(drop_last=True), "r[0] not inflated": dict(inflate=False)}


@pytest.mark.parametrize("error", sorted(ANALYSIS_ERRORS))
def test_analysis_cases_notice(error):
    rows = []
    for c in C.analysis_cases():
        m = C.analysis_models(c)
        sg, k = _analyse_variant(c["e"], c["H"], c["p"], **ANALYSIS_ERRORS[error])
        rows.append((c["name"] + " k", float(np.abs(k - m["refl"]).max()), m["dev_k"]))
        rows.append((c["name"] + " sigma", float(np.abs(sg - m["sigma"]).max() / m["smax"]), m["dev_s"]))
    ratio, name = _worst(rows)
    print("%s: %s moves by %.3g x its bar" % (error, name, ratio))
    assert ratio > 1, "%s: no analysis case notices it; the nearest is %s at %.3g of its bar" % (error, name, ratio)


SYNTHESIS_ERRORS = {"frames past the last model frame zero instead of held": dict(hold=False),
                    "blend fraction not capped at 1": dict(cap=False), "excitation index off by one": dict(shift=1),
                    "fade-in of frame q + 1 added when q + 1 == Nq": dict(extra_fade=True),
                    "the 2H warm-up samples of the lattice skipped": dict(warm=False)}


@pytest.mark.parametrize("error", sorted(SYNTHESIS_ERRORS))
def test_synthesis_cases_notice(error):
    rows = []
    for c in C.synthesis_cases(C.SHAPES[:6]):          # the shapes up to (16, 63): the models of the others cost seconds
        m = C.synthesis_models(c)
        got = _synth_variant(c["sigma"], c["refl"], c["H"], c["tau"], c["L_out"], C.SEED, **SYNTHESIS_ERRORS[error])
        rows.append((c["name"], float(np.abs(got - m["out"]).max() / m["top"]), m["dev"]))
    ratio, name = _worst(rows)
    print("%s: %s moves by %.3g x its bar" % (error, name, ratio))
    assert ratio > 1, "%s: no synthesis case notices it; the nearest is %s at %.3g of its bar" % (error, name, ratio)


MODULATION_ERRORS = {"instant by floor instead of nearest": dict(floor=True),
                     "harmonic j read where j + 1 belongs": dict(harmonic_shift=True)}


@pytest.mark.parametrize("error", sorted(MODULATION_ERRORS))
def test_modulation_cases_notice(error):
    rows = []
    for c in C.modulation_cases():
        m = C.modulation_models(c)
        got = _modulation_variant(c, **MODULATION_ERRORS[error])
        rows.append((c["name"], float(np.abs(got - m["mod"]).max()), m["dev"]))
    ratio, name = _worst(rows)
    print("%s: %s moves by %.3g x its bar" % (error, name, ratio))
    assert ratio > 1, "%s: no modulation case notices it; the nearest is %s at %.3g of its bar" % (error, name, ratio)
