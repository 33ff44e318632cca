"""The noise kernels of csrc/eaqhm_noise.hip on the MI355X, directly, at every hop, order and count edge: the cases of
tests/noise_direct_cases.py (tests/test_noise_direct_cases_cpu.py shows that they can judge a kernel) through
eaQHMNoiseAnalysis(order=, hop=), eaQHMNoiseSynthesis, eaQHMNoiseWarp and noise_envelope, and through the context's raw
entry points where the Python layer would get in the way (the modulation, accumulate, non-finite input).

Bars: DESIGN.md §10's rule.  A kernel is held to 100 x the largest deviation between the NumPy model in float64 and in
np.longdouble on the same case, computed when the test runs; sigma relative to the case's largest sigma, synthesis
relative to the output's maximum.  There is no fixed tolerance here and no frame is excluded: no frame of any case
stops its recursion early in either precision (the CPU test), and none may on the device.  Every comparison records
both figures (record_measurement "noise_direct_..."); the largest ratio per kernel is tabulated in DESIGN.md §10.

Measured on the MI355X, the largest kernel error in units of the case's yardstick: analysis k 10.0 (H 2, p 7, L 2),
sigma 25.8 (H 16, p 63, L 16); synthesis 0.59; modulated cross-fade 0.25; scale warp k' 29.6, sigma' 19.7; map warp k'
6.0, sigma' 5.8; envelope 2.5 (map 1.4); modulation 3.3.  The scale warp at alpha = 0.5 first came to 150 (sigma', p 63,
3 frames) and 105 (p 1, 1 frame): its lag sums added the held Nyquist value 128 times running; a frame with a held
stretch is now summed 64 grid points at a time (5.0 and 2.7).

Beside the bars, exact: silent frames give sigma == 0 and k == 0, L = 1 gives k == 0, unit alpha and identity map rows
come back bit for bit, an all-zero mod is the plain synthesis, and a frame, a range or a count does not depend on what
else the call holds (bit for bit, no model)."""
import numpy as np
import pytest

import noise_direct_cases as C
import noise_model_ref as N
from conftest import record_measurement

pytestmark = pytest.mark.gpu


def _id(shape):
    return "H%d_p%d" % shape


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


@pytest.fixture(scope="module")
def ctx(amd):
    from eaqhm_amd.functions import _ctx
    return _ctx(0)


@pytest.fixture(scope="module", autouse=True)
def models():
    """Every case's models in float64 and longdouble, once (about half a minute, most of it the longdouble lattices)."""
    with np.errstate(all="ignore"):
        for cases, make in ((C.analysis_cases(), C.analysis_models), (C.synthesis_cases(), C.synthesis_models),
                            (C.warp_cases(), C.warp_models), (C.envelope_cases(), C.envelope_models),
                            (C.map_cases(), C.map_models), (C.modulation_cases(), C.modulation_models),
                            (C.crossfade_cases(), C.crossfade_models)):
            for c in cases:
                make(c)
        for c in C.map_cases():
            for F in C.ENVELOPE_SIZES:
                C.map_envelope_models(c, F)
        yield


class Bars:
    """The comparisons of one test against their bars: every case is measured and recorded, then all of them must hold."""

    def __init__(self):
        self.missed = []

    def hold(self, name, err, dev):
        if not err <= 100 * dev:
            self.missed.append("%s: gpu err %.3g > 100 x model dev %.3g" % (name, err, dev))

    def check(self):
        assert not self.missed, self.missed


def _dev(ctx, *arrays):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(a), device=ctx.device) for a in arrays]


def _analyse(amd, e, H, p):
    return amd.eaQHMNoiseAnalysis(e, np.zeros(len(e)), C.FS, order=p, hop=H)


# ---- analysis
@pytest.mark.parametrize("shape", C.SHAPES, ids=_id)
def test_analysis_cases(amd, shape):
    bars = Bars()
    for c in [c for c in C.analysis_cases() if (c["H"], c["p"]) == shape]:
        H, p, L = c["H"], c["p"], c["L"]
        m = C.analysis_models(c)
        nz = _analyse(amd, c["e"], H, p)
        Nf = (L - 1) // H + 1
        assert (nz["hop"], nz["order"], nz["fs"], nz["length"]) == (H, p, C.FS, L)
        assert nz["sigma"].shape == (Nf,) and nz["refl"].shape == (Nf, p)
        assert nz["sigma"].dtype == nz["refl"].dtype == np.float64
        silent = C.expected_silent(H, L, c["stretch"])
        err_k = float(np.abs(nz["refl"] - m["refl"]).max())
        err_s = float(np.abs(nz["sigma"] - m["sigma"]).max() / m["smax"])
        print("noise direct analysis %s: frames %d silent %d  k: model dev %.3g gpu err %.3g  sigma: model dev %.3g gpu "
              "err %.3g" % (c["name"], Nf, int(silent.sum()), m["dev_k"], err_k, m["dev_s"], err_s))
        record_measurement("noise_direct_analysis_%s" % c["name"], frames=Nf, silent=int(silent.sum()),
                           model_dev_k=m["dev_k"], gpu_err_k=err_k, model_dev_sigma=m["dev_s"], gpu_err_sigma=err_s)
        assert np.array_equal(nz["sigma"] == 0, silent), c["name"]
        assert np.all(nz["refl"][silent] == 0), c["name"]
        if L == 1:
            assert np.all(nz["refl"] == 0), c["name"]            # every lag but r[0] is exactly zero
        # no frame stops on the device: k is zero from some stage on only where the model's, which ran through, is (a
        # window with one sample in it has no lag but r[0])
        assert np.array_equal(N.stop_stage(nz["sigma"], nz["refl"]), N.stop_stage(m["sigma"], m["refl"])), c["name"]
        bars.hold(c["name"] + " k", err_k, m["dev_k"])
        bars.hold(c["name"] + " sigma", err_s, m["dev_s"])
    bars.check()


@pytest.mark.parametrize("shape", C.LENGTH_SHAPES, ids=_id)
def test_analysis_of_a_prefix_is_the_prefix_of_the_analysis(amd, shape):
    """Frame m of e[:L'] equals frame m of e wherever its window ends inside the prefix (mH + 2H <= L')."""
    H, p = shape
    e = C.residual(10 * H, 5)
    whole = _analyse(amd, e, H, p)
    compared = 0
    for Lp in C.short_lengths(H) + [9 * H + 1]:
        part = _analyse(amd, e[:Lp], H, p)
        same = np.flatnonzero(np.arange(len(part["sigma"])) * H + 2 * H <= Lp)
        assert np.array_equal(part["sigma"][same], whole["sigma"][same]), (shape, Lp)
        assert np.array_equal(part["refl"][same], whole["refl"][same]), (shape, Lp)
        compared += len(same)
    assert compared >= 20


def test_analysis_stop_path(amd, ctx):
    """What the `break` of the recursion leaves behind, through the raw entry point (Python rejects non-finite input;
    no finite input reaches the stop): the float64 model's frames, frame by frame."""
    import torch
    H, p = C.STOP_SHAPE
    s = C.stop_path_inputs()
    cov = s["covered"]
    L = len(s["clean"])
    Nf = len(cov)

    def run(e):
        e_d, = _dev(ctx, e)
        sigma = torch.full((Nf,), 7.0, dtype=torch.float64, device=ctx.device)
        refl = torch.full((Nf, p), 7.0, dtype=torch.float64, device=ctx.device)
        ctx.noise_analyse(e_d, L, H, p, sigma, refl)
        ctx.sync()
        return sigma.cpu().numpy(), refl.cpu().numpy()

    sg0, k0 = run(s["clean"])
    assert np.all(sg0 > 0) and np.all(N.stop_stage(sg0, k0) == 0)
    with np.errstate(all="ignore"):
        ref_h, ref_n = N.analyse(s["huge"], H, p), N.analyse(s["nan"], H, p)
    assert np.array_equal(ref_h[2], np.where(cov, 1, 0)) and not ref_n[2].any() and int(cov.sum()) == 4
    sg, k = run(s["huge"])
    assert np.array_equal(np.isposinf(sg), cov) and np.all(np.isposinf(ref_h[0][cov]))
    assert np.all(k[cov] == 0) and np.all(ref_h[1][cov] == 0)
    assert np.array_equal(N.stop_stage(sg, k), ref_h[2])
    assert np.array_equal(sg[~cov], sg0[~cov]) and np.array_equal(k[~cov], k0[~cov])
    sg, k = run(s["nan"])
    assert np.array_equal(sg == 0, cov) and np.all(ref_n[0][cov] == 0)
    assert np.all(k[cov] == 0) and np.all(ref_n[1][cov] == 0)
    assert np.array_equal(sg[~cov], sg0[~cov]) and np.array_equal(k[~cov], k0[~cov])


# ---- synthesis
@pytest.mark.parametrize("shape", C.SHAPES, ids=_id)
def test_synthesis_cases(amd, shape):
    bars = Bars()
    for c in C.synthesis_cases([shape]):
        m = C.synthesis_models(c)
        nz = C.noise_model(c["sigma"], c["refl"], c["H"])
        out = amd.eaQHMNoiseSynthesis(nz, c["tau"], c["L_out"], seed=C.SEED)
        assert out.shape == (c["L_out"],) and out.dtype == np.float64
        err = float(np.abs(out - m["out"]).max() / m["top"])
        print("noise direct synthesis %s: Nq %d model dev %.3g gpu err %.3g" % (c["name"], c["Nq"], m["dev"], err))
        record_measurement("noise_direct_synthesis_%s" % c["name"], output_frames=c["Nq"], model_dev=m["dev"], gpu_err=err)
        bars.hold(c["name"], err, m["dev"])
    bars.check()


def _range_sets(H, L_out):
    """Range ends inside a frame, on a frame boundary and one sample before it; a split exactly at output frame 64;
    the first and the last sample alone."""
    return [(0, 3 * H + max(H // 2, 1), 40 * H + 1, L_out), (0, 10 * H, 30 * H - 1, L_out), (0, 64 * H, L_out),
            (0, 1, L_out - 1, L_out)]


@pytest.mark.parametrize("shape", C.CROSSFADE_SHAPES, ids=_id)
def test_synthesis_ranges_and_accumulate(amd, ctx, shape):
    H, p = shape
    sigma, refl = C.synthesis_model(H, p)
    nz = C.noise_model(sigma, refl, H)
    L_out = 66 * H + H // 2 + 1
    tau = N.time_map(H, L_out, 2.9)
    Nq = len(tau)
    rng = np.random.default_rng([H, p])
    mod = rng.uniform(-0.04, 0.04, (len(sigma), 16))
    fund = (rng.uniform(0, 1, Nq), rng.uniform(0.005, 0.03, Nq))
    nzm = dict(nz, mod=mod, mod_harmonics=8)
    plain = amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=C.SEED)
    modded = amd.eaQHMNoiseSynthesis(nzm, tau, L_out, seed=C.SEED, fundamental=fund)
    assert not np.array_equal(plain, modded)
    for cuts in _range_sets(H, L_out):
        ranges = list(zip(cuts[:-1], cuts[1:]))
        assert np.array_equal(amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=C.SEED, _ranges=ranges), plain), (shape, cuts)
        assert np.array_equal(amd.eaQHMNoiseSynthesis(nzm, tau, L_out, seed=C.SEED, fundamental=fund, _ranges=ranges),
                              modded), (shape, cuts)
    # accumulate into a buffer that is not zero: one addition per sample
    base = rng.normal(size=L_out)
    sg_d, k_d, tau_d, mod_d, th_d, nu_d = _dev(ctx, sigma, refl, tau, mod, fund[0], fund[1])
    for group, want in ((None, plain), ((mod_d, 8, th_d, nu_d), modded)):
        buf, = _dev(ctx, base.copy())
        for t_lo, t_hi in ((0, 64 * H), (64 * H, L_out)):
            ctx.noise_synth(sg_d, k_d, len(sigma), H, p, tau_d, Nq, C.SEED, L_out, t_lo, t_hi, buf, accumulate=True,
                            mod=group)
        ctx.sync()
        assert np.array_equal(buf.cpu().numpy(), base + want), shape


@pytest.mark.parametrize("shape", C.CROSSFADE_SHAPES, ids=_id)
def test_modulated_crossfade_cases(amd, shape):
    bars = Bars()
    for c in [c for c in C.crossfade_cases() if (c["H"], c["p"]) == shape]:
        m = C.crossfade_models(c)
        nz = dict(C.noise_model(c["sigma"], c["refl"], c["H"]), mod=c["mod"], mod_harmonics=c["M"])
        fund = (c["theta"], c["nu"])
        out = amd.eaQHMNoiseSynthesis(nz, c["tau"], c["L_out"], seed=C.SEED, fundamental=fund)
        plain = amd.eaQHMNoiseSynthesis(nz, c["tau"], c["L_out"], seed=C.SEED)
        assert out.shape == (c["L_out"],) and out.dtype == np.float64
        err = float(np.abs(out - m["out"]).max() / m["top"])
        moved = float(np.abs(out - plain).max() / m["top"])
        print("noise direct crossfade %s: model dev %.3g gpu err %.3g (modulation moves %.3g)"
              % (c["name"], m["dev"], err, moved))
        record_measurement("noise_direct_crossfade_%s" % c["name"], model_dev=m["dev"], gpu_err=err, moved=moved)
        assert moved > 1e-3, c["name"]
        bars.hold(c["name"], err, m["dev"])
        zero = dict(nz, mod=np.zeros_like(c["mod"]))
        assert np.array_equal(amd.eaQHMNoiseSynthesis(zero, c["tau"], c["L_out"], seed=C.SEED, fundamental=fund), plain), \
            c["name"]
    bars.check()


# ---- warp and envelope
def _check_warp(bars, kind, c, m, got, passes):
    """The bars and the exact parts of one warp call; `passes` marks the frames that come back bit for bit."""
    Nf, p = c["Nf"], c["p"]
    assert got["sigma"].shape == (Nf,) and got["refl"].shape == (Nf, p)
    assert got["sigma"].dtype == got["refl"].dtype == np.float64
    silent = c["sigma"] == 0
    err_k = float(np.abs(got["refl"] - m["refl"]).max())
    err_s = float(np.abs(got["sigma"] - m["sigma"]).max() / m["smax"])
    print("noise direct %s %s: k: model dev %.3g gpu err %.3g  sigma: model dev %.3g gpu err %.3g"
          % (kind, c["name"], m["dev_k"], err_k, m["dev_s"], err_s))
    record_measurement("noise_direct_%s_%s" % (kind, c["name"]), frames=Nf, silent=int(silent.sum()),
                       passed_through=int(passes.sum()), model_dev_k=m["dev_k"], gpu_err_k=err_k,
                       model_dev_sigma=m["dev_s"], gpu_err_sigma=err_s)
    assert np.array_equal(got["sigma"][passes], c["sigma"][passes]), c["name"]
    assert np.array_equal(got["refl"][passes], c["refl"][passes]), c["name"]
    gone = silent & ~passes
    assert np.all(got["sigma"][gone] == 0) and np.all(got["refl"][gone] == 0), c["name"]
    assert np.array_equal(got["sigma"] == 0, silent), c["name"]
    assert np.all(N.stop_stage(got["sigma"], got["refl"]) == 0), c["name"]
    bars.hold(c["name"] + " k", err_k, m["dev_k"])
    bars.hold(c["name"] + " sigma", err_s, m["dev_s"])


def _check_envelope(bars, name, sigma, got, m, F):
    assert got.shape == m["out"].shape == (len(sigma), F) and got.dtype == np.float64
    fin = np.isfinite(m["out"])
    assert np.array_equal(np.isneginf(got), ~fin) and np.array_equal(fin.all(axis=1), sigma > 0), name
    err = float(np.abs(got[fin] - m["out"][fin]).max())
    print("noise direct envelope %s: model dev %.3g gpu err %.3g" % (name, m["dev"], err))
    bars.hold(name, err, m["dev"])
    return err


@pytest.mark.parametrize("p", C.WARP_ORDERS)
def test_warp_cases(amd, p):
    bars = Bars()
    for c in [c for c in C.warp_cases() if c["p"] == p]:
        got = amd.eaQHMNoiseWarp(C.noise_model(c["sigma"], c["refl"], 80), c["alpha"])
        _check_warp(bars, "warp", c, C.warp_models(c), got, c["alpha"] == 1.0)
    bars.check()


@pytest.mark.parametrize("p", C.WARP_ORDERS)
def test_envelope_cases(amd, p):
    bars, by_warp = Bars(), {}
    for c in [c for c in C.envelope_cases() if c["p"] == p]:
        m = C.envelope_models(c)
        got = amd.noise_envelope(C.noise_model(c["sigma"], c["refl"], 80), C.FS, c["freqs"], c["alpha"])
        err = _check_envelope(bars, c["name"], c["sigma"], got, m, c["F"])
        by_warp.setdefault(c["name"].rsplit("_", 1)[0], {}).update(
            {"model_dev_F%d" % c["F"]: m["dev"], "gpu_err_F%d" % c["F"]: err})
    for name, values in by_warp.items():
        record_measurement("noise_direct_envelope_%s" % name, **values)
    bars.check()


def test_map_cases(amd):
    bars = Bars()
    for c in C.map_cases():
        nz = C.noise_model(c["sigma"], c["refl"], 80)
        got = amd.eaQHMNoiseWarp(nz, formant_warp=(c["x"], c["y"]))
        passes = np.arange(c["Nf"]) == c["identity"]
        _check_warp(bars, "warp_map", c, C.map_models(c), got, passes)
        values = {}
        for F in C.ENVELOPE_SIZES:
            m = C.map_envelope_models(c, F)
            env = amd.noise_envelope(nz, C.FS, C.envelope_freqs(F), formant_warp=(c["x"], c["y"]))
            err = _check_envelope(bars, "map %s F%d" % (c["name"], F), c["sigma"], env, m, F)
            values.update({"model_dev_F%d" % F: m["dev"], "gpu_err_F%d" % F: err})
        record_measurement("noise_direct_envelope_map_%s" % c["name"], **values)
    bars.check()


@pytest.mark.parametrize("p", [1, 63])
def test_warp_and_envelope_of_a_slice_are_the_slice(amd, p):
    """The first and the last Nf frames of a 37-frame model, for every count of the tables, against the whole call:
    scale and map, warp and envelope, bit for bit."""
    Nw = 37
    sigma, refl = C.warp_model(p, Nw)
    alpha = C.alphas(Nw)[3][1]
    x, y = C.warp_map(Nw, 16)
    freqs = C.envelope_freqs(65)

    def calls(lo, hi):
        nz = C.noise_model(sigma[lo:hi], refl[lo:hi], 80)
        a = amd.eaQHMNoiseWarp(nz, alpha[lo:hi])
        b = amd.eaQHMNoiseWarp(nz, formant_warp=(x, y[lo:hi]))
        return (a["sigma"], a["refl"], b["sigma"], b["refl"], amd.noise_envelope(nz, C.FS, freqs, alpha[lo:hi]),
                amd.noise_envelope(nz, C.FS, freqs, formant_warp=(x, y[lo:hi])))

    whole = calls(0, Nw)
    assert not np.array_equal(whole[1], refl) and not np.array_equal(whole[3], refl)
    for count in C.WARP_COUNTS:
        for lo, hi in ((0, count), (Nw - count, Nw)):
            for i, (part, full) in enumerate(zip(calls(lo, hi), whole)):
                assert np.array_equal(part, full[lo:hi]), (p, count, lo, i)


# ---- modulation
def _modulation(ctx, c, e=None, M=None):
    import torch
    e = c["e"] if e is None else e
    M = c["M"] if M is None else M
    L = len(e)
    Nf = (L - 1) // c["H"] + 1
    e_d, th_d, f0_d, v_d = _dev(ctx, e, c["theta"], c["f0"], c["voiced"].astype(np.uint8))
    mod = torch.full((Nf, 2 * M), np.nan, dtype=torch.float64, device=ctx.device)
    ctx.noise_modulation(e_d, L, c["H"], th_d, f0_d, v_d, c["n"], c["ti0"], c["D"], C.FS, M, mod)
    ctx.sync()
    return mod.cpu().numpy()


@pytest.mark.parametrize("H", C.MOD_HOPS)
def test_modulation_cases(ctx, H):
    bars = Bars()
    for c in [c for c in C.modulation_cases() if c["H"] == H]:
        m = C.modulation_models(c)
        got = _modulation(ctx, c)
        assert got.shape == (c["Nf"], 2 * c["M"]) and got.dtype == np.float64 and np.all(np.isfinite(got)), c["name"]
        zero, zero_ref = np.all(got == 0, axis=1), np.all(m["mod"] == 0, axis=1)
        err = float(np.abs(got - m["mod"]).max())
        print("noise direct modulation %s: zero frames %d model dev %.3g gpu err %.3g"
              % (c["name"], int(zero_ref.sum()), m["dev"], err))
        record_measurement("noise_direct_modulation_%s" % c["name"], frames=c["Nf"], zero_frames=int(zero_ref.sum()),
                           model_dev=m["dev"], gpu_err=err)
        assert np.array_equal(zero, zero_ref), c["name"]
        bars.hold(c["name"], err, m["dev"])
        if c["M"] == 8:      # the coefficients do not depend on how many are asked for
            assert np.array_equal(_modulation(ctx, c, M=1), got[:, :2]), c["name"]
    bars.check()


@pytest.mark.parametrize("H", C.MOD_HOPS)
def test_modulation_of_a_prefix_is_the_prefix_of_the_modulation(ctx, H):
    """The first frames of a signal, for every count of the table: frame m of e[:L'] equals frame m of e wherever its
    window ends inside the prefix."""
    c = dict(C.modulation_inputs(H, 10), H=H, M=8)
    whole = _modulation(ctx, c)
    compared = 0
    for count in C.MOD_COUNTS:
        Lp = (count - 1) * H + 1
        part = _modulation(ctx, c, e=c["e"][:Lp])
        same = np.flatnonzero(np.arange(count) * H + 2 * H <= Lp)
        assert part.shape == (count, 16) and np.array_equal(part[same], whole[same]), (H, count)
        compared += len(same)
    assert compared >= 10
