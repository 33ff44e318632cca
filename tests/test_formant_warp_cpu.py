"""The piecewise-linear formant warp, the parts that need no GPU: the NumPy model of the
definition (tests/formant_warp_ref.py), B = 1 against the formant scale's model, the argument checks of
check_formant_warp and its users, the VTLN helper, the per-frame rows, the binding and the CLI."""
import os
import re

import numpy as np
import pytest

import formant_warp_ref as FW
import model_formant_ref as MF
import noise_model_ref as N
import noise_warp_ref as W
from conftest import ROOT

FS = 16000.0
NEW_SYMBOLS = {"eaqhm_modify_amp_warp": 10, "eaqhm_model_envelope_warp": 10, "eaqhm_noise_warp_map": 10,
               "eaqhm_noise_envelope_map": 11}


def _maps(fs=FS):
    """(label, f_in, f_out): VTLN 0.8 and 1.25, three breakpoints, B = 16, B = 1."""
    nyq = fs / 2
    x16 = nyq * np.arange(1, 17) / 16.0
    y16 = x16 * (1.0 + 0.15 * np.sin(np.pi * np.arange(1, 17) / 16.0))
    return [("vtln0.8",) + FW.vtln(fs, 0.8), ("vtln1.25",) + FW.vtln(fs, 1.25),
            ("three", np.array([0.125, 0.4, 1.0]) * nyq, np.array([0.15, 0.42, 1.0]) * nyq),
            ("b16", x16, y16), ("b1", np.array([1000.0]), np.array([1180.0]))]


@pytest.mark.parametrize("dt", [np.float64, np.longdouble])
def test_inverse_of_forward_is_the_frequency(dt):
    """V(W(f)) == f to rounding: a few ulp of the largest frequency involved (two roundings of each map, slopes in
    [0.25, 4] amplify the inner one by at most 4)."""
    f = np.linspace(0.0, 1.3 * FS / 2, 4001)
    for label, x, y in _maps():
        back = FW.warp_inverse(x, y, np.asarray(FW.warp_forward(x, y, f, dt), dtype=np.float64), dt)
        assert back.dtype == dt
        err = float(np.abs(back - f).max())
        assert err <= 16 * np.finfo(np.float64).eps * 1.3 * FS / 2 * 4, (label, err)
        assert np.all(np.diff(np.asarray(FW.warp_inverse(x, y, f), dtype=np.float64)) >= 0), label


def test_identity_row_is_exact_and_breakpoints_map_onto_breakpoints():
    q = np.r_[0.0, np.random.default_rng(0).uniform(0, 12000, 500)]
    for label, x, y in _maps():
        assert np.array_equal(FW.warp_inverse(x, x.copy(), q), q), label
        # a read exactly on y_j gives x_j: segment j+1 starts there with (q - y_j) = 0 (the last one by its ratio)
        got = FW.warp_inverse(x, y, y)
        assert np.array_equal(got[:-1], x[:-1]) and abs(got[-1] - x[-1]) <= 2 * np.spacing(x[-1]), label
        # beyond the last breakpoint the last slope continues
        B = len(x)
        xp, yp = (x[B - 2], y[B - 2]) if B > 1 else (0.0, 0.0)
        far = y[-1] * 1.2
        assert FW.warp_inverse(x, y, far) == xp + (far - yp) * ((x[-1] - xp) / (y[-1] - yp))
    # a near-identity row is not the identity: arithmetic runs
    x = np.array([1000.0, 8000.0])
    y = np.array([1000.0, np.nextafter(8000.0, 9000.0)])
    assert not np.array_equal(FW.warp_inverse(x, y, q), q)


@pytest.mark.parametrize("alpha", [0.8, 1.25])
def test_one_breakpoint_is_the_formant_scale(alpha):
    """B = 1 with (x, alpha x) against model_formant_ref: the read frequency is q * (x / (alpha x)) instead of
    q / alpha.  The first rounds three times (alpha x, the ratio, the product), the second once, each by at most 2^-53
    relative: they differ by at most 4 * 2^-53 = 2^-51 relative (measured: DESIGN.md §9.4).  Through the envelope a
    shift dq of the read frequency moves ln A' by at most (steepest slope between two nodes) * dq, and the
    interpolation itself rounds a few times at the size of ln A' (|ln A'| <= 6 here): 8 eps * 6 is allowed for that."""
    q = np.linspace(0.0, 8000.0, 20001)
    x = np.array([1000.0])
    v = np.asarray(FW.warp_inverse(x, alpha * x, q))
    rel = float(np.abs(v[1:] / (q[1:] / alpha) - 1.0).max())
    print("B = 1 against q / alpha at alpha %g: max relative difference %.3g" % (alpha, rel))
    assert v[0] == 0.0 and rel <= 2.0 ** -51
    rng = np.random.default_rng(3)
    n, K = 9, 12
    fm = np.sort(rng.uniform(80.0, 7900.0, (n, K)), axis=1)
    am = np.exp(rng.uniform(-6.0, -3.0, (n, K)))
    am[4] = 0.0
    steepest = float(np.abs(np.diff(np.log(np.delete(am, 4, axis=0)), axis=1) / np.diff(np.delete(fm, 4, axis=0), axis=1)).max())
    bar = steepest * (1.25 * 7900.0 / 0.8) * 2.0 ** -51 + 8 * np.finfo(np.float64).eps * 6.0
    for beta in (1.0, 1.25):
        a = FW.amplitudes(am, fm, FS, beta, x, alpha * x)
        b = MF.formant_amplitudes(am, fm, FS, beta, alpha)
        assert np.array_equal(a == 0, b == 0)
        live = b != 0
        d = float(np.abs(np.log(a[live]) - np.log(b[live])).max())
        print("  amplitudes at beta %g: max |d ln A'| %.3g (bar %.3g)" % (beta, d, bar))
        assert d <= bar
    grid = np.linspace(0.0, 9000.0, 500)
    rec = np.concatenate((am, fm, np.zeros((n, K + 1))), axis=1)
    a, b = FW.envelope_readout(rec, grid, x, alpha * x), MF.envelope_readout(rec, grid, alpha)
    assert np.array_equal(np.isneginf(a), np.isneginf(b)) and np.isneginf(a[4]).all()
    fin = np.isfinite(b)
    assert np.abs(a[fin] - b[fin]).max() <= steepest * (9000.0 / 0.8) * 2.0 ** -51 + 8 * np.finfo(np.float64).eps * 6.0


def test_identity_amplitudes_are_a_copy_and_muting_follows_the_output_frequency():
    rng = np.random.default_rng(5)
    fm = np.sort(rng.uniform(80.0, 7900.0, (5, 7)), axis=1)
    am = np.exp(rng.uniform(-6.0, -3.0, (5, 7)))
    x, y = FW.vtln(FS, 0.8)
    assert np.array_equal(FW.amplitudes(am, fm, FS, 1.0, x, x.copy()), am)
    a = FW.amplitudes(am, fm, FS, 1.25, x, y)
    assert np.array_equal(a == 0, 1.25 * fm >= FS / 2)
    yrows = np.tile(x, (5, 1))
    yrows[2] = y
    a = FW.amplitudes(am, fm, FS, 1.0, x, yrows)
    assert np.array_equal(a[[0, 1, 3, 4]], am[[0, 1, 3, 4]]) and not np.array_equal(a[2], am[2])


def test_vtln_reaches_nyquist_where_no_scale_does():
    """With a VTLN map the envelope at fs/2 is the model's at fs/2; a scale alpha > 1 has lost the band above
    fs / (2 alpha) by then."""
    f = np.array([500.0, 3000.0, 7000.0, 8000.0])
    rec = np.concatenate((np.exp([-3.0, -4.0, -5.0, -7.0]), f, np.zeros(5)))[None, :]
    base = MF.envelope_readout(rec, [FS / 2], 1.0)[0, 0]
    for alpha in (0.8, 1.25):
        x, y = FW.vtln(FS, alpha)
        assert FW.envelope_readout(rec, [FS / 2], x, y)[0, 0] == base
    # a scale above 1 reads fs/2 at 6400 Hz, inside the band (below 1 it reads past the last node, where E is held)
    assert MF.envelope_readout(rec, [FS / 2], 1.25)[0, 0] != base


# ---- the host layer
def _arrays_model(n=8, K=2, step=15):
    ti = np.arange(n) * step
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
                frange=np.tile([200.0, 400.0], (n, 1))[:, :K], pk=np.zeros((n, K)))


def _noise_model(Nf=26, p=4, hop=8, fs=FS):
    return dict(sigma=np.full(Nf, 0.1), refl=np.zeros((Nf, p)), hop=hop, order=p, fs=fs, length=(Nf - 1) * hop + 1)


@pytest.fixture()
def no_device(monkeypatch):
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


def test_vtln_helper():
    from eaqhm_amd import formant_warp_vtln
    for alpha, slope in ((0.8, 2.4), (1.25, 0.125 / 0.3)):
        x, y = formant_warp_vtln(FS, alpha)
        assert x.dtype == y.dtype == np.float64 and x.shape == y.shape == (2,)
        assert x[1] == y[1] == FS / 2                                      # Nyquist to Nyquist
        assert np.array_equal(x, FW.vtln(FS, alpha)[0]) and np.array_equal(y, FW.vtln(FS, alpha)[1])
        assert abs(y[0] / x[0] - alpha) <= 2e-16
        assert abs((y[1] - y[0]) / (x[1] - x[0]) - slope) <= 1e-12, alpha
    assert abs(0.125 / 0.3 - 0.4167) < 5e-5
    x, y = formant_warp_vtln(FS, 0.8)
    assert np.allclose(x, [7000.0, 8000.0]) and np.allclose(y, [5600.0, 8000.0])
    x, y = formant_warp_vtln(FS, 1.25)
    assert np.allclose(x, [5600.0, 8000.0]) and np.allclose(y, [7000.0, 8000.0])
    x, y = formant_warp_vtln(FS, 1.0)
    assert np.array_equal(x, y)
    x, y = formant_warp_vtln(48000, 1.1, knee=0.5)
    assert np.allclose(x, [12000 / 1.1, 24000.0]) and np.allclose(y, [12000.0, 24000.0])
    for kw in (dict(alpha=0.25), dict(alpha=0.5, knee=0.9), dict(alpha=4.0), dict(alpha=5.0), dict(alpha=0.2),
               dict(alpha=1.1, knee=0.0), dict(alpha=1.1, knee=1.0), dict(alpha=1.1, knee=-0.5),
               dict(alpha=1.1, knee=np.nan), dict(alpha=1.1, knee="x"), dict(alpha=np.nan), dict(alpha=1.1, fs=0.0)):
        args = dict(fs=FS, alpha=1.1, knee=0.875)
        args.update(kw)
        with pytest.raises(ValueError):
            formant_warp_vtln(args["fs"], args["alpha"], args["knee"])


def test_check_formant_warp_accepts_and_returns_rows():
    from eaqhm_amd.model import check_formant_warp, unpack_model
    model = unpack_model(_arrays_model())
    x, y = check_formant_warp(model, FS, ([1000, 8000], [900, 8000]))
    assert x.dtype == y.dtype == np.float64 and x.shape == (2,) and y.shape == (8, 2)
    assert y.flags["C_CONTIGUOUS"] and np.array_equal(y, np.tile([900.0, 8000.0], (8, 1)))
    rows_ = np.linspace([900.0, 8000.0], [1100.0, 8000.0], 8)
    x, y = check_formant_warp(model, FS, (np.array([1000.0, 8000.0]), rows_), 1.0, True)
    assert np.array_equal(y, rows_)
    for label, fx, fy in _maps():
        check_formant_warp(model, FS, (fx, fy))
    check_formant_warp(model, FS, ([1000.0], [4000.0]))            # the slopes' limits are inside
    check_formant_warp(model, FS, ([1000.0], [250.0]))


@pytest.mark.parametrize("warp", [
    None, 5.0, "ab", ([1000.0],), ([1000.0], [1100.0], [1.0]),                      # not a pair
    (["a"], ["b"]), ([[1000.0]], [1100.0]), (1000.0, 1100.0),                      # not numbers / not 1-D
    ([], []), (np.arange(1, 18) * 100.0, np.arange(1, 18) * 100.0),                # B = 0, B = 17
    ([1000.0, 2000.0], [1000.0]), ([1000.0, 2000.0], np.ones((7, 2))),             # f_out's shape
    ([1000.0, 2000.0], np.ones((8, 3))), ([1000.0, 2000.0], np.ones((1, 8, 2))),
    ([1000.0, np.nan], [1000.0, 2000.0]), ([1000.0, 2000.0], [1000.0, np.inf]),    # finite
    ([0.0, 2000.0], [100.0, 2000.0]), ([1000.0, 2000.0], [0.0, 2000.0]), ([-1.0], [1.0]),   # > 0
    ([2000.0, 1000.0], [1000.0, 2000.0]), ([1000.0, 1000.0], [1000.0, 2000.0]),    # strictly increasing
    ([1000.0, 2000.0], [1500.0, 1500.0]), ([1000.0, 2000.0], [1500.0, 1400.0]),
    ([1000.0], [4100.0]), ([1000.0], [240.0]),                                     # slopes: the one from the origin
    ([1000.0, 2000.0], [1000.0, 6000.0]), ([1000.0, 5000.0], [1000.0, 1900.0])])   # slopes: a later segment
def test_check_formant_warp_rejects(warp, no_device):
    from eaqhm_amd import eaQHMSynthesis, model_envelope
    from eaqhm_amd.model import check_formant_warp, unpack_model
    det = _arrays_model()
    if warp is not None:
        with pytest.raises(ValueError):
            check_formant_warp(unpack_model(det), FS, warp)
        with pytest.raises(ValueError):
            eaQHMSynthesis(det, FS, 200, formant_warp=warp)
        with pytest.raises(ValueError):
            model_envelope(det, FS, [100.0], formant_warp=warp)
    else:
        with pytest.raises(ValueError):
            check_formant_warp(unpack_model(det), FS, warp)


def test_one_bad_row_among_good_ones_is_found(no_device):
    from eaqhm_amd.model import check_formant_warp, unpack_model
    model = unpack_model(_arrays_model())
    for bad in ([1500.0, 1400.0], [1000.0, np.nan], [1000.0, 7000.0], [-5.0, 2000.0]):
        rows_ = np.tile([1000.0, 2000.0], (8, 1))
        rows_[5] = bad
        with pytest.raises(ValueError):
            check_formant_warp(model, FS, ([1000.0, 2000.0], rows_))


def test_warp_excludes_a_formant_scale_and_needs_the_envelope(no_device):
    from eaqhm_amd import eaQHMNoiseWarp, eaQHMSynthesis, model_envelope, noise_envelope
    from eaqhm_amd.model import check_formant_warp, unpack_model
    det = _arrays_model()
    model = unpack_model(det)
    good = ([1000.0, 8000.0], [900.0, 8000.0])
    for scale in (1.2, np.ones(8), np.full(8, 1.1), 9.0, "x"):
        with pytest.raises(ValueError):
            check_formant_warp(model, FS, good, scale, True)
        with pytest.raises(ValueError):
            eaQHMSynthesis(det, FS, 200, formant_scale=scale, formant_warp=good)
        with pytest.raises(ValueError):
            model_envelope(det, FS, [100.0], scale, good)
    with pytest.raises(ValueError):
        check_formant_warp(model, FS, good, 1.0, False)
    with pytest.raises(ValueError):
        eaQHMSynthesis(det, FS, 200, preserve_envelope=False, formant_warp=good)
    with pytest.raises(ValueError):
        check_formant_warp(model, 0.0, good)
    nz = _noise_model()
    for scale in (1.2, np.ones(26)):
        with pytest.raises(ValueError):
            eaQHMNoiseWarp(nz, scale, formant_warp=good)
        with pytest.raises(ValueError):
            noise_envelope(nz, FS, [100.0], scale, formant_warp=good)
    for bad in (([1000.0, 2000.0], np.ones((25, 2))), ([2000.0, 1000.0], [1000.0, 2000.0]), ([1000.0], [4100.0])):
        with pytest.raises(ValueError):
            eaQHMNoiseWarp(nz, formant_warp=bad)
        with pytest.raises(ValueError):
            noise_envelope(nz, FS, [100.0], formant_warp=bad)
    # good calls pass the checks and reach the device
    with pytest.raises(AssertionError):
        eaQHMSynthesis(det, FS, 200, formant_warp=good)
    with pytest.raises(AssertionError):
        model_envelope(det, FS, [100.0], formant_warp=good)
    with pytest.raises(AssertionError):
        eaQHMNoiseWarp(nz, formant_warp=(good[0], np.tile(good[1], (26, 1))))
    with pytest.raises(AssertionError):
        noise_envelope(nz, FS, [100.0], formant_warp=good)
    nz2 = dict(nz, length=200, sigma=np.full(25, 0.1), refl=np.zeros((25, 4)))
    with pytest.raises(AssertionError):
        eaQHMSynthesis(det, FS, 200, noise=nz2, noise_formant=True, formant_warp=good)
    with pytest.raises(ValueError):       # noise_formant still needs noise=
        eaQHMSynthesis(det, FS, 200, noise_formant=True, formant_warp=good)


def test_per_frame_rows_are_np_interp_and_stay_valid():
    from eaqhm_amd import formant_warp_vtln, noise_formant_warp
    from eaqhm_amd.model import _warp_rows, check_noise_warp_map_arguments
    det = _arrays_model(n=12)                      # instants 0, 15, .., 165
    nz = _noise_model(Nf=26, hop=8)                # frames 0, 8, .., 200: the last ones lie past the last instant
    x = np.array([3000.0, 6000.0, 8000.0])
    a = np.array([2400.0, 6500.0, 8000.0])
    b = np.array([3600.0, 5000.0, 8000.0])
    u = (np.arange(12) / 11.0)[:, None]
    rows_ = (1 - u) * a + u * b
    rows_[:, 2] = 8000.0
    f_in, got = noise_formant_warp(nz, det, (x, rows_))
    assert np.array_equal(f_in, x) and got.shape == (26, 3) and got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, FW.frame_rows(8, 26, det["ti"], rows_))
    for j in range(3):
        assert np.array_equal(got[:, j], np.interp(np.arange(26) * 8.0, det["ti"].astype(np.float64), rows_[:, j]))
    assert np.array_equal(got[0], rows_[0]) and np.all(got[21:] == rows_[-1])
    assert np.all(got[:, 2] == 8000.0)                         # a constant column comes back exactly
    _warp_rows((f_in, got), 26, "noise frame")                 # convex combinations of valid rows are valid rows
    nz2, xn, yn = check_noise_warp_map_arguments(nz, (f_in, got))
    assert np.array_equal(xn, x / FS) and np.array_equal(yn, got / FS) and yn.flags["C_CONTIGUOUS"]
    # one row for all instants: every frame gets it; an identity row stays the identity bit for bit, also normalised
    f_in, got = noise_formant_warp(nz, det, (x, x.copy()))
    assert np.array_equal(got, np.tile(x, (26, 1)))
    _, xn, yn = check_noise_warp_map_arguments(nz, (f_in, got))
    assert np.array_equal(yn, np.tile(xn, (26, 1)))
    # a ramp between two VTLN maps of one knee frequency shares f_in
    x0, y0 = formant_warp_vtln(FS, 0.9)
    y1 = np.array([1.1 * x0[0], 8000.0])
    f_in, got = noise_formant_warp(nz, det, (x0, (1 - u) * y0 + u * y1))
    _warp_rows((f_in, got), 26, "noise frame")
    with pytest.raises(ValueError):
        noise_formant_warp(nz, det, (x, np.ones((11, 3))))
    with pytest.raises(ValueError):
        noise_formant_warp("model", det, (x, x))


def test_reference_noise_warp_stays_inside_the_exclusion_cap():
    """Before the GPU test relies on it: on the AR(4) fixture, analysed by noise_model_ref, the model in float64 and in
    longdouble stops at the same stage in every frame for the maps the GPU test uses (none excluded, none stopping), and
    the two differ (the bar 100 x deviation is not zero)."""
    sigma, refl, stop = N.analyse(N.ar_fixture(), 80, 18)
    assert not stop.any()
    frames = np.r_[np.flatnonzero(sigma > 0)[::9], np.flatnonzero(sigma == 0)[:2]]
    for label, x, y in _maps():
        s2, k2, st = FW.noise_warp(sigma[frames], refl[frames], x / FS, y / FS)
        s2l, k2l, stl = FW.noise_warp(sigma[frames], refl[frames], x / FS, y / FS, np.longdouble)
        assert np.array_equal(st, stl) and not st.any(), label
        assert 0 < np.abs(k2 - k2l).max() < 1e-9 and np.all(s2[-2:] == 0), label
        assert np.abs(k2).max() < 1
    # the identity returns the frames; B = 1 is the scale's model to the rounding of the read angle
    s2, k2, _ = FW.noise_warp(sigma[frames], refl[frames], np.array([0.25]), np.array([0.25]))
    assert np.array_equal(s2, sigma[frames]) and np.array_equal(k2, refl[frames])
    s2, k2, _ = FW.noise_warp(sigma[frames[:6]], refl[frames[:6]], np.array([0.25]), np.array([0.25 * 1.2]))
    s3, k3, _ = W.warp(sigma[frames[:6]], refl[frames[:6]], 1.2)
    assert np.abs(k2 - k3).max() < 1e-9 and np.abs(s2 / s3 - 1).max() < 1e-9
    e1 = FW.noise_envelope(sigma[frames[:6]], refl[frames[:6]], np.array([0.25]), np.array([0.3]), np.linspace(0, 0.7, 50))
    e2 = W.envelope(sigma[frames[:6]], refl[frames[:6]], 1.2, np.linspace(0, 0.7, 50))
    assert np.abs(e1 - e2).max() < 1e-9


# ---- binding and CLI
def test_binding_header_and_exports():
    import eaqhm_amd
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    sym = {n: a for n, _, a in hip.SYMBOLS}
    with open(os.path.join(ROOT, "include", "eaqhm_hip.h")) as f:
        header = f.read()
    for name, nargs in NEW_SYMBOLS.items():
        assert len(sym[name]) == nargs, name
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert len(sym["eaqhm_noise_warp"]) == 8 and len(sym["eaqhm_noise_envelope"]) == 9
    for name in ("formant_warp_vtln", "noise_formant_warp", "eaQHMNoiseWarp", "model_envelope", "noise_envelope"):
        assert callable(getattr(eaqhm_amd, name))
    for name in ("modify_amp_warp", "model_envelope_warp", "noise_warp_map", "noise_envelope_map"):
        assert callable(getattr(hip.Context, name))
    assert callable(eaqhm_amd.model.check_formant_warp)


def test_cli_flags_and_their_exclusions(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav", "--formant-vtln", "1.15", "--formant-knee", "0.8", "--noise", "--noise-formant"])
    assert a.formant_vtln == 1.15 and a.formant_knee == 0.8 and a.noise_formant and a.formant_warp_curve is None
    a = cli.parser().parse_args(["x.wav", "--formant-warp-curve", "w.txt"])
    assert a.formant_warp_curve == "w.txt" and a.formant_vtln is None and a.formant_knee is None
    curve = tmp_path / "warp.txt"
    curve.write_text("# Hz in, Hz out\n1000 1150\n4000 4200 # F2\n8000 8000\n")
    scale = tmp_path / "alpha.txt"
    scale.write_text("0 1.0\n1 1.2\n")
    missing = str(tmp_path / "missing.wav")
    for flags in (["--formant-vtln", "1.1", "--formant-scale", "1.1"], ["--formant-vtln", "1.1", "--formant-warp-curve", str(curve)],
                  ["--formant-warp-curve", str(curve), "--formant-scale", "1.1"],
                  ["--formant-warp-curve", str(curve), "--formant-scale-curve", str(scale)],
                  ["--formant-vtln", "1.1", "--formant-scale-curve", str(scale)],
                  ["--formant-knee", "0.8"], ["--formant-knee", "0.8", "--formant-scale", "1.1"],
                  ["--formant-vtln", "1.1", "--no-envelope"], ["--formant-warp-curve", str(curve), "--no-envelope"],
                  ["--formant-vtln", "1.1", "--noise-formant"]):
        with pytest.raises(SystemExit):
            cli.main([missing] + flags)
    for flags in (["--formant-vtln", "9"], ["--formant-vtln", "0.25"], ["--formant-vtln", "1.1", "--formant-knee", "1.5"]):
        with pytest.raises(ValueError):
            cli.main([missing] + flags)                        # rejected before the analysis
    for text in ("1000 1150\n900 4000\n", "1000 5000\n", "1000 1100 3\n", "", "a b\n",
                 "\n".join("%d %d" % (100 * i, 100 * i) for i in range(1, 18))):
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        with pytest.raises(ValueError):
            cli.main([missing, "--formant-warp-curve", str(bad)])
    with pytest.raises(ValueError):
        cli.main([missing, "--formant-warp-curve", str(tmp_path / "nofile.txt")])
    for flags in (["--formant-vtln", "1.15"], ["--formant-vtln", "1.15", "--noise", "--noise-formant"],
                  ["--formant-warp-curve", str(curve)], ["--formant-warp-curve", str(curve), "--noise", "--noise-formant"],
                  ["--formant-vtln", "0.9", "--formant-knee", "0.7", "--pitch-scale", "1.3"]):
        with pytest.raises(FileNotFoundError):
            cli.main([missing] + flags)                        # accepted: the analysis starts
    x, y = cli.read_warp_curve(str(curve), "curve")
    assert np.array_equal(x, [1000.0, 4000.0, 8000.0]) and np.array_equal(y, [1150.0, 4200.0, 8000.0])
    t, v = cli.read_scale_curve(str(scale), "curve")           # the scale reader is what it was
    assert np.array_equal(t, [0.0, 1.0]) and np.array_equal(v, [1.0, 1.2])
