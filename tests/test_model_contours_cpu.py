"""Time and pitch scale contours, the parts that need no GPU: the NumPy contour model anchored to the
reference's s_recon and to the scalar model of §9, the time map, the frequency rule, scale_contour and the argument
checks of the array forms."""
import numpy as np
import pytest

import model_contour_ref as MC
import model_synthesis_ref as M
from test_model_synthesis_cpu import golden_model

GOLDEN_MODELS = ["sa19_female_default.npz", "seed16k_1p2s_adpt6.npz"]


@pytest.fixture(scope="module", params=GOLDEN_MODELS)
def golden(request):
    from eaqhm_amd.functions import pack_results
    from eaqhm_amd.model import unpack_model
    g, plan, fin = golden_model(request.param)
    m = unpack_model(pack_results(plan, fin))
    return g, m


def test_unit_contours_reproduce_reference_s_recon(golden):
    g, m = golden
    n = len(m["records"])
    out = MC.synthesize_contour(m["records"], m["step"], 16000, len(g["s_recon"]), np.ones(n), np.ones(n))
    assert out.shape == g["s_recon"].shape
    assert np.abs(out - g["s_recon"]).max() <= 1e-9


@pytest.mark.parametrize("rho", [0.75, 1.5, 2.0])
@pytest.mark.parametrize("beta", [1.0, 1.2])
def test_constant_contours_equal_scalar_model(golden, rho, beta):
    """Dyadic scales: the knot positions C_j = rho j D are exact, so both time maps place every knot alike."""
    g, m = golden
    n = len(m["records"])
    L = len(g["s_recon"])
    ref = M.synthesize(m["records"], m["step"], 16000, L, rho, beta, True)
    out = MC.synthesize_contour(m["records"], m["step"], 16000, L, np.full(n, rho), np.full(n, beta), True)
    assert out.shape == ref.shape == (int(np.rint(rho * L)),)
    assert np.abs(out - ref).max() <= 1e-10 * np.abs(ref).max()


def test_time_map_of_a_piecewise_contour():
    """rho = 1 on the first half of the instants, 2 on the second: the interval across the step has rate 1.5."""
    from eaqhm_amd.model import contour_time_map
    n, D, L = 40, 15, 39 * 15 + 7
    rho = np.where(np.arange(n) < n // 2, 1.0, 2.0)
    beta = np.full(n, 1.1)
    tm = contour_time_map(rho, beta, D, L)
    h = n // 2
    expect_C = np.concatenate((np.arange(h) * D, (h - 1) * D + 1.5 * D + np.arange(n - h) * 2.0 * D))
    assert np.array_equal(tm["C"], expect_C)
    assert tm["L_out"] == int(np.rint((h - 1) * D + 1.5 * D + (n - 1 - h) * 2 * D + 2 * 7))   # 891.5 -> 892
    assert np.array_equal(tm["rate"][:h - 1], np.ones(h - 1)) and tm["rate"][h - 1] == 1.5
    assert np.all(tm["rate"][h:] == 2.0) and tm["rate_min"] == 1.0
    assert np.allclose(tm["gain"], tm["rate"][:-1] * 1.1, rtol=0, atol=1e-15)
    r, g, C, L_out = MC.time_map(rho, beta, D, L)
    assert np.array_equal(C, tm["C"]) and L_out == tm["L_out"] and np.array_equal(g, tm["gain"])
    # constant contours: the length of §9
    for k in (0.25, 0.7, 1.0, 1.3, 4.0):
        assert contour_time_map(np.full(n, k), np.ones(n), D, L)["L_out"] == int(np.rint(k * L))


def _steady_partial(n=400, D=15, fs=16000, f=250.0):
    rec = np.zeros((n, 4))
    rec[:, 0] = 0.3
    rec[:, 1] = f
    rec[:, 2] = np.angle(np.exp(1j * 2 * np.pi * f / fs * np.arange(n) * D))
    return rec, (n - 1) * D + 1


def _zero_crossing_rate(x, fs):
    s = np.signbit(x)
    z = np.flatnonzero(s[1:] != s[:-1])
    return (len(z) - 1) / 2.0 / ((z[-1] - z[0]) / fs)


def test_frequency_rule_with_a_pitch_step():
    """§9.1: inside interval j the output frequency is b_j times the model's, whatever the time map does."""
    fs, D, f = 16000, 15, 250.0
    rec, L = _steady_partial(D=D, fs=fs, f=f)
    n = len(rec)
    beta = np.where(np.arange(n) < n // 2, 0.8, 1.3)
    rho = np.where(np.arange(n) < n // 2, 1.5, 0.75)
    out = MC.synthesize_contour(rec, D, fs, L, rho, beta, preserve_envelope=False)
    _, _, C, L_out = MC.time_map(rho, beta, D, L)
    assert len(out) == L_out
    h = n // 2
    first = out[int(C[5]):int(C[h - 5])]
    second = out[int(C[h + 5]):int(C[n - 5])]
    assert abs(_zero_crossing_rate(first, fs) - 0.8 * f) < 0.5
    assert abs(_zero_crossing_rate(second, fs) - 1.3 * f) < 0.5


def test_scale_contour_interpolates_and_holds():
    from eaqhm_amd import scale_contour
    n, D, fs = 50, 160, 16000
    det = dict(ti=np.arange(n) * D)
    t = ti_s = np.arange(n) * D / fs                              # 10 ms per instant
    out = scale_contour(det, fs, [0.1, 0.3], [1.0, 2.0])
    assert out.shape == (n,) and out.dtype == np.float64
    assert np.all(out[ti_s <= 0.1] == 1.0) and np.all(out[ti_s >= 0.3] == 2.0)
    mid = (t > 0.1) & (t < 0.3)
    assert np.allclose(out[mid], 1.0 + (t[mid] - 0.1) / 0.2, rtol=0, atol=1e-12)
    assert np.all(scale_contour(det, fs, [0.2], [0.5]) == 0.5)
    # the structs form gives the same contour
    from eaqhm_amd.structs import Deterministic
    structs = []
    for ti in det["ti"]:
        x = Deterministic()
        x.ti = int(ti)
        structs.append(x)
    assert np.array_equal(scale_contour(structs, fs, [0.1, 0.3], [1.0, 2.0]), out)


@pytest.mark.parametrize("times, values", [([0.3, 0.1], [1.0, 2.0]), ([0.1, 0.1], [1.0, 2.0]),
                                           ([0.1, np.nan], [1.0, 2.0]), ([0.1, 0.3], [1.0, 4.5]),
                                           ([0.1, 0.3], [0.2, 1.0]), ([0.1, 0.3], [1.0, np.inf]),
                                           ([0.1, 0.3], [1.0]), ([], []), (["a", "b"], [1.0, 2.0]),
                                           ([[0.1, 0.3]], [[1.0, 2.0]])])
def test_scale_contour_rejects(times, values):
    from eaqhm_amd import scale_contour
    with pytest.raises(ValueError):
        scale_contour(dict(ti=np.arange(10) * 15), 16000, times, values)


def _arrays_model(n=8, K=2, step=15):
    ti = np.arange(n) * step
    am = np.full((n, K), 0.1)
    fm = np.tile([200.0, 400.0], (n, 1))[:, :K]
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=am, frange=fm, pk=np.zeros((n, K)))


@pytest.mark.parametrize("kw", [dict(time_scale=np.ones(7)), dict(pitch_scale=np.ones(9)),
                                dict(time_scale=np.r_[np.ones(7), np.nan]), dict(pitch_scale=np.r_[np.ones(7), 4.5]),
                                dict(time_scale=np.r_[0.2, np.ones(7)]), dict(pitch_scale=np.ones((2, 8))),
                                dict(time_scale=np.ones((8, 1))), dict(time_scale=["x"] * 8),
                                dict(time_scale=np.ones(8), pitch_scale="x"), dict(time_scale=np.ones(8), pitch_scale=5.0),
                                dict(pitch_scale=np.ones(8, dtype=bool)), dict(time_scale=[])])
def test_bad_contours_raise(kw):
    """These raise before any device work, so they run without a GPU."""
    from eaqhm_amd.model import eaQHMSynthesis
    with pytest.raises(ValueError):
        eaQHMSynthesis(_arrays_model(), 16000, 200, **kw)


def test_contour_arguments_are_broadcast():
    from eaqhm_amd.model import check_contour_arguments, unpack_model
    m = unpack_model(_arrays_model())
    rho, beta, fs, length = check_contour_arguments(m, 16000, 200, [1.0, 1.2, 1.4, 1.6, 1.8, 2.0, 2.2, 2.4], 1.5)
    assert rho.dtype == beta.dtype == np.float64 and np.array_equal(beta, np.full(8, 1.5))
    assert rho[-1] == 2.4 and fs == 16000.0 and length == 200
