"""CPU tests (no GPU) of the shape-invariant phase mode on its NumPy model (tests/model_shape_ref.py):
the relative phases of the harmonics are the model's own at every scale, model_f0, the argument checks of
eaQHMSynthesis(phase=, f0=), the binding and the CLI flag."""
import os

import numpy as np
import pytest

import model_shape_ref as MS
import model_synthesis_ref as M
from conftest import load_golden
from fake_backend import OracleBackend


@pytest.fixture(scope="module")
def sa19_records():
    g = load_golden("sa19_female_default.npz")
    cells = g["det_cells"]
    n, K = len(g["det_ti"]), int(cells[:, 1].max()) + 1
    rec = M.records_from_cells(n, K, cells, g["det_am"], g["det_fm"], g["det_pk"],
                               np.where(g["det_isVoiced"], g["det_a0"], 0.0))
    return rec, len(g["s_recon"])


def _relative_phase_error(rec, L, rho, beta, mode="shape"):
    """max over slots k >= 1 and output samples where slots 0 and k are both in a run of the distance mod 2 pi between
    phase_k - (k+1) phase_0 of the output and of the model at tau, and the bar for it: each of the four phases is
    rounded once when it is formed and once more when it is multiplied by (k+1) and subtracted, so the error is at most
    a few ulp of the largest term; the bar is 8 * 2^-52 * max(|phase_k|, (k+1) |phase_0|) over both sides."""
    out, info = MS.synthesize_shape(rec, 15, 16000, L, rho, beta, phases=True, mode=mode)
    ph, cov = info["phase"], info["cover"]
    mp, mc = MS.model_phases(rec, 15, 16000, info["tau"])
    assert np.array_equal(cov, mc)
    worst, top, count = 0.0, 0.0, 0
    for k in range(1, ph.shape[1]):
        both = cov[:, 0] & cov[:, k]
        if not both.any():
            continue
        d = (ph[both, k] - (k + 1) * ph[both, 0]) - (mp[both, k] - (k + 1) * mp[both, 0])
        d -= 2 * np.pi * np.rint(d / (2 * np.pi))
        worst = max(worst, float(np.abs(d).max()))
        top = max(top, float(np.abs(ph[both, k]).max()), float((k + 1) * np.abs(ph[both, 0]).max()),
                  float(np.abs(mp[both, k]).max()), float((k + 1) * np.abs(mp[both, 0]).max()))
        count += int(both.sum())
    assert count > 100000
    return worst, 8 * 2.0 ** -52 * top


@pytest.mark.parametrize("rho, beta", [(2.0, 1.0), (0.5, 1.0), (1.0, 1.3), (1.6, 0.8), ("sinus", "ramp")])
def test_relative_phases_are_the_models(sa19_records, rho, beta):
    rec, L = sa19_records
    if rho == "sinus":
        x = np.arange(len(rec)) / (len(rec) - 1)
        rho, beta = 1.1 + 0.5 * np.sin(2 * np.pi * 3.0 * x), 1.3 - 0.5 * x
    worst, bar = _relative_phase_error(rec, L, rho, beta)
    print("relative phase error", worst, "bar", bar)
    assert worst <= bar


def test_independent_mode_moves_the_relative_phases(sa19_records):
    rec, L = sa19_records
    worst, _ = _relative_phase_error(rec, L, 2.0, 1.0, mode="independent")
    assert worst > 1.0


def test_unit_scales_are_the_default_mode(sa19_records):
    rec, L = sa19_records
    a, info = MS.synthesize_shape(rec, 15, 16000, L, 1.0, 1.0, phases=True)
    assert np.all(info["s"] == 0.0)
    assert np.abs(a - M.synthesize(rec, 15, 16000, L)).max() <= 1e-12 * np.abs(a).max()


def test_reference_advance_matches_the_host(sa19_records):
    from eaqhm_amd.model import _records_f0, contour_time_map, fundamental_advance
    rec, L = sa19_records
    n = len(rec)
    f0 = MS.model_f0(rec)
    assert np.abs(_records_f0(rec, (rec.shape[1] - 1) // 3) - f0).max() <= 1e-12 * f0.max()
    x = np.arange(n) / (n - 1)
    g = contour_time_map(0.7 + x, 1.4 - 0.6 * x, 15, L)["gain"]
    S = fundamental_advance(f0, g, 15, 16000)
    assert np.array_equal(S, MS.advance(f0, g, 15, 16000)) and S[0] == 0 and np.all((S >= 0) & (S < 1))
    assert np.all(fundamental_advance(f0, np.ones(n - 1), 15, 16000) == 0.0)


def _model(n=12, K=3, step=15):
    ti = np.arange(n) * step
    am = np.full((n, K), 0.1) / np.arange(1, K + 1)
    fm = np.tile(200.0 * np.arange(1, K + 1), (n, 1))
    return dict(ti=ti, a0=np.zeros(n), amplitudes=am, frange=fm.astype(float), pk=np.zeros((n, K)))


def test_model_f0_holds_over_silent_instants():
    from eaqhm_amd import model_f0
    d = _model()
    d["frange"][:, :] *= (1.0 + 0.01 * np.arange(12))[:, None]        # f0_i = 200 (1 + 0.01 i)
    d["amplitudes"][[0, 1, 5, 6, 11]] = 0.0
    f0 = model_f0(d, 16000)
    want = 200.0 * (1.0 + 0.01 * np.array([2, 2, 2, 3, 4, 4, 4, 7, 8, 9, 10, 10]))
    assert f0.dtype == np.float64 and np.allclose(f0, want, rtol=1e-14, atol=0)
    d["amplitudes"][:] = 0.0
    assert np.array_equal(model_f0(d, 16000), np.zeros(12))
    d = _model()
    d["frange"][:, 1] = 430.0                                           # a^2-weighted mean of f_k / (k+1)
    w = (0.1 / np.arange(1, 4)) ** 2
    assert np.allclose(model_f0(d, 16000), (w * np.array([200.0, 215.0, 200.0])).sum() / w.sum(), rtol=1e-14)


def test_model_f0_of_the_constructed_model():
    """f_k / (k+1) = f0 + theta_k' / (2 pi (k+1)): every term of the mean is within max|theta_k'| / 2 pi of f0."""
    from eaqhm_amd import model_f0
    det, L, _ = MS.constructed_model()
    f0 = model_f0(det, 16000)
    assert f0.shape == (len(det["ti"]),)
    assert np.abs(f0 - 140.0).max() <= 0.9 * 2 * np.pi * 1.3 / (2 * np.pi)


@pytest.fixture
def backend(monkeypatch):
    """A stand-in backend that counts how often it is asked for: the argument checks must come first."""
    from eaqhm_amd import functions
    touched = []

    def ctx(*a, **k):
        touched.append(a)
        return OracleBackend()
    monkeypatch.setattr(functions, "_ctx", ctx)
    return touched


@pytest.mark.parametrize("kw", [dict(phase="Shape"), dict(phase=None), dict(phase="relative"), dict(phase=1),
                                dict(f0=np.full(12, 200.0)),                              # f0 without "shape"
                                dict(phase="independent", f0=np.full(12, 200.0)),
                                dict(phase="shape", f0=np.full(11, 200.0)),
                                dict(phase="shape", f0=200.0),
                                dict(phase="shape", f0=np.full((12, 1), 200.0)),
                                dict(phase="shape", f0=np.r_[np.full(11, 200.0), np.nan]),
                                dict(phase="shape", f0=np.r_[np.full(11, 200.0), np.inf]),
                                dict(phase="shape", f0=np.r_[np.full(11, 200.0), 0.0]),
                                dict(phase="shape", f0=np.r_[-1.0, np.full(11, 200.0)]),
                                dict(phase="shape", f0=["a"] * 12),
                                dict(phase="shape", time_scale=9.0),
                                dict(phase="shape", formant_scale=1.2, preserve_envelope=False)])
def test_synthesis_rejects_bad_phase_arguments(kw, backend):
    from eaqhm_amd import eaQHMSynthesis
    with pytest.raises(ValueError):
        eaQHMSynthesis(_model(), 16000, 200, **kw)
    assert backend == []


def test_good_phase_arguments_reach_the_backend(backend):
    from eaqhm_amd import eaQHMSynthesis
    from eaqhm_amd.model import check_phase_arguments, unpack_model
    m = unpack_model(_model())
    assert check_phase_arguments(m, "independent", None) == (False, None)
    shape, f0 = check_phase_arguments(m, "shape", None)
    assert shape and np.allclose(f0, 200.0)
    assert np.array_equal(check_phase_arguments(m, "shape", [150] * 12)[1], np.full(12, 150.0))
    with pytest.raises(AttributeError):       # the stand-in has no modify calls: the checks passed, the device is next
        eaQHMSynthesis(_model(), 16000, 200, phase="shape", f0=np.full(12, 200.0), time_scale=2.0)
    assert len(backend) == 1


def test_binding_exports_and_cli_flag():
    import eaqhm_amd
    from eaqhm_amd import cli, hip
    import ctypes as C
    from conftest import ROOT
    assert hip.ABI_VERSION == 6
    sig = {n: a for n, _, a in hip.SYMBOLS}
    with open(os.path.join(ROOT, "include", "eaqhm_hip.h")) as fh:
        header = fh.read()
    # one entry point: the scalar list, then the optional groups (C, rate, gain, rate_min) and (f0, S)
    P, I32, I64, F64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    plain = [P] * 7 + [I32] * 3 + [F64] * 3 + [I64] * 3 + [P]          # ctx .. fs, rho, beta, L_out, t_lo, t_hi, out
    assert sig["eaqhm_modify_synth"] == plain + [P, P, P, F64] + [P, P]
    assert "int eaqhm_modify_synth(" in header
    for gone in ("synth_curve", "synth_shape", "synth_curve_shape"):
        assert "eaqhm_modify_" + gone not in sig and "eaqhm_modify_" + gone not in header
        assert not hasattr(hip.Context, "modify_" + gone)
    assert callable(eaqhm_amd.model_f0)
    assert callable(hip.Context.modify_synth)
    a = cli.parser().parse_args(["x.wav", "--phase", "shape", "--time-scale", "2"])
    assert a.phase == "shape" and cli.parser().parse_args(["x.wav"]).phase == "independent"
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["x.wav", "--phase", "other"])
