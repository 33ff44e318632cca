"""The discrete cepstrum on an all-pass warped axis without a GPU: the identities of the warp, the
matrix that moves rows between axes (the host's and the model's recursion against quadrature), cepstrum_warp, the
resolution claim the feature rests on (in the NumPy model alone, tests/cepstrum_warp_ref.py), the host layer's argument
checks and its dispatch at cep_warp = 0, the binding and the CLI flag."""
import os
import re

import numpy as np
import pytest

import cepstrum_warp_ref as W
import model_cepstrum_ref as CR
from conftest import ROOT, record_measurement
from test_gmm_cpu import host_conversion

LD = np.longdouble
EPS = 2.0 ** -52
WARPED_SYMBOLS = {"eaqhm_model_cepstrum_warped": 9, "eaqhm_modify_amp_cepstrum_warped": 14,
                  "eaqhm_cepstrum_envelope_warped": 13, "eaqhm_cepstrum_phase_warped": 13,
                  "eaqhm_model_build_warped": 14, "eaqhm_noise_from_cepstrum_warped": 8}


# ---- the warp
@pytest.mark.parametrize("a", [0.42, -0.3, 0.9])
def test_identities_of_the_warp(a):
    """On 1001 points of [0, pi]: Omega_{-a} inverts Omega_a, and the rational map gives the cosine and sine of the atan2
    form.  Bars: a few ulp of pi, times the slope (1 + |a|) / (1 - |a|) of the warp for the inverse (the rounding of
    Omega_a(w) is carried through Omega_{-a}); this model measured <= 7e-16 and <= 4e-15 at a = 0.9."""
    from eaqhm_amd import allpass_warp
    w = np.linspace(0.0, np.pi, 1001)
    slope = (1 + abs(a)) / (1 - abs(a))
    om = W.omega(a, w)
    assert np.array_equal(allpass_warp(a, w), om)                      # the host's function is the definition
    assert om[0] == 0 and abs(om[-1] - np.pi) <= 2 * EPS * np.pi and np.all(np.diff(om) > 0)
    inv = float(np.abs(W.omega(-a, om) - w).max())
    cs, sn = W.rational(a, w)
    e_cos, e_sin = float(np.abs(cs - np.cos(om)).max()), float(np.abs(sn - np.sin(om)).max())
    edge = float(max(abs((om[1] - om[0]) / (w[1] - w[0]) / ((1 + a) / (1 - a)) - 1),
                     abs((om[-1] - om[-2]) / (w[1] - w[0]) / ((1 - a) / (1 + a)) - 1)))
    print("warp a %g: inverse %.3g, rational cos %.3g sin %.3g, edge slopes off by %.3g" % (a, inv, e_cos, e_sin, edge))
    record_measurement("cepwarp_identities_a%g" % a, inverse=inv, rational_cos=e_cos, rational_sin=e_sin)
    assert inv <= 4 * EPS * np.pi * slope
    assert e_cos <= 4 * EPS * np.pi * slope and e_sin <= 4 * EPS * np.pi * slope
    assert edge < 0.05                                                 # (1 + a) / (1 - a) at 0, its reciprocal at pi


# ---- moving rows between axes
@pytest.mark.parametrize("orders", [(20, 30), (63, 63)])
@pytest.mark.parametrize("b", [0.42, -0.42, 0.9])
def test_rewarp_matrix_against_quadrature(b, orders):
    """The recursion (the host's, rounded once to float64, and the model's in np.longdouble) against the midpoint rule
    on 2^14 points.  Bar: the quadrature's own error, its difference from the rule on 2^13 points, plus the rounding of
    its integrand's arguments (p x and j Omega at p, j <= 63 in np.longdouble: 2 x 63 pi eps_ld); the host's matrix adds
    its one rounding, eps / 2 of the entry."""
    from eaqhm_amd import rewarp_matrix
    Pi, Po = orders
    Q, Q2 = W.rewarp_quadrature(b, Pi, Po), W.rewarp_quadrature(b, Pi, Po, 2 ** 13)
    halving = float(np.abs(Q - Q2).max())
    bar = halving + 2 * 63 * np.pi * float(np.finfo(LD).eps)
    A_ld = W.rewarp_matrix(b, Pi, Po)
    A = rewarp_matrix(b, Pi, Po)
    assert A.dtype == np.float64 and A.shape == (Po + 1, Pi + 1)
    e_ld, e_host = float(np.abs(A_ld - Q).max()), float(np.abs(A - Q).max())
    print("rewarp b %g %d -> %d: quadrature halving %.3g, recursion %.3g, host %.3g" % (b, Pi, Po, halving, e_ld, e_host))
    record_measurement("cepwarp_rewarp_vs_quadrature_b%g_%d_%d" % (b, Pi, Po), halving=halving, recursion=e_ld,
                       host=e_host, bar=bar)
    assert e_ld <= bar
    assert e_host <= bar + 0.5 * EPS * float(np.abs(Q).max())
    assert np.array_equal(A, A_ld.astype(np.float64))                   # the same recursion, rounded once


def _geometric_rows(n=5, P=20, r=0.5):
    signs = np.where((np.arange(P + 1)[None, :] * (np.arange(n)[:, None] + 2)) % 3 == 0, -1.0, 1.0)
    C = signs * r ** np.arange(P + 1)[None, :]
    C[:, 0] = -4.0 + 0.5 * np.arange(n)
    return C


@pytest.mark.parametrize("a", [0.42, -0.3, 0.6])
def test_rewarp_round_trip_within_the_tail(a):
    """Rows of order 20 falling off as 0.5^p: to the axis a at order 63 and back to order 20.  What the cut at 63 drops
    moves the envelope by at most T = 2 sum_{p > 63} |c~_p|, taken from the transform of order 255, and a coefficient
    on the way back, a mean of the envelope against a cosine, by no more than T; two float64 products of at most 64
    terms with entries of A below 2 add 2 x 64 x 2 eps sum |c|."""
    from eaqhm_amd import cepstrum_rewarp
    C = _geometric_rows()
    full = C.astype(LD) @ W.rewarp_matrix(W.compose(0.0, a), 20, 255).T
    tail = 2 * np.abs(full[:, 64:]).sum(axis=1).astype(np.float64)
    there = cepstrum_rewarp(C, 0.0, a, 63)
    assert there.shape == (len(C), 64)
    assert np.abs(there - full[:, :64].astype(np.float64)).max() <= 64 * 2 * EPS * np.abs(C).sum(axis=1).max()
    back = cepstrum_rewarp(there, a, 0.0, 20)
    err = np.abs(back - C).max(axis=1)
    bar = tail + 2 * 64 * 2 * EPS * np.abs(C).sum(axis=1)
    print("rewarp round trip a %g: worst error %.3g, tail %.3g" % (a, err.max(), tail.max()))
    record_measurement("cepwarp_rewarp_round_trip_a%g" % a, error=float(err.max()), tail=float(tail.max()))
    assert np.all(err <= bar), (err, bar)
    # the envelope is the same function on either axis (the model's readout, no device)
    f = np.linspace(0.0, 8000.0, 41)
    same = np.abs(W.readout(there, 16000, f, a) - CR.readout(C, 16000, f)).max(axis=1)
    assert np.all(same <= tail + 1e-12 * (np.abs(C[:, 0]) + 2 * np.abs(C[:, 1:]).sum(axis=1)))


def test_rewarp_edge_cases():
    from eaqhm_amd import cepstrum_rewarp
    from eaqhm_amd.model import check_cepstrum_rewarp_arguments
    C = _geometric_rows()
    C[2] = 0.0
    C[2, 0] = -np.inf
    out = cepstrum_rewarp(C, 0.0, 0.42, 30)
    assert np.isneginf(out[2, 0]) and np.all(out[2, 1:] == 0) and np.all(np.isfinite(np.delete(out, 2, axis=0)))
    for a in (0.0, 0.42, -0.9):
        same = cepstrum_rewarp(C, a, a)
        assert np.array_equal(same, C) and same is not C                # equal warps and orders: the same bits
    padded = cepstrum_rewarp(C, 0.3, 0.3, 25)                           # equal warps, another order: cut or padded
    assert np.array_equal(padded[:, :21], C) and np.all(padded[:, 21:] == 0)
    assert np.array_equal(cepstrum_rewarp(C, 0.3, 0.3, 7), C[:, :8])
    assert check_cepstrum_rewarp_arguments(C, 0.2, 0.5)[1] == pytest.approx(0.3 / 0.9)
    for a_in, a_out in ((-0.6, 0.7), (0.9, -0.9), (0.7, -0.6)):         # |b| > 0.9
        with pytest.raises(ValueError, match="composed"):
            cepstrum_rewarp(C, a_in, a_out)
    for kw in (dict(cep_warp_in=np.nan), dict(cep_warp_in=0.91), dict(cep_warp_out="mel"), dict(cep_warp_out=-0.95),
               dict(order=0), dict(order=64), dict(order=2.5), dict(ceps=C[0]), dict(ceps=np.zeros((0, 5)))):
        args = dict(dict(ceps=C, cep_warp_in=0.0, cep_warp_out=0.42), **kw)
        with pytest.raises(ValueError):
            cepstrum_rewarp(**args)


# ---- cepstrum_warp
def test_cepstrum_warp_values():
    """The mel values of a 1e-4 grid search within twice that grid; the Bark values are the closed form."""
    from eaqhm_amd import cepstrum_warp
    for fs, want in ((8000, 0.3624), (16000, 0.4595), (22050, 0.5019), (44100, 0.5853), (48000, 0.5946)):
        got = cepstrum_warp(fs)
        record_measurement("cepwarp_mel_fs%d" % fs, a=got)
        assert abs(got - want) <= 2e-4, (fs, got)
        assert cepstrum_warp(fs, "mel") == got
        # the minimiser to 1e-6: the criterion is no smaller 2e-6 to either side
        t = np.arange(513)
        mel = np.log10(1 + (t * fs / 1024.0) / 700.0)

        def cost(a):
            return float(((W.omega(a, np.pi * t / 512.0) - np.pi * mel / mel[-1]) ** 2).sum())
        assert cost(got) <= cost(got + 2e-6) and cost(got) <= cost(got - 2e-6)
    for fs, want in ((16000, 0.5755), (44100, 0.7564)):
        got = cepstrum_warp(fs, "bark")
        assert got == 1.0674 * np.sqrt((2 / np.pi) * np.arctan(0.06583 * fs / 1000.0)) - 0.1916
        assert abs(got - want) <= 5e-5, (fs, got)
    for bad in (dict(scale="erb"), dict(scale=None), dict(fs=0), dict(fs=np.nan)):
        with pytest.raises(ValueError):
            cepstrum_warp(**dict(dict(fs=16000), **bad))
    assert "0.42" in cepstrum_warp.__doc__ and "caller's choice" in cepstrum_warp.__doc__


# ---- the claim the feature rests on
@pytest.mark.parametrize("f0,P,required", [(200.0, 18, 0.5), (110.0, 24, 0.6)])
def test_warped_fit_resolves_the_low_band(f0, P, required):
    """A four-formant all-pole envelope (450, 1100, 2600, 3600 Hz; bandwidths 60, 80, 120, 160 Hz) sampled at the
    harmonics of f0 up to 7.8 kHz, fs = 16 kHz, lam = 5e-4, fitted by the model on the linear axis and at a = 0.42: the
    rms log-amplitude error at the nodes below 1.5 kHz.  Required: the ratio warped / linear (measured 0.13 and 0.39)."""
    fs, lam = 16000, 5e-4
    f = np.arange(f0, 7800.0 + 1e-9, f0)
    v = W.four_formant_envelope(f, fs)
    rec = np.concatenate((np.exp(v), f, np.zeros(len(f)), [0.0]))[None, :]
    low = f < 1500.0
    lin = CR.readout(CR.fit(rec, fs, P, lam), fs, f)[0] - v
    assert np.array_equal(W.fit(rec, fs, P, lam, 0.0), CR.fit(rec, fs, P, lam))        # a = 0 is the linear model
    wrp = W.readout(W.fit(rec, fs, P, lam, 0.42), fs, f, 0.42)[0] - v
    e_lin, e_wrp = float(np.sqrt(np.mean(lin[low] ** 2))), float(np.sqrt(np.mean(wrp[low] ** 2)))
    print("low band f0 %g P %d: linear %.3f, warp 0.42 %.3f, ratio %.3f (required <= %g)"
          % (f0, P, e_lin, e_wrp, e_wrp / e_lin, required))
    record_measurement("cepwarp_low_band_f0%g_P%d" % (f0, P), linear=e_lin, warped=e_wrp, ratio=e_wrp / e_lin)
    assert e_wrp / e_lin <= required


def test_minimum_phase_of_the_warped_rows():
    """Phi of the warped rows is the minimum-phase response of the envelope they describe: moved to the linear axis at
    order 255, where the tail is below 1e-13, the linear model's Phi agrees to that tail and the rounding of the sums."""
    import model_build_ref as MB
    C = _geometric_rows(3, 20, 0.4)
    a, fs = 0.42, 16000
    f = np.linspace(0.0, 8000.0, 57)
    lin = (C.astype(LD) @ W.rewarp_matrix(W.compose(a, 0.0), 20, 255).T).astype(np.float64)
    assert np.abs(lin[:, 200:]).max() < 1e-13
    phi_w = W.phase(C, fs, f, a)
    phi_l = MB.series(lin, fs, f)[1]
    err = float(np.abs(phi_w - phi_l).max())
    record_measurement("cepwarp_minimum_phase", error=err)
    assert err <= 1e-11 and np.abs(phi_w).max() > 0.1


# ---- the host layer
@pytest.fixture()
def no_device(monkeypatch):
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


def _det(n=6, K=3):
    return dict(ti=np.arange(n) * 80, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
                frange=np.tile([200.0, 400.0, 600.0], (n, 1)), pk=np.zeros((n, K)))


BAD_WARPS = (np.nan, 0.91, -0.91, np.inf, "0.42", "mel", None, [0.42], True)


def test_every_new_keyword_is_checked_before_the_device(no_device):
    import eaqhm_amd as E
    det, fs = _det(), 16000
    C = np.zeros((6, 5))
    f0 = np.full(6, 200.0)
    calls = [lambda a: E.model_cepstrum(det, fs, 4, cep_warp=a),
             lambda a: E.cepstrum_envelope(C, fs, [100.0], cep_warp=a),
             lambda a: E.cepstrum_phase(C, fs, [100.0], cep_warp=a),
             lambda a: E.eaQHMSynthesis(det, fs, 401, envelope=C, cep_warp=a),
             lambda a: E.model_from_parameters(f0, C, fs, 80, cep_warp=a),
             lambda a: E.model_parameters(det, fs, 4, cep_warp=a),
             lambda a: E.noise_from_cepstrum(C, 64, fs, cep_warp=a),
             lambda a: E.cepstrum_rewarp(C, a, 0.0),
             lambda a: E.cepstrum_rewarp(C, 0.0, a),
             lambda a: E.check_cepstrum_warp(a)]
    for call in calls:
        for a in BAD_WARPS:
            with pytest.raises(ValueError, match="cep_warp|warp"):
                call(a)
    for a in (0.3, -0.9, 0.9):
        with pytest.raises(ValueError, match="envelope="):              # the axis of rows that are not there
            E.eaQHMSynthesis(det, fs, 401, cep_warp=a)
    assert E.check_cepstrum_warp(np.float32(0.5)) == 0.5 and E.check_cepstrum_warp(0) == 0.0
    assert E.check_cepstrum_warp(-0.9) == -0.9
    with pytest.raises(TypeError):                                      # keyword-only
        E.model_cepstrum(det, fs, 4, 5e-4, 0.42)
    with pytest.raises(TypeError):
        E.cepstrum_envelope(C, fs, [100.0], 1.0, None, 0.42)


class Recorder:
    """Stands in for hip.Context: records every call (tensors by shape, dtype and content) and zeroes the outputs."""

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")
        self.calls = []

    def _plain(self, x):
        if isinstance(x, self.torch.Tensor):
            return ("tensor", tuple(x.shape), str(x.dtype), x.detach().numpy().tobytes())
        if isinstance(x, tuple):
            return tuple(self._plain(v) for v in x)
        return x

    def __getattr__(self, name):
        def call(*args, **kw):
            outs = {"model_cepstrum": [6], "model_build": [11], "noise_from_cepstrum": [4, 5], "cepstrum_envelope": [6],
                    "cepstrum_phase": [6], "modify_amp_cepstrum": [7], "modify_prep": [11, 12, 13],
                    "spline_solve": [4, 5], "modify_synth": [15]}[name.replace("_warped", "")]
            for j in outs:
                args[j].zero_()
            self.calls.append((name, tuple(self._plain(v) for j, v in enumerate(args) if j not in outs),
                               {k: self._plain(v) for k, v in kw.items()}))
        return call


def _recorded(monkeypatch, fn):
    from eaqhm_amd import functions
    rec = Recorder()
    monkeypatch.setattr(functions, "_ctx", lambda device_index=0: rec)
    fn()
    return rec.calls


def test_cep_warp_zero_makes_the_old_calls(monkeypatch):
    """With cep_warp left out or 0 the host calls the Context methods that existed before, with the same arguments and
    no new keyword; with a != 0 it calls the *_warped sibling with the same arguments and cep_warp=a."""
    import eaqhm_amd as E
    det, fs = _det(), 16000
    rng = np.random.default_rng(3)
    C = np.concatenate((np.full((6, 1), -3.0), 0.1 * rng.standard_normal((6, 4))), axis=1)
    f0 = np.full(6, 200.0)
    warp = ([1000.0, 3000.0], [1100.0, 3000.0])
    cases = {
        "model_cepstrum": lambda **k: E.model_cepstrum(det, fs, 4, 1e-3, **k),
        "cepstrum_envelope": lambda **k: E.cepstrum_envelope(C, fs, [100.0, 9000.0], **k),
        "cepstrum_envelope_alpha": lambda **k: E.cepstrum_envelope(C, fs, [100.0], 1.2, **k),
        "cepstrum_phase_map": lambda **k: E.cepstrum_phase(C, fs, [100.0], formant_warp=warp, **k),
        "synthesis": lambda **k: E.eaQHMSynthesis(det, fs, 401, pitch_scale=1.2, formant_scale=1.1, envelope=C, **k),
        "model_build": lambda **k: E.model_from_parameters(f0, C, fs, 80, phase="zero", **k),
        "noise_from_cepstrum": lambda **k: E.noise_from_cepstrum(C, 64, fs, order=10, **k),
    }
    for label, fn in cases.items():
        old = _recorded(monkeypatch, lambda: fn())
        zero = _recorded(monkeypatch, lambda: fn(cep_warp=0.0))
        warped = _recorded(monkeypatch, lambda: fn(cep_warp=0.42))
        assert old and old == zero, label
        assert not any(name.endswith("_warped") or "cep_warp" in kw for name, _, kw in old), label
        assert [n for n, _, _ in old] == [n.replace("_warped", "") for n, _, _ in warped], label
        moved = [(o, w) for o, w in zip(old, warped) if o != w]
        assert len(moved) == 1, label                                   # one call changes: the one that reads the rows
        (name, args, kw), (wname, wargs, wkw) = moved[0]
        assert wname == name + "_warped" and wargs == args and wkw == dict(kw, cep_warp=0.42), label


def test_model_parameters_passes_the_axis_on(monkeypatch):
    from eaqhm_amd import cepstrum, model
    det, n = _det(), 6
    calls = []
    monkeypatch.setattr(cepstrum, "model_f0", lambda d, fs: np.full(n, 201.0))
    monkeypatch.setattr(cepstrum, "model_cepstrum", lambda d, fs, order, lam, **kw: calls.append(kw) or np.ones((n, 7)))
    p = model.model_parameters(det, 16000, 6, 1e-3)
    assert calls[-1] == dict(device_index=0) and "cep_warp" not in p
    p = model.model_parameters(det, 16000, 6, 1e-3, cep_warp=0.0)
    assert calls[-1] == dict(device_index=0) and "cep_warp" not in p
    p = model.model_parameters(det, 16000, 6, 1e-3, cep_warp=0.42, device_index=1)
    assert calls[-1] == dict(device_index=1, cep_warp=0.42) and p["cep_warp"] == 0.42
    assert sorted(p) == ["cep_warp", "ceps", "f0", "fs", "step", "voiced"]


# ---- the binding
def test_binding_header_and_library():
    import ctypes
    import eaqhm_amd
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    names = [n for n, _, _ in hip.SYMBOLS_CEPWARP]
    assert sorted(names) == sorted(WARPED_SYMBOLS)
    others = {n for n, _, _ in hip.SYMBOLS + hip.SYMBOLS_MLPG + hip.SYMBOLS_GV}
    assert not others & set(names)
    sibling = {n: a for n, _, a in hip.SYMBOLS}
    with open(os.path.join(ROOT, "include", "eaqhm_cepwarp.h")) as f:
        header = f.read()
    assert '#include "eaqhm_cepwarp.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    for name, res, args in hip.SYMBOLS_CEPWARP:
        assert res is ctypes.c_int and len(args) == WARPED_SYMBOLS[name], name
        assert args == sibling[name[:-len("_warped")]] + [ctypes.c_double], name      # the sibling's list plus one double
        decl = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert decl and len(decl.group(1).split(",")) == len(args) and "double cep_warp" in decl.group(1), name
        assert callable(getattr(hip.Context, name[len("eaqhm_"):]))
    lib = hip.load_library()
    for name in names:
        assert getattr(lib, name) is not None
    # a null context is EINVAL before anything else is read
    assert lib.eaqhm_model_cepstrum_warped(None, None, 1, 1, 16000.0, 4, 5e-4, None, 0.42) == -1
    assert lib.eaqhm_noise_from_cepstrum_warped(None, None, 1, 4, 4, None, None, 0.42) == -1
    csrc = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert "eaqhm_cepwarp.h" in makefile
    # the library is rebuilt when any file it is compiled from changes: every file that a source names in an
    # #include "..." and that exists in the tree is a prerequisite, listed in SRC or HDR
    listed = set()
    for var in ("SRC", "HDR"):
        listed |= {os.path.normpath(os.path.join(csrc, f))
                   for f in re.search(r"^%s\s*:?=\s*(.*)$" % var, makefile, re.M).group(1).split()}
    units = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".inc"))]
    assert units
    for unit in units:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(csrc, unit)).read(), re.M):
            path = os.path.normpath(os.path.join(csrc, inc))
            assert not os.path.exists(path) or path in listed, "%s includes %s: not in the Makefile" % (unit, inc)
    for name in ("cepstrum_rewarp", "cepstrum_warp", "allpass_warp", "rewarp_matrix", "check_cepstrum_warp"):
        assert callable(getattr(eaqhm_amd, name))


# ---- the CLI
def _saved_map(tmp_path, name, **extra):
    path = os.path.join(tmp_path, name)
    np.savez(path, order=np.int64(3), lam=np.float64(2e-3), fs=np.int64(16000), src_f0=np.array([5.0, 0.2]),
             tgt_f0=np.array([5.3, 0.25]), **dict(host_conversion(), **extra))
    return path


def test_cli_flag_and_its_errors(tmp_path):
    from eaqhm_amd import cli
    assert cli.parser().parse_args(["x.wav"]).cepstral_warp is None
    for text, want in (("0.42", 0.42), ("-0.9", -0.9), ("mel", "mel"), ("bark", "bark"), ("0", 0.0)):
        assert cli.parser().parse_args(["x.wav", "--cepstral-envelope", "--cepstral-warp", text]).cepstral_warp == want
    plain, warped = _saved_map(tmp_path, "plain.npz"), _saved_map(tmp_path, "warped.npz", cep_warp=np.float64(0.42))
    for argv in (["x.wav", "--cepstral-warp", "0.42"],                                    # none of its flags
                 ["x.wav", "--cepstral-warp", "0.42", "--pitch-scale", "1.2"],
                 ["x.wav", "--cepstral-warp", "mel", "--noise", "--noise-cepstrum"],
                 ["x.wav", "--cepstral-warp", "mel", "--noise", "--noise-from", "o.wav"],
                 ["x.wav", "--cepstral-envelope", "--cepstral-warp", "0.91"],
                 ["x.wav", "--cepstral-envelope", "--cepstral-warp", "-1"],
                 ["x.wav", "--cepstral-envelope", "--cepstral-warp", "nan"],
                 ["x.wav", "--cepstral-envelope", "--cepstral-warp", "erb"],
                 ["x.wav", "--cepstral-envelope", "--cepstral-warp"],
                 ["x.wav", "--conversion", warped, "--cepstral-warp", "0.5"],            # differs from the map's
                 ["x.wav", "--conversion", plain, "--cepstral-warp", "0.42"]):           # a map without the key: 0
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    missing = str(tmp_path / "missing.wav")
    for flags in (["--cepstral-envelope", "--cepstral-warp", "0.42"], ["--from-parameters", "24", "--cepstral-warp", "-0.3"],
                  ["--envelope-from", "o.wav", "--cepstral-warp", "0.42"], ["--timing-from", "o.wav", "--cepstral-warp", "0.9"],
                  ["--conversion-train", "t.wav", "--conversion-save", "m.npz", "--cepstral-warp", "0.42"],
                  ["--conversion", warped, "--cepstral-warp", "0.42"], ["--conversion", warped],
                  ["--conversion", plain, "--cepstral-warp", "0"],
                  ["--cepstral-envelope", "--cepstral-warp", "mel"]):
        with pytest.raises(FileNotFoundError):
            cli.main([missing] + flags)                                 # accepted: the analysis (or the read of fs) starts
    assert "--cepstral-warp" in cli.__doc__


def test_map_file_round_trip(tmp_path):
    from eaqhm_amd import check_conversion, cli
    plain, warped = _saved_map(tmp_path, "plain.npz"), _saved_map(tmp_path, "warped.npz", cep_warp=np.float64(0.42))
    assert "cep_warp" not in cli.load_conversion(plain)[0]
    conv = cli.load_conversion(warped)[0]
    assert conv["cep_warp"] == 0.42 and isinstance(conv["cep_warp"], float)
    again = check_conversion(conv)                                      # a validated map validates again
    assert again["cep_warp"] == 0.42
    assert check_conversion(dict(host_conversion(), cep_warp=0))["cep_warp"] == 0.0
    for bad in (np.nan, 0.95, -1.0, np.array([0.42]), "mel", True):
        with pytest.raises(ValueError):
            check_conversion(dict(host_conversion(), cep_warp=bad))


def _run_cli(tmp_path, monkeypatch, argv):
    """cli.main with stand-ins for the analysis and every device function: the keyword arguments they saw."""
    from eaqhm_amd import cli, convert, model
    n, L = 6, 200
    calls = []

    def model_cepstrum(det, fs, order=None, lam=5e-4, **kw):
        calls.append(("cepstrum", det["who"], kw))
        return np.zeros((n, (order or 18) + 1))

    def model_parameters(det, fs, order=None, lam=5e-4, **kw):
        calls.append(("parameters", det["who"], kw))
        return dict(f0=np.full(n, 100.0), ceps=np.zeros((n, (order or 18) + 1)), voiced=np.ones(n, bool), step=80,
                    fs=float(fs))

    def from_parameters(f0, ceps, fs, step, **kw):
        calls.append(("build", None, {k: v for k, v in kw.items() if k != "voiced"}))
        return {"who": "built"}

    def synthesis(det, fs, length, **kw):
        calls.append(("synth", det["who"], {k: kw[k] for k in ("cep_warp",) if k in kw},
                      kw.get("envelope") is not None))
        return np.zeros(length)

    monkeypatch.setattr(cli, "eaQHMAnalysisAndSynthesis", lambda path, gender, **o: (np.zeros(L), [1.0], {"who": path}, 0.0))
    monkeypatch.setattr(cli.wavfile, "read", lambda path: (16000, np.zeros(L)))
    monkeypatch.setattr(cli.wavfile, "write", lambda path, fs, x: None)
    monkeypatch.setattr(model, "model_cepstrum", model_cepstrum)
    monkeypatch.setattr(model, "model_parameters", model_parameters)
    monkeypatch.setattr(model, "model_from_parameters", from_parameters)
    monkeypatch.setattr(model, "model_align", lambda CA, CB, band=None, **kw: (np.stack((np.arange(n),) * 2, axis=1), 0.0))
    monkeypatch.setattr(model, "unpack_model", lambda det: {"step": 80})
    monkeypatch.setattr(model, "eaQHMSynthesis", synthesis)
    monkeypatch.setattr(convert, "conversion_apply", lambda conv, C, **kw: np.full((len(C), conv["dy"] + 1), -1.0))
    assert cli.main(argv) == 0
    return calls


def test_cli_dispatch(tmp_path, monkeypatch):
    from eaqhm_amd import cepstrum_warp
    ax = dict(cep_warp=0.42)
    # without the flag: today's calls, no new keyword anywhere
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--cepstral-envelope", "20"]) \
        == [("cepstrum", "x.wav", {}), ("synth", "x.wav", {}, True)]
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--cepstral-envelope", "20", "--cepstral-warp", "0"]) \
        == [("cepstrum", "x.wav", {}), ("synth", "x.wav", {}, True)]
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--cepstral-envelope", "20", "--cepstral-warp", "0.42"]) \
        == [("cepstrum", "x.wav", ax), ("synth", "x.wav", ax, True)]
    mel = dict(cep_warp=cepstrum_warp(16000))
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--cepstral-envelope", "--cepstral-warp", "mel"]) \
        == [("cepstrum", "x.wav", mel), ("synth", "x.wav", mel, True)]
    bark = dict(cep_warp=cepstrum_warp(16000, "bark"))
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--from-parameters", "24", "--cepstral-warp", "bark"]) \
        == [("parameters", "x.wav", bark), ("build", None, bark), ("synth", "built", {}, False)]
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--envelope-from", "o.wav", "--cepstral-warp", "0.42"]) \
        == [("cepstrum", "x.wav", ax), ("cepstrum", "o.wav", ax), ("synth", "x.wav", ax, True)]
    # the timing alone: the rows are aligned on the axis, the synthesis reads no envelope and gets no axis
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--timing-from", "o.wav", "--cepstral-warp", "0.42"]) \
        == [("cepstrum", "x.wav", ax), ("cepstrum", "o.wav", ax), ("synth", "x.wav", {}, False)]
    # a conversion: the map's axis, with or without the flag; a map without the key is on the linear axis
    warped, plain = _saved_map(tmp_path, "warped.npz", cep_warp=np.float64(0.42)), _saved_map(tmp_path, "plain.npz")
    want = [("parameters", "x.wav", ax), ("synth", "x.wav", ax, True)]
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--conversion", warped]) == want
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--conversion", warped, "--cepstral-warp", "0.42"]) == want
    assert _run_cli(tmp_path, monkeypatch, ["x.wav", "--conversion", plain]) \
        == [("parameters", "x.wav", {}), ("synth", "x.wav", {}, True)]


def test_cli_training_stores_the_axis(tmp_path, monkeypatch):
    from eaqhm_amd import cli, convert, model
    n = 12
    seen = []
    monkeypatch.setattr(model, "model_parameters", lambda det, fs, order=None, lam=5e-4, **kw: seen.append(kw) or dict(
        f0=np.full(n, 100.0), ceps=np.zeros((n, 4)), voiced=np.ones(n, bool), step=80, fs=fs))
    monkeypatch.setattr(cli, "align_other", lambda *a, **k: seen.append(k) or (np.zeros((n, 4)), np.zeros((n, 2), dtype=np.int64), {}, None))
    monkeypatch.setattr(convert, "conversion_pairs", lambda CA, CB, path, span=None, **k: (np.zeros((n, 3)), np.zeros((n, 3))))
    monkeypatch.setattr(convert, "conversion_train", lambda X, Y, components, **kw: host_conversion())
    out = os.path.join(tmp_path, "m.npz")
    a = cli.parser().parse_args(["x.wav", "--conversion-train", "t.wav", "--conversion-save", out])
    cli.train_conversion(a, "male", {}, 16000, {})
    assert seen == [{}, {}, {}] and "cep_warp" not in np.load(out).files
    assert "cep_warp" not in cli.load_conversion(out)[0]
    del seen[:]
    cli.train_conversion(a, "male", {}, 16000, {}, cep_warp=0.42)
    assert seen == [dict(cep_warp=0.42)] * 3
    assert float(np.load(out)["cep_warp"]) == 0.42 and cli.load_conversion(out)[0]["cep_warp"] == 0.42
