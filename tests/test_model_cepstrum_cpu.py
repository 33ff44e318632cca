"""The discrete-cepstrum envelope without a GPU: the NumPy model of DESIGN.md §9.5 (tests/model_cepstrum_ref.py) against
itself (two fits, the shift property, the normal equations, Clenshaw against the direct sum), the host validation of
model_cepstrum / cepstrum_envelope / eaQHMSynthesis(envelope=), the binding and the CLI flags."""
import os
import re

import numpy as np
import pytest

import model_cepstrum_ref as CR
from conftest import ROOT

FS = 16000.0
EPS = np.finfo(np.float64).eps
NEW_SYMBOLS = {"eaqhm_model_cepstrum": 8, "eaqhm_modify_amp_cepstrum": 13, "eaqhm_cepstrum_envelope": 12}


def harmonic_records(n, fs, seed, kmax=None):
    """n random harmonic instants as records: f0 in [80, 300] Hz, harmonics up to 0.45 fs, ln am a two-formant shape
    plus 0.3 of noise.  Rows are padded with inactive slots."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        f0 = rng.uniform(80.0, 300.0)
        f = f0 * np.arange(1, int(0.45 * fs / f0) + 1)
        lna = (-3.0 - f / 4000.0 + 2.0 * np.exp(-((f - 700.0) / 300.0) ** 2) + 1.5 * np.exp(-((f - 2400.0) / 500.0) ** 2)
               + 0.3 * rng.standard_normal(len(f)))
        rows.append((f, np.exp(lna)))
    K = max(len(f) for f, _ in rows) if kmax is None else kmax
    rec = np.zeros((n, 3 * K + 1))
    for i, (f, a) in enumerate(rows):
        rec[i, :len(f)] = a
        rec[i, K:K + len(f)] = f
    return rec


SETTINGS = [(16000.0, 18), (16000.0, 63), (48000.0, 50), (48000.0, 63)]


@pytest.mark.parametrize("lam", [5e-4, 1e-6])
@pytest.mark.parametrize("fs,P", SETTINGS)
def test_the_two_reference_fits_agree(fs, P, lam):
    """The normal equations in float64, the same in np.longdouble and the QR of the augmented system give the same
    coefficients.  Bar per instant: 8 n cond(G) eps max|c| with n = P + 1: the normal equations solved by a backward
    stable method lose cond(G) eps, and forming G and b from n-term sums of rounded cosines a small multiple of n more."""
    rec = harmonic_records(24, fs, seed=int(fs) + P)
    K = (rec.shape[1] - 1) // 3
    c64, cld, cqr = CR.fit(rec, fs, P, lam), CR.fit(rec, fs, P, lam, np.longdouble), CR.fit_qr(rec, fs, P, lam)
    worst = worst_qr = worst_cond = 0.0
    for i in range(len(rec)):
        G, _ = CR.system(*CR.nodes(rec[i, :K], rec[i, K:2 * K], fs), P, lam)
        cond = float(np.linalg.cond(G))
        bar = 8 * (P + 1) * cond * EPS * float(np.abs(c64[i]).max())
        d = float(np.abs(c64[i] - cld[i]).max())
        dq = float(np.abs(cqr[i] - cld[i]).max())
        assert d <= bar and dq <= bar, (i, d, dq, bar, cond)
        worst, worst_qr, worst_cond = max(worst, d), max(worst_qr, dq), max(worst_cond, cond)
    print("fs %g P %d lam %g: float64 - longdouble %.3g, QR - longdouble %.3g, cond <= %.3g"
          % (fs, P, lam, worst, worst_qr, worst_cond))
    assert worst > 0


def test_a_constant_on_ln_am_moves_c0_alone():
    """M's first column is the constant, and c_0 is not penalised."""
    rec = harmonic_records(6, FS, seed=3)
    K = (rec.shape[1] - 1) // 3
    shifted = rec.copy()
    shifted[:, :K] *= np.exp(1.75)
    for P, lam in ((5, 5e-4), (18, 5e-4), (40, 1e-6)):
        a, b = CR.fit(rec, FS, P, lam, np.longdouble), CR.fit(shifted, FS, P, lam, np.longdouble)
        # ln(am e^1.75) is 1.75 + ln am up to the rounding of the float64 amplitudes: a few eps of |ln am| <= 10
        assert np.abs((b[:, 0] - a[:, 0]) - 1.75).max() <= 1e-12
        assert np.abs(b[:, 1:] - a[:, 1:]).max() <= 1e-12


def test_the_normal_equations_hold_for_the_fit():
    rec = harmonic_records(6, 48000.0, seed=4)
    K = (rec.shape[1] - 1) // 3
    for P, lam in ((18, 5e-4), (63, 1e-6)):
        c = CR.fit(rec, 48000.0, P, lam, np.longdouble)
        for i in range(len(rec)):
            G, b = CR.system(*CR.nodes(rec[i, :K], rec[i, K:2 * K], 48000.0, np.longdouble), P, lam, np.longdouble)
            res = np.abs(G @ c[i] - b).max()
            scale = np.abs(G).sum(axis=1).max() * np.abs(c[i]).max()
            assert res <= 64 * (P + 1) * np.finfo(np.longdouble).eps * scale, (P, lam, i, res, scale)


def test_fewer_nodes_than_coefficients_and_no_node():
    rec = np.zeros((3, 3 * 4 + 1))
    rec[0, :2], rec[0, 4:6] = [0.1, 0.05], [300.0, 600.0]
    rec[1, 2], rec[1, 6] = 0.2, 1234.5             # a single node
    c = CR.fit(rec, FS, 12, 5e-4)
    assert np.all(np.isfinite(c[:2]))
    assert np.isneginf(c[2, 0]) and np.all(c[2, 1:] == 0)
    # one node: the penalty wants every c_p, p >= 1, at 0 and c_0 is free: c_0 = ln am
    assert abs(c[1, 0] - np.log(0.2)) <= 1e-12 and np.abs(c[1, 1:]).max() <= 1e-12
    env = CR.envelope(c, FS, np.array([0.0, 1234.5, 9000.0]))
    assert np.all(np.isneginf(env[2])) and np.abs(env[1] - np.log(0.2)).max() <= 1e-12


@pytest.mark.parametrize("fs,P", SETTINGS)
def test_clenshaw_equals_the_direct_sum(fs, P):
    """On fitted cepstra, on a grid from 0 to beyond fs/2 (the hold): within 1e-13 (|c_0| + 2 sum |c_p|), a tenth of
    the GPU readout's bar."""
    rec = harmonic_records(8, fs, seed=P)
    c = CR.fit(rec, fs, P, 5e-4)
    q = np.linspace(0.0, 0.6 * fs, 33)
    direct, rec_ = CR.readout(c, fs, q), CR.clenshaw(c, fs, q)
    scale = np.abs(c[:, 0]) + 2 * np.abs(c[:, 1:]).sum(axis=1)
    err = np.abs(direct - rec_).max(axis=1) / scale
    print("fs %g P %d: Clenshaw - direct sum, relative to the coefficient sum: %.3g" % (fs, P, err.max()))
    assert err.max() <= 1e-13
    past = q >= fs / 2
    assert past.sum() > 1 and np.array_equal(direct[:, past], np.repeat(CR.readout(c, fs, [fs / 2]), past.sum(), axis=1))
    empty = np.zeros((1, P + 1))
    empty[0, 0] = -np.inf
    assert np.all(np.isneginf(CR.clenshaw(empty, fs, q))) and np.all(np.isneginf(CR.readout(empty, fs, q)))


def test_amplitude_rule():
    rec = harmonic_records(5, FS, seed=9, kmax=100)
    K = 100
    am, fm = rec[:, :K], rec[:, K:2 * K]
    c = CR.fit(rec, FS, 18, 5e-4)
    c[3] = 0.0
    c[3, 0] = -np.inf
    A1 = CR.amplitudes(am, fm, FS, 1.0, c)
    active = (am != 0) & (fm > 0)
    assert np.all(A1[~active] == 0) and np.all(A1[3] == 0) and np.all(A1[[0, 1, 2, 4]][active[[0, 1, 2, 4]]] > 0)
    assert not np.array_equal(A1[0], am[0])                       # no unit rule: the envelope is the caller's
    A2 = CR.amplitudes(am, fm, FS, 1.25, c)
    assert np.array_equal(A2 == 0, ~(active & (1.25 * fm < FS / 2)) | (np.arange(5) == 3)[:, None])
    # alpha and beta cancel: the envelope is read where it was
    A3 = CR.amplitudes(am, fm, FS, 1.25, c, alpha=1.25)
    keep = A3 != 0
    assert np.abs(np.log(A3[keep]) - np.log(A1[keep])).max() <= 1e-12
    # B = 1 with (x, alpha x) is the scale alpha
    A4 = CR.amplitudes(am, fm, FS, 1.0, c, warp=(np.array([1000.0]), np.array([1180.0])))
    A5 = CR.amplitudes(am, fm, FS, 1.0, c, alpha=1.18)
    keep = A5 != 0
    assert np.abs(np.log(A4[keep]) - np.log(A5[keep])).max() <= 1e-10


# ---- the host layer
def _arrays_model(n=8, K=2, step=15):
    ti = np.arange(n) * step
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
                frange=np.tile([200.0, 400.0], (n, 1))[:, :K], pk=np.zeros((n, K)))


@pytest.fixture()
def no_device(monkeypatch):
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


def test_check_model_cepstrum_arguments(no_device):
    from eaqhm_amd import model_cepstrum
    from eaqhm_amd.model import check_model_cepstrum_arguments, unpack_model
    det = _arrays_model()
    m = unpack_model(det)
    assert check_model_cepstrum_arguments(m, 16000, None, 5e-4) == (16000.0, 18, 5e-4)
    assert check_model_cepstrum_arguments(m, 48000)[1] == 50 and check_model_cepstrum_arguments(m, 96000)[1] == 63
    assert check_model_cepstrum_arguments(m, FS, 1, 1e-6) == (FS, 1, 1e-6)
    assert check_model_cepstrum_arguments(m, FS, 63, 1.0) == (FS, 63, 1.0)
    for order in (0, 64, -3, 2.5, "x", True):
        with pytest.raises(ValueError):
            check_model_cepstrum_arguments(m, FS, order)
        with pytest.raises(ValueError):
            model_cepstrum(det, FS, order)
    for lam in (0.0, 9e-7, 1.0001, -1e-3, np.nan, np.inf, "x", None):
        with pytest.raises(ValueError):
            check_model_cepstrum_arguments(m, FS, 18, lam)
        with pytest.raises(ValueError):
            model_cepstrum(det, FS, lam=lam)
    for fs in (0.0, np.nan, "x"):
        with pytest.raises(ValueError):
            model_cepstrum(det, fs)
    bad = _arrays_model()
    bad["amplitudes"][3, 1] = np.nan
    with pytest.raises(ValueError):
        model_cepstrum(bad, FS)
    bad = _arrays_model()
    bad["amplitudes"][3, 1] = -0.1
    with pytest.raises(ValueError):
        model_cepstrum(bad, FS)


def _good_envelope(n=8, P=5):
    C = np.zeros((n, P + 1))
    C[:, 0] = -3.0
    C[:, 1] = 0.4
    return C


def test_check_envelope_cepstrum(no_device):
    from eaqhm_amd import eaQHMSynthesis
    from eaqhm_amd.model import check_envelope_cepstrum, unpack_model
    det = _arrays_model()
    m = unpack_model(det)
    C = _good_envelope()
    out = check_envelope_cepstrum(m, C, True)
    assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, C)
    assert check_envelope_cepstrum(m, C[:, :2], True).shape == (8, 2)                  # P = 1
    assert check_envelope_cepstrum(m, np.zeros((8, 64)), True).shape == (8, 64)          # P = 63
    row = C.copy()
    row[2] = 0.0
    row[2, 0] = -np.inf                                                                # an empty row is allowed
    assert np.isneginf(check_envelope_cepstrum(m, row, True)[2, 0])
    bad = []
    for i, j, v in ((1, 2, np.nan), (1, 0, np.nan), (1, 2, np.inf), (1, 2, -np.inf), (1, 0, np.inf)):
        B = C.copy()
        B[i, j] = v
        bad.append(B)
    half = C.copy()
    half[4, 0] = -np.inf                # -inf with nonzero coefficients behind it
    bad += [half, C[:7], C[:, :1], np.zeros((8, 65)), C[0], C[None], "x", None, C.astype(complex), [[None] * 6] * 8]
    for B in bad:
        with pytest.raises(ValueError):
            check_envelope_cepstrum(m, B, True)
        if B is not None:
            with pytest.raises(ValueError):
                eaQHMSynthesis(det, FS, 200, envelope=B)
    with pytest.raises(ValueError):
        check_envelope_cepstrum(m, C, False)
    with pytest.raises(ValueError):
        eaQHMSynthesis(det, FS, 200, envelope=C, preserve_envelope=False)
    with pytest.raises(ValueError):                                   # the existing rules still hold next to it
        eaQHMSynthesis(det, FS, 200, envelope=C, formant_scale=1.2, formant_warp=([1000.0], [1100.0]))


def test_cepstrum_envelope_arguments(no_device):
    from eaqhm_amd import cepstrum_envelope
    C = _good_envelope()
    good = ([1000.0, 8000.0], [900.0, 8000.0])
    for scale in (1.2, np.ones(8), np.full(8, 1.1)):
        with pytest.raises(ValueError):
            cepstrum_envelope(C, FS, [100.0], scale, good)
    for kw in (dict(formant_scale=9.0), dict(formant_scale=np.ones(7)), dict(formant_warp=([1000.0], [4100.0])),
               dict(formant_warp=(good[0], np.tile(good[1], (7, 1)))), dict(formant_scale="x")):
        with pytest.raises(ValueError):
            cepstrum_envelope(C, FS, [100.0], **kw)
    for freqs in ([], [-1.0], [np.nan], [[1.0]]):
        with pytest.raises(ValueError):
            cepstrum_envelope(C, FS, freqs)
    nan = C.copy()
    nan[0, 3] = np.nan
    for ceps in (nan, C[:, :1], np.zeros((8, 65)), C[0], np.zeros((0, 6))):
        with pytest.raises(ValueError):
            cepstrum_envelope(ceps, FS, [100.0])
    with pytest.raises(ValueError):
        cepstrum_envelope(C, 0.0, [100.0])


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
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(eaqhm_\w+)\(", header, re.M))
    assert declared == set(sym), declared ^ set(sym)
    with open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "eaqhm_common.h")) as f:
        assert re.search(r"#define EAQHM_ABI_VERSION 6\b", f.read())
    for name in ("model_cepstrum", "cepstrum_envelope", "eaQHMSynthesis"):
        assert callable(getattr(eaqhm_amd, name))
    for name in ("model_cepstrum", "modify_amp_cepstrum", "cepstrum_envelope"):
        assert callable(getattr(hip.Context, name))
    for name in ("check_model_cepstrum_arguments", "check_envelope_cepstrum"):
        assert callable(getattr(eaqhm_amd.model, name))


def test_cli_flags_and_their_exclusions(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav"])
    assert a.cepstral_envelope is None and a.cepstral_lambda is None
    a = cli.parser().parse_args(["x.wav", "--cepstral-envelope"])
    assert a.cepstral_envelope == 0 and a.cepstral_lambda is None                 # 0: the default order
    a = cli.parser().parse_args(["x.wav", "--cepstral-envelope", "24", "--cepstral-lambda", "1e-4", "--pitch-scale", "1.2"])
    assert a.cepstral_envelope == 24 and a.cepstral_lambda == 1e-4 and a.pitch_scale == 1.2
    missing = str(tmp_path / "missing.wav")
    for flags in (["--cepstral-envelope", "--no-envelope"], ["--cepstral-envelope", "20", "--no-envelope"],
                  ["--cepstral-lambda", "1e-3"], ["--cepstral-lambda", "1e-3", "--pitch-scale", "1.2"]):
        with pytest.raises(SystemExit):
            cli.main([missing] + flags)
    for flags in (["--cepstral-envelope", "64"], ["--cepstral-envelope", "-2"],
                  ["--cepstral-envelope", "--cepstral-lambda", "2"], ["--cepstral-envelope", "--cepstral-lambda", "1e-7"]):
        with pytest.raises(ValueError):
            cli.main([missing] + flags)                        # rejected before the analysis
    for flags in (["--cepstral-envelope"], ["--cepstral-envelope", "30", "--cepstral-lambda", "1e-5"],
                  ["--cepstral-envelope", "--time-scale", "1.5", "--pitch-scale", "0.8", "--formant-scale", "1.1"],
                  ["--cepstral-envelope", "--formant-vtln", "1.1", "--phase", "shape"],
                  ["--cepstral-envelope", "--noise", "--noise-formant", "--formant-scale", "1.1"]):
        with pytest.raises(FileNotFoundError):
            cli.main([missing] + flags)                        # accepted: the analysis starts
