"""The noise model to and from cepstral rows, the parts that need no GPU: the NumPy model
(tests/noise_cepstrum_ref.py) against the closed form and through its own round trip, the argument checks of
noise_cepstrum and noise_from_cepstrum (no device work before them), noise_alignment_index, the binding, the header and
the CLI flags."""
import os

import numpy as np
import pytest

import noise_cepstrum_ref as R
from conftest import ROOT


@pytest.mark.parametrize("p", [1, 2, 4, 18])
@pytest.mark.parametrize("r", [0.7, 0.9])
def test_recursion_agrees_with_the_closed_form(p, r):
    """c_n = Re sum_i z_i^n / (2 n) from the poles the fixture was built from, n = 1..63, within 1e-12 (p <= 18: at
    p = 50 np.poly's conditioning, not the recursion, separates the two)."""
    sigma, refl, poles = R.pole_frames(5, p, r, seed=3)
    got = R.cepstrum(sigma, refl, 63)
    worst = 0.0
    for m in range(5):
        worst = max(worst, float(np.abs(got[m, 1:] - R.closed_form(poles[m], 63)).max()))
        assert got[m, 0] == np.log(sigma[m])
    print("recursion against closed form p %d r %g: %.3g" % (p, r, worst))
    assert worst <= 1e-12


def test_silent_frames_and_orders():
    sigma, refl, _ = R.pole_frames(6, 4, 0.7, silent=(0, 3, 5))
    for Q in (1, 3, 4, 5, 63):
        C = R.cepstrum(sigma, refl, Q)
        assert C.shape == (6, Q + 1)
        assert np.array_equal(np.isneginf(C[:, 0]), sigma == 0) and np.all(C[sigma == 0, 1:] == 0)
        assert np.all(np.isfinite(C[sigma > 0]))
        assert np.array_equal(C, R.cepstrum(sigma, refl, 63)[:, :Q + 1])       # a lower order is a prefix
    s2, k2, stop = R.from_cepstrum(R.cepstrum(sigma, refl, 63), 4)
    assert np.array_equal(s2 == 0, sigma == 0) and np.all(k2[sigma == 0] == 0) and not stop.any()


@pytest.mark.parametrize("p", [4, 18, 50])
def test_model_round_trip(p):
    """frames -> cepstrum (Q = 63) -> frames on the smooth fixture (r = 0.7): refl within 1e-8, sigma within 1e-8
    relative.  On the sharp fixture (r = 0.9) the error is what the cut at Q = 63 and the grid leave: printed, no bar."""
    for r, bar in ((0.7, 1e-8), (0.9, None)):
        sigma, refl, _ = R.pole_frames(7, p, r, seed=11)
        s2, k2, stop = R.from_cepstrum(R.cepstrum(sigma, refl, 63), p)
        err_k = float(np.abs(k2 - refl).max())
        err_s = float(np.abs(s2 / sigma - 1).max())
        print("model round trip p %d r %g: refl %.3g sigma %.3g (relative)" % (p, r, err_k, err_s))
        assert not stop.any()
        if bar is not None:
            assert err_k <= bar and err_s <= bar


def test_column_zero_only_sets_the_level():
    sigma, refl, _ = R.pole_frames(3, 18, 0.7, seed=5)
    C = R.cepstrum(sigma, refl, 63)
    s1, k1, _ = R.from_cepstrum(C, 18)
    C2 = C.copy()
    C2[:, 0] += 2.5
    s2, k2, _ = R.from_cepstrum(C2, 18)
    assert np.array_equal(k1, k2)
    assert np.abs(s2 / (s1 * np.exp(2.5)) - 1).max() <= 16 * np.finfo(float).eps


def test_cepstrum_reads_as_the_envelope():
    """2 C(w) is the log power spectrum of noise_warp_ref up to the cut's remainder 2 p r^{Q+1} / ((Q+1)(1-r)) (in C)."""
    import noise_warp_ref as W
    p, r, Q = 18, 0.7, 63
    sigma, refl, _ = R.pole_frames(5, p, r, seed=2)
    fn = np.linspace(0, 0.5, 65)
    rem = 2 * p * r ** (Q + 1) / ((Q + 1) * (1 - r))
    diff = np.abs(2 * R.readout(R.cepstrum(sigma, refl, Q), 2 * np.pi * fn) - W.envelope(sigma, refl, 1.0, fn)).max()
    assert diff <= 2 * rem + 1e-12


# ---- host logic
def _model(Nf=26, p=4, hop=8, fs=1600.0):
    return dict(sigma=np.full(Nf, 0.1), refl=np.zeros((Nf, p)), hop=hop, order=p, fs=fs, length=(Nf - 1) * hop + 1)


def _arrays_model(n=8, K=2, step=15):
    ti = np.arange(n) * step
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
                frange=np.tile([200.0, 400.0], (n, 1))[:, :K], pk=np.zeros((n, K)))


def _rows(Nf=26, Q=5):
    C = np.zeros((Nf, Q + 1))
    C[:, 0] = np.log(0.1)
    C[:, 1] = 0.2
    return C


@pytest.fixture()
def no_device(monkeypatch):
    """Any device work is a failure: the argument checks come first."""
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


def test_noise_cepstrum_rejects(no_device):
    from eaqhm_amd import noise_cepstrum
    for bad in ("model", dict(sigma=np.zeros(3)), dict(_model(), order=64), dict(_model(), refl=np.ones((26, 4))),
                dict(_model(), sigma=np.full(26, -1.0))):
        with pytest.raises(ValueError):
            noise_cepstrum(bad)
    for order in (0, 64, -1, 2.5, "x", None, True):
        with pytest.raises(ValueError):
            noise_cepstrum(_model(), order)
    with pytest.raises(AssertionError):        # a good call passes the checks and reaches the device
        noise_cepstrum(_model(), 1)
    with pytest.raises(AssertionError):
        noise_cepstrum(_model())


@pytest.mark.parametrize("kw", [
    dict(ceps="x"), dict(ceps=np.zeros(6)), dict(ceps=np.zeros((4, 1))), dict(ceps=np.zeros((4, 65))),
    dict(ceps=np.zeros((0, 6))), dict(ceps=np.full((4, 6), np.nan)), dict(ceps=np.full((4, 6), -np.inf)),
    dict(ceps=np.r_[[[-np.inf, 0, 0, 1.0]], np.zeros((3, 4))]),              # an empty row with a nonzero coefficient
    dict(ceps=np.r_[[[0.0, 151.0, 0, 0]], np.zeros((3, 4))]),                # 4 sum |c_q| = 604 > 600
    dict(ceps=np.r_[[[0.0, 100.0, -51.0, 0]], np.zeros((3, 4))]),
    dict(ceps=np.r_[[[650.0, 30.0, 0, 0]], np.zeros((3, 4))]),               # sigma would overflow
    dict(hop=0), dict(hop=1025), dict(hop=2.5), dict(hop="x"), dict(hop=True),
    dict(order=0), dict(order=64), dict(order=1.5), dict(hop=2, order=8),    # order < 4 hop
    dict(fs=0.0), dict(fs=np.nan), dict(fs="x"),
    dict(length=0), dict(length=26 * 8 + 1), dict(length=25 * 8), dict(length=2.5),
    dict(mod=np.zeros((26, 4))), dict(mod_harmonics=2), dict(mod=np.zeros((26, 3)), mod_harmonics=2),
    dict(mod=np.zeros((25, 4)), mod_harmonics=2), dict(mod=np.zeros((26, 18)), mod_harmonics=9),
    dict(mod=np.full((26, 4), np.nan), mod_harmonics=2)])
def test_noise_from_cepstrum_rejects(kw, no_device):
    from eaqhm_amd import noise_from_cepstrum
    args = dict(ceps=_rows(), hop=8, fs=1600.0)
    args.update(kw)
    with pytest.raises(ValueError):
        noise_from_cepstrum(args.pop("ceps"), args.pop("hop"), args.pop("fs"), **args)


def test_noise_from_cepstrum_checks_pass_good_calls(no_device):
    from eaqhm_amd import noise_from_cepstrum
    from eaqhm_amd.model import check_noise_from_cepstrum_arguments, check_noise_cepstrum_arguments
    C, shell = check_noise_from_cepstrum_arguments(_rows(), 8, 1600)
    assert C.flags["C_CONTIGUOUS"] and C.dtype == np.float64
    assert shell == dict(hop=8, order=4, fs=1600.0, length=201)              # min(63, 2 + round(1.6)), (Nf - 1) hop + 1
    C, shell = check_noise_from_cepstrum_arguments(_rows(), 8, 16000.0, length=208)
    assert shell["order"] == 18 and shell["length"] == 208
    rows = _rows()
    rows[3] = 0
    rows[3, 0] = -np.inf                                                      # an empty row is fine
    rows[4, 1:] = [150.0, 0, 0, 0, 0]                                         # 4 sum |c_q| = 600 exactly
    C, shell = check_noise_from_cepstrum_arguments(rows, 8, 1600.0, order=7, mod=np.zeros((26, 4)), mod_harmonics=2)
    assert shell["order"] == 7 and shell["mod_harmonics"] == 2 and shell["mod"].shape == (26, 4)
    assert "sigma" not in shell and "refl" not in shell
    nz, Q = check_noise_cepstrum_arguments(_model(), 7)
    assert Q == 7 and nz["order"] == 4
    assert check_noise_cepstrum_arguments(_model())[1] == 63
    with pytest.raises(AssertionError):        # a good call passes the checks and reaches the device
        noise_from_cepstrum(_rows(), 8, 1600.0)


def test_noise_alignment_index_identity_is_exact():
    from eaqhm_amd import noise_alignment_index
    for n, step, hop in ((12, 15, 8), (30, 7, 5), (400, 15, 80), (9, 48, 240)):
        det = _arrays_model(n=n, step=step)
        Nf = (n - 1) * step // hop + 1                                        # every frame at or before the last instant
        nz = _model(Nf=Nf, hop=hop)
        j = noise_alignment_index(np.arange(n), det, nz, det, nz)
        assert j.dtype == np.float64 and np.array_equal(j, np.arange(Nf)), (n, step, hop)


def test_noise_alignment_index_by_hand():
    """A: instants 0, 10, 20, 30 (step 10), noise hop 4, 9 frames at 0, 4, .., 32.  B: instants 0, 6, .., 30 (step 6),
    noise hop 5, 7 frames.  idx = (0, 1.5, 2, 5): A's instants sit at B's samples 0, 9, 12, 30."""
    from eaqhm_amd import noise_alignment_index
    detA, detB = _arrays_model(n=4, step=10), _arrays_model(n=6, step=6)
    nzA, nzB = _model(Nf=9, hop=4), _model(Nf=7, hop=5)
    j = noise_alignment_index([0, 1.5, 2, 5], detA, nzA, detB, nzB)
    # sample of A -> sample of B: 0->0, 4->3.6, 8->7.2, 12->9.6, 16->10.8, 20->12, 24->19.2, 28->26.4, 32->30 (held)
    want = np.array([0, 3.6, 7.2, 9.6, 10.8, 12, 19.2, 26.4, 30]) / 5
    assert j.shape == (9,) and np.abs(j - want).max() <= 1e-14
    assert j[-1] == 6.0
    # clipped at both ends: B's noise model has fewer frames than its instants span; idx past B's instants is held
    short = _model(Nf=4, hop=5)
    j = noise_alignment_index([0, 1.5, 2, 5], detA, nzA, detB, short)
    assert j.max() == 3.0 and np.all(j[want >= 3] == 3.0) and np.all(j[:3] == want[:3])
    j = noise_alignment_index([-2, 1.5, 2, 9], detA, nzA, detB, nzB)
    assert j[0] == 0.0 and j[-1] == 6.0 and np.all(np.diff(j) >= 0)
    for bad in ([0, 1, 2], [0, 1, np.nan, 3], "x", np.zeros((4, 1))):
        with pytest.raises(ValueError):
            noise_alignment_index(bad, detA, nzA, detB, nzB)
    with pytest.raises(ValueError):
        noise_alignment_index([0, 1.5, 2, 5], detA, nzA, detB, dict(nzB, fs=8000.0))
    with pytest.raises(ValueError):
        noise_alignment_index([0, 1.5, 2, 5], detA, "model", detB, nzB)


def test_binding_header_and_exports():
    import eaqhm_amd
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    sym = {n: a for n, _, a in hip.SYMBOLS}
    assert len(sym["eaqhm_noise_cepstrum"]) == 7 and len(sym["eaqhm_noise_from_cepstrum"]) == 7
    for name in ("noise_cepstrum", "noise_from_cepstrum", "noise_alignment_index"):
        assert callable(getattr(eaqhm_amd, name))
    assert callable(hip.Context.noise_cepstrum) and callable(hip.Context.noise_from_cepstrum)
    header = open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    for name in sym:
        assert name + "(" in header, name
    assert "int eaqhm_noise_cepstrum(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf" in header
    assert "int eaqhm_noise_from_cepstrum(eaqhm_ctx* ctx, const double* ceps, int32_t Nf" in header


def test_cli_flags(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav", "--noise", "--noise-cepstrum"])
    assert a.noise_cepstrum == 63 and a.noise_from is None
    assert cli.parser().parse_args(["x.wav", "--noise", "--noise-cepstrum", "24"]).noise_cepstrum == 24
    assert cli.parser().parse_args(["x.wav", "--noise"]).noise_cepstrum is None
    assert cli.parser().parse_args(["x.wav", "--noise", "--noise-from", "y.wav"]).noise_from == "y.wav"
    missing, other = str(tmp_path / "missing.wav"), str(tmp_path / "other.wav")
    for argv in (["--noise-cepstrum"], ["--noise-from", other],                              # both need --noise
                 ["--noise", "--noise-from", other, "--noise-modulation"],
                 ["--noise", "--noise-from", other, "--noise-modulation", "3"],
                 ["--noise", "--noise-cepstrum", "--align-band", "1.0"]):                   # nothing to align
        with pytest.raises(SystemExit):
            cli.main([missing] + argv)
    for q in ("0", "64", "-3"):
        with pytest.raises(ValueError):
            cli.main([missing, "--noise", "--noise-cepstrum", q])                            # rejected before the analysis
    for argv in (["--noise", "--noise-cepstrum"], ["--noise", "--noise-cepstrum", "12", "--noise-modulation"],
                 ["--noise", "--noise-from", other], ["--noise", "--noise-from", other, "--align-band", "1.0"],
                 ["--noise", "--noise-from", other, "--envelope-from", other, "--noise-cepstrum", "30"]):
        with pytest.raises(FileNotFoundError):
            cli.main([missing] + argv)                                                       # accepted: the analysis starts
