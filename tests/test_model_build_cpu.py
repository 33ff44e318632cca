"""A harmonic model from f0 and cepstral rows without a GPU: the NumPy model of the definition
(tests/model_build_ref.py) against independent routes, the host layer of model_from_parameters / cepstrum_phase /
model_parameters, the binding and the CLI flag."""
import os
import re

import numpy as np
import pytest

import model_build_ref as MB
import model_cepstrum_ref as CR
import model_synthesis_ref as M
from conftest import record_measurement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000.0
NEW_SYMBOLS = {"eaqhm_model_build": 13, "eaqhm_cepstrum_phase": 12}


def _rows(n, P, seed=0, c0=-4.0):
    rng = np.random.default_rng(seed)
    return np.concatenate((c0 + 0.3 * rng.standard_normal((n, 1)),
                           rng.standard_normal((n, P)) / (1.0 + np.arange(1, P + 1)) ** 1.2), axis=1)


def _bar(C):
    return 1e-12 * (np.abs(C[:, 0]) + 2 * np.abs(C[:, 1:]).sum(axis=1))


# ---- the model of the definition
@pytest.mark.parametrize("P", [1, 18, 63])
def test_minimum_phase_against_the_fft_of_the_causal_cepstrum(P):
    """H = exp(FFT(c_0, 2 c_1, .., 2 c_P, 0, ..)) on 1024 points: ln |H| is C and arg H is Phi (mod 2 pi) at
    f = k fs / 1024, k = 0..512."""
    N, n = 1024, 5
    C = _rows(n, P, seed=P)
    seq = np.zeros((n, N))
    seq[:, 0] = C[:, 0]
    seq[:, 1:P + 1] = 2 * C[:, 1:]
    H = np.exp(np.fft.fft(seq, axis=1))[:, :N // 2 + 1]
    f = np.arange(N // 2 + 1) * FS / N
    Cv, Phi = MB.series(C, FS, f)
    bar = _bar(C)[:, None]
    e_c = np.abs(np.log(np.abs(H)) - Cv)
    e_p = np.abs(np.angle(np.exp(1j * (np.angle(H) - Phi))))
    record_measurement("model_build_minimum_phase_vs_fft_P%d" % P, ln_error_over_bar=float((e_c / bar).max()),
                       phase_error_over_bar=float((e_p / bar).max()))
    assert np.all(e_c <= bar) and np.all(e_p <= bar), ((e_c / bar).max(), (e_p / bar).max())
    assert np.abs(Phi).max() > 0.1                                        # not a test of zeros
    assert np.array_equal(Cv, CR.clenshaw(C, FS, f))                      # §9.5's readout, operation for operation
    assert np.array_equal(Phi[:, 0], np.zeros(n)) and np.abs(Phi[:, -1]).max() <= bar.max()     # real at 0 and at fs/2


def test_series_in_longdouble_agrees_and_holds_past_nyquist():
    C = _rows(4, 18, seed=3)
    f = np.array([0.0, 310.0, 7999.0, 8000.0, 9000.0, -5.0])
    c64, p64 = MB.series(C, FS, f)
    cld, pld = MB.series(C, FS, f, np.longdouble)
    assert cld.dtype == np.longdouble and np.abs(c64 - cld).max() < 1e-13 and np.abs(p64 - pld).max() < 1e-13
    assert np.array_equal(c64[:, 3], c64[:, 4]) and np.array_equal(p64[:, 3], p64[:, 4])
    assert np.array_equal(c64[:, 0], c64[:, 5])


def _case(fs=16000, P=18, **kw):
    """9 instants: 1, 63, 64, 65 harmonics and some in between; instant 4 unvoiced, instant 7 an empty row."""
    f0 = np.array([5000.0, 125.0, 124.0, 123.0, 150.0, 310.0, 200.0, 180.0, 97.5])
    voiced = np.ones(9, bool)
    voiced[4] = False
    C = _rows(9, P, seed=11)
    C[7] = 0.0
    C[7, 0] = -np.inf
    return f0, voiced, C, fs, 80


def test_active_set():
    from eaqhm_amd.model import _records_f0, check_model_build_arguments, harmonic_counts, unpack_model
    f0, voiced, C, fs, D = _case()
    b = MB.build(f0, voiced, C, fs, D)
    assert b["counts"].tolist() == [1, 63, 64, 65, 0, 25, 39, 0, 82]
    assert b["Kmax"] == 82 and np.array_equal(b["active"].sum(axis=1), b["counts"])
    rec, K = b["records"], b["Kmax"]
    assert np.all(rec[:, :3 * K].reshape(9, 3, K)[np.broadcast_to(~b["active"][:, None, :], (9, 3, K))] == 0)
    assert np.all(rec[4] == 0) and np.all(rec[7] == 0)
    act = b["active"]
    assert np.all(rec[:, K:2 * K][act] < fs / 2) and np.all(np.abs(rec[:, 2 * K:3 * K]) <= np.pi)
    # the host's counts are the brute-force ones, at the edges too: f0 = (fs/2) / m exactly, and one ulp either side
    edge = np.concatenate([[8000.0 / m, np.nextafter(8000.0 / m, 0), np.nextafter(8000.0 / m, 1e9)]
                           for m in (1.5, 2, 3, 7, 63, 64, 65, 100, 1000, 1705, 1706, 1707, 3000)])
    for cap in (1706, 40, 1):
        assert np.array_equal(harmonic_counts(edge, 16000, cap), MB.counts(edge, np.ones(len(edge), bool), 16000, cap))
    assert harmonic_counts([5000.0], 16000, 1706)[0] == 1 and harmonic_counts([160.0], 48000, 1706)[0] == 149
    assert MB.build(np.full(3, 160.0), np.ones(3, bool), _rows(3, 5), 48000, 240)["Kmax"] == 149
    # the cap
    b40 = MB.build(f0, voiced, C, fs, D, kmax=40)
    assert b40["Kmax"] == 40 and b40["counts"].tolist() == [1, 40, 40, 40, 0, 25, 39, 0, 40]
    assert np.array_equal(b40["records"][:, :40], rec[:, :40]) and np.array_equal(b40["records"][:, 80:120],
                                                                                 rec[:, 2 * K:2 * K + 40])
    # the host agrees with the model on what it owes the kernel
    a = check_model_build_arguments(f0, C, fs, D, voiced)
    assert a["Kmax"] == 82 and a["Kcap"] == 1706 and np.array_equal(a["counts"], b["counts"])
    assert np.array_equal(a["theta"], b["theta"]) and a["f0"][4] == 0 and not a["zero_phase"]
    assert check_model_build_arguments(f0, C, fs, D, voiced, kmax=40)["Kmax"] == 40
    # f0 is held through the gap: instants 4 (unvoiced) and 7 (empty) advance theta at the previous f0
    g = MB.held(np.where(voiced, f0, 0.0), voiced & ~np.isneginf(C[:, 0]))
    assert g[4] == f0[3] and g[7] == f0[6] and np.array_equal(np.delete(g, [4, 7]), np.delete(f0, [4, 7]))
    th = b["theta"]
    assert th[5] == pytest.approx((th[4] + (D / fs) * (f0[3] + f0[5]) / 2) % 1.0, abs=1e-15)
    lead = MB.held(np.array([0.0, 0.0, 210.0, 0.0]), np.array([False, False, True, False]))
    assert lead.tolist() == [210.0] * 4                                   # none earlier: the nearest later one
    # model_f0's formula returns f0; unpack_model takes the records whole
    m = unpack_model(MB.det(rec, K, D, voiced))
    assert m["quirk_cells"] == 0 and m["Kmax"] == K and m["step"] == D and np.array_equal(m["records"], rec)
    got = _records_f0(rec, K)
    has = b["counts"] > 0
    assert np.abs(got[has] / f0[has] - 1).max() <= 1e-12
    assert got[4] == got[3] and got[7] == got[6]
    # the default voicing
    assert np.array_equal(check_model_build_arguments(np.where(voiced, f0, 0.0), C, fs, D)["voiced"], voiced)
    assert np.array_equal(check_model_build_arguments(np.where(voiced, f0, np.nan), C, fs, D)["voiced"], voiced)


def test_phases():
    f0, voiced, C, fs, D = _case()
    b = MB.build(f0, voiced, C, fs, D, theta0=0.3)
    z = MB.build(f0, voiced, C, fs, D, theta0=0.3, zero_phase=True)
    K = b["Kmax"]
    act = b["active"]
    assert np.array_equal(b["records"][:, :2 * K], z["records"][:, :2 * K]) and np.all(z["phi"] == 0)
    h = np.arange(1, K + 1)
    want = np.angle(np.exp(2j * np.pi * h[None, :] * b["theta"][:, None]))
    d = np.angle(np.exp(1j * (z["records"][:, 2 * K:3 * K] - want)))
    assert np.abs(d[act]).max() < 1e-12
    d = np.angle(np.exp(1j * (b["records"][:, 2 * K:3 * K] - want - b["phi"])))
    assert np.abs(d[act]).max() < 1e-12 and np.abs(b["phi"][act]).max() > 0.1
    assert b["theta"][0] == 0.3 and np.all((b["theta"][1:] >= 0) & (b["theta"][1:] < 1))
    x = np.array([np.pi, -np.pi, 0.0, 3 * np.pi, 7.0, -7.0, 2 * np.pi])
    w = MB.wrap(x)
    assert np.all((w > -np.pi) & (w <= np.pi)) and w[0] == np.pi and w[1] == np.pi
    assert np.abs(np.angle(np.exp(1j * (w - x)))).max() < 1e-15
    # longdouble: the same active set, nearly the same numbers
    bl = MB.build(f0, voiced, C, fs, D, theta0=0.3, dtype=np.longdouble)
    assert np.array_equal(bl["active"], act) and np.array_equal(bl["records"][:, K:2 * K], b["records"][:, K:2 * K])
    dev = np.abs(np.angle(np.exp(1j * (bl["phase"] - b["phase"]).astype(np.float64))))[act].max()
    assert 0 < dev < 1e-11


def test_an_underflowing_cell_is_inactive():
    C = np.zeros((3, 3))
    C[:, 0] = -700.0
    C[:, 1] = 30.0                       # C(0) = -640, C(fs/2) = -760: exp underflows towards Nyquist
    b = MB.build(np.full(3, 500.0), np.ones(3, bool), C, 16000, 80)
    act = b["active"]
    assert act[:, 0].all() and not act[:, -1].any() and b["Kmax"] == 15
    assert np.all(b["records"][:, :45].reshape(3, 3, 15)[:, :, ~act[0]] == 0)


def test_periodicity_of_a_constant_model():
    """f0 = 200 Hz at 16 kHz, step 80 = one period: every instant holds the same record, and the synthesis of
    model_synthesis_ref repeats with the period.  The residue y[n + 80] - y[n] is the model's own periodicity error."""
    n, D, fs = 12, 80, 16000
    C = np.tile(_rows(1, 18, seed=2), (n, 1))
    b = MB.build(np.full(n, 200.0), np.ones(n, bool), C, fs, D)
    rec, K = b["records"], b["Kmax"]
    assert K == 39 and np.array_equal(rec, np.tile(rec[:1], (n, 1)))
    L = (n - 1) * D + 1
    y = M.synthesize(rec, D, fs, L)
    core = y[D:L - D]
    err = float(np.abs(core[D:] - core[:-D]).max() / np.abs(y).max())
    print("model build periodicity: %.3g of the peak" % err)
    record_measurement("model_build_periodicity", error_over_peak=err)
    assert err < 1e-8
    assert np.abs(y).max() > 1e-3


# ---- the host layer
@pytest.fixture()
def no_device(monkeypatch):
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


def test_check_model_build_arguments(no_device):
    from eaqhm_amd import model_from_parameters
    from eaqhm_amd.model import check_model_build_arguments
    f0, voiced, C, fs, D = _case()
    good = check_model_build_arguments(f0, C, fs, D, voiced, "zero", 0.25, 1706, np.arange(9.0))
    assert good["zero_phase"] and good["theta"][0] == 0.25 and good["a0"][8] == 8 and good["step"] == 80
    assert good["ceps"].flags["C_CONTIGUOUS"] and good["fs"] == 16000.0
    assert check_model_build_arguments(f0[:2], C[:2], fs, D)["Kmax"] == 63             # n = 2 is a model
    assert check_model_build_arguments(f0, C, fs, D, voiced, kmax=1)["Kmax"] == 1
    nan = f0.copy()
    nan[4] = np.nan                                                                     # unvoiced: not read
    assert check_model_build_arguments(nan, C, fs, D, voiced)["f0"][4] == 0
    bad_C = C.copy()
    bad_C[2, 3] = np.nan
    half = C.copy()
    half[2, 0] = -np.inf
    bad = [dict(f0=f0[:1], ceps=C[:1], voiced=None), dict(step=0), dict(step=-80), dict(step=80.5), dict(step="x"),
           dict(step=True), dict(fs=0.0), dict(fs=np.nan)]
    for j, v in ((1, np.nan), (1, np.inf), (1, 0.0), (1, -100.0), (1, 8000.0), (1, 9000.0)):
        f = f0.copy()
        f[j] = v
        bad.append(dict(f0=f))
    bad += [dict(f0=f0[None]), dict(f0="x"), dict(f0=f0.astype(complex)),
            dict(ceps=bad_C), dict(ceps=half), dict(ceps=C[:8]), dict(ceps=C[:, :1]), dict(ceps=np.zeros((9, 65))),
            dict(ceps=C[0]), dict(ceps=None),
            dict(theta0=np.nan), dict(theta0=np.inf), dict(theta0="x"), dict(theta0=None),
            dict(kmax=0), dict(kmax=1707), dict(kmax=-1), dict(kmax=2.5), dict(kmax="x"),
            dict(phase="independent"), dict(phase="shape"), dict(phase=None), dict(phase=0),
            dict(voiced=np.zeros(9, bool)), dict(voiced=voiced[:8]), dict(voiced=np.ones(9)), dict(voiced="x"),
            dict(f0=np.zeros(9), voiced=None),
            dict(a0=np.zeros(8)), dict(a0=np.full(9, np.nan)), dict(a0="x")]
    base = dict(f0=f0, ceps=C, fs=fs, step=D, voiced=voiced)
    for kw in bad:
        args = dict(base, **kw)
        with pytest.raises(ValueError):
            check_model_build_arguments(**args)
        with pytest.raises(ValueError):
            model_from_parameters(args.pop("f0"), args.pop("ceps"), args.pop("fs"), args.pop("step"), **args)


def test_cepstrum_phase_arguments(no_device):
    from eaqhm_amd import cepstrum_phase
    C = _rows(8, 5)
    good = ([1000.0, 8000.0], [900.0, 8000.0])
    for kw in (dict(formant_scale=9.0), dict(formant_scale=np.ones(7)), dict(formant_warp=([1000.0], [4100.0])),
               dict(formant_scale=1.2, formant_warp=good), dict(formant_scale="x")):
        with pytest.raises(ValueError):
            cepstrum_phase(C, FS, [100.0], **kw)
    for freqs in ([], [-1.0], [np.nan], [[1.0]]):
        with pytest.raises(ValueError):
            cepstrum_phase(C, FS, freqs)
    nan = C.copy()
    nan[0, 3] = np.nan
    for ceps in (nan, C[:, :1], np.zeros((8, 65)), C[0], np.zeros((0, 6))):
        with pytest.raises(ValueError):
            cepstrum_phase(ceps, FS, [100.0])
    with pytest.raises(ValueError):
        cepstrum_phase(C, 0.0, [100.0])


def test_model_parameters_is_a_composition(monkeypatch):
    from eaqhm_amd import cepstrum, model
    n, K = 6, 3
    det = dict(ti=np.arange(n) * 15, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
               frange=np.tile([200.0, 400.0, 600.0], (n, 1)), pk=np.zeros((n, K)))
    det["amplitudes"][2] = 0.0
    det["isVoiced"][4] = False
    calls = []
    monkeypatch.setattr(cepstrum, "model_f0", lambda d, fs: calls.append(("f0", d is det, fs)) or np.full(n, 201.0))
    monkeypatch.setattr(cepstrum, "model_cepstrum", lambda d, fs, order, lam, device_index=0:
                        calls.append(("ceps", d is det, fs, order, lam, device_index)) or np.ones((n, 7)))
    p = model.model_parameters(det, 16000, 6, 1e-3, device_index=2)
    assert calls == [("f0", True, 16000), ("ceps", True, 16000, 6, 1e-3, 2)]
    assert sorted(p) == ["ceps", "f0", "fs", "step", "voiced"]
    assert p["voiced"].tolist() == [True, True, False, True, False, True] and p["step"] == 15 and p["fs"] == 16000.0
    assert np.all(p["f0"] == 201.0) and p["ceps"].shape == (n, 7)
    p = model.model_parameters(det, 16000)
    assert calls[-1] == ("ceps", True, 16000, None, 5e-4, 0)


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
    for name in ("model_from_parameters", "cepstrum_phase", "model_parameters"):
        assert callable(getattr(eaqhm_amd, name))
    for name in ("model_build", "cepstrum_phase"):
        assert callable(getattr(hip.Context, name))
    assert callable(eaqhm_amd.model.check_model_build_arguments)
    with open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "eaqhm_cepstrum.hip")) as f:
        src = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r'extern "C" int %s\(' % name, src) and (name + "_kernel") in src


def test_cli_flag_and_its_exclusions(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav"])
    assert a.from_parameters is None
    assert cli.parser().parse_args(["x.wav", "--from-parameters"]).from_parameters == 0      # 0: the default order
    a = cli.parser().parse_args(["x.wav", "--from-parameters", "24", "--cepstral-lambda", "1e-4"])
    assert a.from_parameters == 24 and a.cepstral_lambda == 1e-4
    missing = str(tmp_path / "missing.wav")
    for flags in (["--from-parameters", "--no-envelope"], ["--from-parameters", "20", "--no-envelope"]):
        with pytest.raises(SystemExit):
            cli.main([missing] + flags)
    for flags in (["--from-parameters", "64"], ["--from-parameters", "-2"], ["--from-parameters", "--cepstral-lambda", "2"],
                  ["--from-parameters", "--pitch-scale", "9"]):
        with pytest.raises(ValueError):
            cli.main([missing] + flags)                        # rejected before the analysis
    for flags in (["--from-parameters"], ["--from-parameters", "30", "--cepstral-lambda", "1e-5"],
                  ["--from-parameters", "--time-scale", "1.5", "--pitch-scale", "0.8", "--formant-scale", "1.1"],
                  ["--from-parameters", "--phase", "shape", "--noise"], ["--from-parameters", "--cepstral-envelope", "20"]):
        with pytest.raises(FileNotFoundError):
            cli.main([missing] + flags)                        # accepted: the analysis starts


def test_cli_writes_the_vocoded_file(tmp_path, monkeypatch):
    """The flag's data flow, with every device call replaced: analysis -> model_parameters -> model_from_parameters ->
    eaQHMSynthesis of the rebuilt model -> <name>_vocoded.wav."""
    from scipy.io import wavfile
    from eaqhm_amd import cli, model
    fs, L = 16000, 400
    wav = str(tmp_path / "a.wav")
    wavfile.write(wav, fs, np.zeros(L, dtype=np.int16))
    det, built = object(), object()
    seen = {}
    monkeypatch.setattr(cli, "eaQHMAnalysisAndSynthesis", lambda path, gender, **kw: (np.zeros(L), [1.0], det, None))

    def parameters(d, fs_, order, lam, **kw):
        seen["parameters"] = (d is det, fs_, order, lam)
        return dict(f0="f0", ceps="ceps", voiced="voiced", step=15, fs=float(fs_))

    def from_parameters(f0, ceps, fs_, step, **kw):
        seen["build"] = (f0, ceps, fs_, step, kw)
        return built

    def synthesis(d, fs_, length, **kw):
        seen.setdefault("synth", []).append((d, fs_, length, kw))
        return np.full(length, 0.25 if d is built else 0.5)

    monkeypatch.setattr(model, "model_parameters", parameters)
    monkeypatch.setattr(model, "model_from_parameters", from_parameters)
    monkeypatch.setattr(model, "eaQHMSynthesis", synthesis)
    assert cli.main([wav, "--from-parameters", "20", "--cepstral-lambda", "1e-3", "--pitch-scale", "1.25"]) == 0
    assert seen["parameters"] == (True, fs, 20, 1e-3)
    assert seen["build"] == ("f0", "ceps", float(fs), 15, dict(voiced="voiced"))
    by = {id(d): kw for d, _, _, kw in seen["synth"]}
    assert by[id(built)]["pitch_scale"] == 1.25 and "envelope" not in by[id(built)]
    assert by[id(det)]["pitch_scale"] == 1.25                   # a scale flag still writes _modified.wav from the model
    rate, out = wavfile.read(str(tmp_path / "a_vocoded.wav"))
    assert rate == fs and len(out) == L and np.all(out == np.float32(0.25))
    assert np.all(wavfile.read(str(tmp_path / "a_modified.wav"))[1] == np.float32(0.5))
    # the flag alone: the default order and lambda, and no _modified.wav
    os.remove(str(tmp_path / "a_modified.wav"))
    seen.clear()
    assert cli.main([wav, "--from-parameters"]) == 0
    assert seen["parameters"] == (True, fs, None, 5e-4) and [d for d, *_ in seen["synth"]] == [built]
    assert not os.path.exists(str(tmp_path / "a_modified.wav"))
