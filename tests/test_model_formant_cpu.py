"""The formant scale, the parts that need no GPU: the NumPy model against the §9 / §9.1 models at
alpha = 1 and alpha = beta, the shift property of the envelope, and the argument checks of eaQHMSynthesis,
model_envelope and the CLI."""
import numpy as np
import pytest

import model_contour_ref as MC
import model_formant_ref as MF
import model_synthesis_ref as M
from test_model_synthesis_cpu import golden_model

GOLDEN_MODELS = ["sa19_female_default.npz", "seed16k_1p2s_adpt6.npz"]


@pytest.fixture(scope="module", params=GOLDEN_MODELS)
def golden(request):
    from eaqhm_amd.functions import pack_results
    from eaqhm_amd.model import unpack_model
    g, plan, fin = golden_model(request.param)
    return unpack_model(pack_results(plan, fin))


def _fields(m):
    K = m["Kmax"]
    rec = m["records"]
    return rec[:, :K], rec[:, K:2 * K]


@pytest.mark.parametrize("beta", [0.5, 0.8, 1.0, 1.25, 2.0])
def test_unit_alpha_gives_the_envelope_amplitudes_bit_for_bit(golden, beta):
    am, fm = _fields(golden)
    ref = M.envelope_amplitudes(am, fm, 16000, beta, True)
    assert np.array_equal(MF.formant_amplitudes(am, fm, 16000, beta, 1.0), ref)
    n = len(am)
    b = np.where(np.arange(n) % 3 == 0, 1.0, beta * (1 + 0.1 * np.sin(np.arange(n))))
    ref_c = MC.envelope_amplitudes_per_instant(am, fm, 16000, b, True)
    assert np.array_equal(MF.formant_amplitudes(am, fm, 16000, b, np.ones(n)), ref_c)


def _tied(am, fm):
    """Active slots whose frequency another active slot of the same instant shares."""
    act = (am != 0) & (fm > 0)
    tied = np.zeros_like(act)
    for i in range(len(am)):
        ks = np.flatnonzero(act[i])
        _, inv, cnt = np.unique(fm[i, ks], return_inverse=True, return_counts=True)
        tied[i, ks] = cnt[inv] > 1
    return tied


def _slopes(am, fm):
    """Per active slot: the steeper |d ln a / d f| of the envelope's two segments at the slot's node, and the distance
    to the nearest other node."""
    slope = np.zeros_like(am)
    gap = np.full_like(am, np.inf)
    for i in range(len(am)):
        ks = np.flatnonzero((am[i] != 0) & (fm[i] > 0))
        if len(ks) < 2:
            continue
        f, v = MF.envelope_nodes(am[i], fm[i])
        d = np.abs(np.diff(v) / np.where(np.diff(f) > 0, np.diff(f), np.inf))
        s = np.maximum(np.r_[0.0, d], np.r_[d, 0.0])
        g = np.minimum(np.r_[np.inf, np.diff(f)], np.r_[np.diff(f), np.inf])
        pos = np.searchsorted(f, fm[i, ks], side="left")
        slope[i, ks], gap[i, ks] = s[pos], g[pos]
    return slope, gap


@pytest.mark.parametrize("beta", [0.7, 1.2, 1.5, 3.0])
def test_alpha_equal_beta_keeps_each_partials_amplitude(beta):
    """SA19, the reference's model: exp(E(beta f / beta)) is each partial's own amplitude up to the rounding of q.
    That rounding (an ulp of f) is multiplied by the envelope's slope, which is steep between nodes a few Hz apart:
    1e-12 relative where both neighbour nodes are >= 10 Hz away, |q - f| times the slope everywhere."""
    from eaqhm_amd.functions import pack_results
    from eaqhm_amd.model import unpack_model
    _, plan, fin = golden_model("sa19_female_default.npz")
    am, fm = _fields(unpack_model(pack_results(plan, fin)))
    ref = M.envelope_amplitudes(am, fm, 16000, beta, False)
    out = MF.formant_amplitudes(am, fm, 16000, beta, beta)
    keep = ~_tied(am, fm) & (ref != 0)
    assert np.count_nonzero(keep) > 1000
    assert np.array_equal(out[~keep & (am != 0)] == 0, ref[~keep & (am != 0)] == 0)
    slope, gap = _slopes(am, fm)
    rel = np.abs(out[keep] - ref[keep]) / ref[keep]
    far = gap[keep] >= 10.0
    assert np.count_nonzero(far) > 0.9 * len(far)
    assert rel[far].max() <= 1e-12
    dq = np.abs((beta * fm[keep]) / beta - fm[keep])
    assert np.all(np.abs(np.log(out[keep]) - np.log(ref[keep])) <= dq * slope[keep] * (1 + 1e-9) + 1e-13)


def test_envelope_shift_property(golden):
    """E read at f / alpha off the unscaled envelope is the scaled envelope at f; a feature at F moves to alpha F."""
    rec = golden["records"]
    am, fm = _fields(golden)
    freqs = np.linspace(0.0, 8000.0, 257)
    for alpha in (0.5, 0.8, 1.25, 2.0):
        scaled = MF.envelope_readout(rec, freqs, alpha)
        assert np.array_equal(scaled, MF.envelope_readout(rec, freqs / alpha, 1.0))
    # dyadic scales move a feature exactly: E_alpha(alpha F) == E_1(F)
    for alpha in (0.5, 2.0):
        assert np.array_equal(MF.envelope_readout(rec, alpha * freqs, alpha), MF.envelope_readout(rec, freqs, 1.0))
    # at the node frequencies the unscaled envelope is ln am (the first of tied nodes)
    i = int(np.argmax(np.count_nonzero(am, axis=1)))
    ks = np.flatnonzero((am[i] != 0) & (fm[i] > 0) & ~_tied(am, fm)[i])
    row = MF.envelope_readout(rec[i:i + 1], fm[i, ks], 1.0)[0]
    assert np.array_equal(row, np.log(am[i, ks]))
    # instants without active slots read -inf
    empty = ~np.any((am != 0) & (fm > 0), axis=1)
    assert empty.any()
    assert np.all(np.isneginf(MF.envelope_readout(rec[empty], freqs, 1.3)))


def test_formant_amplitudes_mute_at_the_output_frequency():
    """Muting follows beta f, not q: alpha moves the reading point only."""
    am = np.array([[0.1, 0.2, 0.3]])
    fm = np.array([[1000.0, 5000.0, 7000.0]])
    out = MF.formant_amplitudes(am, fm, 16000, 1.2, 2.0)        # 1.2 * 7000 = 8400 >= 8000
    assert out[0, 2] == 0.0 and out[0, 0] > 0 and out[0, 1] > 0
    out = MF.formant_amplitudes(am, fm, 16000, 1.0, 0.5)         # q = 14000 beyond the last node: flat
    assert out[0, 2] == pytest.approx(0.3, rel=1e-15) and out[0, 1] == pytest.approx(0.3, rel=1e-15)


def _arrays_model(n=8, K=2, step=15):
    ti = np.arange(n) * step
    am = np.full((n, K), 0.1)
    fm = np.tile([200.0, 400.0], (n, 1))[:, :K]
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=am, frange=fm, pk=np.zeros((n, K)))


@pytest.mark.parametrize("kw", [dict(formant_scale=5.0), dict(formant_scale=0.2), dict(formant_scale=np.nan),
                                dict(formant_scale=np.inf), dict(formant_scale="x"), dict(formant_scale=np.ones(7)),
                                dict(formant_scale=np.ones(9)), dict(formant_scale=np.r_[np.ones(7), np.nan]),
                                dict(formant_scale=np.r_[np.ones(7), 4.5]), dict(formant_scale=np.ones((2, 8))),
                                dict(formant_scale=1.2, preserve_envelope=False),
                                dict(formant_scale=np.r_[np.ones(7), 1.1], preserve_envelope=False),
                                dict(formant_scale=1.2, time_scale=np.ones(7))])
def test_bad_formant_scales_raise(kw):
    """These raise before any device work, so they run without a GPU."""
    from eaqhm_amd.model import eaQHMSynthesis
    with pytest.raises(ValueError):
        eaQHMSynthesis(_arrays_model(), 16000, 200, **kw)


def test_formant_scale_checks():
    from eaqhm_amd.model import check_formant_scale, unpack_model
    m = unpack_model(_arrays_model())
    assert check_formant_scale(m, 1.2, True) == 1.2
    assert check_formant_scale(m, 1, False) == 1.0
    a = check_formant_scale(m, np.ones(8), False)     # a contour of ones scales nothing: no envelope needed
    assert a.dtype == np.float64 and np.array_equal(a, np.ones(8))
    assert np.array_equal(check_formant_scale(m, [0.9] * 8, True), np.full(8, 0.9))


@pytest.mark.parametrize("freqs, kw", [([], {}), ([100.0, np.nan], {}), ([100.0, -1.0], {}), ([100.0, np.inf], {}),
                                       ([[100.0, 200.0]], {}), (["a"], {}), ([100.0], dict(formant_scale=5.0)),
                                       ([100.0], dict(formant_scale=np.ones(7))), ([100.0], dict(fs=-1.0)),
                                       ([100.0], dict(formant_scale=np.r_[np.ones(7), np.nan]))])
def test_model_envelope_rejects(freqs, kw):
    from eaqhm_amd.model import model_envelope
    args = dict(fs=16000)
    args.update(kw)
    fs = args.pop("fs")
    with pytest.raises(ValueError):
        model_envelope(_arrays_model(), fs, freqs, **args)


def test_model_envelope_needs_four_instants():
    from eaqhm_amd.model import model_envelope
    with pytest.raises(ValueError):
        model_envelope(_arrays_model(n=3), 16000, [100.0])


@pytest.mark.parametrize("flags", [["--formant-scale", "1.2", "--formant-scale-curve", "c.txt"],
                                   ["--formant-scale", "1.2", "--no-envelope"],
                                   ["--formant-scale-curve", "c.txt", "--no-envelope"],
                                   ["--pitch-scale", "1.5", "--formant-scale", "1.2", "--no-envelope"]])
def test_cli_rejects_formant_flag_conflicts(flags, tmp_path):
    from eaqhm_amd import cli
    with pytest.raises(SystemExit):
        cli.main([str(tmp_path / "missing.wav")] + flags)


def test_cli_rejects_a_bad_formant_scale_before_the_analysis(tmp_path):
    from eaqhm_amd import cli
    with pytest.raises(ValueError):
        cli.main([str(tmp_path / "missing.wav"), "--formant-scale", "5"])
    bad = tmp_path / "bad.txt"
    bad.write_text("0.0 1.0\n1.0 9.0\n")
    with pytest.raises(ValueError):
        cli.main([str(tmp_path / "missing.wav"), "--formant-scale-curve", str(bad)])
