"""Resynthesis from the model (model.py), the parts that need no GPU: the NumPy model of the definition anchored to the
reference's own returned model and s_recon, unpack_model as the inverse of pack_results / pack_arrays, the envelope
rules and the argument checks."""
import types

import numpy as np
import pytest

import model_synthesis_ref as M
from conftest import load_golden


def golden_model(name):
    """The reference's returned model of a fixture as (records, L, structs-like plan/fin for pack_results)."""
    g = load_golden(name)
    cells = g["det_cells"]
    n = len(g["det_ti"])
    K = int(cells[:, 1].max()) + 1
    i, k = cells[:, 0], cells[:, 1]
    am = np.zeros((n, K))
    fm = np.zeros((n, K))
    pk = np.zeros((n, K))
    am[i, k], fm[i, k], pk[i, k] = g["det_am"], g["det_fm"], g["det_pk"]
    a0 = np.where(g["det_isVoiced"], g["det_a0"], 0.0)
    plan = types.SimpleNamespace(ti=g["det_ti"] + 1, analysed=g["det_isVoiced"].astype(bool),
                                 in_bounds=g["det_isSpeech"].astype(bool), No_ti=n)
    fin = dict(am=am, fm=fm, pk=pk, a0=a0)
    return g, plan, fin


@pytest.mark.parametrize("name, quirks", [("sa19_female_default.npz", 0), ("seed16k_1p2s_adpt6.npz", 170)])
def test_numpy_model_reproduces_reference_s_recon(name, quirks):
    """Reference anchor: at rho = beta = 1 the definition, run on the model the reference returned, is its s_recon.
    The seeding fixture holds 170 slot-0 cells of amplitude 10e-4 and frequency 0 that s_recon never used: treated as
    active they break the identity."""
    from eaqhm_amd.functions import pack_results
    from eaqhm_amd.model import unpack_model
    g, plan, fin = golden_model(name)
    m = unpack_model(pack_results(plan, fin))
    assert m["quirk_cells"] == quirks and m["step"] == 15
    out = M.synthesize(m["records"], m["step"], 16000, len(g["s_recon"]))
    assert out.shape == g["s_recon"].shape
    assert np.abs(out - g["s_recon"]).max() <= 1e-9
    if quirks:
        rec = m["records"].copy()
        K = m["Kmax"]
        q = (fin["am"] != 0) & (fin["fm"] <= 0)
        rec[:, :K][q] = fin["am"][q]
        assert np.abs(M.synthesize(rec, 15, 16000, len(g["s_recon"])) - g["s_recon"]).max() > 1e-6


@pytest.mark.parametrize("form", ["structs", "arrays"])
@pytest.mark.parametrize("name", ["sa19_female_default.npz", "seed16k_1p2s_adpt6.npz"])
def test_unpack_model_inverts_packing(name, form):
    from eaqhm_amd.functions import pack_arrays, pack_results
    from eaqhm_amd.model import unpack_model
    g, plan, fin = golden_model(name)
    det = pack_results(plan, fin) if form == "structs" else pack_arrays(plan, fin)
    m = unpack_model(det)
    K = fin["am"].shape[1]
    assert m["Kmax"] == K and m["step"] == 15 and np.array_equal(m["ti"], g["det_ti"])
    rec = m["records"]
    assert rec.shape == (plan.No_ti, 3 * K + 1)
    quirk = (fin["am"] != 0) & (fin["fm"] <= 0)
    assert m["quirk_cells"] == int(quirk.sum())
    keep = (fin["am"] != 0) & ~quirk
    for col, key in ((0, "am"), (1, "fm"), (2, "pk")):
        got = rec[:, col * K:(col + 1) * K]
        assert np.array_equal(got[keep], fin[key][keep])
        assert np.all(got[~keep] == 0)
    assert np.array_equal(rec[:, 3 * K], fin["a0"])


def test_unpack_model_of_hand_edited_structs():
    """Cells written by hand as plain numbers, a zeroed slot and a row without slots."""
    from eaqhm_amd.functions import pack_results
    from eaqhm_amd.model import unpack_model
    g, plan, fin = golden_model("sa19_female_default.npz")
    det = pack_results(plan, fin)
    i = int(np.flatnonzero(plan.analysed)[10])
    det[i].amplitudes[0] = 0.5
    det[i].amplitudes[1] = 0
    m = unpack_model(det)
    K = m["Kmax"]
    assert m["records"][i, 0] == 0.5 and m["records"][i, 1] == 0 and m["records"][i, K + 1] == 0


def test_envelope_rules():
    f = np.array([100.0, 200.0, 200.0, 400.0])
    v = np.log([1.0, 2.0, 3.0, 5.0])
    q = np.array([50.0, 100.0, 150.0, 200.0, 300.0, 400.0, 900.0])
    e = M.interp_envelope(f, v, q)
    assert e[0] == v[0] and e[-1] == v[-1]                       # flat below and above the nodes
    assert e[1] == v[0] and e[5] == v[3]
    assert e[3] == v[1]                                          # a tie: the first node in (f, k) order
    assert np.isclose(e[2], 0.5 * (v[0] + v[1]))                 # between nodes: linear in ln a
    assert np.isclose(e[4], 0.5 * (v[2] + v[3]))                 # from the last of the tied nodes
    assert np.all(M.interp_envelope(np.array([300.0]), np.array([0.7]), q) == 0.7)   # one node: flat
    # the Nyquist mute, and beta == 1 leaves the amplitudes alone
    am = np.array([[1.0, 2.0, 0.0, 4.0]])
    fm = np.array([[1000.0, 5000.0, 0.0, 7000.0]])
    out = M.envelope_amplitudes(am, fm, 16000, 1.2, True)
    assert out[0, 3] == 0 and out[0, 2] == 0 and out[0, 0] > 0 and out[0, 1] > 0
    out = M.envelope_amplitudes(am, fm, 16000, 1.2, False)
    assert np.array_equal(out, [[1.0, 2.0, 0.0, 0.0]])
    assert np.array_equal(M.envelope_amplitudes(am, fm, 16000, 1.0, True), am)
    # ties sorted by slot: the node of the lower slot wins at the shared frequency
    am = np.array([[2.0, 3.0]])
    fm = np.array([[300.0, 300.0]])
    assert np.allclose(M.envelope_amplitudes(am, fm, 16000, 0.5, True), [[2.0, 2.0]])


def _arrays_model(n=8, K=2, step=15):
    ti = np.arange(n) * step
    am = np.full((n, K), 0.1)
    fm = np.tile([200.0, 400.0], (n, 1))[:, :K]
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=am, frange=fm, pk=np.zeros((n, K)))


@pytest.mark.parametrize("kw", [dict(time_scale=0.2), dict(time_scale=4.5), dict(time_scale=float("nan")),
                                dict(pitch_scale=0.0), dict(pitch_scale=float("inf")), dict(pitch_scale=-1.0),
                                dict(time_scale="x")])
def test_bad_scales_raise(kw):
    from eaqhm_amd.model import eaQHMSynthesis
    with pytest.raises(ValueError):
        eaQHMSynthesis(_arrays_model(), 16000, 200, **kw)


def test_bad_model_and_length_raise():
    from eaqhm_amd.model import eaQHMSynthesis, unpack_model
    m = _arrays_model()
    with pytest.raises(ValueError):
        eaQHMSynthesis(m, 16000, 105)                           # length < last ti + 1 = 106
    bad = dict(m, ti=np.array([0, 15, 30, 46, 60, 75, 90, 105]))
    with pytest.raises(ValueError):
        unpack_model(bad)                                        # ti not uniformly spaced
    with pytest.raises(ValueError):
        eaQHMSynthesis(bad, 16000, 200)
    with pytest.raises(ValueError):
        eaQHMSynthesis(m, 0, 200)                                # fs
    neg = dict(m, amplitudes=-m["amplitudes"])
    with pytest.raises(ValueError):
        eaQHMSynthesis(neg, 16000, 200)


def test_definition_properties_of_the_numpy_model():
    """Sanity of the NumPy model itself on a steady two-partial model: length rint(rho L), a constant partial keeps its
    frequency times beta, and rho stretches it without changing that frequency."""
    fs, D, n = 16000, 15, 200
    K = 1
    rec = np.zeros((n, 3 * K + 1))
    f = 250.0
    rec[:, 0] = 0.3
    rec[:, 1] = f
    rec[:, 2] = np.angle(np.exp(1j * 2 * np.pi * f / fs * np.arange(n) * D))
    L = (n - 1) * D + 1
    for rho, beta in ((1.0, 1.0), (1.5, 1.0), (0.7, 1.3)):
        out = M.synthesize(rec, D, fs, L, rho, beta, preserve_envelope=False)
        assert len(out) == int(np.rint(rho * L))
        seg = out[200:int(rho * L) - 200]
        spec = np.abs(np.fft.rfft(seg * np.hanning(len(seg)), 1 << 16))
        peak = np.argmax(spec) * fs / (1 << 16)
        assert abs(peak - beta * f) < 1.0
