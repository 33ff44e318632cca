"""Formant tracks without a GPU: the NumPy model of tests/formant_ref.py against what defines it
(numpy.roots, an enumeration of all state sequences, SA19), the inputs of tests/formant_cases.py against the conditions
their builder promises, and the host side of eaqhm_amd.formant: argument checks, tables, plumbing, CLI."""
import inspect
import os
import re
from math import comb

import numpy as np
import pytest

import formant_cases as FC
import formant_ref as R
from conftest import ROOT

PKG = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd")
LD = np.longdouble


@pytest.fixture(scope="module")
def formant():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import formant
    return formant


# ---- 1. the roots model
@pytest.mark.parametrize("p", FC.ORDERS)
def test_model_converges_within_48_steps(p):
    """A condition of the case builder: every frame finishes, in at most 48 of the 64 steps, in both arithmetics."""
    ref = FC.root_reference(p)
    print("p %d: steps %s (float64), %s (long double)" % (p, ref["it64"].tolist(), ref["itld"].tolist()))
    assert ref["it64"].max() <= 48 and ref["itld"].max() <= 48
    pe = [R.effective_degree(k) for k in FC.root_case(p)]
    assert {0, 1, max(p - 1, 0), p} <= set(pe)
    assert all(it == 0 for it, e in zip(ref["it64"], pe) if e == 0)


def test_near_double_pair_is_the_slow_case():
    ref = FC.root_reference(2)
    assert len(FC.root_case(2)) == len(FC.ROOT_FRAMES) + 1
    assert 30 <= ref["it64"][-1] <= 48
    assert np.allclose(np.sort(ref["z64"][-1].real), FC.NEAR_DOUBLE, rtol=0, atol=1e-10)


@pytest.mark.parametrize("p", FC.ORDERS)
def test_model_backward_error(p):
    """Every model root satisfies |P(z)| <= 16 pe u s re-evaluated in long double: the acceptance threshold 8 plus the 8
    that bounds the float64 evaluation which accepted it."""
    ref = FC.root_reference(p)
    worst = 0.0
    for k, z in zip(FC.root_case(p), ref["z64"]):
        be = R.backward_error(k, z)
        worst = max(worst, float(be.max(initial=0)))
    print("p %d: largest |P| / (pe u s) = %.3f" % (p, worst))
    assert worst <= 16.0


@pytest.mark.parametrize("p", [p for p in FC.ORDERS if p <= 18])
def test_model_agrees_with_numpy_roots(p):
    """For p <= 18 the model's roots are numpy.roots' after matching: within 1e-9 on the well-separated frames, within
    2e-6 where two roots nearly coincide (an error of sqrt(u) is what a double root allows)."""
    ref = FC.root_reference(p)
    for i, (k, z) in enumerate(zip(FC.root_case(p), ref["z64"])):
        pe = R.effective_degree(k)
        if pe == 0:
            continue
        want = np.roots(R.stepup(k)[:pe + 1])
        perm = FC.match(z[:pe], want)
        gap = np.abs(want[:, None] - want[None, :])[~np.eye(pe, dtype=bool)].min(initial=1.0)
        d = float(np.abs(z[:pe] - want[perm]).max())
        assert d <= (1e-9 if gap > 1e-2 else 2e-6), (p, i, d, gap)
        assert np.all(np.abs(z[:pe]) < 1.0)


@pytest.mark.parametrize("p", FC.ORDERS)
def test_model_zero_places(p):
    ref = FC.root_reference(p)
    for k, z, zl in zip(FC.root_case(p), ref["z64"], ref["zld"]):
        pe = R.effective_degree(k)
        a = R.stepup(k)
        assert np.all(a[pe + 1:] == 0.0) and (pe == 0 or a[pe] == k[pe - 1])
        assert np.all(z[pe:] == 0) and np.all(zl[pe:] == 0) and np.all(z[:pe] != 0)


def test_stepup_is_the_noise_models():
    import noise_model_ref as NM
    for p in (1, 2, 18, 63):
        for k in FC.root_case(p):
            assert np.array_equal(R.stepup(k), NM.stepup(k))


# ---- 2. the candidates model on the hand-built frames
def test_candidate_cases_hit_what_they_name():
    by = {c[0]: c for c in FC.candidate_cases()}
    count = {n: R.candidates(*c[1:])[2] for n, c in by.items()}
    assert count["fmin-edge"][0] == count["fmin-above-edge"][0] + 1
    assert count["fmax-edge"][0] == count["fmax-below-edge"][0] + 1
    assert count["bw-edge"][0] == count["bw-below-edge"][0] + 1
    assert count["unit-circle-bw-0"].tolist() == [2]
    assert count["nine-and-more"].tolist() == [8, 8, 8] and count["none-qualifies"].tolist() == [0, 0]
    assert count["real-roots-only"].tolist() == [0] * 5 and count["unfinished-between"].tolist() == [8, 0, 8, 0, 8]
    f, b, c, idx = R.candidates(*by["nine-and-more"][1:])
    z = by["nine-and-more"][1]
    assert (np.diff(f, axis=1) >= 0).all()
    for m in range(3):                                      # 0.95j and 0.9j have equal f: the lower root index first
        at = [int(np.flatnonzero(z[m] == v)[0]) for v in (0.95j, 0.9j)]
        tied = [i for i in idx[m] if i in at]
        assert tied == sorted(at) or len(tied) < 2
    assert any(len([i for i in idx[m] if z[m][i] in (0.95j, 0.9j)]) == 2 for m in range(3))
    f, b, c, idx = R.candidates(*by["fmin-edge"][1:])
    assert np.isnan(f[0, c[0]:]).all() and np.isnan(b[0, c[0]:]).all() and (idx[0, c[0]:] == -1).all()


# ---- 3. the tracker model
@pytest.mark.parametrize("N", (1, 2, 3, 4))
def test_state_table(formant, N):
    st = formant.formant_states(N)
    assert st.dtype == np.int8 and st.shape == (comb(8 + N, N), N)
    assert np.array_equal(st, R.states(N))
    rows = [tuple(r) for r in st.tolist()]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    assert rows[0] == (-1,) * N and rows[-1] == (7,) + (-1,) * (N - 1) and tuple(range(N)) in rows
    for r in rows:
        used = [v for v in r if v >= 0]
        assert all(-1 <= v < 8 for v in r) and used == sorted(set(used))
    assert not st.flags.writeable


@pytest.mark.parametrize("N", (1, 2))
@pytest.mark.parametrize("T", (1, 2, 3))
def test_tracker_is_the_least_of_all_sequences(N, T):
    """Counts in {0, 1, 2, 3} per frame, costs on a 2^-10 grid (every sum exact, equal totals abound): the model's path
    has the least total of ALL state sequences, and among the sequences of that total it is the one the tie rule names:
    the first minimum at the end, then at every step back the first predecessor, which is the least sequence read
    from its last frame to its first."""
    from itertools import product
    rng = np.random.default_rng(10 * N + T)
    st = R.states(N)
    S = len(st)
    ties = 0
    for count in product(range(4), repeat=T):
        count = np.array(count, np.int32)
        L, lf = FC._tables(rng, T, N, count, True, levels=2)
        wj, absent = 0.5, int(rng.integers(0, 3)) / 1024.0
        m = R.forward(L, lf, count, N, wj, absent)
        loc = R.local_costs(L, count, st, absent)
        idx = st.astype(np.int64) + 1
        total = loc[0].copy()                                                  # [s0]
        for t in range(1, T):
            J = R.jump_table(lf, count, t, wj)
            tr = np.zeros((S, S))
            for n in range(N):
                tr = tr + J[idx[:, n][:, None], idx[:, n][None, :]]
            total = (total[..., None] + tr.reshape((1,) * (t - 1) + (S, S))) + loc[t].reshape((1,) * t + (S,))
        least = total.min()
        assert np.isfinite(least) and m["total"] == least == total[tuple(m["q"])]
        assert R.path_cost(L, lf, count, N, wj, absent, m["q"]) == least
        best = np.argwhere(total == least)
        ties += len(best) > 1
        assert tuple(m["q"]) == min((tuple(b) for b in best), key=lambda q: q[::-1])
        assert np.array_equal(m["bp"][0], np.arange(S)) and m["last"][m["q"][-1]] == least
        assert all((st[m["q"][t]] < count[t]).all() for t in range(T))
    print("N %d, T %d: %d of %d inputs have more than one least sequence" % (N, T, ties, 4 ** T))
    assert T == 1 or ties >= 4 ** T // 4


@pytest.mark.parametrize("N", (1, 2, 3, 4))
def test_tracker_cases_cover_what_they_name(N):
    cases = FC.tracker_cases(N)
    assert {c[1].shape[0] for c in cases} >= {1, 2, 3, 9, 65}
    by = {c[0]: c for c in cases}
    assert by["all-empty"][3].max() == 0 and by["full"][3].min() == 8
    assert by["empty-first-and-last"][3][0] == 0 == by["empty-first-and-last"][3][-1]
    assert by["fewer-than-N"][3].max() < max(N, 1) and by["absent-cost-0"][6] == 0.0 and by["zero-weights"][5] == 0.0
    ref = FC.tracker_reference(N)
    st = R.states(N)
    for name, L, lf, count, _, wj, absent in cases:
        m = ref[name]
        assert all((st[m["q"][t]] < count[t]).all() for t in range(len(count))), name     # never the garbage
        assert m["total"] == R.path_cost(L, lf, count, N, wj, absent, m["q"]) < FC.GARBAGE, name
    assert (ref["all-empty"]["q"] == 0).all() and ref["all-empty"]["total"] == 9 * N * 2.0
    assert (ref["zero-weights"]["q"] == 0).all() and ref["zero-weights"]["total"] == 0.0


# ---- 4. SA19 through the NumPy stand-in of signal_allpole (order 18, hop 80, n_formants = 4)
@pytest.fixture(scope="module")
def sa19_tracks(formant):
    refl, fs = FC.sa19_allpole()
    z, it = R.roots(refl)
    f, b, count, _ = R.candidates(z, it, fs, 50.0, 5500.0, 1000.0)
    L, lf = formant.formant_cost_tables(dict(f=f, b=b, count=count), 4, (550, 1650, 2750, 3850))
    m = R.forward(L, lf, count, 4, 1.0, 2.0)
    F, B = formant.tracks_from_path(f, b, R.states(4), m["q"])
    return dict(refl=refl, z=z, it=it, f=f, b=b, count=count, F=F, B=B)


def _octave_steps(F):
    return [int(np.nansum(np.abs(np.diff(np.log2(F[:, n]))) > 0.25)) for n in range(F.shape[1])]


def test_sa19_conditions(sa19_tracks):
    t = sa19_tracks
    assert t["refl"].shape == (794, 18) and t["it"].max() <= 48
    worst = max(float(R.backward_error(k, z).max(initial=0)) for k, z in zip(t["refl"][::8], t["z"][::8]))
    assert worst <= 16.0
    med = np.nanmedian(t["F"], axis=0)
    absent = np.isnan(t["F"]).mean(axis=0)
    lowest = np.where(np.arange(8)[None, :] < t["count"][:, None], t["f"], np.nan)[:, :4]
    mine, naive = _octave_steps(t["F"]), _octave_steps(lowest)
    print("SA19: steps %d at most, medians %s Hz, absent %s, steps > 0.25 octave %s against %s"
          % (t["it"].max(), np.round(med).tolist(), np.round(absent, 4).tolist(), mine, naive))
    assert (np.diff(med) > 0).all()
    for m, (lo, hi) in zip(med, ((300, 1000), (1000, 2500), (2000, 3500), (3000, 4500))):
        assert lo <= m <= hi
    assert all(2 * a <= b for a, b in zip(mine, naive))
    assert absent.max() <= 0.10
    assert np.array_equal(np.isnan(t["F"]), np.isnan(t["B"]))
    Fm = np.where(np.isnan(t["F"]), np.inf, t["F"])
    for n in range(3):                                     # along the slots the present formants ascend
        later = np.min(Fm[:, n + 1:], axis=1)
        assert (t["F"][:, n][~np.isnan(t["F"][:, n])] < later[~np.isnan(t["F"][:, n])]).all()


# ---- 5. formant_warp_from_tracks
def test_warp_from_tracks(formant):
    from eaqhm_amd.args import _warp_rows
    rng = np.random.default_rng(3)
    FA = np.array([500.0, 1500.0, 2500.0])[None, :] * (1 + 0.01 * rng.standard_normal((41, 3)))
    x, y = formant.formant_warp_from_tracks(FA, FA, 16000)
    assert np.array_equal(x, y) and x.shape == (4,) and x[-1] == 8000.0
    assert np.array_equal(x[:3], np.median(FA, axis=0))
    x, y = formant.formant_warp_from_tracks(FA, FA, 16000, anchor_nyquist=False)
    assert x.shape == (3,) and np.array_equal(x, y)
    x, y = formant.formant_warp_from_tracks(FA, 1.18 * FA, 16000)            # a uniform 1.18
    assert np.allclose(y[:3] / x[:3], 1.18, rtol=1e-15) and x[-1] == y[-1] == 8000.0
    fx, fy = _warp_rows((x, y), 1, "row")                                   # what formant_warp's own check accepts
    assert np.array_equal(fx, x) and np.array_equal(fy[0], y)
    FB = FA.copy()
    FB[:, 1] = FA[:, 1] * 3.5                                               # slot 1 rises at a slope beyond 4
    with pytest.raises(ValueError, match=r"slot 1 \(F2\).*slope"):
        formant.formant_warp_from_tracks(FA, FB, 16000)
    FB = FA.copy()
    FB[:, 0] = 5.0 * FA[:, 0]                                               # the slope from the origin
    with pytest.raises(ValueError, match=r"slot 0 \(F1\).*slope"):
        formant.formant_warp_from_tracks(FA, FB, 16000)
    FB = FA.copy()
    FB[:, 2] = FA[:, 1] * 0.99
    with pytest.raises(ValueError, match=r"slot 2 \(F3\).*does not lie above"):
        formant.formant_warp_from_tracks(FA, FB, 16000)
    gaps = FA.copy()
    gaps[::2, 0] = np.nan                                                    # present in half the frames
    gaps[:, 1] = np.nan                                                      # a NaN column: the slot gives no breakpoint
    x, y = formant.formant_warp_from_tracks(gaps, FA, 16000)
    assert x.shape == (3,) and x[0] == np.median(FA[1::2, 0]) and y[0] == np.median(FA[:, 0]) and x[1] == np.median(FA[:, 2])
    with pytest.raises(ValueError, match="no slot"):
        formant.formant_warp_from_tracks(np.full((5, 2), np.nan), np.full((5, 2), np.nan), 16000)
    hi = np.array([[3000.0, 7900.0]])                                        # the Nyquist anchor is not admissible
    x, y = formant.formant_warp_from_tracks(hi, hi * np.array([1.0, 0.9]), 16000)
    assert x.shape == (2,)
    for bad in (FA[:, :2], np.zeros((0, 3)), -FA, FA[0], np.full((4, 3), np.inf), np.zeros((4, 5))):
        with pytest.raises(ValueError):
            formant.formant_warp_from_tracks(FA, bad, 16000)
    with pytest.raises(ValueError):
        formant.formant_warp_from_tracks(FA, FA, 0)


# ---- 6. argument checks: ValueError before any device work
def _model(Nf=5, p=4, hop=80):
    rng = np.random.default_rng(0)
    return dict(sigma=np.ones(Nf), refl=rng.uniform(-0.5, 0.5, (Nf, p)), hop=hop, order=p, fs=16000,
                length=(Nf - 1) * hop + 1)


def _cand(T=4):
    f = np.tile(np.array([500.0, 1500, 2500, 3500, np.nan, np.nan, np.nan, np.nan]), (T, 1))
    return dict(f=f, b=np.where(np.isnan(f), np.nan, 100.0), count=np.full(T, 4, np.int32))


@pytest.fixture()
def no_device(monkeypatch):
    from eaqhm_amd import records

    def refuse(*a, **k):
        pytest.fail("device work before the argument checks")
    monkeypatch.setattr(records, "_device", refuse)


def test_model_checks(formant, no_device):
    m = _model()
    for change in (dict(refl=np.ones((5, 4))), dict(refl=m["refl"][:, :3]), dict(order=64), dict(hop=0), dict(fs=-1),
                   dict(length=1000), dict(sigma=-m["sigma"]), dict(refl=np.full((5, 4), np.nan))):
        bad = dict(m, **change)
        for fn in (formant.allpole_roots, formant.formant_candidates, formant.check_allpole_model):
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (formant.allpole_roots, formant.formant_candidates):
        with pytest.raises(ValueError):
            fn([1, 2, 3])
        for dev in (-1, 1.5, True, "0"):
            with pytest.raises(ValueError, match="device_index"):
                fn(m, device_index=dev)
    for kw in (dict(fmin=-1), dict(fmin=float("nan")), dict(fmax=float("inf")), dict(fmin=9000.0), dict(fmin=600, fmax=500),
               dict(max_bandwidth=0), dict(max_bandwidth=-5), dict(fmax="x")):
        with pytest.raises(ValueError):
            formant.formant_candidates(m, **kw)
    nz, fmin, fmax, bw = formant.check_candidate_arguments(m, 50, 20000.0, 700)
    assert (fmin, fmax, bw) == (50.0, 8000.0, 700.0) and nz["refl"].flags.c_contiguous


def test_track_checks(formant, no_device):
    c = _cand()
    for change in (dict(f=c["f"][:, :7]), dict(b=c["b"][:3]), dict(count=c["count"][:3]), dict(count=np.full(4, 9)),
                   dict(count=np.full(4, -1)), dict(count=np.full(4, 4.0)), dict(f=-c["f"]), dict(count=np.full(4, 5)),
                   dict(f=np.zeros((0, 8)), b=np.zeros((0, 8)), count=np.zeros(0, np.int32))):
        with pytest.raises(ValueError):
            formant.formant_tracks(dict(c, **change))
    with pytest.raises(ValueError):
        formant.formant_tracks(dict(f=c["f"], b=c["b"]))
    for kw in (dict(n_formants=0), dict(n_formants=5), dict(n_formants=2.5), dict(n_formants=True),
               dict(reference=(550, 500, 2750)), dict(reference=(550, 1650)), dict(reference=(0, 1650, 2750)),
               dict(reference=(550, 1650, float("nan"))), dict(freq_cost=-1), dict(bandwidth_cost=float("inf")),
               dict(jump_cost=float("nan")), dict(absent_cost=-0.5), dict(absent_cost="x"), dict(device_index=-1)):
        with pytest.raises(ValueError):
            formant.formant_tracks(c, **kw)
    f, b, count, N, ref, wf, wb, wj, ac = formant.check_track_arguments(c, 2, (500, 1500, 2400))
    assert N == 2 and ref.tolist() == [500.0, 1500.0] and (wf, wb, wj, ac) == (1.0, 1.0, 1.0, 2.0)   # the first N count


def test_cost_tables(formant):
    c = _cand(3)
    c["count"] = np.array([4, 2, 0], np.int32)
    L, lf = formant.formant_cost_tables(c, 3, (550, 1650, 2750), 2.0, 0.5)
    assert L.shape == (3, 3, 8) and lf.shape == (3, 8) and L.flags.c_contiguous
    assert L[0, 1, 2] == 2.0 * abs(2500.0 - 1650.0) / 1000.0 + 0.5 * 100.0 / 2500.0
    assert np.array_equal(lf[0, :4], np.log2(c["f"][0, :4]))
    assert (L[1, :, 2:] == 0).all() and (L[2] == 0).all() and (lf[1, 2:] == 0).all() and np.isfinite(L).all()
    F, B = formant.tracks_from_path(c["f"], c["b"], formant.formant_states(2), np.array([0, 11, 1]))
    st = formant.formant_states(2)
    assert np.isnan(F[0]).all() and st[11].tolist() == [0, 2] and F[1].tolist() == [500.0, 2500.0]
    assert np.isnan(F[2, 0]) and F[2, 1] == 500.0 and B[1].tolist() == [100.0, 100.0]


def test_signal_allpole_checks(formant, no_device):
    s = np.sin(np.arange(2000) * 0.1)
    for kw in (dict(preemphasis=1.0), dict(preemphasis=-0.1), dict(preemphasis=float("nan")), dict(order=64), dict(hop=0),
               dict(order=400, hop=80)):
        with pytest.raises(ValueError):
            formant.signal_allpole(s, 16000, **kw)
    for bad in (np.zeros((3, 3)), [], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            formant.signal_allpole(bad, 16000)
    with pytest.raises(ValueError):
        formant.signal_allpole(s, 0)
    x, fs, hop, order = formant.check_signal_allpole_arguments(s, 16000)
    assert (fs, hop, order) == (16000.0, 80, 18) and x[0] == s[0] and np.array_equal(x[1:], s[1:] - 0.97 * s[:-1])


def test_signal_and_model_allpole_call_the_existing_kernels(formant, monkeypatch):
    from eaqhm_amd import cepstrum, noise, records
    seen = []
    monkeypatch.setattr(noise, "eaQHMNoiseAnalysis",
                        lambda s, r, fs, order, hop, device_index=0: seen.append((len(s), float(np.abs(r).max()), fs, order, hop)))
    formant.signal_allpole(np.ones(500), 16000, 12, 40)
    assert seen == [(500, 0.0, 16000.0, 12, 40)]
    monkeypatch.setattr(records, "unpack_model", lambda det: dict(step=15))
    monkeypatch.setattr(cepstrum, "model_cepstrum", lambda det, fs, device_index=0: ("ceps of", det))
    monkeypatch.setattr(noise, "noise_from_cepstrum",
                        lambda ceps, hop, fs, order=None, device_index=0: (ceps, hop, fs, order))
    assert formant.model_allpole("det", 16000) == (("ceps of", "det"), 15, 16000, None)
    assert formant.model_allpole("det", 16000, 20, 30) == (("ceps of", "det"), 30, 16000, 20)


# ---- 7. plumbing
def test_symbols_header_and_makefile():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import formant, hip
    counts = dict(eaqhm_allpole_roots=6, eaqhm_formant_candidates=12, eaqhm_formant_forward=11, eaqhm_formant_backtrack=7)
    assert hip.ABI_VERSION == 6
    bound = {name: len(args) for name, _, args in hip.SYMBOLS_FORMANT}
    others = (hip.SYMBOLS + hip.SYMBOLS_MLPG + hip.SYMBOLS_GV + hip.SYMBOLS_CEPWARP + hip.SYMBOLS_KMEANS
              + hip.SYMBOLS_MLPG_EM + hip.SYMBOLS_NN + hip.SYMBOLS_SWIPE + hip.SYMBOLS_VITERBI)
    assert not set(bound) & {name for name, _, _ in others}
    header = open(os.path.join(ROOT, "include", "eaqhm_formant.h")).read()
    assert '#include "eaqhm_formant.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(bound) == set(counts)
    for name, n in counts.items():
        assert bound[name] == n, name
        decl = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, header, re.M)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
        before = header[:decl.start()]                      # every declaration cites its DESIGN section
        assert re.search(r"DESIGN\.md §14\.\d", before[before.rfind("/*"):]), name
    for name in ("allpole_roots", "formant_candidates", "formant_forward", "formant_backtrack"):
        assert callable(getattr(hip.Context, name))
    for const, macro in (("FORMANT_ITMAX", "EAQHM_FORMANT_ITMAX"), ("FORMANT_CANDIDATES", "EAQHM_FORMANT_CAND"),
                         ("FORMANT_TRACKS_MAX", "EAQHM_FORMANT_TRACKS")):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == getattr(formant, const)
    assert int(re.search(r"#define\s+EAQHM_FORMANT_STATES\s+(\d+)", header).group(1)) == comb(12, 4)
    assert R.ITMAX == formant.FORMANT_ITMAX and R.KC == formant.FORMANT_CANDIDATES
    lib = hip.load_library()                                                 # a null context: EAQHM_EINVAL
    assert lib.eaqhm_allpole_roots(None, None, 1, 1, None, None) == -1
    assert lib.eaqhm_formant_candidates(None, None, None, 1, 1, 16000.0, 50.0, 5500.0, 1000.0, None, None, None) == -1
    assert lib.eaqhm_formant_forward(None, None, None, None, None, 1, 1, 1.0, 2.0, None, None) == -1
    assert lib.eaqhm_formant_backtrack(None, None, None, 1, 1, None, None) == -1
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\beaqhm_formant\.hip\b", makefile, re.M)
    assert re.search(r"^HDR\s*:=.*include/eaqhm_formant\.h\b", makefile, re.M)
    source = open(os.path.join(PKG, "csrc", "eaqhm_formant.hip")).read()
    assert "#pragma clang fp contract(off)" in source and "atomic" not in source.replace("No atomics", "")


def test_not_reexported_and_surface_unchanged():
    import json
    import eaqhm_amd
    from eaqhm_amd import formant
    for name in ("allpole_roots", "formant_candidates", "formant_tracks", "formant_states", "signal_allpole",
                 "model_allpole", "formant_warp_from_tracks"):
        assert callable(getattr(formant, name)) and not hasattr(eaqhm_amd, name)
    assert "§14" in formant.__doc__
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "python_api.json")))["eaqhm_amd"]
    assert {n for n in vars(eaqhm_amd) if not n.startswith("_") and not inspect.ismodule(getattr(eaqhm_amd, n))
            and getattr(getattr(eaqhm_amd, n), "__module__", "eaqhm_amd").startswith("eaqhm_amd")} <= set(recorded)
    assert str(inspect.signature(formant.allpole_roots)) == "(model, *, device_index=0)"
    assert str(inspect.signature(formant.formant_candidates)) == \
        "(model, *, fmin=50.0, fmax=5500.0, max_bandwidth=1000.0, device_index=0)"
    assert str(inspect.signature(formant.formant_tracks)) == \
        ("(cand, n_formants=3, reference=(550, 1650, 2750, 3850), *, freq_cost=1.0, bandwidth_cost=1.0, jump_cost=1.0, "
         "absent_cost=2.0, device_index=0, return_path=False)")
    assert str(inspect.signature(formant.formant_warp_from_tracks)) == "(FA, FB, fs, *, anchor_nyquist=True)"


def test_cli_flags(monkeypatch, tmp_path, capsys):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav"])
    assert a.formants_out is None and a.formant_count is None and a.formant_warp_from is None
    a = cli.parser().parse_args(["x.wav", "--formants-out", "f.txt", "--formant-count", "4"])
    assert (a.formants_out, a.formant_count) == ("f.txt", 4)
    for flag in ("--formants-out", "--formant-count", "--formant-warp-from"):
        assert flag in cli.__doc__
    for other in (["--formant-scale", "1.1"], ["--formant-vtln", "1.1"], ["--formant-warp-curve", "c.txt"],
                  ["--formant-scale-curve", "c.txt"]):
        with pytest.raises(SystemExit):
            cli.parser().parse_args(["x.wav", "--formant-warp-from", "o.wav"] + other)
    for argv in (["x.wav", "--formant-count", "3"], ["x.wav", "--formants-out", "f", "--formant-count", "5"],
                 ["x.wav", "--formant-warp-from", "o.wav", "--formant-count", "0"],
                 ["x.wav", "--formant-warp-from", "o.wav", "--no-envelope"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    capsys.readouterr()
    # stand-ins: the analysis, the formant measurement and the synthesis
    from scipy.io import wavfile
    wav = str(tmp_path / "a.wav")
    wavfile.write(wav, 16000, np.zeros(1600, np.int16))
    calls = []
    monkeypatch.setattr(cli, "analyse", lambda path, gender, opts: (np.zeros(1600), [0.0], "det", None))
    sec = np.arange(3) * 0.005
    F = np.array([[500.0, 1500.0], [510.0, np.nan], [490.0, 1490.0]])
    table = lambda path, fc, n: calls.append((os.path.basename(path), fc, n)) or \
        (16000, sec, F * (1.1 if path.endswith("o.wav") else 1.0), F / 10)   # noqa: E731
    monkeypatch.setattr(cli, "formant_table", table)
    out = str(tmp_path / "formants.txt")
    assert cli.main([wav, "--formants-out", out, "--formant-count", "2"]) == 0
    assert calls == [("a.wav", 0, 2)]
    rows = np.loadtxt(out)
    assert rows.shape == (3, 5) and np.array_equal(rows[:, 0], sec) and np.isnan(rows[1, 2]) and rows[2, 4] == 149.0
    assert open(out).readline().split() == ["#", "seconds", "F1", "F2", "B1", "B2"]
    from eaqhm_amd import model
    synth = []
    monkeypatch.setattr(model, "eaQHMSynthesis", lambda det, fs, L, **kw: synth.append(kw) or np.zeros(L))
    del calls[:]
    assert cli.main([wav, "--formant-warp-from", str(tmp_path / "o.wav")]) == 0
    assert calls == [("a.wav", 0, 3), ("o.wav", 0, 3)]
    x, y = synth[0]["formant_warp"]
    assert np.allclose(y[:2] / x[:2], 1.1) and x[-1] == y[-1] == 8000.0 and synth[0]["formant_scale"] == 1.0
    assert os.path.exists(wav[:-4] + "_modified.wav")
    del synth[:], calls[:]
    assert cli.main([wav, "--pitch-scale", "1.2"]) == 0                      # without the flags: the call as it was
    assert calls == [] and synth[0]["formant_warp"] is None
