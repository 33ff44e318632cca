"""Formant tracks on the MI355X (eaqhm_amd.formant -> eaqhm_allpole_roots, eaqhm_formant_candidates,
eaqhm_formant_forward / _backtrack) against tests/formant_ref.py, the NumPy model that tests/test_formant_cpu.py ties to
numpy.roots, to an enumeration of all state sequences and to SA19.

Roots.  Every device root satisfies |P(z)| <= 16 pe u s re-evaluated in long double (8, the acceptance threshold, plus
the 8 that bounds the float64 evaluation which accepted it), every frame finishes within 48 steps, the zero places are
exact, and after matching every root lies within 100 x the model's own float64-to-long-double distance for the same
frame of the long-double model's root, at least 64 u |z|.  Candidates: the model is fed the device's roots; counts and
order are equal, f and b are held to the same yardstick.  Tracker: the recurrence's tables come from the host and every
tie is decided by rule, so q, bp, the last column and the total are EQUAL to the model's: integers equal, doubles as
bits."""
import os

import numpy as np
import pytest

import formant_cases as FC
import formant_ref as R
from conftest import GOLDEN, record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
SENTINEL = -12345


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def ctx():
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    return torch, c, c.device


def up(a):
    torch, _, d = ctx()
    return torch.as_tensor(np.ascontiguousarray(a), device=d)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. roots
def gpu_roots(refl):
    """-> (z complex128[Nf, p], iters int32[Nf]) with nothing written behind either array."""
    torch, c, d = ctx()
    Nf, p = refl.shape
    roots = torch.full((Nf + 2, p, 2), float(SENTINEL), dtype=torch.float64, device=d)
    iters = torch.full((Nf + 4,), SENTINEL, dtype=torch.int32, device=d)
    c.allpole_roots(up(refl), Nf, p, roots[:Nf], iters[:Nf])
    r, it = roots.cpu().numpy(), iters.cpu().numpy()
    assert (r[Nf:] == SENTINEL).all() and (it[Nf:] == SENTINEL).all()
    return r[:Nf, :, 0] + 1j * r[:Nf, :, 1], it[:Nf]


def frame_bars(p):
    """Per distinct frame of root_case(p): (the long-double model's roots in the float64 model's order, the frame's
    float64-to-long-double distance)."""
    ref = FC.root_reference(p)
    out = []
    for k, z64, zld in zip(FC.root_case(p), ref["z64"], ref["zld"]):
        pe = R.effective_degree(k)
        perm = FC.match(z64[:pe], zld[:pe]) if pe else np.zeros(0, np.int64)
        zl = zld[:pe][perm]
        out.append((zl, float(np.abs(z64[:pe] - zl).max(initial=0))))
    return out


@pytest.mark.parametrize("p", FC.ORDERS)
def test_roots(amd, p):
    base, ref, bars = FC.root_case(p), FC.root_reference(p), frame_bars(p)
    first = {}
    worst_be, worst_ratio, most = 0.0, 0.0, 0
    for Nf in FC.BATCHES:                                   # below, at and above the four waves of a block
        refl, index = FC.tiled(p, Nf)
        z, it = gpu_roots(refl)
        z2, it2 = gpu_roots(refl)
        assert np.array_equal(bits(z.real), bits(z2.real)) and np.array_equal(bits(z.imag), bits(z2.imag))
        assert np.array_equal(it, it2)
        for i, d in enumerate(index):
            k, pe = base[d], R.effective_degree(base[d])
            assert it[i] <= 48 and (pe > 0 or it[i] == 0), (p, Nf, i, it[i])
            assert (z[i, pe:] == 0).all() and not np.signbit(z[i, pe:].real).any(), (p, Nf, i)     # the zero places
            be = R.backward_error(k, z[i])
            assert (be <= 16.0).all(), (p, Nf, i, float(be.max()))
            zl, dist = bars[d]
            if pe:
                perm = FC.match(z[i, :pe], zl)
                err = np.abs(z[i, :pe].astype(np.clongdouble) - zl[perm]).astype(np.float64)
                bar = np.maximum(100.0 * dist, 64.0 * U * np.abs(z[i, :pe]))
                assert (err <= bar).all(), (p, Nf, i, float((err / bar).max()))
                worst_ratio = max(worst_ratio, float((err / np.maximum(dist, 0.64 * U * np.abs(z[i, :pe]))).max()))
                worst_be = max(worst_be, float(be.max()))
            most = max(most, int(it[i]))
            # a frame's bits depend neither on its neighbours nor on its place in the block
            mine = (bits(z[i].real).tobytes(), bits(z[i].imag).tobytes(), int(it[i]))
            assert first.setdefault(int(d), mine) == mine, (p, Nf, i)
    assert set(first) == set(range(len(base)))
    print("p %d: largest |P| / (pe u s) %.3f, largest distance / model distance %.3f, %d steps at most (model %d)"
          % (p, worst_be, worst_ratio, most, ref["it64"].max()))
    record_measurement("formant_roots_p%d" % p, backward=worst_be, ratio=worst_ratio, steps=most)


def test_roots_silent_frame_between_live_ones(amd):
    refl, index = FC.tiled(18, 5)
    assert FC.ROOT_FRAMES[1] == "silent" and (refl[1] == 0).all() and refl[0].any() and refl[2].any()
    z, it = gpu_roots(refl)
    assert it[1] == 0 and (z[1] == 0).all() and it[0] > 0 and it[2] > 0


# ---- 2. candidates
def gpu_candidates(z, iters, fs, fmin, fmax, bmax):
    torch, c, d = ctx()
    Nf, p = z.shape
    f = torch.full((Nf + 1, R.KC), float(SENTINEL), dtype=torch.float64, device=d)
    b = torch.full((Nf + 1, R.KC), float(SENTINEL), dtype=torch.float64, device=d)
    count = torch.full((Nf + 4,), SENTINEL, dtype=torch.int32, device=d)
    zz = np.stack((z.real, z.imag), axis=-1)
    c.formant_candidates(up(zz), up(np.asarray(iters, np.int32)), Nf, p, fs, fmin, fmax, bmax, f[:Nf], b[:Nf], count[:Nf])
    f_h, b_h, c_h = f.cpu().numpy(), b.cpu().numpy(), count.cpu().numpy()
    assert (f_h[Nf:] == SENTINEL).all() and (b_h[Nf:] == SENTINEL).all() and (c_h[Nf:] == SENTINEL).all()
    return f_h[:Nf], b_h[:Nf], c_h[:Nf]


def check_candidates(name, z, iters, fs, fmin, fmax, bmax):
    """Counts and order equal to the model's on the same roots; f and b within 100 x the model's own
    float64-to-long-double distance, at least 64 u of the value; NaN beyond the count.  Returns the largest ratio."""
    f, b, count = gpu_candidates(z, iters, fs, fmin, fmax, bmax)
    mf, mb, mcount, idx = R.candidates(z, iters, fs, fmin, fmax, bmax)
    assert np.array_equal(count, mcount), (name, count.tolist(), mcount.tolist())
    lf, lb, _, _ = R.candidate_values(z, fs, LD)
    worst = 0.0
    for m in range(len(count)):
        n = int(count[m])
        assert np.isnan(f[m, n:]).all() and np.isnan(b[m, n:]).all(), (name, m)
        for got, mine, ld in ((f[m, :n], mf[m, :n], lf[m][idx[m, :n]]), (b[m, :n], mb[m, :n], lb[m][idx[m, :n]])):
            dist = np.abs(mine - ld).astype(np.float64)
            err = np.abs(got - ld).astype(np.float64)
            bar = np.maximum(100.0 * dist, 64.0 * U * np.abs(ld).astype(np.float64))
            assert (err <= bar).all(), (name, m, got.tolist(), mine.tolist())
            worst = max(worst, float((err / np.maximum(np.maximum(dist, 0.64 * U * np.abs(ld).astype(np.float64)),
                                                       1e-300)).max(initial=0)))
    return worst, count


def test_candidates_hand_built(amd):
    seen = {}
    for name, z, iters, fs, fmin, fmax, bmax in FC.candidate_cases():
        worst, count = check_candidates(name, z, iters, fs, fmin, fmax, bmax)
        seen[name] = count.tolist()
        record_measurement("formant_candidates_%s" % name, ratio=worst)
    assert seen["fmin-edge"][0] == seen["fmin-above-edge"][0] + 1 and seen["fmax-edge"][0] == seen["fmax-below-edge"][0] + 1
    assert seen["bw-edge"][0] == seen["bw-below-edge"][0] + 1
    assert seen["nine-and-more"] == [8, 8, 8] and seen["none-qualifies"] == [0, 0] and seen["real-roots-only"] == [0] * 5
    assert seen["unfinished-between"] == [8, 0, 8, 0, 8]


@pytest.mark.parametrize("p", (3, 18, 31, 63))
def test_candidates_on_the_devices_roots(amd, p):
    refl, _ = FC.tiled(p, 65)
    z, it = gpu_roots(refl)
    worst, count = check_candidates("p%d" % p, z, it, 16000.0, 50.0, 5500.0, 1000.0)
    print("p %d: counts %s, largest distance / model distance %.3f" % (p, np.bincount(count, minlength=9).tolist(), worst))
    record_measurement("formant_candidates_p%d" % p, ratio=worst)
    assert p < 18 or count.max() >= 1


# ---- 3. the tracker
def gpu_decode(L, lf, count, N, wj, absent):
    """-> (bp, last, q, total) with nothing written behind any of them."""
    torch, c, d = ctx()
    st = R.states(N)
    T, S = len(count), len(st)
    bp = torch.full((T + 1, S), SENTINEL, dtype=torch.int16, device=d)
    last = torch.full((S + 4,), np.nan, dtype=torch.float64, device=d)
    q = torch.full((T + 4,), SENTINEL, dtype=torch.int32, device=d)
    total = torch.full((3,), np.nan, dtype=torch.float64, device=d)
    c.formant_forward(up(L), up(lf), up(count), up(st), N, T, wj, absent, bp[:T], last[:S])
    c.formant_backtrack(bp[:T], last[:S], N, T, q[:T], total[:1])
    bp_h, last_h, q_h, tot_h = bp.cpu().numpy(), last.cpu().numpy(), q.cpu().numpy(), total.cpu().numpy()
    assert (bp_h[T:] == SENTINEL).all() and np.isnan(last_h[S:]).all() and (q_h[T:] == SENTINEL).all()
    assert np.isnan(tot_h[1:]).all()
    return bp_h[:T], last_h[:S], q_h[:T], tot_h[0]


@pytest.mark.parametrize("N", (1, 2, 3, 4))
def test_tracker(amd, N):
    cases, ref = FC.tracker_cases(N), FC.tracker_reference(N)
    assert {c[1].shape[0] for c in cases} >= {1, 2, 3, 9, 65}
    for name, L, lf, count, _, wj, absent in cases:
        m = ref[name]
        bp, last, q, total = gpu_decode(L, lf, count, N, wj, absent)
        assert np.array_equal(q, m["q"]), name
        assert np.array_equal(bp, m["bp"]), name
        assert np.array_equal(bits(last), bits(m["last"])), name
        assert bits(total) == bits(m["total"]), name
        again = gpu_decode(L, lf, count, N, wj, absent)
        assert np.array_equal(bp, again[0]) and np.array_equal(bits(last), bits(again[1])), name
        assert np.array_equal(q, again[2]) and bits(total) == bits(again[3]), name
    record_measurement("formant_tracker_N%d" % N, cases=len(cases))


# ---- 4. end to end
@pytest.fixture(scope="module")
def sa19(amd):
    from scipy.io import wavfile
    from eaqhm_amd import formant
    fs, x = wavfile.read(os.path.join(GOLDEN, "SA19.WAV"))
    model = formant.signal_allpole(x / 32768.0, fs, 18, 80)
    cand = formant.formant_candidates(model)
    return fs, model, cand


def test_sa19_path_is_the_models(amd, sa19):
    from eaqhm_amd import formant
    fs, model, cand = sa19
    assert model["refl"].shape == (794, 18) and cand["unfinished"] == 0
    z, it = formant.allpole_roots(model)
    assert z.shape == (794, 18) and z.dtype == np.complex128 and it.dtype == np.int32 and it.max() <= 48
    assert max(float(R.backward_error(k, r).max(initial=0)) for k, r in zip(model["refl"][::16], z[::16])) <= 16.0
    mf, mb, mcount, _ = R.candidates(z, it, fs, 50.0, 5500.0, 1000.0)
    assert np.array_equal(cand["count"], mcount)
    F, B, q, total = formant.formant_tracks(cand, 3, return_path=True)
    L, lf = formant.formant_cost_tables(cand, 3, (550, 1650, 2750, 3850))
    m = R.forward(L, lf, cand["count"], 3, 1.0, 2.0)
    assert np.array_equal(q, m["q"]) and bits(total) == bits(m["total"])
    wantF, wantB = formant.tracks_from_path(cand["f"], cand["b"], R.states(3), m["q"])
    assert np.array_equal(F, wantF, equal_nan=True) and np.array_equal(B, wantB, equal_nan=True)
    med = np.nanmedian(F, axis=0)
    print("SA19 on the device: medians %s Hz, absent %s" % (np.round(med).tolist(), np.isnan(F).mean(axis=0).round(4).tolist()))
    assert (np.diff(med) > 0).all() and 300 <= med[0] <= 1000 and 1000 <= med[1] <= 2500 and 2000 <= med[2] <= 3500
    F2, B2 = formant.formant_tracks(cand, 3)
    assert np.array_equal(F, F2, equal_nan=True) and np.array_equal(B, B2, equal_nan=True)


def test_warp_from_tracks_feeds_the_synthesis(amd, sa19):
    from eaqhm_amd import formant
    from test_gpu_model_synthesis import reference_model
    fs, model, cand = sa19
    FA, _ = formant.formant_tracks(cand, 3)
    warp = formant.formant_warp_from_tracks(FA, 1.12 * FA, fs)
    g, det = reference_model()
    L = len(g["s_recon"])
    out = amd.eaQHMSynthesis(det, fs, L, formant_warp=warp)
    same = amd.eaQHMSynthesis(det, fs, L)
    assert out.shape == (L,) and np.isfinite(out).all() and not np.array_equal(out, same)
    other = formant.model_allpole(det, fs)                  # the all-pole fit of the model's own envelope
    assert other["refl"].shape[0] == len(g["det_ti"]) and (np.abs(other["refl"]) < 1).all()
    FB, _ = formant.formant_tracks(formant.formant_candidates(other), 3)
    assert FB.shape == (len(g["det_ti"]), 3) and np.isfinite(np.nanmedian(FB, axis=0)).all()


# ---- 5. refusals: EAQHM_EINVAL, nothing launched, the outputs untouched
def test_refusals(amd):
    torch, c, d = ctx()
    lib, h = c.lib, c.h
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    refl = up(FC.root_case(3))
    Nf = refl.shape[0]
    roots = torch.full((Nf, 3, 2), float(SENTINEL), dtype=torch.float64, device=d)
    iters = torch.full((Nf,), SENTINEL, dtype=torch.int32, device=d)
    for args in ((None, Nf, 3, roots, iters), (refl, Nf, 3, None, iters), (refl, Nf, 3, roots, None),
                 (refl, 0, 3, roots, iters), (refl, -1, 3, roots, iters), (refl, Nf, 0, roots, iters),
                 (refl, Nf, 64, roots, iters), (refl, 2 ** 31, 3, roots, iters)):
        r, n, p, o1, o2 = args
        assert lib.eaqhm_allpole_roots(h, P(r), n, p, P(o1), P(o2)) == -1, args[1:3]
    f = torch.full((Nf, 8), float(SENTINEL), dtype=torch.float64, device=d)
    b = torch.full((Nf, 8), float(SENTINEL), dtype=torch.float64, device=d)
    cnt = torch.full((Nf,), SENTINEL, dtype=torch.int32, device=d)
    z = torch.zeros((Nf, 3, 2), dtype=torch.float64, device=d)
    it = torch.zeros((Nf,), dtype=torch.int32, device=d)
    ok = dict(z=z, it=it, n=Nf, p=3, fs=16000.0, lo=50.0, hi=5500.0, bw=1000.0, f=f, b=b, c=cnt)
    for change in (dict(z=None), dict(it=None), dict(f=None), dict(b=None), dict(c=None), dict(n=0), dict(p=0), dict(p=64),
                   dict(fs=0.0), dict(fs=float("nan")), dict(lo=float("nan")), dict(hi=float("inf")), dict(bw=float("nan"))):
        a = dict(ok, **change)
        assert lib.eaqhm_formant_candidates(h, P(a["z"]), P(a["it"]), a["n"], a["p"], a["fs"], a["lo"], a["hi"], a["bw"],
                                            P(a["f"]), P(a["b"]), P(a["c"])) == -1, change
    N, T = 2, 3
    st = up(R.states(N))
    S = st.shape[0]
    L, lf, count = up(np.zeros((T, N, 8))), up(np.zeros((T, 8))), up(np.zeros(T, np.int32))
    bp = torch.full((T, S), SENTINEL, dtype=torch.int16, device=d)
    last = torch.full((S,), float(SENTINEL), dtype=torch.float64, device=d)
    q = torch.full((T,), SENTINEL, dtype=torch.int32, device=d)
    total = torch.full((1,), float(SENTINEL), dtype=torch.float64, device=d)
    ok = dict(L=L, lf=lf, c=count, st=st, N=N, T=T, wj=1.0, ac=2.0, bp=bp, last=last)
    for change in (dict(L=None), dict(lf=None), dict(c=None), dict(st=None), dict(bp=None), dict(last=None), dict(N=0),
                   dict(N=5), dict(T=0), dict(T=2 ** 31), dict(wj=-1.0), dict(wj=float("nan")), dict(wj=float("inf")),
                   dict(ac=-1.0), dict(ac=float("nan")), dict(ac=float("inf"))):
        a = dict(ok, **change)
        assert lib.eaqhm_formant_forward(h, P(a["L"]), P(a["lf"]), P(a["c"]), P(a["st"]), a["N"], a["T"], a["wj"], a["ac"],
                                         P(a["bp"]), P(a["last"])) == -1, change
    ok = dict(bp=bp, last=last, N=N, T=T, q=q, total=total)
    for change in (dict(bp=None), dict(last=None), dict(q=None), dict(total=None), dict(N=0), dict(N=5), dict(T=0)):
        a = dict(ok, **change)
        assert lib.eaqhm_formant_backtrack(h, P(a["bp"]), P(a["last"]), a["N"], a["T"], P(a["q"]), P(a["total"])) == -1, change
    c.sync()
    for t in (roots, iters, f, b, cnt, bp, last, q, total):
        assert (t.cpu().numpy() == SENTINEL).all()
    assert b"eaqhm_formant_backtrack" in lib.eaqhm_last_error(h)
    z_ok, it_ok = gpu_roots(FC.root_case(3))                 # the context still works
    assert it_ok.max() <= 48
