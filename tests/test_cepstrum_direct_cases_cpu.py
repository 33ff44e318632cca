"""The cases of tests/cepstrum_direct_cases.py are fit to judge the cepstrum kernels (csrc/eaqhm_cepstrum.hip), shown with
the NumPy models alone: the tables hold every K, P, n, F, B and pattern; every case has a non-zero yardstick (the
deviation between the model in float64 and in np.longdouble, from which tests/test_gpu_cepstrum_direct.py takes its
bars); every fit instant factors by float64 Cholesky and has a finite longdouble solution, so the GPU test excludes
nothing; the kernel's own route to the fit (nodes packed 64 slots at a time, the Gramian from the cosine sums T_d),
restated here in float64, stays within the bar of every launch; and each of twelve deliberate errors, written here as
variants of the models, moves at least one case by more than 100 x that case's yardstick, or breaks an exact claim (an
error of inf).

"c_0 added before the recurrence" is not among the errors: in IEEE arithmetic -inf plus a finite sum is -inf in either
order, and a finite row moves by one rounding, so no case can notice it and none should.

What the yardsticks came to here (float64 vs longdouble; linear axis, a = 0.42, a = -0.9): fit, per launch, 6.9e-16 ..
1.9e-9, 8.6e-16 .. 1.6e-9, 1.9e-15 .. 1.3e-7 (per instant from 1.2e-18, which is why an instant is no case); envelope
2.2e-16 .. 2.9e-15, 2.9e-16 .. 2.8e-15, 3.6e-16 .. 8.9e-14; phase 1.2e-16 .. 4.8e-15, 1.2e-16 .. 2.4e-15, 4.6e-17 ..
7.1e-14; amplitudes (relative) 1.8e-18 .. 2.6e-15, 1.3e-16 .. 2.4e-15, 1.1e-16 .. 1.9e-14; build am (relative) 1.2e-17 ..
3.4e-14, 2.3e-17 .. 3.7e-15, 2.2e-17 .. 3.9e-14; build phase 6.1e-18 .. 9.0e-14, 3.8e-18 .. 8.9e-14, 6.1e-18 .. 1.0e-13.
The fit by the kernel's route comes to at most 0.114 of a bar (K 129, P 63, lam 1e-6, a = 0.42)."""
import numpy as np
import pytest

import cepstrum_direct_cases as C
import cepstrum_warp_ref as CW
import model_build_ref as MB
import model_cepstrum_ref as CR


@pytest.fixture(scope="module", autouse=True)
def _quiet():
    with np.errstate(all="ignore"):
        yield


# ---- the tables
def test_case_tables_hold_every_size_order_and_pattern():
    assert C.FIT_K == [1, 2, 63, 64, 65, 128, 129, 416] and C.FIT_P == [1, 2, 31, 32, 33, 62, 63]
    assert C.FIT_LAMS == [1e-6, 5e-4, 1.0] and C.FIT_COUNTS == [1, 4, 5] and C.AXES == [None, 0.42, -0.9]
    for K in C.FIT_K:
        names = C.fit_patterns(K)
        rec = C.fit_records(K)
        act = C.active_slots(rec)
        assert rec.shape == (len(names), 3 * K + 1) and len(names) % C.CEP_WAVES != 0 and len(names) >= 5
        assert names[0] == "full" and names[-1] == "full_again" and np.array_equal(rec[0, :2 * K], rec[-1, :2 * K])
        assert act[0].all() and not act[names.index("empty")].any()
        am, f = rec[:, :K], rec[:, K:2 * K]
        i = names.index("empty")
        assert (am[i] != 0).any() or K == 1                       # off by f <= 0 with am != 0, and off by am == 0
        i = names.index("denormal")
        assert (am[i] == 5e-324).sum() == 1 and act[i].all()
        i = names.index("above_nyquist")
        assert (f[i] > C.FS / 2).sum() == 1 and act[i].all()
        if K == 1:
            continue
        assert set(names) == set(C.FIT_PATTERNS) - (set() if K >= 65 else {"chunk1_off"})
        assert np.flatnonzero(act[names.index("first")]).tolist() == [0]
        assert np.flatnonzero(act[names.index("last")]).tolist() == [K - 1]
        i = names.index("tied")
        assert len(np.unique(f[i])) == (K - 2 if K >= 4 else K - 1) and act[i].all()
        i = names.index("holes")
        if K >= 63:
            off = ~act[i]
            assert 0.25 < off.mean() < 0.55 and act[i, 0] and act[i, K - 1]
            assert (am[i] == 0).sum() >= 5 and ((f[i] == 0) & (am[i] != 0)).sum() >= 2 and ((f[i] < 0) & (am[i] != 0)).sum() >= 2
        if K >= 65:
            i = names.index("chunk1_off")
            assert not act[i, 64:128].any() and act[i, :64].all() and act[i, 128:].all()
            assert (am[i, 64:128] == 0).any() and (K == 65 or ((am[i, 64:128] != 0) & (f[i, 64:128] <= 0)).any())
    # a last chunk with one live lane (K = 65, 129), an empty chunk before a live one (K = 129, 416), an empty last chunk
    assert C.active_slots(C.fit_records(129))[C.fit_patterns(129).index("chunk1_off"), 128]
    assert not C.active_slots(C.fit_records(128))[C.fit_patterns(128).index("chunk1_off"), 64:].any()
    # the LDS ceiling: cep_wave_doubles as in csrc/eaqhm_cepstrum.hip
    assert C.cep_stride(31) == C.cep_stride(32) == 33 and C.cep_stride(63) == 65 and C.cep_stride(1) == 3
    for (K, P), (Kr, Pr) in zip(C.LDS_ACCEPTED, C.LDS_REFUSED):
        assert C.fit_lds_bytes(K, P) == C.CEPSTRUM_LDS_MAX == 163840 and (Kr, Pr) == (K + 1, P)
        assert C.fit_lds_bytes(Kr, Pr) > C.CEPSTRUM_LDS_MAX
    assert C.LDS_ACCEPTED == [(416, 63), (2555, 1)]
    # the grid readouts
    shapes = C.grid_shapes()
    assert {s[0] for s in shapes} == set(C.GRID_N) == {1, 3, 4, 5, 9} and {s[1] for s in shapes} == set(C.GRID_F) == {1, 63, 64, 65, 129}
    assert {s[2] for s in shapes} == set(C.GRID_P) == {1, 2, 32, 63} and len(set(shapes)) == len(shapes)
    assert C.GRID_B == [1, 2, 16] and C.GRID_ALPHAS == [0.25, 1.0, 4.0]
    assert C.GRID_MODES == ["none"] + ["alpha%g" % v for v in C.GRID_ALPHAS] + ["alpha_rows"] + ["map_B%d" % B for B in C.GRID_B]
    waves = {i % C.CEP_WAVES for i in C.EMPTY_ROWS[9]}
    assert waves == {0, 1, 2, 3} and all(len(C.EMPTY_ROWS[n]) < n for n in C.GRID_N)
    for n in C.GRID_N:
        for B in C.GRID_B:
            x, y = C.grid_map(n, B)
            assert y.shape == (n, B) and sum(np.array_equal(r, x) for r in y) == (1 if n > 1 else 0)
            assert n == 1 or (np.array_equal(y[n // 3], x) and n // 3 not in C.EMPTY_ROWS[n])
        al = C.grid_mode("alpha_rows", n)[0]
        live = ~np.isin(np.arange(n), C.EMPTY_ROWS[n])
        assert n == 1 or (((al == 1.0) & live).any() and ((al != 1.0) & live).any() and (n < 9 or (al.min() < 0.5 and al.max() > 2)))
        for F in C.GRID_F:
            fr = C.grid_freqs(F, n)
            nyq = C.FS / 2
            assert len(fr) == F and nyq in fr
            if F > 1:
                want = [0.0, np.nextafter(nyq, 0.0), np.nextafter(nyq, np.inf), 0.6 * C.FS]
                for B in C.GRID_B:
                    for k in C.grid_map(n, B)[1][C.knot_row(n)]:
                        want += [k, np.nextafter(k, 0.0), np.nextafter(k, np.inf)]
                assert all(v in fr for v in want), (n, F)
    # the amplitude readout and the build
    assert C.AMP_COUNTS == [4, 5, 9] and C.AMP_K == [1, 63, 64, 65, 129]
    for n in C.AMP_COUNTS:
        for K in C.AMP_K:
            c = C.amp_case(n, K)
            f = c["rec"][:, K:2 * K]
            for i in range(n):
                if c["edge"][i] >= 0:
                    assert c["beta"][i] * f[i, c["edge"][i]] == C.FS / 2
                if c["below"][i] >= 0:
                    assert c["beta"][i] * f[i, c["below"][i]] == np.nextafter(C.FS / 2, 0.0)
            live = ~np.isin(np.arange(n), C.EMPTY_ROWS[n])
            assert ((c["edge"] >= 0) & live).any() and ((c["below"] >= 0) & live).any()
    assert C.BUILD_N == [2, 3, 4, 5, 9] and C.BUILD_K == [1, 63, 64, 65, 129] and C.KCAP == 1706
    assert {"nyquist", "unvoiced", "empty", "underflow", "theta0", "theta_top"} <= set(C.INSTANTS) and len(C.INSTANTS) == 9
    for n in C.BUILD_N:
        for K in C.BUILD_K:
            c = C.build_case(n, K)
            assert c["fs"] == (48000.0 if K == 129 else 16000.0) and np.float64(c["edge_h"]) * c["f0"][1] == c["fs"] / 2
            assert c["edge_h"] == (1 if K == 1 else 128 if K == 129 else 8) and (K != 129 or abs(c["f0"][0] - 180) <= 2)
            if n == 9:
                assert c["theta"][3] == 0.0 and c["theta"][6] == np.nextafter(1.0, 0.0) and not c["voiced"][2]
                rows = C.build_rows(n, K, 63, None)
                assert np.isneginf(rows[4, 0]) and rows[5, 0] == -800.0
                m = C.build_models(n, K, 63, None, 0)["m"]
                assert not m["active"][[2, 4, 5]].any() and not m["active"][1, c["edge_h"] - 1:].any()
                assert m["active"][[0, 3, 6, 7, 8]].all() and (K == 1 or m["active"][1, c["edge_h"] - 2])


# ---- the yardsticks
def _cholesky_and_longdouble(rec, fs, P, lam, a, m):
    K = (rec.shape[1] - 1) // 3
    for i in np.flatnonzero(~m["empty"]):
        w, v = CR.nodes(rec[i, :K], rec[i, K:2 * K], fs) if a is None else CW.nodes(rec[i, :K], rec[i, K:2 * K], fs, a)
        np.linalg.cholesky(CR.system(w, v, P, lam)[0])          # raises if the instant does not factor in float64
    assert np.all(np.isfinite(m["c_l"][~m["empty"]])) and np.all(np.isfinite(m["c"][~m["empty"]]))
    assert np.all(m["dev"][~m["empty"]] > 0) and np.all(m["dev"][m["empty"]] == 0) and m["dev_case"] == m["dev"].max()
    top = np.abs(m["c"][~m["empty"]]).max(axis=1)
    assert np.all(m["dev"][~m["empty"]] < 1e-6 * top), (m["dev"], top)


@pytest.mark.slow
@pytest.mark.parametrize("a", C.AXES, ids=C.axis_name)
def test_fit_yardsticks_and_every_instant_factors(a):
    devs = []
    for K in C.FIT_K:
        for P in C.FIT_P:
            for lam in C.FIT_LAMS:
                m = C.fit_models(K, P, lam, a)
                _cholesky_and_longdouble(C.fit_records(K), C.FS, P, lam, a, m)
                devs.append(m["dev_case"])
    for K, P in C.LDS_ACCEPTED:
        for lam in (1e-6, 5e-4):
            m = C.fit_models_of(("lds", K), C.lds_records(K), C.FS, P, lam, a)
            _cholesky_and_longdouble(C.lds_records(K), C.FS, P, lam, a, m)
    print("fit yardsticks %s: %.3g .. %.3g" % (C.axis_name(a), min(devs), max(devs)))


def test_breakdown_inputs_in_the_model():
    good, bad = C.breakdown_records()
    K = C.BREAK_K
    assert len(good) == 8 and C.active_slots(bad[None, :]).sum() == 1
    for P, a in C.BREAK_CASES:
        assert C.first_pivots(bad, C.FS, C.BREAK_LAM, a) == (1.0, 2.0, 4.0, 0.0)
        for i in range(len(good)):
            w, v = CR.nodes(good[i, :K], good[i, K:2 * K], C.FS) if a is None else CW.nodes(good[i, :K], good[i, K:2 * K], C.FS, a)
            G = CR.system(w, v, P, C.BREAK_LAM)[0]
            np.linalg.cholesky(G)
            assert np.linalg.cond(G) < 1e9, (P, a, i)
    assert {P for P, _ in C.BREAK_CASES} >= {1, 2, 8} and {a for _, a in C.BREAK_CASES} == set(C.AXES)


@pytest.mark.parametrize("a", C.AXES, ids=C.axis_name)
def test_readout_amplitude_and_build_yardsticks(a):
    env, ph, amp, bam, bph = [], [], [], [], []
    for n, F, P in C.grid_shapes():
        for mode in C.GRID_MODES:
            m = C.grid_models(n, F, P, a, mode)
            assert m["dev_env"] > 0 and m["dev_ph"] > 0, (n, F, P, mode)
            assert np.all(np.isneginf(m["env"][m["empty"]])) and np.all(m["ph"][m["empty"]] == 0)
            assert np.all(np.isfinite(m["env"][~m["empty"]]))
            env.append(m["dev_env"])
            ph.append(m["dev_ph"])
    for n in C.AMP_COUNTS:
        for K in C.AMP_K:
            for P in C.AMP_P:
                for mode in C.AMP_MODES:
                    m = C.amp_models(n, K, P, a, mode)
                    c = C.amp_case(n, K)
                    assert 0 < m["dev"] < np.inf, (n, K, P, mode)
                    live = ~np.isneginf(C.amp_rows(n, P, a)[:, 0])
                    for i in range(n):
                        assert c["edge"][i] < 0 or m["amp"][i, c["edge"][i]] == 0
                        assert c["below"][i] < 0 or not live[i] or m["amp"][i, c["below"][i]] > 0
                    amp.append(m["dev"])
    for n in C.BUILD_N:
        for K in C.BUILD_K:
            for P in C.BUILD_P:
                for z in (0, 1):
                    m = C.build_models(n, K, P, a, z)
                    assert 0 < m["dev_am"] < np.inf and m["dev_ph"] > 0, (n, K, P, z)
                    bam.append(m["dev_am"])
                    bph.append(m["dev_ph"])
    print("yardsticks %s: envelope %.3g .. %.3g, phase %.3g .. %.3g, amplitudes %.3g .. %.3g, build am %.3g .. %.3g, "
          "build ph %.3g .. %.3g" % (C.axis_name(a), min(env), max(env), min(ph), max(ph), min(amp), max(amp), min(bam),
                                     max(bam), min(bph), max(bph)))


# ---- the kernels' route, and the deliberate errors as switches of it
def _fit_variant(rec, fs, P, lam, a, restart=False, drop_partial=False, bP_single=False, linear_penalty=False,
                 shift=0, flip=False):
    """The fit by the kernel's route in float64: the active slots packed 64 at a time behind a running count, T_d = sum
    cos(d w_n), d = 0..2P, G_00 = T_0, G_p0 = 2 T_p, G_pq = 2 (T_|p-q| + T_{p+q}) + lam 8 pi^2 p^2 [p == q], b_0 = sum v,
    b_p = 2 sum v cos(p w_n).  Switches: the count restarted at each chunk; the last partial chunk dropped; b_P without
    its factor 2; the penalty in p; T read at p + q - shift; the axis at -a."""
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    out = np.zeros((n, P + 1))
    for i in range(n):
        am, f = rec[i, :K], rec[i, K:2 * K]
        sw, sv, nn = np.zeros(K), np.zeros(K), 0
        for k0 in range(0, K, 64):
            if drop_partial and k0 + 64 > K:
                break
            ks = np.arange(k0, min(k0 + 64, K))
            act = (am[ks] != 0) & (f[ks] > 0)
            pos = (0 if restart else nn) + np.cumsum(act) - act
            w = (2 * np.pi) * f[ks][act] / fs
            sw[pos[act]] = w if a is None else CW.omega(-a if flip else a, w)
            sv[pos[act]] = np.log(am[ks][act])
            nn += int(act.sum())
        if nn == 0:
            out[i] = CR._empty_row(P, np.float64)
            continue
        w, v = sw[:nn], sv[:nn]
        cs = np.cos(np.arange(2 * P + 1)[:, None] * w[None, :])
        T = cs.sum(axis=1)
        b = 2 * (cs[:P + 1] * v[None, :]).sum(axis=1)
        b[0] /= 2
        if bP_single:
            b[P] /= 2
        G = np.zeros((P + 1, P + 1))
        for r in range(P + 1):
            for q in range(r + 1):
                g = (T[0] if r == 0 else 2 * T[r]) if q == 0 else 2 * (T[r - q] + T[r + q - shift])
                if r == q:
                    g += lam * (8 * np.pi ** 2) * (r if linear_penalty else r * r)
                G[r, q] = G[q, r] = g
        out[i] = np.linalg.solve(G, b)
    return out


def _fit_rows(variant_kw, Ks=C.FIT_K, Ps=(1, 32, 63), lams=(1e-6, 1.0), axes=C.AXES):
    """(instant name, coefficient difference, the launch's yardstick) of the variant against the model; inf where
    emptiness differs."""
    rows = []
    for K in Ks:
        rec, names = C.fit_records(K), C.fit_patterns(K)
        for P in Ps:
            for lam in lams:
                for a in axes:
                    m = C.fit_models(K, P, lam, a)
                    got = _fit_variant(rec, C.FS, P, lam, a, **variant_kw)
                    for i in np.flatnonzero(~m["empty"]):
                        d = float(np.abs(got[i] - m["c"][i]).max()) if np.isfinite(got[i, 0]) else np.inf
                        rows.append(("K%d_P%d_lam%g_%s_%s" % (K, P, lam, C.axis_name(a), names[i]), d, m["dev_case"]))
    return rows


def _series_variant(Cr, fs, q, a, hold=0.5, flip=False):
    """(C, Phi) at the read frequencies q [n, F] by the direct sums; switches: the hold at `hold` fs, the axis at -a."""
    Cr = np.asarray(Cr, dtype=np.float64)
    x = np.minimum(np.maximum(q, 0.0), hold * fs)
    th = ((2 * np.pi) * x) / fs
    if a is not None:
        th = CW.omega(-a if flip else a, th)
    fin = np.where(np.isfinite(Cr), Cr, 0.0)
    sc, ss = np.zeros(x.shape), np.zeros(x.shape)
    for p in range(1, Cr.shape[1]):
        sc += Cr[:, p, None] * np.cos(p * th)
        ss += fin[:, p, None] * np.sin(p * th)
    return 2 * sc + Cr[:, 0, None], -2 * ss


def _grid_rows_of(hold=0.5, flip=False, drop_knot=False):
    rows = []
    for n, F, P in C.grid_shapes():
        for a in C.AXES:
            for mode in C.GRID_MODES:
                m = C.grid_models(n, F, P, a, mode)
                alpha, warp = C.grid_mode(mode, n)
                if drop_knot and warp is not None and len(warp[0]) > 1:
                    warp = (warp[0][:-1], warp[1][:, :-1])
                env, ph = _series_variant(C.grid_rows(n, P, a), C.FS, CR.read_frequency(C.grid_freqs(F, n), n, alpha, warp),
                                          a, hold, flip)
                live = ~m["empty"]
                name = "n%d_F%d_P%d_%s_%s" % (n, F, P, C.axis_name(a), mode)
                rows.append((name + " envelope", float(np.abs(env[live] - m["env"][live]).max()), m["dev_env"]))
                rows.append((name + " phase", float(np.abs(C.wrapped(ph[live] - m["ph"][live])).max()), m["dev_ph"]))
    return rows


def _amp_rows_of(mute_gt=False):
    rows = []
    for n in C.AMP_COUNTS:
        for K in C.AMP_K:
            c = C.amp_case(n, K)
            am, fm = c["rec"][:, :K], c["rec"][:, K:2 * K]
            bf = c["beta"][:, None] * fm
            active = (am != 0) & (fm > 0)
            for P in C.AMP_P:
                for a in C.AXES:
                    for mode in C.AMP_MODES:
                        m = C.amp_models(n, K, P, a, mode)
                        alpha, warp = C.grid_mode(mode, n)
                        q = CR.read_frequency(np.where(active, bf, 0.0), n, alpha, warp)
                        A = np.exp(_series_variant(C.amp_rows(n, P, a), C.FS, q, a)[0])
                        got = np.where(active & ((bf <= C.FS / 2) if mute_gt else (bf < C.FS / 2)), A, 0.0)
                        rows.append(("n%d_K%d_P%d_%s_%s" % (n, K, P, C.axis_name(a), mode), C.rel_error(got, m["amp"]), m["dev"]))
    return rows


def _build_rows_of(le=False, h_from_zero=False):
    """cepstrum_direct_cases.model_build with switches: slot k active while h f0 <= fs/2; the carrier of harmonic k
    where k + 1 belongs."""
    rows = []
    for n in C.BUILD_N:
        for K in C.BUILD_K:
            case = C.build_case(n, K)
            fs, f0, th = case["fs"], case["f0"], case["theta"]
            for P in C.BUILD_P:
                for a in C.AXES:
                    Cr = C.build_rows(n, K, P, a)
                    mm = C.build_models(n, K, P, a, 0)
                    has = case["voiced"] & ~np.isneginf(Cr[:, 0])
                    h = np.arange(1, K + 1, dtype=np.float64)
                    fm = h[None, :] * f0[:, None]
                    live = has[:, None] & ((fm <= fs / 2) if le else (fm < fs / 2))
                    Cs = np.where(has[:, None], Cr, 0.0)
                    lnam, phi = MB.series(Cs, fs, fm) if a is None else CW.series(Cs, fs, fm, a)
                    am = np.exp(lnam)
                    active = live & (am != 0)
                    ht = (h - 1 if h_from_zero else h)[None, :] * th[:, None]
                    ph = np.where(active, MB.wrap((2 * np.pi) * (ht - np.floor(ht)) + phi), 0.0)
                    name = "n%d_K%d_P%d_%s" % (n, K, P, C.axis_name(a))
                    rows.append((name + " am", C.rel_error(np.where(active, am, 0.0), mm["m"]["am"]), mm["dev_am"]))
                    same = active == mm["m"]["active"]
                    rows.append((name + " ph", float(np.abs(C.wrapped(ph - mm["m"]["ph"]))[same].max()), mm["dev_ph"]))
    return rows


def _worst(rows):
    """rows of (case name, difference, yardstick): the largest difference in units of 100 yardsticks and its case."""
    ratio, name = max((d / (100 * y), nm) for nm, d, y in rows if y > 0)
    return ratio, name


def test_the_kernels_route_without_an_error_stays_within_every_bar():
    ratio, name = _worst(_fit_rows({}))
    print("the fit by packed nodes and T_d: at most %.3g of the bar (%s)" % (ratio, name))
    assert ratio <= 1, (ratio, name)
    for rows in (_grid_rows_of(), _amp_rows_of(), _build_rows_of()):      # the linear phase: direct sum against Clenshaw
        ratio, name = _worst(rows)
        assert ratio <= 1, (ratio, name)


FIT_ERRORS = {"a compaction that restarts its count at each 64-slot chunk": dict(restart=True),
              "a compaction that drops the last partial chunk": dict(drop_partial=True),
              "b_P without its factor 2": dict(bP_single=True),
              "a penalty in p instead of p^2": dict(linear_penalty=True),
              "T read at r + q - 1": dict(shift=1),
              "the warped axis with the sign of a flipped (fit)": dict(flip=True)}


@pytest.mark.parametrize("error", sorted(FIT_ERRORS))
def test_fit_cases_notice(error):
    kw = FIT_ERRORS[error]
    rows = _fit_rows(kw, Ks=(65, 129) if ("restart" in kw or "drop_partial" in kw) else (2, 64),
                     axes=(0.42,) if "flip" in kw else (None, -0.9))
    ratio, name = _worst(rows)
    print("%s: %s moves by %.3g x its bar" % (error, name, ratio))
    assert ratio > 1, "%s: no fit case notices it; the nearest is %s at %.3g of its bar" % (error, name, ratio)
    if "restart" in kw or "drop_partial" in kw:      # every instant with a node past slot 63 notices it, by itself
        hit = [nm for nm, d, y in rows if d > 100 * y]
        for pat in ("full", "holes", "tied") + (("last",) if "drop_partial" in kw else ()):    # `last` restarts at 0 anyway
            assert any(nm.endswith(pat) for nm in hit), (error, pat)


OTHER_ERRORS = {"a hold at fs instead of fs/2": lambda: _grid_rows_of(hold=1.0),
                "the warped axis with the sign of a flipped (readout)": lambda: _grid_rows_of(flip=True),
                "a map that ignores its last knot": lambda: _grid_rows_of(drop_knot=True),
                "muting at > instead of >=": lambda: _amp_rows_of(mute_gt=True),
                "h f0 <= fs/2": lambda: _build_rows_of(le=True),
                "the carrier of harmonic k where k + 1 belongs": lambda: _build_rows_of(h_from_zero=True)}


@pytest.mark.parametrize("error", sorted(OTHER_ERRORS))
def test_readout_amplitude_and_build_cases_notice(error):
    ratio, name = _worst(OTHER_ERRORS[error]())
    print("%s: %s moves by %.3g x its bar" % (error, name, ratio))
    assert ratio > 1, "%s: no case notices it; the nearest is %s at %.3g of its bar" % (error, name, ratio)


def test_dtype_arguments_of_the_linear_model():
    """model_cepstrum_ref's readout, clenshaw, envelope and amplitudes in np.longdouble: the float64 call is the former
    function bit for bit (the direct sum of model_build_ref.series' argument), the long double one is long double and
    agrees with cepstrum_warp_ref's at a = 0."""
    Cr = C.grid_rows(9, 63, None)
    fr = C.grid_freqs(65, 9)
    al = C.grid_mode("alpha_rows", 9)[0]
    ld = np.longdouble
    assert CR.readout(Cr, C.FS, fr).dtype == np.float64 and CR.readout(Cr, C.FS, fr, ld).dtype == ld
    live = ~np.isneginf(Cr[:, 0])
    for fn in (CR.readout, CR.clenshaw):
        assert np.abs(fn(Cr, C.FS, fr, ld) - CW.readout(Cr, C.FS, fr, 0.0, ld))[live].max() < 1e-15
        assert np.all(np.isneginf(fn(Cr, C.FS, fr, ld)[~live]))
    assert np.array_equal(CR.envelope(Cr, C.FS, fr, al), CR.readout(Cr, C.FS, CR.read_frequency(fr, 9, al)))
    assert np.abs(CR.envelope(Cr, C.FS, fr, al, None, ld) - CW.envelope(Cr, C.FS, fr, 0.0, al, None, ld))[live].max() < 1e-15
    c = C.amp_case(9, 65)
    am, fm = c["rec"][:, :65], c["rec"][:, 65:130]
    A, Al = CR.amplitudes(am, fm, C.FS, c["beta"], Cr), CR.amplitudes(am, fm, C.FS, c["beta"], Cr, dtype=ld)
    assert A.dtype == np.float64 and Al.dtype == ld and np.array_equal(A == 0, Al == 0) and 0 < C.rel_error(Al, A) < 1e-12
