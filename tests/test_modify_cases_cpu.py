"""The hand-built models of tests/modify_cases.py and the NumPy model of DESIGN.md §9 on them, without a GPU: the cases
hold the patterns, block sizes and row caches they were built for; the fm piece of a short run whose pad instants are its
own knots is the polynomial of lowest degree through its nodes, in float64 and in long double, and every other run is
what it was; and the long-double model decides every whole-turn count of every case with the project's margin to
spare, so that nothing has to be left out of the GPU comparison."""
import numpy as np
import pytest
from scipy.interpolate import make_interp_spline

import model_contour_ref as MC
import model_synthesis_ref as M
import modify_cases as C

CASES = C.cases()
NAMES = [c["name"] for c in CASES]
MARGIN = 1e-9
EPS = np.finfo(np.float64).eps


def case(name):
    return CASES[NAMES.index(name)]


def test_the_named_cases_and_their_shapes():
    assert NAMES == ["chunks", "k150", "k300", "tiny_run4", "tiny_start3", "step2", "long", "start", "harm125"]
    shapes = {c["name"]: (c["No_ti"], c["Kmax"], c["step"], c["fs"]) for c in CASES}
    assert shapes == dict(chunks=(140, 70, 15, 16000.0), k150=(12, 150, 15, 48000.0), k300=(12, 300, 15, 48000.0),
                          tiny_run4=(4, 1, 15, 16000.0), tiny_start3=(4, 1, 15, 16000.0), step2=(40, 3, 2, 16000.0),
                          long=(4200, 3, 15, 16000.0), start=(12, 6, 15, 16000.0), harm125=(8, 40, 15, 16000.0))
    for c in CASES:
        n, K = c["No_ti"], c["Kmax"]
        rec = c["records"]
        assert rec.shape == (n, 3 * K + 1) and np.all(np.isfinite(rec))
        assert c["L"] == (n - 1) * c["step"] + 1 + 133
        assert np.all(rec[:, 3 * K] != 0)                                       # an a0 column that is not zero
        act = c["active"]
        assert np.array_equal(rec[:, :K] != 0, act) and np.all(rec[:, :K] >= 0)
        assert np.all(rec[:, K:2 * K][act] > 0) and np.all(rec[:, K:2 * K][act] < c["fs"] / 2)
        assert np.all(rec[:, K:3 * K][~np.tile(act, (1, 2))] == 0)
        assert c["settings"] == (C.SETTINGS_LONG if c["name"] == "long" else C.SETTINGS)
        assert max(int(np.rint(rho * c["L"])) for rho, _, _ in c["settings"]) <= 95000
    assert C.SETTINGS == [(1.0, 1.0, True), (0.25, 1.3, True), (4.0, 0.5, True), (0.7, 1.0, False), (1.5, 2.0, True)]
    assert len(C.SETTINGS_LONG) == 4


@pytest.mark.parametrize("name", NAMES)
def test_every_pattern_by_its_run_code(name):
    c = case(name)
    code, _ = M.run_codes(c["active"])
    assert c["checks"]
    for label, k, i, want in c["checks"]:
        assert code[i, k] == want, (label, k, i, int(code[i, k]), want)


def test_chunks_patterns():
    c = case("chunks")
    code, runs = M.run_codes(c["active"])
    n = c["No_ti"]
    assert runs[0] == [(0, n - 1)] and runs[1] == [] and runs[2][-1][1] == 63 and runs[3][0][0] == 64
    assert runs[4] == [(63, 64)] and runs[5] == [(62, 65)] and runs[6] == [(64, 64)]
    assert runs[7] == [(0, 126), (129, n - 1)] and runs[8] == [(0, 0), (n - 1, n - 1)]
    assert runs[9] == [(n - 2, n - 1)] and runs[10] == [(n - 3, n - 1)]
    # short interior runs of 1, 2 and 3 knots behind an active and behind an empty start
    for k, start_active in ((11, True), (12, False)):
        assert bool(c["active"][:3, k].all()) == start_active and bool(c["active"][:3, k].any()) == start_active
        assert {b - a + 1 for a, b in runs[k] if a > 3} >= {1, 2, 3}
    # gaps in the second 64-lane pass of env_compact / env_rank, at instants where the first pass has them too
    hi = c["active"][:, 64:]
    assert not hi.all() and hi.any() and any(0 < hi[i].sum() < hi.shape[1] for i in range(n))
    # the slot order is not the frequency order, at any instant with two active slots
    K = c["Kmax"]
    f = c["records"][:, K:2 * K]
    for i in (0, 64, n - 1):
        ks = np.flatnonzero(c["active"][i])
        assert not np.array_equal(np.argsort(f[i, ks], kind="stable"), np.arange(len(ks)))
    assert not np.array_equal(c["freq_rank"], np.arange(K))


def test_block_sizes_and_row_caches():
    """Through the mirror of modify_block_samples: (samples per block, staged rows, rows wanted)."""
    for rho, _, _ in C.SETTINGS:
        assert C.modify_block_samples(70, 15, rho)[0] == 64
        assert C.modify_block_samples(150, 15, rho)[0] == 32
        tbs, nr, want, b = C.modify_block_samples(300, 15, rho)
        assert (tbs, nr) == (16, 4) and want > nr and b > C.LDS_BUDGET        # the tbs == 16 fall-through
        assert C.modify_block_samples(1, 15, rho)[0] == 64 and C.modify_block_samples(3, 2, rho)[0] == 64
    assert C.modify_block_samples(70, 15, 0.25)[:3] == (64, 18, 23)
    assert C.modify_block_samples(70, 15, 1.0)[1:3] == (11, 11)                 # uncapped where the rows fit
    # the contour and shape kernels of the direct tests on `chunks`: rate_min of rho = 0.25 + 0.5 x, and (1.5, 1.2)
    rho, beta = C.contour_scales(140)
    rmin = float(MC.time_map(rho, beta, 15, case("chunks")["L"])[0].min())
    tbs, nr, want, _ = C.modify_block_samples(70, 15, rmin, crow=3)
    assert tbs == 64 and nr < want
    tbs, nr, want, _ = C.modify_block_samples(70, 15, rmin, crow=3, shape=1)
    assert (tbs, nr) == (64, 17) and nr < want
    assert C.modify_block_samples(150, 15, 0.25)[1:3] == (8, 15)
    # an inconsistency between the mirror and the formula would show here: bytes grow with every argument
    assert C.modify_lds_bytes(70, 15, 64, 18) <= C.LDS_BUDGET < C.modify_lds_bytes(70, 15, 64, 19)


def test_step2_long_start_and_tiny_patterns():
    c = case("step2")
    code, runs = M.run_codes(c["active"])
    assert [a for a, b in runs[0]] == list(range(0, 40, 2)) and all(a == b for a, b in runs[0])
    assert [a for a, b in runs[1]] == list(range(1, 40, 4)) and all(a == b for a, b in runs[1])
    # several isolated knots on one output sample (the walk of iso_range): isolated knots of one slot lie two instants
    # or more apart, so they are knots of slots 0 and 1, under the contour rho = 0.25 + 0.5 x and at rho = 0.25
    iso = np.array(sorted([a for a, _ in runs[0]] + [a for a, _ in runs[1]]))
    rho, beta = C.contour_scales(40)
    _, _, Ck, _ = MC.time_map(rho, beta, 2, c["L"])
    for ns in (np.rint(Ck[iso]).astype(int), np.rint(0.25 * (iso * 2.0)).astype(int)):
        assert np.bincount(ns).max() >= 2
    c = case("long")
    code, runs = M.run_codes(c["active"])
    assert (c["No_ti"] + C.SCAN_CH - 1) // C.SCAN_CH == 66
    assert runs[0] == [(0, 4199)] and (4096, 4199) in runs[1] and (100, 4095) in runs[2]
    assert 4096 == C.SCAN_CH * C.CARRY_TILE
    c = case("start")
    code, runs = M.run_codes(c["active"])
    for k, r in {**C.START_COLLIDING, **C.START_PLAIN}.items():
        assert runs[k][0] == r
    assert M.run_codes(case("tiny_run4")["active"])[1] == [[(0, 3)]]
    assert M.run_codes(case("tiny_start3")["active"])[1] == [[(0, 2)]]


def test_harm125_envelope_reads():
    c = case("harm125")
    K, fs = c["Kmax"], c["fs"]
    rec = c["records"]
    am, fm = rec[:, :K], rec[:, K:2 * K]
    slot = c["slot_of"]
    f = np.where(c["active"], fm, 0.0)
    harm = 125.0 * (np.arange(K) + 1)
    dup_from, dup_to = C.HARM_DUP
    for h in range(K):
        want = harm[dup_to] if h == dup_from else harm[h]
        assert np.all(f[c["active"][:, slot[h]], slot[h]] == want)
    assert np.array_equal(c["active"].sum(axis=1), [K, K, K, 1, K, 0, K, K])
    i = 0
    ks = np.flatnonzero(c["active"][i])
    nodes = np.sort(fm[i, ks])
    # beta = 2: every read frequency up to the top node is exactly a node; 4000 Hz lands on fs/2 and is muted, 3875 not
    q = 2.0 * fm[i, ks]
    assert np.all(np.isin(q[q <= nodes[-1]], nodes)) and np.count_nonzero(q <= nodes[-1]) >= 19
    A2 = M.envelope_amplitudes(am, fm, fs, 2.0, True)
    A2l = M.envelope_amplitudes(am, fm, fs, 2.0, True, np.longdouble)
    assert A2[i, slot[31]] == 0 and A2l[i, slot[31]] == 0 and 2.0 * harm[31] == fs / 2
    assert A2[i, slot[30]] > 0 and A2l[i, slot[30]] > 0 and harm[30] == 3875.0
    assert np.all(A2[i, slot[32:]] == 0) and np.all(A2[i, slot[:31]] > 0)
    # a node hit returns the node's own amplitude, exactly up to exp(log()): harmonic 4 reads harmonic 8's node
    assert abs(A2[i, slot[3]] / am[i, slot[7]] - 1.0) <= 4 * EPS
    # the tie at 750 Hz: the lower slot's node wins
    first = min(slot[dup_from], slot[dup_to])
    assert abs(A2[i, slot[2]] / am[i, first] - 1.0) <= 4 * EPS
    # beta = 0.5: odd harmonics read exactly half way between two nodes: the geometric mean of their amplitudes
    Ah = M.envelope_amplitudes(am, fm, fs, 0.5, True)
    for h in (8, 20, 38):                                                      # harmonic h+1 odd, away from the tie
        lo, hi = am[i, slot[(h + 1) // 2 - 1]], am[i, slot[(h + 1) // 2]]
        assert abs(Ah[i, slot[h]] / np.sqrt(lo * hi) - 1.0) <= 16 * EPS
    assert np.all(Ah[C.HARM_NONE] == 0) and np.count_nonzero(Ah[C.HARM_SINGLE]) == 1


# ---------------------------------------------------------------------------------------------- the node rule
def _old_four_node_path(fm_col, active_col, s, e, D):
    """The fm piece of a short run as the model had it before the node rule: always 4 - m pad nodes."""
    m = e - s + 1
    knots = np.arange(s, e + 1) * D
    npad = 4 - m
    pad = np.arange(npad)
    x = np.concatenate((pad * D, knots))
    y = np.concatenate((np.where(active_col[pad], fm_col[pad], 0.0), fm_col[s:e + 1]))
    return make_interp_spline(x.astype(np.float64), y, k=3)(np.arange(knots[0], knots[-1] + 1, dtype=np.float64))


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_colliding_start_runs_are_the_lowest_degree_polynomial(dtype):
    c = case("start")
    K, D = c["Kmax"], c["step"]
    fm, act = c["records"][:, K:2 * K], c["active"]
    eps = float(np.finfo(dtype).eps)
    for k, (s, e) in C.START_COLLIDING.items():
        with pytest.raises(ValueError):
            _old_four_node_path(fm[:, k], act[:, k], s, e, D)                   # the hole this rule closes
        got = M._fm_piece_values(fm[:, k], act[:, k], s, e, D, dtype)
        x = np.arange(s * D, e * D + 1).astype(dtype)
        y = fm[:, k].astype(dtype)
        h = dtype(D)
        if (s, e) == (0, 1):                                                    # the line through its 2 knots
            want = y[0] + (y[1] - y[0]) * (x / h)
        else:                                                                   # the parabola through instants 0, 1, 2
            y0 = dtype(0.0) if s == 1 else y[0]                                 # instant 0 is an inactive pad: 0
            t = x / h
            d1, d2 = y[1] - y0, (y[2] - dtype(2) * y[1]) + y0
            want = y0 + t * d1 + t * (t - dtype(1)) * d2 / dtype(2)             # Newton's forward form
        assert got.dtype == np.dtype(dtype) and np.all(np.isfinite(got.astype(np.float64)))
        scale = float(np.abs(y[:3]).max())
        assert float(np.abs(got - want).max()) <= 64 * eps * scale, (k, float(np.abs(got - want).max()))
        assert abs(float(got[0] - y[s])) <= 16 * eps * scale and abs(float(got[-1] - y[e])) <= 16 * eps * scale
    nodes = {k: M.short_run_nodes(fm[:, k], act[:, k], s, e, D)[0].tolist() for k, (s, e) in C.START_COLLIDING.items()}
    assert nodes == {0: [0, 1], 1: [0, 1, 2], 2: [0, 1, 2]}


def test_other_start_runs_are_bit_for_bit_what_they_were():
    c = case("start")
    K, D = c["Kmax"], c["step"]
    fm, act = c["records"][:, K:2 * K], c["active"]
    for k, (s, e) in C.START_PLAIN.items():
        if s == e:
            continue                                                            # isolated: no fm piece
        assert np.array_equal(M._fm_piece_values(fm[:, k], act[:, k], s, e, D), _old_four_node_path(fm[:, k], act[:, k], s, e, D))
        assert len(M.short_run_nodes(fm[:, k], act[:, k], s, e, D)[0]) == 4
    c = case("chunks")
    K = c["Kmax"]
    fm, act = c["records"][:, K:2 * K], c["active"]
    code, runs = M.run_codes(act)
    for k in (11, 12, 9, 10, 4):
        for s, e in runs[k]:
            if 2 <= e - s + 1 <= 3:
                assert np.array_equal(M._fm_piece_values(fm[:, k], act[:, k], s, e, D),
                                      _old_four_node_path(fm[:, k], act[:, k], s, e, D))


@pytest.mark.parametrize("name", ["start", "tiny_start3", "harm125"])
def test_models_are_finite_on_the_colliding_starts(name):
    c = case(name)
    for rho, beta, env in c["settings"]:
        for dt in (np.float64, np.longdouble):
            out = M.synthesize(c["records"], c["step"], c["fs"], c["L"], rho, beta, env, dtype=dt)
            assert out.dtype == np.dtype(dt) and len(out) == int(np.rint(rho * c["L"]))
            assert np.all(np.isfinite(out.astype(np.float64)))


# ---------------------------------------------------------------------------------------------- a condition on the inputs
@pytest.mark.parametrize("name", NAMES)
def test_every_whole_turn_count_is_decided_with_the_margin(name):
    """In the long-double model every in-run interval of the case decides rint(e / 2 pi) with at least MARGIN to spare,
    so the GPU tests leave no cell out.  A seed that falls short is changed, not excused."""
    c = case(name)
    mg = M.round_margins(c["records"], c["step"], c["fs"], np.longdouble)
    code, _ = M.run_codes(c["active"])
    inrun = (code[:-1] != 0) & (code[1:] != 0)
    assert np.array_equal(np.isfinite(mg), inrun)
    short = int(np.count_nonzero(mg[inrun] < MARGIN))
    print("%s: %d in-run intervals, smallest margin %.3g" % (name, int(inrun.sum()), float(mg[inrun].min())))
    assert short == 0
    mg64 = M.round_margins(c["records"], c["step"], c["fs"], np.float64)
    assert int(np.count_nonzero(mg64[inrun] < MARGIN)) == 0


def test_float64_and_long_double_models_agree():
    """The two arithmetics of the model on the smaller cases: same paths, rounding apart."""
    for name in ("start", "step2", "harm125", "tiny_run4"):
        c = case(name)
        for rho, beta, env in c["settings"]:
            a = M.synthesize(c["records"], c["step"], c["fs"], c["L"], rho, beta, env)
            b = M.synthesize(c["records"], c["step"], c["fs"], c["L"], rho, beta, env, dtype=np.longdouble)
            assert float(np.abs(a - b).max()) <= 1e-10 * float(np.abs(a).max()), (name, rho, beta)
