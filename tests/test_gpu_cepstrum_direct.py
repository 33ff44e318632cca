"""The cepstrum kernels of csrc/eaqhm_cepstrum.hip on the MI355X, directly, at every node count, order and grid edge:
the cases of tests/cepstrum_direct_cases.py (tests/test_cepstrum_direct_cases_cpu.py shows that they can judge a kernel)
through the context's raw entry points on hand-built device tensors: Context.model_cepstrum, modify_amp_cepstrum,
cepstrum_envelope, cepstrum_phase and model_build, and their `_warped` forms at a = 0.42 and a = -0.9.  No analysis
runs and no signals.

Bars: DESIGN.md §10's rule.  A kernel output is held to 100 x the deviation between the NumPy model in float64 and in
np.longdouble on the same case, computed when the test runs.  A case is one call.  For the fit that is a launch, which
carries every activity pattern as its instants: each instant's largest coefficient error against the launch's largest
deviation.  Amplitudes (readout and
build) relative, per call; envelopes absolute in log amplitude; phases as wrapped differences mod 2 pi, for the
yardstick and for the kernel alike.  There is no fixed tolerance and nothing is excluded.  Every test records both
figures of its worst comparisons (record_measurement "cepstrum_direct_..."); DESIGN.md §9.5 tabulates the largest
ratio per kernel and axis.

Measured on the MI355X, the largest kernel error in units of the call's yardstick (linear, a = 0.42, a = -0.9): fit 79.8
(K 2, P 2, lam 1), 43.8, 19.6; envelope 4.0, 3.0, 1.7; phase 2.2, 2.4, 1.1; amplitudes 3.9, 2.0, 1.2; build am 5.9, 2.4,
20.5 (n 3, Kmax 1: a single cell); build phase 1.1, 2.7, 1.3; a = 0 through the warped entry points at most 1.5 (the
fit: the plain kernel's bits).  Two calls first missed, both at a = -0.9 and P = 63: the warped envelope at (n 9, F 1)
under the alpha contour came to 264, the warped build's amplitude at (n 3, Kmax 1) to 102: the recurrence ran from
2 cos Omega, which no longer tells Omega where the axis crowds a band towards 0; the warped readouts now run it in
Reinsch's form (1.7 and 20.5).

Beside the bars, exact: an empty instant fits (-inf, 0, .., 0); an empty row reads -inf from the envelope, 0 from the
phase and gives 0 amplitudes; muted and inactive cells are 0; every cell whose read frequency is >= fs/2 equals the
row's value at fs/2 bit for bit; alpha = 1.0 and identity-map rows equal the plain call bit for bit; an instant or a
row gives the same bits wherever it lies in the call and whatever else the call holds; the build's f = h f0 and a0.
Through a `_warped` entry point a = 0 is held to the plain model's bar only: DESIGN.md §9.8 promises equal bits at
`cep_warp == 0` for the host functions, which then call the plain entry points ("At `cep_warp == 0` nothing changes: the
host calls the Context methods that existed before"); the warped kernels take their cosine through the half-angle map at
any a, so their bits are their own.

The breakdown of the factorisation (a pivot that is not > 0: a NaN row) is reached through the raw entry point only,
with lam = 1e-300 and one node at 1e-300 Hz.  model_cepstrum() cannot reach it: it refuses lam < 1e-6, and with
lam >= 1e-6 the matrix is positive definite."""
import numpy as np
import pytest

import cepstrum_direct_cases as C
from conftest import record_measurement

pytestmark = pytest.mark.gpu

FILL = 7.0


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd.functions import _ctx
    return _ctx(0)


@pytest.fixture(scope="module", autouse=True)
def _quiet():
    with np.errstate(all="ignore"):
        yield


class Bars:
    """The comparisons of one test against their bars: every case is measured, then all of them must hold.  `worst`
    keeps, per group, the comparison with the largest error in units of its yardstick."""

    def __init__(self):
        self.missed, self.worst = [], {}

    def hold(self, group, name, err, dev):
        assert dev > 0, name
        if not err <= 100 * dev:
            self.missed.append("%s %s: gpu err %.3g > 100 x model dev %.3g" % (group, name, err, dev))
        if group not in self.worst or err / dev > self.worst[group][0]:
            self.worst[group] = (err / dev, dev, err, name)

    def check(self, record):
        for group, (ratio, dev, err, name) in sorted(self.worst.items()):
            print("cepstrum direct %s %s: worst %.3g x its yardstick (model dev %.3g, gpu err %.3g) at %s"
                  % (record, group, ratio, dev, err, name))
        record_measurement("cepstrum_direct_" + record,
                           **{g: dict(ratio=r, model_dev=d, gpu_err=e, case=nm) for g, (r, d, e, nm) in self.worst.items()})
        assert not self.missed, self.missed


def _t(ctx, a, dtype=np.float64):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=ctx.device)


def _full(ctx, shape, value):
    import torch
    return torch.full(shape, value, dtype=torch.float64, device=ctx.device)


def _group(ctx, alpha, warp):
    kw = {}
    if alpha is not None:
        kw["alpha"] = _t(ctx, alpha)
    if warp is not None:
        kw["warp"] = (_t(ctx, warp[0]), _t(ctx, warp[1]), len(warp[0]))
    return kw


def _fit(ctx, rec, fs, P, lam, a, guard=0):
    """The rows of one launch; `guard` more rows follow the output and must keep their fill."""
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    out = _full(ctx, (n + guard, P + 1), FILL)
    if a is None:
        ctx.model_cepstrum(_t(ctx, rec), n, K, float(fs), P, lam, out)
    else:
        ctx.model_cepstrum_warped(_t(ctx, rec), n, K, float(fs), P, lam, out, a)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.all(got[n:] == FILL)
    return got[:n]


def _read(ctx, phase, C_rows, fs, freqs, a, alpha=None, warp=None):
    n, P, F = C_rows.shape[0], C_rows.shape[1] - 1, len(freqs)
    out = _full(ctx, (n, F), FILL)
    name = ("cepstrum_phase" if phase else "cepstrum_envelope") + ("" if a is None else "_warped")
    args = (_t(ctx, C_rows), n, P, float(fs), _t(ctx, freqs), F, out) + (() if a is None else (a,))
    getattr(ctx, name)(*args, **_group(ctx, alpha, warp))
    ctx.sync()
    return out.cpu().numpy()


def _amp(ctx, rec, fs, beta, C_rows, a, alpha=None, warp=None):
    n, K, P = rec.shape[0], (rec.shape[1] - 1) // 3, C_rows.shape[1] - 1
    amp = _full(ctx, (n, K), -1.0)
    name = "modify_amp_cepstrum" + ("" if a is None else "_warped")
    args = (_t(ctx, rec), n, K, float(fs), _t(ctx, beta), _t(ctx, C_rows), P, amp) + (() if a is None else (a,))
    getattr(ctx, name)(*args, **_group(ctx, alpha, warp))
    ctx.sync()
    return amp.cpu().numpy()


def _build(ctx, case, C_rows, Kmax, Kcap, zero_phase, a):
    n, P = len(case["f0"]), C_rows.shape[1] - 1
    rec = _full(ctx, (n, 3 * Kmax + 1), np.nan)
    args = (_t(ctx, case["f0"]), _t(ctx, case["theta"]), _t(ctx, case["voiced"], np.uint8), _t(ctx, C_rows), P,
            _t(ctx, case["a0"]), n, case["fs"], Kmax, Kcap, zero_phase, rec)
    if a is None:
        ctx.model_build(*args)
    else:
        ctx.model_build_warped(*args, a)
    ctx.sync()
    return rec.cpu().numpy()


# ---- 1. the fit
def _hold_fit(bars, group, names, got, m):
    empty = m["empty"]
    assert np.all(np.isneginf(got[empty, 0])) and np.all(got[empty, 1:] == 0), group       # exactly (-inf, 0, .., 0)
    assert np.all(np.isfinite(got[~empty])), group
    for i in np.flatnonzero(~empty):
        bars.hold(group, names[i], float(np.abs(got[i] - m["c"][i]).max()), m["dev_case"])


@pytest.mark.parametrize("P", C.FIT_P)
@pytest.mark.parametrize("K", C.FIT_K)
def test_fit_cases(ctx, K, P):
    """Every pattern of the table as the instants of one launch per (lam, axis); the launch in reverse order and the
    repeated instant give the same bits."""
    bars = Bars()
    rec, names = C.fit_records(K), C.fit_patterns(K)
    assert len(names) % C.CEP_WAVES != 0
    for a in C.AXES:
        for lam in C.FIT_LAMS:
            m = C.fit_models(K, P, lam, a)
            got = _fit(ctx, rec, C.FS, P, lam, a, guard=2)
            assert got.shape == (len(names), P + 1)
            _hold_fit(bars, "%s_lam%g" % (C.axis_name(a), lam), names, got, m)
            assert np.array_equal(got[names.index("full_again")], got[0]), (K, P, lam, a)
            assert np.array_equal(_fit(ctx, rec[::-1], C.FS, P, lam, a)[::-1], got, equal_nan=True), (K, P, lam, a)
    for lam in C.FIT_LAMS:      # a = 0 through the warped entry point: the plain model's bar
        _hold_fit(bars, "warped_entry_a0_lam%g" % lam, names, _fit(ctx, rec, C.FS, P, lam, 0.0),
                  C.fit_models(K, P, lam, None))
    bars.check("fit_K%d_P%d" % (K, P))


@pytest.mark.parametrize("count", C.FIT_COUNTS)
def test_fit_of_the_first_instants_is_the_first_of_the_fit(ctx, count):
    """No_ti = 1, 4, 5 around the four waves of a block: the model's bar, the bits of the whole launch, and guard rows
    after the last instant untouched."""
    bars = Bars()
    for K, P in ((65, 63), (129, 1), (2, 32)):
        rec, names = C.fit_records(K), C.fit_patterns(K)
        for a in C.AXES:
            for lam in (1e-6, 1.0):
                got = _fit(ctx, rec[:count], C.FS, P, lam, a, guard=3)
                m = C.fit_models(K, P, lam, a)
                _hold_fit(bars, "K%d_P%d_%s_lam%g" % (K, P, C.axis_name(a), lam), names[:count], got,
                          dict({k: v[:count] for k, v in m.items() if k != "dev_case"}, dev_case=float(m["dev"][:count].max())))
                assert np.array_equal(got, _fit(ctx, rec, C.FS, P, lam, a)[:count]), (K, P, a, lam)
    bars.check("fit_count%d" % count)


# ---- 2. the LDS ceiling
@pytest.mark.parametrize("K,P", C.LDS_ACCEPTED, ids=lambda v: str(v))
def test_fit_at_the_lds_ceiling(ctx, K, P):
    """The largest Kmax the launch accepts: 160 KiB of dynamic LDS, fitted and compared like any other case."""
    assert C.fit_lds_bytes(K, P) == C.CEPSTRUM_LDS_MAX
    bars = Bars()
    rec = C.lds_records(K)
    for a in C.AXES:
        for lam in (1e-6, 5e-4):
            m = C.fit_models_of(("lds", K), rec, C.FS, P, lam, a)
            _hold_fit(bars, "%s_lam%g" % (C.axis_name(a), lam), ["full", "holes"], _fit(ctx, rec, C.FS, P, lam, a, guard=1), m)
    bars.check("fit_lds_K%d_P%d" % (K, P))


@pytest.mark.parametrize("K,P", C.LDS_REFUSED, ids=lambda v: str(v))
def test_fit_past_the_lds_ceiling_is_refused_and_launches_nothing(ctx, K, P):
    assert C.fit_lds_bytes(K, P) > C.CEPSTRUM_LDS_MAX >= C.fit_lds_bytes(K - 1, P)
    rec = _t(ctx, np.ones((2, 3 * K + 1)))
    out = _full(ctx, (2, P + 1), FILL)
    with pytest.raises(RuntimeError, match="error -1"):
        ctx.model_cepstrum(rec, 2, K, C.FS, P, 5e-4, out)
    with pytest.raises(RuntimeError, match="error -1"):
        ctx.model_cepstrum_warped(rec, 2, K, C.FS, P, 5e-4, out, 0.42)
    ctx.sync()
    assert bool((out == FILL).all())


# ---- 3. the breakdown
@pytest.mark.parametrize("P,a", C.BREAK_CASES, ids=lambda v: str(v))
def test_fit_breakdown_gives_a_nan_row_and_leaves_the_other_waves_alone(ctx, P, a):
    """Raw entry only (see the module docstring).  The bad instant in each of the four wave positions of the first
    block: its row is NaN in all P + 1 entries; the eight other rows, in its block and in the next, are finite and
    bit-equal to the same rows fitted in a call of their own."""
    good, bad = C.breakdown_records()
    assert C.first_pivots(bad, C.FS, C.BREAK_LAM, a) == (1.0, 2.0, 4.0, 0.0)
    alone = np.concatenate([_fit(ctx, good[i:i + 1], C.FS, P, C.BREAK_LAM, a) for i in range(len(good))])
    assert alone.shape == (8, P + 1) and np.all(np.isfinite(alone))
    assert np.all(np.isnan(_fit(ctx, bad[None, :], C.FS, P, C.BREAK_LAM, a)))
    for pos in range(C.CEP_WAVES):
        rec = np.concatenate((good[:pos], bad[None, :], good[pos:]))
        got = _fit(ctx, rec, C.FS, P, C.BREAK_LAM, a, guard=1)
        assert np.all(np.isnan(got[pos])), pos
        assert np.array_equal(np.delete(got, pos, axis=0), alone), pos


# ---- 4. the grid readouts
def _hold_grid(bars, group, name, C_rows, q, env, ph, m):
    """The bars and the exact parts of one envelope and one phase call; q [n, F] is the read frequency."""
    empty = m["empty"]
    assert env.shape == ph.shape == m["env"].shape
    assert np.all(np.isneginf(env[empty])) and np.all(ph[empty] == 0), name
    assert np.all(np.isfinite(env[~empty])) and np.all(np.isfinite(ph[~empty])), name
    for i in np.flatnonzero(~empty):     # the hold: every read frequency >= fs/2 gives the bits of fs/2
        past = q[i] >= C.FS / 2
        if past.any():
            assert len(np.unique(env[i, past])) == 1 and len(np.unique(ph[i, past])) == 1, (name, i)
    bars.hold(group + "_envelope", name, float(np.abs(env[~empty] - m["env"][~empty]).max()), m["dev_env"])
    bars.hold(group + "_phase", name, float(np.abs(C.wrapped(ph[~empty] - m["ph"][~empty])).max()), m["dev_ph"])


@pytest.mark.parametrize("n,F,P", C.grid_shapes())
def test_grid_cases(ctx, n, F, P):
    bars = Bars()
    freqs = C.grid_freqs(F, n)
    assert len(freqs) == F and C.FS / 2 in freqs
    at = int(np.flatnonzero(freqs == C.FS / 2)[0])
    for a in C.AXES:
        rows = C.grid_rows(n, P, a)
        got = {}
        for mode in C.GRID_MODES:
            alpha, warp = C.grid_mode(mode, n)
            q = C.CR.read_frequency(freqs, n, alpha, warp)
            env, ph = (_read(ctx, phase, rows, C.FS, freqs, a, alpha, warp) for phase in (False, True))
            got[mode] = (env, ph)
            _hold_grid(bars, C.axis_name(a), mode, rows, q, env, ph, C.grid_models(n, F, P, a, mode))
            if mode == "none":       # every grid point >= fs/2 is the value at fs/2
                past = freqs >= C.FS / 2
                assert past.sum() >= (1 if F == 1 else 3)
                for x in (env, ph):
                    assert np.array_equal(x[:, past], np.repeat(x[:, at:at + 1], past.sum(), axis=1)), (a, mode)
        plain = got["none"]
        for x, y in zip(got["alpha1"], plain):
            assert np.array_equal(x, y), a
        unit = C.grid_mode("alpha_rows", n)[0] == 1.0
        ident = np.arange(n) == n // 3 if n > 1 else np.zeros(1, dtype=bool)
        assert n < 3 or (unit.any() and not unit.all())
        for mode, same in [("alpha_rows", unit)] + [("map_B%d" % B, ident) for B in C.GRID_B]:
            for x, y in zip(got[mode], plain):
                assert np.array_equal(x[same], y[same]), (a, mode)
                live = ~same & ~np.isneginf(rows[:, 0])
                assert F == 1 or not live.any() or not np.array_equal(x[live], y[live]), (a, mode)   # the mode acts
        if a is None:     # a = 0 through the warped entry points: the plain model's bar
            m = C.grid_models(n, F, P, None, "none")
            env, ph = (_read(ctx, phase, rows, C.FS, freqs, 0.0) for phase in (False, True))
            _hold_grid(bars, "warped_entry_a0", "none", rows, np.broadcast_to(freqs, (n, F)), env, ph, m)
    bars.check("grid_n%d_F%d_P%d" % (n, F, P))


@pytest.mark.parametrize("P", [1, 63])
def test_grid_rows_alone_and_slices_are_the_rows_of_the_whole(ctx, P):
    """Each of the nine rows in a call of its own, and the first and the last 1, 3, 4, 5 rows, against the call of nine:
    plain, a contour of alpha and a map of 16 breakpoints, envelope and phase, bit for bit."""
    n, F = 9, 65
    freqs = C.grid_freqs(F, n)
    for a in C.AXES:
        rows = C.grid_rows(n, P, a)
        for mode in ("none", "alpha_rows", "map_B16"):
            alpha, warp = C.grid_mode(mode, n)
            for phase in (False, True):
                whole = _read(ctx, phase, rows, C.FS, freqs, a, alpha, warp)
                parts = [(i, i + 1) for i in range(n)] + [s for c in (3, 4, 5) for s in ((0, c), (n - c, n))]
                for lo, hi in parts:
                    part = _read(ctx, phase, rows[lo:hi], C.FS, freqs, a, None if alpha is None else alpha[lo:hi],
                                 None if warp is None else (warp[0], warp[1][lo:hi]))
                    assert np.array_equal(part, whole[lo:hi]), (P, a, mode, phase, lo, hi)


# ---- 5. the amplitude readout
@pytest.mark.parametrize("K", C.AMP_K)
@pytest.mark.parametrize("n", C.AMP_COUNTS)
def test_amplitude_cases(ctx, n, K):
    bars = Bars()
    c = C.amp_case(n, K)
    rec, beta = c["rec"], c["beta"]
    act = C.active_slots(rec)
    for a in C.AXES:
        for P in C.AMP_P:
            rows = C.amp_rows(n, P, a)
            live = ~np.isneginf(rows[:, 0])
            plain = None
            for mode in C.AMP_MODES:
                alpha, warp = C.grid_mode(mode, n)
                m = C.amp_models(n, K, P, a, mode)
                got = _amp(ctx, rec, C.FS, beta, rows, a, alpha, warp)
                name = "P%d_%s" % (P, mode)
                assert got.shape == (n, K) and not np.any(got == -1.0), name          # every cell is written
                assert np.array_equal(got == 0, m["zero"]), name                      # inactive, muted, the empty rows
                assert np.all(got[~act] == 0) and np.all(got[~live] == 0), name
                for i in range(n):
                    if c["edge"][i] >= 0:
                        assert got[i, c["edge"][i]] == 0, (name, i)                   # beta f == fs/2 exactly: muted
                    if c["below"][i] >= 0 and live[i]:
                        assert got[i, c["below"][i]] > 0, (name, i)                   # its lower neighbour is not
                assert (c["edge"] >= 0).any() and ((c["below"] >= 0) & live).any()
                bars.hold(C.axis_name(a), name, C.rel_error(got, m["amp"]), m["dev"])
                if mode == "none":
                    plain = got
                else:
                    same = (alpha == 1.0) if alpha is not None else (np.arange(n) == n // 3)
                    assert same.any() and np.array_equal(got[same], plain[same]), name
            for i in range(n):      # an instant alone (No_ti >= 4: among copies of itself) gives the same bits
                alone = _amp(ctx, np.repeat(rec[i:i + 1], 4, axis=0), C.FS, beta[:4], np.repeat(rows[i:i + 1], 4, axis=0), a)
                assert np.array_equal(alone, np.repeat(plain[i:i + 1], 4, axis=0)), (a, P, i)
        if a is None:
            m = C.amp_models(n, K, 63, None, "none")
            got = _amp(ctx, rec, C.FS, beta, C.amp_rows(n, 63, None), 0.0)
            bars.hold("warped_entry_a0", "P63_none", C.rel_error(got, m["amp"]), m["dev"])
    bars.check("amplitudes_n%d_K%d" % (n, K))


# ---- 6. the build
@pytest.mark.parametrize("Kmax", C.BUILD_K)
@pytest.mark.parametrize("n", C.BUILD_N)
def test_build_cases(ctx, n, Kmax):
    bars = Bars()
    case = C.build_case(n, Kmax)
    kinds = C.INSTANTS[:n]
    for a in C.AXES:
        for P in C.BUILD_P:
            rows = C.build_rows(n, Kmax, P, a)
            for zero_phase in (0, 1):
                mm = C.build_models(n, Kmax, P, a, zero_phase)
                m = mm["m"]
                rec = _build(ctx, case, rows, Kmax, Kmax, zero_phase, a)
                name = "P%d_%s" % (P, "zero" if zero_phase else "min")
                assert rec.shape == (n, 3 * Kmax + 1) and not np.isnan(rec).any(), name      # every cell is written
                assert np.array_equal(_build(ctx, case, rows, Kmax, C.KCAP, zero_phase, a), rec), name
                am, fm, ph = rec[:, :Kmax], rec[:, Kmax:2 * Kmax], rec[:, 2 * Kmax:3 * Kmax]
                assert np.array_equal(rec[:, 3 * Kmax], case["a0"]), name
                assert np.array_equal(am != 0, m["active"]), name
                assert np.array_equal(fm, m["fm"]), name                                # h f0, the float64 product
                assert np.all(ph[~m["active"]] == 0), name
                for i, kind in enumerate(kinds):
                    if kind in ("unvoiced", "empty", "underflow"):
                        assert not rec[i, :3 * Kmax].any(), (name, kind)
                    elif kind == "nyquist":
                        e = case["edge_h"] - 1
                        assert not am[i, e:].any() and not fm[i, e:].any() and not ph[i, e:].any(), name
                        assert e == 0 or am[i, e - 1] > 0, name
                    else:
                        assert np.all(am[i] > 0), (name, kind)
                bars.hold(C.axis_name(a) + "_am", name, C.rel_error(am, m["am"]), mm["dev_am"])
                bars.hold(C.axis_name(a) + "_ph", name, float(np.abs(C.wrapped(ph - m["ph"])).max()), mm["dev_ph"])
                for i in range(n - 1):      # two instants in a call of their own: the same bits
                    sub = {k: (v[i:i + 2] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
                    assert np.array_equal(_build(ctx, sub, rows[i:i + 2], Kmax, Kmax, zero_phase, a), rec[i:i + 2]), (name, i)
        if a is None:
            mm = C.build_models(n, Kmax, 63, None, 0)
            rec = _build(ctx, case, C.build_rows(n, Kmax, 63, None), Kmax, Kmax, 0, 0.0)
            bars.hold("warped_entry_a0_am", "P63_min", C.rel_error(rec[:, :Kmax], mm["m"]["am"]), mm["dev_am"])
            bars.hold("warped_entry_a0_ph", "P63_min",
                      float(np.abs(C.wrapped(rec[:, 2 * Kmax:3 * Kmax] - mm["m"]["ph"])).max()), mm["dev_ph"])
    bars.check("build_n%d_K%d" % (n, Kmax))
