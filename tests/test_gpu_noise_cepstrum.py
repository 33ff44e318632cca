"""The noise model to and from cepstral rows on the MI355X (noise_cepstrum -> eaqhm_noise_cepstrum,
noise_from_cepstrum -> eaqhm_noise_from_cepstrum, noise_alignment_index) against the NumPy model of DESIGN.md §10.4
(tests/noise_cepstrum_ref.py).

Bars (§10's rule).  The kernels sum in another order than the model, read cos(pi t / M) from cospi and call the
device's exp and log, so they are held to 100 x the largest difference between the model run in float64 and in
np.longdouble on the same input, computed when the test runs; both figures are recorded.  Frames whose stop stage
differs between the model's two precisions could be left out of the way back (at most 1 % of the non-silent frames);
on the smooth (r = 0.7) and sharp (r = 0.9) fixtures none is, which is asserted on the model alone.

Shapes.  LPC orders p in {1, 2, 18, 50, 63}, cepstral orders Q in {1, 2, p - 1, p, p + 1, 63}; frame counts one below
and one above the waves per block of both kernels (4 and 8) besides 1 and 37; silent frames first, last and in the
middle.  Every (p, Q) runs at 37 frames one way and at 9 frames the other way; every frame count runs at (18, 63) and
(63, 1): a frame's path through either kernel depends on (p, Q) alone, its place in the grid on the count alone.
What the bars came to on the MI355X is in DESIGN.md §10.4: the forward kernel at most 0.36 x the model's difference, the
way back at most 28 x, the bar being 100 x."""
import os

import numpy as np
import pytest

import noise_cepstrum_ref as R
import noise_warp_ref as W
from conftest import GOLDEN, record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
ORDERS = (1, 2, 18, 50, 63)
COUNTS = (1, 3, 5, 7, 9, 37)            # 4 and 8 waves per block: one below, one above; one frame; several blocks
FIXTURES = (("smooth", 0.7), ("sharp", 0.9))
EPS = np.finfo(np.float64).eps


def cepstral_orders(p):
    return sorted({q for q in (1, 2, p - 1, p, p + 1, 63) if 1 <= q <= 63})


def silent_frames(Nf):
    return sorted({0, Nf // 2, Nf - 1}) if Nf >= 3 else ()


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


@pytest.fixture(scope="module")
def forward():
    """{(fixture, p): (noise model of 37 frames, model rows at Q = 63 in float64, in longdouble)}; a lower Q is the
    prefix of the same rows."""
    out = {}
    for label, r in FIXTURES:
        for p in ORDERS:
            sigma, refl, _ = R.pole_frames(37, p, r, seed=1, silent=silent_frames(37))
            out[label, p] = (R.noise_model(sigma, refl), R.cepstrum(sigma, refl, 63), R.cepstrum(sigma, refl, 63, LD))
    return out


@pytest.fixture(scope="module")
def backward(forward):
    """{(fixture, p, Q): (rows float64[9, Q + 1], model (sigma, refl, stop) in float64, in longdouble)}: the first nine
    frames' model rows (silent first, in the middle and last), cut at Q, fitted at order p."""
    out = {}
    for label, _ in FIXTURES:
        for p in ORDERS:
            C = forward[label, p][1][:9].copy()
            C[[0, 4, 8]] = 0.0
            C[[0, 4, 8], 0] = -np.inf
            for Q in cepstral_orders(p):
                rows = np.ascontiguousarray(C[:, :Q + 1])
                out[label, p, Q] = (rows, R.from_cepstrum(rows, p), R.from_cepstrum(rows, p, LD))
    return out


def test_model_leaves_no_frame_out(backward):
    """The stop stage of every frame of both fixtures is the same in float64 and longdouble, and is 0."""
    for key, (rows, m64, mld) in backward.items():
        assert np.array_equal(m64[2], mld[2]) and not m64[2].any(), key


def test_noise_cepstrum_against_model(amd, forward):
    for (label, p), (nz, c64, cld) in forward.items():
        live = nz["sigma"] > 0
        for Q in cepstral_orders(p):
            got = amd.noise_cepstrum(nz, Q)
            assert got.shape == (37, Q + 1) and got.dtype == np.float64
            assert np.array_equal(np.isneginf(got[:, 0]), ~live) and np.all(got[~live, 1:] == 0), (label, p, Q)
            assert np.all(np.isfinite(got[live]))
            c0 = np.log(nz["sigma"][live])
            assert np.all(np.abs(got[live, 0] - c0) <= np.spacing(np.abs(c0))), (label, p, Q)
            dev = float(np.abs(c64[live, 1:Q + 1] - cld[live, 1:Q + 1]).max())
            err = float(np.abs(got[live, 1:] - c64[live, 1:Q + 1]).max())
            print("noise cepstrum %s p %d Q %d: model dev %.3g gpu err %.3g" % (label, p, Q, dev, err))
            record_measurement("noise_cepstrum_vs_numpy_%s_p%d_Q%d" % (label, p, Q), model_dev=dev, gpu_err=err)
            assert err <= 100 * dev, (label, p, Q, err, dev)
    assert np.array_equal(amd.noise_cepstrum(forward["smooth", 18][0]), amd.noise_cepstrum(forward["smooth", 18][0], 63))


def _head(nz, lo, hi):
    s, k = nz["sigma"][lo:hi], nz["refl"][lo:hi]
    return dict(nz, sigma=s, refl=k, length=(len(s) - 1) * nz["hop"] + 1)


def test_noise_cepstrum_at_every_frame_count(amd, forward):
    """A frame's row does not depend on how many frames the call has or where the frame sits in its block."""
    for p, Q in ((18, 63), (63, 1)):
        nz = forward["sharp", p][0]
        whole = amd.noise_cepstrum(nz, Q)
        for Nf in COUNTS:
            assert np.array_equal(amd.noise_cepstrum(_head(nz, 0, Nf), Q), whole[:Nf]), (p, Q, Nf)        # silent first
            assert np.array_equal(amd.noise_cepstrum(_head(nz, 37 - Nf, 37), Q), whole[37 - Nf:]), (p, Q, Nf)   # and last


def test_cepstrum_reads_as_the_noise_envelope(amd, forward):
    """2 cepstrum_envelope(noise_cepstrum(nz, 63)) against noise_envelope(nz) on the smooth fixture: the rounding bar of
    the two readouts plus the remainder of the cut, 2 p r^{Q+1} / ((Q + 1)(1 - r))."""
    r, Q = 0.7, 63
    for p in ORDERS:
        nz, c64, cld = forward["smooth", p]
        fs = nz["fs"]
        live = nz["sigma"] > 0
        f = np.linspace(0.0, fs / 2, 65)
        a = 2 * amd.cepstrum_envelope(amd.noise_cepstrum(nz, Q), fs, f)
        b = amd.noise_envelope(nz, fs, f)
        assert np.array_equal(np.isneginf(a), np.isneginf(b)) and np.array_equal(np.isneginf(a).all(axis=1), ~live)
        w = 2 * np.pi * f / fs
        dev = float(np.abs(W.envelope(nz["sigma"], nz["refl"], 1.0, f / fs)[live]
                           - W.envelope(nz["sigma"], nz["refl"], 1.0, f / fs, LD)[live]).max()
                    + 2 * np.abs(R.readout(c64[live], w) - R.readout(cld[live], w, LD)).max())
        rem = 2 * p * r ** (Q + 1) / ((Q + 1) * (1 - r))
        err = float(np.abs(a[live] - b[live]).max())
        print("noise cepstrum as envelope p %d: difference %.3g, rounding dev %.3g, remainder bound %.3g"
              % (p, err, dev, rem))
        record_measurement("noise_cepstrum_envelope_p%d" % p, difference=err, model_dev=dev, remainder_bound=rem)
        assert err <= 100 * dev + rem, (p, err, dev, rem)


def _compare_back(got_sigma, got_refl, m64, mld, what):
    """(dev_k, err_k, dev_s, err_s) of one call against the model; asserts the silent frames and the bars."""
    s64, k64, stop = m64
    sld, kld, stop_l = mld
    live = s64 > 0
    keep = stop == stop_l
    assert int(np.count_nonzero(~keep)) <= 0.01 * int(live.sum()), what
    assert np.array_equal(got_sigma == 0, ~live) and np.all(got_refl[~live] == 0), what
    smax = float(s64.max())
    dev_k = float(np.abs(k64[keep] - kld[keep]).max())
    dev_s = float(np.abs(s64[keep] - sld[keep]).max() / smax)
    err_k = float(np.abs(got_refl[keep] - k64[keep]).max())
    err_s = float(np.abs(got_sigma[keep] - s64[keep]).max() / smax)
    print("%s: k: model dev %.3g gpu err %.3g  sigma: model dev %.3g gpu err %.3g" % (what, dev_k, err_k, dev_s, err_s))
    record_measurement(what.replace(" ", "_"), model_dev_k=dev_k, gpu_err_k=err_k, model_dev_sigma=dev_s,
                       gpu_err_sigma=err_s, max_abs_k=float(np.abs(k64).max()))
    assert err_k <= 100 * dev_k, (what, err_k, dev_k)
    assert err_s <= 100 * dev_s, (what, err_s, dev_s)


def test_noise_from_cepstrum_against_model(amd, backward):
    from eaqhm_amd.model import check_noise_model
    for (label, p, Q), (rows, m64, mld) in backward.items():
        got = amd.noise_from_cepstrum(rows, 80, 16000, order=p)
        assert (got["hop"], got["order"], got["fs"], got["length"]) == (80, p, 16000.0, 8 * 80 + 1)
        assert got["sigma"].shape == (9,) and got["refl"].shape == (9, p)
        assert got["sigma"].dtype == got["refl"].dtype == np.float64
        check_noise_model(got)
        _compare_back(got["sigma"], got["refl"], m64, mld, "noise from cepstrum %s p %d Q %d" % (label, p, Q))


def test_noise_from_cepstrum_at_every_frame_count(amd, forward):
    for p, Q in ((18, 63), (63, 1)):
        rows = np.ascontiguousarray(forward["sharp", p][1][:, :Q + 1])
        whole = amd.noise_from_cepstrum(rows, 80, 16000, order=p)
        assert np.array_equal(whole["sigma"] == 0, np.isneginf(rows[:, 0]))
        for Nf in COUNTS:
            for lo in (0, 37 - Nf):
                got = amd.noise_from_cepstrum(rows[lo:lo + Nf], 80, 16000, order=p, length=(Nf - 1) * 80 + 7)
                assert got["length"] == (Nf - 1) * 80 + 7
                assert np.array_equal(got["sigma"], whole["sigma"][lo:lo + Nf]), (p, Q, Nf, lo)
                assert np.array_equal(got["refl"], whole["refl"][lo:lo + Nf]), (p, Q, Nf, lo)


def test_column_zero_only_sets_the_level(amd, backward):
    for key in (("smooth", 18, 63), ("sharp", 50, 51), ("sharp", 2, 1)):
        rows = backward[key][0]
        base = amd.noise_from_cepstrum(rows, 80, 16000, order=key[1])
        live = base["sigma"] > 0
        for d in (-3.0, 2.5):
            moved = rows.copy()
            moved[:, 0] += d                                                   # -inf stays -inf
            got = amd.noise_from_cepstrum(moved, 80, 16000, order=key[1])
            assert np.array_equal(got["refl"], base["refl"]), (key, d)
            assert np.array_equal(got["sigma"] == 0, ~live)
            rel = float(np.abs(got["sigma"][live] / (base["sigma"][live] * np.exp(d)) - 1).max())
            print("column 0 moved by %g on %s: sigma off e^d by %.3g relative" % (d, key, rel))
            assert rel <= 16 * EPS, (key, d, rel)


def test_guard_rows_and_empty_rows(amd, forward):
    """The Context methods on buffers with guard rows after the last frame: untouched at every frame count; empty rows
    give silent frames and silent frames empty rows."""
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    dev = c.device
    for p, Q in ((18, 63), (63, 1), (1, 2)):
        nz = forward["smooth", p][0]
        for Nf in COUNTS:
            sigma = torch.as_tensor(nz["sigma"][:Nf + 2].copy(), device=dev)       # two more frames than the call names
            refl = torch.as_tensor(nz["refl"][:Nf + 2].copy(), device=dev)
            ceps = torch.full((Nf + 2, Q + 1), 7.25, dtype=torch.float64, device=dev)
            c.noise_cepstrum(sigma, refl, Nf, p, Q, ceps)
            so = torch.full((Nf + 2,), 7.25, dtype=torch.float64, device=dev)
            ro = torch.full((Nf + 2, p), 7.25, dtype=torch.float64, device=dev)
            c.noise_from_cepstrum(ceps, Nf, Q, p, so, ro)
            c.sync()
            ceps, so, ro = ceps.cpu().numpy(), so.cpu().numpy(), ro.cpu().numpy()
            assert np.all(ceps[Nf:] == 7.25) and np.all(so[Nf:] == 7.25) and np.all(ro[Nf:] == 7.25), (p, Q, Nf)
            silent = nz["sigma"][:Nf] == 0
            assert np.array_equal(np.isneginf(ceps[:Nf, 0]), silent) and np.all(ceps[:Nf][silent, 1:] == 0)
            assert np.array_equal(so[:Nf] == 0, silent) and np.all(ro[:Nf][silent] == 0)
            assert np.all(so[:Nf][~silent] > 0) and np.all(np.abs(ro[:Nf]) < 1)


def test_round_trip(amd, forward):
    """frames -> rows (Q = 63) -> frames on the device against the model's round trip, within the rounding bar; the
    rebuilt model is a valid noise model and synthesises.  Recorded, no bar: the round trip's own error (the cut at Q
    and the grid, not the kernels) and, with the same seed, the rms difference of the two syntheses over the rms."""
    from eaqhm_amd.model import check_noise_model, noise_time_map
    for label, _ in FIXTURES:
        for p in (18, 50):
            nz, c64, cld = forward[label, p]
            rows = amd.noise_cepstrum(nz, 63)
            back = amd.noise_from_cepstrum(rows, nz["hop"], nz["fs"], order=p, length=nz["length"])
            check_noise_model(back)
            assert {k: back[k] for k in ("hop", "order", "fs", "length")} == \
                {k: nz[k] for k in ("hop", "order", "fs", "length")}
            _compare_back(back["sigma"], back["refl"], R.from_cepstrum(c64, p), R.from_cepstrum(cld, p, LD),
                          "noise round trip %s p %d" % (label, p))
            live = nz["sigma"] > 0
            err_k = float(np.abs(back["refl"][live] - nz["refl"][live]).max())
            err_s = float(np.abs(back["sigma"][live] / nz["sigma"][live] - 1).max())
            L = nz["length"]
            tau = noise_time_map(nz["hop"], L, 1.0)
            y0 = amd.eaQHMNoiseSynthesis(nz, tau, L, seed=5)
            y1 = amd.eaQHMNoiseSynthesis(back, tau, L, seed=5)
            assert y1.shape == (L,) and np.all(np.isfinite(y1)) and np.any(y1 != 0)
            rel = float(np.sqrt(np.mean((y1 - y0) ** 2) / np.mean(y0 ** 2)))
            print("noise round trip %s p %d: refl off by %.3g, sigma by %.3g relative, synthesis rms difference %.3g of "
                  "the rms" % (label, p, err_k, err_s, rel))
            record_measurement("noise_round_trip_%s_p%d" % (label, p), refl_error=err_k, sigma_rel_error=err_s,
                               synthesis_rms_ratio=rel)


def _arrays_model(n, step, K=2):
    ti = np.arange(n) * step
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
                frange=np.tile([200.0, 400.0], (n, 1))[:, :K], pk=np.zeros((n, K)))


def _rows_at(X, j):
    """warp_rows in the dtype of X (warp_rows itself returns float64): the same blend and the same rule for empty rows."""
    lo = np.floor(j).astype(np.int64)
    hi = np.minimum(lo + 1, len(X) - 1)
    u = j - lo
    w = u.astype(X.dtype)[:, None]
    with np.errstate(invalid="ignore"):
        out = (1 - w) * X[lo] + w * X[hi]
    out[u == 0] = X[lo[u == 0]]
    empty = np.isneginf(X[:, 0])
    copy = (u != 0) & (empty[lo] | empty[hi])
    out[copy] = X[np.where(u > 0.5, hi, lo)[copy]]
    return out


def test_transplant_follows_the_alignment(amd):
    """B's noise at A's timing: two synthetic models at hops 80 and 96, instants 15 and 20 samples apart, a hand-made
    monotone idx; the device's result against the NumPy composition of noise_alignment_index, warp_rows and the model."""
    p, Q = 18, 40
    sA, kA, _ = R.pole_frames(31, p, 0.7, seed=21, silent=(3,))
    sB, kB, _ = R.pole_frames(23, p, 0.9, seed=22, silent=(0, 11, 12, 22))
    nzA, nzB = R.noise_model(sA, kA, hop=80), R.noise_model(sB, kB, hop=96)
    detA, detB = _arrays_model(161, 15), _arrays_model(106, 20)      # 0..2400 and 0..2100: the frames lie inside
    x = np.arange(161) / 160.0
    idx = 105 * (0.6 * x + 0.4 * x ** 3)                               # monotone, (0, 0) to (160, 105), uneven tempo
    j = amd.noise_alignment_index(idx, detA, nzA, detB, nzB)
    assert j.shape == (31,) and np.all(np.diff(j) >= 0) and j[0] == 0 and j[-1] <= 22
    rows = amd.warp_rows(amd.noise_cepstrum(nzB, Q), j)
    got = amd.noise_from_cepstrum(rows, nzA["hop"], nzA["fs"], order=p, length=nzA["length"])
    assert (got["hop"], got["length"], got["order"], got["fs"]) == (80, nzA["length"], p, 16000.0)
    assert len(got["sigma"]) == 31
    assert np.array_equal(_rows_at(R.cepstrum(sB, kB, Q), j), amd.warp_rows(R.cepstrum(sB, kB, Q), j))
    want = [R.from_cepstrum(_rows_at(R.cepstrum(sB, kB, Q, dt), j), p, dt) for dt in (np.float64, LD)]
    assert 0 < int((want[0][0] == 0).sum()) < 31                       # B's silence arrives in A's frames
    _compare_back(got["sigma"], got["refl"], want[0], want[1], "noise transplant")
    # the transplant is B's, not A's: its frames differ from A's own round trip
    own = amd.noise_from_cepstrum(amd.noise_cepstrum(nzA, Q), 80, 16000.0, order=p, length=nzA["length"])
    assert np.abs(got["refl"] - own["refl"]).max() > 1e-2


def test_entry_points_reject_bad_shapes(amd):
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=c.device)

    Nf, p, Q = 5, 4, 6
    sigma, refl, ceps, so, ro = z(Nf) + 0.1, z(Nf, p), z(Nf, Q + 1), z(Nf), z(Nf, p)
    c.noise_cepstrum(sigma, refl, Nf, p, Q, ceps)                    # the good calls: a white frame
    c.noise_from_cepstrum(ceps, Nf, Q, p, so, ro)
    c.sync()
    assert torch.all(ceps[:, 1:] == 0) and float(ro.abs().max()) <= 1e-14       # the lag sums of a flat spectrum: rounding
    assert float((so - 0.1).abs().max()) <= 4 * EPS
    for bad in (0, 64, -1):
        for args in ((sigma, refl, Nf, bad, Q, ceps), (sigma, refl, Nf, p, bad, ceps)):
            with pytest.raises(RuntimeError, match="error -1"):
                c.noise_cepstrum(*args)
        for args in ((ceps, Nf, bad, p, so, ro), (ceps, Nf, Q, bad, so, ro)):
            with pytest.raises(RuntimeError, match="error -1"):
                c.noise_from_cepstrum(*args)
    for bad_nf in (0, -3):
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_cepstrum(sigma, refl, bad_nf, p, Q, ceps)
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_from_cepstrum(ceps, bad_nf, Q, p, so, ro)
    args = [sigma, refl, Nf, p, Q, ceps]
    for i in (0, 1, 5):
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_cepstrum(*[None if j == i else a for j, a in enumerate(args)])
    args = [ceps, Nf, Q, p, so, ro]
    for i in (0, 4, 5):
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_from_cepstrum(*[None if j == i else a for j, a in enumerate(args)])
    assert c.abi_version == 6


def test_cli_noise_cepstrum_and_noise_from(amd, tmp_path):
    import shutil
    from scipy.io import wavfile
    from eaqhm_amd import cli
    wav, other = str(tmp_path / "SA19.WAV"), str(tmp_path / "OTHER.WAV")
    shutil.copy(os.path.join(GOLDEN, "SA19.WAV"), wav)
    fs, x = wavfile.read(wav)
    wavfile.write(other, fs, x[3200:])                               # the same speech 0.2 s early: another length
    base = [wav, "--gender", "female", "--max-adpt", "1", "--noise", "--noise-seed", "3"]
    assert cli.main(base + ["--noise-cepstrum", "40"]) == 0
    _, through = wavfile.read(str(tmp_path / "SA19_resynthesis.wav"))
    assert through.shape == x.shape and np.all(np.isfinite(through)) and np.any(through != 0)
    assert cli.main(base + ["--noise-from", other]) == 0
    fs2, y = wavfile.read(str(tmp_path / "SA19_modified.wav"))
    assert fs2 == fs and y.shape == x.shape and np.all(np.isfinite(y)) and not np.array_equal(y, through)
