"""The time alignment without a GPU: the NumPy model of DESIGN.md §9.6 (tests/model_align_ref.py) against brute-force
enumeration, the band helpers of the model and of the host, alignment_index / warp_rows / alignment_time_scale on
hand-computed cases, every ValueError of the host layer, the CLI flags and the binding."""
import itertools
import os
import re

import numpy as np
import pytest

import model_align_ref as AR
from conftest import ROOT

NEW_SYMBOLS = {"eaqhm_cepstrum_cost": 10, "eaqhm_dtw": 9}


# ---- the model against enumeration
@pytest.mark.parametrize("nA,nB", list(itertools.product(range(1, 6), repeat=2)))
def test_reference_dp_equals_enumeration(nA, nB):
    """Every table up to 5 x 5, full band and minimal band, integer costs 0..2 (many ties, exact sums) and all-equal
    costs: the cost is the cheapest path's, and the path is the one the tie rule picks among the cheapest."""
    rng = np.random.default_rng(100 * nA + nB)
    tables = [rng.integers(0, 3, size=(nA, nB)).astype(np.float64) for _ in range(6)]
    tables += [np.zeros((nA, nB)), np.ones((nA, nB))]
    for r in sorted({AR.full_radius(nA, nB), AR.min_radius(nA, nB)}):
        for d in tables:
            path, total, D, ptr = AR.align(d, r)
            want, best = AR.brute_force(d, r)
            assert total == best, (nA, nB, r, d)
            assert np.array_equal(path, want), (nA, nB, r, d, path, want)
            assert AR.path_is_valid(path, nA, nB, r)
            assert ptr[0, r] == 3 and D[0, r] == d[0, 0]


@pytest.mark.parametrize("nA,nB", [(4, 4), (5, 3), (3, 5), (5, 5), (1, 4), (4, 1)])
def test_equal_costs_take_the_diagonal_while_they_can(nA, nB):
    path = AR.align(np.ones((nA, nB)))[0]
    k = min(nA, nB)
    assert np.array_equal(path[-k:], np.stack((np.arange(nA - k, nA), np.arange(nB - k, nB)), axis=1))
    # read from the end the diagonal comes first; the rest is one straight run along an edge
    rest = path[:-k + 1] if k > 1 else path
    assert np.all(rest[:, 0] == 0) or np.all(rest[:, 1] == 0)
    assert len(path) == max(nA, nB)


# ---- the band
def test_centres_at_70000_rows_are_exact():
    n = 70000
    c = AR.centres(n, n)
    assert c.dtype == np.int64 and np.array_equal(c, np.arange(n))          # (2 i (n-1) + (n-1)) // (2 (n-1)) = i
    assert 2 * (n - 1) * (n - 1) > 2 ** 32                                  # the product a 32-bit index would wrap
    from eaqhm_amd.model import band_centres
    assert np.array_equal(band_centres(n, n), c)
    for nA, nB in ((70001, 69997), (7, 130), (130, 7), (1, 9), (9, 1), (2, 2)):
        c = AR.centres(nA, nB)
        assert np.array_equal(band_centres(nA, nB), c), (nA, nB)
        assert c[0] == 0 and c[-1] == (nB - 1 if nA > 1 else 0) and np.all(np.diff(c) >= 0)
        want = [int(np.floor((i * (nB - 1)) / (nA - 1) + 0.5)) if nA > 1 else 0 for i in (0, nA // 3, nA - 1)]
        assert [int(c[i]) for i in (0, nA // 3, nA - 1)] == want


def test_minimal_radius():
    from eaqhm_amd.model import band_min_radius
    cases = {(1, 1): 0, (1, 7): 6, (7, 1): 0, (2, 2): 1, (5, 5): 1, (3, 5): 2, (5, 3): 1, (70, 130): 2, (130, 70): 1,
             (2, 10): 9, (4, 11): 4}
    for (nA, nB), want in cases.items():
        assert AR.min_radius(nA, nB) == want == band_min_radius(nA, nB), (nA, nB)
    for nA, nB in itertools.product(range(1, 7), repeat=2):          # a path exists at r_min: the rule is sufficient
        assert len(AR.all_paths(nA, nB, AR.min_radius(nA, nB))) >= 1   # (not always necessary: 2 x 2 has its diagonal)


@pytest.mark.parametrize("nA,nB,r", [(7, 13, 2), (13, 7, 1), (13, 7, 4), (1, 5, 4), (5, 1, 0), (6, 6, 5), (6, 6, 1)])
def test_dense_band_dense_round_trip(nA, nB, r):
    from eaqhm_amd.model import dense_to_band
    d = np.arange(nA * nB, dtype=np.float64).reshape(nA, nB) + 1.0
    band = AR.to_band(d, r)
    assert band.shape == (nA, 2 * r + 1)
    assert np.array_equal(dense_to_band(d, r), band)
    inside = AR.in_band(nA, nB, r)
    assert np.all(np.isposinf(band[~inside])) and np.all(np.isfinite(band[inside]))
    back = AR.to_dense(band, nB)
    c = AR.centres(nA, nB)
    member = np.abs(np.arange(nB)[None, :] - c[:, None]) <= r
    assert np.array_equal(back[member], d[member]) and np.all(np.isposinf(back[~member]))
    assert inside.sum() == member.sum()


# ---- the cost
def test_reference_cost_rules():
    rng = np.random.default_rng(2)
    A, B = rng.standard_normal((5, 4)), rng.standard_normal((6, 4))
    B[2] = A[1]
    for M in (A, B):
        M[3] = 0.0
        M[3, 0] = -np.inf
    A[0] = 0.0
    A[0, 0] = -np.inf
    for w in (0.0, 1.0):
        d, dl = AR.cost(A, B, w, 4.0), AR.cost(A, B, w, 4.0, np.longdouble)
        assert d[1, 2] == 0 and d[3, 3] == 0 and d[0, 3] == 0
        assert np.all(d[0, [0, 1, 2, 4, 5]] == 4.0) and np.all(d[[1, 2, 4], 3] == 4.0)
        assert abs(d[2, 1] - (w * (A[2, 0] - B[1, 0]) ** 2 + 2 * ((A[2, 1:] - B[1, 1:]) ** 2).sum())) <= 1e-14
        assert np.abs(d - dl.astype(np.float64)).max() <= 8 * 2.0 ** -52 * d.max()
    assert AR.cost(A, B, 0.0, 0.5)[0, 0] == 0.5


# ---- the host functions
def test_alignment_index_by_hand():
    from eaqhm_amd import alignment_index
    path = np.array([(0, 0), (1, 1), (1, 2), (1, 3), (2, 4), (3, 4), (4, 5), (4, 6)])
    idx = alignment_index(path, 5)
    assert idx.dtype == np.float64 and np.array_equal(idx, [0.0, 2.0, 4.0, 4.0, 5.5])
    assert np.array_equal(idx, AR.alignment_index(path, 5))
    diag = np.stack((np.arange(6), np.arange(6)), axis=1)
    assert np.array_equal(alignment_index(diag, 6), np.arange(6.0))
    for bad, n in ((path, 6), (path, 4), (path[:, :1], 5), (path.astype(float), 5), (path[None], 5), (-path, 5),
                   (path[:0], 5), (path, 0), (path, 2.5)):
        with pytest.raises(ValueError):
            alignment_index(bad, n)


def test_alignment_time_scale_by_hand():
    from eaqhm_amd import alignment_time_scale
    diag = np.stack((np.arange(6), np.arange(6)), axis=1)
    assert np.array_equal(alignment_time_scale(diag, 6), np.ones(6))
    assert np.array_equal(alignment_time_scale(diag, 6, step_ratio=2.0), np.full(6, 2.0))
    # B twice as slow: every instant of A held over two of B; idx = 0.5, 2.5, 4.5, 6.5
    slow = np.array([(i, 2 * i + k) for i in range(4) for k in (0, 1)])
    assert np.array_equal(alignment_time_scale(slow, 4), np.full(4, 2.0))
    # a hold of 9 instants of B on one of A: the gradient 5 is clipped to 4; the skipped run is clipped to 0.25
    hold = np.array([(0, 0)] + [(1, j) for j in range(1, 10)] + [(2, 10), (3, 10), (4, 10), (5, 10), (6, 11)])
    ts = alignment_time_scale(hold, 7)
    idx = np.array([0.0, 5.0, 10.0, 10.0, 10.0, 10.0, 11.0])
    assert np.array_equal(ts, np.clip(np.gradient(idx), 0.25, 4.0))
    assert ts[0] == 4.0 and ts[3] == 0.25 and ts.min() >= 0.25 and ts.max() <= 4.0
    for ratio in (0.0, -1.0, np.nan, np.inf, "x"):
        with pytest.raises(ValueError):
            alignment_time_scale(diag, 6, ratio)
    with pytest.raises(ValueError):
        alignment_time_scale(np.array([(0, 0), (0, 1)]), 1)


def _rows():
    X = np.array([[-3.0, 0.5, 0.25], [-2.0, 1.5, -0.25], [-np.inf, 0.0, 0.0], [-1.0, 0.1, 0.7], [-0.5, -0.3, 0.2]])
    return X


def test_warp_rows_by_hand():
    from eaqhm_amd import warp_rows
    X = _rows()
    # integer indices: the rows bit for bit, the empty row included; held at the ends
    out = warp_rows(X, [0.0, 1.0, 2.0, 3.0, 4.0, -2.0, 9.5])
    assert out.dtype == np.float64 and out.shape == (7, 3)
    assert np.array_equal(out[:5], X) and np.array_equal(out[5], X[0]) and np.array_equal(out[6], X[4])
    odd = np.array([[0.1, 1 / 3.0, -0.0], [np.pi, 5e-324, 1e308]])
    back = warp_rows(odd, [1, 0, 1])
    assert back.tobytes() == odd[[1, 0, 1]].tobytes()                    # -0.0 and a denormal survive
    # between two finite rows: linear
    assert np.array_equal(warp_rows(X, [0.25])[0], 0.75 * X[0] + 0.25 * X[1])
    assert np.array_equal(warp_rows(X, [3.5])[0], 0.5 * X[3] + 0.5 * X[4])
    # next to the empty row 2: the nearer neighbour decides (the lower one at exactly one half)
    assert np.array_equal(warp_rows(X, [1.25])[0], X[1])                 # nearer 1, farther empty: a copy of 1
    assert np.array_equal(warp_rows(X, [1.5])[0], X[1])
    assert np.array_equal(warp_rows(X, [1.75])[0], X[2])                 # nearer is the empty row
    assert np.array_equal(warp_rows(X, [2.25])[0], X[2])
    assert np.array_equal(warp_rows(X, [2.5])[0], X[2])
    assert np.array_equal(warp_rows(X, [2.75])[0], X[3])
    got = warp_rows(X, np.linspace(0, 4, 33))
    empty = np.isneginf(got[:, 0])
    assert np.all(got[empty, 1:] == 0) and np.all(np.isfinite(got[~empty]))   # only whole empty rows, never a NaN
    # 1-D: a track
    f0 = np.array([100.0, 110.0, 130.0])
    assert np.array_equal(warp_rows(f0, [0.0, 0.5, 1.0, 1.25, 2.0, 7.0]), [100.0, 105.0, 110.0, 115.0, 130.0, 130.0])
    assert warp_rows(X, []).shape == (0, 3)
    for bad_X, bad_i in ((X[None], [0.0]), ("x", [0.0]), (X[:0], [0.0]), (X, [np.nan]), (X, [[0.0]]), (X, "x"),
                         (X, [np.inf]), (np.float64(1.0), [0.0])):
        with pytest.raises(ValueError):
            warp_rows(bad_X, bad_i)


@pytest.fixture()
def no_device(monkeypatch):
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


def _ceps(n, P, seed=0):
    C = np.random.default_rng(seed).standard_normal((n, P + 1))
    C[:, 0] -= 4.0
    return C


def test_model_align_rejects_bad_arguments(no_device):
    from eaqhm_amd import model_align
    from eaqhm_amd.model import check_model_align_arguments
    A, B = _ceps(7, 5), _ceps(13, 5, 1)
    CA, CB, r, w, e = check_model_align_arguments(A, B)
    assert r == 12 and w == 0.0 and e == 4.0 and CA.flags["C_CONTIGUOUS"] and np.array_equal(CB, B)
    assert check_model_align_arguments(A, B, band=2)[2] == 2               # the minimum for 7 x 13
    assert check_model_align_arguments(A, B, band=500)[2] == 12            # never more than the full table
    assert check_model_align_arguments(A[:1], B)[2] == 12 and check_model_align_arguments(B, A[:1])[2] == 12
    nan, half = A.copy(), A.copy()
    nan[2, 3] = np.nan
    half[2, 0] = -np.inf                                                  # -inf ahead of nonzero coefficients
    calls = [dict(CA=A, CB=_ceps(13, 6)),                                  # different P
             dict(CA=A, CB=B, band=1), dict(CA=A, CB=B, band=-1), dict(CA=A, CB=B, band=2.5), dict(CA=A, CB=B, band="x"),
             dict(CA=A[:1], CB=B, band=11), dict(CA=A, CB=B, band=True),
             dict(CA=nan, CB=B), dict(CA=A, CB=nan.repeat(2, axis=0)[:13]), dict(CA=half, CB=B),
             dict(CA=A[0], CB=B), dict(CA=A, CB=B[None]), dict(CA=A[:, :1], CB=B[:, :1]), dict(CA=A[:0], CB=B),
             dict(CA=np.zeros((3, 65)), CB=np.zeros((3, 65))), dict(CA="x", CB=B)]
    for v in (-1.0, np.nan, np.inf, -np.inf, "x", None):
        calls += [dict(CA=A, CB=B, c0_weight=v), dict(CA=A, CB=B, empty_cost=v)]
    for kw in calls:
        with pytest.raises(ValueError):
            check_model_align_arguments(**kw)
        with pytest.raises(ValueError):
            model_align(**kw)
    with pytest.raises(ValueError, match="band >= 2"):
        model_align(A, B, band=1)


def test_dtw_rejects_bad_arguments(no_device):
    from eaqhm_amd import dtw
    from eaqhm_amd.model import check_dtw_arguments
    d = np.ones((7, 13))
    out, r = check_dtw_arguments(d.astype(np.int32))
    assert out.dtype == np.float64 and r == 12 and check_dtw_arguments(d, 2)[1] == 2
    for v in (-1e-300, np.nan, np.inf, -np.inf):
        bad = d.copy()
        bad[3, 4] = v
        with pytest.raises(ValueError):
            dtw(bad)
    for bad in (d[0], d[None], d[:0], d[:, :0], "x", None, d.astype(complex)):
        with pytest.raises(ValueError):
            dtw(bad)
    for band in (1, 0, -3, 1.5, "x"):
        with pytest.raises(ValueError):
            dtw(d, band)


def test_the_working_set_must_fit_the_device():
    from eaqhm_amd.model import _fits_device

    class Cuda:
        @staticmethod
        def mem_get_info(dev):
            return (9 * 100 * 41, 0)

    class Torch:
        cuda = Cuda

    _fits_device(Torch, None, 100, 20)
    with pytest.raises(ValueError, match="band="):
        _fits_device(Torch, None, 101, 20)


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
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(eaqhm_\w+)\(", header, re.M))
    assert declared == set(sym), declared ^ set(sym)
    csrc = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc")
    with open(os.path.join(csrc, "eaqhm_common.h")) as f:
        assert re.search(r"#define EAQHM_ABI_VERSION 6\b", f.read())
    with open(os.path.join(csrc, "Makefile")) as f:
        assert re.search(r"^SRC\s*:=.*\beaqhm_align\.hip\b", f.read(), re.M)
    with open(os.path.join(csrc, "eaqhm_align.hip")) as f:
        src = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r'extern "C" int %s\(' % name, src), name
    for name in ("model_align", "dtw", "alignment_index", "warp_rows", "alignment_time_scale"):
        assert callable(getattr(eaqhm_amd, name)), name
    for name in ("cepstrum_cost", "dtw"):
        assert callable(getattr(hip.Context, name)), name


def test_cli_flags_and_their_exclusions(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav"])
    assert a.envelope_from is None and a.timing_from is None and a.align_band is None
    a = cli.parser().parse_args(["x.wav", "--envelope-from", "b.wav", "--timing-from", "c.wav", "--align-band", "1.5",
                                 "--cepstral-envelope", "24"])
    assert (a.envelope_from, a.timing_from, a.align_band, a.cepstral_envelope) == ("b.wav", "c.wav", 1.5, 24)
    missing, other = str(tmp_path / "missing.wav"), str(tmp_path / "other.wav")
    tc = tmp_path / "curve.txt"
    tc.write_text("0 1\n1 1.2\n")
    for flags in (["--timing-from", other, "--time-scale", "1.2"], ["--timing-from", other, "--time-scale-curve", str(tc)],
                  ["--envelope-from", other, "--no-envelope"], ["--align-band", "1.0"],
                  ["--align-band", "1.0", "--pitch-scale", "1.2"], ["--envelope-from", other, "--align-band", "-1"],
                  ["--envelope-from", other, "--align-band", "nan"], ["--envelope-from"], ["--timing-from"]):
        with pytest.raises(SystemExit):
            cli.main([missing] + flags)
    for flags in (["--envelope-from", other, "--cepstral-envelope", "64"],
                  ["--timing-from", other, "--pitch-scale", "9"]):
        with pytest.raises(ValueError):
            cli.main([missing] + flags)                        # rejected before the analysis
    for flags in (["--envelope-from", other], ["--timing-from", other], ["--envelope-from", other, "--timing-from", other],
                  ["--envelope-from", other, "--cepstral-envelope", "20", "--cepstral-lambda", "1e-4", "--align-band", "0.5"],
                  ["--timing-from", other, "--pitch-scale", "1.1", "--no-envelope"],
                  ["--envelope-from", other, "--time-scale", "1.2", "--formant-scale", "1.1", "--phase", "shape"]):
        with pytest.raises(FileNotFoundError):
            cli.main([missing] + flags)                        # accepted: the analysis starts
