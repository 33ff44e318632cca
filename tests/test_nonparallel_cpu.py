"""CPU tests of the non-parallel training: the NumPy model's own properties (tests/nn_ref.py), the
conditions on every input set of tests/test_gpu_nonparallel.py, the host side of eaqhm_amd.nonparallel (every argument
check, the loop driven through NumPy stand-ins for the search and the training), the new symbols, the split rule and the
CLI flag.  No GPU.

The quality case (nn_ref.inca_set(): 2400 x 3, six clusters, the first third's x against the SECOND third's y, the last
third held out; nn_ref.loop with 6 components, 8 rounds, symmetric, every column mapped, the mixture initialised on the x
columns as conversion_train does): the figures are printed by test_model_quality_case and recorded in DESIGN.md §12.5."""
import os
import re

import numpy as np
import pytest

import gmm_ref as G
import nn_ref as N
from conftest import ROOT

LD = np.longdouble
PKG = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd")


@pytest.fixture()
def no_device(monkeypatch):
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


_MODEL = {}


def model_loop(dtype=np.float64):
    """nn_ref.loop on the quality case, once per precision."""
    if dtype not in _MODEL:
        S = N.inca_set()
        _MODEL[dtype] = N.loop(S["X"], S["Y"], S["components"], dtype=dtype)
    return _MODEL[dtype]


# ---- the model against itself
def test_model_ties_take_the_lowest_index():
    A, B, want = N.tie_case()
    assert np.array_equal(B[5], B[40]) and np.array_equal(B[60], B[70]) and np.array_equal(B[2700], B[2800])
    s = N.scores(A, B)
    assert np.array_equal(s, np.round(s)) and np.array_equal(s.astype(LD), N.scores(A, B, LD))      # integers: exact
    assert s[3, 100] == s[3, 6000] == s[3].min() and s[0, 5] == s[0, 40] == s[0].min()
    assert s[1, 60] == s[1, 70] == s[1].min() and s[2, 2700] == s[2, 2800] == s[2].min()
    for dtype in (np.float64, LD):
        idx = N.nearest(A, B, dtype)
        for i, j in want.items():
            assert idx[i] == j
    assert not N.decided(A, B)[:4].any()                                # a tie is never "decided"
    d2 = N.dist2(A, B, N.nearest(A, B))
    assert np.all(d2[:3] == 0.0) and d2[3] == 4.0


def test_model_permutations_and_dist2():
    A, B = N.random_case(70, 300, 5, 1)
    idx = N.nearest(A, B)
    perm = np.random.default_rng(2).permutation(len(A))
    assert np.array_equal(N.nearest(A[perm], B), idx[perm])
    pb = np.random.default_rng(3).permutation(len(B))
    assert np.array_equal(pb[N.nearest(A, B[pb])], idx)               # no ties in this set: B's order does not matter
    d2 = N.dist2(A, B, idx)
    assert np.all(d2 >= 0) and np.array_equal(N.dist2(A[perm], B, idx[perm]), d2[perm])
    brute = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(np.argmin(brute, axis=1), idx) and np.allclose(brute.min(axis=1), d2, rtol=1e-14, atol=0)
    assert np.all(np.abs(d2 - N.dist2(A, B, idx, LD)) <= N.dist2_bar(A, B, idx))
    assert np.all(N.dist2(B, B, np.arange(len(B))) == 0.0)


def test_pairs_are_deduplicated_and_sorted():
    from eaqhm_amd import nonparallel
    p, q = np.array([2, 0, 2]), np.array([1, 1, 0, 2])
    want = [[0, 2], [1, 0], [1, 1], [2, 2], [2, 3]]                      # (0, 2) twice, once kept
    for fn in (N.pairs, nonparallel.nonparallel_pairs):
        assert np.array_equal(fn(p, q), want) and fn(p, q).dtype == np.int64
        assert np.array_equal(fn(p), [[0, 2], [1, 0], [2, 2]])


# ---- conditions on the inputs of the GPU tests
@pytest.mark.parametrize("i", range(len(N.SEARCH_SHAPES)))
def test_search_inputs_are_decided(i):
    """The undecided share in the model alone is at most 1 %."""
    from eaqhm_amd import nonparallel
    A, B = N.search_case(i)
    nA, nB, D, lda, ldb = N.SEARCH_SHAPES[i]
    assert A.shape == (nA, lda or D) and B.shape == (nB, ldb or D)
    assert np.all(np.isnan(A[:, D:])) and np.all(np.isnan(B[:, D:])) and np.all(np.isfinite(A[:, :D]))
    ok = N.decided(A[:, :D], B[:, :D])
    print("search %s: %d of %d rows decided, %d splits" % (N.SEARCH_SHAPES[i], ok.sum(), nA, nonparallel.nn_splits(nA, nB)))
    assert (~ok).sum() <= 0.01 * nA
    assert np.array_equal(N.nearest(A[:, :D], B[:, :D])[ok], N.nearest(A[:, :D], B[:, :D], LD)[ok])


def test_search_shapes_cover_the_edges():
    from eaqhm_amd import nonparallel
    nAs, nBs, Ds = ({s[i] for s in N.SEARCH_SHAPES} for i in range(3))
    assert nAs == {1, 15, 16, 17, 63, 64, 65, 130} and Ds == {1, 3, 4, 5, 36, 127, 128}
    assert nBs == {1, 16, 17, 63, 64, 65, 129, 4160, 8200}
    split = {nB: {nonparallel.nn_splits(s[0], nB) for s in N.SEARCH_SHAPES if s[1] == nB} for nB in (4160, 8200)}
    assert split == {4160: {2}, 8200: {3}} and 4160 % 64 == 0 and 8200 % 64 != 0
    assert any(s[2] == 128 and s[1] > 64 for s in N.SEARCH_SHAPES)
    assert any(s[3] for s in N.SEARCH_SHAPES) and any(s[4] for s in N.SEARCH_SHAPES)
    A, B, _ = N.tie_case()
    assert nonparallel.nn_splits(len(A), len(B)) == 3 and 2700 < 43 * 64 <= 2800 and 100 < 43 * 64 and 6000 >= 86 * 64


def test_loop_inputs_are_decided_in_every_round():
    f, g = model_loop(), model_loop(LD)
    S = N.inca_set()
    assert len(f["xc"]) == len(g["xc"]) == len(f["trace"])
    for xc in f["xc"]:
        assert N.decided(xc, S["Y"]).all() and N.decided(S["Y"], xc).all()
    for a, b in zip(f["pairs"], g["pairs"]):
        assert np.array_equal(a, b)
    for a, b in zip(f["fits"], g["fits"]):
        assert len(a["loglik"]) == len(b["loglik"])
    assert f["best"] == g["best"]


def test_model_quality_case():
    """Held-out rms of the returned map at most 0.6 x the identity's."""
    f = model_loop()
    S = N.inca_set()
    dx = S["X"].shape[1]
    ident = N.rms(S["Xh"], S["Yh"])
    held = [N.rms(G.convert(fit, dx, S["Xh"]), S["Yh"]) for fit in f["fits"]]
    par = G.fit(np.hstack((S["Xtrue"], S["Ytrue"])), S["components"], split=dx)
    print("trace", " ".join("%.4f" % t for t in f["trace"]))
    print("held-out rms", " ".join("%.3f" % h for h in held), "identity %.3f parallel %.3f best %d"
          % (ident, N.rms(G.convert(par, dx, S["Xh"]), S["Yh"]), f["best"]))
    assert np.all(np.diff(f["trace"]) < 0) and len(f["trace"]) == 9 and f["best"] == 8
    assert held[f["best"] - 1] <= 0.6 * ident


# ---- the host loop through NumPy stand-ins for the search and the training
def fake_train(X, Y, components=8, *, level=False, iters=20, tol=1e-5, floor=1e-6, init=None, device_index=0):
    assert init is None and len(X) == len(Y)
    skip = 0 if level else 1
    dx = X.shape[1] - skip
    return dict(fit=G.fit(np.hstack((X[:, skip:], Y[:, skip:])), components, iters=iters, tol=tol, floor=floor, split=dx),
                dx=dx, skip=skip)


def fake_apply(conv, C, *, device_index=0):
    assert np.all(np.isfinite(C))
    out = np.array(C)
    out[:, conv["skip"]:] = G.convert(conv["fit"], conv["dx"], C[:, conv["skip"]:])
    return out


def fake_nearest(A, B, *, device_index=0):
    idx = N.nearest(A, B)
    return idx, N.dist2(A, B, idx)


@pytest.fixture()
def stand_in(monkeypatch, no_device):
    from eaqhm_amd import convert, nonparallel
    monkeypatch.setattr(nonparallel, "nearest_rows", fake_nearest)
    monkeypatch.setattr(convert, "conversion_train", fake_train)
    monkeypatch.setattr(convert, "conversion_apply", fake_apply)
    return nonparallel


def test_host_loop_is_the_model(stand_in):
    S = N.inca_set()
    f = model_loop()
    conv, info = stand_in.conversion_train_nonparallel(S["X"], S["Y"], S["components"], level=True)
    assert set(info) == {"ix", "iy", "trace", "rounds", "best"}
    assert np.array_equal(info["trace"], f["trace"]) and info["trace"].dtype == np.float64
    assert info["rounds"] == len(f["fits"]) == 8 and info["best"] == f["best"]
    pr = f["pairs"][f["best"] - 1]
    assert np.array_equal(info["ix"], pr[:, 0]) and np.array_equal(info["iy"], pr[:, 1]) and info["ix"].dtype == np.int64
    assert np.array_equal(conv["fit"]["means"], f["fits"][f["best"] - 1]["means"])


def test_host_loop_with_empty_rows_and_level_column(stand_in):
    """level=False: column 0 is not searched; empty rows are never searched or matched and the indices count them."""
    S = N.inca_set()
    rng = np.random.default_rng(5)
    X = np.hstack((rng.standard_normal((800, 1)) * 50, S["X"]))           # a level that would wreck the search if used
    Y = np.hstack((rng.standard_normal((800, 1)) * 50, S["Y"]))
    _, plain = stand_in.conversion_train_nonparallel(X, Y, 6, rounds=2)
    f = N.loop(S["X"], S["Y"], 6, rounds=2)
    assert np.array_equal(plain["trace"], f["trace"]) and np.array_equal(plain["ix"], f["pairs"][plain["best"] - 1][:, 0])
    empty = np.zeros((1, 4))
    empty[0, 0] = -np.inf
    ex, ey = np.sort(rng.choice(801, size=40)), np.sort(rng.choice(801, size=25))
    Xe, Ye = np.insert(X, ex, empty, axis=0), np.insert(Y, ey, empty, axis=0)
    _, info = stand_in.conversion_train_nonparallel(Xe, Ye, 6, rounds=2)
    gx, gy = np.flatnonzero(~np.isneginf(Xe[:, 0])), np.flatnonzero(~np.isneginf(Ye[:, 0]))
    assert len(gx) == 800 and len(gy) == 800
    assert np.array_equal(info["trace"], plain["trace"]) and info["best"] == plain["best"]
    assert np.array_equal(info["ix"], gx[plain["ix"]]) and np.array_equal(info["iy"], gy[plain["iy"]])
    assert np.all(np.isfinite(Xe[info["ix"]])) and np.all(np.isfinite(Ye[info["iy"]]))
    assert np.all(np.diff(info["ix"]) >= 0)


class Script:
    """Stand-ins that play a given trace: every search returns the round's value as each squared distance."""

    def __init__(self, trace):
        self.trace, self.calls, self.trained = list(trace), 0, 0

    def nearest(self, A, B, *, device_index=0):
        r = self.calls // self.per_round
        self.calls += 1
        return np.zeros(len(A), dtype=np.int64), np.full(len(A), self.trace[r])

    def train(self, X, Y, components=8, **kw):
        self.trained += 1
        return dict(tag=self.trained)

    @staticmethod
    def apply(conv, C, *, device_index=0):
        return np.array(C)


# dyadic values: the mean of equal numbers is then that number exactly
@pytest.mark.parametrize("trace,kw,stop,best", [
    ((1.0, 0.5, 0.25, 0.5, 0.125), {}, 3, 2),                           # a rise stops it; the map before the rise
    ((1.0, 0.5, 0.375, 0.75), dict(tol=0.25), 3, 2),                    # 0.375 = (1 - tol) x 0.5 is no rise: goes on
    ((1.0, 0.5, 0.4375, 0.125), dict(tol=0.25), 2, 2),                  # 0.4375 > 0.375 stops, and is the smallest
    ((1.0, 0.5, 0.5, 0.5, 0.5), dict(tol=0.0, rounds=3), 3, 1),        # equal is no rise at tol = 0; the lowest r on ties
    ((1.0, 2.0, 0.125), {}, 1, 1),                                      # worse than no map at all: still conv_1
    ((1.0, 0.5, 0.25, 0.125), dict(rounds=1), 1, 1),
    ((1.0, 0.5, 0.25, 0.125, 0.0625), dict(rounds=2, symmetric=False), 2, 2),
])
def test_stop_rule_and_choice_of_the_map(monkeypatch, no_device, trace, kw, stop, best):
    from eaqhm_amd import convert, nonparallel
    s = Script(trace)
    s.per_round = 2 if kw.get("symmetric", True) else 1
    monkeypatch.setattr(nonparallel, "nearest_rows", s.nearest)
    monkeypatch.setattr(convert, "conversion_train", s.train)
    monkeypatch.setattr(convert, "conversion_apply", s.apply)
    X = np.random.default_rng(0).standard_normal((40, 3))
    conv, info = nonparallel.conversion_train_nonparallel(X, X[:30], 2, **kw)
    assert np.array_equal(info["trace"], trace[:stop + 1]) and info["rounds"] == stop == s.trained
    assert info["best"] == best and conv == dict(tag=best)
    assert s.calls == s.per_round * (stop + 1)                          # symmetric=False never searches from Y


def test_linalg_error_passes_through(monkeypatch, no_device):
    from eaqhm_amd import convert, nonparallel

    def starved(*a, **k):
        raise np.linalg.LinAlgError("component 1 is starved")
    monkeypatch.setattr(nonparallel, "nearest_rows", fake_nearest)
    monkeypatch.setattr(convert, "conversion_train", starved)
    X = np.random.default_rng(0).standard_normal((40, 3))
    with pytest.raises(np.linalg.LinAlgError, match="starved"):
        nonparallel.conversion_train_nonparallel(X, X, 2)


# ---- every ValueError, before any device work
def test_argument_errors(no_device):
    from eaqhm_amd import nonparallel as P
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((40, 4)), rng.standard_normal((30, 4))
    got = P.check_nonparallel_arguments(X.astype(np.float32), Y, 3, np.int64(50), 0, False, True)
    assert got[0].dtype == np.float64 and got[2:] == (50, 0.0, False, True)
    assert P.check_nonparallel_arguments(X, Y, init="kmeans")[2:] == (8, 1e-3, True, False)
    nan = X.copy()
    nan[3, 1] = np.nan
    half = X.copy()
    half[2, 0] = -np.inf                                                # -inf with coefficients behind it: not an empty row
    empty = np.zeros((5, 4))
    empty[:, 0] = -np.inf
    few = np.vstack((X[:5], empty))                                     # 5 non-empty rows cannot carry 3 components
    bad = [dict(X=nan), dict(Y=nan), dict(X=half), dict(X=X[0]), dict(X="rows"), dict(X=X[:, :3]), dict(X=X[:, :1], Y=Y[:, :1]),
           dict(X=np.zeros((40, 65)), Y=np.zeros((30, 65))), dict(X=empty), dict(Y=empty), dict(X=few),
           dict(X=np.zeros((0, 4))), dict(rounds=0), dict(rounds=51), dict(rounds=2.5), dict(rounds="a"), dict(rounds=True),
           dict(tol=-1e-9), dict(tol=1.0), dict(tol=np.nan), dict(tol="a"), dict(tol=True), dict(symmetric=1),
           dict(symmetric=None), dict(level=1), dict(components=0), dict(components=65), dict(components=2.5),
           dict(iters=0), dict(iters=1001), dict(em_tol=-1.0), dict(em_tol=np.inf), dict(floor=0.0), dict(floor=1.0),
           dict(init="lbg"), dict(init=np.zeros(40, dtype=np.int64)), dict(init=2.5)]
    for kw in bad:
        args = dict(dict(X=X, Y=Y, components=3), **kw)
        with pytest.raises(ValueError):
            P.check_nonparallel_arguments(**args)
        with pytest.raises(ValueError):
            P.conversion_train_nonparallel(**args)
    with pytest.raises(AssertionError, match="device work"):           # good arguments reach the device
        P.conversion_train_nonparallel(X, Y, 3)
    for A, B in ((X, Y[:, :3]), (nan, Y), (X, nan[:30]), (X[0], Y), (np.zeros((0, 4)), Y), (X, np.zeros((0, 4))),
                 (np.zeros((3, 129)), np.zeros((3, 129))), (np.zeros((3, 0)), np.zeros((3, 0))), ("a", Y),
                 (few, Y)):
        with pytest.raises(ValueError):
            P.nearest_rows(A, B)
    with pytest.raises(AssertionError, match="device work"):
        P.nearest_rows(X, Y)


# ---- the binding, the header and the split rule
NN_ARGUMENT_COUNTS = dict(eaqhm_nn_splits=2, eaqhm_nn_work_len=3, eaqhm_nn_rows=11)
RULE = "S = min(ceil(nB / 4096), max(1, ceil(1024 / ceil(nA / 64))))"


def rule(nA, nB):
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    return min(ceil(nB, 4096), max(1, ceil(1024, ceil(nA, 64))))


def test_symbols():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    common = open(os.path.join(PKG, "csrc", "eaqhm_common.h")).read()
    assert re.search(r"#define\s+EAQHM_ABI_VERSION\s+6\b", common)
    bound = {name: len(args) for name, _, args in hip.SYMBOLS_NN}
    others = hip.SYMBOLS + hip.SYMBOLS_MLPG + hip.SYMBOLS_GV + hip.SYMBOLS_CEPWARP + hip.SYMBOLS_KMEANS + hip.SYMBOLS_MLPG_EM
    assert not set(bound) & {name for name, _, _ in others}                            # a table of their own
    header = open(os.path.join(ROOT, "include", "eaqhm_nn.h")).read()
    assert '#include "eaqhm_nn.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(bound) == set(NN_ARGUMENT_COUNTS)
    for name, n in NN_ARGUMENT_COUNTS.items():
        assert bound[name] == n, name
        decl = re.search(r"^(?:int|int32_t|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header, re.M)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
    for name in ("nn_splits", "nn_work_len", "nn_rows"):
        assert callable(getattr(hip.Context, name))
    lib = hip.load_library()
    assert lib.eaqhm_nn_rows(None, None, 1, 1, None, 1, 1, 1, None, None, None) == -1            # EAQHM_EINVAL
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\beaqhm_nn\.hip\b", makefile, re.M)
    assert re.search(r"^HDR\s*:=.*include/eaqhm_nn\.h\b", makefile, re.M)


def test_splits_follow_the_headers_rule():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import hip, nonparallel
    header = open(os.path.join(ROOT, "include", "eaqhm_nn.h")).read()
    assert RULE in header and RULE[4:] in nonparallel.nn_splits.__doc__
    lib = hip.load_library()
    sizes = (1, 63, 64, 65, 130, 2000, 4096, 4097, 8192, 8193, 60000, 65536, 65537, 10 ** 6, 2 ** 31 - 1)
    for nA in sizes:
        for nB in sizes:
            S = rule(nA, nB)
            assert lib.eaqhm_nn_splits(nA, nB) == nonparallel.nn_splits(nA, nB) == S, (nA, nB)
            assert 1 <= S <= -(-nB // 64)                                               # no split without a panel
            for D in (1, 24, 128):
                assert lib.eaqhm_nn_work_len(nA, nB, D) == nonparallel.nn_work_len(nA, nB, D) == nB + 2 * S * nA
    assert rule(130, 4097) == 2 and rule(2000, 60000) == 15 and rule(60000, 60000) == 2 and rule(10 ** 6, 10 ** 6) == 1
    for nA, nB in ((0, 1), (1, 0), (2 ** 31, 1), (1, 2 ** 31), (-1, 5)):
        assert lib.eaqhm_nn_splits(nA, nB) == -1 and lib.eaqhm_nn_work_len(nA, nB, 4) == -1
        with pytest.raises(ValueError):
            nonparallel.nn_splits(nA, nB)
    assert lib.eaqhm_nn_work_len(5, 5, 0) == -1 and lib.eaqhm_nn_work_len(5, 5, 129) == -1


def test_not_reexported():
    import eaqhm_amd
    from eaqhm_amd import nonparallel
    for name in ("conversion_train_nonparallel", "nearest_rows", "nn_splits", "check_nonparallel_arguments"):
        assert callable(getattr(nonparallel, name)) and not hasattr(eaqhm_amd, name)
    assert "§12.5" in nonparallel.__doc__ and "INCA" in nonparallel.__doc__


# ---- the CLI
def test_cli_flag():
    from eaqhm_amd import cli
    train = ["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz"]
    assert cli.parser().parse_args(train).conversion_nonparallel is None
    assert cli.parser().parse_args(train + ["--conversion-nonparallel"]).conversion_nonparallel == 8
    assert cli.parser().parse_args(train + ["--conversion-nonparallel", "3"]).conversion_nonparallel == 3
    for argv in (["x.wav", "--conversion-nonparallel"], ["x.wav", "--conversion-nonparallel", "4"],
                 train + ["--conversion-nonparallel", "0"], train + ["--conversion-nonparallel", "51"],
                 train + ["--conversion-nonparallel", "2.5"],
                 ["x.wav", "--conversion", "m.npz", "--conversion-nonparallel"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    assert "--conversion-nonparallel" in cli.__doc__


def test_cli_training_without_an_alignment(tmp_path, monkeypatch):
    from eaqhm_amd import cli, convert, model, nonparallel
    from test_mlpg_cpu import host_dynamic_conversion
    conv, _, _ = host_dynamic_conversion()
    n, m = 12, 9
    seen = dict(np=[], train=[])
    monkeypatch.setattr(model, "model_parameters", lambda det, fs, order=None, lam=5e-4, **kw: dict(
        f0=np.full(n, 100.0), ceps=np.zeros((n, 3)), voiced=np.ones(n, bool), step=80, fs=fs))
    monkeypatch.setattr(model, "model_cepstrum", lambda det, fs, order=None, lam=5e-4, **kw: np.ones((m, 3)))
    monkeypatch.setattr(cli.wavfile, "read", lambda path: (16000, None))
    monkeypatch.setattr(cli, "eaQHMAnalysisAndSynthesis", lambda path, gender, **kw: (None, None, "det_t", None))
    monkeypatch.setattr(cli, "align_other", lambda *a, **k: pytest.fail("the alignment ran"))
    info = dict(ix=np.array([0, 3, 3]), iy=np.array([1, 1, 8]), trace=np.array([2.0, 1.0]), rounds=1, best=1)
    monkeypatch.setattr(nonparallel, "conversion_train_nonparallel",
                        lambda X, Y, M, **kw: seen["np"].append((X.shape, Y.shape, M, kw)) or (dict(conv), info))
    monkeypatch.setattr(convert, "dynamic_rows", lambda C, span=2, **k: np.hstack((C, C)))
    monkeypatch.setattr(convert, "conversion_train",
                        lambda X, Y, M, **kw: seen["train"].append((X.shape, Y.shape, M, kw)) or dict(conv))
    out = os.path.join(tmp_path, "m.npz")
    base = ["x.wav", "--conversion-train", "t.wav", "--conversion-save", out, "--conversion-nonparallel"]
    cli.train_conversion_nonparallel(cli.parser().parse_args(base), "male", {}, 16000, {})
    assert seen["np"] == [((n, 3), (m, 3), 8, dict(rounds=8))] and not seen["train"]
    d = np.load(out)
    assert {"order", "lam", "fs", "src_f0", "tgt_f0", "weights", "A"} <= set(d.files) and int(d["order"]) == 2
    cli.train_conversion_nonparallel(cli.parser().parse_args(base + ["5", "--conversion-span", "2", "--conversion-init",
                                                                     "kmeans", "--conversion-components", "4"]),
                                     "male", {}, 16000, {})
    assert seen["np"][-1] == ((n, 3), (m, 3), 4, dict(rounds=5, init="kmeans"))
    assert seen["train"] == [((3, 6), (3, 6), 4, dict(span=2, gv=None, init="kmeans"))]
