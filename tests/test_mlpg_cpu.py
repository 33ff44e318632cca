"""CPU tests of the trajectory conversion: the NumPy model's own properties and limits
(tests/mlpg_ref.py), the host side of eaqhm_amd.convert (every new argument check, the dynamic map's fields, the npz round
trip), the new symbols and the CLI flags.  No GPU: the kernels are tested in tests/test_gpu_mlpg.py.

What the model gave when these tests were written: the step case's largest adjacent difference 0.19900743719394792
(float64) and 0.19900743719394796 (long double) against 2.0 for the frame-wise rule; M = 1 against the closed form
<= 2e-13 of the largest entry."""
import os
import re

import numpy as np
import pytest

import gmm_ref as G
import mlpg_ref as R
from conftest import ROOT

LD = np.longdouble


@pytest.fixture()
def no_device(monkeypatch):
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


# ---- the delta rule
@pytest.mark.parametrize("span", [1, 2, 3, 8])
def test_delta_matrix_properties(span):
    w = R.window(span)
    assert w[0] == 1.0 / (2 * sum(k * k for k in range(1, span + 1)))
    for T in (1, 2, 3, 2 * span, 2 * span + 1, 4 * span + 1, 40):
        W = R.delta_matrix(T, span, LD)
        assert np.abs(W.sum(axis=1)).max() <= 4 * span * 2.0 ** -64                  # rows sum to 0
        i, j = np.nonzero(W.T @ W)
        assert np.abs(i - j).max(initial=0) <= min(2 * span, T - 1)                  # half-bandwidth 2 L, edges included
        rng = np.random.default_rng(T)
        c = rng.standard_normal((T, 3))
        assert np.abs(W.astype(np.float64) @ c - R.delta_rows(np.hstack((np.zeros((T, 1)), c)), span)[:, 1:]).max() < 1e-15
    assert np.all(R.delta_matrix(1, span) == 0.0)                                    # a run of one row: delta 0
    W2 = R.delta_matrix(2, span)                                                     # two rows: both (c_1 - c_0) sum_tau w_tau
    assert np.allclose(W2, w.sum() * np.array([[-1.0, 1.0], [-1.0, 1.0]]), atol=1e-16)
    if span < 40:                                                                    # a ramp has slope 1 inside the run
        ramp = R.delta_matrix(40, span) @ np.arange(40.0)
        assert np.allclose(ramp[span:40 - span], 1.0, atol=1e-14)


def test_delta_rows_respect_the_gaps():
    rng = np.random.default_rng(2)
    C = rng.standard_normal((30, 3))
    for i in (0, 7, 8, 12, 14, 29):
        C[i] = (-np.inf, 0.0, 0.0)
    D = R.dynamic_rows(C, 2)
    assert D.shape == (30, 6)
    empty = np.isneginf(C[:, 0])
    assert np.all(np.isneginf(D[empty, 0])) and np.all(D[empty, 1:] == 0.0)
    assert np.all(D[13, 3:] == 0.0)                                                  # the run of one row between two gaps
    assert np.all(np.isfinite(D[~empty]))
    moved = C.copy()
    moved[15:29] += 100.0                                                            # another run does not matter
    assert np.array_equal(R.dynamic_rows(moved, 2)[1:7], D[1:7])
    start, length = R.runs_of(~empty)
    assert list(start) == [1, 9, 13, 15] and list(length) == [6, 3, 1, 14]


# ---- the model's limits
def random_system(T, dy, seed, ratio=1.0):
    rng = np.random.default_rng(seed)
    P = np.exp(rng.uniform(-1.0, 1.0, (T, 2 * dy)))
    P[:, dy:] *= ratio
    return P, rng.standard_normal((T, 2 * dy)) * P


@pytest.mark.parametrize("span", [1, 2, 8])
def test_no_delta_precision_is_the_frame_wise_quotient(span):
    P, r = random_system(23, 3, span, ratio=0.0)
    Y = R.solve(P, r, span, [0, 12], [11, 11], LD)
    assert np.all(np.isnan(Y[11]))
    keep = np.arange(23) != 11
    ref = (r[:, :3].astype(LD) / P[:, :3].astype(LD))[keep]
    assert np.all(np.abs(Y[keep] - ref) <= 4 * 2.0 ** -63 * np.abs(ref))             # sqrt, two quotients: a few long-double ulps


def test_one_component_is_the_closed_form():
    """M = 1: gamma = 1, P_t = py and r_t = py (b + ybar + A X_t), so that y = (diag(py^s) + py^D W^T W)^-1 (py^s mu^s + py^D W^T
    mu^D) column by column, mu = ybar + b + A X the frame-wise conversion of both halves."""
    rng = np.random.default_rng(4)
    T, d, span = 60, 2, 2
    CA = np.hstack((np.full((T, 1), -3.0), np.cumsum(rng.standard_normal((T, d)), axis=0) * 0.3))
    CB = np.hstack((np.full((T, 1), -2.0), CA[:, 1:] @ rng.standard_normal((d, d)) + 0.1 * rng.standard_normal((T, d))))
    g = R.train(R.dynamic_rows(CA, span), R.dynamic_rows(CB, span), 1, iters=2)
    out = R.trajectory(g, CA, span)
    X = R.select(R.dynamic_rows(CA, span), d + 1, False) - g["zbar"][:2 * d]
    mu = g["zbar"][2 * d:] + g["b"][0] + X @ g["A"][0].T
    W = R.delta_matrix(T, span)
    for k in range(d):
        ps, pd = g["py"][0, k], g["py"][0, d + k]
        ref = np.linalg.solve(ps * np.eye(T) + pd * W.T @ W, ps * mu[:, k] + pd * W.T @ mu[:, d + k])
        assert np.abs(out[:, 1 + k] - ref).max() <= 1e-11 * np.abs(ref).max()
    assert np.array_equal(out[:, 0], CA[:, 0])


def test_step_response():
    conv, C = R.step_case()
    y = R.trajectory(conv, C, 1)
    rough = float(np.abs(np.diff(y[:, 1])).max())
    assert abs(rough - R.STEP_ROUGHNESS) <= 1e-9 and abs(rough - 0.19900743719) <= 1e-9
    full, P, r, gamma = R.trajectory_inputs(conv, C, 1)
    frame = r[:, 0] / P[:, 0]                                                        # the frame-wise rule on the same map
    assert float(np.abs(np.diff(frame)).max()) == pytest.approx(2.0, abs=1e-12)
    assert abs(y[0, 1] + 1.0) < 1e-4 and abs(y[-1, 1] - 1.0) < 1e-4 and np.all(np.diff(y[:, 1]) >= -1e-12)
    assert np.array_equal(y[:, 0], C[:, 0])


# ---- the host side of the package
def host_dynamic_conversion(level=False):
    """A dynamic conversion dict as conversion_train(span=2) builds it, from the model's fit (no device)."""
    from eaqhm_amd.convert import gmm_conditional_precisions, gmm_conversion_parameters
    CA, CB, X, Y, M, span = R.dynamic_case(N=400, d=2)
    f = R.train(X, Y, M, level=level, iters=3)
    dx = f["dx"]
    A, b, Wx, kx = gmm_conversion_parameters(f["weights"], f["means"] - f["zbar"], f["covs"], dx)
    return dict(weights=f["weights"], means=f["means"], covs=f["covs"], zbar=f["zbar"], phi=f["phi"], loglik=f["loglik"],
                n=np.int64(f["n"]), dx=np.int64(dx), dy=np.int64(f["dy"]), level=np.bool_(level), A=A, b=b, Wx=Wx, kx=kx,
                span=np.int64(span), py=gmm_conditional_precisions(f["covs"], A, dx)), f, CA


def static_conversion():
    from eaqhm_amd.convert import gmm_conversion_parameters
    X, Y, _, M = G.case("sep_600x3")
    f = G.fit(np.hstack((X, Y)), M, iters=4, split=3)
    A, b, Wx, kx = gmm_conversion_parameters(f["weights"], f["means"] - f["zbar"], f["covs"], 3)
    return dict(weights=f["weights"], means=f["means"], covs=f["covs"], zbar=f["zbar"], phi=f["phi"], loglik=f["loglik"],
                n=np.int64(f["n"]), dx=np.int64(3), dy=np.int64(3), level=np.bool_(False), A=A, b=b, Wx=Wx, kx=kx)


def test_conditional_precisions_match_the_model():
    from eaqhm_amd.convert import gmm_conditional_precisions
    conv, f, _ = host_dynamic_conversion()
    assert conv["py"].shape == (3, 4) and np.all(conv["py"] > 0)
    assert np.abs(conv["py"] - f["py"]).max() <= 1e-12 * np.abs(f["py"]).max()
    for m in range(3):                                                               # the diagonal of the Schur complement
        S = conv["covs"][m]
        schur = S[4:, 4:] - S[4:, :4] @ np.linalg.solve(S[:4, :4], S[:4, 4:])
        assert np.abs(1.0 / conv["py"][m] - np.diag(schur)).max() <= 1e-12 * np.abs(schur).max()
    bad = conv["covs"].copy()
    bad[1, 5, 5] = -1.0
    with pytest.raises(np.linalg.LinAlgError, match="component 1"):
        gmm_conditional_precisions(bad, conv["A"], 4)


def test_static_paths_are_unchanged(no_device):
    from eaqhm_amd import check_conversion, conversion_apply, conversion_pairs, conversion_trajectory
    CA = np.arange(12.0).reshape(4, 3)
    CB = 100.0 + np.arange(10.0).reshape(5, 2)
    CA[1] = (-np.inf, 0, 0)
    CB[3] = (-np.inf, 0)
    path = np.array([[0, 0], [1, 1], [2, 2], [2, 3], [3, 4]])
    for X, Y in (conversion_pairs(CA, CB, path), conversion_pairs(CA, CB, path, None), conversion_pairs(CA, CB, path, span=None)):
        assert np.array_equal(X, CA[[0, 2, 3]]) and np.array_equal(Y, CB[[0, 2, 4]])    # host only, bit for bit
    conv = static_conversion()
    back = check_conversion(conv)
    assert "span" not in back and "py" not in back
    assert set(back) == {"weights", "means", "covs", "zbar", "dx", "dy", "level", "A", "b", "Wx", "kx", "phi", "loglik", "n"}
    with pytest.raises(ValueError, match="conversion_apply"):
        conversion_trajectory(conv, np.zeros((3, 4)))
    with pytest.raises(AssertionError, match="device work"):                           # the static map still reaches the device
        conversion_apply(conv, np.zeros((3, 4)))


def test_new_argument_errors(no_device):
    from eaqhm_amd import (check_conversion_arguments, conversion_apply, conversion_pairs, conversion_train,
                           conversion_trajectory, dynamic_rows)
    rng = np.random.default_rng(1)
    C = rng.standard_normal((20, 4))
    for span in (0, 9, -1, 2.5, "two", True, None, np.nan):
        with pytest.raises(ValueError):
            dynamic_rows(C, span)
    for bad in (C[:, :1], np.full((20, 4), np.nan), np.zeros(4), np.zeros((0, 4)), np.zeros((3, 66))):
        with pytest.raises(ValueError):
            dynamic_rows(bad, 2)
    with pytest.raises(AssertionError, match="device work"):
        dynamic_rows(C, 2)
    with pytest.raises(AssertionError, match="device work"):
        dynamic_rows(C)                                                                # the default span is 2
    path = np.stack((np.arange(20), np.arange(20)), axis=1)
    for span in (0, 9, 1.5, "a"):
        with pytest.raises(ValueError):
            conversion_pairs(C, C, path, span)
    with pytest.raises(ValueError):
        conversion_pairs(C, C, path[:5], 2)                                            # a bad path: before any device work
    with pytest.raises(AssertionError, match="device work"):
        conversion_pairs(C, C, path, 2)
    X, Y = rng.standard_normal((50, 6)), rng.standard_normal((50, 8))
    for kw in (dict(span=0), dict(span=9), dict(span=1.5), dict(X=X[:, :5]), dict(Y=Y[:, :7]), dict(X=X[:, :2]),
               dict(Y=Y[:49]), dict(level=1), dict(components=26), dict(X=np.where(X > 9, X, np.nan))):
        args = dict(X=X, Y=Y, components=2, span=2)
        args.update(kw)
        with pytest.raises(ValueError):
            conversion_train(args.pop("X"), args.pop("Y"), args.pop("components"), **args)
    wide = np.zeros((300, 68))                                                         # 33 mapped columns and their deltas: 66
    with pytest.raises(ValueError, match="64"):
        conversion_train(wide, np.zeros((300, 6)), 2, span=2)
    with pytest.raises(ValueError, match="64"):
        conversion_train(np.zeros((300, 6)), wide, 2, span=2)
    assert check_conversion_arguments(rng.standard_normal((300, 66)), rng.standard_normal((300, 66)), 2, span=2)[2] is False
    with pytest.raises(ValueError):                                                    # ... and with the level 66 a side
        check_conversion_arguments(np.zeros((300, 66)), np.zeros((300, 66)), 2, level=True, span=2)
    with pytest.raises(ValueError):                                                    # without a span: 64 columns at most
        conversion_train(np.zeros((300, 66)), np.zeros((300, 66)), 2)
    with pytest.raises(AssertionError, match="device work"):
        conversion_train(rng.standard_normal((300, 66)), rng.standard_normal((300, 66)), 2, span=2)
    conv, _, CA = host_dynamic_conversion()
    with pytest.raises(ValueError, match="conversion_trajectory"):
        conversion_apply(conv, CA)
    for bad in (np.zeros((3, 4)), np.full((3, 3), np.nan), np.zeros(3), CA[:, :2]):
        with pytest.raises(ValueError):
            conversion_trajectory(conv, bad)
    out = conversion_trajectory(conv, np.array([[-np.inf, 0, 0]] * 2))                 # only empty rows: no device work
    assert out.shape == (2, 3) and np.all(np.isneginf(out[:, 0])) and np.all(out[:, 1:] == 0)
    with pytest.raises(AssertionError, match="device work"):
        conversion_trajectory(conv, CA)


def test_npz_round_trip_and_check_conversion(tmp_path):
    from eaqhm_amd import check_conversion
    conv, _, _ = host_dynamic_conversion()
    path = os.path.join(tmp_path, "map.npz")
    np.savez(path, **conv)
    with np.load(path, allow_pickle=False) as z:
        back = check_conversion({k: z[k] for k in z.files})
    assert back["span"] == 2 and isinstance(back["span"], int) and back["dx"] == 4 and back["dy"] == 4
    for k in ("weights", "means", "covs", "zbar", "phi", "A", "b", "Wx", "kx", "loglik", "py"):
        assert np.array_equal(back[k], conv[k]), k
    assert check_conversion(back)["span"] == 2                                         # the validated dict validates again

    def broken(**kw):
        d = dict(conv)
        d.update(kw)
        return d
    neg = conv["py"].copy()
    neg[0, 1] = 0.0
    nan = conv["py"].copy()
    nan[2, 3] = np.nan
    bad = [broken(py=neg), broken(py=nan), broken(py=conv["py"][:, :3]), broken(py=conv["py"][:2]),
           broken(py=conv["py"].astype(str)), broken(span=np.int64(0)), broken(span=np.int64(9)), broken(span=np.float64(2.0)),
           broken(span=np.array([2, 2])), {k: v for k, v in conv.items() if k != "py"},
           broken(dx=np.int64(3), A=conv["A"][:, :, :3], Wx=conv["Wx"][:, :3, :3], means=conv["means"][:, 1:],
                  covs=conv["covs"][:, 1:, 1:], zbar=conv["zbar"][1:], phi=conv["phi"][1:])]
    for i, d in enumerate(bad):
        with pytest.raises(ValueError):
            check_conversion(d)
            print("case", i, "passed the check")


# ---- symbols
NEW_ARGUMENT_COUNTS = dict(eaqhm_ceps_delta=6, eaqhm_mlpg_work_len=3, eaqhm_mlpg_solve=11)


def test_symbols():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import convert, hip
    assert hip.ABI_VERSION == 6
    bound = {name: len(args) for name, _, args in hip.SYMBOLS_MLPG}
    assert not set(bound) & {name for name, _, _ in hip.SYMBOLS}                      # a table of their own
    header = open(os.path.join(ROOT, "include", "eaqhm_mlpg.h")).read()
    assert '#include "eaqhm_mlpg.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(bound) == set(NEW_ARGUMENT_COUNTS)
    for name, n in NEW_ARGUMENT_COUNTS.items():
        assert bound[name] == n, name
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
    for name in ("ceps_delta", "mlpg_work_len", "mlpg_solve"):
        assert callable(getattr(hip.Context, name))
    lib = hip.load_library()
    for n, dy, span in ((1, 1, 1), (700, 17, 2), (60000, 24, 2), (2 ** 31, 64, 8)):
        assert lib.eaqhm_mlpg_work_len(n, dy, span) == convert.mlpg_work_len(n, dy, span) == n * (2 * span + 2) * dy
    for n, dy, span in ((0, 1, 1), (1, 0, 1), (1, 65, 1), (1, 1, 0), (1, 1, 9), (2 ** 31 + 1, 1, 1), (-1, 1, 1)):
        assert lib.eaqhm_mlpg_work_len(n, dy, span) == -1, (n, dy, span)
    assert lib.eaqhm_ceps_delta(None, None, 1, 1, 1, None) == -1                       # no context: EAQHM_EINVAL, no device
    assert lib.eaqhm_mlpg_solve(None, None, None, 1, 1, 1, None, None, 0, None, None) == -1
    makefile = open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "Makefile")).read()
    assert "eaqhm_mlpg.hip" in makefile


# ---- the CLI
def test_cli_flags(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz", "--conversion-span", "2"])
    assert (a.conversion_train, a.conversion_span) == ("t.wav", 2)
    assert cli.parser().parse_args(["x.wav"]).conversion_span is None
    conv, _, _ = host_dynamic_conversion()
    good = os.path.join(tmp_path, "map.npz")
    extra = dict(lam=np.float64(5e-4), fs=np.int64(16000), src_f0=np.array([5.0, 0.2]), tgt_f0=np.array([5.3, 0.25]))
    np.savez(good, order=np.int64(2), **extra, **conv)
    loaded, order, lam, fs, src, tgt = cli.load_conversion(good)
    assert loaded["span"] == 2 and order == 2 and loaded["dx"] == 4                    # order 2: two mapped columns, four with deltas
    wrong = os.path.join(tmp_path, "wrong.npz")
    np.savez(wrong, order=np.int64(4), **extra, **conv)                                # the static reading of dx = 4
    with pytest.raises(ValueError):
        cli.load_conversion(wrong)
    train = ["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz"]
    for argv in (["x.wav", "--conversion-span", "2"], ["x.wav", "--conversion", good, "--conversion-span", "2"],
                 train + ["--conversion-span", "0"], train + ["--conversion-span", "9"],
                 train + ["--conversion-span", "1.5"], train + ["--conversion-span", "2", "--conversion", good]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    assert "--conversion-span" in cli.__doc__ and "conversion_trajectory" in cli.__doc__


def test_cli_uses_the_trajectory_for_a_dynamic_map(tmp_path, monkeypatch):
    """--conversion MAP.npz with a map that carries a span calls conversion_trajectory, not conversion_apply; the analysis
    and the device functions are stand-ins that record their arguments."""
    from eaqhm_amd import cli, convert, model
    conv, _, _ = host_dynamic_conversion()
    good = os.path.join(tmp_path, "map.npz")
    np.savez(good, order=np.int64(2), lam=np.float64(2e-3), fs=np.int64(16000), src_f0=np.array([5.0, 0.2]),
             tgt_f0=np.array([5.3, 0.25]), **conv)
    n, L = 6, 200
    calls = []

    def model_parameters(det, fs, order=None, lam=5e-4, **kw):
        return dict(f0=np.full(n, 100.0), ceps=np.zeros((n, order + 1)), voiced=np.ones(n, bool), step=80, fs=fs)

    def trajectory(conv, C, **kw):
        calls.append(("trajectory", C.shape, conv["span"]))
        return np.full((len(C), conv["dy"] // 2 + 1), -1.0)

    def apply(conv, C, **kw):
        calls.append(("apply", C.shape))
        return np.full((len(C), conv["dy"] + 1), -1.0)

    def synthesis(det, fs, length, **kw):
        calls.append(("synth", kw["envelope"].shape))
        return np.zeros(length)
    monkeypatch.setattr(cli, "eaQHMAnalysisAndSynthesis", lambda path, gender, **o: (np.zeros(L), [1.0], {"who": path}, 0.0))
    monkeypatch.setattr(cli.wavfile, "read", lambda path: (16000, np.zeros(L)))
    monkeypatch.setattr(cli.wavfile, "write", lambda path, fs, x: None)
    monkeypatch.setattr(model, "model_parameters", model_parameters)
    monkeypatch.setattr(model, "unpack_model", lambda det: {"step": 80})
    monkeypatch.setattr(model, "eaQHMSynthesis", synthesis)
    monkeypatch.setattr(convert, "conversion_trajectory", trajectory)
    monkeypatch.setattr(convert, "conversion_apply", apply)
    assert cli.main(["x.wav", "--conversion", good]) == 0
    assert calls == [("trajectory", (n, 3), 2), ("synth", (n, 3))]
