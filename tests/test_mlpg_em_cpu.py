"""CPU tests of the EM refinement of the mixture sequence: the NumPy model's own properties
(tests/mlpg_em_ref.py), the host side of eaqhm_amd.convert (check_em_arguments, the errors raised before any device work),
the new symbol and its table, the unchanged public surface and the CLI flag.  No GPU: the kernel is tested in
tests/test_gpu_mlpg_em.py.

The hand case, ambiguous_case(): 50 rows, two components with the same x marginal, weights 0.6 / 0.4, static y means +1 /
-1, static precision 4, delta precision 100, span 1.  The model gives y = 0.2 on every row at first and 0.76273937238846,
0.99701967873932, 0.99954202885099 (the inner rows; the rows differ by 1e-15) after 1, 2 and 3 iterations, the digits
the issue quotes.  The log-likelihood sum_t ln p(Y_t | X_t) with the definition's constant kc_m = 1/2 sum_j ln py_mj -
(dy / 2) ln 2 pi is -25.334614833245, 26.796782228667, 32.362041527236, 32.362680067103; the issue's figures 66.559,
118.691, 124.2559, 124.2565 are these plus 50 ln 2 pi = 91.893853...: its prototype left the 2 pi constant out, and the
gains are the same.  Both readings are asserted.

The trace of dynamic_case(N=400, d=3, M=3, span=2, seed=31) rose by 75.8, 7.53, 0.798, 0.212, 0.130 and 0.0428 over six
iterations when this was written, the float64 and long-double models at most 1.9e-13 apart in the trace and 4.3e-15 in
the trajectory, the posteriors moving by up to 0.736."""
import inspect
import json
import math
import os
import re

import numpy as np
import pytest

import mlpg_em_ref as E
import mlpg_ref as R
from conftest import ROOT

LD = np.longdouble
HAND_Y = (0.2, 0.76273937238846, 0.99701967873932, 0.99954202885099)
HAND_LOGLIK = (-25.334614833245, 26.796782228667, 32.362041527236, 32.362680067103)
QUOTED_Y = (0.2, 0.7627, 0.99702, 0.99954)
QUOTED_LOGLIK = (66.559, 118.691, 124.2559, 124.2565)


@pytest.fixture()
def no_device(monkeypatch):
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import functions, hip

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)
    monkeypatch.setattr(hip, "load_library", boom)


_DYN = {}


def dynamic():
    """(CA, span, the model's map trained for 6 rounds) of the issue's dynamic case, built once."""
    if not _DYN:
        CA, CB, X, Y, M, span = R.dynamic_case(N=400, d=3, M=3, span=2, seed=31)
        _DYN.update(CA=CA, span=span, f=R.train(X, Y, M, iters=6, tol=-1.0))
    return _DYN["CA"], _DYN["span"], _DYN["f"]


# ---- the model
@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_hand_case(dtype):
    conv, C = E.ambiguous_case()
    assert conv["weights"].tolist() == [0.6, 0.4] and int(conv["span"]) == 1 and len(C) == 50
    assert np.array_equal(conv["py"], [[4.0, 100.0]] * 2)
    prior = E.inputs(conv, C, 1, dtype)["prior"]
    assert np.abs(prior - dtype(0.6) * np.array([1, 0]) - dtype(0.4) * np.array([0, 1])).max() <= 1e-15
    for k in range(4):
        out, trace, _ = E.refine(conv, C, 1, k, dtype)
        assert np.abs(out[:, 1] - HAND_Y[k]).max() <= 1e-9, (k, out[:, 1])
        assert abs(out[25, 1] - QUOTED_Y[k]) <= 0.5 * 10.0 ** -len(str(QUOTED_Y[k]).split(".")[1])
        assert len(trace) == k + 1 and np.array_equal(out[:, 0], C[:, 0])
    assert np.abs(trace - np.array(HAND_LOGLIK)).max() <= 1e-9
    shifted = trace + 50 * math.log(2.0 * math.pi)                                   # the issue's prototype: no 2 pi constant
    for got, quoted in zip(shifted, QUOTED_LOGLIK):
        assert abs(got - quoted) <= 0.5 * 10.0 ** -len(str(quoted).split(".")[1]), (got, quoted)


@pytest.mark.parametrize("case", ["ambiguous", "dynamic"])
def test_trace_does_not_fall(case):
    if case == "ambiguous":
        g, C, span = E.ambiguous_case() + (1,)
    else:
        C, span, g = dynamic()
    _, t64, g64 = E.refine(g, C, span, 6)
    _, tld, _ = E.refine(g, C, span, 6, LD)
    assert len(t64) == 7
    allowance = 100.0 * np.abs(t64.astype(LD) - tld).astype(np.float64)
    rise = np.diff(t64)
    assert np.all(rise >= -allowance[1:]), (rise, allowance)
    assert rise[0] > 50.0                                                            # and it does rise
    if case == "dynamic":
        assert np.abs(g64 - E.inputs(g, C, span)["prior"]).max() > 0.5               # the posteriors move


def test_step_case_is_a_fixed_point():
    conv, C = R.step_case()
    start = R.trajectory(conv, C, 1)
    for dtype in (np.float64, LD):
        out, trace, gamma = E.refine(conv, C, 1, 3, dtype)
        assert np.array_equal(out, R.trajectory(conv, C, 1, dtype))                  # no bit changes
        assert trace[0] == trace[1] == trace[2] == trace[3]
    assert np.array_equal(E.refine(conv, C, 1, 3)[0], start)


def test_one_component_is_a_fixed_point():
    rng = np.random.default_rng(4)
    T, d, span = 60, 2, 2
    CA = np.hstack((np.full((T, 1), -3.0), np.cumsum(rng.standard_normal((T, d)), axis=0) * 0.3))
    CB = np.hstack((np.full((T, 1), -2.0), CA[:, 1:] @ rng.standard_normal((d, d)) + 0.1 * rng.standard_normal((T, d))))
    CA[17] = (-np.inf, 0.0, 0.0)
    g = R.train(R.dynamic_rows(CA, span)[CA[:, 0] > -np.inf], R.dynamic_rows(CB, span)[CA[:, 0] > -np.inf], 1, iters=2)
    out, trace, gamma = E.refine(g, CA, span, 3)
    assert np.all(gamma == 1.0)
    assert np.array_equal(out, R.trajectory(g, CA, span))
    assert np.all(np.isfinite(trace))


def small_problem(n=12, dx=2, dy=1, M=3, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dx))
    prior = rng.uniform(0.1, 1.0, (n, M))
    prior /= prior.sum(axis=1, keepdims=True)
    A = rng.standard_normal((M, 2 * dy, dx))
    bq = rng.standard_normal((M, 2 * dy))
    py = np.exp(rng.uniform(-1, 1, (M, 2 * dy)))
    Y = rng.standard_normal((n, dy))
    return X, prior, A, bq, py, Y


@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_rules(dtype):
    X, prior, A, bq, py, Y = small_problem()
    start, length = np.array([0, 5, 7]), np.array([4, 1, 5])                          # rows 4 and 6 lie outside every run
    prior[2] = (0.0, 0.25, 0.75)                                                      # zero priors
    prior[8] = (0.5, 0.0, 0.5)
    Y[5] = 1e200                                                                      # a lost row: a run of its own
    lp, ll, gamma = E.estep(X, prior, A, bq, py, Y, 2, start, length, dtype)
    assert np.all(np.isnan(gamma[[4, 6]])) and np.all(np.isnan(ll[[4, 6]]))
    assert gamma[2, 0] == 0.0 and gamma[8, 1] == 0.0 and np.isneginf(lp[2, 0])
    assert np.isneginf(ll[5]) and np.array_equal(gamma[5], prior[5].astype(dtype))
    live = np.array([t for t in range(12) if t not in (4, 5, 6)])
    assert np.all(np.isfinite(ll[live])) and np.all(np.abs(gamma[live].sum(axis=1) - 1) <= 4 * 2.0 ** -52)
    # the zero-prior component is out of the row altogether: the others are what they are without it
    keep = [1, 2]
    _, ll2, g2 = E.estep(X, prior[:, keep], A[keep], bq[keep], py[keep], Y, 2, start, length, dtype)
    assert abs(ll2[2] - ll[2]) <= 4 * 2.0 ** -52 * abs(ll[2]) and np.abs(g2[2] - gamma[2, keep]).max() <= 4 * 2.0 ** -52
    # against the definition, row by row
    W = R.delta_matrix(5, 2, dtype)
    Yd = np.hstack((Y[7:12].astype(dtype), W @ Y[7:12].astype(dtype)))
    for i, t in enumerate(range(7, 12)):
        dens = [prior[t, m] * np.exp(E.constants(py, dtype)[m] - (py[m] * (Yd[i] - A[m] @ X[t] - bq[m]) ** 2).sum() / 2)
                for m in range(3)]
        assert abs(np.log(sum(dens)) - ll[t]) <= 1e-13 * max(1.0, abs(ll[t]))
        assert np.abs(np.array(dens) / sum(dens) - gamma[t]).max() <= 1e-13


def test_stop_rule_of_the_model():
    conv, C = E.ambiguous_case()
    _, trace, _ = E.refine(conv, C, 1, 6)
    assert E.stop_iteration(trace, 50, 1e-3, 6) == 3                                 # 0.11 a row, then 1.3e-5
    assert E.stop_iteration(trace, 50, 0.5, 6) == 2
    assert E.stop_iteration(trace, 50, 1e-12, 4) == 4


# ---- the host side of the package
def test_check_em_arguments():
    from eaqhm_amd.convert import EM_MAX_ITERS, check_em_arguments
    assert EM_MAX_ITERS == 100
    assert check_em_arguments() == (4, 0.0, False)
    assert check_em_arguments(0, 1e-3, True) == (0, 1e-3, True)
    assert check_em_arguments(np.int64(100), np.float64(2.0), np.bool_(True)) == (100, 2.0, True)
    assert check_em_arguments(3.0, 0, False) == (3, 0.0, False)
    for bad in (-1, 101, 2.5, "four", None, True, np.nan, np.inf, [4]):
        with pytest.raises(ValueError, match="em_iters"):
            check_em_arguments(bad)
    for bad in (-1e-9, np.nan, np.inf, -np.inf, "small", None, True, [0.0]):
        with pytest.raises(ValueError, match="em_tol"):
            check_em_arguments(4, bad)
    for bad in (0, 1, "yes", None, np.array([True])):
        with pytest.raises(ValueError, match="em_trace"):
            check_em_arguments(4, 0.0, bad)


def test_errors_come_before_any_device_work(no_device):
    from test_mlpg_cpu import host_dynamic_conversion, static_conversion
    from eaqhm_amd.convert import conversion_trajectory_em
    conv, _, CA = host_dynamic_conversion()
    with pytest.raises(ValueError, match="conversion_apply"):
        conversion_trajectory_em(static_conversion(), np.zeros((3, 4)))
    for kw in (dict(em_iters=-1), dict(em_iters=101), dict(em_iters=1.5), dict(em_iters=True), dict(em_tol=-1.0),
               dict(em_tol=np.nan), dict(em_tol="x"), dict(em_trace=1), dict(em_trace=None), dict(gv=True),
               dict(gv_iters=-1), dict(gv_weight=0.0), dict(trace=True)):
        with pytest.raises(ValueError):
            conversion_trajectory_em(conv, CA, **kw)
            print(kw, "passed the checks")
    for bad in (np.zeros((3, 4)), np.full((3, 3), np.nan), np.zeros(3), CA[:, :2]):
        with pytest.raises(ValueError):
            conversion_trajectory_em(conv, bad)
    empty = np.array([[-np.inf, 0, 0]] * 2)                                           # only empty rows: no device work
    out = conversion_trajectory_em(conv, empty)
    assert out.shape == (2, 3) and np.all(np.isneginf(out[:, 0])) and np.all(out[:, 1:] == 0)
    out, ll = conversion_trajectory_em(conv, empty, em_trace=True)
    assert out.shape == (2, 3) and ll.shape == (1,)
    gv = dict(gv_mean=np.ones(2), gv_prec=np.ones(2))
    out, obj, ll = conversion_trajectory_em(conv, empty, em_trace=True, gv=gv, trace=True, gv_iters=3)
    assert obj.shape == (4, 2) and ll.shape == (1,)
    with pytest.raises(AssertionError, match="device work"):                          # good arguments reach the device
        conversion_trajectory_em(conv, CA)


# ---- symbols
def test_symbols():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    assert [name for name, _, _ in hip.SYMBOLS_MLPG_EM] == ["eaqhm_mlpg_estep"]
    name, res, args = hip.SYMBOLS_MLPG_EM[0]
    assert len(args) == 18
    others = hip.SYMBOLS + hip.SYMBOLS_MLPG + hip.SYMBOLS_GV + hip.SYMBOLS_CEPWARP + hip.SYMBOLS_KMEANS
    assert name not in {n for n, _, _ in others}                                      # a table of its own
    header = open(os.path.join(ROOT, "include", "eaqhm_mlpg_em.h")).read()
    assert '#include "eaqhm_mlpg_em.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == {"eaqhm_mlpg_estep"}
    decl = re.search(r"\beaqhm_mlpg_estep\s*\(([^)]*)\)\s*;", header)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 18
    import ctypes
    for p, a in zip(params, args):                                                    # the kinds agree, one by one
        want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int32
        assert a is want, (p, a)
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "ctx", "X", "prior", "A", "bq", "py", "kc", "Y", "n", "dx", "dy", "M", "span", "run_start", "run_len", "n_runs",
        "gamma_out", "ll_out"]
    assert callable(hip.Context.mlpg_estep)
    assert list(inspect.signature(hip.Context.mlpg_estep).parameters)[1:] == [p.split()[-1].lstrip("*") for p in params][1:]
    makefile = open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\beaqhm_mlpg_em\.hip\b", makefile, re.M)
    assert re.search(r"^HDR\s*:=.*include/eaqhm_mlpg_em\.h\b", makefile, re.M) and "eaqhm_gmm_mfma.h" in makefile
    lib = hip.load_library()
    assert lib.eaqhm_mlpg_estep(*([None] * 8), 1, 1, 1, 1, 1, None, None, 0, None, None) == -1   # no context: no device


# ---- the recorded surface
def test_public_surface_is_unchanged():
    import eaqhm_amd
    from eaqhm_amd import convert
    assert not hasattr(eaqhm_amd, "conversion_trajectory_em") and not hasattr(eaqhm_amd, "check_em_arguments")
    assert callable(convert.conversion_trajectory_em) and callable(convert.check_em_arguments)
    api = json.load(open(os.path.join(ROOT, "tests", "golden", "python_api.json")))
    recorded = [v["conversion_trajectory"]["signature"] for v in api.values()
                if isinstance(v, dict) and "conversion_trajectory" in v]
    assert recorded and all(str(inspect.signature(eaqhm_amd.conversion_trajectory)) == s for s in recorded)
    assert eaqhm_amd.conversion_trajectory is convert.conversion_trajectory
    assert str(inspect.signature(convert.conversion_trajectory_em)) == (
        "(conv, C, *, em_iters=4, em_tol=0.0, em_trace=False, gv=None, gv_weight=1.0, gv_iters=30, trace=False, "
        "device_index=0)")
    src = open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "convert.py")).read()
    assert set(re.findall(r"^from \.(\w+) import", src, re.M)) == {"args", "records", "cepstrum", "align", "mixture",
                                                                   "dynamics", "mapping"}


# ---- the CLI
def dynamic_map_file(tmp_path, name="map.npz", static=False):
    from test_mlpg_cpu import host_dynamic_conversion, static_conversion
    extra = dict(lam=np.float64(2e-3), fs=np.int64(16000), src_f0=np.array([5.0, 0.2]), tgt_f0=np.array([5.3, 0.25]))
    path = os.path.join(tmp_path, name)
    if static:
        np.savez(path, order=np.int64(3), **extra, **static_conversion())
    else:
        np.savez(path, order=np.int64(2), **extra, **host_dynamic_conversion()[0])
    return path


def test_cli_flag(tmp_path):
    from eaqhm_amd import cli
    good = dynamic_map_file(tmp_path)
    a = cli.parser().parse_args(["x.wav", "--conversion", good, "--conversion-em-iters", "3"])
    assert a.conversion_em_iters == 3 and cli.parser().parse_args(["x.wav"]).conversion_em_iters is None
    static = dynamic_map_file(tmp_path, "static.npz", static=True)
    assert "span" not in cli.load_conversion(static)[0]
    for argv in (["x.wav", "--conversion-em-iters", "3"],
                 ["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz", "--conversion-em-iters", "3"],
                 ["x.wav", "--conversion", good, "--conversion-em-iters", "-1"],
                 ["x.wav", "--conversion", good, "--conversion-em-iters", "101"],
                 ["x.wav", "--conversion", good, "--conversion-em-iters", "2.5"],
                 ["x.wav", "--conversion", static, "--conversion-em-iters", "3"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    assert "--conversion-em-iters" in cli.__doc__ and "conversion_trajectory_em" in cli.__doc__


@pytest.mark.parametrize("flag", [None, 0, 5])
def test_cli_routes_the_conversion(tmp_path, monkeypatch, flag):
    """--conversion-em-iters K calls conversion_trajectory_em(em_iters=K) with the GV options; without the flag the CLI
    calls conversion_trajectory as before.  The analysis and the device functions are stand-ins."""
    from eaqhm_amd import cli, convert, model
    good = dynamic_map_file(tmp_path)
    n, L = 6, 200
    calls = []

    def model_parameters(det, fs, order=None, lam=5e-4, **kw):
        return dict(f0=np.full(n, 100.0), ceps=np.zeros((n, order + 1)), voiced=np.ones(n, bool), step=80, fs=fs)

    def plain(conv, C, **kw):
        calls.append(("trajectory", kw))
        return np.full((len(C), conv["dy"] // 2 + 1), -1.0)

    def refined(conv, C, **kw):
        calls.append(("em", kw))
        return np.full((len(C), conv["dy"] // 2 + 1), -1.0)
    monkeypatch.setattr(cli, "eaQHMAnalysisAndSynthesis", lambda path, gender, **o: (np.zeros(L), [1.0], {"who": path}, 0.0))
    monkeypatch.setattr(cli.wavfile, "read", lambda path: (16000, np.zeros(L)))
    monkeypatch.setattr(cli.wavfile, "write", lambda path, fs, x: None)
    monkeypatch.setattr(model, "model_parameters", model_parameters)
    monkeypatch.setattr(model, "unpack_model", lambda det: {"step": 80})
    monkeypatch.setattr(model, "eaQHMSynthesis", lambda det, fs, length, **kw: np.zeros(length))
    monkeypatch.setattr(convert, "conversion_trajectory", plain)
    monkeypatch.setattr(convert, "conversion_trajectory_em", refined)
    argv = ["x.wav", "--conversion", good] + ([] if flag is None else ["--conversion-em-iters", str(flag)])
    assert cli.main(argv) == 0
    assert calls == ([("trajectory", {})] if flag is None else [("em", dict(em_iters=flag))])
