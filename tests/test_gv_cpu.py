"""CPU tests of the global-variance term: the NumPy model's own properties on the inputs of the GPU tests
(tests/gv_ref.py), the host side of eaqhm_amd.convert (every new argument check, the statistics against hand values, the
map's two fields and the npz round trip), the new symbols and the CLI flags.  No GPU: the kernels are tested in
tests/test_gpu_gv.py.

What the model gave when these tests were written (cases A, B, C): the long-double trace's smallest step relative to its
value 1.6e-4, -2.4e-18, -2.0e-18 (flat columns: rounding); the float64 model 2.6e-15, 1.9e-14, 4.5e-14 from the long-double
one; the result without the term 4e13, 1e13, 7e12 times the GPU bar away."""
import os
import re

import numpy as np
import pytest

import gv_ref as V
import mlpg_ref as R
from conftest import ROOT
from test_mlpg_cpu import host_dynamic_conversion, static_conversion

LD = np.longdouble


@pytest.fixture()
def no_device(monkeypatch):
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


# ---- the model on the GPU tests' inputs
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_model_properties(name):
    c = V.case(name)
    (y64, t64, _), (yld, tld, _) = c["ref64"], c["refld"]
    for trace in (t64, tld):                                                          # (i) the objective does not fall
        assert np.all(np.diff(trace, axis=0) >= -4 * 2.0 ** -53 * np.abs(trace[1:])), name
    mu = c["gv_mean"]
    before, after = np.abs(V.variance(c["y_ml"]) - mu), np.abs(V.variance(y64) - mu)
    moved = before > 1e-9 * mu                                                        # (ii) v comes nearer to mu
    assert moved.sum() >= max(1, c["dy"] * 5 // 7) and np.all(after[moved] < before[moved])
    assert np.all(after[~moved] <= 1e-9 * mu[~moved])                                 # ... or stays on it
    bar_y, _ = V.bars(c)                                                              # (iii) the bar sees a missing term
    assert float(np.abs(y64 - c["nogv"][0]).max()) > 10 * bar_y
    assert np.abs(y64 - c["y_ml"]).max() > 1e-3                                       # and the ascent does something


def test_model_freezes_what_the_definition_freezes():
    c = V.case("D1")                                                                  # one row: N < 2
    Y, trace, _ = c["ref64"]
    assert np.array_equal(Y, c["y_ml"]) and np.all(trace == trace[0])
    c = V.case("F")                                                                   # a constant column
    Y, trace, _ = c["ref64"]
    assert np.array_equal(Y[:, 1], c["y_ml"][:, 1]) and np.all(trace[:, 1] == trace[0, 1])
    assert not np.array_equal(Y[:, 0], c["y_ml"][:, 0])
    c = V.case("H")                                                                   # no sweep: the scaled start
    Y, trace, _ = c["ref64"]
    assert trace.shape == (1, 5) and np.abs(V.variance(Y) - c["gv_mean"]).max() <= 1e-12 * c["gv_mean"].max()
    m0, m1 = c["y_ml"].mean(axis=0), Y.mean(axis=0)
    assert np.abs(m0 - m1).max() <= 1e-13 * np.abs(c["y_ml"]).max()                   # around the same mean
    c = V.case("E")                                                                   # rows outside the runs stay NaN
    live = ~np.isnan(c["y_ml"][:, 0])
    assert np.all(np.isnan(c["ref64"][0][~live])) and np.all(np.isfinite(c["ref64"][0][live]))
    assert V.case("G")["n"] == 2 * 64 + 37


def test_model_band_is_the_dense_system():
    c = V.case("G")
    y = np.random.default_rng(0).standard_normal((c["n"], c["dy"]))
    got = V.apply_R(c["sys64"], y)
    for s, T in zip(c["start"], c["length"]):
        for d in range(c["dy"]):
            Rm, q = R.system(c["P"][s:s + T], c["r"][s:s + T], c["span"], d)
            assert np.abs(got[s:s + T, d] - Rm @ y[s:s + T, d]).max() <= 1e-12 * np.abs(Rm).max() * np.abs(y).max()


# ---- the statistics
def test_global_variance_and_statistics_hand_values(no_device):
    from eaqhm_amd import global_variance, gv_statistics
    C = np.array([[-3.0, 1.0, 10.0], [-np.inf, 0.0, 0.0], [-1.0, 3.0, 10.0], [-2.0, 5.0, 40.0]])
    assert np.allclose(global_variance(C), [8.0 / 3.0, 200.0], rtol=1e-15)
    assert np.allclose(global_variance(C, level=True), [2.0 / 3.0, 8.0 / 3.0, 200.0], rtol=1e-15)
    assert global_variance(C).dtype == np.float64
    C2 = np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 4.0]])                                # variances 1 and 4
    s = gv_statistics([C, C2])
    assert set(s) == {"gv_mean", "gv_prec"}
    assert np.allclose(s["gv_mean"], [(8.0 / 3.0 + 1.0) / 2, 102.0], rtol=1e-15)
    assert np.allclose(s["gv_prec"], [1.0 / ((8.0 / 3.0 - 1.0) / 2) ** 2, 1.0 / 98.0 ** 2], rtol=1e-14)
    s = gv_statistics([C], rel_std=0.25)
    assert np.allclose(s["gv_mean"], [8.0 / 3.0, 200.0]) and np.allclose(s["gv_prec"], [1 / (2.0 / 3.0) ** 2, 1 / 2500.0])
    s = gv_statistics((C, C2), level=True, rel_std=10)
    assert s["gv_mean"].shape == (3,)
    for bad in (dict(utterances=[C]), dict(utterances=[]), dict(utterances=[C, C]), dict(utterances=[C, C2[:, :2]]),
                dict(utterances=[C], rel_std=0), dict(utterances=[C], rel_std=10.5), dict(utterances=[C], rel_std=-1),
                dict(utterances=[C], rel_std="a"), dict(utterances=[C], rel_std=np.nan), dict(utterances=5),
                dict(utterances=[C, C2], level=1), dict(utterances=[np.array([[0.0, 1.0], [0.0, 1.0]])], rel_std=0.2),
                dict(utterances=[C, np.array([[-np.inf, 0.0, 0.0]])]), dict(utterances=[C, np.zeros(3)])):
        with pytest.raises(ValueError):
            gv_statistics(bad.pop("utterances"), **bad)
    for bad in (np.array([[-np.inf, 0.0]]), np.zeros(3), np.full((2, 2), np.nan), np.zeros((2, 1))):
        with pytest.raises(ValueError):
            global_variance(bad)
    with pytest.raises(ValueError):
        global_variance(C, level=0)


# ---- the map and the arguments
def gv_for(conv, value=2.0):
    dys = int(conv["dy"]) // 2
    return dict(gv_mean=np.full(dys, value), gv_prec=np.full(dys, 1.0 / (0.25 * value) ** 2))


def test_map_fields_round_trip(tmp_path):
    from eaqhm_amd import check_conversion
    conv, _, _ = host_dynamic_conversion()
    plain = check_conversion(conv)
    assert "gv_mean" not in plain and "gv_prec" not in plain                          # without the fields: today's keys
    assert set(plain) == {"weights", "means", "covs", "zbar", "dx", "dy", "level", "A", "b", "Wx", "kx", "phi", "loglik", "n",
                          "span", "py"}
    gv = gv_for(conv)
    for fields, has in ((conv, False), (dict(conv, **gv), True)):
        path = os.path.join(tmp_path, "map%d.npz" % has)
        np.savez(path, **fields)
        with np.load(path, allow_pickle=False) as z:
            back = check_conversion({k: z[k] for k in z.files})
        assert ("gv_mean" in back) == has and ("gv_prec" in back) == has
        if has:
            assert np.array_equal(back["gv_mean"], gv["gv_mean"]) and np.array_equal(back["gv_prec"], gv["gv_prec"])
            assert back["gv_mean"].dtype == np.float64 and back["gv_mean"].shape == (2,)
            assert np.array_equal(check_conversion(back)["gv_prec"], gv["gv_prec"])   # the validated dict validates again
    from eaqhm_amd.convert import _CONVERSION_FIELDS
    assert "gv_mean" not in _CONVERSION_FIELDS and "span" not in _CONVERSION_FIELDS and len(_CONVERSION_FIELDS) == 14
    good = dict(conv, **gv)
    bad = [dict(good, gv_mean=gv["gv_mean"][:1]), dict(good, gv_prec=np.array([1.0, 0.0])),
           dict(good, gv_mean=np.array([1.0, -2.0])), dict(good, gv_mean=np.array([1.0, np.nan])),
           dict(good, gv_prec=np.array([np.inf, 1.0])), dict(good, gv_mean=np.array(["a", "b"])),
           dict(good, gv_mean=gv["gv_mean"][None]), dict(conv, gv_mean=gv["gv_mean"]), dict(conv, gv_prec=gv["gv_prec"]),
           dict(static_conversion(), gv_mean=np.ones(3), gv_prec=np.ones(3))]         # a static map: the fields need span
    for i, d in enumerate(bad):
        with pytest.raises(ValueError):
            check_conversion(d)
            print("case", i, "passed the check")


def test_argument_errors_come_before_device_work(no_device):
    from eaqhm_amd import check_conversion, check_gv_arguments, conversion_train, conversion_trajectory
    conv, _, CA = host_dynamic_conversion()
    gv = gv_for(conv)
    stored = dict(conv, **gv)
    v, vs = check_conversion(conv), check_conversion(stored)
    assert check_gv_arguments(v) == (None, 1.0, 30, False)
    assert check_gv_arguments(vs, gv=False)[0] is None and check_gv_arguments(v, gv=False)[0] is None
    s, w, k, tr = check_gv_arguments(vs, None, 2, 0, True)
    assert np.array_equal(s["gv_mean"], gv["gv_mean"]) and (w, k, tr) == (2.0, 0, True) and isinstance(k, int)
    other = gv_for(conv, 3.0)
    assert np.array_equal(check_gv_arguments(vs, other)[0]["gv_mean"], other["gv_mean"])   # a dict overrides the map
    assert check_gv_arguments(v, other, 1e-6, 10000)[1:3] == (1e-6, 10000)
    for kw in (dict(gv=True), dict(gv=dict(gv_mean=np.ones(2))), dict(gv=dict(gv_mean=np.ones(3), gv_prec=np.ones(3))),
               dict(gv=dict(gv_mean=np.zeros(2), gv_prec=np.ones(2))), dict(gv=5), dict(gv="yes"),
               dict(gv_weight=0), dict(gv_weight=1e-7), dict(gv_weight=1e7), dict(gv_weight=np.nan), dict(gv_weight="a"),
               dict(gv_iters=-1), dict(gv_iters=10001), dict(gv_iters=2.5), dict(gv_iters="a"), dict(trace=1),
               dict(trace="yes")):
        with pytest.raises(ValueError):
            check_gv_arguments(vs, **kw)
        with pytest.raises(ValueError):
            conversion_trajectory(stored, CA, **kw)
    with pytest.raises(ValueError):                                                   # a trace of nothing
        conversion_trajectory(conv, CA, trace=True)
    with pytest.raises(ValueError):
        conversion_trajectory(stored, CA, gv=False, trace=True)
    with pytest.raises(ValueError):
        check_gv_arguments(check_conversion(static_conversion()), gv=other)
    with pytest.raises(ValueError, match="conversion_apply"):
        conversion_trajectory(static_conversion(), np.zeros((3, 4)), gv=other)
    with pytest.raises(AssertionError, match="device work"):                           # good arguments reach the device
        conversion_trajectory(stored, CA, gv_weight=2.0, gv_iters=5, trace=True)
    empty = np.array([[-np.inf, 0, 0]] * 2)                                            # only empty rows: no device work
    out, trace = conversion_trajectory(stored, empty, gv_iters=3, trace=True)
    assert out.shape == (2, 3) and np.all(np.isneginf(out[:, 0])) and trace.shape == (4, 2) and np.all(trace == 0)
    rng = np.random.default_rng(1)
    X, Y = rng.standard_normal((50, 6)), rng.standard_normal((50, 8))                 # dynamic rows: 3 mapped static columns in Y
    tgv = dict(gv_mean=np.ones(3), gv_prec=np.ones(3))
    for kw in (dict(gv=tgv), dict(span=2, gv=dict(gv_mean=np.ones(4), gv_prec=np.ones(4))),
               dict(span=2, gv=dict(gv_mean=np.ones(3))), dict(span=2, gv=dict(gv_mean=np.ones(3), gv_prec=-np.ones(3))),
               dict(span=2, gv=7)):
        with pytest.raises(ValueError):
            conversion_train(X, Y, 2, **kw)
    with pytest.raises(AssertionError, match="device work"):
        conversion_train(X, Y, 2, span=2, gv=tgv)
    with pytest.raises(AssertionError, match="device work"):                           # level=True: 4 static columns
        conversion_train(X, Y, 2, span=2, level=True, gv=dict(gv_mean=np.ones(4), gv_prec=np.ones(4)))


def test_sizes_mirror_the_library():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import convert, hip
    lib = hip.load_library()
    for n in (1, 63, 64, 65, 165, 32768, 32769, 60000, 10 ** 6, 2 ** 31):
        rows = convert.gv_chunk_rows(n)
        assert lib.eaqhm_gv_chunk_rows(n) == rows and rows % 64 == 0 and -(-n // rows) <= 512
        for dy, span in ((1, 1), (17, 2), (24, 2), (64, 8)):
            assert lib.eaqhm_gv_work_len(n, dy, span) == convert.gv_work_len(n, dy, span), (n, dy, span)
    assert convert.gv_chunk_rows(165) == 64 and convert.gv_chunk_rows(60000) == 128
    for n, dy, span in ((0, 1, 1), (1, 0, 1), (1, 65, 1), (1, 1, 0), (1, 1, 9), (2 ** 31 + 1, 1, 1), (-1, 1, 1)):
        assert lib.eaqhm_gv_work_len(n, dy, span) == -1, (n, dy, span)
    assert lib.eaqhm_gv_chunk_rows(0) == -1 and lib.eaqhm_gv_chunk_rows(2 ** 31 + 1) == -1


# ---- symbols
GV_ARGUMENT_COUNTS = dict(eaqhm_gv_chunk_rows=1, eaqhm_gv_work_len=3, eaqhm_gv_ascend=15)


def test_symbols():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    bound = {name: len(args) for name, _, args in hip.SYMBOLS_GV}
    assert not set(bound) & {name for name, _, _ in hip.SYMBOLS + hip.SYMBOLS_MLPG}     # a table of their own
    header = open(os.path.join(ROOT, "include", "eaqhm_gv.h")).read()
    assert '#include "eaqhm_gv.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(bound) == set(GV_ARGUMENT_COUNTS)
    for name, n in GV_ARGUMENT_COUNTS.items():
        assert bound[name] == n, name
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
    for name in ("gv_chunk_rows", "gv_work_len", "gv_ascend"):
        assert callable(getattr(hip.Context, name))
    lib = hip.load_library()
    assert lib.eaqhm_gv_ascend(None, None, None, 1, 1, 1, None, None, 0, None, None, 1, None, None, None) == -1
    makefile = open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "Makefile")).read()
    assert "eaqhm_gv.hip" in makefile and "eaqhm_gv.h" in makefile


# ---- the CLI
def saved_map(tmp_path, name, with_gv):
    conv, _, _ = host_dynamic_conversion()
    if with_gv:
        conv = dict(conv, **gv_for(conv))
    path = os.path.join(tmp_path, name)
    np.savez(path, order=np.int64(2), lam=np.float64(2e-3), fs=np.int64(16000), src_f0=np.array([5.0, 0.2]),
             tgt_f0=np.array([5.3, 0.25]), **conv)
    return path


def test_cli_flags(tmp_path):
    from eaqhm_amd import cli
    train = ["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz"]
    a = cli.parser().parse_args(train + ["--conversion-span", "2", "--conversion-gv"])
    assert a.conversion_gv == 0.25
    a = cli.parser().parse_args(train + ["--conversion-span", "2", "--conversion-gv", "0.1"])
    assert a.conversion_gv == 0.1
    a = cli.parser().parse_args(["x.wav"])
    assert a.conversion_gv is None and a.conversion_no_gv is False and a.conversion_gv_iters is None \
        and a.conversion_gv_weight is None
    a = cli.parser().parse_args(["x.wav", "--conversion", "m.npz", "--conversion-gv-iters", "5", "--conversion-gv-weight", "2"])
    assert (a.conversion_gv_iters, a.conversion_gv_weight) == (5, 2.0)
    assert cli.gv_options(a) == dict(gv_iters=5, gv_weight=2.0)
    assert cli.gv_options(cli.parser().parse_args(["x.wav", "--conversion", "m.npz", "--conversion-no-gv"])) == dict(gv=False)
    assert cli.gv_options(cli.parser().parse_args(["x.wav", "--conversion", "m.npz"])) == {}
    with_gv, without = saved_map(tmp_path, "gv.npz", True), saved_map(tmp_path, "plain.npz", False)
    assert "gv_mean" in cli.load_conversion(with_gv)[0] and "gv_mean" not in cli.load_conversion(without)[0]
    use = ["x.wav", "--conversion", with_gv]
    for argv in (["x.wav", "--conversion-gv"], train + ["--conversion-gv"], use + ["--conversion-gv"],
                 train + ["--conversion-span", "2", "--conversion-gv", "0"],
                 train + ["--conversion-span", "2", "--conversion-gv", "11"],
                 train + ["--conversion-span", "2", "--conversion-gv", "a"],
                 ["x.wav", "--conversion-no-gv"], ["x.wav", "--conversion-gv-iters", "5"],
                 ["x.wav", "--conversion-gv-weight", "2"], train + ["--conversion-span", "2", "--conversion-no-gv"],
                 train + ["--conversion-span", "2", "--conversion-gv", "--conversion-gv-iters", "5"],
                 use + ["--conversion-no-gv", "--conversion-gv-iters", "5"],
                 use + ["--conversion-no-gv", "--conversion-gv-weight", "2"],
                 use + ["--conversion-gv-iters", "-1"], use + ["--conversion-gv-iters", "10001"],
                 use + ["--conversion-gv-iters", "1.5"], use + ["--conversion-gv-weight", "0"],
                 use + ["--conversion-gv-weight", "1e7"], use + ["--conversion-gv-weight", "nan"],
                 ["x.wav", "--conversion", without, "--conversion-no-gv"],
                 ["x.wav", "--conversion", without, "--conversion-gv-iters", "5"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    for flag in ("--conversion-gv", "--conversion-no-gv", "--conversion-gv-iters", "--conversion-gv-weight"):
        assert flag in cli.__doc__
    assert "gv_statistics" in cli.__doc__


def run_cli(tmp_path, monkeypatch, argv_tail, with_gv=True):
    """cli.main on a saved map with stand-ins for the analysis and the device functions: the calls they saw."""
    from eaqhm_amd import cli, convert, model
    good = saved_map(tmp_path, "map.npz", with_gv)
    n, L = 6, 200
    calls = []

    def model_parameters(det, fs, order=None, lam=5e-4, **kw):
        return dict(f0=np.full(n, 100.0), ceps=np.zeros((n, order + 1)), voiced=np.ones(n, bool), step=80, fs=fs)

    def trajectory(conv, C, **kw):
        calls.append(("trajectory", "gv_mean" in conv, kw))
        return np.full((len(C), conv["dy"] // 2 + 1), -1.0)

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
    assert cli.main(["x.wav", "--conversion", good] + argv_tail) == 0
    return calls


def test_cli_dispatch(tmp_path, monkeypatch):
    assert run_cli(tmp_path, monkeypatch, []) == [("trajectory", True, {}), ("synth", (6, 3))]
    assert run_cli(tmp_path, monkeypatch, ["--conversion-no-gv"])[0] == ("trajectory", True, dict(gv=False))
    assert run_cli(tmp_path, monkeypatch, ["--conversion-gv-iters", "7", "--conversion-gv-weight", "0.5"])[0] \
        == ("trajectory", True, dict(gv_iters=7, gv_weight=0.5))
    assert run_cli(tmp_path, monkeypatch, [], with_gv=False)[0] == ("trajectory", False, {})


def test_cli_training_stores_the_statistics(tmp_path, monkeypatch):
    """--conversion-gv S hands gv_statistics([C_target], rel_std=S) to conversion_train, and MAP.npz carries the fields."""
    from eaqhm_amd import cli, convert, model
    conv, _, _ = host_dynamic_conversion()
    n = 12
    rng = np.random.default_rng(5)
    C_t = np.hstack((np.full((n, 1), -2.0), rng.standard_normal((n, 2))))
    seen = {}

    def train(X, Y, components, **kw):
        seen.update(kw)
        return dict(conv, **kw["gv"]) if kw.get("gv") is not None else dict(conv)
    monkeypatch.setattr(model, "model_parameters", lambda det, fs, order=None, lam=5e-4, **kw: dict(
        f0=np.full(n, 100.0), ceps=np.zeros((n, 3)), voiced=np.ones(n, bool), step=80, fs=fs))
    monkeypatch.setattr(cli, "align_other", lambda *a, **k: (C_t, np.zeros((n, 2), dtype=np.int64), {}, None))
    monkeypatch.setattr(convert, "conversion_pairs", lambda CA, CB, path, span=None, **k: (np.zeros((n, 6)), np.zeros((n, 6))))
    monkeypatch.setattr(convert, "conversion_train", train)
    out = os.path.join(tmp_path, "m.npz")
    a = cli.parser().parse_args(["x.wav", "--conversion-train", "t.wav", "--conversion-save", out, "--conversion-span", "2",
                                 "--conversion-gv", "0.5"])
    cli.train_conversion(a, "male", {}, 16000, {})
    ref = convert.gv_statistics([C_t], rel_std=0.5)
    assert seen["span"] == 2 and np.array_equal(seen["gv"]["gv_mean"], ref["gv_mean"])
    assert np.array_equal(seen["gv"]["gv_prec"], ref["gv_prec"])
    loaded = cli.load_conversion(out)[0]
    assert np.array_equal(loaded["gv_mean"], ref["gv_mean"]) and np.array_equal(loaded["gv_prec"], ref["gv_prec"])
    a = cli.parser().parse_args(["x.wav", "--conversion-train", "t.wav", "--conversion-save", out, "--conversion-span", "2"])
    cli.train_conversion(a, "male", {}, 16000, {})
    assert seen["gv"] is None and "gv_mean" not in cli.load_conversion(out)[0]
