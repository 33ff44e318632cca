"""CPU tests of the spectral conversion: the NumPy model's own properties (tests/gmm_ref.py), the host
side of eaqhm_amd.convert (initialisation, pairing, pitch statistics, every argument check, the npz round trip), the
symbols and the CLI flags.  No GPU: the device steps are tested in tests/test_gpu_gmm.py.

What the model gave when these tests were written (float64 against long double after 10 rounds, tol never reached):
weights <= 6.0e-16, means <= 8.2e-15, covariances <= 3.3e-13, log-likelihood <= 3.5e-11 (the 400 x (64 + 64) set; <=
1.8e-12 on the others); the smallest step of the log-likelihood was -1.2e-15 (rounding on a converged separated set).
The conversion of the separated sets had an rms error of 0.993 and 0.994 sigma, 0.027 and 0.039 of a global linear
regression's."""
import os
import re

import numpy as np
import pytest

import gmm_ref as R
from conftest import ROOT, record_measurement


@pytest.fixture(scope="module")
def fits():
    """Every data set of the issue's table fitted once by the model in float64 and long double, 10 rounds each."""
    out = {}
    for name, N, d, M, *_ in R.CASES:
        X, Y, labels, M = R.case(name)
        Z = np.hstack((X, Y))
        out[name] = (X, Y, Z, M, R.fit(Z, M, iters=10, tol=-1.0, split=d),
                     R.fit(Z, M, iters=10, tol=-1.0, split=d, dtype=np.longdouble))
    return out


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_model_properties(fits, name):
    X, Y, Z, M, f, g = fits[name]
    steps = np.diff(f["loglik"])
    assert len(f["loglik"]) == 10 and steps.min() >= -1e-12, steps
    # gamma = exp(lp - ll): ll and lp - ll are each rounded once at the size of |ll| (where gamma is not negligible,
    # |lp| <= |ll| + 40), exp adds an ulp or two per term and the sum M more
    assert np.all(np.abs(f["gamma"].sum(axis=1) - 1.0) <= 2.0 ** -52 * (M + 4 + 2 * (np.abs(f["ll"]) + 40)))
    assert abs(f["weights"].sum() - 1.0) <= M * 2.0 ** -52
    for S in f["covs"]:
        assert np.array_equal(S, S.T)
        assert np.linalg.eigvalsh(S).min() > 0
    diff = {k: float(np.abs(f[k] - g[k]).max()) for k in ("weights", "means", "covs", "loglik")}
    record_measurement("gmm_model_f64_vs_longdouble_" + name, min_step=float(steps.min()), **diff)
    # rounding is not amplified by the iteration: generous multiples of the figures in the docstring
    assert diff["weights"] <= 1e-13 and diff["means"] <= 1e-12 and diff["covs"] <= 1e-10 and diff["loglik"] <= 1e-8


def test_soft_case_is_soft(fits):
    """The 257 x (1 + 1) set exercises soft responsibilities: most rows belong to both components."""
    f = fits["ovl_257x1"][4]
    assert np.mean(f["gamma"].max(axis=1) < 0.99) > 0.5


@pytest.mark.parametrize("name", ["sep_600x3", "sep_1500x8"])
def test_model_learns_the_map(fits, name):
    """The figures the GPU test relies on: rms error about sigma, far below a global linear regression's."""
    X, Y, Z, M, f, _ = fits[name]
    rms = float(np.sqrt(np.mean((R.convert(f, X.shape[1], X) - Y) ** 2)))
    Xa = np.hstack((X, np.ones((len(X), 1))))
    lin = float(np.sqrt(np.mean((Xa @ np.linalg.lstsq(Xa, Y, rcond=None)[0] - Y) ** 2)))
    record_measurement("gmm_model_conversion_" + name, rms_over_sigma=rms / R.SIGMA, rms_over_linear=rms / lin)
    assert 0.95 * R.SIGMA <= rms <= 1.05 * R.SIGMA
    assert rms <= 0.05 * lin


def test_row_algebra_matches_lapack():
    rng = np.random.default_rng(3)
    B = rng.standard_normal((40, 17))
    S = B.T @ B + 0.1 * np.eye(17)
    L = R.cholesky(S)
    assert np.abs(L - np.linalg.cholesky(S)).max() < 1e-12
    assert np.abs(R.tri_inverse(L) @ L - np.eye(17)).max() < 1e-12
    assert R.cholesky(S.astype(np.longdouble)).dtype == np.longdouble
    with pytest.raises(np.linalg.LinAlgError):
        R.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]]))


# ---- the host side of the package
@pytest.fixture()
def no_device(monkeypatch):
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


def test_initialisation():
    from eaqhm_amd.convert import check_gmm_arguments, gmm_init_labels
    for name, N, d, M, *_ in R.CASES:
        X = R.case(name)[0]
        lab = gmm_init_labels(X, M)
        assert np.array_equal(lab, gmm_init_labels(X.copy(), M))                    # deterministic
        assert np.array_equal(lab, R.init_labels(X, M))                              # the model's
        count = np.bincount(lab, minlength=M)
        assert count.min() >= 1 and count.max() - count.min() <= 1
    X = R.case("sep_600x3")[0]
    init = np.arange(600) % 3
    assert np.array_equal(check_gmm_arguments(X, 3, init=init)[5], init)             # an explicit init is kept as it is
    zbar, c, phi = R.centre(X)
    w, mu, _ = R.mstep(c, R.one_hot(init, 3), phi)                                   # the first M-step sees those labels
    assert np.array_equal(w, np.full(3, 200.0) / 600.0)
    assert np.allclose(mu + zbar, np.stack([X[init == m].mean(axis=0) for m in range(3)]), atol=1e-12)
    # the sign rule: the mirrored data gives the mirrored order
    x = np.linspace(-1.0, 2.0, 10)[:, None]
    assert np.array_equal(gmm_init_labels(x, 2), np.repeat([0, 1], 5))


def test_chunking_and_work_len():
    from eaqhm_amd.convert import gmm_chunk_rows, gmm_work_len
    from eaqhm_amd.hip import load_library
    lib = load_library()
    assert gmm_chunk_rows(1) == gmm_chunk_rows(65536) == 512 and gmm_chunk_rows(65537) == 576
    assert gmm_chunk_rows(10 ** 6) == 7872
    assert gmm_work_len(10 ** 6, 128, 64) * 8 < 10 ** 9
    for N, D, M in ((1, 1, 1), (513, 37, 5), (10 ** 6, 128, 64), (70000, 36, 8), (512, 15, 64), (1027, 16, 2)):
        assert lib.eaqhm_gmm_work_len(N, D, M) == gmm_work_len(N, D, M), (N, D, M)
    for N, D, M in ((0, 1, 1), (1, 0, 1), (1, 129, 1), (1, 1, 0), (1, 1, 65), (2 ** 36 + 1, 1, 1)):
        assert lib.eaqhm_gmm_work_len(N, D, M) == -1, (N, D, M)


def test_conversion_pairs():
    from eaqhm_amd.convert import conversion_pairs
    CA = np.arange(12.0).reshape(4, 3)
    CB = 100.0 + np.arange(10.0).reshape(5, 2)
    CA[1] = (-np.inf, 0, 0)
    CB[3] = (-np.inf, 0)
    path = np.array([[0, 0], [1, 1], [2, 2], [2, 3], [3, 4]])
    X, Y = conversion_pairs(CA, CB, path)
    assert np.array_equal(X, CA[[0, 2, 3]]) and np.array_equal(Y, CB[[0, 2, 4]])
    for bad in (np.array([[0, 0], [1, 1]]), np.array([[0, 0], [1, 1], [2, 2], [3, 5]]), np.zeros((4, 3), dtype=int),
                np.array([[0.0, 0.0]])):
        with pytest.raises(ValueError):
            conversion_pairs(CA, CB, bad)
    with pytest.raises(ValueError):
        conversion_pairs(np.full((4, 3), np.nan), CB, path)


def test_pitch_statistics_and_contour():
    from eaqhm_amd.convert import f0_statistics, pitch_conversion_contour
    from eaqhm_amd.model import SCALE_RANGE
    f0 = np.array([100.0, 0.0, 200.0, 400.0, 0.0])
    vo = np.array([1, 0, 1, 1, 0], dtype=bool)
    m, s = f0_statistics(f0, vo)
    lf = np.log([100.0, 200.0, 400.0])
    assert m == pytest.approx(lf.mean(), abs=1e-15) and s == pytest.approx(lf.std(), abs=1e-15)
    same = pitch_conversion_contour(f0, vo, (m, s), (m, s))
    assert np.allclose(same, 1.0, atol=1e-14) and np.all(same[~vo] == 1.0)
    up = pitch_conversion_contour(f0, vo, (m, s), (m + np.log(1.5), s))
    assert np.allclose(up[vo], 1.5) and np.all(up[~vo] == 1.0)
    flat = pitch_conversion_contour(f0, vo, (m, s), (m, 0.0))                        # every voiced instant to exp(m) = 200
    assert np.allclose(flat * np.where(vo, f0, 1.0), np.where(vo, 200.0, 1.0))
    far = pitch_conversion_contour(f0, vo, (m, s), (m + 5.0, s))
    assert np.all(far[vo] == SCALE_RANGE[1]) and np.all(far[~vo] == 1.0)
    low = pitch_conversion_contour(f0, vo, (m, s), (m - 5.0, s))
    assert np.all(low[vo] == SCALE_RANGE[0])
    assert np.all(pitch_conversion_contour(f0, vo, (m, 0.0), (m, s)) == pitch_conversion_contour(f0, vo, (m, 1.0), (m, 1.0)))
    for bad in ((f0, vo[:4]), (f0, np.ones(5, dtype=bool)), ([[1.0]], [[True]]), (f0, np.zeros(5, dtype=bool))):
        with pytest.raises(ValueError):
            f0_statistics(*bad)
    for bad in ((m, -1.0), (np.nan, 1.0), "ab", (1.0,)):
        with pytest.raises(ValueError):
            pitch_conversion_contour(f0, vo, bad, (m, s))


def test_gmm_argument_errors(no_device):
    from eaqhm_amd import gmm_fit
    Z = np.random.default_rng(0).standard_normal((40, 4))
    bad_Z = Z.copy()
    bad_Z[3, 1] = np.nan
    inf_Z = Z.copy()
    inf_Z[0, 0] = np.inf
    cases = [dict(Z=bad_Z), dict(Z=inf_Z), dict(Z=Z[:, 0]), dict(Z=np.zeros((40, 129))), dict(Z=np.zeros((40, 0))),
             dict(Z=Z.astype(complex)), dict(Z=[["a"]]), dict(components=0), dict(components=65), dict(components=2.5),
             dict(components=True), dict(components=21), dict(iters=0), dict(iters=1001), dict(iters=1.5),
             dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf), dict(tol="x"), dict(floor=1e-13), dict(floor=0.2),
             dict(floor=np.nan), dict(init=np.zeros(39, dtype=int)), dict(init=np.zeros(40)),
             dict(init=np.zeros(40, dtype=int)), dict(init=np.full(40, 2)), dict(init=-np.ones(40, dtype=int)),
             dict(split=0), dict(split=5), dict(split=1.5)]
    for kw in cases:
        args = dict(Z=Z, components=2)
        args.update(kw)
        with pytest.raises(ValueError):
            gmm_fit(args.pop("Z"), args.pop("components"), **args)
    with pytest.raises(AssertionError, match="device work"):                           # good arguments reach the device
        gmm_fit(Z, 2)


def test_conversion_argument_errors(no_device):
    from eaqhm_amd import conversion_apply, conversion_train, gmm_posteriors
    rng = np.random.default_rng(1)
    X, Y = rng.standard_normal((50, 5)), rng.standard_normal((50, 7))
    for kw in (dict(Y=Y[:49]), dict(X=X[:, :1]), dict(Y=Y[:, :1]), dict(level=1), dict(level="yes"),
               dict(X=np.zeros((50, 66))), dict(components=26), dict(components=0), dict(iters=0), dict(floor=1.0),
               dict(tol=-1.0), dict(init=np.zeros(50, dtype=int)), dict(X=np.where(X > 2.5, np.nan, X) * np.nan)):
        args = dict(X=X, Y=Y, components=2)
        args.update(kw)
        with pytest.raises(ValueError):
            conversion_train(args.pop("X"), args.pop("Y"), args.pop("components"), **args)
    for level in (False, True):                                            # cepstral rows: 2 to 64 columns
        with pytest.raises(ValueError):
            conversion_train(np.zeros((300, 65)), np.zeros((300, 64)), 2, level=level)
        with pytest.raises(ValueError):
            conversion_train(np.zeros((300, 2)), np.zeros((300, 1)), 2, level=level)
    with pytest.raises(AssertionError, match="device work"):                           # 64 columns pass the checks
        conversion_train(rng.standard_normal((300, 64)), rng.standard_normal((300, 64)), 2, level=True)
    conv = host_conversion()
    for C in (np.zeros((3, 5)), np.full((3, 4), np.nan), np.zeros(4)):
        with pytest.raises(ValueError):
            conversion_apply(conv, C)
    with pytest.raises(ValueError):
        gmm_posteriors(conv, np.zeros((3, 5)))
    with pytest.raises(ValueError):
        gmm_posteriors(conv, np.full((3, 6), np.inf))
    out = conversion_apply(conv, np.array([[-np.inf, 0, 0, 0]] * 2))                   # only empty rows: no device work
    assert out.shape == (2, 4) and np.all(np.isneginf(out[:, 0])) and np.all(out[:, 1:] == 0)
    with pytest.raises(AssertionError, match="device work"):
        conversion_apply(conv, np.zeros((3, 4)))


def host_conversion(level=False):
    """A conversion dict as conversion_train builds it, from the model's fit (no device): 3 + 3 mapped columns."""
    from eaqhm_amd.convert import gmm_conversion_parameters
    X, Y, _, M = R.case("sep_600x3")
    f = R.fit(np.hstack((X, Y)), M, iters=4, split=3)
    A, b, Wx, kx = gmm_conversion_parameters(f["weights"], f["means"] - f["zbar"], f["covs"], 3)
    return dict(weights=f["weights"], means=f["means"], covs=f["covs"], zbar=f["zbar"], phi=f["phi"],
                loglik=f["loglik"], n=np.int64(f["n"]), dx=np.int64(3), dy=np.int64(3), level=np.bool_(level), A=A, b=b,
                Wx=Wx, kx=kx)


def test_conversion_parameters_match_the_model():
    conv = host_conversion()
    mu_c = conv["means"] - conv["zbar"]
    A, b, Wx, kx = R.conversion(conv["weights"], mu_c, conv["covs"], 3)
    for got, want in ((conv["A"], A), (conv["b"], b), (conv["Wx"], Wx), (conv["kx"], kx)):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    for m in range(3):                                                                 # A Sigma_xx = Sigma_yx
        assert np.abs(conv["A"][m] @ conv["covs"][m, :3, :3] - conv["covs"][m, 3:, :3]).max() < 1e-12


def test_npz_round_trip_and_check_conversion(tmp_path):
    from eaqhm_amd import check_conversion
    conv = host_conversion()
    path = os.path.join(tmp_path, "map.npz")
    np.savez(path, **conv)
    with np.load(path, allow_pickle=False) as z:
        back = check_conversion({k: z[k] for k in z.files})
    assert back["dx"] == 3 and back["dy"] == 3 and back["level"] is False and back["n"] == 600
    for k in ("weights", "means", "covs", "zbar", "phi", "A", "b", "Wx", "kx", "loglik"):
        assert np.array_equal(back[k], conv[k]), k

    def broken(**kw):
        d = dict(conv)
        d.update(kw)
        return d
    asym = conv["covs"].copy()
    asym[0, 0, 1] += 1e-12
    full = conv["Wx"].copy()
    full[0, 0, 1] = 1e-3
    bad = [broken(weights=conv["weights"] * 1.001), broken(weights=-conv["weights"]), broken(covs=asym),
           broken(means=conv["means"][:, :5]), broken(A=conv["A"][:, :2]), broken(b=conv["b"][:, :2]), broken(Wx=full),
           broken(kx=np.full(3, np.nan)), broken(dx=np.int64(2)), broken(dx=np.int64(0)), broken(dy=np.int64(65)),
           broken(zbar=np.zeros(5)), broken(weights=np.array(["a", "b", "c"])), broken(phi=np.zeros(2)),
           broken(covs=conv["covs"] - 10.0 * np.eye(6)), {k: v for k, v in conv.items() if k != "kx"}, None, 3]
    for i, d in enumerate(bad):
        with pytest.raises(ValueError):
            check_conversion(d)
            print("case", i, "passed the check")


# ---- symbols
PARENT_ARGUMENT_COUNTS = dict(
    eaqhm_ctx_create=2, eaqhm_ctx_destroy=1, eaqhm_set_stream=2, eaqhm_sync=1, eaqhm_last_error=1, eaqhm_set_option=3,
    eaqhm_debug_read=2, eaqhm_device_info=2, eaqhm_ls_faults=2, eaqhm_frame_prep=12, eaqhm_ls_batch=27,
    eaqhm_ls_explicit=11, eaqhm_phase_integrate=8, eaqhm_spline_solve=7, eaqhm_spline_solve_range=9, eaqhm_eval_synth=23,
    eaqhm_eval_partials_len=3, eaqhm_modify_prep=15, eaqhm_modify_synth=23, eaqhm_model_envelope=8,
    eaqhm_noise_analyse=7, eaqhm_noise_synth=18, eaqhm_noise_warp=8, eaqhm_noise_envelope=9, eaqhm_noise_modulation=13,
    eaqhm_modify_amp_warp=10, eaqhm_model_envelope_warp=10, eaqhm_noise_warp_map=10, eaqhm_noise_envelope_map=11,
    eaqhm_model_cepstrum=8, eaqhm_modify_amp_cepstrum=13, eaqhm_cepstrum_envelope=12, eaqhm_cepstrum_cost=10,
    eaqhm_dtw=9, eaqhm_model_build=13, eaqhm_cepstrum_phase=12, eaqhm_noise_cepstrum=7, eaqhm_noise_from_cepstrum=7)
NEW_ARGUMENT_COUNTS = dict(eaqhm_gmm_estep=10, eaqhm_gmm_mstep=10, eaqhm_gmm_regress=10, eaqhm_gmm_work_len=3)


def test_symbols():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    bound = {name: len(args) for name, _, args in hip.SYMBOLS}
    for name, n in PARENT_ARGUMENT_COUNTS.items():
        assert bound[name] == n, name                                                  # no existing list changed
    for name, n in NEW_ARGUMENT_COUNTS.items():
        assert bound[name] == n, name
    assert set(bound) == set(PARENT_ARGUMENT_COUNTS) | set(NEW_ARGUMENT_COUNTS)
    header = open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    for name, n in NEW_ARGUMENT_COUNTS.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
    for name in ("gmm_estep", "gmm_mstep", "gmm_regress", "gmm_work_len"):
        assert callable(getattr(hip.Context, name))
    lib = hip.load_library()
    for name in NEW_ARGUMENT_COUNTS:
        assert getattr(lib, name) is not None
    makefile = open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "Makefile")).read()
    assert "eaqhm_gmm.hip" in makefile


# ---- the CLI
def test_cli_flags(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz",
                                 "--conversion-components", "4"])
    assert (a.conversion_train, a.conversion_save, a.conversion_components, a.conversion) == ("t.wav", "m.npz", 4, None)
    assert cli.parser().parse_args(["x.wav", "--conversion", "m.npz"]).conversion == "m.npz"
    good = os.path.join(tmp_path, "map.npz")
    np.savez(good, order=np.int64(3), lam=np.float64(5e-4), fs=np.int64(16000), src_f0=np.array([5.0, 0.2]),
             tgt_f0=np.array([5.3, 0.25]), **host_conversion())
    conv, order, lam, fs, src, tgt = cli.load_conversion(good)
    assert (order, lam, fs, src, tgt) == (3, 5e-4, 16000, (5.0, 0.2), (5.3, 0.25)) and conv["dx"] == 3
    for argv in (["x.wav", "--conversion-train", "t.wav"], ["x.wav", "--conversion-save", "m.npz"],
                 ["x.wav", "--conversion-components", "4"],
                 ["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz", "--conversion-components", "65"],
                 ["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz", "--conversion", good],
                 ["x.wav", "--conversion", good, "--envelope-from", "o.wav"],
                 ["x.wav", "--conversion", good, "--no-envelope"],
                 ["x.wav", "--conversion", good, "--cepstral-envelope", "5"],
                 ["x.wav", "--conversion", good, "--cepstral-lambda", "1e-3"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    with pytest.raises(ValueError):
        cli.main(["x.wav", "--conversion", os.path.join(tmp_path, "missing.npz")])
    short = os.path.join(tmp_path, "short.npz")
    np.savez(short, **host_conversion())                                               # a bare map: no order, fs, f0
    with pytest.raises(ValueError):
        cli.main(["x.wav", "--conversion", short])


def test_cli_conversion_keeps_the_alignment_settings(tmp_path, monkeypatch):
    """--conversion MAP with --timing-from OTHER: the two alignment cepstra are fitted with the same order and lambda
    (this file's flags or defaults), whatever order and lambda the map was trained at; only the rows that are converted
    use the map's.  The analysis and the device functions are stand-ins that record their arguments."""
    from eaqhm_amd import cli, convert, model
    good = os.path.join(tmp_path, "map.npz")
    np.savez(good, order=np.int64(3), lam=np.float64(2e-3), fs=np.int64(16000), src_f0=np.array([5.0, 0.2]),
             tgt_f0=np.array([5.3, 0.25]), **host_conversion())
    n, L = 6, 200
    calls = dict(cepstrum=[], parameters=[], align=[], apply=[], synth=[])

    def analysis(path, gender, **options):
        return np.zeros(L), [1.0], {"who": path}, 0.0

    def model_cepstrum(det, fs, order=None, lam=5e-4, **kw):
        calls["cepstrum"].append((det["who"], order, lam))
        return np.zeros((n, (order or 18) + 1))

    def model_parameters(det, fs, order=None, lam=5e-4, **kw):
        calls["parameters"].append((det["who"], order, lam))
        return dict(f0=np.full(n, 100.0), ceps=np.zeros((n, order + 1)), voiced=np.ones(n, bool), step=80, fs=fs)

    def model_align(CA, CB, band=None, **kw):
        calls["align"].append((CA.shape, CB.shape))
        assert CA.shape[1] == CB.shape[1], "the two sides of the alignment have different orders"
        return np.stack((np.arange(n), np.arange(n)), axis=1), 0.0

    def conversion_apply(conv, C, **kw):
        calls["apply"].append(C.shape)
        return np.full((len(C), conv["dy"] + 1), -1.0)

    def synthesis(det, fs, length, **kw):
        calls["synth"].append((kw["envelope"].shape, np.shape(kw["time_scale"]), np.shape(kw["pitch_scale"])))
        return np.zeros(length)
    monkeypatch.setattr(cli, "eaQHMAnalysisAndSynthesis", analysis)
    monkeypatch.setattr(cli.wavfile, "read", lambda path: (16000, np.zeros(L)))
    monkeypatch.setattr(cli.wavfile, "write", lambda path, fs, x: None)
    monkeypatch.setattr(model, "model_cepstrum", model_cepstrum)
    monkeypatch.setattr(model, "model_parameters", model_parameters)
    monkeypatch.setattr(model, "model_align", model_align)
    monkeypatch.setattr(model, "unpack_model", lambda det: {"step": 80})
    monkeypatch.setattr(model, "eaQHMSynthesis", synthesis)
    monkeypatch.setattr(convert, "conversion_apply", conversion_apply)
    assert cli.main(["x.wav", "--conversion", good, "--timing-from", "o.wav"]) == 0
    assert calls["cepstrum"] == [("x.wav", None, 5e-4), ("o.wav", None, 5e-4)]        # the alignment: its own settings
    assert calls["parameters"] == [("x.wav", 3, 2e-3)]                                # the converted rows: the map's
    assert calls["align"] == [((n, 19), (n, 19))] and calls["apply"] == [(n, 4)]
    assert calls["synth"] == [((n, 4), (n,), (n,))]               # converted envelope, OTHER's tempo, the target's pitch
    for k in calls:
        calls[k].clear()
    assert cli.main(["x.wav", "--conversion", good, "--pitch-scale", "1.2"]) == 0     # a pitch flag wins
    assert calls["cepstrum"] == [] and calls["synth"] == [((n, 4), (), ())]

