"""The time alignment on the MI355X (model_align / dtw -> eaqhm_cepstrum_cost, eaqhm_dtw) against the NumPy model of
DESIGN.md §9.6 (tests/model_align_ref.py).  Hand-built inputs only, except the CLI test.

Bars.  The recursion on integer costs: every sum is exact, so path, length, total and every D cell inside the band are
compared bit for bit.  The cost kernel: (P + 4) 2^-52 d per cell against the np.longdouble model: each non-negative
term carries at most four roundings (the difference, the square, the weight), any summation order adds at most P more,
nothing cancels, so the error is at most (P + 4) 2^-53 d and the bar is twice that; out-of-table cells, empty rows and
identical rows are exact.  model_align on noisy rows: the same plus one addition per path cell,
(P + 4 + L) 2^-52 cost_ref."""
import os

import numpy as np
import pytest

import model_align_ref as AR
from conftest import GOLDEN, record_measurement

pytestmark = pytest.mark.gpu

U = 2.0 ** -52


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def gpu_dtw(band):
    """(the context, r, the band on the device) for Context.dtw."""
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    nA, W = band.shape
    r = (W - 1) // 2
    return c, r, torch.as_tensor(np.ascontiguousarray(band), device=c.device)


def run_gpu_dtw(band, nA, nB):
    """Context.dtw on a band of costs: (path int64[L, 2], total, D band, ptr band)."""
    import torch
    c, r, band_d = gpu_dtw(band)
    ptr = torch.full(band.shape, 255, dtype=torch.uint8, device=c.device)
    path = torch.full((nA + nB - 1, 2), -7, dtype=torch.int32, device=c.device)
    n = torch.zeros(1, dtype=torch.int32, device=c.device)
    total = torch.zeros(1, dtype=torch.float64, device=c.device)
    c.dtw(band_d, nA, nB, r, ptr, path, n, total)
    L = int(n.item())
    assert 1 <= L <= nA + nB - 1
    return path[:L].cpu().numpy().astype(np.int64), float(total.item()), band_d.cpu().numpy(), ptr.cpu().numpy()


def check_against_model(band, nA, nB, label):
    r = (band.shape[1] - 1) // 2
    want_path, want_total, want_D, want_ptr = AR.align_band(band, nA, nB, r)
    path, total, D, ptr = run_gpu_dtw(band, nA, nB)
    inside = AR.in_band(nA, nB, r)
    assert np.array_equal(D[inside], want_D[inside]), label            # every cell of the band, bit for bit
    assert np.all(np.isposinf(D[~inside])), label                         # storage outside the table: untouched
    assert np.array_equal(ptr[inside], want_ptr[inside]), label
    assert np.all(ptr[~inside] == 255), label
    assert path.shape == want_path.shape and np.array_equal(path, want_path), label
    assert total == want_total, label
    return want_path, want_total


# ---- 1. the recursion, exact
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (63, 64), (64, 64), (65, 65), (70, 130), (130, 70), (200, 150)]


def radii(nA, nB):
    lo, full = AR.min_radius(nA, nB), AR.full_radius(nA, nB)
    return sorted({r for r in (full, lo, lo + 1, 20) if lo <= r <= full})


@pytest.mark.parametrize("nA,nB", SHAPES)
def test_recursion_is_exact_on_integer_costs(amd, nA, nB):
    """Costs 0..7 as doubles (many ties) and all zeros, through Context.dtw (D, ptr, path, total) and through dtw()
    (the host's band layout).  Bands: full, r_min, r_min + 1 and 20 where admissible."""
    rng = np.random.default_rng(1000 * nA + nB)
    for dense in (rng.integers(0, 8, size=(nA, nB)).astype(np.float64), np.zeros((nA, nB))):
        for r in radii(nA, nB):
            label = (nA, nB, r, float(dense.max()))
            want_path, want_total = check_against_model(AR.to_band(dense, r), nA, nB, label)
            path, total = amd.dtw(dense, band=r)
            assert path.dtype == np.int64 and np.array_equal(path, want_path) and total == want_total, label
        path, total = amd.dtw(dense)                                     # band=None: the full table
        full = AR.align(dense)
        assert np.array_equal(path, full[0]) and total == full[1]
    if nA == nB:                                                          # all zeros: the diagonal
        assert np.array_equal(path, np.stack((np.arange(nA), np.arange(nA)), axis=1))


# ---- 2. long and thin: the 64-bit indices
def test_long_thin_band(amd):
    """nA = 70 001, nB = 69 997, r = 2: i (nB - 1) passes 2^32, about 2 200 launches, 350 k cells."""
    nA, nB, r = 70001, 69997, 2
    assert (nA - 1) * (nB - 1) > 2 ** 32 and AR.min_radius(nA, nB) == 1
    rng = np.random.default_rng(7)
    band = rng.integers(0, 8, size=(nA, 2 * r + 1)).astype(np.float64)
    band[~AR.in_band(nA, nB, r)] = np.inf
    path, total = check_against_model(band, nA, nB, "long_thin")
    assert AR.path_is_valid(path, nA, nB, r) and np.isfinite(total)
    record_measurement("align_long_thin", path_len=int(len(path)), total=float(total))


# ---- 3. the cost kernel
def cepstra(n, P, seed):
    """Smooth cepstrum-like rows: c_0 about -4, c_p decaying as (1 + p)^-1.5, moving from row to row."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((n, P + 1)) / (1.0 + np.arange(P + 1))[None, :] ** 1.5
    C[:, 0] = -4.0 + 0.5 * rng.standard_normal(n)
    return C


def empty_row(C, i):
    C[i] = 0.0
    C[i, 0] = -np.inf


_COST = {}


def cost_case(P):
    """(A, B) shared by the cases of one order: nA = 70, nB = 130, empty rows on both sides (A's 10 and B's 19 face
    each other on the scaled diagonal), rows of A copied into B."""
    if P not in _COST:
        A, B = cepstra(70, P, 10 + P), cepstra(130, P, 20 + P)
        c = AR.centres(70, 130)
        assert c[10] == 19
        for i in (10, 33, 69):
            empty_row(A, i)
        for j in (0, 19, 20, 77):
            empty_row(B, j)
        for i, j in ((5, 9), (5, 12), (40, 75), (68, 129), (0, 1)):
            B[j] = A[i]
        _COST[P] = (A, B)
    return _COST[P]


@pytest.mark.parametrize("c0_weight", [0.0, 1.0])
@pytest.mark.parametrize("P", [1, 18, 63])
def test_cost_kernel(amd, P, c0_weight):
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    A, B = cost_case(P)
    nA, nB = len(A), len(B)
    empty_cost = 4.0 if c0_weight == 0.0 else 0.75
    ref = AR.cost(A, B, c0_weight, empty_cost, np.longdouble)
    ea, eb = AR.is_empty(A), AR.is_empty(B)
    A_d, B_d = (torch.as_tensor(x, device=c.device) for x in (A, B))
    for r in (AR.full_radius(nA, nB), 20):
        band = torch.full((nA, 2 * r + 1), -1.0, dtype=torch.float64, device=c.device)
        c.cepstrum_cost(A_d, nA, B_d, nB, P, c0_weight, empty_cost, r, band)
        got = band.cpu().numpy()
        inside = AR.in_band(nA, nB, r)
        assert np.all(np.isposinf(got[~inside]))                          # outside the table: exactly +inf
        want = AR.to_band(ref, r)
        both = AR.to_band((ea[:, None] & eb[None, :]).astype(np.float64), r, 0.0) == 1
        one = AR.to_band((ea[:, None] ^ eb[None, :]).astype(np.float64), r, 0.0) == 1
        same = AR.to_band((A[:, None, :] == B[None, :, :]).all(axis=2).astype(np.float64), r, 0.0) == 1
        assert both[10, 19 - 19 + r] and both.sum() >= 1 and one.sum() > 100 and same.sum() >= 3
        assert np.all(got[both] == 0.0) and np.all(got[one] == empty_cost) and np.all(got[same] == 0.0)
        rest = inside & ~both & ~one & ~same
        assert rest.sum() > 0.8 * inside.sum()
        d = want[rest]
        assert np.all(d > 0) and np.all(np.isfinite(got[rest]))
        frac = np.abs(got[rest].astype(np.longdouble) - d) / ((P + 4) * U * d)
        worst = float(frac.max())
        print("cost kernel P %d c0_weight %g r %d: worst error / bar %.3g over %d cells" % (P, c0_weight, r, worst, rest.sum()))
        record_measurement("align_cost_kernel_P%d_c0w%g_r%d" % (P, c0_weight, r), worst_error_over_bar=worst,
                           cells=int(rest.sum()))
        assert worst <= 1.0, (P, c0_weight, r, worst)                     # every other cell, none left out


# ---- 4. model_align end to end
def held_rows(n_base, n, seed):
    """A nondecreasing map of n rows onto n_base base rows that uses every base row: some rows are held."""
    rng = np.random.default_rng(seed)
    extra = np.sort(rng.integers(0, n_base, size=n - n_base))
    return np.sort(np.concatenate((np.arange(n_base), extra)))


def base_cepstrum(n):
    """A harmonic-model-style cepstrum: the NumPy fit (order 18) of n instants of 20 harmonics of 180 Hz under a moving
    formant."""
    import model_cepstrum_ref as CR
    from test_gpu_model_cepstrum import _records, harmonic_model
    det, fs, _ = harmonic_model(n, 20, 180.0, 16000)
    C = CR.fit(_records(det)[0], fs, 18, 5e-4)
    assert np.all(np.isfinite(C))
    return C


def test_model_align_recovers_a_known_map_exactly(amd):
    """A (90 rows) and B (104 rows) hold rows of the same 70 distinct base rows, each side holding some of them: seen
    from A, B repeats some rows and skips others.  A zero-cost path exists, so the cost is exactly 0, every pair of the
    path joins equal base rows, and the path is the model's (the tie rule decides along the repeats: only exact zeros
    are tied)."""
    S = base_cepstrum(70)
    ia, ib = held_rows(70, 90, 1), held_rows(70, 104, 2)
    A, B = S[ia], S[ib]
    d = AR.cost(A, B)
    assert np.all(d[ia[:, None] != ib[None, :]] > 0)
    for band in (None, 30):
        path, cost = amd.model_align(A, B, band=band)
        assert cost == 0.0
        assert np.array_equal(ia[path[:, 0]], ib[path[:, 1]])
        want = AR.align(d, AR.full_radius(90, 104) if band is None else band)
        assert want[1] == 0.0 and np.array_equal(path, want[0])
        assert AR.path_is_valid(path, 90, 104, AR.full_radius(90, 104) if band is None else band)


def test_model_align_on_noisy_rows(amd):
    S = base_cepstrum(120)
    ia, ib = held_rows(120, 150, 3), held_rows(120, 210, 4)
    rng = np.random.default_rng(5)
    A, B = S[ia], S[ib]
    B = B + 0.01 * np.linalg.norm(B, axis=1)[:, None] * rng.standard_normal(B.shape) / np.sqrt(B.shape[1])
    nA, nB, P = 150, 210, 18
    dl = AR.cost(A, B, dtype=np.longdouble)
    for band in (None, 40):
        r = AR.full_radius(nA, nB) if band is None else band
        path, cost = amd.model_align(A, B, band=band)
        assert AR.path_is_valid(path, nA, nB, r)
        cost_ref = AR.align(dl, r)[1]
        L = len(path)
        bound = (P + 4 + L) * U
        own = float(abs(np.longdouble(cost) - cost_ref) / (bound * cost_ref))
        priced = sum(dl[i, j] for i, j in path)
        excess = float((priced - cost_ref) / (bound * cost_ref))
        print("model_align noisy r %d: L %d cost %.17g, |cost - ref| / bar %.3g, path excess / bar %.3g"
              % (r, L, cost, own, excess))
        record_measurement("align_noisy_r%d" % r, path_len=L, cost=cost, cost_error_over_bar=own,
                           path_excess_over_bar=excess)
        assert cost_ref > 0 and own <= 1.0, (r, own)
        assert priced <= cost_ref * (1 + bound), (r, excess)


# ---- 5. through the synthesis
def test_a_model_aligned_with_itself_is_the_diagonal(amd):
    """small_model's instant 4 is empty: zero-cost cells off the diagonal, so the diagonal is the tie rule's."""
    from test_gpu_model_cepstrum import small_model
    det, fs, L = small_model()
    C = amd.model_cepstrum(det, fs, 8, 5e-4)
    n = len(C)
    assert np.isneginf(C[4, 0])
    for band in (None, 1, 3):
        path, cost = amd.model_align(C, C, band=band)
        assert cost == 0.0 and np.array_equal(path, np.stack((np.arange(n), np.arange(n)), axis=1))
    idx = amd.alignment_index(path, n)
    assert np.array_equal(idx, np.arange(n))
    W = amd.warp_rows(C, idx)
    assert W.tobytes() == C.tobytes()
    out = amd.eaQHMSynthesis(det, fs, L, envelope=W)
    assert np.array_equal(out, amd.eaQHMSynthesis(det, fs, L, envelope=C))
    assert np.array_equal(amd.alignment_time_scale(path, n), np.ones(n))


# ---- 6. the CLI
def test_cli_envelope_from_the_same_file(amd, tmp_path):
    import shutil
    from eaqhm_amd import cli
    outs = []
    for name, flags in (("a", ["--cepstral-envelope", "--envelope-from", os.path.join(GOLDEN, "SA19.WAV")]),
                        ("b", ["--cepstral-envelope"])):
        d = tmp_path / name
        d.mkdir()
        wav = str(d / "SA19.WAV")
        shutil.copy(os.path.join(GOLDEN, "SA19.WAV"), wav)
        assert cli.main([wav, "--gender", "female", "--max-adpt", "1"] + flags) == 0
        with open(str(d / "SA19_modified.wav"), "rb") as f:
            outs.append(f.read())
    assert len(outs[0]) > 1000 and outs[0] == outs[1]


def test_entry_points_reject_bad_arguments(amd):
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    nA, nB, P, r = 7, 13, 5, 3
    W = 2 * r + 1
    A, B = (torch.zeros((n, P + 1), dtype=torch.float64, device=c.device) for n in (nA, nB))
    band = torch.zeros((nA, W), dtype=torch.float64, device=c.device)
    ptr = torch.zeros((nA, W), dtype=torch.uint8, device=c.device)
    path = torch.zeros((nA + nB - 1, 2), dtype=torch.int32, device=c.device)
    n = torch.zeros(1, dtype=torch.int32, device=c.device)
    total = torch.zeros(1, dtype=torch.float64, device=c.device)
    c.cepstrum_cost(A, nA, B, nB, P, 0.0, 4.0, r, band)                  # the good calls
    c.dtw(band, nA, nB, r, ptr, path, n, total)
    c.sync()
    assert int(n.item()) == nB and float(total.item()) == 0.0

    def bad(fn, *a):
        with pytest.raises(RuntimeError, match="error -1"):
            fn(*a)

    for order in (0, 64, -1):
        bad(c.cepstrum_cost, A, nA, B, nB, order, 0.0, 4.0, r, band)
    for v in (-1.0, float("nan"), float("inf")):
        bad(c.cepstrum_cost, A, nA, B, nB, P, v, 4.0, r, band)
        bad(c.cepstrum_cost, A, nA, B, nB, P, 0.0, v, r, band)
    for a, b, rr in ((0, nB, r), (nA, 0, r), (nA, nB, 1), (nA, nB, -1), (1, nB, nB - 2), (-3, nB, r)):
        bad(c.cepstrum_cost, A, a, B, b, P, 0.0, 4.0, rr, band)
        bad(c.dtw, band, a, b, rr, ptr, path, n, total)
    for j in (0, 2, 8):
        args = [A, nA, B, nB, P, 0.0, 4.0, r, band]
        args[j] = None
        bad(c.cepstrum_cost, *args)
    for j in (0, 4, 5, 6, 7):
        args = [band, nA, nB, r, ptr, path, n, total]
        args[j] = None
        bad(c.dtw, *args)
    assert c.abi_version == 6
