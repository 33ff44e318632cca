"""NumPy model of the formant scale (model.eaQHMSynthesis with formant_scale, model.model_envelope).

Written from the definition in DESIGN.md §9.2, independently of the HIP kernels; the GPU tests compare the kernels with
it.  Only the amplitude rule and the envelope readout are new: the phases, the time map and the synthesis are those of
model_synthesis_ref (§9) and model_contour_ref (§9.1), run with the amplitudes of this module in place of theirs.

    envelope_readout(records, freqs, alpha=1) -> float64[No_ti, len(freqs)]
    formant_amplitudes(am, fm, fs, beta, alpha) -> A' (float64[No_ti, Kmax])
    synthesize_formant(records, step, fs, L, rho, beta, alpha) -> float64[rint(rho * L)]   (numbers)
    synthesize_formant_contour(records, step, fs, L, rho, beta, alpha) -> float64[L_out]    (numbers or contours)
"""
from contextlib import contextmanager

import numpy as np

import model_contour_ref as MC
import model_synthesis_ref as M


def envelope_nodes(am_row, fm_row):
    """The nodes of E_i: the active slots (am != 0, f > 0) sorted by (f, k), as (f, ln am)."""
    ks = np.flatnonzero((am_row != 0) & (fm_row > 0))
    order = np.lexsort((ks, fm_row[ks]))
    return fm_row[ks][order], np.log(am_row[ks][order])


def _per_instant(x, n):
    return np.broadcast_to(np.asarray(x, dtype=np.float64), (n,))


def envelope_readout(records, freqs, alpha=1.0):
    """out[i, t] = E_i(freqs[t] / alpha_i); -inf on the rows of instants without active slots."""
    rec = np.asarray(records, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    alpha = _per_instant(alpha, n)
    freqs = np.asarray(freqs, dtype=np.float64)
    out = np.full((n, len(freqs)), -np.inf)
    for i in range(n):
        f, v = envelope_nodes(rec[i, :K], rec[i, K:2 * K])
        if len(f):
            out[i] = M.interp_envelope(f, v, freqs / alpha[i])
    return out


def formant_amplitudes(am, fm, fs, beta, alpha):
    """A' of §9.2: am where beta_i == alpha_i == 1; otherwise exp(E_i(q)) with q = (beta_i * f) / alpha_i, muted where
    beta_i * f >= fs/2.  beta and alpha are numbers or one value per instant."""
    n = am.shape[0]
    beta, alpha = _per_instant(beta, n), _per_instant(alpha, n)
    out = np.zeros_like(am)
    for i in range(n):
        if beta[i] == 1.0 and alpha[i] == 1.0:
            out[i] = am[i]
            continue
        ks = np.flatnonzero((am[i] != 0) & (fm[i] > 0))
        if len(ks) == 0:
            continue
        f, v = envelope_nodes(am[i], fm[i])
        bf = beta[i] * fm[i, ks]
        out[i, ks] = np.exp(M.interp_envelope(f, v, bf / alpha[i]))
        out[i, ks[bf >= fs / 2]] = 0.0
    return out


@contextmanager
def _amplitudes(Ap):
    """The §9 / §9.1 models with A' replaced: both look their amplitude functions up at call time."""
    saved = M.envelope_amplitudes, MC.envelope_amplitudes_per_instant
    M.envelope_amplitudes = lambda *args: Ap.copy()
    MC.envelope_amplitudes_per_instant = lambda *args: Ap.copy()
    try:
        yield
    finally:
        M.envelope_amplitudes, MC.envelope_amplitudes_per_instant = saved


def synthesize_formant(records, step, fs, L, rho, beta, alpha):
    """§9 with the formant amplitudes (rho, beta, alpha numbers)."""
    rec = np.asarray(records, dtype=np.float64)
    K = (rec.shape[1] - 1) // 3
    Ap = formant_amplitudes(rec[:, :K], rec[:, K:2 * K], fs, beta, alpha)
    with _amplitudes(Ap):
        return M.synthesize(rec, step, fs, L, rho, beta, True)


def synthesize_formant_contour(records, step, fs, L, rho, beta, alpha):
    """§9.1 with the formant amplitudes; numbers are broadcast to contours."""
    rec = np.asarray(records, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    rho, beta = _per_instant(rho, n).copy(), _per_instant(beta, n).copy()
    Ap = formant_amplitudes(rec[:, :K], rec[:, K:2 * K], fs, beta, alpha)
    with _amplitudes(Ap):
        return MC.synthesize_contour(rec, step, fs, L, rho, beta, True)
