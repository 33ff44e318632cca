"""The conversion map: a joint-density Gaussian mixture over paired cepstral rows, trained, checked and applied row by
row (not in the reference).  The third layer below convert: a mixture (mixture) over static or dynamic rows (dynamics).

    conversion_pairs(CA, CB, path, span=None, *, device_index=0) -> (X, Y): the rows a model_align path pairs
    conversion_train(X, Y, components=8, *, level=False, iters=20, tol=1e-5, floor=1e-6, init=None, span=None, gv=None,
                     device_index=0)
        -> flat dict of arrays (np.savez): the gmm fields + dx, dy, level, A, b, Wx, kx; span, py, gv_mean, gv_prec
    conversion_apply(conv, C, *, device_index=0) -> float64[n, dy_cols]: a static map, row by row
    check_conversion_arguments, check_conversion: validation, no device work
    gmm_conversion_parameters, gmm_conditional_precisions: the regression's host algebra
    _nonempty_rows, _put_rows: the empty-row and level bookkeeping, shared with convert's trajectory

The definition is DESIGN.md §12: the regression of Stylianou, Cappe & Moulines (1998) in Kain & Macon's joint-density
form.  The fit is mixture.gmm_fit; the posteriors and the regression run in libeaqhm_hip.so (eaqhm_gmm_estep,
eaqhm_gmm_regress); A_m, b_m and the conditional precisions are host NumPy.  There is no CPU path.
"""
import numpy as np

from .align import _path
from .args import _rows
from .cepstrum import CEPSTRUM_MAX_ORDER, _cepstrum_rows, check_cepstrum_warp
from .dynamics import _dynamic_columns, _gv_fields, check_span, dynamic_rows
from .mixture import (GMM_MAX_COLUMNS, GMM_MAX_SIDE, _field, _Mixture, check_gmm, check_gmm_arguments,
                      gmm_estep_parameters, gmm_fit)

_CONVERSION_FIELDS = ("weights", "means", "covs", "zbar", "phi", "loglik", "n", "dx", "dy", "level", "A", "b", "Wx", "kx")


def _has(conv, name):
    try:
        conv[name]
    except (KeyError, TypeError, IndexError):
        return False
    return True


def check_conversion_arguments(X, Y, components=8, level=False, iters=20, tol=1e-5, floor=1e-6, init=None, span=None):
    """Validates everything conversion_train gets (no device work): returns (X, Y, level) with X, Y float64 rows.  With
    level=False column 0 stays out of the map.  Rows are cepstral rows, order 1 to 63, 2 to 64 columns: what
    conversion_apply and envelope= accept; so level=False maps at most 63 columns a side and level=True 64.  With a span
    the rows are dynamic rows [c | delta c], an even number of columns, and the mapped columns with their deltas are at
    most 64 a side (the regression's limit) and 128 together (the mixture's)."""
    if span is not None:
        span = check_span(span)
    width = (CEPSTRUM_MAX_ORDER + 1) * (1 if span is None else 2)
    X, Y = _rows(X, "X", width), _rows(Y, "Y", width)
    if X.shape[0] != Y.shape[0]:
        raise ValueError("X and Y must pair row by row, got %d and %d rows" % (X.shape[0], Y.shape[0]))
    if not isinstance(level, (bool, np.bool_)):
        raise ValueError("level must be True or False")
    if span is not None:
        for A, name in ((X, "X"), (Y, "Y")):
            if A.shape[1] % 2 or A.shape[1] < 4:
                raise ValueError("%s must be dynamic rows [c | delta c]: an even number of columns, 4 to %d, got %d"
                                 % (name, width, A.shape[1]))
        dx, dy = (A.shape[1] - (0 if level else 2) for A in (X, Y))
        if dx > GMM_MAX_SIDE or dy > GMM_MAX_SIDE or dx + dy > GMM_MAX_COLUMNS:
            raise ValueError("a dynamic map takes at most %d mapped columns a side with their deltas and %d together, got "
                             "%d and %d" % (GMM_MAX_SIDE, GMM_MAX_COLUMNS, dx, dy))
    for A, name in ((X, "X"), (Y, "Y")):
        if A.shape[1] < 2:
            raise ValueError("%s must have 2 to %d columns (order 1 to %d), got %d"
                             % (name, CEPSTRUM_MAX_ORDER + 1, CEPSTRUM_MAX_ORDER, A.shape[1]))
    check_gmm_arguments(np.zeros((X.shape[0], 1)), components, iters, tol, floor, init, None)
    return X, Y, bool(level)


def check_conversion(conv):
    """Validates a conversion dict (conversion_train's, or one loaded with np.load(allow_pickle=False)): every field,
    shapes, finiteness, the mixture's rules (check_gmm).  Returns a dict of float64 / int arrays ready for use."""
    for name in _CONVERSION_FIELDS:
        _field(conv, name)
    dx, dy = (int(_field(conv, k, ())) for k in ("dx", "dy"))
    level = bool(_field(conv, "level", ()))
    if not (1 <= dx <= GMM_MAX_SIDE and 1 <= dy <= GMM_MAX_SIDE):
        raise ValueError("the conversion's dx and dy must be in [1, %d]" % GMM_MAX_SIDE)
    w, mu, S, zbar = check_gmm(conv)
    M = len(w)
    if mu.shape[1] != dx + dy:
        raise ValueError("the conversion's means must have dx + dy = %d columns, got %d" % (dx + dy, mu.shape[1]))
    out = dict(weights=w, means=mu, covs=S, zbar=zbar, dx=dx, dy=dy, level=level)
    for name, shape in (("A", (M, dy, dx)), ("b", (M, dy)), ("Wx", (M, dx, dx)), ("kx", (M,)), ("phi", (dx + dy,))):
        out[name] = np.ascontiguousarray(_field(conv, name, shape), dtype=np.float64)
    if np.any(np.einsum("mii->mi", out["Wx"]) <= 0) or np.any(np.triu(out["Wx"], 1) != 0):
        raise ValueError("the conversion's Wx must be lower triangular with a positive diagonal")
    out["loglik"] = _field(conv, "loglik").astype(np.float64).reshape(-1)
    out["n"] = int(_field(conv, "n", ()))
    if _has(conv, "span"):                        # a dynamic map
        span = _field(conv, "span", ())
        if span.dtype.kind not in "iu":
            raise ValueError("the conversion's span must be an integer")
        out["span"] = check_span(int(span))
        if dx % 2 or dy % 2:
            raise ValueError("a dynamic conversion's dx and dy count the delta columns: they must be even")
        out["py"] = np.ascontiguousarray(_field(conv, "py", (M, dy)), dtype=np.float64)
        if np.any(out["py"] <= 0):
            raise ValueError("the conversion's py must be positive")
    if _has(conv, "gv_mean") or _has(conv, "gv_prec"):    # the global-variance statistics
        if "span" not in out:
            raise ValueError("the conversion's gv_mean and gv_prec need a dynamic map (span)")
        out.update(_gv_fields(conv, dy // 2, "the conversion"))
    if _has(conv, "cep_warp"):    # the axis of the rows the map was learned on; without it the linear one
        a = _field(conv, "cep_warp", ())
        if a.dtype.kind not in "iuf":
            raise ValueError("the conversion's cep_warp must be a number")
        out["cep_warp"] = check_cepstrum_warp(float(a), "the conversion's cep_warp")
    return out


# ---- host algebra (float64)
def gmm_conversion_parameters(w, mu_c, Sigma, dx):
    """(A [M, dy, dx], b [M, dy], Wx [M, dx, dx], kx [M]) on centred coordinates: A_m = Sigma_m^yx (Sigma_m^xx)^-1,
    b_m = mu_m^y - A_m mu_m^x, and the E-step parameters of the marginal mixture on x."""
    Wx, kx = gmm_estep_parameters(w, np.ascontiguousarray(mu_c[:, :dx]), np.ascontiguousarray(Sigma[:, :dx, :dx]))
    A = np.stack([Sigma[m, dx:, :dx] @ Wx[m].T @ Wx[m] for m in range(len(w))])
    b = mu_c[:, dx:] - np.einsum("mij,mj->mi", A, mu_c[:, :dx])
    return np.ascontiguousarray(A), np.ascontiguousarray(b), Wx, kx


def gmm_conditional_precisions(Sigma, A, dx):
    """py [M, dy] = 1 / diag(Sigma_m^yy - A_m Sigma_m^xy): the reciprocal diagonals of the conditional covariances of y
    given x; LinAlgError naming the component when one is not positive."""
    py = np.empty((len(A), A.shape[1]))
    for m in range(len(A)):
        v = np.diag(Sigma[m, dx:, dx:]) - np.einsum("ij,ji->i", A[m], Sigma[m, :dx, dx:])
        if not np.all(v > 0) or not np.all(np.isfinite(1.0 / v)):
            raise np.linalg.LinAlgError("the conditional covariance of component %d has a diagonal entry that is not "
                                        "positive" % m)
        py[m] = 1.0 / v
    return py


# ---- device work
def conversion_pairs(CA, CB, path, span=None, *, device_index=0):
    """The rows a model_align path pairs: (X, Y) = (CA[i], CB[j]) for the pairs (i, j) of `path` int[L, 2], without the
    pairs in which either row is empty, (-inf, 0, .., 0).  np.vstack the results of several utterance pairs for
    conversion_train.  CA and CB may have different orders.  span=None is host only; with a `span` in [1, 8] the rows
    paired are the dynamic rows [c | delta c] of both sides (dynamic_rows: the deltas are taken on each utterance,
    before the pairing), for conversion_train(span=)."""
    CA, CB = _cepstrum_rows(CA, "CA"), _cepstrum_rows(CB, "CB")
    p, _ = _path(path, len(CA))
    if p[:, 1].max() >= len(CB):
        raise ValueError("path must pair instants of A with instants 0..%d of B" % (len(CB) - 1))
    if span is not None:
        span = check_span(span)
        CA, CB = (dynamic_rows(C, span, device_index=device_index) for C in (CA, CB))
    X, Y = CA[p[:, 0]], CB[p[:, 1]]
    keep = ~(np.isneginf(X[:, 0]) | np.isneginf(Y[:, 0]))
    return X[keep], Y[keep]


def conversion_train(X, Y, components=8, *, level=False, iters=20, tol=1e-5, floor=1e-6, init=None, span=None,
                     gv=None, device_index=0):
    """Learns the map from rows `X` float64[N, P + 1] to rows `Y` float64[N, Q + 1] (conversion_pairs') as a joint
    mixture of `components` Gaussians over [x | y].  level=False leaves column 0, the level c_0, out of
    both sides: conversion_apply copies it from the source row (a recording level is not a property of the speaker);
    level=True maps it like any other column.  The default initialisation and init="kmeans" (gmm_fit) look at the x
    columns only.  Returns a flat dict of arrays that np.savez stores and np.load(allow_pickle=False) returns: gmm_fit's fields, dx, dy, level,
    A[M, dy, dx], b[M, dy] and the marginal mixture's Wx[M, dx, dx], kx[M].
    With `span` in [1, 8] the rows are dynamic rows [c | delta c] (conversion_pairs(span=)) and the map is a dynamic one
    for conversion_trajectory: the mixture is over [x | delta x | y | delta y], level=False leaves
    column 0 and its delta out, dx and dy count the delta columns (at most 64 a side), and the dict gains span and
    py[M, dy], the reciprocal diagonals of the conditional covariances.  `gv`, a gv_statistics dict of the target speaker
    (span= only), is stored in the map as gv_mean[dy / 2] and gv_prec[dy / 2]: conversion_trajectory then adds the
    global-variance term."""
    X, Y, level = check_conversion_arguments(X, Y, components, level, iters, tol, floor, init, span)
    skip = 0 if level else 1
    if gv is not None:
        if span is None:
            raise ValueError("gv needs span=: a static map has no trajectory to trade against")
        gv = _gv_fields(gv, Y.shape[1] // 2 - skip, "gv")
    if span is None:
        x, y = X[:, skip:], Y[:, skip:]
    else:
        x, y = _dynamic_columns(X, X.shape[1] // 2, skip), _dynamic_columns(Y, Y.shape[1] // 2, skip)
    Z = np.ascontiguousarray(np.hstack((x, y)))
    dx, dy = x.shape[1], y.shape[1]
    g = gmm_fit(Z, components, iters=iters, tol=tol, floor=floor, init=init, split=dx, device_index=device_index)
    A, b, Wx, kx = gmm_conversion_parameters(g["weights"], g["means"] - g["zbar"], g["covs"], dx)
    g.update(n=np.int64(g["n"]), dx=np.int64(dx), dy=np.int64(dy), level=np.bool_(level), A=A, b=b, Wx=Wx, kx=kx)
    if span is not None:
        g.update(span=np.int64(check_span(span)), py=gmm_conditional_precisions(g["covs"], A, dx))
    if gv is not None:
        g.update(gv)
    return g


def _nonempty_rows(C, width, skip):
    """The empty-row and level bookkeeping of a conversion of cepstral rows `C`, its first half: (full, rows, out), the
    mask of the non-empty rows, their columns from `skip` on, compacted, and the result float64[n, width + skip], all 0
    but for the -inf in column 0 of the empty rows."""
    full = ~np.isneginf(C[:, 0])
    out = np.zeros((len(C), width + skip))
    out[~full, 0] = -np.inf
    return full, np.ascontiguousarray(C[full, skip:]), out


def _put_rows(out, full, skip, C, Y):
    """The second half: the converted rows `Y` into the non-empty rows of `out` from column `skip` on, and with skip = 1
    column 0 of the source rows `C` as it is.  Returns `out`."""
    out[full, skip:] = Y
    if skip:
        out[full, 0] = C[full, 0]
    return out


def conversion_apply(conv, C, *, device_index=0):
    """Converts cepstral rows `C` float64[n, dx_cols] (model_cepstrum's layout) with a conversion_train map: yhat_n =
    sum_m p(m | x_n) (b_m + A_m x_n).  An empty row (-inf, 0, .., 0) comes back empty; with level=False column 0 is the
    source row's.  Returns float64[n, dy_cols], accepted by eaQHMSynthesis(envelope=), model_from_parameters and
    cepstrum_envelope as it stands."""
    v = check_conversion(conv)
    if "span" in v:
        raise ValueError("this conversion is a dynamic map (span %d): use conversion_trajectory" % v["span"])
    skip = 0 if v["level"] else 1
    dx, dy, M = v["dx"], v["dy"], len(v["weights"])
    C = _cepstrum_rows(C, "C")
    if C.shape[1] != dx + skip:
        raise ValueError("C must have %d columns for this conversion, got %d" % (dx + skip, C.shape[1]))
    full, rows, out = _nonempty_rows(C, dy, skip)
    n = len(rows)
    if n == 0:
        return out
    mu_c = v["means"] - v["zbar"]
    mix = _Mixture(rows, v["zbar"][:dx], M, device_index)
    gamma, _ = mix.estep(mu_c[:, :dx], v["Wx"], v["kx"])
    t = mix.torch
    Y = t.empty((n, dy), dtype=t.float64, device=mix.dev)
    mix.c.gmm_regress(mix.Z, gamma, t.as_tensor(v["A"], device=mix.dev), t.as_tensor(v["b"], device=mix.dev), n, dx, dy,
                      M, Y)
    return _put_rows(out, full, skip, C, Y.cpu().numpy() + v["zbar"][dx:])
