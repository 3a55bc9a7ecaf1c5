"""The metrics that are euclidean distance after a fixed linear map of the rows: ``seuclidean`` / ``standardised_euclidean``,
``wminkowski`` / ``weighted_minkowski`` with ``p = 2``, ``mahalanobis``, and ``minkowski`` with ``p = 2`` (no map at all).

    seuclidean(x, y; V)      = sqrt(sum (x_i - y_i)^2 / V_i)   = |D (x - y)|,  D = diag(V^-1/2)
    wminkowski(x, y; w, 2)   = sqrt(sum w_i (x_i - y_i)^2)     = |D (x - y)|,  D = diag(sqrt w)
    mahalanobis(x, y; VI)    = sqrt((x - y)^T VI (x - y))      = |A (x - y)|,  A^T A = (VI + VI^T) / 2

(reference distances.py:95-197).  Host only, numpy only: this module parses and validates ``metric_kwds`` and factors ``VI`` in
float64; the transform itself is the device's (csrc/linear.hip, ``y = A (x - c)``), and everything behind it runs the
euclidean path unchanged.  The reference hands ``tuple(metric_kwds.values())`` to its distance positionally
(pynndescent_.py:1271-1304), so the dict's ORDER decides here too and the key names do not.
"""
from typing import NamedTuple, Optional

import numpy as np

NND_LINEAR_DIAGONAL, NND_LINEAR_DENSE = 0, 1  # include/pynnd_amd.h NND_LINEAR_*

DIAGONAL_V = ("seuclidean", "standardised_euclidean")
DIAGONAL_W = ("wminkowski", "weighted_minkowski")
DENSE = ("mahalanobis",)
PLAIN = ("minkowski",)
LINEAR_METRICS = DIAGONAL_V + DIAGONAL_W + DENSE + PLAIN


class LinearMap(NamedTuple):
    """What an index keeps (and pickles) of its metric's map: ``y = a (x - shift)``, both float32."""
    kind: int  # NND_LINEAR_DIAGONAL: a is (d,); NND_LINEAR_DENSE: a is (d, d), y_j = sum_k a[j, k] (x_k - shift_k)
    a: np.ndarray
    shift: Optional[np.ndarray]  # (d,), fixed when the index is first built; None until then


def _vector(metric, name, v, dim):
    v = np.asarray(v, dtype=np.float64)
    if v.shape != (dim,):
        raise ValueError("metric %r: %s must have shape (%d,), got %s" % (metric, name, dim, v.shape))
    if not np.isfinite(v).all():
        raise ValueError("metric %r: %s holds a NaN or an infinity" % (metric, name))
    return v


def _require_p2(metric, p):
    try:
        two = float(p) == 2.0
    except (TypeError, ValueError):
        raise ValueError("metric %r: p must be a number, got %r" % (metric, p))
    if not two:
        raise NotImplementedError("pynndescent_amd accelerates metric %r for p = 2 only (got p = %r); use pynndescent.NNDescent"
                                  % (metric, p))


def mahalanobis_factor(vi):
    """A float64 ``A`` with ``A^T A = (VI + VI^T) / 2``: the transposed Cholesky factor; where Cholesky fails (a
    semi-definite or slightly indefinite matrix) ``Lambda^1/2 Q^T`` of ``eigh``, eigenvalues within
    ``d * eps64 * lambda_max`` of zero clipped to zero.  A symmetric part with an eigenvalue below that is not positive
    semi-definite: ValueError."""
    vi = np.asarray(vi, dtype=np.float64)
    s = (vi + vi.T) / 2.0
    try:
        return np.ascontiguousarray(np.linalg.cholesky(s).T)
    except np.linalg.LinAlgError:
        pass
    lam, q = np.linalg.eigh(s)
    tol = s.shape[0] * np.finfo(np.float64).eps * max(float(np.abs(lam).max()), 0.0)
    if lam.min() < -tol:
        raise ValueError("metric 'mahalanobis': the symmetric part of VI is not positive semi-definite "
                         "(smallest eigenvalue %g)" % float(lam.min()))
    lam = np.where(lam <= tol, 0.0, lam)
    return np.ascontiguousarray(np.sqrt(lam)[:, None] * q.T)


def parse_metric_kwds(metric, metric_kwds, dim):
    """The map of ``metric`` (one of ``LINEAR_METRICS``) for rows of ``dim`` columns from ``metric_kwds``, read positionally:
    a ``LinearMap`` without its shift, or None where the metric is plain euclidean (``minkowski``).  ValueError: a missing
    vector or matrix, a wrong shape, a non-finite entry, ``V <= 0``, ``w < 0``, a ``VI`` whose symmetric part is not positive
    semi-definite.  NotImplementedError: ``p != 2``."""
    args = tuple((metric_kwds or {}).values())
    dim = int(dim)
    if metric in PLAIN:
        if len(args) > 1:
            raise ValueError("metric %r takes at most one argument (p), got %d" % (metric, len(args)))
        if args:
            _require_p2(metric, args[0])
        return None
    if metric in DIAGONAL_V:
        if len(args) != 1:
            raise ValueError("metric %r needs the variances V in metric_kwds: one vector of length %d (got %d arguments)"
                             % (metric, dim, len(args)))
        v = _vector(metric, "V", args[0], dim)
        if (v <= 0).any():
            raise ValueError("metric %r: every entry of V must be > 0" % (metric,))
        return LinearMap(NND_LINEAR_DIAGONAL, (1.0 / np.sqrt(v)).astype(np.float32), None)
    if metric in DIAGONAL_W:
        if len(args) not in (1, 2):
            raise ValueError("metric %r needs the weights w in metric_kwds: a vector of length %d, then optionally p "
                             "(got %d arguments)" % (metric, dim, len(args)))
        if len(args) == 2:
            _require_p2(metric, args[1])
        w = _vector(metric, "w", args[0], dim)
        if (w < 0).any():
            raise ValueError("metric %r: every entry of w must be >= 0" % (metric,))
        return LinearMap(NND_LINEAR_DIAGONAL, np.sqrt(w).astype(np.float32), None)
    if metric in DENSE:
        if len(args) != 1:
            raise ValueError("metric %r needs the inverse covariance VI in metric_kwds: one (%d, %d) matrix (got %d arguments)"
                             % (metric, dim, dim, len(args)))
        vi = np.asarray(args[0], dtype=np.float64)
        if vi.shape != (dim, dim):
            raise ValueError("metric %r: VI must have shape (%d, %d), got %s" % (metric, dim, dim, vi.shape))
        if not np.isfinite(vi).all():
            raise ValueError("metric %r: VI holds a NaN or an infinity" % (metric,))
        return LinearMap(NND_LINEAR_DENSE, mahalanobis_factor(vi).astype(np.float32), None)
    raise KeyError(metric)


SHIFT_SAMPLE = 4096  # rows of the strided sample whose column mean is the shift


def shift_rows(n):
    """The rows whose column mean is the shift ``c`` of an index of ``n`` training rows: every ``n // 4096``-th one."""
    return np.arange(0, int(n), max(1, int(n) // SHIFT_SAMPLE), dtype=np.int64)


def shift_of(rows_view):
    """The shift ``c``: float32 of the float64 column mean of the sampled rows (``rows_view[ids]`` gives them as float32 --
    a host array, or a gathering view of a device tensor: the one place ``c`` comes from, so both give the same bits)."""
    sample = np.asarray(rows_view[shift_rows(rows_view.shape[0])], dtype=np.float32)
    return sample.astype(np.float64).mean(axis=0).astype(np.float32)

