"""The comparison rule of the exact-search tests (tests/test_gpu_exact.py): returned ids against a brute-force truth, position
by position, with an exemption only where the truth itself is a near-tie in float64.  Test helpers only."""
import numpy as np

from oracle import oracle as O
from tests import metric_util as MU

FLT_MAX = MU.FLT_MAX
EUCLID = ("euclidean", "l2", "sqeuclidean")
TIE_RTOL = 1e-6            # truth distances this close (relative) to a neighbouring position's may come in either order
DIST_RTOL, DIST_ATOL = 1e-5, 1e-6  # the project's tight bound for float64-accumulated distances (gpu_util, test_gpu_build)
MAX_EXEMPT_SHARE = 0.01


def alt_pairs(metric, xq, xnb):
    """float64 alt-space distances of the pairs (xq[i], xnb[i, j]): (m, d) x (m, k, d) -> (m, k), the conventions of
    nnd_gram_to_dist (FLT_MAX / 0 for zero rows and non-positive products, clamped at 0)."""
    a = np.asarray(xq, np.float64)[:, None, :]
    b = np.asarray(xnb, np.float64)
    if metric in EUCLID:
        return ((a - b) ** 2).sum(-1)
    if metric == "cosine":
        dot = (a * b).sum(-1)
        na, nb = (a * a).sum(-1), (b * b).sum(-1)
        out = np.full(dot.shape, FLT_MAX)
        ok = (na > 0) & (nb > 0) & (dot > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[ok] = np.log2(np.sqrt(na * nb) / dot)[ok]
        out[(na == 0) & (nb == 0)] = 0.0
        return np.maximum(out, 0.0)
    return np.maximum(MU.alt_dist_pairs(metric, a, b)[0], 0.0)


def alt_pairs_ids(metric, x, xq, ids, chunk=128):
    out = np.empty(ids.shape, np.float64)
    for s in range(0, ids.shape[0], chunk):
        out[s:s + chunk] = alt_pairs(metric, xq[s:s + chunk], x[ids[s:s + chunk]])
    return out


def oracle_truth(x, k, metric, rows=None):
    """ids of the k + 1 (at most n) nearest rows, self included, ties by index: the position after the k-th counts."""
    name = "euclidean" if metric in EUCLID else metric
    return O.brute_force_knn(x, min(k + 1, x.shape[0]), name, rows=rows)[0].astype(np.int64)


def matrix_truth(metric, x, q, k):
    """the same for external queries, from the float64 distance matrix (stable argsort: ties by index)"""
    kk = min(k + 1, x.shape[0])
    out = np.empty((q.shape[0], kk), np.int64)
    for s in range(0, q.shape[0], 128):
        qs = q[s:s + 128]
        dm = alt_pairs(metric, qs, np.broadcast_to(x[None, :, :], (qs.shape[0],) + x.shape))
        out[s:s + 128] = np.argsort(dm, axis=1, kind="stable")[:, :kk]
    return out


def _near(a, b):
    return np.abs(a - b) <= TIE_RTOL * np.maximum(np.abs(a), np.abs(b))


def check_exact(name, metric, x, xq, idx, dist, truth_idx, k, max_exempt_share=MAX_EXEMPT_SHARE):
    """The comparison rule.  x: the point set as the kernels got it; xq: the query rows (m, d); idx / dist: the result,
    alt-space; truth_idx: (m, >= k) ids of the truth, one position beyond k where the set has one.  Returns the share of
    exempt positions."""
    idx = np.asarray(idx)
    m = idx.shape[0]
    assert idx.shape == (m, k) and dist.shape == (m, k), name
    assert idx.min() >= 0 and idx.max() < x.shape[0], name + ": ids out of range"
    td = alt_pairs_ids(metric, x, xq, truth_idx)
    assert np.all(np.diff(td, axis=1) >= -TIE_RTOL * np.abs(td[:, 1:])), name + ": the truth itself is not ascending"
    exempt = np.zeros((m, k), bool)
    exempt[:, 1:] |= _near(td[:, 1:k], td[:, :k - 1])
    if td.shape[1] > 1:
        nxt = td[:, 1:k + 1]
        exempt[:, :nxt.shape[1]] |= _near(td[:, :nxt.shape[1]], nxt)
    share = float(exempt.mean())
    assert share <= max_exempt_share, "%s: %.3f %% of the positions are near-ties of the truth" % (name, 100 * share)
    wrong = idx != truth_idx[:, :k]
    bad = wrong & ~exempt
    assert not bad.any(), "%s: %d ids differ from the truth outside its near-ties, first at row %d: got %s want %s" % (
        name, int(bad.sum()), int(np.nonzero(bad.any(1))[0][0]), idx[bad.any(1)][0], truth_idx[bad.any(1)][0, :k])
    rd = alt_pairs_ids(metric, x, xq, idx)  # the returned ids' own distances, recomputed here
    tk = td[:, :k]
    big = tk >= FLT_MAX
    assert np.array_equal(rd >= FLT_MAX, big), name + ": FLT_MAX convention of the returned ids"
    ok = np.abs(rd - tk) <= DIST_RTOL * np.abs(tk) + DIST_ATOL
    assert np.all(ok | big), name + ": a returned id at a near-tie is not as close as the truth's"
    d64 = dist.astype(np.float64)
    assert np.all((np.abs(d64 - tk) <= DIST_RTOL * np.abs(tk) + DIST_ATOL) | big), "%s: distances off by up to %g" % (
        name, np.abs(d64 - tk)[~big].max())
    assert np.all(dist[big] >= np.float32(FLT_MAX)), name + ": FLT_MAX convention of the distances"
    assert np.all(np.diff(d64, axis=1) >= 0), name + ": rows not ascending"
    srt = np.sort(idx, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), name + ": an id repeats in a row"
    return share


def agree(name, metric, x, xq, a, b, k):
    """two results of the same search under the same rule: a's ids serve as the truth of b (no position beyond the k-th)"""
    ai, ad = a
    bi, bd = b
    check_exact(name, metric, x, xq, bi, bd, np.asarray(ai, np.int64), k)
