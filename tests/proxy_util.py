"""float64 evaluations of the reference's proxy_inner_product (distances.py:810-838) and of its true distance, the negative
inner product, with the a-priori float32 error radii the GPU tests compare within, and the fixture inputs of
tests/golden/make_golden_proxy.py.  Test helpers only.

The kernels' convention (DESIGN.md "Proxy distances"): FLT_MAX for a zero row and for <a, b> <= 0 (the reference gives +inf at
<a, b> = 0: both mean "infinitely far"), otherwise max(-log2(<a,b> / sqrt(|a|^2 |b|^2)), 0) + 1 / sqrt(<a,b>)."""
import os

import numpy as np

from tests import metric_util as MU

FLT_MAX = float(np.finfo(np.float32).max)
U24 = 2.0 ** -24
METRIC = "proxy_inner_product"
CODE = 6
K = 10
SEEDS = (3, 4, 5, 6, 7)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proxy_inner_product.npz")


def fixture_data():
    """The 2000 x 16 build rows and the 200 held-out queries of the inner-product fixtures (clustered, shifted by 0.5: mostly
    positive inner products, some negative ones)."""
    return MU.metric_data("inner_product")


def _formula(g, s):
    """The proxy of Gram values g > 0 and norm products s = |a|^2 |b|^2 > 0 (float64 arrays)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.maximum(-np.log2(g / np.sqrt(s)), 0.0) + 1.0 / np.sqrt(g)


def proxy_from_gram(g, na, nb):
    """The kernels' proxy distance from float64 <a,b>, |a|^2, |b|^2 (broadcast)."""
    g, na, nb = np.broadcast_arrays(np.asarray(g, np.float64), np.asarray(na, np.float64), np.asarray(nb, np.float64))
    far = (na == 0.0) | (nb == 0.0) | ~(g > 0.0)
    r = _formula(np.where(far, 1.0, g), np.where(far, 1.0, na * nb))
    return np.where(far, FLT_MAX, np.minimum(r, FLT_MAX))


def proxy_dist(a, b):
    """(len(a), len(b)) float64 matrix of the proxy distance."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return proxy_from_gram(a @ b.T, (a * a).sum(1)[:, None], (b * b).sum(1)[None, :])


def proxy_pairs(a, b):
    """The proxy of the pairs (a[i], b[i]) for any leading shape: (..., d) x (..., d) -> (...) float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return proxy_from_gram((a * b).sum(-1), (a * a).sum(-1), (b * b).sum(-1))


def gamma(d):
    """Relative error bound of a float32 sum of d products (any order, fused or not), over sum |a_i b_i|: the kernels pad a
    row to a multiple of four columns (zeros) and add the partial sums of four lanes or of the MFMA's four K steps, so
    (dp + 4) roundings bound every path -- the gamma of tests/search_reference.py _Distances."""
    return (((int(d) + 3) & ~3) + 4) * U24


def _ulp32(v):
    a = np.minimum(np.abs(np.asarray(v, np.float64)), FLT_MAX).astype(np.float32)
    with np.errstate(over="ignore"):
        return np.spacing(a).astype(np.float64)


# What the float32 evaluation of the formula adds to the error of its inputs, derived from the operations, never measured:
#   * the log term: the cosine is g * rsq(|a|^2) * rsq(|b|^2) -- two hardware inverse roots (1 ulp: 2^-23 relative each) and
#     two multiplies (2^-24 each), 1.5 * 2^-22 relative on the argument, so 1.5 * 2^-22 / ln 2 absolute on the result -- and
#     the hardware log2 itself (1 ulp; near an argument of 1 as if the argument were off by 2^-23: 2^-23 / ln 2 absolute);
#     together 2.9 * 2^-22, below 2^-20;
#   * the inverse root of g: one hardware rsq (1 ulp); the sum: one add -- 4 float32 ulps of the result cover them.
LOG_TERM_ABS = 2.0 ** -20


def proxy_interval(g, dg, na, nb, rel):
    """(mid, lo, hi) of the float32 kernel value for exact Gram value g known to +-dg and squared norms known to `rel`
    relative: the formula is monotone (falling in g, rising in the norms), so it is evaluated at both ends, then widened by the
    evaluation error above.  FLT_MAX where the operands say so; an interval that reaches g <= 0 has hi = FLT_MAX."""
    g, dg, na, nb = (np.asarray(v, np.float64) for v in np.broadcast_arrays(g, dg, na, nb))
    mid = proxy_from_gram(g, na, nb)
    zero = (na == 0.0) | (nb == 0.0)
    s = na * nb
    g_hi, g_lo = g + dg, g - dg
    lo = np.where(zero | ~(g_hi > 0.0), FLT_MAX, _formula(np.where(g_hi > 0.0, g_hi, 1.0), np.where(zero, 1.0, s * (1.0 - rel) ** 2)))
    hi = np.where(zero | ~(g_lo > 0.0), FLT_MAX, _formula(np.where(g_lo > 0.0, g_lo, 1.0), np.where(zero, 1.0, s * (1.0 + rel) ** 2)))
    lo, hi = np.minimum(lo, FLT_MAX), np.minimum(hi, FLT_MAX)
    lo = np.where(lo < FLT_MAX, np.maximum(lo - 4.0 * _ulp32(lo) - LOG_TERM_ABS, 0.0), lo)
    hi = np.where(hi < FLT_MAX, np.minimum(hi + 4.0 * _ulp32(hi) + LOG_TERM_ABS, FLT_MAX), hi)
    return mid, lo, hi


def proxy_pairs_f32(a, b):
    """(mid, lo, hi) of the pairs (a[i], b[i]) as a float32 Gram kernel may compute them (the build kernels, the walk)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    gm = gamma(a.shape[-1])
    return proxy_interval((a * b).sum(-1), gm * (np.abs(a) * np.abs(b)).sum(-1), (a * a).sum(-1), (b * b).sum(-1), gm)


def proxy_matrix_f32(a, b):
    """The same for every (a[i], b[j])."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    gm = gamma(a.shape[-1])
    return proxy_interval(a @ b.T, gm * (np.abs(a) @ np.abs(b).T), (a * a).sum(1)[:, None], (b * b).sum(1)[None, :], gm)


def within(got, lo, hi):
    """got (float32 values) inside [lo, hi]; FLT_MAX and +inf count as the same "infinitely far"."""
    got = np.minimum(np.asarray(got, np.float64), FLT_MAX)
    return (got >= lo) & (got <= hi)


def proxy_pairs_f64(a, b):
    """(mid, radius) of the values k_finalize hands out: float64 accumulation of the formula, rounded to float32 once -- the
    float64 errors are far below a float32 ulp, so 2 ulps bound the rounding and the float64 library's own last bits."""
    mid = proxy_pairs(a, b)
    return mid, np.where(mid < FLT_MAX, 2.0 * _ulp32(mid), 0.0)


def neg_inner(q, x):
    """(mid, radius) of -<q, x[i]> for every row of x: the rerank's float32 sum of d products."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    return -(x @ q), gamma(x.shape[-1]) * (np.abs(x) @ np.abs(q))


def mips_truth(x, q, k=K):
    """Ids of the k largest float64 inner products of every query (ties to the smaller id)."""
    g = np.asarray(q, np.float64) @ np.asarray(x, np.float64).T
    return np.argsort(-g, axis=1, kind="stable")[:, :k]


def proxy_truth(x, q=None, k=K):
    """Ids of the k proxy-nearest rows (float64, the row itself included when q is None; ties to the smaller id)."""
    q = x if q is None else q
    out = np.empty((len(q), k), np.int64)
    for s in range(0, len(q), 512):
        out[s:s + 512] = np.argsort(proxy_dist(q[s:s + 512], x), axis=1, kind="stable")[:, :k]
    return out


def recall(true_idx, idx):
    return MU.recall(true_idx, idx)


def margin(ours, theirs):
    """How far two means of per-seed recalls may lie apart: the larger of 0.01 (the uint8 fixture's margin) and three standard
    errors of the difference of the two means."""
    ours, theirs = np.asarray(ours, np.float64), np.asarray(theirs, np.float64)
    se = np.sqrt(ours.var(ddof=1) / len(ours) + theirs.var(ddof=1) / len(theirs))
    return max(0.01, 3.0 * float(se))
