"""A step-exact restatement of the search-graph pruning pass (csrc/prune.hip and the glue of csrc/searchgraph.hip) in float64
numpy: test infrastructure, nothing under pynndescent_amd/ imports it.

What is restated, and from where:
  * csrc/prune.hip k_diversify_rows<FAM, AWARE> :41-94 and k_diversify_rows_wide<FAM, AWARE> :174-231 (one walk, two forms: the row in
    lanes for k <= 64, in LDS for k 65-256) -> ``diversify_rows``.  Position 0 is always kept (:60, :195); the walk stops at the
    first -1 (:63, :200); entry j is tested against the entries kept so far, in position order (:67-80, :204-213), those with a
    stored distance > PRUNE_EPS only (:72, :206); the row's own vertex as a comparison point takes the stored d(i, j) (:74, :207);
    the test is strict, d < lim (:75, :208), lim = d(i, j) -- times factor(j) times alpha in the degree-aware variant (:53-59, :65,
    :190-193, :202), which has no coin; kept entries are packed to the front in order, the tail is (-1, +inf) (:83-93, :217-230).
    Precondition: position 0 holds an id wherever position 1 does (the kernel -- like the reference -- reads the point of an
    entry it kept without looking at its id).
  * k_diversify_csr<FAM, AWARE> :103-159 and k_diversify_csr_wide<FAM, AWARE> :233-296 -> ``diversify_csr``.  Rows of length <= 1 are left
    alone (:114, :245).  order[] = the storage positions by ascending (weight, position) (:127-132, :265-271).  The standard walk
    starts at rank 1, the aware walk at rank 0 and skips entries of weight 0 (:134-137, :273-276).  Entry j = order[idx] is tested
    against kk < idx: the retained flag and the weight come from l = order[kk], the comparison POINT from storage position kk in
    the standard variant and from l in the aware one (:140-146, :279-284); the standard variant has the PRUNE_EPS guard on the
    weight of l, the aware one has none and takes w_j for the distance where that weight is <= PRUNE_EPS (:144-149, :283-285);
    the own vertex takes w_j (:149, :285); standard: d < w_j, aware: d * factor(j) < w_j (:150, :286).  Pruned entries get
    weight 0 at the end (:158, :294-295): the weights the walk reads are the incoming ones.  The launcher hands the kernels
    seed ^ 0x51ED270B (:353-376) and the coin applies in both variants.
  * k_degree_prune :298-326 -> ``degree_prune``: rows longer than max_degree keep the entries <= sorted(row)[max_degree]; on stored
    float32 values only, exact, no radius.
  * prune_coin :30-35 with common.h nnd_prune_coin_word / nnd_hash3 -> ``coin``: the hash of (seed, row, a * 256 + b), its top 24
    bits times 2^-24 against the float32 probability: exact in float64.
  * csrc/searchgraph.hip nnd_search_graph_impl :223-352 -> ``search_graph_from_forward``: 0 -> FLOAT32_EPS (k_sg_compact :131-151),
    COO -> CSR in row order, the csr pass, the union max(F', F'^T) without the diagonal (:152-191), max_degree =
    round-half-even(multiplier * n_neighbors) (:322), degree prune, binarise, columns sorted (:192-208); the four stage counts and
    min_distance (:340-348).

Arithmetic.  The kernels take pair distances of the PREPARED rows from metric.h nnd_row_pair_dist :181-192.  The model evaluates
the same form in float64 and attaches an a-priori float32 radius to every value, never a measured one:
  * codes 1-5: the Gram form on the prepared rows -- descent_reference.Prepared.block, the same rows, conversion and
    any-summation-order radius.
  * code 0 is the DIFFERENCE form S = sum (p - q)^2 over dp terms, not the Gram form that Prepared bounds.  With u = 2^-24: every
    term carries the roundings of p - q and of the square (or one, where the compiler fuses the square into the sum), and the sum
    of dp non-negative terms in ANY order at most dp - 1 more on a term: |fl(S') - S'| <= ((1 + u)^(dp + 2) - 1) S' <=
    (dp + 4) u S' =: g S', S' being the exact sum over the float32 prepared rows.  Those rows are themselves rounded:
    |fl(x - m) - (x - m)| <= u |x - m| per component (Prepared's docstring; an error of the mean is a translation and moves
    nothing), so |S' - S| <= e := 2 u (|a| + |b|) |a - b| + u^2 (|a| + |b|)^2.  Radius: g S + (1 + g) e.  It scales with the
    distance itself; the Gram radius (dp + 8) u (|a| + |b|)^2 would be valid too, and flag most rows of clustered data.
  * exact=True (the lattice): integer coordinates, the point set closed under negation, dp (2 R)^2 < 2^24 -- every difference,
    square and partial sum is an exact integer: radius 0.
  * stored distances and weights that come in are the kernels' own float32 values: radius 0.  The own-vertex rule hands one of
    them on as the distance: radius 0 too.
  * the degree-aware factors are float32 expressions that the device compiler may contract into fused multiply-adds, so no bit
    equality is claimed.  Forward: ratio = deg / max_degree, ratio - 1, base_rate * excess, 1 + ., d_j * factor, * alpha: six
    roundings at most.  Csr: ratio, ratio - 1, 0.04f * aggressiveness, * excess, 1 + ., d * factor: six.  A rounding moves a
    value v by at most u |v| <= ulp32(v), the clamps (fmin / fmax against float32 constants) only shrink an error, and the
    errors of the factor's ingredients enter the product scaled by base_rate * ratio / factor < 1: six ulps of the product in
    all.  The model evaluates the expressions in float64 and widens the decision's interval by AWARE_ULPS = 8 float32 ulps of
    the product (six roundings, their second-order terms and the float64 evaluation itself).  Where the factor is exactly 1 --
    degree <= max_degree: both clamps return the constant -- and alpha is 1 the product is the stored value: no widening.

Ambiguity (narrow on purpose).  A decision "entry j is pruned" is the OR of its tests.  It is clear when a test passes clearly
(the interval of d lies below the limit, coin true) or when no test can pass; it is unclear when no test passes clearly and one
was taken on an interval that contains the limit and is not exact.  A ROW is flagged iff one of ITS OWN decisions was unclear.
``n_unclear`` counts the entries whose fate is then not pinned: the unclear one and every entry the walk visits after it in that
row (their tests depend on what was kept).  That number bounds how far a stage count may lie from the model's.
"""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from tests.descent_reference import Prepared  # noqa: F401  (the cases and tests take it from here)
from tests.forest_reference import hash3v
from tests.search_reference import U24, _ulp32, hash3

EPS32 = float(np.float32(1.1920929e-07))  # PRUNE_EPS / SG_EPS: np.finfo(np.float32).eps
CSR_SEED = 0x51ED270B
WIDE_K = 256                               # common.h NND_WIDE_K
AWARE_ULPS = 8.0
C004 = float(np.float32(0.04))
R_FORWARD, R_CSR = 1, 2
REASONS = {R_FORWARD: "a forward d < lim test", R_CSR: "a csr d < w test"}
CHUNK = 8192

RowsResult = namedtuple("RowsResult", ["ids", "dists", "kept", "flags", "n_unclear"])
# ids / dists: (n, k) int32 / float32, packed, tail (-1, +inf); kept: (n, k) bool by INPUT position; flags: (n,) uint8 R_* bits
CsrResult = namedtuple("CsrResult", ["data", "flags", "n_unclear"])
GraphResult = namedtuple("GraphResult", [
    "indptr", "indices",                      # the final search graph, binary, columns sorted
    "f_indptr", "f_indices", "f_data",        # F: the forward matrix in row order (0 -> FLOAT32_EPS)
    "fp_data",                                # F': F's weights after the csr pass (pruned: 0)
    "u_indptr", "u_indices", "u_data",        # the union before degree_prune
    "stats",                                  # forward_nnz, reverse_nnz, union_nnz, final_nnz, min_distance (np.float32)
    "flags", "tainted",                       # (n,): the csr pass's flags; rows whose final row depends on a flagged row
    "n_unclear",
])


def reason_text(bits):
    return ", ".join(t for b, t in REASONS.items() if bits & b) or "clear"


def coin_word(a, b):
    """common.h nnd_prune_coin_word: (entry, compared entry) -> the hash's third word."""
    return a * WIDE_K + b


def coin(seed, row, a, b, prob):
    """prune.hip prune_coin on arrays: (float)(h >> 8) * 2^-24 < prob, prob a float32.  h >> 8 < 2^24 converts exactly and the
    product is a power-of-two scaling: the float32 comparison is the float64 one."""
    p = float(np.float32(prob))
    if p >= 1.0:
        return np.ones(np.broadcast(row, a, b).shape, bool)
    h = hash3v(seed & 0xFFFFFFFF, row, coin_word(np.asarray(a, np.uint64), np.asarray(b, np.uint64)))
    return (h >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 < p


def base_rate_of(aggressiveness):
    """prune.hip :332, :343: 0.04f * fmaxf(0, aggressiveness), one float32 product on the host."""
    return float(np.float32(0.04) * np.float32(max(0.0, float(np.float32(aggressiveness)))))


def forward_max_degree(multiplier, n_neighbors):
    """searchgraph.hip :267 (pynndescent_.py:1478): int(multiplier * n_neighbors), at least 1."""
    v = float(np.float32(multiplier) * np.float32(n_neighbors))
    return int(v) if v > 1.0 else 1


def compute_degrees(idx):
    """k_sg_degrees (searchgraph.hip :103-110, pynndescent_.py:406-418): entries of the row + occurrences as a neighbour."""
    idx = np.asarray(idx)
    n = idx.shape[0]
    valid = idx >= 0
    return (valid.sum(1) + np.bincount(idx[valid], minlength=n)[:n]).astype(np.int32)


def compute_degrees_csr(indptr, indices):
    """k_sg_degrees_csr (searchgraph.hip :112-121, pynndescent_.py:591-622)."""
    n = len(indptr) - 1
    ind = np.asarray(indices[: indptr[-1]])
    return (np.diff(indptr) + np.bincount(ind[(ind >= 0) & (ind < n)], minlength=n)[:n]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ distances
def pair_dist(prep, a, b):
    """(mid, radius) of nnd_row_pair_dist of row a[r] to the rows b[r, :]: two (m, J) float64 arrays."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if prep.code != 0:
        mid, rad = prep.block(a[:, None], b)
        return mid[:, 0, :], rad[:, 0, :]
    df = prep.rows[a][:, None, :] - prep.rows[b]
    mid = (df * df).sum(-1)
    if prep.exact:
        return mid, np.zeros_like(mid)
    dp = (prep.d + 3) & ~3
    g = (dp + 4) * U24
    ll = prep.len[a][:, None] + prep.len[b]
    e = 2.0 * U24 * ll * np.sqrt(mid) + (U24 * ll) ** 2
    return mid, g * mid + (1.0 + g) * e


def _less(mid, rad, lim, lim_rad):
    """(mid < lim, the interval contains the limit and is not exact)."""
    unclear = (mid - rad < lim + lim_rad) & (mid + rad >= lim - lim_rad) & ((rad > 0.0) | (lim_rad > 0.0))
    return mid < lim, unclear


# ------------------------------------------------------------------------------------------------ forward pass
def _forward_factors(ids, degree, max_degree, base_rate):
    """prune.hip :53-59 / :190-193 in float64: 1, or clamp(1 + base_rate * min(ratio - 1, 2), 0.8f, 1.2f) where ratio > 1
    (deg / max_degree rounds monotonically and 1 is a float32: ratio > 1 iff deg > max_degree)."""
    deg = np.asarray(degree, np.int64)[np.maximum(ids, 0)]
    ratio = deg / float(max_degree)
    f = np.clip(1.0 + base_rate * np.minimum(ratio - 1.0, 2.0), float(np.float32(0.8)), float(np.float32(1.2)))
    return np.where((ids >= 0) & (deg > max_degree), f, 1.0)


def diversify_rows(prep, idx, dist, *, aware=False, prob=1.0, seed=0, degree=None, max_degree=1, base_rate=0.0, alpha=1.0):
    """k_diversify_rows / k_diversify_rows_wide on an (n, k) graph; returns a RowsResult."""
    ids = np.asarray(idx, np.int64)
    n, k = ids.shape
    assert n == prep.n and k <= WIDE_K
    d32 = np.asarray(dist, np.float32)
    dd = d32.astype(np.float64)
    assert k < 2 or not ((ids[:, 0] < 0) & (ids[:, 1] >= 0)).any(), "position 0 must hold an id where position 1 does"
    alpha = float(np.float32(alpha))
    walked = np.zeros((n, k), bool)
    if k > 1:
        walked[:, 1:] = np.logical_and.accumulate(ids[:, 1:] >= 0, axis=1)
    if aware:
        fac = _forward_factors(ids, degree, max_degree, base_rate)
        lim = dd * fac * alpha
        with np.errstate(invalid="ignore"):
            lim_rad = np.where((fac == 1.0) & (alpha == 1.0) | ~np.isfinite(lim), 0.0, AWARE_ULPS * _ulp32(lim))
    else:
        lim, lim_rad = dd, np.zeros((n, k))
    kept = np.zeros((n, k), bool)
    kept[:, 0] = True
    first_unclear = np.full(n, k, np.int64)   # the position of the row's first unclear decision
    for j in range(1, k):
        for s in range(0, n, CHUNK):
            r = s + np.nonzero(walked[s:s + CHUNK, j])[0]
            if not len(r):
                continue
            cid = ids[r, :j]
            cand = kept[r, :j] & (dd[r, :j] > EPS32)
            mid, rad = pair_dist(prep, ids[r, j], np.maximum(cid, 0))
            own = cid == r[:, None]
            mid, rad = np.where(own, dd[r, j][:, None], mid), np.where(own, 0.0, rad)
            lt, un = _less(mid, rad, lim[r, j][:, None], lim_rad[r, j][:, None])
            if not aware:
                cand = cand & coin(seed, r[:, None], j, np.arange(j)[None, :], prob)
            sure = (cand & lt & ~un).any(1)
            unclear = ~sure & (cand & un).any(1)
            kept[r, j] = ~(cand & lt).any(1)
            first_unclear[r[unclear]] = np.minimum(first_unclear[r[unclear]], j)
    flags = np.where(first_unclear < k, R_FORWARD, 0).astype(np.uint8)
    n_unclear = int((walked & (np.arange(k)[None, :] >= first_unclear[:, None])).sum())
    o = np.argsort(~kept, axis=1, kind="stable")
    packed = np.take_along_axis(kept, o, 1)
    out_i = np.where(packed, np.take_along_axis(ids, o, 1), -1).astype(np.int32)
    out_d = np.where(packed, np.take_along_axis(d32, o, 1), np.float32(np.inf)).astype(np.float32)
    return RowsResult(out_i, out_d, kept, flags, n_unclear)


def explain_row(prep, idx_row, dist_row, i, *, aware=False, prob=1.0, seed=0, degree=None, max_degree=1, base_rate=0.0, alpha=1.0):
    """The walk of row i one test at a time, as the kernel takes it (first hit ends an entry's tests): the kept positions and
    the decision trail as text.  A second, sequential statement of ``diversify_rows`` -- the CPU tests hold the two together."""
    ids = np.asarray(idx_row, np.int64)
    dd = np.asarray(dist_row, np.float32).astype(np.float64)
    k = len(ids)
    alpha = float(np.float32(alpha))
    fac = _forward_factors(ids[None, :], degree, max_degree, base_rate)[0] if aware else np.ones(k)
    kept, trail = [0], []
    for j in range(1, k):
        if ids[j] < 0:
            trail.append("  [%d] id %d: the walk ends" % (j, ids[j]))
            break
        lim = dd[j] * fac[j] * alpha if aware else dd[j]
        lrad = 0.0 if not aware or (fac[j] == 1.0 and alpha == 1.0) or not np.isfinite(lim) else AWARE_ULPS * float(_ulp32(lim))
        verdict = "kept"
        for c in kept:
            if not dd[c] > EPS32:
                continue
            if ids[c] == i:
                mid, rad = dd[j], 0.0
            else:
                m, r = pair_dist(prep, ids[j:j + 1], np.maximum(ids[c:c + 1], 0)[None, :])
                mid, rad = float(m[0, 0]), float(r[0, 0])
            heads = aware or bool(coin(seed, np.uint64(i), j, c, prob))
            lt, un = _less(np.float64(mid), np.float64(rad), np.float64(lim), np.float64(lrad))
            if lt and heads:
                verdict = "pruned by [%d] id %d: d %.9g +- %.3g < lim %.9g +- %.3g%s" % (c, ids[c], mid, rad, lim, lrad, " UNCLEAR" if un else "")
                break
            if un and heads:
                verdict = "kept, UNCLEAR against [%d] id %d: d %.9g +- %.3g vs lim %.9g +- %.3g" % (c, ids[c], mid, rad, lim, lrad)
        else:
            kept.append(j)
        trail.append("  [%d] id %d d %.9g: %s" % (j, ids[j], dd[j], verdict))
    return kept, "\n".join(trail)


# ------------------------------------------------------------------------------------------------ csr pass
def _pad(indptr, *arrays):
    indptr = np.asarray(indptr, np.int64)
    n = len(indptr) - 1
    ln = np.diff(indptr)
    L = int(ln.max()) if n else 0
    pos = np.arange(L)[None, :]
    on = pos < ln[:, None]
    src = np.minimum(indptr[:-1, None] + pos, max(int(indptr[-1]) - 1, 0))
    return ln, on, src, [np.where(on, np.asarray(a)[src], 0) for a in arrays]


def diversify_csr(prep, indptr, indices, data, *, aware=False, prob=1.0, seed=0, degree=None, max_degree=1, aggressiveness=0.0):
    """k_diversify_csr / k_diversify_csr_wide; ``seed`` is the caller's (the launcher's xor is applied here).  Returns a
    CsrResult: the weights with the pruned entries at 0, the rows' flags, the entries that are not pinned."""
    seed = (int(seed) & 0xFFFFFFFF) ^ CSR_SEED
    data32 = np.asarray(data, np.float32)
    n = len(indptr) - 1
    assert n == prep.n
    out = data32.copy()
    flags = np.zeros(n, np.uint8)
    if not len(data32):
        return CsrResult(out, flags, 0)
    ln, on, src, (ids, w) = _pad(indptr, np.asarray(indices, np.int64), data32.astype(np.float64))
    L = ids.shape[1]
    assert L <= WIDE_K
    w = np.where(on, w, np.inf)
    order = np.argsort(w, axis=1, kind="stable")   # ascending weight, ties by position (:127-132)
    rows = np.arange(n)
    if aware:
        deg = np.where(ids < n, np.asarray(degree, np.int64)[np.minimum(ids, n - 1)], 0)
        ratio = deg / float(max(max_degree, 1))
        fac = np.maximum(1.0 + C004 * float(np.float32(aggressiveness)) * np.minimum(ratio - 1.0, 2.0), 1.0)
    retained = on.copy()
    first_unclear = np.full(n, L, np.int64)   # the walk step of the row's first unclear decision
    visited = np.zeros((n, L), bool)          # [row, step]: the walk tested an entry at this step
    for step in range(0 if aware else 1, L):
        for s in range(0, n, CHUNK):
            r = s + np.nonzero((ln[s:s + CHUNK] > step) & (ln[s:s + CHUNK] > 1))[0]
            if len(r):
                j = order[r, step]
                if aware:
                    r, j = r[w[r, j] != 0.0], j[w[r, j] != 0.0]
            if not len(r) or step == 0:
                continue
            visited[r, step] = True
            wj = w[r, j]
            l = order[r, :step]
            R = r[:, None]
            wl = w[R, l]
            cand = retained[R, l]
            if not aware:
                cand = cand & (wl > EPS32)
            idk = ids[R, l] if aware else ids[r, :step]
            mid, rad = pair_dist(prep, ids[r, j], idk)
            own = idk == R
            if aware:
                own = own | (wl <= EPS32)
            mid, rad = np.where(own, wj[:, None], mid), np.where(own, 0.0, rad)
            if aware:
                fj = fac[r, j][:, None]
                with np.errstate(invalid="ignore", over="ignore"):
                    mid, rad = mid * fj, rad * fj
                    rad = rad + np.where((fj == 1.0) | ~np.isfinite(mid), 0.0, AWARE_ULPS * _ulp32(mid))
            lt, un = _less(mid, rad, wj[:, None], 0.0)
            cand = cand & coin(seed, R, j[:, None], np.arange(step)[None, :], prob)
            sure = (cand & lt & ~un).any(1)
            unclear = ~sure & (cand & un).any(1)
            retained[r, j] = ~(cand & lt).any(1)
            first_unclear[r[unclear]] = np.minimum(first_unclear[r[unclear]], step)
    flags = np.where(first_unclear < L, R_CSR, 0).astype(np.uint8)
    n_unclear = int((visited & (np.arange(L)[None, :] >= first_unclear[:, None])).sum())
    out[src[on & ~retained]] = 0.0
    return CsrResult(out, flags, n_unclear)


def explain_csr_row(prep, ids, w32, i, *, aware=False, prob=1.0, seed=0, degree=None, max_degree=1, aggressiveness=0.0):
    """The csr walk of one row, test by test (the first hit ends an entry's tests): (retained flags, the trail as text)."""
    seed = (int(seed) & 0xFFFFFFFF) ^ CSR_SEED
    ids = np.asarray(ids, np.int64)
    w = np.asarray(w32, np.float32).astype(np.float64)
    ln = len(ids)
    retained = np.ones(ln, bool)
    if ln <= 1:
        return retained, "  (a row of %d entries is left alone)" % ln
    order = np.argsort(w, kind="stable")
    trail = []
    for step in range(0 if aware else 1, ln):
        j = int(order[step])
        if aware and w[j] == 0.0:
            trail.append("  rank %d = [%d] id %d: weight 0, skipped" % (step, j, ids[j]))
            continue
        fj = 1.0
        if aware:
            tgt = int(degree[ids[j]]) if ids[j] < prep.n else 0
            fj = max(1.0 + C004 * float(np.float32(aggressiveness)) * min(tgt / float(max(max_degree, 1)) - 1.0, 2.0), 1.0)
        verdict = "kept"
        for kk in range(step):
            l = int(order[kk])
            if not retained[l] or not (aware or w[l] > EPS32):
                continue
            idk = int(ids[l] if aware else ids[kk])
            if idk == i or (aware and w[l] <= EPS32):
                mid, rad = w[j], 0.0
            else:
                m, r = pair_dist(prep, ids[j:j + 1], np.array([[idk]]))
                mid, rad = float(m[0, 0]), float(r[0, 0])
            if aware:
                mid, rad = mid * fj, rad * fj + (0.0 if fj == 1.0 or not np.isfinite(mid) else AWARE_ULPS * float(_ulp32(mid * fj)))
            heads = bool(coin(seed, np.uint64(i), j, kk, prob))
            lt, un = _less(np.float64(mid), np.float64(rad), np.float64(w[j]), 0.0)
            if lt and heads:
                retained[j] = False
                verdict = "pruned at kk %d (weight of [%d], point id %d): d %.9g +- %.3g < w %.9g%s" % (kk, l, idk, mid, rad, w[j], " UNCLEAR" if un else "")
                break
            if un and heads:
                verdict = "kept, UNCLEAR at kk %d (weight of [%d], point id %d): d %.9g +- %.3g vs w %.9g" % (kk, l, idk, mid, rad, w[j])
        trail.append("  rank %d = [%d] id %d w %.9g: %s" % (step, j, ids[j], w[j], verdict))
    return retained, "\n".join(trail)


# ------------------------------------------------------------------------------------------------ degree prune
def degree_prune(indptr, data, max_degree):
    """k_degree_prune: cut = sorted(row)[max_degree] for rows longer than max_degree; entries above the cut become 0 (every
    entry equal to the cut stays: the row may remain longer than max_degree, pynndescent_.py:728-738)."""
    out = np.asarray(data, np.float32).copy()
    if not len(out):
        return out
    ln, on, src, (w,) = _pad(indptr, out)
    w = np.where(on, w, np.float32(np.inf)).astype(np.float32)
    if w.shape[1] <= max_degree:
        return out
    cut = np.sort(w, axis=1)[:, max_degree]
    drop = on & (ln > max_degree)[:, None] & (w > cut[:, None])
    out[src[drop]] = 0.0
    return out


# ------------------------------------------------------------------------------------------------ the glue
def union_max(f_indptr, f_indices, fp_data):
    """searchgraph.hip k_sg_edge_keys .. k_sg_unique (pynndescent_.py:1588-1604): F' without its zeros, max(F', F'^T) without the
    diagonal, columns sorted: (indptr, indices, data, nnz of F')."""
    n = len(f_indptr) - 1
    fp = sp.csr_array((np.asarray(fp_data, np.float32).copy(), np.asarray(f_indices).copy(), np.asarray(f_indptr).copy()), shape=(n, n))
    fp.eliminate_zeros()
    reverse_nnz = int(fp.nnz)
    fp.sort_indices()
    rev = fp.transpose().tocsr()
    rev.sort_indices()
    u = fp.maximum(rev).tocsr()
    u.setdiag(0.0)
    u.eliminate_zeros()
    u.sort_indices()
    return u.indptr.astype(np.int32), u.indices.astype(np.int32), u.data.astype(np.float32), reverse_nnz


def final_graph(u_indptr, u_indices, p_data):
    """k_sg_flags .. k_sg_final_ptr: the union's entries that degree_prune left, as (indptr, indices)."""
    n = len(u_indptr) - 1
    alive = np.asarray(p_data) != 0.0
    u_row = np.repeat(np.arange(n), np.diff(u_indptr))
    return np.concatenate([[0], np.cumsum(np.bincount(u_row[alive], minlength=n))]).astype(np.int32), np.asarray(u_indices)[alive]


def final_max_degree(multiplier, n_neighbors):
    """searchgraph.hip :322: nearbyintf(multiplier * n_neighbors), half to even as np.round (pynndescent_.py:1606-1609)."""
    return int(np.round(float(np.float32(multiplier) * np.float32(n_neighbors))))


def search_graph_from_forward(prep, fwd_idx, fwd_dist, n_neighbors, *, multiplier=1.5, prob=1.0, aware=False, aggressiveness=1.0,
                              seed=0):
    """nnd_search_graph_impl behind its forward pass, on the forward rows (n, k) as the pass left them (pruned slots -1)."""
    rows = np.asarray(fwd_idx, np.int32)
    n = rows.shape[0]
    dd = np.asarray(fwd_dist, np.float32).copy()
    dd[dd == 0.0] = np.float32(EPS32)                                   # k_sg_compact :140-143 (pynndescent_.py:1525)
    keep = rows >= 0
    f_indptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
    f_indices, f_data = rows[keep].astype(np.int32), dd[keep]           # row order: ascending distance
    forward_nnz = int(f_data.shape[0])
    min_distance = np.float32(f_data.min()) if forward_nnz else np.float32(0.0)
    kw = dict(aware=True, degree=compute_degrees_csr(f_indptr, f_indices), max_degree=int(n_neighbors),
              aggressiveness=aggressiveness) if aware else {}
    res = diversify_csr(prep, f_indptr, f_indices, f_data, prob=prob, seed=seed, **kw)
    u_indptr, u_indices, u_data, reverse_nnz = union_max(f_indptr, f_indices, res.data)
    p_data = degree_prune(u_indptr, u_data, final_max_degree(multiplier, n_neighbors))
    indptr, indices = final_graph(u_indptr, u_indices, p_data)
    tainted = res.flags != 0
    flagged = np.nonzero(tainted)[0]
    for t in flagged:   # a flagged row's entries may or may not reach the rows they point at
        tainted[f_indices[f_indptr[t]:f_indptr[t + 1]]] = True
    stats = {"forward_nnz": forward_nnz, "reverse_nnz": reverse_nnz, "union_nnz": int(len(u_data)), "final_nnz": int(len(indices)),
             "min_distance": min_distance}
    return GraphResult(indptr, indices, f_indptr, f_indices, f_data, res.data, u_indptr, u_indices, u_data, stats, res.flags,
                       tainted, res.n_unclear)


def csr_rows_equal(indptr_a, indices_a, indptr_b, indices_b):
    """(n,) bool: row i of the two CSR patterns holds the same columns in the same order."""
    n = len(indptr_a) - 1
    la, lb = np.diff(indptr_a), np.diff(indptr_b)
    same = la == lb
    L = int(max(la.max(), lb.max(), 1))
    pos = np.arange(L)[None, :]
    a = np.where(pos < la[:, None], np.asarray(indices_a)[np.minimum(indptr_a[:-1, None] + pos, max(len(indices_a) - 1, 0))], -1) if len(indices_a) else np.full((n, L), -1)
    b = np.where(pos < lb[:, None], np.asarray(indices_b)[np.minimum(indptr_b[:-1, None] + pos, max(len(indices_b) - 1, 0))], -1) if len(indices_b) else np.full((n, L), -1)
    return same & (a == b).all(1)


__all__ = ["Prepared", "hash3", "coin", "coin_word", "diversify_rows", "diversify_csr", "degree_prune", "search_graph_from_forward"]
