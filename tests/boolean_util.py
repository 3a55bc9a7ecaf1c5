"""The nine boolean metrics (reference distances.py:259-552) as functions of the exact Gram counts of indicator rows, in float64
and in float32 numpy; recall counted by distance; the fixture inputs of tests/golden/make_golden_boolean.py; and the family for
the step-exact models (tests/descent_reference.py and its siblings, used unchanged).  Test helpers only.

For indicator rows b_x = (x != 0):  c = <b_x, b_y> = n_TT,  a = nnz(x),  b = nnz(y),  ne = a + b - 2c,  n_FF = d - a - b + c.
The kernels' convention (DESIGN.md "Boolean metrics"): jaccard is the reference's alternative_jaccard, with FLT_MAX where the
reference has +inf (c = 0 on a non-empty union); both correct to exactly 1."""
import os

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
# name -> metric code (include/pynnd_amd.h); rogerstanimoto and sokalmichener are one formula under two names
CODES = {"jaccard": 8, "dice": 9, "sokalsneath": 10, "matching": 11, "rogerstanimoto": 12, "sokalmichener": 13, "kulsinski": 14,
         "russellrao": 15, "yule": 16}
METRICS = tuple(CODES)
RATIONAL = tuple(m for m in METRICS if m != "jaccard")
K = 10
SEEDS = (3, 17, 42)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boolean_metrics.npz")


def _dist(metric, c, a, b, d, ft):
    """The kernel distance from the counts (broadcast), every operation in the float type `ft`: numpy rounds each operation
    once (IEEE), fuses nothing, and every operand below is an integer below 2^24 or a product the device forms the same way."""
    c, a, b, d = (np.asarray(v, ft) for v in np.broadcast_arrays(c, a, b, d))
    ne = a + b - (c + c)
    one, zero = ft(1.0), ft(0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if metric == "jaccard":
            union = c + ne
            r = -np.log2(np.where(c > 0, c, one) / np.where(union > 0, union, one))
            r = np.where(r > 0, r, zero)
            return np.where(union == 0, zero, np.where(c == 0, ft(FLT_MAX), r))
        if metric in ("dice", "sokalsneath"):
            w = ft(2.0) if metric == "dice" else ft(0.5)
            den = w * c + ne
            return np.where(ne == 0, zero, ne / np.where(ne == 0, one, den))
        if metric == "matching":
            return ne / d
        if metric in ("rogerstanimoto", "sokalmichener"):
            return (ne + ne) / (d + ne)
        if metric == "kulsinski":
            return np.where(ne == 0, zero, (ne - c + d) / (ne + d))
        if metric == "russellrao":
            return np.where((c == a) & (c == b), zero, (d - c) / d)
        if metric == "yule":
            tf, tf_ = a - c, b - c
            ff = d - a - b + c
            p = tf * tf_
            skip = (tf == 0) | (tf_ == 0)
            return np.where(skip, zero, (p + p) / np.where(skip, one, c * ff + p))
    raise ValueError(metric)


def dist_from_counts(metric, c, a, b, d):
    """float64 kernel distance from the counts."""
    return _dist(metric, c, a, b, d, np.float64)


def dist_from_counts_f32(metric, c, a, b, d):
    """The float32 expression the device evaluates (IEEE division); jaccard's log2 is numpy's here, the hardware's there."""
    return _dist(metric, c, a, b, d, np.float32)


def indicators(x):
    return (np.asarray(x) != 0).astype(np.float64)


def counts(a, b):
    """(c, na, nb) of every (a[i], b[j]) as float64 integers."""
    ia, ib = indicators(a), indicators(b)
    return ia @ ib.T, ia.sum(1)[:, None], ib.sum(1)[None, :]


def dist(metric, a, b, f32=False):
    """(len(a), len(b)) matrix of the kernel distance (float64, or the float32 expression)."""
    c, na, nb = counts(a, b)
    return _dist(metric, c, na, nb, float(np.asarray(a).shape[1]), np.float32 if f32 else np.float64)


def dist_pairs(metric, a, b, f32=False):
    """The kernel distance of the pairs (a[i], b[i]) for any leading shape."""
    ia, ib = indicators(a), indicators(b)
    return _dist(metric, (ia * ib).sum(-1), ia.sum(-1), ib.sum(-1), float(ia.shape[-1]), np.float32 if f32 else np.float64)


def correct(metric, v):
    """What the class hands out (float64): 1 - 2^-v for jaccard (correct_alternative_jaccard), the value itself otherwise."""
    v = np.asarray(v, np.float64)
    return 1.0 - np.power(2.0, -v) if metric == "jaccard" else v


def brute(metric, x, q=None, k=K):
    """(ids, distances) of the k nearest rows of x for every row of q (default x, the row included) under (distance, id)."""
    q = x if q is None else q
    dm = dist(metric, q, x)
    idx = np.argsort(dm, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(dm, idx, 1)


def distance_recall(metric, x, idx, q=None, k=K, kth=None):
    """Recall counted by distance: a returned neighbour counts if its true distance is <= the k-th true distance (the family
    is full of ties: id recall would punish legitimate tie choices).  Negative ids and repeated ids do not count."""
    q = x if q is None else q
    dm = dist(metric, q, x)
    if kth is None:
        kth = np.sort(dm, axis=1)[:, k - 1]
    idx = np.asarray(idx)[:, :k]
    hits = 0
    for r in range(idx.shape[0]):
        ids = np.unique(idx[r][idx[r] >= 0])
        hits += int(np.sum(dm[r, ids] <= kth[r]))
    return hits / float(idx.shape[0] * k)


def fixture_data(n=2000, d=48, nq=200, seed=11):
    """Clustered binary rows: 24 cluster prototypes of density 0.1 .. 0.4, every member a prototype with each bit flipped with
    probability 0.04; two all-zero rows, one all-ones row, five exact duplicates; held-out queries, one of them all-zero."""
    rng = np.random.RandomState(seed)
    nc = 24
    dens = rng.uniform(0.1, 0.4, nc)
    proto = rng.random_sample((nc, d)) < dens[:, None]
    lab = rng.randint(0, nc, n + nq)
    x = proto[lab] ^ (rng.random_sample((n + nq, d)) < 0.04)
    x = x.astype(np.float32)
    x[[7, 500]] = 0.0
    x[900] = 1.0
    x[[100, 101, 102, 103, 104]] = x[[1100, 1101, 1102, 1103, 1104]]
    if nq > 5:
        x[n + 5] = 0.0
    return np.ascontiguousarray(x[:n]), np.ascontiguousarray(x[n:])


# --------------------------------------------------------------------------------------- the step-exact models' family
# jaccard's -log2 is the hardware's logarithm of one correctly rounded quotient: 2^-20 absolute plus 4 float32 ulps, the a-priori
# band of the log term in tests/proxy_util.py (derived there from the operations, never measured)
LOG_TERM_ABS = 2.0 ** -20


def _ulp32(v):
    a = np.minimum(np.abs(np.asarray(v, np.float64)), FLT_MAX).astype(np.float32)
    with np.errstate(over="ignore"):
        return np.spacing(a).astype(np.float64)


def kernel_interval(metric, c, a, b, d):
    """(mid, radius) of the float32 kernel distance from exact counts: radius 0 for the eight rational formulas (the model
    evaluates the same float32 expression on the same integers), the log term's band for jaccard."""
    mid = _dist(metric, c, a, b, d, np.float32).astype(np.float64)
    if metric != "jaccard":
        return mid, np.zeros_like(mid)
    return mid, np.where((mid < FLT_MAX) & (mid > 0.0), LOG_TERM_ABS + 4.0 * _ulp32(mid), 0.0)


def make_prepared(data, metric):
    """A tests/descent_reference.py Prepared of the family: indicator rows, nrm = nnz, distances by kernel_interval; the self
    pair is 0.  (Built here so that importing this module does not import the oracle.)"""
    from tests import descent_reference as DR

    class BoolPrepared(DR.Prepared):
        def __init__(self, rows, name):
            ind = (np.asarray(rows) != 0).astype(np.float32)
            super().__init__(ind, "inner_product", True)  # rows as given, nrm = |x|^2 = nnz, every sum exact
            self.metric, self.code, self.true_d = name, CODES[name], int(ind.shape[1])
            self.exact = name != "jaccard"
            self.self_mid, self.self_rad = np.zeros(self.n), np.zeros(self.n)

        def block(self, a_ids, b_ids):
            c = self.rows[a_ids] @ self.rows[b_ids].transpose(0, 2, 1)
            return kernel_interval(self.metric, c, self.nrm[a_ids][:, :, None], self.nrm[b_ids][:, None, :], float(self.true_d))

    return BoolPrepared(data, metric)


def make_builder(x, metric, k=15, n_trees=2, leaf_size=None, mc=None, n_iters=None, delta=0.001, seed=1, join_blocks=1, flags=0):
    """tests/gpu_util.py make_builder for the family's codes (the oracle does not know them)."""
    from oracle import oracle as O
    from pynndescent_amd import _capi

    n, d = x.shape
    state, _, tree_states = O.draw_rng_states(seed, max(n_trees, 1))
    b = _capi.Builder(n, d, CODES[metric], k, n_trees, O.default_leaf_size(k) if leaf_size is None else leaf_size, 200,
                      min(60, k) if mc is None else mc, O.default_n_iters(n) if n_iters is None else n_iters, delta, state,
                      tree_states[0], join_blocks=join_blocks, flags=flags)
    b.set_data_host(np.ascontiguousarray(x, np.float32))
    return b


def random_rows(n, d, seed, density=0.3):
    """n x d binary rows with an all-zero row (3), an all-ones row (4) and a duplicate pair (5, 6)."""
    rs = np.random.RandomState(seed)
    x = (rs.random_sample((n, d)) < density).astype(np.float32)
    x[3], x[4], x[6] = 0.0, 1.0, x[5]
    return x


def golden():
    """The fixture as a dict of arrays (indicators back to float32)."""
    with np.load(GOLDEN) as f:
        g = {key: f[key] for key in f.files}
    g["x"], g["queries"] = g["x"].astype(np.float32), g["queries"].astype(np.float32)
    return g


def tie_free_leaves(sizes=(10, 11, 12, 13, 14), repeats=60):
    """(rows, leaf_array) on which no point has two run-mates at the same distance under any of the nine formulas, so that the
    k smallest of a leaf are decided by the distances alone and the leaf model flags nothing (its one ambiguity is a tie at the
    k-th place, whatever the metric: tests/leaf_reference.py).  A leaf of m points: every pair (p, q) owns w(p, q) = 1 + (p + q)
    mod m columns that are set in both rows and in no other row of the leaf, so c(p, q) = w(p, q), which for a fixed p takes
    m - 1 different values; private columns bring every row of the leaf to the same nnz A.  Then ne = 2A - 2c, and every formula
    is strictly monotone in c at fixed A and d.  Leaves reuse the same columns: points of different leaves are never run-mates."""
    designs, width = {}, 0
    for m in sizes:
        cols = [[] for _ in range(m)]
        nxt = 0
        for p in range(m):
            for q in range(p + 1, m):
                w = 1 + (p + q) % m
                for r in (p, q):
                    cols[r].extend(range(nxt, nxt + w))
                nxt += w
        top = max(len(c) for c in cols)
        for p in range(m):
            extra = top - len(cols[p])
            cols[p].extend(range(nxt, nxt + extra))
            nxt += extra
        designs[m], width = cols, max(width, nxt)
    order = [m for _ in range(repeats) for m in sizes]
    n = sum(order)
    x = np.zeros((n, width), np.float32)
    la = np.full((len(order), max(sizes)), -1, np.int32)
    at = 0
    for leaf, m in enumerate(order):
        for p in range(m):
            x[at + p, designs[m][p]] = 1.0
        la[leaf, :m] = np.arange(at, at + m)
        at += m
    return x, la
