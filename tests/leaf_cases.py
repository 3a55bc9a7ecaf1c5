"""The cases of the step-exact leaf-seeding tests (tests/test_leaf_reference_cpu.py, tests/test_gpu_leaf_exact.py) and their
ambiguity caps.  The leaf arrays are built HERE, not by the forest: a case reaches the kernel instance it names whatever the
forest would do at its k.

Which instance a (k, longest run) pair reaches (csrc/leaf_plan.h nnd_leaf_table, the one statement of this table in the library;
restated by leaf_reference.forms, and the two compared pair by pair in tests/test_leaf_plan_cpu.py).  The names are written
without the kernels' first template argument, the metric family: NND_CODES_BOOL for the boolean metrics (the leaf cases of
tests/test_gpu_boolean_metrics.py), NND_CODES_ANY for every case of this file.

    longest run   k <= 16                        k 17-32                 k 33-64                 k > 64
    <= 64         k_leaf_join<4,8,64,true>       k_leaf_join_sym<6,8>    k_leaf_join<4,8,64>     k_leaf_join_rb<8,8,true>
    65-80         <4,4,64,true> + <5,8,64,true>  k_leaf_join_sym<6,8>    k_leaf_join<5,8,64>     k_leaf_join_rb<8,8,true>
    81-96         k_leaf_join<6,8,64,true>       k_leaf_join_sym<6,8>    k_leaf_join<6,8,64>     k_leaf_join_rb<8,8,true>
    97-128        k_leaf_join_rb<8,8>            sym<6> + sym<10>        k_leaf_join_rb<8,8>     k_leaf_join_rb<8,8,true>
    129-160       k_leaf_join_rb<10,8>           sym<6> + sym<10>        k_leaf_join_rb<10,8>    k_leaf_join_rb<10,8,true>
    > 160         k_leaf_join_rb<16,8>           k_leaf_join_rb<16,8>    k_leaf_join_rb<16,8>    k_leaf_join_rb<16,8,true>

The merges behind them (csrc/merge.h): nnd_merge_rows_q16b in the <.,.,64,true> instances, nnd_merge_rows_q32b in
k_leaf_join_sym, nnd_merge_row_regs<1 | 2 | 3 | 4> in the plain k_leaf_join and k_leaf_join_rb instances (one candidate chunk
per 64 run-mates, so the sizes 64 / 65 and 128 / 129 change the path inside one instance), nnd_merge_row_lds in the
<.,8,true> instances.

Shape of a partition case: n in 3000..6000 and never a multiple of 64; ``rounds`` rounds, each a fresh random partition of all
n points into leaves whose sizes sit on the edges of tiles, size classes and row blocks (EDGES, each size up to the case's
longest at least once a round), half of the remaining leaves shorter than k + 1 (rows stay partly filled after round 1), the
others of any size up to the longest.  d picks the K blocking: 5 and 16 (one 32-wide block), 24 and 40, 64 (one full block),
130 (dp = 160: two blocks of 64 and a 32-wide tail).

Lattice twins (descent_cases.lattice_points: integer coordinates, the set closed under negation, every distance an exact
integer in any summation order): ids, distance bits and flags must be equal on every row without a tie at its k-th place.

Caps: at most 10 % of the rows of a float case may be flagged (the project's FLOAT_CAP), at most 2 % of a lattice case: the
merges test d < worst on the distance alone, so a distance tie at the k-th place is truly order dependent and the lattice cap
cannot be 0 as it is for the descent pin.  On lattice_points(4002, 16, 60) with random partitions into leaves of 17..256 points
0.07 % .. 0.67 % of the rows have such a tie (worst: k = 100 with leaves of 256).
"""
from collections import namedtuple

import numpy as np

from tests import descent_cases as DC
from tests import descent_reference as DR
from tests import metric_util as MU

FLOAT_CAP, LATTICE_CAP = DC.FLOAT_CAP, 0.02
EDGES = (2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 79, 80, 81, 95, 96, 97, 127, 128, 129, 159, 160, 161, 255, 256)

# kind: "partition" (above) | "chain" | "cut" | "garbage" (the host logic of nnd_launch_leaf_init_array, below)
Case = namedtuple("Case", ["name", "metric", "k", "d", "n", "longest", "rounds", "kind", "exact", "seed", "forms", "doc"])


def _c(name, metric, k, d, n, longest, forms, doc="", rounds=3, kind="partition", exact=False, seed=3):
    return Case("leaf_" + name, metric, k, d, n, longest, rounds, kind, exact, seed, tuple(forms), doc)


QW4, QW44, QW5, QW6 = ("k_leaf_join<%s,64,true>" % s for s in ("4,8", "4,4", "5,8", "6,8"))
P4, P5, P6 = ("k_leaf_join<%d,8,64>" % t for t in (4, 5, 6))
SYM6, SYM10 = "k_leaf_join_sym<6,8>", "k_leaf_join_sym<10,8>"
RB8, RB10, RB16 = ("k_leaf_join_rb<%d,8>" % t for t in (8, 10, 16))
W8, W10, W16 = ("k_leaf_join_rb<%d,8,true>" % t for t in (8, 10, 16))

FLOAT = {c.name: c for c in [
    # ---- k <= 16: quarter-wave merges, every lane of a 16-lane row an entry at k = 16 ----
    _c("qw4_k8_d5", "euclidean", 8, 5, 3001, 64, [QW4], "rows that end before the 16th lane; one 32-wide K block"),
    _c("qw45_k15_d40", "euclidean", 15, 40, 4001, 80, [QW44, QW5], "two size classes, m_lo = 64: the benchmark's shape"),
    _c("qw6_k16_d24", "euclidean", 16, 24, 4003, 96, [QW6], "rows of exactly 16"),
    _c("rb8_k16_d16", "euclidean", 16, 16, 4001, 128, [RB8], "nnd_merge_row_regs<1 | 2>, rows of 16"),
    _c("rb10_k8_d64", "euclidean", 8, 64, 4005, 160, [RB10], "nnd_merge_row_regs<1 | 2 | 3>; one full K block; three row blocks"),
    _c("rb16_k15_d130", "euclidean", 15, 130, 5001, 256, [RB16], "nnd_merge_row_regs<1 | 2 | 4>; three K blocks; four row blocks"),
    # ---- k 17..32: two rows per wave ----
    _c("sym6_k17_d16", "euclidean", 17, 16, 4001, 96, [SYM6], "one lane past the half row; passes of 64 rows"),
    _c("sym610_k30_d24", "euclidean", 30, 24, 5003, 160, [SYM6, SYM10], "both size classes, m_lo = 96: the reference's default k"),
    _c("sym610_k32_d130", "euclidean", 32, 130, 4001, 128, [SYM6, SYM10], "every lane of the 32-lane row an entry; three K blocks"),
    _c("rb16_k32_d40", "euclidean", 32, 40, 5001, 256, [RB16], "k <= 32 past the sym forms"),
    # ---- k 33..64: one row per wave, one entry per lane ----
    _c("plain4_k33_d5", "euclidean", 33, 5, 3001, 64, [P4], "nnd_merge_row_regs<1>"),
    _c("plain5_k40_d64", "euclidean", 40, 64, 4001, 80, [P5], "nnd_merge_row_regs<1 | 2> (m <= 64 takes one chunk)"),
    _c("plain6_k64_d24", "euclidean", 64, 24, 4003, 96, [P6], "every lane of the wave an entry"),
    _c("rb8_k40_d40", "euclidean", 40, 40, 4001, 128, [RB8], "nnd_merge_row_regs<1 | 2>"),
    _c("rb10_k64_d16", "euclidean", 64, 16, 4005, 160, [RB10], "every lane an entry; three chunks"),
    _c("rb16_k64_d24", "euclidean", 64, 24, 5001, 256, [RB16], "every lane an entry; four chunks"),
    # ---- k > 64: rows merged through LDS ----
    _c("wide8_k65_d24", "euclidean", 65, 24, 3001, 64, [W8], "one entry past the wave; the <8,8,true> form on short leaves"),
    _c("wide8_k256_d64", "euclidean", 256, 64, 4001, 128, [W8], "four entries a lane; no row ever fills"),
    _c("wide10_k100_d40", "euclidean", 100, 40, 4005, 160, [W10], "two entries a lane"),
    _c("wide16_k200_d16", "euclidean", 200, 16, 5001, 256, [W16], "four entries a lane, four candidate chunks"),
    # ---- the other metrics on one quarter-wave form, one sym form and one row-block form each ----
] + [
    _c("%s_%s" % (metric, form), metric, k, 24, n, longest, fs, doc, rounds=2)
    for metric, doc in (("cosine", "unit rows, -log2 conversion"), ("dot", "code 2: zero rows at FLT_MAX, also against each other"),
                        ("inner_product", "code 3: 1 / <a, b> on the raw rows"), ("correlation", "code 4: constant rows"),
                        ("hellinger", "code 5: rows clipped at 0, some all zero"),
                        ("proxy_inner_product", "code 6: -log2 cos + 1 / sqrt<a, b> on the raw rows, zero rows at FLT_MAX"))
    for form, k, n, longest, fs in (("qw", 15, 3001, 80, [QW44, QW5]), ("sym", 30, 3003, 160, [SYM6, SYM10]), ("rb", 40, 3005, 200, [RB16]))
] + [
    # ---- the host logic of nnd_launch_leaf_init_array ----
    _c("chain_k15", "euclidean", 15, 24, 3001, 80, [QW44, QW5], "30 leaves of 40 points, leaf i shares its last point with leaf i + 1: "
       "30 rounds; then a partition of all points", rounds=31, kind="chain"),
    _c("cut_k15", "euclidean", 15, 24, 4001, 256, [RB16], "leaves of 257, 300, 512 and 513 points: cut into runs of 256, the one point "
       "left at 257 and 513 dropped, no pair across two runs", rounds=2, kind="cut"),
    _c("cut_k100", "euclidean", 100, 24, 4001, 256, [W16], "the same array on wide rows", rounds=2, kind="cut"),
    _c("garbage_k30", "euclidean", 30, 24, 3001, 96, [SYM6], "rows with entries after their first -1, all-empty rows, one-point leaves, "
       "an array wider than its longest leaf", rounds=2, kind="garbage"),
]}

LATTICE = {c.name: c for c in [
    _c("lattice_qw_k15", "euclidean", 15, 16, 4002, 80, [QW44, QW5], "bit for bit", exact=True),
    _c("lattice_sym_k30", "euclidean", 30, 16, 4002, 160, [SYM6, SYM10], "bit for bit", exact=True),
    _c("lattice_plain_k40", "euclidean", 40, 16, 4002, 96, [P6], "bit for bit", exact=True),
    _c("lattice_rb_k40", "euclidean", 40, 16, 4002, 256, [RB16], "bit for bit", exact=True),
    _c("lattice_wide_k100", "euclidean", 100, 16, 4002, 256, [W16], "bit for bit", exact=True),
    _c("lattice_cut_k15", "euclidean", 15, 16, 4002, 256, [RB16], "leaves of 257, 300, 512 and 513 points, bit for bit: a pair across "
       "two runs would show", rounds=2, kind="cut", exact=True),
]}
ALL = dict(FLOAT, **LATTICE)
assert all(c.n % 64 and 3000 <= c.n <= 6000 for c in ALL.values())

# seeding on rows that are not empty (init_from_graph with a partial graph first): one case per merge form
BEFORE = ("leaf_qw45_k15_d40", "leaf_sym610_k30_d24", "leaf_rb8_k40_d40", "leaf_wide10_k100_d40", "leaf_lattice_sym_k30")

_ARRAYS, _DATA6 = {}, {}


def cap(case):
    return LATTICE_CAP if case.exact else FLOAT_CAP


def data(case):
    """descent_cases.data: clustered rows; hellinger rows clipped at 0 with zero rows; dot on normalised rows with zero rows.
    Code 6 takes the rows of tests/proxy_descent.py: the inner-product fixture with three zero rows."""
    if case.metric != "proxy_inner_product":
        return DC.data(case)
    if case.name not in _DATA6:
        x = MU.metric_data("inner_product", case.n, case.d, seed=11)[0]
        x[[7, 500, 1500]] = 0.0
        x.setflags(write=False)
        _DATA6[case.name] = x
    return _DATA6[case.name]


def prepared(case):
    """the prepared rows and the Gram-form distance of the case's metric (code 6: tests/proxy_descent.py ProxyPrepared)."""
    if case.metric == "proxy_inner_product":
        from tests.proxy_descent import ProxyPrepared
        return ProxyPrepared(data(case))
    return DR.Prepared(data(case), case.metric, case.exact)


def builder(case, **kw):
    """a builder on the case's rows, without a forest unless asked for (the oracle's metric table does not know code 6)."""
    kw.setdefault("n_trees", 0)
    if case.metric == "proxy_inner_product":
        from tests.proxy_descent import make_builder
    else:
        from tests.gpu_util import make_builder
        kw["metric"] = case.metric
    return make_builder(np.array(data(case)), k=case.k, **kw)


def _sizes(rng, n, longest, k):
    sizes = sorted({e for e in EDGES if e <= longest} | {longest})  # every edge size once, and the longest itself
    left = n - sum(sizes)
    assert left >= 2
    while left > 0:
        s = int(rng.randint(2, min(k, longest) + 1) if rng.randint(2) else rng.randint(2, longest + 1))
        s = min(s, left)
        if left - s == 1:  # never leave one point alone: a partition case covers every point in every round
            s = s + 1 if s < longest else s - 1
        sizes.append(s)
        left -= s
    return np.asarray(sizes)[rng.permutation(len(sizes))]


def _rows(leaves, width):
    out = np.full((len(leaves), width), -1, np.int32)
    for i, m in enumerate(leaves):
        out[i, :len(m)] = m
    return out


def partition(rng, n, longest, k, width=None):
    """one round: a random partition of all n points into leaves of mixed sizes, as an int32 (n_leaves, width) array."""
    sizes = _sizes(rng, n, longest, k)
    return _rows(np.split(rng.permutation(n).astype(np.int32), np.cumsum(sizes)[:-1]), longest if width is None else width)


def chain(n_leaves=30, m=40):
    """leaf i = m consecutive points, its last point the first of leaf i + 1: every leaf lands one round after its predecessor."""
    return _rows([np.arange(i * (m - 1), i * (m - 1) + m, dtype=np.int32) for i in range(n_leaves)], m)


def long_leaves(rng, n):
    """leaves of 257, 300, 512 and 513 points (disjoint) and the rest of the points in leaves of up to 200."""
    p = rng.permutation(n).astype(np.int32)
    cuts = np.cumsum([257, 300, 512, 513])
    leaves = np.split(p[:cuts[-1]], cuts[:-1])
    rest = p[cuts[-1]:]
    leaves += np.split(rest, np.cumsum(_sizes(rng, len(rest), 200, 15))[:-1])
    return _rows(leaves, 513)


def garbage(rng, n, longest, k):
    """a partition, wider than its longest leaf, with ids (valid ones, others' members, ids >= n) after the first -1 of many rows,
    all-empty rows and one-point leaves in between."""
    la = partition(rng, n, longest, k, width=longest + 7)
    for i in range(0, len(la), 3):
        m = int((la[i] >= 0).sum())
        if m + 1 < la.shape[1]:
            la[i, m + 1:] = rng.randint(0, 2 * n, la.shape[1] - m - 1)  # after the first -1: never read
    extra = np.full((12, la.shape[1]), -1, np.int32)
    extra[::2, 0] = rng.randint(0, n, 6)  # one-point leaves; the odd rows stay all empty
    extra[0, 2:5] = [5, 5, n + 3]         # ... and one with a repeated id and an id >= n behind its -1
    out = np.concatenate([la, extra])
    return out[rng.permutation(len(out))]


def leaf_array(case):
    """the case's leaf array (cached, read-only)."""
    if case.name not in _ARRAYS:
        rng = np.random.RandomState(case.seed + 7 * case.k + case.longest)
        if case.kind == "partition":
            la = np.concatenate([partition(rng, case.n, case.longest, case.k) for _ in range(case.rounds)])
        elif case.kind == "chain":
            la = np.concatenate([_rows(list(chain()), case.longest), partition(rng, case.n, case.longest, case.k)])
        elif case.kind == "cut":
            la = np.concatenate([long_leaves(rng, case.n), partition(rng, case.n, case.longest, case.k, width=513)])
        else:
            la = np.concatenate([garbage(rng, case.n, case.longest, case.k), garbage(rng, case.n, case.longest, case.k)])
        la.setflags(write=False)
        _ARRAYS[case.name] = la
    return _ARRAYS[case.name]


def partial_graph(case):
    """a graph for init_from_graph that leaves work for the seeding: per row up to k random ids (self and repeats taken out),
    a third of the rows half filled, every 11th row empty."""
    rng = np.random.RandomState(case.seed + 1000)
    g = rng.randint(0, case.n, (case.n, case.k)).astype(np.int32)
    g[g == np.arange(case.n)[:, None]] = -1
    g[::3, case.k // 2:] = -1
    g[::11] = -1
    return g
