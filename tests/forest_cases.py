"""The shapes at which the forest is compared with tests/forest_reference.py: the smallest at which each path of
csrc/rpforest.hip can go wrong.  Shared by tests/test_forest_reference_cpu.py (dry-run) and tests/test_gpu_forest_exact.py.

Behind every case: the model's own dry-run count "unclear / decisions" (float64 signs at unclear decisions), to be compared
with the cap of 1 unclear decision in 1000 that the GPU test asserts.
"""
from collections import namedtuple

import numpy as np

from oracle import oracle as O
from tests.forest_reference import ForestModel
from tests.util_data import clustered, nn_data_like

UNCLEAR_CAP = 1e-3   # at most 1 in 1000 (member, node) decisions of a case may be unclear: a condition on the case, not a tolerance
K = 10               # the builders' n_neighbors (the forest does not read it)

Case = namedtuple("Case", "name data n d metric T leaf_size max_depth exact seed")


def _case(name, data, n, d, metric, T, leaf_size=60, max_depth=200, exact=False, seed=1):
    return Case(name, data, n, d, metric, T, leaf_size, max_depth, exact, seed)


def lattice(n, d, seed, symmetric=False, groups=False):
    """integer rows in {-2..2}^d; ``symmetric``: closed under negation (column mean exactly 0); ``groups``: blocks of 3 to 6
    identical rows (zero hyperplanes, all-coin nodes, both stages of the finisher's one-sided rule at leaf_size 2)."""
    rs = np.random.RandomState(seed)
    m = n // 2 if symmetric else n
    if groups:
        rows, left = [], m
        while left > 0:
            g = min(int(rs.randint(3, 7)), left)
            rows.append(np.repeat(rs.randint(-2, 3, (1, d)), g, 0))
            left -= g
        x = np.concatenate(rows)[rs.permutation(m)]
    else:
        x = rs.randint(-2, 3, (m, d))
    if symmetric:
        x = np.concatenate([x, -x])[rs.permutation(2 * m)]
    return np.ascontiguousarray(x, np.float32)


def float_groups(n, d, seed):
    """clustered float rows in blocks of 3 to 6 identical rows: under cosine the pivots of a block's node give |h| = 0 < 1e-8."""
    rs = np.random.RandomState(seed)
    base = clustered(n, d, 4, 12, seed)
    reps = rs.randint(3, 7, n)
    x = np.repeat(base, reps, 0)[:n]
    return np.ascontiguousarray(x[rs.permutation(n)])


def grid(n, d, seed):
    """clustered rows on the integer grid [-63, 63]^d (1/8 steps of the clustered set): every product and partial sum of d <= 256 such
    terms is an exact float32, so a set with the structure of the float cases qualifies as exact=True."""
    return np.ascontiguousarray(np.clip(np.rint(clustered(n, d, 6, 30, seed) * 8.0), -63, 63), np.float32)


def case_data(c):
    if c.data == "grid":
        return grid(c.n, c.d, c.n + c.d)
    if c.data == "nn":
        return nn_data_like()
    if c.data == "clustered":
        return clustered(c.n, c.d, 6, 30, seed=c.n + c.d, nonneg=c.metric == "hellinger")
    if c.data == "lattice":
        return lattice(c.n, c.d, 5)
    if c.data == "lattice_sym":
        return lattice(c.n, c.d, 6, symmetric=True)
    if c.data == "lattice_groups":
        return lattice(c.n, c.d, 7, groups=True)
    if c.data == "lattice_sym_groups":
        return lattice(c.n, c.d, 8, symmetric=True, groups=True)
    if c.data == "float_groups":
        return float_groups(c.n, c.d, 9)
    raise ValueError(c.data)


def case_model(c, x=None, **hooks):
    x = case_data(c) if x is None else x
    _, _, ts = O.draw_rng_states(c.seed, max(c.T, 1))  # tests/gpu_util.py make_builder: the forest's seed is the first tree's state
    return ForestModel(x, c.metric, c.T, c.leaf_size, ts[0], max_depth=c.max_depth, exact=c.exact, **hooks)


def recording_clear_seed(c, x=None, seeds=range(1, 41)):
    """The search behind the seed of a clustered routing case: the smallest seed whose sample forest (dry-run) has no unclear
    decision in any tree.  The sample forest cannot be observed through the leaf array, so only such a seed pins it."""
    x = case_data(c) if x is None else x
    for s in seeds:
        m = case_model(c._replace(seed=s), x)
        m.record_tops()
        if not any(m.recording_unclear):
            return s
    return None


WHOLE = [
    # finisher from the root (n <= 2048)
    _case("nn-euclidean", "nn", 1002, 5, "euclidean", 3),
    _case("nn-cosine", "nn", 1002, 5, "cosine", 3),                      # two zero rows
    _case("one-leaf", "clustered", 60, 8, "euclidean", 2),               # n = leaf_size: not splittable
    _case("leaf+1", "clustered", 61, 8, "euclidean", 2),
    _case("n2048", "clustered", 2048, 16, "euclidean", 2),
    # level passes, then the LDS finisher
    _case("n2049-d33-T1", "clustered", 2049, 33, "euclidean", 1),        # dp = 64
    _case("n6000-d100-T3", "clustered", 6000, 100, "cosine", 3),
    _case("n6000-d130-T5", "clustered", 6000, 130, "euclidean", 5),      # dp = 160, nch = 20: the second 16-chunk step is partial; two tree batches
    _case("n6000-d256-T1", "clustered", 6000, 256, "euclidean", 1),      # dp = 256: the widest rows the routing mode takes
    _case("n6000-ip", "clustered", 6000, 24, "inner_product", 3),        # rows as given, euclidean-style planes
    _case("n6000-hellinger", "clustered", 6000, 24, "hellinger", 3),     # transformed unit rows
    # the global-memory tail: level passes, BIG finisher, hand-over to the LDS finisher
    _case("n20000-T2", "clustered", 20000, 40, "euclidean", 2),
    _case("n40000-T2", "clustered", 40000, 24, "cosine", 2),
    # max_depth: reached inside the level passes / inside a finisher; leaves longer than leaf_size
    _case("depth3", "clustered", 20000, 40, "euclidean", 2, max_depth=3),
    _case("depth9", "clustered", 6000, 24, "euclidean", 2, max_depth=9),
    # the exact lattice: many points exactly on the bisecting planes, every coin pinned
    _case("lattice-ip", "lattice", 6000, 8, "inner_product", 2, exact=True),
    _case("lattice-euclidean", "lattice_sym", 6000, 8, "euclidean", 2, exact=True),
    _case("groups-ip", "lattice_groups", 6000, 8, "inner_product", 2, leaf_size=2, exact=True),
    _case("groups-euclidean", "lattice_sym_groups", 6000, 8, "euclidean", 2, leaf_size=2, exact=True),
    _case("groups-small-euclidean", "lattice_sym_groups", 1500, 8, "euclidean", 3, leaf_size=2, exact=True),   # finisher from the root
    _case("groups-cosine", "float_groups", 3000, 12, "cosine", 2, leaf_size=2),                                # the |h| < 1e-8 branch
]

# The seeds of the clustered cases are recording_clear_seed(case): the smallest seed in 1..40 whose dry-run has
# recording_unclear == 0 in every tree (tests/test_forest_reference_cpu.py re-runs the search for the first of them).
ROUTING = [
    _case("route-131072-d32-T2", "clustered", 131072, 32, "euclidean", 2, seed=1),
    _case("route-140000-d32-T2", "clustered", 140000, 32, "euclidean", 2, seed=15),
    _case("route-131072-d20-T3", "clustered", 131072, 20, "cosine", 3, seed=19),
    _case("route-140000-d20-T3", "clustered", 140000, 20, "cosine", 3, seed=39),
    _case("route-lattice-ip", "lattice", 131072, 8, "inner_product", 2, exact=True),
    # d = 256 (8 chunks per lane): on float rows the a-priori radius of a 256-term sum leaves about 5 unclear recording decisions
    # per tree and no seed in 1..40 is clear, so the widest rows run on the integer grid, where nothing is unclear (the float rows
    # of that width are the whole-set case n6000-d256-T1)
    _case("route-131072-d256-T1", "grid", 131072, 256, "inner_product", 1, exact=True),
]

# The model's dry-run counts, unclear / decisions (the largest share, n6000-hellinger, is 5.0e-4: shifted-to-positive rows are nearly
# parallel after the square root, so the pivots are close and their normalisation errors weigh most).  Both stages of the finisher's
# one-sided rule are reached by the four "groups" cases (140 to 408 re-drawn nodes each, 70 to 183 of them down to "the first pivot
# goes left alone"); no case reaches the level passes' even/odd rule.
#   nn-euclidean                 0 / 15329
#   nn-cosine                    1 / 16494
#   one-leaf                     0 / 0
#   leaf+1                       0 / 122
#   n2048                        0 / 28147
#   n2049-d33-T1                 0 / 14099
#   n6000-d100-T3                3 / 147029
#   n6000-d130-T5               10 / 258822
#   n6000-d256-T1                1 / 51853
#   n6000-ip                     0 / 158337
#   n6000-hellinger             79 / 158283
#   n20000-T2                    8 / 446439
#   n40000-T2                   15 / 926329
#   depth3                       1 / 120000
#   depth9                       0 / 95930
#   lattice-ip                   0 / 96225
#   lattice-euclidean            0 / 98561
#   groups-ip                    0 / 157812
#   groups-euclidean             0 / 157291
#   groups-small-euclidean       0 / 49696
#   groups-cosine                6 / 74178
#   route-131072-d32-T2         32 / 3703343
#   route-140000-d32-T2         44 / 4118053
#   route-131072-d20-T3        144 / 5433981
#   route-140000-d20-T3        140 / 5771171
#   route-lattice-ip             0 / 3446852
#   route-131072-d256-T1         0 / 1801297

CASES = {c.name: c for c in WHOLE + ROUTING}
