"""The nine boolean metrics (metric codes 8..16) on a real MI355X, through the C ABI and the class.  Truth is float64 numpy
(tests/boolean_util.py: the oracle does not know these codes) and the fixture the reference wrote (tests/golden/boolean_metrics.npz).

The counts of indicator rows are exact float32 integers in every summation order, so a distance is a function of four integers:
every kernel must give the same BITS for a pair, and for the eight rational formulas those of the float32 numpy expression.
jaccard's -log2 is the hardware's logarithm: the same bits in every kernel, and within 2^-20 + 4 ulp of numpy's."""
import importlib.util
import pickle

import numpy as np
import pytest

import pynndescent_amd
from pynndescent_amd import NNDescent, _capi
from tests import boolean_util as BU
from tests import descent_cases as DC
from tests import descent_reference as DR
from tests import leaf_cases as LC
from tests import leaf_reference as LR
from tests import prune_reference as PR

pytestmark = pytest.mark.gpu
K = BU.K


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pairwise(x, metric):
    """k_pairwise on every pair of x: the reference value of the bit comparisons, itself held to numpy below."""
    b = BU.make_builder(x, metric, k=8, n_trees=0)
    try:
        rows = np.arange(x.shape[0], dtype=np.int32)
        return b.pairwise_gram(rows, rows)
    finally:
        b.close()


def _stored_equal(label, pw, idx, dist):
    """every stored (row, id, distance) holds the bits of k_pairwise's value of the pair; the self pair holds 0"""
    ok = idx >= 0
    rows = np.broadcast_to(np.arange(idx.shape[0])[:, None], idx.shape)
    want = np.where(idx == rows, np.float32(0.0), pw[rows, np.maximum(idx, 0)])
    bad = ok & (_bits(dist) != _bits(want))
    assert ok.any() and not bad.any(), "%s: %d stored distances differ from k_pairwise, first (row, slot) %s: %r vs %r" % (
        label, int(bad.sum()), np.argwhere(bad)[0], dist[bad][0], want[bad][0])


# (k, longest run) -> the launches of the leaf table (csrc/leaf_plan.h; names as tests/leaf_cases.py writes them, without the
# family argument): all 15 forms, the smallest k and the upper edge of the size class of each
LEAF_FORMS = {
    (16, 64): (LC.QW4,), (16, 80): (LC.QW44, LC.QW5), (16, 96): (LC.QW6,), (16, 128): (LC.RB8,),
    (30, 160): (LC.SYM6, LC.SYM10), (32, 256): (LC.RB16,),
    (40, 64): (LC.P4,), (40, 80): (LC.P5,), (64, 96): (LC.P6,), (40, 160): (LC.RB10,),
    (100, 128): (LC.W8,), (100, 160): (LC.W10,), (100, 256): (LC.W16,),
}
assert {f for fs in LEAF_FORMS.values() for f in fs} == {LC.QW4, LC.QW44, LC.QW5, LC.QW6, LC.P4, LC.P5, LC.P6, LC.SYM6, LC.SYM10,
                                                        LC.RB8, LC.RB10, LC.RB16, LC.W8, LC.W10, LC.W16}


def _leaf_rows(n, longest):
    """disjoint leaves over n rows as an int32 leaf array, and their sizes: the longest run first, then sizes on both sides of
    the tile, size-class and row-block edges below it, until the rows run out"""
    perm = np.random.RandomState(longest).permutation(n).astype(np.int32)
    sizes, left = [], n
    for s in [longest] + [e for e in (97, 96, 65, 64, 33, 17, 2) if e < longest] * 4:
        s = min(s, left)
        if s < 2:
            break
        sizes.append(s)
        left -= s
    la = np.full((len(sizes), longest), -1, np.int32)
    for i, (a, s) in enumerate(zip(np.cumsum([0] + sizes[:-1]), sizes)):
        la[i, :s] = perm[a:a + s]
    return la, sizes


# ------------------------------------------------------------------------------------------------ 1. kernel agreement
@pytest.mark.parametrize("d", [20, 133])
@pytest.mark.parametrize("metric", BU.METRICS)
def test_kernels_agree_bit_for_bit(metric, d):
    """k_pairwise against float32 numpy; then the leaf kernels (the library's forest at k = 8 / 16 / 17 / 32 / 100, and every
    form of the leaf table on hand-built leaves: LEAF_FORMS), nnd_row_pair_dist (random init) and k_query's reported distances
    against k_pairwise, bit for bit, on 300 rows (dp != d, several K blocks)."""
    x = BU.random_rows(300, d, 100 + d)
    pw = _pairwise(x, metric)
    want = BU.dist(metric, x, x, f32=True).astype(np.float32)
    assert np.isfinite(pw).all() and (pw >= 0.0).all()
    if metric == "jaccard":
        far = want >= BU.FLT_MAX
        assert far.any() and np.array_equal(pw >= BU.FLT_MAX, far)
        err = np.abs(pw.astype(np.float64) - want)[~far]
        assert (err <= BU.LOG_TERM_ABS + 4.0 * BU._ulp32(want[~far])).all(), float(err.max())
        assert (pw[want == 0.0] == 0.0).all()
    else:
        assert np.array_equal(_bits(pw), _bits(want)), np.argwhere(_bits(pw) != _bits(want))[:3]
    assert np.array_equal(_bits(pw), _bits(pw.T)) and (np.diag(pw) == 0.0).all()
    for k in (8, 16, 17, 32, 100):
        b = BU.make_builder(x, metric, k=k, n_trees=2, leaf_size=max(60, 2 * k))
        try:
            b.make_forest()
            b.init_from_leaves()
            idx, dist, _ = b.graph()
            _stored_equal("leaf seeding k = %d" % k, pw, idx, dist)
            b.reset_graph()
            b.init_random()
            idx, dist, _ = b.graph()
            _stored_equal("random init k = %d" % k, pw, idx, dist)
        finally:
            b.close()
    # every form of the leaf table (csrc/leaf_plan.h) in the family's instance: a hand-built leaf array whose longest run sits in
    # the form's size class, at the form's k.  leaf_pairs / leaf_rows / leaf_mfma are the model's counts for the forms named: that
    # separates the row-block forms (whole blocks) from the others (upper triangle) and catches a leaf that no launch of the round
    # took (a wrong m_lo or size class), not two forms that count alike (QW4 / QW6, P4 / P6 on the same leaves); which form a
    # (k, longest run) pair launches is pinned on the CPU (tests/test_leaf_plan_cpu.py)
    for (k, longest), names in sorted(LEAF_FORMS.items()):
        la, sizes = _leaf_rows(x.shape[0], longest)
        pairs, rows, mfma, fs = LR.counters(sizes, k, d)
        assert tuple(f.name for f in fs) == names
        b = BU.make_builder(x, metric, k=k, n_trees=0)
        try:
            b.init_from_leaf_array(la)
            idx, dist, _ = b.graph()
            st = b.stats()
        finally:
            b.close()
        _stored_equal("leaf array k = %d, longest run %d (%s)" % (k, longest, ", ".join(names)), pw, idx, dist)
        assert (st["leaf_pairs"], st["leaf_rows"], st["leaf_mfma"]) == (pairs, rows, mfma), (k, longest, names)
    # k_query: both tiers and every KU (k <= 64, <= 128, <= 256) report the bits of the pair
    index = NNDescent(x, metric=metric, n_neighbors=10, random_state=2)
    index.prepare()
    inv = np.asarray(index._vertex_order)
    for tier, k in ((0, 10), (0, 100), (0, 200), (1, 10), (1, 100), (1, 200)):
        index._searcher.set_tier(tier)
        qi, qd = index._searcher.query(x[:40], k, 0.1)
        ok = qi >= 0
        wantq = pw[np.arange(40)[:, None], inv[np.maximum(qi, 0)]]
        # (the walk over a 10-neighbour graph need not fill 100 or 200 slots; whatever it reports must be the pair's bits)
        assert ok[:, :10].mean() > 0.9 and np.array_equal(_bits(qd)[ok], _bits(wantq)[ok]), (tier, k)


@pytest.mark.parametrize("mc,k,n", [(15, 15, DC.N16), (30, 30, DC.NW32), (60, 100, DC.NW64)])
@pytest.mark.parametrize("metric", BU.METRICS)
def test_join_iteration_stores_the_pair_bits(metric, mc, k, n):
    """One descent iteration at mc 15 / 30 / 60 (k_local_join16, k_local_join_w<32>, k_local_join_w<64>, the family's XM = 3
    instances, at the smallest n at which each join kernel reaches its steady state): every stored distance is the float32
    numpy value of its pair (jaccard: k_pairwise's bits)."""
    x = BU.fixture_data(n, 20, 0, seed=n)[0]
    b = BU.make_builder(x, metric, k=k, n_trees=2, mc=mc)
    try:
        b.make_forest()
        b.init_from_leaves()
        b.init_random()
        b.descent_iter()
        idx, dist, _ = b.graph()
        st = b.stats(raw=True)
        assert int(st.join_pairs[0]) > 0
        rows = np.arange(0, n, 7, dtype=np.int32)
        sub_i, sub_d = idx[rows], dist[rows]
        if metric == "jaccard":
            cols = np.unique(np.maximum(sub_i, 0)).astype(np.int32)
            pw = b.pairwise_gram(rows, cols)
            want = pw[np.arange(len(rows))[:, None], np.searchsorted(cols, np.maximum(sub_i, 0))]
        else:
            want = BU.dist_pairs(metric, x[rows][:, None, :], x[np.maximum(sub_i, 0)], f32=True).astype(np.float32)
    finally:
        b.close()
    ok = sub_i >= 0
    want = np.where(sub_i == rows[:, None], np.float32(0.0), want)
    assert ok.mean() > 0.99 and np.array_equal(_bits(sub_d)[ok], _bits(want)[ok]), np.argwhere(ok & (_bits(sub_d) != _bits(want)))[:3]
    assert (np.diff(np.where(ok, sub_d.astype(np.float64), np.inf), axis=1) >= 0).all()


# --------------------------------------------------------------------------------------------- 2. the step-exact models
class _Case:
    """What the checks of tests/test_gpu_leaf_exact.py and tests/test_gpu_descent_exact.py read off a case."""

    def __init__(self, metric, n, k):
        self.metric, self.n, self.k, self.exact, self.doc = metric, n, k, metric != "jaccard", "boolean family"


@pytest.mark.parametrize("k,mc", [(15, 15), (30, 30)])
@pytest.mark.parametrize("metric", ["jaccard", "dice", "kulsinski", "russellrao", "yule", "matching"])
def test_seeding_and_one_iteration_equal_the_model(metric, k, mc):
    """Leaf seeding (tests/leaf_reference.py) and one descent iteration, join + merge (tests/descent_reference.py), entry for
    entry, with the family's Prepared: radius 0 and no ambiguous row for the rational formulas, the log term's band for jaccard."""
    from tests.test_gpu_descent_exact import _check as check_iteration
    from tests.test_gpu_leaf_exact import _check as check_leaves

    n = 3001
    x = BU.fixture_data(n, 24, 0, seed=5)[0]
    prep = BU.make_prepared(x, metric)
    case = _Case(metric, n, k)
    b = BU.make_builder(x, metric, k=k, n_trees=2, mc=mc, seed=1)
    try:
        b.make_forest()
        la = b.leaf_array()
        b.init_from_leaves()
        got = b.graph()
        res = LR.reference_seed(prep, None, k, la)
        leaf_share = float((res.ambiguous != 0).mean())
        print("%s k = %d leaf seeding: %.2f %% of the rows flagged %s" % (metric, k, 100 * leaf_share, np.bincount(res.ambiguous, minlength=4).tolist()))
        check_leaves("%s leaf seeding" % metric, case, None, got, res)
        # the rows the model flags are flagged for EQUAL distances at the k-th place (R_TIE: which of the tied entries stay
        # depends on the order of batches and lanes, tests/leaf_reference.py), never for an inexact one
        if metric != "jaccard":
            assert not (res.ambiguous & LR.R_BOUNDARY).any() and not res.radius.any()
        b.init_random()
        s0 = b.graph()
        c = b.descent_iter()
        new, old = b.candidates()
        got = b.graph()
        st = b.stats(raw=True)
        rng_state = BU_rng_state(1)
        res = DR.reference_iter(prep, None, s0[0], s0[1], s0[2], new, old, k, rng_state, 0, 1)
        share = float((res.ambiguous != 0).mean())
        print("%s k = %d iteration 0: %.2f %% of the rows ambiguous, %d unclear; c / proposals / pairs gpu %s model %s" % (
            metric, k, 100 * share, res.n_unclear, (int(c), int(st.proposals[0]), int(st.join_pairs[0])), (res.c, res.proposals, res.join_pairs)))
        check_iteration("%s iteration 0" % metric, case, prep, s0, got, res)
        assert int(st.join_pairs[0]) == res.join_pairs
        if metric != "jaccard":  # nothing is decided inside a radius: the model's own count of unclear decisions is 0
            assert res.n_unclear == 0 and not res.radius[np.isfinite(res.dists)].any()
            assert (int(c), int(st.proposals[0])) == (res.c, res.proposals)
            assert share == 0.0, "%s iteration 0: %.2f %% of the rows ambiguous" % (metric, 100 * share)
    finally:
        b.close()


@pytest.mark.parametrize("metric", BU.RATIONAL)
def test_leaf_seeding_equals_the_model_with_no_flagged_row(metric):
    """Leaf seeding entry for entry with NO ambiguous row.  The one thing tests/leaf_reference.py cannot pin, for any metric, is
    which of several run-mates at EQUAL distance stay at the k-th place (it depends on the order of batches and lanes), and the
    clustered binary rows of the test above are full of such ties (the model flags 94 .. 98 % of their rows, for the tie alone, and
    they pass its weak checks).  Here the leaves are built so that no point has two run-mates at the same distance under any of
    the formulas (tests/boolean_util.py tie_free_leaves: 3600 x 770, leaves of 10 .. 14 points, k = 8, so every row drops 1 .. 5
    candidates): with radius 0 the model then flags nothing and every row of the kernel's output must be the model's, ids,
    flags and distance bits."""
    from tests.test_gpu_leaf_exact import _check as check_leaves

    k = 8
    x, la = BU.tie_free_leaves()
    prep = BU.make_prepared(x, metric)
    res = LR.reference_seed(prep, None, k, la)
    assert not res.ambiguous.any() and not res.radius.any(), np.bincount(res.ambiguous, minlength=4).tolist()
    assert (res.n_union > k).all()  # every row had to choose
    b = BU.make_builder(x, metric, k=k, n_trees=1)
    try:
        b.init_from_leaf_array(la)
        got = b.graph()
        st = b.stats()
    finally:
        b.close()
    check_leaves("%s tie-free leaves" % metric, _Case(metric, x.shape[0], k), None, got, res)
    np.testing.assert_array_equal(np.sort(got[0], axis=1), np.sort(res.ids, axis=1))
    assert (st["leaf_pairs"], st["leaf_rows"]) == (res.leaf_pairs, res.leaf_rows)


def BU_rng_state(seed):
    from oracle import oracle as O

    return O.draw_rng_states(seed, 2)[0]


@pytest.mark.parametrize("metric", ["jaccard", "dice", "yule"])
def test_pruning_pass_has_the_models_edges(metric):
    """The forward diversify pass at k = 30 (nnd_row_pair_dist on the family's distances) against tests/prune_reference.py."""
    x = BU.fixture_data(3000, 24, 0, seed=9)[0]
    k = 30
    index = NNDescent(x, metric=metric, n_neighbors=k, random_state=7)
    idx, dist = index._neighbor_graph
    prep = BU.make_prepared(x, metric)
    fw = PR.diversify_rows(prep, idx, dist)
    b = _capi.Builder(x.shape[0], x.shape[1], BU.CODES[metric], k, 0, 60, 200, min(60, k), 1, 0.001, [1, 2, 3], [4, 5, 6],
                      flags=_capi.NND_FLAG_NO_GRAPH)
    try:
        b.set_data_host(x)
        gi, gd = b.diversify(idx, dist)
    finally:
        b.close()
    clear = fw.flags == 0
    same = (gi == fw.ids).all(1) & (_bits(gd) == _bits(fw.dists)).all(1)
    print("%s: %d of %d rows flagged by the model, %.1f %% of the entries kept" % (
        metric, int((~clear).sum()), len(clear), 100.0 * (gi >= 0).sum() / (idx >= 0).sum()))
    assert (same | ~clear).all(), np.nonzero(clear & ~same)[0][:5]
    assert clear.all() if metric != "jaccard" else clear.mean() > 0.9
    assert (gi >= 0).sum() < (idx >= 0).sum()  # something was pruned


# ------------------------------------------------------------------------------------------------------- 3. finalize
@pytest.mark.parametrize("k", [10, 30, 100])
@pytest.mark.parametrize("metric", BU.METRICS)
def test_finalize_hands_out_the_float64_formula(metric, k):
    """k_finalize<code> (k <= 64) and k_finalize_wide<NND_CODES_BOOL>: within 1 ulp of the float64 formula rounded to float32; duplicates at
    0; an all-zero row against a non-zero row as the table says; rows by (distance, id)."""
    x = BU.fixture_data(1500, 48, 0)[0]
    x = x * np.float32(2.5)  # non-indicator values: the counts are taken on x != 0
    b = BU.make_builder(x, metric, k=k, n_trees=2, n_iters=2)
    try:
        b.make_forest()
        b.init_from_leaves()
        b.init_random()
        b.descent_iter()
        fi, fd = b.finalize()
    finally:
        b.close()
    ok = fi >= 0
    assert ok.mean() > 0.99
    want = BU.dist_pairs(metric, x[:, None, :], x[np.maximum(fi, 0)])
    w32 = np.minimum(want, BU.FLT_MAX).astype(np.float32)
    assert np.isfinite(fd[ok]).all() and (fd[ok] >= 0.0).all()
    assert (np.abs(fd.astype(np.float64) - w32.astype(np.float64))[ok] <= BU._ulp32(w32)[ok]).all()
    assert np.array_equal(fd[ok] == BU.FLT_MAX, want[ok] == BU.FLT_MAX)
    key = np.where(ok, fd.astype(np.float64), np.inf)
    tied = (np.diff(key, axis=1) == 0) & ok[:, 1:]
    assert (np.diff(key, axis=1) >= 0).all() and (np.diff(fi, axis=1)[tied] > 0).all(), "rows by (distance, id)"
    ind = x != 0
    dup = (ind[np.maximum(fi, 0)] == ind[:, None, :]).all(-1) & ok
    assert dup.any() and (fd[dup] == 0.0).all(), "equal indicator rows are at 0"
    zero_row = np.nonzero(~(x != 0).any(1))[0]
    assert len(zero_row) == 2
    for z in zero_row:  # every neighbour of an all-zero row: the table's value for a = 0, c = 0
        nb = fi[z][fi[z] >= 0]
        t = BU.dist_from_counts(metric, 0.0, 0.0, (x[nb] != 0).sum(1).astype(np.float64), float(x.shape[1]))
        assert np.array_equal(fd[z][fi[z] >= 0], np.minimum(t, BU.FLT_MAX).astype(np.float32)), (metric, z)


# -------------------------------------------------------------------------------------- 4. whole builds on the fixture
_G = {}


def _golden():
    if not _G:
        _G.update(BU.golden())
        _G["kth"] = {}
    return _G


def _recall(metric, x, idx, q=None):
    g = _golden()
    key = (metric, q is None)
    if key not in g["kth"]:
        g["kth"][key] = np.sort(BU.dist(metric, x if q is None else q, x), axis=1)[:, K - 1]
    return BU.distance_recall(metric, x, idx, q=q, kth=g["kth"][key])


@pytest.mark.parametrize("metric", BU.METRICS)
def test_builds_match_the_reference_fixture(metric):
    g = _golden()
    x, q = g["x"], g["queries"]
    ours, theirs = [], []
    for seed in BU.SEEDS:
        index = NNDescent(x, metric=metric, n_neighbors=K, random_state=int(seed))
        assert index._angular_trees == (metric in ("jaccard", "dice")) and index._raw_data is not None
        gi, gd = index.neighbor_graph
        ri, rc = g["%s_idx_%d" % (metric, seed)].astype(np.int64), g.get("%s_corrected_%d" % (metric, seed))
        rc = g["%s_dist_%d" % (metric, seed)].astype(np.float64) if rc is None else rc
        ours.append(_recall(metric, x, gi))
        theirs.append(float(g["%s_recall_%d" % (metric, seed)]))
        assert abs(_recall(metric, x, ri) - theirs[-1]) < 1e-12  # the fixture and this file agree on the truth
        # corrected distances of the (row, neighbour) pairs both graphs hold
        shared = (gi[:, :, None] == ri[:, None, :]) & (gi[:, :, None] >= 0)
        a, b_ = np.nonzero(shared.any(2)), shared.argmax(2)[shared.any(2)]
        mine, ref = gd[a].astype(np.float64), rc[a[0], b_]
        assert len(mine) > 0.5 * gi.size and np.allclose(mine, ref, rtol=1e-6, atol=0.0), metric
        if seed == BU.SEEDS[0]:
            index.prepare()
            qi, qd = index.query(q, k=K, epsilon=0.1)
            r_gpu, r_ref = _recall(metric, x, qi, q), float(g["%s_q_recall" % metric])
            assert abs(_recall(metric, x, g["%s_q_idx" % metric].astype(np.int64), q) - r_ref) < 1e-12
            print("%s query distance-recall@10: gpu %.4f reference %.4f" % (metric, r_gpu, r_ref))
            assert r_gpu >= r_ref - 0.02
            tq = BU.correct(metric, BU.dist_pairs(metric, q[:, None, :], x[np.maximum(qi, 0)]))
            assert np.allclose(np.asarray(qd, np.float64)[qi >= 0], tq[qi >= 0], rtol=1e-6, atol=0.0)
    print("%s graph distance-recall@10: gpu %s reference %s" % (metric, np.round(ours, 4).tolist(), np.round(theirs, 4).tolist()))
    assert np.mean(ours) >= np.mean(theirs) - 0.01


# ------------------------------------------------------------------------------------------------ 5. the other paths
def _same_graph(a, b, tol=0.0):
    ai, ad, bi, bd = (np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in (a[0], a[1], b[0], b[1]))
    np.testing.assert_array_equal(ai, bi)
    assert (np.abs(ad.astype(np.float64) - bd.astype(np.float64)) <= tol).all()


@pytest.mark.parametrize("metric", ["jaccard", "dice", "yule"])
def test_tensor_builds_equal_the_host_build(metric):
    torch = pytest.importorskip("torch")
    g = _golden()
    x, q = g["x"], g["queries"]
    host = NNDescent(x, metric=metric, n_neighbors=K, random_state=3)
    want_q = host.query(q, k=K)
    tol = 2.0 ** -52 if metric == "jaccard" else 0.0
    for dtype in (torch.float32, torch.float16):
        dev = NNDescent(torch.from_numpy(x).cuda().to(dtype), metric=metric, n_neighbors=K, random_state=3)
        _same_graph(dev._neighbor_graph, host._neighbor_graph)  # ids and kernel distances, bit for bit
        # (handed out: jaccard's 1 - 2^-v is float64 on both sides, the device's pow and numpy's may differ in the last bit)
        _same_graph(dev.neighbor_graph, host.neighbor_graph, tol)
        _same_graph(dev.query(torch.from_numpy(q).cuda().to(dtype), k=K), want_q, tol)
    np.testing.assert_array_equal(host._raw_data[np.argsort(host._vertex_order)], x)  # the caller's rows, not the indicators


@pytest.mark.parametrize("metric", ["jaccard", "rogerstanimoto"])
def test_update_pickle_and_from_graph(metric):
    g = _golden()
    x, q = g["x"], g["queries"]
    index = NNDescent(x[:1800], metric=metric, n_neighbors=K, random_state=5)
    index.update(xs_fresh=x[1800:])
    gi, gd = index.neighbor_graph
    assert gi.shape == (2000, K) and _recall(metric, x, gi) >= float(np.mean([g["%s_recall_%d" % (metric, s)] for s in BU.SEEDS])) - 0.02
    want = index.query(q, k=K)
    clone = pickle.loads(pickle.dumps(index))
    _same_graph(clone.query(q, k=K), want)
    _same_graph(clone.neighbor_graph, index.neighbor_graph)
    again = NNDescent.from_graph(x, index._neighbor_graph[0], index._neighbor_graph[1], metric=metric, random_state=5)
    _same_graph(again.neighbor_graph, index.neighbor_graph)
    assert _recall(metric, x, again.query(q, k=K)[0], q) > 0.5
    if importlib.util.find_spec("pynndescent") is not None:
        ref = index.to_reference()
        assert ref.metric == metric and ref._angular_trees == (metric == "jaccard")


@pytest.mark.parametrize("metric", BU.METRICS)
def test_exact_knn_and_recall(metric):
    """exact_knn against float64 brute force under the (distance, id) order -- ids equal, position by position -- and recall()."""
    torch = pytest.importorskip("torch")
    g = _golden()
    x, q = g["x"], g["queries"]
    ti, td = BU.brute(metric, x)
    for data in (x, torch.from_numpy(x).cuda()):
        gi, gd = pynndescent_amd.exact_knn(data, k=K, metric=metric)
        gi, gd = (np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in (gi, gd))
        np.testing.assert_array_equal(gi, ti)
        assert np.allclose(gd.astype(np.float64), BU.correct(metric, td), rtol=1e-6, atol=0.0)
    qi, qd = pynndescent_amd.exact_knn(x, queries=q, k=K, metric=metric)
    np.testing.assert_array_equal(qi, BU.brute(metric, x, q)[0])
    index = NNDescent(x, metric=metric, n_neighbors=K, n_iters=1, n_trees=1, random_state=1)
    sample = NNDescent._recall_rows(x.shape[0], 300, 7)
    hits = sum(int(np.isin(a, b).sum()) for a, b in zip(ti[sample], index._neighbor_graph[0][sample]))
    assert index.recall(k=K, n_rows=300, random_state=7) == hits / float(300 * K)


def test_nn_descent_takes_the_names():
    g = _golden()
    x = g["x"]
    index = NNDescent(x, metric="jaccard", n_neighbors=K, random_state=3, n_trees=2)
    from pynndescent_amd import nn_descent

    b = BU.make_builder(x, "jaccard", k=K, n_trees=2)
    try:
        b.make_forest()
        la = b.leaf_array()
    finally:
        b.close()
    for name in ("jaccard", "alternative_jaccard", "dice"):
        idx, dst = nn_descent(x, K, np.array([1, 2, 3], np.int64), max_candidates=K, dist=name, leaf_array=la)
        m = "dice" if name == "dice" else "jaccard"
        assert _recall(m, x, idx) > 0.9
        t = BU.dist_pairs(m, x[:, None, :], x[idx])
        t = BU.correct(m, t) if name == "jaccard" else np.minimum(t, BU.FLT_MAX)
        assert np.allclose(dst.astype(np.float64), t, rtol=1e-6, atol=0.0)
    assert index._distance_correction is not None


# ----------------------------------------------------------------------------------------------- 6. non-indicator input
@pytest.mark.parametrize("metric", ["jaccard", "kulsinski", "yule"])
def test_scaled_rows_build_the_identical_graph(metric):
    g = _golden()
    x = g["x"]
    w = np.random.RandomState(4).uniform(0.1, 9.0, x.shape).astype(np.float32) * np.where(np.random.RandomState(5).rand(*x.shape) < 0.5, -1, 1)
    a = NNDescent(x, metric=metric, n_neighbors=K, random_state=11)._neighbor_graph
    b = NNDescent(np.ascontiguousarray(x * w.astype(np.float32)), metric=metric, n_neighbors=K, random_state=11)._neighbor_graph
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]))
