"""The pruning pass's host model (tests/prune_reference.py) tested without a GPU: it reproduces the reference's own recorded runs
and the CPU oracle row for row, its vectorised walks equal their sequential statements, its lattice cases contain the exact ties
that pin the strict `<` and flag nothing, its float cases stay under the ambiguity cap, and its coins are the library's.  Without
these pins the comparison of tests/test_gpu_prune_exact.py could be vacuous."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import prune_cases as PC
from tests import prune_reference as PR
from tests.search_reference import hash3

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pynndescent_amd", "csrc")
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or shutil.which("/opt/rocm/bin/hipcc")

_Mode = PC.Case


def whole_model(prep, idx, dist, mode, n_neighbors):
    """forward model, then the glue on the model's own forward rows: (RowsResult, GraphResult, tainted rows, unclear entries).
    Tainted: flagged in either pass, or listed in a flagged row's input list."""
    fw = PR.diversify_rows(prep, idx, dist, **PC.forward_opts(mode, idx, n_neighbors))
    g = PR.search_graph_from_forward(prep, fw.ids, fw.dists, n_neighbors, prob=mode.prob, aware=mode.aware, aggressiveness=mode.aggr,
                                     seed=mode.seed)
    tainted = g.tainted | (fw.flags != 0)
    for t in np.nonzero(fw.flags)[0]:
        tainted[idx[t][idx[t] >= 0]] = True
    return fw, g, tainted, fw.n_unclear + g.n_unclear


def _mode(prob, aware, aggr, seed=0):
    return _Mode("", "", 0, 0, 0, "", "", prob, aware, aggr, False, seed, "")


def _compare(label, fw, g, tainted, unclear, ref_rows, ref_indptr, ref_indices, ref_rev, ref_union):
    n = len(tainted)
    clear = fw.flags == 0
    bad = np.nonzero(clear & (fw.ids != ref_rows).any(1))[0]
    assert not len(bad), "%s: %d unflagged forward rows differ, first %d: model %s reference %s" % (
        label, len(bad), bad[0], fw.ids[bad[0]].tolist(), ref_rows[bad[0]].tolist())
    same = PR.csr_rows_equal(g.indptr, g.indices, ref_indptr, ref_indices)
    bad = np.nonzero(~tainted & ~same)[0]
    assert not len(bad), "%s: %d untainted rows of the search graph differ, first %d" % (label, len(bad), bad[0])
    print("%s: %d of %d rows flagged forward, %d in the csr pass, %d tainted, %d entries not pinned; reverse / union nnz model %d / %d "
          "reference %d / %d" % (label, int((~clear).sum()), n, int((g.flags != 0).sum()), int(tainted.sum()), unclear,
                                 g.stats["reverse_nnz"], g.stats["union_nnz"], ref_rev, -1 if ref_union is None else ref_union))
    assert abs(g.stats["reverse_nnz"] - ref_rev) <= unclear
    assert ref_union is None or abs(g.stats["union_nnz"] - ref_union) <= unclear
    assert tainted.mean() <= PC.FLOAT_CAP


@pytest.mark.parametrize("tag", sorted(PC.FIXTURES))
def test_model_reproduces_the_references_recorded_run(tag):
    """tests/golden/search_graph*.npz hold pynndescent's own diversify / diversify_csr / degree_prune on a graph it built."""
    _, metric, prob, aware, aggr = PC.FIXTURES[tag]
    x, prep, idx, dist, g = PC.fixture(tag)
    fw, res, tainted, unclear = whole_model(prep, idx, dist, _mode(prob, aware, aggr), 15)
    _compare(tag, fw, res, tainted, unclear, g[tag + "_fwd_rows"], g[tag + "_indptr"], g[tag + "_indices"], int(g[tag + "_rev_nnz"]),
             int(g[tag + "_pre_prune_nnz"]))


ORACLE_CASES = ["euclidean_k15", "cosine_k15", "dot_k15", "inner_product_k15", "correlation_k15", "hellinger_k15", "euclidean_k100",
                "lat_k15", "lat_dups_k15", "lat_k16", "aware_a07_g20", "aware_k100_g20"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_model_against_the_oracle(name):
    """The strict build of the CPU oracle runs the reference's pass in the reference's arithmetic order."""
    c = PC.ALL[name]
    x, prep = PC.data(c), PC.prepared(c)
    idx, dist = PC.graph(c)
    fw, res, tainted, unclear = whole_model(prep, idx, dist, c, c.k)
    osg, st = O.search_graph(np.array(x), idx, dist, c.metric, c.k, lib=O.load("strict"), return_stages=True, diversify_prob=c.prob,
                             diversify_method="degree_aware" if c.aware else "standard", degree_prune_aggressiveness=c.aggr)
    if c.prob < 1.0:   # the csr pass flips coins there (the reference's from its Tausworthe stream): the forward pass, which has none
        assert c.aware
        bad = np.nonzero((fw.flags == 0) & (fw.ids != st["forward_rows"]).any(1))[0]
        assert not len(bad), (name, bad[:5])
        return
    # (the oracle counts its "union_nnz" after its degree prune: the rows of the final graph, compared one by one, say more)
    _compare(name, fw, res, tainted, unclear, st["forward_rows"], osg.indptr, osg.indices, st["reverse_nnz"], None)
    assert tainted.any() or res.stats["final_nnz"] == st["union_nnz"]
    if c.exact:
        assert not tainted.any() and unclear == 0


@pytest.mark.parametrize("name", sorted(PC.ALL))
def test_ambiguity_caps(name):
    c = PC.ALL[name]
    idx, dist = PC.graph(c)
    fw, res, tainted, unclear = whole_model(PC.prepared(c), idx, dist, c, c.k)
    flagged = (fw.flags != 0) | (res.flags != 0)
    print("%s (%s): %.2f %% of %d rows flagged, %.2f %% tainted, %d entries not pinned; kept %.1f %% forward; stage counts %s" % (
        name, c.doc, 100 * flagged.mean(), c.n, 100 * tainted.mean(), unclear, 100 * fw.kept[idx >= 0].mean(), res.stats))
    cap = PC.LATTICE_CAP if c.exact else PC.FLOAT_CAP
    assert flagged.mean() <= cap and tainted.mean() <= cap
    if c.exact:
        assert unclear == 0
    if name == "scan_rounds":   # both scans of the device pass must need a second round of k_sg_scan_single
        assert 2 * res.stats["reverse_nnz"] > PC.SCAN_WORDS and res.stats["union_nnz"] > PC.SCAN_WORDS
        assert res.stats["forward_nnz"] == c.n * c.k, "the constructed graph must lose nothing"
    else:
        assert 0.02 < fw.kept[idx >= 0].mean() < 1.0 or c.k <= 2, "the case prunes nothing or everything"


def test_lattice_cases_hold_exact_ties_and_stored_zeros():
    """the small coordinate range makes d(j, c) == d(i, j) frequent: a `<=` for the `<` shows in hundreds of rows."""
    c = PC.ALL["lat_k15"]
    prep = PC.prepared(c)
    idx, dist = PC.graph(c)
    fw = PR.diversify_rows(prep, idx, dist)
    ties = 0
    for j in range(1, c.k):
        mid, _ = PR.pair_dist(prep, idx[:, j], idx[:, :j])
        ties += int((fw.kept[:, :j] & (dist[:, :j] > PR.EPS32) & (mid == dist[:, j].astype(np.float64)[:, None])).sum())
    assert ties > c.n, ties
    # and the csr pass meets d == w_j: a model with <= prunes more
    g = PR.search_graph_from_forward(prep, fw.ids, fw.dists, c.k)
    assert (g.fp_data != 0).sum() == len(g.fp_data)  # (with `<` the second pass finds nothing on rows the first pass diversified)
    cd = PC.ALL["lat_dups_k15"]
    idx, dist = PC.graph(cd)
    assert ((dist == 0.0) & (idx != np.arange(cd.n)[:, None])).sum() > 100, "duplicate points must store distance 0"
    assert (idx[:, 0] != np.arange(cd.n)).any()


@pytest.mark.parametrize("name", ["lat_k15", "lat_k15_p50", "lat_k100_p50", "lat_k15_aware", "aware_cosine_a07_g10", "inner_product_k15",
                                  "lat_dups_k15", "lat_k16"])
def test_vectorised_walks_equal_their_sequential_statements(name):
    """diversify_rows / diversify_csr decide an entry by the OR of its tests; explain_row / explain_csr_row walk test by test and
    stop at the first hit, as the kernels do."""
    c = PC.ALL[name]
    prep = PC.prepared(c)
    idx, dist = PC.graph(c)
    opts = PC.forward_opts(c, idx, c.k)
    fw = PR.diversify_rows(prep, idx, dist, **opts)
    rows = np.r_[0:12, c.n - 3:c.n] if c.k > 64 else np.r_[0:60, c.n - 3:c.n]
    for i in rows:
        kept, trail = PR.explain_row(prep, idx[i], dist[i], int(i), **opts)
        assert kept == np.nonzero(fw.kept[i])[0].tolist(), (i, trail)
    g = PR.search_graph_from_forward(prep, fw.ids, fw.dists, c.k, prob=c.prob, aware=c.aware, aggressiveness=c.aggr, seed=c.seed)
    kw = dict(aware=True, degree=PR.compute_degrees_csr(g.f_indptr, g.f_indices), max_degree=c.k, aggressiveness=c.aggr) if c.aware else {}
    for i in rows:
        a, b = g.f_indptr[i], g.f_indptr[i + 1]
        ret, trail = PR.explain_csr_row(prep, g.f_indices[a:b], g.f_data[a:b], int(i), prob=c.prob, seed=c.seed, **kw)
        assert np.array_equal(ret, g.fp_data[a:b] != 0), (i, trail)


def test_k64_and_k65_decide_the_first_64_columns_alike():
    """the prefix property the lane and LDS forms share (prune.hip: "same decisions ... on rows that fit both")."""
    c65 = PC.ALL["lat_k65"]
    prep = PC.prepared(c65)
    idx, dist = PC.graph(c65)
    a = PR.diversify_rows(prep, idx, dist)
    b = PR.diversify_rows(prep, idx[:, :64], dist[:, :64])
    assert np.array_equal(a.kept[:, :64], b.kept)


def test_csr_and_degree_prune_models_against_the_oracle():
    """constructed rows: the csr walk (standard and degree aware, own vertices, weight-0 entries) without repeated weights -- the
    reference's argsort is not stable, so only the kernel's own tie-break is defined where weights repeat -- and degree_prune
    with repeats at the cut."""
    lib = O.load("strict")
    c = PC.ALL["lat_k64"]
    x, prep = np.array(PC.data(c)), PC.prepared(c)
    indptr, indices, data = PC.csr_alone(c.n, 64, seed=2, repeat=False)
    mine = PR.diversify_csr(prep, indptr, indices, data)
    ref = data.copy()
    lib.orc_diversify_csr(indptr, indices, ref, c.n, x, x.shape[1], O.METRICS[c.metric])
    assert np.array_equal(mine.data, ref) and 0.05 < (ref == 0).mean() < 0.95
    deg = PR.compute_degrees_csr(indptr, indices)
    mine = PR.diversify_csr(prep, indptr, indices, data, aware=True, degree=deg, max_degree=40, aggressiveness=2.0)
    ref = data.copy()
    lib.orc_diversify_csr_degree_aware(indptr, indices, ref, c.n, x, x.shape[1], O.METRICS[c.metric], np.array([1, 2, 3], np.int64), 40, 2.0, 1.0)
    clear = np.repeat(mine.flags == 0, np.diff(indptr))
    assert np.array_equal(mine.data[clear], ref[clear]) and (mine.flags != 0).mean() < 0.1
    for md in (1, 22, 23):
        ip, w = PC.degree_prune_alone(c.n, md, seed=4)
        ref = w.copy()
        lib.orc_degree_prune(ip, ref, c.n, md)
        got = PR.degree_prune(ip, w, md)
        assert np.array_equal(got, ref)
        ln = np.diff(ip)
        left = np.add.reduceat(np.r_[got != 0, False].astype(int), ip[:-1]) * (ln > 0)
        assert (left[ln > md] > md).all() and (left[ln > md] > md + 1).any(), "repeats at the cut must leave rows longer than max_degree + 1"
        assert np.array_equal(got[np.repeat(ln <= md, ln)], w[np.repeat(ln <= md, ln)])


def test_coin_is_exact_and_its_hash_input_injective():
    """(entry, compared entry) -> hash word must be one-to-one below NND_WIDE_K: a * 64 + b gave (a, b) and (a + 1, b - 64) one
    coin in rows of more than 64 entries."""
    a, b = np.meshgrid(np.arange(PR.WIDE_K), np.arange(PR.WIDE_K), indexing="ij")
    assert len(np.unique(PR.coin_word(a, b))) == PR.WIDE_K ** 2
    # the vectorised coin is the scalar formula
    for seed, row, aa, bb, p in ((77, 5, 14, 3, 0.5), (77 ^ PR.CSR_SEED, 1201, 255, 254, 0.7), (0xFFFFFFFF, 36001, 64, 0, 0.25)):
        want = float(np.float32(hash3(seed, row, aa * 256 + bb) >> 8) * np.float32(1.0 / 16777216.0)) < float(np.float32(p))
        assert bool(PR.coin(seed, np.uint64(row), aa, bb, p)) == want
    heads = PR.coin(9, np.arange(4000)[:, None], np.arange(1, 65)[None, :], 0, 0.5)
    assert abs(heads.mean() - 0.5) < 0.01
    assert PR.coin(9, np.arange(10), 1, 0, 1.0).all()


@pytest.mark.skipif(HIPCC is None, reason="no hipcc: csrc/common.h needs the HIP headers")
def test_coin_word_and_hash_are_the_librarys(tmp_path):
    """tests/prune_hash_cpu.cpp includes csrc/common.h and prints nnd_prune_coin_word / nnd_hash3 on the host, and the number of
    different words over all pairs below NND_WIDE_K."""
    exe = str(tmp_path / "prune_hash_cpu")
    r = subprocess.run([HIPCC, "--offload-host-only", "-O1", "-I", CSRC, os.path.join(HERE, "prune_hash_cpu.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == 46
    for f in lines[:-1]:
        assert f[0] == "coin"
        seed, row, a, b, word, h = (int(t) for t in f[1:])
        assert PR.coin_word(a, b) == word
        assert hash3(seed, row, word) == h
        assert int(PR.hash3v(seed, np.array([row]), word)[0]) == h
    assert lines[-1] == ["distinct", str(PR.WIDE_K ** 2), "of", str(PR.WIDE_K ** 2)]
