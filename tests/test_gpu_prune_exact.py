"""The search-graph pruning pass (csrc/prune.hip: k_diversify_rows, k_diversify_csr, their _wide forms, k_degree_prune; the device
glue of csrc/searchgraph.hip) against the step-exact host model (tests/prune_reference.py), row by row.  Every stage runs through
its granular entry point and is compared with the model applied to the GPU's OWN previous stage, so one deviation does not
compound.  Rows the model does not flag must be the model's: ids, distance bits, packing, tail; zero pattern; final columns.
Flagged rows keep the weak checks.  Stage counts must be the model's: exactly on the lattice, within the number of entries the
model could not pin on float data.

The cases, which kernel form each reaches and the ambiguity caps are in tests/prune_cases.py; the model and the caps are pinned
without a GPU in tests/test_prune_reference_cpu.py."""
import numpy as np
import pytest

from pynndescent_amd import _capi
from tests import prune_cases as PC
from tests import prune_reference as PR

pytestmark = pytest.mark.gpu


def _builder(x, metric, k):
    """a handle that holds the point set only, as pynndescent_amd/search_graph.py makes it for the pass"""
    x = np.ascontiguousarray(x, np.float32)
    b = _capi.Builder(x.shape[0], x.shape[1], _capi.METRIC_CODES[metric], k, 0, 60, 200, min(60, k), 1, 0.001, [1, 2, 3], [4, 5, 6],
                      flags=_capi.NND_FLAG_NO_GRAPH)
    b.set_data_host(x)
    return b


# ------------------------------------------------------------------------------------------------ the comparisons
def _check_forward(label, case, prep, idx, dist, opts, fw, gi, gd, zero=np.float32(0.0)):
    """unflagged rows: ids, distance bits, packing and tail are the model's.  Flagged rows: the kept ids are a subsequence of
    the input row, position 0 is kept, stored distances unchanged (``zero``: what a stored 0 comes back as), packed, tail
    (-1, +inf)."""
    n, k = idx.shape
    bad = {}
    clear = fw.flags == 0
    same = (gi == fw.ids).all(1) & (gd.view(np.uint32) == fw.dists.view(np.uint32)).all(1)
    for t in np.nonzero(clear & ~same)[0][:4]:
        bad[int(t)] = "differs from the model"
    for t in np.nonzero(~clear)[0]:
        got = gi[t][gi[t] >= 0]
        m = len(got)
        pos, p = [], 0
        for v in got.tolist():   # the kept ids in input order: each found behind the one before
            while p < k and idx[t, p] != v:
                p += 1
            pos.append(p)
            p += 1
        if (pos and pos[-1] >= k) or (gi[t, m:] >= 0).any() or not np.all(np.isinf(gd[t, m:])) or (idx[t, 0] >= 0 and (m == 0 or pos[0] != 0)):
            bad[int(t)] = "flagged row: not a packed subsequence of its input that keeps position 0"
        elif not np.array_equal(gd[t, :m].view(np.uint32), np.where(dist[t, pos] == 0.0, zero, dist[t, pos]).view(np.uint32)):
            bad[int(t)] = "flagged row: a stored distance changed"
    assert not bad, "%s: forward rows, first %d:\n%s" % (label, len(bad), "\n".join(
        "%s: row %d (%s)\n    input    %s\n             %s\n    walk\n%s\n    expected %s\n    got      %s\n             %s" % (
            why, t, PR.reason_text(int(fw.flags[t])), idx[t].tolist(), dist[t].tolist(), PR.explain_row(prep, idx[t], dist[t], t, **opts)[1],
            fw.ids[t].tolist(), gi[t].tolist(), gd[t].tolist()) for t, why in list(bad.items())[:4]))


def _check_csr(label, prep, indptr, indices, data, kw, res, got):
    """unflagged rows: the zero pattern is the model's; everywhere nothing but zeroing happened to the weights."""
    assert np.array_equal(got[got != 0], data[got != 0]) and got.shape == data.shape, label + ": a weight changed other than to 0"
    diff = np.add.reduceat(np.r_[(got != 0) != (res.data != 0), False].astype(np.int64), indptr[:-1]) * (np.diff(indptr) > 0)
    bad = np.nonzero((res.flags == 0) & (diff > 0))[0]
    assert not len(bad), "%s: %d unflagged csr rows differ from the model, first:\n%s" % (label, len(bad), "\n".join(
        "row %d\n    columns  %s\n    weights  %s\n    walk\n%s\n    expected %s\n    got      %s" % (
            t, indices[indptr[t]:indptr[t + 1]].tolist(), data[indptr[t]:indptr[t + 1]].tolist(),
            PR.explain_csr_row(prep, indices[indptr[t]:indptr[t + 1]], data[indptr[t]:indptr[t + 1]], int(t), **kw)[1],
            res.data[indptr[t]:indptr[t + 1]].tolist(), got[indptr[t]:indptr[t + 1]].tolist()) for t in bad[:4]))


def _csr_kw(case, f_indptr, f_indices, n_neighbors):
    """the csr pass's options as nnd_search_graph_impl derives them (searchgraph.hip :283-291), for the model and the Builder"""
    if case.aware:
        deg = PR.compute_degrees_csr(f_indptr, f_indices)
        return (dict(aware=True, degree=deg, max_degree=n_neighbors, aggressiveness=case.aggr, prob=case.prob, seed=case.seed),
                dict(degree=deg, degree_aware=True, max_degree=n_neighbors, aggressiveness=case.aggr, prune_probability=case.prob, seed=case.seed))
    return dict(prob=case.prob, seed=case.seed), dict(prune_probability=case.prob, seed=case.seed)


def _row_text(indptr, indices, t):
    return indices[indptr[t]:indptr[t + 1]].tolist()


@pytest.mark.parametrize("name", sorted(PC.ALL))
def test_pruning_pass_equals_the_model(name):
    """forward pass, csr pass, degree_prune (the three kernels, through Builder.diversify / diversify_csr / degree_prune with the
    host-side glue between them) and the whole device pass (Builder.search_graph), each against the model of the stage before."""
    c = PC.ALL[name]
    prep = PC.prepared(c)
    idx, dist = (np.array(a) for a in PC.graph(c))
    n, k = idx.shape
    b = _builder(PC.data(c), c.metric, k)
    try:
        # ---- forward pass
        opts = PC.forward_opts(c, idx, k)
        fw = PR.diversify_rows(prep, idx, dist, **opts)
        gi, gd = b.diversify(idx, dist, **PC.builder_forward_opts(c, idx, k))
        print("%s (%s): forward pass: %d of %d rows flagged, %d entries not pinned, %.1f %% of the entries kept" % (
            name, c.doc, int((fw.flags != 0).sum()), n, fw.n_unclear, 100.0 * (gi >= 0).sum() / max(1, (idx >= 0).sum())))
        _check_forward(name + " forward", c, prep, idx, dist, opts, fw, gi, gd)
        # ---- csr pass on the GPU's own forward rows
        g = PR.search_graph_from_forward(prep, gi, gd, k, prob=c.prob, aware=c.aware, aggressiveness=c.aggr, seed=c.seed)
        m_kw, b_kw = _csr_kw(c, g.f_indptr, g.f_indices, k)
        rdata = b.diversify_csr(g.f_indptr, g.f_indices, g.f_data, **b_kw)
        res = PR.CsrResult(g.fp_data, g.flags, g.n_unclear)
        _check_csr(name + " csr", prep, g.f_indptr, g.f_indices, g.f_data, m_kw, res, rdata)
        # ---- degree_prune on the union of the GPU's own F'
        u_indptr, u_indices, u_data, rev_nnz = PR.union_max(g.f_indptr, g.f_indices, rdata)
        md = PR.final_max_degree(1.5, k)
        if len(u_data):
            pdata = b.degree_prune(u_indptr, u_data, md)
            want = PR.degree_prune(u_indptr, u_data, md)
            bad = np.nonzero(np.add.reduceat(np.r_[pdata.view(np.uint32) != want.view(np.uint32), False].astype(np.int64), u_indptr[:-1]) *
                             (np.diff(u_indptr) > 0))[0]
            assert not len(bad), "%s degree_prune (max_degree %d): %d rows differ, first %d: weights %s expected %s got %s" % (
                name, md, len(bad), bad[0], _row_text(u_indptr, u_data, bad[0]), _row_text(u_indptr, want, bad[0]), _row_text(u_indptr, pdata, bad[0]))
        else:
            pdata = u_data
        h_indptr, h_indices = PR.final_graph(u_indptr, u_indices, pdata)   # the host-glued form's search graph
        # ---- the whole pass on the device
        indptr, indices, st, fr, fd = b.search_graph(idx, dist, k, 1.5, c.prob, c.aware, c.aggr, c.seed, want_forward=True)
    finally:
        b.close()
    fw_eps = fw._replace(dists=np.where(fw.dists == 0.0, np.float32(PR.EPS32), fw.dists))   # k_sg_compact: 0 -> FLOAT32_EPS
    _check_forward(name + " device pass, forward", c, prep, idx, dist, opts, fw_eps, fr, fd, zero=np.float32(PR.EPS32))
    assert np.array_equal(fr, gi), name + ": the device pass and Builder.diversify run one kernel on one input"
    live = fd[fr >= 0]
    assert np.float32(st["min_distance"]).view(np.uint32) == (live.min() if len(live) else np.float32(0.0)).view(np.uint32), (name, st["min_distance"])
    # the two forms share their kernels and differ in their glue: the same graph, edge for edge
    same = PR.csr_rows_equal(indptr, indices, h_indptr, h_indices)
    assert same.all() and len(indices) == len(h_indices), "%s: the device pass and the host-glued stages differ in %d rows, first %d: %s / %s" % (
        name, int((~same).sum()), np.nonzero(~same)[0][0], _row_text(indptr, indices, np.nonzero(~same)[0][0]),
        _row_text(h_indptr, h_indices, np.nonzero(~same)[0][0]))
    # the final CSR against the model applied to the GPU's own forward output
    assert indptr[0] == 0 and indptr[-1] == len(indices) == st["final_nnz"]
    rows = np.repeat(np.arange(n), np.diff(indptr))
    assert not (indices == rows).any(), name + ": a diagonal entry"
    assert (np.diff(indices.astype(np.int64) + rows * np.int64(n)) > 0).all(), name + ": columns not ascending within the rows"
    same = PR.csr_rows_equal(indptr, indices, g.indptr, g.indices)
    bad = np.nonzero(~g.tainted & ~same)[0]
    assert not len(bad), "%s: %d untainted rows of the search graph differ from the model, first:\n%s" % (name, len(bad), "\n".join(
        "row %d: forward %s\n    union    %s\n             %s\n    expected %s\n    got      %s" % (
            t, fr[t].tolist(), _row_text(g.u_indptr, g.u_indices, t), _row_text(g.u_indptr, g.u_data, t), _row_text(g.indptr, g.indices, t),
            _row_text(indptr, indices, t)) for t in bad[:4]))
    slack = 0 if c.exact else g.n_unclear
    print("%s: device pass: %d rows flagged in the csr pass, %d tainted, %d entries not pinned; stage counts gpu %s model %s" % (
        name, int((g.flags != 0).sum()), int(g.tainted.sum()), g.n_unclear, {s: st[s] for s in ("forward_nnz", "reverse_nnz", "union_nnz", "final_nnz")}, g.stats))
    assert st["forward_nnz"] == g.stats["forward_nnz"] == int((fr >= 0).sum())
    for key in ("reverse_nnz", "union_nnz", "final_nnz"):
        assert abs(st[key] - g.stats[key]) <= slack, (name, key, st[key], g.stats[key], slack)
    cap = PC.LATTICE_CAP if c.exact else PC.FLOAT_CAP
    assert (fw.flags != 0).mean() <= cap and g.tainted.mean() <= cap, name + ": more rows are ambiguous than the cap allows"
    if name == "scan_rounds":
        assert 2 * st["reverse_nnz"] > PC.SCAN_WORDS and st["union_nnz"] > PC.SCAN_WORDS, "the case no longer reaches a second scan round"


def test_k64_and_k65_decide_the_first_64_columns_alike():
    """the lane form on a graph cut to 64 columns and the LDS form on all 65: the same decisions for the 64 (prune.hip: "same
    decisions ... on rows that fit both")."""
    c = PC.ALL["lat_k65"]
    idx, dist = (np.array(a) for a in PC.graph(c))
    out = {}
    for k in (65, 64):
        b = _builder(PC.data(c), c.metric, k)
        try:
            out[k] = b.diversify(idx[:, :k], dist[:, :k])[0]
        finally:
            b.close()
    kept65 = (out[65][:, :, None] == idx[:, None, :64]).any(1)   # input positions < 64 that the LDS form kept (ids are unique in a row)
    kept64 = (out[64][:, :, None] == idx[:, None, :64]).any(1)
    bad = np.nonzero((kept65 != kept64).any(1))[0]
    assert not len(bad), "%d rows differ, first %d: input %s\n k = 64: %s\n k = 65: %s" % (
        len(bad), bad[0], idx[bad[0]].tolist(), out[64][bad[0]].tolist(), out[65][bad[0]].tolist())
    model = PR.diversify_rows(PC.prepared(c), idx[:, :64], dist[:, :64])
    assert np.array_equal(kept64, model.kept)


@pytest.mark.parametrize("length,aware,prob", [(64, False, 1.0), (64, True, 1.0), (64, False, 0.5), (256, False, 1.0), (256, True, 1.0),
                                               (256, False, 0.5)])
def test_csr_kernel_alone_on_constructed_rows(length, aware, prob):
    """rows of exactly 64 entries under a k <= 64 handle (every lane an entry, len == 64 ? ~0ull) and of 256 under a k > 64 handle
    (every LDS slot); repeated weights (the rank's tie-break by position, and with it the standard variant's "point from storage
    position kk, weight from order[kk]"), weight-0 entries, rows that hold their own vertex, rows of 0, 1 and 2 entries."""
    c = PC.ALL["lat_k64" if length == 64 else "lat_k256"]
    prep = PC.prepared(c)
    indptr, indices, data = PC.csr_alone(c.n, length, seed=length + aware)
    assert (np.diff(indptr) == length).sum() >= c.n // 4 and np.diff(indptr).max() == length
    deg = PR.compute_degrees_csr(indptr, indices)
    m_kw = dict(prob=prob, seed=9)
    b_kw = dict(prune_probability=prob, seed=9)
    if aware:
        m_kw.update(aware=True, degree=deg, max_degree=12, aggressiveness=2.0)
        b_kw.update(degree=deg, degree_aware=True, max_degree=12, aggressiveness=2.0)
    res = PR.diversify_csr(prep, indptr, indices, data, **m_kw)
    b = _builder(PC.data(c), c.metric, c.k)
    try:
        got = b.diversify_csr(indptr, indices, data, **b_kw)
    finally:
        b.close()
    print("csr alone, rows of %d, aware %s, prob %.1f: %.1f %% pruned, %d rows flagged" % (length, aware, prob, 100 * (got == 0).mean(), int((res.flags != 0).sum())))
    _check_csr("csr alone", prep, indptr, indices, data, m_kw, res, got)
    assert 0.05 < (res.data == 0).mean() < 0.95 and (res.flags != 0).mean() <= (0.0 if not aware else PC.FLOAT_CAP)


@pytest.mark.parametrize("max_degree", [1, 22, 45])
def test_degree_prune_alone(max_degree):
    """rows of max_degree - 1, max_degree (untouched), max_degree + 1, 64, 65, 150 and 300 entries (the e0 loop), weights that
    repeat at the cut (every entry equal to the cut stays): equal to the model, bit for bit."""
    c = PC.ALL["lat_k15"]
    indptr, data = PC.degree_prune_alone(c.n, max_degree, seed=max_degree)
    want = PR.degree_prune(indptr, data, max_degree)
    b = _builder(PC.data(c), c.metric, c.k)
    try:
        got = b.degree_prune(indptr, data, max_degree)
    finally:
        b.close()
    bad = np.nonzero(np.add.reduceat(np.r_[got.view(np.uint32) != want.view(np.uint32), False].astype(np.int64), indptr[:-1]) * (np.diff(indptr) > 0))[0]
    assert not len(bad), "max_degree %d: %d rows differ, first %d (%d entries): weights %s expected %s got %s" % (
        max_degree, len(bad), bad[0], indptr[bad[0] + 1] - indptr[bad[0]], _row_text(indptr, data, bad[0]), _row_text(indptr, want, bad[0]),
        _row_text(indptr, got, bad[0]))
    assert (want == 0).any() and (want != 0).any()
