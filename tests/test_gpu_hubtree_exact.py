"""The hub search tree of prepare() (csrc/hubtree.hip, entry nnd_hub_tree_build) against its step-exact host model
(tests/hubtree_reference.py) at the shapes of tests/hubtree_cases.py: every table byte for byte against the model's float32
arithmetic, and every split through check mode.  A mismatch names the node, the depth, the hubs, the candidate and the members."""
import time

import numpy as np
import pytest

from pynndescent_amd import _capi
from pynndescent_amd.search_tree import make_hub_tree
from tests import hubtree_cases as HC
from tests import hubtree_reference as HR

pytestmark = pytest.mark.gpu


def _differences(got, want):
    names = ("hyperplanes", "offsets", "children", "indices")
    out = []
    for name, a, b in zip(names, got[:4], want[:4]):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            out.append("%s: shape %s, the model's %s" % (name, a.shape, b.shape))
        elif not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            rows = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(1))
            out.append("%s: %d rows differ, first %s" % (name, len(rows), rows[:5].tolist()))
    if int(got[4]) != int(want[4]):
        out.append("leaf_size %d, the model's %d" % (got[4], want[4]))
    return out


def _builder(c, seed=0):
    n, d = c.x.shape
    b = _capi.Builder(n, d, _capi.METRIC_CODES[c.metric], 1, 1, max(int(c.leaf_size), 1), c.max_depth, 1, 1, 0.001, [seed, 2, 3], [4, 5, 6],
                      device=0, flags=_capi.NND_FLAG_NO_GRAPH | _capi.NND_FLAG_NO_PREP)   # (search_tree.py make_hub_tree's handle)
    return b


@pytest.mark.parametrize("name", HC.NAMES)
def test_hub_tree_is_the_models(name):
    c = HC.case(name)
    n = c.x.shape[0]
    t0 = time.perf_counter()
    tree = make_hub_tree(c.x, c.nbr, c.metric, leaf_size=c.leaf_size, max_depth=c.max_depth)   # the C ABI entry nnd_hub_tree_build
    t1 = time.perf_counter()
    want = HR.exact32(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric)
    if name == "segments-n4096":
        assert max(want.stats["level_segments"].values()) > 256, "the case did not reach what it is for"
    res = HR.check(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric, tree, c.exact)
    t2 = time.perf_counter()
    diff = _differences(tree, want.tree)
    print("%s: %d nodes (model %d), unclear %d / %d decisions, %d mismatches, differences from exact32: %s" % (
        name, tree.children.shape[0], len(want.nodes), res.unclear, res.decisions, len(res.mismatch), diff or "none"))
    assert not res.mismatch, "%s:\n%s" % (name, HR.describe(res.mismatch))
    assert res.unclear <= HC.UNCLEAR_CAP * max(res.decisions, 1), (name, res.unclear, res.decisions)
    if c.exact:
        assert res.unclear == 0
    assert not diff, "%s: the tree is not the model's float32 tree: %s" % (name, diff)
    assert np.asarray(tree.hyperplanes).dtype == np.float32 and np.asarray(tree.children).dtype == np.int32
    # the tree does not depend on the handle's seed, nor on what the handle built before
    other = make_hub_tree(c.x, c.nbr, c.metric, leaf_size=c.leaf_size, max_depth=c.max_depth, seed=987654321)
    assert HR.same_tables(other, tree), "a handle with another seed builds another tree"
    b = _builder(c, seed=5)
    try:
        b.set_data_host(c.x)
        ro = HR.rank_order(HR.degrees(c.nbr, n))
        first = b.hub_tree(ro, c.leaf_size, c.max_depth)
        second = b.hub_tree(ro, c.leaf_size, c.max_depth)
    finally:
        b.close()
    assert HR.same_tables(first, tree) and HR.same_tables(second, tree), "a second build on the handle differs"
    print("%s: GPU build %.2f s, host model and check %.2f s, all %.2f s" % (name, t1 - t0, t2 - t1, time.perf_counter() - t0))


@pytest.mark.parametrize("name", HC.DEVICE_ENTRY)
def test_device_entry_builds_the_same_bytes(name):
    """the graph, the rank order and the rows on the device (rank_order_device + hub_tree_device, the path of an index built from a
    device array): the same tables."""
    torch = pytest.importorskip("torch")
    c = HC.case(name)
    n, k = c.nbr.shape
    t0 = time.perf_counter()
    want = HR.exact32(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric).tree
    g = torch.from_numpy(np.array(c.nbr)).to("cuda:0")
    x = torch.from_numpy(np.array(c.x)).to("cuda:0")
    rank = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    _capi.rank_order_device(0, 0, g.data_ptr(), n, k, rank.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(rank.cpu().numpy(), HR.rank_order(HR.degrees(c.nbr, n)))
    b = _builder(c)
    try:
        b.set_data_device(x.data_ptr(), keepalive=x)
        tables = b.hub_tree_device(rank.data_ptr(), c.leaf_size, c.max_depth)
    finally:
        b.close()
    diff = _differences(tables, want)
    assert not diff, "%s: %s" % (name, diff)
    print("%s: %.2f s" % (name, time.perf_counter() - t0))
