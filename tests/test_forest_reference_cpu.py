"""The forest's host model (tests/forest_reference.py) tested without a GPU: its dry-run forests are forests of the oracle's family,
its checker accepts them and rejects every mutation at the node where the mutation first takes effect, and its hashes are the
library's.  Without the mutation tests the comparison of tests/test_gpu_forest_exact.py could be vacuous."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import forest_cases as FC
from tests import forest_reference as FR
from tests.search_reference import hash2, hash3, searcher_seed

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pynndescent_amd", "csrc")
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or shutil.which("/opt/rocm/bin/hipcc")

SMALL_ROUTING = FC.Case("routing-8192", "clustered", 8192, 20, "cosine", 2, 60, 200, False, 1)  # the routing machinery, forced
_RUNS = {}


def _run(c, **hooks):
    """(data, model, dry-run result) of a case, computed once and left unchanged."""
    key = (c, repr(sorted(hooks.items())))
    if key not in _RUNS:
        x = FC.case_data(c)
        m = FC.case_model(c, x, **hooks)
        _RUNS[key] = (x, m, m.run(), list(m.trace))
    return _RUNS[key]


def _leaves(la):
    return [row[row >= 0] for row in la]


def _array(leaves, leaf_size):
    out = np.full((len(leaves), max([leaf_size] + [len(v) for v in leaves])), -1, np.int32)
    for i, v in enumerate(leaves):
        out[i, :len(v)] = v
    return out


def _lca(trace, tree, lo, hi):
    """the deepest split of ``tree`` whose segment holds the positions [lo, hi)."""
    best = None
    for regime, t, depth, a, ln in trace:
        if regime != "cell" and t == tree and a <= lo and hi <= a + ln and (best is None or depth > best[2]):
            best = (regime, t, depth, a, ln)
    return best


CPU_CASES = ["nn-euclidean", "nn-cosine", "one-leaf", "leaf+1", "n2048", "n2049-d33-T1", "n6000-d130-T5", "n6000-hellinger", "n20000-T2",
             "depth3", "depth9", "lattice-ip", "lattice-euclidean", "groups-small-euclidean", "groups-cosine"]


@pytest.mark.parametrize("name", CPU_CASES + ["routing-8192"])
def test_dry_run_is_a_partition_and_the_checker_accepts_it(name):
    c = SMALL_ROUTING if name == "routing-8192" else FC.CASES[name]
    x, m, res, _ = _run(c, **({"routing": True} if c is SMALL_ROUTING else {}))
    la = res.leaf_array
    ids = la[la >= 0]
    assert ids.shape[0] == c.T * c.n and np.all(np.bincount(ids, minlength=c.n) == c.T)  # every tree holds every point once
    lens = (la >= 0).sum(1)
    assert lens.min() >= 1 and np.all((la >= 0) == (np.arange(la.shape[1])[None, :] < lens[:, None]))  # -1 only at the row tails
    if c.max_depth >= 200:
        assert la.shape[1] == c.leaf_size and lens.max() <= c.leaf_size
    else:
        assert la.shape[1] == lens.max() > c.leaf_size  # the array is as wide as the longest leaf
    assert (res.n_cells > 0) == (c is SMALL_ROUTING)
    chk = m.run(la)
    assert all(mm is None for mm in chk.mismatch), FR.describe(chk.mismatch)
    assert (chk.decisions, chk.unclear) == (res.decisions, res.unclear)
    assert np.array_equal(chk.leaf_array, la)
    assert res.unclear <= FC.UNCLEAR_CAP * max(res.decisions, 1)
    if c.exact:
        assert res.unclear == 0  # the lattice: nothing is unclear


@pytest.mark.parametrize("name", ["nn-euclidean", "nn-cosine", "n2048", "n6000-d130-T5", "n20000-T2", "routing-8192"])
def test_dry_run_forests_are_the_oracles_family(name):
    """mean leaf fill against the reference algorithm's forest within the 15 % the GPU forest is held to (test_forest_partitions)."""
    c = SMALL_ROUTING if name == "routing-8192" else FC.CASES[name]
    x, _, res, _ = _run(c, **({"routing": True} if c is SMALL_ROUTING else {}))
    _, _, ts = O.draw_rng_states(1, c.T)
    ola = O.make_leaf_array(x, c.T, c.leaf_size, ts, O.ANGULAR[c.metric])
    fill, ofill = (res.leaf_array >= 0).sum(1).mean(), (ola >= 0).sum(1).mean()
    assert abs(fill - ofill) <= 0.15 * ofill, (fill, ofill)


# ------------------------------------------------------------------------------------------------ mutations
MUTATED = ["n2048", "n6000-d130-T5", "n20000-T2"]  # finisher from the root; level passes + LDS finisher; the global-memory tail


def _first_two_leaves(c, res, tree):
    leaves = _leaves(res.leaf_array)
    i = int(np.searchsorted(np.cumsum([len(v) for v in leaves]), tree * c.n, side="right"))  # first leaf of the tree
    return leaves, i


@pytest.mark.parametrize("name", MUTATED)
def test_checker_rejects_a_member_moved_across_a_split(name):
    c = FC.CASES[name]
    x, m, res, trace = _run(c)
    tree = c.T - 1
    leaves, i = _first_two_leaves(c, res, tree)
    last = len(leaves) - 1  # the tree's last leaf: the root separates it from the first
    moved = 0
    for v in leaves[i][:4]:  # (an unclear member may move: hardly any member is unclear)
        mut = list(leaves)
        mut[i] = leaves[i][leaves[i] != v]
        mut[last] = np.sort(np.append(leaves[last], v))
        chk = m.run(_array(mut, c.leaf_size))
        if chk.mismatch[tree] is not None:
            moved += 1
            mm = chk.mismatch[tree]
            assert (mm["depth"], mm["a"], mm["len"]) == (0, 0, c.n), mm
            assert v in [mem[0] for mem in mm["members"]], mm
            assert all(chk.mismatch[t] is None for t in range(tree))
    assert moved >= 3


@pytest.mark.parametrize("name", MUTATED)
def test_checker_rejects_a_swap_between_neighbouring_leaves(name):
    c = FC.CASES[name]
    x, m, res, trace = _run(c)
    leaves, i = _first_two_leaves(c, res, 0)
    a, b = leaves[i], leaves[i + 1]
    want = _lca(trace, 0, 0, len(a) + len(b))
    mut = list(leaves)
    mut[i] = np.sort(np.append(a[1:], b[0]))
    mut[i + 1] = np.sort(np.append(b[1:], a[0]))
    mm = m.run(_array(mut, c.leaf_size)).mismatch[0]
    assert mm is not None and (mm["regime"], mm["depth"], mm["a"], mm["len"]) == (want[0], want[2], want[3], want[4]), (mm, want)


@pytest.mark.parametrize("name", MUTATED)
def test_checker_rejects_a_leaf_cut_one_position_early(name):
    c = FC.CASES[name]
    x, m, res, trace = _run(c)
    leaves, i = _first_two_leaves(c, res, 0)
    a, b = leaves[i], leaves[i + 1]
    want = _lca(trace, 0, 0, len(a) + len(b))
    mut = list(leaves)
    mut[i], mut[i + 1] = a[:-1], np.append(a[-1:], b)  # the same permutation, the boundary one position early
    mm = m.run(_array(mut, c.leaf_size)).mismatch[0]
    assert mm is not None and (mm["regime"], mm["depth"], mm["a"], mm["len"]) == (want[0], want[2], want[3], want[4]), (mm, want)


@pytest.mark.parametrize("name", MUTATED)
def test_checker_rejects_an_unsorted_leaf(name):
    c = FC.CASES[name]
    x, m, res, trace = _run(c)
    leaves = _leaves(res.leaf_array)
    j = len(leaves) // 2
    start = sum(len(v) for v in leaves[:j])
    mut = list(leaves)
    mut[j] = np.concatenate([leaves[j][1:2], leaves[j][0:1], leaves[j][2:]])
    chk = m.run(_array(mut, c.leaf_size))
    tree = start // c.n
    mm = chk.mismatch[tree]
    assert mm is not None and (mm["regime"], mm["a"], mm["len"]) == ("leaf", start - tree * c.n, len(leaves[j])), mm
    assert all(chk.mismatch[t] is None for t in range(c.T) if t != tree)


@pytest.mark.parametrize("name", MUTATED + ["routing-8192"])
def test_checker_rejects_a_tree_built_with_another_trees_salt(name):
    c = SMALL_ROUTING if name == "routing-8192" else FC.CASES[name]
    hooks = {"routing": True} if c is SMALL_ROUTING else {}
    x, m, res, trace = _run(c, **hooks)
    _, _, wrong, _ = _run(c, tree_alias={1: 0}, **hooks)
    assert not np.array_equal(wrong.leaf_array, res.leaf_array)
    chk = m.run(wrong.leaf_array)
    mm = chk.mismatch[1]
    assert mm is not None and (mm["depth"], mm["a"]) == (0, 0), mm  # the root: the first draw of the tree
    if name in ("n2048", "routing-8192"):  # (level passes: the other trees' regimes depend on this tree's sizes through active_pos)
        assert all(chk.mismatch[t] is None for t in range(c.T) if t != 1)


def test_checker_rejects_cells_finished_from_depth_0():
    c = SMALL_ROUTING
    x, m, res, trace = _run(c, routing=True)
    _, _, wrong, _ = _run(c, routing=True, cells_from_depth0=True)
    chk = m.run(wrong.leaf_array)
    cells = {(t, depth, a, ln) for regime, t, depth, a, ln in trace if regime == "cell" and ln > c.leaf_size}
    assert len(cells) > 20 and min(depth for _, depth, _, _ in cells) > 0
    for t in range(c.T):
        mm = chk.mismatch[t]
        assert mm is not None and mm["regime"] == "finisher", mm
        assert (t, mm["depth"], mm["a"], mm["len"]) in cells, mm  # the root of a cell's subtree


def test_checker_rejects_what_is_not_a_partition():
    c = FC.CASES["n2048"]
    x, m, res, _ = _run(c)
    la = res.leaf_array.copy()
    la[0, 0] = la[0, 1]
    chk = m.run(la)
    assert chk.mismatch[0] is not None and chk.mismatch[0]["regime"] == "partition" and chk.mismatch[1] is None


# ------------------------------------------------------------------------------------------------ routing cases, hashes
@pytest.mark.parametrize("name", ["route-131072-d32-T2", "route-140000-d32-T2"])
def test_routing_seed_is_the_smallest_recording_clear_seed(name):
    c = FC.CASES[name]
    assert FC.recording_clear_seed(c) == c.seed


@pytest.mark.parametrize("name", [c.name for c in FC.ROUTING])
def test_routing_cases_have_clear_recording_decisions(name):
    c = FC.CASES[name]
    m = FC.case_model(c)
    assert m.routing
    m.record_tops()
    assert not any(m.recording_unclear), m.recording_unclear


def test_routing_case_dry_run():
    c = FC.CASES["route-131072-d32-T2"]
    x, m, res, _ = _run(c)
    assert res.n_cells > 0 and not any(res.recording_unclear) and res.unclear <= FC.UNCLEAR_CAP * res.decisions
    chk = m.run(res.leaf_array)
    assert all(mm is None for mm in chk.mismatch), FR.describe(chk.mismatch)
    _RUNS.clear()  # (the largest arrays of the module)


def test_vector_hashes_are_the_scalar_ones():
    a = np.array([0, 1, 2, 59, 131071, 0x7FFFFFFF, 0xFFFFFFF0], np.int64)
    for seed in (1, 0x9E3779B9, 0xFFFFFFFF):
        assert [int(v) for v in FR.hash2v(seed, a)] == [hash2(seed, int(i)) for i in a]
        for b in (0, 7, 401):
            assert [int(v) for v in FR.hash3v(seed, a, b)] == [hash3(seed, int(i), b) for i in a]
            assert int(FR.hash3v(seed, 5, b)) == hash3(seed, 5, b)


@pytest.mark.skipif(HIPCC is None, reason="no hipcc: csrc/common.h needs the HIP headers")
def test_python_hashes_and_seed_are_the_librarys(tmp_path):
    """tests/forest_hash_cpu.cpp includes csrc/common.h and prints nnd_hash2 / nnd_hash3 / the seed derivation on the host."""
    exe = str(tmp_path / "forest_hash_cpu")
    r = subprocess.run([HIPCC, "--offload-host-only", "-O1", "-I", CSRC, os.path.join(HERE, "forest_hash_cpu.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == 51
    for f in lines:
        v = [int(t) for t in f[1:]]
        if f[0] == "hash2":
            assert hash2(v[0], v[1]) == v[2] == int(FR.hash2v(v[0], v[1])), f
        elif f[0] == "hash3":
            assert hash3(v[0], v[1], v[2]) == v[3] == int(FR.hash3v(v[0], v[1], v[2])), f
        else:
            assert searcher_seed(np.array(v[:3], np.int64)) == v[3] == FR.tree_seed_of(np.array(v[:3], np.int64)), f
