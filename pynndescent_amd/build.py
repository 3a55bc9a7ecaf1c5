"""The single-GPU build driver: every build of one ``_capi.Builder`` goes through ``_build_graph``; ``nn_descent`` is the
reference's function of that name on it.  Also the derived defaults and the input checks every build entry point shares.
"""
import time

import numpy as np
from sklearn.utils import check_array

from . import _capi
from .device_arrays import _is_device_array, _shape_of
from .metrics import _ND_ALIASES, _ND_DISTS, _NEGATIVE_HELLINGER, _metric_of


def ts():
    """Timestamp used in verbose output (reference utils.py:881-883)."""
    return time.ctime(time.time())


def _reference_defaults(n, n_neighbors, n_trees=None, n_iters=None, leaf_size=None, max_candidates=None):
    """The reference's derived defaults for what is None: (n_trees, n_iters, leaf_size, max_candidates) for ``n`` rows
    (pynndescent_.py:1009-1012, 1135-1138; rp_trees.py:2845-2846)."""
    if n_trees is None:
        n_trees = max(3, min(12, int(round(2.0 * np.log10(n)))))
    if n_iters is None:
        n_iters = max(5, int(round(np.log2(n))))
    if leaf_size is None:
        leaf_size = max(60, min(256, 5 * int(n_neighbors)))
    if max_candidates is None:
        max_candidates = min(60, n_neighbors)
    return n_trees, n_iters, leaf_size, max_candidates


def _check_array_no_scan(data):
    try:
        return check_array(data, dtype=np.float32, order="C", ensure_all_finite=False)
    except TypeError:  # scikit-learn < 1.6
        return check_array(data, dtype=np.float32, order="C", force_all_finite=False)


def _raise_if_nonfinite(builder, data):
    """The ValueError check_array raises in the reference for NaN / inf input (pynndescent_.py:1054), from the device flag."""
    if builder.data_nonfinite():
        from sklearn.utils import assert_all_finite

        if callable(data):  # a device array: only this error path brings the rows to the host, for sklearn's wording
            data = data()
        assert_all_finite(data)  # raises "Input contains NaN." / "... infinity or a value too large ..."
        raise ValueError("Input contains NaN or infinity.")  # (unreachable unless the two scans disagree)


def _check_supported_sizes(n_neighbors, max_candidates, init_graph):
    """The GPU k-lists hold at most 256 entries (four per lane of a wave; rows above 64 take the LDS-merge kernels) and the
    candidate lists at most 128 (above 64: five passes of the 64-slot join over blocks of the lists); the reference has no such bounds (pynndescent_.py:976-982), so the limits are reported up
    front and by name."""
    if int(n_neighbors) > 256 or (max_candidates is not None and int(max_candidates) > 128):
        raise NotImplementedError(
            "pynndescent_amd supports n_neighbors <= 256 and max_candidates <= 128 (got n_neighbors=%s, max_candidates=%s); "
            "use pynndescent.NNDescent (or pynndescent_amd.make_index) for wider graphs" % (n_neighbors, max_candidates))
    if init_graph is not None and len(_shape_of(init_graph)) == 2 and _shape_of(init_graph)[1] > 256:
        raise NotImplementedError("pynndescent_amd supports init_graph with at most 256 columns (got %d); use "
                                  "pynndescent.NNDescent" % _shape_of(init_graph)[1])


def _build_graph(data, m, n_neighbors, n_trees, leaf_size, max_depth, max_candidates, n_iters, delta, rng_state, tree_rng,
                 device, forest=False, leaf_array=None, init_graph=None, init_dist=None, old_graph=None, random_fill=False,
                 check_finite=False, stats=True, verbose=False, announce=False, dev_in=None):
    """Every single-GPU build (``_capi.Builder``): the data in, its flags read (the NaN / inf one only when
    ``check_finite``), ``forest`` built on the device, the graph seeded -- ``old_graph`` (ids, distances) as "old" edges,
    then ``init_graph`` / ``init_dist``, the caller's ``leaf_array`` or the forest's leaves, then the random fill when
    ``random_fill`` -- NN-descent to the stop rule, the graph out.  ``announce``: the constructor's verbose line.  ``dev_in``
    (a ``_DeviceInput``): the rows are a device array, read in place on torch's stream, and the graph comes out as tensors;
    ``old_graph`` and ``init_graph`` / ``init_dist`` may then be tensors as well (int32 / float32, read in place).  Returns
    ``((indices, distances), the stats (when ``stats``), the forest's leaf count)``."""
    n = data.shape[0]
    dim = data.shape[1] if dev_in is None else dev_in.work_dim()  # (a row map may change the width: 2 in, 3 out)
    builder = _capi.Builder(n, dim, m.code, n_neighbors, n_trees, leaf_size, max_depth, max_candidates, n_iters,
                            delta, rng_state, tree_rng, device=device)
    try:
        if dev_in is None:
            builder.set_data_host(data)
        else:
            dev_in.set_data(builder, m)
        if check_finite:
            _raise_if_nonfinite(builder, data if dev_in is None else dev_in.host_rows)
        if m.nonnegative and builder.data_negative():
            raise ValueError(_NEGATIVE_HELLINGER)
        n_leaves = None
        if forest:
            builder.make_forest()
            n_leaves = builder.stats()["n_leaves"]
        if announce:
            print(ts(), "NN descent for", str(n_iters), "iterations")
        if old_graph is not None:
            builder.reset_graph()
            if _is_device_array(old_graph[0]):  # (update() of a device-built index: the invalidated graph is a pair of tensors)
                builder.init_from_neighbor_graph_device(old_graph[0].data_ptr(), old_graph[1].data_ptr(), old_graph[0].shape[1])
            else:
                builder.init_from_neighbor_graph(*old_graph)
        if init_graph is not None and _is_device_array(init_graph):  # int32 / float32, contiguous, on the data's device
            builder.init_from_graph_device(init_graph.data_ptr(), 0 if init_dist is None else init_dist.data_ptr(), init_graph.shape[1])
        elif init_graph is not None:
            builder.init_from_graph(init_graph, init_dist)
        elif leaf_array is not None:
            builder.init_from_leaf_array(leaf_array)
        elif forest:
            builder.init_from_leaves()
        if random_fill:
            builder.init_random()
        _descend(builder, n, n_neighbors, n_iters, delta, verbose)
        graph = builder.finalize() if dev_in is None else dev_in.finalize(builder)
        return graph, builder.stats() if stats else None, n_leaves
    finally:
        builder.close()
        if dev_in is not None:
            dev_in.close()


def _descend(builder, n, n_neighbors, n_iters, delta, verbose):
    """nn_descent_internal (pynndescent_.py:296-320): the library's loop (nnd_descent, no host round trip per iteration),
    or with ``verbose`` the same iterations and stop rule driven from here, so that the output matches the reference's."""
    if not verbose:
        builder.descent()
        return
    for it in range(n_iters):
        print("\t", it + 1, " / ", n_iters)
        c = builder.descent_iter()
        if c <= delta * n_neighbors * n:
            print("\tStopping threshold met -- exiting after", it + 1, "iterations")
            break


EMPTY_GRAPH = (np.array([[-1]], dtype=np.int32), np.array([[np.inf]], dtype=np.float32),
               np.array([[0]], dtype=np.uint8))  # pynndescent_.py:64-68


def nn_descent(data, n_neighbors, rng_state, max_candidates=50, dist="squared_euclidean", n_iters=10, delta=0.001,
               init_graph=EMPTY_GRAPH, rp_tree_init=True, leaf_array=None, low_memory=True, verbose=False, device=0):
    """The reference's ``nn_descent`` (pynndescent_.py:323-366) with the same arguments, on the GPU: the seam a caller
    uses who keeps the reference's ``make_forest`` / ``rptree_leaf_array`` and hands the leaves in.

    data float32 (n, d); rng_state int64[3]; ``dist``: "squared_euclidean" / "alternative_cosine" / "alternative_dot" /
    "alternative_inner_product" / "correlation" / "alternative_hellinger" (what NNDescent passes, pynndescent_.py:1247-1260),
    "euclidean" / "cosine" / "dot" / "inner_product" / "hellinger" (true distances: the same kernels, corrected on return),
    "proxy_inner_product" (the proxy distances themselves: it has no correction), the boolean metrics "jaccard" (corrected
    on return; "alternative_jaccard": its kernel distance) / "dice" / "sokalsneath" / "matching" / "rogerstanimoto" /
    "sokalmichener" / "kulsinski" / "russellrao" / "yule",
    or the reference function of one of those names (dot: the kernels rank by the L2-normalised rows, as NNDescent's
    normalised data gives; hand in normalised rows for the reference's ranking); ``init_graph``: EMPTY_GRAPH, or the heap triple ``(indices (n, k),
    distances (n, k), flags (n, k))`` the reference accepts (entries with index -1 are empty); ``leaf_array`` int32
    (n_leaves, max_leaf_size), -1 padded, used when ``rp_tree_init``.  ``low_memory`` is accepted and unused, as in the
    reference (pynndescent_.py:335).  Returns ``(indices int32 (n, k), distances float32 (n, k))``, rows ascending."""
    name = dist if isinstance(dist, str) else getattr(dist, "__name__", None)
    if name not in _ND_DISTS:
        raise NotImplementedError("pynndescent_amd.nn_descent: dist must be one of %s (got %r)" % (sorted(_ND_DISTS), dist))
    m, correction = _metric_of(_ND_ALIASES.get(name, name)), _ND_DISTS[name][1]
    data = np.ascontiguousarray(data, dtype=np.float32)
    n = data.shape[0]
    _check_supported_sizes(n_neighbors, max_candidates, None)
    empty = init_graph[0].shape[0] == 1  # EMPTY_GRAPH
    if not empty and not (init_graph[0].shape[0] == n and init_graph[0].shape[1] == n_neighbors):
        raise ValueError("Invalid initial graph specified!")  # pynndescent_.py:352
    if empty and rp_tree_init and leaf_array is None:
        raise ValueError("rp_tree_init=True needs a leaf_array (rptree_leaf_array of a forest)")
    leaf_size = _reference_defaults(n, n_neighbors, 0, n_iters, None, max_candidates)[2]
    # (a heap handed over: its entries, with their distances; flags restart as "new": they were never sampled here)
    (idx, dst), _, _ = _build_graph(
        data, m, n_neighbors, 0, leaf_size, 200, max_candidates, n_iters, delta, np.asarray(rng_state, np.int64),
        np.zeros(3, np.int64), device, leaf_array=leaf_array if empty and rp_tree_init else None,
        init_graph=None if empty else np.asarray(init_graph[0], np.int32),
        init_dist=None if empty else np.asarray(init_graph[1], np.float32), random_fill=empty, stats=False, verbose=verbose)
    if correction is not None:
        dst = correction(dst).astype(np.float32)
    return idx, dst
