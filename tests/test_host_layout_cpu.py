"""The layout of the host package: which module holds what, that ``pynndescent_amd.nndescent`` still hands out every name it
once defined (the same objects), that the metrics are one table, and that an index drops exactly the device state it dropped
before the names of that state were grouped.  No GPU, no library."""
import os
import pickle
import subprocess
import sys

import pytest

from pynndescent_amd import build, device_arrays, exact, metrics, nndescent
from pynndescent_amd.nndescent import NNDescent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every module-level name nndescent.py defined when it was one file, by the module that holds it now
HOMES = {
    metrics: ["_ANGULAR_METRICS", "_BOOLEAN_METRICS", "_DISTANCE_CORRECTIONS", "_KNOWN_REFERENCE_METRICS", "_LINEAR_METRICS",
              "_METRICS", "_Metric", "_ND_ALIASES", "_ND_DISTS", "_NEGATIVE_HELLINGER", "_check_quantization", "_linear_map_of",
              "_metric_of", "_metric_record", "_no_exact_for_proxy", "_raise_if_negative_host", "correct_alternative_cosine",
              "correct_alternative_hellinger", "correct_alternative_inner_product"],
    device_arrays: ["_DEVICE_DTYPES", "_DeviceInput", "_DeviceLinear", "_DeviceRowsView", "_OnTorchStream", "_check_device_array",
                    "_device_corrected", "_dtype_name", "_ids_to_host", "_is_device_array", "_resolve_updated_indices",
                    "_rows_to_host", "_shape_of", "_stream_ms", "_torch", "_update_dtype"],
    build: ["EMPTY_GRAPH", "_build_graph", "_check_array_no_scan", "_check_supported_sizes", "_descend", "_raise_if_nonfinite",
            "_reference_defaults", "nn_descent", "ts"],
    exact: ["_exact_knn_device", "_exact_linear_rows", "exact_knn"],
}
STAYED = ["INT32_MAX", "INT32_MIN", "NNDescent", "_DeviceForestSentinel", "_FROM_GRAPH_DEFAULTS", "_prepares_on_device",
          "_proxy_search_k", "_updates_on_device", "make_index", "tau_rand_int", "uint8_codebook"]
RENAMED = {"_refuse_with_linear": (metrics, "_refuse_uint8_and_sharding")}

PLAIN = ["euclidean", "l2", "sqeuclidean", "cosine", "dot", "inner_product", "correlation", "hellinger", "proxy_inner_product"]
LINEAR = ["seuclidean", "standardised_euclidean", "wminkowski", "weighted_minkowski", "mahalanobis", "minkowski"]
BOOLEAN = ["jaccard", "dice", "sokalsneath", "matching", "rogerstanimoto", "sokalmichener", "kulsinski", "russellrao", "yule"]


def test_every_name_is_still_in_nndescent_and_is_its_home_modules_object():
    assert sum(len(names) for names in HOMES.values()) + len(STAYED) + len(RENAMED) == 59  # what the one file defined
    for module, names in HOMES.items():
        for name in names:
            assert getattr(nndescent, name) is getattr(module, name), name
    for name in STAYED:
        assert hasattr(nndescent, name), name
        assert not any(hasattr(module, name) for module in HOMES), name
    for old, (module, new) in RENAMED.items():
        assert getattr(nndescent, old) is getattr(module, new) is getattr(nndescent, new)


def test_the_functions_tests_replace_have_one_home():
    """``ts`` and ``_torch`` are called through their home module everywhere, so one ``setattr`` replaces them for all callers:
    no other module of the package may bind them by name and call that."""
    import ast

    for name, home in (("ts", "build"), ("_torch", "device_arrays")):
        for module in ("nndescent", "build", "device_arrays", "exact", "metrics", "sharded"):
            if module == home:
                continue
            tree = ast.parse(open(os.path.join(ROOT, "pynndescent_amd", module + ".py")).read())
            bare = [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == name]
            assert not bare, "%s.py calls %s() by its bare name at lines %s" % (module, name, bare)


def test_the_package_exports_what_it_did():
    import pynndescent_amd

    for name in ("EMPTY_GRAPH", "NNDescent", "exact_knn", "make_index", "nn_descent"):
        assert getattr(pynndescent_amd, name) is getattr(nndescent, name)


def test_one_table_and_three_disjoint_views():
    table = metrics._METRIC_TABLE
    views = [metrics._METRICS, metrics._LINEAR_METRICS, metrics._BOOLEAN_METRICS]
    assert [list(v) for v in views] == [PLAIN, LINEAR, BOOLEAN]
    assert list(table) == PLAIN + LINEAR + BOOLEAN
    for i, a in enumerate(views):
        for b in views[i + 1:]:
            assert not set(a) & set(b)
    assert {k: v for view in views for k, v in view.items()} == table
    for name in table:
        assert metrics._metric_record(name) is metrics._metric_of(name) is table[name]
        assert table[name] is [v for v in views if name in v][0][name]
    assert not any(m.linear or m.boolean for m in metrics._METRICS.values())
    assert all(m.linear and not m.boolean for m in metrics._LINEAR_METRICS.values())
    assert all(m.boolean and not m.linear for m in metrics._BOOLEAN_METRICS.values())
    # the views by one field stay views of the plain records
    assert set(metrics._DISTANCE_CORRECTIONS) == set(PLAIN)
    assert metrics._ANGULAR_METRICS == frozenset(["cosine", "dot", "correlation", "hellinger"])


def test_a_name_off_the_table_raises_what_it_did():
    with pytest.raises(NotImplementedError, match="use pynndescent.NNDescent for metric 'manhattan'"):
        metrics._metric_record("manhattan")
    with pytest.raises(NotImplementedError):
        metrics._metric_record(lambda a, b: 0.0)
    with pytest.raises(ValueError, match="Metric is neither callable, nor a recognised string"):
        metrics._metric_record("manhattan", reference_fallback=False)
    with pytest.raises(ValueError, match="Metric is neither callable, nor a recognised string"):
        metrics._metric_record("no such metric")
    with pytest.raises(KeyError):
        metrics._metric_of("manhattan")


def test_the_names_nn_descent_takes():
    assert sorted(metrics._ND_DISTS) == [
        "alternative_cosine", "alternative_dot", "alternative_hellinger", "alternative_inner_product", "alternative_jaccard",
        "correlation", "cosine", "dice", "dot", "euclidean", "hellinger", "inner_product", "jaccard", "kulsinski", "l2", "matching",
        "proxy_inner_product", "rogerstanimoto", "russellrao", "sokalmichener", "sokalsneath", "sqeuclidean", "squared_euclidean",
        "yule"]
    assert {name: (code, correction is None) for name, (code, correction) in metrics._ND_DISTS.items()} == {
        "euclidean": (0, False), "l2": (0, False), "sqeuclidean": (0, True), "cosine": (1, False), "dot": (2, False),
        "inner_product": (3, False), "correlation": (4, True), "hellinger": (5, False), "proxy_inner_product": (6, True),
        "squared_euclidean": (0, True), "alternative_cosine": (1, True), "alternative_dot": (2, True),
        "alternative_inner_product": (3, True), "alternative_hellinger": (5, True), "jaccard": (8, False), "dice": (9, True),
        "sokalsneath": (10, True), "matching": (11, True), "rogerstanimoto": (12, True), "sokalmichener": (13, True),
        "kulsinski": (14, True), "russellrao": (15, True), "yule": (16, True), "alternative_jaccard": (8, True)}
    assert metrics._ND_ALIASES == {
        "squared_euclidean": "sqeuclidean", "alternative_cosine": "cosine", "alternative_dot": "dot",
        "alternative_inner_product": "inner_product", "alternative_hellinger": "hellinger", "alternative_jaccard": "jaccard"}
    for name, (_, correction) in metrics._ND_DISTS.items():  # a name that is corrected: by its metric's own correction
        if correction is not None:
            assert correction is metrics._METRIC_TABLE[name].correction


@pytest.mark.parametrize("module", ["metrics", "device_arrays", "build", "exact"])
def test_no_new_module_imports_torch(module):
    code = "import sys; import pynndescent_amd.%s; sys.exit(1 if 'torch' in sys.modules else 0)" % module
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, "torch was imported by `import pynndescent_amd.%s`\n%s" % (module, r.stderr)


def test_sharded_does_not_import_nndescent():
    """``sharded`` takes the derived defaults from ``build``; ``nndescent`` imports ``sharded`` (lazily), not the other way round."""
    import ast

    tree = ast.parse(open(os.path.join(ROOT, "pynndescent_amd", "sharded.py")).read())
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level:
            imported |= {node.module} if node.module else {a.name for a in node.names}
    assert "nndescent" not in imported and "build" in imported


@pytest.mark.parametrize("name", ["correct_alternative_cosine", "correct_alternative_inner_product", "correct_alternative_hellinger"])
def test_pickles_that_name_the_old_module_load(name):
    """``__getstate__`` copies ``_distance_correction`` into the state: an index pickled when the corrections lived in
    nndescent.py names them there."""
    fn = getattr(metrics, name)
    assert pickle.loads(b"cpynndescent_amd.nndescent\n" + name.encode() + b"\n.") is fn
    assert pickle.loads(pickle.dumps(fn)) is fn


def test_drop_device_copies_drops_what_it_dropped():
    groups = (NNDescent._DEVICE_TENSORS, NNDescent._LINEAR_COPIES, NNDescent._SEARCH_STRUCTURES, NNDescent._HOST_MIRRORS)
    every = set().union(*groups)
    assert every == {"_device_graph", "_device_data", "_device_raw", "_device_order", "_device_search_graph",
                     "_device_prepare_stats", "_device_linear", "_lin_data", "_search_graph", "_search_forest", "_vertex_order",
                     "_searcher", "_raw_data", "_neighbor_graph", "_quantized_data"}
    index = object.__new__(NNDescent)
    index.__dict__.update({name: object() for name in every}, metric="euclidean")
    index._drop_device_copies()
    assert set(index.__dict__) == {"metric", "_device_linear", "_lin_data", "_search_graph", "_search_forest", "_vertex_order",
                                   "_searcher", "_raw_data", "_neighbor_graph", "_quantized_data"}


def test_getstate_drops_what_it_dropped():
    """The pickled state leaves behind the device tensors, both copies made of the linear map, the build forest's stand-in and
    the searcher; the host mirrors and the search structures travel."""
    every = set().union(NNDescent._DEVICE_TENSORS, NNDescent._LINEAR_COPIES, NNDescent._SEARCH_STRUCTURES, NNDescent._HOST_MIRRORS)
    index = object.__new__(NNDescent)
    index.__dict__.update({name: object() for name in every}, metric="euclidean", _rp_forest=object(), _search_forest=[])
    state = index.__getstate__()
    assert set(state) == {"metric", "_search_graph", "_search_forest", "_vertex_order", "_raw_data", "_neighbor_graph",
                          "_quantized_data"}
    assert set(index.__dict__) == every | {"metric", "_rp_forest"}  # (the index itself keeps everything)
