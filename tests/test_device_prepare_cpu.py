"""The host side of the device prepare() that needs neither a GPU nor torch: the new entry points are declared, exported and
bound; the path chooser, on stub objects; and the "is this index prepared?" flag, which must not fetch a host mirror."""
import os
import re

import pytest

from pynndescent_amd import _capi
from pynndescent_amd import nndescent as N
from pynndescent_amd.search_graph import DEVICE_PASS_MAX_EDGES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nnd_rank_order_device", "nnd_hub_tree_build_device", "nnd_search_graph_device", "nnd_reorder_csr_device",
               "nnd_reorder_host", "nnd_searcher_create_device")


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "pynnd_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nnd_[a-z_0-9]+)\s*\(", text))
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, "include/pynnd_amd.h does not declare %s" % name
        assert name in _capi.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    assert lib.nnd_abi_version() == 6
    for name in ("rank_order_device", "reorder_csr_device", "reorder_host"):
        assert callable(getattr(_capi, name))
    assert callable(_capi.Searcher.from_device) and callable(_capi.Builder.hub_tree_device) and callable(_capi.Builder.search_graph_device)


class _Tensor:
    """What the chooser reads of a device tensor: its shape.  Anything that would bring it to the host raises."""

    def __init__(self, *shape):
        self.shape = tuple(shape)

    def _no(self, *a, **k):
        raise AssertionError("the device tensor was touched")

    detach = cpu = float = numpy = __getitem__ = _no


class _Index:
    """The attributes ``_prepares_on_device`` looks at, on an object that is no NNDescent."""

    def __init__(self, n=1000, k=10, **over):
        self.metric, self.quantization, self.n_devices = "euclidean", None, 1
        self._device_data, self._device_graph = _Tensor(n, 8), (_Tensor(n, k), _Tensor(n, k))
        for name, value in over.items():
            if value is None and name.startswith("_device"):
                self.__dict__.pop(name)
            else:
                setattr(self, name, value)


def test_path_chooser():
    assert N._prepares_on_device(_Index())
    assert N._prepares_on_device(_Index(metric="cosine", quantization="uint8"))
    assert N._prepares_on_device(_Index(metric="dot"))
    # host-built (no tensors), or one of the two gone (compressed: no graph; after update(): neither)
    assert not N._prepares_on_device(_Index(_device_data=None, _device_graph=None))
    assert not N._prepares_on_device(_Index(_device_graph=None))
    assert not N._prepares_on_device(_Index(_device_data=None))
    assert not N._prepares_on_device(_Index(n_devices=2))
    assert not N._prepares_on_device(_Index(metric="dot", quantization="uint8"))  # codes of rows other than the searcher's copy
    assert not N._prepares_on_device(_Index(_host_prepare=True))  # the host-path switch
    # 2 n k edges with int32 positions: the bound of the device pass
    k = 256
    n_fits = (DEVICE_PASS_MAX_EDGES - 1) // (2 * k)
    assert 2 * n_fits * k < DEVICE_PASS_MAX_EDGES <= 2 * (n_fits + 1) * k
    assert N._prepares_on_device(_Index(n=n_fits, k=k))
    assert not N._prepares_on_device(_Index(n=n_fits + 1, k=k))


def test_host_path_switch_is_off_by_default():
    assert N.NNDescent._host_prepare is False
    index = object.__new__(N.NNDescent)
    index.__dict__.update(_Index().__dict__)
    assert N._prepares_on_device(index)
    index._host_prepare = True
    assert not N._prepares_on_device(index)


def test_prepared_flag_fetches_no_mirror():
    index = object.__new__(N.NNDescent)
    index.__dict__.update(_Index().__dict__)  # tensors whose every way to the host raises
    assert index._prepared is False
    index._vertex_order = [0]
    assert index._prepared is True
    with pytest.raises(AssertionError, match="touched"):  # (the stub does raise when a mirror is asked for)
        index._raw_data
    for name in ("_raw_data", "_neighbor_graph", "_search_graph", "_quantized_data"):
        assert name not in index.__dict__
    with pytest.raises(RuntimeError, match="prepared already"):  # decided by the flag, before any mirror is read
        index.build_search_graph()
