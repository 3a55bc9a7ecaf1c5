"""The host side of the device-array path that needs neither a GPU nor torch: the validator of device arrays, driven by a stub
with the attributes the package looks at, and the promise that importing the package does not import torch."""
import os
import subprocess
import sys

import pytest

from pynndescent_amd import _capi
from pynndescent_amd import nndescent as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Device:
    def __init__(self, index):
        self.type, self.index = "cuda", index


class StubArray:
    """What the package reads of a device array: is_cuda, data_ptr(), dtype, shape, device, is_contiguous(), contiguous()."""

    def __init__(self, shape, dtype="torch.float32", device=0, contiguous=True, is_cuda=True):
        self.shape, self.dtype, self.device, self.is_cuda = tuple(shape), dtype, _Device(device), is_cuda
        self._contiguous, self.made_contiguous = contiguous, 0

    def data_ptr(self):
        return 0x1000

    def is_contiguous(self):
        return self._contiguous

    def contiguous(self):
        out = StubArray(self.shape, self.dtype, self.device.index)
        out.made_contiguous = self.made_contiguous + 1
        return out


def test_what_counts_as_a_device_array():
    import numpy as np

    assert N._is_device_array(StubArray((4, 3)))
    assert not N._is_device_array(StubArray((4, 3), is_cuda=False))  # a host tensor goes through check_array as before
    assert not N._is_device_array(np.zeros((4, 3), np.float32))
    assert not N._is_device_array([[1.0, 2.0]])


@pytest.mark.parametrize("dtype, code", [("torch.float32", _capi.NND_DTYPE_FLOAT32), ("torch.float16", _capi.NND_DTYPE_FLOAT16),
                                         ("torch.bfloat16", _capi.NND_DTYPE_BFLOAT16), ("torch.float64", _capi.NND_DTYPE_FLOAT64),
                                         ("float16", _capi.NND_DTYPE_FLOAT16)])
def test_dtype_table(dtype, code):
    a = StubArray((5, 7), dtype, device=2)
    out, got, ordinal = N._check_device_array(a)
    assert out is a and got == code and ordinal == 2
    assert (_capi.NND_DTYPE_FLOAT32, _capi.NND_DTYPE_FLOAT16, _capi.NND_DTYPE_BFLOAT16, _capi.NND_DTYPE_FLOAT64) == (0, 1, 2, 3)


@pytest.mark.parametrize("dtype", ["torch.int32", "torch.int64", "torch.uint8", "torch.bool", "torch.complex64", "torch.float8_e4m3fn"])
def test_other_dtypes_raise_type_error_naming_the_dtype(dtype):
    with pytest.raises(TypeError, match=r"float32, float16, bfloat16 or float64 \(data has dtype %s\)" % dtype.replace(".", r"\.")):
        N._check_device_array(StubArray((5, 7), dtype))
    with pytest.raises(TypeError, match="query_data has dtype"):
        N._check_device_array(StubArray((5, 7), dtype), what="query_data")


@pytest.mark.parametrize("shape", [(5,), (5, 7, 2), ()])
def test_not_two_dimensional_raises_value_error(shape):
    with pytest.raises(ValueError, match="Expected 2D array, got %dD" % len(shape)):
        N._check_device_array(StubArray(shape))


def test_contiguity():
    a = StubArray((5, 7), contiguous=False, device=1)
    out, _, ordinal = N._check_device_array(a)
    assert out is not a and out.made_contiguous == 1 and out.is_contiguous() and ordinal == 1 and out.shape == (5, 7)
    b = StubArray((5, 7))
    assert N._check_device_array(b)[0] is b  # kept by reference, no copy


def test_device_argument():
    a = StubArray((5, 7), device=0)
    assert N._check_device_array(a, device=0)[2] == 0
    with pytest.raises(ValueError, match="device=1, but data is on device 0"):
        N._check_device_array(a, device=1)
    on3 = StubArray((5, 7), device=3)
    assert N._check_device_array(on3, device=0)[2] == 3  # 0 is the default: the index runs where the data is
    assert N._check_device_array(on3, device=3)[2] == 3
    with pytest.raises(ValueError, match="device=2, but data is on device 3"):
        N._check_device_array(on3, device=2)
    unindexed = StubArray((5, 7))
    unindexed.device.index = None  # torch.device("cuda")
    assert N._check_device_array(unindexed)[2] == 0


def test_constructor_rejects_before_any_device_work():
    """dtype, shape and device mismatch are found by the validator: no library call, no torch (the stub has no memory behind it)."""
    with pytest.raises(TypeError, match="torch.int32"):
        N.NNDescent(StubArray((50, 4), "torch.int32"), n_neighbors=5)
    with pytest.raises(ValueError, match="device=1, but data is on device 0"):
        N.NNDescent(StubArray((50, 4)), n_neighbors=5, device=1)


def test_every_metric_has_a_device_correction():
    kinds = {name: m.device_kind for name, m in N._METRICS.items()}
    assert kinds == {"euclidean": _capi.NND_CORRECT_SQRT, "l2": _capi.NND_CORRECT_SQRT, "sqeuclidean": _capi.NND_CORRECT_COPY,
                     "cosine": _capi.NND_CORRECT_ALT_COSINE, "dot": _capi.NND_CORRECT_ALT_COSINE,
                     "inner_product": _capi.NND_CORRECT_ALT_INNER_PRODUCT, "correlation": _capi.NND_CORRECT_COPY,
                     "hellinger": _capi.NND_CORRECT_ALT_HELLINGER, "proxy_inner_product": _capi.NND_CORRECT_COPY}


def test_importing_the_package_does_not_import_torch():
    code = "import sys; import pynndescent_amd; import pynndescent_amd.nndescent; sys.exit(1 if 'torch' in sys.modules else 0)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, "torch was imported by `import pynndescent_amd`\n" + r.stderr
