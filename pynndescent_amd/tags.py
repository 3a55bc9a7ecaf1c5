"""Tag and mask words of the per-query filters (DESIGN.md "Per-query filters"): 64 bits per row (``tags``) and per query
(``masks``); row r may be returned to query i iff ``tags[r] & masks[i] != 0``.  What this module holds is the one rule for what
such an array may be, and its two homes: a numpy ``uint64`` array on the host, an ``int64`` tensor on the device (torch has no
unsigned 64-bit arithmetic; the bit pattern is what counts, bit 63 is a tag like any other).
"""
import numpy as np

from . import device_arrays
from .device_arrays import _dtype_name, _is_device_array


def check_words(words, count, device, what, per):
    """``words`` as ``(values, on_device)`` -- a contiguous numpy uint64 array or a contiguous int64 tensor, where the caller put
    it -- or ``ValueError``: not 1-D, not ``count`` entries (one per ``per``), a dtype other than uint64 / int64 (a tensor: int64), a
    tensor on another device than ``device``."""
    if _is_device_array(words):
        if (getattr(words.device, "index", None) or 0) != int(device):
            raise ValueError("%s is on device %d, the index on device %d" % (what, words.device.index or 0, int(device)))
        if _dtype_name(words) != "int64":
            raise ValueError("%s must be an int64 tensor, 64 tag bits per %s (got dtype %s)" % (what, per, _dtype_name(words)))
        if words.dim() != 1 or int(words.shape[0]) != int(count):
            raise ValueError("%s must be 1-D with one entry per %s (%d), got shape %s" % (what, per, count, tuple(words.shape)))
        return words.contiguous(), True
    a = np.asarray(words)
    if a.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)):
        raise ValueError("%s must be uint64 or int64, 64 tag bits per %s (got dtype %s)" % (what, per, a.dtype))
    if a.ndim != 1 or a.shape[0] != int(count):
        raise ValueError("%s must be 1-D with one entry per %s (%d), got shape %s" % (what, per, count, a.shape))
    return np.ascontiguousarray(a).view(np.uint64), False


def to_host(values, on_device):
    """The words as a numpy uint64 array."""
    if on_device:
        return np.ascontiguousarray(values.cpu().numpy()).view(np.uint64)
    return values


def to_device(values, on_device, where):
    """The words as an int64 tensor on the torch device ``where``."""
    if on_device:
        return values
    return device_arrays._torch().from_numpy(np.ascontiguousarray(values).view(np.int64)).to(where)
