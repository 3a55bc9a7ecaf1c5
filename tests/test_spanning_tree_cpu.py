"""What ``spanning_tree`` refuses before any device work."""
import numpy as np
import pytest

from pynndescent_amd import spanning_tree


@pytest.mark.parametrize("metric, k, rows, error", [
    ("hellinger", 3, 20, NotImplementedError),  # a device metric outside the tree's list
    ("manhattan", 3, 20, NotImplementedError),  # a metric of the reference alone
    ("euclidean", 257, 300, NotImplementedError),
    ("euclidean", 3, 19, ValueError),           # data rows and list rows differ
])
def test_refusals(metric, k, rows, error):
    ids = np.zeros((300 if k > 256 else 20, k), np.int32)
    with pytest.raises(error):
        spanning_tree(np.zeros((rows, 4), np.float32), ids, np.zeros(ids.shape, np.float32), metric=metric)
