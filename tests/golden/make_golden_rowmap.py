"""Generate tests/golden/metric_rowmap.npz for spearmanr / haversine from the REFERENCE ITSELF.

Run in the build container only (needs the reference tree, loaded un-jitted through ``oracle/ref_t0.py`` exactly as
``make_golden_metrics.py`` does):

    python tests/golden/make_golden_rowmap.py

Contents: ``rank_x`` (300 x 8 float32 rows with ties: values rounded to one decimal, some rows drawn from six integers, a
constant row, a row of -0.0 / 0.0) and ``sphere_x`` (300 x 2 float32 (lat, lon) rows in radians: global, a regional cluster, both
poles, lon = +-pi); ``pairs`` (2000 x 2 row ids, drawn once for both point sets, the first 300 of them (i, i)); the reference's
``spearmanr`` / ``haversine`` of every pair (float64, evaluated on the float64 view of the float32 rows); and the brute-force 10 nearest neighbours of every row under the
reference's two functions (ids by (distance, id), and the distances).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_t0  # noqa: E402
from tests import rowmap_util as RU  # noqa: E402

N, K, N_PAIRS = 300, 10, 2000


def rank_rows():
    x = RU.decimal_rows(N, 8, seed=5)
    x[:40] = RU.tied_rows(40, 8, seed=6)  # (its rows 1 and 2: the constant row and the row of signed zeros)
    x[41] = x[40]  # a duplicate pair
    return x


def sphere_rows():
    x = RU.latlon_rows(N, seed=7)
    x[100:200] = RU.latlon_rows(100, seed=8, region=(0.7, 2.1, 0.05))
    x[0], x[1] = (np.pi / 2, 0.3), (-np.pi / 2, -1.0)
    x[2], x[3] = (0.2, np.pi), (0.2, -np.pi)
    x[5] = x[4]  # a duplicate pair
    return x.astype(np.float32)


def all_pairs(fn, x):
    out = np.empty((x.shape[0], x.shape[0]), np.float64)
    x64 = x.astype(np.float64)  # the float32 values, the arithmetic in float64 (the un-jitted stub would keep float32 under NumPy 2)
    for i in range(x.shape[0]):
        for j in range(x.shape[0]):
            out[i, j] = fn(x64[i], x64[j])
    return out


def main():
    ref_t0.load_reference()
    from pynndescent import distances as D

    rs = np.random.RandomState(9)
    pairs = rs.randint(0, N, size=(N_PAIRS, 2)).astype(np.int32)
    pairs[:N] = np.arange(N, dtype=np.int32)[:, None]
    out = dict(rank_x=rank_rows(), sphere_x=sphere_rows(), pairs=pairs)
    for name, fn, key in (("spearmanr", D.spearmanr, "rank_x"), ("haversine", D.haversine, "sphere_x")):
        x = out[key]
        dm = all_pairs(fn, x)
        out[name + "_pairs"] = dm[pairs[:, 0], pairs[:, 1]]
        order = np.lexsort((np.broadcast_to(np.arange(N), dm.shape), dm), axis=1)[:, :K]
        out[name + "_knn_idx"] = order.astype(np.int32)
        out[name + "_knn_dist"] = np.take_along_axis(dm, order, 1)
        print("%s: pairs in [%.3g, %.3g], self distance max %.3g" % (name, out[name + "_pairs"].min(), out[name + "_pairs"].max(),
                                                                     np.abs(np.diag(dm)).max()))
    path = os.path.join(HERE, "metric_rowmap.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
