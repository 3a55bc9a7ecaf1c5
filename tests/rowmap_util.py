"""numpy models of the two row maps (csrc/rowmap.hip) and float64 evaluations of the distances they serve -- spearmanr
(reference distances.py:1430-1480) and haversine (distances.py:503-521) -- plus the inputs the tests share.  Test helpers only."""
import numpy as np

from pynndescent_amd import linear_map
from tests import metric_util as MU


def model_ranks(x):
    """Average ranks of every row, float32: r_j = #{i : x_i < x_j} + (#{i : x_i == x_j} + 1) / 2, from the sorted row (two binary
    searches per element).  Exact: both counts are integers, the result a half-integer far below 2^24."""
    x = np.asarray(x, np.float32)
    out = np.empty(x.shape, np.float32)
    for i, row in enumerate(x):
        s = np.sort(row)
        lt, le = np.searchsorted(s, row, "left"), np.searchsorted(s, row, "right")
        out[i] = (lt + le + 1).astype(np.float32) * np.float32(0.5)
    return out


def model_ranks_counting(x):
    """The same ranks by the defining formula, all pairs compared (small rows only)."""
    x = np.asarray(x, np.float32)
    lt = (x[:, None, :] < x[:, :, None]).sum(-1)
    eq = (x[:, None, :] == x[:, :, None]).sum(-1)
    return (2 * lt + eq + 1).astype(np.float32) * np.float32(0.5)


def sphere_points(rows):
    """P(lat, lon) = (cos lat cos lon, cos lat sin lon, sin lat), float64, of (n, 2) rows."""
    rows = np.asarray(rows, np.float64)
    cl = np.cos(rows[:, 0])
    return np.stack([cl * np.cos(rows[:, 1]), cl * np.sin(rows[:, 1]), np.sin(rows[:, 0])], 1)


def sphere_shift(rows):
    """The shift an index of the float32 rows fixes: float32 of the float64 mean of P over the strided sample."""
    rows = np.asarray(rows, np.float32)
    return sphere_points(rows[linear_map.shift_rows(rows.shape[0])]).mean(0).astype(np.float32)


def model_sphere(rows, shift):
    """The sphere map: float32 of (P - shift) taken in float64, one rounding per component."""
    return (sphere_points(np.asarray(rows, np.float32)) - np.asarray(shift, np.float32).astype(np.float64)).astype(np.float32)


def haversine_of_chord2(s):
    """2 arcsin(min(1, sqrt(s) / 2)) in float64: the angle of a squared chord of the unit sphere."""
    return 2.0 * np.arcsin(np.minimum(1.0, np.sqrt(np.asarray(s, np.float64)) / 2.0))


def haversine64(a, b):
    """The haversine formula in float64 on the pairs (a[i], b[i]) of (lat, lon) rows."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    h = np.sin((a[..., 0] - b[..., 0]) / 2.0) ** 2 + np.cos(a[..., 0]) * np.cos(b[..., 0]) * np.sin((a[..., 1] - b[..., 1]) / 2.0) ** 2
    return 2.0 * np.arcsin(np.sqrt(np.minimum(1.0, h)))


def spearmanr64(a, b):
    """The float64 correlation distance of the model's rank rows, pair by pair."""
    return MU.alt_dist_pairs("correlation", model_ranks(a), model_ranks(b))[0]


def haversine_bound(theta, m_abs):
    """The derived error bound of a handed-out haversine distance (DESIGN.md "Row maps"): 4e-7 * M / cos(theta / 2) rad, M the
    largest component magnitude of the shifted rows."""
    return 4e-7 * float(m_abs) / np.cos(np.asarray(theta, np.float64) / 2.0)


def tied_rows(n, d, seed, levels=6):
    """(n, d) float32 rows drawn from ``levels`` integers (ties everywhere), row 1 constant, row 2 holding -0.0 and 0.0."""
    x = np.random.RandomState(seed).randint(-2, levels - 2, size=(n, d)).astype(np.float32)
    if n > 2:
        x[1] = 3.0
        x[2] = np.where(np.arange(d) % 2 == 0, np.float32(-0.0), np.float32(0.0))
        if d > 2:
            x[2, 2] = 1.0
    return x


def decimal_rows(n, d, seed):
    """(n, d) float32 clustered rows rounded to one decimal: ties inside a row, and duplicate-free enough to build on."""
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((12, d)) * 2.0
    x = centres[rs.randint(0, 12, n)] + rs.standard_normal((n, d))
    return np.round(x, 1).astype(np.float32)


def latlon_rows(n, seed, region=None):
    """(n, 2) float32 (lat, lon) rows in radians: uniform on the sphere, or within ``region`` = (lat0, lon0, radius) of a centre
    (a box in lat / lon)."""
    rs = np.random.RandomState(seed)
    if region is None:
        lat = np.arcsin(rs.uniform(-1.0, 1.0, n))
        lon = rs.uniform(-np.pi, np.pi, n)
    else:
        lat0, lon0, r = region
        lat = lat0 + rs.uniform(-r, r, n)
        lon = lon0 + rs.uniform(-r, r, n)
    return np.stack([lat, lon], 1).astype(np.float32)
