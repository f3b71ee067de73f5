"""Ball query: the DEFINITION of include/snowgpu.h (snowgpu_ball_query_device) restated as a brute-force NumPy program -- all usable rows
of a frame against every centre, arrays of the rows' dtype, every subtraction, product and sum a ufunc call of its own, the strict
comparison against the separately rounded squared radius -- and the shared inputs of tests/test_ball_reference.py and
tests/test_gpu_ball_query.py with their expected outputs.  grid() restates the choice of the cells (csrc/sg_ball.h: sg_ball_make_grid) so
that the inputs can be held to conditions on cells.  Nothing here imports the package's native code."""
import functools
import math

import numpy as np

from fps_reference import BOUND, DTYPES, RANGE, SECOND_RANGE, STEP, usable_rows      # the usable test is the keypoint stage's

EMPTY = -1
SENSOR = 120.0
MIN_CELLS, MAX_CELLS = 1024, 81920


def squared_radius(radius, dtype):
    t = np.dtype(dtype).type
    return np.multiply(t(radius), t(radius))


def centre_usable(centres):
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(centres)[..., :3].astype(np.float64)) <= BOUND).all(axis=-1)


def ball_query(rows, centres, radii, samples, point_cloud_range=None, num_features=4, keep=None, offsets=None):
    """index (F, K, S), count (F, K, R) and points (F, K, S, C) of the definition, as a dict of NumPy arrays."""
    rows, centres = np.asarray(rows), np.asarray(centres)
    assert centres.dtype == rows.dtype and centres.ndim == 3
    offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    radii, samples = list(np.atleast_1d(radii)), [int(s) for s in np.atleast_1d(samples)]
    F, K, R, S, C = len(offsets) - 1, centres.shape[1], len(radii), sum(samples), int(num_features)
    assert centres.shape[0] == F and len(samples) == R
    ok = usable_rows(rows, point_cloud_range, keep)
    cok = centre_usable(centres)
    index = np.full((F, K, S), EMPTY, np.int32)
    count = np.zeros((F, K, R), np.int32)
    points = np.zeros((F, K, S, C), rows.dtype)
    seg = np.concatenate(([0], np.cumsum(samples)))
    for f in range(F):
        u = int(offsets[f]) + np.flatnonzero(ok[offsets[f]:offsets[f + 1]])
        if not len(u):
            continue
        x, y, z = (np.ascontiguousarray(rows[u, j]) for j in range(3))
        for k in range(K):
            if not cok[f, k]:
                continue
            dx, dy, dz = np.subtract(x, centres[f, k, 0]), np.subtract(y, centres[f, k, 1]), np.subtract(z, centres[f, k, 2])
            d = np.add(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(dz, dz))
            for i in range(R):
                inside = u[np.less(d, squared_radius(radii[i], rows.dtype))]          # (ascending: u is)
                n = len(inside)
                count[f, k, i] = n
                if n:
                    first = inside[:samples[i]]
                    index[f, k, seg[i]:seg[i] + len(first)] = first
                    index[f, k, seg[i] + len(first):seg[i + 1]] = first[0]
    got = index >= 0
    points[got] = rows[index[got], :C]
    return dict(index=index, count=count, points=points)


# ---- the cells (csrc/sg_ball.h) --------------------------------------------------------------------------------------------------------------
def cell_budget(max_frame_rows):
    return min(max(4 * int(max_frame_rows), MIN_CELLS), MAX_CELLS)


def grid(point_cloud_range, radii, max_frame_rows):
    """The grid sg_ball_make_grid lays out: x0, y0, inv, nx, ny, and `wanted`: the cells at the edge of half the largest radius."""
    lo, hi = [-SENSOR, -SENSOR], [SENSOR, SENSOR]
    if point_cloud_range is not None:
        for j in range(2):
            if abs(point_cloud_range[j]) <= BOUND:
                lo[j] = float(point_cloud_range[j])
            if abs(point_cloud_range[3 + j]) <= BOUND:
                hi[j] = float(point_cloud_range[3 + j])
            if not lo[j] < hi[j]:
                hi[j] = lo[j] + 2 * SENSOR
    budget = cell_budget(max_frame_rows)
    edge, k = 0.5 * float(max(np.atleast_1d(radii))), 1.0
    wanted = None
    while True:
        fx, fy = math.floor((hi[0] - lo[0]) / (edge * k)) + 1.0, math.floor((hi[1] - lo[1]) / (edge * k)) + 1.0
        wanted = fx * fy if wanted is None else wanted
        if fx * fy <= budget:
            break
        k *= max(math.sqrt(fx * fy / budget), 1.05)
    return dict(x0=lo[0], y0=lo[1], inv=1.0 / (edge * k), nx=int(fx), ny=int(fy), wanted=wanted, budget=budget)


def cells(g, xy):
    """Cell numbers iy nx + ix of points (n x 2, any dtype), clamped as the index functions clamp."""
    p = np.asarray(xy, np.float64)
    ix = np.clip(np.floor((p[:, 0] - g["x0"]) * g["inv"]), 0, g["nx"] - 1).astype(np.int64)
    iy = np.clip(np.floor((p[:, 1] - g["y0"]) * g["inv"]), 0, g["ny"] - 1).astype(np.int64)
    return iy * g["nx"] + ix


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _columns(xyz, rng, dtype):
    n = len(xyz)
    return np.ascontiguousarray(np.column_stack((xyz, rng.integers(1, 255, n), rng.integers(0, 64, n))).astype(dtype))


def cloud(n_rows, dtype="float32", seed=0, span=10.0):
    """n_rows rows whose coordinates are random multiples of STEP in [0, span) x [-span / 2, span / 2) x [-1, 1)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, (int(span / STEP), int(span / STEP), int(2.0 / STEP)), (n_rows, 3)).astype(np.float64) * STEP
    q[:, 1] -= span / 2
    q[:, 2] -= 1.0
    return _columns(q, rng, dtype)


def _around(rng, centre, n, reach):
    """n distinct points on the STEP lattice within `reach` of `centre` (a lattice point itself)."""
    out = set()
    while len(out) < n:
        p = rng.integers(-int(reach / STEP), int(reach / STEP) + 1, 3)
        if 0 < (p * p).sum() * STEP * STEP < reach * reach:
            out.add(tuple(p.tolist()))
    return np.array(sorted(out), np.float64) * STEP + np.asarray(centre, np.float64)


CONSTRUCTED_RANGE = (0.0, -8.0, -2.0, 16.0, 8.0, 2.0)
CONSTRUCTED_PAIR = ((1.0,), (16,))
# what the centres of the constructed frame are for, by their number
ROLE = {"n0": 0, "n15": 1, "n16": 2, "n17": 3, "high_cells_first": 4, "low_cells_first": 5, "on_the_sphere": 6, "dtype": 7, "corner_lo": 8,
        "corner_hi": 9, "off_boundary": 10, "outside_range": 11}


def constructed_case(dtype):
    """One frame under CONSTRUCTED_RANGE, radius 1 (its square is exact), 16 samples, 24 centres 3 m apart; see ROLE.  The cell edge is
    0.5 m (33 x 33 cells, within the budget of the frame), so a ball spans some 25 cells and every integer coordinate is a cell boundary."""
    rng = np.random.default_rng(17)
    t = np.dtype(dtype).type
    spots = [(x, y, 0.0) for y in (-6.0, -3.0, 0.0, 3.0, 6.0) for x in (2.0, 5.0, 8.0, 11.0, 14.0)]
    centres = np.array(spots[:24], np.float64)
    centres[ROLE["corner_lo"]] = (0.0, -8.0, 0.0)
    centres[ROLE["corner_hi"]] = (16.0, 8.0, 0.0)
    centres[ROLE["off_boundary"]] = (11.25, -2.75, 0.125)
    centres[ROLE["outside_range"]] = (-0.25, 0.0, 0.0)
    g = grid(CONSTRUCTED_RANGE, CONSTRUCTED_PAIR[0], 400)
    parts = []
    for role, n in (("n15", 15), ("n16", 16), ("n17", 17)):
        parts.append(_around(rng, centres[ROLE[role]], n, 0.6))
    many = _around(rng, centres[ROLE["high_cells_first"]], 200, 0.95)
    parts.append(many[np.argsort(-cells(g, many[:, :2]), kind="stable")])          # the smallest indices in the highest-numbered cells
    some = _around(rng, centres[ROLE["low_cells_first"]], 70, 0.95)
    parts.append(some[np.argsort(cells(g, some[:, :2]), kind="stable")])           # ... in the lowest-numbered cells
    c = centres[ROLE["on_the_sphere"]]
    inside = float(np.nextafter(t(c[0] + 1.0), t(0)))                              # one ulp of the rows' dtype inside the sphere
    parts.append(np.array([(c[0] + 1.0, c[1], c[2]), (inside, c[1], c[2]), (c[0], c[1] + 1.0, c[2]), (c[0], c[1], c[2] - 1.0)]))
    c = centres[ROLE["dtype"]]
    parts.append(np.array([(c[0] + 1.0 - 1e-9, c[1], c[2])]))                      # inside in float64; float32 rounds it onto the sphere
    for role in ("corner_lo", "corner_hi", "off_boundary", "outside_range"):
        parts.append(_around(rng, centres[ROLE[role]], 12, 0.9))                   # (those beyond the range are not usable)
    for k in range(12, 24):
        parts.append(_around(rng, centres[k], int(rng.integers(1, 6)), 1.4))
    xyz = np.concatenate(parts)
    return _columns(xyz, rng, dtype), np.ascontiguousarray(centres.astype(dtype))[None]


def batch_case(dtype):
    """Frames of 0, 1, 37, 300 and 1500 rows of a dense cloud, 8 centres each: rows of the frame where it has that many, points beside."""
    sizes = (0, 1, 37, 300, 1500)
    offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    rows = cloud(int(offsets[-1]), dtype, seed=31, span=6.0)
    rng = np.random.default_rng(32)
    centres = cloud(5 * 8, dtype, seed=33, span=6.0)[:, :4].reshape(5, 8, 4).copy()
    for f, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        take = rng.choice(np.arange(a, b), min(6, b - a), replace=False)
        centres[f, :len(take)] = rows[take, :4]
    return rows, offsets, np.ascontiguousarray(centres)


def unusable_case(dtype):
    """50 rows, none usable: NaN, beyond 1e6, or outside RANGE."""
    rows = cloud(50, "float64", seed=41)
    rows[0::3, 0] = np.nan
    rows[1::3, 2] = 2e6
    rows[2::3, 1] = RANGE[4]
    return np.ascontiguousarray(rows.astype(dtype)), np.ascontiguousarray(rows[:6, :3].astype(dtype))[None]


def absent_case(dtype):
    """Two frames of 100 rows, the second made absent through the mask (and 20 rows of the first)."""
    rows = cloud(200, dtype, seed=43, span=4.0)
    keep = np.ones(200, bool)
    keep[100:] = False
    keep[np.random.default_rng(44).choice(100, 20, replace=False)] = False
    centres = np.stack((rows[:8, :3], rows[100:108, :3]))
    return rows, np.array([0, 100, 200], np.int64), keep, np.ascontiguousarray(centres)


def outside_case(dtype):
    """No range: the grid covers |x|, |y| <= 120 m.  Clusters 500 m beyond it on x, beyond its corner, and at the origin; centres among
    them, and centres that are not usable.  The cells wanted at an edge of 0.2 m are far above the budget."""
    rng = np.random.default_rng(51)
    spots = np.array([(620.0, 0.0, 0.0), (-130.0, 125.0, 1.0), (0.0, 0.0, 0.0), (119.75, -119.75, 0.0)])
    xyz = np.concatenate([_around(rng, s, 75, 0.5) for s in spots])
    xyz = xyz[rng.permutation(len(xyz))]
    centres = np.concatenate((spots, spots[:2] + (0.25, -0.125, 0.0), [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (2e6, 0.0, 0.0), (620.0, 0.0, -1.5e6)]))
    return _columns(xyz, rng, dtype), np.ascontiguousarray(centres.astype(dtype))[None]


def cluster_case(dtype):
    """5000 rows within 5 cm of one point -- one cell -- shuffled, and 40 rows within 0.3 m of another: the balls of n = 5000 and n = 40."""
    rng = np.random.default_rng(61)
    near = np.stack(np.meshgrid(np.arange(-24, 25), np.arange(-24, 25), np.arange(-2, 3), indexing="ij"), -1).reshape(-1, 3)
    near = near[rng.permutation(len(near))[:5000]].astype(np.float64) * STEP + (20.0, 0.0, 0.0)
    xyz = np.concatenate((near, _around(rng, (10.0, 5.0, 0.0), 39, 0.3), [(10.0, 5.0, 0.0)]))
    xyz = xyz[rng.permutation(len(xyz))]
    centres = np.array([(20.0, 0.0, 0.0), (10.0, 5.0, 0.0), (30.0, -5.0, 0.0)])
    return _columns(xyz, rng, dtype), np.ascontiguousarray(centres.astype(dtype))[None]


@functools.lru_cache(maxsize=None)
def case(name, dtype="float32"):
    """(rows N x 5 read-only, offsets, keep or None, centres F x K x Cq, (range or None, radii, samples)) of a shared input."""
    offsets = keep = None
    if name == "constructed":
        (rows, centres), setting = constructed_case(dtype), (CONSTRUCTED_RANGE,) + CONSTRUCTED_PAIR
    elif name == "batch":
        (rows, offsets, centres), setting = batch_case(dtype), (RANGE, (0.8,), (16,))
    elif name == "unusable":
        (rows, centres), setting = unusable_case(dtype), (RANGE, (0.8,), (16,))
    elif name == "absent":
        (rows, offsets, keep, centres), setting = absent_case(dtype), (None, (0.8,), (16,))
    elif name == "outside":
        (rows, centres), setting = outside_case(dtype), (None, (0.4,), (16,))
    elif name == "cluster":
        (rows, centres), setting = cluster_case(dtype), (RANGE, (0.5,), (16,))
    else:
        raise KeyError(name)
    offsets = np.array([0, len(rows)], np.int64) if offsets is None else offsets
    rows.setflags(write=False)
    centres.setflags(write=False)
    return rows, offsets, keep, centres, setting


CASES = ("constructed", "batch", "unusable", "absent", "outside", "cluster")


@functools.lru_cache(maxsize=None)
def expected(name, dtype="float32", num_features=4, radii=None, samples=None):
    """ball_query() of a shared input (its own pairs unless given), computed once."""
    rows, offsets, keep, centres, (rng, r, s) = case(name, dtype)
    return _frozen(ball_query(rows, centres, r if radii is None else radii, s if samples is None else samples, rng, num_features, keep, offsets))


def _frozen(out):
    for a in out.values():
        a.setflags(write=False)
    return out
