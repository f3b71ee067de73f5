"""Nearest centres of every row: the DEFINITION of include/snowgpu.h (snowgpu_nearest_centres_device) restated as a brute-force NumPy
program -- the full distance matrix of a frame's usable rows against its usable centres in the rows' dtype, every subtraction, product and
sum a ufunc call of its own, np.lexsort on (centre number, d), the float64 weight chain -- and the shared inputs of
tests/test_nn_reference.py and tests/test_gpu_nearest.py with their expected outputs.  grid() restates the choice of the cells
(csrc/sg_nn.h: sg_nn_make_grid) so that the inputs can be held to conditions on cells.  Nothing here imports the package's native code."""
import functools
import math

import numpy as np

from ball_reference import centre_usable                                             # the usable test of a centre is the ball query's
from fps_reference import BOUND, DTYPES, RANGE, SECOND_RANGE, STEP, usable_rows      # ... of a row the keypoint stage's

EMPTY = -1
SENSOR = 120.0
PER_CELL, MIN_CELLS, MAX_CELLS = 2, 16, 2048
MAX_K = 8
PAIRS = 4_000_000          # (row, centre) pairs of one block of the distance matrix


def distances(rows_xyz, centres_xyz):
    """d[i, j] = ((dx dx) + (dy dy)) + (dz dz) in the arrays' dtype, every operation a ufunc call."""
    dx, dy, dz = (np.subtract(rows_xyz[:, None, j], centres_xyz[None, :, j]) for j in range(3))
    return np.add(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(dz, dz))


def weights(index, dist2):
    """The float64 chain of the definition: u = 1 / (sqrt(d) + 1e-8), n = ((u_0 + u_1) + u_2) + ..., T(u / n); 0 where the index is -1."""
    filled = index >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(filled, np.divide(1.0, np.add(np.sqrt(dist2.astype(np.float64)), 1e-8)), 0.0)
        n = u[:, 0].copy()
        for j in range(1, u.shape[1]):
            n = np.add(n, u[:, j])
        w = np.where(filled, np.divide(u, n[:, None]), 0.0)
    return w.astype(dist2.dtype)


def nearest(rows, centres, k=3, point_cloud_range=None, keep=None, offsets=None):
    """index (N, k), dist2 (N, k) and weight (N, k) of the definition, as a dict of NumPy arrays."""
    rows, centres = np.asarray(rows), np.asarray(centres)
    assert centres.dtype == rows.dtype and centres.ndim == 3 and 1 <= k <= MAX_K
    offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    assert centres.shape[0] == len(offsets) - 1
    ok, cok = usable_rows(rows, point_cloud_range, keep), centre_usable(centres)
    index = np.full((len(rows), k), EMPTY, np.int32)
    dist2 = np.full((len(rows), k), np.inf, rows.dtype)
    for f in range(len(offsets) - 1):
        u = int(offsets[f]) + np.flatnonzero(ok[offsets[f]:offsets[f + 1]])
        cu = np.flatnonzero(cok[f])
        if not len(u) or not len(cu):
            continue
        cxyz, n = np.ascontiguousarray(centres[f, cu, :3]), min(k, len(cu))
        step = max(1, PAIRS // len(cu))
        for a in range(0, len(u), step):
            part = u[a:a + step]
            d = distances(np.ascontiguousarray(rows[part, :3]), cxyz)
            order = np.lexsort((np.broadcast_to(cu, d.shape), d), axis=-1)[:, :n]          # by d, then by centre number
            index[part, :n] = cu[order]
            dist2[part, :n] = np.take_along_axis(d, order, axis=1)
    return dict(index=index, dist2=dist2, weight=weights(index, dist2))


# ---- the cells (csrc/sg_nn.h) ---------------------------------------------------------------------------------------------------------------
def cell_budget(n_centres):
    return min(max(-(-int(n_centres) // PER_CELL), MIN_CELLS), MAX_CELLS)


def grid(point_cloud_range, n_centres):
    """The grid sg_nn_make_grid lays out: x0, y0, edge, inv, nx, ny and the budget."""
    lo, hi = [-SENSOR, -SENSOR], [SENSOR, SENSOR]
    if point_cloud_range is not None:
        for j in range(2):
            if abs(point_cloud_range[j]) <= BOUND:
                lo[j] = float(point_cloud_range[j])
            if abs(point_cloud_range[3 + j]) <= BOUND:
                hi[j] = float(point_cloud_range[3 + j])
            if not lo[j] < hi[j]:
                hi[j] = lo[j] + 2 * SENSOR
    budget = cell_budget(n_centres)
    wx, wy = hi[0] - lo[0], hi[1] - lo[1]
    edge = math.sqrt(wx * wy / budget)
    while True:
        fx, fy = max(1.0, math.ceil(wx / edge)), max(1.0, math.ceil(wy / edge))
        if fx * fy <= budget:
            break
        edge *= 1.05
    return dict(x0=lo[0], y0=lo[1], edge=edge, inv=1.0 / edge, nx=int(fx), ny=int(fy), budget=budget)


def cells(g, xy):
    """(ix, iy) of points (n x 2, any dtype), clamped as the index functions clamp."""
    p = np.asarray(xy, np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        ix = np.clip(np.nan_to_num(np.floor((p[:, 0] - g["x0"]) * g["inv"]), nan=0.0), 0, g["nx"] - 1).astype(np.int64)
        iy = np.clip(np.nan_to_num(np.floor((p[:, 1] - g["y0"]) * g["inv"]), nan=0.0), 0, g["ny"] - 1).astype(np.int64)
    return ix, iy


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _columns(xyz, rng, dtype):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(xyz)
    return np.ascontiguousarray(np.column_stack((xyz, rng.integers(1, 255, n), rng.integers(0, 64, n))).astype(dtype))


def lattice(rng, n, box):
    """n points whose coordinates are random multiples of STEP in box = (x0, y0, z0, x1, y1, z1), float64."""
    lo, hi = np.asarray(box[:3], np.float64), np.asarray(box[3:], np.float64)
    return lo + rng.integers(0, np.maximum(((hi - lo) / STEP).astype(np.int64), 1), (n, 3)).astype(np.float64) * STEP


CONSTRUCTED_RANGE = (0.0, -8.0, -2.0, 16.0, 8.0, 2.0)
CONSTRUCTED_K = 32          # 16 cells of 4 m: every multiple of 4 is a cell boundary
# the frames of the constructed batch, by their number
FRAME = {"tie": 0, "edge": 1, "boundaries": 2, "duplicates": 3, "no_centre": 4, "one_centre": 5, "two_centres": 6, "three_centres": 7,
         "no_row": 8, "one_row": 9, "dtype": 10}


def constructed_case(dtype):
    """Eleven frames under CONSTRUCTED_RANGE, K = 32 centres each (those a frame does not need are NaN: not usable), k = 3; see FRAME.
    Returns rows, offsets, keep, centres and `special`: the batch rows that the conditions of tests/test_nn_reference.py speak about."""
    rng = np.random.default_rng(23)
    t = np.dtype(dtype).type
    box = CONSTRUCTED_RANGE
    frames, cents, special = [], [], {}

    def frame(first_rows, n_random, centres):
        c = np.full((CONSTRUCTED_K, 3), np.nan)
        for number, xyz in centres.items():
            c[number] = xyz
        cents.append(c)
        frames.append(np.concatenate((np.asarray(first_rows, np.float64).reshape(-1, 3), lattice(rng, n_random, box))))

    # tie: centre 5 in the row's own cell and centre 0 two rings out, both at d = 64 exactly; everything else is farther
    frame([(5.0, 1.0, 0.0)], 200, {0: (13.0, 1.0, 0.0), 5: (5.0, 1.0, 8.0), 2: (1.0, -7.0, 0.0), 3: (15.0, 7.0, 1.0)})
    # edge: the row an ulp inside x = 8; its nearest centre, 0, a quarter of a metre across that edge; the decoy, 1, 3 m away in its cell
    inside = float(np.nextafter(t(8.0), t(0.0)))
    frame([(inside, -6.0, 0.0)], 100, {0: (8.25, -6.0, 0.0), 1: (5.0, -6.0, 0.0), 2: (12.0, 2.0, 0.0), 3: (2.0, 6.0, 1.0)})
    # boundaries: centres on cell boundaries and on the four corners of the domain, and eight anywhere
    on = {0: (4.0, -4.0, 0.0), 1: (8.0, 0.0, 0.0), 2: (12.0, 4.0, 0.0), 3: (4.0, 4.0, 0.5), 4: (0.0, -8.0, 0.0), 5: (16.0, 8.0, 0.0), 6: (0.0, 8.0, 0.0),
          7: (16.0, -8.0, 0.0)}
    on.update({8 + i: p for i, p in enumerate(lattice(rng, 8, box))})
    frame([(8.0, 0.0, 0.0), (4.0, -4.0, 1.0), (12.0, 0.0, -1.0)], 300, on)
    # duplicates: centres 3, 7 and 9 are one point, and a row coincides with it; centres 0 and 1 are one point too
    dup = {3: (3.0, 3.0, 0.5), 7: (3.0, 3.0, 0.5), 9: (3.0, 3.0, 0.5), 0: (10.0, -2.0, 0.0), 1: (10.0, -2.0, 0.0)}
    dup.update({12 + i: p for i, p in enumerate(lattice(rng, 10, box))})
    frame([(3.0, 3.0, 0.5), (10.0, -2.0, 0.25)], 100, dup)
    # frames with 0, 1, k - 1 = 2 and k = 3 usable centres (the others NaN; in the first, every other kind of unusable centre)
    frame([], 20, {0: (np.inf, 0.0, 0.0), 1: (0.0, -np.inf, 0.0), 2: (2e6, 0.0, 0.0), 3: (1.0, 1.0, -1.5e6), 4: (np.nan, 1.0, 1.0)})
    frame([], 20, {17: (7.0, 7.0, 0.0)})
    frame([], 20, {4: (7.0, -7.0, 0.0), 30: (9.0, 1.0, 1.0)})
    frame([], 20, {0: (1.0, 1.0, 0.0), 1: (15.0, -7.0, 0.0), 31: (8.0, 0.0, -1.0)})
    # frames of 0 rows and of 1 row
    frame([], 0, dict(enumerate(lattice(rng, CONSTRUCTED_K, box))))
    frame([], 1, dict(enumerate(lattice(rng, CONSTRUCTED_K, box))))
    # dtype: centre 0 at distance 1 + 1e-9 (float32 rounds it to 1: a tie that the smaller number wins), centre 1 at distance 1;
    # and rows that are not usable: NaN, beyond 1e6, on the upper bound of the range, below its lower bound
    frame([(2.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (1.0, 1.0, 2e6), (1.0, 8.0, 0.0), (-STEP, 0.0, 0.0), (1.0, 1.0, np.inf)], 30,
          {0: (2.0, 1.0 + 1e-9, 0.0), 1: (3.0, 0.0, 0.0), 2: (10.0, 5.0, 0.0)})
    offsets = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
    for name in ("tie", "edge", "duplicates", "dtype"):
        special[name] = int(offsets[FRAME[name]])
    keep = np.ones(int(offsets[-1]), bool)
    keep[rng.choice(np.arange(offsets[2] + 3, offsets[3]), 40, replace=False)] = False          # absent rows in the boundaries frame
    keep[offsets[FRAME["duplicates"]] + 1] = False
    return _columns(np.concatenate(frames), rng, dtype), offsets, keep, np.ascontiguousarray(np.stack(cents).astype(dtype)), special


def batch_case(dtype):
    """Frames of 0, 1, 37, 300 and 1500 rows under RANGE, 64 centres each: six of them rows of the frame where it has that many."""
    sizes = (0, 1, 37, 300, 1500)
    offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    rng = np.random.default_rng(31)
    rows = _columns(lattice(rng, int(offsets[-1]), RANGE), rng, dtype)
    centres = _columns(lattice(rng, 5 * 64, RANGE), rng, dtype)[:, :4].reshape(5, 64, 4).copy()
    for f, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        take = rng.choice(np.arange(a, b), min(6, b - a), replace=False)
        centres[f, :len(take)] = rows[take, :4]
    return rows, offsets, np.ascontiguousarray(centres)


def _around(rng, centre, n, reach):
    return np.asarray(centre, np.float64) + rng.integers(-int(reach / STEP), int(reach / STEP) + 1, (n, 3)).astype(np.float64) * STEP


BEYOND_SPOTS = ((620.0, 0.0, 0.0), (-130.0, 125.0, 1.0), (0.0, 0.0, 0.0), (119.75, -119.75, 0.0), (-600.0, -600.0, 2.0))


def beyond_case(dtype):
    """No range: the grid covers |x|, |y| <= 120 m.  Rows and centres in clusters 500 m beyond it on x, beyond its corners and at the
    origin, and centres that are not usable."""
    rng = np.random.default_rng(51)
    xyz = np.concatenate([_around(rng, s, 60, 2.0) for s in BEYOND_SPOTS])
    xyz = xyz[rng.permutation(len(xyz))]
    centres = np.concatenate([_around(rng, s, 4, 1.0) for s in BEYOND_SPOTS] + [[(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (2e6, 0.0, 0.0), (620.0, 0.0, -1.5e6)]])
    return _columns(xyz, rng, dtype), np.ascontiguousarray(centres.astype(dtype))[None]


def corner_case(dtype):
    """All 40 centres in the lowest corner cell of RANGE, 500 rows in the opposite corner and 20 anywhere: far rows."""
    rng = np.random.default_rng(57)
    centres = lattice(rng, 40, (0.0, -20.0, -1.0, 5.0, -15.0, 1.0))
    xyz = np.concatenate((lattice(rng, 500, (35.0, 15.0, -1.0, 40.0, 20.0, 1.0)), lattice(rng, 20, RANGE)))
    return _columns(xyz, rng, dtype), np.ascontiguousarray(centres.astype(dtype))[None]


def cluster_case(dtype):
    """5000 centres within 5 cm of one point -- one cell of the largest grid -- in any order, and 2000 rows anywhere under RANGE."""
    rng = np.random.default_rng(61)
    near = np.stack(np.meshgrid(np.arange(-24, 25), np.arange(-24, 25), np.arange(-2, 3), indexing="ij"), -1).reshape(-1, 3)
    near = near[rng.permutation(len(near))[:5000]].astype(np.float64) * STEP + (20.0, 0.0, 0.0)
    xyz = np.concatenate((lattice(rng, 1990, RANGE), near[:10] + (0.0, 0.0, STEP / 2)))
    return _columns(xyz, rng, dtype), np.ascontiguousarray(near.astype(dtype))[None]


def sized_case(n_centres, dtype, n_rows=3000):
    """n_rows rows and n_centres centres anywhere under RANGE, one frame."""
    rng = np.random.default_rng(70 + n_centres)
    return _columns(lattice(rng, n_rows, RANGE), rng, dtype), np.ascontiguousarray(lattice(rng, n_centres, RANGE).astype(dtype))[None]


SIZES = (1, 2, 3, 64, 4096)
CASES = ("constructed", "batch", "beyond", "corner", "cluster")


@functools.lru_cache(maxsize=None)
def case(name, dtype="float32"):
    """(rows N x 5 read-only, offsets, keep or None, centres F x K x Cq, range or None) of a shared input; "sized<K>" is sized_case(K)."""
    offsets = keep = None
    if name == "constructed":
        (rows, offsets, keep, centres, _), rng = constructed_case(dtype), CONSTRUCTED_RANGE
    elif name == "batch":
        (rows, offsets, centres), rng = batch_case(dtype), RANGE
    elif name == "beyond":
        (rows, centres), rng = beyond_case(dtype), None
    elif name == "corner":
        (rows, centres), rng = corner_case(dtype), RANGE
    elif name == "cluster":
        (rows, centres), rng = cluster_case(dtype), RANGE
    elif name.startswith("sized"):
        (rows, centres), rng = sized_case(int(name[5:]), dtype), RANGE
    else:
        raise KeyError(name)
    offsets = np.array([0, len(rows)], np.int64) if offsets is None else offsets
    for a in (rows, centres) + ((keep,) if keep is not None else ()):
        a.setflags(write=False)
    return rows, offsets, keep, centres, rng


def special(dtype="float32"):
    return constructed_case(dtype)[4]


@functools.lru_cache(maxsize=None)
def _first_eight(name, dtype):
    rows, offsets, keep, centres, rng = case(name, dtype)
    return nearest(rows, centres, MAX_K, rng, keep, offsets)


@functools.lru_cache(maxsize=None)
def expected(name, dtype="float32", k=3):
    """nearest() of a shared input for k neighbours: the first k columns of the brute-force order, computed once, and their weights."""
    e = _first_eight(name, dtype)
    index, dist2 = np.ascontiguousarray(e["index"][:, :k]), np.ascontiguousarray(e["dist2"][:, :k])
    return _frozen(dict(index=index, dist2=dist2, weight=weights(index, dist2)))


def _frozen(out):
    for a in out.values():
        a.setflags(write=False)
    return out
