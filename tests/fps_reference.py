"""Farthest point sampling: the DEFINITION of include/snowgpu.h (snowgpu_fps_device) restated as a sequential NumPy program -- arrays of the
rows' dtype, every subtraction, product and sum a ufunc call of its own, np.minimum for the running minima and np.argmax, which returns
the first of equal maxima -- and the shared inputs of tests/test_fps_reference.py and tests/test_gpu_fps.py with their expected outputs.
Nothing here imports the package's native code."""
import functools

import numpy as np

DTYPES = ("float32", "float64")
BOUND = 1e6
RANGE = (0.0, -20.0, -2.0, 40.0, 20.0, 2.0)
SECOND_RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
STEP = 2.0 ** -10          # every generated coordinate is a multiple of it: no non-zero difference below 2^-20, no subnormal product


def usable_rows(rows, point_cloud_range=None, keep=None):
    """The usable test of the definition for every row, without the frames."""
    p = np.asarray(rows)[:, :3].astype(np.float64)          # (exact for float32)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(p) <= BOUND).all(axis=1)
        if point_cloud_range is not None:
            r = np.asarray(point_cloud_range, np.float64)
            ok &= ((r[:3] <= p) & (p < r[3:])).all(axis=1)
    if keep is not None:
        ok &= np.asarray(keep) != 0
    return ok


def walk(xyz, n_samples):
    """(positions K, dist K, ties K) of the walk over the m >= 1 rows of `xyz` (m x 3, the rows' dtype): ties[j] = the rows that attained
    the maximum of round j where it was positive (0 where it was 0; ties[0] = 0)."""
    x, y, z = (np.ascontiguousarray(xyz[:, j]) for j in range(3))
    dt = xyz.dtype.type
    t = np.full(len(x), np.inf, xyz.dtype)
    pos, dist, ties = np.zeros(n_samples, np.int64), np.zeros(n_samples, xyz.dtype), np.zeros(n_samples, np.int64)
    dist[0] = dt(np.inf)
    s = 0
    for j in range(1, n_samples):
        dx, dy, dz = np.subtract(x, x[s]), np.subtract(y, y[s]), np.subtract(z, z[s])
        d = np.add(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(dz, dz))
        t = np.minimum(t, d)
        s = int(np.argmax(t))
        pos[j], dist[j] = s, t[s]
        ties[j] = int((t == t[s]).sum()) if t[s] > 0 else 0
    return pos, dist, ties


def fps(rows, n_samples, point_cloud_range=None, num_features=4, keep=None, offsets=None):
    """The four outputs of the definition in their static shapes, and `ties` per frame and round, as a dict of NumPy arrays."""
    rows = np.asarray(rows)
    offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    F, K, C = len(offsets) - 1, int(n_samples), int(num_features)
    ok = usable_rows(rows, point_cloud_range, keep)
    index = np.full((F, K), -1, np.int32)
    points = np.zeros((F, K, C), rows.dtype)
    dist = np.full((F, K), -1, rows.dtype)
    usable = np.zeros(F, np.int32)
    ties = np.zeros((F, K), np.int64)
    for f in range(F):
        u = int(offsets[f]) + np.flatnonzero(ok[offsets[f]:offsets[f + 1]])
        usable[f] = len(u)
        if not len(u):
            continue
        pos, dist[f], ties[f] = walk(np.ascontiguousarray(rows[u, :3]), K)
        index[f] = u[pos]
        points[f] = rows[index[f], :C]
    return dict(index=index, points=points, dist=dist, usable=usable, ties=ties)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _columns(xyz, rng, dtype):
    """N x 5 rows of `dtype` from N x 3 coordinates: an intensity and a channel beside them."""
    n = len(xyz)
    return np.ascontiguousarray(np.column_stack((xyz, rng.integers(1, 255, n), rng.integers(0, 64, n))).astype(dtype))


def cloud(n_rows, dtype="float32", seed=0, span=40.0):
    """n_rows rows whose coordinates are random multiples of STEP in [0, span) x [-span / 2, span / 2) x [-2, 2): all usable under RANGE
    for span = 40."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, (int(span / STEP), int(span / STEP), int(4.0 / STEP)), (n_rows, 3)).astype(np.float64) * STEP
    q[:, 1] -= span / 2
    q[:, 2] -= 2.0
    return _columns(q, rng, dtype)


def lattice_case(dtype):
    """The 16 x 16 x 4 points of a grid of step 0.25 and 200 of them once more, shuffled: distances are exact and many are equal."""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(4), indexing="ij"), -1).reshape(-1, 3) * 0.25
    g = np.concatenate((g, g[rng.choice(len(g), 200, replace=False)]))
    return _columns(g[rng.permutation(len(g))], rng, dtype)


def constructed_case(dtype):
    """3000 rows inside RANGE; then, 24 rows each: one coordinate NaN, one beyond 1e6, one below lo, one ON hi, one ON lo (usable); 150
    more rows are masked.  (rows, keep, kinds): kinds[i] names what was done to row i."""
    rng = np.random.default_rng(5)
    rows = cloud(3000, "float64", seed=6)
    kinds = np.full(3000, "plain", object)
    lo, hi = np.array(RANGE[:3]), np.array(RANGE[3:])
    picks = rng.choice(3000, 5 * 24 + 150, replace=False)
    for n, kind in enumerate(("nan", "far", "below", "on_hi", "on_lo")):
        for i in picks[24 * n:24 * n + 24]:
            j = int(rng.integers(0, 3))
            rows[i, j] = {"nan": np.nan, "far": (1e6 + 1.0) * (1 if i % 2 else -1), "below": lo[j] - STEP, "on_hi": hi[j], "on_lo": lo[j]}[kind]
            kinds[i] = kind
    keep = np.ones(3000, bool)
    keep[picks[120:]] = False
    kinds[picks[120:]] = "masked"
    return np.ascontiguousarray(rows.astype(dtype)), keep, kinds


def fewer_case(m, dtype):
    """60 rows of which m are usable (the others NaN), no two alike."""
    rows = cloud(60, dtype, seed=40 + m).copy()
    bad = np.random.default_rng(m).permutation(60)[m:]
    rows[bad, 1] = np.nan
    return rows


def batch_case(dtype):
    """Frames of 6000, 0, 1500 and 300 rows: a cloud, an empty frame, the cloud's rows 2000 .. 3499 once more (the same coordinates in
    two frames) and a frame that the mask takes away whole.  (rows, offsets, keep)"""
    pc = cloud(6000, dtype, seed=3)
    rows = np.ascontiguousarray(np.concatenate((pc, pc[2000:3500], pc[100:400])))
    offsets = np.array([0, 6000, 6000, 7500, 7800], np.int64)
    keep = np.random.default_rng(21).random(7800) < 0.8
    keep[7500:] = False
    return rows, offsets, keep


@functools.lru_cache(maxsize=None)
def case(name, dtype="float32"):
    """(rows N x 5 read-only, offsets, keep or None, (range or None, K)) of a shared input."""
    offsets = keep = None
    if name == "lattice":
        rows, setting = lattice_case(dtype), (None, 64)
    elif name == "constructed":
        rows, keep, _ = constructed_case(dtype)
        setting = (RANGE, 64)
    elif name in ("fewer37", "fewer1", "fewer0"):
        rows, setting = fewer_case(int(name[5:]), dtype), (RANGE, 64)
    elif name == "batch":
        rows, offsets, keep = batch_case(dtype)
        setting = (RANGE, 48)
    else:
        raise KeyError(name)
    offsets = np.array([0, len(rows)], np.int64) if offsets is None else offsets
    rows.setflags(write=False)
    return rows, offsets, keep, setting


CASES = ("lattice", "constructed", "fewer37", "fewer1", "fewer0", "batch")


@functools.lru_cache(maxsize=None)
def expected(name, dtype="float32", num_features=4, n_samples=None):
    """fps() of a shared input (its own K unless given), computed once."""
    rows, offsets, keep, (rng, K) = case(name, dtype)
    return _frozen(fps(rows, K if n_samples is None else n_samples, rng, num_features, keep, offsets))


@functools.lru_cache(maxsize=None)
def cloud_case(n_rows, dtype="float32", seed=0):
    rows = cloud(n_rows, dtype, seed)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def cloud_expected(n_rows, dtype, n_samples, seed=0):
    """fps() of cloud_case(n_rows, dtype, seed) as one frame under RANGE -- every row is usable --, computed once."""
    return _frozen(fps(cloud_case(n_rows, dtype, seed), n_samples, RANGE))


def _frozen(out):
    for a in out.values():
        a.setflags(write=False)
    return out
