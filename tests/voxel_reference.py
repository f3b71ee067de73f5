"""Point-to-voxel grouping: the DEFINITION of include/snowgpu.h (snowgpu_voxelize_device) restated as a sequential NumPy walk over a
dict of open cells -- the cell of a row is a float64 subtraction, a true division and a floor, each a ufunc call of its own -- and the shared
inputs of tests/test_voxel_reference.py and tests/test_gpu_voxelize.py with their expected outputs.  Nothing here imports the package's
native code."""
import functools
import math

import numpy as np

from lidar_snow_sim_amd.synthetic import firing_order, synthetic_sweep

# (point_cloud_range, voxel_size, max_points T, max_voxels V)
SECOND = ((0.0, -40.0, -3.0, 70.4, 40.0, 1.0), (0.05, 0.05, 0.1), 5, 40000)          # SECOND / PV-RCNN on DENSE
PILLARS = ((0.0, -39.68, -3.0, 69.12, 39.68, 1.0), (0.16, 0.16, 4.0), 32, 16000)     # PointPillars
CONSTRUCTED = ((0.0, -20.0, -2.0, 40.0, 20.0, 2.0), (1.0, 1.0, 1.0), 8, 300)
FACES_SECOND = (SECOND[0], SECOND[1], 5, 2048)
SETTINGS = {"second": SECOND, "pillars": PILLARS, "constructed": CONSTRUCTED, "faces_second": FACES_SECOND}
DTYPES = ("float32", "float64")


def grid_dims(point_cloud_range, voxel_size):
    """(n_x, n_y, n_z): n_j = llround((hi_j - lo_j) / size_j) in float64 (half away from zero; the quotients are positive)."""
    r, s = np.asarray(point_cloud_range, np.float64), np.asarray(voxel_size, np.float64)
    return tuple(int(math.floor(float(q) + 0.5)) for q in np.divide(np.subtract(r[3:], r[:3]), s))


def cells(rows, point_cloud_range, voxel_size):
    """(usable without a mask, c): c[i] = (c_x, c_y, c_z) of row i as int64 (meaningless where the row is not usable)."""
    r, s = np.asarray(point_cloud_range, np.float64), np.asarray(voxel_size, np.float64)
    n = np.asarray(grid_dims(point_cloud_range, voxel_size), np.float64)
    p = np.asarray(rows)[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(np.divide(np.subtract(p, r[:3]), s))
        ok = np.isfinite(p).all(axis=1) & ((c >= 0.0) & (c < n)).all(axis=1)
    return ok, np.where(ok[:, None], c, 0.0).astype(np.int64)


def voxelize(rows, point_cloud_range, voxel_size, max_points, max_voxels, num_features=4, keep=None, offsets=None):
    """The five outputs of the definition in their static shapes, as a dict of NumPy arrays."""
    rows = np.asarray(rows)
    n_total = rows.shape[0]
    offsets = np.array([0, n_total], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    n_frames, T, V, C = len(offsets) - 1, int(max_points), int(max_voxels), int(num_features)
    ok, c = cells(rows, point_cloud_range, voxel_size)
    if keep is not None:
        ok = ok & (np.asarray(keep) != 0)
    voxels = np.zeros((n_frames * V, T, C), rows.dtype)
    coords = np.full((n_frames * V, 4), -1, np.int32)
    num = np.zeros(n_frames * V, np.int32)
    voxel_offsets = np.zeros(n_frames + 1, np.int32)
    voxel_of = np.full(n_total, -1, np.int32)
    total = np.zeros(n_frames * V, np.int64)          # rows of every voxel, stored or not
    for f in range(n_frames):
        base = int(voxel_offsets[f])
        opened = {}
        for i in range(int(offsets[f]), int(offsets[f + 1])):
            if not ok[i]:
                continue
            cell = (int(c[i, 2]), int(c[i, 1]), int(c[i, 0]))
            v = opened.get(cell)
            if v is None:
                v = opened[cell] = len(opened) if len(opened) < V else -1      # -1: the cell is dropped, with every later row of it
                if v >= 0:
                    coords[base + v] = (f,) + cell
            if v < 0:
                continue
            voxel_of[i] = base + v
            if num[base + v] < T:
                voxels[base + v, num[base + v]] = rows[i, :C]
                num[base + v] += 1
            total[base + v] += 1
        voxel_offsets[f + 1] = base + min(len(opened), V)
    return dict(voxels=voxels, coords=coords, num_points=num, voxel_offsets=voxel_offsets, voxel_of=voxel_of, rows_per_voxel=total, usable=ok)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def constructed_frame(dtype=np.float32, seed=7, n_rows=6000):
    """6000 rows drawn into a pool of 500 cells of the CONSTRUCTED grid with weights 1 / k^0.7 (the walk sees more than V cells, voxels
    above, at and below T rows); 5 % shifted out of the range, 1 % with one NaN coordinate, 4 % with x rounded onto a cell face."""
    rng = np.random.default_rng(seed)
    (x0, y0, z0, x1, y1, z1), _, _, _ = CONSTRUCTED
    pool = rng.choice(40 * 40 * 4, 500, replace=False)
    w = 1.0 / np.arange(1, 501) ** 0.7
    cell = pool[rng.choice(500, n_rows, p=w / w.sum())]
    cx, cy, cz = cell % 40, (cell // 40) % 40, cell // 1600
    pc = np.empty((n_rows, 5), np.float64)
    pc[:, 0] = x0 + cx + rng.uniform(0.05, 0.95, n_rows)
    pc[:, 1] = y0 + cy + rng.uniform(0.05, 0.95, n_rows)
    pc[:, 2] = z0 + cz + rng.uniform(0.05, 0.95, n_rows)
    pc[:, 3] = rng.integers(1, 255, n_rows)
    pc[:, 4] = rng.integers(0, 64, n_rows)
    kind = rng.random(n_rows)
    out = kind < 0.05
    axis = rng.integers(0, 3, n_rows)
    shift = np.where(rng.random(n_rows) < 0.5, -1.0, 1.0) * np.array([40.0, 40.0, 4.0])[axis]
    pc[out, axis[out]] += shift[out]
    nan = (kind >= 0.05) & (kind < 0.06)
    pc[nan, axis[nan]] = np.nan
    face = (kind >= 0.06) & (kind < 0.10)
    pc[face, 0] = np.rint(pc[face, 0])                 # x on a face: the upper cell's (x = 40: out)
    return np.ascontiguousarray(pc.astype(dtype))


def face_rows(setting, dtype=np.float32):
    """Rows on lo_j, on hi_j and on lo_j + k size_j, and one ulp of the row dtype either side of each, on each axis; the other two
    coordinates in the middle of a cell."""
    (x0, y0, z0, x1, y1, z1), size, _, _ = setting
    lo, hi, size = np.array([x0, y0, z0]), np.array([x1, y1, z1]), np.asarray(size, np.float64)
    n = grid_dims(setting[0], size)
    mid = lo + (np.array(n) // 2 + 0.5) * size
    dt = np.dtype(dtype).type
    rows = []
    for j in range(3):
        ks = sorted({1, 2, 3, 7, n[j] // 3, n[j] // 2, n[j] - 2, n[j] - 1} & set(range(1, n[j])))
        for v in [lo[j], hi[j]] + [lo[j] + k * size[j] for k in ks]:
            v = dt(v)
            for p in (np.nextafter(v, dt(-np.inf)), v, np.nextafter(v, dt(np.inf))):
                row = [mid[0], mid[1], mid[2], float(len(rows) % 200 + 1), float(j)]
                row[j] = p
                rows.append(np.array(row, np.float64).astype(dtype))      # (p is a value of the row dtype: the cast keeps it)
    return np.ascontiguousarray(np.stack(rows))


def batch_case(dtype=np.float32):
    """Frames of 6000, 0, 1500 and 300 rows: the constructed frame, an empty frame, the constructed frame's rows 2000 .. 3499 once more
    (the same coordinates in two frames) and a frame that the mask takes away whole.  (rows, offsets, keep)"""
    pc = constructed_frame(dtype)
    rows = np.ascontiguousarray(np.concatenate((pc, pc[2000:3500], pc[100:400])))
    offsets = np.array([0, 6000, 6000, 7500, 7800], np.int64)
    keep = np.random.default_rng(21).random(7800) < 0.8
    keep[7500:] = False
    return rows, offsets, keep


STRADDLE = ((-60.0, -60.0, -3.0, 60.0, 60.0, 5.0), (2.0, 2.0, 8.0), 32, 2000)


@functools.lru_cache(maxsize=None)
def case(name, dtype="float32"):
    """(rows N x 5 read-only, offsets, keep or None, (range, size, T, V)) of a shared input."""
    dt = np.dtype(dtype).type
    offsets = keep = None
    if name == "constructed":
        rows, setting = constructed_frame(dt), CONSTRUCTED
    elif name == "faces":
        rows, setting = face_rows(CONSTRUCTED, dt), CONSTRUCTED
    elif name == "faces_second":
        rows, setting = face_rows(FACES_SECOND, dt), FACES_SECOND
    elif name == "own_voxel":
        rows, setting = np.ascontiguousarray(synthetic_sweep(16, 256, dtype=dt)), SECOND
    elif name in ("batch", "batch_nokeep"):
        rows, offsets, keep = batch_case(dt)
        keep, setting = (keep if name == "batch" else None), CONSTRUCTED
    elif name == "straddle":
        rows, setting = np.ascontiguousarray(synthetic_sweep(64, 128, dtype=dt)), STRADDLE
    elif name == "straddle_firing":
        rows, setting = firing_order(synthetic_sweep(64, 128, dtype=dt), 64, 128), STRADDLE
    else:
        raise KeyError(name)
    offsets = np.array([0, len(rows)], np.int64) if offsets is None else offsets
    rows.setflags(write=False)
    return rows, offsets, keep, setting


CASES = ("constructed", "faces", "faces_second", "own_voxel", "batch", "batch_nokeep", "straddle", "straddle_firing")


@functools.lru_cache(maxsize=None)
def expected(name, dtype="float32", num_features=4, max_points=None, max_voxels=None):
    """voxelize() of a shared input (its own T and V unless given), computed once."""
    rows, offsets, keep, (rng, size, T, V) = case(name, dtype)
    out = voxelize(rows, rng, size, T if max_points is None else max_points, V if max_voxels is None else max_voxels, num_features, keep, offsets)
    for a in out.values():
        a.setflags(write=False)
    return out
