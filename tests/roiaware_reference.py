"""RoI-aware voxel pooling: the DEFINITION of include/snowgpu.h (snowgpu_roi_voxel_pool_device) restated as a brute-force NumPy program --
per roi the members of roipool_reference (the float64 membership vector over all rows of its frame, ascending), their sub-voxels by
separate float64 ufunc calls, a stable grouping by voxel, and per voxel a Python loop over its pooled members with np.float32 adds one
after the other; the pose is an INPUT -- and the shared inputs of tests/test_roiaware_reference.py and tests/test_gpu_roiaware.py with
their expected outputs.  Nothing here imports the package's native code."""
import functools

import numpy as np

import box_reference as br
import roipool_reference as rr

DTYPES = rr.DTYPES
RUN = rr.RUN
EW = (0.5, 0.25, 1.0)              # the extra width of the cases that have one
GRIDS = ((2, 3, 4), (12, 12, 12))
CHANNELS = (1, 5, 8, 65)          # 8: the pooling kernel takes four channels per lane when Cf is a multiple of 4


def grid3(out_size):
    g = np.asarray(out_size).reshape(-1)
    return tuple(int(v) for v in (np.repeat(g, 3) if g.shape == (1,) else g))


def axis_index(l, d, n):
    """The voxel index along one axis: l (k,) float64 local coordinates, d the enlarged size (float64), n the voxels of the axis.  One
    ufunc call per operation; the clamp on the floor, NaN counted as below 0."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        half = np.multiply(np.float64(d), 0.5)
        step = np.divide(np.float64(d), np.float64(n))
        u = np.floor(np.divide(np.add(np.asarray(l, np.float64), half), step))
    low = ~(u >= 0.0)
    u = np.where(low, 0.0, np.where(u >= n, n - 1.0, u))
    return u.astype(np.int64)


def voxel_ids(lx, ly, sz, sizes, grid):
    """The flat voxel (ix Gy + iy) Gz + iz of members with local coordinates lx, ly, sz in a roi of enlarged sizes (dx', dy', dz')."""
    gx, gy, gz = grid
    return (axis_index(lx, sizes[0], gx) * gy + axis_index(ly, sizes[1], gy)) * gz + axis_index(sz, sizes[2], gz)


def roi_lists(rows, roi, pose, grid, P, ew=(0.0, 0.0, 0.0), keep=None):
    """(all members ascending, the voxel of each of the first P) of one roi against the rows of ITS frame."""
    at, lx, ly, sz = rr.members(rows, roi, pose, ew, keep)
    first = at[:P]
    sizes = rr.enlarged(np.asarray(roi)[None], ew)[0, 3:6]
    return at, voxel_ids(lx[first], ly[first], sz[first], sizes, grid)


def pool_members(values):
    """(max, argmax position or -1, avg) per channel of the pooled members' values (k, Cf) float32, k >= 1: pcdet's loop for the maximum,
    the float32 sum one add after the other from +0, one float32 division."""
    k, Cf = values.shape
    best, arg, total = np.zeros(Cf, np.float32), np.full(Cf, -1, np.int64), np.zeros(Cf, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(k):
            x = values[i]
            wins = ((arg < 0) & ~np.isnan(x)) | (x > best)
            best, arg = np.where(wins, x, best), np.where(wins, i, arg)
            total = np.add(total, x, dtype=np.float32)
        avg = np.divide(total, np.float32(k), dtype=np.float32)
    return np.where(arg >= 0, best, np.float32(0)).astype(np.float32), arg, avg


def roi_voxel_pool(rows, rois, pose, out_size, T, P=8192, features=None, ew=(0.0, 0.0, 0.0), keep=None, offsets=None):
    """roi_count (F, M), count (F, M, G), index (F, M, G, T), pose (F, M, 2) and -- with features (N, Cf) float32 -- max, argmax and avg
    (F, M, G, Cf) of the definition."""
    rows, rois = np.asarray(rows), np.asarray(rois)
    assert rois.dtype == rows.dtype and rois.ndim == 3 and pose.shape == rois.shape[:2] + (2,) and pose.dtype == np.float64
    offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    grid = grid3(out_size)
    F, M = rois.shape[:2]
    G, T, P = grid[0] * grid[1] * grid[2], int(T), int(P)
    assert F == len(offsets) - 1
    out = dict(roi_count=np.zeros((F, M), np.int32), count=np.zeros((F, M, G), np.int32), index=np.full((F, M, G, T), -1, np.int32))
    if features is not None:
        features = np.asarray(features)
        assert features.dtype == np.float32 and features.shape[0] == rows.shape[0]
        Cf = features.shape[1]
        out.update(max=np.zeros((F, M, G, Cf), np.float32), argmax=np.full((F, M, G, Cf), -1, np.int32), avg=np.zeros((F, M, G, Cf), np.float32))
    for f in range(F):
        a, b = int(offsets[f]), int(offsets[f + 1])
        for m in range(M):
            at, vox = roi_lists(rows[a:b], rois[f, m], pose[f, m], grid, P, ew, None if keep is None else keep[a:b])
            out["roi_count"][f, m] = len(at)
            for g in np.unique(vox):
                mine = a + at[:P][vox == g]                                # (ascending: row order within the voxel)
                out["count"][f, m, g] = len(mine)
                pooled = mine[:T]
                out["index"][f, m, g, :len(pooled)] = pooled
                if features is not None:
                    best, arg, avg = pool_members(features[pooled])
                    out["max"][f, m, g], out["avg"][f, m, g] = best, avg
                    out["argmax"][f, m, g] = np.where(arg >= 0, pooled[np.maximum(arg, 0)], -1)
    out["pose"] = rr.used_pose(rois, pose, ew)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
OFFSETS = (0, 901, 901, 1503)      # three frames of unequal length, one empty; the first crosses the seam of the 512-row runs
M = 70                             # two 64-bit cell words
ROI = dict(planes=0, hand=1, big=2, lapping=3, empty=4, nan=5)
FIRST_RANDOM, FIRST_ZERO = 6, 60   # rois 6 .. 59 are cars with clusters of rows, 60 .. 69 zero rows (absent)
PLANES_ROI = (16.0, -8.0, 0.5, 6.0, 3.0, 1.5, 0.0)      # sizes 12 x a power of two, dyadic centre, pose (1, 0): every voxel plane of both grids is exact
HAND_ROI = (-16.0, 8.0, 0.0, 8.0, 4.0, 2.0, 0.0)
MARGIN_STEP = 2.0 ** -18           # beyond an x / y face, inside the 1e-5 margin; representable at these coordinates in float32
# name -> (local position in HAND_ROI, the feature value of its rows in row order): every position is well inside one voxel of both grids
HAND = dict(order=((-3.9, -1.9, -0.9), (1e8, -1e8, 1.0)), equal=((3.9, 1.9, 0.9), (2.0, 5.0, 5.0, 1.0)), nan=((-3.9, 1.9, -0.9), (np.nan, np.nan)),
            neginf=((3.9, -1.9, 0.9), (-np.inf, np.nan, -np.inf)))
HAND_AT = dict(order=(10, 300, 700), equal=(20, 21, 22, 23), nan=(30, 600), neginf=(40, 41, 42))        # rows of frame 0; `order` spans the run seam


def plane_rows():
    """name -> (x, y, z) about PLANES_ROI, all dyadic: rows exactly on interior voxel planes, on the closed z faces, and beyond the x / y
    faces inside the margin."""
    cx, cy, cz, dx, dy, dz = PLANES_ROI[:6]
    out = {"x_plane": (cx + 0.5, cy + 0.125, cz + 0.0625), "x_plane_low": (cx - 1.5, cy + 0.125, cz + 0.0625), "y_plane": (cx + 0.25, cy + 0.5, cz + 0.0625),
           "z_plane": (cx + 0.25, cy + 0.125, cz + 0.375), "centre": (cx, cy, cz),
           "z_top": (cx + 0.25, cy + 0.125, cz + dz / 2), "z_bottom": (cx + 0.25, cy + 0.125, cz - dz / 2),
           "x_beyond": (cx + dx / 2 + MARGIN_STEP, cy + 0.125, cz + 0.0625), "x_before": (cx - dx / 2 - MARGIN_STEP, cy + 0.125, cz + 0.0625),
           "y_beyond": (cx + 0.25, cy + dy / 2 + MARGIN_STEP, cz + 0.0625), "y_before": (cx + 0.25, cy - dy / 2 - MARGIN_STEP, cz + 0.0625)}
    return out


PLANE_AT = {name: 100 + 7 * i for i, name in enumerate(plane_rows())}          # rows of frame 0


@functools.lru_cache(maxsize=None)
def case(dtype="float32"):
    """dict(rows N x 5, offsets, keep, rois (F, M, 8), pose (F, M, 2), features {Cf: (N, Cf) float32}), read-only."""
    rng = np.random.default_rng(6100)
    F = len(OFFSETS) - 1
    rois = np.zeros((M, 8))
    rois[ROI["planes"], :7], rois[ROI["hand"], :7] = PLANES_ROI, HAND_ROI
    rois[ROI["big"], :7] = (0.0, 0.0, 0.0, 100.0, 100.0, 20.0, 0.7)
    rois[ROI["lapping"], :7] = (17.0, -7.5, 0.5, 5.0, 3.0, 2.0, 0.4)
    rois[ROI["empty"], :7] = (100.0, 100.0, 0.0, 4.0, 2.0, 2.0, 0.3)
    rois[ROI["nan"], :7] = (5.0, 5.0, np.nan, 4.0, 2.0, 2.0, 0.3)
    k = FIRST_ZERO - FIRST_RANDOM
    rois[FIRST_RANDOM:FIRST_ZERO, :7] = np.column_stack((rng.uniform(-45, 45, k), rng.uniform(-45, 45, k), rng.uniform(-1, 0, k), rng.uniform(3.5, 5, k),
                                                         rng.uniform(1.6, 2.2, k), rng.uniform(1.4, 2, k), rng.uniform(-3.1, 3.1, k)))
    rois[:FIRST_ZERO, 7] = 1 + np.arange(FIRST_ZERO) % 3
    frames = []
    for f in range(F):
        n = OFFSETS[f + 1] - OFFSETS[f]
        p = br._fill(rng, n, dtype)
        if n:
            at = rng.choice(n, n // 2, replace=False)
            own = rng.integers(FIRST_RANDOM, FIRST_ZERO, len(at))
            p[at] = np.vstack([br._around(rng, rois[j], 1, 1.1) for j in own])
            some = rng.choice(n, 60, replace=False)
            p[some] = br._around(rng, rois[ROI["planes"]], 60, 1.05)
            near_hand = (np.abs(p[:, 0] - HAND_ROI[0]) < 7) & (np.abs(p[:, 1] - HAND_ROI[1]) < 5)
            p[near_hand, 2] += 30.0                                        # the hand roi holds the hand rows alone
        frames.append(p)
    for name, xyz in plane_rows().items():
        frames[0][PLANE_AT[name]] = xyz
    for name, (local, values) in HAND.items():
        for i in HAND_AT[name]:
            frames[0][i] = np.add(HAND_ROI[:3], local)
    xyz = np.vstack(frames)
    rows = br._rows(xyz, rng, dtype)
    keep = rng.uniform(0, 1, len(rows)) < 0.9
    special = sorted(list(PLANE_AT.values()) + [i for at in HAND_AT.values() for i in at])
    keep[special] = True
    bad = [200, 450, 1000]                                                 # unusable rows, kept by the mask
    keep[bad] = True
    rows[200, 0], rows[450, 2], rows[1000, 1] = np.nan, np.inf, 1e6 + 1
    features = {}
    for Cf in CHANNELS:
        v = rng.normal(0, 1, (len(rows), Cf)).astype(np.float32)
        v[rng.uniform(0, 1, v.shape) < 0.2] = np.float32(0.5)              # ties among the maxima
        for name, (_, values) in HAND.items():
            for i, x in zip(HAND_AT[name], values):
                v[i] = np.float32(x)
        features[Cf] = v
    rois = np.ascontiguousarray(np.broadcast_to(rois.astype(dtype), (F, M, 8)))
    pose = br.numpy_pose(rois)
    pose[:, ROI["planes"]] = (1.0, 0.0)
    pose[:, ROI["hand"]] = (1.0, 0.0)
    for a in (rows, keep, rois, pose) + tuple(features.values()):
        a.setflags(write=False)
    return dict(rows=rows, offsets=np.array(OFFSETS, np.int64), keep=keep, rois=rois, pose=pose, features=features)


# name -> (dtype, out_size, T, Cf or None, P, keep mask used, extra width): the settings the GPU comparisons run under
SETTINGS = {
    "small_grid": ("float32", (2, 3, 4), 4, 5, 8192, True, (0.0, 0.0, 0.0)),
    "twelve": ("float32", 12, 4, 65, 8192, True, (0.0, 0.0, 0.0)),
    "double_one": ("float64", 12, 1, 1, 8192, False, EW),
    "double_small": ("float64", (2, 3, 4), 1, 5, 8192, True, (0.0, 0.0, 0.0)),
    "capacity": ("float32", (2, 3, 4), 4, 5, 64, False, (0.0, 0.0, 0.0)),
    "four_wide": ("float32", (2, 3, 4), 4, 8, 8192, True, (0.0, 0.0, 0.0)),
    "no_features": ("float32", (2, 3, 4), 4, None, 8192, False, EW),
}


def pool_setting(name, pose=None, rois=None, **kw):
    dtype, out_size, T, Cf, P, masked, ew = SETTINGS[name]
    c = case(dtype)
    a = dict(out_size=out_size, T=T, P=P, features=None if Cf is None else c["features"][Cf], ew=ew, keep=c["keep"] if masked else None)
    a.update(kw)
    return roi_voxel_pool(c["rows"], c["rois"] if rois is None else rois, c["pose"] if pose is None else pose, a["out_size"], a["T"], a["P"], a["features"],
                          a["ew"], a["keep"], c["offsets"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement on the shared input under a setting and the case's given pose."""
    e = pool_setting(name)
    for v in e.values():
        v.setflags(write=False)
    return e
