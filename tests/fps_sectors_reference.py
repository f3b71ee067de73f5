"""Sectorized, proposal-centric keypoint sampling: the DEFINITION of include/snowgpu.h (snowgpu_fps_sectors_device) restated in NumPy -- the
reach and the near test in float64, every operation a ufunc call of its own; the sector from the correctly rounded atan2 of
tests/range_reference.py; the quota in Python integers; the walk of every sector by tests/fps_reference.walk -- and the shared inputs of
tests/test_fps_sectors_reference.py and tests/test_gpu_fps_sectors.py with their expected outputs.  Nothing here imports the package's
native code."""
import functools
import math

import numpy as np

import fps_reference as fr
from range_reference import arctan2

DTYPES = fr.DTYPES
BOUND = fr.BOUND
SECTORS = (1, 4, 6, 16)
EDGE_SECTORS = (4, 6, 16)


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def reach2_of(rois, roi_margin):
    """(present, reach2) of rois (..., Cb): float64, 0 for an absent roi."""
    b = np.asarray(rois)[..., :6].astype(np.float64)
    with np.errstate(invalid="ignore"):
        present = (np.abs(b[..., :3]) <= BOUND).all(axis=-1) & (b[..., 3:] > 0).all(axis=-1) & (b[..., 3:] <= BOUND).all(axis=-1)
    h = np.divide(np.where(present[..., None], b[..., 3:], 0.0), 2.0)
    sq = np.multiply(h, h)
    reach = np.add(np.sqrt(np.add(np.add(sq[..., 0], sq[..., 1]), sq[..., 2])), np.float64(roi_margin))
    return present, np.where(present, np.multiply(reach, reach), 0.0)


def near_any(xyz, rois, roi_margin):
    """Which rows (n x 3, any dtype) are near a present roi of `rois` (B x Cb)."""
    p = np.asarray(xyz).astype(np.float64)
    present, r2 = reach2_of(rois, roi_margin)
    c = np.asarray(rois)[:, :3].astype(np.float64)
    near = np.zeros(len(p), bool)
    for b in np.flatnonzero(present):
        sx, sy, sz = np.subtract(p[:, 0], c[b, 0]), np.subtract(p[:, 1], c[b, 1]), np.subtract(p[:, 2], c[b, 2])
        d = np.add(np.add(np.multiply(sx, sx), np.multiply(sy, sy)), np.multiply(sz, sz))
        near |= d < r2[b]
    return near


def sector_of(x, y, n_sectors):
    """The sector of rows with the coordinates x, y (any dtype; computed in float64)."""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    q = np.floor(np.divide(np.add(arctan2(y, x), np.pi), np.divide(2 * np.pi, n_sectors)))
    return np.minimum(q.astype(np.int64), n_sectors - 1)


def quota(n, K):
    """q_s of the sectors' usable rows n_s for K samples: largest-remainder apportionment, in Python integers."""
    n = [int(v) for v in n]
    m = sum(n)
    if m < K:
        return list(n)
    q, r = [v * K // m for v in n], [v * K % m for v in n]
    L = K - sum(q)
    for s in sorted(range(len(n)), key=lambda s: (-r[s], s))[:L]:
        q[s] += 1
    return q


def fps_sectors(rows, n_samples, n_sectors, point_cloud_range=None, num_features=4, keep=None, offsets=None, rois=None, roi_margin=1.6):
    """The outputs of the definition in their static shapes, as a dict of NumPy arrays."""
    rows = np.asarray(rows)
    offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    F, K, C, S = len(offsets) - 1, int(n_samples), int(num_features), int(n_sectors)
    ok = fr.usable_rows(rows, point_cloud_range, keep)
    out = dict(index=np.full((F, K), -1, np.int32), points=np.zeros((F, K, C), rows.dtype), dist=np.full((F, K), -1, rows.dtype),
               usable=np.zeros(F, np.int32), sector_offsets=np.zeros((F, S + 1), np.int32), sector_count=np.zeros((F, S), np.int32),
               sector_of=np.full(len(rows), -1, np.int8))
    if rois is not None:
        out["reach2"] = reach2_of(rois, roi_margin)[1]
    for f in range(F):
        a, b = int(offsets[f]), int(offsets[f + 1])
        u = a + np.flatnonzero(ok[a:b])
        if rois is not None and len(u):
            u = u[near_any(rows[u, :3], rois[f], roi_margin)]
        sec = sector_of(rows[u, 0], rows[u, 1], S) if len(u) else np.zeros(0, np.int64)
        out["sector_of"][u] = sec
        n = np.bincount(sec, minlength=S)
        q = quota(n, K)
        out["sector_count"][f], out["usable"][f] = n, len(u)
        out["sector_offsets"][f] = np.concatenate(([0], np.cumsum(q)))
        if not len(u):
            continue
        for s in range(S):
            if q[s]:
                us, o = u[sec == s], int(out["sector_offsets"][f, s])
                pos, out["dist"][f, o:o + q[s]], _ = fr.walk(np.ascontiguousarray(rows[us, :3]), q[s])
                out["index"][f, o:o + q[s]] = us[pos]
        filled = int(out["sector_offsets"][f, S])
        out["index"][f, filled:], out["dist"][f, filled:] = out["index"][f, 0], 0
        out["points"][f] = rows[out["index"][f], :C]
    return out


def coverage_radius(rows, index):
    """The largest distance from a row to its nearest keypoint (float64)."""
    p, k = np.asarray(rows)[:, :3].astype(np.float64), np.asarray(rows)[np.asarray(index), :3].astype(np.float64)
    best = np.full(len(p), np.inf)
    for a in range(0, len(k), 64):
        d = ((p[:, None, :] - k[None, a:a + 64, :]) ** 2).sum(axis=2)
        best = np.minimum(best, d.min(axis=1))
    return float(np.sqrt(best.max()))


# ---- inputs: the sector edges ------------------------------------------------------------------------------------------------------------
def _key(v):
    b = int(np.float32(v).view(np.int32))
    return b if b >= 0 else -(b & 0x7FFFFFFF)


def _unkey(k):
    return np.uint32(k if k >= 0 else (-k) | 0x80000000).view(np.float32)


def _sec1(x, y, S):
    return int(sector_of(np.array([x], np.float32), np.array([y], np.float32), S)[0])


def edge_pair(S, k, radius=10.0):
    """Two float32 points ONE float32 step apart on either side of the edge between the sectors k - 1 and k of S (1 <= k < S): one
    coordinate is fixed, the other found by bisection over the float32 numbers.  ((x, y) in k - 1, (x, y) in k)"""
    th = k * (2 * math.pi / S) - math.pi
    lo, hi = th - 0.05, th + 0.05
    along_y = abs(math.cos(th)) >= abs(math.sin(th))
    fixed = np.float32(radius * (math.cos(th) if along_y else math.sin(th)))
    at = (lambda v: (fixed, v)) if along_y else (lambda v: (v, fixed))
    a, b = (_key(radius * (math.sin(t) if along_y else math.cos(t))) for t in (lo, hi))
    assert _sec1(*at(_unkey(a)), S) == k - 1 and _sec1(*at(_unkey(b)), S) == k, (S, k)
    while abs(b - a) > 1:
        mid = (a + b) // 2
        if _sec1(*at(_unkey(mid)), S) == k - 1:
            a = mid
        else:
            b = mid
    return at(_unkey(a)), at(_unkey(b))


@functools.lru_cache(maxsize=None)
def edge_points():
    """The float32 (x, y) of the edge frame: per S of EDGE_SECTORS and inner edge a pair one step apart; the seam (y = -0 and +0, x < 0);
    the origin in its four signs; points on the four half axes.  (xy n x 2 float32, pairs: (S, k, row below, row above))"""
    xy, pairs = [], []
    for S in EDGE_SECTORS:
        for k in range(1, S):
            p, q = edge_pair(S, k)
            pairs.append((S, k, len(xy), len(xy) + 1))
            xy += [p, q]
    xy += [(-7.5, -0.0), (-7.5, 0.0), (-0.25, -0.0), (-0.25, 0.0)]                                   # the seam
    xy += [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]                                       # the origin
    xy += [(3.0, 0.0), (3.0, -0.0), (0.0, 3.0), (-0.0, 3.0), (0.0, -3.0), (-0.0, -3.0)]              # the axes
    return np.array(xy, np.float32), tuple(pairs)


def edges_case(dtype):
    """The edge points (z = 0.5) among 900 rows of a cloud around the sensor: every edge row is usable, and m is far above K, so that the
    tiny distances between the partners of a pair decide no round."""
    rng = np.random.default_rng(31)
    xy, _ = edge_points()
    filler = fr.cloud(900, "float64", seed=32)[:, :3]
    filler[:, 0] -= 20.0                                                 # x in [-20, 20)
    special = np.column_stack((xy.astype(np.float64), np.full(len(xy), 0.5)))
    at = np.sort(rng.choice(900 + len(xy), len(xy), replace=False))      # the edge rows, in their order, spread over the frame
    xyz = np.empty((900 + len(xy), 3))
    mask = np.zeros(len(xyz), bool)
    mask[at] = True
    xyz[mask], xyz[~mask] = special, filler
    return fr._columns(xyz, rng, dtype), at


# ---- inputs: the quota --------------------------------------------------------------------------------------------------------------------
QUOTA_K = 12
QUOTA_COUNTS = ((5, 0, 1, 7), (7, 7, 5, 5), (2, 3, 0, 4), (3, 3, 3, 3), (0, 0, 0, 0))      # usable rows per quadrant sector of S = 4


def quota_case(dtype):
    """Five frames whose rows lie well inside the quadrants -- the sectors of S = 4: third, fourth, first, second quadrant -- in the
    counts of QUOTA_COUNTS, shuffled, with three unusable rows (NaN) each.  (rows, offsets)"""
    rng = np.random.default_rng(41)
    sign = ((-1, -1), (1, -1), (1, 1), (-1, 1))
    frames = []
    for counts in QUOTA_COUNTS:
        pts = [(sx * rng.integers(1024, 30720) * fr.STEP, sy * rng.integers(1024, 30720) * fr.STEP, rng.integers(-2048, 2048) * fr.STEP)
               for (sx, sy), c in zip(sign, counts) for _ in range(c)]
        pts += [(np.nan, 1.0, 0.0)] * 3
        frames.append(np.array(pts, np.float64)[rng.permutation(len(pts))])
    offsets = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
    return fr._columns(np.concatenate(frames), rng, dtype), offsets


# ---- inputs: the rois ---------------------------------------------------------------------------------------------------------------------
ROI_MARGIN = 1.0
ROI_REACH2 = 64.0                      # of the first roi: half edges (2, 3, 6), sqrt(4 + 9 + 36) = 7, + 1


def _below_reach2():
    """A float32 point whose squared distance from the origin, summed as the definition sums it, is the float64 neighbour BELOW 64."""
    x = np.nextafter(np.float32(8.0), np.float32(0.0))
    want = np.nextafter(ROI_REACH2, 0.0)
    rest = want - float(x) * float(x)                                     # exact: a few bits
    y = np.float32(math.sqrt(rest))
    while float(y) * float(y) > rest:
        y = np.nextafter(y, np.float32(0.0))
    z = np.float32(math.sqrt(rest - float(y) * float(y)))
    return float(x), float(y), float(z)


ROI_ROWS = {"equal": (8.0, 0.0, 0.0), "above": (8.0, 2.0 ** -23, 0.0), "below": _below_reach2()}


def roi_case(dtype):
    """Two frames of 1500 rows of one cloud around the sensor.  Frame 0: the roi at the origin whose reach2 is 64, the three rows of
    ROI_ROWS at the head of the frame, two overlapping car-sized rois, a zero-padded roi, one with NaN and one with a negative edge.
    Frame 1: every roi absent.  (rows, offsets, rois (2, 6, 8))"""
    rng = np.random.default_rng(51)
    xyz = fr.cloud(3000, "float64", seed=52)[:, :3]
    xyz[:, 0] -= 20.0
    xyz[:3] = [ROI_ROWS["equal"], ROI_ROWS["above"], ROI_ROWS["below"]]
    rois = np.zeros((2, 6, 8))
    rois[0, 0, :7] = (0.0, 0.0, 0.0, 4.0, 6.0, 12.0, 0.3)
    rois[0, 1, :7] = (12.0, 5.0, -0.5, 3.9, 1.6, 1.56, 1.2)
    rois[0, 2, :7] = (13.5, 5.5, -0.5, 4.2, 1.8, 1.6, -0.4)             # overlaps the one before
    rois[0, 4, :7] = (-10.0, np.nan, 0.0, 4.0, 2.0, 2.0, 0.0)
    rois[0, 5, :7] = (-10.0, -6.0, 0.0, -4.0, 2.0, 2.0, 0.0)
    rois[1, 1, :7] = (5.0, 5.0, 0.0, 0.0, 2.0, 2.0, 0.0)                 # dx = 0: absent
    rois[1, 2, :7] = (2e6, 5.0, 0.0, 4.0, 2.0, 2.0, 0.0)                 # beyond the bound: absent
    rois[:, :, 7] = 1.0                                                  # a class column
    return fr._columns(xyz, rng, dtype), np.array([0, 1500, 3000], np.int64), np.ascontiguousarray(rois.astype(dtype))


def batch_rois(dtype):
    """Rois for fps_reference.batch_case, on frames 0 and 2 only: (4, 3, 7); frame 2's second roi is zero padding."""
    rois = np.zeros((4, 3, 7))
    rois[0, 0] = (10.0, -5.0, 0.0, 8.0, 6.0, 3.0, 0.5)
    rois[0, 1] = (30.0, 10.0, 0.5, 4.0, 2.0, 1.5, 0.0)
    rois[0, 2] = (12.0, -4.0, 0.0, 5.0, 5.0, 2.0, 1.0)
    rois[2, 0] = (20.0, 0.0, 0.0, 12.0, 10.0, 4.0, 0.0)
    rois[2, 2] = (5.0, 15.0, 0.0, 4.0, 4.0, 4.0, 0.0)
    return np.ascontiguousarray(rois.astype(dtype))


@functools.lru_cache(maxsize=None)
def case(name, dtype="float32"):
    """(rows N x 5 read-only, offsets, keep or None, rois or None, (range or None, K, margin)) of a shared input."""
    keep = rois = None
    if name == "edges":
        (rows, _), offsets, setting = edges_case(dtype), None, (None, 32, 1.6)
    elif name == "quota":
        (rows, offsets), setting = quota_case(dtype), (None, QUOTA_K, 1.6)
    elif name == "roi":
        (rows, offsets, rois), setting = roi_case(dtype), (None, 16, ROI_MARGIN)
    elif name in ("batch", "batch_rois"):
        rows, offsets, keep = fr.batch_case(dtype)
        rois, setting = batch_rois(dtype) if name == "batch_rois" else None, (fr.RANGE, 48, 1.6)
    else:
        raise KeyError(name)
    offsets = np.array([0, len(rows)], np.int64) if offsets is None else offsets
    rows.setflags(write=False)
    if rois is not None:
        rois.setflags(write=False)
    return rows, offsets, keep, rois, setting


CASES = ("edges", "quota", "roi")


@functools.lru_cache(maxsize=None)
def expected(name, dtype="float32", n_sectors=6, num_features=4):
    """fps_sectors() of a shared input, computed once."""
    rows, offsets, keep, rois, (rng, K, margin) = case(name, dtype)
    return fr._frozen(fps_sectors(rows, K, n_sectors, rng, num_features, keep, offsets, rois, margin))


def tier_frames(dtype):
    """Three frames for S = 2 whose two sectors (y < 0, y > 0) straddle the three capacities of the walk: c and c + 1 rows for the edge
    between the register tier and the LDS tier, c - 1 and c + 1 around the other two.  (rows, offsets, rows per (frame, sector))"""
    from lidar_snow_sim_amd.fps import TIER_ROWS
    t0, t1, t2 = TIER_ROWS[dtype]
    sizes = ((t1, t1 + 1), (t0 - 1, t0 + 1), (t2 - 1, t2 + 1))
    total = sum(a + b for a, b in sizes)
    pool = fr.cloud(total + 4096, dtype, seed=61)                        # y in [-20, 20): its sign decides the sector of S = 2
    neg, pos = pool[pool[:, 1] < -fr.STEP], pool[pool[:, 1] > fr.STEP]
    frames, i, j = [], 0, 0
    rng = np.random.default_rng(62)
    for a, b in sizes:
        part = np.concatenate((neg[i:i + a], pos[j:j + b]))
        frames.append(part[rng.permutation(a + b)])
        i, j = i + a, j + b
    assert i <= len(neg) and j <= len(pos)
    offsets = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(frames)), offsets, sizes


@functools.lru_cache(maxsize=None)
def tier_case(dtype):
    rows, offsets, sizes = tier_frames(dtype)
    rows.setflags(write=False)
    return rows, offsets, sizes, fr._frozen(fps_sectors(rows, 24, 2, fr.RANGE, 4, None, offsets))
