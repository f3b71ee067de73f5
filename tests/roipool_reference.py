"""RoI point pooling: the DEFINITION of include/snowgpu.h (snowgpu_roi_point_pool_device) restated as a brute-force NumPy program -- per
roi a float64 membership vector over all rows of its frame by box_reference's matrices on the ENLARGED roi (the same operations in the
same order, every one a ufunc call of its own), then np.flatnonzero, the modulo fill, the gather and `local`; the pose is an INPUT -- and
the shared inputs of tests/test_roipool_reference.py and tests/test_gpu_roipool.py with their expected outputs.  Nothing here imports
the package's native code."""
import functools

import numpy as np

import box_reference as br

DTYPES = br.DTYPES
RUN = 512                          # rows of a run (csrc/sg_roipool.h): the seams of the counting
EW = (0.5, 0.25, 1.0)              # the extra width of the cases that have one


def enlarged(rois, ew):
    """(..., 7) float64: the rois with ew added once to dx, dy, dz -- one float64 add each."""
    b = np.asarray(rois)[..., :7].astype(np.float64)
    b[..., 3:6] = np.add(b[..., 3:6], np.asarray(ew, np.float64))
    return b


def present(rois, pose, ew=(0.0, 0.0, 0.0)):
    """Which rois are present: the rule of points_in_boxes on the enlarged roi, and original sizes > 0."""
    with np.errstate(invalid="ignore"):
        return br.present(enlarged(rois, ew), pose) & (np.asarray(rois)[..., 3:6].astype(np.float64) > 0).all(-1)


def used_pose(rois, pose, ew=(0.0, 0.0, 0.0)):
    return np.where(present(rois, pose, ew)[..., None], pose, 0.0)


def members(rows, roi, pose, ew=(0.0, 0.0, 0.0), keep=None):
    """(indices ascending, lx, ly, sz of all rows) for one roi (7 ..) under pose (2,) against the rows of ITS frame."""
    rows = np.asarray(rows)
    big = enlarged(np.asarray(roi)[None], ew)
    lx, ly, sz, inside = br.frame_matrices(rows[:, :3].astype(np.float64), big, np.asarray(pose, np.float64)[None])
    ok = br.usable_rows(rows, keep) & bool(present(np.asarray(roi)[None], np.asarray(pose, np.float64)[None], ew)[0])
    return np.flatnonzero(inside[:, 0] & ok), lx[:, 0], ly[:, 0], sz[:, 0]


def roi_point_pool(rows, rois, pose, n_samples, num_features=4, ew=(0.0, 0.0, 0.0), keep=None, offsets=None):
    """index (F, M, S), count (F, M), points (F, M, S, C), local (F, M, S, 3) and pose (F, M, 2) of the definition."""
    rows, rois = np.asarray(rows), np.asarray(rois)
    assert rois.dtype == rows.dtype and rois.ndim == 3 and pose.shape == rois.shape[:2] + (2,) and pose.dtype == np.float64
    offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    F, M = rois.shape[:2]
    S, C = int(n_samples), int(num_features)
    assert F == len(offsets) - 1
    index = np.full((F, M, S), -1, np.int32)
    count = np.zeros((F, M), np.int32)
    points = np.zeros((F, M, S, C), rows.dtype)
    local = np.zeros((F, M, S, 3), rows.dtype)
    for f in range(F):
        a, b = int(offsets[f]), int(offsets[f + 1])
        for m in range(M):
            at, lx, ly, sz = members(rows[a:b], rois[f, m], pose[f, m], ew, None if keep is None else keep[a:b])
            count[f, m] = len(at)
            if len(at):
                pick = at[np.arange(S) % len(at)]
                index[f, m] = a + pick
                points[f, m] = rows[a + pick, :C]
                local[f, m] = np.stack((lx[pick], ly[pick], sz[pick]), axis=1).astype(rows.dtype)
    return dict(index=index, count=count, points=points, local=local, pose=used_pose(rois, pose, ew))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _case(rows, offsets, keep, rois, pose, S, ew=(0.0, 0.0, 0.0), C=4, **more):
    rois = np.ascontiguousarray(rois)
    for a in (rows, offsets, keep, rois, pose):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(rows=rows, offsets=offsets, keep=keep, rois=rois, pose=pose, S=S, ew=tuple(ew), C=C, **more)


def count_targets(S):
    return (0, 1, S - 1, S, S + 1, 3 * S + 7)


def _counts(S, dtype):
    """Two frames; roi j holds count_targets(S)[j] rows of frame 0 (and another number of frame 1), shuffled among fill rows so that the
    members of a roi are spread over the runs."""
    rng = np.random.default_rng(5100 + S)
    targets = count_targets(S)
    rois = np.zeros((2, len(targets) + 1, 8))
    for j in range(len(targets)):
        rois[:, j] = (-50 + 16.0 * j, 20 - 7.0 * j, -0.5, 4.0, 2.0, 2.0, 0.3 * j - 0.7, 1 + j % 3)
    rois[:, len(targets)] = rois[:, 3]                                     # a twin of roi 3
    frames = []
    for f in range(2):
        parts = [br._around(rng, rois[f, j], t + 3 * f, 0.9) for j, t in enumerate(targets)]
        fill = br._fill(rng, 700 + 77 * f, dtype) + (0, 0, 30)             # above every roi
        p = np.vstack(parts + [fill])
        frames.append(p[rng.permutation(len(p))])
    offsets = np.concatenate(([0], np.cumsum([len(p) for p in frames]))).astype(np.int64)
    rois = rois.astype(dtype)
    return _case(br._rows(np.vstack(frames), rng, dtype), offsets, None, rois, br.numpy_pose(rois), S, C=3 + S % 3)


SEAM_OFFSETS = (0, 1000, 1000, 2345, 4045)
SEAM_ROI = dict(ends=0, first63=1, first64=2, first65=3, all=4, cluster=5)


def _seams(dtype):
    """Four frames with boundaries mid-wave, one empty; the last is more than three runs long.  The same rois in every frame."""
    rng = np.random.default_rng(5200)
    rois = np.zeros((4, 6, 7))
    rois[:, 0] = (50.0, 50.0, 0.0, 2.0, 2.0, 2.0, 0.0)
    for j, dx in ((1, 2.0), (2, 4.0), (3, 6.0)):
        rois[:, j] = (-50.0, 50.0, 0.0, dx, 2.0, 2.0, 0.0)
    rois[:, 4] = (0.0, 0.0, 0.0, 1000.0, 1000.0, 100.0, 0.7)
    rois[:, 5] = (10.0, -20.0, 0.0, 6.0, 5.0, 3.0, 1.1)
    n = np.diff(SEAM_OFFSETS)
    frames = []
    for f in range(4):
        p = br._fill(rng, int(n[f]), dtype) * (0.6, 0.6, 1.0)              # within +-36 m: away from rois 0 .. 3
        if n[f]:
            at = rng.choice(int(n[f]), int(n[f]) // 5, replace=False)
            p[at] = br._around(rng, rois[f, 5], len(at), 1.3)
        frames.append(p)
    last = frames[3]
    last[0] = (50.25, 49.75, 0.5)
    last[-1] = (49.5, 50.5, -0.25)
    last[1:64] = np.column_stack((-50 + rng.integers(-7, 8, 63) / 8.0, 50 + rng.integers(-7, 8, 63) / 8.0, np.zeros(63)))
    last[64] = (-48.5, 50.0, 0.0)                                          # |lx| = 1.5: in rois 2 and 3
    last[65] = (-52.5, 50.0, 0.0)                                          # |lx| = 2.5: in roi 3 alone
    rois = rois.astype(dtype)
    return _case(br._rows(np.vstack(frames), rng, dtype), np.array(SEAM_OFFSETS, np.int64), None, rois, br.numpy_pose(rois), 100, C=5)


OVERLAP_M = (1, 64, 65, 512)


def _overlap(M, dtype):
    """Two frames of 300 rows about M rois that all contain (10, 10, 0): row 0 of frame 0 lies in every roi; the last roi is the first again."""
    rng = np.random.default_rng(5300 + M)
    rois = np.zeros((2, M, 7))
    for f in range(2):
        rois[f] = np.column_stack((10 + rng.uniform(-0.5, 0.5, M), 10 + rng.uniform(-0.5, 0.5, M), rng.uniform(-0.2, 0.2, M), rng.uniform(3.5, 5, M),
                                   rng.uniform(2.0, 2.4, M), rng.uniform(1.5, 2, M), rng.uniform(-3.1, 3.1, M)))
        rois[f, M - 1] = rois[f, 0]
    frames = []
    for f in range(2):
        p = np.vstack((np.array([10.0, 10.0, 0.0]) + rng.normal(0, 1.5, (150, 3)) * (1, 1, 0.5), br._fill(rng, 150, dtype)))
        p = p[rng.permutation(300)]
        p[0] = (10.0, 10.0, 0.0)
        frames.append(p)
    rois = rois.astype(dtype)
    return _case(br._rows(np.vstack(frames), rng, dtype), np.array([0, 300, 600], np.int64), None, rois, br.numpy_pose(rois), 100)


FACE_ROI = (0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0)           # centred on the origin under the pose (1, 0): lx = x, ly = y, sz = z exactly
ONLY_EW_ROI = (16.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0)


def face_rows(dtype, ew):
    """name -> (x, y, z) in `dtype` about FACE_ROI enlarged by ew: z exactly on +-dz' / 2 and one step beyond; |x| (|y|) the smallest
    value of the dtype at or beyond dx' / 2 + 1e-5 -- in float64 that value itself -- and one step inside."""
    t = np.dtype(dtype).type
    big = enlarged(np.array(FACE_ROI), ew)
    hx, hy = (np.add(np.multiply(big[j], 0.5), br.MARGIN) for j in (3, 4))
    hz = np.multiply(big[5], 0.5)
    out = {"top_in": (0.5, 0.25, t(hz)), "top_out": (0.5, 0.25, np.nextafter(t(hz), t(10))), "bottom_in": (-0.5, 0.25, t(-hz)),
           "bottom_out": (-0.5, 0.25, np.nextafter(t(-hz), t(-10)))}
    for name, axis, h in (("x", 0, hx), ("y", 1, hy)):
        at = t(h)
        if np.float64(at) < h:
            at = np.nextafter(at, t(10))
        for sign, pre in ((1, ""), (-1, "-")):
            for kind, v in (("out", at), ("in", np.nextafter(at, t(0)))):
                p = [0.25, 0.25, 0.125]
                p[axis] = sign * v
                out[pre + name + "_" + kind] = tuple(p)
    return out


def _faces(dtype, ew):
    """One frame: the face rows of FACE_ROI for ew = 0 and for EW alike (the restatement decides which are inside under the ew of the
    case), rows that only the enlarged ONLY_EW_ROI holds, and dyadic fill."""
    rng = np.random.default_rng(5400)
    names, pts = [], []
    for tag, e in (("", (0.0, 0.0, 0.0)), ("ew:", EW)):
        for name, p in face_rows(dtype, e).items():
            names.append(tag + name)
            pts.append(p)
    only = [(16 + 1.125, 0.5, 0.0), (16 - 1.0625, -0.25, 0.5), (16.0, 1.0625, -0.25), (16.25, 0.0, 1.25)]
    fill = rng.integers(-64, 65, (40, 3)) / 16.0
    t = np.dtype(dtype).type
    xyz = np.array([[t(v) for v in p] for p in pts] + only + fill.tolist(), dtype)
    rows = np.ascontiguousarray(np.column_stack((xyz, rng.integers(1, 255, len(xyz)).astype(dtype), rng.integers(0, 64, len(xyz)).astype(dtype))))
    rois = np.array([[FACE_ROI, ONLY_EW_ROI]], dtype)
    pose = np.array([[[1.0, 0.0], [1.0, 0.0]]])
    special = {n: i for i, n in enumerate(names)}
    special["only_ew"] = (len(pts), len(pts) + len(only))
    return _case(rows, np.array([0, len(rows)], np.int64), None, rois, pose, 100, ew, special=special)


ABSENT = dict(zero=0, dx0=1, nan=2, inf=3, bad_pose=4, good=5, far=6, edge=7, dz_negative=8)


def _absent(dtype):
    """One frame, ew = EW: absent rois of every kind at the place of a good one, rows inside the good one that are not usable, a roi
    beyond +-120 m and one at the 1e6 bound."""
    rng = np.random.default_rng(5500)
    good = (5.0, 5.0, 0.0, 4.0, 2.0, 2.0, 0.25)
    rois = np.zeros((1, len(ABSENT), 7))
    rois[0, 1] = good[:3] + (0.0,) + good[4:]
    rois[0, 2] = (np.nan,) + good[1:]
    rois[0, 3] = good[:6] + (np.inf,)
    rois[0, 4] = good
    rois[0, 5] = good
    rois[0, 6] = (150.0, -130.0, 0.0, 4.0, 2.0, 2.0, 0.9)
    rois[0, 7] = (999998.0, 0.0, 0.0, 8.0, 2.0, 2.0, 0.0)
    rois[0, 8] = good[:5] + (-0.5,) + good[6:]                             # dz' = 0.5 > 0, the original is not
    inside = br._around(rng, good, 60, 0.9)
    far = br._around(rng, rois[0, 6], 30, 1.2)
    edge = np.array([[999999.0, 0.0, 0.0], [1e6 + 1, 0.0, 0.0], [1e6, 0.5, 0.0], [999996.0, 0.0, 0.5]])
    xyz = np.vstack((inside, far, edge, br._fill(rng, 100, dtype)))
    rows = br._rows(xyz, rng, dtype)
    keep = np.ones(len(rows), bool)
    keep[0:60:4] = False                                                   # a quarter of the good roi's rows
    rows[1, 0] = np.nan
    rows[5, 2] = np.inf
    rows[9, 1] = 1e6 + 1
    rois = rois.astype(dtype)
    pose = br.numpy_pose(rois)
    pose[0, 4] = (2.0, 0.0)
    return _case(rows, np.array([0, len(rows)], np.int64), keep, rois, pose, 100, EW, C=5)


def _headings(dtype):
    """box_reference's random case -- two frames of about 2000 clustered rows, 40 rois of car size with random headings, a quarter of the
    slots zero -- with an extra width."""
    rows, offsets, keep, boxes, pose = br.case("random", dtype)
    return _case(rows, offsets, keep, boxes, pose, 16, (0.3, 0.3, 0.3))


CASES = tuple(f"counts{S}" for S in (1, 100, 512)) + ("seams",) + tuple(f"overlap{M}" for M in OVERLAP_M) + ("faces", "faces_ew", "absent", "headings")


@functools.lru_cache(maxsize=None)
def case(name, dtype="float32"):
    """dict(rows N x 5, offsets, keep or None, rois (F, M, Cb), pose (F, M, 2), S, ew, C[, special]), read-only."""
    if name.startswith("counts"):
        return _counts(int(name[6:]), dtype)
    if name.startswith("overlap"):
        return _overlap(int(name[7:]), dtype)
    if name.startswith("faces"):
        return _faces(dtype, EW if name.endswith("_ew") else (0.0, 0.0, 0.0))
    return {"seams": _seams, "absent": _absent, "headings": _headings}[name](dtype)


def pool_case(c, pose=None, **kw):
    a = dict(c, **kw)
    return roi_point_pool(a["rows"], a["rois"], a["pose"] if pose is None else pose, a["S"], a["C"], a["ew"], a["keep"], a["offsets"])


@functools.lru_cache(maxsize=None)
def expected(name, dtype="float32"):
    """The restatement on a shared input under the case's given pose."""
    e = pool_case(case(name, dtype))
    for v in e.values():
        v.setflags(write=False)
    return e
