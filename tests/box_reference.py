"""Points in 3D boxes: the DEFINITION of include/snowgpu.h (snowgpu_points_in_boxes_device) restated as a brute-force NumPy program -- the
full (rows x boxes) matrices of a frame in float64, every subtraction, product and sum a ufunc call of its own, the pose an INPUT -- and
the shared inputs of tests/test_box_reference.py and tests/test_gpu_boxes.py with their expected outputs.  cells() restates the grid of
csrc/sg_box.h so that the inputs can be held to conditions on cells.  Nothing here imports the package's native code."""
import functools
import math

import numpy as np

DTYPES = ("float32", "float64")
BOUND = 1e6
MARGIN = 1e-5
POSE_TOL = 1e-6
SENSOR, SIDE = 120.0, 64
EDGE = 2 * SENSOR / SIDE           # 3.75 m


def numpy_pose(boxes):
    """(..., 2) float64: cos and sin of the heading in float64, NumPy's."""
    h = np.asarray(boxes)[..., 6].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack((np.cos(h), np.sin(h)), axis=-1)


def present(boxes, pose):
    """Which boxes are present under `pose` (..., 2)."""
    b = np.asarray(boxes)[..., :7].astype(np.float64)
    c, s = pose[..., 0], pose[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(b[..., 0:3]) <= BOUND).all(-1) & ((b[..., 3:6] > 0) & (b[..., 3:6] <= BOUND)).all(-1) & (np.abs(b[..., 6]) <= BOUND)
        unit = np.abs(np.subtract(np.add(np.multiply(c, c), np.multiply(s, s)), 1.0)) <= POSE_TOL
    return ok & unit


def used_pose(boxes, pose):
    """What d_out_pose receives: the pose of a present box, (0, 0) of an absent one."""
    return np.where(present(boxes, pose)[..., None], pose, 0.0)


def usable_rows(rows, keep=None):
    with np.errstate(invalid="ignore"):
        ok = (np.abs(rows[:, :3].astype(np.float64)) <= BOUND).all(axis=1)
    return ok if keep is None else ok & np.asarray(keep, bool)


def frame_matrices(xyz, boxes, pose):
    """lx, ly, sz and inside, each (n, B), of float64 points against the boxes of one frame under `pose` (B, 2)."""
    b = np.asarray(boxes)[:, :7].astype(np.float64)
    ok = present(boxes, pose)
    c, s = pose[None, :, 0], pose[None, :, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy, sz = (np.subtract(xyz[:, None, j], b[None, :, j]) for j in range(3))
        lx = np.add(np.multiply(sx, c), np.multiply(sy, s))
        ly = np.subtract(np.multiply(sy, c), np.multiply(sx, s))
        hx, hy, hz = np.add(np.multiply(b[:, 3], 0.5), MARGIN), np.add(np.multiply(b[:, 4], 0.5), MARGIN), np.multiply(b[:, 5], 0.5)
        inside = (np.abs(sz) <= hz[None]) & (np.abs(lx) < hx[None]) & (np.abs(ly) < hy[None]) & ok[None]
    return lx, ly, sz, inside


def points_in_boxes(rows, boxes, pose, keep=None, offsets=None):
    """box_of (N), count (F, B) and local (N, 3) of the definition, as a dict of NumPy arrays."""
    rows, boxes = np.asarray(rows), np.asarray(boxes)
    assert boxes.dtype == rows.dtype and boxes.ndim == 3 and pose.shape == boxes.shape[:2] + (2,) and pose.dtype == np.float64
    offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    F, B = boxes.shape[:2]
    assert F == len(offsets) - 1
    ok = usable_rows(rows, keep)
    box_of = np.full(len(rows), -1, np.int32)
    count = np.zeros((F, B), np.int32)
    local = np.zeros((len(rows), 3), rows.dtype)
    for f in range(F):
        u = int(offsets[f]) + np.flatnonzero(ok[offsets[f]:offsets[f + 1]])
        if not len(u):
            continue
        lx, ly, sz, inside = frame_matrices(rows[u, :3].astype(np.float64), boxes[f], pose[f])
        count[f] = inside.sum(axis=0)
        hit = inside.any(axis=1)
        first = inside.argmax(axis=1)
        box_of[u] = np.where(hit, first, -1)
        at = np.arange(len(u))
        loc = np.stack((lx[at, first], ly[at, first], sz[at, first]), axis=1)
        local[u] = np.where(hit[:, None], loc, 0.0).astype(rows.dtype)
    return dict(box_of=box_of, count=count, local=local)


# ---- the cells (csrc/sg_box.h) ---------------------------------------------------------------------------------------------------------------
def cells(v):
    """The cell index of coordinates on either axis, clamped as sg_box_index clamps."""
    with np.errstate(invalid="ignore"):
        t = np.floor((np.asarray(v, np.float64) + SENSOR) * (SIDE / (2.0 * SENSOR)))
    return np.clip(np.nan_to_num(t, nan=0.0), 0, SIDE - 1).astype(np.int64)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _rows(xyz, rng, dtype):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(xyz)
    return np.ascontiguousarray(np.column_stack((xyz, rng.integers(1, 255, n), rng.integers(0, 64, n))).astype(dtype))


def world(box, local):
    """Points given in the frame of `box` (lx, ly, lz about its centre), in world coordinates, float64 (rounded: the restatement decides
    on which side of a face they fall)."""
    l = np.asarray(local, np.float64).reshape(-1, 3)
    c, s = math.cos(float(box[6])), math.sin(float(box[6]))
    return np.column_stack((box[0] + l[:, 0] * c - l[:, 1] * s, box[1] + l[:, 0] * s + l[:, 1] * c, box[2] + l[:, 2]))


def _around(rng, box, n, reach=1.4):
    """n points about `box`: local coordinates uniform within `reach` half extents, so some fall outside."""
    return world(box, rng.uniform(-reach, reach, (n, 3)) * np.asarray(box[3:6], np.float64) * 0.5)


def _fill(rng, n, dtype):
    """n rows of a sweep-like cloud within +-60 m"""
    return np.column_stack((rng.uniform(-60, 60, n), rng.uniform(-60, 60, n), rng.uniform(-2, 1, n)))


CONSTRUCTED_B = 12
COUNTS = (0, 1, 63, 64, 65, 257, 1000)
FRAME = dict(no_row=0, absent=1, faces=2, headings=3, overlap=4, all_rows=5, extremes=6)
FACE_BOX = (0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0)      # (centred on the origin: sx = x, sy = y and sz = z exactly)
THIN_BOX = (8.5, 7.5, 0.0, 0.05, 6.0, 2.0, math.pi / 4)
TWIN_BOX = (20.0, -10.0, 0.0, 4.0, 2.0, 2.0, 0.3)
HEADINGS = (0.0, math.pi / 2, -math.pi / 2, math.pi, 7.5, -20.0, 1.234, -2.9)


def _box(b, cls=1.0):
    return list(b) + [cls]


def face_values(dtype):
    """The z and x / y values of the face rows of FACE_BOX in `dtype`: z exactly on cz +- dz / 2 and one nextafter beyond; x (and y) the
    smallest value of the dtype at or beyond dx / 2 + 1e-5 -- that value itself in float64 -- and one nextafter inside."""
    t = np.dtype(dtype).type
    out = {}
    for name, edge in (("top", 0.75), ("bottom", -0.75)):
        out[name + "_in"] = t(edge)
        out[name + "_out"] = np.nextafter(t(edge), t(edge * 10))
    for name, half in (("x", 2.0), ("y", 1.0)):
        h = np.add(np.float64(half), MARGIN)
        at = t(h)
        if np.float64(at) < h:
            at = np.nextafter(at, t(10))
        out[name + "_out"] = at
        out[name + "_in"] = np.nextafter(at, t(0))
    return out


@functools.lru_cache(maxsize=None)
def _constructed(dtype):
    rng = np.random.default_rng(4100)
    B = CONSTRUCTED_B
    zero = [0.0] * 8
    boxes = np.zeros((len(COUNTS), B, 8))
    rows, special, keep_off = [], {}, []
    # frame 0: no row; one present box, which stays empty
    boxes[0, 3] = _box((5, 5, 0, 4, 2, 2, 0.5))
    rows.append(np.zeros((0, 3)))
    # frame 1: one row, inside what every box would be were it present; box 6 is absent only under the given pose (2, 0)
    good = (1.0, 1.0, 0.0, 4.0, 2.0, 2.0, 0.25)
    bad = [zero, _box((np.nan,) + good[1:]), _box(good[:3] + (0.0,) + good[4:]), _box(good[:3] + (-4.0,) + good[4:]), _box(good[:6] + (np.inf,)),
           _box((2e6,) + good[1:]), _box(good), _box(good[:5] + (np.nan, 0.25)), _box(good[:4] + (1.5e6,) + good[5:]), _box(good[:6] + (-3e6,)),
           _box(good[:2] + (-np.inf,) + good[3:]), zero]
    boxes[1] = np.array(bad)
    rows.append(np.array([[1.0, 1.0, 0.0]]))
    # frame 2: the faces of FACE_BOX (heading 0, centred on the origin's cell corner, so lx = x and ly = y exactly)
    boxes[2, 0] = _box(FACE_BOX)
    boxes[2, 1] = _box((30, 30, 0, 4, 2, 2, 1.0))
    rows.append(np.vstack((np.zeros((12, 3)), _around(rng, FACE_BOX, 51))))      # rows 0 .. 11 are set in the dtype below
    # frame 3: headings, and a thin rotated box across several cells
    for j, h in enumerate(HEADINGS):
        boxes[3, j] = _box((-40 + 11 * j, 12 - 5 * j, -0.5, 4.5, 1.9, 1.6, h), 1 + j % 3)
    boxes[3, 9] = _box(THIN_BOX, 2)
    along = world(THIN_BOX, np.column_stack((np.zeros(14), np.linspace(-2.9, 2.9, 14), np.zeros(14))))
    beside = world(THIN_BOX, np.column_stack((np.full(6, 0.1), np.linspace(-2.5, 2.5, 6), np.zeros(6))))
    rows.append(np.vstack([along, beside] + [_around(rng, boxes[3, j], 5 if j < 4 else 6, 1.15) for j in range(8)]))
    # frame 4: overlapping and nested boxes; the containing box has the smaller number once and the larger number once
    boxes[4, 1] = _box((10, 10, 0, 8, 6, 3, 0.4))
    boxes[4, 4] = _box((10, 10, 0, 2, 1.5, 1, 1.1), 2)            # nested in 1
    boxes[4, 6] = _box((13, 12, 0, 6, 4, 3, -0.3), 3)             # overlaps 1
    boxes[4, 2] = _box((-20, 5, 0, 2, 2, 2, 0.0), 2)              # nested in 8: the nested one wins
    boxes[4, 8] = _box((-20, 5, 0, 9, 9, 4, 2.0))
    rows.append(np.vstack((_around(rng, boxes[4, 4], 15), _around(rng, boxes[4, 6], 15), _around(rng, boxes[4, 1], 15), _around(rng, boxes[4, 8], 10, 1.1),
                           _around(rng, boxes[4, 2], 10, 0.95))))
    # frame 5: a box that contains every row of its frame (rows beyond +-120 m among them) and the twin of frame 6's box, empty here
    boxes[5, 0] = _box(TWIN_BOX, 3)
    boxes[5, 7] = _box((0, 0, 0, 1000, 1000, 100, 0.7))
    far = np.column_stack((rng.uniform(-300, 300, 57), rng.uniform(-300, 300, 57), rng.uniform(-3, 3, 57)))
    fill = _fill(rng, 200, dtype)
    fill = fill[np.abs(frame_matrices(fill, np.array([_box(TWIN_BOX)]), numpy_pose(np.array([_box(TWIN_BOX)])))[0][:, 0]) > 4][:200]
    rows.append(np.vstack((far, fill, _fill(rng, 257 - 57 - len(fill), dtype) + (0, 0, 20))))
    # frame 6: the twin box with rows; a box smaller than a cell on a cell corner; boxes and rows beyond +-120 m and at 9e5; rows that
    # are not usable; a keep mask that removes rows inside boxes
    boxes[6, 0] = _box(TWIN_BOX, 3)
    boxes[6, 2] = _box((3 * EDGE, -2 * EDGE, 0, 0.5, 0.5, 1, 0.6), 2)
    boxes[6, 3] = _box((150, -130, 0, 4, 2, 2, 0.9))
    boxes[6, 5] = _box((9e5, -9e5, 0, 4, 2, 2, 0.0))
    boxes[6, 6] = _box((-125, 0, 0, 12, 3, 3, 1.5))               # across the domain's border
    boxes[6, 11] = _box((40, 40, 30, 4, 2, 2, 0.2))               # present and empty
    parts = [_around(rng, boxes[6, j], m) for j, m in ((0, 60), (2, 40), (3, 40), (6, 40))]
    parts.append(world(boxes[6, 5], rng.integers(-40, 40, (40, 3)) * (0.0625, 0.0625, 0.0625)))      # multiples of float32's step at 9e5
    bad_rows = np.array([[np.nan, 0, 0], [0, np.inf, 0], [20, -10, -np.inf], [1.5e6, 0, 0], [20, -1.0000001e6, 0], [20, -10, 2e6]])
    rows.append(np.vstack(parts + [bad_rows, _fill(rng, 1000 - 220 - len(bad_rows), dtype)]))
    counts = [len(r) for r in rows]
    assert tuple(counts) == COUNTS, counts
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    out = _rows(np.vstack(rows), rng, dtype)
    # the face rows, in the dtype
    fv, t, a = face_values(dtype), np.dtype(dtype).type, int(offsets[2])
    faces = [("top_in", (1, 0.5, fv["top_in"])), ("top_out", (1, 0.5, fv["top_out"])), ("bottom_in", (-1, -0.5, fv["bottom_in"])),
             ("bottom_out", (-1, -0.5, fv["bottom_out"])), ("x_out", (fv["x_out"], 0.25, 0.5)), ("x_in", (fv["x_in"], 0.25, 0.5)),
             ("-x_out", (-fv["x_out"], 0.25, -0.5)), ("-x_in", (-fv["x_in"], 0.25, -0.5)), ("y_out", (0.5, fv["y_out"], 0.5)), ("y_in", (0.5, fv["y_in"], 0.5)),
             ("-y_out", (0.5, -fv["y_out"], -0.5)), ("-y_in", (0.5, -fv["y_in"], -0.5))]
    for j, (name, p) in enumerate(faces):
        out[a + j, :3] = [t(v) for v in p]
        special[name] = a + j
    special["thin_along"] = (int(offsets[3]), int(offsets[3]) + 14)
    special["thin_beside"] = (int(offsets[3]) + 14, int(offsets[3]) + 20)
    special["unusable"] = (int(offsets[6]) + 220, int(offsets[6]) + 226)
    keep = np.ones(len(out), bool)
    keep[int(offsets[6]):int(offsets[6]) + 60:3] = False          # a third of the twin box's rows
    keep[int(offsets[4]) + 2] = False
    b = np.ascontiguousarray(boxes.astype(dtype))
    pose = numpy_pose(b)
    pose[FRAME["absent"], 6] = (2.0, 0.0)
    return out, offsets, keep, b, pose, special


def _words(B, dtype):
    """Two frames of 100 rows, B present boxes on a lattice away from the rows but the LAST, which holds a cluster of them."""
    rng = np.random.default_rng(4200 + B)
    boxes = np.zeros((2, B, 7))
    for f in range(2):
        j = np.arange(B)
        boxes[f] = np.column_stack((-100 + 12.0 * (j % 16), 30 + 6.0 * (j // 16), np.zeros(B), np.full(B, 4.0), np.full(B, 2.0), np.full(B, 2.0), 0.1 * j))
        boxes[f, B - 1, :3] = (15.0 + f, -20.0, 0.0)
    rows = []
    for f in range(2):
        fill = _fill(rng, 60, dtype)
        fill[:, 1] = -np.abs(fill[:, 1]) - 25                      # south of every box
        rows.append(np.vstack((_around(rng, boxes[f, B - 1], 40, 1.2), fill)))
    return _rows(np.vstack(rows), rng, dtype), np.array([0, 100, 200], np.int64), None, np.ascontiguousarray(boxes.astype(dtype))


RANDOM_B = 40


def _random(dtype):
    """Two frames of about 2000 rows in clusters, boxes of car size centred on rows with random headings, a quarter of the slots absent
    and one present box above every row."""
    rng = np.random.default_rng(4300)
    rows, boxes, counts = [], np.zeros((2, RANDOM_B, 10)), (2000, 1937)
    for f, n in enumerate(counts):
        hubs = np.column_stack((rng.uniform(-70, 70, 25), rng.uniform(-70, 70, 25), rng.uniform(-1, 0, 25)))
        own = hubs[rng.integers(0, 25, n // 2)] + rng.normal(0, 1.2, (n // 2, 3)) * (1, 1, 0.4)
        p = np.vstack((own, _fill(rng, n - n // 2, dtype)))
        pick = rng.integers(0, n // 2, RANDOM_B)
        for b in range(RANDOM_B):
            if b % 4 == 1:
                continue                                           # an absent slot: zeros
            boxes[f, b] = list(p[pick[b]]) + [rng.uniform(3.5, 5), rng.uniform(1.6, 2.1), rng.uniform(1.4, 2), rng.uniform(-math.pi, math.pi), b % 3 + 1,
                                              rng.normal(), rng.normal()]
        boxes[f, 38, :3] = (0, 0, 50)
        rows.append(p)
    return _rows(np.vstack(rows), rng, dtype), np.array([0, counts[0], sum(counts)], np.int64), None, np.ascontiguousarray(boxes.astype(dtype))


WORDS = (1, 64, 65, 256)
CASES = ("constructed",) + tuple(f"words{B}" for B in WORDS) + ("random",)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(name, dtype="float32"):
    """(rows N x 5, offsets, keep or None, boxes (F, B, Cb), pose (F, B, 2): NumPy's but for the one given pose (2, 0)), read-only."""
    if name == "constructed":
        rows, offsets, keep, boxes, pose, _ = _constructed(dtype)
        return _frozen(rows, offsets, keep, boxes, pose)
    rows, offsets, keep, boxes = _random(dtype) if name == "random" else _words(int(name[5:]), dtype)
    return _frozen(rows, offsets, keep, boxes, numpy_pose(boxes))


def special(dtype="float32"):
    return _constructed(dtype)[5]


@functools.lru_cache(maxsize=None)
def expected(name, dtype="float32", given=True):
    """The restatement on a shared input under the case's given pose, or (given=False) under NumPy's pose of every box."""
    rows, offsets, keep, boxes, pose = case(name, dtype)
    e = points_in_boxes(rows, boxes, pose if given else numpy_pose(boxes), keep, offsets)
    _frozen(*e.values())
    return e
