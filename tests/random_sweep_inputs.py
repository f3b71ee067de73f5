"""Seeded random configurations of the ten point stages and their expected outputs: the CROSS PRODUCT that the hand-built cases of the
stages' own test files never run -- frame sizes on the kernels' borders, a keep mask, the dtype, num_features, the input form, out= and
the optional outputs, all drawn together.  Pure NumPy; the expected outputs come from the stages' restatements (tests/*_reference.py),
which are exact, so every coordinate follows the convention of fps_reference.STEP: a multiple of 2^-10 (or of a coarser step, which makes
exact ties and rows on faces frequent), no subnormal product.  Nothing here imports the package's native code.

configs(stage, dtype) is a tuple of read-only dicts, config i seeded by [2026, crc32(stage), dtype == "float64", i] -- (stage, dtype, i)
names a configuration on any machine:

  rows, offsets, keep     the batch as the restatement takes it (keep: a bool array or None); for the form "padded" the rows ARE the
                          F x N x 5 tensor, flattened: every frame N rows long, NaN rows behind its own, keep False on them
  sizes                   the rows every frame really has (= diff(offsets) but for "padded")
  form                    "batch" (DeviceBatch), "list" (per-frame tensors) or "padded" (one F x N x 5 tensor)
  keep_kind, keep_form    how the mask was drawn (KEEP_KINDS) and how it is handed over ("bool", "uint8", "list")
  out                     whether the call gets out= pre-filled with 0x7f bytes
  args                    the stage's arguments, arrays among them (centres, boxes, rois, pose, ring, features)
  flags                   the optional outputs, on or off

What is drawn by position rather than by the generator's stream is what tests/test_random_sweep_inputs.py must find among 24 configs
whatever the stream gives: the border sizes (one per unpadded config, in turn), the empty first frame, the empty last frame, two
empty frames in a row, the keep kinds and the forms (in turn).  Everything else comes from the stream."""
import functools
import math
import zlib

import numpy as np

import ball_reference as qr
import box_reference as br
import dror_reference as dr
import fps_reference as fr
import fps_sectors_reference as sr
import nn_reference as nr
import range_reference as rr
import roiaware_reference as ra
import roipool_reference as rp
import voxel_reference as vr

DTYPES = fr.DTYPES
STAGES = ("dror_keep", "voxelize", "sample_keypoints", "sample_keypoints_sectors", "ball_query", "nearest_keypoints", "range_image",
          "points_in_boxes", "roi_point_pool", "roi_voxel_pool")
N_CONFIGS = 24
MAX_ROWS = 6000
BORDERS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)      # a wave, SG_BLOCK, SG_ROI_RUN, SG_TILE and around them
STEPS = (2.0 ** -10, 2.0 ** -4, 2.0 ** -1)
KEEP_KINDS = ("none", "p0.5", "all_true", "p0.1", "frame_false", "p0.9", "ends_false")
FORMS = ("batch", "padded", "list")                 # config i has FORMS[i % 3]: 16 of 24 are unpadded, one per border size
KEEP_FORMS = ("bool", "uint8", "list")
RANGE = fr.RANGE                                    # (0, -20, -2, 40, 20, 2): the stages that take a range, but for the sectors
CENTRED = (-20.0, -20.0, -2.0, 20.0, 20.0, 2.0)     # every azimuth: the sectors, and the stages without a range
INF_RANGE = (-math.inf,) * 3 + (math.inf,) * 3
RANGE_STAGES = ("voxelize", "sample_keypoints", "sample_keypoints_sectors", "ball_query", "nearest_keypoints", "range_image")
FEATURE_STAGES = ("voxelize", "sample_keypoints", "sample_keypoints_sectors", "ball_query", "range_image", "roi_point_pool")
BAD_KINDS = ("nan", "+inf", "-inf", "far")


# ---- the shared draws ---------------------------------------------------------------------------------------------------------------------
def _pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def _sizes(rng, i, form, keep_kind):
    """The rows of every frame of config i: half from BORDERS, half uniform in 3 .. 1500; by position: border j in the j-th unpadded
    config, an empty first frame (i = 0), an empty last one (i = 2), two empty frames in a row (i = 3), one frame alone (i = 5)."""
    F = 1 if i == 5 else int(rng.integers(1, 7))          # (config 5: a batch of one frame, of a border size)
    if i in (0, 2):
        F = max(F, 2)
    if keep_kind == "frame_false":
        F = max(F, 3)
    if i == 3:
        F = max(F, 4)
    sizes = [int(_pick(rng, BORDERS)) if rng.random() < 0.5 else int(rng.integers(3, 1501)) for _ in range(F)]
    if keep_kind == "frame_false":                   # the frame the mask takes away lies between frames that have rows
        sizes[:3] = [s if s >= 3 else int(rng.integers(3, 1501)) for s in sizes[:3]]
    held = set()
    if i == 0:
        sizes[0] = 0
        held.add(0)
    if i == 2:
        sizes[-1] = 0
        held.add(F - 1)
    if i == 3:
        sizes[1] = sizes[2] = 0
        sizes[0], sizes[3] = max(sizes[0], 3), max(sizes[3], 3)
        held.update((1, 2))
    if form != "padded":
        j = (i - (i + 1) // 3) % len(BORDERS)         # the unpadded configs before this one
        free = [f for f in range(F) if f not in held and not (keep_kind == "frame_false" and f < 3)]
        f = free[int(rng.integers(0, len(free)))] if free else None
        if f is None:
            sizes.append(BORDERS[j])
            f = len(sizes) - 1
        else:
            sizes[f] = BORDERS[j]
        held.add(f)
    F = len(sizes)
    cap = MAX_ROWS // F if form == "padded" else None
    while (cap is not None and max(sizes) > cap) or (cap is None and sum(sizes) > MAX_ROWS):
        big = max((f for f in range(F) if f not in held), key=lambda f: sizes[f], default=None)
        if big is None:
            break
        sizes[big] = int(rng.integers(3, max(4, min(sizes[big], cap or sizes[big]) // 2 + 1)))
    if not sum(sizes):                                # (no config is a batch without a row: that is a refusal-side case of its own)
        sizes[0 if i != 0 else 1] = int(rng.integers(3, 200))
    return sizes


def _lattice(rng, n, box, step):
    """n x 3 float64: random multiples of `step` in box = (x0, y0, z0, x1, y1, z1), both ends possible."""
    lo = np.ceil(np.asarray(box[:3], np.float64) / step).astype(np.int64)
    hi = np.floor(np.asarray(box[3:], np.float64) / step).astype(np.int64)
    return rng.integers(lo, hi + 1, (n, 3)).astype(np.float64) * step


def _grown(box, share=0.1):
    lo, hi = np.asarray(box[:3], np.float64), np.asarray(box[3:], np.float64)
    return tuple(lo - share * (hi - lo)) + tuple(hi + share * (hi - lo))


def _cluster(rng, box, step):
    """A part of `box` an eighth as long and as wide about a lattice point of it: a frame drawn there is 64 times as dense -- long cell
    lists, full voxels, contested pixels, balls and rois with many rows."""
    c = _lattice(rng, 1, box, step)[0]
    half = (np.asarray(box[3:]) - np.asarray(box[:3])) / 16
    lo, hi = np.maximum(c - half, box[:3]), np.minimum(c + half, box[3:])
    return (lo[0], lo[1], box[2], hi[0], hi[1], box[5])


def _frame(rng, n, box, step, dtype, unusable=0.03):
    """n rows of one frame: lattice points, a tenth of them copies of other rows' coordinates, `unusable` of them NaN, +-inf or beyond
    1e6 in one coordinate; the intensity and the channel of fps_reference._columns."""
    xyz = _lattice(rng, n, box, step)
    if n > 1:
        twin = np.flatnonzero(rng.random(n) < 0.1)
        xyz[twin] = xyz[rng.integers(0, n, len(twin))]
    for r in np.flatnonzero(rng.random(n) < unusable):
        kind = _pick(rng, BAD_KINDS)
        xyz[r, int(rng.integers(0, 3))] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "far": (1e6 + 1.0) * (1 if r % 2 else -1)}[kind]
    return fr._columns(xyz, rng, dtype)


def _keep(rng, kind, sizes):
    """The mask over the REAL rows of every frame, as a list of bool arrays (None for "none")."""
    if kind == "none":
        return None
    if kind.startswith("p"):
        return [rng.random(n) < float(kind[1:]) for n in sizes]
    keep = [np.ones(n, bool) for n in sizes]
    if kind == "frame_false":
        keep[1][:] = False                            # (frames 0 and 2 have rows: _sizes)
    if kind == "ends_false":
        at = -1 if rng.random() < 0.5 else 0
        for k in keep:
            if len(k):
                k[at] = False
    return keep


def _batch(rng, i, dtype, box, step=None):
    """The draws every stage shares: the frames, the mask, the forms."""
    form, keep_kind = FORMS[i % 3], KEEP_KINDS[i % 7]
    sizes = _sizes(rng, i, form, keep_kind)
    step = _pick(rng, STEPS) if step is None else step
    frames = [_frame(rng, n, _cluster(rng, _grown(box), step) if rng.random() < 0.4 else _grown(box), step, dtype) for n in sizes]
    keep = _keep(rng, keep_kind, sizes)
    F = len(sizes)
    if form == "padded":
        N = max(sizes)
        rows = np.full((F, N, 5), np.nan, dtype)
        mask = np.zeros((F, N), bool)
        for f, p in enumerate(frames):
            rows[f, :len(p)] = p
            mask[f, :len(p)] = True if keep is None else keep[f]
        rows, offsets = rows.reshape(-1, 5), np.arange(F + 1, dtype=np.int64) * N
        keep = None if keep is None else mask.reshape(-1)
    else:
        rows = np.ascontiguousarray(np.concatenate(frames)) if F > 1 else frames[0]
        offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        keep = None if keep is None else np.concatenate(keep)
    return dict(rows=np.ascontiguousarray(rows), offsets=offsets, keep=keep, sizes=tuple(sizes), form=form, keep_kind=keep_kind,
                keep_form=KEEP_FORMS[(i // 3 + i) % 3], out=bool((i // 2 + i // 7) % 2), step=step)


def _on(rng):
    return bool(rng.random() < 0.5)


def _frame_rows(c, f):
    """The real rows of frame f of a batch drawn by _batch."""
    a = int(c["offsets"][f])
    return c["rows"][a:a + c["sizes"][f]]


def _centres(rng, c, K, Cq, box, dtype):
    """(F, K, Cq): about half of a frame's centres are rows of it (where it has some), the others lattice points; one in twelve is NaN or
    beyond 1e6."""
    F = len(c["sizes"])
    out = np.zeros((F, K, 5))
    for f in range(F):
        out[f, :, :3] = _lattice(rng, K, _grown(box), c["step"])
        own = _frame_rows(c, f)
        if len(own):
            at = np.flatnonzero(rng.random(K) < 0.5)
            out[f, at] = own[rng.integers(0, len(own), len(at))].astype(np.float64)
        for k in np.flatnonzero(rng.random(K) < 1 / 12):
            out[f, k, int(rng.integers(0, 3))] = np.nan if rng.random() < 0.5 else -1e7
    return np.ascontiguousarray(out[:, :, :Cq].astype(dtype))


def _boxes(rng, F, B, Cb, dtype, step, big=0.0, absent=0.15, far=0.0):
    """(F, B, Cb) boxes about CENTRED: car and truck sizes, headings multiples of pi / 8 or random; `absent` of them zero rows, a zero
    size or a NaN; `far` of them beyond every row (empty); with `big`, box 0 of a share of the frames holds the whole cloud."""
    b = np.zeros((F, B, 10))
    b[..., :3] = _lattice(rng, F * B, CENTRED, step).reshape(F, B, 3)
    b[..., 3] = rng.integers(2, 17, (F, B)) * 0.5
    b[..., 4] = rng.integers(2, 9, (F, B)) * 0.5
    b[..., 5] = rng.integers(2, 7, (F, B)) * 0.5
    eighth = rng.random((F, B)) < 0.5
    b[..., 6] = np.where(eighth, rng.integers(-8, 9, (F, B)) * (np.pi / 8), rng.uniform(-7.0, 7.0, (F, B)))
    b[..., 7] = rng.integers(1, 4, (F, B))
    b[..., 8:] = rng.uniform(-3, 3, (F, B, 2))
    b[rng.random((F, B)) < far, :2] += 200.0
    for f in range(F):
        if f == 0 and big or rng.random() < big:
            b[f, 0, :7] = (0.0, 0.0, 0.0, 60.0, 60.0, 8.0, b[f, 0, 6])
        for m in np.flatnonzero(rng.random(B) < absent):
            kind = int(rng.integers(0, 3))
            if kind == 0:
                b[f, m] = 0.0
            elif kind == 1:
                b[f, m, 3 + int(rng.integers(0, 3))] = 0.0
            else:
                b[f, m, int(rng.integers(0, 7))] = np.nan
    return np.ascontiguousarray(b[..., :Cb].astype(dtype))


def _rows_on_faces(rng, c, boxes, dtype, per_frame=12):
    """Overwrite a few real rows of every frame with points ON a face of a present box of the frame (box_reference.world; rounded to the
    rows' dtype, so they fall on either side or on it) and with points at its centre."""
    rows = c["rows"]
    pose = br.numpy_pose(boxes)
    ok = br.present(boxes, pose)
    for f, n in enumerate(c["sizes"]):
        good = np.flatnonzero(ok[f])
        if not n or not len(good):
            continue
        a = int(c["offsets"][f])
        for r in rng.integers(0, n, min(per_frame, n)):
            box = boxes[f, int(_pick(rng, good))].astype(np.float64)
            local = rng.uniform(-0.5, 0.5, 3) * box[3:6]
            axis = int(rng.integers(0, 4))
            if axis < 3:
                local[axis] = (0.5 if rng.random() < 0.5 else -0.5) * box[3 + axis]
            else:
                local[:] = 0.0
            rows[a + r, :3] = br.world(box, local)[0].astype(dtype)


# ---- the stages' own draws ------------------------------------------------------------------------------------------------------------------
def _dror(rng, i, dtype):
    c = _batch(rng, i, dtype, CENTRED)
    alpha, beta = _pick(rng, ((0.45, 3), (0.16, 3), (2.0, 5), (2.8, 5), (0.45, 1), (14.3239, 1)))      # c in (0, 0.25]: 14.3239 pi / 180 = 0.249999...
    c["args"] = dict(alpha=alpha, beta=beta, sr_min=_pick(rng, (0.0, 0.04, 0.5, 2.0)), k_min=_pick(rng, (0, 1, 3, 1000)))
    c["flags"] = dict(neighbours=_on(rng))
    return c


def _voxelize(rng, i, dtype):
    c = _batch(rng, i, dtype, RANGE)
    size = _pick(rng, ((40.0, 40.0, 4.0), (8.0, 8.0, 4.0), (2.0, 2.0, 2.0), (1.0, 1.0, 2.0), (1.6, 1.6, 4.0), (0.5, 8.0, 1.0)))      # 1 .. 3200 cells
    ok, cell = vr.cells(c["rows"], RANGE, size)
    if c["keep"] is not None:
        ok = ok & c["keep"]
    opened = max([len(np.unique(cell[a:b][ok[a:b]], axis=0)) for a, b in zip(c["offsets"][:-1], c["offsets"][1:])] + [1])
    V = _pick(rng, (max(1, opened // 2), opened, opened + 5))          # below, at and above the cells the fullest frame opens
    c["args"] = dict(range=RANGE, voxel_size=size, max_points=_pick(rng, (1, 2, 5, 32)), max_voxels=int(V), num_features=_pick(rng, (3, 4, 5)))
    c["flags"] = dict(voxel_of=_on(rng))
    return c


def _usable_of_a_frame(rng, c, rng6):
    ok = fr.usable_rows(c["rows"], rng6, c["keep"])
    per = [int(ok[a:b].sum()) for a, b in zip(c["offsets"][:-1], c["offsets"][1:])]
    some = [m for m in per if 0 < m <= 400]
    return _pick(rng, some) if some else None


def _fps(rng, i, dtype):
    c = _batch(rng, i, dtype, RANGE)
    rng6 = _pick(rng, (RANGE, RANGE, None))
    m = _usable_of_a_frame(rng, c, rng6)
    K = _pick(rng, (1, 64, 257) if m is None else (1, max(m - 1, 1), m, m + 1, 64, 257))      # around the usable rows of one of the frames
    c["args"] = dict(n_samples=int(K), range=rng6, num_features=_pick(rng, (3, 4, 5)))
    c["flags"] = dict(dist=_on(rng))
    return c


def _sectors(rng, i, dtype):
    c = _batch(rng, i, dtype, CENTRED)
    F = len(c["sizes"])
    rois = _boxes(rng, F, _pick(rng, (1, 3, 8)), _pick(rng, (7, 8, 10)), dtype, c["step"], absent=0.25) if rng.random() < 0.6 else None
    c["args"] = dict(n_samples=_pick(rng, (1, 16, 64, 257)), sectors=_pick(rng, (1, 2, 5, 6, 8)), range=_pick(rng, (CENTRED, CENTRED, None)),
                     num_features=_pick(rng, (3, 4, 5)), rois=rois, roi_margin=_pick(rng, (0.0, 1.0, 1.6)))
    c["flags"] = dict(dist=_on(rng), sector_of=_on(rng))
    return c


def _ball(rng, i, dtype):
    c = _batch(rng, i, dtype, RANGE)
    R = int(rng.integers(1, 4))
    c["args"] = dict(centres=_centres(rng, c, _pick(rng, (1, 7, 64, 130)), _pick(rng, (3, 4, 5)), RANGE, dtype),
                     radii=tuple(_pick(rng, (0.5, 1.0, 2.0, 4.0, 0.3)) for _ in range(R)), samples=tuple(_pick(rng, (1, 16, 33)) for _ in range(R)),
                     range=_pick(rng, (RANGE, RANGE, None)), num_features=_pick(rng, (3, 4, 5)))
    c["flags"] = dict(points=_on(rng))
    return c


def _nearest(rng, i, dtype):
    c = _batch(rng, i, dtype, RANGE)
    c["args"] = dict(centres=_centres(rng, c, _pick(rng, (1, 2, 3, 64, 65, 300)), _pick(rng, (3, 4, 5)), RANGE, dtype), k=1 + i % nr.MAX_K,
                     range=_pick(rng, (RANGE, RANGE, None)))
    c["flags"] = dict(weight=_on(rng))
    return c


def _range_image(rng, i, dtype):
    c = _batch(rng, i, dtype, CENTRED)
    H, W = _pick(rng, rr.SHAPES) if rng.random() < 0.5 else (int(rng.integers(2, 41)), int(rng.integers(2, 201)))
    ring = np.ascontiguousarray(np.nan_to_num(c["rows"][:, 4], nan=0.0).astype(np.int32)) if _on(rng) else None      # 0 .. 63: beyond a low image
    limits = _pick(rng, (rr.NO_LIMITS, (2.0, 25.0), (0.0, 10.5), (2.0, 2.0 + 2.0 ** -40)))      # the last: lo < hi, and T(lo) = T(hi) in float32
    c["args"] = dict(height=H, width=W, fov=_pick(rng, (rr.FOV, (15.0, -15.0), (90.0, -90.0), (2.0, -2.0))), ring=ring, limits=limits,
                     num_features=_pick(rng, (3, 4, 5)))
    c["flags"] = dict(count=_on(rng))
    return c


def _points_in_boxes(rng, i, dtype):
    c = _batch(rng, i, dtype, CENTRED)
    boxes = _boxes(rng, len(c["sizes"]), _pick(rng, (1, 5, 64, 65, 256)), _pick(rng, (7, 8, 9, 10)), dtype, c["step"])
    _rows_on_faces(rng, c, boxes, dtype)
    c["args"] = dict(boxes=boxes, pose=br.numpy_pose(boxes))
    c["flags"] = dict(count=_on(rng), local=_on(rng), pose=_on(rng))
    return c


def _roi_point_pool(rng, i, dtype):
    c = _batch(rng, i, dtype, CENTRED)
    M = _pick(rng, (1, 16, 16, 512))
    S = _pick(rng, (1, 16) if M == 512 else (1, 16, 512))          # (the restatement's cost is M rois, the outputs' size M S)
    rois = _boxes(rng, len(c["sizes"]), M, _pick(rng, (7, 8, 10)), dtype, c["step"], big=0.3, far=0.15)
    _rows_on_faces(rng, c, rois, dtype, per_frame=6)
    c["args"] = dict(rois=rois, pose=br.numpy_pose(rois), n_samples=S, extra_width=_pick(rng, ((0.0, 0.0, 0.0), rp.EW, (0.0, 0.0, 0.25), (100.0, 0.0, 0.0))),
                     num_features=_pick(rng, (3, 4, 5)))
    c["flags"] = dict(points=_on(rng), local=_on(rng), pose=_on(rng))
    return c


def _roi_voxel_pool(rng, i, dtype):
    c = _batch(rng, i, dtype, CENTRED)
    rois = _boxes(rng, len(c["sizes"]), _pick(rng, (1, 4, 12)), _pick(rng, (7, 8, 10)), dtype, c["step"], big=0.3, far=0.15)
    _rows_on_faces(rng, c, rois, dtype, per_frame=6)
    out_size = int(rng.integers(1, 7)) if _on(rng) else tuple(int(v) for v in rng.integers(1, 7, 3))
    Cf = _pick(rng, (None, 1, 5, 8))
    features = None
    if Cf is not None:
        features = rng.normal(0.0, 4.0, (len(c["rows"]), Cf)).astype(np.float32)
        features[rng.random(features.shape) < 0.02] = np.nan
        features[rng.random(features.shape) < 0.02] = -np.inf
        features[rng.random(features.shape) < 0.1] = 2.5          # equal maxima
    c["args"] = dict(rois=rois, pose=br.numpy_pose(rois), out_size=out_size, max_points=_pick(rng, (1, 3, 127)),
                     roi_capacity=_pick(rng, (64, 64, 4096)),      # SG_ROIAWARE_CAP_MIN, below the members of a roi that holds the cloud, and above them
                     features=features, extra_width=_pick(rng, (0.0, ra.EW, (0.0, 0.0, 0.25))))
    c["flags"] = dict(index=_on(rng))
    return c


DRAW = dict(zip(STAGES, (_dror, _voxelize, _fps, _sectors, _ball, _nearest, _range_image, _points_in_boxes, _roi_point_pool, _roi_voxel_pool)))


def _freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, dict):
        for x in v.values():
            _freeze(x)
    return v


@functools.lru_cache(maxsize=None)
def configs(stage, dtype, n=N_CONFIGS):
    out = []
    for i in range(n):
        rng = np.random.default_rng([2026, zlib.crc32(stage.encode()), dtype == "float64", i])
        c = DRAW[stage](rng, i, dtype)
        c.update(stage=stage, dtype=dtype, i=i)
        out.append(_freeze(c))
    return tuple(out)


# ---- the expected outputs -------------------------------------------------------------------------------------------------------------------
KEPT = object()
PER_FRAME = ("centres", "boxes", "rois", "pose")      # the arguments with one entry per frame


def restate(stage, c, keep=KEPT, offsets=KEPT, num_features=KEPT, range=KEPT):
    """The restatement's outputs for config c as a dict of NumPy arrays, named as the fields of the stage's batch object -- with one of the
    drawn dimensions replaced, for tests/test_random_sweep_inputs.py: keep=None, offsets="one frame", num_features=4, range=INF_RANGE."""
    a = dict(c["args"])
    rows = c["rows"]
    keep = c["keep"] if keep is KEPT else keep
    off = c["offsets"]
    if offsets is not KEPT:
        off = np.array([0, len(rows)], np.int64)
        for name in PER_FRAME:
            if a.get(name) is not None:
                a[name] = a[name][:1]
    if num_features is not KEPT:
        a["num_features"] = num_features
    if range is not KEPT:
        if stage == "range_image":
            a["limits"] = rr.NO_LIMITS
        elif stage == "voxelize":                     # (its range is finite by its domain: half as wide again on every side)
            a["range"] = _grown(a["range"], 0.5)
        else:
            a["range"] = range
    if stage == "dror_keep":
        mask, nb, full = dr.dror(rows, a["alpha"], a["beta"], a["k_min"], a["sr_min"], keep, off)
        return dict(keep=mask, neighbours=nb, full_counts=full)
    if stage == "voxelize":
        return vr.voxelize(rows, a["range"], a["voxel_size"], a["max_points"], a["max_voxels"], a["num_features"], keep, off)
    if stage == "sample_keypoints":
        return fr.fps(rows, a["n_samples"], a["range"], a["num_features"], keep, off)
    if stage == "sample_keypoints_sectors":
        return sr.fps_sectors(rows, a["n_samples"], a["sectors"], a["range"], a["num_features"], keep, off, a["rois"], a["roi_margin"])
    if stage == "ball_query":
        return qr.ball_query(rows, a["centres"], a["radii"], a["samples"], a["range"], a["num_features"], keep, off)
    if stage == "nearest_keypoints":
        return nr.nearest(rows, a["centres"], a["k"], a["range"], keep, off)
    if stage == "range_image":
        return rr.project(rows, a["height"], a["width"], a["fov"], a["ring"], a["limits"], a["num_features"], keep, off)
    if stage == "points_in_boxes":
        out = br.points_in_boxes(rows, a["boxes"], a["pose"], keep, off)
        out["pose"] = br.used_pose(a["boxes"], a["pose"])
        return out
    if stage == "roi_point_pool":
        return rp.roi_point_pool(rows, a["rois"], a["pose"], a["n_samples"], a["num_features"], a["extra_width"], keep, off)
    if stage == "roi_voxel_pool":
        ew = np.repeat(np.float64(a["extra_width"]), 3) if np.ndim(a["extra_width"]) == 0 else a["extra_width"]
        return ra.roi_voxel_pool(rows, a["rois"], a["pose"], a["out_size"], a["max_points"], a["roi_capacity"], a["features"], tuple(ew), keep, off)
    raise KeyError(stage)


@functools.lru_cache(maxsize=None)
def _expected(stage, dtype, i):
    return _freeze(restate(stage, configs(stage, dtype)[i]))


def expected(stage, cfg):
    """The restatement of config cfg, computed once per (stage, dtype, i), read-only."""
    return _expected(stage, cfg["dtype"], cfg["i"])


ALWAYS = dict(dror_keep=("keep",), voxelize=("voxels", "coords", "num_points", "voxel_offsets"), sample_keypoints=("index", "points", "usable"),
              sample_keypoints_sectors=("index", "points", "usable", "sector_offsets", "sector_count"), ball_query=("index", "count"),
              nearest_keypoints=("index", "dist2"), range_image=("image", "index", "pixel_of"), points_in_boxes=("box_of",),
              roi_point_pool=("index", "count"), roi_voxel_pool=("roi_count", "count", "pose"))


def fields(stage, cfg):
    """The fields the call of cfg produces: the stage's fixed ones, the optional ones that were drawn on, and the pooled ones with features."""
    more = tuple(name for name, on in cfg["flags"].items() if on)
    if stage == "roi_voxel_pool" and cfg["args"]["features"] is not None:
        more += ("max", "argmax", "avg")
    return ALWAYS[stage] + more
