"""The documented training step as ONE chain of device stages: the outlier filter on the aligned result, voxels,
keypoints, neighbour groups, nearest keypoints, the range image and the box labels under its mask, the ways back from each to the rows,
and a second filter under the mask they give.  compose() is a COMPOSITION of the restatements of the single stages (tests/dror_reference.py,
voxel_reference.py, fps_reference.py, ball_reference.py, nn_reference.py, range_reference.py, box_reference.py): no stage is restated a
second time here, and the ways back are the NumPy indexing the classes of lidar_snow_sim_amd.tensors document.  The batches, boxes and
per-pixel / per-keypoint values of tests/test_chain_reference.py and tests/test_gpu_chain.py are made here too.  No GPU, no conftest;
nothing here imports the package's native code."""
import functools
import hashlib

import numpy as np

import ball_reference as ball
import box_reference as box
import dror_reference as dr
import fps_reference as fps
import nn_reference as nnr
import range_reference as rr
import voxel_reference as vr

DTYPES = ("float32", "float64")
# (alpha, beta, k_min, sr_min).  On a 64 x 128 synthetic sweep (8192 rows, azimuth steps of 2.8 degrees) the viewer's default (0.45, 3, 3)
# keeps no row and (2.0, 5, 8) keeps every row; this setting keeps 5493 and 5509 rows of the sweeps of seeds 1600 and 1601.
DROR = (1.0, 3, 3, 0.04)
PCR = fps.SECOND_RANGE                    # holds 3852 of the 8192 rows of such a sweep
K = 64                                    # keypoints per frame
RADII, SAMPLES = (0.4, 0.8), (16, 16)
NN = 3
H, W = 64, 128                            # the image: one row per laser, one column per azimuth step of the full sweeps
VOXEL = (vr.SECOND[0], vr.SECOND[1], vr.SECOND[2], 4096)
B = 12                                    # boxes per frame, PADDING of them a zero row
PADDING = 5
D = 4                                     # per-keypoint feature columns
MIN_POINTS = 5
FORWARD = (2, 3, 4, 5, 6, 7)              # the stages behind the first filter, by their number in compose()
RECIPE = dict(width=W, seed=2024)

RAGGED_SIZES = (8192, 6144, 1025, 1, 0, 1023)
FULL = (0, 1)                             # the full-size frames of the ragged batch
TRIVIAL = (3, 4, 5)                       # its one-row, empty and all-absent frames
WEATHER_SEEDS = (1600, 1601, 1602)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
CLUSTER = 8                               # rows of a sweep moved into ONE voxel cell: more than max_points, so that the cap decides something


def sweep(seed, dtype="float32"):
    """A 64 x 128 synthetic sweep, channel-major, in which CLUSTER rows of one laser at neighbouring azimuth steps -- ground rows 5 .. 15 m
    ahead -- lie a millimetre apart around the centre of the voxel cell of the first of them.  (At SECOND's 5 cm cells every row of a
    sweep of this size has a voxel of its own: without the cluster no voxel would reach max_points.)"""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    pc = synthetic_sweep(64, W, seed=seed, intensity="lambert").astype(np.float64)
    grid = pc.reshape(64, W, 5)
    c = next(c for c in range(64) if 5.0 < grid[c, 44, 0] < 15.0 and grid[c, 44, 2] < -1.0)
    lo, size = np.asarray(VOXEL[0][:3]), np.asarray(VOXEL[1])
    centre = lo + (np.floor((grid[c, 44, :3] - lo) / size) + 0.5) * size
    for k in range(CLUSTER):
        grid[c, 44 + k, :3] = centre + (k - CLUSTER / 2 + 0.5) * 1e-3
    return np.ascontiguousarray(pc.astype(dtype))


@functools.lru_cache(maxsize=None)
def frames(name, dtype="float32"):
    """(frames, masks) of a batch, read-only.  'ragged': a 64 x 128 sweep; 64 x 96 of one in firing order (the first 96 azimuth steps: the
    sweep's own density, which a sweep of 96 steps around the circle does not have -- the filter keeps a seventh of such a one); the first 1025
    rows of a sweep; one row; no row; and 1023 rows that the mask takes away whole.  3 % of the rows of the two large frames are absent
    as well.  'ragged_reversed': the same frames, last first.  'small': one frame of 1023 rows.  'weather': three 64 x 128 sweeps, every
    row present.  'twins': the first 64 azimuth steps of two sweeps of the same scene geometry (the seed moves the walls only), so that
    rows of one are neighbours of the other's."""
    from lidar_snow_sim_amd.synthetic import firing_order
    if name == "ragged":
        part = np.ascontiguousarray(sweep(1601, dtype).reshape(64, W, 5)[:, :96].reshape(-1, 5))
        fr = [sweep(1600, dtype), firing_order(part, 64, 96), sweep(1602, dtype)[:1025], sweep(1603, dtype)[4000:4001], np.zeros((0, 5), dtype),
              sweep(1604, dtype)[3000:4023]]
        masks = [np.random.default_rng(1700 + f).random(len(p)) < 0.97 if f in FULL else np.ones(len(p), bool) for f, p in enumerate(fr)]
        masks[5] = np.zeros(1023, bool)
    elif name == "ragged_reversed":
        fr, masks = (list(reversed(v)) for v in frames("ragged", dtype))
    elif name == "small":
        fr, masks = [sweep(1605, dtype)[2000:3023]], [np.ones(1023, bool)]
    elif name == "weather":
        fr = [sweep(s, dtype) for s in WEATHER_SEEDS]
        masks = [np.ones(8192, bool) for _ in fr]
    elif name == "twins":
        fr = [np.ascontiguousarray(sweep(s, dtype).reshape(64, W, 5)[:, :64].reshape(-1, 5)) for s in (1600, 1601)]
        masks = [np.ones(4096, bool) for _ in fr]
    else:
        raise KeyError(name)
    fr, masks = [np.ascontiguousarray(p) for p in fr], [np.ascontiguousarray(m) for m in masks]
    for a in fr + masks:
        a.setflags(write=False)
    return tuple(fr), tuple(masks)


def offsets_of(fr):
    return np.concatenate(([0], np.cumsum([len(p) for p in fr]))).astype(np.int64)


def frame_of(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def make_boxes(rows, kept, offsets, seeds):
    """(F, B, 8) boxes in the rows' dtype: per frame B car-sized boxes centred on rows of `kept` (a mask) with seeded headings, the class
    1 .. 3 in column 7 and box PADDING a zero row; a frame with fewer than B such rows has zero rows only.  As the boxes of
    tests/test_gpu_boxes.py::test_synthetic_sweep_behind_the_aligned_call."""
    F = len(offsets) - 1
    boxes = np.zeros((F, B, 8), rows.dtype)
    for f in range(F):
        a, b = int(offsets[f]), int(offsets[f + 1])
        at = a + np.flatnonzero(kept[a:b] & box.usable_rows(rows[a:b]))
        if len(at) < B:
            continue
        rng = np.random.default_rng(seeds[f])
        at = rng.choice(at, B, replace=False)
        boxes[f, :, :3] = rows[at, :3]
        boxes[f, :, 3:6] = np.column_stack((rng.uniform(3.5, 5, B), rng.uniform(1.6, 2.1, B), rng.uniform(1.4, 2, B)))
        boxes[f, :, 6] = rng.uniform(-np.pi, np.pi, B)
        boxes[f, :, 7] = 1 + np.arange(B) % 3
        boxes[f, PADDING] = 0
    return boxes


@functools.lru_cache(maxsize=None)
def batch(name, dtype="float32"):
    """A batch as the tests feed it: frames, masks, offsets, rows and keep0 (concatenated), channel (the INPUT's column 4 as int32), boxes
    centred on rows that the first filter keeps of the INPUT (the augmentation moves few rows, and boxes have to exist before the chain
    is queued) and their NumPy pose.  Read-only."""
    if name == "ragged_reversed":
        fwd = batch("ragged", dtype)
        fr, masks = frames(name, dtype)
        boxes = np.ascontiguousarray(fwd["boxes"][::-1])
    else:
        fr, masks = frames(name, dtype)
        boxes = None
    offsets = offsets_of(fr)
    rows, keep0 = np.ascontiguousarray(np.concatenate(fr)), np.concatenate(masks)
    if boxes is None:
        boxes = make_boxes(rows, first_filter(rows, keep0, offsets), offsets, [1800 + f for f in range(len(fr))])
    out = dict(frames=fr, masks=masks, offsets=offsets, rows=rows, keep0=keep0, channel=np.ascontiguousarray(rows[:, 4].astype(np.int32)), boxes=boxes,
               pose=box.numpy_pose(boxes))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def values(n_frames, dtype="float32", seed=RECIPE["seed"], width=W):
    """What a model would hand back, fixed and seeded: a per-pixel keep map (F, H, W bool, 70 % set), a per-keypoint decision (F, K bool,
    75 % set) and per-keypoint features (F, K, D in the rows' dtype), read-only."""
    rng = np.random.default_rng(seed)
    out = dict(keep_map=rng.random((n_frames, H, width)) < 0.7, flag=rng.random((n_frames, K)) < 0.75,
               feats=np.ascontiguousarray(rng.normal(0.0, 1.0, (n_frames, K, D)).astype(dtype)))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the composition -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=256)
def _dror_frame(xyz_bytes, keep_bytes, dtype):
    """dror_reference.dror of ONE frame (the filter never looks across frames), cached by the frame's bytes: the brute force costs about
    1.5 s per 8192 present rows, and the same frame comes back in several batches."""
    xyz = np.frombuffer(xyz_bytes, dtype).reshape(-1, 3)
    mask, _, _ = dr.dror(xyz, *DROR, keep=np.frombuffer(keep_bytes, bool))
    mask.setflags(write=False)
    return mask


def first_filter(rows, keep, offsets):
    """dror_reference.dror(rows[:, :3], *DROR, keep=keep, offsets=offsets), frame by frame through the cache."""
    keep = np.asarray(keep).astype(bool)
    out = np.zeros(len(rows), bool)
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b > a:
            out[a:b] = _dror_frame(np.ascontiguousarray(rows[a:b, :3]).tobytes(), np.ascontiguousarray(keep[a:b]).tobytes(), rows.dtype.name)
    return out


def compose(rows, keep0, offsets, channel, boxes, pose, recipe=None):
    """The expected bytes of every tensor the chain produces, as a dict of NumPy arrays, from the bytes of an aligned result (rows, keep0),
    the frames' offsets, the input's channel column, the boxes and their pose.  recipe: dict(width=, seed=) of the image and of values()."""
    recipe = dict(RECIPE, **(recipe or {}))
    rows, keep0, offsets = np.asarray(rows), np.asarray(keep0).astype(bool), np.asarray(offsets, np.int64)
    F, n, width = len(offsets) - 1, len(rows), int(recipe["width"])
    out = {}
    # 1. the filter on the aligned result
    K1 = out["K1"] = first_filter(rows, keep0, offsets)
    # 2. voxels
    v = vr.voxelize(rows, *VOXEL, num_features=4, keep=K1, offsets=offsets)
    for name in ("voxels", "coords", "num_points", "voxel_offsets", "voxel_of"):
        out["vox." + name] = v[name]
    # 3. keypoints
    kp = fps.fps(rows, K, PCR, 4, K1, offsets)
    for name in ("index", "points", "usable"):
        out["kp." + name] = kp[name]
    # 4. neighbour groups around them
    nb = ball.ball_query(rows, kp["points"], RADII, SAMPLES, PCR, 4, K1, offsets)
    for name in ("index", "count", "points"):
        out["nb." + name] = nb[name]
    # 5. every row's nearest keypoints
    nn = nnr.nearest(rows, kp["points"], NN, PCR, K1, offsets)
    for name in ("index", "dist2", "weight"):
        out["nn." + name] = nn[name]
    # 6. the range image, image rows by channel
    img = rr.project(rows, H, width, ring=channel, keep=K1, offsets=offsets)
    for name in ("image", "index", "pixel_of"):
        out["img." + name] = img[name]
    # 7. the boxes
    lab = box.points_in_boxes(rows, boxes, pose, K1, offsets)
    for name in ("box_of", "count", "local"):
        out["lab." + name] = lab[name]
    # 8. the ways back: indexing
    val = values(F, rows.dtype.name, recipe["seed"], width)
    frame = frame_of(offsets)
    pix = img["pixel_of"].astype(np.int64)
    to_rows = out["back.to_rows"] = np.where(pix >= 0, val["keep_map"].reshape(-1)[np.maximum(pix, 0)], False)
    flat = np.where(nn["index"] >= 0, nn["index"].astype(np.int64) + frame[:, None] * K, -1)
    nearest = out["back.nearest"] = np.where(flat[:, 0] >= 0, val["flag"].reshape(-1)[np.maximum(flat[:, 0], 0)], False)
    feats = val["feats"].reshape(F * K, D)
    terms = [np.multiply(feats[np.maximum(flat[:, j], 0)], nn["weight"][:, j, None]) for j in range(NN)]      # (the weight of a -1 slot is 0)
    acc = np.zeros((n, D), feats.dtype)                           # a sum from +0 in slot order: a row without a neighbour gets +0, whatever
    for term in terms:                                            # the sign of the features its zero weights multiply
        acc = np.add(acc, term)
    out["back.interpolate"] = acc
    at = np.where(lab["box_of"] >= 0, lab["box_of"].astype(np.int64) + frame * B, -1)
    cls = boxes[:, :, 7].astype(np.int64).reshape(-1)
    out["back.labels"] = np.where(at >= 0, cls[np.maximum(at, 0)], 0)
    out["back.keep_boxes"] = lab["count"] >= MIN_POINTS
    rows_in = out["back.rows_in"] = lab["box_of"] >= 0
    index = kp["index"]
    out["back.kp_labels"] = np.where(index >= 0, lab["box_of"][np.maximum(index, 0)], -1).astype(np.int32)
    # 9. the second filter: the objects' rows, and what the first filter, the image's verdict and the keypoints' verdict all leave
    out["K2"] = first_filter(rows, rows_in | (K1 & to_rows & nearest), offsets)
    for a in out.values():
        a.setflags(write=False)
    return out


_CACHE = {}


def expected(rows, keep0, offsets, channel, boxes, pose, recipe=None):
    """compose(), cached by the bytes of its inputs; the result is shared and read-only."""
    h = hashlib.sha1()
    for a in (rows, np.asarray(keep0).astype(bool), np.asarray(offsets, np.int64), channel, boxes, pose):
        a = np.ascontiguousarray(a)
        h.update(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes())
    key = (h.digest(), tuple(sorted(dict(RECIPE, **(recipe or {})).items())))
    if key not in _CACHE:
        _CACHE[key] = compose(rows, keep0, offsets, channel, boxes, pose, recipe)
    return _CACHE[key]


def expected_of(name, dtype="float32"):
    """expected() of a batch as it is made here: the chain on the UN-augmented rows under the batch's own mask."""
    b = batch(name, dtype)
    return expected(b["rows"], b["keep0"], b["offsets"], b["channel"], b["boxes"], b["pose"])


# ---- the conditions that keep a comparison against compose() from being vacuous --------------------------------------------------------------
def conditions(e, offsets, boxes, full):
    """The counts that say a chain was exercised on the frames `full`, as a dict per frame; check() asserts them.  Used on the
    un-augmented batches by tests/test_chain_reference.py and on the augmented rows, at run time, by tests/test_gpu_chain.py.
    `rescued`: rows that the image's or the keypoints' verdict cleared and that the second filter keeps because they lie in a box (the
    boxes are labelled under the first filter's mask, so rows_in never holds a row which that filter dropped)."""
    out = {}
    for f in full:
        a, b = int(offsets[f]), int(offsets[f + 1])
        va, vb = int(e["vox.voxel_offsets"][f]), int(e["vox.voxel_offsets"][f + 1])
        num = e["vox.num_points"][va:vb]
        counts = e["nb.count"][f]
        present = box.present(boxes[f], box.numpy_pose(boxes[f]))
        K1, K2 = e["K1"][a:b], e["K2"][a:b]
        out[f] = dict(rows=b - a, K1=int(K1.sum()), usable=int(e["kp.usable"][f]), voxels=vb - va, full_voxels=int((num == VOXEL[2]).sum()),
                      short_voxels=int((num < VOXEL[2]).sum()), balls_below=int((counts < SAMPLES[0]).sum()), balls_above=int((counts > SAMPLES[0]).sum()),
                      to_rows=(int((K1 & e["back.to_rows"][a:b]).sum()), int((K1 & ~e["back.to_rows"][a:b]).sum())),
                      nearest=(int((K1 & e["back.nearest"][a:b]).sum()), int((K1 & ~e["back.nearest"][a:b]).sum())),
                      boxes=int(present.sum()), box_min=int(e["lab.count"][f][present].min()) if present.any() else 0,
                      box_max=int(e["lab.count"][f].max()), K2=int(K2.sum()), K2_differs=int((K1 != K2).sum()),
                      rescued=int((e["back.rows_in"][a:b] & K2 & ~(e["back.to_rows"][a:b] & e["back.nearest"][a:b])).sum()))
    return out


def check(cond):
    for f, c in cond.items():
        assert 0.25 * c["rows"] <= c["K1"] <= 0.90 * c["rows"], (f, c)
        assert c["usable"] >= 1000, (f, c)
        assert c["full_voxels"] >= 1 and c["short_voxels"] >= 1, (f, c)
        assert c["balls_below"] >= 1 and c["balls_above"] >= 1, (f, c)
        assert min(c["to_rows"]) >= 1 and min(c["nearest"]) >= 1, (f, c)
        assert c["boxes"] == B - 1 and c["box_min"] >= 1 and c["box_max"] >= MIN_POINTS, (f, c)
        assert c["K2_differs"] >= 1, (f, c)
        assert c["rescued"] >= 1, (f, c)
