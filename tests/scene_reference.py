"""Scene transforms (snowgpu_transform_scene_device) restated from their definition in include/snowgpu.h, one frame and one box after the
other: NumPy for presence and box_of (box_reference), the overlap (iou_reference.clip_area) and the float64 arithmetic of rows and
boxes, Python integers for the Philox words (seeded_reference.philox4x32_10).  Every cos / sin is an INPUT -- the gts' pose, (cos, sin) of
every frame's theta and of every try's delta -- as paste_reference takes poses; left out, they are NumPy's of the restated angle.  Nothing
here touches a GPU, and this module is no conftest: the tests import it by name.  The named cases the GPU tests run live here too, so
that tests/test_scene_reference.py can check on any machine that each of them decides something."""
import math
from functools import lru_cache

import numpy as np

import box_reference as br
import iou_reference as ir
from seeded_reference import philox4x32_10

DTYPES = br.DTYPES
TAG = 0x5846524D                    # "XFRM"
FIELDS = ("rows", "keep", "gt_boxes", "world", "state", "tried", "local", "pose", "tries")
STILL, MOVED, BLOCKED = range(3)
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0)
PI = math.pi


def config(flip=("x",), rotation=(-PI / 4, PI / 4), scaling=(0.95, 1.05), local=None):
    """The ranges of a call as the restatement takes them; local: None or dict(translation, rotation, scaling, tries)."""
    if local is not None:
        local = dict(translation=local.get("translation"), rotation=local.get("rotation"), scaling=local.get("scaling"), tries=int(local.get("tries", 8)))
    return dict(flip=tuple(flip or ()), rotation=rotation or None, scaling=scaling or None, local=local)


def tries_of(cfg):
    return cfg["local"]["tries"] if cfg["local"] else 0


def uniform(w, lo, hi):
    """lo + (w 2^-32) (hi - lo) in float64, the difference, the product and the sum rounded each (Python floats are IEEE doubles)."""
    return float(lo) + (float(w) * 2.0 ** -32) * (float(hi) - float(lo))


def world_draw(cfg, seed, step, frame):
    """(flip_x, flip_y, theta, sigma) of a frame: block 0."""
    w = philox4x32_10(seed, step, frame, TAG)
    fx = 1.0 if "x" in cfg["flip"] and w[0] < 2 ** 31 else 0.0
    fy = 1.0 if "y" in cfg["flip"] and w[1] < 2 ** 31 else 0.0
    theta = uniform(w[2], *cfg["rotation"]) if cfg["rotation"] else 0.0
    sigma = uniform(w[3], *cfg["scaling"]) if cfg["scaling"] else 1.0
    return fx, fy, theta, sigma


def try_draw(cfg, seed, step, frame, i, t):
    """(tx, ty, tz, delta, s) of try t of box i: blocks 1 + 2 (i T + t) and the next."""
    loc = cfg["local"]
    blk = 1 + 2 * (i * loc["tries"] + t)
    a, b = philox4x32_10(seed, step, frame, TAG + blk), philox4x32_10(seed, step, frame, TAG + blk + 1)
    tr = loc["translation"]
    txyz = [uniform(a[j], -float(tr[j]), float(tr[j])) if tr is not None else 0.0 for j in range(3)]
    delta = uniform(a[3], *loc["rotation"]) if loc["rotation"] else 0.0
    s = uniform(b[0], *loc["scaling"]) if loc["scaling"] else 1.0
    return (*txyz, delta, s)


def angles(gt_boxes, pose, cfg, seed, step, frames=None):
    """theta (F) and delta (F, B, T; 0 for an absent box) of a call: what the device takes cos / sin of."""
    F, B = gt_boxes.shape[:2]
    T = tries_of(cfg)
    ok = br.present(gt_boxes, pose)
    theta, delta = np.zeros(F), np.zeros((F, B, T))
    for f in range(F):
        key = f if frames is None else frames[f]
        theta[f] = world_draw(cfg, seed, step, key)[2]
        for i in np.flatnonzero(ok[f]):
            for t in range(T):
                delta[f, i, t] = try_draw(cfg, seed, step, key, int(i), t)[3]
    return theta, delta


def _cs(angle):
    return np.stack((np.cos(angle), np.sin(angle)), axis=-1)


def _areas(cand, cand_cs, cur, cur_cs):
    """AREA(candidate t, box j) for T candidates against n boxes: (T, n)."""
    T, n = len(cand), len(cur)
    a, pa = np.repeat(cand, n, axis=0), np.repeat(cand_cs, n, axis=0)
    b, pb = np.tile(cur, (T, 1)), np.tile(cur_cs, (T, 1))
    return ir.clip_area(a, pa, b, pb).reshape(T, n)


def transform_scene(rows, offsets, keep, gt_boxes, pose, cfg, seed, step, world_cs=None, tries_cs=None, box_of=None, frames=None):
    """Every output of the stage as a dict of NumPy arrays.  pose: (F, B, 2) float64, used as it is.  keep: (N) bool or None.  world_cs
    (F, 2) and tries_cs (F, B, T, 2): the cos / sin to use where the part is on (None: NumPy's).  box_of: (N) int32 or None: the
    restatement of points_in_boxes.  frames: the frame numbers that key the draws, 0 .. F - 1 unless given."""
    rows, gt_boxes, offsets = np.asarray(rows), np.asarray(gt_boxes), np.asarray(offsets, np.int64)
    F, B, Cb = gt_boxes.shape
    N, dt, T, loc = len(rows), rows.dtype, tries_of(cfg), cfg["local"]
    assert gt_boxes.dtype == dt and pose.shape == (F, B, 2) and F == len(offsets) - 1
    present = np.ones(N, bool) if keep is None else np.asarray(keep).astype(bool)
    usable = br.usable_rows(rows, present)
    ok = br.present(gt_boxes, pose)
    if world_cs is None or tries_cs is None:
        theta, delta = angles(gt_boxes, pose, cfg, seed, step, frames)
        world_cs = _cs(theta) if world_cs is None else world_cs
        tries_cs = _cs(delta) if tries_cs is None else tries_cs
    if T and box_of is None:
        box_of = br.points_in_boxes(rows, gt_boxes, pose, keep, offsets)["box_of"]
    e = dict(rows=rows.copy(), keep=present.copy(), gt_boxes=gt_boxes.copy(), world=np.zeros((F, 8)), state=np.zeros((F, B), np.int32),
             tried=np.full((F, B), -1, np.int32), local=np.tile(np.array(IDENTITY), (F, B, 1)), pose=np.zeros((F, B, 2)),
             tries=np.tile(np.array(IDENTITY), (F, B, T, 1)))
    for f in range(F):
        key = f if frames is None else frames[f]
        fx, fy, theta, sigma = world_draw(cfg, seed, step, key)
        cw, sw = (float(world_cs[f, 0]), float(world_cs[f, 1])) if cfg["rotation"] else (1.0, 0.0)
        e["world"][f] = (fx, fy, cw, sw, theta, sigma, 0.0, 0.0)
        g = gt_boxes[f, :, :7].astype(np.float64)
        cur, cur_cs, centre0 = g.copy(), pose[f].copy(), g[:, :3].copy()          # the settled records (columns 0 .. 5 and the pose) and the ORIGINAL centres
        cur[:, 6] = 0.0
        here = np.flatnonzero(ok[f])
        for i in (here if T else ()):
            i = int(i)
            rec = e["tries"][f, i]
            for t in range(T):
                tx, ty, tz, d, s = try_draw(cfg, seed, step, key, i, t)
                cd, sd = (float(tries_cs[f, i, t, 0]), float(tries_cs[f, i, t, 1])) if loc["rotation"] else (1.0, 0.0)
                rec[t] = (tx, ty, tz, cd, sd, d, s, 0.0)
            cand = np.zeros((T, 7))
            cand[:, :3] = cur[i, :3] + rec[:, :3]
            cand[:, 3:6] = cur[i, 3:6] * rec[:, 6:7]
            ci, si = cur_cs[i]
            cand_cs = np.stack((ci * rec[:, 3] - si * rec[:, 4], si * rec[:, 3] + ci * rec[:, 4]), axis=-1)
            others = here[here != i]
            hit = (_areas(cand, cand_cs, cur[others], cur_cs[others]) > 0.0).any(axis=1) if len(others) else np.zeros(T, bool)
            rec[:, 7] = hit
            clear = np.flatnonzero(~hit)
            if len(clear):
                t = int(clear[0])
                cur[i], cur_cs[i] = cand[t], cand_cs[t]
                e["state"][f, i], e["tried"][f, i] = MOVED, t
                e["local"][f, i, :7] = rec[t, :7]
            else:
                e["state"][f, i] = BLOCKED
        moved, lc = e["state"][f] == MOVED, e["local"][f]
        # the boxes (absent ones, NaN and all, go through the arithmetic too and are left out at the store)
        old = np.seterr(all="ignore")
        h = np.where(moved, g[:, 6] + lc[:, 5], g[:, 6])
        cx, cy, c, s = cur[:, 0].copy(), cur[:, 1].copy(), cur_cs[:, 0].copy(), cur_cs[:, 1].copy()
        if fx:
            cy, h, s = -cy, -h, -s
        if fy:
            cx, h, c = -cx, -(h + PI), -c
        nx, ny = cx * cw - cy * sw, cx * sw + cy * cw
        h = h + theta
        pc, ps = c * cw - s * sw, s * cw + c * sw
        out = np.column_stack((nx * sigma, ny * sigma, cur[:, 2] * sigma, cur[:, 3] * sigma, cur[:, 4] * sigma, cur[:, 5] * sigma, h))
        e["gt_boxes"][f, here, :7] = out[here].astype(dt)
        e["pose"][f, here] = np.column_stack((pc, ps))[here]
        np.seterr(**old)
        # the rows
        a, b = int(offsets[f]), int(offsets[f + 1])
        u = a + np.flatnonzero(usable[a:b])
        if not len(u):
            continue
        x, y, z = (rows[u, j].astype(np.float64) for j in range(3))
        if T:
            bo = box_of[u].astype(np.int64)
            m = (bo >= 0) & (bo < B)
            m[m] = moved[bo[m]]
            k = bo[m]
            sx, sy, sz = x[m] - centre0[k, 0], y[m] - centre0[k, 1], z[m] - centre0[k, 2]
            rx, ry = sx * lc[k, 3] - sy * lc[k, 4], sx * lc[k, 4] + sy * lc[k, 3]
            x[m] = (rx * lc[k, 6] + centre0[k, 0]) + lc[k, 0]
            y[m] = (ry * lc[k, 6] + centre0[k, 1]) + lc[k, 1]
            z[m] = (sz * lc[k, 6] + centre0[k, 2]) + lc[k, 2]
        if fx:
            y = -y
        if fy:
            x = -x
        nx, ny = x * cw - y * sw, x * sw + y * cw
        e["rows"][u, 0], e["rows"][u, 1], e["rows"][u, 2] = (nx * sigma).astype(dt), (ny * sigma).astype(dt), (z * sigma).astype(dt)
    return e


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
LOCAL = dict(translation=(2.0, 2.0, 0.25), rotation=(-PI / 20, PI / 20), scaling=(0.95, 1.05), tries=4)
LENGTHS = (0, 1, 63, 64, 65, 513)


def _rows_of(rng, xyz, dtype):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.column_stack((xyz, rng.integers(1, 255, len(xyz)), rng.integers(0, 64, len(xyz)))).astype(dtype)


def _finish(frames, keeps, gt, cfg, seed, step, **special):
    rows = np.ascontiguousarray(np.concatenate(frames))
    offsets = np.concatenate(([0], np.cumsum([len(p) for p in frames]))).astype(np.int64)
    gt = np.ascontiguousarray(gt)
    c = dict(rows=rows, offsets=offsets, keep=None if keeps is None else np.ascontiguousarray(np.concatenate(keeps)), gt_boxes=gt,
             pose=np.ascontiguousarray(br.numpy_pose(gt)), cfg=cfg, seed=seed, step=step, **special)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _random(dtype, seed, sizes, B, Cb, cfg, spread=30.0, absent=0.25, gt_absent=0.3):
    """Frames of the given sizes: boxes of car size within +-spread, a share absent (zero rows, one NaN); each frame's rows lie half about
    its boxes, half anywhere; a share of rows absent, some of those NaN / inf, and a present row beyond 1e6."""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    gt = np.zeros((F, B, Cb))
    gt[..., 0:2] = rng.uniform(-spread, spread, (F, B, 2))
    gt[..., 2] = rng.uniform(-1.5, 0.0, (F, B))
    gt[..., 3:6] = rng.uniform((3.0, 1.4, 1.3), (5.0, 2.2, 2.0), (F, B, 3))
    gt[..., 6] = rng.uniform(-7, 7, (F, B))
    gt[..., 7:] = rng.integers(1, 4, (F, B, Cb - 7))
    gt[rng.uniform(size=(F, B)) < gt_absent] = 0
    if B > 2:
        gt[0, 1, 3] = np.nan
    gt = gt.astype(dtype)
    frames, keeps = [], []
    for f, n in enumerate(sizes):
        at = gt[f, rng.integers(0, B, n)].astype(np.float64)
        near = at[:, :3] + rng.uniform(-1.2, 1.2, (n, 3)) * np.where(at[:, 3:6] > 0, at[:, 3:6], 1.0) * 0.5
        far = np.column_stack((rng.uniform(-spread, spread, (n, 2)), rng.uniform(-2, 1, n)))
        rows = _rows_of(rng, np.where(rng.uniform(size=(n, 1)) < 0.5, np.nan_to_num(near), far), dtype)
        keep = rng.uniform(size=n) >= absent
        bad = ~keep & (rng.uniform(size=n) < 0.3)
        rows[bad] = np.where(rng.uniform(size=(int(bad.sum()), 5)) < 0.5, np.nan, np.inf).astype(dtype)
        if n > 10:
            keep[5] = True
            rows[5, 0] = 1e7
        frames.append(rows)
        keeps.append(keep)
    return _finish(frames, keeps, gt, cfg, seed, seed % 5)


# the constructed frame: groups of small boxes 20 m apart, so that no group meets another (translation within +-2 m)
GROUP = dict(free=0, third=1, walled=4, earlier=6, later=8, twins=10, face=12, zero=13, nan=14)
CONSTRUCTED_B = 15
CONSTRUCTED_SEED, CONSTRUCTED_STEP = 7, 4             # (at this step the frame is flipped about both axes)
SMALL = (0.5, 0.5, 1.0)


def _constructed(dtype):
    """One frame, T = 4, every box placed with the draws of (CONSTRUCTED_SEED, CONSTRUCTED_STEP, frame 0) in hand:
      free     box 0 alone at (0, 0): its first try is free;
      third    box 1 at (20, 0); boxes 2 and 3 (later, so at their ORIGINAL places when box 1 is tried) sit on the centres of its tries 0 and 1:
               try 2 is its first free one -- unless it meets them too, which the no-GPU test excludes;
      walled   box 4 at (40, 0) inside box 5, 12 m wide: every try collides; the two overlap, and the rows inside both have box_of 4;
      earlier  box 6 at (60, 0) alone takes try 0 and moves; box 7 is placed so that ITS try 0 lands on box 6's MOVED centre and nowhere near
               its original one: blocked only by an earlier box's moved position;
      later    box 8 at (80, 0); box 9 sits at the centre of box 8's try 0: blocked only by a later box's ORIGINAL position;
      twins    boxes 10 and 11 at (100, 0) and (100.4, 0), 0.5 wide: they overlap in a strip whose rows have box_of 10;
      face     box 12 = a 4 x 2 x 1.5 box at (0, 40) with heading 0 and rows on and just beyond its faces;
      zero, nan   box 13 a zero row, box 14 with a NaN: absent.
    Rows: a cluster in every present box, rows between the groups, absent rows (some NaN, some INSIDE boxes), a present row at 1e7."""
    rng = np.random.default_rng(8100)
    cfg = config(("x", "y"), local=LOCAL)
    G, T = GROUP, LOCAL["tries"]
    draw = lambda i, t: try_draw(cfg, CONSTRUCTED_SEED, CONSTRUCTED_STEP, 0, i, t)          # noqa: E731
    gt = np.zeros((CONSTRUCTED_B, 8))

    def put(i, x, y, dims=SMALL, h=0.0, cls=1.0):
        gt[i] = (x, y, 0.0, *dims, h, cls)

    put(G["free"], 0.0, 0.0, h=0.3)
    put(G["third"], 20.0, 0.0, h=-0.2)
    for k in (0, 1):
        tx, ty = draw(G["third"], k)[:2]
        put(G["third"] + 1 + k, 20.0 + tx, ty, (0.3, 0.3, 1.0))
    put(G["walled"], 40.0, 0.0, h=1.0)
    put(G["walled"] + 1, 40.0, 0.0, (12.0, 12.0, 1.0), cls=2.0)
    put(G["earlier"], 60.0, 0.0)
    ex, ey = draw(G["earlier"], 0)[:2]
    lx, ly = draw(G["earlier"] + 1, 0)[:2]
    put(G["earlier"] + 1, (60.0 + ex) - lx, ey - ly)
    put(G["later"], 80.0, 0.0, h=2.0)
    tx, ty = draw(G["later"], 0)[:2]
    put(G["later"] + 1, 80.0 + tx, ty, (0.3, 0.3, 1.0))
    put(G["twins"], 100.0, 0.0)
    put(G["twins"] + 1, 100.4, 0.0)
    put(G["face"], 0.0, 40.0, (4.0, 2.0, 1.5))
    gt[G["nan"]] = (5.0, 5.0, 0.0, 1.0, np.nan, 1.0, 0.0, 1.0)
    gt = gt.astype(dtype)
    t = np.dtype(dtype).type
    pts, names = [], {}

    def add(name, xyz):
        names[name] = len(pts)
        pts.append([float(t(v)) for v in xyz])

    for i in range(CONSTRUCTED_B):
        if gt[i, 3] > 0 and not np.isnan(gt[i]).any():
            for p in br.world(gt[i].astype(np.float64), rng.uniform(-0.45, 0.45, (6, 3)) * gt[i, 3:6].astype(np.float64)):
                pts.append(p.tolist())
    add("strip", (100.2, 0.0, 0.0))                                        # inside both twins
    add("in_wall_only", (43.0, 3.0, 0.0))                                  # inside box 5 only
    add("in_both_walled", (40.1, 0.1, 0.0))
    add("top_in", (0.5, 40.5, 0.75))
    add("top_out", (0.5, 40.5, float(np.nextafter(t(0.75), t(1.0)))))
    add("x_in", (2.0, 40.0, 0.0))                                          # |lx| = dx / 2 < dx / 2 + 1e-5
    add("x_out", (float(np.nextafter(t(2.0 + 2e-5), t(3.0))), 40.0, 0.0))
    add("unusable", (1e7, 0.0, 0.0))
    add("origin", (0.0, 0.0, 0.0))
    for p in np.column_stack((rng.uniform(-10, 110, 60), rng.uniform(-10, 50, 60), rng.uniform(-1, 1, 60))):
        pts.append(p.tolist())
    scene = _rows_of(rng, pts, dtype)
    n_absent = 24
    n = len(scene) + n_absent
    absent_at = np.sort(rng.choice(n, n_absent, replace=False))
    keep = np.ones(n, bool)
    keep[absent_at] = False
    frame = np.zeros((n, 5), dtype)
    frame[keep] = scene
    frame[absent_at[::3]] = np.nan
    frame[absent_at[1::3]] = _rows_of(rng, [(0.1, 0.1, 0.0)] * len(absent_at[1::3]), dtype)      # absent rows inside box 0: never moved
    frame[absent_at[2::3]] = np.inf
    special = {nm: int(np.flatnonzero(keep)[i]) for nm, i in names.items()}
    special["absent_inside"] = tuple(int(v) for v in absent_at[1::3])
    return _finish([frame], [keep], gt[None], cfg, CONSTRUCTED_SEED, CONSTRUCTED_STEP, special=special)


FLIPS_SEED = 2


def _flips(dtype):
    """Six frames of 20 rows and one box, the world part alone with both axes asked for: every (flip_x, flip_y) pair occurs."""
    return dict(_random(dtype, 8200, (20,) * 6, 1, 7, config(("x", "y")), gt_absent=0.0), seed=FLIPS_SEED, step=0)


CASE_NAMES = ("constructed", "lengths", "b1", "b65", "b256", "flips", "world")
OFF = {                                 # the constructed frame with a part switched off
    "no_flip": dict(flip=()), "flip_x": dict(flip=("x",)), "flip_y": dict(flip=("y",)), "no_rotation": dict(rotation=None), "no_scaling": dict(scaling=None),
    "no_world": dict(flip=(), rotation=None, scaling=None), "no_local": dict(local=None),
    "no_local_translation": dict(local=dict(LOCAL, translation=None)), "no_local_rotation": dict(local=dict(LOCAL, rotation=None)),
    "no_local_scaling": dict(local=dict(LOCAL, scaling=None)), "no_local_part_on": dict(local=dict(tries=2)),
}


@lru_cache(maxsize=None)
def case(name, dtype):
    """dict(rows, offsets, keep, gt_boxes, pose, cfg, seed, step[, special]) of a named case, read-only; the poses are NumPy's."""
    if name == "constructed":
        return _constructed(dtype)
    if name in OFF:
        c = _constructed(dtype)
        return dict(c, cfg=config(**{**dict(flip=c["cfg"]["flip"], rotation=c["cfg"]["rotation"], scaling=c["cfg"]["scaling"], local=c["cfg"]["local"]), **OFF[name]}))
    if name == "lengths":
        return _random(dtype, 8301, LENGTHS, 3, 7, config(("x",), local=LOCAL))
    if name == "b1":
        return _random(dtype, 8302, (150, 90), 1, 8, config(("y",), local=dict(LOCAL, tries=1)), gt_absent=0.0)
    if name == "b65":
        return _random(dtype, 8303, (400, 300), 65, 10, config(("x", "y"), local=dict(LOCAL, tries=16)), spread=25.0)
    if name == "b256":
        return _random(dtype, 8304, (600,), 256, 8, config(("x",), local=LOCAL), spread=60.0)
    if name == "flips":
        return _flips(dtype)
    if name == "world":
        return dict(_random(dtype, 8305, (300, 0, 200), 5, 9, config(("x", "y"))), keep=None)
    raise KeyError(name)


def expected_of(c, **changed):
    """The restatement on a case, with some of its entries replaced."""
    c = {**c, **changed}
    return transform_scene(c["rows"], c["offsets"], c["keep"], c["gt_boxes"], c["pose"], c["cfg"], c["seed"], c["step"], c.get("world_cs"), c.get("tries_cs"),
                           c.get("box_of"), c.get("frames"))


@lru_cache(maxsize=None)
def expected(name, dtype):
    e = expected_of(case(name, dtype))
    for a in e.values():
        a.setflags(write=False)
    return e
