"""Centre heatmap targets (snowgpu_assign_centers_device) restated from the definition in include/snowgpu.h as sequential NumPy: one gt
after the other in ascending number, float64 scalars, every operation rounded on its own, the Gaussian of a gt as one patch that is
maximum-ed into its class's map.  Nothing here touches a GPU, and this module is no conftest: the tests import it by name.  The named
cases the GPU tests run live here too, so that tests/test_centers_reference.py can check on any machine that each of them decides
something."""
from functools import lru_cache

import numpy as np

from anchors_reference import gt_class           # presence: assign_anchors' rule

DTYPES = ("float32", "float64")
FIELDS = ("heatmap", "gt_index", "ind", "mask", "offset", "radius", "count", "state")
RADIUS_MAX = 512
TILE_W, TILE_H = 64, 16                          # a tile of k_center_heat (csrc/sg_centers.h)
ABSENT, DRAWN, DROPPED, NO_SLOT = 0, 1, 2, 3
F64 = np.float64


def roots(h, w, o):
    """pcdet's three roots, in the header's order and parenthesisation."""
    h, w, o = F64(h), F64(w), F64(o)
    with np.errstate(all="ignore"):
        b1 = h + w
        c1 = w * h * (1 - o) / (1 + o)
        r1 = (b1 + np.sqrt(b1 * b1 - 4 * c1)) / 2
        b2 = 2 * (h + w)
        c2 = (1 - o) * w * h
        r2 = (b2 + np.sqrt(b2 * b2 - 16 * c2)) / 2
        b3 = -2 * o * (h + w)
        c3 = (o - 1) * w * h
        r3 = (b3 + np.sqrt(b3 * b3 - 16 * o * c3)) / 2
    return r1, r2, r3


def smallest_root(h, w, o):
    r1, r2, r3 = roots(h, w, o)
    m = r1
    if r2 < m:
        m = r2
    if r3 < m:
        m = r3
    return m


def radius_of(h, w, o, min_radius):
    m = smallest_root(h, w, o)
    if not m >= min_radius:
        return int(min_radius)
    return RADIUS_MAX if m >= RADIUS_MAX else int(m)


def pixel(coord, size):
    """(ci, offset) of a coordinate on an axis of `size` pixels."""
    c = coord if coord > 0 else F64(0.0)
    c = c if c < size - 0.5 else F64(size - 0.5)
    ci = int(c)
    return ci, c - ci


def gaussian(r, den, ex, ey):
    """float32(exp(-(ex ex + ey ey) / den)) on the grid of the integer offsets ey x ex."""
    s = (ey.astype(np.int64) ** 2)[:, None] + (ex.astype(np.int64) ** 2)[None, :]
    return np.exp(np.divide(np.negative(s.astype(F64)), den)).astype(np.float32)


def assign(gt_boxes, point_cloud_range, voxel_size, stride, feature_map_size, n_classes=3, class_head=None, max_objs=500, gaussian_overlap=0.1,
           min_radius=2, outside="clamp"):
    """The outputs of the entry as a dict of arrays (FIELDS), and beside them `coord` (F, B, 2 float64), `root` (F, B float64: the smallest
    root before it is truncated), `owner` and `first` (F, NC, H, W int32: the gt that gave the pixel its value -- the earliest of equal
    ones -- and the first drawn gt whose patch holds the pixel, -1 without one) and `covered` (F, NC, H, W int32: the patches on a pixel)."""
    gt = np.asarray(gt_boxes)
    F, B, Cg = gt.shape
    W, H = (int(v) for v in feature_map_size)
    NC, M = int(n_classes), int(max_objs)
    heads = [0] * NC if class_head is None else [int(h) for h in class_head]
    NH = max(heads) + 1
    x0, y0, vx, vy, st, o = F64(point_cloud_range[0]), F64(point_cloud_range[1]), F64(voxel_size[0]), F64(voxel_size[1]), F64(stride), float(gaussian_overlap)
    assert outside in ("clamp", "drop") and len(heads) == NC and 1 <= M <= 512 and 0 <= min_radius <= RADIUS_MAX
    heat = np.zeros((F, NC, H, W), np.float32)
    gt_index, ind, mask = np.full((F, NH, M), -1, np.int32), np.zeros((F, NH, M), np.int32), np.zeros((F, NH, M), np.uint8)
    offset, radius = np.zeros((F, NH, M, 2), gt.dtype), np.zeros((F, NH, M), np.int32)
    count, state = np.zeros((F, NH), np.int32), np.zeros((F, B), np.uint8)
    coord, root = np.full((F, B, 2), np.nan), np.full((F, B), np.nan)
    owner, first, covered = np.full((F, NC, H, W), -1, np.int32), np.full((F, NC, H, W), -1, np.int32), np.zeros((F, NC, H, W), np.int32)
    for f in range(F):
        cls = gt_class(gt[f], NC)
        taken = [0] * NH
        for g in range(B):
            c = int(cls[g])
            if c == 0:
                continue                                                                  # state 0
            x, y, dx, dy = (F64(gt[f, g, j]) for j in (0, 1, 3, 4))
            cx, cy = ((x - x0) / vx) / st, ((y - y0) / vy) / st
            coord[f, g] = (cx, cy)
            if outside == "drop" and not (0 <= cx < W and 0 <= cy < H):
                state[f, g] = DROPPED
                continue
            (cix, ox), (ciy, oy) = pixel(cx, W), pixel(cy, H)
            h, w = (dx / vx) / st, (dy / vy) / st
            root[f, g] = smallest_root(h, w, o)
            r = radius_of(h, w, o, min_radius)
            head = heads[c - 1]
            slot, taken[head] = taken[head], taken[head] + 1
            if slot >= M:
                state[f, g] = NO_SLOT
                continue
            state[f, g] = DRAWN
            gt_index[f, head, slot], ind[f, head, slot], mask[f, head, slot], radius[f, head, slot] = g, ciy * W + cix, 1, r
            offset[f, head, slot] = (ox, oy)                                              # (rounded once to the boxes' dtype)
            d = F64(2 * r + 1)
            sigma = d / 6
            den = 2 * sigma * sigma
            xa, xb, ya, yb = max(cix - r, 0), min(cix + r, W - 1), max(ciy - r, 0), min(ciy + r, H - 1)
            v = gaussian(r, den, np.arange(xa, xb + 1) - cix, np.arange(ya, yb + 1) - ciy)
            at = (f, c - 1, slice(ya, yb + 1), slice(xa, xb + 1))
            owner[at] = np.where(v > heat[at], g, owner[at])
            first[at] = np.where(first[at] < 0, g, first[at])
            covered[at] += 1
            heat[at] = np.maximum(heat[at], v)
        count[f] = [min(n, M) for n in taken]
    return dict(heatmap=heat, gt_index=gt_index, ind=ind, mask=mask, offset=offset, radius=radius, count=count, state=state, coord=coord, root=root,
                owner=owner, first=first, covered=covered)


def target_boxes(e, gt_boxes):
    """CenterTargetBatch.target_boxes in NumPy, float64 throughout: (F, NH, M, Cg)."""
    gt = np.asarray(gt_boxes).astype(F64)
    F, NH, M = e["gt_index"].shape
    out = np.zeros((F, NH, M, gt.shape[2]))
    for f, h, m in zip(*np.nonzero(e["gt_index"] >= 0)):
        b = gt[f, e["gt_index"][f, h, m]]
        out[f, h, m] = np.concatenate((e["offset"][f, h, m].astype(F64), b[2:3], np.log(b[3:6]), [np.cos(b[6]), np.sin(b[6])], b[8:]))
    return out


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------------------
def box(cx, cy, dx=1.0, dy=1.0, cls=1, h=0.0, cz=0.0, dz=1.5, *extra):
    return [cx, cy, cz, dx, dy, dz, h, cls, *extra]


ZERO = [0.0] * 8


def _case(dtype, gt, W, H, x0=0.0, y0=0.0, vx=1.0, vy=1.0, stride=1, **kw):
    gt = np.array(gt, F64).astype(dtype)
    gt.setflags(write=False)
    out = dict(gt_boxes=gt, point_cloud_range=(x0, y0, -3.0, x0 + W * vx * stride, y0 + H * vy * stride, 1.0), voxel_size=(vx, vy, 0.1), stride=stride,
               feature_map_size=(W, H), n_classes=3, class_head=None, max_objs=500, gaussian_overlap=0.1, min_radius=2, outside="clamp")
    out.update(kw)
    return out


def settings(c):
    """The arguments of assign() and assign_centers() behind the gt boxes."""
    return {k: v for k, v in c.items() if k != "gt_boxes"}


def _by_hand(dtype):
    """An 8 x 8 map; g0 of class 1 at (3.5, 4.25) with the radius 2 of min_radius, g1 of class 2 two pixels to its right."""
    return _case(dtype, [[box(3.5, 4.25), box(5.5, 4.5, cls=2)]], 8, 8, n_classes=2)


BELOW = 2.0 ** -51               # with this x0 = y0 the coordinate of a whole x in [2, 4) is the last double below it
EDGE_W, EDGE_H = 10, 6
EDGE_GTS = dict(whole=0, last_below=1, below_0=2, at_w_half=3, inside_last_half=4, at_w=5, beyond_w=6, at_h=7, below_0_y=8, left=9, right=10, top=11, bottom=12,
                corner=13, far_corner=14)


def _edges(dtype, outside, x0):
    t = np.dtype(dtype).type
    below = lambda v: float(np.nextafter(t(v), t(0)))              # noqa: E731  (the last value of the dtype below v)
    gt = [None] * len(EDGE_GTS)
    for name, b in (("whole", box(3.0, 2.0)), ("last_below", box(below(3.0), below(2.0))), ("below_0", box(-0.5, 1.0)), ("at_w_half", box(9.5, 3.0)),
                    ("inside_last_half", box(9.75, 3.0, cls=2)), ("at_w", box(10.0, 2.0, cls=2)), ("beyond_w", box(12.0, 4.0, cls=3)), ("at_h", box(5.0, 6.0, cls=3)),
                    ("below_0_y", box(6.0, -2.0, cls=2)), ("left", box(0.25, 3.5, cls=3)), ("right", box(9.25, 3.5, cls=3)), ("top", box(4.5, 0.5, cls=2)),
                    ("bottom", box(4.5, 5.25, cls=2)), ("corner", box(0.5, 0.5)), ("far_corner", box(9.5, 5.5, cls=3))):
        gt[EDGE_GTS[name]] = b
    return _case(dtype, [gt], EDGE_W, EDGE_H, x0=x0, y0=x0, outside=outside)


EDGE_NAMES = tuple(f"edges_{o}_{n}" for o in ("clamp", "drop") for n in ("origin0", "below"))


def _tiles(dtype):
    """A map of 70 x 19 -- no multiple of the 64 x 16 tile --: radius-3 patches around the tiles' common corner (64, 16), around (63, 15), one
    that ends on the tile's last column, one in the last column and row of the map, in three classes; one of radius 40 over all four tiles."""
    gt = [[box(64.5, 16.5, 7, 7), box(63.25, 15.75, 7, 7, cls=2), box(60.5, 8.5, 7, 7, cls=3), box(69.5, 18.5, 7, 7, cls=2), box(30.0, 9.0, 93, 93, cls=3),
           box(66.5, 3.5, 7, 7)]]
    return _case(dtype, gt, 70, 19, min_radius=0)


def _whole_map(dtype):
    """A 64 x 64 map under one gt of 4000 x 4000 pixels: its root of about 1730 meets the cap, and the patch of radius 512 covers every pixel."""
    return _case(dtype, [[box(20.5, 40.5, 4000.0, 4000.0), box(3.0, 3.0, cls=2)]], 64, 64)


RADIUS_KS = (3, 7, 20)
RADIUS_DY, RADIUS_V, RADIUS_STRIDE = 30.0, 0.1, 4


def adjacent_dx(k, dtype, dy=RADIUS_DY, v=RADIUS_V, stride=RADIUS_STRIDE, o=0.1):
    """Two adjacent values of the dtype, lo < hi: the smallest root of a box lo x dy is below k, that of hi x dy is not.  By bisection over
    the bit patterns of the positive values, which order as the values do."""
    t, bits = np.dtype(dtype).type, (np.uint32 if dtype == "float32" else np.uint64)

    def root_of(dx):
        return smallest_root((F64(dx) / F64(v)) / F64(stride), (F64(t(dy)) / F64(v)) / F64(stride), o)
    a, b = int(np.array(t(0.01)).view(bits)), int(np.array(t(1000.0)).view(bits))
    value = lambda n: np.array(n, bits).view(t)[()]                # noqa: E731
    assert root_of(value(a)) < k <= root_of(value(b))
    while b - a > 1:
        mid = a + (b - a) // 2
        if root_of(value(mid)) >= k:
            b = mid
        else:
            a = mid
    return value(a), value(b)


def _radius(dtype):
    """Per k two boxes on either side of the truncation; two boxes min_radius takes over (one of them below it by one ulp of the root's
    pair); every gt in a class and place of its own on a 96 x 96 map."""
    gt, at = [], 0
    for k in RADIUS_KS:
        for dx in adjacent_dx(k, dtype):
            gt.append(box(3.0 + 9.5 * (at % 4), 4.0 + 9.0 * (at // 4), float(dx), RADIUS_DY, cls=1 + at % 3))
            at += 1
    gt.append(box(80.0, 70.0, 0.4, 0.4))                           # root about 0.43: min_radius
    gt.append(box(60.0, 80.0, 1.7, 1.7, cls=2))                    # root about 1.8: min_radius
    return _case(dtype, [gt], 96, 96, x0=-2.0, y0=1.0, vx=RADIUS_V, vy=RADIUS_V, stride=RADIUS_STRIDE)


def _overlap(dtype):
    """g0, g1: two patches of radius 3 three pixels apart; g2 a third of radius 2 over both; g3, g4: equal centres, radii 2 and 4 -- the later
    and larger decides every pixel but the centre; g5: the same centre and radius as g4, deciding nothing; g6 of another class on g0."""
    gt = [[box(8.5, 8.5, 7, 7), box(11.5, 8.5, 7, 7), box(10.5, 10.5, 5, 5), box(18.5, 5.5, 5, 5), box(18.25, 5.75, 9.5, 9.5), box(18.0, 5.0, 9.5, 9.5),
           box(8.5, 8.5, 7, 7, cls=2)]]
    return _case(dtype, gt, 24, 16, min_radius=0)


SLOT_HEADS = (0, 1, 0)
SLOTS_M = 4


def _slots(dtype):
    """B = 256, two heads of four slots.  Frame 0: head 0 (classes 1 and 3) overflows -- seven gts, on either side of the lanes 63 / 64,
    127 / 128 and 191 / 192 --, head 1 holds three; absent gts of every kind between them.  Frame 1: no present gt.  Frame 2: head 0 holds
    exactly four, one per wave of the kernel, head 1 four on the waves' last lanes."""
    gt = np.zeros((3, 256, 8))

    def put(f, g, cls):
        gt[f, g] = box(1.5 + g % 13, 1.25 + g % 11, cls=cls)
    for g, cls in ((63, 1), (64, 3), (127, 1), (128, 1), (191, 3), (192, 1), (255, 3), (5, 2), (100, 2), (200, 2)):
        put(0, g, cls)
    for g, (col, v) in zip((3, 62, 65, 126, 129, 190, 193, 254), ((0, np.nan), (7, 0.0), (7, 1.5), (7, 4.0), (3, 0.0), (0, 1.5e6), (7, -1.0), (5, np.inf))):
        put(0, g, 1)
        gt[0, g, col] = v
    gt[1, 10] = box(2.0, 2.0, cls=0)
    gt[1, 70, 7] = 2.0                                             # a class on a zero row: dx = 0
    for g, cls in ((64, 1), (128, 3), (192, 1), (255, 3), (0, 2), (63, 2), (127, 2), (191, 2)):
        put(2, g, cls)
    return _case(dtype, gt, 16, 16, class_head=SLOT_HEADS, max_objs=SLOTS_M)


SWEEP_N = 40
SWEEP_NAMES = tuple(f"sweep_{k:02d}" for k in range(SWEEP_N))


def _sweep(dtype, k):
    rng = np.random.default_rng(7100 + k)
    F, B, Cg = int(rng.integers(1, 4)), int(rng.integers(1, 41)), int(rng.integers(8, 11))
    W, H, NC = int(rng.integers(1, 97)), int(rng.integers(1, 97)), int(rng.integers(1, 5))
    stride = int(rng.choice((1, 2, 4, 8)))
    vx, vy = float(rng.choice((0.05, 0.075, 0.1, 0.16, 0.2))), float(rng.choice((0.05, 0.075, 0.1, 0.16, 0.2)))
    x0, y0 = float(rng.choice((0.0, -51.2, -75.2, -40.0))), float(rng.choice((0.0, -51.2, -75.2, -40.0)))
    sx, sy = W * vx * stride, H * vy * stride
    gt = np.zeros((F, B, Cg))
    gt[..., 0], gt[..., 1] = x0 + rng.uniform(-0.15, 1.15, (F, B)) * sx, y0 + rng.uniform(-0.15, 1.15, (F, B)) * sy
    gt[..., 2] = rng.uniform(-2, 1, (F, B))
    scale = rng.choice((0.02, 0.1, 0.3, 3.0), (F, B, 1), p=(0.2, 0.4, 0.3, 0.1)) * np.array([sx, sy, 1.0])
    gt[..., 3:6] = rng.uniform(0.2, 1.0, (F, B, 3)) * scale
    gt[..., 6] = rng.uniform(-4, 4, (F, B))
    gt[..., 7] = rng.integers(0, NC + 2, (F, B))
    gt[..., 8:] = rng.normal(size=(F, B, Cg - 8))
    kind = rng.integers(0, 12, (F, B))
    gt[kind == 0] = 0.0
    gt[kind == 1, int(rng.integers(0, 7))] = np.nan
    gt[kind == 2, 7] += 0.5
    heads = [int(h) for h in rng.integers(0, int(rng.integers(1, NC + 1)), NC)]
    return _case(dtype, gt, W, H, x0=x0, y0=y0, vx=vx, vy=vy, stride=stride, n_classes=NC, class_head=heads, max_objs=int(rng.integers(1, max(B // 2, 2) + 1)),
                 gaussian_overlap=float(rng.uniform(0.05, 0.9)), min_radius=int(rng.integers(0, 4)), outside=str(rng.choice(("clamp", "drop"))))


_MAKERS = dict(by_hand=_by_hand, tiles=_tiles, whole_map=_whole_map, radius=_radius, overlap=_overlap, slots=_slots)
NAMED = tuple(_MAKERS) + EDGE_NAMES
CASE_NAMES = NAMED + SWEEP_NAMES


@lru_cache(maxsize=None)
def case(name, dtype):
    if name in _MAKERS:
        return _MAKERS[name](dtype)
    if name in EDGE_NAMES:
        _, outside, origin = name.split("_")
        return _edges(dtype, outside, 0.0 if origin == "origin0" else BELOW)
    return _sweep(dtype, SWEEP_NAMES.index(name))


def expected_of(c):
    return assign(c["gt_boxes"], **settings(c))


@lru_cache(maxsize=None)
def expected(name, dtype):
    e = expected_of(case(name, dtype))
    for v in e.values():
        v.setflags(write=False)
    return e
