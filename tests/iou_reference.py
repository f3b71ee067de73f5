"""The definition of rotated box IoU and NMS (include/snowgpu.h: snowgpu_boxes_iou_device, snowgpu_nms_device; its C++: csrc/sg_iou.h)
restated in NumPy, an independent method beside it, the shared inputs of tests/test_iou_reference.py and tests/test_gpu_iou.py -- the
cases, which keep every decision away from its threshold, and apart from them the adversarial pair families and the exact ties, which
do not --, and the tolerance between the two methods with its derivation.

The restatement takes the pose as an input.  Behind the pose the definition is separately rounded float64 arithmetic in a fixed order, and
NumPy's element-wise + - * / round each operation on its own: clip_area() keeps the definition's padded vertex list as (P, CAP) arrays and
walks its passes, edges and emits in the definition's order for P pairs at once; area_scalar() is the same text as a plain loop over one
pair, held equal to it on a sample by the tests.  Device and host results are compared with it byte for byte.

THE TOLERANCE between the restatement and the independent method (never used against the device).  eps = 2^-53.  Let R bound the
coordinates that enter either method (centres plus half diagonals) and L the diagonal of a box.
  * A corner or a crossing is a handful of products and sums of numbers no larger than 2 R: the restatement's corner takes 3 roundings in
    world coordinates and 4 more into b's frame, the independent method's 3, a crossing 4 more on operands no larger than what they
    interpolate.  Counting 16 roundings of relative size eps on magnitudes <= 2 R bounds the displacement of ANY vertex of either
    method's polygon by d = 32 eps R -- for a crossing, measured ALONG the edge it moves on this is not bounded (near-parallel edges),
    but the polygon's boundary moves by no more than the edges do: both polygons lie between the intersections of the two boxes shrunk
    and grown by d.
  * The area between those two is at most (perimeter of a + perimeter of b) d <= 4 sqrt(2) L d (a box's perimeter is <= 2 sqrt(2) L).
  * The shoelace sums: at most 8 terms, each a difference of products of coordinates.  The restatement sums in b's frame, where an
    overlapping polygon has |u|, |v| <= L / 2; the independent method sums about the mean of its points, <= L likewise.  9 roundings per
    sum on magnitudes <= L^2: 16 eps L^2 for both together.
  TOL_AREA(R, L) = 4 sqrt(2) L 32 eps R + 16 eps L^2.  For the cases here (|centre| <= 50 m, L <= 8 m: R = 64 m) that is
  1.03e-11 + 1.1e-13 < 1.1e-11 m^2.  (One trial of 20 000 car-sized pairs saw 3.6e-13 m^2.)
  An IoU moves by at most 2 / Amin per unit of area, Amin the smallest footprint dx dy of the case: d iou / d inter = (Aa + Ab) / U^2 with
  U >= max(Aa, Ab); in 3D h (Va + Vb) / U3^2 <= 2 h / (A dz) <= 2 / A.  The quotient and the sums in front of it add a few eps.
  TOL_IOU = 2 TOL_AREA / Amin + 8 eps.
"""
import functools
import math

import numpy as np

from box_reference import BOUND, numpy_pose, present  # noqa: F401  (the presence rule is that of points_in_boxes)

DTYPES = ("float32", "float64")
CAP = 20                                         # 4 -> 6 -> 9 -> 13 -> 19: no input fills it (csrc/sg_iou.h)
EPS_BEV, EPS_3D = 1e-8, 1e-6
MODES = ("bev", "3d")
EPS = 2.0 ** -53


def tol_area(R, L):
    return 4 * math.sqrt(2) * L * 32 * EPS * R + 16 * EPS * L * L


def tol_iou(R, L, amin):
    return 2 * tol_area(R, L) / amin + 8 * EPS


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def corners_in_frame(a, pa, b, pb):
    """(P, 4) u and v: the corners of a (P, 7 float64; pose pa (P, 2)) in the frame of b, in the definition's order."""
    hxa, hya = a[:, 3] * 0.5, a[:, 4] * 0.5
    u, v = np.empty((len(a), 4)), np.empty((len(a), 4))
    for k in range(4):
        lx = hxa if k in (0, 3) else -hxa
        ly = hya if k < 2 else -hya
        x = a[:, 0] + (lx * pa[:, 0] - ly * pa[:, 1])
        y = a[:, 1] + (lx * pa[:, 1] + ly * pa[:, 0])
        sx, sy = x - b[:, 0], y - b[:, 1]
        u[:, k] = sx * pb[:, 0] + sy * pb[:, 1]
        v[:, k] = sy * pb[:, 0] - sx * pb[:, 1]
    return u, v


def clip_area(a, pa, b, pb, return_most=False, boundary_inside=True):
    """area(a, b) of P pairs of PRESENT boxes (P, 7 float64 each, poses (P, 2)): the definition, its slots, its order.  return_most: also the
    largest number of vertices any pass emitted, per pair.  boundary_inside=False is NOT the definition: a point on a clip line counts as
    outside; the families below use it to find the pairs whose area the boundary rule decides."""
    P = len(a)
    ar = np.arange(P)
    u4, v4 = corners_in_frame(a, pa, b, pb)
    pu, pv = np.zeros((P, CAP)), np.zeros((P, CAP))
    pu[:, :4], pv[:, :4] = u4, v4
    n = np.full(P, 4)
    most = np.zeros(P, np.int64)
    hxb, hyb = b[:, 3] * 0.5, b[:, 4] * 0.5
    with np.errstate(all="ignore"):
        for pas in range(4):
            on_v, neg = pas >= 2, bool(pas & 1)
            h = hyb if on_v else hxb
            qu, qv, m = np.zeros((P, CAP)), np.zeros((P, CAP)), np.zeros(P, np.int64)
            for i in range(int(n.max(initial=0))):
                act = i < n
                j = np.where(i + 1 >= n, 0, i + 1)
                iu, iv, ju, jv = pu[:, i], pv[:, i], pu[ar, j], pv[ar, j]
                p_c, p_o, q_c, q_o = (iv, iu, jv, ju) if on_v else (iu, iv, ju, jv)
                dp, dq = (-p_c, -q_c) if neg else (p_c, q_c)
                in_p, in_q = (dp <= h, dq <= h) if boundary_inside else (dp < h, dq < h)
                want = act & in_p
                e1 = np.flatnonzero(want & (m < CAP))
                qu[e1, m[e1]], qv[e1, m[e1]] = iu[e1], iv[e1]
                m[e1] += 1
                want = act & (in_p != in_q)
                t = (h - dp) / (dq - dp)
                o = p_o + t * (q_o - p_o)
                e = -h if neg else h
                e2 = np.flatnonzero(want & (m < CAP))
                nu, nv = (o, e) if on_v else (e, o)
                qu[e2, m[e2]], qv[e2, m[e2]] = nu[e2], nv[e2]
                m[e2] += 1
            pu, pv, n = qu, qv, m
            most = np.maximum(most, m)
        s = np.zeros(P)
        for i in range(int(n.max(initial=0))):
            act = i < n
            j = np.where(i + 1 >= n, 0, i + 1)
            s = np.where(act, s + (pu[:, i] * pv[ar, j] - pu[ar, j] * pv[:, i]), s)
    area = 0.5 * np.abs(s)
    return (area, most) if return_most else area


def area_scalar(a, pa, b, pb):
    """area(a, b) of ONE pair of present boxes as a plain loop over Python floats (IEEE doubles, one rounding per operation)."""
    a, b = [float(x) for x in a[:7]], [float(x) for x in b[:7]]
    ca, sa, cb, sb = float(pa[0]), float(pa[1]), float(pb[0]), float(pb[1])
    hxa, hya, hxb, hyb = a[3] * 0.5, a[4] * 0.5, b[3] * 0.5, b[4] * 0.5
    poly = []
    for k in range(4):
        lx = hxa if k in (0, 3) else -hxa
        ly = hya if k < 2 else -hya
        x, y = a[0] + (lx * ca - ly * sa), a[1] + (lx * sa + ly * ca)
        sx, sy = x - b[0], y - b[1]
        poly.append((sx * cb + sy * sb, sy * cb - sx * sb))
    for pas in range(4):
        axis, neg = pas // 2, bool(pas & 1)
        h = hyb if axis else hxb
        out = []
        for i, p in enumerate(poly):
            q = poly[(i + 1) % len(poly)]
            dp, dq = (-p[axis], -q[axis]) if neg else (p[axis], q[axis])
            in_p, in_q = dp <= h, dq <= h
            if in_p and len(out) < CAP:
                out.append(p)
            if in_p != in_q and len(out) < CAP:
                t = (h - dp) / (dq - dp)
                o = p[1 - axis] + t * (q[1 - axis] - p[1 - axis])
                e = -h if neg else h
                out.append((o, e) if axis else (e, o))
        poly = out
        if not poly:
            return 0.0
    s = 0.0
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        s = s + (p[0] * q[1] - q[0] * p[1])
    return 0.5 * abs(s)


def iou_from_area(inter, a, b, mode):
    """The IoU of P present pairs from their overlap area, float64."""
    Aa, Ab = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    if mode == "bev":
        u = Aa + Ab - inter
        return inter / np.where(u > EPS_BEV, u, EPS_BEV)
    hza, hzb = a[:, 5] * 0.5, b[:, 5] * 0.5
    ta, tb, ba, bb = a[:, 2] + hza, b[:, 2] + hzb, a[:, 2] - hza, b[:, 2] - hzb
    d = np.where(ta < tb, ta, tb) - np.where(ba > bb, ba, bb)
    h = np.where(d > 0.0, d, 0.0)
    i3 = inter * h
    u = Aa * a[:, 5] + Ab * b[:, 5] - i3
    return i3 / np.where(u > EPS_3D, u, EPS_3D)


def pair_iou(a, pa, oka, b, pb, okb, mode, area=clip_area):
    """iou of P pairs, float64; 0 where either box is absent.  `area`: clip_area, or area_independent."""
    both = np.flatnonzero(oka & okb)
    out = np.zeros(len(a))
    if len(both):
        out[both] = iou_from_area(area(a[both], pa[both], b[both], pb[both]), a[both], b[both], mode)
    return out


def _f64(boxes):
    return np.asarray(boxes)[..., :7].astype(np.float64)


def boxes_iou(boxes_a, boxes_b, pose_a, pose_b, mode="3d", area=clip_area):
    """iou (F, M, B) T, best (F, M) int32 and best_iou (F, M) T of the definition, as a dict; iou64 is the matrix before the rounding to T."""
    boxes_a, boxes_b = np.asarray(boxes_a), np.asarray(boxes_b)
    F, M, B = boxes_a.shape[0], boxes_a.shape[1], boxes_b.shape[1]
    a, b = _f64(boxes_a), _f64(boxes_b)
    oka, okb = present(boxes_a, pose_a), present(boxes_b, pose_b)
    iou = np.zeros((F, M, B))
    for f in range(F):
        mi, bi = (x.reshape(-1) for x in np.meshgrid(np.arange(M), np.arange(B), indexing="ij"))
        iou[f] = pair_iou(a[f][mi], pose_a[f][mi], oka[f][mi], b[f][bi], pose_b[f][bi], okb[f][bi], mode, area).reshape(M, B)
    top = iou.max(axis=2)
    best = np.where(top > 0.0, iou.argmax(axis=2), -1).astype(np.int32)                 # (argmax: the first of equals)
    return dict(iou=iou.astype(boxes_a.dtype), best=best, best_iou=np.where(top > 0.0, top, 0.0).astype(boxes_a.dtype), iou64=iou)


def ranking(boxes, scores, pose, score_thresh=-np.inf):
    """The candidates of ONE frame in rank order (box numbers): score descending, the smallest number first among equals."""
    s = np.asarray(scores).astype(np.float64)                                            # (exact, and it keeps the order of T)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(present(boxes, pose) & (s >= score_thresh))
    return cand[np.argsort(-s[cand], kind="stable")]                                     # (-0 and +0 are equal; stable: ascending numbers)


def nms_frame(boxes, scores, pose, iou_thresh, post_max, score_thresh=-np.inf, mode="bev", area=clip_area, trace=None):
    """The kept box numbers of ONE frame in rank order.  Sequential by definition; walked in blocks of 64 ranked candidates so that the pairs
    come in large vectors: a block against the boxes kept before it, then the survivors among themselves, resolved in rank order.  Every
    pair evaluated is (candidate, earlier box) with area(candidate, earlier); the decisions are those of the one-by-one walk.  `trace`, a
    list, receives arrays of the IoUs of every pair the ONE-BY-ONE walk can decide by -- a candidate against every box kept before it --,
    when the caller wants the margins."""
    b = _f64(boxes)
    ok = present(boxes, pose)
    order = ranking(boxes, scores, pose, score_thresh)
    kept = []
    for r0 in range(0, len(order), 64):
        if len(kept) >= post_max:
            break
        blk = order[r0:r0 + 64]
        alive = np.ones(len(blk), bool)
        if kept:
            ci, ki = (x.reshape(-1) for x in np.meshgrid(blk, np.array(kept), indexing="ij"))
            v = pair_iou(b[ci], pose[ci], ok[ci], b[ki], pose[ki], ok[ki], mode, area).reshape(len(blk), len(kept))
            alive = ~(v > iou_thresh).any(axis=1)
            if trace is not None:
                trace.append(v.reshape(-1))
        idx = np.flatnonzero(alive)
        jj, ii = np.triu_indices(len(idx), 1)
        jj, ii = idx[ii], idx[jj]                                                        # (pairs j > i of survivors, by position in the block)
        sup, vals = np.zeros((len(blk), len(blk)), bool), {}
        if len(jj):
            v = pair_iou(b[blk[jj]], pose[blk[jj]], ok[blk[jj]], b[blk[ii]], pose[blk[ii]], ok[blk[ii]], mode, area)
            sup[jj, ii] = v > iou_thresh
            vals = dict(zip(zip(jj.tolist(), ii.tolist()), v.tolist()))
        mine = []
        for j in idx:
            if len(kept) + len(mine) >= post_max:
                break
            if trace is not None:
                trace.append(np.array([vals[(int(j), int(i))] for i in mine]))
            if not sup[j, mine].any():
                mine.append(int(j))
        kept.extend(int(blk[j]) for j in mine)
    return np.array(kept, np.int64)


def nms_frame_plain(boxes, scores, pose, iou_thresh, post_max, score_thresh=-np.inf, mode="bev"):
    """The kept box numbers of ONE frame by the definition's own walk, one candidate at a time: candidate j against the boxes kept so far,
    kept unless one of them has iou(j, i) > iou_thresh; stop at post_max.  No blocks -- nms_frame(), which has the structure of the
    device's sweep, is held equal to this by the tests."""
    b = _f64(boxes)
    ok = present(boxes, pose)
    kept = []
    for j in ranking(boxes, scores, pose, score_thresh):
        if len(kept) >= post_max:
            break
        if kept:
            k, jj = np.array(kept), np.full(len(kept), j)
            if (pair_iou(b[jj], pose[jj], ok[jj], b[k], pose[k], ok[k], mode) > iou_thresh).any():
                continue
        kept.append(int(j))
    return np.array(kept, np.int64)


def nms(boxes, scores, pose, iou_thresh, post_max, score_thresh=-np.inf, mode="bev", area=clip_area):
    """index (F, post_max) int32, count (F) int32, boxes (F, post_max, Cb) T, scores (F, post_max) T and kept (F, B) uint8 of the definition."""
    boxes, scores = np.asarray(boxes), np.asarray(scores)
    F, B, Cb = boxes.shape
    out = dict(index=np.full((F, post_max), -1, np.int32), count=np.zeros(F, np.int32), boxes=np.zeros((F, post_max, Cb), boxes.dtype),
               scores=np.zeros((F, post_max), boxes.dtype), kept=np.zeros((F, B), np.uint8))
    for f in range(F):
        k = nms_frame(boxes[f], scores[f], pose[f], iou_thresh, post_max, score_thresh, mode, area)
        out["index"][f, :len(k)], out["count"][f] = k, len(k)
        out["boxes"][f, :len(k)], out["scores"][f, :len(k)] = boxes[f, k], scores[f, k]
        out["kept"][f, k] = 1
    return out


# ---- the independent method ---------------------------------------------------------------------------------------------------------------
def _world_corners(b, p):
    hx, hy = b[3] / 2, b[4] / 2
    return np.array([[b[0] + lx * p[0] - ly * p[1], b[1] + lx * p[1] + ly * p[0]] for lx, ly in ((hx, hy), (-hx, hy), (-hx, -hy), (hx, -hy))])


def _inside(pt, b, p):
    sx, sy = pt[0] - b[0], pt[1] - b[1]
    return abs(sx * p[0] + sy * p[1]) <= b[3] / 2 and abs(sy * p[0] - sx * p[1]) <= b[4] / 2


def area_independent_one(a, pa, b, pb):
    """The overlap of one pair by another route: edge-edge intersections in WORLD coordinates plus the corners of either box inside the
    other, ordered by np.arctan2 about their mean, shoelace about the mean."""
    ca, cb = _world_corners(a, pa), _world_corners(b, pb)
    pts = [c for c in ca if _inside(c, b, pb)] + [c for c in cb if _inside(c, a, pa)]
    for i in range(4):
        p, r = ca[i], ca[(i + 1) % 4] - ca[i]
        for j in range(4):
            q, s = cb[j], cb[(j + 1) % 4] - cb[j]
            den = r[0] * s[1] - r[1] * s[0]
            if den == 0.0:
                continue
            t = ((q[0] - p[0]) * s[1] - (q[1] - p[1]) * s[0]) / den
            w = ((q[0] - p[0]) * r[1] - (q[1] - p[1]) * r[0]) / den
            if 0.0 <= t <= 1.0 and 0.0 <= w <= 1.0:
                pts.append(p + t * r)
    if len(pts) < 3:
        return 0.0
    pts = np.array(pts)
    rel = pts - pts.mean(axis=0)
    rel = rel[np.argsort(np.arctan2(rel[:, 1], rel[:, 0]), kind="stable")]
    nxt = np.roll(rel, -1, axis=0)
    return 0.5 * abs(float(np.sum(rel[:, 0] * nxt[:, 1] - nxt[:, 0] * rel[:, 1])))


def area_independent(a, pa, b, pb, slack=0.0):
    """area_independent_one for P pairs at once (the same route, vectorised; the tests hold the two together on a sample): up to 8 contained
    corners and 16 crossings per pair, the missing ones replaced by the first point in angular order, which adds edges of no area.
    `slack` (a length, or one per pair; 0: the route as it stands) is for pairs AT a degeneracy -- equal boxes, headings 1 ulp apart, edges
    on one line --, where rounding decides which corner is "inside" and at which garbage parameter two edges on one line "cross", and the
    plain route loses corners of the true overlap.  With the vertex error d of the derivation above as slack, a corner no further than d
    outside counts as inside, and two edges are taken as parallel (no crossing) when over their length they stay within 8 d of one
    line: the points added or dropped are within d of the true boundary, so the polygon still lies between the shrunk and the grown
    overlap and TOL_AREA holds as derived."""
    slack = np.broadcast_to(np.asarray(slack, np.float64), (len(a),))
    P = len(a)
    sgn = np.array([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]])

    def world(b_, p_):
        lx, ly = sgn[None, :, 0] * (b_[:, 3] / 2)[:, None], sgn[None, :, 1] * (b_[:, 4] / 2)[:, None]
        return np.stack((b_[:, None, 0] + lx * p_[:, None, 0] - ly * p_[:, None, 1], b_[:, None, 1] + lx * p_[:, None, 1] + ly * p_[:, None, 0]), axis=-1)

    def inside(pts, b_, p_):
        sx, sy = pts[..., 0] - b_[:, None, 0], pts[..., 1] - b_[:, None, 1]
        return ((np.abs(sx * p_[:, None, 0] + sy * p_[:, None, 1]) <= (b_[:, 3] / 2 + slack)[:, None]) &
                (np.abs(sy * p_[:, None, 0] - sx * p_[:, None, 1]) <= (b_[:, 4] / 2 + slack)[:, None]))

    ca, cb = world(a, pa), world(b, pb)                                                   # (P, 4, 2)
    p, r = ca[:, :, None, :], (np.roll(ca, -1, axis=1) - ca)[:, :, None, :]               # (P, 4, 1, 2)
    q, s = cb[:, None, :, :], (np.roll(cb, -1, axis=1) - cb)[:, None, :, :]               # (P, 1, 4, 2)
    with np.errstate(all="ignore"):
        den = r[..., 0] * s[..., 1] - r[..., 1] * s[..., 0]
        t = ((q[..., 0] - p[..., 0]) * s[..., 1] - (q[..., 1] - p[..., 1]) * s[..., 0]) / den
        w = ((q[..., 0] - p[..., 0]) * r[..., 1] - (q[..., 1] - p[..., 1]) * r[..., 0]) / den
        longer = np.maximum(np.hypot(r[..., 0], r[..., 1]), np.hypot(s[..., 0], s[..., 1]))
        hit = (den != 0.0) & (np.abs(den) > 8.0 * slack[:, None, None] * longer) & (t >= 0.0) & (t <= 1.0) & (w >= 0.0) & (w <= 1.0)
        cross = p + t[..., None] * r
    pts = np.concatenate((ca, cb, cross.reshape(P, 16, 2)), axis=1)                       # (P, 24, 2)
    ok = np.concatenate((inside(ca, b, pb), inside(cb, a, pa), hit.reshape(P, 16)), axis=1)
    cnt = ok.sum(axis=1)
    mean = np.where(ok[..., None], pts, 0.0).sum(axis=1) / np.maximum(cnt, 1)[:, None]
    rel = np.where(ok[..., None], pts - mean[:, None, :], 0.0)
    ang = np.where(ok, np.arctan2(rel[..., 1], rel[..., 0]), np.inf)
    order = np.argsort(ang, axis=1, kind="stable")
    rel, oks = np.take_along_axis(rel, order[..., None], axis=1), np.take_along_axis(ok, order, axis=1)
    rel = np.where(oks[..., None], rel, rel[:, :1, :])
    nxt = np.roll(rel, -1, axis=1)
    area = 0.5 * np.abs((rel[..., 0] * nxt[..., 1] - nxt[..., 0] * rel[..., 1]).sum(axis=1))
    return np.where(cnt >= 3, area, 0.0)


# ---- shared inputs --------------------------------------------------------------------------------------------------------------------------
CASE_R, CASE_L = 64.0, 8.0                      # every case: |centre| <= 50, dx <= 6, dy <= 3 (diagonal < 8): coordinates within 64 m
CASE_AMIN = 1.5 * 3.0                            # the smallest footprint any case draws


def case_tol_area():
    return tol_area(CASE_R, CASE_L)


def case_tol_iou():
    return tol_iou(CASE_R, CASE_L, CASE_AMIN)


def clustered(rng, B, centres, Cb=8, spread=0.35, turn=0.12):
    """B car-sized boxes jittered about `centres` cluster centres within +-45 m: members of a cluster overlap, so NMS suppresses."""
    cen = np.column_stack((rng.uniform(-45, 45, (centres, 2)), rng.uniform(-1.5, -0.5, centres), rng.uniform(3.6, 5.0, centres), rng.uniform(1.6, 2.1, centres),
                           rng.uniform(1.4, 2.0, centres), rng.uniform(-np.pi, np.pi, centres)))
    of = rng.integers(0, centres, B)
    box = cen[of]
    box[:, :2] += rng.normal(0, spread, (B, 2)).clip(-1.5, 1.5)
    box[:, 2] += rng.normal(0, 0.1, B).clip(-0.4, 0.4)
    box[:, 3:6] *= rng.uniform(0.92, 1.08, (B, 3))
    box[:, 6] += rng.normal(0, turn, B).clip(-0.5, 0.5)
    out = np.zeros((B, Cb))
    out[:, :7] = box
    out[:, 7:] = rng.integers(1, 4, (B, Cb - 7))
    return out


# name: (B, cluster centres, post_max or None = B, seed)
NMS_SHAPES = {"b1": (1, 1, None, 1), "b2": (2, 1, None, 2), "b63": (63, 6, None, 3), "b64": (64, 6, 9, 4), "b65": (65, 6, None, 5), "b129": (129, 10, None, 6),
              "b4160": (4160, 30, None, 7), "b9216": (9216, 24, None, 8)}
NMS_CASES = tuple(NMS_SHAPES) + ("chain", "mixed")
IOU_THRESH, SCORE_CUT = 0.45, 0.05
CHAIN = np.array([[10.0, 5.0, -1.0, 4.0, 2.0, 1.5, 0.3, 1.0], [10.9, 5.3, -1.0, 4.0, 2.0, 1.5, 0.3, 1.0], [11.8, 5.6, -1.0, 4.0, 2.0, 1.5, 0.3, 1.0],
                  [-20.0, 0.0, -1.0, 4.0, 2.0, 1.5, 1.0, 2.0]])           # A, B, C along A's axis, 0.95 m apart; a loner


def _cast(dtype, **arrays):
    out = {}
    for k, v in arrays.items():
        v = np.ascontiguousarray(np.asarray(v).astype(dtype))
        v.setflags(write=False)
        out[k] = v
    return out


@functools.lru_cache(maxsize=None)
def nms_case(name, dtype="float32"):
    """dict(boxes (F, B, 8) T, scores (F, B) T, pose (F, B, 2) float64 = NumPy's, iou_thresh, score_thresh, post_max, mode) -- read-only."""
    if name in NMS_SHAPES:
        B, centres, post_max, seed = NMS_SHAPES[name]
        rng = np.random.default_rng(4000 + seed)
        boxes, scores = clustered(rng, B, centres)[None], rng.uniform(0.1, 1.0, (1, B))
        if B >= 63:
            boxes[0, 7] = boxes[0, 3]                                  # an exact duplicate
            scores[0, 11] = scores[0, 12] = scores[0, 13]              # equal scores
        if name == "b2":
            boxes[0, 1, :7] = boxes[0, 0, :7] + np.array([0.2, 0.1, 0, 0, 0, 0, 0.02])
        kw = dict(iou_thresh=IOU_THRESH, score_thresh=-np.inf, post_max=post_max or B, mode="bev")
    elif name == "chain":
        boxes, scores = CHAIN[None].copy(), np.array([[0.9, 0.8, 0.7, 0.6]])
        kw = dict(iou_thresh=IOU_THRESH, score_thresh=-np.inf, post_max=4, mode="bev")
    else:                                                              # mixed: three frames of different content in one call, 3D
        rng = np.random.default_rng(4100)
        B = 150
        boxes, scores = np.stack([clustered(rng, B, 12) for _ in range(3)]), rng.uniform(0.0, 1.0, (3, B))
        boxes[1] = 0.0                                                 # frame 1: every box absent
        boxes[0, 5] = 0.0                                              # padding
        boxes[0, 6, 3] = -1.0                                          # a negative extent: absent
        boxes[0, 9] = boxes[0, 8]                                      # duplicates
        scores[0, 20:24] = 0.75                                        # ties
        scores[0, 30] = -0.0
        scores[0, 31] = 0.0
        scores[0, 40] = np.nan
        scores[0, 41] = np.inf
        scores[2, :60] = np.round(scores[2, :60], 1)                   # many ties
        kw = dict(iou_thresh=0.3, score_thresh=SCORE_CUT, post_max=40, mode="3d")
    c = _cast(dtype, boxes=boxes, scores=scores)
    pose = numpy_pose(c["boxes"])
    pose.setflags(write=False)
    return dict(c, pose=pose, **kw)


@functools.lru_cache(maxsize=None)
def nms_expected(name, dtype="float32"):
    c = nms_case(name, dtype)
    return nms(c["boxes"], c["scores"], c["pose"], c["iou_thresh"], c["post_max"], c["score_thresh"], c["mode"])


# name: (M, B, seed)
IOU_SHAPES = {"m1b1": (1, 1, 1), "m63b65": (63, 65, 2), "m64b64": (64, 64, 3), "m65b129": (65, 129, 4), "m3b9216": (3, 9216, 5), "m9216b2": (9216, 2, 6)}
IOU_CASES = tuple(IOU_SHAPES)


@functools.lru_cache(maxsize=None)
def iou_case(name, dtype="float32"):
    """dict(a (3, M, 7) T, b (3, B, 9) T, pose_a, pose_b float64 = NumPy's) -- read-only.  Frame 0: every b present; frame 1: every other b
    is padding and some a are; frame 2: no b is present.  The a boxes are jittered copies of b boxes, so they overlap; a few are lifted out
    of their partner's height (BEV > 0, 3D exactly 0); b[1] repeats b[0] where there are two (a tie for best)."""
    M, B, seed = IOU_SHAPES[name]
    rng = np.random.default_rng(4200 + seed)
    b = np.stack([clustered(rng, B, max(1, min(B, 512) // 3), Cb=9, spread=2.0, turn=1.0) for _ in range(3)])
    a = np.zeros((3, M, 7))
    for f in range(3):
        of = rng.integers(0, B, M)
        a[f] = b[f, of, :7]
        a[f, :, :2] += rng.normal(0, 0.5, (M, 2)).clip(-1.5, 1.5)
        a[f, :, 6] += rng.normal(0, 0.2, M).clip(-0.5, 0.5)
        a[f, ::5, 2] += 4.0                                            # apart in z only
        if M == 1:
            a[f, :, 2] = b[f, of, 2]
    if B >= 2:
        b[:, 1] = b[:, 0]
    if M >= 2:
        a[0, 1] = b[0, 0, :7]                                          # exactly a b box: the same IoU, near 1, with b[0] and b[1], the tie
    b[1, 1::2] = 0.0
    a[1, 2::7] = 0.0
    b[2] = 0.0
    c = _cast(dtype, a=a, b=b)
    pa, pb = numpy_pose(c["a"]), numpy_pose(c["b"])
    pa.setflags(write=False), pb.setflags(write=False)
    return dict(c, pose_a=pa, pose_b=pb)


@functools.lru_cache(maxsize=None)
def iou_expected(name, dtype="float32", mode="3d"):
    c = iou_case(name, dtype)
    return boxes_iou(c["a"], c["b"], c["pose_a"], c["pose_b"], mode)


# ---- adversarial pair families: the kinds of tests/host_harness/iou_clip.cpp, z_sliver and clamped, for host and device -----------------------
# One frame per family of a (families, 130, 130) call: two full tiles of 64 b boxes and a partial one.  a[i] and b[i] are DESIGNED partners
# (the diagonal); the 16 770 other pairs of a frame come for free.  Every family is built IN THE DTYPE UNDER TEST: a float64 construction
# cast to float32 moves a shared face or a stacked height by 1e-7 of the coordinate and the pair is no longer at its edge.  Where float32
# has to hit a face or a height exactly, sizes and offsets are dyadic and the heading is 0 (cos and sin exact); headings 1 ulp apart are
# nextafter in T.  These inputs VIOLATE the margins of the cases above on purpose: nothing here is compared with a tolerance against
# the device, only byte for byte with the restatement.
FAMILIES = ("equal", "right_angle", "one_ulp", "shared_face", "sliver", "far", "sizes", "collapsed", "z_sliver", "clamped")
FAMILY_N = 130
F32_TINY = float(np.finfo(np.float32).tiny)


def _cars(rng, n, T, reach=45.0):
    """n car-sized boxes (n, 7) T, as the harness draws them."""
    return np.column_stack((rng.uniform(-reach, reach, (n, 2)), rng.uniform(-2, 0, n), rng.uniform(3.5, 5.0, n), rng.uniform(1.6, 2.1, n),
                            rng.uniform(1.4, 2.0, n), rng.uniform(-np.pi, np.pi, n))).astype(T)


def _dyadic(rng, n, T):
    """n axis-aligned boxes of dyadic centres and sizes, heading 0: every operation of the definition on them is exact in either dtype."""
    return np.column_stack((rng.integers(-160, 161, (n, 2)) / 4, rng.integers(-16, 1, n) / 8, rng.integers(2, 25, n) / 4, rng.integers(2, 13, n) / 4,
                            rng.integers(2, 11, n) / 4, np.zeros(n))).astype(T)


def _ulps(x, towards, steps):
    """x moved `steps` (an integer array) ulps of its dtype towards `towards`."""
    x = x.copy()
    for k in range(int(steps.max(initial=0))):
        x = np.where(steps > k, np.nextafter(x, towards.astype(x.dtype)), x)
    return x


def designed_stats(a, b):
    """area, most emitted vertices, BEV and 3D IoU (float64), BEV and 3D unions of the pairs (a[i], b[i]) under NumPy's pose."""
    a64, b64 = _f64(a), _f64(b)
    pa, pb = numpy_pose(a), numpy_pose(b)
    ok = present(a, pa) & present(b, pb)
    assert ok.all()
    area, most = clip_area(a64, pa, b64, pb, return_most=True)
    Aa, Ab = a64[:, 3] * a64[:, 4], b64[:, 3] * b64[:, 4]
    bev, i3d = iou_from_area(area, a64, b64, "bev"), iou_from_area(area, a64, b64, "3d")
    hza, hzb = a64[:, 5] * 0.5, b64[:, 5] * 0.5
    d = np.minimum(a64[:, 2] + hza, b64[:, 2] + hzb) - np.maximum(a64[:, 2] - hza, b64[:, 2] - hzb)
    u3 = Aa * a64[:, 5] + Ab * b64[:, 5] - area * np.where(d > 0.0, d, 0.0)
    return dict(area=area, most=most, bev=bev, i3d=i3d, u_bev=Aa + Ab - area, u_3d=u3)


def _family_pool(name, T, more=0):
    """A fixed-seed draw of designed pairs of one family, (n, 7) T each; _family() takes the first FAMILY_N, or selects.  more: a second draw
    of `more` pairs by the harness's recipe alone, to select from."""
    T = np.dtype(T).type
    rng = np.random.default_rng(4400 + FAMILIES.index(name) + (100 if more else 0))
    n = more or (24000 if name == "equal" else FAMILY_N)

    def u(lo, hi, k=n):
        return rng.uniform(lo, hi, k).astype(T)

    def p10(lo, hi, k=n):
        return (10.0 ** rng.uniform(lo, hi, k)).astype(T)

    a = _cars(rng, n, T)
    b = a.copy()
    coin = rng.integers(0, 2, n).astype(bool)
    if name == "equal":
        a[:10] = _dyadic(rng, 10, T)                                     # every corner exactly on its clip line
        b = a.copy()
    elif name == "right_angle":
        a[:, 6] = (rng.integers(-4, 5, n) * (np.pi / 2)).astype(T)
        b = a.copy()
        b[:, 6] = a[:, 6] + (rng.integers(-4, 5, n) * (np.pi / 2)).astype(T)
        b[:, 0] = np.where(coin, b[:, 0] + u(-1, 1), b[:, 0])
        b[:, 3] = np.where(coin, u(1, 6), b[:, 3])
    elif name == "one_ulp":
        b[:, 6] = np.nextafter(a[:, 6], np.where(coin, T(10), T(-10)))
        b[:, 3] = np.where(rng.integers(0, 2, n).astype(bool), a[:, 3] * T(0.5), a[:, 3])
    elif name == "shared_face":
        h = n if more else n // 2                                        # [0, h): the harness's recipe in T; [h, n): dyadic, exact in T
        square = rng.integers(0, 2, n).astype(bool)
        a[:, 6] = np.where(square, (rng.integers(-2, 3, n) * (np.pi / 2)).astype(T), a[:, 6])
        b = a.copy()
        c, s, d = np.cos(a[:, 6]), np.sin(a[:, 6]), np.where(coin, a[:, 4], a[:, 3])
        b[:, 0] = a[:, 0] + np.where(coin, -s, c) * d
        b[:, 1] = a[:, 1] + np.where(coin, c, s) * d
        k = n - h
        a[h:] = _dyadic(rng, k, T)
        b[h:] = _dyadic(rng, k, T)
        b[h:, 0] = a[h:, 0] + (a[h:, 3] + b[h:, 3]) * T(0.5)             # b's -x face on a's +x face, exactly
        b[h:, 1] = a[h:, 1] + (rng.integers(-4, 5, k) / 4).astype(T)
        kind = np.arange(k) % 3                                          # 0: exact; 1: 1 .. 3 ulps of overlap; 2: 1 .. 3 ulps of gap
        steps = np.where(kind == 0, 0, rng.integers(1, 4, k))
        b[h:, 0] = _ulps(b[h:, 0], np.where(kind == 1, -1e9, 1e9), steps)
    elif name == "sliver":
        a[:, 3], a[:, 4] = p10(-6, -3), u(5, 20)
        b = a.copy()
        b[:, 6] = a[:, 6] + u(-1e-3, 1e-3)
        b[:, 3] = np.where(coin, u(1, 5), b[:, 3])
        b[:, 4] = np.where(coin, p10(-6, -3), b[:, 4])
    elif name == "far":
        lim = T(BOUND)
        a[:, 0], a[:, 1] = u(-1e6, 1e6), u(-1e6, 1e6)
        a[:, 3], a[:, 4] = np.minimum(p10(0, 6), lim), np.minimum(p10(0, 6), lim)
        b = a.copy()
        b[:, 0] = np.clip(a[:, 0] + u(-1, 1) * a[:, 3], -lim, lim)
        b[:, 6] = u(-1e6, 1e6)
        b[:, 3] = np.minimum(p10(0, 6), lim)
    elif name == "sizes":
        for k in (3, 4):
            a[:, k], b[:, k] = p10(-2, 2), p10(-2, 2)
        b[:, 0] = a[:, 0] + u(-1, 1) * a[:, 3]
        b[:, 1] = a[:, 1] + u(-1, 1) * a[:, 4]
        b[:, 6] = u(-np.pi, np.pi)
    elif name == "collapsed":
        for k in (3, 4):
            a[:, k] = p10(-15, -12)
            b[:, k] = np.where(rng.integers(0, 2, n).astype(bool), a[:, k], p10(-15, -12))
        b[:, 0] = a[:, 0] + u(-1, 1) * a[:, 3]
        b[:, 6] = np.where(coin, a[:, 6], u(-np.pi, np.pi))
    elif name == "z_sliver":
        b[:, 0], b[:, 1] = a[:, 0] + u(-0.5, 0.5), a[:, 1] + u(-0.5, 0.5)
        b[:, 6] = a[:, 6] + u(-0.2, 0.2)
        meet = (np.arange(n) % 2).astype(bool)                           # odd: the heights meet; even: they miss
        sign = np.where(meet, T(1), T(-1))
        frac = p10(-15, -10)
        k = 44
        # A [0, 44): a's top is dz / 2 + delta with a.cz = +-delta = dz 1e-15 .. 1e-10, b stands on dz / 2 exactly -- in either dtype
        a[:k, 5], b[:k, 5] = (rng.integers(4, 11, k) / 4).astype(T), (rng.integers(4, 11, k) / 4).astype(T)
        a[:k, 2] = sign[:k] * (a[:k, 5] * frac[:k])
        b[:k, 2] = (a[:k, 5] + b[:k, 5]) * T(0.5)
        # B [44, 88): dyadic heights that touch exactly, then 0 .. 3 ulps of T in (meet) or out
        s = slice(k, 2 * k)
        a[s, 5], b[s, 5] = (rng.integers(4, 11, k) / 4).astype(T), (rng.integers(4, 11, k) / 4).astype(T)
        a[s, 2] = (rng.integers(-16, 1, k) / 8).astype(T)
        b[s, 2] = a[s, 2] + (a[s, 5] + b[s, 5]) * T(0.5)
        b[s, 2] = _ulps(b[s, 2], np.where(meet[s], -1e9, 1e9), rng.integers(0, 4, k))
        # C [88, n): car heights, the stacking computed in T with dz 1e-15 .. 1e-10 taken off or added: rounding decides
        s = slice(2 * k, n)
        b[s, 2] = a[s, 2] + (a[s, 5] + b[s, 5]) * T(0.5) - sign[s] * (a[s, 5] * frac[s])
    elif name == "clamped":
        def near(lo, hi, k):                                             # k pairs about the origin whose BEV union is near 10^U(lo, hi)
            A = 10.0 ** rng.uniform(lo, hi, k) / 1.6
            r = rng.uniform(1, 3, k)
            x = np.zeros((k, 7))
            x[:, 0], x[:, 1], x[:, 2] = rng.uniform(-0.01, 0.01, k), rng.uniform(-0.01, 0.01, k), rng.uniform(-1, 0, k)
            x[:, 3], x[:, 4], x[:, 5], x[:, 6] = np.sqrt(A * r), np.sqrt(A / r), rng.uniform(0.5, 2, k), rng.uniform(-np.pi, np.pi, k)
            return x.astype(T), A
        g1, _ = near(-9.6, -8.05, 44)                                    # both unions under their clamps
        g2, _ = near(-7.95, -6.7, 25)                                    # BEV above 1e-8, 3D under 1e-6
        g3, A3 = near(-4, -2, 25)                                        # both above
        g3[:, 5] = (10.0 ** rng.uniform(-5.9, -5, 25) / (3.2 * A3)).astype(T)
        g4, A4 = near(-4, -2, 20)                                        # BEV above, 3D just under
        g4[:, 5] = (10.0 ** rng.uniform(-7, -6.1, 20) / (3.2 * A4)).astype(T)
        tiny = np.zeros((16, 7), T)                                      # about the origin, 2^-77 .. 2^-81 m wide: overlap / clamp is a float32 subnormal
        tiny[:, 3], tiny[:, 4] = np.ldexp(T(1), -rng.integers(77, 82, 16)), np.ldexp(T(1), -rng.integers(77, 82, 16))
        tiny[:, 5], tiny[:, 6] = u(0.5, 2, 16), np.where(np.arange(16) % 2, u(-np.pi, np.pi, 16), T(0))
        a = np.concatenate((tiny, g1, g2, g3, g4))
        b = a.copy()
        k = len(a)
        b[:, 0], b[:, 1] = a[:, 0] + u(-0.4, 0.4, k) * a[:, 3], a[:, 1] + u(-0.4, 0.4, k) * a[:, 4]
        b[:, 2] = a[:, 2] + u(-0.3, 0.3, k) * a[:, 5]
        b[:, 3:6] = a[:, 3:6] * rng.uniform(0.8, 1.25, (k, 3)).astype(T)
        b[16:, 6] = a[16:, 6] + u(-0.3, 0.3, k - 16)
        b[:16, 3:5] = np.ldexp(T(1), -rng.integers(77, 82, (16, 2)))
        b[:16, 0] = np.where(np.arange(16) % 4 == 0, T(0), np.ldexp(T(1), -83) * (rng.integers(-3, 4, 16)).astype(T))
        b[:16, 1] = T(0)
    assert a.dtype == b.dtype == np.dtype(T) and len(a) == len(b) == n
    return a, b


BOUNDARY_FAMILIES, BOUNDARY_PAIRS = ("equal", "right_angle", "one_ulp", "shared_face"), 16


def boundary_decides(a, b):
    """Which pairs (a[i], b[i]) have another area when a point on a clip line counts as outside."""
    a64, b64, pa, pb = _f64(a), _f64(b), numpy_pose(a), numpy_pose(b)
    return clip_area(a64, pa, b64, pb) != clip_area(a64, pa, b64, pb, boundary_inside=False)


@functools.lru_cache(maxsize=None)
def _family(name, dtype):
    """The FAMILY_N designed pairs of one family: a (130, 7), b (130, 7) T.  Two rare kinds of pair are selected from larger fixed-seed
    draws by the restatement's own results and frozen with the seed: pairs of which a pass emits more than 8 vertices (a few in a thousand
    equal pairs; up to 8 of them, behind the 10 dyadic pairs of `equal`), and pairs whose area the boundary rule decides (about one in a
    hundred of the four BOUNDARY_FAMILIES, fewer in float32; up to 16, in the last slots of the frame)."""
    a, b = _family_pool(name, dtype)
    if name == "equal":
        most = designed_stats(a, b)["most"]
        rare = np.flatnonzero(most > 8)
        rare = rare[rare >= 10][:8]
        edge = np.setdiff1d(np.flatnonzero(boundary_decides(a, b)), rare)[:BOUNDARY_PAIRS]
        rest = np.setdiff1d(np.arange(len(a)), np.concatenate((rare, edge)))[:FAMILY_N - len(rare) - len(edge)]
        pick = np.concatenate((rest[:10], rare, rest[10:], edge))
        a, b = a[pick], b[pick]
    elif name in BOUNDARY_FAMILIES:
        xa, xb = _family_pool(name, dtype, more=12000)
        edge = np.flatnonzero(boundary_decides(xa, xb))[:BOUNDARY_PAIRS]
        a, b = a.copy(), b.copy()
        if len(edge):
            a[-len(edge):], b[-len(edge):] = xa[edge], xb[edge]
    return a[:FAMILY_N], b[:FAMILY_N]


@functools.lru_cache(maxsize=None)
def family_case(dtype="float32"):
    """dict(a (10, 130, 7) T, b (10, 130, 9) T, pose_a, pose_b float64 = NumPy's): frame k holds FAMILIES[k] -- read-only."""
    a = np.stack([_family(name, dtype)[0] for name in FAMILIES])
    b = np.ones((len(FAMILIES), FAMILY_N, 9), a.dtype)
    b[..., :7] = np.stack([_family(name, dtype)[1] for name in FAMILIES])
    c = _cast(dtype, a=a, b=b)
    pa, pb = numpy_pose(c["a"]), numpy_pose(c["b"])
    pa.setflags(write=False), pb.setflags(write=False)
    return dict(c, pose_a=pa, pose_b=pb)


@functools.lru_cache(maxsize=None)
def family_expected(dtype="float32", mode="3d"):
    c = family_case(dtype)
    return boxes_iou(c["a"], c["b"], c["pose_a"], c["pose_b"], mode)


def family_pairs(c):
    """The designed pairs of a family_case as frames of one box each: a (1300, 1, 7), b (1300, 1, 9) and their poses."""
    d = np.arange(FAMILY_N)
    return dict(a=np.ascontiguousarray(c["a"][:, d].reshape(-1, 1, 7)), b=np.ascontiguousarray(c["b"][:, d].reshape(-1, 1, 9)),
                pose_a=np.ascontiguousarray(c["pose_a"][:, d].reshape(-1, 1, 2)), pose_b=np.ascontiguousarray(c["pose_b"][:, d].reshape(-1, 1, 2)))


def pairs_expected(p, mode):
    """boxes_iou() of M = B = 1 frames, all frames as one vector of pairs."""
    a, b, pa, pb = p["a"][:, 0], p["b"][:, 0], p["pose_a"][:, 0], p["pose_b"][:, 0]
    v = pair_iou(_f64(a), pa, present(a, pa), _f64(b), pb, present(b, pb), mode)
    T = p["a"].dtype
    return dict(iou=v.astype(T).reshape(-1, 1, 1), best=np.where(v > 0.0, 0, -1).astype(np.int32).reshape(-1, 1),
                best_iou=np.where(v > 0.0, v, 0.0).astype(T).reshape(-1, 1), iou64=v.reshape(-1, 1, 1))


# ---- exact ties and thresholds at equality ----------------------------------------------------------------------------------------------------
def _grid(n, pitch=8.0):
    """n dyadic centres on a square grid `pitch` metres apart: boxes no longer than 6 m diagonal on them are pairwise disjoint."""
    side = int(math.ceil(math.sqrt(n)))
    k = np.arange(n)
    return np.column_stack(((k % side - side // 2) * pitch, (k // side - side // 2) * pitch))


BEST_TIE_B, BEST_TIE_GROUPS = 200, ((5, 69, 133), (3, 70), (9, 66))   # (9, 66): the larger number sits in the smaller lane


@functools.lru_cache(maxsize=None)
def best_tie_case(dtype="float32"):
    """IoU ties for `best` across the 64-wide tiles of the b side: 200 b boxes on a grid, identical ones at 5, 69 and 133 (one lane, three
    tiles), at 3 and 70 (a later tile) and at 9 and 66 (a later tile AND a smaller lane); two frames, frame 1 turned and lifted.  Four a
    boxes per frame: one over each group, one over no box."""
    rng = np.random.default_rng(4500)
    B = BEST_TIE_B
    b = np.zeros((2, B, 9))
    for f in range(2):
        b[f, :, :2] = _grid(B)
        b[f, :, 2:7] = np.column_stack((rng.uniform(-1.5, -0.5, B), rng.uniform(3.0, 4.5, B), rng.uniform(1.6, 2.1, B), rng.uniform(1.4, 2.0, B), rng.uniform(-np.pi, np.pi, B)))
        b[f, :, 7:] = rng.integers(1, 4, (B, 2))
    a = np.zeros((2, 4, 7))
    for f in range(2):
        for g, group in enumerate(BEST_TIE_GROUPS):
            for k in group[1:]:
                b[f, k, :7] = b[f, group[0], :7]
            a[f, g] = b[f, group[0], :7] + np.array([0.3, -0.2, 0.1, 0.2, -0.1, 0.05, 0.15]) * (1 + f)
        a[f, 3] = a[f, 0]
        a[f, 3, :2] += 4.0                                                 # between the grid's boxes: no partner
        a[f, 3, 3:5] = 0.5
    c = _cast(dtype, a=a, b=b)
    pa, pb = numpy_pose(c["a"]), numpy_pose(c["b"])
    pa.setflags(write=False), pb.setflags(write=False)
    return dict(c, pose_a=pa, pose_b=pb)


RANK_TIES = ((254, 255, 256, 257), (1023, 1024), (2046, 2047, 2048), (5, 1029))
TIE_CASES = ("rank_ties", "equal_bev", "equal_3d", "stack", "stack_cut")
EQ_PAIRS = 70


@functools.lru_cache(maxsize=None)
def tie_case(name, dtype="float32"):
    """NMS cases of exact ties, as nms_case() gives them (one frame each):
    rank_ties   2100 pairwise disjoint boxes, post_max = B, all kept; equal scores across the borders of k_nms_rank's groups (255 | 256) and
                tiles (1023 | 1024, 2047 | 2048) and at (5, 1029), one lane of two tiles: the kept order is score, then number.
    equal_bev   70 dyadic axis-aligned 4 x 2 boxes and, behind them in rank, their partners shifted by 1: every partner has BEV IoU 6 / 10 with
                its box, the same bits for every pair (integer translations), and 0 with every other.  iou_thresh is THAT IoU.
    equal_3d    the same with the partner lifted by 0.5 of dz = 2: 3D IoU 9 / 23.
    stack       130 copies of one box, every third turned 1 ulp of T, distinct scores: one box is kept.
    stack_cut   the same with score_thresh at the median score: the upper half are candidates."""
    T = np.dtype(dtype).type
    rng = np.random.default_rng(4600 + TIE_CASES.index(name))
    if name == "rank_ties":
        B = 2100
        boxes = np.ones((1, B, 8))
        boxes[0, :, :2] = _grid(B)
        boxes[0, :, 2:7] = np.column_stack((rng.uniform(-1.5, -0.5, B), rng.uniform(3.0, 4.5, B), rng.uniform(1.6, 2.1, B), rng.uniform(1.4, 2.0, B), rng.uniform(-np.pi, np.pi, B)))
        scores = rng.permutation(np.arange(1, B + 1) / 4096.0)[None]       # distinct, exact in float32
        for group in RANK_TIES:
            scores[0, list(group)] = scores[0, group[0]]
        kw = dict(iou_thresh=IOU_THRESH, score_thresh=-np.inf, post_max=B, mode="bev")
    elif name in ("equal_bev", "equal_3d"):
        n = EQ_PAIRS
        boxes = np.ones((1, 2 * n, 8))
        boxes[0, :, :7] = (0.0, 0.0, -1.0, 4.0, 2.0, 2.0, 0.0)
        at = _grid(n, 16.0)[rng.permutation(n)]
        boxes[0, :n, :2], boxes[0, n:, :2] = at, at + (1.0, 0.0)
        if name == "equal_3d":
            boxes[0, n:, 2] += 0.5
        scores = np.concatenate((1.0 - np.arange(n) / 256.0, 0.5 - rng.permutation(n) / 256.0))[None]   # the boxes, then the partners in another order
        mode = "bev" if name == "equal_bev" else "3d"
        one = boxes[:1, [0, n], :7]
        thresh = float(pair_iou(one[0, 1:], numpy_pose(one[0, 1:]), np.ones(1, bool), one[0, :1], numpy_pose(one[0, :1]), np.ones(1, bool), mode)[0])
        kw = dict(iou_thresh=thresh, score_thresh=-np.inf, post_max=2 * n, mode=mode)
    else:
        B = FAMILY_N
        one = _cars(rng, 1, T)[0]
        boxes = np.ones((1, B, 8), T)
        boxes[0, :, :7] = one
        boxes[0, 1::3, 6] = np.nextafter(one[6], T(10))
        boxes[0, 2::3, 6] = np.nextafter(one[6], T(-10))
        scores = rng.permutation(np.arange(1, B + 1) / 256.0)[None]
        cut = float(np.sort(scores[0])[B // 2]) if name == "stack_cut" else -np.inf
        kw = dict(iou_thresh=IOU_THRESH, score_thresh=cut, post_max=B, mode="bev")
    c = _cast(dtype, boxes=boxes, scores=scores)
    pose = numpy_pose(c["boxes"])
    pose.setflags(write=False)
    return dict(c, pose=pose, **kw)


def tie_thresholds(c):
    """The three thresholds of an equal_* case: the IoU itself (nothing is suppressed), the double below it (every partner is), the one above."""
    t = c["iou_thresh"]
    return (("at", t), ("below", float(np.nextafter(t, -1.0))), ("above", float(np.nextafter(t, 2.0))))


@functools.lru_cache(maxsize=None)
def tie_expected(name, dtype="float32", iou_thresh=None):
    c = tie_case(name, dtype)
    return nms(c["boxes"], c["scores"], c["pose"], c["iou_thresh"] if iou_thresh is None else iou_thresh, c["post_max"], c["score_thresh"], c["mode"])
