"""Proposal target sampling (snowgpu_sample_rois_device) restated from its definition in include/snowgpu.h: NumPy for the classes, Python
integers for the Philox words (seeded_reference.philox4x32_10), the walk and the picks, Python floats -- IEEE doubles, one rounding per
operation -- for the labels and the gt in its roi's frame.  Nothing here touches a GPU, and this module is no conftest: the tests import it
by name.  The named cases the GPU tests run live here too, so that tests/test_targets_reference.py can check on any machine that each
of them decides something."""
import math
from functools import lru_cache

import numpy as np

import box_reference as br
from seeded_reference import philox4x32_10

DTYPES = br.DTYPES
TAG = 0x524F4953                    # "ROIS"
PI, TWO_PI, HALF_PI, THREE_HALF_PI = np.pi, 2 * np.pi, 0.5 * np.pi, 1.5 * np.pi
FIELDS = ("index", "rois", "roi_iou", "gt_index", "gt_of_rois", "reg_valid", "cls_label", "segments", "class_count", "pose", "gt_local")
DEFAULTS = dict(roi_per_image=128, fg_ratio=0.5, reg_fg_thresh=0.55, cls_fg_thresh=0.75, cls_bg_thresh=0.25, cls_bg_thresh_lo=0.1, hard_bg_ratio=0.8,
                cls_score_type="roi_iou")


def settings(**changed):
    """The keyword arguments of tensors.sample_rois, the defaults with `changed`."""
    unknown = set(changed) - set(DEFAULTS)
    assert not unknown, unknown
    return {**DEFAULTS, **changed}


def fg_per_image(cfg):
    return int(np.round(cfg["fg_ratio"] * cfg["roi_per_image"]))


def words(seed, step, frame, n):
    """r_0 .. r_(n-1) of frame `frame`."""
    out = []
    for b in range((n + 3) // 4):
        out.extend(philox4x32_10(seed, step, frame, TAG + b))
    return out[:n]


def class_lists(cfg, rois, overlap, pose):
    """The ascending lists (fg, hard, easy) of one frame, as Python lists."""
    with np.errstate(invalid="ignore"):
        ov = overlap.astype(np.float64)
        cand = br.present(rois, pose) & ~np.isnan(ov)
        reg_fg, lo = cfg["reg_fg_thresh"], cfg["cls_bg_thresh_lo"]
        fg = cand & (ov >= min(reg_fg, cfg["cls_fg_thresh"]))
        hard = cand & (ov < reg_fg) & (ov >= lo)
        easy = cand & (ov < lo)
    return [np.flatnonzero(x).tolist() for x in (fg, hard, easy)]


def background(cfg, n, n_hard, n_easy):
    """(hard_this, easy_this) of n background picks."""
    if n_hard > 0 and n_easy > 0:
        hard_this = min(int(float(n) * cfg["hard_bg_ratio"]), n_hard)
        return hard_this, n - hard_this
    return (n if n_hard > 0 else 0), (n if n_easy > 0 else 0)


def picks(cfg, fg, hard, easy, r):
    """(the roi of every slot or -1, (fg_this, hard_this, easy_this), the branch 'a' .. 'd') from the class lists and the words r."""
    S, n_fg, n_hard, n_easy = cfg["roi_per_image"], len(fg), len(hard), len(easy)

    def with_replacement(lst, k):
        return lst[(r[k] * len(lst)) >> 32]
    if n_fg > 0 and n_hard + n_easy > 0:
        branch, fg_this, lst = "a", min(fg_per_image(cfg), n_fg), list(fg)
        for i in range(fg_this):
            j = i + ((r[i] * (n_fg - i)) >> 32)
            lst[i], lst[j] = lst[j], lst[i]
        slots = lst[:fg_this]
        hard_this, easy_this = background(cfg, S - fg_this, n_hard, n_easy)
    elif n_fg > 0:
        branch, fg_this, hard_this, easy_this = "b", S, 0, 0
        slots = [with_replacement(fg, k) for k in range(S)]
    elif n_hard + n_easy > 0:
        branch, fg_this, slots = "c", 0, []
        hard_this, easy_this = background(cfg, S, n_hard, n_easy)
    else:
        return [-1] * S, (0, 0, 0), "d"
    slots += [with_replacement(hard, k) for k in range(fg_this, fg_this + hard_this)]
    slots += [with_replacement(easy, k) for k in range(fg_this + hard_this, fg_this + hard_this + easy_this)]
    assert len(slots) == S
    return slots, (fg_this, hard_this, easy_this), branch


def cls_label(cfg, ov):
    fg, bg = cfg["cls_fg_thresh"], cfg["cls_bg_thresh"]
    if ov > fg:
        return 1.0
    if cfg["cls_score_type"] == "roi_iou":
        return 0.0 if ov < bg else (ov - bg) / (fg - bg)
    return -1.0 if bg < ov < fg else 0.0


def pmod(x):
    r = math.fmod(x, TWO_PI)
    if r < 0.0:
        r += TWO_PI
    return 0.0 if r == 0.0 else r


def heading_label(h_roi, h_gt, trace=None):
    """The heading label; trace, a list, receives the names of the branches taken."""
    note = (lambda s: None) if trace is None else trace.append
    ry = pmod(h_roi)
    hl = pmod(h_gt - ry)
    if HALF_PI < hl < THREE_HALF_PI:
        note("flipped")
        hl = pmod(hl + PI)
    else:
        note("kept")
    if hl > PI:
        note("wrapped")
        hl -= TWO_PI
    else:
        note("unwrapped")
    if hl < -HALF_PI or hl > HALF_PI:
        note("clamped")
    return min(max(hl, -HALF_PI), HALF_PI)


def gt_local(roi, c, s, gt, dtype, trace=None):
    """The seven values of the gt in the frame of the roi of pose (c, s), in `dtype`; zeros for a gt beyond the bounds."""
    g = [float(v) for v in gt[:7]]
    b = [float(v) for v in roi[:7]]
    if not all(abs(v) <= br.BOUND for v in g):                          # (false for NaN)
        return np.zeros(7, dtype)
    sx, sy, lz = g[0] - b[0], g[1] - b[1], g[2] - b[2]
    lx, ly = sx * c + sy * s, sy * c - sx * s
    out = np.array([lx, ly, lz, 0, 0, 0, heading_label(b[6], g[6], trace)], np.float64).astype(dtype)
    out[3:6] = gt[3:6]
    return out


def sample_rois(rois, gt_boxes, overlap, assignment, pose, cfg, seed, step, frames=None):
    """Every output of the stage as a dict of NumPy arrays.  pose: (F, M, 2) float64, used as it is.  frames: the frame numbers that key
    the draws, 0 .. F - 1 unless given."""
    rois, gt_boxes, overlap, assignment = (np.asarray(a) for a in (rois, gt_boxes, overlap, assignment))
    F, M, Cb = rois.shape
    B, Cg = gt_boxes.shape[1:]
    S, dt = cfg["roi_per_image"], rois.dtype
    assert gt_boxes.dtype == dt and overlap.dtype == dt and overlap.shape == (F, M) and assignment.shape == (F, M) and pose.shape == (F, M, 2)
    e = dict(index=np.full((F, S), -1, np.int32), rois=np.zeros((F, S, Cb), dt), roi_iou=np.zeros((F, S), dt), gt_index=np.full((F, S), -1, np.int32),
             gt_of_rois=np.zeros((F, S, Cg), dt), reg_valid=np.zeros((F, S), np.uint8), cls_label=np.full((F, S), -1, dt), segments=np.zeros((F, 3), np.int32),
             class_count=np.zeros((F, 3), np.int32), pose=np.zeros((F, S, 2), np.float64), gt_local=np.zeros((F, S, 7), dt))
    e["branch"] = []
    for f in range(F):
        fg, hard, easy = class_lists(cfg, rois[f], overlap[f], pose[f])
        slots, seg, branch = picks(cfg, fg, hard, easy, words(seed, step, f if frames is None else frames[f], S))
        e["segments"][f], e["class_count"][f] = seg, (len(fg), len(hard), len(easy))
        e["branch"].append(branch)
        for k, m in enumerate(slots):
            if m < 0:
                continue
            ov = float(overlap[f, m])
            a = int(assignment[f, m])
            a = a if 0 <= a < B else -1
            e["index"][f, k], e["rois"][f, k], e["roi_iou"][f, k], e["gt_index"][f, k] = m, rois[f, m], overlap[f, m], a
            e["reg_valid"][f, k] = ov > cfg["reg_fg_thresh"]
            e["cls_label"][f, k] = cls_label(cfg, ov)
            e["pose"][f, k] = pose[f, m]
            if a >= 0:
                e["gt_of_rois"][f, k] = gt_boxes[f, a]
                e["gt_local"][f, k] = gt_local(rois[f, m], float(pose[f, m, 0]), float(pose[f, m, 1]), gt_boxes[f, a], dt)
    return e


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def _boxes(rng, shape, C, dtype):
    """Random present boxes with C columns: centres within 60 m, car-like sizes, headings within +-7."""
    b = np.zeros(shape + (C,), np.float64)
    b[..., 0:2] = rng.uniform(-60, 60, shape + (2,))
    b[..., 2] = rng.uniform(-2, 1, shape)
    b[..., 3:6] = rng.uniform((3.0, 1.4, 1.3), (5.0, 2.2, 2.0), shape + (3,))
    b[..., 6] = rng.uniform(-7, 7, shape)
    b[..., 7:] = rng.integers(1, 4, shape + (C - 7,))
    return b.astype(dtype)


def _random(dtype, F, M, B, Cb, Cg, seed, nan_share=0.05, absent_share=0.1):
    """A batch with overlaps uniform in 0 .. 1, assignments in -1 .. B, some NaN overlaps and some zero rows."""
    rng = np.random.default_rng(seed)
    rois, gt = _boxes(rng, (F, M), Cb, dtype), _boxes(rng, (F, B), Cg, dtype)
    ov = rng.uniform(0, 1, (F, M)).astype(dtype)
    ov[rng.uniform(size=(F, M)) < nan_share] = np.nan
    rois[rng.uniform(size=(F, M)) < absent_share] = 0
    return rois, gt, ov, rng.integers(-1, B + 1, (F, M)).astype(np.int32)


DYADIC = dict(reg_fg_thresh=0.5, cls_fg_thresh=0.75, cls_bg_thresh=0.25, cls_bg_thresh_lo=0.125)      # (exact in float32: overlaps can sit ON them)
HEADING_PAIRS = (                    # (roi heading, gt heading): either side of every branch of the heading rule
    (0.0, 0.3), (0.0, 2.0), (0.0, 4.0), (0.0, 5.5), (0.0, -0.3), (1.0, 1.0), (-2.5, 0.4), (6.5, -6.5), (0.0, HALF_PI), (0.0, THREE_HALF_PI),
    (0.0, PI), (0.0, TWO_PI), (-7.0, 7.0), (3.0, 0.5), (0.25, 0.25 + PI), (-1e-20, 0.0), (0.0, -1e-20), (2.0, 2.0 - 1e-17))


def _spec(name):
    """(F, M, B, Cb, Cg, settings, seed, step) of a random case."""
    return {
        "m1": (2, 1, 1, 7, 7, settings(roi_per_image=1, fg_ratio=1.0), 3, 0),
        "m2": (3, 2, 1, 7, 8, settings(roi_per_image=4, fg_ratio=0.0), 4, 1),
        "m63": (2, 63, 65, 8, 8, settings(roi_per_image=5), 5, 2),
        "m64": (2, 64, 65, 9, 7, settings(roi_per_image=128, cls_score_type="cls"), 6, 3),
        "m65": (3, 65, 1, 10, 10, settings(roi_per_image=4, fg_ratio=1.0, cls_score_type="cls"), 7, (1 << 40) + 5),
        "m129": (2, 129, 65, 7, 8, settings(roi_per_image=128, reg_fg_thresh=0.75, cls_fg_thresh=0.5), 8, 4),
    }[name]


RANDOM_NAMES = ("m1", "m2", "m63", "m64", "m65", "m129")
CASE_NAMES = RANDOM_NAMES + ("branches", "edges", "headings", "full_walk")
BRANCH_FRAMES = dict(many_fg=0, few_fg=1, fg_only=2, hard_only=3, nothing=4, easy_only=5)


def _branches(dtype):
    """F = 6, M = 129, B = 65, S = 128, fg_per_image = 32, hard_bg_ratio 0.4: one frame per branch (BRANCH_FRAMES)."""
    F, M, B = 6, 129, 65
    rois, gt, _, assign = _random(dtype, F, M, B, 8, 8, 21, 0.0, 0.0)
    rng = np.random.default_rng(22)
    ov = np.zeros((F, M), np.float64)
    fr = BRANCH_FRAMES
    ov[fr["many_fg"]] = np.where(np.arange(M) % 3 == 0, rng.uniform(0.0, 0.05, M), np.where(np.arange(M) % 3 == 1, rng.uniform(0.6, 1.0, M), rng.uniform(0.2, 0.5, M)))
    ov[fr["few_fg"]] = rng.uniform(0.0, 0.09, M)                      # 10 fg, 5 hard, the rest easy: hard_this is clipped by n_hard
    ov[fr["few_fg"], 5:105:10] = rng.uniform(0.56, 1.0, 10)
    ov[fr["few_fg"], 7:107:20] = rng.uniform(0.11, 0.5, 5)
    ov[fr["fg_only"]] = rng.uniform(0.56, 1.0, M)
    ov[fr["hard_only"]] = rng.uniform(0.11, 0.5, M)
    ov[fr["nothing"]] = rng.uniform(0.0, 1.0, M)
    ov[fr["easy_only"]] = rng.uniform(0.0, 0.09, M)
    ov = ov.astype(dtype)
    ov[fr["many_fg"], [1, 4]] = np.nan                                   # would be fg: no candidates
    ov[fr["nothing"], ::2] = np.nan
    rois[fr["nothing"], 1::2] = 0                                        # ... and the other half absent
    rois[fr["many_fg"], 7] = 0                                           # absent rois that would be fg
    rois[fr["many_fg"], 10, 3] = -1.0
    rois[fr["few_fg"], 15, 0] = np.inf
    assign[fr["many_fg"], 13], assign[fr["many_fg"], 16], assign[fr["few_fg"], 25] = -1, B, -7
    return rois, gt, ov, assign, settings(fg_ratio=0.25, hard_bg_ratio=0.4), 31, 9


EDGE_VALUES = (0.5, 0.75, 0.25, 0.125)


def edge_overlaps(dtype):
    """Each of the four thresholds of DYADIC exactly, one step of the dtype below and above it, and the ends of the scale."""
    t = np.dtype(dtype).type
    values = []
    for v in EDGE_VALUES:
        values += [t(v), np.nextafter(t(v), t(0)), np.nextafter(t(v), t(1))]
    return np.array(values + [t(0), t(1), t(np.inf), t(-np.inf), t(-0.25)], dtype)


def _edges(dtype):
    """Overlaps exactly on each of the four thresholds (DYADIC) and one step of the dtype to either side.  The hard picks of a frame with
    easy rois beside them are n_hard draws with replacement, which need not reach every hard roi: frame 0 has no easy roi (those overlaps
    are 0.3 there) and frame 1 no hard one (0.0625 there), so S = 1024 picks reach every value in one of the two."""
    values = edge_overlaps(dtype)
    M = len(values) * 2
    rois, gt, _, _ = _random(dtype, 2, M, 65, 7, 8, 23, 0.0, 0.0)
    ov = np.tile(np.concatenate((values, values)), (2, 1))
    ov[0, ov[0] < 0.125] = 0.3
    ov[1, (ov[1] >= 0.125) & (ov[1] < 0.5)] = 0.0625
    assign = np.tile((np.arange(M) % 65).astype(np.int32), (2, 1))
    return rois, gt, ov, assign, settings(roi_per_image=1024, **DYADIC), 32, 2


def _headings(dtype):
    """Every roi an fg candidate assigned to its own gt, (roi heading, gt heading) = HEADING_PAIRS; S = 1024 with replacement from 64."""
    n = len(HEADING_PAIRS)
    M = B = 64
    rois, gt, _, _ = _random(dtype, 1, M, B, 7, 8, 24, 0.0, 0.0)
    for m in range(M):
        rois[0, m, 6], gt[0, m, 6] = HEADING_PAIRS[m % n]
    gt[0, 60, 0], gt[0, 61, 4], gt[0, 62, 6] = np.nan, np.inf, 2e6                       # gts beyond the bounds: zeros
    gt[0, 63, 3] = -1.0                                                                 # (a size need not be positive)
    ov = np.full((1, M), 0.9, dtype)
    assign = np.arange(M, dtype=np.int32)[None].copy()
    assign[0, 59] = -1
    return rois, gt, ov, assign, settings(roi_per_image=1024), 33, 3


def _full_walk(dtype):
    """M = 9216, S = fg_per_image = 1024, n_fg > 1024 and background beside it: a walk of 1024 steps."""
    rois, gt, ov, assign = _random(dtype, 2, 9216, 1, 7, 7, 25)
    return rois, gt, ov, assign, settings(roi_per_image=1024, fg_ratio=1.0), 34, 1


@lru_cache(maxsize=None)
def case(name, dtype):
    """dict(rois, gt_boxes, overlap, assignment, pose, cfg, seed, step) of a named case; pose is NumPy's."""
    if name in RANDOM_NAMES:
        F, M, B, Cb, Cg, cfg, seed, step = _spec(name)
        rois, gt, ov, assign = _random(dtype, F, M, B, Cb, Cg, 100 + seed)
    else:
        rois, gt, ov, assign, cfg, seed, step = {"branches": _branches, "edges": _edges, "headings": _headings, "full_walk": _full_walk}[name](dtype)
    c = dict(rois=np.ascontiguousarray(rois), gt_boxes=np.ascontiguousarray(gt), overlap=np.ascontiguousarray(ov), assignment=np.ascontiguousarray(assign),
             pose=np.ascontiguousarray(br.numpy_pose(rois)), cfg=cfg, seed=seed, step=step)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def expected_of(c, **changed):
    """The restatement on a case, with some of its entries replaced."""
    c = {**c, **changed}
    return sample_rois(c["rois"], c["gt_boxes"], c["overlap"], c["assignment"], c["pose"], c["cfg"], c["seed"], c["step"], c.get("frames"))


@lru_cache(maxsize=None)
def expected(name, dtype):
    return expected_of(case(name, dtype))
