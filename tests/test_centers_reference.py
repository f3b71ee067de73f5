"""Centre heatmap targets without a GPU: the conditions under which the comparisons of tests/test_gpu_centers.py are not vacuous, asserted
on the shared cases of tests/centers_reference.py; how far every value a Gaussian can take stays from the float32 rounding midpoints;
csrc/sg_centers.h compiled for the host (tests/host_harness/centers_walk.cpp) against the restatement, byte for byte; what
snowgpu_assign_centers_device refuses, in which words and in which order (tests/host_harness/centers_refusals.cpp); and that the entry
is declared and bound."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import centers_reference as cr
from conftest import ROOT
from lidar_snow_sim_amd.stages import CenterTargetBatch, assign_centers  # noqa: F401  (the stage all of this is about: without it nothing here runs)

DTYPES = cr.DTYPES
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
f32 = np.float32


# ---- the shared cases meet the conditions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_by_hand(dtype):
    """g0 at (3.5, 4.25): pixel (3, 4), offset (0.5, 0.25), radius 2 = min_radius (its root is 0.43), d = 5, sigma = 5 / 6, den = 25 / 18:
    the value at squared distance s is exp(-0.72 s).  g1 of class 2 at pixel (5, 4): channel 1 holds the same patch two pixels to the
    right, cut at the map's last column, and neither channel knows of the other's gt."""
    e = cr.expected("by_hand", dtype)
    v = {s: f32(np.exp(-0.72 * s)) for s in (0, 1, 2, 4, 5, 8)}
    assert v[0] == 1 and [float(v[s]) for s in (1, 2, 4, 5, 8)] == pytest.approx([0.48675224, 0.23692776, 0.05613476, 0.02732372, 0.00315111], rel=1e-6)
    patch = [[v[8], v[5], v[4], v[5], v[8]],
             [v[5], v[2], v[1], v[2], v[5]],
             [v[4], v[1], v[0], v[1], v[4]],
             [v[5], v[2], v[1], v[2], v[5]],
             [v[8], v[5], v[4], v[5], v[8]]]
    want = np.zeros((1, 2, 8, 8), f32)
    want[0, 0, 2:7, 1:6] = patch
    want[0, 1, 2:7, 3:8] = patch
    assert e["heatmap"].dtype == f32 and e["heatmap"].tobytes() == want.tobytes()
    assert e["gt_index"][0, 0, :3].tolist() == [0, 1, -1] and e["ind"][0, 0, :3].tolist() == [4 * 8 + 3, 4 * 8 + 5, 0] and e["mask"][0, 0, :3].tolist() == [1, 1, 0]
    assert e["offset"].dtype == np.dtype(dtype) and e["offset"][0, 0, :3].tolist() == [[0.5, 0.25], [0.5, 0.5], [0, 0]]
    assert e["radius"][0, 0, :3].tolist() == [2, 2, 0] and e["count"].tolist() == [[2]] and e["state"].tolist() == [[1, 1]]
    assert e["gt_index"].shape == (1, 1, 500) and (e["gt_index"][0, 0, 2:] == -1).all() and not e["mask"][0, 0, 2:].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cr.EDGE_NAMES)
def test_edges(name, dtype):
    c, e = cr.case(name, dtype), cr.expected(name, dtype)
    G, (W, H) = cr.EDGE_GTS, (cr.EDGE_W, cr.EDGE_H)
    drop, below = c["outside"] == "drop", c["point_cloud_range"][0] != 0
    coord, state = e["coord"][0], e["state"][0]
    t = np.dtype(dtype).type
    # the integer itself and the last value below it: of the dtype with the origin at 0, of float64 (by the subtraction) with the origin 2^-51
    if below:
        assert coord[G["whole"], 0] == np.nextafter(3.0, 0.0) and coord[G["whole"], 1] < 2.0 and coord[G["below_0"], 0] < 0
    else:
        assert coord[G["whole"]].tolist() == [3.0, 2.0] and coord[G["last_below"]].tolist() == [float(np.nextafter(t(3), t(0))), float(np.nextafter(t(2), t(0)))]
    slot = {int(g): k for k, g in enumerate(e["gt_index"][0, 0]) if g >= 0}
    pix = lambda name: divmod(int(e["ind"][0, 0, slot[G[name]]]), W)[::-1]              # noqa: E731  ((cix, ciy))
    assert pix("whole") == ((2, 1) if below else (3, 2)) and pix("last_below") == (2, 1)
    if below:                                                   # 1 - 2^-51 rounds to 1 in float32 and stays below 1 in float64
        off = e["offset"][0, 0, slot[G["whole"]], 0]
        assert off == (1.0 if dtype == "float32" else 1.0 - 2.0 ** -51)
    # outside the map: clamped onto its border, or dropped
    outside = ("below_0", "at_w", "beyond_w", "at_h", "below_0_y")
    assert all(not (0 <= coord[G[n], 0] < W and 0 <= coord[G[n], 1] < H) for n in outside)
    if drop:
        assert all(state[G[n]] == cr.DROPPED for n in outside) and (state == cr.DROPPED).sum() == len(outside) and e["count"][0, 0] == len(G) - len(outside)
    else:
        assert (state == cr.DRAWN).all()
        assert pix("below_0")[0] == 0 and pix("at_w")[0] == pix("beyond_w")[0] == W - 1 and pix("at_h")[1] == H - 1 and pix("below_0_y")[1] == 0       # both ends
        assert e["offset"][0, 0, slot[G["below_0"]], 0] == 0 and e["offset"][0, 0, slot[G["at_w"]], 0] == 0.5 and e["offset"][0, 0, slot[G["at_h"]], 1] == 0.5
    # W - 0.5 itself, and between it and W: inside under either setting, the latter clamped
    assert coord[G["at_w_half"], 0] == W - 0.5 - (cr.BELOW if below else 0) and W - 0.5 < coord[G["inside_last_half"], 0] < W
    assert state[G["at_w_half"]] == state[G["inside_last_half"]] == cr.DRAWN and pix("inside_last_half")[0] == W - 1
    assert e["offset"][0, 0, slot[G["inside_last_half"]], 0] == 0.5
    # patches cut at each border and at two corners: the radius 2 does not fit
    for n, cut in (("left", "x0"), ("right", "x1"), ("top", "y0"), ("bottom", "y1"), ("corner", "x0y0"), ("far_corner", "x1y1")):
        x, y = pix(n)
        assert ("x0" in cut) == (x - 2 < 0) and ("x1" in cut) == (x + 2 > W - 1) and ("y0" in cut) == (y - 2 < 0) and ("y1" in cut) == (y + 2 > H - 1), n
        assert e["radius"][0, 0, slot[G[n]]] == 2 and e["heatmap"][0, int(c["gt_boxes"][0, G[n], 7]) - 1, y, x] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiles(dtype):
    c, e = cr.case("tiles", dtype), cr.expected("tiles", dtype)
    W, H = c["feature_map_size"]
    assert (W, H) == (70, 19) and W % cr.TILE_W and H % cr.TILE_H and W > cr.TILE_W and H > cr.TILE_H
    tiles_of = []
    for k in range(6):
        r, (y, x) = int(e["radius"][0, 0, k]), divmod(int(e["ind"][0, 0, k]), W)
        xs, ys = range(max(x - r, 0), min(x + r, W - 1) + 1), range(max(y - r, 0), min(y + r, H - 1) + 1)
        tiles_of.append({(px // cr.TILE_W, py // cr.TILE_H) for px in xs for py in ys})
    assert [len(t) for t in tiles_of] == [4, 4, 1, 2, 4, 2] and e["radius"][0, 0, :6].tolist() == [3, 3, 3, 3, 40, 3]
    assert divmod(int(e["ind"][0, 0, 2]), W) == (8, 60) and 60 + 3 == cr.TILE_W - 1                 # ends on the tile's last column
    assert divmod(int(e["ind"][0, 0, 3]), W) == (H - 1, W - 1)
    assert (e["covered"][0, 2] > 0).sum() > 0.6 * W * H and (e["heatmap"][0, 0] == 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_map(dtype):
    e = cr.expected("whole_map", dtype)
    assert e["root"][0, 0] > 1700 and e["radius"][0, 0, 0] == cr.RADIUS_MAX and (e["covered"][0, 0] == 1).all() and (e["heatmap"][0, 0] > 0.8).all()
    assert (e["heatmap"][0, 0] == 1).sum() == 1 and len(np.unique(e["heatmap"][0, 0])) > 700


@pytest.mark.parametrize("dtype", DTYPES)
def test_radius(dtype):
    """Both sides of the truncation at three integers, by two adjacent values of the dtype; min_radius in place of a smaller root.  Which root
    is the minimum: r3 <= 2 sqrt(o (1 - o) w h) <= sqrt(w h) <= (h + w) / 2 <= r1 <= r2 for every 0 < o < 1, so r1 and r2 can never be --
    asserted here over every present gt of every case, so that the two comparisons of the minimum are at least met from the side they have."""
    c, e = cr.case("radius", dtype), cr.expected("radius", dtype)
    t = np.dtype(dtype).type
    for i, k in enumerate(cr.RADIUS_KS):
        lo, hi = c["gt_boxes"][0, 2 * i, 3], c["gt_boxes"][0, 2 * i + 1, 3]
        assert hi == np.nextafter(lo, t(np.inf)) and lo.dtype == np.dtype(dtype)
        assert e["root"][0, 2 * i] < k <= e["root"][0, 2 * i + 1] and e["root"][0, 2 * i] > k - 1e-3
        assert e["radius"][0, 0, 2 * i: 2 * i + 2].tolist() == [k - 1, k]
    n = 2 * len(cr.RADIUS_KS)
    assert 0 < e["root"][0, n] < 1 < e["root"][0, n + 1] < 2 == c["min_radius"] and e["radius"][0, 0, n:n + 2].tolist() == [2, 2]
    seen = 0
    for name in cr.CASE_NAMES:
        cc, ee = cr.case(name, dtype), cr.expected(name, dtype)
        vx, vy, st = cc["voxel_size"][0], cc["voxel_size"][1], cc["stride"]
        for f, g in zip(*np.nonzero(np.isfinite(ee["root"]))):
            r1, r2, r3 = cr.roots((np.float64(cc["gt_boxes"][f, g, 3]) / vx) / st, (np.float64(cc["gt_boxes"][f, g, 4]) / vy) / st, cc["gaussian_overlap"])
            assert r3 < r1 <= r2 and ee["root"][f, g] == r3
            seen += 1
    assert seen > 500


@pytest.mark.parametrize("dtype", DTYPES)
def test_overlap(dtype):
    e = cr.expected("overlap", dtype)
    owner, first, covered = e["owner"][0, 0], e["first"][0, 0], e["covered"][0, 0]
    assert e["radius"][0, 0, :7].tolist() == [3, 3, 2, 2, 4, 4, 3]
    later = (owner != first) & (covered >= 2)
    assert {1, 2, 4} <= set(owner[later].tolist()) and (covered == 3).any() and (owner[covered == 3] == 2).any()       # two and three patches on a pixel
    assert ((owner == 0) & (covered >= 2)).any() and ((owner == 1) & (covered >= 2)).any()
    # equal centres: g3, g4 and g5 share pixel (18, 5); the wider g4 decides g3's patch but for the centre, g5 nothing
    assert e["ind"][0, 0, 3] == e["ind"][0, 0, 4] == e["ind"][0, 0, 5] == 5 * 24 + 18
    assert owner[5, 18] == 3 and (owner[3:8, 16:21] == 4).sum() == 24 and not (owner == 5).any() and (covered[3:8, 16:21] == 3).all()
    assert (e["owner"][0, 1] == 6).sum() == 49 and e["heatmap"][0, 1, 8, 8] == 1 and e["heatmap"][0, 0, 8, 8] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_slots(dtype):
    c, e = cr.case("slots", dtype), cr.expected("slots", dtype)
    assert c["gt_boxes"].shape == (3, 256, 8) and c["max_objs"] == 4 and tuple(c["class_head"]) == (0, 1, 0)
    s0 = e["state"][0]
    assert e["gt_index"][0].tolist() == [[63, 64, 127, 128], [5, 100, 200, -1]] and e["count"][0].tolist() == [4, 3]
    assert np.flatnonzero(s0 == cr.NO_SLOT).tolist() == [191, 192, 255] and (s0 == cr.DRAWN).sum() == 7 and (s0 == cr.ABSENT).sum() == 246
    assert (s0[[3, 62, 65, 126, 129, 190, 193, 254]] == cr.ABSENT).all() and c["gt_boxes"][0, [3, 62, 65, 126, 129, 190, 193, 254]].any(axis=1).all()
    assert not e["state"][1].any() and not e["heatmap"][1].any() and (e["gt_index"][1] == -1).all() and e["count"][1].tolist() == [0, 0]
    assert c["gt_boxes"][1].any()
    assert e["gt_index"][2].tolist() == [[64, 128, 192, 255], [0, 63, 127, 191]] and (e["state"][2] == cr.DRAWN).sum() == 8 and e["count"][2].tolist() == [4, 4]
    assert {g // 64 for g in (64, 128, 192, 255)} == {1, 2, 3} and {g // 64 for g in (0, 63, 127, 191)} == {0, 1, 2}
    assert e["heatmap"][0].any(axis=(1, 2)).all() and e["mask"].sum() == 15


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep(dtype):
    assert len(cr.SWEEP_NAMES) == 40
    states, shapes, later, settings = set(), set(), 0, set()
    for name in cr.SWEEP_NAMES:
        c, e = cr.case(name, dtype), cr.expected(name, dtype)
        F, B, Cg = c["gt_boxes"].shape
        W, H = c["feature_map_size"]
        assert F <= 3 and B <= 40 and W <= 96 and H <= 96 and c["n_classes"] <= 4
        states |= set(e["state"].reshape(-1).tolist())
        shapes.add((F, Cg, W > cr.TILE_W, H > cr.TILE_H, max(c["class_head"]) + 1))
        settings.add((c["outside"], c["stride"], c["min_radius"]))
        later += int(((e["owner"] != e["first"]) & (e["covered"] >= 2)).sum())
    assert states == {0, 1, 2, 3} and later > 100
    assert {s[0] for s in shapes} == {1, 2, 3} and {s[1] for s in shapes} == {8, 9, 10} and {s[2] for s in shapes} == {s[3] for s in shapes} == {False, True}
    assert {s[4] for s in shapes} >= {1, 2, 3} and {s[0] for s in settings} == {"clamp", "drop"} and {s[1] for s in settings} == {1, 2, 4, 8}


def test_every_state_and_both_clamps_are_met():
    states = set()
    for name in cr.NAMED:
        states |= set(cr.expected(name, "float32")["state"].reshape(-1).tolist())
    assert states == {cr.ABSENT, cr.DRAWN, cr.DROPPED, cr.NO_SLOT}
    assert {"by_hand", "tiles", "whole_map", "radius", "overlap", "slots"} <= set(cr.CASE_NAMES) and len(cr.EDGE_NAMES) == 4


# ---- the margin of the Gaussian ---------------------------------------------------------------------------------------------------------------
def test_every_gaussian_value_is_far_from_a_float32_midpoint():
    """Every radius 0 .. 512 and every distinct ex ex + ey ey of its patch: the float64 value of NumPy's exp lies more than 4 float64 ulp
    from every float32 rounding midpoint -- one ulp for NumPy's exp, one for the device library's, two spare --, so that the two faithful
    exps round to the same float32; and the smallest value is far above 2^-52, the level of gaussian2D's rule that the definition omits."""
    worst, where, smallest, n = np.inf, None, np.inf, 0
    for r in range(cr.RADIUS_MAX + 1):
        sq = np.arange(r + 1, dtype=np.int64) ** 2
        seen = np.zeros(2 * r * r + 1, bool)
        seen[(sq[:, None] + sq[None, :]).reshape(-1)] = True
        s = np.flatnonzero(seen)
        d = np.float64(2 * r + 1)
        sigma = d / 6
        den = 2 * sigma * sigma
        v = np.exp(np.divide(np.negative(s.astype(np.float64)), den))
        f = v.astype(f32)
        up, dn = np.nextafter(f, f32(np.inf)).astype(np.float64), np.nextafter(f, f32(-np.inf)).astype(np.float64)
        f = f.astype(np.float64)
        dist = np.minimum((f + up) / 2 - v, v - (f + dn) / 2) / np.spacing(v)
        assert (dist >= 0).all()
        k = int(dist.argmin())
        if dist[k] < worst:
            worst, where = float(dist[k]), (r, int(s[k]))
        smallest, n = min(smallest, float(v.min())), n + len(s)
    print(f"margin {worst} float64 ulp at radius {where[0]}, squared distance {where[1]}; {n} values; smallest {smallest}")
    assert n > 14_000_000 and worst > 4.0
    assert 1.2e-4 < smallest < 1.3e-4 and smallest > 1e9 * 2.0 ** -52


# ---- csrc/sg_centers.h on the host --------------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra, "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / "centers_walk.cpp"), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("centers"), "centers_walk")


def _walk(exe, tmp_path, c):
    """The outputs of the harness on case c, as a dict of arrays shaped like the restatement's."""
    gt = c["gt_boxes"]
    F, B, Cg = gt.shape
    W, H = c["feature_map_size"]
    NC, M = c["n_classes"], c["max_objs"]
    heads = list(c["class_head"] or [0] * NC)
    NH = max(heads) + 1
    fin, fout = tmp_path / "case.in", tmp_path / "case.out"
    fin.write_bytes(np.ascontiguousarray(gt).tobytes())
    args = [int(gt.dtype == np.float64), F, B, Cg, *(repr(float(v)) for v in (*c["point_cloud_range"][:2], *c["voxel_size"][:2])), c["stride"], W, H, NC, NH, M,
            repr(float(c["gaussian_overlap"])), c["min_radius"], int(c["outside"] == "drop"), *heads]
    r = subprocess.run([str(exe), *(str(a) for a in args), str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    shapes = dict(heatmap=((F, NC, H, W), f32), gt_index=((F, NH, M), np.int32), ind=((F, NH, M), np.int32), mask=((F, NH, M), np.uint8),
                  offset=((F, NH, M, 2), gt.dtype), radius=((F, NH, M), np.int32), count=((F, NH), np.int32), state=((F, B), np.uint8))
    blob, at, got = fout.read_bytes(), 0, {}
    for name in cr.FIELDS:
        shape, kind = shapes[name]
        n = int(np.prod(shape)) * np.dtype(kind).itemsize
        got[name] = np.frombuffer(blob[at:at + n], kind).reshape(shape)
        at += n
    assert at == len(blob)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_header_on_the_host_equals_the_restatement(walk, tmp_path, dtype):
    for name in cr.CASE_NAMES:
        c, e = cr.case(name, dtype), cr.expected(name, dtype)
        got = _walk(walk, tmp_path, c)
        for field in cr.FIELDS:
            assert got[field].dtype == e[field].dtype and got[field].tobytes() == e[field].tobytes(), (name, field)


def test_the_header_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UBSan -- host code only, a stand-alone program: the records, the slots and the pixels stay
    inside their arrays at B = 256, with every kind of absent box, with patches cut at every border and with the radius at its cap."""
    exe = _compile(tmp_path, "centers_walk_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name, dtype in (("slots", "float64"), ("edges_clamp_below", "float32"), ("edges_drop_origin0", "float64"), ("whole_map", "float32"), ("tiles", "float32"),
                        ("sweep_07", "float32")):
        c, e = cr.case(name, dtype), cr.expected(name, dtype)
        got = _walk(exe, tmp_path, c)
        for field in cr.FIELDS:
            assert got[field].tobytes() == e[field].tobytes(), (name, dtype, field)


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_assign_centers_device"
APART = "; the gt boxes are read while the targets are written: pass a buffer apart from them"
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "gt": WHO + ": n_gt must lie in 1 .. 256",
    "gt_features": WHO + ": gt_features must lie in 8 .. 10: cx, cy, cz, dx, dy, dz, heading, class first",
    "classes": WHO + ": n_classes must lie in 1 .. 16",
    "heads": WHO + ": n_heads must lie in 1 .. 16",
    "class_head": WHO + ": every class needs a head in 0 .. n_heads - 1",
    "objs": WHO + ": max_objs must lie in 1 .. 512",
    "map": WHO + ": the feature map needs at least one pixel on either axis",
    "elements": WHO + ": n_frames * n_classes * height * width exceeds 2^31 - 1; split the batch",
    "voxel": WHO + ": the origin of the range must be finite, the voxel's x and y edges positive and finite",
    "stride": WHO + ": stride must be at least 1",
    "overlap": WHO + ": gaussian_overlap must lie strictly between 0 and 1",
    "min_radius": WHO + ": min_radius must lie in 0 .. 512",
    "outside": WHO + ": outside must be 0 (clamp) or 1 (drop)",
}
ORDER = tuple(MESSAGES)              # the order of the checks: a call wrong in two ways gets the earlier message
DOUBLY = ("null_gt_boxes_and_gt_0", "gt_0_and_gt_features_7", "gt_features_7_and_classes_0", "classes_17_and_heads_0", "heads_17_and_head_negative",
          "head_negative_and_objs_0", "objs_513_and_height_negative", "height_negative_and_map_overflowing", "elements_at_2p31_and_vx_0", "vx_0_and_stride_0",
          "stride_0_and_overlap_0", "overlap_0_and_min_radius_513", "min_radius_513_and_outside_2", "outside_2_and_heatmap_is_gt_boxes")       # one per check and the one behind it
PAIRS = {"heatmap": ("heatmap_is_gt_boxes", "heatmap_overlaps_gt_boxes"), "gt_index": ("gt_index_overlaps_gt_boxes",), "ind": ("ind_is_gt_boxes",),
         "mask": ("mask_overlaps_gt_boxes",), "offset": ("offset_is_gt_boxes",), "radius": ("radius_overlaps_gt_boxes",), "count": ("count_is_gt_boxes",),
         "state": ("state_overlaps_gt_boxes",)}
OUTS = {("gt_index", "heatmap"): ("gt_index_is_heatmap",), ("ind", "gt_index"): ("ind_overlaps_gt_index",), ("mask", "ind"): ("mask_is_ind",),
        ("offset", "mask"): ("offset_overlaps_mask",), ("radius", "offset"): ("radius_is_offset",), ("count", "radius"): ("count_overlaps_radius",),
        ("state", "count"): ("state_is_count",), ("state", "heatmap"): ("state_overlaps_heatmap",)}
ACCEPTED = ("clean", "float64", "gt_1", "gt_256", "gt_features_10", "classes_1", "classes_16", "heads_16", "a_head_beyond_nc_is_not_read", "objs_1", "objs_512",
            "map_1x1", "elements_at_2p31_minus_1", "stride_1", "overlap_just_below_1", "min_radius_0", "min_radius_512", "outside_drop", "heatmap_behind_gt_boxes",
            "mask_behind_gt_boxes", "ind_behind_gt_index", "offset_behind_mask")
REFUSED = {
    "null": ("null_gt_boxes", "null_cfg", "null_out_heatmap", "null_out_gt_index", "null_out_ind", "null_out_mask", "null_out_offset", "null_out_radius",
             "null_out_count", "null_out_state", "bad_dtype", "no_frames", "null_gt_boxes_and_gt_0"),
    "gt": ("gt_0", "gt_257", "gt_0_and_gt_features_7"),
    "gt_features": ("gt_features_7", "gt_features_11", "gt_features_7_and_classes_0"),
    "classes": ("classes_0", "classes_17", "classes_17_and_heads_0"),
    "heads": ("heads_0", "heads_17", "heads_17_and_head_negative"),
    "class_head": ("head_negative", "head_at_n_heads", "head_negative_and_objs_0"),
    "objs": ("objs_0", "objs_513", "objs_513_and_height_negative"),
    "map": ("width_0", "height_negative", "height_negative_and_map_overflowing"),
    "elements": ("elements_at_2p31", "map_overflowing", "elements_at_2p31_and_vx_0"),
    "voxel": ("vx_0", "vy_negative", "vx_nan", "vy_inf", "x0_nan", "y0_inf", "vx_0_and_stride_0"),
    "stride": ("stride_0", "stride_0_and_overlap_0"),
    "overlap": ("overlap_0", "overlap_1", "overlap_nan", "overlap_0_and_min_radius_513"),
    "min_radius": ("min_radius_negative", "min_radius_513", "min_radius_513_and_outside_2"),
    "outside": ("outside_2", "outside_negative", "outside_2_and_heatmap_is_gt_boxes"),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "centers_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "centers_refusals.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split("|", 1) for ln in r.stdout.splitlines())
    want = {case: "0|OK" for case in ACCEPTED}
    for key, cases in REFUSED.items():
        want.update({case: "1|" + MESSAGES[key] for case in cases})
    for out, cases in PAIRS.items():
        want.update({case: f"1|{WHO}: d_out_{out} overlaps d_gt_boxes{APART}" for case in cases})
    for (out, other), cases in OUTS.items():
        want.update({case: f"1|{WHO}: d_out_{out} overlaps d_out_{other}{OWN}" for case in cases})
    assert got == want
    assert set(MESSAGES) == set(REFUSED) and set(PAIRS) == set(cr.FIELDS)              # every message is reached, every output is held apart from the input
    # the order: the checks stand in sg_check_centers_args in the order of MESSAGES, the overlaps behind them -- every "<first>_and_<second>"
    # case of the harness is wrong in two ways, of checks next to each other, and is filed above under the earlier one
    for key, later, case in zip(ORDER, ORDER[1:] + (None,), DOUBLY):
        first, second = case.split("_and_")
        assert first in REFUSED[key] and case in REFUSED[key], case
        assert second in REFUSED[later] if later else any(second in cases for cases in PAIRS.values()), case


def test_the_entry_is_declared_and_bound():
    from lidar_snow_sim_amd import _native
    header = (ROOT / "include" / "snowgpu.h").read_text()
    assert "int snowgpu_assign_centers_device(" in header and "typedef struct snowgpu_center_cfg {" in header and "snowgpu_assign_centers_device" in _native.EXPORTS
    assert "NOT CHECKED against pcdet" in header[header.index("CENTRE HEATMAP TARGETS"):header.index("typedef struct snowgpu_center_cfg")]
    assert hasattr(_native.lib(), "snowgpu_assign_centers_device") and hasattr(_native.Context, "assign_centers_device")
    assert "snowgpu_centers.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import centers, stages, tensors
    assert tensors.assign_centers is stages.assign_centers and tensors.CenterTargetBatch is stages.CenterTargetBatch and "assign_centers(" in tensors.__doc__
    assert callable(centers.assign_targets) and tuple(centers.FIELDS) == tuple(cr.FIELDS) == tuple(CenterTargetBatch.FIELDS)
    assert callable(CenterTargetBatch.empty) and callable(CenterTargetBatch.target_boxes) and callable(CenterTargetBatch.head_heatmap)
    assert stages.CENTER_STATES == dict(absent=cr.ABSENT, drawn=cr.DRAWN, dropped=cr.DROPPED, no_slot=cr.NO_SLOT)
    # the struct Python fills is the header's, field for field
    fields = [n for n, _ in _native.CenterCfgStruct._fields_]
    assert fields == ["x0", "y0", "vx", "vy", "gaussian_overlap", "stride", "width", "height", "n_classes", "n_heads", "max_objs", "min_radius", "outside", "class_head"]
    import ctypes
    assert ctypes.sizeof(_native.CenterCfgStruct) == 5 * 8 + 8 * 4 + 16 * 4
