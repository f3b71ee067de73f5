"""The scene transforms without a GPU: the restatement (tests/scene_reference.py) on a frame worked by hand; the conditions that keep the
GPU comparisons from being vacuous, asserted on the shared cases; csrc/sg_scene.h compiled for the host
(tests/host_harness/scene_sweep.cpp) against the restatement, byte for byte, fed the same cos / sin, and once under sanitizers; what
snowgpu_transform_scene_device refuses, in which words and in which order (tests/host_harness/scene_refusals.cpp); and that the entry is
declared and bound."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import box_reference as br
import iou_reference as ir
import scene_reference as sr

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
G = sr.GROUP
ALL_CASES = sr.CASE_NAMES + tuple(sr.OFF)


def test_the_restatement_on_a_frame_by_hand():
    """One frame, one box, no local part, flip about x asked for, theta = pi / 2 exactly in range (lo = hi), sigma = 2: a row at (1, 2, 3)
    becomes (x cos - y sin, x sin + y cos, z) 2 after y = -y if the frame is flipped; the box likewise; an absent row and a row beyond
    1e6 keep their bytes."""
    rows = np.array([[1, 2, 3, 9, 1], [np.nan, 0, 0, 8, 2], [1e7, 1, 1, 7, 3]], np.float64)
    keep = np.array([1, 0, 1], bool)
    gt = np.array([[[4, 1, 0, 2, 1, 1, 0.25, 3, 5]]], np.float64)
    cfg = sr.config(("x",), (math.pi / 2, math.pi / 2), (2.0, 2.0))
    for step in range(8):
        e = sr.transform_scene(rows, [0, 3], keep, gt, br.numpy_pose(gt), cfg, seed=1, step=step)
        fx, fy, c, s, th, sg = e["world"][0, :6]
        assert fy == 0.0 and th == math.pi / 2 and sg == 2.0 and (c, s) == (math.cos(th), math.sin(th))
        y = -2.0 if fx else 2.0
        assert e["rows"][0].tolist() == [(1.0 * c - y * s) * 2.0, (1.0 * s + y * c) * 2.0, 6.0, 9.0, 1.0]
        assert e["rows"][1:].tobytes() == rows[1:].tobytes() and e["keep"].tolist() == [True, False, True]
        cy, h = (-1.0, -0.25) if fx else (1.0, 0.25)
        assert e["gt_boxes"][0, 0].tolist() == [(4.0 * c - cy * s) * 2.0, (4.0 * s + cy * c) * 2.0, 0.0, 4.0, 2.0, 2.0, h + th, 3.0, 5.0]
        assert e["state"].tolist() == [[0]] and e["tried"].tolist() == [[-1]] and e["local"][0, 0].tolist() == list(sr.IDENTITY) and e["tries"].shape == (1, 1, 0, 8)
    assert {sr.world_draw(cfg, 1, step, 0)[0] for step in range(8)} == {0.0, 1.0}


def test_words_are_the_weather_draws_positions():
    """Block 0 is the world's; blocks 1 + 2 (i T + t) and the next are try t of box i; step in the index, the frame in the group."""
    from seeded_reference import philox4x32_10
    cfg = sr.config(("x", "y"), (0.0, 1.0), (1.0, 2.0), dict(translation=(1.0, 1.0, 1.0), rotation=(0.0, 1.0), scaling=(1.0, 2.0), tries=4))
    step = (1 << 40) + 3
    w = philox4x32_10(11, step, 2, 0x5846524D)
    assert sr.world_draw(cfg, 11, step, 2) == (float(w[0] < 2 ** 31), float(w[1] < 2 ** 31), 0.0 + (w[2] * 2.0 ** -32) * 1.0, 1.0 + (w[3] * 2.0 ** -32) * 1.0)
    a, b = philox4x32_10(11, step, 2, 0x5846524D + 1 + 2 * (5 * 4 + 3)), philox4x32_10(11, step, 2, 0x5846524D + 2 + 2 * (5 * 4 + 3))
    assert sr.try_draw(cfg, 11, step, 2, 5, 3) == (*(-1.0 + (a[j] * 2.0 ** -32) * 2.0 for j in range(3)), (a[3] * 2.0 ** -32) * 1.0, 1.0 + (b[0] * 2.0 ** -32) * 1.0)


def _area(a, pa, b, pb):
    return float(ir.clip_area(np.asarray(a, np.float64)[None], np.asarray(pa, np.float64)[None], np.asarray(b, np.float64)[None], np.asarray(pb, np.float64)[None])[0])


@pytest.mark.parametrize("dtype", sr.DTYPES)
def test_every_constructed_situation_occurs_and_decides(dtype):
    c, e = sr.case("constructed", dtype), sr.expected("constructed", dtype)
    st, tk, tr = e["state"][0].tolist(), e["tried"][0].tolist(), e["tries"][0]
    assert set(st) == {0, 1, 2}                                          # every state
    assert e["world"][0, :2].tolist() == [1.0, 1.0]                     # flipped about both axes
    assert tk[G["free"]] == 0 and st[G["free"]] == 1                    # the first try is free
    assert tk[G["third"]] == 2 and tr[G["third"], :3, 7].tolist() == [1.0, 1.0, 0.0]      # the third try is the first free one
    assert st[G["walled"]] == 2 and tk[G["walled"]] == -1 and tr[G["walled"], :, 7].all()                      # every try collides
    assert st[G["zero"]] == st[G["nan"]] == 0 and not br.present(c["gt_boxes"][0, [G["zero"], G["nan"]]], c["pose"][0, [G["zero"], G["nan"]]]).any()

    def without(i):
        gt = c["gt_boxes"].copy()
        gt[0, i] = 0
        return sr.expected_of(c, gt_boxes=gt, pose=br.numpy_pose(gt))

    # blocked only by an EARLIER box's moved position: box 6 took try 0; box 7's try 0 meets the moved box 6, not the original, and is free without it
    a, b = G["earlier"], G["earlier"] + 1
    assert tk[a] == 0 and tk[b] > 0 and tr[b, 0, 7] == 1.0 and without(a)["tried"][0, b] == 0
    g, p = c["gt_boxes"][0, :, :7].astype(np.float64), c["pose"][0]
    cand = g[b].copy()
    cand[:3] += tr[b, 0, :3]
    cand[3:6] *= tr[b, 0, 6]
    cand_cs = (p[b, 0] * tr[b, 0, 3] - p[b, 1] * tr[b, 0, 4], p[b, 1] * tr[b, 0, 3] + p[b, 0] * tr[b, 0, 4])
    assert _area(cand, cand_cs, g[a], p[a]) == 0.0                      # the ORIGINAL box 6 is out of its way
    # blocked only by a LATER box's original position: box 9 sits on box 8's try 0
    a, b = G["later"], G["later"] + 1
    assert tk[a] > 0 and tr[a, 0, 7] == 1.0 and without(b)["tried"][0, a] == 0
    # overlapping gts: the rows inside both belong to the smaller number
    box_of = br.points_in_boxes(c["rows"], c["gt_boxes"], c["pose"], c["keep"], c["offsets"])["box_of"]
    sp = c["special"]
    inside = br.frame_matrices(c["rows"][[sp["strip"], sp["in_both_walled"]], :3].astype(np.float64), c["gt_boxes"][0], c["pose"][0])[3]
    assert inside[0, [G["twins"], G["twins"] + 1]].all() and box_of[sp["strip"]] == G["twins"] and st[G["twins"]] == 1
    assert inside[1, [G["walled"], G["walled"] + 1]].all() and box_of[sp["in_both_walled"]] == G["walled"] and box_of[sp["in_wall_only"]] == G["walled"] + 1
    # rows on the faces of box 12
    assert [int(box_of[sp[n]]) for n in ("top_in", "top_out", "x_in", "x_out")] == [G["face"], -1, G["face"], -1] and st[G["face"]] == 1
    # at least one row of every moved box changes its bytes beyond what the world part does to it
    world_only = sr.expected_of(c, cfg=dict(c["cfg"], local=None))
    for i in np.flatnonzero(e["state"][0] == 1):
        mine = np.flatnonzero(box_of == i)
        assert len(mine) and (e["rows"][mine] != world_only["rows"][mine]).any(), i
    blocked = np.flatnonzero(box_of == G["walled"])
    assert len(blocked) and e["rows"][blocked].tobytes() == world_only["rows"][blocked].tobytes()
    # absent rows, NaN or inside a moved box, and the unusable row keep their bytes; everything else moved
    gone = ~c["keep"]
    assert np.isnan(c["rows"][gone]).any() and e["rows"][gone].tobytes() == c["rows"][gone].tobytes() and len(sp["absent_inside"]) > 0
    assert e["rows"][sp["unusable"]].tobytes() == c["rows"][sp["unusable"]].tobytes() and c["keep"][sp["unusable"]]
    usable = br.usable_rows(c["rows"], c["keep"])
    assert (e["rows"][usable, :3] != c["rows"][usable, :3]).any(axis=1).sum() >= usable.sum() - 1       # (the row at the origin may stay)
    assert e["rows"][:, 3:].tobytes() == c["rows"][:, 3:].tobytes() and e["keep"].tobytes() == c["keep"].tobytes()


@pytest.mark.parametrize("dtype", sr.DTYPES)
def test_shapes_states_tries_and_flips_of_the_shared_cases(dtype):
    shapes = {n: (sr.case(n, dtype)["gt_boxes"].shape, sr.tries_of(sr.case(n, dtype)["cfg"])) for n in sr.CASE_NAMES}
    assert {1, 3, 65, 256} <= {s[0][1] for s in shapes.values()} and {1, 4, 16} <= {s[1] for s in shapes.values()}
    assert {7, 10} <= {s[0][2] for s in shapes.values()} and max(s[0][0] for s in shapes.values()) <= 6
    assert tuple(np.diff(sr.case("lengths", dtype)["offsets"])) == sr.LENGTHS == (0, 1, 63, 64, 65, 513)
    flips, tried4 = set(), set()
    for n in sr.CASE_NAMES:
        e = sr.expected(n, dtype)
        flips |= set(map(tuple, e["world"][:, :2].tolist()))
        if shapes[n][1] == 4:
            tried4 |= set(e["tried"].ravel().tolist())
    assert flips == {(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)}    # every flip pair
    assert {-1, 0, 2, 3} <= tried4                                       # no try, the first, the third and the last of T = 4
    assert len(set(map(tuple, sr.expected("flips", dtype)["world"][:, :2].tolist()))) >= 3
    for n in ("b65", "b256"):
        assert set(sr.expected(n, dtype)["state"].ravel().tolist()) == {0, 1, 2}, n
    assert sr.case("world", dtype)["keep"] is None and not sr.expected("world", dtype)["state"].any()
    # a part that is off has the identity's values
    for n, cols in (("no_rotation", (2, 3, 4)), ("no_scaling", (5,)), ("no_world", (0, 1, 2, 3, 4, 5))):
        assert sr.expected(n, dtype)["world"][0, list(cols)].tolist() == [[0.0, 0.0, 1.0, 0.0, 0.0, 1.0][j] for j in cols], n
    assert sr.expected("flip_x", dtype)["world"][0, :2].tolist() == [1.0, 0.0] and sr.expected("flip_y", dtype)["world"][0, :2].tolist() == [0.0, 1.0]
    for n, cols in (("no_local_translation", (0, 1, 2)), ("no_local_rotation", (3, 4, 5)), ("no_local_scaling", (6,)), ("no_local_part_on", tuple(range(7)))):
        e = sr.expected(n, dtype)
        assert (e["tries"][0][..., list(cols)] == np.array(sr.IDENTITY)[list(cols)]).all() and (e["state"][0] == 1).any(), n
    assert not sr.expected("no_local", dtype)["state"].any() and sr.expected("no_local", dtype)["tries"].shape[2] == 0


def test_step_seed_and_frame_change_the_draws():
    c = sr.case("lengths", "float32")
    base = sr.expected("lengths", "float32")
    for changed in (dict(step=c["step"] + 1), dict(seed=c["seed"] + 1), dict(frames=(1, 0, 2, 3, 4, 5))):
        e = sr.expected_of(c, **changed)
        assert not np.array_equal(e["world"], base["world"]) and not np.array_equal(e["tries"], base["tries"]), changed
    assert np.array_equal(sr.expected_of(c)["rows"], base["rows"], equal_nan=True)


# ---- csrc/sg_scene.h on the host --------------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra, "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / "scene_sweep.cpp"), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("scene_sweep"), "scene_sweep")


def _on(v, n):
    return [0] + [0.0] * n if v is None else [1] + [repr(float(x)) for x in v]


def _harness(exe, tmp, c):
    """Every output of the harness on case c, fed NumPy's cos / sin of the restated angles and the restatement's box_of."""
    gt, cfg = c["gt_boxes"], c["cfg"]
    F, B, Cb = gt.shape
    N, T, dt = len(c["rows"]), sr.tries_of(cfg), gt.dtype
    keep = np.ones(N, bool) if c["keep"] is None else c["keep"]
    box_of = br.points_in_boxes(c["rows"], gt, c["pose"], c["keep"], c["offsets"])["box_of"]
    theta, delta = sr.angles(gt, c["pose"], cfg, c["seed"], c["step"])
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    with open(fin, "wb") as fp:
        for a in (c["offsets"], c["rows"], keep.astype(np.uint8), box_of.astype(np.int32), gt, c["pose"], sr._cs(theta), sr._cs(delta)):
            fp.write(np.ascontiguousarray(a).tobytes())
    loc = cfg["local"] or dict(translation=None, rotation=None, scaling=None)
    args = [0 if dt == np.float32 else 1, F, N, B, Cb, T, c["seed"], c["step"], fin, fout, sum({"x": 1, "y": 2}[a] for a in cfg["flip"]),
            *_on(cfg["rotation"], 2), *_on(cfg["scaling"], 2), *_on(loc["translation"], 3), *_on(loc["rotation"], 2), *_on(loc["scaling"], 2)]
    r = subprocess.run([str(exe), *(str(a) for a in args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw, out, at = fout.read_bytes(), {}, 0
    for name, kind, shape in (("rows", dt, (N, 5)), ("keep", np.bool_, (N,)), ("gt_boxes", dt, (F, B, Cb)), ("world", np.float64, (F, 8)), ("state", np.int32, (F, B)),
                              ("tried", np.int32, (F, B)), ("local", np.float64, (F, B, 8)), ("pose", np.float64, (F, B, 2)), ("tries", np.float64, (F, B, T, 8))):
        size = int(np.prod(shape)) * np.dtype(kind).itemsize
        out[name] = np.frombuffer(raw[at:at + size], kind).reshape(shape)
        at += size
    assert at == len(raw)
    return out


def _held_to_the_restatement(exe, tmp, name, dtype):
    got, e = _harness(exe, tmp, sr.case(name, dtype)), sr.expected(name, dtype)
    for f in sr.FIELDS:
        assert got[f].dtype == e[f].dtype and got[f].tobytes() == e[f].tobytes(), (name, dtype, f)


@pytest.mark.parametrize("dtype", sr.DTYPES)
@pytest.mark.parametrize("name", ALL_CASES)
def test_the_header_on_the_host_equals_the_restatement(sweep, tmp_path, name, dtype):
    _held_to_the_restatement(sweep, tmp_path, name, dtype)


def test_the_header_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UBSan -- host code only, a stand-alone program: the records, the tries and the sweep stay
    inside their arrays at B = 256, at T = 16 and on the constructed frame."""
    exe = _compile(tmp_path, "scene_sweep_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name, dtype in (("b256", "float64"), ("b65", "float32"), ("constructed", "float32"), ("lengths", "float32"), ("world", "float64")):
        _held_to_the_restatement(exe, tmp_path, name, dtype)


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_transform_scene_device"
APART = "; the mask, the rows, the boxes, the pose, box_of and the step are read while the scene is written: pass a buffer apart from them"
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "boxes": WHO + ": n_boxes must lie in 1 .. 256",
    "box_features": WHO + ": box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first",
    "flip": WHO + ": flip must lie in 0 .. 3: bit 0 the x axis, bit 1 the y axis",
    "tries": WHO + ": tries must lie in 0 .. 16",
    "range": WHO + ": a range must be finite with lo <= hi",
    "scaling": WHO + ": a scaling range must be above 0",
    "translation": WHO + ": every component of the local translation must be finite and lie in 0 .. 100",
    "elements": WHO + ": n_frames * n_boxes * max(tries, 1) * 10 exceeds 2^31 - 1; split the batch",
    "rows": "batch too large: split it below 2^31 rows",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "step": WHO + ": d_step is NULL; one uint64 in device memory",
}
ORDER = tuple(MESSAGES)              # the order of the checks: a call wrong in two ways gets the earlier message
DOUBLY = ("null_gt_boxes_and_boxes_0", "boxes_0_and_box_features_6", "box_features_6_and_flip_4", "flip_4_and_tries_17", "tries_17_and_rotation_nan",
          "rotation_nan_and_scaling_0", "scaling_0_and_translation_nan", "translation_nan_and_elements_at_2p31", "elements_at_2p31_and_rows_at_2p31",
          "rows_at_2p31_and_frame_above_2p30", "frame_above_2p30_and_null_step", "null_step_and_out_rows_overlaps_rows")
PAIRS = {("rows", "rows"): ("out_rows_overlaps_rows",), ("keep", "keep_in"): ("out_keep_is_keep_in",), ("gt_boxes", "gt_boxes"): ("out_gt_boxes_is_gt_boxes",),
         ("world", "frame_offsets"): ("world_overlaps_frame_off",), ("state", "box_of"): ("state_is_box_of",), ("tried", "step"): ("tried_is_step",),
         ("local", "pose_in"): ("local_is_pose_in",), ("pose", "pose_in"): ("pose_is_pose_in",), ("tries", "gt_boxes"): ("tries_is_gt_boxes",)}
OUTS = {("keep", "rows"): ("out_keep_is_out_rows", "in_place_and_keep_in_the_rows"), ("tried", "state"): ("tried_is_state",), ("local", "world"): ("local_is_world",),
        ("pose", "gt_boxes"): ("pose_is_out_gt_boxes",), ("tries", "local"): ("tries_is_local",)}
ACCEPTED = ("clean", "null_pose_in", "null_keep_in", "null_box_of", "null_out_pose", "null_out_tries", "every_part_off", "no_rows_needs_no_row_buffers", "float64",
            "boxes_1", "boxes_256", "box_features_7", "box_features_10", "flip_0", "tries_0", "tries_16", "rotation_lo_is_hi", "local_ranges_are_not_read_without_tries",
            "translation_100", "elements_below_2p31", "frame_of_2p30", "in_place", "out_rows_behind_rows", "out_keep_behind_keep_in", "state_behind_box_of",
            "box_of_is_not_read_without_tries", "out_keep_behind_out_rows")
REFUSED = {
    "null": ("null_frame_off", "null_rows", "null_gt_boxes", "null_out_rows", "null_out_keep", "null_out_gt_boxes", "null_out_world", "null_out_state", "null_out_tried",
             "null_out_local", "bad_dtype", "no_frames", "rows_negative", "null_gt_boxes_and_boxes_0"),
    "boxes": ("boxes_0", "boxes_257", "boxes_0_and_box_features_6"),
    "box_features": ("box_features_6", "box_features_11", "box_features_6_and_flip_4"),
    "flip": ("flip_negative", "flip_4", "flip_4_and_tries_17"),
    "tries": ("tries_negative", "tries_17", "tries_17_and_rotation_nan"),
    "range": ("rotation_nan", "rotation_inf", "rotation_lo_above_hi", "scaling_lo_above_hi", "local_rotation_nan", "local_scaling_lo_above_hi", "rotation_nan_and_scaling_0"),
    "scaling": ("scaling_0", "scaling_negative", "local_scaling_0", "scaling_0_and_translation_nan"),
    "translation": ("translation_negative", "translation_above_100", "translation_nan", "translation_nan_and_elements_at_2p31"),
    "elements": ("elements_at_2p31", "elements_at_2p31_and_rows_at_2p31"),
    "rows": ("rows_at_2p31", "rows_at_2p31_and_frame_above_2p30"),
    "frame": ("frame_above_2p30", "frame_above_2p30_and_null_step"),
    "step": ("null_step", "null_step_and_out_rows_overlaps_rows"),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "scene_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "scene_refusals.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split("|", 1) for ln in r.stdout.splitlines())
    want = {case: "0|OK" for case in ACCEPTED}
    for key, cases in REFUSED.items():
        want.update({case: "1|" + MESSAGES[key] for case in cases})
    for (out, inp), cases in PAIRS.items():
        want.update({case: f"1|{WHO}: d_out_{out} overlaps d_{inp}{APART}" for case in cases})
    for (out, other), cases in OUTS.items():
        want.update({case: f"1|{WHO}: d_out_{out} overlaps d_out_{other}{OWN}" for case in cases})
    assert got == want
    assert set(MESSAGES) == set(REFUSED)              # every message is reached
    # the order: the checks stand in sg_check_scene_args in the order of MESSAGES, the overlaps behind them -- every "<first>_and_<second>"
    # case of the harness is wrong in two ways, of checks next to each other, and is filed above under the earlier one
    for key, later, case in zip(ORDER, ORDER[1:] + (None,), DOUBLY):
        first, second = case.split("_and_")
        assert first in REFUSED[key] and case in REFUSED[key], case
        assert second in REFUSED[later] if later else any(second in cases for cases in PAIRS.values()), case


def test_the_entry_is_declared_and_bound():
    from lidar_snow_sim_amd import _native
    header = (ROOT / "include" / "snowgpu.h").read_text()
    assert "int snowgpu_transform_scene_device(" in header and "snowgpu_transform_scene_device" in _native.EXPORTS
    text = " ".join(header.split("SCENE TRANSFORMS")[1].split("*/")[0].replace("*", " ").split())
    assert "NOT CHECKED against" in text and "VELOCITY COLUMNS ARE OUT OF SCOPE" in text and "BEHIND the weather stages" in text
    assert hasattr(_native.lib(), "snowgpu_transform_scene_device") and hasattr(_native.Context, "transform_scene_device")
    assert "snowgpu_scene.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import scene, stages, tensors
    assert tensors.transform_scene is stages.transform_scene and tensors.SceneBatch is stages.SceneBatch and tensors.SCENE_STATES == dict(still=0, moved=1, blocked=2)
    assert callable(scene.transform_scene) and tuple(scene.FIELDS) == tuple(sr.FIELDS)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        assert "transform_scene" in text and "behind the weather" in text.lower(), doc
