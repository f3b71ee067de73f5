"""-m gpu: scene transforms on the device (tensors.transform_scene, tensors.SceneBatch, scene.transform_scene,
snowgpu_transform_scene_device; csrc/snowgpu_scene.hip, csrc/sg_scene.h) against the restatement of their definition
(tests/scene_reference.py, whose cases tests/test_scene_reference.py holds to the conditions that keep these comparisons from being
vacuous).  The restatement takes every cos / sin as an input: it is fed the gts' pose and the cos / sin the call returned (`world`,
`tries`); the draws are Philox words in Python integers and everything else is separately rounded float64 arithmetic in the definition's
order: every output is compared byte for byte, for both dtypes, with no element left out.  The returned cos / sin themselves are held
to the bound of tests/test_gpu_boxes.py's pose test."""
import numpy as np
import pytest
import torch

import box_reference as br
import scene_reference as sr
from lidar_snow_sim_amd.tensors import transform_scene  # noqa: F401  (the stage under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

DTYPES = sr.DTYPES
FIELDS = sr.FIELDS
ALL_CASES = sr.CASE_NAMES + tuple(sr.OFF)
EPS = 2.0 ** -53                                                      # the unit roundoff of float64


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _step(v):
    return torch.tensor([int(v)], dtype=torch.int64, device="cuda")


def _fields(c):
    return FIELDS if sr.tries_of(c["cfg"]) else FIELDS[:-1]


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy() if not isinstance(got, dict) else got[name]
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


def _call_args(c, pose="given"):
    cfg = c["cfg"]
    return dict(step=_step(c["step"]), seed=c["seed"], flip=cfg["flip"], rotation=cfg["rotation"], scaling=cfg["scaling"], local=cfg["local"],
                keep=None if c["keep"] is None else _t(c["keep"]), pose=_t(c["pose"]) if pose == "given" else None, return_pose=True,
                return_tried=sr.tries_of(cfg) > 0)


def _run(c, pose="given", frames=None, **kw):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    args = _call_args(c, pose)
    args.update(kw)
    return transform_scene(DeviceBatch(_t(c["rows"]), c["offsets"]) if frames is None else frames, _t(c["gt_boxes"]), **args)


def _want(c, got, **changed):
    """The restatement on c, fed the cos / sin that the call returned."""
    world = got.world.cpu().numpy() if not isinstance(got, dict) else got["world"]
    tries = None if not sr.tries_of(c["cfg"]) else (got.tries.cpu().numpy() if not isinstance(got, dict) else got["tries"])
    return sr.expected_of(c, world_cs=world[:, 2:4], tries_cs=None if tries is None else tries[..., 3:5], **changed)


# ---- 1. the shared cases and every part switched off ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ALL_CASES)
def test_cases_equal_the_restatement(name, dtype):
    """B in 1, 3, 5, 15, 65, 256; T in 0, 1, 2, 4, 16; Cb in 7 .. 10; frames of 0, 1, 63, 64, 65 and 513 rows in one batch; the constructed
    frame with each part switched off, each flip alone and no local part; keep=None and the world part alone ("world")."""
    c = sr.case(name, dtype)
    got = _run(c)
    _same(got, _want(c, got), (name, dtype), _fields(c))
    assert torch.equal(got.moved, got.state == 1) and (got.tries is None) == (sr.tries_of(c["cfg"]) == 0)


def test_returned_cos_and_sin():
    """cos / sin of theta and of every delta, as returned, against the correctly rounded values of the RESTATED angle: within 4 ulp of glibc's
    cosl / sinl on the 80-bit format, 4 + 1 ulp where NumPy's float64 is the reference -- the bound and method of test_gpu_boxes.py's pose
    test.  Exactly (1, 0) where the part is off and for absent boxes.  Seen on one MI355X: 0.574 ulp at most over 4 232 values."""
    extended = np.finfo(np.longdouble).nmant >= 63
    worst, n = 0.0, 0
    for name in ("constructed", "b65", "b256", "flips", "lengths"):
        c = sr.case(name, "float64")
        got = _run(c)
        theta, delta = sr.angles(c["gt_boxes"], c["pose"], c["cfg"], c["seed"], c["step"])
        world = got.world.cpu().numpy()
        assert world[:, 4].tobytes() == theta.tobytes()
        pairs = [(theta, world[:, 2:4])]
        if got.tries is not None:
            tries = got.tries.cpu().numpy()
            assert tries[..., 5].tobytes() == delta.tobytes()
            ok = br.present(c["gt_boxes"], c["pose"])
            assert (tries[~ok][..., 3:5] == (1.0, 0.0)).all()
            pairs.append((delta[ok].ravel(), tries[ok][..., 3:5].reshape(-1, 2)))
        for angle, cs in pairs:
            al = angle.astype(np.longdouble)
            true = np.stack((np.cos(al), np.sin(al)), axis=-1)
            ulp = np.spacing(np.abs(true.astype(np.float64))).astype(np.longdouble)
            err = np.abs(cs.astype(np.longdouble) - true) / ulp
            worst, n = max(worst, float(err.max())), n + err.size
    print("scene cos / sin: largest error %.3f ulp over %d values" % (worst, n))
    assert n > 2000 and worst <= (4.0 if extended else 5.0)
    for name in ("no_rotation", "no_local_rotation", "no_world"):
        got = _run(sr.case(name, "float64"))
        if name != "no_local_rotation":
            assert got.world.cpu().numpy()[:, 2:5].tolist() == [[1.0, 0.0, 0.0]]
        if name == "no_local_rotation":
            assert (got.tries.cpu().numpy()[..., 3:6] == (1.0, 0.0, 0.0)).all()


# ---- 2. the same bytes by other routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_box_of_in_place_pose_and_aligned_input(dtype):
    from lidar_snow_sim_amd.tensors import AlignedResult, DeviceBatch, points_in_boxes
    c = sr.case("constructed", dtype)
    base = _run(c)
    fields = _fields(c)

    def same_as_base(other, what):
        for f in fields:
            assert torch.equal(getattr(other, f).view(torch.uint8), getattr(base, f).view(torch.uint8)), (what, f)

    same_as_base(_run(c), "two calls")
    # a caller's box_of, from points_in_boxes on the ORIGINAL boxes
    labels = points_in_boxes(DeviceBatch(_t(c["rows"]), c["offsets"]), _t(c["gt_boxes"]), pose=_t(c["pose"]), keep=_t(c["keep"]))
    assert (labels.box_of >= 0).any()
    same_as_base(_run(c, box_of=labels.box_of), "box_of=")
    # in place: the input rows are the output rows
    rows = _t(c["rows"])
    inp = _run(c, frames=DeviceBatch(rows, c["offsets"]), in_place=True)
    assert inp.rows.data_ptr() == rows.data_ptr()
    same_as_base(inp, "in_place")
    # an aligned result as input; its keep is ANDed with keep=
    res = AlignedResult(None, _t(c["rows"]), _t(c["keep"]), None, None, None, c["offsets"], None)
    same_as_base(_run(c, frames=res, keep=None), "AlignedResult")
    half = c["keep"] & (np.arange(len(c["keep"])) % 2 == 0)
    anded = _run(c, frames=res, keep=_t(np.arange(len(c["keep"])) % 2 == 0))
    _same(anded, _want(dict(c, keep=half), anded), "AlignedResult and keep=", fields)
    # the device's own pose: what it used comes back composed in `pose`; NumPy's and the device's cos / sin of the heading agree to 1e-15
    own = _run(c, pose=None)
    ok = br.present(c["gt_boxes"], c["pose"])
    used = points_in_boxes(DeviceBatch(_t(c["rows"]), c["offsets"]), _t(c["gt_boxes"]), return_pose=True).pose.cpu().numpy()
    assert np.allclose(used[ok], c["pose"][ok], rtol=0, atol=1e-15) and not used[~ok].any()
    d = dict(c, pose=np.where(ok[..., None], used, c["pose"]))
    _same(own, _want(d, own), "pose=None", fields)


# ---- 3. the ways back -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_invert_points_and_apply_boxes(dtype):
    """invert_points(rows of the world-only call) against the input, apply_boxes(gt) against the world-only gt_boxes, invert_boxes against gt.
    THE BOUND, derived: u = the unit roundoff of the rows' dtype, e = 2^-53, r = |x| + |y| of the input row.  Forward: x c - y s has two
    rounded products and a rounded sum, at most 3 e r off; times sigma, one more rounding; the store rounds to the dtype: the stored value
    is within sigma r (u + 4 e) of sigma (x c - y s).  Inverse, float64 in torch: the division by sigma adds one rounding, so each of px, py
    is within r (u + 5 e) of the exact rotated coordinate; px c + py s carries these two errors times |c| + |s| <= 1.5 and three roundings
    of its own on terms of size <= 2 r: 6 e r; in exact arithmetic it equals x (c c + s s), and the device's (c, s) is within 4 ulp <= 8 e
    of (cos, sin) per component (test_returned_cos_and_sin), so |c c + s s - 1| <= 2 x 8 e x 1.5 < 32 e.  Sum: r (1.5 u + 7.5 e + 6 e + 32 e)
    <= r (1.5 u + 48 e) with the second-order terms.  z: two roundings and the store, |z| (u + 3 e) -- inside the same expression with
    r = |z|.  A box centre is a point; a dimension and the heading see a product or two sums and the store: the same expression with r the
    value's size (for the heading |h| + pi + |theta|) holds them too.  Seen on one MI355X: the largest error was 0.65 of the bound in
    float32 and 0.04 of it in float64."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    c = sr.case("world", dtype)
    u = float(np.finfo(dtype).eps) / 2
    sb = _run(c)
    rows, gt = c["rows"], c["gt_boxes"]
    usable = br.usable_rows(rows)
    back = sb.invert_points(sb.rows.double()).cpu().numpy()
    assert back.dtype == np.float64 and back[usable, 3:].tobytes() == rows[usable, 3:].astype(np.float64).tobytes()
    x = rows[usable, :3].astype(np.float64)
    r = np.abs(x[:, :2]).sum(axis=1)
    bound = np.column_stack((r, r, np.abs(x[:, 2]))) * (1.5 * u + 48 * EPS)
    err = np.abs(back[usable, :3] - x)
    print("invert_points: largest error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert usable.sum() > 300 and (err <= bound).all() and (err > 0).any()
    assert (sb.world[:, :2].cpu().numpy() != 0).any() and not np.array_equal(sb.rows.cpu().numpy()[usable, :3], rows[usable, :3])
    # the boxes, forward and back
    ok = br.present(gt, c["pose"])
    g = gt[ok][:, :7].astype(np.float64)
    theta = np.abs(sb.world.cpu().numpy()[:, 4])[:, None].repeat(gt.shape[1], 1)[ok]
    rc = np.abs(g[:, :2]).sum(axis=1)
    size = np.column_stack((rc, rc, np.abs(g[:, 2]), g[:, 3], g[:, 4], g[:, 5], np.abs(g[:, 6]) + np.pi + theta))
    sigma = sb.world.cpu().numpy()[:, 5][:, None].repeat(gt.shape[1], 1)[ok][:, None]
    fwd = sb.apply_boxes(_t(gt).double()).cpu().numpy()
    out = sb.gt_boxes.cpu().numpy().astype(np.float64)
    assert (np.abs(fwd[ok][:, :7] - out[ok][:, :7]) <= size * np.maximum(sigma, 1.0) * (1.5 * u + 48 * EPS)).all() and fwd[..., 7:].tobytes() == out[..., 7:].tobytes()
    inv = sb.invert_boxes(sb.gt_boxes.double()).cpu().numpy()
    assert (np.abs(inv[ok][:, :7] - g) <= size * (1.5 * u + 48 * EPS)).all() and inv[..., 7:].tobytes() == out[..., 7:].tobytes()
    # gradients pass
    p = sb.rows.double().clone().requires_grad_(True)
    sb.invert_points(p)[:, :3].sum().backward()
    assert p.grad is not None and bool((p.grad[:, :3] != 0).any())
    with pytest.raises(ValueError, match="one point per row"):
        sb.invert_points(sb.rows[:-1])


# ---- 4. out=, the counter, one graph ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_is_fully_written_and_calls_repeat(dtype):
    from lidar_snow_sim_amd.tensors import SceneBatch
    c = sr.case("lengths", dtype)
    B, Cb, T = c["gt_boxes"].shape[1], c["gt_boxes"].shape[2], sr.tries_of(c["cfg"])
    out = SceneBatch.empty(c["offsets"], B, Cb, T, getattr(torch, dtype), with_pose=True, with_tries=True)
    snaps = []
    for _ in range(2):
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0xFF)
        got = _run(c, out=out)
        assert got is out
        snaps.append([getattr(out, f).clone() for f in FIELDS])
        _same(out, _want(c, out), ("out=", dtype))
    for a, b in zip(*snaps):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    bare = _run(c, return_pose=False, return_tried=False)
    assert bare.pose is None and bare.tries is None
    _same(bare, _want(c, out), "bare", FIELDS[:7])


def test_step_seed_and_position_change_the_draws():
    c = sr.case("lengths", "float32")
    base = _run(c)
    for changed in (dict(step=c["step"] + 1), dict(step=c["step"] + (1 << 32)), dict(seed=c["seed"] + 1), dict(seed=c["seed"] + (1 << 32))):
        d = dict(c, **changed)
        got = _run(d)
        _same(got, _want(d, got), changed)
        assert not torch.equal(got.world, base.world) and not torch.equal(got.tries, base.tries)
    # the last frame alone is frame 0 of its call: another draw than at position 5
    a, b = int(c["offsets"][5]), int(c["offsets"][6])
    one = dict(c, rows=c["rows"][a:b], keep=c["keep"][a:b], offsets=np.array([0, b - a], np.int64), gt_boxes=c["gt_boxes"][5:], pose=c["pose"][5:])
    alone = _run(one)
    _same(alone, _want(one, alone), "one frame")
    assert not torch.equal(alone.world[0], base.world[5])
    keyed = sr.expected_of(one, frames=[5], world_cs=base.world.cpu().numpy()[5:, 2:4], tries_cs=base.tries.cpu().numpy()[5:, ..., 3:5])
    assert keyed["rows"].tobytes() == base.rows.cpu().numpy()[a:b].tobytes()


def test_points_in_boxes_transform_scene_voxelize_and_step_in_one_graph():
    """points_in_boxes -> transform_scene -> voxelize -> step += 1 captured once on a side stream after one warm-up and replayed twice,
    rows, boxes, pose and mask rewritten in place before each replay: every replay equals the restatement on its own data at its own
    step, the voxels are those of an uncaptured call on the replay's rows, and the two draws differ."""
    from lidar_snow_sim_amd.tensors import BoxLabelBatch, DeviceBatch, SceneBatch, VoxelBatch, points_in_boxes, voxelize
    c = sr.case("lengths", "float32")
    cfg, F, (B, Cb), T = c["cfg"], len(c["offsets"]) - 1, c["gt_boxes"].shape[1:], sr.tries_of(c["cfg"])
    mirrored_rows, mirrored_gt = c["rows"].copy(), c["gt_boxes"].copy()
    mirrored_rows[:, :2] = -mirrored_rows[:, :2]
    mirrored_gt[..., :2] = -mirrored_gt[..., :2]
    other = dict(c, rows=mirrored_rows, gt_boxes=mirrored_gt, keep=c["keep"] & (np.arange(len(c["keep"])) % 7 != 0))
    data = (c, other)
    rows, gt, keep, pose = _t(c["rows"]), _t(c["gt_boxes"]), _t(c["keep"]), _t(c["pose"])
    batch = DeviceBatch(rows, c["offsets"])
    labels = BoxLabelBatch.empty(c["offsets"], B, torch.float32)
    out = SceneBatch.empty(c["offsets"], B, Cb, T, torch.float32, with_pose=True, with_tries=True)
    rng6, size3, P, V = (-64.0, -64.0, -4.0, 64.0, 64.0, 4.0), (0.5, 0.5, 1.0), 4, 128
    vox = VoxelBatch.empty(F, P, V, 4, torch.float32, n_rows=len(c["rows"]))
    s0 = c["step"]
    step = _step(s0 - 1)

    def call():
        points_in_boxes(batch, gt, pose=pose, keep=keep, out=labels)
        transform_scene(batch, gt, step=step, seed=c["seed"], flip=cfg["flip"], rotation=cfg["rotation"], scaling=cfg["scaling"], local=cfg["local"], box_of=labels.box_of,
                        pose=pose, keep=keep, out=out, return_pose=True, return_tried=True)
        voxelize(DeviceBatch(out.rows, c["offsets"]), rng6, size3, P, V, keep=out.keep, out=vox)
        step.add_(1)

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()                                                            # warm-up: the captured call allocates nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        got = []
        for k in range(2):                                                # no host read between the replays
            d = data[k]
            rows.copy_(_t(d["rows"])), gt.copy_(_t(d["gt_boxes"])), keep.copy_(_t(d["keep"])), pose.copy_(_t(d["pose"]))
            g.replay()
            got.append(({n: getattr(out, n).clone() for n in FIELDS}, vox.voxels.clone(), vox.num_points.clone(), vox.coords.clone()))
        s.synchronize()
    assert int(step[0]) == s0 + 2
    for k in range(2):
        scene = {n: v.cpu().numpy() for n, v in got[k][0].items()}
        _same(scene, _want(data[k], scene, step=s0 + k), ("replay", k))
        direct = voxelize(DeviceBatch(got[k][0]["rows"], c["offsets"]), rng6, size3, P, V, keep=got[k][0]["keep"])
        assert torch.equal(direct.num_points, got[k][2]) and torch.equal(direct.coords, got[k][3]) and int(direct.num_points.sum()) > 0
        assert torch.equal(direct.voxels.view(torch.int32), got[k][1].view(torch.int32))
    assert not torch.equal(got[0][0]["world"], got[1][0]["world"]) and not torch.equal(got[0][0]["tries"], got[1][0]["tries"])


# ---- 5. the NumPy mirror ------------------------------------------------------------------------------------------------------------------------
def test_the_host_array_mirror():
    from lidar_snow_sim_amd import scene
    c = sr.case("constructed", "float64")
    cfg = c["cfg"]
    got = scene.transform_scene(c["rows"], c["gt_boxes"][0], c["keep"], seed=c["seed"], step=c["step"], flip=cfg["flip"], rotation=cfg["rotation"], scaling=cfg["scaling"],
                                local=cfg["local"])
    e = sr.expected_of(c, world_cs=got["world"][None, 2:4], tries_cs=got["tries"][None, ..., 3:5])
    for name in FIELDS:
        want = e[name][0] if name in ("gt_boxes", "world", "state", "tried", "local", "pose", "tries") else e[name]
        assert got[name].tobytes() == want.tobytes(), name
    world_only = scene.transform_scene(c["rows"].astype(np.float32), c["gt_boxes"][0].astype(np.float32))
    assert "tries" not in world_only and world_only["rows"].dtype == np.float32 and not world_only["state"].any()


# ---- 6. what Python refuses ---------------------------------------------------------------------------------------------------------------------
def test_python_refusals_in_the_stages_order():
    from lidar_snow_sim_amd.tensors import DeviceBatch, SceneBatch
    c = sr.case("b1", "float32")
    rows, gt, keep = _t(c["rows"]), _t(c["gt_boxes"]), _t(c["keep"])
    batch, step = DeviceBatch(rows, c["offsets"]), _step(0)

    def refused(words, *args, **kw):
        kw.setdefault("step", step)
        with pytest.raises(ValueError, match=words):
            transform_scene(*args, **kw)

    refused("torch CUDA tensors or an aligned result", c["rows"], gt)
    refused("flip holds any of 'x' and 'y'", batch, gt, flip=("z",))
    refused("rotation holds 2 numbers", batch, gt, rotation=(1.0,))
    refused("local is None or a dict", batch, gt, local=dict(jitter=1))
    refused(r"local\['tries'\] must be an integer", batch, gt, local=dict(tries=1.5))
    refused(r"local\['tries'\] must lie in 1 .. 16", batch, gt, local=dict(tries=17))
    refused(r"local\['translation'\] holds 3 numbers", batch, gt, local=dict(translation=(1.0, 1.0)))
    refused("keep must have one element per row", batch, gt, keep=keep[:-1])
    refused("gt_boxes must be a contiguous", batch, gt.double())
    refused("step must be a one-element int64", batch, gt, step=torch.zeros(1, dtype=torch.int32, device="cuda"))
    refused("n_boxes must lie in 1 .. 256", batch, _t(np.zeros((2, 257, 8), np.float32)))
    refused("box_features must lie in 7 .. 10", batch, _t(np.zeros((2, 1, 6), np.float32)))
    refused("pose must be a contiguous", batch, gt, pose=torch.zeros((2, 2, 2), device="cuda"))
    refused("box_of must be a contiguous", batch, gt, local=dict(tries=2), box_of=torch.zeros(3, dtype=torch.int32, device="cuda"))
    refused("return_tried needs a local part", batch, gt, return_tried=True)
    refused("out must be a SceneBatch whose rows", batch, gt, out=SceneBatch.empty(c["offsets"][:2], 1))
    refused("with in_place, out.rows must be the input rows", batch, gt, in_place=True, out=SceneBatch.empty(c["offsets"], 1))
    # wrong in two ways: the earlier check speaks
    refused("flip holds any of", batch, gt.double(), flip=("z",))
    refused("gt_boxes must be a contiguous", batch, gt.double(), pose=torch.zeros((2, 2, 2), device="cuda"))
    # what only the entry refuses comes back in the entry's words
    refused("snowgpu_transform_scene_device: a range must be finite with lo <= hi", batch, gt, rotation=(1.0, 0.5))
    refused("snowgpu_transform_scene_device: a scaling range must be above 0", batch, gt, scaling=(0.0, 1.0))
    refused("the local translation must be finite and lie in 0 .. 100", batch, gt, local=dict(translation=(1.0, -1.0, 0.0)))
    out = SceneBatch.empty(c["offsets"], 1)
    out.tried = out.state
    refused("d_out_tried overlaps d_out_state; every output needs memory of its own", batch, gt, out=out)
    out = SceneBatch.empty(c["offsets"], 1)
    out.gt_boxes = gt
    refused("snowgpu_transform_scene_device: d_out_gt_boxes overlaps d_gt_boxes", batch, gt, out=out)
