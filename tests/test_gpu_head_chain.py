"""-m gpu: the second stage and the anchor targets of INTEGRATION.md as ONE chain of device stages -- nms of the proposals, sectorized
sample_keypoints around the kept boxes, ball_query around the keypoints, boxes_iou of the kept boxes with the gts, sample_rois,
roi_point_pool and roi_voxel_pool of the sampled rois, points_in_boxes of the gts, keep_boxes and assign_anchors against the gts that are
left, and the ways back of every result class (rt.gather, rt.valid, rp.gather, rp.labels, rp.empty_flag, rv.nonempty, rv.max_features,
rv.avg_features, rv.as_grid, at.matched, at.reg_weights, at.cls_weights, at.positive) -- queued without a host read, on a side stream, on
torch's legacy default stream, in any order of the independent groups, after batches of other sizes and dtypes have left their records,
run tables and offsets in the context's scratch, on two contexts at once, and captured with `step += 1` into one HIP graph.

Every comparison is byte for byte against tests/head_reference.py: the composition of the single stages' restatements under the poses the
device library gives for the proposals and the gts (points_in_boxes(..., return_pose=True), as tests/test_gpu_iou.py takes them).  The
aligned result is built from rows and a keep mask: the snowfall call in front of it is pinned by tests/test_gpu_chain.py.
tests/test_head_reference.py holds the inputs to the conditions that keep this from being vacuous; the first test asserts them once more on
what the device gave."""
import numpy as np
import pytest
import torch

import head_reference as hr

pytestmark = pytest.mark.gpu

GROUPS = ("keypoints", "rois", "anchors")            # independent of each other behind nms
POOLS = ("rp", "rv")                                 # independent of each other behind sample_rois
STEPS = 10                                           # the steps _steps() yields
INPUTS = ("rows", "keep", "proposals", "scores", "gt_boxes")          # what a replay rewrites in place


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


_POSES = {}


def device_poses(name, dtype):
    """The (cos, sin) the device library gives for the proposals and the gts of a batch, (0, 0) for an absent box: points_in_boxes returns
    the pose it used; the boxes go through it 256 at a time, one row per frame.  Once per batch."""
    from lidar_snow_sim_amd.tensors import DeviceBatch, points_in_boxes
    if (name, dtype) not in _POSES:
        got = []
        for boxes in (hr.batch(name, dtype)["proposals"], hr.batch(name, dtype)["gt_boxes"]):
            flat = boxes.reshape(-1, boxes.shape[-1])
            G = (len(flat) + 255) // 256
            padded = np.zeros((G * 256, flat.shape[1]), flat.dtype)
            padded[:len(flat)] = flat
            rows = DeviceBatch(_t(np.zeros((G, 5), flat.dtype)), np.arange(G + 1, dtype=np.int64))
            pose = points_in_boxes(rows, _t(padded.reshape(G, 256, -1)), return_count=False, return_pose=True).pose.cpu().numpy()
            got.append(np.ascontiguousarray(pose.reshape(-1, 2)[:len(flat)].reshape(boxes.shape[:-1] + (2,))))
        b = hr.batch(name, dtype)
        for mine, numpy_s in zip(got, (b["pose_proposals"], b["pose_gt"])):
            assert np.abs(mine - np.where((mine != 0).any(axis=-1, keepdims=True), numpy_s, 0.0)).max() < 1e-15
        _POSES[name, dtype] = tuple(got)
    return _POSES[name, dtype]


def want_of(name, dtype, step=0):
    return hr.expected(name, dtype, step, *device_poses(name, dtype))


class Inputs:
    """Device copies of a batch of tests/head_reference.py, the aligned result over its rows and keep mask, and the step word."""

    def __init__(self, name, dtype, step=0):
        b = self.host = hr.batch(name, dtype)
        self.name, self.dtype, self.offsets, self.shape = name, dtype, b["offsets"].copy(), b["shape"]
        self.F, self.n = len(b["sizes"]), int(b["offsets"][-1])
        self.rows, self.keep, self.proposals, self.scores, self.gt_boxes = (_t(b[k]) for k in INPUTS)
        self.anchors, self.anchor_class, self.feats = _t(b["anchors"]), _t(b["anchor_class"]), _t(b["point_features"])
        self.per_row = self.feats[:, 0].contiguous()
        self.step = torch.tensor([step], dtype=torch.int64, device="cuda")

    def result(self, slot=0):
        """An AlignedResult over the rows and the mask, of the context of `slot`, for torch's current stream."""
        from lidar_snow_sim_amd import engine
        from lidar_snow_sim_amd.tensors import AlignedResult
        eng = engine.get_engine(torch.cuda.current_device(), slot)
        z = torch.zeros(1, dtype=torch.int64, device="cuda")
        return AlignedResult(eng.ctx, self.rows, self.keep, z, z, z, self.offsets, torch.cuda.current_stream())

    def load(self, other):
        """The rows, mask, proposals, scores and gts of another batch of the same shape, copied in place (device to device)."""
        for k in INPUTS:
            getattr(self, k).copy_(getattr(other, k))


class Buffers:
    """out= buffers of every stage for a batch: static addresses for a captured graph."""

    def __init__(self, inp):
        from lidar_snow_sim_amd.tensors import (AnchorTargetBatch, BoxLabelBatch, IouBatch, KeypointBatch, NeighbourBatch, NmsBatch, RoiPointBatch, RoiTargetBatch,
                                                RoiVoxelBatch)
        dt, sh, F = getattr(torch, inp.dtype), inp.shape, inp.F
        self.nb = NmsBatch.empty(F, sh["B"], sh["P"], 8, dt, with_scores=True)
        self.kp = KeypointBatch.empty(F, sh["K"], 4, dt, sectors=hr.SECTORS)
        self.groups = NeighbourBatch.empty(F, sh["K"], hr.SAMPLES, 4, dt, with_points=True)
        self.io = IouBatch.empty(F, sh["P"], sh["G"], dt, with_iou=False, with_best=True)
        self.rt = RoiTargetBatch.empty(F, sh["S"], 8, 8, dt, with_pose=True, with_local=True)
        self.rp = RoiPointBatch.empty(F, sh["S"], hr.NS, 4, dt, with_local=True)
        self.rv = RoiVoxelBatch.empty(F, sh["S"], hr.OUT_SIZE, hr.MAX_POINTS, hr.CF, with_index=True)
        self.lab = BoxLabelBatch.empty(inp.offsets, sh["G"], dt)
        self.at = AnchorTargetBatch.empty(F, sh["A"], sh["G"], dt, with_iou=True)
        self.live = torch.empty_like(inp.gt_boxes)

    def tensors(self):
        return [self.live] + [getattr(getattr(self, name), f) for name, fields in hr.FIELDS.items() for f in fields]


def _steps(res, inp, bufs=None, order=GROUPS, pools=POOLS, slot=0):
    """The calls of the chain as INTEGRATION.md writes them, one stage per step (a generator: two chains can be queued alternately); yields
    the dict of results, which is complete after the last step.  `order` permutes the three groups behind nms, `pools` the two poolings.
    No host read, wait() or synchronize in here."""
    from lidar_snow_sim_amd.tensors import assign_anchors, ball_query, boxes_iou, nms, points_in_boxes, roi_point_pool, roi_voxel_pool, sample_keypoints, sample_rois
    sh = inp.shape
    o = (lambda name: None) if bufs is None else (lambda name: getattr(bufs, name))
    out = {}
    nb = out["nb"] = nms(inp.proposals, inp.scores, hr.IOU_THRESH, post_max=sh["P"], score_thresh=hr.SCORE_THRESH, return_scores=True, out=o("nb"), slot=slot)
    yield out
    for group in order:
        if group == "keypoints":
            kp = out["kp"] = sample_keypoints(res, sh["K"], sectors=hr.SECTORS, rois=nb.boxes, out=o("kp"), slot=slot)
            yield out
            out["groups"] = ball_query(res, kp, hr.RADII, hr.SAMPLES, return_points=True, out=o("groups"), slot=slot)
            yield out
        elif group == "rois":
            io = out["io"] = boxes_iou(nb.boxes, inp.gt_boxes, return_iou=False, return_best=True, out=o("io"), slot=slot)
            yield out
            rt = out["rt"] = sample_rois(nb, inp.gt_boxes, io, step=inp.step, seed=hr.SEED, roi_per_image=sh["S"], return_pose=True, return_local=True, out=o("rt"),
                                         slot=slot)
            yield out
            for pool in pools:
                if pool == "rp":
                    out["rp"] = roi_point_pool(res, rt.rois, hr.NS, extra_width=hr.EXTRA_WIDTH, pose=rt.pose, return_local=True, out=o("rp"), slot=slot)
                elif pool == "rv":
                    out["rv"] = roi_voxel_pool(res, rt.rois, hr.OUT_SIZE, hr.MAX_POINTS, inp.feats, pose=rt.pose, return_index=True, out=o("rv"), slot=slot)
                else:
                    raise ValueError(pool)
                yield out
        elif group == "anchors":
            lab = out["lab"] = points_in_boxes(res, inp.gt_boxes, out=o("lab"), slot=slot)
            kept = out["back.keep_boxes"] = lab.keep_boxes(hr.MIN_POINTS)
            live = inp.gt_boxes * kept[..., None]
            if bufs is not None:
                bufs.live.copy_(live)
                live = bufs.live
            out["back.live"] = live
            yield out
            out["at"] = assign_anchors(inp.anchors, inp.anchor_class, live, return_iou=True, out=o("at"), slot=slot)
            yield out
        else:
            raise ValueError(group)
    rt, rp, rv, lab, at = out["rt"], out["rp"], out["rv"], out["lab"], out["at"]
    out["back.rt_scores"], out["back.rt_valid"] = rt.gather(nb.scores), rt.valid
    out["back.rp_gather"], out["back.rp_labels"], out["back.rp_empty"] = rp.gather(inp.per_row), rp.labels(lab), rp.empty_flag
    out["back.rv_nonempty"] = rv.nonempty
    out["back.rv_max_grid"], out["back.rv_avg_grid"] = rv.as_grid(rv.max_features(inp.feats)), rv.as_grid(rv.avg)
    out["back.rv_avg_features"] = rv.avg_features(inp.feats)
    out["back.at_matched"], out["back.at_positive"] = at.matched(out["back.live"]), at.positive
    out["back.at_reg_weights"], out["back.at_cls_weights"] = at.reg_weights(), at.cls_weights()
    yield out


def chain(res, inp, bufs=None, order=GROUPS, pools=POOLS, slot=0):
    """The chain queued on torch's current stream; returns the results."""
    out = None
    for out in _steps(res, inp, bufs, order, pools, slot):
        pass
    return out


def flat(out):
    """name -> tensor for every tensor of a chain's results, under the names of head_reference.compose."""
    got = {}
    for name, v in out.items():
        if torch.is_tensor(v):
            got[name] = v
        else:
            for f in hr.FIELDS[name]:
                got[name + "." + f] = getattr(v, f)
    return got


def snapshot(out):
    """Clones of a chain's results, queued on torch's current stream."""
    return {name: t.clone() for name, t in flat(out).items()}


def host(tensors):
    return {name: t.cpu().numpy() for name, t in tensors.items()}


def same(got, want, what):
    """Byte for byte, in chain order: the first differing tensor names the stage.  (Names with a '_' are notes of the composition, not
    outputs of the chain.)"""
    names = [name for name in want if not name.startswith("_")]
    assert set(names) == set(got), (what, set(names) ^ set(got))
    for name in names:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.reshape(g.size, -1).view(np.uint8) != w.reshape(w.size, -1).view(np.uint8)).any(axis=1)) if g.size else []
            raise AssertionError((what, name, "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], w.reshape(-1)[bad[:4]]))


def run(name, dtype, order=GROUPS, pools=POOLS, slot=0, stream=None):
    """One batch through the chain under a side stream; (host results, inputs) after ONE synchronize."""
    want_of(name, dtype)                                                    # (the poses are asked for before anything is queued)
    inp = Inputs(name, dtype)
    s = stream or torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())                              # (the inputs were uploaded on the default stream)
    with torch.cuda.stream(s):
        out = chain(inp.result(slot), inp, order=order, pools=pools, slot=slot)
    s.synchronize()
    return host(flat(out)), inp


_SIDE = {}


def side_stream_run(dtype):
    """The ragged batch under a side stream, run once per dtype and shared (read-only) by the tests that compare against it."""
    if dtype not in _SIDE:
        _SIDE[dtype] = run("ragged", dtype)
    return _SIDE[dtype]


# ---- 1. a side stream ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", hr.DTYPES)
def test_chain_on_a_side_stream(dtype):
    """The ragged batch -- two large frames, a 1025-row frame, one row, no row, an all-absent frame; 96 proposals and 12 gts each -- through
    the chain under torch.cuda.stream(s), nothing read before the end.  The conditions of tests/test_head_reference.py hold on what the
    device gave.  Seen on one MI355X, float32 and float64 alike: 48, 29, 33, 0, 7, 31 kept boxes; (fg, hard, easy) candidates (3, 2, 43),
    (3, 4, 22), (4, 3, 26), (0, 0, 0), (7, 0, 0), (0, 0, 31) and segments (3, 2, 27), (3, 4, 25), (4, 3, 25), (0, 0, 0), (32, 0, 0),
    (0, 0, 32); 42 of 160 sampled rois regression targets; 75 sampled rois without a row, 72 below and 13 above n_samples; 94 sub-voxels at
    max_points; 3771 of 7954 and 2892 of 5942 present rows within reach of a roi, sectors (528, 1184, 1027, 1032) and (854, 1156, 882, 0);
    384 empty balls, 23 and 83 over their sample count; gts kept per frame 5, 5, 1, 0, 0, 0; positives per frame 5, 5, 1, 0, 0, 0; 3
    ignored anchors."""
    got, inp = side_stream_run(dtype)
    want = want_of("ragged", dtype)
    cond = hr.conditions(got, inp.host)
    print(dtype, cond)
    hr.check(cond)
    same(got, want, dtype)


# ---- 2. torch's legacy default stream ----------------------------------------------------------------------------------------------------------
def test_chain_on_the_default_stream():
    """No stream context: every call forks from the default stream to the engine's side stream and joins back, and the ways back are
    torch's own kernels on the default stream in between.  Clones queued behind the chain hold the result, and every byte equals the
    side-stream run's."""
    side, _ = side_stream_run("float32")
    inp = Inputs("ragged", "float32")
    assert torch.cuda.current_stream().cuda_stream == 0
    out = chain(inp.result(), inp)
    snap = snapshot(out)
    torch.cuda.current_stream().synchronize()
    same(host(snap), side, "default stream")
    same(host(flat(out)), side, "default stream, read directly")


# ---- 3. the order of the independent groups ------------------------------------------------------------------------------------------------
def test_group_order_changes_no_byte():
    """Behind nms the groups {keypoints -> balls}, {overlaps -> sampled rois -> the two poolings} and {box labels -> kept gts -> anchor
    targets} forwards, backwards and in one seeded permutation, the poolings in both orders, on one context and one stream: identical
    bytes for every output (nms and boxes_iou share their records, the two poolings their run tables' size; a stage that left something
    for the next, or read what the one before left, would show here)."""
    side, _ = side_stream_run("float32")
    inp = Inputs("ragged", "float32")
    shuffled = tuple(GROUPS[i] for i in np.random.default_rng(5).permutation(3))          # (rois, anchors, keypoints)
    orders = ((GROUPS, POOLS), (GROUPS[::-1], POOLS[::-1]), (shuffled, POOLS[::-1]), (GROUPS, POOLS[::-1]))
    assert len({o for o, _ in orders}) == 3
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res = inp.result()
        outs = [chain(res, inp, order=order, pools=pools) for order, pools in orders]
    s.synchronize()
    for order, out in zip(orders, outs):
        same(host(flat(out)), side, order)


# ---- 4. the context's scratch after other batches ----------------------------------------------------------------------------------------------
def test_scratch_survives_a_change_of_batch():
    """Ragged, small, ragged, ragged reversed on one engine and one stream, float64 first and float32 after it (buffers sized in bytes are
    reused across the widths): every run equals its own composition, whatever the batch before it left in the grow-only scratch -- small is
    smaller than ragged in every quantity that sizes a buffer (tests/test_head_reference.py), so it runs in the front of buffers that
    still hold ragged's records, run tables and offsets."""
    s = torch.cuda.Stream()
    for dtype in ("float64", "float32"):
        for name in ("ragged", "small", "ragged", "ragged_reversed"):
            got, inp = run(name, dtype, stream=s)
            same(got, want_of(name, dtype), (dtype, name))
            if name == "small":
                assert got["back.rt_valid"].all() and (got["rp.count"] > 0).any() and got["back.rv_nonempty"].any() and (got["kp.index"] >= 0).all()
                assert got["back.keep_boxes"].any() and (got["at.count"][:, 0] > 0).all() and got["back.at_matched"].any() and (got["groups.count"] > 0).all()


# ---- 5. two contexts -------------------------------------------------------------------------------------------------------------------------
def test_two_slots_in_flight():
    """slot=0 under stream A and slot=1 under stream B -- one context per stream, never one context on two --, the ragged batch on one
    and its reverse on the other, queued alternately stage by stage, one synchronize at the end."""
    for name in ("ragged", "ragged_reversed"):
        want_of(name, "float32")
    a, b = Inputs("ragged", "float32"), Inputs("ragged_reversed", "float32")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(torch.cuda.current_stream())
    sb.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(sa):
        steps_a = _steps(a.result(0), a, slot=0)
    with torch.cuda.stream(sb):
        steps_b = _steps(b.result(1), b, slot=1)
    out_a = out_b = None
    for _ in range(STEPS):
        with torch.cuda.stream(sa):
            out_a = next(steps_a)
        with torch.cuda.stream(sb):
            out_b = next(steps_b)
    assert next(steps_a, None) is None and next(steps_b, None) is None and "back.at_cls_weights" in out_a and "back.at_cls_weights" in out_b
    torch.cuda.synchronize()
    for inp, out in ((a, out_a), (b, out_b)):
        same(host(flat(out)), want_of(inp.name, "float32"), inp.name)


# ---- 6. the documented capture ---------------------------------------------------------------------------------------------------------------
NO_STEP = tuple(hr.BEFORE_SAMPLING) + ("back.keep_boxes", "back.live", "back.at_matched", "back.at_positive", "back.at_reg_weights", "back.at_cls_weights", "rt.segments",
                                       "rt.class_count", "back.rt_valid")


def test_the_second_stage_and_the_anchor_targets_in_one_graph():
    """INTEGRATION.md's recipe: one eager warm-up of the whole chain into out= buffers with a device step word, then the chain and
    `step += 1` captured once on a side stream -- no parallel branch -- and replayed four times, on scenes 0, 1, 2 and 0 again: rows, keep
    mask, proposals, scores and gts copied in place and every output buffer filled with 0x7f bytes before each replay, nothing read in
    between.  Replay k equals the eager chain on the same inputs at step k + 1 and the composition; the two replays of scene 0 agree in
    everything that does not depend on the step and differ in the picks.  Seen on one MI355X: kept boxes (24, 11, 15), (17, 13, 24),
    (0, 24, 12) in scenes 0, 1, 2; branches aaa, aca, daa; gts kept (3, 1, 1), (2, 0, 1), (3, 2, 1), as many positives each."""
    names = [f"scenes{v}" for v in range(hr.SCENES)]
    for name in names:
        want_of(name, "float32")
    scenes = [Inputs(name, "float32") for name in names]
    inp = Inputs(names[0], "float32")
    played = (0, 1, 2, 0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res = inp.result()
        eager = []
        for k, v in enumerate(played):                                      # the yardstick: the eager chain at the step the replay will see
            inp.load(scenes[v])
            inp.step.fill_(k + 1)
            eager.append(snapshot(chain(res, inp)))
        inp.load(scenes[0])
        inp.step.fill_(0)
        bufs = Buffers(inp)
        chain(res, inp, bufs)                                               # warm-up of everything: step 0
        inp.step += 1
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = chain(res, inp, bufs)
            inp.step += 1
        assert out["nb"] is bufs.nb and out["rt"] is bufs.rt and out["rv"] is bufs.rv and out["at"] is bufs.at and out["back.live"] is bufs.live
        snaps = []
        for v in played:                                                    # no host read between the replays
            inp.load(scenes[v])
            for t in bufs.tensors() + list(flat(out).values()):
                t.view(torch.uint8).fill_(0x7f)
            g.replay()
            snaps.append(snapshot(out))
        s.synchronize()
    assert int(inp.step[0]) == 1 + len(played)
    got = [host(snap) for snap in snaps]
    for k, v in enumerate(played):
        same(got[k], host(eager[k]), ("replay against the eager chain", k))
        want = want_of(names[v], "float32", k + 1)
        print("replay", k, "scene", v, "kept", want["nb.count"].tolist(), "branches", want["_branch"].tolist(), "gts kept", want["back.keep_boxes"].sum(axis=1).tolist(),
              "positives", want["at.count"][:, 0].tolist())
        same(got[k], want, ("replay", k))
    for name in got[0]:
        if name.split(".")[0] in NO_STEP or name in NO_STEP:
            assert got[0][name].tobytes() == got[3][name].tobytes(), name
    assert not np.array_equal(got[0]["rt.index"], got[3]["rt.index"]) and not np.array_equal(got[0]["rp.index"], got[3]["rp.index"])
