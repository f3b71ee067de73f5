"""-m gpu: seeded random sweeps of the six box stages (boxes_iou, nms, sample_rois, assign_anchors, paste_objects, transform_scene)
against their restatements -- the cross product that the hand-built cases of the stages' own files never run: a Cb = 10 box set beside a
Cb = 7 one, a frame in which every box is absent between two full ones, an out= object holding stale bytes with the optional fields off,
B on a tile border with post_max on the kept count, step and seed past 2^32 in a batch whose first frame is empty, all in one call.
tests/box_sweep_inputs.py draws the configurations and computes what the restatements (tests/*_reference.py) give for them;
tests/test_box_sweep_inputs.py shows on any machine that the sweep is not vacuous.  The restatements are exact and take every cos / sin
as an input: every comparison is of bytes, every element of every produced field, no configuration left out.  The pose comes from three
sources in turn: NumPy's, handed over; the device's own (pose=None), which test_gpu_iou._device_pose reads back for the restatement; and
that read-back pose handed over.  transform_scene's restatement is fed the cos / sin the call returned, as test_gpu_scene._want does.

One test per stage and dtype walks its 24 configs in order in the process's shared context (slot 0), whose scratch only grows
(csrc/snowgpu_stages.cpp) and by now has served every earlier test --

  history      configs 0 .. 5 once more after the last: the bytes of the first pass;
  forms agree  paste_objects and transform_scene: configs 0, 1, 2 under every other input form the data allows and every other keep form.

test_box_stages_in_turn runs config i of every stage and a seeded assign_centers case in turn, i = 0 .. 5, and then nms directly behind a
boxes_iou that grew the shared box records (ctx->iou_rec) past it, and the reverse.  The calls are built through the helpers of the
stages' own test files (_t, _same and the entry wrappers).  Every test prints one [box-sweep] line with what it ran.

That the sweep bites.  Three one-line variants, each changing a comparison or a constant only (none can move an index), each built apart
from the tree and run once against this file on the same device; 10 of the 13 tests pass under each, the three named fail:
  - k_nms_sweep `>=` for `>` in both tests (csrc/snowgpu_iou.hip): test_sweep_equals_the_restatement[nms-float32, nms-float64] and
    test_box_stages_in_turn, first at config 2 (B = 63, iou_thresh equal to the IoU of the two best-scored boxes: box 61 is kept at
    equality and the variant drops it);
  - the sample_rois draw keyed by `frame + 1` (k_sample_rois, csrc/snowgpu_targets.hip): test_sweep_equals_the_restatement[sample_rois-float32,
    sample_rois-float64] and test_box_stages_in_turn, first at configs 1 and 2 (config 0 draws one roi of one: no word decides there);
  - the conflict test of k_scene_frame `>= 0.0` for `> 0.0` (csrc/snowgpu_scene.hip): test_sweep_equals_the_restatement[transform_scene-float32,
    transform_scene-float64] and test_box_stages_in_turn, first at configs 1 and 2 (config 0 has no local part)."""
import numpy as np
import pytest
import torch

import box_reference as br
import box_sweep_inputs as bs
import centers_reference as cr
import test_gpu_anchors as tga
import test_gpu_centers as tgc
import test_gpu_iou as tgi
import test_gpu_paste as tgp
import test_gpu_random_sweep as tsw
import test_gpu_scene as tgs
import test_gpu_targets as tgt

pytestmark = pytest.mark.gpu

MODULE = dict(zip(bs.STAGES, (tgi, tgi, tgt, tga, tgp, tgs)))
HISTORY = 6
FORMS_OF = (0, 1, 2)
ROW_STAGES = ("paste_objects", "transform_scene")
_fed = {}                                                                    # the restatements under a device pose, by config and the pose's bytes


# ---- a config as a call ---------------------------------------------------------------------------------------------------------------------
def _pose(c, boxes, given):
    """(the pose argument of the call, the pose the restatement takes) for one box set of config c under its pose source."""
    if c["pose_source"] == "given":
        return tgi._t(given), given
    ok = br.present(boxes, given)
    used = tgi._device_pose(boxes)
    assert np.abs(used[ok] - given[ok]).max(initial=0.0) < 1e-15 and not used[~ok].any()
    used = np.where(ok[..., None], used, given)
    return (None if c["pose_source"] == "device" else tgi._t(used)), used


def _expected(stage, c, **fed):
    """bs.expected, the restatements under a fed-back pose kept by the pose's bytes: the replays ask for the same ones again."""
    own = dict(c["args"], bank_pose=c["args"]["bank"]["pose"]) if stage == "paste_objects" else c["args"]
    if stage != "transform_scene" and all(v.tobytes() == own[k].tobytes() for k, v in fed.items()):
        return bs.expected(stage, c)
    key = (stage, c["dtype"], c["i"]) + tuple((k, v.tobytes()) for k, v in sorted(fed.items()) if v is not None)
    if key not in _fed:
        _fed[key] = bs.expected(stage, c, **fed)
    return _fed[key]


def _boxes_iou(c):
    from lidar_snow_sim_amd.tensors import IouBatch
    a, fl = c["args"], c["flags"]
    (pa, fa), (pb, fb) = _pose(c, a["a"], a["pose_a"]), _pose(c, a["b"], a["pose_b"])
    F, M, B = a["a"].shape[0], a["a"].shape[1], a["b"].shape[1]
    out = tsw._stale(IouBatch.empty(F, M, B, getattr(torch, c["dtype"]), with_iou=fl["iou"], with_best=fl["best"])) if c["out"] else None
    got = tgi._iou(tgi._t(a["a"]), tgi._t(a["b"]), mode=a["mode"], pose_a=pa, pose_b=pb, out=out, return_iou=fl["iou"], return_best=fl["best"])
    assert (got.iou is not None) == fl["iou"] and (got.best is not None) == (got.best_iou is not None) == fl["best"]
    return got, out, _expected("boxes_iou", c, pose_a=fa, pose_b=fb)


def _nms(c):
    from lidar_snow_sim_amd.tensors import NmsBatch
    a, fl = c["args"], c["flags"]
    pose, fed = _pose(c, a["boxes"], a["pose"])
    F, B, Cb = a["boxes"].shape
    out = None
    if c["out"]:
        out = tsw._stale(NmsBatch.empty(F, B, a["post_max"], Cb, getattr(torch, c["dtype"]), with_boxes=fl["boxes"], with_scores=fl["scores"], with_kept=fl["kept"]))
    got = tgi._nms(tgi._t(a["boxes"]), tgi._t(a["scores"]), a["iou_thresh"], post_max=a["post_max"], score_thresh=a["score_thresh"], mode=a["mode"], pose=pose, out=out,
                   return_boxes=fl["boxes"], return_scores=fl["scores"], return_kept=fl["kept"])
    return got, out, _expected("nms", c, pose=fed)


def _sample_rois(c):
    from lidar_snow_sim_amd.tensors import IouBatch, NmsBatch, RoiTargetBatch, sample_rois
    a, fl, _t = c["args"], c["flags"], tgt._t
    pose, fed = _pose(c, a["rois"], a["pose"])
    F, M, Cb = a["rois"].shape
    rois = _t(a["rois"])
    if c["rois_form"] == "nms_batch":
        rois = NmsBatch(torch.zeros((F, M), dtype=torch.int32).cuda(), torch.zeros(F, dtype=torch.int32).cuda(), rois)
    overlaps = (_t(a["overlap"]), _t(a["assignment"])) if c["overlaps_form"] == "pair" else IouBatch(None, _t(a["assignment"]), _t(a["overlap"]))
    out = None
    if c["out"]:
        out = tsw._stale(RoiTargetBatch.empty(F, a["cfg"]["roi_per_image"], Cb, a["gt_boxes"].shape[2], getattr(torch, c["dtype"]), with_pose=fl["pose"], with_local=fl["gt_local"]))
    got = sample_rois(rois, _t(a["gt_boxes"]), overlaps, step=tgt._step(a["step"]), seed=a["seed"], pose=pose, out=out, return_local=fl["gt_local"], return_pose=fl["pose"],
                      **a["cfg"])
    return got, out, _expected("sample_rois", c, pose=fed)


def _assign_anchors(c):
    from lidar_snow_sim_amd.stages import AnchorTargetBatch
    a, fl = c["args"], c["flags"]
    F, B = a["gt_boxes"].shape[:2]
    out = tsw._stale(AnchorTargetBatch.empty(F, a["anchors"].shape[0], B, getattr(torch, c["dtype"]), with_iou=fl["iou"])) if c["out"] else None
    return tga._run(a, out=out, return_iou=fl["iou"]), out, bs.expected("assign_anchors", c)


def _paste_objects(c, form, keep_form):
    from lidar_snow_sim_amd.tensors import PasteBatch, paste_objects
    a, fl, _t = c["args"], c["flags"], tgp._t
    pose, fed = _pose(c, a["gt_boxes"], a["pose"])
    bank = tgp._bank(a["bank"], pose="given" if c["pose_source"] == "given" else None)
    bank_pose = bank.pose.cpu().numpy()
    assert np.allclose(bank_pose, a["bank"]["pose"], rtol=0, atol=1e-15, equal_nan=True)
    F, B, Cb = a["gt_boxes"].shape
    out = None
    if c["out"]:
        out = tsw._stale(PasteBatch.empty(c["offsets"], B, sum(a["groups"]), Cb, getattr(torch, c["dtype"]), with_source=fl["source"], with_pose=fl["pose"]))
    got = paste_objects(tsw._input(c, form, _t), _t(a["gt_boxes"]), bank, a["groups"], step=tgp._step(a["step"]), seed=a["seed"], keep=tsw._keep(c, form, keep_form, _t),
                        remove_extra_width=a["ew"], pose=pose, out=out, return_source=fl["source"], return_pose=fl["pose"])
    return got, out, _expected("paste_objects", c, pose=fed, bank_pose=bank_pose)


def _transform_scene(c, form, keep_form):
    from lidar_snow_sim_amd.tensors import SceneBatch, transform_scene
    a, fl, _t = c["args"], c["flags"], tgs._t
    cfg, T = a["cfg"], c["tries"]
    pose, fed = _pose(c, a["gt_boxes"], a["pose"])
    F, B, Cb = a["gt_boxes"].shape
    box_of = _t(br.points_in_boxes(c["rows"], a["gt_boxes"], fed, c["keep"], c["offsets"])["box_of"]) if a["box_of_given"] else None
    kw = dict(step=tgs._step(a["step"]), seed=a["seed"], flip=cfg["flip"], rotation=cfg["rotation"], scaling=cfg["scaling"], local=cfg["local"], pose=pose, box_of=box_of)
    tries_cs = None
    if T and not fl["tries"]:                                                 # every try's cos / sin comes back in `tries` only: ask for them once, apart
        side = transform_scene(tsw._input(c, form, _t), _t(a["gt_boxes"]), keep=tsw._keep(c, form, keep_form, _t), return_tried=True, **kw)
        tries_cs = side.tries.cpu().numpy()[..., 3:5]
    frames = tsw._input(c, form, _t)
    in_place = a["in_place"] and form == "batch"
    out = None
    if c["out"]:
        out = tsw._stale(SceneBatch.empty(c["offsets"], B, Cb, T, getattr(torch, c["dtype"]), with_pose=fl["pose"], with_tries=fl["tries"]))
        if in_place:
            out.rows = frames.rows
    got = transform_scene(frames, _t(a["gt_boxes"]), keep=tsw._keep(c, form, keep_form, _t), in_place=in_place, out=out, return_pose=fl["pose"], return_tried=fl["tries"], **kw)
    assert not in_place or got.rows.data_ptr() == frames.rows.data_ptr()
    if fl["tries"]:
        tries_cs = got.tries.cpu().numpy()[..., 3:5]
    return got, out, _expected("transform_scene", c, pose=fed, world_cs=got.world.cpu().numpy()[:, 2:4], tries_cs=tries_cs)


CALL = dict(zip(bs.STAGES, (_boxes_iou, _nms, _sample_rois, _assign_anchors, _paste_objects, _transform_scene)))
_sources = {}


def _call(stage, c, form=None, keep_form=None):
    """The call of config c -- under another input or keep form if given --, every produced field compared with the restatement byte for
    byte by the stage's own _same, every other optional field None; the result as {field: NumPy array}."""
    got, out, want = CALL[stage](c, form or c["form"], keep_form or c["keep_form"]) if stage in ROW_STAGES else CALL[stage](c)
    assert out is None or got is out, (stage, c["i"], "the result is not the out= object")
    for name, on in c["flags"].items():
        assert (getattr(got, name) is not None) == on, (stage, c["i"], name)
    produced = bs.fields(stage, c)
    MODULE[stage]._same(got, want, (stage, c["dtype"], c["i"], form, keep_form, c["pose_source"]), produced)
    _sources[c["pose_source"]] = _sources.get(c["pose_source"], 0) + 1
    return {name: tgc._np(getattr(got, name)) for name in produced}


def _count(stage, c):
    a = c["args"]
    return {"boxes_iou": lambda: a["a"].shape[1] * a["b"].shape[1], "nms": lambda: a["boxes"].shape[1], "sample_rois": lambda: a["rois"].shape[1],
            "assign_anchors": lambda: a["anchors"].shape[0], "paste_objects": lambda: a["gt_boxes"].shape[1] + sum(a["groups"]), "transform_scene": lambda: a["gt_boxes"].shape[1]}[stage]()


def _say(what, dtype, pairs, **more):
    counts = [_count(stage, c) for stage, c in pairs]
    print(f"\n[box-sweep] {what} {dtype}: configs {len(pairs)}, frames {sum(c['frames'] for _, c in pairs)}, largest box count {max(counts)}, smallest box count {min(counts)}, "
          f"calls with out= {sum(c['out'] for _, c in pairs)}" + "".join(f", {k} {v}" for k, v in more.items()) +
          ", poses by source " + ", ".join(f"{k} {v}" for k, v in sorted(_sources.items(), key=str)))
    _sources.clear()


# ---- the sweeps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", bs.DTYPES)
@pytest.mark.parametrize("stage", bs.STAGES)
def test_sweep_equals_the_restatement(stage, dtype):
    cs = bs.configs(stage, dtype)
    _sources.clear()
    first = [_call(stage, c) for c in cs]
    for c in cs[:HISTORY]:                                    # history: behind every other config of the walk, the bytes of the first pass
        tsw._equal(_call(stage, c), first[c["i"]], (stage, dtype, c["i"], "second pass"))
    agreed = 0
    if stage in ROW_STAGES:                                   # forms agree
        for i in FORMS_OF:
            for form, keep_form in tsw._other_forms(cs[i]):
                tsw._equal(_call(stage, cs[i], form=form, keep_form=keep_form), first[i], (stage, dtype, i, form, keep_form))
                agreed += 1
        assert agreed >= 4
    _say(stage, dtype, [(stage, c) for c in cs], replayed=HISTORY, other_forms=agreed)


def test_box_stages_in_turn():
    """History across the stages: config i of every stage and a seeded assign_centers case, one after the other, i = 0 .. 5, float32, slot 0;
    then nms directly behind a boxes_iou that grew the shared box records past it, and boxes_iou directly behind the largest nms."""
    _sources.clear()
    ran = []
    for i in range(HISTORY):
        for stage in bs.STAGES:
            c = bs.configs(stage, "float32")[i]
            _call(stage, c)
            ran.append((stage, c))
        name = cr.SWEEP_NAMES[7 * i]
        case = cr.case(name, "float32")
        tgc._same(tgc._run(case, out=tgc._empty(case, "float32")), cr.expected(name, "float32"), (name, "in turn"))
    iou, nms = bs.configs("boxes_iou", "float32"), bs.configs("nms", "float32")
    grown = max(iou, key=lambda c: c["args"]["a"].shape[1] * c["frames"] + c["args"]["b"].shape[1] * c["frames"])
    for stage, c in (("boxes_iou", grown), ("nms", nms[0]), ("nms", nms[2]), ("nms", nms[11]), ("boxes_iou", iou[0]), ("boxes_iou", iou[2])):
        _call(stage, c)
        ran.append((stage, c))
    assert nms[11]["args"]["boxes"].shape[1] == 2049 and grown["args"]["a"].shape[1] + grown["args"]["b"].shape[1] > 2 * nms[2]["args"]["boxes"].shape[1]
    _say("every stage in turn", "float32", ran, calls=len(ran), assign_centers=HISTORY)
