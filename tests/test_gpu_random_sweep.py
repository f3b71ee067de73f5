"""-m gpu: seeded random sweeps of the ten point stages against their restatements -- the cross product that the hand-built cases of the
stages' own files never run: a float64 batch with num_features = 5, a per-frame keep list, an empty frame between a 1025-row frame and a
63-row one, an out= object holding stale bytes and a range that cuts rows off on a face, all in one call.  tests/random_sweep_inputs.py
draws the configurations and computes what the restatements (tests/*_reference.py) give for them; tests/test_random_sweep_inputs.py shows
on any machine that the sweep is not vacuous.  The restatements are exact and the coordinates lie on fps_reference.STEP's lattice: every
comparison is of bytes, every element of every produced field, no configuration left out.

One test per stage and dtype walks its 24 configs in order in the process's shared context (slot 0), whose scratch only grows
(csrc/snowgpu_stages.cpp) and by now has served every earlier test: a result that depended on the calls before it would differ from the
restatement here, or from itself in the two passes behind the walk --

  history      configs 0 .. 5 once more after the last: the bytes of the first pass, although the scratch has meanwhile served larger and
               smaller batches, other grids and other arguments;
  forms agree  configs 0, 1, 2 (a DeviceBatch, an F x N x 5 tensor, a list of frames) under every other input form the data allows and every
               other keep form: equal bytes in every field.

test_stages_in_turn runs config i of every stage in turn, i = 0 .. 5: the plain and the sectorized walk share fps_* scratch, the two roi
pools share theirs.  The calls are built through the helpers of the stages' own test files (_t, _same and the entry wrappers).  Every
test prints one [random-sweep] line with what it ran."""
import numpy as np
import pytest
import torch

import random_sweep_inputs as rs
import test_gpu_ball_query as tgq
import test_gpu_boxes as tgb
import test_gpu_dror as tgd
import test_gpu_fps as tgf
import test_gpu_fps_sectors as tgs
import test_gpu_nearest as tgn
import test_gpu_range_image as tgr
import test_gpu_roiaware as tga
import test_gpu_roipool as tgp
import test_gpu_voxelize as tgv

pytestmark = pytest.mark.gpu

MODULE = dict(zip(rs.STAGES, (tgd, tgv, tgf, tgs, tgq, tgn, tgr, tgb, tgp, tga)))
STALE = 0x7f
HISTORY = 6
FORMS_OF = (0, 1, 2)


# ---- a config as a call ---------------------------------------------------------------------------------------------------------------------
def _input(c, form, _t):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    off = c["offsets"]
    if form == "batch":
        return DeviceBatch(_t(c["rows"]), np.array(off))
    if form == "list":
        return [_t(c["rows"][a:b]) for a, b in zip(off[:-1], off[1:])]
    per = np.diff(off)
    assert form == "padded" and (per == per[0]).all()
    return _t(c["rows"].reshape(len(per), int(per[0]), 5))


def _keep(c, form, keep_form, _t):
    keep, off = c["keep"], c["offsets"]
    if keep is None:
        return None
    if keep_form == "list":
        return [_t(keep[a:b]) for a, b in zip(off[:-1], off[1:])]
    keep = keep.astype(np.uint8) if keep_form == "uint8" else keep
    return _t(keep.reshape(len(off) - 1, -1) if form == "padded" else keep)      # (F x N beside an F x N x 5 tensor)


def _stale(out):
    for t in ([out] if torch.is_tensor(out) else vars(out).values()):
        if torch.is_tensor(t):
            t.view(torch.uint8).fill_(STALE)
    return out


def _out(stage, c):
    """The stage's batch object for config c with exactly the fields the call asks for, every byte of them stale."""
    from lidar_snow_sim_amd import tensors as T
    a, fl, dt = c["args"], c["flags"], getattr(torch, c["dtype"])
    F, n, off = len(c["offsets"]) - 1, len(c["rows"]), np.array(c["offsets"])
    if stage == "dror_keep":
        out = torch.empty(n, dtype=torch.bool, device="cuda:0")
    elif stage == "voxelize":
        out = T.VoxelBatch.empty(F, a["max_points"], a["max_voxels"], a["num_features"], dt, n_rows=n if fl["voxel_of"] else None)
    elif stage == "sample_keypoints":
        out = T.KeypointBatch.empty(F, a["n_samples"], a["num_features"], dt, with_dist=fl["dist"])
    elif stage == "sample_keypoints_sectors":
        out = T.KeypointBatch.empty(F, a["n_samples"], a["num_features"], dt, with_dist=fl["dist"], sectors=a["sectors"], with_sector_of=n if fl["sector_of"] else None)
    elif stage == "ball_query":
        out = T.NeighbourBatch.empty(F, a["centres"].shape[1], a["samples"], a["num_features"], dt, with_points=fl["points"])
    elif stage == "nearest_keypoints":
        out = T.NearestBatch.empty(off, a["centres"].shape[1], a["k"], dt, with_weights=fl["weight"])
    elif stage == "range_image":
        out = T.RangeImageBatch.empty(F, a["height"], a["width"], n, a["num_features"], dt, with_count=fl["count"])
    elif stage == "points_in_boxes":
        out = T.BoxLabelBatch.empty(off, a["boxes"].shape[1], dt, with_count=fl["count"], with_local=fl["local"], with_pose=fl["pose"])
    elif stage == "roi_point_pool":
        out = T.RoiPointBatch.empty(F, a["rois"].shape[1], a["n_samples"], a["num_features"], dt, with_points=fl["points"], with_local=fl["local"], with_pose=fl["pose"])
    else:
        Cf = None if a["features"] is None else a["features"].shape[1]
        out = T.RoiVoxelBatch.empty(F, a["rois"].shape[1], a["out_size"], a["max_points"], Cf, with_index=fl["index"])
    return _stale(out)


def _call(stage, c, form=None, keep_form=None):
    """The call of config c -- under another input or keep form if given --, every produced field compared with the restatement byte for
    byte by the stage's own _same; the result as {field: NumPy array}."""
    m = MODULE[stage]
    _t, a, fl = m._t, c["args"], c["flags"]
    form, keep_form = form or c["form"], keep_form or c["keep_form"]
    frames, keep, out = _input(c, form, _t), _keep(c, form, keep_form, _t), _out(stage, c) if c["out"] else None
    opt = lambda v: None if v is None else _t(v)
    if stage == "dror_keep":
        got = m._keep(frames, a["alpha"], a["beta"], a["k_min"], a["sr_min"], keep, out=out, return_neighbours=fl["neighbours"])
        mask, nb = got if fl["neighbours"] else (got, None)
        assert out is None or mask is out
        assert mask.dtype == torch.bool and (nb is None or nb.dtype == torch.int32)
        res = dict(keep=mask.view(torch.uint8).cpu().numpy().view(np.bool_))      # (the bytes: a stale 0x7f would read as True)
        if nb is not None:
            res["neighbours"] = nb.cpu().numpy()
        want = rs.expected(stage, c)
        for name, g in res.items():
            assert g.dtype == want[name].dtype and g.tobytes() == want[name].tobytes(), (stage, c["dtype"], c["i"], form, keep_form, name)
        return res
    if stage == "voxelize":
        got = m._voxelize(frames, a["range"], a["voxel_size"], a["max_points"], a["max_voxels"], keep=keep, num_features=a["num_features"], out=out,
                          return_voxel_of=fl["voxel_of"])
    elif stage == "sample_keypoints":
        got = m._sample(frames, a["n_samples"], point_cloud_range=a["range"], keep=keep, num_features=a["num_features"], out=out, return_dist=fl["dist"])
    elif stage == "sample_keypoints_sectors":
        got = m._sample(frames, a["n_samples"], point_cloud_range=a["range"], keep=keep, num_features=a["num_features"], out=out, return_dist=fl["dist"],
                        sectors=a["sectors"], rois=opt(a["rois"]), roi_margin=a["roi_margin"], return_sector_of=fl["sector_of"])
    elif stage == "ball_query":
        got = m._query(frames, _t(a["centres"]), list(a["radii"]), list(a["samples"]), point_cloud_range=a["range"], keep=keep, num_features=a["num_features"],
                       out=out, return_points=fl["points"])
    elif stage == "nearest_keypoints":
        got = m._nn(frames, _t(a["centres"]), a["k"], point_cloud_range=a["range"], keep=keep, out=out, return_weights=fl["weight"])
    elif stage == "range_image":
        got = m._project(frames, a["height"], a["width"], fov_up=a["fov"][0], fov_down=a["fov"][1], ring=opt(a["ring"]), range_limits=a["limits"], keep=keep,
                         num_features=a["num_features"], out=out, return_count=fl["count"])
    elif stage == "points_in_boxes":
        got = m._pib(frames, _t(a["boxes"]), pose=_t(a["pose"]), keep=keep, out=out, return_count=fl["count"], return_local=fl["local"], return_pose=fl["pose"])
    elif stage == "roi_point_pool":
        got = m._pool(frames, _t(a["rois"]), a["n_samples"], extra_width=a["extra_width"], pose=_t(a["pose"]), keep=keep, num_features=a["num_features"], out=out,
                      return_points=fl["points"], return_local=fl["local"], return_pose=fl["pose"])
    else:
        got = m._pool(frames, _t(a["rois"]), a["out_size"], a["max_points"], features=opt(a["features"]), extra_width=a["extra_width"], roi_capacity=a["roi_capacity"],
                      pose=_t(a["pose"]), keep=keep, return_index=fl["index"], out=out)
    assert out is None or got is out, (stage, c["i"], "the result is not the out= object")
    produced = rs.fields(stage, c)
    for name, on in fl.items():
        assert (getattr(got, name) is not None) == on, (stage, c["i"], name)
    m._same(got, rs.expected(stage, c), (stage, c["dtype"], c["i"], form, keep_form), produced)
    return {name: getattr(got, name).cpu().numpy() for name in produced}


def _equal(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), what + (name,)


def _other_forms(c):
    uniform = len(set(np.diff(c["offsets"]).tolist())) == 1
    forms = [f for f in rs.FORMS if f != c["form"] and (f != "padded" or uniform)]
    keep_forms = [k for k in rs.KEEP_FORMS if k != c["keep_form"]] if c["keep"] is not None else [c["keep_form"]]
    pairs = [(f, k) for f in forms + [c["form"]] for k in keep_forms + [c["keep_form"]] if (f, k) != (c["form"], c["keep_form"])]
    return list(dict.fromkeys(pairs))


def _say(stage, dtype, cs, **more):
    sizes = [s for c in cs for s in c["sizes"]]
    print(f"\n[random-sweep] {stage} {dtype}: configs {len(cs)}, rows {sum(len(c['rows']) for c in cs)}, frames {len(sizes)}, largest frame {max(sizes)}, "
          f"smallest frame {min(sizes)}" + "".join(f", {k} {v}" for k, v in more.items()))


# ---- the sweeps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", rs.DTYPES)
@pytest.mark.parametrize("stage", rs.STAGES)
def test_sweep_equals_the_restatement(stage, dtype):
    cs = rs.configs(stage, dtype)
    first = [_call(stage, c) for c in cs]
    for c in cs[:HISTORY]:                                    # history: behind every other config of the walk, the bytes of the first pass
        _equal(_call(stage, c), first[c["i"]], (stage, dtype, c["i"], "second pass"))
    agreed = 0
    for i in FORMS_OF:                                        # forms agree
        for form, keep_form in _other_forms(cs[i]):
            _equal(_call(stage, cs[i], form=form, keep_form=keep_form), first[i], (stage, dtype, i, form, keep_form))
            agreed += 1
    _say(stage, dtype, cs, replayed=HISTORY, other_forms=agreed, with_out=sum(c["out"] for c in cs), masked=sum(c["keep"] is not None for c in cs))
    assert agreed >= 4


def test_stages_in_turn():
    """History across the stages: config i of every stage, one after the other, i = 0 .. 5, float32, slot 0."""
    ran = 0
    for i in range(HISTORY):
        for stage in rs.STAGES:
            _call(stage, rs.configs(stage, "float32")[i])
            ran += 1
    _say("every stage in turn", "float32", [rs.configs(stage, "float32")[i] for i in range(HISTORY) for stage in rs.STAGES], calls=ran)
