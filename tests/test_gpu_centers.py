"""-m gpu: centre heatmap targets on the device (tensors.assign_centers, centers.assign_targets, snowgpu_assign_centers_device;
csrc/snowgpu_centers.hip, csrc/sg_centers.h) against the restatement of its definition (tests/centers_reference.py, whose cases
tests/test_centers_reference.py holds to the conditions that keep these comparisons from being vacuous).  Everything but one exp is
separately rounded float64 arithmetic, integer ranks and a maximum; the exp's float64 value stays more than 4 ulp from every float32
rounding midpoint (the same no-GPU module walks all of them): every output is compared byte for byte, for both dtypes, with no element
left out."""
import numpy as np
import pytest
import torch

import centers_reference as cr
from lidar_snow_sim_amd.stages import CenterTargetBatch, assign_centers  # noqa: F401  (the stage under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

DTYPES = cr.DTYPES
FIELDS = cr.FIELDS


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _np(t):
    return (t.view(torch.uint8) if t.dtype == torch.bool else t).cpu().numpy()


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = _np(getattr(got, name))
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


def _empty(c, dtype, fill=0xFF):
    F, B, _ = c["gt_boxes"].shape
    heads = c["class_head"] or [0] * c["n_classes"]
    out = CenterTargetBatch.empty(F, B, c["n_classes"], max(heads) + 1, c["max_objs"], c["feature_map_size"], getattr(torch, dtype))
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(fill)
    return out


def _run(c, **kw):
    return assign_centers(_t(c["gt_boxes"]), **cr.settings(c), **kw)


# ---- 1. the shared cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cr.NAMED)
def test_cases(name, dtype):
    """Maps of 8 x 8, 10 x 6, 16 x 16, 24 x 16, 64 x 64, 70 x 19 and 96 x 96; B in 2, 6, 7, 8, 15, 256; F in 1, 3; once into buffers of its own and once
    into out= buffers filled with 0xFF bytes."""
    c, e = cr.case(name, dtype), cr.expected(name, dtype)
    got = _run(c)
    _same(got, e, (name, dtype))
    assert got.mask.dtype == torch.bool and got.heatmap.dtype == torch.float32 and got.state.dtype == torch.uint8
    out = _empty(c, dtype)
    assert _run(c, out=out) is out
    _same(out, e, (name, dtype, "out="))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep(dtype):
    """The 40 seeded configurations, each into out= buffers filled with 0xFF bytes; every output, no case left out."""
    for name in cr.SWEEP_NAMES:
        c = cr.case(name, dtype)
        _same(_run(c, out=_empty(c, dtype)), cr.expected(name, dtype), (name, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_give_the_same_bytes(dtype):
    for name in ("overlap", "slots", "tiles"):
        c = cr.case(name, dtype)
        a, b = _run(c, out=_empty(c, dtype, 0x5A)), _run(c, out=_empty(c, dtype, 0xA5))
        for f in FIELDS:
            assert torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), (name, f)


def test_a_side_stream_and_the_default_stream():
    c, e = cr.case("tiles", "float32"), cr.expected("tiles", "float32")
    gt = _t(c["gt_boxes"])
    torch.cuda.synchronize()
    on_default = assign_centers(gt, **cr.settings(c))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_side = assign_centers(gt, **cr.settings(c), slot=1)
    s.synchronize()
    _same(on_default, e, "default stream")
    _same(on_side, e, "side stream")


# ---- 2. the NumPy call shape and the helpers ---------------------------------------------------------------------------------------------------
def _tolerance(want, dtype):
    """What torch's own log, cos and sin may differ by from NumPy's float64 on the same inputs -- it is theirs, not the kernels'.  The device
    library's logf / log is documented at 1 ulp, sinf / cosf and sin / cos at 2 ulp at most (as recalled: supposed); rounding the float64
    reference to the dtype adds half an ulp, NumPy's float64 functions less than one float64 ulp, which matters for float64 only: at most
    3.5 ulp, and an ulp of x is at most eps |x|.  Hence 4 eps |want|, and exactly 0 where want is 0 (log 1, sin 0)."""
    return 4 * np.finfo(dtype).eps * np.abs(want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_target_boxes(dtype):
    for name in ("sweep_03", "sweep_11", "slots", "radius"):
        c, e = cr.case(name, dtype), cr.expected(name, dtype)
        gt = _t(c["gt_boxes"])
        got = _run(c).target_boxes(gt)
        want = cr.target_boxes(e, c["gt_boxes"])
        F, NH, M = e["gt_index"].shape
        assert got.dtype == gt.dtype and tuple(got.shape) == (F, NH, M, c["gt_boxes"].shape[2])
        g = got.cpu().numpy().astype(np.float64)
        exact = [0, 1, 2] + list(range(8, g.shape[-1]))                 # offset, z and the extra columns: copies
        assert np.array_equal(g[..., exact], want[..., exact].astype(dtype).astype(np.float64)), name
        assert (np.abs(g[..., 3:8] - want[..., 3:8]) <= _tolerance(want[..., 3:8], dtype)).all(), (name, np.abs(g[..., 3:8] - want[..., 3:8]).max())
        assert not g[e["gt_index"] < 0].any() and np.abs(want[..., 3:8]).max() > 0.5 and (e["gt_index"] >= 0).any()
    with pytest.raises(ValueError, match="target_boxes: gt_boxes must be"):
        _run(c).target_boxes(gt[:, :-1])


def test_the_host_array_mirror():
    from lidar_snow_sim_amd import centers
    for name, dtype in (("overlap", "float64"), ("by_hand", "float32"), ("edges_drop_below", "float32")):
        c, e = cr.case(name, dtype), cr.expected(name, dtype)
        heatmap, ret_boxes, inds, mask, fields = centers.assign_targets(c["gt_boxes"][0], **cr.settings(c), return_batch=True)
        for field in FIELDS:
            assert fields[field].dtype == (np.bool_ if field == "mask" else e[field].dtype) and fields[field].tobytes() == e[field][0].tobytes(), (name, field)
        assert heatmap.tobytes() == e["heatmap"][0].tobytes() and inds.dtype == np.int64 and np.array_equal(inds, e["ind"][0]) and mask.dtype == np.bool_
        assert np.array_equal(mask, e["mask"][0].astype(bool)) and ret_boxes.shape == e["gt_index"].shape[1:] + (8,) and ret_boxes.dtype == np.dtype(dtype)
        assert np.array_equal(ret_boxes[..., :2], e["offset"][0]) and len(centers.assign_targets(c["gt_boxes"][0], **cr.settings(c))) == 4


def test_head_heatmap_is_a_channel_slice():
    c = cr.case("slots", "float32")
    got = _run(c)
    assert got.class_head == (0, 1, 0)
    assert torch.equal(got.head_heatmap(1), got.heatmap[:, 1:2]) and got.head_heatmap(1).data_ptr() == got.heatmap[:, 1:2].data_ptr()
    assert torch.equal(got.head_heatmap(0), got.heatmap[:, [0, 2]])
    with pytest.raises(ValueError, match="no class has head 2"):
        got.head_heatmap(2)
    both = assign_centers(_t(c["gt_boxes"]), **dict(cr.settings(c), class_head=(0, 0, 1)))
    assert both.head_heatmap(0).data_ptr() == both.heatmap.data_ptr() and tuple(both.head_heatmap(0).shape) == (3, 2, 16, 16)


# ---- 3. one graph -----------------------------------------------------------------------------------------------------------------------------
def _scene(seed, B, n, W, H, voxel, stride):
    """F = 3 frames of n rows, most of them inside the frame's gts (a gt holds none, a few or many), a keep mask and the gts."""
    rng = np.random.default_rng(seed)
    F = 3
    gt = np.zeros((F, B, 8), np.float32)
    gt[..., 0], gt[..., 1] = rng.uniform(-2, W * voxel * stride + 2, (F, B)), rng.uniform(-2, H * voxel * stride + 2, (F, B))
    gt[..., 2], gt[..., 3:6] = rng.uniform(-1, 1, (F, B)), rng.uniform(0.6, 6.0, (F, B, 3))
    gt[..., 6], gt[..., 7] = rng.uniform(-3, 3, (F, B)), rng.integers(1, 4, (F, B))
    rows = np.zeros((F * n, 5), np.float32)
    for f in range(F):
        g = gt[f, rng.integers(0, B // 2, n)]                             # only the first half of the gts gets rows
        rows[f * n:(f + 1) * n, :3] = g[:, :3] + rng.uniform(-0.3, 0.3, (n, 3)) * g[:, 3:6]
    rows[:, 3], rows[:, 4] = rng.integers(1, 255, F * n), rng.integers(0, 64, F * n)
    return rows, rng.uniform(0, 1, F * n) < 0.8, gt


def test_keep_boxes_assign_and_target_boxes_in_one_graph():
    """points_in_boxes(res, gt).keep_boxes(5) -> the gts zeroed by that mask -> assign_centers(out=) -> .target_boxes(), captured once and
    replayed after rows, keep mask and gt boxes were rewritten in place -- and, before the last replay, after the stage ran in the same
    context with another configuration (another map, stride, heads, slots and `outside`; no more frames and gts than the captured call,
    since scratch that grows is reallocated, for this stage as for every other, and a captured graph holds its address): each replay equals
    the restatement on the gts the chain kept."""
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import AlignedResult, BoxLabelBatch, points_in_boxes
    F, B, n, W, H, voxel, stride = 3, 24, 900, 70, 40, 0.1, 4
    cfg = dict(point_cloud_range=(0.0, 0.0, -3.0, W * voxel * stride, H * voxel * stride, 1.0), voxel_size=(voxel, voxel, 0.1), stride=stride,
               feature_map_size=(W, H), n_classes=3, class_head=(0, 1, 1), max_objs=5, gaussian_overlap=0.1, min_radius=2, outside="drop")
    offsets = np.arange(F + 1, dtype=np.int64) * n
    scenes = [_scene(70 + k, B, n, W, H, voxel, stride) for k in range(3)]
    eng = engine.get_engine(torch.cuda.current_device(), 0)
    z = torch.zeros(1, dtype=torch.int64).cuda()
    rows, keep, gt = _t(scenes[0][0]), _t(scenes[0][1]), _t(scenes[0][2])
    live = torch.empty_like(gt)

    def chain(res, labels, out):
        lab = points_in_boxes(res, gt, out=labels)
        live.copy_(gt * lab.keep_boxes(5)[..., None].to(gt.dtype))
        ct = assign_centers(live, **cfg, out=out)
        return ct, ct.target_boxes(live)

    other = cr.case("slots", "float64")                                    # 3 frames of 256 gts would be more scratch: its first 20 gts of two frames
    other_gt, other_cfg = np.ascontiguousarray(other["gt_boxes"][::2, 44:64]), cr.settings(other)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res = AlignedResult(eng.ctx, rows, keep, z, z, z, offsets, s)
        labels, out = BoxLabelBatch.empty(offsets, B, torch.float32), CenterTargetBatch.empty(F, B, 3, 2, 5, (W, H), torch.float32)
        chain(res, labels, out)                                            # warm-up: the captured calls allocate no scratch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ct, tb = chain(res, labels, out)
        assert ct is out
        got = []
        for k, (r, m, b) in enumerate(scenes):                             # no host read between the replays
            rows.copy_(_t(r)); keep.copy_(_t(m)); gt.copy_(_t(b))
            if k == 2:
                between = assign_centers(_t(other_gt), **other_cfg)
            for f in FIELDS:
                getattr(out, f).view(torch.uint8).fill_(0xFF)
            g.replay()
            got.append(({f: getattr(out, f).clone() for f in FIELDS}, tb.clone(), live.clone()))
        s.synchronize()
    _same(between, cr.assign(other_gt, **other_cfg), "the other configuration")
    assert between.mask.any()
    states = set()
    for k in range(3):
        kept = got[k][2].cpu().numpy()
        present = kept[..., 3] > 0
        assert present.any(axis=1).all() and (~present & (scenes[k][2][..., 3] > 0)).any()      # the mask keeps some gts and drops some
        want = cr.assign(kept, **cfg)
        for f in FIELDS:
            assert _np(got[k][0][f]).tobytes() == want[f].tobytes(), (k, f)
        tb_want = cr.target_boxes(want, kept)
        assert (np.abs(got[k][1].cpu().numpy() - tb_want) <= _tolerance(tb_want, "float32") + 0).all() and got[k][1].any()
        states |= set(want["state"].reshape(-1).tolist())
    assert states == {0, 1, 2, 3}
    assert not torch.equal(got[0][0]["heatmap"], got[1][0]["heatmap"]) and not torch.equal(got[1][0]["ind"], got[2][0]["ind"])


# ---- 4. what Python refuses -------------------------------------------------------------------------------------------------------------------
def test_python_refusals_in_the_stages_order():
    c = cr.case("overlap", "float32")
    gt, cfg = _t(c["gt_boxes"]), cr.settings(c)

    def refused(words, gt=gt, out=None, **kw):
        with pytest.raises(ValueError, match=words):
            assign_centers(gt, **dict(cfg, **kw), out=out)

    refused("point_cloud_range holds 6 numbers", point_cloud_range=(0, 0, 1, 1))
    refused("voxel_size 3", voxel_size=(1, 1))
    refused("feature_map_size holds 2 whole numbers", feature_map_size=24)
    refused("stride must be an integer", stride=1.5)
    refused("outside must be 'clamp' or 'drop'", outside="skip")
    refused("class_head holds one whole number per class", class_head=(0, 1))
    refused("gt_boxes must be a contiguous", gt=gt.cpu())
    refused("gt_boxes must be a contiguous", gt=gt[0])
    refused("n_gt must lie in 1 .. 256", gt=torch.zeros((1, 257, 8), device="cuda"))
    refused("n_classes must lie in 1 .. 16", n_classes=17, class_head=None)
    refused("every class needs a head in 0 .. 15", class_head=(0, 16, 1))
    refused("every class needs a head in 0 .. 15", class_head=(0, -1, 1))
    refused("max_objs must lie in 1 .. 512", max_objs=513)
    refused("the feature map needs at least one pixel", feature_map_size=(0, 16))
    refused("exceeds 2\\^31 - 1; split the batch", feature_map_size=(65536, 16384))
    refused("out must be a CenterTargetBatch whose heatmap", out=CenterTargetBatch.empty(1, 7, 3, 1, 500, (24, 17)))
    refused("out must be a CenterTargetBatch whose offset", out=CenterTargetBatch.empty(1, 7, 3, 1, 500, (24, 16), torch.float64))
    refused("out must be a CenterTargetBatch whose state", out=CenterTargetBatch.empty(1, 8, 3, 1, 500, (24, 16)))
    # wrong in two ways: the earlier check speaks
    refused("outside must be 'clamp' or 'drop'", gt=gt.cpu(), outside="skip")
    refused("gt_boxes must be a contiguous", gt=gt.double()[0], max_objs=0)
    # what only the entry refuses comes back in the entry's words
    refused("snowgpu_assign_centers_device: gt_features must lie in 8 .. 10", gt=gt[..., :7].contiguous())
    refused("snowgpu_assign_centers_device: the origin of the range must be finite, the voxel's x and y edges positive and finite", voxel_size=(0.0, 1.0, 1.0))
    refused("snowgpu_assign_centers_device: stride must be at least 1", stride=0)
    refused("snowgpu_assign_centers_device: gaussian_overlap must lie strictly between 0 and 1", gaussian_overlap=1.0)
    refused("snowgpu_assign_centers_device: min_radius must lie in 0 .. 512", min_radius=513)
    out = CenterTargetBatch.empty(1, 7, 3, 1, 500, (24, 16))
    out.ind = out.gt_index
    refused("d_out_ind overlaps d_out_gt_index; every output needs memory of its own", out=out)
