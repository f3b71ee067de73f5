"""-m gpu: the object paste in front of the documented training step -- paste_objects, augment_batch(layout='aligned', keep=) on its rows
and keep mask, points_in_boxes(res, pb.gt_boxes) on the result -- on the frames and tables of tests/chain_reference.py, with a bank cropped
from those frames (so channels and ranges are valid for the snowfall stage), eagerly and as ONE captured graph.  Both must equal, byte for
byte, the same two later stages run on the restatement's rows, keep mask and boxes (tests/paste_reference.py) uploaded from NumPy."""
import numpy as np
import pytest
import torch

import box_reference as br
import chain_reference as cr
import paste_reference as pr
from lidar_snow_sim_amd.tensors import paste_objects  # noqa: F401  (the stage under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

BD = float(np.degrees(3e-3))
POLY = [1e-3, 0.05, 12.0]
GROUPS = (6, 6, 6)                        # a frame of the ragged batch holds 3 or 4 boxes of each class: 2 or 3 slots of each are active
SEED, STEP = 77, 4
EW = (0.2, 0.2, 0.2)
LATER = ("rows", "keep", "counts", "stats", "box_of", "count", "local")


@pytest.fixture(scope="module")
def tl(tables):
    return [tables["t"][i % 4] for i in range(64)]


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _crop_bank(b):
    """The rows of the two full frames inside their boxes (the first box of a row, rows the batch's own mask keeps), at least
    chain_reference.MIN_POINTS of them, sorted by class."""
    lab = br.points_in_boxes(b["rows"], b["boxes"], b["pose"], b["keep0"], b["offsets"])
    objects = []
    for f in cr.FULL:
        a, z = int(b["offsets"][f]), int(b["offsets"][f + 1])
        for k in np.flatnonzero(br.present(b["boxes"][f], b["pose"][f])):
            rows = b["rows"][a:z][lab["box_of"][a:z] == k]
            if len(rows) >= cr.MIN_POINTS:
                objects.append((int(b["boxes"][f, k, 7]), rows, b["boxes"][f, k], b["pose"][f, k]))
    objects.sort(key=lambda o: o[0])
    return pr.make_bank(np.concatenate([o[1] for o in objects]), np.concatenate(([0], np.cumsum([len(o[1]) for o in objects]))), np.stack([o[2] for o in objects]),
                        np.stack([o[3] for o in objects]))


class Inputs:
    def __init__(self, dtype):
        from lidar_snow_sim_amd.tensors import DeviceBatch, ObjectBank
        b = self.host = cr.batch("ragged", dtype)
        self.F, self.offsets = len(b["frames"]), b["offsets"].copy()
        self.bank_host = _crop_bank(b)
        self.bank = ObjectBank(_t(self.bank_host["points"]), self.bank_host["offsets"], _t(self.bank_host["boxes"]), _t(self.bank_host["pose"]))
        self.rows, self.mask, self.boxes, self.pose = _t(b["rows"]), _t(b["keep0"]), _t(b["boxes"]), _t(b["pose"])
        self.batch = DeviceBatch(self.rows, self.offsets)
        self.orders = [list(np.random.default_rng(1900 + len(p)).permutation(64)) for p in b["frames"]]

    def expected(self, step):
        b = self.host
        return pr.paste_objects(b["rows"], b["offsets"], b["keep0"], b["boxes"], b["pose"], self.bank_host, GROUPS, SEED, step, EW)


def _later(inp, tl, rows, keep, gt_boxes, pose, res=None):
    """The two stages behind the paste, queued on torch's current stream."""
    from lidar_snow_sim_amd.tensors import DeviceBatch, augment_batch, points_in_boxes
    res = augment_batch(DeviceBatch(rows, inp.offsets), "unused", BD, particles=tl, layout="aligned", keep=keep, thr_polys=[POLY] * inp.F, orders=inp.orders, sync=False,
                        out=res)
    return res, points_in_boxes(res, gt_boxes, pose=pose, return_local=True)


def _host(res, lab):
    return dict(rows=res.rows.cpu().numpy(), keep=res.keep.cpu().numpy(), counts=res.counts.cpu().numpy(), stats=res.stats.cpu().numpy(),
                box_of=lab.box_of.cpu().numpy(), count=lab.count.cpu().numpy(), local=lab.local.cpu().numpy())


def _yardstick(inp, tl, e):
    """The later stages on the restatement's outputs, uploaded from NumPy."""
    res, lab = _later(inp, tl, _t(e["rows"]), _t(e["keep"]), _t(e["gt_boxes"]), _t(e["pose"]))
    res.wait()
    return _host(res, lab)


def _equal(got, want, what):
    for name in LATER:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), (what, name)


@pytest.mark.parametrize("dtype", cr.DTYPES)
def test_paste_snowfall_and_box_labels_eagerly(tl, dtype):
    inp = Inputs(dtype)
    e = inp.expected(STEP)
    B = inp.host["boxes"].shape[1]
    pasted_rows = e["source"] >= 0
    print(dtype, "bank objects", len(inp.bank_host["boxes"]), "states", [np.bincount(s, minlength=6).tolist() for s in e["state"]], "count", e["count"].tolist())
    # the comparison decides something: objects are pasted, among them into the frame whose rows are all absent, and scene rows are removed
    assert e["count"][:, 0].sum() >= 3 and e["count"][5, 0] >= 1 and e["count"][:, 2].sum() >= 1 and (e["state"] == 2).any()
    pb = paste_objects(inp.batch, inp.boxes, inp.bank, GROUPS, step=torch.tensor([STEP], dtype=torch.int64, device="cuda"), seed=SEED, keep=inp.mask,
                       remove_extra_width=EW, pose=inp.pose, return_pose=True)
    res, lab = _later(inp, tl, pb.rows, pb.keep, pb.gt_boxes, pb.pose)
    res.wait()
    for name in pr.FIELDS:
        assert getattr(pb, name).cpu().numpy().tobytes() == e[name].tobytes(), name
    got, want = _host(res, lab), _yardstick(inp, tl, e)
    _equal(got, want, dtype)
    # pasted rows went through the snowfall stage: the all-absent frame has kept rows now, every one of them a pasted row, and its pasted
    # boxes hold rows; rows the stage kept are rows the paste left present
    a, z = int(inp.offsets[5]), int(inp.offsets[6])
    assert 0 < got["counts"][5] == int(got["keep"][a:z].sum()) <= int(e["count"][5, 1]) and pasted_rows[a:z][got["keep"][a:z]].all()
    assert not got["keep"][~e["keep"]].any() and got["count"][5, B:].sum() >= 1
    for f in range(inp.F):
        a, z = int(inp.offsets[f]), int(inp.offsets[f + 1])
        assert got["counts"][f] + got["stats"][f, 1] == int(e["keep"][a:z].sum()), f          # kept + removed = the present rows, pasted ones included


def test_paste_snowfall_and_box_labels_in_one_graph(tl):
    """paste_objects into out=, the aligned call on its rows and keep into out=res, points_in_boxes into out= and step += 1, captured once
    on a side stream after one warm-up and replayed twice: each replay equals the later stages on the restatement at its step."""
    from lidar_snow_sim_amd.tensors import BoxLabelBatch, DeviceBatch, PasteBatch, augment_batch, points_in_boxes
    inp = Inputs("float32")
    B, Q = inp.host["boxes"].shape[1], sum(GROUPS)
    out = PasteBatch.empty(inp.offsets, B, Q, 8, torch.float32, with_pose=True)
    lab = BoxLabelBatch.empty(inp.offsets, B + Q, torch.float32, with_local=True)
    step = torch.tensor([STEP - 1], dtype=torch.int64, device="cuda")
    state = {}

    def call():
        pb = paste_objects(inp.batch, inp.boxes, inp.bank, GROUPS, step=step, seed=SEED, keep=inp.mask, remove_extra_width=EW, pose=inp.pose, out=out, return_pose=True)
        state["res"] = augment_batch(DeviceBatch(pb.rows, inp.offsets), "unused", BD, particles=tl, layout="aligned", keep=pb.keep, thr_polys=[POLY] * inp.F,
                                     orders=inp.orders, sync=False, out=state.get("res"))
        points_in_boxes(state["res"], pb.gt_boxes, pose=pb.pose, return_local=True, out=lab)
        step.add_(1)

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()                                                            # warm-up: the captured calls allocate nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        res = state["res"]
        snaps = []
        for k in range(2):                                                # no host read between the replays
            g.replay()
            snaps.append({n: t.clone() for n, t in dict(rows=res.rows, keep=res.keep, counts=res.counts, stats=res.stats, box_of=lab.box_of, count=lab.count,
                                                        local=lab.local, object=out.object).items()})
        s.synchronize()
    assert int(step[0]) == STEP + 2
    for k, snap in enumerate(snaps):
        e = inp.expected(STEP + k)
        assert snap["object"].cpu().numpy().tobytes() == e["object"].tobytes(), k
        _equal({n: t.cpu().numpy() for n, t in snap.items()}, _yardstick(inp, tl, e), ("replay", k))
    assert not torch.equal(snaps[0]["object"], snaps[1]["object"])
