"""No GPU: the blocks the device stages share (lidar_snow_sim_amd/batch.py, the helpers of _native.py) where they need no device -- the out=
check on CPU tensors, the integer and range checks, the int32 clamp -- and that lidar_snow_sim_amd.tensors still offers every name, as
the object of the module the name now lives in."""
import re

import numpy as np
import pytest
import torch

from lidar_snow_sim_amd import _native, batch, stages, tensors


class Pair:
    def __init__(self, a=None, b=None):
        self.a, self.b = a, b


CPU = torch.device("cpu")
WANT = (("a", torch.float32, (2, 3), True), ("b", torch.int32, (4,), False))


def _refused(words, call, *args, **kw):
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        call(*args, **kw)


# ---- _checked_out ------------------------------------------------------------------------------------------------------------------------------
def test_checked_out_passes_what_was_asked_for_and_ignores_the_rest():
    good = torch.zeros((2, 3))
    assert batch._checked_out(torch, "stage", Pair, Pair(good), WANT, CPU) is None                       # b is missing and was not asked for
    assert batch._checked_out(torch, "stage", Pair, Pair(good, torch.zeros(9)), WANT, CPU) is None       # b is wrong and was not asked for
    asked = (WANT[0], WANT[1][:3] + (True,))
    assert batch._checked_out(torch, "stage", Pair, Pair(good, torch.zeros(4, dtype=torch.int32)), asked, CPU) is None
    _refused("stage: out must be a Pair whose b is a contiguous (4,) torch.int32 tensor on the device of the boxes",
             batch._checked_out, torch, "stage", Pair, Pair(good, torch.zeros(9)), asked, CPU)


@pytest.mark.parametrize("out", (Pair(torch.zeros((3, 2))), Pair(torch.zeros((2, 3), dtype=torch.float64)), Pair(torch.zeros((3, 2)).t()), Pair(None),
                                 Pair(np.zeros((2, 3), np.float32)), object(), None),
                         ids=("shape", "dtype", "contiguity", "missing", "no tensor", "kind", "None"))
@pytest.mark.parametrize("where", ("boxes", "rows"))
def test_checked_out_refuses_word_for_word(out, where):
    _refused(f"stage: out must be a Pair whose a is a contiguous (2, 3) torch.float32 tensor on the device of the {where}",
             batch._checked_out, torch, "stage", Pair, out, WANT, CPU, where)


def test_checked_out_names_the_boxes_by_default_and_the_first_field_that_fails():
    both = (("a", torch.float32, (2, 3), True), ("b", torch.int32, (4,), True))
    _refused("nms: out must be a Pair whose a is a contiguous (2, 3) torch.float32 tensor on the device of the boxes",
             batch._checked_out, torch, "nms", Pair, Pair(), both, CPU)
    _refused("nms: out must be a Pair whose a is a contiguous (2, 3) torch.float32 tensor on the device of the boxes",
             batch._checked_out, torch, "nms", Pair, Pair(torch.zeros((2, 3), device="meta")), both, CPU)      # another device


# ---- _whole, _range6 ----------------------------------------------------------------------------------------------------------------------------
def test_whole_takes_whole_numbers_and_names_the_first_other():
    assert batch._whole("stage", a=3, b=4.0, c=np.int64(5), d=np.float32(2.0)) is None
    assert batch._whole("stage") is None
    for bad in (2.5, True, False, np.float64(0.5)):
        _refused("stage: b must be an integer", batch._whole, "stage", a=1, b=bad, c=2.5)


def test_range6_of_the_stages():
    assert batch._range6("stage", None) is None
    for rng in ((0, 1, 2, 3, 4, 5), [[0, 1, 2], [3, 4, 5]], np.arange(6, dtype=np.float32)):
        got = batch._range6("stage", rng)
        assert got.dtype == np.float64 and got.shape == (6,) and got.tolist() == [0, 1, 2, 3, 4, 5]
    for rng in ((0, 1, 2, 3, 4), (), np.zeros(7)):
        _refused("stage: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)", batch._range6, "stage", rng)


# ---- _native ------------------------------------------------------------------------------------------------------------------------------------
def test_i32_clamps_at_both_ends():
    assert [_native._i32(v) for v in (0, -7, 5.9, 2 ** 31 - 1, -(2 ** 31))] == [0, -7, 5, 2 ** 31 - 1, -(2 ** 31)]
    assert _native._i32(2 ** 31) == 2 ** 31 - 1 and _native._i32(2 ** 70) == 2 ** 31 - 1
    assert _native._i32(-(2 ** 31) - 1) == -(2 ** 31) and _native._i32(-(2 ** 70)) == -(2 ** 31)
    assert _native._i32(np.int64(2 ** 40)) == 2 ** 31 - 1 and type(_native._i32(np.int64(3))) is int


def test_range6_of_the_wrappers():
    assert _native._range6("snowgpu_fps_device", None) is None
    got = _native._range6("snowgpu_fps_device", np.arange(12, dtype=np.float32)[::2])
    assert got.dtype == np.float64 and got.flags.c_contiguous and got.tolist() == [0, 2, 4, 6, 8, 10]
    for who in ("snowgpu_fps_device", "snowgpu_ball_query_device"):
        _refused(f"{who}: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)", _native._range6, who, (0, 0, 0, 1, 1))


# ---- the import path ----------------------------------------------------------------------------------------------------------------------------
HOME = {
    batch: ("LANE_SLOT0", "is_device_input", "DeviceBatch", "DeviceResult", "AlignedResult", "AlignedWetResult"),
    stages: ("fov_keep", "dror_keep", "voxelize", "sample_keypoints", "ball_query", "range_image", "nearest_keypoints", "points_in_boxes", "boxes_iou",
             "nms", "VoxelBatch", "KeypointBatch", "NeighbourBatch", "RangeImageBatch", "NearestBatch", "BoxLabelBatch", "IouBatch", "NmsBatch", "IOU_MODES"),
    tensors: ("WET_DEFAULTS", "table_ids_for", "table_ids_per_frame", "weather_records", "WEATHER_PER_FRAME", "WeatherPlan", "augment_batch",
              "wet_ground_batch_aligned", "augment_wet_batch_aligned"),
}


@pytest.mark.parametrize("name, home", [(name, home) for home, names in HOME.items() for name in names])
def test_tensors_offers_every_name_as_the_object_of_its_module(name, home):
    obj = getattr(home, name)
    assert getattr(tensors, name) is obj
    assert getattr(obj, "__module__", home.__name__) == home.__name__          # (a function or class is defined there, not passing through)


def test_every_public_name_of_the_two_modules_is_offered():
    for home in (batch, stages):
        public = [n for n, v in vars(home).items() if not n.startswith("_") and getattr(v, "__module__", home.__name__) == home.__name__
                  and not isinstance(v, type(np))]
        assert public and all(getattr(tensors, n) is getattr(home, n) for n in public), home.__name__
