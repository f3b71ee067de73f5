"""Device-resident boundary of augment_batch(): torch CUDA tensors in, torch CUDA tensors out, no host copy of a row.

The reference's training-time caller (the OpenPCDet DENSE dataset: `root_path`, tools/snowfall/simulation.py:53, :324-325; SURVEY 8 b
"Ownership": NumPy array or torch tensor data_ptr) holds its sweeps on the GPU.  `augment_batch(frames, ...)` /
`augment(pc, ...)` of lidar_snow_sim_amd.tools.snowfall.simulation hand anything that is a torch CUDA tensor to this module:

  * the rows are read where they lie (`tensor.data_ptr()`), through snowgpu_augment_batch_device (include/snowgpu.h) -- or
    snowgpu_augment_wet_batch_device with `wet=...` (pointcloud_viewer.py:2807-2821) -- on the CALLER's current torch stream;
  * results are torch tensors on the same device, allocated by torch's caching allocator (no hipMalloc after the first call of a size);
  * `sync=False` returns a DeviceResult at once -- nothing has been waited for, the counts are still a device tensor -- so that the
    call can be chained in front of the consumer's kernels; `sync=True` (default) waits, checks the status words and returns
    the reference-shaped list of (stats, aug_pc) with aug_pc a view of the result tensor;
  * `layout='aligned'` returns the rows in the INPUT's order with one keep flag per row (AlignedResult) instead of compacting them: a
    result whose shape does not depend on the data, so a consumer on the same stream -- or in the same HIP graph -- reads it without a
    host round trip, and per-point companions of the sweep (labels, timestamps, further columns) stay aligned with it.
  * `keep=mask` with `layout='aligned'` (and on augment_wet_batch_aligned) is an INPUT keep mask: a row whose element is False is not there
    -- cropped away, padding of an F x Nmax batch, removed by a stage in front -- and the result is, byte for byte, that of the call on the
    frames compacted by the mask, at the present rows' own indices (snowgpu_augment_batch_device_aligned_masked).  `calib=c, pre_crop=True`
    builds that mask on the device from the camera's view (`fov_keep`): precompute.py:96-104 without a boolean index or a host read.
  * `dror_keep(frames, ...)` is dynamic radius outlier removal (the de-noising filter in front of the viewer's chain) as one more producer
    and consumer of such masks (snowgpu_dror_mask_device).
  * `voxelize(frames_or_result, point_cloud_range, voxel_size, max_points, max_voxels)` groups the present rows of an aligned batch into
    voxels of static shape (VoxelBatch; snowgpu_voxelize_device): the hand-off to a detector's first operation, in the same stream or graph.
  * `sample_keypoints(frames_or_result, n_samples)` takes a fixed number of farthest-point samples from the present rows of every frame
    (KeypointBatch; snowgpu_fps_device): the hand-off to a point-based detector, likewise.
  * `ball_query(frames_or_result, centres, radius, n_neighbours)` groups, around every centre (a KeypointBatch, or any centres), the
    first rows of its frame within each radius (NeighbourBatch; snowgpu_ball_query_device): the grouping step of a set-abstraction layer.
  * `range_image(frames_or_result, height, width)` projects the present rows of every frame into an H x W image of nearest returns
    (RangeImageBatch; snowgpu_range_image_device): the hand-off to a range-view network or de-noiser; `to_rows` brings its per-pixel
    prediction back to the rows as a keep mask for the next stage.
  * `nearest_keypoints(frames_or_result, centres, k)` gives every row the k nearest centres of its frame and their inverse-distance
    weights (NearestBatch; snowgpu_nearest_centres_device): pointnet2's three_nn, the way back from a KeypointBatch to the rows;
    `interpolate` and `nearest` carry per-keypoint features, or a keep decision, back to the rows.
  * `points_in_boxes(frames_or_result, boxes)` labels every row with the 3D box of its frame that contains it and counts the rows of
    every box (BoxLabelBatch; snowgpu_points_in_boxes_device): roiaware_pool3d's points_in_boxes_gpu and num_points_in_gt after the
    augmentation; `labels`, `keep_boxes` and `rows_in` are the point heads' targets, filter_by_min_points and a keep mask of the objects.
  * `nms(boxes, scores, iou_thresh, post_max=)` keeps the proposals of every frame by rotated NMS (NmsBatch; snowgpu_nms_device): pcdet's
    nms_gpu without its host sweep, its `boxes` the rois of `sample_keypoints(rois=)` as they stand; `boxes_iou(boxes_a, boxes_b)` is the
    rotated IoU matrix and the best partner of every box (IouBatch; snowgpu_boxes_iou_device): boxes_iou3d_gpu / boxes_iou_bev and the
    target layer's max_overlaps / gt_assignment.
  * `roi_point_pool(frames_or_result, rois, n_samples)` stores for every roi the first n_samples rows inside its slightly enlarged box,
    in row order and in the roi's own frame (RoiPointBatch; snowgpu_roi_point_pool_device): pcdet's roipoint_pool3d, the input of
    PointRCNN's refinement head; `rois` may be the NmsBatch as it stands, `gather` joins per-row features to the pooled rows.
  * `roi_voxel_pool(frames_or_result, rois, out_size, max_points, features)` cuts every slightly enlarged roi into out_size sub-voxels
    and max- / average-pools the features of the rows inside each, members in row order (RoiVoxelBatch; snowgpu_roi_voxel_pool_device):
    pcdet's roiaware_pool3d, the input of a Part-A2-style second stage; `max_features` / `avg_features` are the differentiable gathers.
  * `sample_rois(rois, gt_boxes, overlaps, step=...)` draws the roi_per_image rois of every frame that the second stage trains on --
    foreground without replacement, hard and easy background with replacement, seeded by (seed, step, frame) -- and their targets
    (RoiTargetBatch; snowgpu_sample_rois_device): the sampling of pcdet's ProposalTargetLayer between `boxes_iou(return_best=True)` and
    the two pooling stages, which take its `rois` as they stand.
  * `assign_anchors(anchors, anchor_class, gt_boxes, matched, unmatched)` labels every anchor of a first stage in every frame -- the class
    for a positive, 0 for background, -1 for ignored -- by the nearest axis-aligned BEV overlap per class, with the gt a positive regresses
    to (AnchorTargetBatch; snowgpu_assign_anchors_device): the assignment of pcdet's AxisAlignedTargetAssigner, fed the gts that
    `points_in_boxes(res, gt).keep_boxes(min_points)` left; `anchor_grid(...)` lays the anchors out as pcdet's AnchorGenerator does.
  * `assign_centers(gt_boxes, point_cloud_range, voxel_size, stride, feature_map_size=(W, H))` makes the targets of a centre-based first
    stage in every frame -- the class heatmaps as the maximum of the gts' Gaussians, and per head and slot the gt, its centre pixel, the
    fractional offset and the radius (CenterTargetBatch; snowgpu_assign_centers_device): the assignment of pcdet's CenterHead, fed the
    gts that `points_in_boxes(res, gt).keep_boxes(min_points)` left; `.target_boxes(gt_boxes)` gives the regression targets.
  * `paste_objects(frames, gt_boxes, bank, sample_groups, step=...)` pastes database objects into the ABSENT rows of a padded batch, in
    front of the snowfall stage -- per class as many as the frame lacks, drawn from an `ObjectBank` by (seed, step, frame), dropped where
    they overlap a gt or an earlier object, their boxes appended to the gts and the scene rows inside them cleared (PasteBatch;
    snowgpu_paste_objects_device): pcdet's DataBaseSampler; its `rows`, `keep` and `gt_boxes` feed `augment_batch(..., layout='aligned',
    keep=)` and every stage behind it.
  * `transform_scene(frames, gt_boxes, step=...)` is the geometric augmentation behind gt_sampling: world flip, rotation and scaling and,
    with `local=`, per-object translation, rotation and scaling with their collision test, on rows and gt boxes alike, drawn by (seed, step,
    frame) (SceneBatch; snowgpu_transform_scene_device).  Its place: BEHIND the weather stages and `range_image(ring=)`, which need rows in
    the sensor frame, IN FRONT of `voxelize`, the keypoint stages, `ball_query`, `points_in_boxes` for labels and `assign_anchors`.
  * `augment_wet_batch_aligned(frames, ...)` is the snowfall + wet-ground chain with that aligned result (AlignedWetResult: per-frame
    flags beside it; snowgpu_augment_wet_batch_device_aligned), `wet_ground_batch_aligned(frames, keep)` the wet-ground stage alone on rows
    and a keep mask from any earlier stage (snowgpu_wet_ground_batch_device_aligned).

What crosses the link per call: the frame offsets, the n_frames x n_lasers table ids and the planes (a few KB, cached by value: a
training loop that reshuffles `order` per frame uploads 64 int32 per frame).  PyTorch is plumbing here -- device memory and streams;
no arithmetic of the simulation happens in this file.

This module is the import path of all of it and holds the augmentation entries.  How a batch is read and a result handed back lives in
batch.py, the stages from `fov_keep` to `transform_scene` with their result classes in stages.py; every public name of both is re-exported here.
"""
from __future__ import annotations

import os
import random
from contextlib import contextmanager

import numpy as np

from . import _native
from .batch import (LANE_SLOT0, AlignedResult, AlignedWetResult, DeviceBatch, DeviceResult, _cuda_device, _keep_mask, _on_run_stream,  # noqa: F401
                    _resolve_input, _uploads, is_device_input)
from .stages import (CENTER_STATES, IOU_MODES, PASTE_STATES, SCENE_STATES, AnchorTargetBatch, BoxLabelBatch, CenterTargetBatch, IouBatch, KeypointBatch, NearestBatch, NeighbourBatch, NmsBatch, ObjectBank, PasteBatch, RangeImageBatch, RoiPointBatch, RoiTargetBatch, RoiVoxelBatch, SceneBatch, VoxelBatch,  # noqa: F401
                     _fov_mask, anchor_grid, assign_anchors, assign_centers, ball_query, boxes_iou, dror_keep, fov_keep, nearest_keypoints, nms, paste_objects, points_in_boxes, range_image, roi_point_pool,
                     roi_voxel_pool, sample_keypoints, sample_rois, transform_scene, voxelize)


@contextmanager
def _temporary_settings(ctx, calib=None, plane=None, wet_estimation=None, lines=None):
    """The settings of the context that one call sets and puts back; held under the engine's batch_lock.  calib: the camera crop of the
    result (simulation.py:536); plane: (method, seed, trials) of the device's plane estimate; wet_estimation: (method, seed);
    lines: n_frames x 4 fitted by the caller."""
    if calib is not None:
        ctx.set_fov(calib, (1024, 1920))
    if plane is not None:
        ctx.set_plane_method(plane[0], seed=plane[1], trials=plane[2], min_rows=5)
    if wet_estimation is not None and wet_estimation[0] != 'linear':
        ctx.set_wet_estimation(*wet_estimation)
    if lines is not None:
        ctx.set_wet_lines(lines)
    try:
        yield
    finally:
        if calib is not None:
            ctx.set_fov(None)
        if plane is not None and plane[0] != 'reference':
            ctx.set_plane_method('reference')
        if wet_estimation is not None and wet_estimation[0] != 'linear':
            ctx.set_wet_estimation('linear')
        if lines is not None:
            ctx.set_wet_lines(None)


WET_DEFAULTS = dict(water_height=0.001, pavement_depth=0.0012, noise_floor=0.7, power_factor=15, flat_earth=False, delta=0.5, replace=True)


def _plane_rows(planes, nf):
    """n_frames x 4 float64 (wx, wy, wz, h) from an n_frames x 4 array, per-frame (w, h) pairs, or ONE (w, h) pair for every frame."""
    if isinstance(planes, np.ndarray) and planes.shape == (nf, 4):
        return np.ascontiguousarray(planes, np.float64)
    if len(planes) == 2 and not isinstance(planes[1], (list, tuple)) and np.ndim(planes[1]) == 0:     # (two frames' pairs are not ONE pair)
        planes = [planes] * nf
    return np.asarray([[float(w[0]), float(w[1]), float(w[2]), float(h)] for w, h in planes], np.float64).reshape(nf, 4)


def table_ids_for(eng, n_frames, particle_file_prefix, root_path, particles, orders, shuffle):
    """n_frames x n_lasers int32 device table ids: channel c of frame f reads line orders[f][c] + 1 (simulation.py:78, :482-486)."""
    from .tools.snowfall import simulation as _sim
    nl = eng.n_lasers
    if orders is None:
        orders = np.empty((n_frames, nl), np.int64)
        for f in range(n_frames):
            order = list(range(nl))                                               # simulation.py:483
            if shuffle:
                random.shuffle(order)                                             # simulation.py:485-486: Python's global generator
            orders[f] = order
    else:
        orders = np.asarray([list(o)[:nl] for o in orders] if not isinstance(orders, np.ndarray) else orders[:, :nl], np.int64)
        if orders.shape != (n_frames, nl):
            raise ValueError("orders must be n_frames permutations of the laser lines")
    if isinstance(particles, str):
        if particles not in ('device', 'missing'):
            raise ValueError("particles must be a sequence of tables, 'device' or 'missing'")
        ids = _sim._LazyFileIds(eng, particle_file_prefix, root_path, sample='all' if particles == 'device' else 'missing')
    else:
        ids = _sim._ArrayIds(eng, particles) if particles is not None else _sim._LazyFileIds(eng, particle_file_prefix, root_path)
    return np.ascontiguousarray(ids[orders.reshape(-1)].reshape(n_frames, nl), np.int32)


def _prefix_list(particle_file_prefix, n_frames):
    """None for ONE prefix, else the list of n_frames prefixes."""
    if isinstance(particle_file_prefix, (str, bytes, os.PathLike)) or particle_file_prefix is None:
        return None
    prefixes = list(particle_file_prefix)
    if len(prefixes) != n_frames:
        raise ValueError(f"particle_file_prefix as a sequence needs one prefix per frame: {len(prefixes)} given for {n_frames} frames")
    return prefixes


def table_ids_per_frame(eng, prefixes, root_path, particles, orders, shuffle):
    """table_ids_for with one prefix per frame (particles: None, 'device' or 'missing'): frames of one prefix share its resolved lines."""
    if particles is not None and not isinstance(particles, str):
        raise ValueError("a sequence of prefixes names table files (or 'device' / 'missing' tables): caller-owned arrays have no prefix")
    nf = len(prefixes)
    if orders is not None and len(orders) != nf:
        raise ValueError("orders must be n_frames permutations of the laser lines")
    out = np.empty((nf, eng.n_lasers), np.int32)
    for f, prefix in enumerate(prefixes):
        out[f] = table_ids_for(eng, 1, prefix, root_path, particles, None if orders is None else [orders[f]], shuffle)[0]
    return out


def weather_records(n_frames, snow=True, wet=True, water_height=0.001, pavement_depth=0.0012, noise_floor=0.7, power_factor=15, delta=0.5,
                    device=None):
    """The per-frame weather records of augment_wet_batch_aligned(weather=...): an n_frames x 8 float64 CUDA tensor
    [snow, wet, water_height, pavement_depth, wet noise_floor, power_factor, delta, 0] (include/snowgpu.h).  Every argument is a scalar
    (all frames alike), a sequence of n_frames values or a tensor of them; snow and wet are truth values (the record holds 0.0 or 1.0)."""
    import torch
    nf = int(n_frames)
    dev = _cuda_device(torch, device)
    rec = torch.zeros((nf, 8), dtype=torch.float64, device=dev)
    for col, (name, v) in enumerate((("snow", snow), ("wet", wet), ("water_height", water_height), ("pavement_depth", pavement_depth),
                                     ("noise_floor", noise_floor), ("power_factor", power_factor), ("delta", delta))):
        if torch.is_tensor(v):
            v = v.to(device=dev)
        else:
            v = torch.as_tensor(np.asarray(v), device=dev)
        if col < 2:
            v = (v != 0)
        v = v.to(torch.float64)
        if v.dim() > 1 or (v.dim() == 1 and v.shape[0] != nf):
            raise ValueError(f"weather_records: {name} must be a scalar or hold one value per frame ({nf})")
        rec[:, col] = v
    return rec


WEATHER_PER_FRAME = ("water_height", "pavement_depth", "noise_floor", "power_factor", "delta")


class WeatherPlan:
    """Which weather every frame of a training batch gets, drawn ON THE DEVICE (snowgpu_draw_weather_device): the snow and the wet gate
    with probabilities p_snow / p_wet, one of `prefixes` (a snowfall setting: one table per laser line), the order of its tables over
    the lasers (simulation.py:482-486), one of water_heights and one of pavement_depths; noise_floor, power_factor and delta are shared.

        plan = WeatherPlan(prefixes, root_path, p_snow=0.5, p_wet=0.5, water_heights=(0.0005, 0.001), pavement_depths=(0.0012,))
        table_ids, weather = plan.draw(n_frames)
        augment_wet_batch_aligned(frames, None, bd, table_ids=table_ids, weather=weather, ...)
        plan.step += 1

    prefixes   the table sets (at most 64); particles: None (files under root_path), 'device' / 'missing' (sampled on the device, as for
               table_ids_for) or one sequence of n_lasers arrays per prefix.  Every line of every set is resolved to a resident table here.
    step       an int64 tensor of one element ON THE DEVICE: the draw reads it there, so a captured graph that holds draw(), the
               augmentation and `plan.step += 1` draws anew on every replay.  Draws are Philox4x32-10 keyed by (seed; step, frame): the
               same plan, seed and step give the same batch on every run; parity with the reference's random.shuffle is distributional.
    set_ids    n_sets x n_lasers int32 device tensor of table ids."""

    def __init__(self, prefixes, root_path=None, particles=None, p_snow=0.5, p_wet=0.5, water_heights=(0.001,), pavement_depths=(0.0012,),
                 noise_floor=0.7, power_factor=15, delta=0.5, shuffle=True, seed=0, device=None, slot=0):
        import torch
        from . import engine as _engine
        prefixes = [prefixes] if isinstance(prefixes, (str, bytes, os.PathLike)) else list(prefixes)
        if not prefixes:
            raise ValueError("WeatherPlan needs at least one prefix (one table set)")
        self.device = _cuda_device(torch, device)
        self.eng = _engine.get_engine(self.device.index, slot)
        nl = self.eng.n_lasers
        if particles is not None and not isinstance(particles, str) and len(particles) != len(prefixes):
            raise ValueError("particles as arrays needs one sequence of tables per prefix")
        ident = [list(range(nl))]
        sets = [table_ids_for(self.eng, 1, pf, root_path, particles if particles is None or isinstance(particles, str) else particles[i], ident, False)[0]
                for i, pf in enumerate(prefixes)]
        self.prefixes = prefixes
        self.set_ids = torch.from_numpy(np.ascontiguousarray(sets, np.int32)).to(self.device)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.seed = int(seed)
        self.struct = _native.weather_plan_struct(p_snow, p_wet, water_heights, pavement_depths, noise_floor, power_factor, delta, shuffle)

    def draw(self, n_frames, out=None):
        """(table_ids: n_frames x n_lasers int32, weather: n_frames x 8 float64) for the plan's current step, launched on torch's current
        stream; out: an earlier pair to write into (static addresses for a captured graph)."""
        import torch
        nf, nl = int(n_frames), int(self.set_ids.shape[1])
        if out is None:
            out = (torch.empty((nf, nl), dtype=torch.int32, device=self.device), torch.empty((nf, 8), dtype=torch.float64, device=self.device))
        tids, weather = out
        if tuple(tids.shape) != (nf, nl) or tids.dtype != torch.int32 or tuple(weather.shape) != (nf, 8) or weather.dtype != torch.float64 or \
                not tids.is_contiguous() or not weather.is_contiguous() or tids.device != self.device or weather.device != self.device:
            raise ValueError("out must be (n_frames x n_lasers int32, n_frames x 8 float64) contiguous tensors on the plan's device")
        with torch.cuda.device(self.device), _on_run_stream(torch, self.eng, self.device) as (_, run):
            self.eng.ctx.draw_weather_device(nf, nl, int(self.set_ids.shape[0]), self.set_ids.data_ptr(), self.struct, self.seed,
                                             self.step.data_ptr(), tids.data_ptr(), weather.data_ptr(), run.cuda_stream)
        return tids, weather


def augment_batch(frames, particle_file_prefix, beam_divergence, shuffle=True, noise_floor=0.7, root_path=None, *, planes=None,
                  orders=None, particles=None, thr_polys=None, device=None, return_src=False, slot=0, calib=None, pre_crop=False,
                  q8='first', plane_method='reference', plane_seed=0, plane_trials=1000, sync=True, wet=None, out=None, lane=None,
                  layout='compact', in_place=False, keep=None, **_ignored):
    """augment_batch() of tools/snowfall/simulation.py for torch CUDA tensors (see that docstring for the shared arguments).

    frames   a list of N_i x 5 CUDA tensors (concatenated on the device), an F x N x 5 tensor, one N x 5 tensor, or a DeviceBatch
             (read in place).  float32 or float64.
    sync     True: wait, check, return [(stats, aug_pc)] with aug_pc device tensors.  False: return a DeviceResult immediately
             (asynchronous on torch's current stream of the device).
    wet      optional dict of ground_water_augmentation()'s keyword arguments (water_height, pavement_depth, noise_floor,
             power_factor, flat_earth, delta, replace, plane): the wet-ground model runs behind the snowfall on the same stream
             (snowgpu_augment_wet_batch_device); the result rows are float64 then (wet_ground/augmentation.py:150).
    out      optional DeviceResult of an earlier call with the same shapes whose tensors are reused (no allocation at all).
    lane     None (default): the call is part of torch's current stream -- it starts when that stream gets there and whatever the caller
             queues behind it waits for it.  An integer k: the call runs on compute lane k -- an engine context of its own (streams,
             scratch, tables) with a torch stream of its own -- which waits for what the caller's stream holds NOW (the inputs) and
             nothing waits for it: the caller's stream goes on, a call on another lane may run beside this one (the memory-bound sort and
             compaction of one batch beside the latency-bound per-beam kernels of the other), and the result is claimed through the
             DeviceResult: .wait() (host), .join() (torch's current stream waits, the host does not).  Keep as many results alive as
             lanes in flight; `sync=True` with a lane is a plain synchronous call on that lane.  A lane's context runs every kernel of a
             batch on ONE stream (snowgpu_set_serial) of the context's own (snowgpu_lane_stream); lanes k, k + 1, k + 2 get streams of
             different priorities -- the HIP runtime keeps a queue pool per priority, so they never share a hardware queue (streams of one
             priority may, and then run one after the other).  Measured per 256-sweep batch: two lanes 3.8 ms against 4.0 for one batch at
             a time; with GPU_MAX_HW_QUEUES=32 in the environment before the process first touches the GPU all lanes run at one priority
             on queues of their own: three lanes 3.66 ms (profiles/r06_lanes_ab.txt).  Lanes are engine contexts of their own (slot
             LANE_SLOT0 + k): a plain call never runs on a lane's context.
    layout   'compact' (default): the reference's return value, as above.  'aligned': nothing is compacted -- the result's `rows` hold
             the output row of every input row at the input's own index and `keep` (torch.bool) says which of them the reference
             returns (snowgpu_augment_batch_device_aligned).  sync=False returns an AlignedResult (rows, keep, counts, stats, status,
             offsets; wait() / join() / frames() as a DeviceResult), sync=True its frames(): [(stats, rows_f, keep_f)], views.
             rows_f[keep_f] are the compact rows in input order.  `out=` takes an earlier AlignedResult; lane=, calib=, planes=,
             thr_polys=, orders=, particles=, plane_method= work as for the compact layout.  Frames with more than five columns:
             the result has five, and the caller's further columns are ALREADY aligned with it, row for row -- nothing is gathered.
             Not with wet= (augment_wet_batch_aligned is the aligned chain) and not with return_src (row i IS input row i).
    in_place with layout='aligned': the result's `rows` IS the input tensor, overwritten by its augmented form.  The input must be
             read where it lies -- a DeviceBatch, one contiguous N x 5 tensor or an F x N x 5 tensor; a list that would have to be
             concatenated raises ValueError (the result would land in a temporary).
    keep     with layout='aligned': an INPUT keep mask -- a torch.bool (or uint8) CUDA tensor with one element per row of the batch, an
             F x N tensor, or a list of per-frame tensors; False = the row is not there.  With P the present rows of a frame in input
             order, rows_f[P] / keep_f[P] and the statistics are, byte for byte, those of the call on frame[P]; an absent row comes
             back as it came with keep False and is never looked at (NaNs, far ranges, channels that are no laser do no harm there).
             Nothing is compacted as the caller sees it and nothing is read on the host (snowgpu_augment_batch_device_aligned_masked):
             the call stays capturable.  A padded F x Nmax x 5 batch: keep = torch.arange(Nmax, device=...) < lengths[:, None].
             Not with the compact layout (ValueError), not with a caller's permutation.
    pre_crop with layout='aligned' and calib: the frames are cropped to the camera's view BEFORE they are augmented (precompute.py:96-104)
             -- as a keep mask built on the device (fov_keep), ANDed with `keep` if given; the camera crop of the result stays set as
             well, as in the host entry.  The compact layout raises: its pre-crop is a step of the host entry.
    """
    import torch
    if q8 != 'first':
        raise ValueError("q8='numpy' selects the histogram minima with the HOST's NumPy: it needs host arrays, not CUDA tensors")
    if calib is not None and pre_crop and layout != 'aligned':
        raise ValueError("pre_crop is a step of the host entry (precompute.py:96-99); crop the tensors before the call, or use "
                         "layout='aligned', which crops by a keep mask on the device")
    if keep is not None and layout != 'aligned':
        raise ValueError("keep= is an input mask of layout='aligned': the compact layout returns compacted frames; index them before the call")
    if plane_method not in _native.PLANE_METHODS:
        raise ValueError("plane_method must be 'reference', 'lsq' or 'ransac'")
    if layout not in ('compact', 'aligned'):
        raise ValueError("layout must be 'compact' or 'aligned'")
    aligned = layout == 'aligned'
    if in_place and not aligned:
        raise ValueError("in_place=True needs layout='aligned': compacted rows do not lie where their input rows lay")
    if aligned and wet is not None:
        raise ValueError("wet= with layout='aligned': layout='aligned' promises the compact call's bytes, and the aligned wet-ground stage "
                         "sums over other tiles; call augment_wet_batch_aligned for the aligned chain, or use the compact layout")
    if aligned and return_src:
        raise ValueError("return_src with layout='aligned': there is no src, row i of the result is input row i")
    rows, offsets, extras, eng = _resolve_input(torch, frames, in_place, device, slot, lane)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    if nf == 0:
        return []
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    code = 0 if rows.dtype == torch.float32 else 1
    max_rows = int(np.diff(offsets).max())
    up = _uploads(eng)
    wet_plane = None
    if wet is not None:
        wet = dict(wet)
        wet_plane = wet.pop("plane", None)
    with torch.cuda.device(dev):
        tids = table_ids_for(eng, nf, particle_file_prefix, root_path, particles, orders, shuffle)
        if n == 0:                                   # nothing to simulate (the C ABI wants non-null buffers): empty frames come back empty
            zero = (np.int64(0), np.int64(0), 0)
            empty = [(zero, rows[:0], torch.empty(0, dtype=torch.int32, device=dev)) if return_src else (zero, rows[:0]) for _ in range(nf)]
            z = lambda *shape, dt=torch.int64: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
            if aligned:
                if sync:
                    return [(zero, rows[:0], z(0, dt=torch.bool)) for _ in range(nf)]
                return AlignedResult(eng.ctx, rows[:0], z(0, dt=torch.bool), z(nf), z(nf, 3), z(8, dt=torch.int32), offsets, torch.cuda.current_stream(dev))
            if sync:
                return empty
            return DeviceResult(eng.ctx, rows[:0], z(0, dt=torch.int32), z(nf), z(nf, 3), z(8, dt=torch.int32), offsets, torch.cuda.current_stream(dev))
        out_dt = torch.float64 if wet is not None else rows.dtype
        o_src = o_keep = None
        if aligned:
            o_rows, o_keep, o_cnt, o_st, o_status, o_flags = _aligned_outputs(torch, out, AlignedResult, rows, n, nf, in_place)
        elif out is not None and not isinstance(out, AlignedResult) and out.rows.shape[0] >= n and out.rows.dtype == out_dt and out.rows.device == dev and out.counts.shape[0] == nf:
            o_rows, o_src, o_cnt, o_st, o_status, o_flags = out.rows, out.src, out.counts, out.stats, out.status, out.flags
        else:
            o_rows = torch.empty((n, 5), dtype=out_dt, device=dev)
            o_src = torch.empty(n, dtype=torch.int32, device=dev)
            o_cnt = torch.empty(nf, dtype=torch.int64, device=dev)
            o_st = torch.empty((nf, 3), dtype=torch.int64, device=dev)
            o_status = torch.empty(8, dtype=torch.int32, device=dev)
            o_flags = None
        if wet is not None and o_flags is None:
            o_flags = torch.empty(nf, dtype=torch.int32, device=dev)
        # calculate_plane (simulation.py:449; augmentation.py:41 for the wet stage) on the device where the call brings no plane
        estimated = (thr_polys is None and planes is None) or (wet is not None and wet_plane is None)
        used = (rows, o_rows, o_src, o_keep, o_cnt, o_st, o_status, o_flags, keep)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        with eng.batch_lock, _temporary_settings(eng.ctx, calib=calib, plane=(plane_method, plane_seed, plane_trials) if estimated else None), \
                _on_run_stream(torch, eng, dev, lane, used) as (stream, run):
            d_off = up.get(torch, dev, offsets, run)
            d_tids = up.get(torch, dev, tids, run)
            d_poly = d_plane = None
            if thr_polys is not None:
                d_poly = up.get(torch, dev, np.ascontiguousarray(thr_polys, np.float64).reshape(nf, 3), run)
            elif planes is not None:
                d_plane = up.get(torch, dev, _plane_rows(planes, nf), run)
            d_wet_plane = None if wet_plane is None else up.get(torch, dev, _plane_rows(wet_plane, nf), run)
            if calib is not None and pre_crop:                                      # precompute.py:96-99, as a mask
                keep = _fov_mask(torch, eng, rows[:n], calib, (1024, 1920), keep, run)
                if lane is not None:
                    keep.record_stream(run)
            if aligned and keep is not None:
                eng.ctx.augment_batch_device_aligned_masked(nf, n, max_rows, d_off.data_ptr(), rows.data_ptr(), code, d_tids.data_ptr(),
                                                            float(beam_divergence), ptr(d_poly), ptr(d_plane), float(noise_floor), 0, keep.data_ptr(),
                                                            o_rows.data_ptr(), o_keep.data_ptr(), o_cnt.data_ptr(), o_st.data_ptr(), 0,
                                                            o_status.data_ptr(), run.cuda_stream)
            elif aligned:
                eng.ctx.augment_batch_device_aligned(nf, n, max_rows, d_off.data_ptr(), rows.data_ptr(), code, d_tids.data_ptr(),
                                                     float(beam_divergence), ptr(d_poly), ptr(d_plane), float(noise_floor), 0, o_rows.data_ptr(),
                                                     o_keep.data_ptr(), o_cnt.data_ptr(), o_st.data_ptr(), 0, o_status.data_ptr(), run.cuda_stream)
            elif wet is None:
                eng.ctx.augment_batch_device(nf, n, max_rows, d_off.data_ptr(), rows.data_ptr(), code, d_tids.data_ptr(),
                                             float(beam_divergence), ptr(d_poly), ptr(d_plane), float(noise_floor), 0, o_rows.data_ptr(),
                                             o_src.data_ptr(), o_cnt.data_ptr(), o_st.data_ptr(), 0, o_status.data_ptr(), run.cuda_stream)
            else:                                   # (not _wet_arguments: the compact chain fits 'linear' only and knows no poly_seed)
                unknown = set(wet) - set(WET_DEFAULTS) - {"estimation_method", "debug"}
                if unknown:
                    raise TypeError(f"unknown wet-ground arguments: {sorted(unknown)}")
                if wet.get("estimation_method", "linear") != "linear":
                    raise ValueError("the fused snowfall + wet-ground call fits estimation_method='linear'")
                w = dict(WET_DEFAULTS, **{k: v for k, v in wet.items() if k in WET_DEFAULTS})
                eng.ctx.augment_wet_batch_device(nf, n, max_rows, d_off.data_ptr(), rows.data_ptr(), code, d_tids.data_ptr(),
                                                 float(beam_divergence), ptr(d_poly), ptr(d_plane), float(noise_floor), 0, ptr(d_wet_plane),
                                                 w["water_height"], w["pavement_depth"], w["noise_floor"], w["power_factor"],
                                                 w["flat_earth"], w["delta"], w["replace"], o_rows.data_ptr(), o_src.data_ptr(),
                                                 o_cnt.data_ptr(), o_st.data_ptr(), o_flags.data_ptr(), o_status.data_ptr(), run.cuda_stream)
    if aligned:
        res = AlignedResult(eng.ctx, o_rows, o_keep, o_cnt, o_st, o_status, offsets, stream if lane is None else run, keep=(rows, d_off, d_tids, d_poly, d_plane, keep))
        return res.frames() if sync else res
    res = DeviceResult(eng.ctx, o_rows, o_src, o_cnt, o_st, o_status, offsets, stream if lane is None else run, flags=o_flags, keep=(rows, d_off, d_tids, d_poly, d_plane, d_wet_plane))
    if not sync:
        return res
    from .tools.snowfall.simulation import _raise_like_reference
    try:
        per_frame = res.frames(return_src=True)
    except _native.SnowGPUError as err:
        _raise_like_reference(err)
    results = []
    for i, (st, aug, src) in enumerate(per_frame):
        if extras is not None and extras[i].shape[1] > 5:        # further columns ride through (simulation.py:447, :508-523)
            aug = torch.cat((aug, extras[i][src.long(), 5:].to(aug.dtype)), dim=1)
        results.append((st, aug, src) if return_src else (st, aug))
    return results


def _wet_arguments(wet):
    """(parameters, plane or None, estimation method, RANSAC seed) from ground_water_augmentation()'s keyword arguments."""
    wet = dict(wet or {})
    plane = wet.pop("plane", None)
    method = wet.pop("estimation_method", "linear")
    seed = wet.pop("poly_seed", 0)
    wet.pop("debug", None)
    unknown = set(wet) - set(WET_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown wet-ground arguments: {sorted(unknown)}")
    if method not in _native.WET_ESTIMATION:
        raise ValueError("estimation_method must be 'linear' or 'poly' (augmentation.py:215, :223)")
    return dict(WET_DEFAULTS, **wet), plane, method, seed


def _aligned_outputs(torch, out, kind, rows, n, nf, in_place, with_stats=True):
    """(rows, keep, counts, stats, status, flags) tensors of an aligned call: those of `out` (a `kind` -- AlignedResult or AlignedWetResult --
    of the same shapes) or new ones; keep holds one byte per flag, 0 / 1: what the kernels write.  flags: None for an AlignedResult."""
    dev, wet = rows.device, kind is AlignedWetResult
    if isinstance(out, kind) and out.keep.shape[0] == n and out.keep.device == dev and out.counts.shape[0] == nf and \
            (out.stats is not None) == with_stats and \
            (in_place or (out.rows.shape[0] == n and out.rows.dtype == rows.dtype and out.rows.data_ptr() != rows.data_ptr())):
        return (rows if in_place else out.rows), out.keep, out.counts, out.stats, out.status, (out.flags if wet else None)
    return (rows if in_place else torch.empty((n, 5), dtype=rows.dtype, device=dev), torch.empty(n, dtype=torch.bool, device=dev),
            torch.empty(nf, dtype=torch.int64, device=dev), torch.empty((nf, 3), dtype=torch.int64, device=dev) if with_stats else None,
            torch.empty(8, dtype=torch.int32, device=dev), torch.empty(nf, dtype=torch.int32, device=dev) if wet else None)


def _empty_aligned_wet(torch, eng, rows, nf, offsets, with_stats, sync):
    dev = rows.device
    z = lambda *shape, dt=torch.int64: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    res = AlignedWetResult(eng.ctx, rows[:0], z(0, dt=torch.bool), z(nf), z(nf, 3) if with_stats else None, z(8, dt=torch.int32), offsets,
                           torch.cuda.current_stream(dev), torch.ones(nf, dtype=torch.int32, device=dev))
    return res.frames() if sync else res


def wet_ground_batch_aligned(frames, keep=None, *, plane=None, water_height=0.001, pavement_depth=0.0012, noise_floor=0.7, power_factor=15,
                             flat_earth=False, delta=0.5, replace=True, estimation_method='linear', poly_seed=0, lines=None, device=None,
                             slot=0, in_place=False, sync=True, out=None):
    """ground_water_augmentation() (tools/wet_ground/augmentation.py:25-161) for torch CUDA tensors with the ALIGNED result
    (snowgpu_wet_ground_batch_device_aligned): row i of the result is the output row of input row i, `keep` says which rows the reference
    returns -- the wet-ground model never moves a point, so nothing needs compacting.

    frames   as augment_batch: a list of N_i x 5 CUDA tensors, an F x N x 5 tensor, one N x 5 tensor or a DeviceBatch; float32 or float64.
    keep     optional torch.bool (or uint8) tensor, one element per row of the batch: False = the row is not there (an earlier stage
             removed it -- AlignedResult.keep of augment_batch(layout='aligned')).  The estimator skips such rows and they come back as
             they came.  None: every row is present.
    plane    (w, h) for every frame, per-frame pairs or an n_frames x 4 array; None: the flat-earth plane the reference returns today.
    lines    optional n_frames x 4 (p slope, p intercept, noise-line slope, intercept) fitted by the caller instead of the device's fit.
    in_place the result's `rows` IS the input tensor (which must be read where it lies, as for augment_batch) and `keep` the tensor passed
             as keep (a new one when keep is None).
    sync     True: wait, check, return [(None, rows_f, keep_f, flag_f)] (no statistics: the wet-ground model has none); False: an
             AlignedWetResult at once, asynchronous on torch's current stream.  out: an earlier AlignedWetResult whose tensors are reused.
    Rows come back in the INPUT's dtype -- a float32 row's new intensity is the float64 result rounded once --, unlike the compact entries,
    which return float64 (augmentation.py:150).  flag_f = 1: fewer than 1000 present ground rows, the frame came back as it was.  NumPy
    input raises ValueError: the aligned layout is a result layout of the torch-tensor boundary."""
    if not is_device_input(frames):
        raise ValueError("wet_ground_batch_aligned: the aligned layout is a result layout of the torch-tensor boundary (CUDA tensors); "
                         "host arrays get the reference's compacted return value from ground_water_augmentation")
    import torch
    w, _, method, seed = _wet_arguments(dict(water_height=water_height, pavement_depth=pavement_depth, noise_floor=noise_floor,
                                             power_factor=power_factor, flat_earth=flat_earth, delta=delta, replace=replace,
                                             estimation_method=estimation_method, poly_seed=poly_seed))
    rows, offsets, _, eng = _resolve_input(torch, frames, in_place, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    if nf == 0:
        return []
    if keep is not None:
        if keep.device != dev or keep.dim() != 1 or keep.shape[0] != n or keep.dtype not in (torch.bool, torch.uint8) or not keep.is_contiguous():
            raise ValueError("keep must be a contiguous torch.bool (or uint8) CUDA tensor with one element per row of the batch")
        if keep.dtype == torch.uint8:
            keep = keep.view(torch.bool)
    if n == 0:
        return _empty_aligned_wet(torch, eng, rows, nf, offsets, False, sync)
    code = 0 if rows.dtype == torch.float32 else 1
    up = _uploads(eng)
    if lines is not None:
        lines = np.ascontiguousarray(lines, np.float64).reshape(nf, 4)
    with torch.cuda.device(dev):
        o_rows, o_keep, o_cnt, _, o_status, o_flags = _aligned_outputs(torch, out, AlignedWetResult, rows, n, nf, in_place, False)
        if in_place and keep is not None:
            o_keep = keep
        with eng.batch_lock, _temporary_settings(eng.ctx, wet_estimation=(method, seed), lines=lines), _on_run_stream(torch, eng, dev) as (stream, run):
            d_off = up.get(torch, dev, offsets, run)
            d_plane = None if plane is None else up.get(torch, dev, _plane_rows(plane, nf), run)
            eng.ctx.wet_ground_batch_device_aligned(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr(), code,
                                                    0 if keep is None else keep.data_ptr(), 0 if d_plane is None else d_plane.data_ptr(),
                                                    w["water_height"], w["pavement_depth"], w["noise_floor"], w["power_factor"],
                                                    w["flat_earth"], w["delta"], w["replace"], o_rows.data_ptr(), o_keep.data_ptr(),
                                                    o_cnt.data_ptr(), o_flags.data_ptr(), o_status.data_ptr(), run.cuda_stream)
    res = AlignedWetResult(eng.ctx, o_rows, o_keep, o_cnt, None, o_status, offsets, stream, o_flags, keep=(rows, keep, d_off, d_plane))
    return res.frames() if sync else res


def augment_wet_batch_aligned(frames, particle_file_prefix, beam_divergence, shuffle=True, noise_floor=0.7, root_path=None, *, wet=None,
                              planes=None, orders=None, particles=None, thr_polys=None, device=None, slot=0, calib=None, sync=True,
                              out=None, lane=None, in_place=False, keep=None, pre_crop=False, weather=None, table_ids=None, **_ignored):
    """augment() followed by ground_water_augmentation() on its output (pointcloud_viewer.py:2807-2821) for torch CUDA tensors with the
    ALIGNED result (snowgpu_augment_wet_batch_device_aligned): the snowfall stage finishes into rows in the input's order plus a keep
    mask, and the wet-ground stage rewrites those two arrays in place, skipping the rows the snowfall stage removed.  No compaction, a
    result of static shape in the input's dtype, nothing read on the host: the form a training step wants.

    wet       dict of ground_water_augmentation()'s keyword arguments (water_height, pavement_depth, noise_floor, power_factor, flat_earth,
              delta, replace, plane, estimation_method, poly_seed); plane=None: the flat-earth plane the reference returns today.
    planes, thr_polys, orders, particles, calib, in_place, sync, out (an earlier AlignedWetResult), lane: as augment_batch(layout='aligned').
    keep, pre_crop  as augment_batch(layout='aligned'): an input keep mask for the snowfall stage (and the camera's view as one).  The
              result equals the masked snowfall call followed by wet_ground_batch_aligned(rows, keep) on its result.
    weather   an F x 8 float64 CUDA tensor of per-frame weather records (weather_records, WeatherPlan.draw): the gates `snow` and `wet`
              and the frame's water_height, pavement_depth, noise_floor, power_factor and delta, read on the device
              (snowgpu_augment_weather_batch_device_aligned).  A frame with both gates off comes back bit for bit, one with the snow gate
              off as wet_ground_batch_aligned returns it, one with the wet gate off as the aligned snowfall call does, with flag_f = 2.
              `wet` may then carry only flat_earth, replace, plane, estimation_method and poly_seed; a per-frame field raises ValueError.
    table_ids an F x n_lasers int32 CUDA tensor of table ids used as it is (WeatherPlan.draw): no host shuffle, no upload; orders= or
              particles= beside it raises ValueError.
    particle_file_prefix  may also be a sequence of F prefixes: every frame reads its own table set (ids built on the host).
    Returns an AlignedWetResult (sync=False) or its frames(): [(stats, rows_f, keep_f, flag_f)] -- stats the snowfall statistics,
    keep_f true where the CHAIN returns the row, flag_f = 1 where the wet stage found fewer than 1000 present ground rows and left the
    frame as the snowfall stage made it.

    Why this is a function of its own and not augment_batch(layout='aligned', wet=...): layout='aligned' promises the bytes of the compact
    call of the same arguments, in input order.  The wet-ground estimate is a set of sums over 1024-row tiles, and here the tiles are those
    of the input's rows with the removed ones skipped, not those of the compacted snowfall rows -- so the fitted power line, and with it
    the intensities, differ from the compact fused call's in their last bits; float32 rows also stay float32 here, where the compact
    chain returns float64.  NumPy input raises ValueError, as for the aligned layout."""
    if not is_device_input(frames):
        raise ValueError("augment_wet_batch_aligned: the aligned layout is a result layout of the torch-tensor boundary (CUDA tensors); "
                         "host arrays get the reference's compacted return value from augment_batch / ground_water_augmentation")
    import torch
    if weather is not None and wet is not None and set(wet) & set(WEATHER_PER_FRAME):
        raise ValueError(f"with weather= the per-frame fields {sorted(set(wet) & set(WEATHER_PER_FRAME))} come from the weather records, not from wet=")
    if table_ids is not None and (orders is not None or particles is not None):
        raise ValueError("table_ids= are used as they are: orders= and particles= have nothing to act on")
    w, wet_plane, method, seed = _wet_arguments(wet)
    rows, offsets, _, eng = _resolve_input(torch, frames, in_place, device, slot, lane)
    dev = rows.device
    for name, t, shape, dt in (("weather", weather, (len(offsets) - 1, 8), torch.float64), ("table_ids", table_ids, (len(offsets) - 1, eng.n_lasers), torch.int32)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.device == dev and tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {shape[0]} x {shape[1]} {dt} CUDA tensor on the device of the rows")
    prefixes = None if table_ids is not None else _prefix_list(particle_file_prefix, len(offsets) - 1)
    nf, n = len(offsets) - 1, int(offsets[-1])
    if nf == 0:
        return []
    if n == 0:
        res = _empty_aligned_wet(torch, eng, rows, nf, offsets, True, False)
        if weather is not None:                     # (no row anywhere: "not asked" where the wet gate is off)
            res.flags = torch.where(weather[:, 1] == 0, 2, 1).to(torch.int32)
        return res.frames() if sync else res
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    code = 0 if rows.dtype == torch.float32 else 1
    up = _uploads(eng)
    with torch.cuda.device(dev):
        if table_ids is None:
            tids = table_ids_for(eng, nf, particle_file_prefix, root_path, particles, orders, shuffle) if prefixes is None else \
                table_ids_per_frame(eng, prefixes, root_path, particles, orders, shuffle)
        o_rows, o_keep, o_cnt, o_st, o_status, o_flags = _aligned_outputs(torch, out, AlignedWetResult, rows, n, nf, in_place)
        used = (rows, o_rows, o_keep, o_cnt, o_st, o_status, o_flags, keep, weather, table_ids)
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        with eng.batch_lock, _temporary_settings(eng.ctx, calib=calib, wet_estimation=(method, seed)), \
                _on_run_stream(torch, eng, dev, lane, used) as (stream, run):
            d_off = up.get(torch, dev, offsets, run)
            d_tids = up.get(torch, dev, tids, run) if table_ids is None else table_ids
            d_poly = d_plane = None
            if thr_polys is not None:
                d_poly = up.get(torch, dev, np.ascontiguousarray(thr_polys, np.float64).reshape(nf, 3), run)
            elif planes is not None:
                d_plane = up.get(torch, dev, _plane_rows(planes, nf), run)
            d_wet_plane = None if wet_plane is None else up.get(torch, dev, _plane_rows(wet_plane, nf), run)
            if calib is not None and pre_crop:                                      # precompute.py:96-99, as a mask
                keep = _fov_mask(torch, eng, rows[:n], calib, (1024, 1920), keep, run)
                if lane is not None:
                    keep.record_stream(run)
            snow = (nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr(), code, d_tids.data_ptr(), float(beam_divergence), ptr(d_poly),
                    ptr(d_plane), float(noise_floor), 0, ptr(keep), o_rows.data_ptr(), o_keep.data_ptr(), o_cnt.data_ptr(), o_st.data_ptr(), 0,
                    o_status.data_ptr(), run.cuda_stream, ptr(d_wet_plane))
            if weather is not None:
                eng.ctx.augment_weather_batch_device_aligned(*snow, weather.data_ptr(), w["flat_earth"], w["replace"], o_flags.data_ptr())
            else:
                eng.ctx.augment_wet_batch_device_aligned_masked(*snow, w["water_height"], w["pavement_depth"], w["noise_floor"], w["power_factor"],
                                                                w["flat_earth"], w["delta"], w["replace"], o_flags.data_ptr())
    res = AlignedWetResult(eng.ctx, o_rows, o_keep, o_cnt, o_st, o_status, offsets, stream if lane is None else run, o_flags,
                           keep=(rows, d_off, d_tids, d_poly, d_plane, d_wet_plane, keep, weather))
    return res.frames() if sync else res
