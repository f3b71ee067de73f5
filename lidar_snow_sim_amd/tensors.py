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
  * `augment_wet_batch_aligned(frames, ...)` is the snowfall + wet-ground chain with that aligned result (AlignedWetResult: per-frame
    flags beside it; snowgpu_augment_wet_batch_device_aligned), `wet_ground_batch_aligned(frames, keep)` the wet-ground stage alone on rows
    and a keep mask from any earlier stage (snowgpu_wet_ground_batch_device_aligned).

What crosses the link per call: the frame offsets, the n_frames x n_lasers table ids and the planes (a few KB, cached by value: a
training loop that reshuffles `order` per frame uploads 64 int32 per frame).  PyTorch is plumbing here -- device memory and streams;
no arithmetic of the simulation happens in this file.
"""
from __future__ import annotations

import math
import os
import random
from collections import OrderedDict
from contextlib import contextmanager

import numpy as np

from . import _native


LANE_SLOT0 = 1000           # compute lane k is engine slot LANE_SLOT0 + k: lanes never share a context with plain calls (slot=)


def is_device_input(frames) -> bool:
    """True for a torch CUDA tensor, a DeviceBatch, or a non-empty sequence whose first element is a torch CUDA tensor."""
    if isinstance(frames, DeviceBatch):
        return True
    t = frames
    if isinstance(frames, (list, tuple)):
        if not frames:
            return False
        t = frames[0]
    return type(t).__module__.startswith("torch") and bool(getattr(t, "is_cuda", False))


class DeviceBatch:
    """Frames that lie back to back in ONE N_total x 5 CUDA tensor, with their (host) offsets -- the device twin of FlatBatch.
    `frame_rows=n`: every frame has n rows (a stack of sweeps); else `offsets` (n_frames + 1, host integers)."""

    def __init__(self, rows, offsets=None, frame_rows=None):
        if rows.dim() == 3:                                    # F x N x 5
            frame_rows = int(rows.shape[1])
            rows = rows.reshape(-1, rows.shape[2])
        if rows.dim() != 2 or rows.shape[1] != 5 or not rows.is_cuda or not rows.is_contiguous():
            raise ValueError("a DeviceBatch is a contiguous N x 5 (or F x N x 5) CUDA tensor")
        self.rows = rows
        if offsets is None:
            if not frame_rows or rows.shape[0] % int(frame_rows):
                raise ValueError("give `offsets`, or `frame_rows` dividing the row count")
            offsets = np.arange(rows.shape[0] // int(frame_rows) + 1, dtype=np.int64) * int(frame_rows)
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        if self.offsets[0] != 0 or self.offsets[-1] > rows.shape[0] or np.any(np.diff(self.offsets) < 0):
            raise ValueError("bad frame offsets")

    def __len__(self):
        return len(self.offsets) - 1


class DeviceResult:
    """What an asynchronous device call leaves behind: `rows` (N_total x 5; the first counts[f] rows of frame f's slot
    [offsets[f], offsets[f + 1]) are its output), `src` (input row of every output row, frame-local), `counts` (n_frames, int64),
    `stats` (n_frames x 3: num_attenuated, num_removed, avg_intensity_diff -- simulation.py:516-538), `status` (8 int32 words),
    `flags` (fused wet ground: 1 where a frame had fewer than 1000 ground rows and came back as the snowfall result) -- all device
    tensors, all still being written until the stream the call was made on has caught up."""

    def __init__(self, ctx, rows, src, counts, stats, status, offsets, stream, flags=None, keep=()):
        self.ctx, self.rows, self.src, self.counts, self.stats, self.status = ctx, rows, src, counts, stats, status
        self.offsets, self.stream, self.flags = offsets, stream, flags
        self._keep = keep                                      # inputs of the call: alive until the result has been waited for

    def wait(self):
        """Wait for the call, raise what the status words say (as the host entry does) and drop the references to the inputs."""
        self.stream.synchronize()
        st = self.status.cpu().numpy()
        self._keep = ()
        self.ctx.check_status(st)                              # SnowGPUError with the library's message
        return self

    def join(self, stream=None):
        """torch's current stream (or `stream`) waits for the call; the host does not.  For results of a lane call (lane=k)."""
        import torch
        (stream or torch.cuda.current_stream(self.rows.device)).wait_stream(self.stream)
        return self

    def frames(self, return_src=False):
        """The reference-shaped result: [(stats, aug_pc)] (or (stats, aug_pc, src)), aug_pc / src views of the result tensors."""
        self.wait()
        counts = self.counts.cpu().numpy()
        stats = self.stats.cpu().numpy()
        out = []
        for i in range(len(self.offsets) - 1):
            a, n = int(self.offsets[i]), int(counts[i])
            st = (np.int64(stats[i, 0]), np.int64(stats[i, 1]), int(stats[i, 2]))
            out.append((st, self.rows[a:a + n], self.src[a:a + n]) if return_src else (st, self.rows[a:a + n]))
        return out


class AlignedResult(DeviceResult):
    """What a `layout='aligned'` call leaves behind: `rows` (N_total x 5, input dtype: row i is the output row of INPUT row i -- removed
    rows too, as they stood before the reference drops them), `keep` (N_total, torch.bool: True where the reference returns the row),
    `counts` (n_frames: flags set per frame), `stats`, `status`, `offsets` as in a DeviceResult.  Nothing here has a data-dependent
    shape: `(rows[:, 3] * keep).sum()` and the like can follow on the same stream, or in the same captured graph, without the host."""

    def __init__(self, ctx, rows, keep_mask, counts, stats, status, offsets, stream, keep=()):
        super().__init__(ctx, rows, None, counts, stats, status, offsets, stream, keep=keep)
        self.keep = keep_mask

    def wait(self):
        """DeviceResult.wait(), with the status words raised as the reference's exception types (IndexError for a point at >= 120 m,
        TypeError for a frame without ground rows), as the synchronous call raises them."""
        from .tools.snowfall.simulation import _raise_like_reference
        try:
            return super().wait()
        except _native.SnowGPUError as err:
            _raise_like_reference(err)

    def frames(self):
        """[(stats, rows_f, keep_f)] per frame, rows_f / keep_f views of the result tensors (waits, as DeviceResult.frames does)."""
        self.wait()
        stats = self.stats.cpu().numpy()
        out = []
        for i in range(len(self.offsets) - 1):
            a, b = int(self.offsets[i]), int(self.offsets[i + 1])
            out.append(((np.int64(stats[i, 0]), np.int64(stats[i, 1]), int(stats[i, 2])), self.rows[a:b], self.keep[a:b]))
        return out


class AlignedWetResult(AlignedResult):
    """An AlignedResult of the wet-ground stage (wet_ground_batch_aligned, augment_wet_batch_aligned): `flags` (n_frames, int32) is 1 where
    a frame had fewer than 1000 present ground rows and came back as it was (augmentation.py:51-52) and 2 where the wet stage was not
    asked for the frame (augment_wet_batch_aligned(weather=...) with the frame's wet gate off); `counts` are the keep flags set after
    the wet stage, `stats` the snowfall statistics (None for the wet-ground model on its own)."""

    def __init__(self, ctx, rows, keep_mask, counts, stats, status, offsets, stream, flags, keep=()):
        super().__init__(ctx, rows, keep_mask, counts, stats, status, offsets, stream, keep=keep)
        self.flags = flags

    def frames(self):
        """[(stats, rows_f, keep_f, flag_f)] per frame, rows_f / keep_f views of the result tensors (waits)."""
        self.wait()
        stats = None if self.stats is None else self.stats.cpu().numpy()
        flags = self.flags.cpu().numpy()
        out = []
        for i in range(len(self.offsets) - 1):
            a, b = int(self.offsets[i]), int(self.offsets[i + 1])
            st = None if stats is None else (np.int64(stats[i, 0]), np.int64(stats[i, 1]), int(stats[i, 2]))
            out.append((st, self.rows[a:b], self.keep[a:b], int(flags[i])))
        return out


class _SmallUploads:
    """Device copies of the small per-call arrays (offsets, table ids, planes, polynomials), by value: a few KB each, least
    recently used first out."""

    def __init__(self, cap=64):
        self.cap, self.d = cap, OrderedDict()

    def get(self, torch, dev, arr, user):
        """The device copy of `arr`, safe to read on stream `user`: a copy made by an earlier call on another stream is waited for by event."""
        key = (str(dev), arr.dtype.str, arr.shape, arr.tobytes())
        hit = self.d.get(key)
        if hit is None:
            t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)                # (on torch's current stream)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            hit = self.d[key] = (t, ev)
            while len(self.d) > self.cap:
                self.d.popitem(last=False)
        else:
            self.d.move_to_end(key)
            if torch.cuda.is_current_stream_capturing():
                # The runtime refuses to query an event whose stream is capturing now -- that of a warm-up call made on the stream of the
                # capture.  The copy was made before the capture began, and torch.cuda.graph synchronises the device when it begins.
                return hit[0]
        if not hit[1].query():
            user.wait_event(hit[1])
        return hit[0]


def _uploads(eng):
    u = eng.__dict__.get("_small_uploads")
    if u is None:
        u = eng.__dict__["_small_uploads"] = _SmallUploads()
    return u


def _as_batch(torch, frames):
    """(rows N_total x 5 contiguous, host offsets, extras or None) from a DeviceBatch, an F x N x C tensor or a list of N_i x C tensors."""
    if isinstance(frames, DeviceBatch):
        return frames.rows, frames.offsets, None
    if not isinstance(frames, (list, tuple)):
        if frames.dim() == 3:
            frames = list(frames.unbind(0))
        else:
            frames = [frames]
    for f in frames:
        if f.dim() != 2 or f.shape[1] < 5:
            raise ValueError("pc must be N x 5 (x, y, z, intensity, channel)")
        if f.dtype != frames[0].dtype or f.device != frames[0].device:
            raise TypeError("all frames of a batch must share one dtype and device")
    if frames[0].dtype not in (torch.float32, torch.float64):
        frames = [f.to(torch.float64) for f in frames]
    offsets = np.zeros(len(frames) + 1, np.int64)
    offsets[1:] = np.cumsum([int(f.shape[0]) for f in frames])
    extra = any(f.shape[1] > 5 for f in frames)
    if len(frames) == 1 and frames[0].shape[1] == 5 and frames[0].is_contiguous():
        rows = frames[0]                                                          # read in place
    else:
        rows = torch.cat([f[:, :5] for f in frames]).contiguous()                 # device-to-device; never through the host
    return rows, offsets, (frames if extra else None)


def _rows_where_they_lie(torch, frames):
    """(rows, host offsets) of an input that is ALREADY one contiguous N_total x 5 float32 / float64 tensor -- a DeviceBatch, an F x N x 5
    tensor, one N x 5 tensor (or a list of one) -- for in_place=True; anything that would have to be concatenated or converted raises."""
    if isinstance(frames, DeviceBatch):
        rows, offsets = frames.rows, frames.offsets
    else:
        t = frames[0] if isinstance(frames, (list, tuple)) and len(frames) == 1 else frames
        if isinstance(t, (list, tuple)):
            raise ValueError("in_place=True needs the frames in ONE tensor (a DeviceBatch, an F x N x 5 or an N x 5 tensor): a list is "
                             "concatenated into a temporary, and the result would land there")
        if t.dim() not in (2, 3) or t.shape[-1] != 5 or not t.is_contiguous():
            raise ValueError("in_place=True needs a contiguous N x 5 or F x N x 5 tensor: the result is written over the input's five columns")
        per = int(t.shape[-2])
        offsets = np.arange((int(t.shape[0]) if t.dim() == 3 else 1) + 1, dtype=np.int64) * per
        rows = t.reshape(-1, 5)
    if rows.dtype not in (torch.float32, torch.float64):
        raise ValueError("in_place=True needs float32 or float64 rows: other dtypes are converted into a temporary")
    return rows, offsets


def _run_stream(torch, eng, dev, stream, lane=None):
    """The torch stream a call is launched on: the caller's `stream` itself, or -- for torch's legacy default stream (handle 0, which the C
    ABI reads as "the context's own stream") and for a compute lane -- a side stream of the engine's, made on first use."""
    if stream.cuda_stream != 0 and lane is None:
        return stream
    run = eng.__dict__.get("_torch_side_stream")
    if run is None or run.device != dev:
        if lane is not None:
            # lanes k, k + 1, k + 2 on streams of three different priorities: three queue pools of the runtime, so three hardware
            # queues whatever else the process has created (include/snowgpu.h: snowgpu_lane_stream)
            many = int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) >= 16      # (then every stream has a queue anyway: one priority)
            order = [int(v) for v in os.environ.get("SNOWGPU_LANE_LEVELS", "1" if many else "2,1,0").split(",")]
            run = torch.cuda.ExternalStream(eng.ctx.lane_stream(order[int(lane) % len(order)]), device=dev)
        else:
            run = torch.cuda.Stream(device=dev)
        eng.__dict__["_torch_side_stream"] = run
    return run


def _resolve_input(torch, frames, in_place, device, slot, lane=None):
    """(rows, host offsets, extras or None, engine) of a call: the frames as one N_total x 5 tensor -- read where they lie for in_place --
    on the device that `device` names if it names one, and the engine of `slot`, or of compute lane `lane`: an engine of its own whose
    batches run on one stream (snowgpu_set_serial, once): they overlap OTHER lanes' batches, not their own side streams."""
    from . import engine as _engine
    rows, offsets, extras = _rows_where_they_lie(torch, frames) + (None,) if in_place else _as_batch(torch, frames)
    dev = rows.device
    if device is not None and int(device) != dev.index:
        raise ValueError(f"the tensors live on {dev}, device={device} was asked for")
    eng = _engine.get_engine(dev.index, slot if lane is None else LANE_SLOT0 + int(lane))
    if lane is not None and not eng.__dict__.get("_lane_serial"):
        eng.ctx.set_serial(True)      # (with GPU_MAX_HW_QUEUES >= 16 every lane's stream has a hardware queue of its own: include/snowgpu.h)
        eng.__dict__["_lane_serial"] = True
    return rows, offsets, extras, eng


@contextmanager
def _on_run_stream(torch, eng, dev, lane=None, used=()):
    """(torch's current stream, the stream the call runs on) with the fork and the join around the body.  The C ABI reads stream = NULL as
    "the context's own stream", which is not ordered against anything of torch's.  torch's legacy default stream HAS the handle 0, so a
    call made on it runs on a side stream of the engine, forked from and joined back into the default stream (two event waits): work
    queued before the call is seen, and whoever reads the results on the caller's stream afterwards -- or synchronises it -- waits for
    the call.  A lane's stream forks alike and nothing waits for it (the result is claimed by wait() / join()); the tensors in `used`
    are the caller's stream's, used on the lane's: the allocator must know."""
    stream = torch.cuda.current_stream(dev)
    run = _run_stream(torch, eng, dev, stream, lane)
    if run is not stream:
        run.wait_stream(stream)
        if lane is not None:
            for t in used:
                if t is not None:
                    t.record_stream(run)
    try:
        yield stream, run
    finally:
        if run is not stream and lane is None:
            stream.wait_stream(run)


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
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
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
        index = torch.cuda.current_device() if device is None else (device.index if isinstance(device, torch.device) else int(device))
        self.device = torch.device("cuda", index)
        self.eng = _engine.get_engine(index, slot)
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


def _keep_mask(torch, keep, rows, offsets):
    """One contiguous torch.bool element per row of the batch from `keep`: an N_total tensor, an F x N tensor or a list of per-frame
    tensors, torch.bool or uint8 (non-zero = present)."""
    n = int(offsets[-1])
    if isinstance(keep, (list, tuple)):
        if len(keep) != len(offsets) - 1 or any(int(k.shape[0]) != int(b - a) or k.dim() != 1 for k, a, b in zip(keep, offsets[:-1], offsets[1:])):
            raise ValueError("keep as a list needs one 1-D tensor per frame with one element per row of it")
        if any(k.dtype != keep[0].dtype for k in keep):
            raise ValueError("all keep tensors of a batch must share one dtype")
        keep = torch.cat(list(keep)) if len(keep) != 1 else keep[0]
    if not (type(keep).__module__.startswith("torch") and getattr(keep, "is_cuda", False)) or keep.device != rows.device:
        raise ValueError("keep must be a CUDA tensor on the device of the rows (or a list of them)")
    if keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError("keep must be torch.bool or uint8")
    if keep.dim() == 2:
        keep = keep.reshape(-1)
    if keep.dim() != 1 or keep.shape[0] != n:
        raise ValueError("keep must have one element per row of the batch (N_total, F x N, or a list of per-frame tensors)")
    keep = keep.contiguous()
    return keep.view(torch.bool) if keep.dtype == torch.uint8 else keep


def _fov_mask(torch, eng, rows, calib, img_shape, keep, run):
    """keep AND the camera-FOV test of every row, as a new torch.bool tensor, launched on torch stream `run` (k_fov_mask)."""
    out = torch.empty(rows.shape[0], dtype=torch.bool, device=rows.device)
    if rows.shape[0]:
        eng.ctx.fov_mask_device(rows.shape[0], rows.data_ptr(), 0 if rows.dtype == torch.float32 else 1, calib, img_shape,
                                0 if keep is None else keep.data_ptr(), out.data_ptr(), run.cuda_stream)
    return out


def fov_keep(frames, calib, img_shape=(1024, 1920), keep=None, *, device=None, slot=0):
    """get_fov_flag(calib.lidar_to_rect(pc[:, 0:3]), img_shape, calib) (simulation.py:39-47) for torch CUDA tensors, on the device: a
    torch.bool mask with one element per row of the batch (frames as augment_batch takes them), ANDed with `keep` if given -- the crop of
    precompute.py:96-99 as a keep mask for augment_batch(..., layout='aligned', keep=mask) or any other consumer.  Asynchronous on
    torch's current stream."""
    if not is_device_input(frames):
        raise ValueError("fov_keep: torch CUDA tensors (host arrays: lidar_snow_sim_amd.calibration.get_fov_flag)")
    import torch
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    with torch.cuda.device(rows.device), _on_run_stream(torch, eng, rows.device) as (_, run):
        return _fov_mask(torch, eng, rows[:int(offsets[-1])], calib, img_shape, keep, run)


def dror_keep(frames, alpha=0.45, beta=3, k_min=3, sr_min=0.04, keep=None, *, out=None, return_neighbours=False, device=None, slot=0):
    """Dynamic radius outlier removal (DROR, Charron et al. 2018; pointcloud_viewer.py:2756-2758 with the defaults of :267-270) for torch
    CUDA tensors, on the device: a torch.bool mask with one element per row of the batch (frames as augment_batch takes them), True where
    the row is usable -- present under `keep`, every coordinate finite and within 1e6 m -- and has at least k_min other usable rows of its
    frame within max(sr_min, beta * radians(alpha) * r_xy) of it (the definition: include/snowgpu.h, snowgpu_dror_mask_device).

    frames    torch CUDA tensors, a DeviceBatch -- or an AlignedResult / AlignedWetResult: its rows, offsets and keep mask are used
              (nothing is waited for), as voxelize and the stages behind it take one.
    keep      an input keep mask as augment_batch(layout='aligned') takes it: an absent row is False, nobody's neighbour, never looked at
              (with a result: ANDed with the result's own).
    out       a torch.bool tensor with one element per row to write into (static addresses for a captured graph); not the `keep` tensor.
    return_neighbours   also return an int32 tensor: every row's neighbours, counted up to k_min.

    The mask goes straight into augment_batch(..., layout='aligned', keep=mask), augment_wet_batch_aligned(..., keep=mask) or
    fov_keep(..., keep=mask); dror_keep(res) filters an augmented batch frame by frame.  dror_keep(res.rows, keep=res.keep) is NOT that
    for a batch of several frames: one N_total x 5 tensor is ONE frame, and rows of different frames become each other's neighbours.
    Asynchronous on torch's current stream."""
    import math
    import torch
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError("dror_keep: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.dror.dynamic_radius_outlier_filter)")
    c = float(beta) * (float(alpha) * (math.pi / 180.0))
    if not (0.0 < c <= 0.25):
        raise ValueError("dror_keep: beta * radians(alpha) must lie in (0, 0.25]")
    if not (float(sr_min) >= 0.0 and math.isfinite(float(sr_min))):
        raise ValueError("dror_keep: sr_min must be finite and >= 0")
    if int(k_min) != k_min or not (0 <= int(k_min) <= 65535):
        raise ValueError("dror_keep: k_min must be an integer in 0 .. 65535")
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    if out is None:
        out = torch.empty(n, dtype=torch.bool, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.bool and out.dim() == 1 and out.shape[0] == n and out.is_contiguous() and out.device == dev):
        raise ValueError("dror_keep: out must be a contiguous torch.bool tensor with one element per row, on the device of the rows")
    if keep is not None and n and out.data_ptr() < keep.data_ptr() + n and keep.data_ptr() < out.data_ptr() + n:
        raise ValueError("dror_keep: out must not be (or overlap) the keep tensor; the query of one row reads other rows' keep elements")
    nb = torch.zeros(n, dtype=torch.int32, device=dev) if return_neighbours else None
    if nf and n:
        up = _uploads(eng)
        with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
            d_off = up.get(torch, dev, offsets, run)
            eng.ctx.dror_mask_device(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr(), 0 if rows.dtype == torch.float32 else 1,
                                     float(alpha), float(beta), float(sr_min), int(k_min), 0 if keep is None else keep.data_ptr(), out.data_ptr(),
                                     0 if nb is None else nb.data_ptr(), run.cuda_stream)
    return (out, nb) if return_neighbours else out


class VoxelBatch:
    """What voxelize() leaves behind, F = frames, V = max_voxels, T = max_points, C = num_features -- every shape static:
    `voxels` (F V, T, C; the rows' dtype), `coords` (F V, 4 int32: frame, z, y, x cell), `num_points` (F V, int32), `voxel_offsets`
    (F + 1 int32, ON THE DEVICE: frame f's voxels are [voxel_offsets[f], voxel_offsets[f + 1]), the packed voxels end at
    voxel_offsets[F]; beyond it voxels are 0, coords -1, num_points 0) and `voxel_of` (N_total int32: every row's packed voxel, -1 without
    one; None unless asked for).  All still being written until the stream the call was made on has caught up."""

    def __init__(self, voxels, coords, num_points, voxel_offsets, voxel_of=None):
        self.voxels, self.coords, self.num_points, self.voxel_offsets, self.voxel_of = voxels, coords, num_points, voxel_offsets, voxel_of

    @classmethod
    def empty(cls, n_frames, max_points, max_voxels, num_features=4, dtype=None, device=None, n_rows=None):
        """Uninitialised buffers of the shapes voxelize() writes for such a call (out=): static addresses for a captured graph.
        n_rows: also a `voxel_of` for a batch of that many rows."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
        slots = int(n_frames) * int(max_voxels)
        i32 = dict(dtype=torch.int32, device=dev)
        return cls(torch.empty((slots, int(max_points), int(num_features)), dtype=dtype or torch.float32, device=dev), torch.empty((slots, 4), **i32),
                   torch.empty(slots, **i32), torch.empty(int(n_frames) + 1, **i32), None if n_rows is None else torch.empty(int(n_rows), **i32))

    def frames(self):
        """[(voxels_f, coords_f, num_points_f)] per frame, trimmed views of the result tensors.  Reads the offsets: synchronizes."""
        off = self.voxel_offsets.cpu().numpy()
        return [(self.voxels[a:b], self.coords[a:b], self.num_points[a:b]) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def voxelize(frames, point_cloud_range, voxel_size, max_points, max_voxels, *, keep=None, num_features=4, out=None, return_voxel_of=False,
             device=None, slot=0):
    """Point-to-voxel grouping on the device (snowgpu_voxelize_device; the definition: include/snowgpu.h): the first operation of SECOND,
    PV-RCNN and PointPillars, with static shapes.  Per frame, the rows that are present, finite and inside point_cloud_range
    (x0, y0, z0, x1, y1, z1) are walked in input order; the first row of a new cell opens the frame's next voxel (cells beyond max_voxels
    are dropped), and a voxel stores its first max_points rows, columns 0 .. num_features - 1, bit for bit.

    frames    what dror_keep takes -- or an AlignedResult / AlignedWetResult: its rows, offsets and keep mask are used (nothing is waited for).
    keep      an input keep mask as the aligned calls take it (with a result: ANDed with the result's own).
    out       a VoxelBatch to write into (VoxelBatch.empty): every element is written, nothing needs clearing.
    return_voxel_of   also fill `voxel_of`: every row's packed voxel index, -1 without one (dynamic voxelization's point-to-voxel map).

    Returns a VoxelBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError("voxelize: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.voxel.points_to_voxels)")
    for name, v in (("max_points", max_points), ("max_voxels", max_voxels), ("num_features", num_features)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"voxelize: {name} must be an integer")
    rng, size = np.asarray(point_cloud_range, np.float64).reshape(-1), np.asarray(voxel_size, np.float64).reshape(-1)
    if rng.shape != (6,) or size.shape != (3,):
        raise ValueError("voxelize: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1), voxel_size 3")
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    T, V, C = int(max_points), int(max_voxels), int(num_features)
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    # (the shapes below need these three; the entry refuses them in the same words, and everything else of the domain)
    if not 3 <= C <= 5:
        raise ValueError("voxelize: n_features must be 3, 4 or 5: the columns of a row that a voxel stores")
    if T < 1 or V < 1:
        raise ValueError("voxelize: max_points and max_voxels must be at least 1")
    if nf * V > 2 ** 31 - 1:
        raise ValueError("voxelize: n_frames * max_voxels exceeds 2^31 - 1; split the batch")
    if out is None:
        out = VoxelBatch.empty(nf, T, V, C, rows.dtype, dev, n if return_voxel_of else None)
    else:
        want = (("voxels", (nf * V, T, C), rows.dtype), ("coords", (nf * V, 4), torch.int32), ("num_points", (nf * V,), torch.int32),
                ("voxel_offsets", (nf + 1,), torch.int32)) + ((("voxel_of", (n,), torch.int32),) if return_voxel_of else ())
        for name, shape, dtype in want:
            t = getattr(out, name, None) if isinstance(out, VoxelBatch) else None
            if not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev):
                raise ValueError(f"voxelize: out must be a VoxelBatch whose {name} is a contiguous {tuple(shape)} {dtype} tensor on the device of the rows")
    vof = out.voxel_of if return_voxel_of else None
    if n == 0:                                          # no row: the entry writes the offsets alone
        out.voxels.zero_(); out.coords.fill_(-1); out.num_points.zero_()
    up = _uploads(eng)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        d_off = up.get(torch, dev, offsets, run)
        eng.ctx.voxelize_device(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr() if n else 0, 0 if rows.dtype == torch.float32 else 1,
                                rng, size, T, V, C, 0 if keep is None or not n else keep.data_ptr(), out.voxels.data_ptr(), out.coords.data_ptr(),
                                out.num_points.data_ptr(), out.voxel_offsets.data_ptr(), 0 if vof is None or not n else vof.data_ptr(), run.cuda_stream)
    return out if return_voxel_of or out.voxel_of is None else VoxelBatch(out.voxels, out.coords, out.num_points, out.voxel_offsets)


class KeypointBatch:
    """What sample_keypoints() leaves behind, F = frames, K = n_samples, C = num_features -- every shape static: `index` (F, K int32: the
    sampled rows as indices into the whole batch, so rows[index] gathers; -1 for a frame without a usable row), `points` (F, K, C; the
    rows' dtype; zero for such a frame), `usable` (F int32, ON THE DEVICE: the usable rows of every frame -- beyond them a frame's samples
    repeat its first usable row) and `dist` (F, K; the rows' dtype: the squared distance of every sample to the samples before it at the
    moment it was chosen, +inf for the first, -1 for a frame without a usable row; None unless asked for).  All still being written until
    the stream the call was made on has caught up."""

    def __init__(self, index, points, usable, dist=None, sector_offsets=None, sector_count=None, sector_of=None):
        self.index, self.points, self.usable, self.dist = index, points, usable, dist
        # set by the sectorized call alone (sample_keypoints(sectors=..., rois=...)): (F, S + 1) int32 -- slots [o_s, o_{s+1}) of a frame
        # are its sector s, o_S = min(usable, K) --, (F, S) int32 -- the usable rows of every sector -- and, when asked for, (N) int8:
        # every row's sector, -1 for an absent or unusable row
        self.sector_offsets, self.sector_count, self.sector_of = sector_offsets, sector_count, sector_of

    @classmethod
    def empty(cls, n_frames, n_samples, num_features=4, dtype=None, device=None, with_dist=False, sectors=None, with_sector_of=None):
        """Uninitialised buffers of the shapes sample_keypoints() writes for such a call (out=): static addresses for a captured graph.
        sectors = S adds sector_offsets and sector_count, with_sector_of = the rows of the batch adds sector_of."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
        F, K, dt = int(n_frames), int(n_samples), dtype or torch.float32
        out = cls(torch.empty((F, K), dtype=torch.int32, device=dev), torch.empty((F, K, int(num_features)), dtype=dt, device=dev),
                  torch.empty(F, dtype=torch.int32, device=dev), torch.empty((F, K), dtype=dt, device=dev) if with_dist else None)
        if sectors is not None:
            out.sector_offsets = torch.empty((F, int(sectors) + 1), dtype=torch.int32, device=dev)
            out.sector_count = torch.empty((F, int(sectors)), dtype=torch.int32, device=dev)
            if with_sector_of is not None and with_sector_of is not False:
                out.sector_of = torch.empty(int(with_sector_of), dtype=torch.int8, device=dev)
        return out


def sample_keypoints(frames, n_samples, *, point_cloud_range=None, keep=None, num_features=4, out=None, return_dist=False, device=None, slot=0,
                     sectors=None, rois=None, roi_margin=1.6, return_sector_of=False):
    """Farthest point sampling on the device (snowgpu_fps_device; the definition: include/snowgpu.h): the keypoints of PV-RCNN and the
    fixed-size point set of PointRCNN / Part-A2, with static shapes.  Per frame, among the rows that are present, within 1e6 of the origin
    on every axis and inside point_cloud_range (x0, y0, z0, x1, y1, z1; None: no range), the first is taken, then n_samples - 1 times the
    row farthest from everything taken so far (squared distance in the rows' dtype; the smallest row index among equals).

    frames    what voxelize takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult: its rows, offsets and keep
              mask are used (nothing is waited for).
    keep      an input keep mask as the aligned calls take it (with a result: ANDed with the result's own).
    out       a KeypointBatch to write into (KeypointBatch.empty): every element is written, nothing needs clearing.
    return_dist   also fill `dist`.
    sectors, rois, roi_margin, return_sector_of
              PV-RCNN++'s sectorized, proposal-centric sampling (snowgpu_fps_sectors_device): with rois -- an (F, B, 7 .. 10) device
              tensor of the rows' dtype, OpenPCDet's rois / gt_boxes, zero rows are padding -- only the rows within a roi's half diagonal
              + roi_margin of its centre are usable; the usable rows are split by azimuth into `sectors` sectors (1 .. 16; 1 when only
              rois are given) and every sector is walked on its own for its share of n_samples.  The result carries sector_offsets and
              sector_count, and with return_sector_of every row's sector.  With both None the plain walk runs, untouched.

    Returns a KeypointBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    if sectors is not None or rois is not None:
        return _sample_keypoints_sectors(torch, frames, n_samples, point_cloud_range, keep, num_features, out, return_dist, device, slot,
                                         1 if sectors is None else sectors, rois, roi_margin, return_sector_of)
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError("sample_keypoints: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.fps.farthest_point_sample)")
    for name, v in (("n_samples", n_samples), ("num_features", num_features)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"sample_keypoints: {name} must be an integer")
    rng = None
    if point_cloud_range is not None:
        rng = np.asarray(point_cloud_range, np.float64).reshape(-1)
        if rng.shape != (6,):
            raise ValueError("sample_keypoints: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)")
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    K, C = int(n_samples), int(num_features)
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 3 <= C <= 5:
        raise ValueError("sample_keypoints: n_features must be 3, 4 or 5: the columns of a row that a keypoint carries")
    if K < 1:
        raise ValueError("sample_keypoints: n_samples must be at least 1")
    if nf * K > 2 ** 31 - 1:
        raise ValueError("sample_keypoints: n_frames * n_samples exceeds 2^31 - 1; split the batch")
    if out is None:
        out = KeypointBatch.empty(nf, K, C, rows.dtype, dev, return_dist)
    else:
        want = (("index", (nf, K), torch.int32), ("points", (nf, K, C), rows.dtype), ("usable", (nf,), torch.int32)) + \
               ((("dist", (nf, K), rows.dtype),) if return_dist else ())
        for name, shape, dtype in want:
            t = getattr(out, name, None) if isinstance(out, KeypointBatch) else None
            if not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev):
                raise ValueError(f"sample_keypoints: out must be a KeypointBatch whose {name} is a contiguous {tuple(shape)} {dtype} tensor on the device of the rows")
    dist = out.dist if return_dist else None
    up = _uploads(eng)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        d_off = up.get(torch, dev, offsets, run)
        eng.ctx.fps_device(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr() if n else 0, 0 if rows.dtype == torch.float32 else 1,
                           rng, K, C, 0 if keep is None or not n else keep.data_ptr(), out.index.data_ptr(), out.points.data_ptr(),
                           0 if dist is None else dist.data_ptr(), out.usable.data_ptr(), run.cuda_stream)
    return out if return_dist or out.dist is None else KeypointBatch(out.index, out.points, out.usable)


def _sample_keypoints_sectors(torch, frames, n_samples, point_cloud_range, keep, num_features, out, return_dist, device, slot, sectors, rois, roi_margin,
                              return_sector_of):
    """sample_keypoints() with sectors or rois: snowgpu_fps_sectors_device."""
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError("sample_keypoints: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.fps.sectorized_sample)")
    for name, v in (("n_samples", n_samples), ("num_features", num_features), ("sectors", sectors)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"sample_keypoints: {name} must be an integer")
    rng = None
    if point_cloud_range is not None:
        rng = np.asarray(point_cloud_range, np.float64).reshape(-1)
        if rng.shape != (6,):
            raise ValueError("sample_keypoints: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)")
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    K, C, S = int(n_samples), int(num_features), int(sectors)
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 3 <= C <= 5:
        raise ValueError("sample_keypoints: n_features must be 3, 4 or 5: the columns of a row that a keypoint carries")
    if K < 1:
        raise ValueError("sample_keypoints: n_samples must be at least 1")
    if nf * K > 2 ** 31 - 1:
        raise ValueError("sample_keypoints: n_frames * n_samples exceeds 2^31 - 1; split the batch")
    if not 1 <= S <= 16:
        raise ValueError("sample_keypoints: n_sectors must lie in 1 .. 16")
    B = Cb = 0
    if rois is not None:
        if not (torch.is_tensor(rois) and rois.is_cuda and rois.device == dev and rois.dtype == rows.dtype and rois.dim() == 3 and rois.shape[0] == nf
                and rois.is_contiguous()):
            raise ValueError("sample_keypoints: rois must be a contiguous (frames, B, 7 .. 10) tensor of the rows' dtype on the device of the rows")
        B, Cb = int(rois.shape[1]), int(rois.shape[2])
    if out is None:
        out = KeypointBatch.empty(nf, K, C, rows.dtype, dev, return_dist, S, n if return_sector_of else None)
    else:
        want = (("index", (nf, K), torch.int32), ("points", (nf, K, C), rows.dtype), ("usable", (nf,), torch.int32),
                ("sector_offsets", (nf, S + 1), torch.int32), ("sector_count", (nf, S), torch.int32)) + \
               ((("dist", (nf, K), rows.dtype),) if return_dist else ()) + ((("sector_of", (n,), torch.int8),) if return_sector_of else ())
        for name, shape, dtype in want:
            t = getattr(out, name, None) if isinstance(out, KeypointBatch) else None
            if not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev):
                raise ValueError(f"sample_keypoints: out must be a KeypointBatch whose {name} is a contiguous {tuple(shape)} {dtype} tensor on the device of the rows")
    dist = out.dist if return_dist else None
    sof = out.sector_of if return_sector_of else None
    up = _uploads(eng)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        d_off = up.get(torch, dev, offsets, run)
        eng.ctx.fps_sectors_device(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr() if n else 0, 0 if rows.dtype == torch.float32 else 1,
                                   rng, K, C, 0 if keep is None or not n else keep.data_ptr(), S, 0 if rois is None else rois.data_ptr(), B, Cb,
                                   roi_margin, out.index.data_ptr(), out.points.data_ptr(), 0 if dist is None else dist.data_ptr(), out.usable.data_ptr(),
                                   out.sector_offsets.data_ptr(), out.sector_count.data_ptr(), 0 if sof is None or not n else sof.data_ptr(), 0,
                                   run.cuda_stream)
    if (dist is None) == (out.dist is None) and (sof is None) == (out.sector_of is None):
        return out
    return KeypointBatch(out.index, out.points, out.usable, dist, out.sector_offsets, out.sector_count, sof)      # (without what was not asked for)


class NeighbourBatch:
    """What ball_query() leaves behind, F = frames, K = centres per frame, R = (radius, samples) pairs, S = the sum of their samples,
    C = num_features -- every shape static: `index` (F, K, S int32: per centre the segments of the R pairs side by side, each the smallest
    row indices of the ball, ascending, as indices into the whole batch, padded with its first; -1 for an empty ball), `count` (F, K, R
    int32: the rows in every ball, not saturated), `points` (F, K, S, C; the rows' dtype; zero where the index is -1; None unless asked
    for) and `segments` (the samples of every pair, a tuple: index[..., sum(segments[:i]):sum(segments[:i + 1])] is pair i).  All still
    being written until the stream the call was made on has caught up."""

    def __init__(self, index, count, points=None, segments=()):
        self.index, self.count, self.points, self.segments = index, count, points, tuple(int(s) for s in segments)

    @classmethod
    def empty(cls, n_frames, n_centres, n_neighbours, num_features=4, dtype=None, device=None, with_points=False):
        """Uninitialised buffers of the shapes ball_query() writes for such a call (out=): static addresses for a captured graph."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
        seg = tuple(int(s) for s in (n_neighbours if isinstance(n_neighbours, (tuple, list, np.ndarray)) else (n_neighbours,)))
        F, K, S = int(n_frames), int(n_centres), sum(seg)
        return cls(torch.empty((F, K, S), dtype=torch.int32, device=dev), torch.empty((F, K, len(seg)), dtype=torch.int32, device=dev),
                   torch.empty((F, K, S, int(num_features)), dtype=dtype or torch.float32, device=dev) if with_points else None, seg)


def ball_query(frames, centres, radius, n_neighbours, *, point_cloud_range=None, keep=None, num_features=4, out=None, return_points=False,
               device=None, slot=0):
    """Ball-query neighbour groups on the device (snowgpu_ball_query_device; the definition: include/snowgpu.h): for every centre the
    n_neighbours smallest row indices of its frame among the rows that are present, within 1e6 of the origin on every axis, inside
    point_cloud_range (None: no range) and STRICTLY within `radius` of the centre (squared distance in the rows' dtype), ascending and
    padded with the first -- what the pointnet2 ball_query op returns --, -1 for an empty ball, and the full number of rows in the ball.

    frames    what sample_keypoints takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult: its rows, offsets
              and keep mask are used (nothing is waited for).
    centres   a KeypointBatch (its points), or an (F, K, 3 .. 5) tensor in the rows' dtype on their device: x, y, z first.
    radius, n_neighbours   scalars, or sequences of equal length <= 4: several balls per centre from one walk, side by side in `index`.
    keep      an input keep mask as the aligned calls take it (with a result: ANDed with the result's own).
    out       a NeighbourBatch to write into (NeighbourBatch.empty): every element is written, nothing needs clearing.
    return_points   also fill `points` with the first num_features columns of the indexed rows.

    Returns a NeighbourBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError("ball_query: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.ball.ball_query)")
    seq = lambda v: list(v) if isinstance(v, (tuple, list, np.ndarray)) else [v]
    radii, seg = seq(radius), seq(n_neighbours)
    if len(radii) != len(seg):
        raise ValueError("ball_query: as many radii as sample counts")
    for name, v in (("num_features", num_features),) + tuple(("n_neighbours", s) for s in seg):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"ball_query: {name} must be an integer")
    rng = None
    if point_cloud_range is not None:
        rng = np.asarray(point_cloud_range, np.float64).reshape(-1)
        if rng.shape != (6,):
            raise ValueError("ball_query: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)")
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    cen = centres.points if isinstance(centres, KeypointBatch) else centres
    if not (torch.is_tensor(cen) and cen.dim() == 3 and cen.shape[0] == nf and cen.dtype == rows.dtype and cen.device == dev and cen.is_contiguous()):
        raise ValueError("ball_query: centres must be a KeypointBatch or a contiguous (frames, K, 3 .. 5) tensor in the rows' dtype on their device")
    K, Cq, C, R = int(cen.shape[1]), int(cen.shape[2]), int(num_features), len(radii)
    seg = [int(s) for s in seg]
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 3 <= C <= 5:
        raise ValueError("ball_query: n_features must be 3, 4 or 5: the columns of a row that a neighbour carries")
    if not 3 <= Cq <= 5:
        raise ValueError("ball_query: centre_features must be 3, 4 or 5: x, y, z first")
    if K < 1:
        raise ValueError("ball_query: n_centres must be at least 1")
    if not 1 <= R <= 4:
        raise ValueError("ball_query: n_radii must lie in 1 .. 4")
    if any(not 1 <= s <= 64 for s in seg):
        raise ValueError("ball_query: the samples of a radius must lie in 1 .. 64")
    S = sum(seg)
    if nf * K * S > 2 ** 31 - 1:
        raise ValueError("ball_query: n_frames * n_centres * samples exceeds 2^31 - 1; split the batch")
    if out is None:
        out = NeighbourBatch.empty(nf, K, seg, C, rows.dtype, dev, return_points)
    else:
        want = (("index", (nf, K, S), torch.int32), ("count", (nf, K, R), torch.int32)) + ((("points", (nf, K, S, C), rows.dtype),) if return_points else ())
        for name, shape, dtype in want:
            t = getattr(out, name, None) if isinstance(out, NeighbourBatch) else None
            if not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev):
                raise ValueError(f"ball_query: out must be a NeighbourBatch whose {name} is a contiguous {tuple(shape)} {dtype} tensor on the device of the rows")
    points = out.points if return_points else None
    up = _uploads(eng)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        d_off = up.get(torch, dev, offsets, run)
        eng.ctx.ball_query_device(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr() if n else 0, 0 if rows.dtype == torch.float32 else 1,
                                  rng, K, cen.data_ptr(), Cq, radii, seg, C, 0 if keep is None or not n else keep.data_ptr(), out.index.data_ptr(),
                                  out.count.data_ptr(), 0 if points is None else points.data_ptr(), run.cuda_stream)
    return NeighbourBatch(out.index, out.count, points, seg) if (out.segments != tuple(seg) or (points is None) != (out.points is None)) else out


class RangeImageBatch:
    """What range_image() leaves behind, F = frames, H x W the image, C = num_features -- every shape static: `image` (F, 1 + C, H, W; the
    rows' dtype: plane 0 the range of the pixel's nearest row, planes 1 .. C its columns 0 .. C - 1, bit for bit; -1 in an empty pixel),
    `index` (F, H, W int32: that row as an index into the whole batch, so rows[index] gathers; -1 in an empty pixel), `pixel_of` (N_total
    int32: every row's flat pixel f H W + row W + col, whether it won or not; -1 for absent and unusable rows) and `count` (F, H, W int32:
    the usable rows that fell in the pixel; None unless asked for).  All still being written until the stream the call was made on has
    caught up."""

    def __init__(self, image, index, pixel_of, count=None):
        self.image, self.index, self.pixel_of, self.count = image, index, pixel_of, count

    @classmethod
    def empty(cls, n_frames, height, width, n_rows, num_features=4, dtype=None, device=None, with_count=False):
        """Uninitialised buffers of the shapes range_image() writes for such a call on a batch of n_rows rows (out=): static addresses
        for a captured graph."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
        F, H, W = int(n_frames), int(height), int(width)
        i32 = dict(dtype=torch.int32, device=dev)
        return cls(torch.empty((F, 1 + int(num_features), H, W), dtype=dtype or torch.float32, device=dev), torch.empty((F, H, W), **i32),
                   torch.empty(int(n_rows), **i32), torch.empty((F, H, W), **i32) if with_count else None)

    def to_rows(self, values, fill=0):
        """The way back: a per-pixel tensor (F, H, W) or (F, X, H, W) -- a de-noiser's keep or class map -- as a per-row tensor (N,) or
        (N, X): every row gets the value of its pixel, `fill` where pixel_of is -1.  Pure indexing on the device, nothing is read on
        the host: a predicted mask goes straight into augment_batch(..., keep=) or dror_keep(..., keep=)."""
        import torch
        F, H, W = self.index.shape
        if not (torch.is_tensor(values) and values.dim() in (3, 4) and values.shape[0] == F and tuple(values.shape[-2:]) == (H, W)):
            raise ValueError(f"to_rows: values must be a ({F}, {H}, {W}) or ({F}, X, {H}, {W}) tensor: one value, or X of them, per pixel")
        p = self.pixel_of.long()
        at = p.clamp(min=0)
        if values.dim() == 3:
            got = values.reshape(-1)[at]
            return torch.where(p >= 0, got, torch.full_like(got, fill))
        f = torch.div(at, H * W, rounding_mode="floor")
        got = values.reshape(F, values.shape[1], H * W)[f, :, at - f * (H * W)]
        return torch.where((p >= 0)[:, None], got, torch.full_like(got, fill))


def range_image(frames, height, width, *, fov_up=3.0, fov_down=-25.0, ring=None, range_limits=(0.0, float("inf")), keep=None, num_features=4,
                out=None, return_count=False, device=None, slot=0):
    """Range-image projection on the device (snowgpu_range_image_device; the definition: include/snowgpu.h): every frame as a height x
    width image of its nearest returns, the input of the range-view networks (RangeNet++, SalsaNext) and of the snow de-noisers
    (WeatherNet, 4DenoiseNet, LiSnowNet), with static shapes.  The column is the azimuth, the image row the elevation between fov_down and
    fov_up (DEGREES, as the RangeNet++ configs give them; rows beyond are clamped to the first and last image row) -- or, with `ring`,
    the row's laser channel.  Per pixel the usable row (present, within 1e6 of the origin on every axis, range strictly inside
    range_limits) with the smallest range wins, the smallest row index among equals.

    frames    what voxelize takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult: its rows, offsets and keep
              mask are used (nothing is waited for).
    ring      an int32 CUDA tensor with one image row per row of the batch, e.g. the INPUT's column 4 as int32 beside an aligned result (a
              scattered row moves along its own beam and keeps its channel); rows whose ring is outside 0 .. height - 1 are unusable.
    keep      an input keep mask as the aligned calls take it (with a result: ANDed with the result's own).
    out       a RangeImageBatch to write into (RangeImageBatch.empty): every element is written, nothing needs clearing.
    return_count   also fill `count`.

    Returns a RangeImageBatch; its to_rows() carries a per-pixel prediction back to the rows.  Asynchronous on torch's current stream;
    nothing is read on the host: capturable after one warm-up call."""
    import torch
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError("range_image: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.range_image.project)")
    for name, v in (("height", height), ("width", width), ("num_features", num_features)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"range_image: {name} must be an integer")
    limits = np.asarray(range_limits, np.float64).reshape(-1)
    if limits.shape != (2,):
        raise ValueError("range_image: range_limits holds 2 numbers (lo, hi)")
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    H, W, C = int(height), int(width), int(num_features)
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    if ring is not None and not (torch.is_tensor(ring) and ring.dtype == torch.int32 and ring.dim() == 1 and ring.shape[0] == n and ring.device == dev and
                                 ring.is_contiguous()):
        raise ValueError("range_image: ring must be a contiguous int32 tensor with one element per row of the batch, on the device of the rows")
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 3 <= C <= 5:
        raise ValueError("range_image: n_features must be 3, 4 or 5: the columns of a row that a pixel stores")
    if H < 1 or W < 1:
        raise ValueError("range_image: height and width must be at least 1")
    if nf * H * W > 2 ** 31 - 1:
        raise ValueError("range_image: n_frames * height * width exceeds 2^31 - 1; split the batch")
    if out is None:
        out = RangeImageBatch.empty(nf, H, W, n, C, rows.dtype, dev, return_count)
    else:
        want = (("image", (nf, 1 + C, H, W), rows.dtype), ("index", (nf, H, W), torch.int32), ("pixel_of", (n,), torch.int32)) + \
               ((("count", (nf, H, W), torch.int32),) if return_count else ())
        for name, shape, dtype in want:
            t = getattr(out, name, None) if isinstance(out, RangeImageBatch) else None
            if not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev):
                raise ValueError(f"range_image: out must be a RangeImageBatch whose {name} is a contiguous {tuple(shape)} {dtype} tensor on the device of the rows")
    count = out.count if return_count else None
    by_ring = ring is not None and n > 0          # (without a row there is no channel to read: either mode writes the empty image)
    fov = None if by_ring else np.radians(np.array([fov_up, fov_down], np.float64))
    up = _uploads(eng)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        d_off = up.get(torch, dev, offsets, run)
        eng.ctx.range_image_device(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr() if n else 0, 0 if rows.dtype == torch.float32 else 1,
                                   H, W, fov, ring.data_ptr() if by_ring else 0, limits, C, 0 if keep is None or not n else keep.data_ptr(),
                                   out.image.data_ptr(), out.index.data_ptr(), out.pixel_of.data_ptr() if n else 0, 0 if count is None else count.data_ptr(),
                                   run.cuda_stream)
    return out if return_count or out.count is None else RangeImageBatch(out.image, out.index, out.pixel_of)


class NearestBatch:
    """What nearest_keypoints() leaves behind, N = rows of the batch, k = neighbours, K = centres per frame -- every shape static: `index`
    (N, k int32: per row its k nearest usable centres of its frame by (squared distance, centre number), as centre numbers 0 .. K - 1
    WITHIN THE FRAME; -1 in a slot beyond the frame's usable centres and in every slot of an absent or unusable row), `dist2` (N, k; the
    rows' dtype; +inf where the index is -1) and `weight` (N, k; the rows' dtype: pointnet2's normalised 1 / (dist + 1e-8); 0 where the
    index is -1; None unless asked for).  `offsets` (host) and `n_centres` say which frame a row belongs to and how many centres a frame
    has: flat_index(), interpolate() and nearest() are the way back from per-keypoint values to the rows -- pure indexing, no kernel of
    this library.  All still being written until the stream the call was made on has caught up."""

    def __init__(self, index, dist2, weight=None, offsets=None, n_centres=0):
        self.index, self.dist2, self.weight, self.n_centres = index, dist2, weight, int(n_centres)
        self.offsets = np.array([0, index.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
        self._base = None

    @classmethod
    def empty(cls, offsets, n_centres, k=3, dtype=None, device=None, with_weights=True):
        """Uninitialised buffers of the shapes nearest_keypoints() writes for a batch with these frame offsets (or, for one frame, this
        number of rows) (out=): static addresses for a captured graph."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
        off = np.array([0, int(offsets)], np.int64) if np.ndim(offsets) == 0 else np.asarray(offsets, np.int64)
        n, dt = int(off[-1]), dtype or torch.float32
        return cls(torch.empty((n, int(k)), dtype=torch.int32, device=dev), torch.empty((n, int(k)), dtype=dt, device=dev),
                   torch.empty((n, int(k)), dtype=dt, device=dev) if with_weights else None, off, n_centres)

    def flat_index(self):
        """index + frame * K, -1 kept (N, k int64): gathers from per-keypoint values flattened to (F K, ...).  The first call of a batch of
        several frames uploads their row counts (a few bytes; make it before capturing a graph); later calls reuse the result."""
        import torch
        idx = self.index.long()
        if len(self.offsets) <= 2:
            return idx
        if self._base is None:
            counts = torch.from_numpy(np.diff(self.offsets)).to(idx.device)
            first = torch.arange(len(counts), device=idx.device) * self.n_centres
            self._base = torch.repeat_interleave(first, counts, output_size=int(self.offsets[-1]))[:, None]
        return torch.where(idx >= 0, idx + self._base, idx)

    def _values(self, values, what):
        import torch
        F, K = len(self.offsets) - 1, self.n_centres
        if not (torch.is_tensor(values) and values.dim() in (2, 3) and tuple(values.shape[:2]) == (F, K) and values.device == self.index.device):
            raise ValueError(f"{what}: values must be a ({F}, {K}) or ({F}, {K}, D) tensor on the device of the rows: one value, or D of them, per keypoint")
        return values.reshape(F * K, -1) if values.dim() == 3 else values.reshape(F * K)

    def interpolate(self, features):
        """three_interpolate: per-keypoint features (F, K, D) or (F, K) as per-row features (N, D) or (N,): the sum over the slots of
        weight * features[index], in the features' dtype.  A row without a neighbour gets 0."""
        if self.weight is None:
            raise ValueError("interpolate: this NearestBatch has no weights (nearest_keypoints(..., return_weights=True))")
        flat = self._values(features, "interpolate")
        at = self.flat_index().clamp(min=0)               # (the weight of a -1 slot is 0)
        w = self.weight.to(flat.dtype)
        return (flat[at] * (w[..., None] if flat.dim() == 2 else w)).sum(dim=1)

    def nearest(self, values, default=0):
        """Voronoi labelling: every row gets the value of its nearest keypoint (slot 0) from per-keypoint values (F, K) or (F, K, D) --
        a keypoint-level keep decision becomes a per-row mask for augment_batch(..., keep=) or dror_keep(..., keep=); `default` for a
        row without a neighbour."""
        import torch
        flat = self._values(values, "nearest")
        first = self.flat_index()[:, 0]
        got = flat[first.clamp(min=0)]
        has = first >= 0
        return torch.where(has[:, None] if got.dim() == 2 else has, got, torch.full_like(got, default))


def nearest_keypoints(frames, centres, k=3, *, point_cloud_range=None, keep=None, out=None, return_weights=True, device=None, slot=0):
    """The k nearest centres of every row on the device (snowgpu_nearest_centres_device; the definition: include/snowgpu.h): pointnet2's
    three_nn with its interpolation weights, the way back from keypoints to the rows of the batch.  A row takes part if it is present,
    within 1e6 of the origin on every axis and inside point_cloud_range (None: no range); its neighbours are the usable centres of its
    frame in the order of (squared distance in the rows' dtype, centre number).

    frames    what ball_query takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult: its rows, offsets and
              keep mask are used (nothing is waited for).
    centres   a KeypointBatch (its points), or an (F, K, 3 .. 5) tensor in the rows' dtype on their device: x, y, z first.
    k         1 .. 8 neighbours per row.
    keep      an input keep mask as the aligned calls take it (with a result: ANDed with the result's own).
    out       a NearestBatch to write into (NearestBatch.empty): every element is written, nothing needs clearing.
    return_weights   also fill `weight`.

    Returns a NearestBatch; its interpolate() and nearest() carry per-keypoint values back to the rows.  Asynchronous on torch's current
    stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError("nearest_keypoints: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.nearest.three_nn)")
    if isinstance(k, bool) or int(k) != k:
        raise ValueError("nearest_keypoints: k must be an integer")
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError("nearest_keypoints: k must lie in 1 .. 8")
    rng = None
    if point_cloud_range is not None:
        rng = np.asarray(point_cloud_range, np.float64).reshape(-1)
        if rng.shape != (6,):
            raise ValueError("nearest_keypoints: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)")
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    cen = centres.points if isinstance(centres, KeypointBatch) else centres
    if not (torch.is_tensor(cen) and cen.dim() == 3 and cen.shape[0] == nf and cen.dtype == rows.dtype and cen.device == dev and cen.is_contiguous()):
        raise ValueError("nearest_keypoints: centres must be a KeypointBatch or a contiguous (frames, K, 3 .. 5) tensor in the rows' dtype on their device")
    K, Cq = int(cen.shape[1]), int(cen.shape[2])
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 3 <= Cq <= 5:
        raise ValueError("nearest_keypoints: centre_features must be 3, 4 or 5: x, y, z first (centres)")
    if K < 1:
        raise ValueError("nearest_keypoints: n_centres must be at least 1 (centres)")
    if nf * K > 2 ** 31 - 1:
        raise ValueError("nearest_keypoints: n_frames * n_centres exceeds 2^31 - 1; split the batch")
    if out is None:
        out = NearestBatch.empty(offsets, K, k, rows.dtype, dev, return_weights)
    else:
        want = (("index", torch.int32), ("dist2", rows.dtype)) + ((("weight", rows.dtype),) if return_weights else ())
        for name, dtype in want:
            t = getattr(out, name, None) if isinstance(out, NearestBatch) else None
            if not (torch.is_tensor(t) and tuple(t.shape) == (n, k) and t.dtype == dtype and t.is_contiguous() and t.device == dev):
                raise ValueError(f"nearest_keypoints: out must be a NearestBatch whose {name} is a contiguous {(n, k)} {dtype} tensor on the device of the rows")
    weight = out.weight if return_weights else None
    up = _uploads(eng)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        d_off = up.get(torch, dev, offsets, run)
        eng.ctx.nearest_centres_device(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr() if n else 0, 0 if rows.dtype == torch.float32 else 1,
                                       rng, K, cen.data_ptr(), Cq, k, 0 if keep is None or not n else keep.data_ptr(), out.index.data_ptr() if n else 0,
                                       out.dist2.data_ptr() if n else 0, 0 if weight is None or not n else weight.data_ptr(), run.cuda_stream)
    same = out.n_centres == K and np.array_equal(out.offsets, np.asarray(offsets, np.int64)) and (weight is None) == (out.weight is None)
    return out if same else NearestBatch(out.index, out.dist2, weight, offsets, K)


class BoxLabelBatch:
    """What points_in_boxes() leaves behind, N = rows of the batch, F = frames, B = boxes per frame -- every shape static: `box_of` (N
    int32: the smallest present box number of the row's frame that contains the row, 0 .. B - 1; -1 for a row in no box and for an absent
    or unusable row), `count` (F, B int32: the usable rows inside every box, overlaps included, 0 for an absent box; None unless asked
    for), `local` (N, 3 in the rows' dtype: the row in the frame of its box -- along its length, its width, and up from its centre; zeros
    where box_of is -1; None unless asked for) and `pose` (F, B, 2 float64: the (cos, sin) of the heading that was used, (0, 0) for an
    absent box; None unless asked for).  `offsets` (host) and `n_boxes` say which frame a row belongs to: flat_index(), labels(),
    keep_boxes() and rows_in() are pure indexing, no kernel of this library.  All still being written until the stream the call was made
    on has caught up."""

    def __init__(self, box_of, count, local=None, pose=None, offsets=None, n_boxes=0):
        self.box_of, self.count, self.local, self.pose, self.n_boxes = box_of, count, local, pose, int(n_boxes)
        self.offsets = np.array([0, box_of.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
        self._base = None

    @classmethod
    def empty(cls, offsets, n_boxes, dtype=None, device=None, with_count=True, with_local=False, with_pose=False):
        """Uninitialised buffers of the shapes points_in_boxes() writes for a batch with these frame offsets (or, for one frame, this
        number of rows) (out=): static addresses for a captured graph."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
        off = np.array([0, int(offsets)], np.int64) if np.ndim(offsets) == 0 else np.asarray(offsets, np.int64)
        n, nf, B = int(off[-1]), len(off) - 1, int(n_boxes)
        return cls(torch.empty(n, dtype=torch.int32, device=dev), torch.empty((nf, B), dtype=torch.int32, device=dev) if with_count else None,
                   torch.empty((n, 3), dtype=dtype or torch.float32, device=dev) if with_local else None,
                   torch.empty((nf, B, 2), dtype=torch.float64, device=dev) if with_pose else None, off, B)

    def flat_index(self):
        """box_of + frame * B, -1 kept (N int64): gathers from per-box values flattened to (F B, ...).  The first call of a batch of
        several frames uploads their row counts (a few bytes; make it before capturing a graph); later calls reuse the result."""
        import torch
        idx = self.box_of.long()
        if len(self.offsets) <= 2:
            return idx
        if self._base is None:
            counts = torch.from_numpy(np.diff(self.offsets)).to(idx.device)
            first = torch.arange(len(counts), device=idx.device) * self.n_boxes
            self._base = torch.repeat_interleave(first, counts, output_size=int(self.offsets[-1]))
        return torch.where(idx >= 0, idx + self._base, idx)

    def labels(self, per_box, background=0):
        """Per-box values (F, B) or (F, B, D) -- the class column of gt_boxes, say -- as per-row values (N,) or (N, D): the value of the
        row's box, `background` for a row in no box.  The point heads' point_cls_labels."""
        import torch
        F, B = len(self.offsets) - 1, self.n_boxes
        if not (torch.is_tensor(per_box) and per_box.dim() in (2, 3) and tuple(per_box.shape[:2]) == (F, B) and per_box.device == self.box_of.device):
            raise ValueError(f"labels: per_box must be a ({F}, {B}) or ({F}, {B}, D) tensor on the device of the rows: one value, or D of them, per box")
        flat = per_box.reshape(F * B, -1) if per_box.dim() == 3 else per_box.reshape(F * B)
        at = self.flat_index()
        got = flat[at.clamp(min=0)]
        has = at >= 0
        return torch.where(has[:, None] if got.dim() == 2 else has, got, torch.full_like(got, background))

    def keep_boxes(self, min_points=1):
        """(F, B) bool: count >= min_points, min_points >= 1 -- filter_by_min_points after the augmentation; an absent box is never kept."""
        if self.count is None:
            raise ValueError("keep_boxes: this BoxLabelBatch has no count (points_in_boxes(..., return_count=True))")
        if isinstance(min_points, bool) or int(min_points) != min_points or int(min_points) < 1:
            raise ValueError("keep_boxes: min_points must be an integer of at least 1")
        return self.count >= int(min_points)

    def rows_in(self, box_mask=None):
        """(N,) bool: the rows inside a box -- with box_mask (F, B bool), inside a box whose entry is set, judged by the row's own box
        (box_of).  A keep mask for augment_batch(..., keep=) or dror_keep(..., keep=); its negation clears a pasted object's place."""
        import torch
        if box_mask is None:
            return self.box_of >= 0
        F, B = len(self.offsets) - 1, self.n_boxes
        if not (torch.is_tensor(box_mask) and box_mask.dtype == torch.bool and tuple(box_mask.shape) == (F, B) and box_mask.device == self.box_of.device):
            raise ValueError(f"rows_in: box_mask must be a ({F}, {B}) bool tensor on the device of the rows")
        at = self.flat_index()
        return (at >= 0) & box_mask.reshape(F * B)[at.clamp(min=0)]


def points_in_boxes(frames, boxes, *, pose=None, keep=None, out=None, return_count=True, return_local=False, return_pose=False, device=None, slot=0):
    """The box of every row and the rows of every box on the device (snowgpu_points_in_boxes_device; the definition: include/snowgpu.h):
    roiaware_pool3d's points_in_boxes_gpu with check_pt_in_box3d's faces -- z closed, x and y strict with the 1e-5 margin -- in float64.
    A row takes part if it is present and within 1e6 of the origin on every axis.

    frames    what nearest_keypoints takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult: its rows,
              offsets and keep mask are used (nothing is waited for).
    boxes     a contiguous (F, B, 7 .. 10) tensor in the rows' dtype on their device, 1 <= B <= 256: cx, cy, cz, dx, dy, dz, heading
              first (OpenPCDet's gt_boxes; its zero rows are absent boxes).
    pose      None: cos / sin of the heading in float64 on the device; or a contiguous (F, B, 2) float64 tensor (cos, sin) used as it is.
    keep      an input keep mask as the aligned calls take it (with a result: ANDed with the result's own).
    out       a BoxLabelBatch to write into (BoxLabelBatch.empty): every element is written, nothing needs clearing.

    Returns a BoxLabelBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError("points_in_boxes: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.boxes.points_in_boxes)")
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    if not (torch.is_tensor(boxes) and boxes.dim() == 3 and boxes.shape[0] == nf and boxes.dtype == rows.dtype and boxes.device == dev and boxes.is_contiguous()):
        raise ValueError("points_in_boxes: boxes must be a contiguous (frames, B, 7 .. 10) tensor in the rows' dtype on their device")
    B, Cb = int(boxes.shape[1]), int(boxes.shape[2])
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 1 <= B <= 256:
        raise ValueError("points_in_boxes: n_boxes must lie in 1 .. 256 (boxes)")
    if not 7 <= Cb <= 10:
        raise ValueError("points_in_boxes: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (boxes)")
    if pose is not None and not (torch.is_tensor(pose) and tuple(pose.shape) == (nf, B, 2) and pose.dtype == torch.float64 and pose.device == dev and pose.is_contiguous()):
        raise ValueError(f"points_in_boxes: pose must be a contiguous {(nf, B, 2)} float64 tensor (cos, sin) on the device of the rows")
    want = (("box_of", torch.int32, (n,), True), ("count", torch.int32, (nf, B), return_count), ("local", rows.dtype, (n, 3), return_local),
            ("pose", torch.float64, (nf, B, 2), return_pose))
    if out is None:
        out = BoxLabelBatch.empty(offsets, B, rows.dtype, dev, return_count, return_local, return_pose)
    else:
        for name, dtype, shape, asked in want:
            t = getattr(out, name, None) if isinstance(out, BoxLabelBatch) else None
            if asked and not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev):
                raise ValueError(f"points_in_boxes: out must be a BoxLabelBatch whose {name} is a contiguous {shape} {dtype} tensor on the device of the rows")
    count, local, used = (out.count if return_count else None), (out.local if return_local else None), (out.pose if return_pose else None)
    up = _uploads(eng)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        d_off = up.get(torch, dev, offsets, run)
        eng.ctx.points_in_boxes_device(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr() if n else 0, 0 if rows.dtype == torch.float32 else 1,
                                       B, boxes.data_ptr(), Cb, 0 if pose is None else pose.data_ptr(), 0 if keep is None or not n else keep.data_ptr(),
                                       out.box_of.data_ptr() if n else 0, 0 if count is None else count.data_ptr(),
                                       0 if local is None or not n else local.data_ptr(), 0 if used is None else used.data_ptr(), run.cuda_stream)
    same = (out.n_boxes == B and np.array_equal(out.offsets, np.asarray(offsets, np.int64)) and (count is None) == (out.count is None) and
            (local is None) == (out.local is None) and (used is None) == (out.pose is None))
    return out if same else BoxLabelBatch(out.box_of, count, local, used, offsets, B)


IOU_MODES = {"bev": 0, "3d": 1}


def _box_set(torch, who, name, boxes, limit, like=None):
    """(F, B, Cb) of a box tensor after the checks the box entries share."""
    if not (torch.is_tensor(boxes) and boxes.is_cuda and boxes.dim() == 3 and boxes.dtype in (torch.float32, torch.float64) and boxes.is_contiguous()):
        raise ValueError(f"{who}: {name} must be a contiguous (frames, B, 7 .. 10) float32 or float64 CUDA tensor")
    if like is not None and not (boxes.dtype == like.dtype and boxes.device == like.device and boxes.shape[0] == like.shape[0]):
        raise ValueError(f"{who}: {name} must have the frames, the dtype and the device of the other boxes")
    F, B, Cb = (int(v) for v in boxes.shape)
    if F < 1 or not 1 <= B <= limit:
        raise ValueError(f"{who}: the boxes per frame must lie in 1 .. {limit}, the frames be at least 1 ({name})")
    if not 7 <= Cb <= 10:
        raise ValueError(f"{who}: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first ({name})")
    return F, B, Cb


def _box_pose(torch, who, name, pose, boxes):
    shape = tuple(boxes.shape[:2]) + (2,)
    if pose is not None and not (torch.is_tensor(pose) and tuple(pose.shape) == shape and pose.dtype == torch.float64 and pose.device == boxes.device and pose.is_contiguous()):
        raise ValueError(f"{who}: {name} must be a contiguous {shape} float64 tensor (cos, sin) on the device of the boxes")
    return 0 if pose is None else pose.data_ptr()


def _checked_out(torch, who, kind, out, want, dev):
    for name, dtype, shape, asked in want:
        t = getattr(out, name, None) if isinstance(out, kind) else None
        if asked and not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev):
            raise ValueError(f"{who}: out must be a {kind.__name__} whose {name} is a contiguous {shape} {dtype} tensor on the device of the boxes")


class IouBatch:
    """What boxes_iou() leaves behind, F frames, M boxes a and B boxes b per frame -- every shape static: `iou` (F, M, B in the boxes' dtype:
    the IoU of a_m with b_b, 0 where either is absent; None unless asked for), `best` (F, M int32: the smallest b with the largest IoU of
    a_m if that IoU is > 0, else -1 -- the target layer's gt_assignment; None unless asked for) and `best_iou` (F, M: that IoU, 0 where best
    is -1 -- max_overlaps).  All still being written until the stream the call was made on has caught up."""

    def __init__(self, iou=None, best=None, best_iou=None):
        self.iou, self.best, self.best_iou = iou, best, best_iou

    @classmethod
    def empty(cls, n_frames, n_a, n_b, dtype=None, device=None, with_iou=True, with_best=False):
        """Uninitialised buffers of the shapes boxes_iou() writes (out=): static addresses for a captured graph."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
        F, M, B, dt = int(n_frames), int(n_a), int(n_b), dtype or torch.float32
        return cls(torch.empty((F, M, B), dtype=dt, device=dev) if with_iou else None, torch.empty((F, M), dtype=torch.int32, device=dev) if with_best else None,
                   torch.empty((F, M), dtype=dt, device=dev) if with_best else None)


def boxes_iou(boxes_a, boxes_b, *, mode='3d', pose_a=None, pose_b=None, out=None, return_iou=True, return_best=False, slot=0):
    """The rotated IoU of every box of `boxes_a` with every box of `boxes_b` of its frame on the device (snowgpu_boxes_iou_device; the
    definition: include/snowgpu.h): pcdet's boxes_iou3d_gpu (mode '3d') and boxes_iou_bev (mode 'bev') in float64 by clipping in a fixed
    order, and the best partner of every box a without materialising the matrix.

    boxes_a   a contiguous (F, M, 7 .. 10) float32 or float64 CUDA tensor, 1 <= M <= 9216: cx, cy, cz, dx, dy, dz, heading first (rois; the
              `boxes` of an NmsBatch as they stand: zero rows are absent boxes).
    boxes_b   (F, B, 7 .. 10) likewise, same dtype and device, 1 <= B <= 9216 (gt_boxes); F M B < 2^31.
    pose_a, pose_b   None: cos / sin of the heading in float64 on the device; or contiguous (F, M, 2) / (F, B, 2) float64 tensors used as they are.
    out       an IouBatch to write into (IouBatch.empty): every element is written.
    return_iou, return_best   which outputs to compute; at least one.
    The records of the boxes are scratch of the engine of `slot`, shared by nms() and boxes_iou(): calls made on streams that are not ordered
    against each other (torch's default stream runs on a side stream of the engine) need a `slot` each.

    Returns an IouBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    from . import engine as _engine
    who = "boxes_iou"
    F, M, Ca = _box_set(torch, who, "boxes_a", boxes_a, 9216)
    _, B, Cb = _box_set(torch, who, "boxes_b", boxes_b, 9216, boxes_a)
    if mode not in IOU_MODES:
        raise ValueError(f"{who}: mode must be 'bev' or '3d'")
    if not (return_iou or return_best):
        raise ValueError(f"{who}: nothing to compute: return_iou or return_best")
    if F * M * B > 2 ** 31 - 1:
        raise ValueError(f"{who}: frames * M * B exceeds 2^31 - 1; split the batch")
    dev, dt = boxes_a.device, boxes_a.dtype
    pa, pb = _box_pose(torch, who, "pose_a", pose_a, boxes_a), _box_pose(torch, who, "pose_b", pose_b, boxes_b)
    want = (("iou", dt, (F, M, B), return_iou), ("best", torch.int32, (F, M), return_best), ("best_iou", dt, (F, M), return_best))
    if out is None:
        out = IouBatch.empty(F, M, B, dt, dev, return_iou, return_best)
    else:
        _checked_out(torch, who, IouBatch, out, want, dev)
    iou, best, best_iou = (out.iou if return_iou else None), (out.best if return_best else None), (out.best_iou if return_best else None)
    eng = _engine.get_engine(dev.index, slot)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        eng.ctx.boxes_iou_device(F, M, boxes_a.data_ptr(), Ca, B, boxes_b.data_ptr(), Cb, 0 if dt == torch.float32 else 1, IOU_MODES[mode], pa, pb,
                                 0 if iou is None else iou.data_ptr(), 0 if best is None else best.data_ptr(), 0 if best_iou is None else best_iou.data_ptr(),
                                 run.cuda_stream)
    same = (iou is None) == (out.iou is None) and (best is None) == (out.best is None)
    return out if same else IouBatch(iou, best, best_iou)


class NmsBatch:
    """What nms() leaves behind, F frames of B boxes, P = post_max -- every shape static: `index` (F, P int32: the kept box numbers in rank
    order, -1 behind the count), `count` (F int32), `boxes` (F, P, Cb in the boxes' dtype: the kept boxes with all their columns and ZERO
    rows behind the count -- rois for sample_keypoints(rois=), boxes for points_in_boxes and boxes_iou as they stand; None unless asked
    for), `scores` (F, P: their scores, 0 behind the count; None unless asked for) and `kept` (F, B uint8: 1 for a kept box; None unless
    asked for).  All still being written until the stream the call was made on has caught up."""

    def __init__(self, index, count, boxes=None, scores=None, kept=None):
        self.index, self.count, self.boxes, self.scores, self.kept = index, count, boxes, scores, kept

    @classmethod
    def empty(cls, n_frames, n_boxes, post_max, box_features=7, dtype=None, device=None, with_boxes=True, with_scores=False, with_kept=False):
        """Uninitialised buffers of the shapes nms() writes (out=): static addresses for a captured graph."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
        F, B, P, dt = int(n_frames), int(n_boxes), int(post_max), dtype or torch.float32
        return cls(torch.empty((F, P), dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev),
                   torch.empty((F, P, int(box_features)), dtype=dt, device=dev) if with_boxes else None,
                   torch.empty((F, P), dtype=dt, device=dev) if with_scores else None, torch.empty((F, B), dtype=torch.uint8, device=dev) if with_kept else None)


def nms(boxes, scores, iou_thresh, *, post_max, score_thresh=-math.inf, mode='bev', pose=None, out=None, return_boxes=True, return_scores=False,
        return_kept=False, slot=0):
    """Class-agnostic rotated NMS per frame on the device (snowgpu_nms_device; the definition: include/snowgpu.h): pcdet's nms_gpu without
    its host sweep.  The present boxes whose score is not NaN and is >= score_thresh are ranked by score (the smallest number first among
    equals); a candidate is suppressed iff an already kept box has IoU > iou_thresh with it; the walk stops after post_max kept.

    boxes     a contiguous (F, B, 7 .. 10) float32 or float64 CUDA tensor, 1 <= B <= 9216 (take torch.topk first, as pcdet does).
    scores    a contiguous (F, B) tensor of the same dtype and device.
    post_max  1 .. B: the static length of the keep list.
    mode      'bev' (nms_gpu) or '3d'.
    pose      None, or a contiguous (F, B, 2) float64 tensor (cos, sin) used as it is.
    out       an NmsBatch to write into (NmsBatch.empty): every element is written.
    The records of the boxes are scratch of the engine of `slot`, shared by nms() and boxes_iou(): calls made on streams that are not ordered
    against each other (torch's default stream runs on a side stream of the engine) need a `slot` each.

    Returns an NmsBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    from . import engine as _engine
    who = "nms"
    F, B, Cb = _box_set(torch, who, "boxes", boxes, 9216)
    dev, dt = boxes.device, boxes.dtype
    if not (torch.is_tensor(scores) and tuple(scores.shape) == (F, B) and scores.dtype == dt and scores.device == dev and scores.is_contiguous()):
        raise ValueError(f"{who}: scores must be a contiguous {(F, B)} tensor in the boxes' dtype on their device")
    if mode not in IOU_MODES:
        raise ValueError(f"{who}: mode must be 'bev' or '3d'")
    if isinstance(post_max, bool) or int(post_max) != post_max or not 1 <= int(post_max) <= B:
        raise ValueError(f"{who}: post_max must be an integer in 1 .. B")
    if math.isnan(float(iou_thresh)) or math.isnan(float(score_thresh)):
        raise ValueError(f"{who}: a threshold is NaN")
    P = int(post_max)
    pp = _box_pose(torch, who, "pose", pose, boxes)
    want = (("index", torch.int32, (F, P), True), ("count", torch.int32, (F,), True), ("boxes", dt, (F, P, Cb), return_boxes),
            ("scores", dt, (F, P), return_scores), ("kept", torch.uint8, (F, B), return_kept))
    if out is None:
        out = NmsBatch.empty(F, B, P, Cb, dt, dev, return_boxes, return_scores, return_kept)
    else:
        _checked_out(torch, who, NmsBatch, out, want, dev)
    kb, ks, kk = (out.boxes if return_boxes else None), (out.scores if return_scores else None), (out.kept if return_kept else None)
    eng = _engine.get_engine(dev.index, slot)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        eng.ctx.nms_device(F, B, boxes.data_ptr(), Cb, scores.data_ptr(), 0 if dt == torch.float32 else 1, IOU_MODES[mode], float(iou_thresh), float(score_thresh),
                           P, pp, out.index.data_ptr(), out.count.data_ptr(), 0 if kb is None else kb.data_ptr(), 0 if ks is None else ks.data_ptr(),
                           0 if kk is None else kk.data_ptr(), run.cuda_stream)
    same = (kb is None) == (out.boxes is None) and (ks is None) == (out.scores is None) and (kk is None) == (out.kept is None)
    return out if same else NmsBatch(out.index, out.count, kb, ks, kk)


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
