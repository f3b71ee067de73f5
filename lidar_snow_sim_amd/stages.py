"""The device stages of the torch-tensor boundary (tensors.py is the documented import path and lists what each is for) and the batches
of static shape they leave behind: fov_keep, dror_keep, voxelize, sample_keypoints, ball_query, range_image, nearest_keypoints,
points_in_boxes, boxes_iou, nms, roi_point_pool, roi_voxel_pool, sample_rois, assign_anchors, assign_centers, paste_objects, transform_scene.  Every stage goes through the same steps, in this order -- it is the order in which a call that is wrong
in two ways is refused: the aligned unwrap and the device-input refusal (_stage_frames), the scalar and range checks (_whole, _range6),
the batch and its keep mask (_stage_batch), the stage's own tensors, the checks of the shapes' domain, out= (_checked_out), the launch
(_stage_launch).  PyTorch is plumbing here; the work is the C entries'."""
from __future__ import annotations

import math

import numpy as np

from .batch import (_checked_out, _cuda_device, _keep_mask, _on_run_stream, _range6, _resolve_input, _stage_batch, _stage_frames, _stage_launch,
                    _whole, is_device_input)

_ROWS = "rows"               # (the last word of an out= refusal: the seven row stages' tensors share the device of the rows)


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
    import torch
    frames, keep = _stage_frames(torch, "dror_keep", "lidar_snow_sim_amd.dror.dynamic_radius_outlier_filter", frames, keep)
    c = float(beta) * (float(alpha) * (math.pi / 180.0))
    if not (0.0 < c <= 0.25):
        raise ValueError("dror_keep: beta * radians(alpha) must lie in (0, 0.25]")
    if not (float(sr_min) >= 0.0 and math.isfinite(float(sr_min))):
        raise ValueError("dror_keep: sr_min must be finite and >= 0")
    if int(k_min) != k_min or not (0 <= int(k_min) <= 65535):
        raise ValueError("dror_keep: k_min must be an integer in 0 .. 65535")
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
    if out is None:
        out = torch.empty(n, dtype=torch.bool, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.bool and out.dim() == 1 and out.shape[0] == n and out.is_contiguous() and out.device == dev):
        raise ValueError("dror_keep: out must be a contiguous torch.bool tensor with one element per row, on the device of the rows")
    if keep is not None and n and out.data_ptr() < keep.data_ptr() + n and keep.data_ptr() < out.data_ptr() + n:
        raise ValueError("dror_keep: out must not be (or overlap) the keep tensor; the query of one row reads other rows' keep elements")
    nb = torch.zeros(n, dtype=torch.int32, device=dev) if return_neighbours else None
    if nf and n:
        _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.dror_mask_device, float(alpha), float(beta), float(sr_min), int(k_min),
                      0 if keep is None else keep.data_ptr(), out.data_ptr(), 0 if nb is None else nb.data_ptr())
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
        dev = _cuda_device(torch, device)
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
    who = "voxelize"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.voxel.points_to_voxels", frames, keep)
    _whole(who, max_points=max_points, max_voxels=max_voxels, num_features=num_features)
    rng, size = np.asarray(point_cloud_range, np.float64).reshape(-1), np.asarray(voxel_size, np.float64).reshape(-1)
    if rng.shape != (6,) or size.shape != (3,):                  # (not _range6: the range is no option here, and the sentence names the size too)
        raise ValueError("voxelize: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1), voxel_size 3")
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
    T, V, C = int(max_points), int(max_voxels), int(num_features)
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
        _checked_out(torch, who, VoxelBatch, out, (("voxels", rows.dtype, (nf * V, T, C), True), ("coords", torch.int32, (nf * V, 4), True),
                                                   ("num_points", torch.int32, (nf * V,), True), ("voxel_offsets", torch.int32, (nf + 1,), True),
                                                   ("voxel_of", torch.int32, (n,), return_voxel_of)), dev, _ROWS)
    vof = out.voxel_of if return_voxel_of else None
    if n == 0:                                          # no row: the entry writes the offsets alone
        out.voxels.zero_(); out.coords.fill_(-1); out.num_points.zero_()
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.voxelize_device, rng, size, T, V, C, 0 if keep is None or not n else keep.data_ptr(),
                  out.voxels.data_ptr(), out.coords.data_ptr(), out.num_points.data_ptr(), out.voxel_offsets.data_ptr(),
                  0 if vof is None or not n else vof.data_ptr())
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
        dev = _cuda_device(torch, device)
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
    who = "sample_keypoints"
    plain = sectors is None and rois is None          # the plain walk; else the sectorized one, in one sector when only rois are given
    if not plain and sectors is None:
        sectors = 1
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.fps." + ("farthest_point_sample" if plain else "sectorized_sample"), frames, keep)
    _whole(who, n_samples=n_samples, num_features=num_features, **({} if plain else {"sectors": sectors}))
    rng = _range6(who, point_cloud_range)
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
    K, C, S = int(n_samples), int(num_features), None if plain else int(sectors)
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 3 <= C <= 5:
        raise ValueError("sample_keypoints: n_features must be 3, 4 or 5: the columns of a row that a keypoint carries")
    if K < 1:
        raise ValueError("sample_keypoints: n_samples must be at least 1")
    if nf * K > 2 ** 31 - 1:
        raise ValueError("sample_keypoints: n_frames * n_samples exceeds 2^31 - 1; split the batch")
    if not plain and not 1 <= S <= 16:
        raise ValueError("sample_keypoints: n_sectors must lie in 1 .. 16")
    B = Cb = 0
    if rois is not None:
        if not (torch.is_tensor(rois) and rois.is_cuda and rois.device == dev and rois.dtype == rows.dtype and rois.dim() == 3 and rois.shape[0] == nf
                and rois.is_contiguous()):
            raise ValueError("sample_keypoints: rois must be a contiguous (frames, B, 7 .. 10) tensor of the rows' dtype on the device of the rows")
        B, Cb = int(rois.shape[1]), int(rois.shape[2])
    return_sector_of = return_sector_of and not plain
    if out is None:
        out = KeypointBatch.empty(nf, K, C, rows.dtype, dev, return_dist, S, n if return_sector_of else None)
    else:
        want = (("index", torch.int32, (nf, K), True), ("points", rows.dtype, (nf, K, C), True), ("usable", torch.int32, (nf,), True)) + \
               (() if plain else (("sector_offsets", torch.int32, (nf, S + 1), True), ("sector_count", torch.int32, (nf, S), True))) + \
               (("dist", rows.dtype, (nf, K), return_dist), ("sector_of", torch.int8, (n,), return_sector_of))
        _checked_out(torch, who, KeypointBatch, out, want, dev, _ROWS)
    dist = out.dist if return_dist else None
    sof = out.sector_of if return_sector_of else None
    if plain:
        _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.fps_device, rng, K, C, 0 if keep is None or not n else keep.data_ptr(),
                      out.index.data_ptr(), out.points.data_ptr(), 0 if dist is None else dist.data_ptr(), out.usable.data_ptr())
        return out if return_dist or out.dist is None else KeypointBatch(out.index, out.points, out.usable)
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.fps_sectors_device, rng, K, C, 0 if keep is None or not n else keep.data_ptr(), S,
                  0 if rois is None else rois.data_ptr(), B, Cb, roi_margin, out.index.data_ptr(), out.points.data_ptr(),
                  0 if dist is None else dist.data_ptr(), out.usable.data_ptr(), out.sector_offsets.data_ptr(), out.sector_count.data_ptr(),
                  0 if sof is None or not n else sof.data_ptr(), 0)
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
        dev = _cuda_device(torch, device)
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
    who = "ball_query"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.ball.ball_query", frames, keep)
    seq = lambda v: list(v) if isinstance(v, (tuple, list, np.ndarray)) else [v]
    radii, seg = seq(radius), seq(n_neighbours)
    if len(radii) != len(seg):
        raise ValueError("ball_query: as many radii as sample counts")
    _whole(who, num_features=num_features)
    for s in seg:
        _whole(who, n_neighbours=s)
    rng = _range6(who, point_cloud_range)
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
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
        _checked_out(torch, who, NeighbourBatch, out, (("index", torch.int32, (nf, K, S), True), ("count", torch.int32, (nf, K, R), True),
                                                       ("points", rows.dtype, (nf, K, S, C), return_points)), dev, _ROWS)
    points = out.points if return_points else None
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.ball_query_device, rng, K, cen.data_ptr(), Cq, radii, seg, C,
                  0 if keep is None or not n else keep.data_ptr(), out.index.data_ptr(), out.count.data_ptr(), 0 if points is None else points.data_ptr())
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
        dev = _cuda_device(torch, device)
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
    who = "range_image"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.range_image.project", frames, keep)
    _whole(who, height=height, width=width, num_features=num_features)
    limits = np.asarray(range_limits, np.float64).reshape(-1)
    if limits.shape != (2,):
        raise ValueError("range_image: range_limits holds 2 numbers (lo, hi)")
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
    H, W, C = int(height), int(width), int(num_features)
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
        _checked_out(torch, who, RangeImageBatch, out, (("image", rows.dtype, (nf, 1 + C, H, W), True), ("index", torch.int32, (nf, H, W), True),
                                                        ("pixel_of", torch.int32, (n,), True), ("count", torch.int32, (nf, H, W), return_count)), dev, _ROWS)
    count = out.count if return_count else None
    by_ring = ring is not None and n > 0          # (without a row there is no channel to read: either mode writes the empty image)
    fov = None if by_ring else np.radians(np.array([fov_up, fov_down], np.float64))
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.range_image_device, H, W, fov, ring.data_ptr() if by_ring else 0, limits, C,
                  0 if keep is None or not n else keep.data_ptr(), out.image.data_ptr(), out.index.data_ptr(), out.pixel_of.data_ptr() if n else 0,
                  0 if count is None else count.data_ptr())
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
        dev = _cuda_device(torch, device)
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
    who = "nearest_keypoints"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.nearest.three_nn", frames, keep)
    _whole(who, k=k)
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError("nearest_keypoints: k must lie in 1 .. 8")
    rng = _range6(who, point_cloud_range)
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
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
        _checked_out(torch, who, NearestBatch, out, (("index", torch.int32, (n, k), True), ("dist2", rows.dtype, (n, k), True),
                                                     ("weight", rows.dtype, (n, k), return_weights)), dev, _ROWS)
    weight = out.weight if return_weights else None
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.nearest_centres_device, rng, K, cen.data_ptr(), Cq, k,
                  0 if keep is None or not n else keep.data_ptr(), out.index.data_ptr() if n else 0, out.dist2.data_ptr() if n else 0,
                  0 if weight is None or not n else weight.data_ptr())
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
        dev = _cuda_device(torch, device)
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
    who = "points_in_boxes"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.boxes.points_in_boxes", frames, keep)
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
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
        _checked_out(torch, who, BoxLabelBatch, out, want, dev, _ROWS)
    count, local, used = (out.count if return_count else None), (out.local if return_local else None), (out.pose if return_pose else None)
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.points_in_boxes_device, B, boxes.data_ptr(), Cb, 0 if pose is None else pose.data_ptr(),
                  0 if keep is None or not n else keep.data_ptr(), out.box_of.data_ptr() if n else 0, 0 if count is None else count.data_ptr(),
                  0 if local is None or not n else local.data_ptr(), 0 if used is None else used.data_ptr())
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
        dev = _cuda_device(torch, device)
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
        dev = _cuda_device(torch, device)
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


class RoiPointBatch:
    """What roi_point_pool() leaves behind, F = frames, M = rois per frame, S = n_samples, C = num_features -- every shape static: `index`
    (F, M, S int32: the global row index of the roi's member j mod cnt, members in ascending row order -- pcdet's wrap-around fill; -1
    in every slot of an absent or empty roi), `count` (F, M int32: the members of the roi, NOT clipped at S; 0 for an absent roi), `points`
    (F, M, S, C in the rows' dtype: the first C columns of rows[index], zeros where index is -1; None unless asked for), `local` (F, M, S, 3:
    the row in the frame of its roi -- along its length, its width, and up from its centre --, zeros where index is -1; None unless asked
    for) and `pose` (F, M, 2 float64: the (cos, sin) of the heading that was used, (0, 0) for an absent roi; None unless asked for).
    gather() and labels() are pure indexing, no kernel of this library.  At F = 256, M = 128, S = 512 `index` is 67 MB and `points` at
    C = 4 float32 268 MB.  All still being written until the stream the call was made on has caught up."""

    def __init__(self, index, count, points=None, local=None, pose=None):
        self.index, self.count, self.points, self.local, self.pose = index, count, points, local, pose

    @classmethod
    def empty(cls, n_frames, n_rois, n_samples=512, num_features=4, dtype=None, device=None, with_points=True, with_local=False, with_pose=False):
        """Uninitialised buffers of the shapes roi_point_pool() writes (out=): static addresses for a captured graph."""
        import torch
        dev = _cuda_device(torch, device)
        F, M, S, C, dt = int(n_frames), int(n_rois), int(n_samples), int(num_features), dtype or torch.float32
        return cls(torch.empty((F, M, S), dtype=torch.int32, device=dev), torch.empty((F, M), dtype=torch.int32, device=dev),
                   torch.empty((F, M, S, C), dtype=dt, device=dev) if with_points else None,
                   torch.empty((F, M, S, 3), dtype=dt, device=dev) if with_local else None,
                   torch.empty((F, M, 2), dtype=torch.float64, device=dev) if with_pose else None)

    @property
    def empty_flag(self):
        """(F, M) bool: count == 0 -- roipoint_pool3d's pooled_empty_flag; an absent roi is empty."""
        return self.count == 0

    def gather(self, per_row):
        """Per-row values (N,) or (N, D) -- per-point features, the depth, the first stage's segmentation score -- as (F, M, S) or
        (F, M, S, D): the value of the pooled row, zeros where index is -1.  What joins `points` and `local` to pooled_features."""
        import torch
        if not (torch.is_tensor(per_row) and per_row.dim() in (1, 2) and per_row.device == self.index.device):
            raise ValueError("gather: per_row must be an (N,) or (N, D) tensor on the device of the rows: one value, or D of them, per row")
        at = self.index.long()
        got = per_row[at.clamp(min=0)]
        has = at >= 0
        return torch.where(has[..., None] if got.dim() == 4 else has, got, torch.zeros_like(got))

    def labels(self, box_labels):
        """box_labels.box_of[index] (F, M, S int32) with -1 kept: the points_in_boxes label of every pooled row."""
        import torch
        if not isinstance(box_labels, BoxLabelBatch) or box_labels.box_of.device != self.index.device:
            raise ValueError("labels: box_labels must be a BoxLabelBatch on the device of the rows")
        at = self.index.long()
        return torch.where(at >= 0, box_labels.box_of[at.clamp(min=0)], torch.full_like(self.index, -1))


def roi_point_pool(frames, rois, n_samples=512, *, extra_width=(0., 0., 0.), pose=None, keep=None, num_features=4, out=None, return_points=True,
                   return_local=False, return_pose=False, device=None, slot=0):
    """The first n_samples rows inside every slightly enlarged roi, in row order, on the device (snowgpu_roi_point_pool_device; the
    definition: include/snowgpu.h): pcdet's roipoint_pool3d as PointRCNNHead.roipool3d_gpu calls it, with points_in_boxes' membership test
    in float64 and static shapes.  A row takes part if it is present and within 1e6 of the origin on every axis.

    frames    what points_in_boxes takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult: its rows, offsets
              and keep mask are used (nothing is waited for).
    rois      a contiguous (F, M, 7 .. 10) tensor in the rows' dtype on their device, 1 <= M <= 512: cx, cy, cz, dx, dy, dz, heading
              first -- or an NmsBatch, whose `boxes` are used (the zero rows behind its count are absent rois).
    n_samples 1 .. 2048: S, the rows a roi stores; a roi of fewer members repeats them (slot j holds member j mod count).
    extra_width   a number or three (x, y, z), each in 0 .. 100: added once to dx, dy, dz (enlarge_box3d).
    pose      None: cos / sin of the heading in float64 on the device; or a contiguous (F, M, 2) float64 tensor (cos, sin) used as it is.
    keep      an input keep mask as the aligned calls take it (with a result: ANDed with the result's own).
    num_features  3, 4 or 5: the columns of a row that `points` stores.
    out       a RoiPointBatch to write into (RoiPointBatch.empty): every element is written, nothing needs clearing.

    Returns a RoiPointBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    who = "roi_point_pool"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.roipool.roipoint_pool3d", frames, keep)
    _whole(who, n_samples=n_samples, num_features=num_features)
    ew = np.asarray(extra_width, np.float64).reshape(-1)
    if ew.shape == (1,):
        ew = np.repeat(ew, 3)
    if ew.shape != (3,) or not ((ew >= 0.0) & (ew <= 100.0)).all():
        raise ValueError("roi_point_pool: extra_width is a number or three (x, y, z), each finite and in 0 .. 100")
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
    if isinstance(rois, NmsBatch):
        if rois.boxes is None:
            raise ValueError("roi_point_pool: this NmsBatch has no boxes (nms(..., return_boxes=True))")
        rois = rois.boxes
    if not (torch.is_tensor(rois) and rois.dim() == 3 and rois.shape[0] == nf and rois.dtype == rows.dtype and rois.device == dev and rois.is_contiguous()):
        raise ValueError("roi_point_pool: rois must be a contiguous (frames, M, 7 .. 10) tensor in the rows' dtype on their device, or an NmsBatch of such boxes")
    M, Cb, S, C = int(rois.shape[1]), int(rois.shape[2]), int(n_samples), int(num_features)
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 1 <= M <= 512:
        raise ValueError("roi_point_pool: n_rois must lie in 1 .. 512 (rois)")
    if not 7 <= Cb <= 10:
        raise ValueError("roi_point_pool: roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (rois)")
    if not 1 <= S <= 2048:
        raise ValueError("roi_point_pool: n_samples must lie in 1 .. 2048")
    if not 3 <= C <= 5:
        raise ValueError("roi_point_pool: num_features must be 3, 4 or 5: the columns of a row that a roi stores")
    if nf * M * S * max(C, 3) > 2 ** 31 - 1:
        raise ValueError("roi_point_pool: n_frames * n_rois * n_samples * max(num_features, 3) exceeds 2^31 - 1; split the batch")
    if pose is not None and not (torch.is_tensor(pose) and tuple(pose.shape) == (nf, M, 2) and pose.dtype == torch.float64 and pose.device == dev and pose.is_contiguous()):
        raise ValueError(f"roi_point_pool: pose must be a contiguous {(nf, M, 2)} float64 tensor (cos, sin) on the device of the rows")
    want = (("index", torch.int32, (nf, M, S), True), ("count", torch.int32, (nf, M), True), ("points", rows.dtype, (nf, M, S, C), return_points),
            ("local", rows.dtype, (nf, M, S, 3), return_local), ("pose", torch.float64, (nf, M, 2), return_pose))
    if out is None:
        out = RoiPointBatch.empty(nf, M, S, C, rows.dtype, dev, return_points, return_local, return_pose)
    else:
        _checked_out(torch, who, RoiPointBatch, out, want, dev, _ROWS)
    points, local, used = (out.points if return_points else None), (out.local if return_local else None), (out.pose if return_pose else None)
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.roi_point_pool_device, M, rois.data_ptr(), Cb, ew, S, C, 0 if pose is None else pose.data_ptr(),
                  0 if keep is None or not n else keep.data_ptr(), out.index.data_ptr(), out.count.data_ptr(), 0 if points is None else points.data_ptr(),
                  0 if local is None else local.data_ptr(), 0 if used is None else used.data_ptr())
    same = (points is None) == (out.points is None) and (local is None) == (out.local is None) and (used is None) == (out.pose is None)
    return out if same else RoiPointBatch(out.index, out.count, points, local, used)


class RoiVoxelBatch:
    """What roi_voxel_pool() leaves behind, F = frames, M = rois per frame, G = Gx Gy Gz sub-voxels of a roi in pcdet's (out_x, out_y, out_z)
    order, T = max_points, Cf = feature channels -- every shape static: `roi_count` (F, M int32: all members of the roi, clipped by no cap),
    `count` (F, M, G int32: the voxel's members among the roi's first roi_capacity, NOT clipped at T), `index` (F, M, G, T int32: the global
    rows of the voxel's first T members in row order, -1 behind them; None unless asked for), `max` and `argmax` (F, M, G, Cf float32 /
    int32: the maximum of every channel over those members and the row that holds it -- the first of equal maxima, never a NaN; 0 and -1
    without one; None unless pooled), `avg` (F, M, G, Cf float32: their float32 sum in row order over their number, 0 for an empty voxel;
    None unless pooled) and `pose` (F, M, 2 float64: the (cos, sin) that was used, (0, 0) for an absent roi).  `out_size` is (Gx, Gy, Gz);
    as_grid() views a field as (F, M, Gx, Gy, Gz, ...).  max_features() and avg_features() are pure indexing, no kernel of this library.
    At F = 16, M = 128, G = 12^3, Cf = 128 each pooled field is 1.8 GB.  All still being written until the stream the call was made on has
    caught up."""

    def __init__(self, roi_count, count, index=None, max=None, argmax=None, avg=None, pose=None, out_size=None, max_points=None):
        self.roi_count, self.count, self.index, self.max, self.argmax, self.avg, self.pose = roi_count, count, index, max, argmax, avg, pose
        self.out_size, self.max_points = out_size, max_points

    @classmethod
    def empty(cls, n_frames, n_rois, out_size=12, max_points=127, channels=None, device=None, with_index=False, pool=('max', 'avg')):
        """Uninitialised buffers of the shapes roi_voxel_pool() writes (out=): static addresses for a captured graph.  channels: Cf of the
        features that will be pooled, None for none."""
        import torch
        dev = _cuda_device(torch, device)
        grid = _out_size3("RoiVoxelBatch.empty", out_size)
        F, M, G, T = int(n_frames), int(n_rois), grid[0] * grid[1] * grid[2], int(max_points)
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        Cf = None if channels is None else int(channels)
        mx, av = Cf is not None and 'max' in pool, Cf is not None and 'avg' in pool
        return cls(torch.empty((F, M), **i32), torch.empty((F, M, G), **i32), torch.empty((F, M, G, T), **i32) if with_index else None,
                   torch.empty((F, M, G, Cf), **f32) if mx else None, torch.empty((F, M, G, Cf), **i32) if mx else None,
                   torch.empty((F, M, G, Cf), **f32) if av else None, torch.empty((F, M, 2), dtype=torch.float64, device=dev), grid, T)

    @property
    def nonempty(self):
        """(F, M, G) bool: count > 0."""
        return self.count > 0

    def as_grid(self, field):
        """A field of (F, M, G, ...) viewed as (F, M, Gx, Gy, Gz, ...): pcdet's pooled_features layout per roi."""
        return field.view(field.shape[0], field.shape[1], *self.out_size, *field.shape[3:])

    def _features(self, who, features):
        import torch
        if not (torch.is_tensor(features) and features.dim() == 2 and features.device == self.count.device and features.is_floating_point()):
            raise ValueError(f"{who}: features must be an (N, Cf) floating-point tensor on the device of the rows: Cf values per row")
        return features

    def max_features(self, features):
        """features[argmax] per channel as (F, M, G, Cf), zeros where argmax is -1: bit-equal to `max` for the features that were pooled, and
        differentiable with respect to `features` through torch's own indexing (the gradient of a voxel goes to the row that won)."""
        import torch
        features = self._features("max_features", features)
        if self.argmax is None or self.argmax.shape[-1] != features.shape[1]:
            raise ValueError("max_features: this batch has no argmax for features of that many channels (roi_voxel_pool(..., features=, pool=('max', ...)))")
        at = self.argmax.long()
        got = features[at.clamp(min=0), torch.arange(features.shape[1], device=features.device)]
        return torch.where(at >= 0, got, torch.zeros_like(got))

    def avg_features(self, features):
        """The mean of `features` over every voxel's pooled rows as (F, M, G, Cf), zeros for an empty voxel: the gather over `index`, summed
        slot after slot -- the order in which `avg` was summed -- and divided by the number of rows; differentiable with respect to
        `features`.  One gather and one add per slot: T of each."""
        import torch
        features = self._features("avg_features", features)
        if self.index is None:
            raise ValueError("avg_features: this batch has no index (roi_voxel_pool(..., return_index=True))")
        at = self.index.long()
        has = at >= 0
        total = torch.zeros(at.shape[:3] + (features.shape[1],), dtype=features.dtype, device=features.device)
        for t in range(at.shape[3]):
            got = features[at[..., t].clamp(min=0)]                           # (F, M, G, Cf)
            total = total + torch.where(has[..., t, None], got, torch.zeros_like(got))
        return total / has.sum(dim=3).clamp(min=1)[..., None].to(total.dtype)


def _out_size3(who, out_size):
    """out_size as (Gx, Gy, Gz) ints: a whole number for all three, or three of them, each in 1 .. 16."""
    g = np.asarray(out_size).reshape(-1)
    if g.shape == (1,):
        g = np.repeat(g, 3)
    if g.shape != (3,) or g.dtype == bool or not np.all(g == np.floor(g)) or not ((g >= 1) & (g <= 16)).all():
        raise ValueError(f"{who}: out_size is a whole number or three (x, y, z), each in 1 .. 16")
    return tuple(int(v) for v in g)


def roi_voxel_pool(frames, rois, out_size=12, max_points=127, features=None, extra_width=0.0, roi_capacity=8192, pose=None, keep=None, return_index=False,
                   pool=('max', 'avg'), out=None, *, device=None, slot=0):
    """RoI-aware voxel pooling on the device (snowgpu_roi_voxel_pool_device; the definition: include/snowgpu.h): pcdet's roiaware_pool3d --
    every slightly enlarged roi cut into out_size sub-voxels along its own axes, the rows inside each listed in row order and their
    features max- and average-pooled -- with points_in_boxes' membership test in float64 and static shapes.

    frames    what roi_point_pool takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult: its rows, offsets and
              keep mask are used (nothing is waited for).
    rois      a contiguous (F, M, 7 .. 10) tensor in the rows' dtype on their device, 1 <= M <= 512 -- or an NmsBatch, whose `boxes` are
              used (the zero rows behind its count are absent rois).
    out_size  a whole number or three (x, y, z), each in 1 .. 16: the sub-voxels along the roi's length, width and height.
    max_points    1 .. 128: T, the members of a voxel that are pooled and indexed (pcdet's max_pts_each_voxel = 128 keeps 127).
    features  None, or a contiguous (N, Cf) float32 tensor on the device of the rows, one row per row of the batch, 1 <= Cf <= 256.
    extra_width   a number or three (x, y, z), each in 0 .. 100: added once to dx, dy, dz (Part-A2 passes none).
    roi_capacity  64 .. 65536: only a roi's first roi_capacity members are distributed to voxels (scratch: two int32 per roi and slot).
    pose      None: cos / sin of the heading in float64 on the device; or a contiguous (F, M, 2) float64 tensor (cos, sin) used as it is.
    keep      an input keep mask as the aligned calls take it (with a result: ANDed with the result's own).
    return_index  also fill `index` (F, M, G, T).
    pool      which of 'max' (max and argmax) and 'avg' to compute from `features`.
    out       a RoiVoxelBatch to write into (RoiVoxelBatch.empty): every element is written, nothing needs clearing.

    Returns a RoiVoxelBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    who = "roi_voxel_pool"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.roiaware.roiaware_pool3d", frames, keep)
    _whole(who, max_points=max_points, roi_capacity=roi_capacity)
    grid = _out_size3(who, out_size)
    ew = np.asarray(extra_width, np.float64).reshape(-1)
    if ew.shape == (1,):
        ew = np.repeat(ew, 3)
    if ew.shape != (3,) or not ((ew >= 0.0) & (ew <= 100.0)).all():
        raise ValueError("roi_voxel_pool: extra_width is a number or three (x, y, z), each finite and in 0 .. 100")
    pool = (pool,) if isinstance(pool, str) else tuple(pool)
    if any(p not in ('max', 'avg') for p in pool):
        raise ValueError("roi_voxel_pool: pool holds 'max', 'avg' or both")
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
    if isinstance(rois, NmsBatch):
        if rois.boxes is None:
            raise ValueError("roi_voxel_pool: this NmsBatch has no boxes (nms(..., return_boxes=True))")
        rois = rois.boxes
    if not (torch.is_tensor(rois) and rois.dim() == 3 and rois.shape[0] == nf and rois.dtype == rows.dtype and rois.device == dev and rois.is_contiguous()):
        raise ValueError("roi_voxel_pool: rois must be a contiguous (frames, M, 7 .. 10) tensor in the rows' dtype on their device, or an NmsBatch of such boxes")
    if features is not None and not (torch.is_tensor(features) and features.dim() == 2 and features.shape[0] == rows.shape[0] and features.dtype == torch.float32
                                     and features.device == dev and features.is_contiguous()):
        raise ValueError("roi_voxel_pool: features must be a contiguous (N, Cf) float32 tensor on the device of the rows, one row per row of the batch")
    M, Cb, T, P, G = int(rois.shape[1]), int(rois.shape[2]), int(max_points), int(roi_capacity), grid[0] * grid[1] * grid[2]
    Cf = None if features is None else int(features.shape[1])
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 1 <= M <= 512:
        raise ValueError("roi_voxel_pool: n_rois must lie in 1 .. 512 (rois)")
    if not 7 <= Cb <= 10:
        raise ValueError("roi_voxel_pool: roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (rois)")
    if not 1 <= T <= 128:
        raise ValueError("roi_voxel_pool: max_points must lie in 1 .. 128")
    if not 64 <= P <= 65536:
        raise ValueError("roi_voxel_pool: roi_capacity must lie in 64 .. 65536")
    if Cf is not None and not 1 <= Cf <= 256:
        raise ValueError("roi_voxel_pool: feature_channels must lie in 1 .. 256 (features)")
    if nf * M * G * max(T, Cf or 1) > 2 ** 31 - 1:
        raise ValueError("roi_voxel_pool: n_frames * n_rois * the voxels of a roi * max(max_points, feature_channels) exceeds 2^31 - 1; split the batch")
    if pose is not None and not (torch.is_tensor(pose) and tuple(pose.shape) == (nf, M, 2) and pose.dtype == torch.float64 and pose.device == dev and pose.is_contiguous()):
        raise ValueError(f"roi_voxel_pool: pose must be a contiguous {(nf, M, 2)} float64 tensor (cos, sin) on the device of the rows")
    do_max, do_avg = Cf is not None and 'max' in pool, Cf is not None and 'avg' in pool
    want = (("roi_count", torch.int32, (nf, M), True), ("count", torch.int32, (nf, M, G), True), ("index", torch.int32, (nf, M, G, T), bool(return_index)),
            ("max", torch.float32, (nf, M, G, Cf), do_max), ("argmax", torch.int32, (nf, M, G, Cf), do_max), ("avg", torch.float32, (nf, M, G, Cf), do_avg),
            ("pose", torch.float64, (nf, M, 2), True))
    if out is None:
        out = RoiVoxelBatch.empty(nf, M, grid, T, Cf, dev, return_index, pool)
    else:
        _checked_out(torch, who, RoiVoxelBatch, out, want, dev, _ROWS)
    index, mx, am, av = (out.index if return_index else None), (out.max if do_max else None), (out.argmax if do_max else None), (out.avg if do_avg else None)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.roi_voxel_pool_device, M, rois.data_ptr(), Cb, ew, grid, T, P,
                  ptr(features) if (do_max or do_avg) else 0, Cf or 0, ptr(pose), 0 if keep is None or not n else keep.data_ptr(), out.roi_count.data_ptr(),
                  out.count.data_ptr(), ptr(index), ptr(mx), ptr(am), ptr(av), out.pose.data_ptr())
    same = (index is None) == (out.index is None) and (mx is None) == (out.max is None) and (av is None) == (out.avg is None) and out.out_size == grid \
        and out.max_points == T
    return out if same else RoiVoxelBatch(out.roi_count, out.count, index, mx, am, av, out.pose, grid, T)


class RoiTargetBatch:
    """What sample_rois() leaves behind, F = frames, S = roi_per_image -- every shape static, an empty slot (a frame without a candidate)
    holds -1 / 0: `index` (F, S int32: the sampled roi's number), `rois` (F, S, Cb in the boxes' dtype: bit copies of the sampled rois, zero
    rows in empty slots -- a rois tensor for roi_point_pool, roi_voxel_pool, points_in_boxes and boxes_iou as it stands), `roi_iou` (F, S:
    the roi's overlap), `gt_index` (F, S int32: its gt, -1 for none), `gt_of_rois` (F, S, Cg: that gt box, a zero row for none), `reg_valid`
    (F, S uint8: overlap > reg_fg_thresh), `cls_label` (F, S: the classification target, -1 in an empty slot), `segments` (F, 3 int32: the
    slots of fg, hard and easy picks, in this order), `class_count` (F, 3 int32: the candidates of each class), `pose` (F, S, 2 float64: the
    (cos, sin) used for the pick; None unless asked for) and `gt_local` (F, S, 7: the gt in its roi's frame, [lx, ly, lz, dx, dy, dz,
    heading label]; None unless asked for).  gather() is pure indexing, no kernel of this library.  All still being written until the
    stream the call was made on has caught up."""

    def __init__(self, index, rois, roi_iou, gt_index, gt_of_rois, reg_valid, cls_label, segments, class_count, pose=None, gt_local=None):
        self.index, self.rois, self.roi_iou, self.gt_index, self.gt_of_rois = index, rois, roi_iou, gt_index, gt_of_rois
        self.reg_valid, self.cls_label, self.segments, self.class_count, self.pose, self.gt_local = reg_valid, cls_label, segments, class_count, pose, gt_local

    @classmethod
    def empty(cls, n_frames, roi_per_image=128, roi_features=7, gt_features=8, dtype=None, device=None, with_pose=False, with_local=False):
        """Uninitialised buffers of the shapes sample_rois() writes (out=): static addresses for a captured graph."""
        import torch
        dev = _cuda_device(torch, device)
        F, S, Cb, Cg, dt = int(n_frames), int(roi_per_image), int(roi_features), int(gt_features), dtype or torch.float32

        def new(shape, kind):
            return torch.empty(shape, dtype=kind, device=dev)
        return cls(new((F, S), torch.int32), new((F, S, Cb), dt), new((F, S), dt), new((F, S), torch.int32), new((F, S, Cg), dt), new((F, S), torch.uint8),
                   new((F, S), dt), new((F, 3), torch.int32), new((F, 3), torch.int32), new((F, S, 2), torch.float64) if with_pose else None,
                   new((F, S, 7), dt) if with_local else None)

    @property
    def valid(self):
        """(F, S) bool: index >= 0 -- the slot holds a roi."""
        return self.index >= 0

    def gather(self, per_roi, fill=0):
        """Per-roi values (F, M) or (F, M, D) -- roi_scores, roi_labels -- as (F, S) or (F, S, D): the value of the sampled roi, `fill` in
        empty slots."""
        import torch
        if not (torch.is_tensor(per_roi) and per_roi.dim() in (2, 3) and per_roi.shape[0] == self.index.shape[0] and per_roi.device == self.index.device):
            raise ValueError("gather: per_roi must be an (F, M) or (F, M, D) tensor on the device of the rois: one value, or D of them, per roi")
        at = self.index.long()
        has = at >= 0
        at = at.clamp(min=0)
        got = torch.gather(per_roi, 1, at if per_roi.dim() == 2 else at[..., None].expand(-1, -1, per_roi.shape[2]))
        return torch.where(has if got.dim() == 2 else has[..., None], got, torch.full_like(got, fill))


def sample_rois(rois, gt_boxes, overlaps, *, step, seed=0, roi_per_image=128, fg_ratio=0.5, reg_fg_thresh=0.55, cls_fg_thresh=0.75, cls_bg_thresh=0.25,
                cls_bg_thresh_lo=0.1, hard_bg_ratio=0.8, cls_score_type='roi_iou', pose=None, out=None, return_local=False, return_pose=False, slot=0):
    """Which roi_per_image rois of every frame the second stage trains on, and their targets, on the device (snowgpu_sample_rois_device; the
    definition: include/snowgpu.h): the sampling of pcdet's ProposalTargetLayer with static shapes, nothing read on the host and a seeded
    draw -- foreground rois without replacement, hard and easy background with replacement.  The definition is this library's, modelled on
    pcdet's layer; parity with pcdet's random stream is distributional.  Rois that are absent (zero rows) or whose overlap is NaN are never
    sampled.

    rois       a contiguous (F, M, 7 .. 10) float32 or float64 CUDA tensor, 1 <= M <= 9216 -- or an NmsBatch, whose `boxes` are used.
    gt_boxes   (F, B, 7 .. 10) likewise, same dtype and device, 1 <= B <= 9216.
    overlaps   the IouBatch of boxes_iou(rois, gt_boxes, return_best=True), whose best / best_iou are used, or a pair (max_overlaps,
               gt_assignment): contiguous (F, M) tensors in the boxes' dtype and in int32.
    step       a one-element int64 tensor on the device of the boxes (WeatherPlan.step as it stands): read by the kernel, so a captured
               graph that also holds `step += 1` draws anew on every replay.
    seed       the key of the draw; the picks of frame f depend on (seed, step, f) and the frame's own data.
    roi_per_image   1 .. 1024: S.    fg_ratio   fg_per_image = int(np.round(fg_ratio * roi_per_image)), in 0 .. S.
    reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo, hard_bg_ratio   pcdet's TARGET_CONFIG values of the same names.
    cls_score_type  'roi_iou' or 'cls'.
    pose       None: cos / sin of the heading in float64 on the device; or a contiguous (F, M, 2) float64 tensor (cos, sin) used as it is.
    out        a RoiTargetBatch to write into (RoiTargetBatch.empty): every element is written, nothing needs clearing.

    Returns a RoiTargetBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    from . import _native
    from . import engine as _engine
    who = "sample_rois"
    _whole(who, roi_per_image=roi_per_image)
    values = [float(v) for v in (fg_ratio, reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo, hard_bg_ratio)]
    if not all(math.isfinite(v) for v in values):
        raise ValueError(f"{who}: fg_ratio, the thresholds and hard_bg_ratio must be finite")
    if cls_score_type not in _native.CLS_SCORE_TYPES:
        raise ValueError(f"{who}: cls_score_type must be 'roi_iou' or 'cls'")
    if isinstance(rois, NmsBatch):
        if rois.boxes is None:
            raise ValueError(f"{who}: this NmsBatch has no boxes (nms(..., return_boxes=True))")
        rois = rois.boxes
    F, M, Cb = _box_set(torch, who, "rois", rois, 9216)
    _, B, Cg = _box_set(torch, who, "gt_boxes", gt_boxes, 9216, rois)
    dev, dt = rois.device, rois.dtype
    if isinstance(overlaps, IouBatch):
        if overlaps.best is None or overlaps.best_iou is None:
            raise ValueError(f"{who}: this IouBatch has no best partner (boxes_iou(..., return_best=True))")
        overlaps = (overlaps.best_iou, overlaps.best)
    if not (isinstance(overlaps, (tuple, list)) and len(overlaps) == 2):
        raise ValueError(f"{who}: overlaps must be an IouBatch or a pair (max_overlaps, gt_assignment)")
    ov, assign = overlaps
    if not (torch.is_tensor(ov) and tuple(ov.shape) == (F, M) and ov.dtype == dt and ov.device == dev and ov.is_contiguous()):
        raise ValueError(f"{who}: max_overlaps must be a contiguous {(F, M)} tensor in the boxes' dtype on their device")
    if not (torch.is_tensor(assign) and tuple(assign.shape) == (F, M) and assign.dtype == torch.int32 and assign.device == dev and assign.is_contiguous()):
        raise ValueError(f"{who}: gt_assignment must be a contiguous {(F, M)} int32 tensor on the device of the boxes")
    if not (torch.is_tensor(step) and step.numel() == 1 and step.dtype == torch.int64 and step.device == dev):
        raise ValueError(f"{who}: step must be a one-element int64 tensor on the device of the boxes")
    S = int(roi_per_image)
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 1 <= S <= 1024:
        raise ValueError(f"{who}: roi_per_image must lie in 1 .. 1024")
    fg_per_image = int(np.round(values[0] * S))
    if not 0 <= fg_per_image <= S:
        raise ValueError(f"{who}: fg_per_image must lie in 0 .. roi_per_image (fg_ratio in 0 .. 1)")
    if F * S * max(Cb, Cg) > 2 ** 31 - 1:
        raise ValueError(f"{who}: n_frames * roi_per_image * max(roi_features, gt_features) exceeds 2^31 - 1; split the batch")
    pp = _box_pose(torch, who, "pose", pose, rois)
    want = (("index", torch.int32, (F, S), True), ("rois", dt, (F, S, Cb), True), ("roi_iou", dt, (F, S), True), ("gt_index", torch.int32, (F, S), True),
            ("gt_of_rois", dt, (F, S, Cg), True), ("reg_valid", torch.uint8, (F, S), True), ("cls_label", dt, (F, S), True),
            ("segments", torch.int32, (F, 3), True), ("class_count", torch.int32, (F, 3), True), ("pose", torch.float64, (F, S, 2), return_pose),
            ("gt_local", dt, (F, S, 7), return_local))
    if out is None:
        out = RoiTargetBatch.empty(F, S, Cb, Cg, dt, dev, return_pose, return_local)
    else:
        _checked_out(torch, who, RoiTargetBatch, out, want, dev)
    used, local = (out.pose if return_pose else None), (out.gt_local if return_local else None)
    cfg = _native.roi_sampler_struct(S, fg_per_image, *values[1:], _native.CLS_SCORE_TYPES[cls_score_type])
    eng = _engine.get_engine(dev.index, slot)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        eng.ctx.sample_rois_device(F, M, rois.data_ptr(), Cb, ov.data_ptr(), assign.data_ptr(), B, gt_boxes.data_ptr(), Cg, 0 if dt == torch.float32 else 1,
                                   cfg, seed, step.data_ptr(), pp, out.index.data_ptr(), out.rois.data_ptr(), out.roi_iou.data_ptr(), out.gt_index.data_ptr(),
                                   out.gt_of_rois.data_ptr(), out.reg_valid.data_ptr(), out.cls_label.data_ptr(), out.segments.data_ptr(),
                                   out.class_count.data_ptr(), 0 if used is None else used.data_ptr(), 0 if local is None else local.data_ptr(), run.cuda_stream)
    same = (used is None) == (out.pose is None) and (local is None) == (out.gt_local is None)
    return out if same else RoiTargetBatch(out.index, out.rois, out.roi_iou, out.gt_index, out.gt_of_rois, out.reg_valid, out.cls_label, out.segments,
                                           out.class_count, used, local)


class AnchorTargetBatch:
    """What assign_anchors() leaves behind, F = frames, A = anchors, B = gt boxes per frame -- every shape static, every element written by
    every call: `label` (F, A int32: the class for a positive, 0 for background, -1 for an ignored or absent anchor), `gt_index` (F, A
    int32: the gt number of a positive, -1 otherwise), `count` (F, 3 int32: positives, backgrounds, ignored; absent anchors are in none of
    them), `gt_count` (F, B int32: the positives assigned to each gt) and `iou` (F, A in the boxes' dtype: the anchor's best overlap; None
    unless asked for).  positive, matched(), reg_weights() and cls_weights() are pure indexing, no kernel of this library.  All still being
    written until the stream the call was made on has caught up."""

    def __init__(self, label, gt_index, count, gt_count, iou=None):
        self.label, self.gt_index, self.count, self.gt_count, self.iou = label, gt_index, count, gt_count, iou

    @classmethod
    def empty(cls, n_frames, n_anchors, n_gt, dtype=None, device=None, with_iou=False):
        """Uninitialised buffers of the shapes assign_anchors() writes (out=): static addresses for a captured graph."""
        import torch
        dev = _cuda_device(torch, device)
        F, A, B = int(n_frames), int(n_anchors), int(n_gt)

        def new(shape, kind):
            return torch.empty(shape, dtype=kind, device=dev)
        return cls(new((F, A), torch.int32), new((F, A), torch.int32), new((F, 3), torch.int32), new((F, B), torch.int32),
                   new((F, A), dtype or torch.float32) if with_iou else None)

    @property
    def positive(self):
        """(F, A) bool: label > 0."""
        return self.label > 0

    def matched(self, gt_boxes):
        """(F, A, Cg): the gt box of every positive anchor, a zero row where the anchor is not positive -- what a ResidualCoder encodes
        against the anchors, and whose heading gives the direction targets."""
        import torch
        F, A = self.label.shape
        if not (torch.is_tensor(gt_boxes) and gt_boxes.dim() == 3 and gt_boxes.shape[0] == F and gt_boxes.shape[1] == self.gt_count.shape[1] and
                gt_boxes.device == self.label.device):
            raise ValueError(f"matched: gt_boxes must be the ({F}, {self.gt_count.shape[1]}, Cg) tensor the anchors were assigned to, on their device")
        at = self.gt_index.long()
        got = torch.gather(gt_boxes, 1, at.clamp(min=0)[..., None].expand(-1, -1, gt_boxes.shape[2]))
        return torch.where((at >= 0)[..., None], got, torch.zeros_like(got))

    def reg_weights(self, norm_by_num_examples=True):
        """(F, A) float32: 1 on positives -- with norm_by_num_examples 1 / max(positives + backgrounds, 1) of the frame --, 0 elsewhere."""
        w = self.positive.float()
        if norm_by_num_examples:
            w = w / (self.count[:, 0] + self.count[:, 1]).clamp(min=1).float()[:, None]
        return w

    def cls_weights(self):
        """(F, A) float32: 1 on positives and backgrounds, 0 on ignored and absent anchors."""
        return (self.label >= 0).float()


def anchor_grid(point_cloud_range, grid_size, sizes, rotations, bottom_heights, align_center=False, dtype=None, device=None):
    """The anchors of pcdet's AnchorGenerator and their class numbers, plain torch arithmetic run once at set-up (no kernel): one class per
    entry of `sizes` ((dx, dy, dz) each) with its entry of `bottom_heights`, every rotation of `rotations` at every position of the
    nx x ny grid.  Centres are range_lo + i (range_hi - range_lo) / (n - 1) -- with align_center range_lo + (i + 0.5) stride,
    stride = (range_hi - range_lo) / n --, z is bottom_height + dz / 2.  Anchor number a = ((y nx + x) NC + c) R + r: the order in which an
    anchor head's cls_preds.view(F, -1, NC) lies.  Returns (anchors (A, 7) in `dtype`, anchor_class (A) int32 = c + 1), computed in float64."""
    import torch
    who = "anchor_grid"
    rng = _range6(who, point_cloud_range)
    if rng is None:
        raise ValueError(f"{who}: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)")
    nx, ny = grid_size
    _whole(who, nx=nx, ny=ny)
    nx, ny = int(nx), int(ny)
    sz = np.asarray(sizes, np.float64)
    rot, low = np.asarray(rotations, np.float64).reshape(-1), np.asarray(bottom_heights, np.float64).reshape(-1)
    if sz.ndim != 2 or sz.shape[1] != 3 or len(sz) < 1 or len(low) != len(sz) or len(rot) < 1:
        raise ValueError(f"{who}: sizes holds one (dx, dy, dz) per class, bottom_heights one number per class, rotations at least one")
    if nx < 1 or ny < 1 or (not align_center and (nx < 2 or ny < 2)):
        raise ValueError(f"{who}: the grid needs at least 2 positions per axis (1 with align_center)")

    def centres(lo, hi, n):
        i = np.arange(n, dtype=np.float64)
        return lo + (i + 0.5) * ((hi - lo) / n) if align_center else lo + i * ((hi - lo) / (n - 1))
    NC, R = len(sz), len(rot)
    out = np.zeros((ny, nx, NC, R, 7), np.float64)
    out[..., 0] = centres(rng[0], rng[3], nx)[None, :, None, None]
    out[..., 1] = centres(rng[1], rng[4], ny)[:, None, None, None]
    out[..., 2] = (low + sz[:, 2] / 2)[None, None, :, None]
    out[..., 3:6] = sz[None, None, :, None, :]
    out[..., 6] = rot[None, None, None, :]
    cls = np.broadcast_to(np.arange(1, NC + 1, dtype=np.int32)[None, None, :, None], (ny, nx, NC, R))
    dev = torch.device(device) if isinstance(device, str) else _cuda_device(torch, device)       # ("cpu" is fine: nothing here needs the GPU)
    return (torch.from_numpy(out.reshape(-1, 7)).to(dtype or torch.float32).to(dev).contiguous(),
            torch.from_numpy(np.ascontiguousarray(cls).reshape(-1)).to(dev))


def assign_anchors(anchors, anchor_class, gt_boxes, matched=(0.6, 0.5, 0.5), unmatched=(0.45, 0.35, 0.35), *, out=None, return_iou=False, slot=0):
    """The anchor targets of every frame on the device (snowgpu_assign_anchors_device; the definition: include/snowgpu.h): the assignment
    of pcdet's AxisAlignedTargetAssigner with static shapes and nothing read on the host -- per class the nearest axis-aligned BEV overlap
    of every anchor with every gt in float64, positives by the matched threshold and by being a gt's best anchor, backgrounds by the
    unmatched threshold, the rest ignored.  The definition is this library's, modelled on pcdet's assigner.

    anchors       a contiguous (A, 7 .. 10) float32 or float64 CUDA tensor shared by all frames (anchor_grid): cx, cy, cz, dx, dy, dz,
                  heading first; F A < 2^31.
    anchor_class  a contiguous (A) int32 tensor on their device: the class number, 1 .. NC, of each anchor; anything else is an absent anchor.
    gt_boxes      a contiguous (F, B, 8 .. 10) tensor of the anchors' dtype on their device, 1 <= B <= 256: column 7 is the class; zero rows
                  are padding (zero the gts an augmentation emptied: points_in_boxes(res, gt).keep_boxes(min_points)).
    matched, unmatched   one number per class, 1 <= NC <= 16 of them, 0 < unmatched[c] <= matched[c] <= 1.
    out           an AnchorTargetBatch to write into (AnchorTargetBatch.empty): every element is written, nothing needs clearing.
    The gt records are scratch of the engine of `slot`: calls made on streams that are not ordered against each other need a `slot` each.

    Returns an AnchorTargetBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    from . import engine as _engine
    who = "assign_anchors"
    try:
        m, u = [float(v) for v in matched], [float(v) for v in unmatched]
    except TypeError:
        raise ValueError(f"{who}: matched and unmatched hold one number per class") from None
    if len(m) != len(u):
        raise ValueError(f"{who}: matched and unmatched hold one number per class")
    if not (torch.is_tensor(anchors) and anchors.is_cuda and anchors.dim() == 2 and anchors.dtype in (torch.float32, torch.float64) and anchors.is_contiguous()):
        raise ValueError(f"{who}: anchors must be a contiguous (A, 7 .. 10) float32 or float64 CUDA tensor")
    A, Ca = (int(v) for v in anchors.shape)
    dev, dt = anchors.device, anchors.dtype
    if not (torch.is_tensor(anchor_class) and tuple(anchor_class.shape) == (A,) and anchor_class.dtype == torch.int32 and anchor_class.device == dev and
            anchor_class.is_contiguous()):
        raise ValueError(f"{who}: anchor_class must be a contiguous ({A},) int32 tensor on the device of the anchors")
    if not (torch.is_tensor(gt_boxes) and gt_boxes.dim() == 3 and gt_boxes.dtype == dt and gt_boxes.device == dev and gt_boxes.is_contiguous()):
        raise ValueError(f"{who}: gt_boxes must be a contiguous (frames, B, 8 .. 10) tensor of the anchors' dtype on their device")
    F, B, Cg = (int(v) for v in gt_boxes.shape)
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if F < 1 or A < 1:
        raise ValueError(f"{who}: the frames and the anchors must be at least 1")
    if not 1 <= B <= 256:
        raise ValueError(f"{who}: n_gt must lie in 1 .. 256")
    if F * A > 2 ** 31 - 1:
        raise ValueError(f"{who}: n_frames * n_anchors exceeds 2^31 - 1; split the batch")
    want = (("label", torch.int32, (F, A), True), ("gt_index", torch.int32, (F, A), True), ("count", torch.int32, (F, 3), True),
            ("gt_count", torch.int32, (F, B), True), ("iou", dt, (F, A), return_iou))
    if out is None:
        out = AnchorTargetBatch.empty(F, A, B, dt, dev, return_iou)
    else:
        _checked_out(torch, who, AnchorTargetBatch, out, want, dev, "anchors")
    iou = out.iou if return_iou else None
    eng = _engine.get_engine(dev.index, slot)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        eng.ctx.assign_anchors_device(F, A, anchors.data_ptr(), Ca, anchor_class.data_ptr(), B, gt_boxes.data_ptr(), Cg, 0 if dt == torch.float32 else 1, m, u,
                                      out.label.data_ptr(), out.gt_index.data_ptr(), out.count.data_ptr(), out.gt_count.data_ptr(),
                                      0 if iou is None else iou.data_ptr(), run.cuda_stream)
    return out if (iou is None) == (out.iou is None) else AnchorTargetBatch(out.label, out.gt_index, out.count, out.gt_count, iou)


CENTER_STATES = {"absent": 0, "drawn": 1, "dropped": 2, "no_slot": 3}


class CenterTargetBatch:
    """What assign_centers() leaves behind, F = frames, B = gt boxes per frame, NC = classes, NH = heads, M = max_objs, (W, H) the feature
    map -- every shape static, every element written by every call: `heatmap` (F, NC, H, W float32: channel c - 1 is class c), `gt_index`
    (F, NH, M int32: the gt of each slot, -1 when empty), `ind` (F, NH, M int32: ciy * W + cix, 0 when empty), `mask` (F, NH, M bool),
    `offset` (F, NH, M, 2 in the boxes' dtype: the fractional part of the centre), `radius` (F, NH, M int32), `count` (F, NH int32: the
    filled slots) and `state` (F, B uint8: CENTER_STATES).  head_heatmap() and target_boxes() are pure indexing and torch arithmetic, no
    kernel of this library.  All still being written until the stream the call was made on has caught up."""

    FIELDS = ("heatmap", "gt_index", "ind", "mask", "offset", "radius", "count", "state")

    def __init__(self, heatmap, gt_index, ind, mask, offset, radius, count, state, class_head=None):
        self.heatmap, self.gt_index, self.ind, self.mask, self.offset, self.radius, self.count, self.state = heatmap, gt_index, ind, mask, offset, radius, count, state
        self.class_head = None if class_head is None else tuple(int(h) for h in class_head)

    @classmethod
    def empty(cls, n_frames, n_gt, n_classes, n_heads, max_objs, feature_map_size, dtype=None, device=None):
        """Uninitialised buffers of the shapes assign_centers() writes (out=): static addresses for a captured graph.  feature_map_size: (W, H)."""
        import torch
        dev = _cuda_device(torch, device)
        F, B, NC, NH, M = int(n_frames), int(n_gt), int(n_classes), int(n_heads), int(max_objs)
        W, H = (int(v) for v in feature_map_size)

        def new(shape, kind):
            return torch.empty(shape, dtype=kind, device=dev)
        return cls(new((F, NC, H, W), torch.float32), new((F, NH, M), torch.int32), new((F, NH, M), torch.int32), new((F, NH, M), torch.bool),
                   new((F, NH, M, 2), dtype or torch.float32), new((F, NH, M), torch.int32), new((F, NH), torch.int32), new((F, B), torch.uint8))

    def head_heatmap(self, head):
        """(F, the head's classes, H, W): the channels of the classes whose head is `head`, in ascending class -- a view when they are
        adjacent, as a head's classes usually are."""
        if self.class_head is None:
            raise ValueError("head_heatmap: this batch was not filled by assign_centers() yet: the classes of a head are not known")
        at = [c for c, h in enumerate(self.class_head) if h == int(head)]
        if not at:
            raise ValueError(f"head_heatmap: no class has head {head}")
        return self.heatmap[:, at[0]:at[-1] + 1] if at == list(range(at[0], at[-1] + 1)) else self.heatmap[:, at]

    def target_boxes(self, gt_boxes):
        """(F, NH, M, Cg): per slot the regression targets of a centre head -- offset x, offset y, z, log dx, log dy, log dz, cos and sin of the
        heading, then the columns behind the class -- and a zero row in an empty slot.  Torch arithmetic on `gt_index`."""
        import torch
        F, NH, M = self.gt_index.shape
        if not (torch.is_tensor(gt_boxes) and gt_boxes.dim() == 3 and gt_boxes.shape[0] == F and gt_boxes.shape[1] == self.state.shape[1] and
                gt_boxes.shape[2] >= 8 and gt_boxes.device == self.gt_index.device):
            raise ValueError(f"target_boxes: gt_boxes must be the ({F}, {self.state.shape[1]}, Cg) tensor the centres were assigned to, on their device")
        Cg = gt_boxes.shape[2]
        at = self.gt_index.long().reshape(F, NH * M)
        full = (at >= 0)[..., None]
        got = torch.gather(gt_boxes, 1, at.clamp(min=0)[..., None].expand(-1, -1, Cg))
        safe = torch.where(full, got[..., 3:6], torch.ones_like(got[..., 3:6]))                  # (no log of a padding row's zeros)
        out = torch.cat((self.offset.reshape(F, NH * M, 2).to(got.dtype), got[..., 2:3], torch.log(safe), torch.cos(got[..., 6:7]), torch.sin(got[..., 6:7]),
                         got[..., 8:]), dim=2)
        return torch.where(full, out, torch.zeros_like(out)).reshape(F, NH, M, Cg)


def assign_centers(gt_boxes, point_cloud_range, voxel_size, stride, feature_map_size, n_classes=3, class_head=None, max_objs=500, gaussian_overlap=0.1,
                   min_radius=2, outside="clamp", *, out=None, slot=0):
    """The centre heatmap targets of every frame on the device (snowgpu_assign_centers_device; the definition: include/snowgpu.h): the
    assignment of pcdet's CenterHead with static shapes and nothing read on the host -- per gt the centre pixel, its fractional offset and
    the Gaussian radius in float64, per head the gts' slots in ascending gt number, per class the maximum of the gts' Gaussians.  The
    definition is this library's, modelled on pcdet's CenterHead and centernet_utils.

    gt_boxes           a contiguous (F, B, 8 .. 10) float32 or float64 CUDA tensor, 1 <= B <= 256: cx, cy, cz, dx, dy, dz, heading, class
                       first; zero rows are padding (zero the gts an augmentation emptied: points_in_boxes(res, gt).keep_boxes(min_points)).
    point_cloud_range  6 numbers (x0, y0, z0, x1, y1, z1): x0 and y0 are used.   voxel_size  3 numbers: vx and vy are used.
    stride             the feature map's stride, a whole number >= 1.   feature_map_size  (W, H).
    class_head         the head of every class, n_classes whole numbers from 0; None: one head.  NH is the largest + 1.
    max_objs           the slots of a head, 1 .. 512.   min_radius  0 .. 512.   outside  'clamp' (pcdet) or 'drop'.
    out                a CenterTargetBatch to write into (CenterTargetBatch.empty): every element is written, nothing needs clearing.
    The gt records are scratch of the engine of `slot`: calls made on streams that are not ordered against each other need a `slot` each.

    Returns a CenterTargetBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    from . import engine as _engine
    from ._native import OUTSIDE_MODES, center_cfg_struct
    who = "assign_centers"
    rng, size = np.asarray(point_cloud_range, np.float64).reshape(-1), np.asarray(voxel_size, np.float64).reshape(-1)
    if rng.shape != (6,) or size.shape != (3,):
        raise ValueError(f"{who}: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1), voxel_size 3")
    try:
        W, H = feature_map_size
    except (TypeError, ValueError):
        raise ValueError(f"{who}: feature_map_size holds 2 whole numbers (W, H)") from None
    _whole(who, stride=stride, W=W, H=H, n_classes=n_classes, max_objs=max_objs, min_radius=min_radius)
    W, H, NC, M = int(W), int(H), int(n_classes), int(max_objs)
    if outside not in OUTSIDE_MODES:
        raise ValueError(f"{who}: outside must be 'clamp' or 'drop'")
    heads = [0] * max(NC, 0) if class_head is None else list(class_head)
    if len(heads) != NC or any(int(h) != h for h in heads):
        raise ValueError(f"{who}: class_head holds one whole number per class")
    heads = [int(h) for h in heads]
    NH = max(heads, default=0) + 1
    if not (torch.is_tensor(gt_boxes) and gt_boxes.is_cuda and gt_boxes.dim() == 3 and gt_boxes.dtype in (torch.float32, torch.float64) and gt_boxes.is_contiguous()):
        raise ValueError(f"{who}: gt_boxes must be a contiguous (frames, B, 8 .. 10) float32 or float64 CUDA tensor")
    F, B, Cg = (int(v) for v in gt_boxes.shape)
    dev, dt = gt_boxes.device, gt_boxes.dtype
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if F < 1:
        raise ValueError(f"{who}: the frames must be at least 1")
    if not 1 <= B <= 256:
        raise ValueError(f"{who}: n_gt must lie in 1 .. 256")
    if not 1 <= NC <= 16:
        raise ValueError(f"{who}: n_classes must lie in 1 .. 16")
    if not 1 <= NH <= 16 or min(heads) < 0:
        raise ValueError(f"{who}: every class needs a head in 0 .. 15")
    if not 1 <= M <= 512:
        raise ValueError(f"{who}: max_objs must lie in 1 .. 512")
    if W < 1 or H < 1:
        raise ValueError(f"{who}: the feature map needs at least one pixel on either axis")
    if F * NC * H * W > 2 ** 31 - 1:
        raise ValueError(f"{who}: n_frames * n_classes * height * width exceeds 2^31 - 1; split the batch")
    want = (("heatmap", torch.float32, (F, NC, H, W), True), ("gt_index", torch.int32, (F, NH, M), True), ("ind", torch.int32, (F, NH, M), True),
            ("mask", torch.bool, (F, NH, M), True), ("offset", dt, (F, NH, M, 2), True), ("radius", torch.int32, (F, NH, M), True),
            ("count", torch.int32, (F, NH), True), ("state", torch.uint8, (F, B), True))
    if out is None:
        out = CenterTargetBatch.empty(F, B, NC, NH, M, (W, H), dt, dev)
    else:
        _checked_out(torch, who, CenterTargetBatch, out, want, dev, "gt boxes")
    out.class_head = tuple(heads)
    cfg = center_cfg_struct(rng[0], rng[1], size[0], size[1], stride, W, H, NC, NH, heads, M, gaussian_overlap, min_radius, OUTSIDE_MODES[outside])
    eng = _engine.get_engine(dev.index, slot)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        eng.ctx.assign_centers_device(F, B, gt_boxes.data_ptr(), Cg, 0 if dt == torch.float32 else 1, cfg, out.heatmap.data_ptr(), out.gt_index.data_ptr(),
                                      out.ind.data_ptr(), out.mask.data_ptr(), out.offset.data_ptr(), out.radius.data_ptr(), out.count.data_ptr(),
                                      out.state.data_ptr(), run.cuda_stream)
    return out


PASTE_STATES = {"inactive": 0, "pasted": 1, "hit_gt": 2, "hit_pasted": 3, "no_room": 4, "absent": 5}


class ObjectBank:
    """A database of objects for paste_objects(), resident on the device and made once, outside any capture: `points` (P, 5 in the rows'
    dtype: x, y, z, intensity, channel as cropped from real sweeps -- positions are kept, so channel and range stay valid for the snowfall
    stage), `offsets` (O + 1 int64: object o's points are [offsets[o], offsets[o + 1])), `boxes` (O, 8: the seven box columns and the class
    in column 7), `pose` (O, 2 float64 (cos, sin); None: cos / sin of the heading on the device, computed here once) and `class_offsets` (18
    int32 on the device: the objects of class c = 1 .. 16 are [class_offsets[c], class_offsets[c + 1])).  The constructor reads the offsets
    and the classes on the host: offsets must start at 0, ascend and end at P; classes must be integral, in 1 .. 16 and ascending over the
    objects (lidar_snow_sim_amd.paste.build_bank sorts them).  P and O stay below 2^31."""

    def __init__(self, points, offsets, boxes, pose=None):
        import torch
        who = "ObjectBank"
        if not (torch.is_tensor(points) and points.is_cuda and points.dim() == 2 and points.shape[1] == 5 and points.dtype in (torch.float32, torch.float64) and
                points.is_contiguous()):
            raise ValueError(f"{who}: points must be a contiguous (P, 5) float32 or float64 CUDA tensor")
        dev, dt = points.device, points.dtype
        if not (torch.is_tensor(boxes) and boxes.dim() == 2 and boxes.shape[1] == 8 and boxes.dtype == dt and boxes.device == dev and boxes.is_contiguous()):
            raise ValueError(f"{who}: boxes must be a contiguous (O, 8) tensor of the points' dtype on their device: seven box columns and the class")
        P, O = int(points.shape[0]), int(boxes.shape[0])
        if O < 1 or P >= 2 ** 31 or O >= 2 ** 31:
            raise ValueError(f"{who}: the bank must hold an object and stay below 2^31 points and objects")
        off = offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else np.asarray(offsets)
        if off.dtype.kind not in "iu" or off.shape != (O + 1,):
            raise ValueError(f"{who}: offsets must hold O + 1 = {O + 1} whole numbers")
        off = off.astype(np.int64)
        if off[0] != 0 or off[-1] != P or (np.diff(off) < 0).any():
            raise ValueError(f"{who}: offsets must start at 0, ascend and end at the number of points")
        cls = boxes[:, 7].detach().cpu().numpy().astype(np.float64)
        if not (np.isfinite(cls).all() and (cls == np.floor(cls)).all() and (cls >= 1).all() and (cls <= 16).all() and (np.diff(cls) >= 0).all()):
            raise ValueError(f"{who}: the classes (column 7 of boxes) must be integral, in 1 .. 16 and ascending over the objects")
        if pose is None:
            h = boxes[:, 6].to(torch.float64)
            pose = torch.stack((torch.cos(h), torch.sin(h)), dim=1).contiguous()
        elif not (torch.is_tensor(pose) and tuple(pose.shape) == (O, 2) and pose.dtype == torch.float64 and pose.device == dev and pose.is_contiguous()):
            raise ValueError(f"{who}: pose must be a contiguous {(O, 2)} float64 tensor (cos, sin) on the device of the points")
        self.points, self.boxes, self.pose = points, boxes, pose
        self.offsets = torch.from_numpy(off).to(dev)
        self.classes = cls.astype(np.int64)
        self.class_offsets_host = np.searchsorted(self.classes, np.arange(18), side="left").astype(np.int32)
        self.class_offsets = torch.from_numpy(self.class_offsets_host).to(dev)
        self.n_points, self.n_objects = P, O


class PasteBatch:
    """What paste_objects() leaves behind, N = rows of the batch, F = frames, B = gt boxes per frame on input, Q = slots -- every shape
    static: `rows` (N, 5) and `keep` (N bool): the batch after the paste, same offsets -- with `gt_boxes` they go straight into
    augment_batch(..., layout='aligned', keep=) and every later stage; `gt_boxes` (F, B + Q, Cb: the input's rows, then the box of every
    pasted slot, a zero row for every other slot); `object` (F, Q int32: the bank object a slot drew, -1 for an inactive slot); `state`
    (F, Q int32: PASTE_STATES); `source` (N int32: B + q for a pasted row, -1 otherwise; None unless asked for); `count` (F, 4 int32:
    objects pasted, rows pasted, scene rows removed, free slots on input) and `pose` (F, B + Q, 2 float64: the pose used, (0, 0) for absent
    boxes; None unless asked for).  All still being written until the stream the call was made on has caught up."""

    def __init__(self, rows, keep, gt_boxes, object, state, count, source=None, pose=None, offsets=None):
        self.rows, self.keep, self.gt_boxes, self.object, self.state, self.count, self.source, self.pose = rows, keep, gt_boxes, object, state, count, source, pose
        self.offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
        self._base = None

    @classmethod
    def empty(cls, offsets, n_gt, n_slots, gt_features=8, dtype=None, device=None, with_source=True, with_pose=False):
        """Uninitialised buffers of the shapes paste_objects() writes for a batch with these frame offsets (or, for one frame, this number
        of rows) (out=): static addresses for a captured graph."""
        import torch
        dev, dt = _cuda_device(torch, device), dtype or torch.float32
        off = np.array([0, int(offsets)], np.int64) if np.ndim(offsets) == 0 else np.asarray(offsets, np.int64)
        n, F, BQ, Q = int(off[-1]), len(off) - 1, int(n_gt) + int(n_slots), int(n_slots)

        def new(shape, kind):
            return torch.empty(shape, dtype=kind, device=dev)
        return cls(new((n, 5), dt), new((n,), torch.bool), new((F, BQ, int(gt_features)), dt), new((F, Q), torch.int32), new((F, Q), torch.int32),
                   new((F, 4), torch.int32), new((n,), torch.int32) if with_source else None, new((F, BQ, 2), torch.float64) if with_pose else None, off)

    @property
    def pasted(self):
        """(F, Q) bool: state == 1 -- the slot's object is in the batch."""
        return self.state == 1

    def labels(self, background=0):
        """(N,) in the boxes' dtype: the class (column 7 of gt_boxes) of every pasted row's object, `background` for every other row.
        Plain indexing; the first call of a batch of several frames uploads their row counts (make it before capturing a graph)."""
        import torch
        if self.source is None:
            raise ValueError("labels: this PasteBatch has no source (paste_objects(..., return_source=True))")
        at = self.source.long()
        if len(self.offsets) > 2:
            if self._base is None:
                counts = torch.from_numpy(np.diff(self.offsets)).to(at.device)
                first = torch.arange(len(counts), device=at.device) * self.gt_boxes.shape[1]
                self._base = torch.repeat_interleave(first, counts, output_size=int(self.offsets[-1]))
            at = torch.where(at >= 0, at + self._base, at)
        cls = self.gt_boxes[:, :, 7].reshape(-1)[at.clamp(min=0)]
        return torch.where(at >= 0, cls, torch.full_like(cls, background))


def paste_objects(frames, gt_boxes, bank, sample_groups, *, step, seed=0, keep=None, remove_extra_width=(0., 0., 0.), pose=None, out=None,
                  return_source=True, return_pose=False, device=None, slot=0):
    """Ground-truth sampling on the device (snowgpu_paste_objects_device; the definition: include/snowgpu.h): pcdet's DataBaseSampler with
    static shapes, nothing read on the host and a seeded draw.  Per frame and class, as many bank objects are drawn as the frame lacks of
    sample_groups; a candidate that overlaps a gt or an earlier pasted candidate in the BEV, or has more points than the frame has absent
    rows left, is dropped; the others are written into the frame's ABSENT rows (keep False on input: the padding of an F x Nmax x 5 batch),
    their boxes appended to the gt boxes, and the scene rows inside them cleared from the keep mask.  No shape changes.  The definition is
    this library's, modelled on pcdet's sampler: greedy in slot order, no road-plane correction, no occlusion of the scene behind an object.
    Paste BEFORE the snowfall stage, so that flakes occlude and attenuate the objects as they do the scene.

    frames     what points_in_boxes takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult (its keep is ANDed).
    gt_boxes   a contiguous (F, B, 8 .. 10) tensor in the rows' dtype on their device: column 7 is the class; zero rows are padding.
    bank       an ObjectBank of the rows' dtype on their device.
    sample_groups   one whole number n_c >= 0 per class c = 1 .. NC, NC <= 16 (pcdet's SAMPLE_GROUPS); Q = sum n_c in 1 .. 64, B + Q <= 256.
    step       a one-element int64 tensor on the device of the rows (WeatherPlan.step as it stands), read by the kernel.
    seed       the key of the draw; the objects of frame f depend on (seed, step, f) and the frame's own gts.
    keep       an input keep mask as the aligned calls take it; None: every row is present, so nothing with points can be pasted.
    remove_extra_width   a number or three (x, y, z), each in 0 .. 100 (pcdet's REMOVE_EXTRA_WIDTH).
    pose       None: cos / sin of the gts' heading in float64 on the device; or a contiguous (F, B, 2) float64 tensor used as it is.
    out        a PasteBatch to write into (PasteBatch.empty): every element is written; its rows and keep must not be the inputs.

    Returns a PasteBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    who = "paste_objects"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.paste.paste_objects", frames, keep)
    try:
        groups = list(sample_groups)
    except TypeError:
        raise ValueError(f"{who}: sample_groups holds one whole number per class") from None
    _whole(who, **{f"sample_groups[{c}]": v for c, v in enumerate(groups)})
    groups = [int(v) for v in groups]
    ew = np.asarray(remove_extra_width, np.float64).reshape(-1)
    if ew.shape == (1,):
        ew = np.repeat(ew, 3)
    if ew.shape != (3,) or not ((ew >= 0.0) & (ew <= 100.0)).all():
        raise ValueError(f"{who}: remove_extra_width is a number or three (x, y, z), each finite and in 0 .. 100")
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
    if not (torch.is_tensor(gt_boxes) and gt_boxes.dim() == 3 and gt_boxes.shape[0] == nf and gt_boxes.dtype == rows.dtype and gt_boxes.device == dev and
            gt_boxes.is_contiguous()):
        raise ValueError(f"{who}: gt_boxes must be a contiguous (frames, B, 8 .. 10) tensor in the rows' dtype on their device")
    if not (isinstance(bank, ObjectBank) and bank.points.dtype == rows.dtype and bank.points.device == dev):
        raise ValueError(f"{who}: bank must be an ObjectBank in the rows' dtype on their device")
    if not (torch.is_tensor(step) and step.numel() == 1 and step.dtype == torch.int64 and step.device == dev):
        raise ValueError(f"{who}: step must be a one-element int64 tensor on the device of the rows")
    B, Cb, NC, Q = int(gt_boxes.shape[1]), int(gt_boxes.shape[2]), len(groups), sum(groups[:16])
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 1 <= Q <= 64:
        raise ValueError(f"{who}: the sample groups must add up to 1 .. 64 slots")
    if not 1 <= NC <= 16:
        raise ValueError(f"{who}: n_classes must lie in 1 .. 16 (sample_groups)")
    if B < 1 or B + Q > 256:
        raise ValueError(f"{who}: n_gt must be at least 1 and n_gt plus the slots at most 256")
    if not 8 <= Cb <= 10:
        raise ValueError(f"{who}: gt_features must lie in 8 .. 10: cx, cy, cz, dx, dy, dz, heading, class first (gt_boxes)")
    if min(groups) < 0:
        raise ValueError(f"{who}: a sample group is negative")
    if nf * (B + Q) * Cb > 2 ** 31 - 1:
        raise ValueError(f"{who}: n_frames * (n_gt + slots) * gt_features exceeds 2^31 - 1; split the batch")
    if pose is not None and not (torch.is_tensor(pose) and tuple(pose.shape) == (nf, B, 2) and pose.dtype == torch.float64 and pose.device == dev and pose.is_contiguous()):
        raise ValueError(f"{who}: pose must be a contiguous {(nf, B, 2)} float64 tensor (cos, sin) on the device of the rows")
    want = (("rows", rows.dtype, (n, 5), True), ("keep", torch.bool, (n,), True), ("gt_boxes", rows.dtype, (nf, B + Q, Cb), True),
            ("object", torch.int32, (nf, Q), True), ("state", torch.int32, (nf, Q), True), ("count", torch.int32, (nf, 4), True),
            ("source", torch.int32, (n,), return_source), ("pose", torch.float64, (nf, B + Q, 2), return_pose))
    if out is None:
        out = PasteBatch.empty(offsets, B, Q, Cb, rows.dtype, dev, return_source, return_pose)
    else:
        _checked_out(torch, who, PasteBatch, out, want, dev, _ROWS)
    source, used = (out.source if return_source else None), (out.pose if return_pose else None)
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.paste_objects_device, B, gt_boxes.data_ptr(), Cb, 0 if pose is None else pose.data_ptr(),
                  bank.n_points, bank.n_objects, bank.points.data_ptr() if bank.n_points else 0, bank.offsets.data_ptr(), bank.boxes.data_ptr(),
                  bank.pose.data_ptr(), bank.class_offsets.data_ptr(), groups, ew, seed, step.data_ptr(), 0 if keep is None or not n else keep.data_ptr(),
                  out.rows.data_ptr() if n else 0, out.keep.data_ptr() if n else 0, out.gt_boxes.data_ptr(), out.object.data_ptr(), out.state.data_ptr(),
                  0 if source is None or not n else source.data_ptr(), out.count.data_ptr(), 0 if used is None else used.data_ptr())
    same = np.array_equal(out.offsets, np.asarray(offsets, np.int64)) and (source is None) == (out.source is None) and (used is None) == (out.pose is None)
    return out if same else PasteBatch(out.rows, out.keep, out.gt_boxes, out.object, out.state, out.count, source, used, offsets)


SCENE_STATES = {"still": 0, "moved": 1, "blocked": 2}
_FLIP_BITS = {"x": 1, "y": 2}


class SceneBatch:
    """What transform_scene() leaves behind, N = rows of the batch, F = frames, B = gt boxes per frame, T = tries -- every shape static:
    `rows` (N, 5: x, y, z transformed, columns 3 and 4 bit copies) and `keep` (N bool: the input mask, carried so that the batch goes
    straight into voxelize and the stages behind it); `gt_boxes` (F, B, Cb: the transformed boxes, absent ones as they came); `world`
    (F, 8 float64: flip_x, flip_y, cos theta, sin theta, theta, sigma, 0, 0); `state` (F, B int32: SCENE_STATES -- 0 absent or no local
    part, 1 moved, 2 every try collided); `tried` (F, B int32: the try taken, -1 otherwise); `local` (F, B, 8 float64: tx, ty, tz,
    cos delta, sin delta, delta, s, 0 of the try taken, the identity otherwise); `pose` (F, B, 2 float64: the pose of the OUTPUT boxes, as
    points_in_boxes(pose=), boxes_iou and the pooling stages take it; None unless asked for) and `tries` (F, B, T, 8 float64: every
    candidate's record, column 7 its collision bit; None unless asked for).  invert_points(), invert_boxes() and apply_boxes() are plain
    indexing and arithmetic in torch, no kernel of this library, and carry gradients.  All still being written until the stream the call
    was made on has caught up."""

    def __init__(self, rows, keep, gt_boxes, world, state, tried, local, pose=None, tries=None, offsets=None):
        self.rows, self.keep, self.gt_boxes, self.world, self.state, self.tried, self.local, self.pose, self.tries = (rows, keep, gt_boxes, world, state, tried, local,
                                                                                                                      pose, tries)
        self.offsets = np.array([0, rows.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
        self._frame = None

    @classmethod
    def empty(cls, offsets, n_boxes, box_features=8, tries=0, dtype=None, device=None, with_pose=False, with_tries=False):
        """Uninitialised buffers of the shapes transform_scene() writes for a batch with these frame offsets (or, for one frame, this number
        of rows) (out=): static addresses for a captured graph."""
        import torch
        dev, dt = _cuda_device(torch, device), dtype or torch.float32
        off = np.array([0, int(offsets)], np.int64) if np.ndim(offsets) == 0 else np.asarray(offsets, np.int64)
        n, F, B = int(off[-1]), len(off) - 1, int(n_boxes)

        def new(shape, kind):
            return torch.empty(shape, dtype=kind, device=dev)
        return cls(new((n, 5), dt), new((n,), torch.bool), new((F, B, int(box_features)), dt), new((F, 8), torch.float64), new((F, B), torch.int32),
                   new((F, B), torch.int32), new((F, B, 8), torch.float64), new((F, B, 2), torch.float64) if with_pose else None,
                   new((F, B, int(tries), 8), torch.float64) if with_tries else None, off)

    @property
    def moved(self):
        """(F, B) bool: state == 1 -- the box and its rows took a try."""
        return self.state == 1

    def _frame_of_rows(self):
        """(N) int64: the frame of every row.  The first call of a batch of several frames uploads their row counts (make it before
        capturing a graph); later calls reuse the result."""
        import torch
        if self._frame is None:
            counts = torch.from_numpy(np.diff(self.offsets)).to(self.world.device)
            self._frame = torch.repeat_interleave(torch.arange(len(counts), device=counts.device), counts, output_size=int(self.offsets[-1]))
        return self._frame

    def _world_of(self, like, per_row):
        """The six world values per row (N) or per frame (F, 1), after the shape check of a helper's argument."""
        import torch
        n, F = int(self.offsets[-1]), int(self.world.shape[0])
        fits = torch.is_tensor(like) and like.device == self.world.device and like.is_floating_point() and (
            (like.dim() == 2 and like.shape[0] == n and like.shape[1] >= 3) if per_row else (like.dim() == 3 and like.shape[0] == F and like.shape[2] >= 7))
        if not fits:
            raise ValueError("SceneBatch: one point per row of the batch (N, 3 ..), or boxes per frame (F, M, 7 ..), floating point, on the device of the rows")
        w = self.world[self._frame_of_rows()] if per_row else self.world[:, None, :]
        return (w[..., j] for j in range(6))

    def invert_points(self, xyz):
        """The inverse of the WORLD part on points (N, 3 or more columns; one per row of the batch, in its order): divide by sigma, rotate by
        -theta, undo the flips.  Computed in float64, returned in the dtype of `xyz`; columns 3 and up are copied.  Predictions per point
        go back to the sensor frame with it; the local part is not undone."""
        import torch
        fx, fy, c, s, _, sg = self._world_of(xyz, True)
        p = xyz[..., :3].to(torch.float64) / sg[..., None]
        x, y = p[..., 0] * c + p[..., 1] * s, p[..., 1] * c - p[..., 0] * s
        x, y = torch.where(fy != 0, -x, x), torch.where(fx != 0, -y, y)
        return torch.cat((torch.stack((x, y, p[..., 2]), dim=-1).to(xyz.dtype), xyz[..., 3:]), dim=-1)

    def invert_boxes(self, boxes):
        """The inverse of the WORLD part on boxes (F, M, 7 or more columns) of the same frames: predictions made in the augmented frame go
        back to the sensor frame.  Computed in float64, returned in the dtype of `boxes`; columns 7 and up are copied; the heading is not
        wrapped."""
        import torch
        fx, fy, c, s, th, sg = self._world_of(boxes, False)
        b = boxes[..., :7].to(torch.float64)
        ctr, dims, h = b[..., :3] / sg[..., None], b[..., 3:6] / sg[..., None], b[..., 6] - th
        x, y = ctr[..., 0] * c + ctr[..., 1] * s, ctr[..., 1] * c - ctr[..., 0] * s
        x, h = torch.where(fy != 0, -x, x), torch.where(fy != 0, -h - math.pi, h)
        y, h = torch.where(fx != 0, -y, y), torch.where(fx != 0, -h, h)
        return torch.cat((torch.stack((x, y, ctr[..., 2]), dim=-1).to(boxes.dtype), dims.to(boxes.dtype), h[..., None].to(boxes.dtype), boxes[..., 7:]), dim=-1)

    def apply_boxes(self, boxes):
        """The WORLD part forward on other boxes (F, M, 7 or more columns) of the same frames -- proposals made before the augmentation, say
        -- in the stage's order: flip x, flip y, rotate, scale.  Computed in float64, returned in the dtype of `boxes`; columns 7 and up are
        copied; the heading is not wrapped."""
        import torch
        fx, fy, c, s, th, sg = self._world_of(boxes, False)
        b = boxes[..., :7].to(torch.float64)
        x, y, h = b[..., 0], b[..., 1], b[..., 6]
        y, h = torch.where(fx != 0, -y, y), torch.where(fx != 0, -h, h)
        x, h = torch.where(fy != 0, -x, x), torch.where(fy != 0, -(h + math.pi), h)
        x, y, h = x * c - y * s, x * s + y * c, h + th
        ctr = torch.stack((x, y, b[..., 2]), dim=-1) * sg[..., None]
        return torch.cat((ctr.to(boxes.dtype), (b[..., 3:6] * sg[..., None]).to(boxes.dtype), h[..., None].to(boxes.dtype), boxes[..., 7:]), dim=-1)


def _scene_range(who, name, value, n=2):
    """None / () for a part that is off, else n float64 (lo, hi -- or the three half widths of the translation)."""
    if value is None or (np.ndim(value) == 1 and len(value) == 0):
        return None
    v = np.asarray(value, np.float64).reshape(-1)
    if v.shape != (n,):
        raise ValueError(f"{who}: {name} holds {n} numbers" + (" (lo, hi)" if n == 2 else "") + ", or None for a part that is off")
    return v


def transform_scene(frames, gt_boxes, *, step, seed=0, flip=('x',), rotation=(-math.pi / 4, math.pi / 4), scaling=(0.95, 1.05), local=None, box_of=None, pose=None,
                    keep=None, in_place=False, out=None, return_pose=False, return_tried=False, device=None, slot=0):
    """The geometric augmentation behind gt_sampling on the device (snowgpu_transform_scene_device; the definition: include/snowgpu.h):
    pcdet's random_world_flip, random_world_rotation and random_world_scaling and, with `local`, per-object noise (pcdet's
    random_local_translation / rotation / scaling, SECOND's noise_per_object) with its collision test, for rows and gt boxes alike -- static
    shapes, nothing read on the host, draws keyed by (seed, step, frame).  The definition is this library's, modelled on those two.
    ITS PLACE IN THE CHAIN: BEHIND the weather stages and range_image(ring=), which need rows in the sensor frame, and IN FRONT of
    voxelize, the keypoint stages, ball_query, points_in_boxes for labels and assign_anchors.

    frames     what points_in_boxes takes -- torch CUDA tensors, a DeviceBatch, or an AlignedResult / AlignedWetResult (its keep is ANDed).
    gt_boxes   a contiguous (F, B, 7 .. 10) tensor in the rows' dtype on their device; zero rows are padding.  Columns 7 and up are copied:
               the class is in column 7 here, velocity columns are out of scope.
    step       a one-element int64 tensor on the device of the rows (WeatherPlan.step as it stands), read by the kernel.
    seed       the key of the draw.
    flip       the axes a frame may be flipped about, each with probability 1 / 2: any of 'x', 'y'; None or (): off.
    rotation   (lo, hi) of the world angle theta; None or (): off.       scaling   (lo, hi) > 0 of the world scale sigma; None or (): off.
    local      None: no object noise.  Or a dict: translation (ax, ay, az: uniform in -a .. a, each in 0 .. 100), rotation (lo, hi),
               scaling (lo, hi) > 0 -- None or () each: off -- and tries (1 .. 16, default 8): per present box, the first try that overlaps
               no other box in the BEV is taken, greedy in box order; a box whose every try collides stays as it is.
    box_of     with a local part: the box of every row, (N) int32 from points_in_boxes on THESE boxes (BoxLabelBatch.box_of); None: made
               here, in scratch, by that stage's own kernels.
    pose       None: cos / sin of the gts' heading in float64 on the device; or a contiguous (F, B, 2) float64 tensor used as it is.
    keep       an input keep mask as the aligned calls take it; None: every row is present.
    in_place   write the rows over the input rows (a row is read and written by its own lane only); every other output is new memory.
    out        a SceneBatch to write into (SceneBatch.empty): every element is written.  With in_place its rows must be the input rows.

    Returns a SceneBatch.  Asynchronous on torch's current stream; nothing is read on the host: capturable after one warm-up call."""
    import torch
    who = "transform_scene"
    frames, keep = _stage_frames(torch, who, "lidar_snow_sim_amd.scene.transform_scene", frames, keep)
    axes = () if flip is None else ((flip,) if isinstance(flip, str) else tuple(flip))
    if any(a not in _FLIP_BITS for a in axes):
        raise ValueError(f"{who}: flip holds any of 'x' and 'y', or None")
    flip_bits = sum(_FLIP_BITS[a] for a in set(axes))
    rot, sc = _scene_range(who, "rotation", rotation), _scene_range(who, "scaling", scaling)
    T, ltr, lrot, lsc = 0, None, None, None
    if local is not None:
        if not isinstance(local, dict) or set(local) - {"translation", "rotation", "scaling", "tries"}:
            raise ValueError(f"{who}: local is None or a dict of translation, rotation, scaling and tries")
        T = local.get("tries", 8)
        _whole(who, **{"local['tries']": T})
        T = int(T)
        if not 1 <= T <= 16:
            raise ValueError(f"{who}: local['tries'] must lie in 1 .. 16")
        ltr, lrot, lsc = (_scene_range(who, "local['translation']", local.get("translation"), 3), _scene_range(who, "local['rotation']", local.get("rotation")),
                          _scene_range(who, "local['scaling']", local.get("scaling")))
    rows, offsets, eng, dev, nf, n, keep = _stage_batch(torch, frames, keep, device, slot)
    if not (torch.is_tensor(gt_boxes) and gt_boxes.dim() == 3 and gt_boxes.shape[0] == nf and gt_boxes.dtype == rows.dtype and gt_boxes.device == dev and
            gt_boxes.is_contiguous()):
        raise ValueError(f"{who}: gt_boxes must be a contiguous (frames, B, 7 .. 10) tensor in the rows' dtype on their device")
    if not (torch.is_tensor(step) and step.numel() == 1 and step.dtype == torch.int64 and step.device == dev):
        raise ValueError(f"{who}: step must be a one-element int64 tensor on the device of the rows")
    B, Cb = int(gt_boxes.shape[1]), int(gt_boxes.shape[2])
    # (the shapes below need these; the entry refuses them in the same words, and everything else of the domain)
    if not 1 <= B <= 256:
        raise ValueError(f"{who}: n_boxes must lie in 1 .. 256 (gt_boxes)")
    if not 7 <= Cb <= 10:
        raise ValueError(f"{who}: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (gt_boxes)")
    if pose is not None and not (torch.is_tensor(pose) and tuple(pose.shape) == (nf, B, 2) and pose.dtype == torch.float64 and pose.device == dev and pose.is_contiguous()):
        raise ValueError(f"{who}: pose must be a contiguous {(nf, B, 2)} float64 tensor (cos, sin) on the device of the rows")
    if box_of is not None and not (torch.is_tensor(box_of) and tuple(box_of.shape) == (n,) and box_of.dtype == torch.int32 and box_of.device == dev and
                                   box_of.is_contiguous()):
        raise ValueError(f"{who}: box_of must be a contiguous ({n},) int32 tensor on the device of the rows (BoxLabelBatch.box_of)")
    tried = return_tried and T > 0
    if return_tried and not T:
        raise ValueError(f"{who}: return_tried needs a local part")
    want = (("rows", rows.dtype, (n, 5), True), ("keep", torch.bool, (n,), True), ("gt_boxes", rows.dtype, (nf, B, Cb), True), ("world", torch.float64, (nf, 8), True),
            ("state", torch.int32, (nf, B), True), ("tried", torch.int32, (nf, B), True), ("local", torch.float64, (nf, B, 8), True),
            ("pose", torch.float64, (nf, B, 2), return_pose), ("tries", torch.float64, (nf, B, T, 8), tried))
    if out is None:
        out = SceneBatch.empty(offsets, B, Cb, T, rows.dtype, dev, return_pose, tried)
        if in_place:
            out.rows = rows[:n]
    else:
        _checked_out(torch, who, SceneBatch, out, want, dev, _ROWS)
        if in_place and n and out.rows.data_ptr() != rows.data_ptr():
            raise ValueError(f"{who}: with in_place, out.rows must be the input rows")
    used, tries = (out.pose if return_pose else None), (out.tries if tried else None)
    _stage_launch(torch, eng, dev, nf, n, offsets, rows, eng.ctx.transform_scene_device, B, gt_boxes.data_ptr(), Cb, 0 if pose is None else pose.data_ptr(), flip_bits,
                  rot, sc, T, ltr, lrot, lsc, seed, step.data_ptr(), 0 if box_of is None or not n or not T else box_of.data_ptr(),
                  0 if keep is None or not n else keep.data_ptr(), out.rows.data_ptr() if n else 0, out.keep.data_ptr() if n else 0, out.gt_boxes.data_ptr(),
                  out.world.data_ptr(), out.state.data_ptr(), out.tried.data_ptr(), out.local.data_ptr(), 0 if used is None else used.data_ptr(),
                  0 if tries is None else tries.data_ptr())
    same = np.array_equal(out.offsets, np.asarray(offsets, np.int64)) and (used is None) == (out.pose is None) and (tries is None) == (out.tries is None)
    return out if same else SceneBatch(out.rows, out.keep, out.gt_boxes, out.world, out.state, out.tried, out.local, used, tries, offsets)
