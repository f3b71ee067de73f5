"""Batch plumbing of the torch-tensor boundary (tensors.py is the documented import path): how a batch of CUDA tensors is read where it
lies (DeviceBatch, _resolve_input, _keep_mask), on which stream a call runs (_on_run_stream), how a result is handed back (DeviceResult,
AlignedResult, AlignedWetResult) -- and the blocks every device stage of stages.py is made of, each written once: _stage_frames, _whole,
_range6, _stage_batch, _checked_out, _stage_launch, _cuda_device.  A helper does what the stage's own lines did: no host read, no
allocation and no synchronisation of its own."""
from __future__ import annotations

import os
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


# ---- what the device stages share (stages.py), in the order a stage goes through it -----------------------------------------------------------
def _stage_frames(torch, who, host_hint, frames, keep):
    """(frames, keep) of a stage call: an AlignedResult / AlignedWetResult becomes its rows and offsets, its keep mask ANDed with `keep`
    (nothing is waited for); anything that is not on the device raises, naming the NumPy-facing function `host_hint`."""
    if isinstance(frames, AlignedResult):
        res = frames
        own = res.keep if res.keep.dtype == torch.bool else res.keep.view(torch.bool)
        frames = DeviceBatch(res.rows, res.offsets)
        keep = own if keep is None else (_keep_mask(torch, keep, res.rows, res.offsets) & own)
    if not is_device_input(frames):
        raise ValueError(f"{who}: torch CUDA tensors or an aligned result (host arrays: {host_hint})")
    return frames, keep


def _whole(who, **named):
    """Every named argument is a whole number (and no bool), or ValueError."""
    for name, v in named.items():
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{who}: {name} must be an integer")


def _range6(who, point_cloud_range):
    """point_cloud_range as 6 float64, None for None."""
    if point_cloud_range is None:
        return None
    rng = np.asarray(point_cloud_range, np.float64).reshape(-1)
    if rng.shape != (6,):
        raise ValueError(f"{who}: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)")
    return rng


def _stage_batch(torch, frames, keep, device, slot):
    """(rows, host offsets, engine, device, n_frames, n_rows, keep mask or None) of a stage call."""
    rows, offsets, _, eng = _resolve_input(torch, frames, False, device, slot)
    if keep is not None:
        keep = _keep_mask(torch, keep, rows, offsets)
    return rows, offsets, eng, rows.device, len(offsets) - 1, int(offsets[-1]), keep


def _checked_out(torch, who, kind, out, want, dev, where="boxes"):
    """`out` is a `kind` that has every asked-for field of want -- (name, dtype, shape, asked) -- as such a tensor on `dev`, or
    ValueError; a field that was not asked for is not looked at.  where: what the tensors share their device with, for the message."""
    for name, dtype, shape, asked in want:
        t = getattr(out, name, None) if isinstance(out, kind) else None
        if asked and not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev):
            raise ValueError(f"{who}: out must be a {kind.__name__} whose {name} is a contiguous {shape} {dtype} tensor on the device of the {where}")


def _stage_launch(torch, eng, dev, nf, n, offsets, rows, entry, *args):
    """entry(n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code -- the six leading arguments of every batch entry --, *args,
    stream) with the device set and the fork and join of _on_run_stream around it.  (A plain function: a second generator-based context
    manager around the call cost every stage a microsecond, profiles/stage_helpers_refactor_ab.txt.)"""
    up = _uploads(eng)
    with torch.cuda.device(dev), _on_run_stream(torch, eng, dev) as (_, run):
        d_off = up.get(torch, dev, offsets, run)
        entry(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr() if n else 0, 0 if rows.dtype == torch.float32 else 1, *args, run.cuda_stream)


def _cuda_device(torch, device):
    """`device` (None: the current one, an index or a torch.device) as a torch.device."""
    return torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device

