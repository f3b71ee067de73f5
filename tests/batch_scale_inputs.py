"""Inputs of tests/test_gpu_batch_scale.py, made on any machine (NumPy only): batches past the trip lengths of the scans that carry a
running total from trip to trip -- 64 tiles of a frame (k_mask_scan, k_pre_means), 64 frames a wave and 256 frames a trip (k_mask_offsets,
k_voxel_offsets), 64 tiles a wave and 1024 tiles a trip over the batch (k_voxel_tile_scan), 256 threads over the 512-row runs of a frame
(k_paste_frame).  tests/test_batch_scale_inputs.py checks, without a GPU, that they are what the GPU tests take them for.  Every function
is cached and returns read-only arrays."""
from functools import lru_cache

import numpy as np

from aligned_mask_inputs import bernoulli, firing
from lidar_snow_sim_amd.synthetic import synthetic_sweep

TILE = 1024                                    # rows of a tile (SG_TILE, SG_VOX_TILE)
RUN = 512                                      # rows of a run (SG_ROI_RUN)
SIZES = (65, 256, 257, 321)                    # many(F): past a wave of frames, a full trip, a trip and one frame, a trip and a wave
N_MANY = 321
STRIDE = 16                                    # azimuth steps between the columns of a small frame (0.05 rad: other cells of a 2 m grid)
EMPTY = (10, 11, 100, 200, 258, 300)           # two adjacent, and the first frame behind 256 that may be empty (255 .. 257 may not)
ALL_ABSENT = (20, 150, 280)
ALL_PRESENT = (30, 160, 290)
MIXED = (63, 64, 65, 255, 256, 257, 320)       # non-empty with present and absent rows (320 = F - 1 of the largest batch; 64, 255, 256 of the others)
LONG_ROWS = (131073, 65537, 65536, 131072, 700, 0)
LONG_FIRING = (2, 3)
VOXEL_ROWS = LONG_ROWS[:4] + (131072,) * 5 + (0, 700)
POLY = (1e-3, 0.05, 12.0)                      # the caller polynomial of tests/test_gpu_aligned_mask.py's edge test
BD = float(np.degrees(3e-3))
PLANE = (np.array([0.0, 0.0, -1.0]), -1.7)
# the wet settings of the fused tests of tests/test_gpu_wet_aligned.py and tests/test_gpu_aligned_mask.py
WET = dict(water_height=0.0008, pavement_depth=0.001, flat_earth=False, replace=True, delta=0.5, noise_floor=0.7, power_factor=15)


def _ro(a):
    a.setflags(write=False)
    return a


def _sweep(seed):
    return synthetic_sweep(64, 2048, seed=seed, intensity="lambert").reshape(64, 2048, 5)


@lru_cache(maxsize=None)
def _many_all(dtype):
    sweeps = [_sweep(1700 + k) for k in range(3)]
    width = np.random.default_rng(1710).integers(1, 9, N_MANY)
    width[list(EMPTY)] = 0
    frames, masks = [], []
    for j in range(N_MANY):
        a = (37 * j) % (2048 - 8 * STRIDE)
        fr = np.ascontiguousarray(sweeps[j % 3][:, a:a + int(width[j]) * STRIDE:STRIDE].reshape(-1, 5)).astype(dtype)
        if j % 7 == 0 and len(fr):
            fr = firing(fr)
        m = bernoulli(len(fr), 0.7, 4400 + j)
        if j in ALL_ABSENT:
            m[:] = False
        if j in ALL_PRESENT:
            m[:] = True
        frames.append(_ro(fr))
        masks.append(_ro(m))
    return tuple(frames), tuple(masks)


@lru_cache(maxsize=None)
def many(F, dtype="float32"):
    """(frames, masks): the first F of 321 small frames, 64 channels x w_j azimuth steps of a 64 x 2048 sweep with w_j in 0 .. 8 (at most
    512 rows a frame, about 92 000 rows in all 321); every seventh in firing order; EMPTY are empty; Bernoulli(0.7) masks with a seed per
    frame, ALL_ABSENT and ALL_PRESENT apart."""
    assert F in SIZES
    frames, masks = _many_all(np.dtype(dtype).name)
    return frames[:F], masks[:F]


@lru_cache(maxsize=None)
def long():
    """(frames, masks): frames of 131 073, 65 537, 65 536, 131 072, 700 and 0 rows -- 64 x 2048 and 64 x 1024 slices of sweeps, the first
    two with one more row of the last channel (the only row of tiles 128 and 64, of runs 256 and 128), the third and the fourth in
    firing order.  Bernoulli(0.7) masks; the two lone rows are present."""
    s = [_sweep(1720 + k) for k in range(4)]
    one_more = lambda k: s[k][63, 7 + k][None]          # noqa: E731  (channel 63: the frame stays channel-sorted)
    frames = [np.concatenate((s[0].reshape(-1, 5), one_more(3))), np.concatenate((s[1][:, ::2].reshape(-1, 5), one_more(2))),
              firing(np.ascontiguousarray(s[2][:, 1::2].reshape(-1, 5))), firing(np.ascontiguousarray(s[3].reshape(-1, 5))),
              s[0][:, 5::186].reshape(-1, 5)[:700], np.zeros((0, 5), np.float32)]
    frames = [np.ascontiguousarray(f, np.float32) for f in frames]
    assert tuple(len(f) for f in frames) == LONG_ROWS
    masks = [bernoulli(len(f), 0.7, 4500 + k) for k, f in enumerate(frames)]
    masks[0][131072] = True
    masks[1][65536] = True
    return tuple(_ro(f) for f in frames), tuple(_ro(m) for m in masks)


def offsets(frames):
    return np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)


def orders(n_frames, seed=80):
    """A channel permutation per frame, fixed."""
    return [list(np.random.default_rng(seed + f).permutation(64)) for f in range(n_frames)]


@lru_cache(maxsize=None)
def voxel_batch():
    """(rows, offsets): the frames of long() with five more full sweeps (in firing order: every tile opens cells) in front of the two
    short ones, the empty one first -- 1 049 278 rows = 1025 tiles, the 700-row frame wholly in tile 1024.  No mask."""
    frames = list(long()[0])
    more = [firing(np.ascontiguousarray(_sweep(1730 + k).reshape(-1, 5))) for k in range(5)]
    frames = frames[:4] + more + [frames[5], frames[4]]
    assert tuple(len(f) for f in frames) == VOXEL_ROWS
    return _ro(np.ascontiguousarray(np.concatenate(frames))), _ro(offsets(frames))


# frame 0 of paste_long: (run, first row, rows) of every absent stretch, and the points of the three objects.  The free ranks are
# run 0: 0 .. 9, run 1: 10 .. 19, run 127: 20 .. 35, run 128: 36 .. 51, run 129: 52 .. 61, run 254: 62 .. 71, run 255: 72 .. 83, run 256: 84.
PASTE_ROWS = (131073, 131072, 700)
PASTE_FREE = ((0, 58, 10), (1, 600, 10), (127, 65520, 16), (128, 65536, 16), (129, 66100, 10), (254, 130100, 10), (255, 131060, 12), (256, 131072, 1))
PASTE_POINTS = (28, 34, 23)                    # ranks 0 .. 27 (runs 0, 1, 127), 28 .. 61 (runs 127, 128, 129), 62 .. 84 (runs 254, 255, 256)
PASTE_FREE_1 = ((0, 0, 50), (255, 130660, 70))      # frame 1: 120 free rows = 85 + a remainder of 35
PASTE_FREE_2 = 40                              # frame 2: its first 40 rows -- room for the first object alone


@lru_cache(maxsize=None)
def paste_long(dtype="float32"):
    """A case of tests/paste_reference.py (as its _straddle): frames of 131 073, 131 072 and 700 rows -- 257 runs a frame, two per thread
    of k_paste_frame, thread 128 holding run 256 alone and threads 129 .. 255 none --, three classes of one object each.  In frame 0
    object 0 fills the free rows of runs 0 and 1 and the first of run 127, object 1 runs from run 127 over 128 into 129 (threads 63 and
    64, waves 0 and 1), object 2 from run 254 over 255 into the lone row of run 256, the frame's last row."""
    import paste_reference as pr
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(7600)
    boxes = [pr._box(-30.0, 5.0, -0.5, 4.0, 2.0, 1.5, 0.2, 1.0), pr._box(0.0, 25.0, -0.5, 4.5, 1.8, 1.6, 1.1, 2.0), pr._box(30.0, -12.0, -0.5, 3.8, 1.7, 1.4, -2.0, 3.0)]
    bank = pr._bank_of(rng, boxes, PASTE_POINTS, dt)
    f0, k0 = pr._scene(rng, PASTE_ROWS[0], dt, 0.0)
    for _, a, n in PASTE_FREE:
        k0[a:a + n] = False
    f0[[58, 65536, 131072]] = np.nan
    f1, k1 = pr._scene(rng, PASTE_ROWS[1], dt, 0.0)
    for _, a, n in PASTE_FREE_1:
        k1[a:a + n] = False
    f2, k2 = pr._scene(rng, PASTE_ROWS[2], dt, 0.0)
    k2[:PASTE_FREE_2] = False
    gt = np.zeros((3, 3, 8), dt)
    gt[0, 1] = pr._box(40.0, 40.0, 0.0, 4.0, 2.0, 1.5, 0.0, 9.0)
    return pr._finish([f0, f1, f2], [k0, k1, k2], gt, bank, (1, 1, 1), 45, 0)


ROI_CENTRES = ((700, 66000, 100000, 131072), (300, 33000, 65000, 65536))      # rows of frames 0 and 1 of long(): in front of and behind run 128
ROI_SAMPLES = 64


@lru_cache(maxsize=None)
def roi_long():
    """A case of tests/roipool_reference.py on the first two frames of long() with their masks: 257 runs a frame (frame 1 has 129 of its
    own: the rest lie beyond its length), four rois of car size centred on rows of the frame and one that holds the whole frame; S = 64."""
    import roipool_reference as rr
    frames, masks = long()
    rois = np.zeros((2, 5, 7))
    for f in range(2):
        for j, i in enumerate(ROI_CENTRES[f]):
            rois[f, j] = tuple(float(v) for v in frames[f][i, :3]) + (4.0, 2.0, 1.5, 0.4 * j - 0.5)
        rois[f, 4] = (0.0, 0.0, 0.0, 1000.0, 1000.0, 100.0, 0.7)
    rois = rois.astype(np.float32)
    rows = _ro(np.ascontiguousarray(np.concatenate(frames[:2])))
    import box_reference as br
    return rr._case(rows, offsets(frames[:2]), _ro(np.concatenate(masks[:2])), rois, br.numpy_pose(rois), ROI_SAMPLES)
