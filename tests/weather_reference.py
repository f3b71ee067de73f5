"""Per-frame weather (snowgpu_draw_weather_device, snowgpu_augment_weather_batch_device_aligned): the draw's SPECIFICATION restated in
Python integers on seeded_reference.philox4x32_10, and the batches tests/test_gpu_weather.py runs.  No GPU, no conftest.

The draw (include/snowgpu.h).  W(b) = philox4x32_10(seed, idx=step, group=f, tag=0x57544852 + b):
  block 0: snow = w0 < T(p_snow), wet = w1 < T(p_wet), T(p) = min(2^32, floor(p 2^32)); set = (w2 n_sets) >> 32; water = (w3 n_water) >> 32
  block 1: pavement = (w0 n_pave) >> 32
  order = 0 .. L-1; for i = L-1 .. 1, k = L-1-i: r = word k % 4 of block 2 + k // 4; j = (r (i + 1)) >> 32; swap order[i], order[j]
  table_ids[f][c] = set_ids[set][order[c]];  record = [snow, wet, water[iw], pave[ip], noise_floor, power_factor, delta, 0]"""
import math

import numpy as np

import aligned_mask_inputs as ami
from seeded_reference import philox4x32_10

TAG = 0x57544852
REC = ("snow", "wet", "water_height", "pavement_depth", "noise_floor", "power_factor", "delta")
PLANE4 = [0.0, 0.0, -1.0, -1.7]

DEFAULT_PLAN = dict(p_snow=0.5, p_wet=0.5, water_heights=(0.0004, 0.0008, 0.002), pavement_depths=(0.001, 0.0012), noise_floor=0.7,
                    power_factor=15.0, delta=0.5, shuffle=True)


def threshold(p):
    return min(1 << 32, int(math.floor(p * 4294967296.0)))


def draw_frame(seed, step, f, n_lasers, n_sets, plan):
    """(snow, wet, set, water index, pavement index, order) of frame f."""
    w = philox4x32_10(seed, step, f, TAG)
    v = philox4x32_10(seed, step, f, TAG + 1)
    snow, wet = int(w[0] < threshold(plan["p_snow"])), int(w[1] < threshold(plan["p_wet"]))
    s = (w[2] * n_sets) >> 32
    iw = (w[3] * len(plan["water_heights"])) >> 32
    ip = (v[0] * len(plan["pavement_depths"])) >> 32
    order = list(range(n_lasers))
    if plan["shuffle"]:
        blocks = {}
        for i in range(n_lasers - 1, 0, -1):
            k = n_lasers - 1 - i
            if k // 4 not in blocks:
                blocks[k // 4] = philox4x32_10(seed, step, f, TAG + 2 + k // 4)
            j = (blocks[k // 4][k % 4] * (i + 1)) >> 32
            order[i], order[j] = order[j], order[i]
    return snow, wet, s, iw, ip, order


def draw(seed, step, n_frames, set_ids, plan):
    """(table_ids n_frames x L int32, weather n_frames x 8 float64, sets drawn) for set_ids (n_sets x L)."""
    set_ids = np.asarray(set_ids, np.int32)
    n_sets, L = set_ids.shape
    tids, rec, sets = np.empty((n_frames, L), np.int32), np.zeros((n_frames, 8), np.float64), []
    for f in range(n_frames):
        snow, wet, s, iw, ip, order = draw_frame(seed, step, f, L, n_sets, plan)
        tids[f] = set_ids[s][order]
        rec[f, :7] = (snow, wet, plan["water_heights"][iw], plan["pavement_depths"][ip], plan["noise_floor"], plan["power_factor"], plan["delta"])
        sets.append(s)
    return tids, rec, sets


def abstract_set_ids(n_sets, n_lasers):
    """set s, line c -> s * n_lasers + c: every id names its set and its line."""
    return np.arange(n_sets * n_lasers, dtype=np.int32).reshape(n_sets, n_lasers)


# ---- the draw cases of the host and the device test ------------------------------------------------------------------------------------
DRAW_FRAMES, DRAW_LASERS, DRAW_SETS, DRAW_STEPS, DRAW_SEED = (1, 5, 64, 300), (64, 128), (1, 5), (0, 1, (1 << 32) + 3), 0x1234567890ABCDEF


def draw_cases():
    """(n_frames, n_lasers, n_sets, step, shuffle); every combination of lasers, sets, steps and shuffle at 5 frames, every frame count once
    with each shuffle."""
    cases = [(5, nl, ns, st, sh) for nl in DRAW_LASERS for ns in DRAW_SETS for st in DRAW_STEPS for sh in (1, 0)]
    cases += [(nf, 64 if nf != 300 else 128, 5, DRAW_STEPS[i % 3], sh) for i, nf in enumerate(DRAW_FRAMES) for sh in (1, 0) if nf != 5]
    return cases


# ---- the main batch ----------------------------------------------------------------------------------------------------------------------
MAIN_SEED, MAIN_STEP, MAIN_SETS = 3, 0, 5
# three wet settings (water_height, pavement_depth, noise_floor, power_factor, delta): 0 and 1 differ in every field
SETTINGS = ((0.0008, 0.001, 0.7, 15.0, 0.5), (0.002, 0.0012, 0.5, 1.0, 0.3), (0.0004, 0.001, 0.7, 15.0, 0.5))
#             snow wet setting
MAIN_FRAMES = ((1, 1, 0), (0, 0, 1), (1, 0, 2), (0, 1, 1), (1, 1, 1), (0, 1, 0), (0, 0, 0), (1, 0, 2))
MAIN_SMALL = 5          # the wet = 1 frame with fewer than 1000 ground rows (flag 1)


def main_frames(dtype=np.float32):
    """Eight ragged sweeps: 64 x 256 (frame 4 in firing order), frame 5 a 64 x 17 sweep with fewer than 1000 ground rows, frame 7 64 x 128."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    out = []
    for f in range(8):
        az = 17 if f == MAIN_SMALL else 128 if f == 7 else 256
        pc = synthetic_sweep(64, az, seed=1050 + f, intensity="lambert")
        out.append((ami.firing(pc) if f == 4 else pc).astype(dtype))
    return out


def main_masks(frames):
    """A ragged mask: Bernoulli(0.8) per frame, and the last 1000 rows of frames 2 and 3 absent (padding of an F x Nmax batch)."""
    masks = [ami.bernoulli(len(f), 0.8, 5100 + i) for i, f in enumerate(frames)]
    for f in (2, 3):
        masks[f][-1000:] = False
    return masks


def main_records(spec=MAIN_FRAMES):
    rec = np.zeros((len(spec), 8), np.float64)
    for f, (snow, wet, k) in enumerate(spec):
        rec[f, :7] = (snow, wet) + SETTINGS[k]
    return rec


def table_sets(tables4, n_sets=MAIN_SETS, n_lasers=64):
    """n_sets table lists of n_lasers tables from the four golden tables: set s gives line c the table (c + s) % 4."""
    return [[tables4[(c + s) % 4] for c in range(n_lasers)] for s in range(n_sets)]


def ground_rows(pc, m, delta):
    """Present rows of pc within delta of PLANE4 (augmentation.py:43-47)."""
    hog = np.matmul(pc[m][:, :3].astype(np.float64), np.asarray(PLANE4[:3])) + PLANE4[3]
    return int((np.abs(hog) < delta).sum())


def poison(frames, which):
    """Copies of the frames with NaN, a 500 m range and channel 999 in every row of the frames `which`."""
    out = [f.copy() for f in frames]
    for f in which:
        out[f][0::3, 0:3] = np.nan
        out[f][1::3, 0] = 500.0
        out[f][2::3, 4] = 999.0
        out[f][0::3, 4] = 999.0
    return out
