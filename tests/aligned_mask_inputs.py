"""Inputs of tests/test_gpu_aligned_mask.py, made on any machine (NumPy only): frames, input keep masks, the pre-crop sweep and its
calibration.  tests/test_aligned_mask_inputs.py checks, without a GPU, that they are what the GPU tests take them for."""
import numpy as np

from lidar_snow_sim_amd.calibration import Calibration
from lidar_snow_sim_amd.synthetic import synthetic_sweep

PLANE = (np.array([0.0, 0.0, -1.0]), -1.7)
BD = float(np.degrees(3e-3))
IMG = (1024, 1920)
# the narrow camera of tests/test_gpu_parity.py::test_pre_crop_with_odd_channel_values_and_plane_from_the_cropped_cloud
NARROW = dict(P2=np.array([[7000.0, 0, 960, 0], [0, 700.0, 512, 0], [0, 0, 1, 0]]), R0=np.eye(3),
              V2C=np.array([[0, -1.0, 0, 0], [0, 0, -1.0, 0], [1.0, 0, 0, 0]]))


def narrow_calib():
    return Calibration(**NARROW)


def firing(frame, channels=64):
    """A channel-major frame (channels x azimuths) re-ordered azimuth-major: firing order, which the channel sort has to permute."""
    return np.ascontiguousarray(frame.reshape(channels, -1, 5).transpose(1, 0, 2).reshape(-1, 5))


def ragged_frames(dtype=np.float32):
    """The three ragged frames of tests/test_gpu_aligned.py (16 384 / 8 192 / 16 384 rows), the middle one in firing order."""
    full = [synthetic_sweep(64, 2048, seed=1200 + f, intensity="lambert").reshape(64, 2048, 5) for f in range(3)]
    fr = [np.ascontiguousarray(full[0][:, ::8, :].reshape(-1, 5)), firing(np.ascontiguousarray(full[1][:, 1::16, :].reshape(-1, 5))),
          np.ascontiguousarray(full[2][:, 3::8, :].reshape(-1, 5))]
    return [f.astype(dtype) for f in fr]


def bernoulli(n, p, seed):
    return np.random.default_rng(seed).random(n) < p


def ragged_masks():
    """Bernoulli(0.7) masks of the three ragged frames, fixed seed."""
    return [bernoulli(n, 0.7, 4100 + f) for f, n in enumerate((16384, 8192, 16384))]


def exactly(n, k, seed):
    """A mask of n rows with exactly k of them present, scattered."""
    m = np.zeros(n, bool)
    m[np.random.default_rng(seed).permutation(n)[:k]] = True
    return m


EDGE_NAMES = ("p1023", "p1024", "p1025", "last_of_1025", "all_present", "all_absent", "empty", "wave_edges")
EDGE_PRESENT = (1023, 1024, 1025, 1, 2000, 0, 0, 128)


def edge_batch():
    """(frames, masks) of the edge test: a 5 000-row firing-order frame with exactly 1 023 / 1 024 / 1 025 present rows, a 1 025-row frame
    with only its last row present, an all-present, an all-absent and an empty frame, and a 4 096-row frame whose present rows are the
    first and the last lane of every wave (rows = 0 or 63 mod 64)."""
    full = synthetic_sweep(64, 2048, seed=1410, intensity="lambert").reshape(64, 2048, 5)
    sl = lambda k, n: np.ascontiguousarray(full[:, k::16].reshape(-1, 5)[:n])     # noqa: E731  (channel-sorted)
    fire = firing(np.ascontiguousarray(full[:, 5::16].reshape(-1, 5)))[:5000]
    last = np.zeros(1025, bool)
    last[-1] = True
    lanes = np.arange(4096) % 64
    frames = [fire, fire.copy(), fire.copy(), sl(4, 1025), sl(3, 2000), sl(2, 2000), np.zeros((0, 5), np.float32), sl(1, 4096)]
    masks = [exactly(5000, 1023, 1), exactly(5000, 1024, 2), exactly(5000, 1025, 3), last, np.ones(2000, bool), np.zeros(2000, bool),
             np.zeros(0, bool), (lanes == 0) | (lanes == 63)]
    return frames, masks


def quarter_sweeps():
    """20 quarter sweeps of 32 768 rows: 655 360 rows, above the 16-frame prepass switch and above 2^19 rows."""
    full = [synthetic_sweep(64, 2048, seed=1420 + f, intensity="lambert") for f in range(5)]
    return [np.ascontiguousarray(s.reshape(64, 2048, 5)[:, q::4].reshape(-1, 5)) for s in full for q in range(4)]


# Bernoulli(0.5) leaves about 327 680 of the 655 360 rows: the present total is below 2^19 while n_total is above it -- the masked call
# takes the large-batch side of every switch, the call on compacted frames the small-batch side.  Bernoulli(0.9) leaves about 589 824:
# both calls on the large-batch side.
SWITCH_P = {"half": 0.5, "dense": 0.9}


def switch_masks(case):
    return [bernoulli(32768, SWITCH_P[case], 4200 + f) for f in range(20)]


def precrop_sweep():
    """One 64 x 512 synthetic sweep for the pre-crop and fov_keep tests."""
    return np.ascontiguousarray(synthetic_sweep(64, 512, seed=1500, intensity="lambert"))


def fov_reference(pc, calib=None, img=IMG):
    """(flag, decided): calibration.get_fov_flag in float64 NumPy, and the rows whose pixel coordinates lie farther than 1e-6 from every
    image edge and whose depth lies farther than 1e-9 from 0 -- the rows on which any float64 evaluation order gives the same flag."""
    from lidar_snow_sim_amd.calibration import get_fov_flag
    calib = calib or narrow_calib()
    rect = calib.lidar_to_rect(pc[:, 0:3].astype(np.float64))
    flag = get_fov_flag(rect, img, calib)
    with np.errstate(all="ignore"):
        uv, depth = calib.rect_to_img(rect)
    near = (np.abs(uv[:, 0]) <= 1e-6) | (np.abs(uv[:, 0] - img[1]) <= 1e-6) | (np.abs(uv[:, 1]) <= 1e-6) | (np.abs(uv[:, 1] - img[0]) <= 1e-6) | \
           (np.abs(depth) <= 1e-9) | ~np.isfinite(uv).all(axis=1)
    return flag, ~near


def fused_frames(dtype=np.float32):
    """The frames of the fused-chain test of tests/test_gpu_wet_aligned.py: two with thousands of ground rows (one in firing order), one
    with fewer than 1 000, and their Bernoulli(0.7) masks."""
    base = [synthetic_sweep(64, 512, seed=1300, intensity="lambert"), firing(synthetic_sweep(64, 256, seed=1301, intensity="lambert")),
            synthetic_sweep(64, 17, seed=1303, intensity="lambert")]
    return [f.astype(dtype) for f in base], [bernoulli(len(f), 0.7, 4300 + i) for i, f in enumerate(base)]


def present_ground_rows(pc, m, delta=0.5):
    """Present rows of pc within `delta` of the plane the fused test hands to the wet stage (augmentation.py:43-47)."""
    hog = np.matmul(pc[m][:, :3].astype(np.float64), PLANE[0]) + PLANE[1]
    return int((np.abs(hog) < delta).sum())
