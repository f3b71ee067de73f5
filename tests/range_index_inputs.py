"""Inputs of tests/test_gpu_range_index.py, made on any machine (NumPy only): two 64-channel x 64-azimuth frames and three table sets
that lean on the scan's coarse range index (csrc/sg_range_index.h).  tests/test_range_index.py checks, without a GPU, that the CPU
twin and the oracle -- neither uses the index -- agree on them.

A simulated point from 120.002 m on is an IndexError in the reference once it meets a flake (simulation.py:149), so the rows beyond
that range lie in an azimuth sector (FREE) that every table here keeps clear of flakes; the last step of the index is reached with
flakes around by the rows between 120.0 and 120.002 m."""
import numpy as np

BD = float(np.degrees(3e-3))
POLY = [0.002, -0.1, 12.0]
FREE = (2.0, 2.3)                 # rad: no flake of any table within 0.05 rad of this sector
N_CH, N_AZ = 64, 64


def _frame(d, az, el, rng, dtype):
    """channel-major rows: a wave of the pass over all rows is the 64 azimuths of one channel"""
    x, y, z = d * np.cos(el) * np.cos(az), d * np.cos(el) * np.sin(az), d * np.sin(el)
    ch = np.repeat(np.arange(N_CH), N_AZ).astype(np.float64)
    return np.column_stack((x.ravel(), y.ravel(), z.ravel(), rng.integers(0, 256, N_CH * N_AZ).astype(np.float64), ch)).astype(dtype)


def seam_frame(dtype=np.float32):
    """Every channel's 64 azimuths run from -47 to +47 mrad in steps of half a bin: each wave straddles the 0 / 2 pi seam (first bin
    n_bins - 1, next bin 0 for the beams around azimuth 0)."""
    rng = np.random.default_rng(7001)
    az = np.tile((np.arange(N_AZ) - 31.5) * 1.5e-3, (N_CH, 1))
    el = np.repeat(np.linspace(-0.4, 0.03, N_CH), N_AZ).reshape(N_CH, N_AZ)
    d = np.exp(rng.uniform(np.log(2.0), np.log(119.0), (N_CH, N_AZ)))
    return _frame(d, az, el, rng, dtype)


def edge_frame(dtype=np.float32):
    """Per channel: 15 targets at exactly 8, 16 .. 120 m on the +x axis (the seam), 15 at those ranges give or take a rounding at other
    azimuths, 8 between 120.0 and 120.002 m, 8 beyond 120 m in the flake-free sector, 4 with NaN coordinates, 14 random."""
    rng = np.random.default_rng(7002)
    d = np.exp(rng.uniform(np.log(1.0), np.log(119.0), (N_CH, N_AZ)))
    az = rng.uniform(-np.pi, np.pi, (N_CH, N_AZ))
    az[(az > FREE[0] - 0.05) & (az < FREE[1] + 0.05)] -= 1.0
    el = np.zeros((N_CH, N_AZ))
    edges = 8.0 * np.arange(1, 16)
    d[:, 0:15] = edges; az[:, 0:15] = 0.0
    d[:, 15:30] = edges * (1.0 + rng.integers(-1, 2, (N_CH, 15)) * 2.0 ** -22)
    d[:, 30:38] = rng.uniform(120.0, 120.0015, (N_CH, 8))
    az[:, 30:34] = rng.uniform(-3e-3, 3e-3, (N_CH, 4))
    d[:, 38:46] = np.exp(rng.uniform(np.log(120.01), np.log(400.0), (N_CH, 8)))
    az[:, 38:46] = rng.uniform(FREE[0], FREE[1], (N_CH, 8))
    f = _frame(d, az, el, rng, dtype).reshape(N_CH, N_AZ, 5)
    f[:, 46, 0] = np.nan
    f[:, 47, 1] = np.nan
    f[:, 48, 2] = np.nan
    f[:, 49, 0:3] = np.nan
    return np.ascontiguousarray(f.reshape(-1, 5))


def _flakes(rho, phi, r):
    keep = ~((phi > FREE[0] - 0.05) & (phi < FREE[1] + 0.05))
    return np.column_stack((rho * np.cos(phi), rho * np.sin(phi), r))[keep]


def table_sets():
    """name -> 64 tables (index = channel): two small random tables in turn; empty tables; a table with 400 of its 900 flakes in one
    azimuth bin at the seam (a beam there meets more flakes than any list tier but the global one holds)."""
    rng = np.random.default_rng(7003)
    small = []
    for _ in range(2):
        k = 4000
        small.append(_flakes(np.sqrt(rng.uniform(0.5 ** 2, 125.0 ** 2, k)), rng.uniform(0, 2 * np.pi, k), np.minimum(rng.exponential(4e-3, k) + 5e-4, 0.03)))
    empty = np.zeros((0, 3))
    rho = np.concatenate((rng.uniform(1.0, 121.0, 400), np.sqrt(rng.uniform(1.0, 125.0 ** 2, 500))))
    phi = np.concatenate((rng.uniform(0.0006, 0.0024, 400), rng.uniform(0, 2 * np.pi, 500)))
    heavy = _flakes(rho, phi, np.concatenate((np.full(400, 4e-4), rng.uniform(1e-3, 0.02, 500))))
    return {"small": [small[c % 2] for c in range(N_CH)], "empty": [empty] * N_CH, "heavy": [heavy] * N_CH}
