"""One more input of the range-index GPU tests (tests/test_gpu_fine_index.py), NumPy only: a 64-channel x 64-azimuth frame whose ranges sit
on the 2 m edges of the step-major index the library files (csrc/sg_range_index.h) and at the exact ranges of records of a hand-made
table.  With that index the scan takes every record below the upper count of the target's step as a candidate and drops those at or beyond
the target in its pair loop (sg_beam.h: sg_wave_scan), so these are the rows where a dropped candidate is nearest to counting.

As in tests/range_index_inputs.py, rows from 120.002 m on lie in the flake-free sector FREE (the reference raises once such a row meets a
flake): that is where the last step of the index (126 m on) is reached."""
import numpy as np

import range_index_inputs as rii

RECORD_RANGES = np.array([3.0, 5.5, 10.25, 20.5, 33.25, 60.125, 100.0625])     # exact in float32, none on a 2 m edge


def table():
    """Flakes on the +x axis (the 0 / 2 pi seam: filed under the last bin and bin 0) at RECORD_RANGES and on the 2 m edges 2, 4 .. 118 m
    -- there the range is the x coordinate, exactly --, sixty flakes inside the one step 40 - 42 m a little to either side of the axis, and
    1500 random ones."""
    rng = np.random.default_rng(9101)
    on_axis = np.concatenate((RECORD_RANGES, 2.0 * np.arange(1, 60)))
    axis = np.column_stack((on_axis, np.zeros(on_axis.size), np.where(on_axis < 30, 0.004, 0.012)))
    rho = 40.0 + 2.0 * (np.arange(60) + 0.5) / 60.0
    phi = np.where(np.arange(60) % 2 == 0, 1.0, -1.0) * rng.uniform(0.0004, 0.0010, 60)
    crowd = np.column_stack((rho * np.cos(phi), rho * np.sin(phi), np.full(60, 0.006)))
    k = 1500
    rnd = rii._flakes(np.sqrt(rng.uniform(0.5 ** 2, 125.0 ** 2, k)), rng.uniform(0, 2 * np.pi, k), np.minimum(rng.exponential(4e-3, k) + 5e-4, 0.03))
    return np.concatenate((axis, crowd, rnd))


def tables():
    return [table()] * rii.N_CH


def fine_frame(dtype=np.float32):
    """Per channel, all on the +x axis unless said otherwise: 30 targets at exactly 2, 4 .. 60 m; 10 on 2 m edges between 62 and 118 m
    (which ones turns with the channel); 7 at RECORD_RANGES and 7 at those ranges give or take a rounding; 4 inside and at the ends of the
    crowded step 40 - 42 m; 4 in the flake-free sector at 126, 128, 130 and 200 m; 2 random."""
    rng = np.random.default_rng(9102)
    n_ch, n_az = rii.N_CH, rii.N_AZ
    d = np.exp(rng.uniform(np.log(1.0), np.log(119.0), (n_ch, n_az)))
    az = rng.uniform(-np.pi, np.pi, (n_ch, n_az))
    az[(az > rii.FREE[0] - 0.05) & (az < rii.FREE[1] + 0.05)] -= 1.0
    el = np.zeros((n_ch, n_az))
    ch = np.arange(n_ch)[:, None]
    d[:, 0:30] = 2.0 * np.arange(1, 31); az[:, 0:30] = 0.0
    d[:, 30:40] = 2.0 * (31 + (ch + 3 * np.arange(10)[None, :]) % 29); az[:, 30:40] = 0.0
    d[:, 40:47] = RECORD_RANGES; az[:, 40:47] = 0.0
    d[:, 47:54] = RECORD_RANGES * (1.0 + rng.integers(-1, 2, (n_ch, 7)) * 2.0 ** -22); az[:, 47:54] = 0.0
    d[:, 54:58] = np.array([40.0, 40.5, 41.99, 42.0]); az[:, 54:58] = rng.uniform(-3e-4, 3e-4, (n_ch, 4))
    d[:, 58:62] = np.array([126.0, 128.0, 130.0, 200.0]); az[:, 58:62] = rng.uniform(rii.FREE[0], rii.FREE[1], (n_ch, 4))
    return rii._frame(d, az, el, rng, dtype)
