"""Inputs of tests/test_gpu_scan_segments.py, made on any machine (NumPy only): one batch of four frames -- three with a few thousand rows
and an empty one -- whose (frame, channel) segments are ragged, for the segment order of the pass over all rows (csrc/snowgpu_kernels.hip:
k_beams, SEG), where a block serves one segment and keeps its frame, channel, row base and table descriptor in scalar registers.
tests/test_scan_segments.py checks, without a GPU, that the CPU twin and the oracle agree on them.

The tables, BD, POLY and the flake-free sector FREE are those of tests/range_index_inputs.py: a simulated point from 120.002 m on raises in the
reference once it meets a flake, so every simulated range here stays below 120 m outside that sector."""
import numpy as np

import range_index_inputs as rii

BD, POLY, FREE = rii.BD, rii.POLY, rii.FREE
N_LASERS = 64
WIDE = 3.0                         # the wide-wedge case: BD * WIDE spans three azimuth bins (2048 bins of 3.07 mrad, BD = 3 mrad)
BLOCK = 256                        # beams per block of the pass over all rows (its first tier)

# rows per channel of the ragged frames.  0, 1, 63, 64, 65: segments shorter than, equal to and just over a wave; 255, 256, 257, 300: a partial
# last block, a full block and segments of two blocks; channel 1 is empty between two full ones.  Channels 64, 100 and 255 have no laser:
# their rows are copied through.
RAGGED = {0: 256, 1: 0, 2: 257, 3: 1, 4: 63, 5: 64, 6: 65, 7: 255, 8: 300, 64: 40, 100: 70, 255: 3}
CASES = [("small", 1.0), ("heavy", 1.0), ("empty", 1.0), ("small", WIDE)]      # table set, beam divergence / BD


def counts():
    c = dict(RAGGED)
    for ch in range(9, N_LASERS):
        c[ch] = 17 + 13 * (ch % 5)
    return c


def _rows(seed, dtype):
    """channel-major rows with counts() rows per channel; per channel its first rows lie on or next to the 0 / 2 pi seam, one has a NaN
    coordinate, one lies beyond 120 m in the flake-free sector, a few carry an intensity that is no integer in [0, 255]"""
    rng = np.random.default_rng(seed)
    out = []
    for ch, n in sorted(counts().items()):
        if n == 0:
            continue
        d = np.exp(rng.uniform(np.log(1.5), np.log(119.0), n))
        az = rng.uniform(-np.pi, np.pi, n)
        az[(az > FREE[0] - 0.05) & (az < FREE[1] + 0.05)] -= 1.0
        k = min(n, 12)
        az[:k] = ((np.arange(k) - 5.5) * 1.5e-3)                     # -8 .. +10 mrad: first bin the last one, next bin 0
        if n > 3:
            az[3] = 0.0
        el = -0.4 + 0.43 * (ch % N_LASERS) / (N_LASERS - 1)
        inten = rng.integers(0, 256, n).astype(np.float64)
        if n > 20:
            d[15] = rng.uniform(121.0, 300.0); az[15] = rng.uniform(FREE[0], FREE[1])
            inten[16] = 12.5; inten[17] = 300.0; inten[18] = -1.0
        r = np.column_stack((d * np.cos(el) * np.cos(az), d * np.cos(el) * np.sin(az), d * np.full(n, np.sin(el)), inten, np.full(n, float(ch))))
        if n > 20:
            r[19, int(rng.integers(0, 3))] = np.nan
        out.append(r)
    return np.concatenate(out).astype(dtype)


def frames(dtype=np.float32):
    """[channel-sorted ragged frame (read in place), the same kind in firing order (the device sorts a copy), empty frame, the seam / step-edge /
    NaN frame of range_index_inputs (channel-sorted, every segment one wave)]"""
    a = _rows(8101, dtype)
    b = _rows(8102, dtype)
    b = b[np.random.default_rng(8103).permutation(b.shape[0])]
    return [a, b, np.zeros((0, 5), dtype), rii.edge_frame(dtype)]


def table_sets():
    return rii.table_sets()


def orders():
    """per frame the channel -> table permutation: the identity, a rotation, the identity, a reversal"""
    o = list(range(N_LASERS))
    return [o, o[7:] + o[:7], o, o[::-1]]
