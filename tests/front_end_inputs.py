"""Inputs of tests/test_gpu_front_end.py, made on any machine (NumPy only): frames that put the channel sort and the segment builder
(csrc/snowgpu_sort.hip) at their structural edges.  tests/test_front_end_inputs.py checks, without a GPU, that the CPU twin and the oracle
agree on them and that they are what they are taken for.

Every frame is a channel-major pool of rows (geometry as tests/scan_segment_inputs.py: ranges below 119 m outside the flake-free sector
FREE, rows on the 0 / 2 pi seam, NaN coordinates, intensities no record can carry; the tables, BD and POLY of tests/range_index_inputs.py)
whose rows are re-ordered, nothing else:

  two_runs(n, p)   rows [0, p) and [p, n) each non-descending in channel and ch[p] < ch[p - 1]: ONE descent, at p.  k_sort_hist declares a
                   frame unsorted from per-lane comparisons; for p a multiple of 64 the comparison is the one of lane 0 with the separately
                   loaded channel of the row before (an earlier round, wave or tile).
  level(n, p)      channel-sorted with ch[p] == ch[p - 1]: no descent, read in place.
  THIRTEEN         two_runs(2500, p) for p on and next to round, wave and tile borders: thirteen equal-sized frames in one batch.
  ragged()         nine frames of 2 .. 2049 rows, an empty one among them: more than four, so the three-kernel segment builder.
  rank_frames()    more than 64 distinct channel values, one channel over three tiles, two channels alternating, waves of one channel
                   beside waves of 64."""
import numpy as np

import range_index_inputs as rii

BD, POLY, FREE = rii.BD, rii.POLY, rii.FREE
N_LASERS = 64
TILE = 1024                        # rows per block of the sort (SG_TILE): four waves of four rounds of 64
N = 2500                           # three tiles, the last partial
P_TWO_RUNS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2499]
P_LEVEL = [64, 256, 1024]
RAGGED_TWO_RUNS = [(2, 1), (65, 64), (1025, 1024), (2049, 1024)]
NO_LASER = [64, 100, 255]          # channels without a laser: their rows are copied through
SETS = ["small", "empty"]          # the table sets of the GPU test


def _channels(rng, n):
    """n channels, non-descending, the first smaller than the last for n >= 2: the 64 lasers and, more rarely, channels without one"""
    pool = np.array(list(range(N_LASERS)) + NO_LASER)
    if n <= len(pool):
        return np.sort(rng.choice(pool, n, replace=False)).astype(np.float64)
    w = np.array([1.0] * N_LASERS + [0.4] * len(NO_LASER))
    return np.sort(rng.choice(pool, n, p=w / w.sum())).astype(np.float64)


def _rows(ch, rng, dtype):
    """one row per entry of ch (non-descending).  Per run of a channel: its first rows lie on or next to the 0 / 2 pi seam; in a run of more
    than 20 rows one lies beyond 120 m in the flake-free sector, three carry an intensity that is no integer in [0, 255], one has a NaN
    coordinate."""
    n = ch.shape[0]
    d = np.exp(rng.uniform(np.log(1.5), np.log(119.0), n))
    az = rng.uniform(-np.pi, np.pi, n)
    az[(az > FREE[0] - 0.05) & (az < FREE[1] + 0.05)] -= 1.0
    el = -0.4 + 0.43 * (ch % N_LASERS) / (N_LASERS - 1)
    inten = rng.integers(0, 256, n).astype(np.float64)
    nan_at = []
    start = np.flatnonzero(np.concatenate(([True], ch[1:] != ch[:-1], [True])))
    for a, b in zip(start[:-1], start[1:]):
        k = min(b - a, 12)
        az[a:a + k] = (np.arange(k) - 5.5) * 1.5e-3                  # -8 .. +8 mrad: first bin the last one, next bin 0
        if b - a > 3:
            az[a + 3] = 0.0
        if b - a > 20:
            d[a + 15] = rng.uniform(121.0, 300.0); az[a + 15] = rng.uniform(FREE[0], FREE[1])
            inten[a + 16] = 12.5; inten[a + 17] = 300.0; inten[a + 18] = -1.0
            nan_at.append((a + 19, int(rng.integers(0, 3))))
    r = np.column_stack((d * np.cos(el) * np.cos(az), d * np.cos(el) * np.sin(az), d * np.sin(el), inten, ch))
    for i, j in nan_at:
        r[i, j] = np.nan
    return r.astype(dtype)


def pool(n, seed, dtype=np.float32):
    """a channel-major frame of n rows"""
    rng = np.random.default_rng(seed)
    return _rows(_channels(rng, n), rng, dtype)


def two_runs(n, p, seed, dtype=np.float32):
    """pool(n) as two channel-major pieces appended to each other: p rows of the pool, its last one (the largest channel) among them and its
    first one (the smallest) not, in the pool's order; then the other n - p in the pool's order"""
    assert 1 <= p < n
    rng = np.random.default_rng(seed)
    rows = _rows(_channels(rng, n), rng, dtype)
    first = np.zeros(n, bool)
    first[n - 1] = True
    first[1 + rng.choice(n - 2, p - 1, replace=False)] = True        # (of rows 1 .. n - 2)
    return np.ascontiguousarray(np.concatenate((rows[first], rows[~first])))


def level(n, p, seed, dtype=np.float32):
    """a channel-major frame whose rows p - 1 and p have one channel"""
    rng = np.random.default_rng(seed)
    ch = _channels(rng, n)
    ch[p] = ch[p - 1]
    return _rows(ch, rng, dtype)


def in_order(ch, seed, dtype=np.float32):
    """the frame whose row i has channel ch[i]: a channel-major pool with those channels, re-ordered"""
    ch = np.asarray(ch, np.float64)
    o = np.argsort(ch, kind="stable")
    rows = _rows(ch[o], np.random.default_rng(seed), dtype)
    out = np.empty_like(rows)
    out[o] = rows
    return out


def thirteen(dtype=np.float32):
    """two_runs(N, p) for every p of P_TWO_RUNS: equal-sized frames"""
    return [two_runs(N, p, 9100 + i, dtype) for i, p in enumerate(P_TWO_RUNS)]


def levels(dtype=np.float32):
    return [level(N, p, 9200 + i, dtype) for i, p in enumerate(P_LEVEL)]


RAGGED_KIND = ["two_runs"] * 4 + ["sorted", "sorted", "empty", "one_row", "descending"]


def ragged(dtype=np.float32):
    """nine frames: two_runs at RAGGED_TWO_RUNS, channel-sorted frames of 1023 and 1024 rows, an empty frame, a one-row frame, 2049 rows in
    descending channel order"""
    fr = [two_runs(n, p, 9300 + i, dtype) for i, (n, p) in enumerate(RAGGED_TWO_RUNS)]
    fr += [pool(1023, 9310, dtype), pool(1024, 9311, dtype), np.zeros((0, 5), dtype), pool(1, 9312, dtype)]
    fr.append(np.ascontiguousarray(pool(2049, 9313, dtype)[::-1]))
    return fr


def mixed_waves_channels(n=N):
    """64-row stretches: all of one channel (another one each time), then one row of each of 64 channels in a shuffled order, in turn"""
    rng = np.random.default_rng(9420)
    ch = np.empty(n)
    for k, a in enumerate(range(0, n, 64)):
        m = min(64, n - a)
        ch[a:a + m] = rng.permutation(N_LASERS)[:m] if k % 2 else (7 * k) % N_LASERS
    return ch


RANK_NAMES = ["all256", "one_channel", "alternate", "mixed_waves"]


def rank_frames(dtype=np.float32):
    """all256: channel = row index mod 256 (channels 64 and up have no laser); one_channel: every row channel 5; alternate: 63, 0, 63, 0,
    ...; mixed_waves: see mixed_waves_channels"""
    i = np.arange(N)
    return [in_order(i % 256, 9401, dtype), in_order(np.full(N, 5.0), 9402, dtype), in_order(np.where(i % 2 == 0, 63.0, 0.0), 9403, dtype),
            in_order(mixed_waves_channels(), 9404, dtype)]


def batches(dtype=np.float32):
    """name -> the frames of one call of the GPU test"""
    return {"thirteen": thirteen(dtype), "levels": levels(dtype), "ragged": ragged(dtype), "ranks": rank_frames(dtype)}


def orders(n_frames):
    """per frame the channel -> table permutation: the identity, a rotation and a reversal, in turn"""
    o = list(range(N_LASERS))
    return [[o, o[7:] + o[:7], o[::-1]][f % 3] for f in range(n_frames)]


def table_sets():
    return rii.table_sets()


def descents(frame):
    """the rows whose channel is smaller than that of the row before"""
    return 1 + np.flatnonzero(np.diff(frame[:, 4]) < 0)


def moved(frame):
    """the rows that the stable sort by channel moves to another place"""
    o = np.argsort(frame[:, 4], kind="stable")
    return o[o != np.arange(o.shape[0])]
