"""Inputs of tests/test_gpu_row_tiers.py, made on any machine (NumPy only): small frames whose beams are CONSTRUCTED to take the rare
branches of the row kernels (csrc/snowgpu_rows.hip: rw_slot_walk, rw_scan_sort, rw_zone, the stage-B pair numbering) and of the list-mode
form of the same tiers (k_beams + k_power), with the flake tables that go with them.  tests/test_row_tier_inputs.py checks, without a
GPU, that every beam is what its name claims, and records what the GPU test compares the status words with.

A beam of azimuth az and range D sees the wedge [az - w / 2, az + w / 2] (w = the beam divergence in rad).  A flake at range rho whose
centre lies at azimuth az + c and whose radius is rho sin(h) covers [az + c - h, az + c + h]; where it crosses a limit ray the interval is
clipped to it (geometry.py:14-29).  compute_occlusion_dict (simulation.py:252-295) cuts the wedge at every interval end into elementary
slots; a slot belongs to the nearest flake that covers it, else to the hard target.  So, per beam:

  umbrella(m)   the nearest flake covers the whole wedge, m farther ones lie strictly inside, pairwise disjoint: L = m + 1 flakes meet the
                beam, the nearest owns all 2 m + 1 slots, the others none (they vanish from the dict), the target none (ratio exactly 0).
                umbrella(3) meets 4 flakes, which the pass over all rows holds; umbrella3_twin has one inner flake twice in its table:
                5 flakes, still 7 slots -- a beam of the 8-entry class that is NOT redone, next to umbrella(4), which is.
  comb(m)       m pairwise disjoint flakes with gaps between them and towards both limit rays: L = m, every flake owns one slot, the
                target m + 1.
  both(k, m)    a near flake over the right part of the wedge (clipped to the right limit ray) with k farther flakes inside it, and a
                comb of m over the left part: L = 1 + k + m, the near flake owns 2 k + 1 slots, the target m + 1.
  eclipsed      a comb one of whose table rows appears twice, byte for byte (equal ranges: the copy later in scan order owns nothing),
                and a comb with one more flake wholly behind a nearer one, at a middle range (S < L, the lane that owns nothing in the
                middle of the row).
  seam          beams whose wedge straddles azimuth 0 (theta_r > theta_l), one inner flake's own interval wrapping: umbrella(4) and
                comb(7) with the wrapping flake the rightmost one.  The reference moves a flake's right end by -2 pi only where it
                exceeds the left end (:262-263), so a flake wholly right of azimuth 0 keeps its angles near 2 pi, owns a slot out there,
                and the gap of almost 2 pi before it goes to the target (ratio clipped to 1).  seam_right8 / 16 / 63 are umbrellas with
                1 / 2 / 4 such flakes, redone in the 8-, 16- and 63-entry tier; seam_comb_t24 a comb with three.  All look at
                azimuth 0, so each has a channel (SEAM_CHANNELS) and a table of its own.
  near0         the only beams whose ratios depend on the ORDER of their sums.  Away from azimuth 0 every angle of a wedge lies in one
                binade: the slot widths are multiples of one ulp and every partial sum is exact, so NumPy's blocked pairwise sum, a
                running sum and any other order agree to the last bit.  And the slots of an umbrella lie side by side: their sum
                telescopes.  shaded(n, k) beams 1.6 .. 1.8 mrad left of azimuth 0 (angles of 0.1 .. 3.3 mrad: five binades) whose
                umbrella is shaded by n nearer flakes, so that its 2 k + n + 1 slots lie apart, are redone in the 8-, 16- and
                63-entry tier with a ratio that a running sum gets wrong in the last bit; comb(16) and comb(23) there do the same
                for the target's sum.  One channel and one table each (NEAR0_CHANNELS).
  bins          an umbrella whose nearest flake is filed under four or more azimuth bins of its table; the wedge holds a bin edge.
  partial       comb(5) / comb(12) / comb(20) beams (PARTIAL_L) that bring the 8-, 16- and 63-entry classes to lengths that are no multiple of the
                beams per wave (8, 4) -- together with everything else in the frame; test_row_tier_inputs.py asserts the lengths.

Every gap, every distance of an interval end to a limit ray and every difference between two flakes' ranges is at least GAP = 1e-5 rad /
0.1 m: float32 rows move a beam's azimuth by less than 1e-6 rad, so one set of tables serves both dtypes.

Frames.  The beams of a case live on one channel (CASE_CHANNEL), whose table holds the constructed flakes alone; the other 46 channels
carry three ordinary beams each against the fixture tables (tests/golden/tables.npz, t0 .. t3 in turn).  frames(dtype) returns
  main     every case at BD = np.degrees(3e-3);
  wide     comb and both at BD_WIDE = np.degrees(3e-2), ordinary beams;
  single   one umbrella(4) beam and ordinary beams so short that none meets five flakes: one beam in the 8-entry class, none elsewhere;
  plain    ordinary beams only."""
from functools import lru_cache
from pathlib import Path

import numpy as np

BD = float(np.degrees(3e-3))
BD_WIDE = float(np.degrees(3e-2))
POLY = [0.0, 0.01, 2.0]
N_LASERS = 64
TWO_PI = 2 * np.pi
GAP = 1e-5                          # rad
D_TARGET = 60.0                     # m: range of every constructed beam; every constructed flake is nearer than 45 m
CASE_CHANNEL = {"umbrella": 3, "edges": 10, "comb": 17, "both": 24, "eclipsed": 31, "seam": 38, "bins": 45, "near0": 46, "partial": 52}
SEAM_CHANNELS = (38, 39, 40, 41, 42, 43)     # the seam beams all look at azimuth 0: each has a channel, and so a table, of its own
# name, kind, m, and the flake whose centre lies 1e-5 rad left of azimuth 0: the flakes before it lie wholly right of azimuth 0
SEAM_BEAMS = (("seam_umbrella4", "umbrella", 4, 1), ("seam_comb_t8", "comb", 7, 0), ("seam_right8", "umbrella", 6, 2),
              ("seam_right16", "umbrella", 10, 3), ("seam_right63", "umbrella", 30, 5), ("seam_comb_t24", "comb", 23, 3))
NEAR0_CHANNELS = (46, 47, 48, 49, 50)        # ... and so do the beams just left of azimuth 0
# name, kind, size, azimuth.  The azimuths were chosen, in steps of 1e-5 rad, so that the ORDER of the sum shows in the ratio of the
# umbrella (shaded) or of the target (comb) for float32 and float64 rows: tests/test_row_tier_inputs.py asserts that it does.
NEAR0_BEAMS = (("near0_shaded8", "shaded", (3, 3), 1.70e-3), ("near0_shaded16", "shaded", (6, 5), 1.81e-3),
               ("near0_shaded63", "shaded", (10, 10), 1.71e-3), ("near0_comb_t17", "comb", 16, 1.60e-3), ("near0_comb_t24", "comb", 23, 1.75e-3))
CAPS = (4, 8, 16, 63)               # the list capacities (SG_LCAP = 63); beyond: the global-list tier
UMBRELLA_M = (3, 4, 10, 30)         # 7, 9, 21, 61 slots for the nearest flake
EDGE_L = (8, 9, 16, 17, 63, 64)
COMB_TARGET = (7, 8, 9, 15, 16, 17, 24)
BOTH_KM = ((5, 8), (10, 20))
PARTIAL_L = (5, 5, 5, 12, 12, 20)


@lru_cache(maxsize=None)
def fixture_tables():
    t = np.load(Path(__file__).resolve().parent / "golden" / "tables.npz")
    return [t[f"t{i}"] for i in range(4)]


# ---- one beam's flakes, as (offset of the centre from the beam's azimuth, half width, range) ------------------------------------------
def _ranges(m, lo=8.0, hi=40.0, seed=0):
    """m distinct ranges in [lo, hi], at least 0.1 m apart, in an order that is not the angular one"""
    assert m == 0 or (hi - lo) / max(m, 1) >= 0.1
    return lo + (hi - lo) * np.random.default_rng(1000 + 17 * m + seed).permutation(m) / max(m, 1)


def _cells(lo, hi, m):
    """m disjoint intervals inside (lo, hi), one per cell of (hi - lo) / m: centres within a tenth of a cell of the cell's middle, half
    widths of 0.15 .. 0.28 cells -- gaps of at least 0.24 cells, and widths irregular enough that the order of a sum over them shows in
    its last bits (tests/test_row_tier_inputs.py asserts that it does)"""
    cell = (hi - lo) / m
    assert 0.24 * cell >= GAP
    rng = np.random.default_rng(2000 + m)
    return lo + cell * (np.arange(m) + 0.5 + rng.uniform(-0.1, 0.1, m)), cell * rng.uniform(0.15, 0.28, m)


def umbrella(m, w, near=(3.5, 0.58)):
    rho0, cover = near                                               # the nearest flake: half width cover * w > w / 2
    c, h = _cells(-w / 2 + 2 * GAP, w / 2 - 2 * GAP, m)
    return np.concatenate(([0.0], c)), np.concatenate(([cover * w], h)), np.concatenate(([rho0], _ranges(m)))


def comb(m, w):
    c, h = _cells(-w / 2 + 2 * GAP, w / 2 - 2 * GAP, m)
    return c, h, _ranges(m)


def both(k, m, w):
    cu, hu = -0.31 * w, 0.29 * w                                     # [-0.60 w, -0.02 w]: clipped to the right limit ray
    ci, hi = _cells(-0.46 * w, -0.05 * w, k)
    cc, hc = _cells(0.0, w / 2 - 2 * GAP, m)
    return (np.concatenate(([cu], ci, cc)), np.concatenate(([hu], hi, hc)),
            np.concatenate(([3.5], _ranges(k, 8.0, 20.0, seed=1), _ranges(m, 21.0, 40.0, seed=2))))


def hidden(m, w):
    """comb(m) and one flake wholly behind its flake of median range, itself at a range in the middle of the list"""
    c, h, rho = comb(m, w)
    order = np.argsort(rho)
    front, mid = order[1], order[m // 2]
    r_hidden = 0.5 * (rho[mid] + rho[order[m // 2 + 1]])
    return np.concatenate((c, [c[front]])), np.concatenate((h, [h[front] / 2])), np.concatenate((rho, [r_hidden]))


def shaded(n_front, n_behind, w):
    """an umbrella at 3.5 m with n_front small flakes in front of it and n_behind behind it, in alternating cells: the umbrella owns the
    2 n_behind + n_front + 1 slots that the flakes in front leave, and these do not lie side by side"""
    m = n_front + n_behind
    assert n_behind <= n_front <= n_behind + 1
    c, h = _cells(-w / 2 + 2 * GAP, w / 2 - 2 * GAP, m)
    front = np.arange(m) % 2 == 0
    rho = np.empty(m)
    rho[front], rho[~front] = _ranges(n_front, 1.5, 3.0, seed=3), _ranges(n_behind, 8.0, 40.0, seed=4)
    return np.concatenate(([0.0], c)), np.concatenate(([0.58 * w], h)), np.concatenate(([3.5], rho))


def _flakes(az, c, h, rho):
    phi = az + np.asarray(c)
    return np.column_stack((rho * np.cos(phi), rho * np.sin(phi), rho * np.sin(h)))


# ---- frames ----------------------------------------------------------------------------------------------------------------------------
def _rows(az, d, ch, rng, dtype):
    az, d, ch = np.asarray(az, np.float64), np.asarray(d, np.float64), np.asarray(ch, np.float64)
    el = -0.4 + 0.43 * ch / (N_LASERS - 1)
    inten = rng.integers(0, 256, az.shape[0]).astype(np.float64)
    return np.column_stack((d * np.cos(el) * np.cos(az), d * np.cos(el) * np.sin(az), d * np.sin(el), inten, ch)).astype(dtype)


def _ordinary(rng, channels, per_channel, d_lo, d_hi):
    ch = np.repeat(np.asarray(channels), per_channel)
    return rng.uniform(-np.pi, np.pi, ch.shape[0]), np.exp(rng.uniform(np.log(d_lo), np.log(d_hi), ch.shape[0])), ch


def _case_beams(w):
    """case -> [(name, (c, h, rho))] at wedge width w"""
    return {
        "umbrella": [("umbrella3", umbrella(3, w)), ("umbrella3_twin", umbrella(3, w))] + [(f"umbrella{m}", umbrella(m, w)) for m in UMBRELLA_M[1:]],
        "edges": [(f"umbrella_L{L}", umbrella(L - 1, w)) for L in EDGE_L] + [(f"comb_L{L}", comb(L, w)) for L in EDGE_L],
        "comb": [(f"comb_t{t}", comb(t - 1, w)) for t in COMB_TARGET],
        "both": [(f"both{k}_{m}", both(k, m, w)) for k, m in BOTH_KM],
        "eclipsed": [("twice", comb(6, w)), ("hidden", hidden(5, w)), ("twice_hidden", hidden(7, w))],
        "bins": [("bins", umbrella(4, w, near=(1.5, 2.2)))],
        "partial": [(f"partial{i}_L{L}", comb(L, w)) for i, L in enumerate(PARTIAL_L)],
    }


def _build(cases, w, ordinary, seed, dtype, az_step, only=None):
    """rows, tables (64, index = channel), groups: case -> {beam name: row index}; only: the beam names to keep"""
    rng = np.random.default_rng(seed)
    fix = fixture_tables()
    tables = [fix[c % 4] for c in range(N_LASERS)]
    az_all, d_all, ch_all, groups = [], [], [], {}
    beams = _case_beams(w)
    for case in cases:
        ch, groups[case] = CASE_CHANNEL[case], {}
        if case == "seam":
            # the wedge straddles azimuth 0; the beam's azimuth puts the centre of one inner flake 1e-5 rad above 0: its interval wraps
            todo = []
            for k, (name, kind, m, j) in enumerate(SEAM_BEAMS):
                c, h, rho = (umbrella if kind == "umbrella" else comb)(m, w)
                todo.append((name, (c, h, rho), 1e-5 - c[j], SEAM_CHANNELS[k]))
        elif case == "near0":
            todo = []
            for k, (name, kind, m, az) in enumerate(NEAR0_BEAMS):
                todo.append((name, shaded(*m, w) if kind == "shaded" else comb(m, w), az, NEAR0_CHANNELS[k]))
        else:
            todo = []
            for i, (name, chr_) in enumerate(beams[case]):
                az = 0.5 + az_step * i
                if case == "bins":                                   # a bin edge 0.2 mrad left of the wedge's middle
                    az = 700 * TWO_PI / 2048 - 2e-4
                todo.append((name, chr_, az, ch))
        per_channel = {}
        for name, (c, h, rho), az, bch in todo:
            if only is not None and name not in only:
                continue
            fl = _flakes(az, c, h, rho)
            if name.startswith("twice") or name.endswith("_twin"):
                fl = np.concatenate((fl[:3], fl[2:3], fl[3:]))       # table row 2 again, byte for byte
            per_channel.setdefault(bch, []).append(fl)
            groups[case][name] = sum(a.shape[0] for a in az_all)
            az_all.append(np.array([az])); d_all.append(np.array([D_TARGET])); ch_all.append(np.array([bch]))
        for bch, flakes in per_channel.items():
            tables[bch] = np.ascontiguousarray(np.concatenate(flakes))
    if ordinary:
        per_channel, d_lo, d_hi = ordinary
        free = [c for c in range(N_LASERS) if c not in CASE_CHANNEL.values() and c not in SEAM_CHANNELS + NEAR0_CHANNELS]
        az, d, ch = _ordinary(rng, free, per_channel, d_lo, d_hi)
        az_all.append(az); d_all.append(d); ch_all.append(ch)
    az, d, ch = np.concatenate(az_all), np.concatenate(d_all), np.concatenate(ch_all)
    o = np.argsort(ch, kind="stable")                                # channel-major, the beams of a case in the order they were made
    inv = np.empty_like(o)
    inv[o] = np.arange(o.shape[0])
    groups = {case: {name: int(inv[i]) for name, i in g.items()} for case, g in groups.items()}
    rows = _rows(az[o], d[o], ch[o], rng, dtype)
    rows.setflags(write=False)
    for t in tables:
        t.setflags(write=False)
    return dict(rows=rows, tables=tables, groups=groups, bd=float(np.degrees(w)))


@lru_cache(maxsize=None)
def _frames(dtype_name):
    dtype = np.dtype(dtype_name).type
    every = ["umbrella", "edges", "comb", "both", "eclipsed", "seam", "bins", "near0", "partial"]
    return {
        "main": _build(every, 3e-3, (3, 3.0, 119.0), 8101, dtype, az_step=0.05),
        "wide": _build(["comb", "both"], 3e-2, (3, 3.0, 119.0), 8102, dtype, az_step=0.4),
        "single": _build(["umbrella"], 3e-3, (3, 3.0, 10.0), 8103, dtype, az_step=0.05, only={"umbrella4"}),
        "plain": _build([], 3e-3, (3, 3.0, 119.0), 8104, dtype, az_step=0.05),
    }


def frames(dtype=np.float32):
    """name -> dict(rows, tables, groups, bd), read-only"""
    return _frames(np.dtype(dtype).name)


# ---- what the status words must say ------------------------------------------------------------------------------------------------------
def class_populations(n_hit, first=4):
    """status words [2 .. 5] for per-beam intersecting counts n_hit when the pass over all rows runs with capacity `first`: beams handed to
    the following capacities of CAPS, the last one in use being the global-list tier"""
    caps = [c for c in CAPS if c >= first]
    n_hit = np.asarray(n_hit)
    edges = caps + [np.iinfo(np.int64).max]
    pop = [int(((n_hit > lo) & (n_hit <= hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]
    return pop + [0] * (4 - len(pop))


def redo_count(n_hit, max_owner, first=4):
    """status word [6]: beams of the row tiers (more flakes than `first` holds, at most 63) one of whose flakes owns 8 or more slots"""
    n_hit, max_owner = np.asarray(n_hit), np.asarray(max_owner)
    return int(((n_hit > first) & (n_hit <= CAPS[-1]) & (max_owner >= 8)).sum())

# frame -> capacity of the pass over all rows -> (status words [2 .. 5], status word [6]); the same for float32 and float64 rows.
# tests/test_row_tier_inputs.py derives them from its restatement of the reference and asserts these literals.
EXPECTED = {
    "main": {4: ([23, 15, 12, 2], 18), 8: ([15, 12, 2, 0], 12), 16: ([12, 2, 0, 0], 6), 63: ([2, 0, 0, 0], 0)},
    "wide": {4: ([16, 23, 50, 0], 2), 8: ([23, 50, 0, 0], 2), 16: ([50, 0, 0, 0], 1), 63: ([0, 0, 0, 0], 0)},
    "single": {4: ([1, 0, 0, 0], 1), 8: ([0, 0, 0, 0], 0), 16: ([0, 0, 0, 0], 0), 63: ([0, 0, 0, 0], 0)},
    "plain": {4: ([2, 0, 0, 0], 0), 8: ([0, 0, 0, 0], 0), 16: ([0, 0, 0, 0], 0), 63: ([0, 0, 0, 0], 0)},
}
