"""The inputs of tests/test_gpu_row_tiers.py (tests/row_tier_inputs.py): that every constructed beam is what its name claims -- the
conditions without which the GPU test would pass row kernels whose rare branches are wrong, because no beam took them.  No GPU.

occlusion_dict() below restates compute_occlusion_dict (simulation.py:252-295) in NumPy and also returns how many elementary slots every
flake and the hard target collected; beam_intervals() restates what get_occlusions (simulation.py:338-417) hands it.  Both are held to the
oracle bit for bit -- on constructed and random intervals, and on every beam of every frame -- before anything is read off them."""
from functools import lru_cache

import numpy as np
import pytest

import row_tier_inputs as rti
import table_filing_inputs as tfi

TWO_PI = 2 * np.pi
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    snow_oracle.build()
    return snow_oracle


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def occlusion_dict(beam_angles, intervals, current_range, beam_divergence):
    """simulation.py:252-295.  Returns ([(key, r_j, ratio)] in dict order, slots collected per flake, slots collected by the hard target,
    and whether adding the widths left to right instead gives another ratio for a flake with 8 or more slots / for the target).
    The sums are np.sum over the selected widths, as in the reference (:289, :292): NumPy's pairwise summation."""
    iv = np.array(intervals, np.float64).reshape(-1, 3)
    right, left = float(beam_angles[0]), float(beam_angles[1])
    if right > left:                                                 # :260-263
        right = right - TWO_PI
        wrapped = iv[:, 0] > iv[:, 1]
        iv[wrapped, 0] = iv[wrapped, 0] - TWO_PI
    ends = np.unique(np.concatenate(([right], iv[:, :2].ravel(), [left])))      # :265 sorted(set(...))
    width = np.diff(ends)                                            # :266
    owner = np.full(width.shape[0], -1)
    for j in range(iv.shape[0]):                                     # near -> far: the first flake to cover a slot keeps it (:284)
        i1, i2 = np.searchsorted(ends, iv[j, 0]), np.searchsorted(ends, iv[j, 1])
        mine = owner[i1:i2]
        mine[mine == -1] = j
    delta = np.radians(beam_divergence)
    slots = np.array([int((owner == j).sum()) for j in range(iv.shape[0])], np.int64)
    out = [(j, float(iv[j, 2]), float(np.clip(width[owner == j].sum() / delta, 0, 1))) for j in range(iv.shape[0]) if slots[j]]
    out.append((-1, float(current_range), float(np.clip(width[owner == -1].sum() / delta, 0, 1))))
    def in_turn(v):
        acc = 0.0
        for x in v:
            acc = acc + x
        return acc

    def ratio_of(total):
        return float(np.clip(total / delta, 0, 1))

    order_shows = (any(slots[j] >= 8 and ratio_of(in_turn(width[owner == j])) != ratio_of(width[owner == j].sum()) for j in range(iv.shape[0])),
                   ratio_of(in_turn(width[owner == -1])) != ratio_of(width[owner == -1].sum()))
    return out, slots, int((owner == -1).sum()), order_shows


def beam_angles_of(rows, bd):
    """simulation.py:89-101 in the rows' dtype: range, right and left limit angle per row (float64).  arctan2 is glibc's, as in the
    oracle and in the fixtures (conftest.numpy_is_portable): NumPy's own differs in the last bit where it dispatches to SIMD code."""
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    d = np.linalg.norm([x, y, z], axis=0).astype(np.float64)
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    fn, ct = (libm.atan2f, ctypes.c_float) if rows.dtype == np.float32 else (libm.atan2, ctypes.c_double)
    fn.restype, fn.argtypes = ct, [ct, ct]
    th = np.array([fn(float(b), float(a)) for a, b in zip(x, y)], rows.dtype)
    th = np.where(th < 0, th + rows.dtype.type(TWO_PI), th).astype(np.float64)
    half = np.radians(bd / 2)
    ang = np.column_stack((th - half, th + half))
    ang = np.where(ang < 0, ang + TWO_PI, ang)
    ang = np.where(ang > TWO_PI, ang - TWO_PI, ang)
    return d, ang


def beam_intervals(table, info, right, left, d):
    """simulation.py:345-417 for one beam: the intervals (right end, left end, range) of the flakes that meet it, near -> far.
    info = snow_oracle.flake_table(table): range, azimuth, right and left tangent angle per flake."""
    rho, phi, t_r, t_l = info[:, 0], info[:, 1], info[:, 2], info[:, 3]
    near = rho < d
    inside = (right <= phi) & (phi <= left)
    if right > left:
        inside |= ((right - TWO_PI <= phi) & (phi <= left)) | ((right <= phi) & (phi <= left + TWO_PI))

    def crosses(angle):
        dist = np.abs(table[:, 1] * np.cos(angle) - table[:, 0] * np.sin(angle))
        diff = angle - phi
        ahead = (np.abs(diff) < np.pi / 2) | (np.abs(diff - TWO_PI) < np.pi / 2) | (np.abs(diff + TWO_PI) < np.pi / 2)
        return (dist < table[:, 2]) & ahead

    hit_r, hit_l = crosses(right), crosses(left)
    k = np.flatnonzero(near & (inside | hit_r | hit_l))
    iv = np.column_stack((np.where(hit_r[k], right, t_r[k]), np.where(hit_l[k], left, t_l[k]), rho[k]))
    return iv[np.argsort(iv[:, 2], kind="stable")]


@lru_cache(maxsize=None)
def _analysis(dtype_name, frame):
    """per beam of a frame, from the restatement: flakes met, slots of the flake with most, slots of the target, entries of the dict; and
    the dicts themselves, flattened"""
    from oracle import snow_oracle as so
    so.build()
    fr = rti.frames(np.dtype(dtype_name).type)[frame]
    rows, bd = fr["rows"], fr["bd"]
    d, ang = beam_angles_of(rows, bd)
    n = rows.shape[0]
    n_hit, max_owner, tgt, size = (np.zeros(n, np.int64) for _ in range(4))
    dicts, order_shows = [None] * n, [None] * n
    for ch in np.unique(rows[:, 4]).astype(int):
        table = np.ascontiguousarray(fr["tables"][ch], np.float64)
        info = so.flake_table(table)
        for i in np.flatnonzero(rows[:, 4] == ch):
            iv = beam_intervals(table, info, ang[i, 0], ang[i, 1], d[i])
            dicts[i], slots, tgt[i], order_shows[i] = occlusion_dict(ang[i], iv, d[i], bd)
            n_hit[i], size[i], max_owner[i] = iv.shape[0], len(dicts[i]), slots.max() if slots.size else 0
    return dict(order_shows=order_shows, rows=rows, bd=bd, d=d, ang=ang, n_hit=n_hit, max_owner=max_owner, tgt=tgt, size=size, dicts=dicts, groups=fr["groups"],
                tables=fr["tables"])


def analysis(dtype, frame):
    return _analysis(np.dtype(dtype).name, frame)


# ---- the restatement against the oracle ------------------------------------------------------------------------------------------------------
def _same_dict(got, want):
    return len(got) == len(want) and all(a[0] == b[0] and a[1] == b[1] and a[2] == b[2] for a, b in zip(got, want))


def test_the_restatement_is_the_oracle_on_constructed_and_random_intervals(so):
    w = 3e-3
    cases = []
    for az in (0.5, 1e-4, TWO_PI - 2e-4, 3.0):                       # two of the wedges straddle azimuth 0
        right, left = (az - w / 2) % TWO_PI, (az + w / 2) % TWO_PI
        for c, h, rho in [rti.umbrella(m, w) for m in (1, 3, 4, 10, 30, 63)] + [rti.comb(m, w) for m in (1, 7, 8, 16, 23, 64)] + \
                [rti.both(5, 8, w), rti.hidden(5, w)]:
            o = np.argsort(rho, kind="stable")
            a1, a2 = np.maximum(az + c - h, az - w / 2)[o], np.minimum(az + c + h, az + w / 2)[o]
            cases.append(((right, left), np.column_stack((a1 % TWO_PI, a2 % TWO_PI, rho[o])), rti.BD))
    rng = np.random.default_rng(8201)
    for _ in range(400):
        bd = rti.BD if rng.random() < 0.7 else rti.BD_WIDE
        wr = np.radians(bd)
        az = rng.uniform(0, TWO_PI) if rng.random() < 0.8 else rng.uniform(-wr / 2, wr / 2)
        m = int(rng.integers(0, 40))
        c, h = rng.uniform(-0.6 * wr, 0.6 * wr, m), np.exp(rng.uniform(np.log(1e-5), np.log(0.4 * wr), m))
        a1, a2 = np.maximum(az + c - h, az - wr / 2), np.minimum(az + c + h, az + wr / 2)
        ok = a1 < a2
        if m and rng.random() < 0.3:                                 # a flake twice
            a1[-1], a2[-1] = a1[0], a2[0]
            ok[-1] = ok[0]
        iv = np.column_stack((a1 % TWO_PI, a2 % TWO_PI, np.sort(rng.uniform(1.0, 50.0, m))))[ok]
        cases.append((((az - wr / 2) % TWO_PI, (az + wr / 2) % TWO_PI), iv, bd))
    wrapped = many = 0
    for ang, iv, bd in cases:
        got, slots, tgt, _ = occlusion_dict(ang, iv, 60.0, bd)
        want = so.compute_occlusion_dict(ang, iv.copy(), 60.0, bd)
        assert _same_dict(got, want), (ang, iv.shape)
        wrapped += ang[0] > ang[1]
        many += (slots.max() if slots.size else 0) >= 8 or tgt >= 8
    assert wrapped > 40 and many > 40


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", ["main", "wide", "single", "plain"])
def test_the_restatement_gives_the_oracle_dicts_of_every_beam(so, frame, dtype):
    """process_single_channel(dump=True) on the rows themselves: flakes per dict, ranges and ratios bit for bit; get_occlusions on the
    restated angles: the intersecting counts"""
    a = analysis(dtype, frame)
    rows, las = a["rows"], so.load_lasers()
    for ch in np.unique(rows[:, 4]).astype(int):
        idx = np.flatnonzero(rows[:, 4] == ch)
        _, _, (cnt, keys, rj, ratio) = so.process_single_channel(rows[idx], a["tables"][ch], a["bd"], las, ch, dump=True)
        _, _, _, _, nint = so.get_occlusions(a["ang"][idx], a["d"][idx], a["tables"][ch], a["bd"])
        assert np.array_equal(nint, a["n_hit"][idx]), ch
        start = np.concatenate(([0], np.cumsum(cnt)))
        for k, i in enumerate(idx):
            want = list(zip(keys[start[k]:start[k + 1]], rj[start[k]:start[k + 1]], ratio[start[k]:start[k + 1]]))
            assert _same_dict(a["dicts"][i], want), (ch, k)


# ---- the conditions ------------------------------------------------------------------------------------------------------------------------
def _beam(a, case, name):
    i = a["groups"][case][name]
    return int(a["n_hit"][i]), int(a["max_owner"][i]), int(a["tgt"][i]), int(a["size"][i]), i


@pytest.mark.parametrize("dtype", DTYPES)
def test_umbrella_beams(dtype):
    a = analysis(dtype, "main")
    for m in rti.UMBRELLA_M:
        L, own, tgt, size, i = _beam(a, "umbrella", f"umbrella{m}")
        assert (L, own, tgt, size) == (m + 1, 2 * m + 1, 0, 2), m           # one flake owns everything; the dict: that flake and the target
        assert a["dicts"][i][-1][2] == 0.0 and abs(a["dicts"][i][0][2] - 1.0) < 1e-12     # the target's ratio is exactly 0
    assert [2 * m + 1 for m in rti.UMBRELLA_M] == [7, 9, 21, 61]           # not redone; redone in the 8-, the 16- and the 63-entry tier
    assert [m + 1 for m in rti.UMBRELLA_M] == [4, 5, 11, 31]
    assert _beam(a, "umbrella", "umbrella3_twin")[:4] == (5, 7, 0, 2)      # 8-entry class, 7 slots: finished by the first instantiation ...
    g = a["groups"]["umbrella"]
    assert g["umbrella4"] == g["umbrella3_twin"] + 1 == g["umbrella3"] + 2  # ... in the row beside umbrella(4), which is deferred


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_beams(dtype):
    a = analysis(dtype, "main")
    assert rti.EDGE_L == (8, 9, 16, 17, 63, 64)
    for L in rti.EDGE_L:
        assert _beam(a, "edges", f"umbrella_L{L}")[:4] == (L, 2 * L - 1, 0, 2)
        assert _beam(a, "edges", f"comb_L{L}")[:4] == (L, 1, L + 1, L + 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", ["main", "wide"])
def test_comb_and_both_beams(frame, dtype):
    a = analysis(dtype, frame)
    assert a["bd"] == (rti.BD if frame == "main" else rti.BD_WIDE)
    assert rti.COMB_TARGET == (7, 8, 9, 15, 16, 17, 24)
    for t in rti.COMB_TARGET:
        assert _beam(a, "comb", f"comb_t{t}")[:4] == (t - 1, 1, t, t)       # every flake one slot, the target t
    for k, m in rti.BOTH_KM:
        L, own, tgt, size, _ = _beam(a, "both", f"both{k}_{m}")
        assert k >= 4 and (L, own, tgt, size) == (1 + k + m, 2 * k + 1, m + 1, 1 + m + 1)
        assert own >= 8 and tgt >= 8 and 8 < L <= 63


@pytest.mark.parametrize("dtype", DTYPES)
def test_eclipsed_beams(so, dtype):
    a = analysis(dtype, "main")
    table = a["tables"][rti.CASE_CHANNEL["eclipsed"]]
    assert sum(table[i].tobytes() == table[i + 1].tobytes() for i in range(table.shape[0] - 1)) == 2      # two rows appear twice, byte for byte
    for name, L, S, most in (("twice", 7, 6, 1), ("hidden", 6, 5, 3), ("twice_hidden", 9, 7, 3)):     # (the flake in front of the hidden one: 3 slots)
        n_hit, own, tgt, size, i = _beam(a, "eclipsed", name)
        assert (n_hit, own, size) == (L, most, S + 1) and S < L, name
        keys = [k for k, _, _ in a["dicts"][i][:-1]]
        missing = sorted(set(range(L)) - set(keys))
        assert all(0 < j < L - 1 for j in missing), (name, missing)          # the lanes that own nothing lie inside the row
        if name != "hidden":                                                 # the copy later in scan order is the one that vanishes
            iv = beam_intervals(np.ascontiguousarray(table), so.flake_table(table), a["ang"][i, 0], a["ang"][i, 1], a["d"][i])
            twin = [j for j in range(1, L) if np.array_equal(iv[j], iv[j - 1])]
            assert len(twin) == 1 and twin[0] in missing and twin[0] - 1 in keys


@pytest.mark.parametrize("dtype", DTYPES)
def test_seam_beams(so, dtype):
    a = analysis(dtype, "main")
    assert rti.SEAM_CHANNELS[0] == rti.CASE_CHANNEL["seam"] and [b[0] for b in rti.SEAM_BEAMS] == list(a["groups"]["seam"])
    # flakes met, slots of the nearest flake, slots of the target, dict entries; flakes wholly right of azimuth 0
    want = {"seam_umbrella4": ((5, 9, 0, 2), 0), "seam_comb_t8": ((7, 1, 8, 8), 0), "seam_right8": ((7, 11, 1, 3), 1),
            "seam_right16": ((11, 17, 2, 4), 2), "seam_right63": ((31, 53, 4, 6), 4), "seam_comb_t24": ((23, 1, 24, 24), 3)}
    for k, (name, kind, m, j) in enumerate(rti.SEAM_BEAMS):
        table = np.ascontiguousarray(a["tables"][rti.SEAM_CHANNELS[k]])
        info = so.flake_table(table)
        got = _beam(a, "seam", name)
        assert got[:4] == want[name][0], name
        i = got[4]
        assert a["ang"][i, 0] > a["ang"][i, 1]                               # theta_r > theta_l
        iv = beam_intervals(table, info, a["ang"][i, 0], a["ang"][i, 1], a["d"][i])
        wraps = iv[:, 0] > iv[:, 1]
        assert wraps.sum() == (1 if kind == "comb" else 2)                   # one inner flake, and the umbrella itself
        # flakes wholly right of azimuth 0 stay near 2 pi (:262-263); with one of them the target's ratio is clipped to 1
        right_of_0 = int(((iv[:, 0] < iv[:, 1]) & (iv[:, 0] > 6.0)).sum())
        assert right_of_0 == want[name][1] and (right_of_0 == 0 or a["dicts"][i][-1][2] == 1.0), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_bins_beam(dtype):
    a = analysis(dtype, "main")
    assert _beam(a, "bins", "bins")[:4] == (5, 9, 0, 2)                      # counted once, whatever the number of bins
    table = a["tables"][rti.CASE_CHANNEL["bins"]]
    f = tfi.interval_bins(table)
    assert f["span"][0] >= 4 and (f["span"][1:] <= 2).all()                  # the nearest flake is filed under four or more bins
    assert tfi.guard_rows(table).size == 0
    i = a["groups"]["bins"]["bins"]
    lo, hi = np.floor(a["ang"][i] / tfi.BIN_W)
    assert hi == lo + 1                                                      # the wedge itself holds a bin edge


@pytest.mark.parametrize("dtype", DTYPES)
def test_class_populations_and_redo_counts(dtype):
    """what the GPU test compares status words [2 .. 6] with (rti.EXPECTED), and the partial classes"""
    for frame in ("main", "wide", "single", "plain"):
        a = analysis(dtype, frame)
        for first in rti.CAPS:
            got = (rti.class_populations(a["n_hit"], first), rti.redo_count(a["n_hit"], a["max_owner"], first))
            assert got == rti.EXPECTED[frame][first], (frame, first, got)
    p8, p16, p63, pg = rti.EXPECTED["main"][4][0]
    assert p8 % 8 != 0 and p16 % 4 != 0 and p63 > 1 and pg >= 2              # no class fills its last wave; the 64-flake beams go beyond
    assert rti.EXPECTED["main"][4][1] >= 10
    assert rti.EXPECTED["single"][4] == ([1, 0, 0, 0], 1)                    # one beam in the 8-entry class, redone
    assert rti.EXPECTED["plain"][4][1] == 0 and sum(rti.EXPECTED["plain"][4][0]) > 0
    assert rti.EXPECTED["wide"][4][1] >= 2
    for frame in ("main", "wide", "single", "plain"):
        assert 100 <= rti.frames(dtype)[frame]["rows"].shape[0] <= 400


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_order_of_the_sums_shows_in_the_ratios(dtype):
    """A kernel that adds a redone flake's slots, or the target's, in another order than NumPy must fail the GPU test.  That can show next
    to azimuth 0 only (tests/row_tier_inputs.py says why): for the near0 beams the left-to-right sum of the umbrella's widths gives another
    ratio than np.sum, one beam per row tier, and so does the target's for the two combs."""
    a = analysis(dtype, "main")
    g = a["groups"]["near0"]
    want = {"near0_shaded8": (7, 10, 0, 5), "near0_shaded16": (12, 17, 0, 8), "near0_shaded63": (21, 31, 0, 12),
            "near0_comb_t17": (16, 1, 17, 17), "near0_comb_t24": (23, 1, 24, 24)}
    assert list(g) == list(want) == [b[0] for b in rti.NEAR0_BEAMS]
    for name, i in g.items():
        assert _beam(a, "near0", name)[:4] == want[name], name
        assert a["ang"][i, 0] < a["ang"][i, 1] < 3.5e-3                      # left of azimuth 0, not across it
        assert a["order_shows"][i] == ((True, False) if "shaded" in name else (False, True)), name
    # ... and nowhere else: away from azimuth 0 every partial sum is exact
    others = [i for case, grp in a["groups"].items() if case not in ("seam", "near0") for i in grp.values()]
    assert len(others) > 30 and not any(a["order_shows"][i][0] or a["order_shows"][i][1] for i in others)
