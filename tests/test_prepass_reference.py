"""CPU: the restatement of tests/prepass_reference.py and its settings table, on any machine.

For every setting the GPU tests run (tests/test_gpu_prepass_edges.py, tests/test_gpu_wet_edges.py):
  - the restatement IS the reference: its float64 answers equal oracle.snow_oracle's noise_threshold_poly (float64 rows) and
    ground_water_augmentation (both dtypes, every parameter set) bit for bit;
  - the setting decides what it is listed for (rows per branch, tied rows, usable range rows, rows on the edges, ...);
  - every discrete decision is clear of rounding: keep / drop by a relative 1e-7, the ground band by 1e-9, I / cos clear of every
    y edge but the last by a relative 1e-12;
  - the bounds are sound: NumPy / SciPy's own float64 answer lies inside every bound measured from the long-double value (the
    fraction it uses is printed with -s and recorded in the GPU files' docstrings);
  - the power line does not cancel on the fitted-line wet settings.
"""
import numpy as np
import pytest

import prepass_reference as pr

TAGS = ("f32", "f64")
PRE_FRAMES = tuple(f"tiles{n}" for n in pr.TILE_ROWS) + ("edges", "ties", "m3", "m4", "plain", "sorted", "m3sorted") + pr.FALLBACK_FRAMES


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    return snow_oracle


def _band_clear(pc, delta=0.5):
    hog = np.matmul(pc[:, :3], pr.PLANE_W) + pr.PLANE_H
    return float(np.min(np.abs(np.abs(hog) - delta)))


def _y_edge_clearance(g, h):
    """Smallest relative distance of an I / cos in [5, max) from a y edge."""
    y = g.norm[(g.norm >= 5) & (g.norm < np.max(g.norm))]
    k = np.searchsorted(h.yedges, y, side="right")
    near = np.minimum(np.abs(y - h.yedges[k - 1]), np.abs(h.yedges[np.minimum(k, pr.HY)] - y))
    return float(np.min(near / y)) if y.size else 1.0


def _fractions(e, ld):
    rec = np.abs(e.rec.astype(pr.L) - ld.rec)
    assert (rec[ld.b_rec == 0] == 0).all()                               # the count (and the float32 mean) are exact
    f_rec = float(np.max(rec[ld.b_rec > 0] / ld.b_rec[ld.b_rec > 0]))
    f_min = max(float(abs(pr.L(e.pmin[0]) - ld.pmin[0]) / ld.b_pmin[0]), float(abs(pr.L(e.pmin[1]) - ld.pmin[1]) / ld.b_pmin[1]))
    f_poly = float(np.max(np.abs(pr.poly_at(e.poly, ld) - ld.poly_at) / ld.b_poly_at))
    return f_rec, f_min, f_poly


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", PRE_FRAMES + tuple(f"mean{k}" for k in pr.MEAN32_COUNTS))
def test_prepass_settings_are_clear_of_rounding_and_inside_their_bounds(so, name, tag):
    pc = pr.frame(name, tag)
    assert pc.dtype == pr._dt(tag) and (np.linalg.norm(pc[:, :3].astype(np.float64), axis=1) < 119).all()
    assert set(np.unique(pc[:, 4])) <= set(range(64))
    assert _band_clear(pc) > 1e-9
    for frame_of in (pr.snow_frame, pr.stats_frame):                     # channel-sorted (augment_batch) and as it comes (prepass_stats)
        g, e, ld = frame_of(pc)
        assert np.max(g.norm) > 5                                        # (a frame below that is out of scope: the reference raises)
        assert _y_edge_clearance(g, e.hist) > 1e-12
        if ((g.dist > 10.5) & (g.dist < 69.5)).any():
            assert e.hist.raw[:, pr.HY - 1].sum() >= 1                   # the maximum lands in the last bin
        f_rec, f_min, f_poly = _fractions(e, ld)
        print(f"\n[prepass-reference] {name} {tag}: ground {len(g.dist)}, usable range rows {e.m}, cond {ld.cond:.0f}; NumPy's error / bound: "
              f"record {f_rec:.2e}, noise line {f_min:.2e}, polynomial {f_poly:.2e} (bound <= {float(ld.b_poly_at.max()):.2e})")
        assert f_rec <= 1 and f_min <= 1 and f_poly <= 1
    if tag == "f64":                                                     # the restatement is the oracle's own fit, bit for bit
        srt = pc[np.argsort(pc[:, 4], kind="stable")]
        assert np.array_equal(pr.snow_frame(pc)[1].poly, so.noise_threshold_poly(srt, pr.PLANE_W, pr.PLANE_H, 0.7))
    else:                                                                # within 1e-4 of the oracle's float32 np.polyfit
        g, e, ld = pr.snow_frame(pc)
        host = so.noise_threshold_poly(pc[np.argsort(pc[:, 4], kind="stable")], pr.PLANE_W, pr.PLANE_H, 0.7)
        assert float(np.max(np.abs(pr.poly_at(host, ld) - ld.poly_at))) < 5e-5


@pytest.mark.parametrize("tag", TAGS)
def test_tile_settings_cross_the_tile_and_the_64_tile_trip(tag):
    """Setting 1: 1023 / 1024 / 1025 / 2049 rows and 65 tiles + 1, ground rows in every tile but one."""
    for n in pr.TILE_ROWS:
        pc = pr.frame(f"tiles{n}", tag)
        assert pc.shape[0] == n
        mask = pr.ground_rows(pc).mask
        per_tile = np.add.reduceat(mask.astype(int), np.arange(0, n, pr.TILE))
        if n > 64 * pr.TILE:
            assert len(per_tile) == 66 and per_tile[3] == 0 and (np.delete(per_tile, 3) > 0).all()
            assert per_tile[64:].sum() > 0                               # the second trip carries ground rows
        else:
            assert (per_tile > 0).all()


def test_mean32_settings_have_the_listed_ground_counts_in_several_tiles_and_waves():
    """Setting 2: NumPy's float32 pairwise sum by ground count -- below 8 (sequential), leaves of up to 128 with the 8-wide unroll and its
    tail, splits at n / 2 rounded down to a multiple of 8 (136, 255, 1000 and 4099 split where n / 2 is none)."""
    for k in pr.MEAN32_COUNTS:
        pc = pr.frame(f"mean{k}", "f32")
        mask = pr.ground_rows(pc).mask
        assert mask.sum() == k
        per_tile = np.add.reduceat(mask.astype(int), np.arange(0, len(mask), pr.TILE))
        assert (per_tile > 0).sum() >= 2
        waves = np.add.reduceat(mask.astype(int), np.arange(0, len(mask), 64))
        assert (waves > 0).sum() >= min(k, 3)                            # a gather that forgets the wave offset moves rows
    assert any(k > 128 and (k // 2) % 8 for k in pr.MEAN32_COUNTS) and any(k < 8 for k in pr.MEAN32_COUNTS)
    assert any(k % 8 and k > 8 for k in pr.MEAN32_COUNTS) and {127, 128, 129} <= set(pr.MEAN32_COUNTS)


@pytest.mark.parametrize("tag", TAGS)
def test_edge_setting_puts_rows_on_and_beside_every_x_edge(tag):
    """Setting 3."""
    pc = pr.frame("edges", tag)
    g = pr.ground_rows(pc)
    d = g.dist
    assert d.dtype == pr._dt(tag)
    assert np.isin(pr.edge_targets(tag == "f32" and np.float32 or np.float64), d).all()
    xe = pr.x_edges()
    on_edge = np.isin(d.astype(np.float64), xe).sum()
    assert on_edge >= (51 if tag == "f64" else 11)                       # float32 holds the edges 10, 16, 22, ..., 70 only
    one = d.dtype.type
    assert np.nextafter(one(10), one(0)) in d and np.nextafter(one(70), one(100)) in d and one(10) in d and one(70) in d
    assert (g.norm < 5).sum() > 100
    if tag == "f64":                                                     # floor((v - lo) / step) alone is wrong on some of them: the settle loops decide
        dd = d[(d >= 10) & (d <= 70)]
        true = np.searchsorted(xe, dd, side="right") - 1
        true[dd == 70] = pr.HX - 1
        naive = np.minimum(np.floor((dd - 10.0) / ((70.0 - 10.0) / pr.HX)).astype(int), pr.HX - 1)
        assert (naive != true).sum() >= 3


@pytest.mark.parametrize("tag", TAGS)
def test_tie_setting_has_tied_minima_and_single_bin_rows(tag):
    """Setting 4: the first minimum decides wherever the smallest count occurs in several bins; rows 7 and 49 hold all their rows in one bin."""
    g, e, _ = pr.snow_frame(pr.frame("ties", tag))
    h = e.hist
    assert (h.tied > 1).sum() >= 40
    last = np.array([pr.HY - 1 - np.argmin(h.hist[r, ::-1]) for r in range(pr.HX)])
    assert (last != h.ymins).sum() >= 40                                 # keeping the LAST minimum would move these rows' values
    for row, count in ((7, 5), (30, 1), (49, 3)):
        assert (h.raw[row] > 0).sum() == 1 and h.raw[row].max() == count and h.raw[row].sum() == count
        assert row in h.usable


@pytest.mark.parametrize("tag", TAGS)
def test_m_settings_have_exactly_three_and_four_usable_range_rows(tag):
    """Setting 5: augmentation.py:248 `len(min_vals) > 3`."""
    for name, m in (("m3", 3), ("m3sorted", 3), ("m4", 4)):
        for frame_of in (pr.snow_frame, pr.stats_frame):
            g, e, _ = frame_of(pr.frame(name, tag))
            assert e.m == m and e.fallback == (m == 3)
            if m == 3:
                assert e.pmin == e.p
            else:
                assert abs(e.pmin[0] - e.p[0]) > 1e-3 * abs(e.p[0])      # the two lines differ: `m >= 3` or `m > 4` would show
        w = pr.wet_restated(pr.frame(name, tag), **pr.WET_PARAMS[0])
        assert w.flag == 0 and w.e64.m == m


def test_fallback_frames_have_a_float32_mean_that_depends_on_the_row_order():
    """Setting 5 through augment_batch: shuffled float32 frames whose noise line falls back, with ground counts across NumPy's leaf and
    split sizes.  The float32 mean of the ground ranges in channel-sorted order (the reference's, simulation.py:447) differs from the
    mean in the order the rows come in, and the regression intercept moves with it by far more than its bound: a gather of the ground
    ranges in any other order than the sorted one shows in the device's polynomial."""
    for k in pr.FALLBACK_COUNTS:
        pc = pr.frame(f"fb{k}", "f32")
        assert not (np.diff(pc[:, 4]) >= 0).all()                        # shuffled: the device sorts it
        (gs, es, lds), (ga, ea, _) = pr.snow_frame(pc), pr.stats_frame(pc)
        assert len(gs.dist) == len(ga.dist) == k and es.fallback and ea.fallback and 1 <= es.m <= 3
        ms, ma = np.mean(gs.dist), np.mean(ga.dist)
        assert ms.dtype == np.float32 and ms != ma
        shift = abs(float(es.p[0]) * (float(ms) - float(ma)))            # what the other order's mean does to the intercept ...
        assert shift > 100 * float(lds.b_p[1])
        p1_other = es.p[1] + es.p[0] * (np.float64(ms) - np.float64(ma))  # ... and to the polynomial fitted through that line
        other = pr._scaled_lstsq(pr._columns(gs.dist), 0.7 * (es.p[0] * gs.dist + p1_other) * gs.cos)
        frac = float(np.max(np.abs(pr.poly_at(other, lds) - lds.poly_at) / lds.b_poly_at))
        print(f"\n[prepass-reference] fb{k}: float32 mean sorted {float(ms)!r}, as the rows come {float(ma)!r}; the other order's polynomial is at {frac:.3g} of the bound")
        assert frac > 10
        assert pr.snow_frame(pr.frame(f"fb{k}", "f64"))[1].fallback
    assert any(k > 128 and (k // 2) % 8 for k in pr.FALLBACK_COUNTS) and any(k > 256 for k in pr.FALLBACK_COUNTS)


def test_batches_of_both_paths_hold_the_same_ragged_frames():
    """Settings 6 and 7: the batch at the switch of sg_prepass_run and the one above it; fallback and fitted noise lines, channel-major
    and shuffled frames side by side."""
    lim = pr.small_batch_limit()
    assert 4 <= lim <= 64
    a, b = pr.batch_names(lim), pr.batch_names(lim + 1)
    assert set(a) == set(b) == set(pr.BATCH_FRAMES) and len({pr.frame(n, "f32").shape[0] for n in a}) >= 4
    for tag in TAGS:
        fb = [pr.snow_frame(pr.frame(n, tag))[1].fallback for n in pr.BATCH_FRAMES]
        assert any(fb) and not all(fb)
        srt = [bool((np.diff(pr.frame(n, tag)[:, 4]) >= 0).all()) for n in pr.BATCH_FRAMES]
        assert any(srt) and not all(srt)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("i", range(len(pr.WET_PARAMS)))
def test_wet_settings_equal_the_oracle_and_are_clear_of_rounding(so, i, tag):
    """Setting 8."""
    kw = pr.WET_PARAMS[i]
    for name in ("wet",) + (("m3", "m4", "wet_tiles") if i == 0 else ()):
        pc = pr.frame(name, tag)
        assert _band_clear(pc, kw["delta"]) > 1e-9
        r = pr.wet_restated(pc, **kw)
        ref, src = so.ground_water_augmentation(pc, plane=(pr.PLANE_W, pr.PLANE_H), return_src=True, **kw)
        assert np.array_equal(ref, r.out) and np.array_equal(src, r.src) and r.flag == 0
        ch, ld = r.chain, r.chain_ld
        assert ch.keep.sum() > 100 and (~ch.keep).sum() > 100
        assert np.array_equal(ch.keep, ld.keep)
        margin = np.abs(ld.new_i - ld.lim) / np.abs(ld.lim)
        assert float(margin.min()) > 1e-7
        assert (np.abs(ch.cancel[0] + ch.cancel[1]) >= 1e-3 * (np.abs(ch.cancel[0]) + abs(ch.cancel[1]))).all()
        k = ch.keep & (ch.new_i > 0)
        worst = float(np.max(np.abs(ch.new_i[k] - ld.new_i[k]) / ld.new_i[k]))
        print(f"\n[prepass-reference] wet {i} {name} {tag}: kept {int(ch.keep.sum())} of {len(ch.keep)}, rho > 1: {int((ch.refl > 1).sum())}, "
              f"smallest keep / drop margin {float(margin.min()):.1e}; float64 chain within {worst:.1e} of the long-double one")
        assert worst < 1e-12                                             # the chain is well conditioned: 1e-9 leaves room for the fit
        _, f_min, _ = _fractions(r.e64, pr.estimate_ld(r.g, r.e64, kw["noise_floor"]))
        assert f_min <= 1
    ratio = kw["water_height"] / kw["pavement_depth"]
    if kw["power_factor"] == 1.0:
        assert (pr.wet_restated(pr.frame("wet", tag), **kw).chain.refl > 1).sum() > 500
    assert ratio in (0, 0.4, 0.8, 1, 2)


def test_wet_parameter_sets_cover_the_listed_values():
    ps = pr.WET_PARAMS
    assert {round(p["water_height"] / p["pavement_depth"], 6) for p in ps} == {0, 0.4, 0.8, 1, 2}
    for key, vals in (("flat_earth", {True, False}), ("replace", {True, False}), ("delta", {0.2, 0.5})):
        assert {p[key] for p in ps} == vals
    assert len({(p["noise_floor"], p["power_factor"]) for p in ps}) == 2


@pytest.mark.parametrize("tag", TAGS)
def test_the_1000_row_rule_setting(so, tag):
    """Setting 9: 999 ground rows come back unchanged, 1000 are processed."""
    a, b = pr.frame("g999", tag), pr.frame("g1000", tag)
    assert pr.ground_rows(a).mask.sum() == 999 and pr.ground_rows(b).mask.sum() == 1000
    ra, rb = pr.wet_restated(a, **pr.WET_PARAMS[2] | dict(delta=0.5)), pr.wet_restated(b, **pr.WET_PARAMS[2] | dict(delta=0.5))
    assert ra.flag == 1 and np.array_equal(ra.out, a.astype(np.float64)) and rb.flag == 0 and rb.out.shape[0] < b.shape[0]
    assert so.ground_water_augmentation(a, plane=(pr.PLANE_W, pr.PLANE_H)) is a


@pytest.mark.parametrize("tag", TAGS)
def test_the_callers_lines_reach_every_branch(tag):
    """Setting 10."""
    pc = pr.frame("lines", tag)
    r = pr.wet_restated(pc, lines=pr.LINES, **pr.LINES_PARAMS)
    ch, ld, inten = r.chain, r.chain_ld, r.g.rows[:, 3]
    assert (ch.refl < 0.05).sum() > 100 and ((ch.refl >= 0.05) & (ch.refl <= 1)).sum() > 100 and (ch.refl > 1).sum() > 100
    assert (ch.raw < 0).sum() >= 10 and (ch.raw > inten).sum() >= 50
    assert ch.keep.sum() > 500 and (~ch.keep).sum() > 500
    assert ((ch.lim < 0) & ch.keep & (ch.new_i == 0)).sum() >= 10        # negative threshold: kept with intensity 0
    assert np.array_equal(ch.keep, ld.keep)
    assert float(np.min(np.abs(ld.new_i - ld.lim) / np.abs(ld.lim))) > 1e-7
    assert float(np.min(np.abs(np.abs(ld.refl) - 1))) > 1e-9 and float(np.min(np.abs(ld.refl - 0.05))) > 1e-9
    k = ch.keep & (ch.new_i > 0)
    assert float(np.max(np.abs(ch.new_i[k] - ld.new_i[k]) / ld.new_i[k])) < 1e-12
