"""The same-draw restatements of tests/seeded_reference.py, checked without a GPU: their Philox is Philox4x32-10, and every
setting the GPU tests run (test_gpu_sampler_exact.py, test_gpu_plane.py) decides what it is there to decide -- with margins so
far above rounding that the device's cos / sin / log1p and summation order cannot flip a decision.  A setting changed into a
blind one fails here, on any machine."""
import numpy as np
import pytest

import seeded_reference as sr

MARGIN = 1e-9              # rounding differences are ~1e-15


def test_philox_known_answer_vectors():
    """The three Philox4x32-10 vectors of the Random123 distribution (kat_vectors), through (seed, idx, group, tag) as
    sg_philox.h lays them out: c = {idx lo, idx hi, group, tag}, k = {seed lo, seed hi}."""
    ones = 0xFFFFFFFF
    assert sr.philox4x32_10(0, 0, 0, 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert sr.philox4x32_10(ones << 32 | ones, ones << 32 | ones, ones, ones) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert sr.philox4x32_10(0x299F31D0 << 32 | 0xA4093822, 0x85A308D3 << 32 | 0x243F6A88, 0x13198A2E, 0x03707344) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_scalar_and_vectorised_philox_agree():
    rng = np.random.default_rng(0)
    for seed in (0, 7, 2 ** 40 + 3, 2 ** 64 - 1):
        idx = np.concatenate(([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63], rng.integers(0, 2 ** 62, 40))).astype(np.uint64)
        grp = np.concatenate(([0, 1, 63, 2 ** 32 - 1, 5], rng.integers(0, 2 ** 32, 40))).astype(np.uint64)
        for tag in (sr.TAG_SNOW, sr.TAG_PLAN):
            got = np.stack(sr.philox4x32_10_vec(seed, idx, grp, tag), axis=1)
            want = np.array([sr.philox4x32_10(seed, int(i), int(g), tag) for i, g in zip(idx, grp)], np.uint64)
            assert np.array_equal(got, want)
        # one idx against many groups (the plane RANSAC's use) and the uniforms of philox_u2
        got = np.stack(sr.philox4x32_10_vec(seed, 3, np.arange(50), sr.TAG_PLAN), axis=1)
        assert np.array_equal(got, np.array([sr.philox4x32_10(seed, 3, g, sr.TAG_PLAN) for g in range(50)], np.uint64))
        u0, u1 = sr.u2(seed, idx, 1)
        w = [sr.philox4x32_10(seed, int(i), 1, sr.TAG_SNOW) for i in idx]
        assert np.array_equal(u0, [((a << 32 | b) >> 11) / 2.0 ** 53 for a, b, _, _ in w])
        assert np.array_equal(u1, [((c << 32 | d) >> 11) / 2.0 ** 53 for _, _, c, d in w])
        assert (u0 >= 0).all() and (u0 < 1).all()


def test_the_high_precision_reference_is_wider_than_float64():
    assert np.finfo(np.longdouble).nmant > 60
    a = sr.sampler_candidates(7, 0, 4096, 80.0, 0.5, precise=True)
    b = sr.sampler_candidates(7, 0, 4096, 80.0, 0.5, precise=False)
    assert np.abs(a.x - b.x).max() <= 2.0 ** -51 * 80.0 and np.array_equal(a.valid, b.valid)     # the same darts, a few ULP apart at most


@pytest.mark.parametrize("name", sr.SAMPLER_SETTING_NAMES)
def test_sampler_settings_decide_something(name):
    """Section 'conditions' of the sampler: the float64 restatement takes every decision with a relative margin above 1e-9
    (so the high-precision one and the device take the same), and each setting exercises what it is listed for."""
    s = sr.sampler_settings()[name]
    r = sr.dart_throw_restated(s["seed"], s["occupancy"], s["scale_mm"], s["R0"], precise=False)
    assert r.margin > MARGIN, r.margins
    hp = sr.dart_throw_restated(s["seed"], s["occupancy"], s["scale_mm"], s["R0"], precise=True)
    assert np.array_equal(hp.index, r.index) and hp.cut == r.cut
    # floors: 20 rejects for the small settings -- except d7, whose 86 darts to the cut leave no room for them (floor 1)
    for key in ("rejects", "chain_accepts", "invalid", "invalid_thrown", "redrew"):
        if key in s["floors"]:
            assert getattr(r, key) >= s["floors"][key], (key, getattr(r, key))
    kind = s["kind"]
    if kind == "overflow":                         # a dart the process needs cannot be decided: the entry must refuse
        assert r.max_conf > sr.SG_SAMP_MAXCONF and 0 <= r.first_overflow <= r.cut and r.first_overflow < r.n_cand_entry
        # which half of the host's condition refuses: a cut that was reached, at or beyond the overflow -- or no cut at all
        assert (r.cut < r.n_cand_entry) == s["floors"]["cut_in_first_attempt"], (r.cut, r.n_cand_entry)
        return
    assert r.max_conf <= sr.SG_SAMP_MAXCONF
    assert r.first_overflow < 0 or r.first_overflow > r.cut
    if kind == "dense":                            # a spare candidate the process never reaches overflows its conflict list
        assert r.cut < r.first_overflow < r.n_cand_entry
    if kind in ("small", "full", "filed", "wide"):
        assert r.first_overflow < 0 and r.n_cand == r.n_cand_entry
    if kind == "double":                           # the first attempt of the entry falls short: its doubling loop runs
        assert r.cut >= r.n_cand_entry and r.n_cand > r.n_cand_entry
    if kind == "full":
        assert len(r.rows) > 15000 and r.rejects == 0     # full-size tables at 4.3e-6 occupancy: what the older tests run


def test_sampler_settings_cover_the_list():
    """The figures the settings were chosen for (seed 4: conflict lists filled to 4, chains of depth 3)."""
    s = sr.sampler_settings()["s4"]
    r = sr.dart_throw_restated(s["seed"], s["occupancy"], s["scale_mm"], s["R0"], precise=False)
    assert (r.rejects, r.chain_accepts, r.max_conf, r.depth) == (819, 63, 4, 3)
    s = sr.sampler_settings()["gunn7"]
    r = sr.dart_throw_restated(s["seed"], s["occupancy"], s["scale_mm"], s["R0"], precise=False)
    assert (len(r.rows), r.cut) == (17887, 17886)


@pytest.mark.parametrize("name", sr.PLANE_CASE_NAMES)
def test_plane_cases_identify_the_winner(name):
    """Conditions of the plane RANSAC cases: every res*res is clear of thr, and in the scenes the winner is decided by the
    count (or, in ties, by a mean squared residual that differs by more than rounding) and refits to another plane than the
    runner-up -- so the device's answer says which trial it picked."""
    c = sr.plane_case(name)
    ties, keyed = 0, {}
    for f, pc in enumerate(c["frames"]):
        r = sr.plane_ransac_restated(pc, c["seed"], f, c["trials"], c["min_rows"])
        assert r.model == 2 and r.crop >= 3 and r.m_thr > MARGIN and r.m_det > MARGIN
        if c["kind"] == "edge":
            continue
        a, b = r.ranking[:2]
        assert len(set(r.counts[r.counts >= 0].tolist())) > 0.4 * min(c["trials"], 256)      # the count separates the trials
        (pa, ua), (pb, ub) = r.refit(a), r.refit(b)
        assert abs(pa[3] - pb[3]) > 1e-6 or ua != ub
        if r.counts[a] == r.counts[b]:
            ties += 1
            assert abs(r.mean_ss[a] - r.mean_ss[b]) > 1e-9 * r.mean_ss[b]
        if c["kind"] == "batch" and f > 0:                                                   # the draws are keyed by the frame
            r0 = sr.plane_ransac_restated(pc, c["seed"], 0, c["trials"], c["min_rows"])
            keyed[f] = r0.winner != r.winner and not np.array_equal(r0.plane, r.plane)
    if c["kind"] == "batch":                       # frame 2 is the one the GPU test holds against the draws of frame 0
        assert keyed[2] and sum(keyed.values()) >= 3, keyed
    if c["kind"] == "tie":
        assert ties == 1
    if c["kind"] == "collinear":
        assert r.valid_trials < 0.95 * c["trials"]
    else:
        assert r.valid_trials == c["trials"] or c["kind"] == "edge"


def test_plane_cases_cover_the_list():
    CASES = {name: sr.plane_case(name) for name in sr.PLANE_CASE_NAMES}
    crops = {sr.plane_ransac_restated(c["frames"][0], c["seed"], 0, 3, c["min_rows"]).crop for c in CASES.values()}
    assert {3, 4, 10, sr.PL_CHUNK - 1, sr.PL_CHUNK, sr.PL_CHUNK + 1, 3 * sr.PL_CHUNK + 100} <= crops
    assert {c["trials"] for c in CASES.values()} >= {64, 100, 256, 1024, 1500}
    assert any(c["seed"] >= 2 ** 32 for c in CASES.values()) and any(len(c["frames"]) >= 4 for c in CASES.values())
    assert {c["frames"][0].dtype for c in CASES.values()} == {np.dtype(np.float32), np.dtype(np.float64)}
