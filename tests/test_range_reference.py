"""The range image without a GPU: the conditions under which the comparisons of tests/test_gpu_range_image.py are not vacuous, asserted
on the shared inputs of tests/range_reference.py; the pixel functions of csrc/sg_range.h compiled for the host and walked over those
inputs in the kernels' sequence (tests/host_harness/range_pixels.cpp, once more under the address and undefined-behaviour sanitizers as
a stand-alone program) against the restatement; and what snowgpu_range_image_device refuses, in which words
(tests/host_harness/range_refusals.cpp)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import range_reference as rr
from conftest import ROOT, numpy_is_portable

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = rr.DTYPES


def _pixel_measures(name, dtype, by_ring):
    """(pixels with more than one row, pixels whose minimum r is shared, pixels whose winner is not their first row)"""
    c, e = rr.case(name, dtype), rr.expected(name, dtype, by_ring)
    po, r = e["pixel_of"], rr.ranges(c["rows"])
    who = np.flatnonzero(po >= 0)
    at_min = r[who] == e["image"][:, 0].reshape(-1)[po[who]]
    shared = np.zeros(e["count"].size, np.int64)
    np.add.at(shared, po[who], at_min)
    first = np.full(e["count"].size, -1, np.int64)
    first[po[who[::-1]]] = who[::-1]
    return int((e["count"] > 1).sum()), int((shared > 1).sum()), int(((e["index"].reshape(-1) != first) & (first >= 0)).sum())


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_ring", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_sweep_has_contested_pixels(dtype, by_ring):
    """Measured here (two frames): float32 4544 / 2007 / 1098 by elevation and 4096 / 2179 / 937 by channel, float64 4544 / 1785 / 1193 and
    4096 / 1932 / 1051."""
    several, shared, not_first = _pixel_measures("sweep", dtype, by_ring)
    assert several >= 1000 and shared >= 100 and not_first >= 100, (several, shared, not_first)
    c, e = rr.case("sweep", dtype), rr.expected("sweep", dtype, by_ring)
    assert c["rows"].dtype == np.dtype(dtype) and (e["pixel_of"] >= 0).all() and int(e["count"].sum()) == len(c["rows"])
    assert e["pixel_of"][:8192].max() < 64 * 96 <= e["pixel_of"][8192:].min()              # every frame in its own image


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_sweep_carries_no_edge(dtype):
    """No row of the sweep lies within 1e-6 of a pixel edge and none is clamped: `constructed` alone carries the edges."""
    c = rr.case("sweep", dtype)
    px, py = rr.px_py(c["rows"], c["H"], c["W"], c["fov"])
    assert np.abs(px - np.round(px)).min() > 1e-6 and np.abs(py - np.round(py)).min() > 1e-6
    assert py.min() >= 0.0 and py.max() < c["H"] and px.min() >= 0.0 and px.max() < c["W"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_frame_meets_the_conditions(dtype):
    c = rr.case("constructed", dtype)
    rows, role, H, W = c["rows"], c["role"], c["H"], c["W"]
    e, er = rr.expected("constructed", dtype), rr.expected("constructed", dtype, True)
    po = e["pixel_of"]
    px, py = rr.px_py(rows, H, W, c["fov"])

    def span(name):
        return np.arange(role[name][0], role[name][0] + role[name][1])

    # the edge rows: px within a few ulps of the integer c, and both outcomes of the floor occur (beyond the clipped ends)
    ed = span("edges")
    want = np.repeat(np.arange(W + 1), 3)
    assert np.abs(px[ed] - want).max() < 1e-4 * (1 if dtype == "float64" else 100)
    fl = np.floor(px[ed]).astype(int)
    inner = (want > 0) & (want < W)
    assert set((fl - want)[inner].tolist()) == {0, -1} and (fl[inner] == want[inner]).sum() >= 10 and (fl[inner] == want[inner] - 1).sum() >= 10
    assert (np.floor(px[ed][want == W]) >= W - 1).all() and (po[ed][want == W][po[ed][want == W] >= 0] % W == W - 1).all()
    # the seam: y = +0.0 is column 0, y = -0.0 column W - 1 (px = W, clipped)
    a = role["seam"][0]
    assert px[a] == 0.0 and px[a + 1] == W and po[a] % W == 0 and po[a + 1] % W == W - 1
    # x = +-0.0 with y != 0, and the axis: usable, atan2(0, 0) = 0 and atan2(0, -0) = pi
    assert (po[span("x_zero")] >= 0).all() and (po[span("axis")] >= 0).all()
    assert sorted(set((po[span("axis")] % W).tolist())) == [0, W // 2] and set((po[span("axis")] // W).tolist()) == {0, H - 1}
    # clamped to image rows 0 and H - 1
    assert (py[span("above")] < 0).all() and (po[span("above")] // W == 0).all()
    assert (py[span("below")] >= H).all() and (po[span("below")] // W == H - 1).all()
    # the limits: strict, in the rows' dtype
    a = role["limits"][0]
    assert (po[a:a + 4] >= 0).tolist() == [False, True, False, True]
    r = rr.ranges(rows)
    dt = rows.dtype.type
    assert r[a] == dt(c["limits"][0]) and r[a + 2] == dt(c["limits"][1])
    if dtype == "float32":
        assert float(r[a]) > c["limits"][0] and float(r[a + 2]) < c["limits"][1]        # compared in float64 both would be inside
    # every clause rejects a row that the others accept (the finite clause: with the default limits, whose hi is +inf)
    present, finite, inside, channel = rr.clauses(rows, H, c["ring"], c["limits"], c["keep"])
    for k, clause in enumerate((present, inside, channel)):
        others = [x for j, x in enumerate((present, finite, inside, channel)) if x is not clause]
        assert (~clause & np.logical_and.reduce(others)).sum() >= 2, k
    present, finite, inside, channel = rr.clauses(rows, H, c["ring"], rr.NO_LIMITS, c["keep"])
    assert (~finite & present & inside & channel).sum() >= 3 and finite[role["at_bound"][0]]
    assert not finite[span("not_finite")].any() and (po[span("not_finite")] == -1).all() and po[role["origin"][0]] == -1
    assert (e["pixel_of"][span("bad_ring")] >= 0).all() and (er["pixel_of"][span("bad_ring")] == -1).all()
    # three rows of equal r in one pixel: the first wins; the absent rows on the same rays would have won
    for out in (e, er):
        a = role["equal_r"][0]
        p = out["pixel_of"][a]
        assert (out["pixel_of"][a:a + 3] == p).all() and len(set(r[a:a + 3].tolist())) == 1
        assert out["index"].reshape(-1)[p] == a and out["image"][0, 4].reshape(-1)[p] == 3 and out["count"].reshape(-1)[p] == 3
        b = role["nearest_last"][0]
        q = out["pixel_of"][b]
        last = len(rows) - 1
        assert (out["pixel_of"][[b, b + 1, b + 2, last]] == q).all() and out["index"].reshape(-1)[q] == last and r[last] < r[b:b + 3].min()
        free = rr.project(rows, H, W, c["fov"], c["ring"] if out is er else None, c["limits"], 4, None)
        ab = span("absent")
        assert (free["pixel_of"][ab] == (p, q)).all() and (free["index"].reshape(-1)[[p, q]] == ab).all() and (out["pixel_of"][ab] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_case(dtype):
    c = rr.case("shapes", dtype)
    assert np.diff(c["offsets"]).tolist() == [37, 37, 0, 8192]
    for shape in rr.SHAPES:
        H, W = shape
        e = rr.expected("shapes", dtype, shape=shape)
        assert e["index"].shape == (4, H, W) and (e["index"][2] == -1).all() and not e["count"][2].any()
        po = e["pixel_of"]
        assert po[11] == -1 and po[48] == -1                                          # the origin rows
        rest = np.setdiff1d(np.arange(37), [11])
        assert (po[rest] >= 0).all() and (po[37 + rest] == po[rest] + H * W).all()     # the same (row, col), one frame on
        assert (e["count"][3] > 1).any() or H * W > 8192
    er = rr.expected("shapes", dtype, True)
    assert (er["pixel_of"][74:] == -1).sum() > 7000 and (er["pixel_of"][74:] >= 0).sum() > 500       # channels beyond H = 5


def test_the_restatement_takes_its_atan2_from_libm():
    g = np.random.default_rng(5)
    y, x = g.uniform(-80, 80, 4096), g.uniform(-80, 80, 4096)
    got = rr.arctan2(y, x)
    assert np.abs(got - np.arctan2(y, x)).max() < 1e-15
    if numpy_is_portable():
        assert np.array_equal(got, np.arctan2(y, x))


# ---- csrc/sg_range.h on the host ----------------------------------------------------------------------------------------------------------------
def _compile(tmp, source, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra,
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / source),
           "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def pixels_harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("range"), "range_pixels.cpp", "range_pixels")


@pytest.fixture(scope="module")
def pixels_harness_sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("range_san"), "range_pixels.cpp", "range_pixels_san",
                    ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _walk(exe, tmp_path, name, dtype, by_ring, shape=None, limits=None):
    c = rr.case(name, dtype)
    H, W = shape or (c["H"], c["W"])
    limits = limits or c["limits"]
    rows, n, F = c["rows"], len(c["rows"]), len(c["offsets"]) - 1
    fo, fi, fk, fr, fout = (tmp_path / f"w.{s}" for s in ("off", "in", "keep", "ring", "out"))
    np.asarray(c["offsets"], np.int64).tofile(fo)
    np.ascontiguousarray(rows[:, :3], np.float64).tofile(fi)
    (np.ones(n, np.uint8) if c["keep"] is None else c["keep"].astype(np.uint8)).tofile(fk)
    np.asarray(c["ring"], np.int32).tofile(fr)
    fov = np.radians(np.array(c["fov"], np.float64))
    cmd = [str(exe), "walk", str(DTYPES.index(dtype)), str(int(by_ring)), str(H), str(W), repr(float(fov[0])), repr(float(fov[1])), repr(float(limits[0])),
           repr(float(limits[1])), str(F), str(fo), str(fi), str(fk), str(fr), str(fout)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(fout, np.int32)
    px = F * H * W
    assert len(raw) == n + 2 * px and r.stdout.split() == ["walk", str(n), str(px)]
    want = rr.expected(name, dtype, by_ring, shape=shape, limits=limits)
    what = (name, dtype, by_ring, shape, limits)
    assert np.array_equal(raw[:n], want["pixel_of"]), what
    assert np.array_equal(raw[n:n + px], want["index"].reshape(-1)), what
    assert np.array_equal(raw[n + px:], want["count"].reshape(-1)), what


@pytest.mark.parametrize("by_ring", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_walk_equals_the_restatement(pixels_harness, tmp_path, dtype, by_ring):
    for name in rr.CASES:
        _walk(pixels_harness, tmp_path, name, dtype, by_ring)
    _walk(pixels_harness, tmp_path, "constructed", dtype, by_ring, limits=rr.NO_LIMITS)
    for shape in rr.SHAPES:
        _walk(pixels_harness, tmp_path, "shapes", dtype, by_ring, shape=shape)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_walk_under_sanitizers(pixels_harness_sanitized, tmp_path, dtype):
    """The same program under AddressSanitizer and UBSan: host code only, a stand-alone program."""
    for by_ring in (False, True):
        _walk(pixels_harness_sanitized, tmp_path, "constructed", dtype, by_ring)
        _walk(pixels_harness_sanitized, tmp_path, "shapes", dtype, by_ring, shape=(5, 67))


def test_guarded_angles_give_the_pixels_of_the_definition(pixels_harness):
    """10^7 points and more, most of them within four ulps of a column or an image-row edge, for W in {1, 96, 2048} and H in {1, 64}: the
    fast angle behind its guard band gives the pixel that sg_atan2_cr gives.  (On the host the fast atan2 is libm's.)"""
    r = subprocess.run([str(pixels_harness), "guard", "1700000"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    word, settings, points, different, share = r.stdout.split()
    print("share of the angles decided by sg_atan2_cr:", share)
    assert word == "guard" and int(settings) == 6 and int(points) >= 10 ** 7 and int(different) == 0
    assert 0.0 < float(share) < 0.5              # the edge points do take the slow route; the uniform ones do not


def test_guarded_angles_under_sanitizers(pixels_harness_sanitized):
    r = subprocess.run([str(pixels_harness_sanitized), "guard", "20000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.split()[:2] == ["guard", "6"] and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-2000:]


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_range_image_device"
APART = {"keep_in": " overlaps d_keep_in; the mask is read while the image is written: pass a buffer apart from it",
         "rows": " overlaps d_rows; the rows are read while the image is written: pass a buffer apart from them",
         "ring": " overlaps d_ring; the channels are read while the image is written: pass a buffer apart from them"}
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "mode": WHO + ": needs fov2 (image rows by elevation) or d_ring (image rows by channel)",
    "rows": "batch too large: split it below 2^31 rows",
    "features": WHO + ": n_features must be 3, 4 or 5: the columns of a row that a pixel stores",
    "size": WHO + ": height and width must be at least 1",
    "pixels": WHO + ": n_frames * height * width exceeds 2^31 - 1; split the batch",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "fov_domain": WHO + ": fov_up and fov_down must lie within [-pi/2, pi/2] (radians)",
    "fov_order": WHO + ": the field of view needs fov_down < fov_up",
    "limit_nan": WHO + ": a range limit is NaN; pass NULL for (0, +inf)",
    "limit_order": WHO + ": the range limits need 0 <= lo < hi",
    "image_keep": WHO + ": d_out_image" + APART["keep_in"],
    "index_keep": WHO + ": d_out_index" + APART["keep_in"],
    "pixel_of_keep": WHO + ": d_out_pixel_of" + APART["keep_in"],
    "count_keep": WHO + ": d_out_count" + APART["keep_in"],
    "image_rows": WHO + ": d_out_image" + APART["rows"],
    "index_rows": WHO + ": d_out_index" + APART["rows"],
    "pixel_of_rows": WHO + ": d_out_pixel_of" + APART["rows"],
    "count_rows": WHO + ": d_out_count" + APART["rows"],
    "image_ring": WHO + ": d_out_image" + APART["ring"],
    "index_ring": WHO + ": d_out_index" + APART["ring"],
    "pixel_of_ring": WHO + ": d_out_pixel_of" + APART["ring"],
    "count_ring": WHO + ": d_out_count" + APART["ring"],
    "index_image": WHO + ": d_out_index overlaps d_out_image" + OWN,
    "pixel_of_image": WHO + ": d_out_pixel_of overlaps d_out_image" + OWN,
    "pixel_of_index": WHO + ": d_out_pixel_of overlaps d_out_index" + OWN,
    "count_image": WHO + ": d_out_count overlaps d_out_image" + OWN,
    "count_index": WHO + ": d_out_count overlaps d_out_index" + OWN,
    "count_pixel_of": WHO + ": d_out_count overlaps d_out_pixel_of" + OWN,
}
ACCEPTED = ("clean", "null_out_count", "null_keep_in", "null_limits", "float64", "empty_null_rows", "channel_mode", "channel_mode_ignores_fov",
            "features_3", "features_5", "one_pixel", "pixels_2p31_minus_1", "frame_2p30_rows", "fov_half_pi", "limit_hi_inf", "limit_lo_zero_hi_tiny",
            "keep_in_behind_image", "index_behind_rows", "pixel_of_behind_ring", "index_behind_image")
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_out_image", "null_out_index", "null_out_pixel_of", "bad_dtype", "no_frames", "negative_rows", "null_and_no_mode"),
    "mode": ("no_mode", "no_mode_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_features_2"),
    "features": ("features_2", "features_6", "features_2_and_height_0"),
    "size": ("height_0", "width_0", "height_negative"),
    "pixels": ("pixels_2p31", "pixels_overflowing", "pixels_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_fov_nan"),
    "fov_domain": ("fov_up_above_half_pi", "fov_down_below_half_pi", "fov_nan", "fov_inf", "fov_degrees", "fov_degrees_and_fov_reversed"),
    "fov_order": ("fov_reversed", "fov_up_is_down", "fov_reversed_and_limit_nan_lo"),
    "limit_nan": ("limit_nan_lo", "limit_nan_hi", "limit_nan_hi_and_limit_lo_negative"),
    "limit_order": ("limit_lo_negative", "limit_lo_is_hi", "limit_reversed", "limit_lo_inf", "limit_reversed_and_index_is_keep_in"),
    "image_keep": ("image_overlaps_keep_in",),
    "index_keep": ("index_is_keep_in",),
    "pixel_of_keep": ("pixel_of_overlaps_keep_in",),
    "count_keep": ("count_overlaps_keep_in",),
    "image_rows": ("image_is_rows",),
    "index_rows": ("index_overlaps_rows",),
    "pixel_of_rows": ("pixel_of_overlaps_rows",),
    "count_rows": ("count_overlaps_rows",),
    "image_ring": ("image_overlaps_ring",),
    "index_ring": ("index_is_ring",),
    "pixel_of_ring": ("pixel_of_is_ring",),
    "count_ring": ("count_overlaps_ring",),
    "index_image": ("index_overlaps_image",),
    "pixel_of_image": ("pixel_of_overlaps_image",),
    "pixel_of_index": ("pixel_of_overlaps_index",),
    "count_image": ("count_overlaps_image",),
    "count_index": ("count_is_index",),
    "count_pixel_of": ("count_overlaps_pixel_of",),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "range_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "range_refusals.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split("|", 1) for ln in r.stdout.splitlines())
    want = {case: "0|OK" for case in ACCEPTED}
    for key, cases in REFUSED.items():
        want.update({case: "1|" + MESSAGES[key] for case in cases})
    assert got == want
    assert set(MESSAGES) == set(REFUSED)              # every message is reached


def test_the_entry_is_declared_and_bound():
    from lidar_snow_sim_amd import _native
    header = (ROOT / "include" / "snowgpu.h").read_text()
    assert "int snowgpu_range_image_device(" in header and "snowgpu_range_image_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_range_image_device") and hasattr(_native.Context, "range_image_device")
    assert "snowgpu_range.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import range_image, tensors
    assert callable(tensors.range_image) and callable(tensors.RangeImageBatch.empty) and callable(tensors.RangeImageBatch.to_rows)
    assert callable(range_image.project)
