"""Dynamic radius outlier removal without a GPU: the NumPy restatement of the definition (tests/dror_reference.py) against SciPy's kd-tree,
the conditions under which the comparisons of tests/test_gpu_dror.py are not vacuous, and the binning functions of csrc/sg_dror.h, compiled
for the host (tests/host_harness/dror_cells.cpp), for coverage: a neighbour's cell always lies inside the query's window."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dror_reference as dr
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = ("float32", "float64")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("setting", dr.SETTINGS)
def test_restatement_against_scipy(setting, dtype):
    """The unsaturated count lies between the kd-tree's counts at r (1 - 1e-9) and r (1 + 1e-9) (the query point itself taken off), and
    equals them where the two agree."""
    from scipy.spatial import cKDTree
    alpha, beta, _, sr_min = setting
    for name in dr.cloud_names(setting):
        pc = dr.cloud(name, dtype)
        xyz = np.asarray(pc[:, :3], np.float64)
        _, _, count = dr.expected(name, dtype, setting)
        s2, _ = dr.search_radius2(xyz, alpha, beta, sr_min)
        r = np.sqrt(s2)
        tree = cKDTree(xyz)
        lo = tree.query_ball_point(xyz, r * (1 - 1e-9), return_length=True) - 1
        hi = tree.query_ball_point(xyz, r * (1 + 1e-9), return_length=True) - 1
        assert np.all(lo <= count) and np.all(count <= hi), name
        same = lo == hi
        assert same.mean() > 0.99 and np.array_equal(count[same], lo[same]), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("setting", dr.SETTINGS)
def test_clouds_meet_the_conditions(setting, dtype):
    alpha, beta, k_min, sr_min = setting
    c, c2, s2min = dr.constants(alpha, beta, sr_min)
    at_k = below_k = 0
    for name in dr.cloud_names(setting):
        pc = dr.cloud(name, dtype)
        keep, _, count = dr.expected(name, dtype, setting)
        assert keep.sum() >= 16 and (~keep).sum() >= 16, (name, int(keep.sum()))
        _, q = dr.search_radius2(pc, alpha, beta, sr_min)
        r = np.sqrt(q)
        if r.min() < sr_min / c < r.max():
            static = c2 * q <= s2min
            assert static.sum() >= 16 and (~static).sum() >= 16, (name, int(static.sum()))
        at_k += int((count == k_min).sum())
        below_k += int((count == k_min - 1).sum())
    assert at_k >= 16 and below_k >= 16, (at_k, below_k)


@pytest.mark.parametrize("setting", dr.SETTINGS)
def test_seam_clouds_have_pairs_across_the_seam(setting):
    alpha, beta, _, sr_min = setting
    for i, (_, centre) in enumerate(dr.SECTOR_CASES):
        if centre != np.pi:
            continue
        xyz = np.asarray(dr.cloud(f"sector{i}")[:, :3], np.float64)
        s2, _ = dr.search_radius2(xyz, alpha, beta, sr_min)
        for sign in (1, -1):                                   # queries on either side with a neighbour on the other
            qs = np.flatnonzero((sign * xyz[:, 1] > 0) & (xyz[:, 0] < 0))
            other = xyz[(sign * xyz[:, 1] < 0) & (xyz[:, 0] < 0)]
            d = xyz[qs, None, :] - other[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert int((d2 <= s2[qs, None]).sum()) >= 16, (i, sign)


def test_constructed_frame_has_both_sides():
    for dtype in DTYPES:
        pc, info = dr.constructed_frame(np.dtype(dtype).type)
        assert 1900 <= pc.shape[0] <= 2100
        xyz = np.asarray(pc[:, :3], np.float64)
        s2, _ = dr.search_radius2(xyz, 0.45, 3, 0.04)
        a, b = np.array([p[0] for p in info["pairs"]]), np.array([p[1] for p in info["pairs"]])
        d = xyz[b] - xyz[a]
        inside = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= s2[a]
        assert inside.sum() >= 100 and (~inside).sum() >= 100, (dtype, int(inside.sum()))
        if dtype == "float64":                                  # in float64 every pair falls on the side it was built for
            assert np.array_equal(inside, np.array([p[2] for p in info["pairs"]]) < 0)


# ---- the binning functions on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("dror") / "dror_cells"
    src = ROOT / "tests" / "host_harness" / "dror_cells.cpp"
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-w",
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(src), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


SOURCES = ("random", "edge", "seam", "boundary", "core", "far500", "far1e5")


@pytest.mark.parametrize("setting", dr.SETTINGS)
def test_window_covers_every_neighbour(harness, setting):
    """At least 10^6 neighbour pairs per setting -- float32-valued and float64 coordinates, three cell budgets -- from seven sources: each
    contributes, and no neighbour's cell lies outside the query's window."""
    total = 0
    for f32 in (0, 1):
        for budget in (1024, 16384, 81920):
            r = subprocess.run([str(harness), "pairs", *(repr(float(v)) if i != 2 else str(v) for i, v in enumerate(setting)), str(budget), str(f32), "30000",
                                str(17 + f32)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            lines = [ln.split() for ln in r.stdout.splitlines()]
            assert [ln[0] for ln in lines[:7]] == list(SOURCES)
            for name, checked, bad in lines[:7]:
                assert int(checked) >= 10000 and int(bad) == 0, (setting, f32, budget, name, checked, bad)
                total += int(checked)
    assert total >= 1_000_000, total


@pytest.mark.parametrize("budget", (1024, 16384))
@pytest.mark.parametrize("setting", dr.SETTINGS)
def test_host_walk_equals_restatement(harness, tmp_path, setting, budget):
    """One frame through the kernels' steps on the host (file every row, walk the windows, stop at k_min): the saturated counts of the
    restatement, on a sector cloud across the seam, the full circle and the constructed frame."""
    alpha, beta, k_min, sr_min = setting
    clouds = [dr.cloud("sector3"), dr.cloud("circle", "float64"), dr.constructed_frame(np.float64)[0]]
    for j, pc in enumerate(clouds):
        xyz = np.ascontiguousarray(pc[:, :3], np.float64)
        fi, fo = tmp_path / f"in{j}.bin", tmp_path / f"out{j}.bin"
        xyz.tofile(fi)
        r = subprocess.run([str(harness), "cloud", repr(float(alpha)), repr(float(beta)), str(k_min), repr(float(sr_min)), str(budget), str(fi), str(fo)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(fo, np.int32)
        ok, nb, _ = dr.dror(xyz, alpha, beta, k_min, sr_min)[0:3]
        usable = dr.usable_rows(xyz)
        assert np.array_equal(got[usable], nb[usable]) and np.all(got[~usable] == -1), (setting, budget, j)


def test_domain(harness):
    """The grid maker refuses what the definition excludes (SNOWGPU_E_INVALID in the C ABI): the harness leaves with status 3."""
    def status(alpha, beta, k_min, sr_min):
        return subprocess.run([str(harness), "pairs", repr(alpha), repr(beta), str(k_min), repr(sr_min), "4096", "0", "10", "1"],
                              capture_output=True, text=True, timeout=60).returncode
    assert status(0.45, 3.0, 3, 0.04) == 0 and status(0.45, 3.0, 0, 0.0) == 0 and status(0.45, 3.0, 65535, 1e300) == 0
    assert status(14.3239, 1.0, 3, 0.04) == 0                  # c = 0.249999...
    for bad in ((0.0, 3.0, 3, 0.04), (-0.45, 3.0, 3, 0.04), (14.33, 1.0, 3, 0.04), (float("nan"), 3.0, 3, 0.04), (0.45, 3.0, 3, -0.01),
                (0.45, 3.0, 3, float("inf")), (0.45, 3.0, 3, float("nan")), (0.45, 3.0, -1, 0.04), (0.45, 3.0, 65536, 0.04)):
        assert status(*bad) == 3, bad
