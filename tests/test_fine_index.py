"""The scan without the range search (csrc/sg_beam.h: sg_wave_scan on the step-major index the library files, csrc/sg_range_index.h) on the
host, and the new input of the GPU test.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fine_index_inputs as fii
import range_index_inputs as rii
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_scan_on_the_filed_index_without_a_search_equals_the_full_binary_search(tmp_path):
    """tests/host_harness/fine_index_no_search.cpp: the index the library files (its words checked against a plain count) and the legacy
    shape, each against the scan with no index -- beam for beam the same count, overflow, undecided bit, list, order and overflow slot,
    float32 and float64, deferred and in place.  The sparse table must have shown a run of more than 64 dropped candidates and beams with
    five flakes or more whose dropped candidates lie between them in scan order."""
    exe = tmp_path / "fine_index_no_search"
    src = ROOT / "tests" / "host_harness" / "fine_index_no_search.cpp"
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-w",
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(src), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("fine<")]
    assert len(lines) == 12 and all(" 0 mismatches" in ln for ln in lines), r.stdout
    assert sum("(step-major index)" in ln for ln in lines) == 10 and all("(no step-major index)" in ln for ln in lines[-2:]), r.stdout
    for dt in ("float32", "float64"):
        for mode in ("deferred", "in place"):
            assert sum(ln.startswith(f"fine<{dt}, {mode}>") for ln in lines) >= 2, r.stdout
    for ln in lines:                                       # every case has beams whose first bin is the last and whose next is bin 0
        assert int(ln.split(" beyond the list, ")[1].split(" across the seam")[0]) > 0, ln
    assert "INDEX" not in r.stdout and "not the case meant" not in r.stdout and "expected none" not in r.stdout, r.stdout
    run = [ln for ln in r.stdout.splitlines() if ln.startswith("sparse: longest run")]
    assert len(run) == 1 and int(run[0].split("dropped candidates ")[1].split(",")[0]) > 64, r.stdout


def test_fine_frame_is_what_it_is_taken_for():
    f = fii.fine_frame()
    assert f.shape == (4096, 5) and f.dtype == np.float32
    d = np.linalg.norm(f[:, :3].astype(np.float64), axis=1).reshape(64, 64)
    assert np.array_equal(d[:, :30], np.tile(2.0 * np.arange(1, 31), (64, 1)))                # exactly on the 2 m edges
    assert (np.mod(d[:, 30:40], 2.0) == 0).all() and d[:, 30:40].min() >= 62 and d[:, 30:40].max() <= 118
    assert len(np.unique(d[:, 30:40])) == 29                                                  # every edge between 62 and 118 m
    assert np.array_equal(d[:, 40:47], np.tile(fii.RECORD_RANGES, (64, 1)))                   # exactly at a record's range
    assert (np.abs(d[:, 47:54] / fii.RECORD_RANGES - 1.0) < 3e-7).all() and (d[:, 47:54] != fii.RECORD_RANGES).any()
    assert (np.abs(d[:, 58:62] - np.array([126.0, 128.0, 130.0, 200.0])) < 1e-4).all()       # the last step (off the axes: to a rounding)
    far = np.mod(np.arctan2(f[:, 1], f[:, 0]).reshape(64, 64)[:, 58:62], 2 * np.pi)
    assert ((far > rii.FREE[0] - 1e-6) & (far < rii.FREE[1] + 1e-6)).all() and (d[:, :58] < 120.0).all() and (d[:, 62:] < 120.0).all()
    t = fii.table()
    rho, phi = np.hypot(t[:, 0], t[:, 1]), np.mod(np.arctan2(t[:, 1], t[:, 0]), 2 * np.pi)
    assert not ((phi > rii.FREE[0] - 0.04) & (phi < rii.FREE[1] + 0.04)).any()
    assert all((rho[t[:, 1] == 0] == r).any() for r in fii.RECORD_RANGES) and all((rho[t[:, 1] == 0] == 2.0 * k).any() for k in range(1, 60))
    assert ((rho >= 40.0) & (rho < 42.0) & (np.minimum(phi, 2 * np.pi - phi) < 0.0011)).sum() >= 60   # one crowded step at the seam


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cpu_twin_equals_the_oracle_on_the_fine_frame(dtype):
    """The two references agree on the new frame (neither uses an index): rows kept, labels, intensities, statistics; moved coordinates to
    the tolerance tests/test_range_index.py uses."""
    from lidar_snow_sim_amd import build, _cpu_twin
    from oracle import snow_oracle
    snow_oracle.build()
    build.build_cpu_twin(verbose=False)
    tl = fii.tables()
    pc = fii.fine_frame(dtype)
    order = list(range(64))
    (st, aug, src), = _cpu_twin.augment_batch([pc], tl, [order], rii.BD, [rii.POLY], threads=4)
    s0, a0, src0 = snow_oracle.augment(pc, tl, rii.BD, order, thr_poly=np.array(rii.POLY))
    assert tuple(int(v) for v in st) == tuple(int(v) for v in s0)
    assert np.array_equal(src, src0) and np.array_equal(aug[:, 3:], a0[:, 3:])
    np.testing.assert_allclose(aug[:, :3], a0[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
    assert int(np.isin(aug[:, 4], (1, 2)).sum()) > 20
