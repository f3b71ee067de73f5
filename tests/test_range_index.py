"""The scan's step-major range index (csrc/sg_range_index.h, sg_beam.h: sg_wave_scan) on the host, and the inputs of the GPU test.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import range_index_inputs as rii
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_scan_with_the_step_major_index_equals_the_full_binary_search(tmp_path):
    """tests/host_harness/range_index_vs_search.cpp: tables filed by the product's host filing and indexed by sg_range_index_fill (the
    function k_table_index runs), its counts checked against a plain count; sg_wave_scan with the index the table has, and with bin_q
    alone, against the scan with no index -- beam for beam the same count, list, order and overflow slot.  Tables: random; sparse with a
    crowded step and records at exactly 8, 16 and 120 m; every record beyond the targets; empty; a bin of more than 65 535 records, for
    which no step-major index is filed.  Beams: random, on the step edges, beyond 120 m, NaN, across the 0 / 2 pi seam."""
    exe = tmp_path / "range_index_vs_search"
    src = ROOT / "tests" / "host_harness" / "range_index_vs_search.cpp"
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-w",
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(src), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), "4000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("index<")]
    assert len(lines) == 8 and all(" 0 mismatches" in ln for ln in lines), r.stdout
    assert sum("(step-major index)" in ln for ln in lines) == 7 and "(no step-major index)" in lines[-1], r.stdout
    for ln in lines:                                       # every case has beams whose first bin is the last and whose next is bin 0
        assert int(ln.split(" beyond the list, ")[1].split(" across the seam")[0]) > 0, ln
    assert "INDEX" not in r.stdout and "not the case meant" not in r.stdout and "expected none" not in r.stdout, r.stdout


def test_gpu_test_inputs_are_what_they_are_taken_for():
    f1, f2 = rii.seam_frame(), rii.edge_frame()
    assert f1.shape == f2.shape == (4096, 5) and f1.dtype == np.float32
    az = np.arctan2(f1[:, 1], f1[:, 0]).reshape(64, 64)
    assert (az[:, :32] < 0).all() and (az[:, 32:] > 0).all() and np.abs(az).max() < 0.05      # every wave straddles the seam
    d = np.linalg.norm(f2[:, :3].astype(np.float64), axis=1).reshape(64, 64)
    assert np.array_equal(d[:, :15], np.tile(8.0 * np.arange(1, 16), (64, 1)))               # exactly on the step edges
    assert ((d[:, 30:38] >= 120.0) & (d[:, 30:38] < 120.002)).all() and (d[:, 38:46] > 120.002).all()
    assert np.isnan(d[:, 46:50]).all() and not np.isnan(d[:, :46]).any()
    far = np.mod(np.arctan2(f2[:, 1], f2[:, 0]).reshape(64, 64)[:, 38:46], 2 * np.pi)
    assert ((far > rii.FREE[0] - 1e-6) & (far < rii.FREE[1] + 1e-6)).all()
    sets = rii.table_sets()
    assert sorted(sets) == ["empty", "heavy", "small"] and sets["empty"][0].shape == (0, 3)
    for name, tl in sets.items():
        for t in {id(t): t for t in tl}.values():
            phi = np.mod(np.arctan2(t[:, 1], t[:, 0]), 2 * np.pi)
            assert not ((phi > rii.FREE[0] - 0.04) & (phi < rii.FREE[1] + 0.04)).any(), name
    phi = np.mod(np.arctan2(sets["heavy"][0][:, 1], sets["heavy"][0][:, 0]), 2 * np.pi)
    assert (np.floor(phi * 2048 / (2 * np.pi)) == 0).sum() >= 400                             # one bin holds nearly half the table


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cpu_twin_equals_the_oracle_on_the_gpu_test_inputs(dtype):
    """The two references of tests/test_gpu_range_index.py agree on its inputs (the small tables): rows kept, labels, intensities,
    statistics; moved coordinates to the parity tests' tolerance."""
    from lidar_snow_sim_amd import build, _cpu_twin
    from oracle import snow_oracle
    snow_oracle.build()
    build.build_cpu_twin(verbose=False)
    tl = rii.table_sets()["small"]
    frames = [rii.seam_frame(dtype), rii.edge_frame(dtype)]
    order = list(range(64))
    res = _cpu_twin.augment_batch(frames, tl, [order, order], rii.BD, [rii.POLY, rii.POLY], threads=4)
    for pc, (st, aug, src) in zip(frames, res):
        s0, a0, src0 = snow_oracle.augment(pc, tl, rii.BD, order, thr_poly=np.array(rii.POLY))
        assert tuple(int(v) for v in st) == tuple(int(v) for v in s0)
        assert np.array_equal(src, src0) and np.array_equal(aug[:, 3:], a0[:, 3:])
        np.testing.assert_allclose(aug[:, :3], a0[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
    assert sum(int((r[1][:, 4] == 2).sum()) for r in res) > 20
