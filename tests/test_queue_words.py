"""The dict queue of the pass over all rows (csrc/sg_queue.h: range, azimuth and one word per listed flake, resolved by the reader) without a
GPU: the writer's and the readers' functions on the host against the hand-over they replace, and the populations of the frame that
tests/test_gpu_queue_words.py adds (tests/queue_words_inputs.py) from the oracle alone."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import queue_words_inputs as qwi
import row_tier_inputs as rti
import test_row_tier_inputs as tri

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = [np.float32, np.float64]


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
@pytest.mark.parametrize("row_header", [1, 0])
def test_stored_and_resolved_slots_equal_the_old_hand_over_bit_for_bit(tmp_path, row_header):
    """tests/host_harness/queue_words.cpp: on a filed table, 2 x 300 000 random float32 / float64 beams (a sixteenth each aimed at azimuth 0 and
    at record 0 of the table) scanned with the one-word lists, stored with sg_dq_store_* and, a run of 192 slots at a time (three groups, starting
    inside one), loaded with sg_dq_load_* / sg_dq_resolve_all / sg_dq_resolve: (d, theta, a1[j], a2[j], rho[j], L) are what sg_hit_angles and the
    scan's range column gave in the old plane order, 0 mismatches -- for the layouts of the capacities 4, 8, 16 and 63, and with the header in the
    row dtype (the default) and in float64.  The harness also walks every (slot, plane) cell of four groups per layout: no word is shared, none
    lies outside, slots 63 and 64 fall into neighbouring groups; and it fails if a population -- lists of 1 .. 4, wrapped wedges, each
    combination of the limit-ray bits, words of record 0 -- stayed empty."""
    exe = tmp_path / "queue_words"
    src = ROOT / "tests" / "host_harness" / "queue_words.cpp"
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-w", f"-DSG_DQ_ROW_HEADER={row_header}",
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(src), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), "300000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    runs = [ln for ln in r.stdout.splitlines() if ln.startswith("queue<")]
    layouts = [ln for ln in r.stdout.splitlines() if ln.startswith("layout<")]
    assert len(runs) == 8 and all(" 0 mismatches" in ln for ln in runs), r.stdout
    assert len(layouts) == 8 and all(" 0 faults" in ln for ln in layouts), r.stdout
    words = 1 if row_header else 2
    assert sum(f"float32, capacity {c}, {words} header word" in ln for ln in runs for c in (4, 8, 16, 63)) == 4, r.stdout


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    snow_oracle.build()
    return snow_oracle


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_crowd_frame_fills_a_region_as_its_name_claims(so, dtype):
    """get_occlusions of the oracle on the frame's rows: the flakes every beam meets.  On the crowded channel, for every few-flake limit
    f = 1 .. 3 and every capacity 4, 8, 16 of the pass over all rows: more than 64 beams in the front run (1 .. f flakes), a back run
    (f + 1 .. capacity flakes), neither a multiple of 64; and the status words the GPU test expects."""
    fr = qwi.crowd(dtype)
    rows, bd = fr["rows"], fr["bd"]
    assert (np.diff(rows[:, 4]) >= 0).all()
    d, ang = tri.beam_angles_of(rows, bd)
    n_hit, max_owner = np.zeros(rows.shape[0], np.int64), np.zeros(rows.shape[0], np.int64)
    for ch in np.unique(rows[:, 4]).astype(int):
        idx = np.flatnonzero(rows[:, 4] == ch)
        table = np.ascontiguousarray(fr["tables"][ch], np.float64)
        n_hit[idx] = so.get_occlusions(ang[idx], d[idx], table, bd)[4]
        info = so.flake_table(table)
        for i in idx[n_hit[idx] > 4]:                                # the later tiers' beams: slots of the flake that owns most (the restatement)
            iv = tri.beam_intervals(table, info, ang[i, 0], ang[i, 1], d[i])
            assert iv.shape[0] == n_hit[i]
            max_owner[i] = tri.occlusion_dict(ang[i], iv, d[i], bd)[1].max()
    crowd = n_hit[rows[:, 4] == qwi.CROWD_CHANNEL]
    assert crowd.shape[0] == qwi.CROWD_BEAMS
    for first in (4, 8, 16):
        for few in (1, 2, 3):
            front, back = int(((crowd >= 1) & (crowd <= few)).sum()), int(((crowd > few) & (crowd <= first)).sum())
            assert front > 64 and front % 64 != 0 and back > 0 and back % 64 != 0, (first, few, front, back)
        assert (rti.class_populations(n_hit, first), rti.redo_count(n_hit, max_owner, first)) == qwi.EXPECTED[first], first
    assert qwi.EXPECTED[4][0][0] > 0                                 # ... and the 8-entry tier runs beside the queue
