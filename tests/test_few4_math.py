"""The arithmetic of k_power_few<T, 4> (csrc/sg_few.h with N = 4) against the general per-lane path (csrc/sg_beam.h) on the host.

Both are the device functions the kernels run, compiled for the host by hipcc (--cuda-host-only, -ffp-contract=off).  For float32 and
float64 rows and L = 1 .. 4 flakes, 300 000 random beams each (the generator of few_vs_general.cpp: wedges at azimuth 0 / 2 pi, shared
endpoints, identical intervals, equal ranges) and constructed lists -- the nearest flake spanning the other three and both limit rays
(nine elementary slots), the second nearest with eight, the same across the 0 / 2 pi seam, a byte-identical twin, a flake wholly behind
a nearer one, four disjoint flakes (the hard target at its five slots), inverted intervals that leave the hard target eight and nine --
must give the same S, amplitudes, ranges, bin windows, best sum, arg-max bin, range_error and packed record, bit for bit.

With eight or nine slots np.sum is NumPy's blocked pairwise sum.  Whether that route was taken is judged by the program's own restatement
of compute_occlusion_dict (slot counts, the pairwise and the left-to-right sum of the same widths): 2 x 301 beams just left of azimuth 0
carry an eight-slot owner whose sum stays below the wedge's width, on some of them the two sums give amplitudes that differ in their bits,
and there the register path must give the pairwise one -- the program fails if the order shows on none of them (with the pairwise branch
of sg_few.h disabled it reports those beams as mismatches).  A nine-slot owner holds both limit rays, so its ratio is clipped to 1 in
either order (asserted): such owners must occur and match, more cannot be seen of them.  The program prints the largest slot count per
kind of owner.  No oracle, no GPU."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_four_flake_register_path_equals_the_general_path_bit_for_bit(tmp_path):
    exe = tmp_path / "few4_vs_general"
    src = ROOT / "tests" / "host_harness" / "few4_vs_general.cpp"
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-w",
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), "300000"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("few4<")]
    assert len(lines) == 10 and all(" 0 mismatches" in ln for ln in lines), r.stdout
    random_lines = [ln for ln in lines if " L=" in ln]
    assert len(random_lines) == 8 and all(" 300000 cases" in ln for ln in random_lines), r.stdout
    for ln in (ln for ln in lines if "constructed" in ln):
        m = re.search(r"most slots: nearest (\d+) farther (\d+) target (\d+); pairwise sums that matched: (\d+) of eight, (\d+) of nine; eight-slot owners whose "
                      r"amplitude shows the order of the sum, all equal to the pairwise one: (\d+); nine-slot owners with a ratio below 1: (\d+)", ln)
        assert m, ln
        nearest, farther, target, eight, nine, shows, unclipped = map(int, m.groups())
        assert nearest == 9 and farther == 8 and target == 9 and eight >= 1 and nine >= 1 and shows >= 1 and unclipped == 0, ln
