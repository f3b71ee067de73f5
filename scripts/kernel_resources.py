"""Print registers / scratch / occupancy of every gfx950 kernel in csrc (hipcc resource-usage remarks).

usage: python scripts/kernel_resources.py [file.hip | all] [filter]

With no file (or "all") every .hip of build.SOURCES is reported, the files compiled side by side.  One line per
kernel, keyed by the full demangled name and sorted by it (no file name: a kernel that moves keeps its line), so
    diff <(python scripts/kernel_resources.py) <(python other_tree/scripts/kernel_resources.py)
compares two trees.
"""
import re, subprocess, sys, tempfile, os
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from lidar_snow_sim_amd.build import FLAGS, SOURCES

src = sys.argv[1] if len(sys.argv) > 1 else "all"
flt = sys.argv[2] if len(sys.argv) > 2 else ""
srcs = [s for s in SOURCES if s.endswith(".hip")] if src == "all" else [src]
with tempfile.TemporaryDirectory() as td:
    procs = [subprocess.Popen(["/opt/rocm/bin/hipcc", *[f for f in FLAGS if not f.startswith("-W")], "-w",
                               "-I" + root + "/include", "-c", root + "/lidar_snow_sim_amd/csrc/" + s, "-o", "%s/%d.o" % (td, n),
                               "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
             for n, s in enumerate(srcs)]
    outs = [p.communicate()[1] for p in procs]
    if any(p.returncode for p in procs):
        sys.exit("".join(outs))
cur = None
rows = []
for line in "".join(outs).splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"mangled": m.group(1)}
        rows.append(cur)
        continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
    if m and cur is not None:
        cur[m.group(1).strip()] = int(m.group(2))
names = subprocess.run(["c++filt"], input="\n".join(c["mangled"] for c in rows), capture_output=True, text=True).stdout.splitlines()
for c, n in zip(rows, names):
    c["name"] = n
for c in sorted(rows, key=lambda c: c["name"]):
    if flt in c["name"]:
        print("%s | VGPR %d AGPR %d SGPR %d scratch %d occ %d LDS %d vspill %d sspill %d" % (
            c["name"], c.get("VGPRs", -1), c.get("AGPRs", -1), c.get("TotalSGPRs", c.get("SGPRs", -1)), c.get("ScratchSize", -1),
            c.get("Occupancy", -1), c.get("LDS Size", -1), c.get("VGPRs Spill", -1), c.get("SGPRs Spill", -1)))
