"""Print VGPR / AGPR / scratch / LDS / occupancy and code size of every kernel (tuning aid, not a test).
usage: kernel_resources.py [another tree's cont2_amd.hip]"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "contour-context_amd", "csrc", "cont2_amd.hip")
obj = os.path.join(tempfile.mkdtemp(), "kres.co")  # the gfx950 code object alone: its kernel symbols' sizes are the code sizes
r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-fPIC", "-c", "--offload-device-only", "--no-gpu-bundle-output", src,
                    "-o", obj, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
cur = None
rows = {}
for line in r.stderr.splitlines():
    m = re.search(r"remark: (?:Function Name: )?(\S+)? ?\[-Rpass", line)
    m2 = re.search(r"remark: Function Name: (\S+)", line)
    if m2:
        cur = m2.group(1)
        mangled = cur
        dm = subprocess.run(["c++filt", cur], capture_output=True, text=True).stdout.strip()
        cur = re.sub(r"\(.*", "", dm).replace("void ", "") or cur
        rows[cur] = {"mangled": mangled}
        continue
    m3 = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
    if m3 and cur:
        rows[cur][m3.group(1).strip()] = int(m3.group(2))
size = {}
for line in subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "-sW", obj], capture_output=True, text=True).stdout.splitlines():
    f = line.split()
    if len(f) >= 8 and f[3] == "FUNC":
        size[f[7]] = int(f[2], 0)
for k, v in rows.items():
    print("%-60s VGPR %3d AGPR %3d SGPR %3d scratch %5d LDS %6d occupancy %d code %6d" % (
        k, v.get("VGPRs", -1), v.get("AGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1),
        v.get("LDS Size", -1), v.get("Occupancy", -1), size.get(v["mangled"], -1)))
