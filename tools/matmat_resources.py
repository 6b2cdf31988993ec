#!/usr/bin/env python3
"""The compiler's resource report for every instantiation of the multi-vector kernels (sigma_amd/csrc/sgm_matmat.hip):
compiles that file with -Rpass-analysis=kernel-resource-usage (needs hipcc, no GPU) and prints one line per kernel.

    python tools/matmat_resources.py > profiles/matmat/resource_usage.txt
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "sigma_amd", "csrc", "sgm_matmat.hip")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-I/opt/rocm/include",
         "-Rpass-analysis=kernel-resource-usage"]
NAME = re.compile(r"k_mm_(sl32|slb|sl)ILi(\d+)ELi(\d+)ELb([01])E")
FIELD = re.compile(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass")


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc] + FLAGS + ["-c", SRC, "-o", os.path.join(tmp, "mm.o")], cwd=os.path.dirname(SRC),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout)
        return 1
    rows, cur = [], None
    for line in p.stdout.splitlines():
        if "Function Name:" in line:
            m = NAME.search(line)
            cur = {"form": "k_mm_" + m.group(1), "W": int(m.group(2)), "KB": int(m.group(3)), "ADD": int(m.group(4))} if m else None
            if cur:
                rows.append(cur)
            continue
        m = FIELD.search(line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    rows.sort(key=lambda r: (r["form"], r["KB"], r["W"], r["ADD"]))
    print("# hipcc " + " ".join(FLAGS) + " -c sigma_amd/csrc/sgm_matmat.hip")
    print(f"# {len(rows)} kernels; scratch in bytes per lane, occupancy in waves per SIMD, LDS in bytes per workgroup")
    print(f"{'kernel':<34} {'VGPRs':>5} {'AGPRs':>5} {'SGPRs':>5} {'scratch':>7} {'vspill':>6} {'sspill':>6} {'occupancy':>9} {'LDS':>5}")
    for r in rows:
        name = f"{r['form']}<W={r['W']},KB={r['KB']},ADD={r['ADD']}>"
        print(f"{name:<34} {r['VGPRs']:>5} {r['AGPRs']:>5} {r['TotalSGPRs']:>5} {r['ScratchSize [bytes/lane]']:>7} "
              f"{r['VGPRs Spill']:>6} {r['SGPRs Spill']:>6} {r['Occupancy [waves/SIMD]']:>9} {r['LDS Size [bytes/block]']:>5}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
