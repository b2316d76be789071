#!/usr/bin/env python3
"""Registers, scratch (spills), LDS and occupancy of every kernel instantiation, from hipcc's own remarks
(-Rpass-analysis=kernel-resource-usage) on one kernel translation unit; build container, no GPU.
python tools/kernel_resources.py [filter]     NS=exact (default) | fast: csrc/kernels.hip for that namespace;  NS=plain: csrc/kernels_plain.hip;  NS=sa: csrc/kernels_sa.hip;  NS=wall_heat: csrc/kernels_wall_heat.hip;  NS=face_gradient: csrc/kernels_face_gradient.hip;  NS=statistics: csrc/kernels_statistics.hip"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc")
flt = sys.argv[1] if len(sys.argv) > 1 else ""
NS = os.environ.get("NS", "exact")             # NS=fast: the contracted namespace (with its order-free kernels); NS=plain: the single-flavour kernels
NSFLAGS = {"exact": ["-ffp-contract=off", "-DMGCFD_KERNEL_NS=exact"], "fast": ["-ffp-contract=fast", "-DMGCFD_KERNEL_NS=fast", "-DMGCFD_ORDER_FREE=1"],
           "plain": ["-ffp-contract=off"], "sa": ["-ffp-contract=off"], "wall_heat": ["-ffp-contract=off"], "face_gradient": ["-ffp-contract=off"],
           "statistics": ["-ffp-contract=off"]}[NS]
SRC = {"plain": "kernels_plain.hip", "sa": "kernels_sa.hip", "wall_heat": "kernels_wall_heat.hip", "face_gradient": "kernels_face_gradient.hip",
       "statistics": "kernels_statistics.hip"}.get(NS, "kernels.hip")
r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-Wno-unused-result",
                    "-mllvm", "-amdgpu-kernarg-preload-count=16"] + NSFLAGS + [f"-I{ROOT}/include", f"-I{CS}",
                    "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CS, SRC), "-o", "/tmp/kernel_resources.o"],
                   capture_output=True, text=True)
blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)
names = [b.split("\n")[0].strip() for b in blocks[1:]]
dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
print("VGPR SGPR scratch occ    LDS  kernel")
for b, d in zip(blocks[1:], dem):
    g = lambda k: int(m.group(1)) if (m := re.search(k + r": (\d+)", b)) else -1
    if flt in d:
        sc, occ, lds = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")
        print(f"{g('VGPRs'):4d} {g('SGPRs'):4d} {sc:7d} {occ:3d} {lds:6d}  {d[:150]}")
