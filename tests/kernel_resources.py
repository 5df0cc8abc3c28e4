"""Register, spill, scratch and LDS figures of the kernels of one translation unit, compiled for gfx950 (the CPU resource tests)."""
import os
import re
import subprocess


def kernel_resources(src, workdir):
    """{kernel symbol: (vgpr, vgpr spills, sgpr, sgpr spills, scratch bytes, LDS bytes)} of one translation unit, from the code object's notes"""
    co, elf = os.path.join(workdir, os.path.basename(src) + ".co"), os.path.join(workdir, os.path.basename(src) + ".elf")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "--cuda-device-only", "-c",
                    "-o", co, src], check=True)
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + co,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf], check=True)
    notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", elf], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("  - .agpr_count")[1:]:
        def field(k):
            m = re.search(r"\.%s:\s+(\S+)" % k, block)
            return m.group(1) if m else None
        out[field("name")] = tuple(int(field(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count",
                                                           "private_segment_fixed_size", "group_segment_fixed_size"))
    return out
