"""Print per-kernel VGPR/AGPR/SGPR/scratch/occupancy for a HIP source (hipcc -Rpass-analysis, the Makefile's flags).
    python tools/resource_usage.py <file.hip> [extra hipcc flags ...]"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_build  # noqa: E402

for r in device_build.compile_device(sys.argv[1], device_build.hipflags() + sys.argv[2:]).kernels:
    n = re.sub(r"\(.*", "", device_build.demangle(r["name"]).replace("bf::(anonymous namespace)::", "").replace("void ", ""))
    print(f"{n[:90]:90s} V={r.get('VGPRs')} A={r.get('AGPRs')} S={r.get('SGPRs')} scr={r.get('ScratchSize [bytes/lane]')} occ={r.get('Occupancy [waves/SIMD]')}")
