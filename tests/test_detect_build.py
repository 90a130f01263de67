"""Build hygiene of the detector and incoherent-beam kernels (no GPU), as test_resource_usage.py for the older sources:
every kernel instance compiles for gfx950 with no scratch (register spills) and the compile emits no warnings.  Runs
hipcc on the two sources (device code only, the Makefile's flags) with -Rpass-analysis=kernel-resource-usage."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpdk_dc_sand_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SOURCES = {"bf_detect.hip": 14, "bf_incoherent.hip": 8}  # source -> kernel instances


def makefile_hipflags():
    text = open(os.path.join(ROOT, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert "--offload-arch=gfx950" in flags and "-Wall" in flags
    return [f for f in flags if f != "-fPIC"]


def _usage(src):
    cmd = [HIPCC] + makefile_hipflags() + ["-x", "hip", "--cuda-device-only", "-c", os.path.join(CSRC, src), "-o",
                                           os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            kernels.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return src, kernels, [ln for ln in r.stderr.splitlines() if "warning:" in ln]


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc not available")
    with ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        return {src: (k, w) for src, k, w in ex.map(_usage, SOURCES)}


def test_detect_source_is_in_the_makefile():
    srcs = re.search(r"^SRCS\s*:=((?:.*\\\n)*.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1)
    assert "$(CSRC)/bf_detect.hip" in srcs.split()


def test_every_kernel_instance_is_reported(usage):
    for src, n in SOURCES.items():
        assert len(usage[src][0]) == n, (src, [k["name"] for k in usage[src][0]])


def test_no_scratch(usage):
    spills = []
    for src, (kernels, _) in usage.items():
        for k in kernels:
            if int(k.get("ScratchSize [bytes/lane]", "0")) != 0:
                name = subprocess.run(["c++filt"], input=k["name"], capture_output=True, text=True).stdout.strip()
                spills.append(f"{src}: {name[:120]} scratch {k['ScratchSize [bytes/lane]']} B/lane, "
                              f"VGPRs {k.get('VGPRs')}")
    assert not spills, "\n".join(spills)


def test_no_compiler_warnings(usage):
    warnings = [w for _, (_, ws) in usage.items() for w in ws]
    assert not warnings, "\n".join(warnings[:20])
