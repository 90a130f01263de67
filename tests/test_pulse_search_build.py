"""Build hygiene of the pulse-search kernels (no GPU), as test_dedisperse_build.py for its sibling: the source is in the
Makefile, the two kernel instances (the filter and the per-beam best; none per shape, none per width list: the widths
travel in the kernel arguments) compile for gfx950 with no scratch (register spills), and the compile emits no
warnings.  Runs hipcc on the source (device code only, the Makefile's flags) with
-Rpass-analysis=kernel-resource-usage."""
import os
import re
import shutil
import subprocess

import pytest

from test_detect_build import HIPCC, ROOT, _usage, makefile_hipflags

SOURCE, INSTANCES = "bf_pulse_search.hip", 2


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc not available")
    _, kernels, warnings = _usage(SOURCE)
    return kernels, warnings


def test_pulse_search_source_is_in_the_makefile():
    srcs = re.search(r"^SRCS\s*:=((?:.*\\\n)*.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1)
    assert "$(CSRC)/bf_pulse_search.hip" in srcs.split()


def test_makefile_flags_are_unchanged():
    """The float64 sqrt and division are compared with NumPy's, bit for bit: no fast-math flag."""
    flags = makefile_hipflags()
    assert flags == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function",
                     "-munsafe-fp-atomics"]


def test_every_kernel_instance_is_reported(usage):
    kernels, _ = usage
    names = [k["name"] for k in kernels]
    assert len(kernels) == INSTANCES, names
    assert sum("pulse_search_kernel" in n for n in names) == 1 and sum("pulse_best_kernel" in n for n in names) == 1


def test_no_scratch(usage):
    kernels, _ = usage
    spills = []
    for k in kernels:
        if int(k.get("ScratchSize [bytes/lane]", "0")) != 0:
            name = subprocess.run(["c++filt"], input=k["name"], capture_output=True, text=True).stdout.strip()
            spills.append(f"{name[:120]} scratch {k['ScratchSize [bytes/lane]']} B/lane, VGPRs {k.get('VGPRs')}")
    assert not spills, "\n".join(spills)


def test_no_compiler_warnings(usage):
    _, warnings = usage
    assert not warnings, "\n".join(warnings[:20])
