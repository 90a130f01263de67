"""Build hygiene of the folder kernel (no GPU), as test_dedisperse_build.py for its sibling: the source is in the
Makefile, the one kernel instance (16-byte and element staging, the lane-group widths and the chunking are run-time
arguments: none per shape, none per phase table) compiles for gfx950 with no scratch (register spills, or the fold
tables of the kernel arguments indexed per lane), and the compile emits no warnings.  Runs hipcc on the source (device
code only, the Makefile's flags) with -Rpass-analysis=kernel-resource-usage."""
import os
import re
import shutil
import subprocess

import pytest

from test_detect_build import HIPCC, ROOT, _usage, makefile_hipflags

SOURCE, INSTANCES = "bf_fold.hip", 1


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc not available")
    _, kernels, warnings = _usage(SOURCE)
    return kernels, warnings


def test_fold_source_is_in_the_makefile():
    srcs = re.search(r"^SRCS\s*:=((?:.*\\\n)*.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1)
    assert "$(CSRC)/bf_fold.hip" in srcs.split()


def test_the_naive_kernel_is_not_in_the_product():
    text = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=((?:.*\\\n)*.*)$", text, re.M).group(1)
    assert "fold_naive" not in srcs and re.search(r"^fold-naive:", text, re.M)


def test_makefile_flags_are_unchanged():
    """The float64 sums are compared with NumPy's: no fast-math flag."""
    flags = makefile_hipflags()
    assert flags == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function",
                     "-munsafe-fp-atomics"]


def test_every_kernel_instance_is_reported(usage):
    kernels, _ = usage
    names = [k["name"] for k in kernels]
    assert len(kernels) == INSTANCES, names
    assert "fold_kernel" in names[0]


def test_no_scratch(usage):
    kernels, _ = usage
    spills = []
    for k in kernels:
        if int(k.get("ScratchSize [bytes/lane]", "0")) != 0:
            name = subprocess.run(["c++filt"], input=k["name"], capture_output=True, text=True).stdout.strip()
            spills.append(f"{name[:120]} scratch {k['ScratchSize [bytes/lane]']} B/lane, VGPRs {k.get('VGPRs')}")
    assert not spills, "\n".join(spills)


def test_no_static_lds(usage):
    """The tile is the dynamic region alone, so its base is 16-byte aligned for the 16-byte staging stores."""
    kernels, _ = usage
    assert int(kernels[0]["LDS Size [bytes/block]"]) == 0


def test_no_compiler_warnings(usage):
    _, warnings = usage
    assert not warnings, "\n".join(warnings[:20])
