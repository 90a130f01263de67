"""Build hygiene of the beam-streams kernel (no GPU), as test_vstats_build.py for its sibling: the source is in the
Makefile, the three kernel instances (int8, f32, f32 requantised; none per M, none per list) compile for gfx950 with no
scratch (register spills), and the compile emits no warnings.  Runs hipcc on the source (device code only, the
Makefile's flags) with -Rpass-analysis=kernel-resource-usage."""
import os
import re
import shutil
import subprocess

import pytest

from test_detect_build import HIPCC, ROOT, _usage, makefile_hipflags

SOURCE, INSTANCES = "bf_beam_streams.hip", 3


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc not available")
    _, kernels, warnings = _usage(SOURCE)
    return kernels, warnings


def test_beam_streams_source_is_in_the_makefile():
    srcs = re.search(r"^SRCS\s*:=((?:.*\\\n)*.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1)
    assert "$(CSRC)/bf_beam_streams.hip" in srcs.split()


def test_makefile_flags_are_unchanged():
    """The requantising instance is bit-exact against NumPy's rint: no fast-math flag; -munsafe-fp-atomics stays."""
    flags = makefile_hipflags()
    assert "-munsafe-fp-atomics" in flags
    assert not [f for f in flags if "fast" in f or "finite-math" in f or "reciprocal" in f]


def test_every_kernel_instance_is_reported(usage):
    kernels, _ = usage
    assert len(kernels) == INSTANCES, [k["name"] for k in kernels]
    assert all("beam_streams_kernel" in k["name"] for k in kernels)


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
