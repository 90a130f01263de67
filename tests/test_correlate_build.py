"""Build hygiene of the correlator kernel (no GPU), as test_vstats_build.py for its sibling: the source is in the
Makefile, all four kernel instances (uint8 / int8, plain / accumulating) compile for gfx950 with no scratch (register
spills), the compile emits no warnings, and the two hazards that bit this project's MFMA kernels (a VALU rewriting a
wide store's data right behind the store, an inline-asm result reaching an MFMA unpadded: tools/store_hazard_check.py)
are absent from its ISA."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from test_detect_build import CSRC, HIPCC, ROOT, _usage

SOURCE, INSTANCES = "bf_correlate.hip", 4


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc not available")
    _, kernels, warnings = _usage(SOURCE)
    return kernels, warnings


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import store_hazard_check as shc
    return shc, shc.compile_isa(os.path.join(CSRC, SOURCE))


def test_correlate_source_is_in_the_makefile():
    srcs = re.search(r"^SRCS\s*:=((?:.*\\\n)*.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1)
    assert "$(CSRC)/bf_correlate.hip" in srcs.split()


def test_every_kernel_instance_is_reported(usage):
    kernels, _ = usage
    assert len(kernels) == INSTANCES, [k["name"] for k in kernels]
    assert all("correlate_kernel" in k["name"] for k in kernels)


def test_no_scratch(usage):
    kernels, _ = usage
    spills = []
    for k in kernels:
        if int(k.get("ScratchSize [bytes/lane]", "0")) != 0:
            name = subprocess.run(["c++filt"], input=k["name"], capture_output=True, text=True).stdout.strip()
            spills.append(f"{name[:120]} scratch {k['ScratchSize [bytes/lane]']} B/lane, VGPRs {k.get('VGPRs')}")
    assert not spills, "\n".join(spills)


def test_a_full_workgroup_fits(usage):
    """A workgroup is up to 16 waves, four per SIMD: at most 128 VGPRs; its LDS (two buffers of 8 tiles x 2 pols x
    1 KiB, and the row sums) stays below the 64 KiB of a static allocation."""
    kernels, _ = usage
    assert all(int(k["VGPRs"]) + int(k.get("AGPRs", "0")) <= 128 for k in kernels), [k.get("VGPRs") for k in kernels]
    assert all(0 < int(k["LDS Size [bytes/block]"]) <= 65536 for k in kernels)


def test_no_compiler_warnings(usage):
    _, warnings = usage
    assert not warnings, "\n".join(warnings[:20])


def test_the_kernel_runs_on_the_int8_mfma(isa):
    _, asm = isa
    assert asm.count("v_mfma_i32_16x16x64_i8") >= 8 * INSTANCES  # 4 Re + 4 Im per K step and instance


def test_no_wide_store_data_hazard(isa):
    shc, asm = isa
    total, hits = shc.scan(asm, window=2)
    assert total > 0  # the 16-byte visibility stores were seen
    assert not hits, "\n".join(f"{fn[:90]}: {st} / {n}" for fn, st, n, _ in hits[:20])


def test_no_inline_asm_result_reaches_an_mfma_unpadded(isa):
    shc, asm = isa
    bad = shc.scan_asm_to_mfma(asm, window=2)
    assert not bad, "\n".join(f"{fn[:90]}: {a} -> +{n} {m}" for fn, a, m, n in bad[:20])
