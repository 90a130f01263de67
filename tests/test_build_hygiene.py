"""Build hygiene of every product kernel (no GPU).  Each .hip source of the Makefile's SRCS is compiled once for gfx950
(device code only, the Makefile's flags: tools/device_build.py), and its assembly, per-kernel resource usage and
warnings are checked: the kernel instances are the ones KERNELS lists, none uses scratch (register spills), the compile
is silent, and the two gfx950 hazards that corrupted this project's output (tools/store_hazard_check.py) are absent.
A source new to SRCS needs a row in KERNELS and then has all of it."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import device_build  # noqa: E402
import store_hazard_check as shc  # noqa: E402

# source -> its kernel instances: {substring of the kernel's name: instances}, or their number alone.  None per shape
# and none per table anywhere: an instance more is a template instantiated by accident.
KERNELS = {
    "bf_coeff.hip": 8,
    "bf_reorder.hip": 8,
    "bf_beamform.hip": 60,
    "bf_fused.hip": 104,
    "bf_wide.hip": 34,
    "bf_wide_i8.hip": 14,
    "bf_q14table.hip": 2,
    "bf_requant.hip": 1,
    "bf_study.hip": 1,
    "bf_incoherent.hip": 8,
    "bf_detect.hip": 14,
    "bf_vstats.hip": {"vstats_kernel": 2},  # uint8, int8
    "bf_correlate.hip": {"correlate_kernel": 4},  # uint8 / int8, plain / accumulating
    "bf_beam_streams.hip": {"beam_streams_kernel": 3},  # int8, f32, f32 requantised
    "bf_dedisperse.hip": {"append_kernel": 2, "dedisperse_kernel": 1},  # the append in 16-byte and element accesses
    "bf_pulse_search.hip": {"pulse_search_kernel": 1, "pulse_best_kernel": 1},  # the filter and the per-beam best
    "bf_fold.hip": {"fold_kernel": 1},  # staging width, lane-group widths and chunking are run-time arguments
}
per_source = pytest.mark.parametrize("src", list(KERNELS))


@pytest.fixture(scope="module")
def built():
    """{source name: Build}.  device_build's cache is what keeps every later compile_device() call from compiling."""
    if not os.path.exists(device_build.HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc not available")
    paths = device_build.product_sources()
    yield {os.path.basename(p): b for p, b in zip(paths, device_build.compile_all(paths))}
    print(f"\nhipcc runs: {len(device_build.builds)} for {len(paths)} product sources")


def test_every_product_source_has_a_row():
    names = [os.path.basename(p) for p in device_build.product_sources()]
    assert len(set(names)) == len(names) and names
    assert set(KERNELS) == set(names), f"differ in {sorted(set(KERNELS) ^ set(names))}"


def test_makefile_flags_are_unchanged():
    """No fast-math flag, and -munsafe-fp-atomics stays: the float64 sums (fold, dedisperse, with its one float64
    multiply), the float64 sqrt and division (pulse search, voltage statistics) are compared bit for bit with NumPy's
    and rely on the correctly rounded default lowering, and the requantising beam-streams instance is bit-exact
    against NumPy's rint."""
    assert device_build.hipflags() == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function",
                                       "-munsafe-fp-atomics"]


@per_source
def test_every_kernel_instance_is_reported(built, src):
    names = [k["name"] for k in built[src].kernels]
    want = KERNELS[src]
    assert len(names) == (want if isinstance(want, int) else sum(want.values())), names
    if not isinstance(want, int):
        assert {s: sum(s in n for n in names) for s in want} == want, names


@per_source
def test_no_scratch(built, src):
    spills = [f"{device_build.demangle(k['name'])[:120]} scratch {k['ScratchSize [bytes/lane]']} B/lane, "
              f"VGPRs {k.get('VGPRs')}" for k in built[src].kernels if int(k.get("ScratchSize [bytes/lane]", "0")) != 0]
    assert not spills, "\n".join(spills)


@per_source
def test_no_compiler_warnings(built, src):
    assert not built[src].warnings, "\n".join(built[src].warnings[:20])


@per_source
def test_no_wide_store_data_hazard(built, src):
    """No product kernel lets a VALU rewrite a wide store's data VGPRs right behind the store (tools/
    store_hazard_check.py: the gfx950 store-data hazard hipcc left unguarded once, wrong bytes ~1e-5 of the time)."""
    _, hits = shc.scan(built[src].asm, window=2)
    assert not hits, "\n".join(f"{fn[:90]}: {st} / {n}" for fn, st, n, _ in hits[:20])


@per_source
def test_no_inline_asm_result_reaches_an_mfma_unpadded(built, src):
    """An inline-asm VGPR result read by an MFMA within two instructions of the statement needs the statement to end
    in s_nop 1 (hipcc pads one state after an asm statement; VALU write -> MFMA operand read needs 2): the persistent
    float kernel's uint8 form read a stale fragment in one accumulator without it (tools/store_hazard_check.py)."""
    bad = shc.scan_asm_to_mfma(built[src].asm, window=2)
    assert not bad, "\n".join(f"{fn[:90]}: {a} -> +{n} {m}" for fn, a, m, n in bad[:20])


def test_correlate_full_workgroup_fits(built):
    """A workgroup is up to 16 waves, four per SIMD: at most 128 VGPRs; its LDS (two buffers of 8 tiles x 2 pols x
    1 KiB, and the row sums) stays below the 64 KiB of a static allocation."""
    kernels = built["bf_correlate.hip"].kernels
    assert all(int(k["VGPRs"]) + int(k.get("AGPRs", "0")) <= 128 for k in kernels), [k.get("VGPRs") for k in kernels]
    assert all(0 < int(k["LDS Size [bytes/block]"]) <= 65536 for k in kernels)


def test_correlate_runs_on_the_int8_mfma(built):
    assert built["bf_correlate.hip"].asm.count("v_mfma_i32_16x16x64_i8") >= 8 * 4  # 4 Re + 4 Im per K step, instance


def test_correlate_wide_stores_are_scanned(built):
    assert shc.scan(built["bf_correlate.hip"].asm, window=2)[0] > 0  # the 16-byte visibility stores were seen


def test_fold_has_no_static_lds(built):
    """The tile is the dynamic region alone, so its base is 16-byte aligned for the 16-byte staging stores."""
    assert int(built["bf_fold.hip"].kernels[0]["LDS Size [bytes/block]"]) == 0


def test_the_naive_fold_kernel_is_not_in_the_product():
    srcs = device_build.make_vars()["SRCS"]
    assert "fold_naive" not in srcs and re.search(r"^fold-naive:", open(os.path.join(ROOT, "Makefile")).read(), re.M)


def test_lds_dma_ring_slot_reads_wait_for_their_dma(built):
    """the config-4 int8 kernel's voltage ring (w32r) relies on hipcc's vmcnt bookkeeping for its LDS-DMA
    slots.  Replaying the vector-memory queue of its main loop in issue order (tools/store_hazard_check.py
    scan_lds_dma_ring), every slot read finds at most the next step's 4 DMA pieces outstanding -- the DMA that wrote
    the slot being read has retired -- in both instances."""
    asm = built["bf_wide_i8.hip"].asm
    kernels = sorted(set(re.findall(r"^(_Z\w*beamform_fused_i8_w32r_kernel\w*):", asm, flags=re.M)))
    assert len(kernels) == 2, kernels
    for k in kernels:
        checked, bad = shc.scan_lds_dma_ring(asm, k, depth=2)
        assert checked == 64, (k, checked)  # 16 steps x 4 two-row reads per channel
        assert not bad, (k, bad[:8])


def test_store_hazard_scanner_counts_nop_wait_states():
    """The scanner's window is wait states, not instructions: `s_nop 0` is one state (a VALU right after it still
    hits a 2-state window), `s_nop 1` two."""
    head = "_Zk:\n  buffer_store_dwordx4 v[80:83], v1, s[0:3], 0 offen\n"
    assert len(shc.scan(head + "  s_nop 0\n  v_add_u32 v83, v1, v2\n")[1]) == 1
    assert len(shc.scan(head + "  s_nop 1\n  v_add_u32 v83, v1, v2\n")[1]) == 0
    assert len(shc.scan(head + "  s_nop 0\n  s_nop 0\n  v_add_u32 v83, v1, v2\n")[1]) == 0
    assert len(shc.scan(head + "  v_add_u32 v9, v1, v2\n  v_add_u32 v83, v1, v2\n")[1]) == 1
    assert len(shc.scan(head + "  v_add_u32 v9, v1, v2\n  s_nop 0\n  v_add_u32 v83, v1, v2\n")[1]) == 0
    assert len(shc.scan(head + "  v_add_u32 v84, v1, v2\n")[1]) == 0
    assert shc.nop_states("s_nop 0x3") == 4


def test_lds_dma_ring_check_flags_an_early_read():
    """The replay itself: a slot read issued while its own DMA is still counted is flagged; after the right
    s_waitcnt it is not."""
    body = ["_Zk:", ".LBB0_1:",
            "buffer_load_dwordx4 v1, s[0:3], s4 offen lds"] * 1 + \
        ["buffer_load_dwordx4 v1, s[0:3], s4 offen lds"] * 3 + \
        ["{wait}", "ds_read2st64_b64 v[2:5], v6 offset1:1", "s_cbranch_scc1 .LBB0_1", ".Lfunc_end0:"]
    early = "\n".join(body).replace("{wait}", "s_waitcnt vmcnt(8)")
    ok = "\n".join(body).replace("{wait}", "s_waitcnt vmcnt(4)")
    assert shc.scan_lds_dma_ring(early, "_Zk", depth=2)[1]
    assert shc.scan_lds_dma_ring(ok, "_Zk", depth=2) == (1, [])
