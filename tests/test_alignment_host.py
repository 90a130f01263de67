"""include/bf.h's pointer-alignment table against the host checks: every pointer of every compute entry point, offset by
less than its requirement, is refused with BF_ERR_ARG before anything is launched (no GPU: the pointers are never
dereferenced), and the header states exactly the alignments refused here."""
import os
import re

import pytest

from dpdk_dc_sand_amd import _lib

FAKE = 1 << 20  # 1 MiB: aligned for everything, never dereferenced
TS = 1 / 1712e6

# entry point -> (arguments with every pointer at FAKE, {argument index: (name in the header, required alignment)})
CALLS = {
    "bf_coeff_gen": ([FAKE, FAKE, 1, 2, 2, 64, 4, 3, 0, TS, None], {0: ("delay_vals", 16), 1: ("out", 8)}),
    "bf_coeff_gen_time": ([FAKE, 1, FAKE, 0, 2, 2, 64, 4, 3, 0, TS, 0.0, 1e-3, None],
                          {0: ("delay_vals", 16), 2: ("out", 8)}),
    "bf_coeff_gen_time/f16": ([FAKE, 1, FAKE, 1, 2, 2, 64, 4, 3, 0, TS, 0.0, 1e-3, None], {2: ("out", 4)}),
    "bf_coeff_gen_time_study": ([FAKE, FAKE, 0, 2, 2, 4, 3, 1e-7, 8192, None], {0: ("delay_vals", 16), 1: ("out", 8)}),
    "bf_coeff_gen_time_study/f16": ([FAKE, FAKE, 1, 2, 2, 4, 3, 1e-7, 8192, None], {1: ("out", 4)}),
    "bf_beamform_study_single_channel": ([FAKE, FAKE, FAKE, 2, 32, 4, 3, 1e-7, 8192, None],
                                         {0: ("delay_vals", 16), 1: ("x", 4), 2: ("out", 8)}),
    "bf_reorder": ([FAKE, FAKE, 1, 4, 2, 16, None], {0: ("in", 16), 1: ("out", 16)}),
    "bf_beamform": ([FAKE, FAKE, FAKE, 1, 2, 1, 1, 4, 3, 0, None], {0: ("x", 8), 1: ("w", 4), 2: ("y", 16)}),
    "bf_beamform_fused_ws": ([FAKE, FAKE, 1, FAKE, FAKE, 1, 2, 16, 4, 3, 64, 0, TS, 0.0, 0.0, 0, 1.0, FAKE, 1 << 20,
                              None],
                             {0: ("raw", 16), 1: ("delay_vals", 16), 3: ("gains", 4), 4: ("y", 16),
                              17: ("workspace", 16)}),
    "bf_beamform_fused_weighted": ([FAKE, FAKE, 1, FAKE, FAKE, 1, 2, 16, 4, 3, 64, 0, TS, 0.0, 0.0, 0, 1.0, None],
                                   {0: ("raw", 16), 1: ("delay_vals", 16), 3: ("gains", 4), 4: ("y", 16)}),
    "bf_beamform_fused": ([FAKE, FAKE, 1, FAKE, 1, 2, 16, 4, 3, 64, 0, TS, 0.0, 0.0, 0, 1.0, None],
                          {0: ("raw", 16), 1: ("delay_vals", 16), 3: ("y", 16)}),
    "bf_q14_coeffs": ([FAKE, 1, FAKE, FAKE, 1, 2, 4, 3, 64, 0, TS, 0.0, 0.0, None],
                      {0: ("delay_vals", 16), 2: ("gains", 4), 3: ("out", 4)}),
    "bf_requant": ([FAKE, FAKE, 16, 1.0, None], {0: ("y", 16), 1: ("q", 4)}),
    "bf_incoherent_beam": ([FAKE, FAKE, FAKE, 1, 2, 16, 4, 16, 0, 1.0, None], {0: ("raw", 16), 2: ("out", 4)}),
    "bf_beam_detect": ([FAKE, FAKE, 1, 2, 16, 3, 16, 1, 0, 1.0, None], {0: ("beams", 16), 1: ("out", 4)}),
    "bf_voltage_stats": ([FAKE, FAKE, FAKE, FAKE, 1, 2, 16, 4, 16, 0, 1.0, 0.5, 2.0, None],
                         {0: ("raw", 16), 1: ("out_power", 4), 2: ("out_sk", 4)}),
    "bf_fill_random": ([FAKE, 40, 1, None], {0: ("dst", 16)}),
}
CASES = [(key, i) for key, (_, ptrs) in CALLS.items() for i in ptrs]


@pytest.mark.parametrize("key,index", CASES, ids=[f"{k}-{CALLS[k][1][i][0]}" for k, i in CASES])
def test_pointer_below_its_alignment_is_refused(key, index):
    args, ptrs = CALLS[key]
    need = ptrs[index][1]
    lib = _lib.load()
    before = lib.bf_last_kernel()
    for off in sorted({need // 2, 1}):  # the largest legal-looking offset below the requirement, and an odd one
        bad = list(args)
        bad[index] = FAKE + off
        with pytest.raises(_lib.BeamformerError, match="misaligned|aligned") as e:
            _lib.call(key.split("/")[0], *bad)
        assert e.value.status == -1  # BF_ERR_ARG
    assert lib.bf_last_kernel() == before  # refused before any launch


def test_header_states_the_enforced_alignments():
    """The header's table, row by row: `name  ptr N, ptr N (...)` must list every pointer above with its number."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bf.h")).read()
    table = text[text.index("/* Pointer alignment."):]
    table = table[:table.index("*/")]
    rows = {}
    for line in table.splitlines():
        m = re.match(r"\s*\*\s+(bf_\w+\*?)\s{2,}(.*)", line)
        if m:
            rows[m.group(1)] = {n: int(v) for n, v in re.findall(r"(\w+) (\d+)", m.group(2))}
    for key, (_, ptrs) in CALLS.items():
        name = key.split("/")[0]
        row = rows["bf_beamform_fused*"] if name.startswith("bf_beamform_fused") else rows[name]
        for pname, need in ptrs.values():
            if key.endswith("/f16"):
                assert re.search(r"out 8 \(float2\) or 4 \(half2", table), key
            else:
                assert row.get(pname) == need, (key, pname, need, row)
