"""CPU: the fused beamformer's launch plan (csrc/bf_fused_plan.cpp, asked through bf_fused_plan) -- which kernel a
call takes, with what grid, LDS and workspace -- without a GPU.

  guarded names : every fused case of the guard-band suite (tests/fused_cases.py) is planned onto the kernel it expects
  parent pin    : tests/golden/fused_plan_parent.json holds bf_last_kernel() as recorded on an MI355X from the library
                  before the plan existed (its launchers chose as they went), one real launch per row; the plan names
                  the same kernel for every row
  sweep         : invariants of any plan over a grid of shapes either side of every threshold x every flag combination
  refusals      : bf_beamform_fused_ws still refuses what it refused, in the same words
"""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

import fused_cases as FC
from dpdk_dc_sand_amd import _lib

SIGNED, OUT_I8, EXACT, VIA_F32, PATH, ORDER = FC.SIGNED, FC.OUT_I8, FC.EXACT, FC.VIA_F32, FC.PATH, FC.ORDER
PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_plan_parent.json")


def workspace_bytes(B, C, T, A, M, flags):
    n = ctypes.c_size_t(0)
    _lib.call("bf_fused_workspace_bytes", B, C, T, A, M, flags, ctypes.byref(n))
    return n.value


def test_feature_and_symbol():
    lib = _lib.load()
    assert lib.bf_has_feature(b"fused_plan") == 1 and lib.bf_has_feature(b"fused") == 0


def test_guarded_names():
    calls = FC.all_calls()
    assert len(calls) == 181  # the guarded suite's fused launches
    wrong = [(c, FC.planned_name(c)) for c in calls if FC.planned_name(c) != c.expect]
    assert not wrong, wrong[:5]


def test_parent_pin():
    rows = json.load(open(PIN))
    assert len(rows) >= 200
    wrong = []
    for r in rows:
        got = _lib.fused_plan(r["B"], r["C"], r["T"], r["A"], r["M"], r["dch"], r["gains"], r["flags"], r["scale"],
                              r["workspace_bytes"], cus=r["cus"]).kernel.decode()
        if got != r["name"]:
            wrong.append((r, got))
    assert not wrong, wrong[:5]


# ---- the sweep ----------------------------------------------------------------------------------------------------------
SWEEP_A = [1, 5, 16, 31, 32, 33, 61, 64, 65, 128, 130, 224, 225, 256, 257, 320, 321, 512, 513, 640, 641, 656, 724,
           725, 1024]
SWEEP_M = [1, 3, 8, 9, 12, 16, 20, 24, 32, 33, 40, 64, 65]
SWEEP_T = [16, 48, 256, 272]
SWEEP_C = [3, 8]
MODES = [0, EXACT, OUT_I8, OUT_I8 | VIA_F32]  # float fast / float exact / Q14 / int8 via f32
FLAG_SETS = [(s | m | p | o, g, w) for s in (0, SIGNED) for m in MODES for p in PATH.values() for o in ORDER.values()
             for g in (False, True) for w in (False, True)]  # 2 * 4 * 4 * 3 * 2 * 2 = 384
PER_SHAPE = 16  # flag sets drawn per shape: 2600 shapes x 16 = 41600 plans, every flag set about 108 times
ITEM_FAMILIES = ("beamform_fused_item_kernel", "beamform_fused_i8_item_kernel")
GENERIC_FAMILIES = ("beamform_fused_kernel", "beamform_fused_i8_kernel")
WIDE_FAMILIES = ("beamform_fused_wide_kernel", "beamform_fused_wide_p2_kernel")
W32_FAMILIES = ("beamform_fused_i8_w32_kernel", "beamform_fused_i8_w32t_kernel", "beamform_fused_i8_w32r_kernel")


def check_forced_path(family, flags, A, T):
    """include/bf.h: a forced path is taken when the shape fits it, else the call falls through to one that does."""
    path, q14 = flags & 0x0f00, bool(flags & OUT_I8) and not flags & VIA_F32
    small = A <= 64 and T <= 256
    fallthrough = ITEM_FAMILIES if small else GENERIC_FAMILIES
    if path == PATH["item"]:  # A <= 64, T <= 256, else generic
        assert family in fallthrough
    elif path == PATH["generic"]:
        assert family in GENERIC_FAMILIES
    elif path == PATH["wide"]:
        if q14:  # the 32-beam kernels' limb image fits LDS for 32 <= A <= 512
            assert family in (W32_FAMILIES if 32 <= A <= 512 else fallthrough)
        elif flags & OUT_I8:  # the wide kernels have no requantising form
            assert family in fallthrough
        else:  # 16-beam slabs: 2 KiB of LDS per 16 antennas, A <= 1280; the loads need 16 antennas
            assert family in (WIDE_FAMILIES if A >= 16 else fallthrough)


def test_invariant_sweep():
    rng = np.random.default_rng(2024)
    planned = refused = 0
    seen_flag_sets, families = set(), set()
    for A, M, T, C in itertools.product(SWEEP_A, SWEEP_M, SWEEP_T, SWEEP_C):
        for k in rng.choice(len(FLAG_SETS), PER_SHAPE, replace=False):
            flags, gains, offer = FLAG_SETS[k]
            seen_flag_sets.add(k)
            scale = 1 / 64 if (A + M + k) % 2 else FC.S6
            ws = workspace_bytes(2, C, T, A, M, flags)
            try:
                dch = (1, C)[rng.integers(2)]
                p = _lib.fused_plan(2, C, T, A, M, dch, gains, flags, scale, ws if offer else 0, cus=256)
            except _lib.BeamformerError as e:
                assert e.status == -1 and e.message, (A, M, T, C, hex(flags))
                refused += 1
                # with gains the caller owns the int32 bound: the plan itself must then exist below the LDS limits
                assert "overflows" in e.message or "too large" in e.message
                assert ws == 0
                continue
            planned += 1
            where = (A, M, T, C, hex(flags), gains, offer, p.kernel)
            assert p.lds_bytes <= 160 * 1024, where
            assert 0 < p.grid < 2 ** 31 and p.block in (256, 512), where
            assert not p.xcd_order or p.grid % 8 == 0, where
            assert p.nslabs >= 1, where
            if offer:
                assert (ws > 0) == bool(p.uses_table) and p.workspace_bytes == ws, where
            else:
                assert not p.uses_table and p.workspace_bytes == 0, where
            family = p.kernel.decode().split(":")[0]
            families.add(family)
            check_forced_path(family, flags, A, T)
    assert planned + refused == len(SWEEP_A) * len(SWEEP_M) * len(SWEEP_T) * len(SWEEP_C) * PER_SHAPE
    assert len(seen_flag_sets) == len(FLAG_SETS) and refused > 0
    assert families == set(ITEM_FAMILIES + GENERIC_FAMILIES + WIDE_FAMILIES + W32_FAMILIES)


def test_workspace_offer_below_need_is_declined():
    need = workspace_bytes(1, 2, 256, 256, 64, OUT_I8)
    assert need == 1 * 2 * 2 * 1024 * 8 * 4
    assert _lib.fused_plan(1, 2, 256, 256, 64, flags=OUT_I8, workspace_bytes=need).uses_table == 1
    p = _lib.fused_plan(1, 2, 256, 256, 64, flags=OUT_I8, workspace_bytes=need - 1)
    assert p.uses_table == 0 and p.kernel == b"beamform_fused_i8_w32_kernel:unit"


def test_table_driven_pointer_form_walks_its_own_channel_count():
    """Voltages of 2 GiB per batch at config 4's antennas and samples: the table-driven kernel's pointer form, which
    walks 4 channels per workgroup (8 belong to the straight-line buffer form only): B * ceil(C / 4) groups per slab."""
    B, C, T, A, M = 1, 8192, 256, 256, 64
    ws = workspace_bytes(B, C, T, A, M, OUT_I8)
    p = _lib.fused_plan(B, C, T, A, M, flags=OUT_I8, out_scale=1 / 64, workspace_bytes=ws)
    assert p.kernel == b"beamform_fused_i8_w32t_kernel:general,ptr" and p.nslabs == 2 and p.xcd_order == 1
    assert p.grid == B * (C // 4) * 2
    p = _lib.fused_plan(B, C // 2, T, A, M, flags=OUT_I8, out_scale=1 / 64, workspace_bytes=ws)
    assert p.kernel == b"beamform_fused_i8_w32t_kernel:straight,pow2" and p.grid == B * (C // 2 // 8) * 2


def test_persistent_grid_follows_the_cu_count():
    for cus, ch_run in ((256, 1), (64, 2), (1, 64)):
        p = _lib.fused_plan(1, 64, 256, 256, 64, cus=cus)
        assert p.kernel == b"beamform_fused_wide_p2_kernel" and p.ch_run == ch_run and p.block == 512
        assert p.grid == (64 // ch_run + 7) // 8 * 8 * 2 and p.lds_bytes == 128 * 1024


# ---- refusals of the launch itself: unchanged status and words ----------------------------------------------------
FAKE = 0x10000  # an aligned address that is never dereferenced: each call below is refused before any launch
OVERFLOWS = ("bf_beamform_fused: n_ants={A} overflows the int8 path's int32 beam sums ({kind} samples); use float beams "
             "or BF_FUSED_INT8_VIA_F32")


@pytest.mark.parametrize("A,M,flags,gains,message", [
    (1300, 1, 0, False, "bf_beamform_fused: n_ants=1300 too large"),
    (1300, 1, SIGNED | EXACT | PATH["generic"], False, "bf_beamform_fused: n_ants=1300 too large"),
    (1300, 8, OUT_I8 | VIA_F32, False, "bf_beamform_fused: n_ants=1300 too large"),
    (2600, 3, OUT_I8 | SIGNED, True, "bf_beamform_fused: n_ants=2600 too large"),
    (364, 16, OUT_I8, False, OVERFLOWS.format(A=364, kind="uint8")),
    (725, 16, OUT_I8 | SIGNED, False, OVERFLOWS.format(A=725, kind="int8")),
])
def test_unchanged_refusals(A, M, flags, gains, message):
    with pytest.raises(_lib.BeamformerError) as e:
        _lib.call("bf_beamform_fused_ws", FAKE, FAKE, 1, FAKE if gains else None, FAKE, 1, 2, 32, A, M, 8192, 0, 1e-9,
                  0.0, 0.0, flags, 1.0, None, 0, None)
    assert e.value.status == -1 and e.value.message == message
    with pytest.raises(_lib.BeamformerError) as e:  # and the plan says so beforehand
        _lib.fused_plan(1, 2, 32, A, M, 1, gains, flags)
    assert e.value.message == message


def test_int32_bound_is_the_last_antenna_count_accepted():
    assert _lib.fused_plan(1, 2, 32, 363, 16, flags=OUT_I8).kernel.startswith(b"beamform_fused_i8_w32_kernel")
    assert _lib.fused_plan(1, 2, 32, 724, 16, flags=OUT_I8 | SIGNED).kernel == b"beamform_fused_i8_kernel:nts2"
