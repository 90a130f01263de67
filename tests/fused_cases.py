"""The bf_beamform_fused_ws cases of the guard-band suite as data: shape, flags, scale, gains, workspace and the kernel
name each call must report.  tests/test_gpu_guarded.py runs them on the GPU; tests/test_fused_plan_host.py asks
bf_fused_plan for the same names without one.  A case function turns one point of its test's parameter grid into the
calls that test makes; GRIDS lists every function with its grid, so both files walk the same set.  Shapes are the
smallest that reach a variant; where a name disagrees, the shape (or the planner) is what is wrong."""
import itertools
from collections import namedtuple

import numpy as np

from dpdk_dc_sand_amd import _lib

SIGNED, OUT_I8, EXACT, VIA_F32 = _lib.FUSED_SIGNED, _lib.FUSED_OUT_INT8, _lib.FUSED_EXACT_COEFF, _lib.FUSED_INT8_VIA_F32
PATH, ORDER = _lib.FUSED_PATH, _lib.FUSED_ORDER
S6 = float(np.float32(1 / 6))  # a scale that is no power of two
BOOLS = [False, True]

# gains: seed of the weight table (None: no gains).  amp bounds |x| (so a large output scale does not saturate every
# beam).  requant_of_previous: the oracle is bf_requant of the previous call's float beams.
Call = namedtuple("Call", "A M T B C flags expect dch gains scale workspace amp requant_of_previous",
                  defaults=(1, None, 1.0, False, None, False))

# ---- float beams ------------------------------------------------------------------------------------------------------
ITEM, GEN, WIDE = "beamform_fused_item_kernel:f32,", "beamform_fused_kernel:f32,", "beamform_fused_wide_kernel:"
F32_CASES = [  # (A, M, T), path, expected name ({e} = exact | fast)
    ((19, 16, 48), "auto", ITEM + "nts2,full,{e},staged"), ((64, 16, 256), "auto", ITEM + "nts2,full,{e},staged"),
    ((40, 32, 64), "auto", ITEM + "nts2,full,{e}"),
    ((33, 9, 80), "auto", ITEM + "nts2,partial,{e}"), ((48, 24, 32), "auto", ITEM + "nts2,partial,{e}"),
    ((16, 8, 48), "auto", ITEM + "nts1,full,{e}"),
    ((5, 3, 16), "auto", ITEM + "nts1,partial,{e}"), ((64, 1, 256), "auto", ITEM + "nts1,partial,{e}"),
    ((130, 9, 64), "auto", GEN + "nts2,{e}"),
    ((80, 2, 16), "auto", GEN + "nts1,{e}"), ((4, 1, 272), "auto", GEN + "nts1,{e}"),
    ((16, 3, 32), "wide", WIDE + "tw1,{e},unit,buf"), ((656, 20, 32), "wide", WIDE + "tw1,{e},unit,buf"),
]


def f32(case, signed, exact):
    (A, M, T), path, expect = case
    flags = (SIGNED if signed else 0) | (EXACT if exact else 0) | PATH[path]
    return [Call(A, M, T, 2, 3, flags, expect.format(e="exact" if exact else "fast"), dch=1 if A % 2 else 3)]


F32_WIDE_SHAPES = [(72, 33, 64), (200, 40, 96)]


def f32_wide_32_beam_slabs(shape, signed, exact, weighted):
    A, M, T = shape
    flags = (SIGNED if signed else 0) | (EXACT if exact else 0)
    name = f"{WIDE}tw2,{'exact' if exact else 'fast'},{'gain' if weighted else 'unit'},buf"
    return [Call(A, M, T, 2, 3, flags, name, dch=3, gains=A if weighted else None)]


def f32_item_kernel_with_gains():
    return [Call(33, 9, 80, 2, 3, SIGNED, ITEM + "nts2,partial,fast", gains=1),
            Call(656, 20, 32, 1, 2, PATH["wide"], WIDE + "tw1,fast,gain,buf", gains=2),
            Call(16, 3, 32, 2, 3, PATH["wide"] | EXACT, WIDE + "tw1,exact,gain,buf", gains=3)]


def f32_persistent_wide_p2_and_its_refusal(C, signed):
    s = SIGNED if signed else 0
    calls = [Call(256, 32, 256, 1, C, s, "beamform_fused_wide_p2_kernel"),
             Call(256, 32, 256, 1, C, s | ORDER["channel"], WIDE + "tw2,fast,unit,buf")]
    if C == 2:
        calls.append(Call(256, 32, 256, 1, C, s | EXACT, WIDE + "tw2,exact,unit,buf"))
    return calls


# ---- int8 beams, the Q14 integer contract ---------------------------------------------------------------------------
I8ITEM = "beamform_fused_i8_item_kernel:"
I8_FORM = {1: "nts1,partial", 8: "nts1,full", 12: "nts2,partial", 16: "nts2,full"}
I8_ITEM_SCALES = [1 / 64, S6]


def i8_item_kernel(M, A, scale):
    k = [1, 8, 12, 16].index(M) + (A == 61) + 2 * (scale != 1 / 64)
    T, signed = (16, 144, 256)[k % 3], k % 2 == 0
    name = f"{I8ITEM}{I8_FORM[M]},{'a64' if A == 64 else 'aany'},{'pow2' if scale == 1 / 64 else 'anyscale'}"
    return [Call(A, M, T, 2, 3, OUT_I8 | (SIGNED if signed else 0), name, scale=scale,
                 amp=None if scale == 1 / 64 else 6)]


I8_GENERIC_CASES = [((130, 9, 64), "nts2"), ((19, 3, 48), "nts1")]


def i8_generic_kernel(case, signed):
    (A, M, T), name = case
    return [Call(A, M, T, 2, 3, OUT_I8 | (SIGNED if signed else 0) | PATH["generic"],
                 "beamform_fused_i8_kernel:" + name, scale=1 / 64, dch=3)]


I8_W32_SHAPES = [(40, 32, 64), (72, 33, 64), (200, 40, 96)]


def i8_w32_in_kernel_phasors(shape, signed, weighted):
    A, M, T = shape
    return [Call(A, M, T, 2, 3, OUT_I8 | (SIGNED if signed else 0) | PATH["wide"],
                 "beamform_fused_i8_w32_kernel:" + ("gain" if weighted else "unit"), scale=1 / 128,
                 gains=M if weighted else None, dch=3)]


W32T, W32R = "beamform_fused_i8_w32t_kernel:", "beamform_fused_i8_w32r_kernel:"
I8_WORKSPACE_CASES = [  # A, M, T, B, C, signed, scale, name
    (64, 40, 64, 2, 3, False, 1 / 64, W32T + "general,buf"), (64, 40, 64, 2, 3, True, S6 / 8, W32T + "general,buf"),
    (256, 64, 256, 1, 2, False, 1 / 256, W32T + "straight,pow2"),
    (256, 64, 256, 1, 2, False, S6 / 32, W32T + "straight,anyscale"),
    (256, 40, 256, 1, 2, True, 1 / 128, W32T + "straight,pow2"),
    (256, 40, 256, 1, 2, True, S6 / 16, W32T + "straight,anyscale"),
    (256, 32, 256, 1, 2, True, 1 / 128, W32R + "pow2"), (256, 32, 256, 1, 5, True, 1 / 128, W32R + "pow2"),
    (256, 32, 256, 1, 2, True, S6 / 16, W32R + "anyscale"), (256, 32, 256, 1, 5, True, S6 / 16, W32R + "anyscale")]


def i8_with_guarded_workspace(case, weighted):
    A, M, T, B, C, signed, scale, name = case
    return [Call(A, M, T, B, C, OUT_I8 | (SIGNED if signed else 0) | PATH["wide"], name, scale=scale, workspace=True,
                 gains=A + M if weighted else None)]


VIA_F32_CASES = [  # A, M, T, form
    (64, 16, 256, "item:nts2,full"), (33, 9, 80, "item:nts2,partial"), (16, 8, 48, "item:nts1,full"),
    (5, 3, 16, "item:nts1,partial"), (130, 9, 64, "generic:nts2"), (80, 2, 16, "generic:nts1")]
VIA_F32_SCALES = [1 / 64, S6 / 8]


def i8_via_f32(case, scale, exact):
    A, M, T, form = case
    kind, nts = form.split(":")
    e = "exact" if exact else "fast"
    flags = SIGNED | (EXACT if exact else 0)
    if kind == "item":
        f32_name = f"{ITEM}{nts},{e}" + (",staged" if M == 16 else "")
        name = f"beamform_fused_item_kernel:i8,{nts},{e},{'pow2' if scale == 1 / 64 else 'anyscale'}"
    else:
        f32_name, name = f"{GEN}{nts},{e}", f"beamform_fused_kernel:i8,{nts},{e}"
    return [Call(A, M, T, 2, 3, flags, f32_name),
            Call(A, M, T, 2, 3, flags | OUT_I8 | VIA_F32, name, scale=scale, requant_of_previous=True)]


# every case function with the parameter grid of its test (argument order = the function's)
GRIDS = [
    (f32, [F32_CASES, BOOLS, BOOLS]),
    (f32_wide_32_beam_slabs, [F32_WIDE_SHAPES, BOOLS, BOOLS, BOOLS]),
    (f32_item_kernel_with_gains, []),
    (f32_persistent_wide_p2_and_its_refusal, [[2, 3], BOOLS]),
    (i8_item_kernel, [[1, 8, 12, 16], [64, 61], I8_ITEM_SCALES]),
    (i8_generic_kernel, [I8_GENERIC_CASES, BOOLS]),
    (i8_w32_in_kernel_phasors, [I8_W32_SHAPES, BOOLS, BOOLS]),
    (i8_with_guarded_workspace, [I8_WORKSPACE_CASES, BOOLS]),
    (i8_via_f32, [VIA_F32_CASES, VIA_F32_SCALES, BOOLS]),
]


def all_calls():
    """Every fused call of the guarded suite, in order."""
    return [c for fn, grid in GRIDS for point in itertools.product(*grid) for c in fn(*point)]


def workspace_bytes(c):
    """What the call offers: exactly bf_fused_workspace_bytes when the case has a workspace."""
    import ctypes
    n = ctypes.c_size_t(0)
    if c.workspace:
        _lib.call("bf_fused_workspace_bytes", c.B, c.C, c.T, c.A, c.M, c.flags, ctypes.byref(n))
    return n.value


def planned_name(c):
    """The kernel bf_fused_plan names for the call."""
    return _lib.fused_plan(c.B, c.C, c.T, c.A, c.M, c.dch, c.gains is not None, c.flags, c.scale,
                           workspace_bytes(c)).kernel.decode()
