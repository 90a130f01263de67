"""GPU: every kernel variant of the C ABI writes all and only its output (the guard-band harness, tests/guarded.py).

Each case places every device buffer at its minimum legal alignment between two 64 KiB guards, launches twice over
different fills, and demands: identical output bits in both runs, the case's oracle met, guards and inputs untouched,
and -- through bf_last_kernel -- that the kernel variant the case claims to cover is the one that ran.  The expected
names are written out per case; where a name disagrees, the shape is what is wrong.  The fused cases live in
tests/fused_cases.py: tests/test_fused_plan_host.py holds the host-side launch plan (bf_fused_plan) to the same names
without a GPU, and every fused call here checks that the plan named the kernel that ran.  Shapes are the smallest that
reach a variant.  The >= 2 GiB pointer-form variants (wide `ptr`, w32t `general,ptr`) belong to
tests/test_gpu_fullsize.py."""
import ctypes

import numpy as np
import pytest

import detect_ref
import fused_cases as FC
import guarded as gd
import incoherent_ref
import oracle as O
import vstats_ref
from dpdk_dc_sand_amd import _lib
from tolerance import assert_beams_allclose

pytestmark = pytest.mark.gpu
TS = O.TS_MEERKAT
CTOT, XENG, T0 = 8192, 3, 2.5e-3
BDT = 256 * 8192 * TS
SIGNED, OUT_I8, VIA_F32, S6 = FC.SIGNED, FC.OUT_I8, FC.VIA_F32, FC.S6


@pytest.fixture(scope="module")
def ex(context, command_queue):
    return gd.DeviceExecutor(context, command_queue)


def delays(dch, M, A, seed):
    rng = np.random.default_rng(seed)
    d = np.zeros((dch, M, A, 4), np.float32)
    d[..., 0] = rng.uniform(0, 10 * TS, (dch, M, A))
    d[..., 1] = rng.uniform(-1e-9, 1e-9, (dch, M, A))
    d[..., 2] = rng.uniform(-np.pi, np.pi, (dch, M, A))
    d[..., 3] = rng.uniform(-1.0, 1.0, (dch, M, A))
    return d


def voltages(shape, signed, seed, amp=None):
    """8-bit cube; `amp` bounds |x| (so a large output scale does not saturate every beam)."""
    rng = np.random.default_rng(seed)
    if amp is None:
        raw = rng.integers(0, 256, shape, dtype=np.uint8)
    elif signed:
        raw = rng.integers(-amp, amp, shape).astype(np.int8).view(np.uint8)
    else:
        raw = rng.integers(0, 2 * amp, shape).astype(np.uint8)
    return raw


def unit_gains(M, A, seed):
    return np.random.default_rng(seed).uniform(0.25, 1.0, (M, A)).astype(np.float32)


def fused(ex, c, f32_of=None):
    """One guarded bf_beamform_fused_ws call (a fused_cases.Call) against the oracle of its contract.  Returns the beams."""
    A, M, T, B, C, flags, dch, scale = c.A, c.M, c.T, c.B, c.C, c.flags, c.dch, c.scale
    signed, i8 = bool(flags & SIGNED), bool(flags & OUT_I8)
    raw = voltages((B, A, C, T, 2, 2), signed, A * 131 + M * 7 + T + C, c.amp)
    d = delays(dch, M, A, A * 31 + M)
    gains = None if c.gains is None else unit_gains(M, A, c.gains)
    rawv = raw.view(np.int8) if signed else raw
    bufs = [gd.inp("raw", raw, 16), gd.inp("dv", d, 16),
            gd.out("y", (B, 2, C, T // 16, 16, 2 * M), np.int8 if i8 else np.float32, 16)]
    if gains is not None:
        bufs.append(gd.inp("gains", gains, 4))
    ws_bytes = FC.workspace_bytes(c)
    if c.workspace:
        assert ws_bytes > 0, "the case expects a shape that uses the workspace"
        bufs.append(gd.out("ws", (ws_bytes,), np.uint8, 16))

    def launch(p):
        _lib.call("bf_beamform_fused_ws", p["raw"], p["dv"], dch, p.get("gains"), p["y"], B, C, T, A, M, CTOT, XENG, TS,
                  T0, BDT, flags, scale, p.get("ws"), ws_bytes, ex.queue.handle)

    def oracle(outs):
        y = outs["y"]
        if i8 and flags & VIA_F32:  # the contract: bf_requant of the float beams (the same kernel's float form)
            np.testing.assert_array_equal(y, O.requantise(f32_of, scale))
        elif i8:
            ref = O.fused_beamform_int8(rawv, d, CTOT, xeng_id=XENG, t0=T0, batch_dt=BDT, scale=scale, signed=signed,
                                        gains=gains)
            np.testing.assert_array_equal(y, ref)
            assert np.abs(ref.astype(int)).max() >= 4 and (np.abs(ref.astype(int)) < 127).mean() > 0.5
        else:
            ref = O.fused_beamform(rawv, d, CTOT, xeng_id=XENG, t0=T0, batch_dt=BDT, signed=signed, gains=gains)
            w = O.fused_tables(d, B, C, CTOT, A, xeng_id=XENG, t0=T0, batch_dt=BDT, gains=gains)
            assert_beams_allclose(y, ref, O.reorder(rawv), w, signed=signed)

    y = gd.run_case(ex, bufs, launch, oracle, c.expect)["y"]
    assert FC.planned_name(c) == _lib.load().bf_last_kernel().decode()  # the plan, asked on the host, is what ran
    return y


def run(ex, calls):
    """The calls of one case in order; a call that requantises gets the previous call's float beams as its oracle."""
    y = None
    for c in calls:
        y = fused(ex, c, f32_of=y if c.requant_of_previous else None)


# ---- bf_beamform_fused_ws: the cases and their expected names are tests/fused_cases.py -------------------------------
@pytest.mark.parametrize("case", FC.F32_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, _, _ in FC.F32_CASES])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_fused_f32(ex, case, signed, exact):
    run(ex, FC.f32(case, signed, exact))


@pytest.mark.parametrize("shape", FC.F32_WIDE_SHAPES, ids=str)
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "gain"])
def test_fused_f32_wide_32_beam_slabs(ex, shape, signed, exact, weighted):
    """Per-channel delay models (delay_channels = C), a pulled-back last k-step, a partial last slab."""
    run(ex, FC.f32_wide_32_beam_slabs(shape, signed, exact, weighted))


def test_fused_f32_item_kernel_with_gains(ex):
    run(ex, FC.f32_item_kernel_with_gains())


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_fused_f32_persistent_wide_p2_and_its_refusal(ex, C, signed):
    """Config 4's item shape takes the persistent kernel; BF_FUSED_ORDER_CHANNEL, which it cannot honour, must take
    the slab kernel, and so must exact coefficients."""
    run(ex, FC.f32_persistent_wide_p2_and_its_refusal(C, signed))


@pytest.mark.parametrize("M", [1, 8, 12, 16])
@pytest.mark.parametrize("A", [64, 61])
@pytest.mark.parametrize("scale", FC.I8_ITEM_SCALES, ids=["pow2", "sixth"])
def test_fused_i8_item_kernel(ex, M, A, scale):
    """Every (nts, full) form x (a64, pow2) form; T and the sample type cycle through 16 / 144 / 256, int8 / uint8."""
    run(ex, FC.i8_item_kernel(M, A, scale))


@pytest.mark.parametrize("case", FC.I8_GENERIC_CASES, ids=[str(s) + "-" + n for s, n in FC.I8_GENERIC_CASES])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_fused_i8_generic_kernel(ex, case, signed):
    run(ex, FC.i8_generic_kernel(case, signed))


@pytest.mark.parametrize("shape", FC.I8_W32_SHAPES, ids=str)
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "gain"])
def test_fused_i8_w32_in_kernel_phasors(ex, shape, signed, weighted):
    """No workspace: the 32-beam integer kernel evaluates its phasors itself.  (72, 33): byte stores, a partial slab."""
    run(ex, FC.i8_w32_in_kernel_phasors(shape, signed, weighted))


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "gain"])
@pytest.mark.parametrize("case", FC.I8_WORKSPACE_CASES, ids=["-".join(map(str, c)) for c in FC.I8_WORKSPACE_CASES])
def test_fused_i8_with_guarded_workspace(ex, case, weighted):
    """A workspace of exactly bf_fused_workspace_bytes, guarded as an output: the generated Q14 table (the generator's
    item layout, with and without gains) is written wholly inside it.  C = 5 is not a multiple of the ring kernel's
    channels per workgroup."""
    run(ex, FC.i8_with_guarded_workspace(case, weighted))


@pytest.mark.parametrize("case", FC.VIA_F32_CASES, ids=["-".join(map(str, c)) for c in FC.VIA_F32_CASES])
@pytest.mark.parametrize("scale", FC.VIA_F32_SCALES, ids=["pow2", "sixth"])
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_fused_i8_via_f32(ex, case, scale, exact):
    """BF_FUSED_INT8_VIA_F32 == bf_requant of the same call's float beams (themselves held to the float tolerance):
    every form of the item kernel's requantising instantiation, and the generic kernel's."""
    run(ex, FC.i8_via_f32(case, scale, exact))


# ---- bf_beamform --------------------------------------------------------------------------------------------------------
beamform = gd.beamform  # the guarded bf_beamform call (shared with tests/test_gpu_plan_edges.py)


RING, TABLE = "beamform_table_ring_kernel:", "beamform_table_kernel:"


@pytest.mark.parametrize("A,M,NB,B,C,name", [
    (64, 3, 3, 2, 3, "nts1,r4"), (128, 9, 3, 2, 3, "nts2,r8"), (256, 40, 3, 1, 1, "nts2,r16"),
    (128, 25, 2, 1, 2, "nts4,r8"), (64, 64, 2, 1, 2, "nts8,r4"), (64, 9, 3, 1, 2, "nts2,r4"),
    (64, 25, 2, 1, 2, "nts4,r4"), (128, 3, 3, 1, 2, "nts1,r8"), (256, 3, 2, 1, 2, "nts1,r16"),
    (128, 64, 2, 1, 2, "nts8,r8")])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_beamform_ring_kernel_both_load_widths(ex, A, M, NB, B, C, name, signed):
    """Ring depths 4 / 8 / 16 and slab widths 1 / 2 / 4 / 8, x at +0 (16-byte loads) and at +8 (8-byte loads), the
    table at +4: the same bits from both load widths."""
    y16 = beamform(ex, A, M, NB, B, C, signed, f"{RING}{name},w16", x_off=0)
    y8 = beamform(ex, A, M, NB, B, C, signed, f"{RING}{name},w8", x_off=8)
    np.testing.assert_array_equal(y16.view(np.uint32), y8.view(np.uint32))


@pytest.mark.parametrize("A,M,name", [
    (4, 3, "nts1,vec8"), (5, 3, "nts1,scalar"), (12, 20, "nts2,vec8"), (5, 9, "nts2,scalar"), (12, 25, "nts4,vec8"),
    (5, 25, "nts4,scalar"), (12, 64, "nts8,vec8"), (5, 64, "nts8,scalar")])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_beamform_table_kernel(ex, A, M, name, signed):
    y0 = beamform(ex, A, M, 3, 2, 3, signed, TABLE + name, x_off=0)
    y8 = beamform(ex, A, M, 3, 2, 3, signed, TABLE + name, x_off=8)
    np.testing.assert_array_equal(y0.view(np.uint32), y8.view(np.uint32))


@pytest.mark.parametrize("A", [64, 128])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_beamform_output_stationary(ex, A, signed):
    """(M = 64, T = 256) with x and w at 16 bytes; the table at +4 keeps the same call on the slab kernels, same bits."""
    y = beamform(ex, A, 64, 16, 1, 2, signed, "beamform_table_os_kernel", x_off=16, w_off=16)
    ring = f"{RING}nts8,{'r4' if A == 64 else 'r8'},w16"
    y4 = beamform(ex, A, 64, 16, 1, 2, signed, ring, x_off=16, w_off=4)
    np.testing.assert_array_equal(y.view(np.uint32), y4.view(np.uint32))


@pytest.mark.parametrize("B,C,M", [(2, 2, 12), (1, 5, 12), (1, 4, 40)])
def test_beamform_persistent_kernel(ex, B, C, M):
    """A = 256 with >= 8 (b, p, c) items: 8 items, 10 items (no multiple of 8), and 8 items of three slabs (XCD item
    order).  The same call with x at +8 cannot take it and must name the ring kernel: same bits."""
    yp = beamform(ex, 256, M, 2, B, C, False, "beamform_table_persist_kernel:nts2,r16,u8", x_off=0)
    yr = beamform(ex, 256, M, 2, B, C, False, RING + "nts2,r16,w8", x_off=8)
    np.testing.assert_array_equal(yp.view(np.uint32), yr.view(np.uint32))


# ---- the other entry points -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,C,T", [(1, 1, 16), (3, 7, 48), (257, 2, 64), (8, 3, 32)])
def test_reorder(ex, A, C, T):
    B = 2
    x = O.u8_voltages((B, A, C, T, 2, 2), seed=A * 1000 + T)
    bufs = [gd.inp("in", x, 16), gd.out("out", (B, 2, C, T // 16, 16, A, 2), np.uint8, 16)]
    gd.run_case(ex, bufs, lambda p: _lib.call("bf_reorder", p["in"], p["out"], B, A, C, T, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["out"], O.reorder(x)),
                "reorder_kernel:" + ("oct" if A % 8 == 0 else "any"))


@pytest.mark.parametrize("A,M", [(256, 64), (33, 70), (5, 3)])
@pytest.mark.parametrize("off", [0, 8])
def test_coeff_gen(ex, A, M, off):
    B, P, C = 1, 2, 2
    d = delays(C, M, A, A + M)
    name = "coeff_gen_block_kernel:nt" if off == 0 else "coeff_gen_tile_kernel" if A >= 32 and M >= 32 else "coeff_gen_kernel"
    bufs = [gd.inp("dv", d, 16), gd.out("w", (B, P, C, 2 * A, 2 * M), np.float32, off)]
    gd.run_case(ex, bufs,
                lambda p: _lib.call("bf_coeff_gen", p["dv"], p["w"], B, P, C, CTOT, A, M, XENG, TS, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["w"], O.coeffs(d, B, P, C, CTOT, A, M, XENG)), name)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("dch", [1, 3])
def test_coeff_gen_time(ex, f16, dch):
    C, A, M, nt, step = 3, 5, 3, 4, 8192 * TS
    d = delays(dch, M, A, 7)
    dt = np.float16 if f16 else np.float32
    bufs = [gd.inp("dv", d, 16), gd.out("w", (nt, C, A, M, 2), dt, 4 if f16 else 8)]

    def oracle(o):
        for t in range(nt):
            cos, sin = O.coeffs_at(np.broadcast_to(d, (C, M, A, 4)), C, CTOT, A, M, XENG, TS, T0 + t * step)
            np.testing.assert_array_equal(o["w"][t, ..., 0], cos.transpose(0, 2, 1).astype(dt))
            np.testing.assert_array_equal(o["w"][t, ..., 1], sin.transpose(0, 2, 1).astype(dt))

    gd.run_case(ex, bufs, lambda p: _lib.call("bf_coeff_gen_time", p["dv"], dch, p["w"], int(f16), nt, C, CTOT, A, M,
                                              XENG, TS, T0, step, ex.queue.handle),
                oracle, "coeff_gen_time_kernel:" + ("f16" if f16 else "f32"))


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_coeff_gen_time_study(ex, f16):
    """Bars: the study harness's 1e-4 on every float; the half2 form within half a float16 ulp of 1 more."""
    NT, C, A, M = 3, 6, 5, 3
    d = O.study_delay_ramp(A, M)
    w = O.study_coeffs_time(d, NT, C, A, M)
    ref = np.stack([w.real, w.imag], axis=-1)
    bufs = [gd.inp("dv", d, 16), gd.out("w", (NT, C, A, M, 2), np.float16 if f16 else np.float32, 4 if f16 else 8)]

    def oracle(o):
        assert np.abs(o["w"].astype(np.float32) - ref).max() <= (2 ** -11 + 1e-4 if f16 else 1e-4)

    gd.run_case(ex, bufs, lambda p: _lib.call("bf_coeff_gen_time_study", p["dv"], p["w"], int(f16), NT, C, A, M,
                                              ctypes.c_float(1e-7), 8192, ex.queue.handle),
                oracle, "coeff_gen_time_study_kernel:" + ("f16" if f16 else "f32"))


def test_study_single_channel_ragged(ex):
    """Bars: the study harness's 1e-1 absolute and the float32 bar 2e-5 sum_a |x| of the existing parity test."""
    C, T, A, M = 5, 48, 37, 20
    rng = np.random.default_rng(C * T + A)
    d = np.zeros((M * A, 4), np.float32)
    d[:, 0] = rng.uniform(0, 1e-7 / 3, M * A)
    d[:, 1] = rng.uniform(-3e-6, 3e-6, M * A)
    d[:, 2] = rng.uniform(-np.pi, np.pi, M * A)
    d[:, 3] = rng.uniform(-1e-5, 1e-5, M * A)
    x = rng.integers(-128, 128, (C, T // 16, A, 16, 2), dtype=np.int64).astype(np.int8)
    ref = O.study_beams_single_channel(d, x, C, T, A, M)
    bufs = [gd.inp("dv", d, 16), gd.inp("x", x, 4), gd.out("y", (C, T // 16, M, 16, 2), np.float32, 8)]

    def oracle(o):
        err = np.abs(o["y"].astype(np.float64) - ref)
        assert err.max() <= 1e-1
        mag = np.abs(x.astype(np.float64)).sum(axis=2)[:, :, None]
        assert (err <= 2e-5 * mag + 1e-6).all(), float((err / (2e-5 * mag + 1e-6)).max())

    gd.run_case(ex, bufs, lambda p: _lib.call("bf_beamform_study_single_channel", p["dv"], p["x"], p["y"], C, T, A, M,
                                              ctypes.c_float(1e-7), 8192, ex.queue.handle),
                oracle, "study_beamform_single_channel_kernel")


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "gain"])
@pytest.mark.parametrize("dch", [1, 3])
@pytest.mark.parametrize("A,M", [(19, 3), (64, 5)])
def test_q14_coeffs(ex, weighted, dch, A, M):
    B, C = 2, 3
    d = delays(dch, M, A, A + M + dch)
    g = np.random.default_rng(A + M).uniform(-1.9, 1.9, (M, A)).astype(np.float32) if weighted else None
    w = O.quantise_coeffs(O.fused_tables(d, B, C, CTOT, A, xeng_id=XENG, t0=T0, batch_dt=BDT, gains=g))
    wc, ws = w[:, 0, :, 0::2, 0::2], w[:, 0, :, 0::2, 1::2]  # (B, C, A, M)
    ref = np.ascontiguousarray(((wc & 0xffff) | ((ws & 0xffff) << 16)).transpose(0, 1, 3, 2)).astype(np.uint32)
    bufs = [gd.inp("dv", d, 16), gd.out("w", (B, C, M, A), np.uint32, 4)] + ([gd.inp("g", g, 4)] if weighted else [])
    gd.run_case(ex, bufs, lambda p: _lib.call("bf_q14_coeffs", p["dv"], dch, p.get("g"), p["w"], B, C, A, M, CTOT, XENG,
                                              TS, T0, BDT, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["w"], ref),
                f"q14_table_kernel:{'gain' if weighted else 'unit'},natural")


def splitmix64(z):
    z = (z + np.uint64(0x9e3779b97f4a7c15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


@pytest.mark.parametrize("nbytes", [7, 16, 1000 + 7, 256 * 16 * 3 + 9])
def test_fill_random(ex, nbytes):
    """include/bf.h: splitmix64 of seed and position, two words per 16-byte chunk; the last chunk is cut."""
    seed = 0x1234567890abcdef
    with np.errstate(over="ignore"):
        words = splitmix64(np.uint64(seed) ^ np.arange(2 * ((nbytes + 15) // 16), dtype=np.uint64))
    ref = words.view(np.uint8)[:nbytes]
    gd.run_case(ex, [gd.out("dst", (nbytes,), np.uint8, 16)],
                lambda p: _lib.call("bf_fill_random", p["dst"], nbytes, seed, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["dst"], ref), "bf_fill_random_kernel")


@pytest.mark.parametrize("signed,sum_pols,masked,tint", [(False, False, True, 16), (True, True, False, 48),
                                                         (True, False, True, 4)])
def test_incoherent_beam(ex, signed, sum_pols, masked, tint):
    """Ragged shape, the output at +4, the mask (byte reads) at an odd address; the input's surroundings are checked."""
    B, C, T, A, scale = 2, 3, 48, 5, 0.37
    raw = voltages((B, A, C, T, 2, 2), signed, 5)
    mask = np.array([1, 0, 7, 1, 0], np.uint8) if masked else None
    flags = (_lib.INCOH_SIGNED if signed else 0) | (_lib.INCOH_SUM_POLS if sum_pols else 0)
    ref = incoherent_ref.incoherent_beam(raw.view(np.int8) if signed else raw, tint, signed, sum_pols, scale, mask)
    bufs = [gd.inp("raw", raw, 16), gd.out("out", ref.shape, np.float32, 4)] + ([gd.inp("mask", mask, 1)] if masked else [])
    gd.run_case(ex, bufs, lambda p: _lib.call("bf_incoherent_beam", p["raw"], p.get("mask"), p["out"], B, C, T, A, tint,
                                              flags, scale, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["out"].view(np.uint32), ref.view(np.uint32)),
                "incoherent_kernel")


@pytest.mark.parametrize("int8", [True, False], ids=["i8", "f32"])
@pytest.mark.parametrize("iquv", [True, False], ids=["iquv", "i"])
def test_beam_detect(ex, int8, iquv):
    B, C, T, M, tint, fint, scale = 2, 3, 48, 5, 16, 3, 0.37
    rng = np.random.default_rng(11)
    shape = (B, 2, C, T // 16, 16, 2 * M)
    beams = rng.integers(-128, 128, shape).astype(np.int8) if int8 else rng.normal(0, 300, shape).astype(np.float32)
    sums = detect_ref.stokes_sums(beams, tint, fint, iquv)
    ref = detect_ref.scale_sums(sums, scale)
    flags = (_lib.DETECT_IN_INT8 if int8 else 0) | (_lib.DETECT_STOKES_IQUV if iquv else 0)
    bufs = [gd.inp("beams", beams, 16), gd.out("out", ref.shape, np.float32, 4)]

    def oracle(o):
        if int8:
            np.testing.assert_array_equal(o["out"].view(np.uint32), ref.view(np.uint32))
        else:
            err = np.abs(o["out"].astype(np.float64) - ref.astype(np.float64))
            assert np.isfinite(o["out"]).all() and (err <= detect_ref.tolerance(ref, sums, tint, fint, scale)).all()

    gd.run_case(ex, bufs, lambda p: _lib.call("bf_beam_detect", p["beams"], p["out"], B, C, T, M, tint, fint, flags,
                                              scale, ex.queue.handle), oracle, "detect_kernel")


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_voltage_stats(ex, signed):
    B, C, T, A, tint, scale, lim = 2, 3, 48, 5, 16, 0.37, (0.6, 1.4)
    raw = voltages((B, A, C, T, 2, 2), signed, 9)
    raw[0, 2] = 0  # a dead input: S1 == 0
    power, sk, flg = vstats_ref.voltage_stats(raw.view(np.int8) if signed else raw, tint, signed, scale, lim)
    bufs = [gd.inp("raw", raw, 16), gd.out("power", power.shape, np.float32, 4), gd.out("sk", sk.shape, np.float32, 4),
            gd.out("flags", flg.shape, np.uint8, 1)]

    def oracle(o):
        np.testing.assert_array_equal(o["power"].view(np.uint32), power.view(np.uint32))
        np.testing.assert_array_equal(o["sk"].view(np.uint32), sk.view(np.uint32))
        np.testing.assert_array_equal(o["flags"], flg)

    gd.run_case(ex, bufs, lambda p: _lib.call("bf_voltage_stats", p["raw"], p["power"], p["sk"], p["flags"], B, C, T, A,
                                              tint, _lib.VSTATS_SIGNED if signed else 0, scale, lim[0], lim[1],
                                              ex.queue.handle), oracle, "vstats_kernel")


# ---- bf_requant ---------------------------------------------------------------------------------------------------------
FLT_MAX = np.finfo(np.float32).max


def requant_input(n, scale):
    """Exact ties after scaling (+-0.5, 1.5, 126.5, 127.5), +-0, denormals, products that ROUND onto a tie at a scale that
    is no power of two (3 * float32(1/6) = 0.5 + 2^-26 -> 0.5), +-FLT_MAX, +-inf, then noise; rotated by n so that short
    inputs see different ones."""
    ties = np.array([0.5, 1.5, 2.5, 126.5, 127.5, 128.5], np.float64)
    inv = 64.0 if scale == 1 / 64 else 6.0
    sp = np.concatenate([ties * inv, -ties * inv, 3.0 * np.arange(1, 60, 2), -3.0 * np.arange(1, 60, 2),
                         [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, FLT_MAX, -FLT_MAX, np.inf, -np.inf]])
    sp = np.roll(sp.astype(np.float32), -(n % sp.size))
    rng = np.random.default_rng(n)
    y = (rng.normal(0, 60 * inv, n)).astype(np.float32)
    y[:min(n, sp.size)] = sp[:min(n, sp.size)]
    return y


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1027, 256 * 4096 * 4 + 3])
@pytest.mark.parametrize("q_off", [0, 4])
@pytest.mark.parametrize("scale", [1 / 64, S6], ids=["pow2", "sixth"])
def test_requant(ex, n, q_off, scale):
    """The float4 body, the scalar tail (n % 4 != 0), q at its minimum alignment, and more than one grid-stride pass."""
    y = requant_input(n, scale)
    ref = O.requantise(y, scale)
    if n > 200:
        sp = y[:82]  # the special values, rotated
        prod = sp[np.isfinite(sp)] * np.float32(scale)
        assert (np.abs(prod - np.trunc(prod)) == 0.5).sum() >= 12  # the ties are ties
    gd.run_case(ex, [gd.inp("y", y, 16), gd.out("q", (n,), np.int8, q_off)],
                lambda p: _lib.call("bf_requant", p["y"], p["q"], n, scale, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["q"], ref), "requant_kernel")


def test_requant_nan_gives_minus_127(ex):
    """include/bf.h: the clamp's maxNum(r, -127) drops a NaN, so a NaN product is -127 (body and tail)."""
    y = np.array([np.nan, 1.0, -np.nan, np.inf, np.nan, -np.inf, np.nan], np.float32)
    y[2] = np.frombuffer(np.uint32(0xffffffff).tobytes(), np.float32)[0]
    ref = O.requantise(y, 1.0)
    np.testing.assert_array_equal(ref, [-127, 1, -127, 127, -127, -127, -127])
    gd.run_case(ex, [gd.inp("y", y, 16), gd.out("q", (7,), np.int8, 4)],
                lambda p: _lib.call("bf_requant", p["y"], p["q"], 7, 1.0, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["q"], ref), "requant_kernel")
