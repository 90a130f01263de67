"""GPU: the voltage statistics (bf_voltage_stats, csrc/bf_vstats.hip; beamforming.vstats) against the NumPy restatement
of the contract (vstats_ref.py), bit for bit: float32 outputs as uint32, flags as uint8, every element.

Shapes are (B, A, C, T, tint), the smallest at which each mechanism of the kernel can break: one window with mostly
dead lanes, windows of 16 (one sum of four lanes, no shuffle), lane groups that are no power of two (tint 48, 1040,
4080), one wave, windows across waves (512, 1024), across the 4096-sample workgroup steps (2048 of 4096, 4112, 8192,
16384, 32768), several and partial pieces per run, and the boundaries of the kernel's own sizes: exactly one step
(4096), exactly one piece of 16384 samples and one window more (1024 windows of 16 = both windows a thread owns, then a
second piece with a single window), a piece of four windows with a partial second piece (20480 / 4096)."""
import numpy as np
import pytest

import incoherent_ref as IR
import oracle as O
import vstats_ref as R
from dpdk_dc_sand_amd import _lib, accel
from dpdk_dc_sand_amd.beamforming import (FusedBeamformerTemplate, IncoherentBeamTemplate, VoltageStatsTemplate,
                                          antenna_mask_from_flags)

pytestmark = pytest.mark.gpu

SCALE = 1 / 3  # not a power of two: the float64 product's rounding matters

GRID = [(1, 1, 1, 16, 16), (2, 3, 3, 48, 16), (2, 3, 3, 48, 48), (1, 2, 3, 2080, 1040), (1, 2, 2, 256, 256),
        (1, 2, 1, 1024, 512), (1, 3, 1, 1024, 1024), (1, 2, 1, 4096, 2048), (1, 1, 2, 8224, 4112),
        (1, 1, 1, 16384, 16384), (2, 9, 5, 272, 16), (2, 3, 5, 1040, 16),
        # the kernel's own sizes: one step, one piece and one window more, partial pieces of long windows, windows of
        # two steps and of two pieces, 255 groups of four lanes per window
        (1, 2, 1, 4096, 4096), (1, 1, 1, 16384, 16), (1, 2, 1, 16400, 16), (1, 1, 1, 20480, 4096),
        (1, 1, 2, 16384, 8192), (1, 1, 1, 32768, 32768), (1, 2, 1, 8160, 4080), (1, 1, 3, 16416, 48)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(context, queue, raw, tint, signed, scale=SCALE, power=True, sk=True, limits=None):
    B, A, C, T = raw.shape[:4]
    tmpl = VoltageStatsTemplate(context, B, C, T, A, integration=tint, sample_signed=signed, scale=scale, power=power,
                                sk=sk, sk_limits=limits)
    op = tmpl.instantiate(queue)
    op.ensure_all_bound()
    op.buffer("inSamples").set(queue, raw.view(np.int8 if signed else np.uint8))
    op()
    out = {}
    for name, dtype in (("outPower", np.float32), ("outSK", np.float32), ("outFlags", np.uint8)):
        if name in op.slots:
            out[name] = op.buffer(name).get(queue)
            assert out[name].shape == tmpl.output_shape and out[name].dtype == dtype
    return out


def quantile_limits(sk):
    lo, hi = np.quantile(sk.astype(np.float64), [0.3, 0.7]).astype(np.float32)
    if not lo < hi:  # fewer than two distinct values (a single window): any valid pair
        hi = np.nextafter(lo, np.float32(np.inf))
    return float(lo), float(hi)


def check(got, raw, tint, signed, scale, limits):
    power, sk, flags = R.voltage_stats(raw, tint, signed, scale, limits)
    for name, ref in (("outPower", power), ("outSK", sk), ("outFlags", flags)):
        if name in got:
            np.testing.assert_array_equal(bits(got[name]), bits(ref), err_msg=name)
    return power, sk, flags


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
def test_shape_grid(context, command_queue, shape, signed):
    B, A, C, T, tint = shape
    raw = R.random_voltages((B, A, C, T))
    S1, S2 = R.moments(raw, tint, signed)
    limits = quantile_limits(R.spectral_kurtosis(S1, S2, tint))
    got = run(context, command_queue, raw, tint, signed, limits=limits)
    assert set(got) == {"outPower", "outSK", "outFlags"}
    power, sk, flags = check(got, raw, tint, signed, SCALE, limits)
    assert power.min() > 0 and (sk != 0).all()
    if flags.size >= 8:
        assert flags.any() and not flags.all()


@pytest.mark.parametrize("pattern", ["all255", "alternating"])
def test_full_scale_uint8(context, command_queue, pattern):
    """uint8 at (1, 1, 1, 2^18, 2^18), a 1 MiB cube, the longest window: all 255 gives S1 = 34091827200 (past 2^32) and
    S2 = 4433642127360000 (just below 2^52), SK exactly 0; 255+255i alternating with 0 gives SK = float32((n + 1) /
    (n - 1))."""
    n = 1 << 18
    raw = np.zeros((1, 1, 1, n, 2, 2), np.uint8)
    raw[:, :, :, 0::(1 if pattern == "all255" else 2)] = 255
    S1, S2 = R.moments(raw, n, False)
    if pattern == "all255":
        assert (S1 == 34091827200).all() and (S2 == 4433642127360000).all() and S1.min() > 2 ** 32
    limits = (0.5, 1.5)
    got = run(context, command_queue, raw, n, False, limits=limits)
    power, sk, flags = check(got, raw, n, False, SCALE, limits)
    if pattern == "all255":
        assert (bits(sk) == 0).all() and flags.all()
    else:
        assert (sk == np.float32((n + 1) / (n - 1))).all() and not flags.any()


def test_full_scale_int8(context, command_queue):
    """int8 all -128 at (1, 2, 1, 256, 256): pw = 2^15, pw^2 = 2^30, so four samples pass 2^32 in S2."""
    raw = np.full((1, 2, 1, 256, 2, 2), -128, np.int8)
    S1, S2 = R.moments(raw, 256, True)
    assert (S1 == 2 ** 23).all() and (S2 == 2 ** 38).all()
    got = run(context, command_queue, raw.view(np.uint8), 256, True, limits=(0.5, 1.5))
    _, sk, flags = check(got, raw, 256, True, SCALE, (0.5, 1.5))
    assert (bits(sk) == 0).all() and flags.all()


def test_dead_input(context, command_queue):
    """All zeros: power +0, SK +0, flagged whatever the limits."""
    raw = np.zeros((1, 2, 2, 512, 2, 2), np.uint8)
    got = run(context, command_queue, raw, 256, False, limits=(0.0, 1e30))
    assert not bits(got["outPower"]).any() and not bits(got["outSK"]).any() and got["outFlags"].all()


def test_scaling_is_one_float64_multiply(context, command_queue):
    """Scale 1 / 3 and window sums of more than 24 significant bits (vstats_ref.SCALING_SHAPE; test_vstats_host.py
    checks on the CPU that scaling in float32 gives other bits for these sums)."""
    B, A, C, T, tint = R.SCALING_SHAPE
    raw = R.random_voltages((B, A, C, T))
    S1, _ = R.moments(raw, tint, False)
    ref = R.scale_power(S1, SCALE)
    assert S1.min() > 2 ** 24 and (bits(S1.astype(np.float32) * np.float32(SCALE)) != bits(ref)).any()
    got = run(context, command_queue, raw, tint, False, sk=False)
    assert set(got) == {"outPower"}
    np.testing.assert_array_equal(bits(got["outPower"]), bits(ref))


OPTIONAL_SHAPE = (2, 3, 3, 1040, 208)


@pytest.mark.parametrize("power,sk,flags", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)],
                         ids=["power", "sk", "flags", "power-sk", "power-flags", "sk-flags"])
def test_optional_outputs(context, command_queue, power, sk, flags):
    """Each single output and each pair gives the bytes of the all-three run (which equal the restatement)."""
    B, A, C, T, tint = OPTIONAL_SHAPE
    raw = R.random_voltages((B, A, C, T))
    S1, S2 = R.moments(raw, tint, True)
    limits = quantile_limits(R.spectral_kurtosis(S1, S2, tint))
    full = run(context, command_queue, raw, tint, True, limits=limits)
    check(full, raw, tint, True, SCALE, limits)
    got = run(context, command_queue, raw, tint, True, power=bool(power), sk=bool(sk), limits=limits if flags else None)
    assert set(got) == {n for n, on in (("outPower", power), ("outSK", sk), ("outFlags", flags)) if on}
    for name in got:
        assert got[name].tobytes() == full[name].tobytes(), name


@pytest.mark.parametrize("shape,flags", [((1, 3, 2, 8224, 4112), 0), ((2, 3, 5, 1040, 16), 1),
                                         ((1, 2, 1, 16400, 16), 0), ((2, 3, 3, 48, 48), 1)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"flags{v}")
def test_writes_stay_in_bounds(context, command_queue, shape, flags):
    """The C entry point into output arrays longer than the result, the whole arrays prefilled with a sentinel (the
    kernel assumes no zeroed output): the results are exact, the tails untouched, the input cube unchanged."""
    B, A, C, T, tint = shape
    signed = bool(flags & _lib.VSTATS_SIGNED)
    raw = R.random_voltages((B, A, C, T))
    n, tail = B * A * 2 * C * (T // tint), 4096
    S1, S2 = R.moments(raw, tint, signed)
    limits = quantile_limits(R.spectral_kurtosis(S1, S2, tint))
    sentinel32 = np.full(n + tail, 0x7fc0beef, np.uint32)
    sentinel8 = np.full(n + tail, 0xa5, np.uint8)
    d_raw = accel.DeviceArray(context, raw.shape, np.uint8)
    d_power = accel.DeviceArray(context, (n + tail,), np.uint32)
    d_sk = accel.DeviceArray(context, (n + tail,), np.uint32)
    d_flags = accel.DeviceArray(context, (n + tail,), np.uint8)
    d_raw.set(command_queue, raw)
    d_power.set(command_queue, sentinel32)
    d_sk.set(command_queue, sentinel32)
    d_flags.set(command_queue, sentinel8)
    _lib.call("bf_voltage_stats", d_raw.ptr, d_power.ptr, d_sk.ptr, d_flags.ptr, B, C, T, A, tint, flags, SCALE,
              limits[0], limits[1], command_queue.handle)
    power, sk, flg = R.voltage_stats(raw, tint, signed, SCALE, limits)
    for dev, ref, sentinel in ((d_power, power, sentinel32), (d_sk, sk, sentinel32), (d_flags, flg, sentinel8)):
        out = dev.get(command_queue)
        np.testing.assert_array_equal(out[:n], bits(ref).ravel())
        np.testing.assert_array_equal(out[n:], sentinel[n:])
    np.testing.assert_array_equal(d_raw.get(command_queue), raw)


def test_four_behaviours_and_the_antenna_mask(context, command_queue):
    """Noise, carrier, dead input and pulsed interference (vstats_ref.four_behaviours, limits 0.75 .. 1.25): the flags
    equal the restatement, the mask made of them keeps the noise antenna only, and an IncoherentBeam given that mask
    reproduces incoherent_ref with the same mask."""
    B, A, C, T, tint = R.FOUR_SHAPE
    raw = R.four_behaviours()
    got = run(context, command_queue, raw, tint, True, scale=1.0, limits=R.FOUR_LIMITS)
    check(got, raw, tint, True, 1.0, R.FOUR_LIMITS)
    mask = antenna_mask_from_flags(got["outFlags"], 0.2)
    np.testing.assert_array_equal(mask, [1, 0, 0, 0])
    incoh = IncoherentBeamTemplate(context, B, C, T, A, integration=256, sample_signed=True, scale=SCALE,
                                   antenna_mask=True).instantiate(command_queue)
    incoh.set_antenna_mask(mask)
    incoh.ensure_all_bound()
    incoh.buffer("inSamples").set(command_queue, raw)
    incoh()
    beam = incoh.buffer("outData").get(command_queue)
    np.testing.assert_array_equal(bits(beam), bits(IR.incoherent_beam(raw, 256, True, False, SCALE, mask=mask)))


def test_stream_order_with_the_beamformer(context, command_queue):
    """One inSamples buffer bound to a FusedBeamformer (int8 beams) and a VoltageStats, both launched on one queue,
    twice: the beams equal the oracle's integer contract, the statistics the restatement, the second round gives
    identical bytes, and the input is unchanged."""
    B, A, M, C, Ctot, T, tint = 2, 64, 16, 4, 4096, 256, 64
    rng = np.random.default_rng(21)
    d1 = np.zeros((1, M, A, 4), np.float32)
    d1[..., 0] = rng.uniform(0, 10 * O.TS_MEERKAT, (M, A))
    d1[..., 2] = rng.uniform(-np.pi, np.pi, (M, A))
    raw8 = R.random_voltages((B, A, C, T)).view(np.int8)
    limits = (0.3, 0.45)
    fused = FusedBeamformerTemplate(context, B, C, Ctot, T, A, M, delay_channels=1, sample_signed=True, out_int8=True,
                                    out_scale=1 / 64).instantiate(command_queue)
    stats = VoltageStatsTemplate(context, B, C, T, A, integration=tint, sample_signed=True, scale=SCALE,
                                 sk_limits=limits).instantiate(command_queue)
    fused.ensure_all_bound()
    stats.bind(inSamples=fused.buffer("inSamples"))
    stats.ensure_all_bound()
    assert stats.buffer("inSamples") is fused.buffer("inSamples")
    fused.buffer("inSamples").set(command_queue, raw8)
    fused.buffer("delay_vals").set(command_queue, d1)
    names = ("outPower", "outSK", "outFlags")
    runs = []
    for _ in range(2):
        fused()
        stats()
        runs.append([fused.buffer("outData").get(command_queue)] + [stats.buffer(n).get(command_queue) for n in names])
        fused.buffer("outData").zero(command_queue)
        for n in names:
            stats.buffer(n).zero(command_queue)
    np.testing.assert_array_equal(runs[0][0], O.fused_beamform_int8(raw8, d1, Ctot, scale=1 / 64, signed=True))
    _, _, flags = check(dict(zip(names, runs[0][1:])), raw8, tint, True, SCALE, limits)
    assert flags.any() and not flags.all()
    for first, second in zip(*runs):
        assert first.tobytes() == second.tobytes()
    np.testing.assert_array_equal(fused.buffer("inSamples").get(command_queue), raw8)
