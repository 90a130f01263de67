"""GPU: the correlator (bf_correlate, csrc/bf_correlate.hip; beamforming.correlate) against the NumPy restatement of
the contract (correlate_ref.py): every element compared as int32, no tolerance.

Shapes are the smallest at which each mechanism of the kernel can break: fewer antennas than a 16-antenna tile and
one more than one, two and four tiles (65 antennas: a second block row of one ragged tile, three workgroups per window
and channel, the padded grid), windows of half a K step (16 samples), one and a half (48), whole steps, windows over
several batches, both sample conventions, full scale at the two int32 bounds, and a window whose neighbours differ
grossly from it."""
import numpy as np
import pytest

import correlate_ref as R
import guarded as gd
import incoherent_ref as IR
import oracle as O
from dpdk_dc_sand_amd import _lib, accel
from dpdk_dc_sand_amd.beamforming import (CorrelatorTemplate, FusedBeamformerTemplate, IncoherentBeamTemplate,
                                          baseline_index, visibility_matrix)

pytestmark = pytest.mark.gpu

SIGNED, ACC = _lib.CORR_SIGNED, _lib.CORR_ACCUMULATE
ANTS = [1, 2, 3, 8, 9, 17, 64, 65]
WINDOWS = [(1, 16, 16), (3, 48, 16), (3, 48, 48), (2, 256, 256), (2, 256, 32)]  # (C, T, tint)
BATCHES = [(1, 1), (3, 1), (3, 3)]                                              # (B, bint)
GRID = [(A, C, T, tint, B, bint) for A in ANTS for (C, T, tint) in WINDOWS for (B, bint) in BATCHES
        if bint == 1 or tint == T]


def correlate(context, queue, raw, tint, bint, flags, out=None, fill=None):
    """bf_correlate on a cube; `out` is reused when given (accumulation), else allocated (and filled with the byte
    `fill`: the kernel assumes no zeroed output)."""
    B, A, C, T = raw.shape[:4]
    d_raw = accel.DeviceArray(context, raw.shape, np.uint8)
    d_raw.set(queue, np.ascontiguousarray(raw).view(np.uint8))
    if out is None:
        shape = (B // bint, C, T // tint, R.n_baselines(A), 2, 2, 2)
        out = accel.DeviceArray(context, shape, np.int32)
        if fill is not None:
            out.set(queue, np.full(shape, fill * 0x01010101, np.uint32).view(np.int32))
    _lib.call("bf_correlate", d_raw.ptr, out.ptr, B, C, T, A, tint, bint, flags, queue.handle)
    queue.finish()
    return out


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
@pytest.mark.parametrize("shape", GRID, ids=lambda s: "A{}-C{}-T{}-t{}-B{}-b{}".format(*s))
def test_shape_grid(context, command_queue, shape, signed):
    A, C, T, tint, B, bint = shape
    raw = R.random_voltages((B, A, C, T))
    ref = R.reference((B, A, C, T), tint, bint, signed)
    out = correlate(context, command_queue, raw, tint, bint, SIGNED if signed else 0, fill=0x5A)
    assert _lib.load().bf_last_kernel() == (b"correlate_kernel:i8" if signed else b"correlate_kernel:u8")
    got = out.get(command_queue)
    assert got.shape == ref.shape and got.dtype == np.int32
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
def test_many_workgroups_per_window(context, command_queue, signed):
    """200 antennas: 13 tiles (the last with 8 antennas), 91 tile pairs in ten blocks of 4 x 4, the last block row
    one tile high: diagonal, full and ragged off-diagonal blocks; 18 (window, channel) items are padded to 24 in the
    grid."""
    B, A, C, T, tint = 1, 200, 9, 32, 16
    raw = R.random_voltages((B, A, C, T))
    out = correlate(context, command_queue, raw, tint, 1, SIGNED if signed else 0, fill=0xA5)
    np.testing.assert_array_equal(out.get(command_queue), R.reference((B, A, C, T), tint, 1, signed))


FULL_SCALE = {True: dict(B=3, T=21840, bint=3, lo=-128, hi=127),   # n = 65520 <= 65535
              False: dict(B=1, T=16512, bint=1, lo=0, hi=255)}      # n = 16512


@pytest.mark.parametrize("pattern", ["constant", "random"])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
def test_full_scale_at_the_int32_bound(context, command_queue, signed, pattern):
    """The longest windows of the two conventions, two antennas, one channel: every sample -128 (int8: the sums reach
    2 * 128^2 * 65520 = 2146959360) or 255 (uint8: 130050 * 16512 = 2147385600), and random bytes of the two extreme
    values of the convention.  Intermediate sums of the kernel's biased arithmetic wrap; the results may not."""
    p = FULL_SCALE[signed]
    shape = (p["B"], 2, 1, p["T"], 2, 2)
    if pattern == "constant":
        x = np.full(shape, p["lo"] if signed else p["hi"], np.int16)
    else:
        x = np.where(np.random.default_rng(3).integers(0, 2, shape) == 1, p["hi"], p["lo"])
    raw = x.astype(np.int8 if signed else np.uint8).view(np.uint8)
    ref = R.visibilities(raw, p["T"], p["bint"], signed)
    if pattern == "constant":
        assert int(ref.max()) == (2146959360 if signed else 2147385600)
    got = correlate(context, command_queue, raw, p["T"], p["bint"], SIGNED if signed else 0, fill=0x5A)
    np.testing.assert_array_equal(got.get(command_queue), ref)


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
def test_window_isolation(context, command_queue, signed):
    """tint = 16 fills half of one K step: a window at full scale between windows of zeros.  A kernel that read on into
    the next window, or left the other half of the step unmasked, would show it in the zero windows."""
    B, A, C, T, tint = 2, 3, 2, 80, 16
    raw = np.zeros((B, A, C, T, 2, 2), np.uint8)
    raw[:, :, :, 16:32] = 0x80 if signed else 0xFF
    raw[:, :, :, 64:80] = 0x80 if signed else 0xFF
    ref = R.visibilities(raw, tint, 1, signed)
    assert not ref[:, :, [0, 2, 3]].any() and (ref[:, :, [1, 4], ..., 0] == (2 ** 19 if signed else 130050 * 16)).all()
    got = correlate(context, command_queue, raw, tint, 1, SIGNED if signed else 0, fill=0x5A).get(command_queue)
    np.testing.assert_array_equal(got, ref)
    # and the other way round: zeros between full scale
    raw = raw ^ (0x80 if signed else 0xFF)
    got = correlate(context, command_queue, raw, tint, 1, SIGNED if signed else 0, fill=0xA5).get(command_queue)
    np.testing.assert_array_equal(got, R.visibilities(raw, tint, 1, signed))
    assert not got[:, :, [1, 4]].any()


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
def test_accumulate(context, command_queue, signed):
    """An output filled with 0x5A: one plain call and two accumulating calls give the restatement's sum of the three
    cubes; a plain call after that overwrites."""
    B, A, C, T, tint = 2, 17, 3, 48, 16
    cubes = [R.random_voltages((B, A, C, T)), R.random_voltages((B, A, C, T + 16))[:, :, :, :T],
             R.random_voltages((B, A, C, T + 32))[:, :, :, 16:16 + T]]
    flags = SIGNED if signed else 0
    out = correlate(context, command_queue, cubes[0], tint, 1, flags, fill=0x5A)
    for raw in cubes[1:]:
        correlate(context, command_queue, raw, tint, 1, flags | ACC, out=out)
        assert _lib.load().bf_last_kernel() == (b"correlate_kernel:i8,acc" if signed else b"correlate_kernel:u8,acc")
    np.testing.assert_array_equal(out.get(command_queue), R.accumulate(cubes, tint, 1, signed))
    correlate(context, command_queue, cubes[1], tint, 1, flags, out=out)
    np.testing.assert_array_equal(out.get(command_queue), R.visibilities(cubes[1], tint, 1, signed))


def test_accumulate_wraps_in_uint32(context, command_queue):
    """out += S is uint32 arithmetic: onto 0x7fffffff the sum wraps as two's complement does."""
    B, A, C, T = 1, 2, 1, 16
    raw = R.random_voltages((B, A, C, T))
    ref = R.visibilities(raw, T, 1, True)
    out = accel.DeviceArray(context, ref.shape, np.int32)
    out.set(command_queue, np.full(ref.shape, 0x7fffffff, np.int32))
    correlate(context, command_queue, raw, T, 1, SIGNED | ACC, out=out)
    want = (ref.astype(np.int64) + 0x7fffffff).astype(np.uint32).view(np.int32)
    np.testing.assert_array_equal(out.get(command_queue), want)


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
@pytest.mark.parametrize("A,B,C,T,tint,bint", [(3, 2, 2, 48, 16, 1), (65, 3, 3, 32, 16, 1), (65, 3, 1, 32, 32, 3)],
                         ids=["A3", "A65", "A65-bint3"])
def test_guard_bands(context, command_queue, A, B, C, T, tint, bint, signed):
    """All five verdicts of the guard-band harness, raw at offset 16 and out at offset 4 (their smallest legal
    alignments): every element written in both runs, nothing outside the payload, the input untouched."""
    ex = gd.DeviceExecutor(context, command_queue)
    raw = R.random_voltages((B, A, C, T))
    ref = R.reference((B, A, C, T), tint, bint, signed)
    bufs = [gd.inp("raw", raw, 16), gd.out("out", ref.shape, np.int32, 4)]

    def oracle(outputs):
        np.testing.assert_array_equal(outputs["out"], ref)

    gd.run_case(ex, bufs, lambda p: _lib.call("bf_correlate", p["raw"], p["out"], B, C, T, A, tint, bint,
                                              SIGNED if signed else 0, command_queue.handle), oracle,
                "correlate_kernel:i8" if signed else "correlate_kernel:u8")


def test_through_python_with_the_beamformer(context, command_queue):
    """One inSamples buffer bound to a FusedBeamformer (int8 beams), a Correlator and an IncoherentBeam on one queue:
    the beams equal the oracle's integer contract, the visibilities the restatement, their matrix is Hermitian, and the
    sum of the autos over the antennas is the incoherent beam at scale 1 (sums below 2^24: exact in float32)."""
    B, A, M, C, Ctot, T, tint = 2, 64, 16, 4, 4096, 256, 16
    rng = np.random.default_rng(22)
    d1 = np.zeros((1, M, A, 4), np.float32)
    d1[..., 0] = rng.uniform(0, 10 * O.TS_MEERKAT, (M, A))
    d1[..., 2] = rng.uniform(-np.pi, np.pi, (M, A))
    raw8 = R.random_voltages((B, A, C, T)).view(np.int8)
    fused = FusedBeamformerTemplate(context, B, C, Ctot, T, A, M, delay_channels=1, sample_signed=True, out_int8=True,
                                    out_scale=1 / 64).instantiate(command_queue)
    corr = CorrelatorTemplate(context, B, C, T, A, integration=tint, sample_signed=True).instantiate(command_queue)
    incoh = IncoherentBeamTemplate(context, B, C, T, A, integration=tint, sample_signed=True,
                                   scale=1.0).instantiate(command_queue)
    fused.ensure_all_bound()
    corr.bind(inSamples=fused.buffer("inSamples"))
    incoh.bind(inSamples=fused.buffer("inSamples"))
    corr.ensure_all_bound()
    incoh.ensure_all_bound()
    assert corr.buffer("inSamples") is fused.buffer("inSamples")
    fused.buffer("inSamples").set(command_queue, raw8)
    fused.buffer("delay_vals").set(command_queue, d1)
    fused()
    corr()
    incoh()
    vis = corr.buffer("outVisibilities").get(command_queue)
    np.testing.assert_array_equal(fused.buffer("outData").get(command_queue),
                                  O.fused_beamform_int8(raw8, d1, Ctot, scale=1 / 64, signed=True))
    np.testing.assert_array_equal(vis, R.reference((B, A, C, T), tint, 1, True))
    full = visibility_matrix(vis)                                       # (B, C, J, A, 2, A, 2)
    flat = full.reshape(B, C, T // tint, 2 * A, 2 * A)
    np.testing.assert_array_equal(flat, np.conj(np.swapaxes(flat, -1, -2)))
    i, conj = baseline_index(5, 9)
    np.testing.assert_array_equal(full[..., 5, 0, 9, 1], vis[..., i, 1, 0, 0] - 1j * vis[..., i, 1, 0, 1])
    assert conj
    autos = np.einsum("bcjapap->bpcj", full)                            # sum over antennas of auto (p, p)
    assert not autos.imag.any() and autos.real.max() < 2 ** 24
    beam = incoh.buffer("outData").get(command_queue)                   # (B, 2, C, J) float32
    np.testing.assert_array_equal(beam, autos.real.astype(np.float32))
    np.testing.assert_array_equal(beam, IR.incoherent_beam(raw8, tint, True, False, 1.0))
    np.testing.assert_array_equal(fused.buffer("inSamples").get(command_queue), raw8)


def test_python_accumulate(context, command_queue):
    """accumulate=True: the first call overwrites (the buffer is prefilled), later calls add, reset() starts over, and
    the call that would pass the int32 bound raises with the output unchanged."""
    B, A, C, T = 1, 9, 2, 4096
    raw = R.random_voltages((B, A, C, T))
    one = R.reference((B, A, C, T), T, 1, False).astype(np.int64)
    op = CorrelatorTemplate(context, B, C, T, A, accumulate=True).instantiate(command_queue)
    op.ensure_all_bound()
    op.buffer("inSamples").set(command_queue, raw)
    op.buffer("outVisibilities").set(command_queue, np.full(one.shape, 0x5A5A5A5A, np.int32))
    for k in (1, 2, 3, 4):
        op()
        assert op.samples_accumulated == k * T
        np.testing.assert_array_equal(op.buffer("outVisibilities").get(command_queue), k * one)
    with pytest.raises(OverflowError):  # 5 * 4096 > 16512
        op()
    np.testing.assert_array_equal(op.buffer("outVisibilities").get(command_queue), 4 * one)
    op.reset()
    op()
    np.testing.assert_array_equal(op.buffer("outVisibilities").get(command_queue), one)


def test_full_size_slice(context, command_queue):
    """Configuration 3's antennas, batches and integration on a slice of its channels: A = 64, C = 32, T = 256, B = 8,
    bint = 8 (2048 samples per window), uint8: ten tile pairs, one diagonal block, one workgroup per channel."""
    B, A, C, T = 8, 64, 32, 256
    raw = R.random_voltages((B, A, C, T))
    out = correlate(context, command_queue, raw, T, B, 0, fill=0x5A)
    np.testing.assert_array_equal(out.get(command_queue), R.reference((B, A, C, T), T, B, False))
