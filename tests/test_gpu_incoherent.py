"""GPU: the incoherent beam (bf_incoherent_beam, csrc/bf_incoherent.hip; beamforming.incoherent) against the NumPy
restatement of its integer contract (incoherent_ref.py), bit for bit.

Shapes are (B, A, C, T, tint), the smallest at which each mechanism of the kernel can break: one lane, partial
workgroup pieces, antenna counts around the 4-antenna unroll, windows inside a lane (tint < 4), inside a lane group,
across waves (tint 512, 1024), across the two loads of a lane (tint 2080, 4096), across the 4096-sample workgroup steps
(tint 4112, 8192), lane groups that are no power of two (tint 48, 1040), more windows per piece than threads (tint 4,
C*T >= 4096), several pieces per batch, and antenna counts beyond one 32-bit accumulation run (8192)."""
import functools

import numpy as np
import pytest

import incoherent_ref as R
import oracle as O
from dpdk_dc_sand_amd import _lib, accel
from dpdk_dc_sand_amd.beamforming import FusedBeamformerTemplate, IncoherentBeamTemplate

pytestmark = pytest.mark.gpu

SCALE = 1 / 3  # not a power of two: the float64 product's rounding matters

GRID = [(1, 1, 1, 16, 1), (2, 3, 3, 16, 16), (1, 65, 1, 32, 2), (2, 130, 3, 48, 16), (1, 64, 2, 256, 256),
        (1, 256, 2, 64, 4), (1, 300, 1, 16, 8), (1, 4, 1, 1024, 512), (1, 5, 3, 1024, 1024),
        # beyond the issue's list: 12-lane windows, 260-lane windows, windows over both loads of a lane, over two
        # workgroup steps (ragged and whole), two pieces per batch with a partial second one, 1024 and 2048 windows
        # per piece
        (1, 2, 3, 48, 48), (1, 3, 2, 2080, 1040), (2, 2, 1, 2048, 2048), (2, 9, 5, 272, 16), (1, 3, 2, 4160, 2080),
        (2, 2, 1, 4096, 4096), (1, 3, 2, 8224, 4112), (1, 2, 1, 8192, 8192), (2, 3, 5, 1040, 16), (1, 2, 2, 2048, 4),
        (1, 2, 3, 2048, 2), (1, 3, 5, 1040, 1)]


@functools.lru_cache(maxsize=None)
def voltages(shape):
    """Random full-range bytes, one cube per shape (read as uint8 or int8); never modified."""
    raw = np.random.default_rng(sum(shape)).integers(0, 256, shape + (2, 2), dtype=np.uint8)
    raw.setflags(write=False)
    return raw


def run(context, queue, raw, tint, signed, sum_pols, scale=SCALE, mask=None):
    B, A, C, T = raw.shape[:4]
    tmpl = IncoherentBeamTemplate(context, B, C, T, A, integration=tint, sample_signed=signed, sum_pols=sum_pols,
                                  scale=scale, antenna_mask=mask is not None)
    op = tmpl.instantiate(queue)
    if mask is not None:
        op.set_antenna_mask(mask)
    op.ensure_all_bound()
    op.buffer("inSamples").set(queue, raw.view(np.int8) if signed else raw)
    op()
    out = op.buffer("outData").get(queue)
    assert out.shape == tmpl.output_shape and out.dtype == np.float32
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
@pytest.mark.parametrize("sum_pols", [False, True], ids=["pols", "sum"])
def test_shape_grid(context, command_queue, shape, signed, sum_pols):
    B, A, C, T, tint = shape
    raw = voltages((B, A, C, T))
    got = run(context, command_queue, raw, tint, signed, sum_pols)
    ref = R.incoherent_beam(raw, tint, signed, sum_pols, SCALE)
    np.testing.assert_array_equal(bits(got), bits(ref))
    assert ref.max() > 0


@pytest.mark.parametrize("signed,value,per_sample", [(True, -128, 32768), (False, 255, 130050)], ids=["i8", "u8"])
@pytest.mark.parametrize("sum_pols", [False, True], ids=["pols", "sum"])
def test_full_scale_input(context, command_queue, signed, value, per_sample, sum_pols):
    """Full-scale samples at (1, 256, 1, 256, 256), scale 1/3: window sums of 2^31 (int8, per pol: past int32), 2^32
    (int8, both pols: past uint32) and 130050 * 2^16, 260100 * 2^16 (uint8: past 2^32), so a 32-bit window sum fails.
    These sums have at most 18 significant bits, so float32(S) is exact and a float32 product rounds like the
    contract's float64 one: the check below states that, and test_scaling_is_one_float64_multiply covers the rounding
    with sums of full width."""
    B, A, C, T, tint = 1, 256, 1, 256, 256
    raw = np.full((B, A, C, T, 2, 2), value, np.int8 if signed else np.uint8)
    S = per_sample * A * tint * (2 if sum_pols else 1)
    assert S >= 2 ** 31 and (S >= 2 ** 32 or signed)
    ref = R.incoherent_beam(raw, tint, signed, sum_pols, SCALE)
    assert (R.power_sums(raw, tint, signed, sum_pols) == S).all()
    assert np.float32(S) * np.float32(SCALE) == ref.flat[0]  # no discrimination of the scaling here (docstring)
    got = run(context, command_queue, raw.view(np.uint8), tint, signed, sum_pols)
    np.testing.assert_array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
def test_scaling_is_one_float64_multiply(context, command_queue, signed):
    """Random full-range voltages at (1, 256, 3, 256, 256): window sums near 2^32 with more than 24 significant bits.
    Checked on the CPU first: float32(S) * float32(scale), and a float32 conversion of S before the multiply, give
    other bit patterns than the contract for these values, so a kernel that scales in float32 fails here."""
    B, A, C, T, tint = 1, 256, 3, 256, 256
    raw = voltages((B, A, C, T))
    S = R.power_sums(raw, tint, signed)
    ref = R.scale_sums(S, SCALE)
    f32_product = S.astype(np.float32) * np.float32(SCALE)
    f32_sum_first = (S.astype(np.float32).astype(np.float64) * np.float64(np.float32(SCALE))).astype(np.float32)
    assert (bits(f32_product) != bits(ref)).any() and (bits(f32_sum_first) != bits(ref)).any()
    got = run(context, command_queue, raw, tint, signed, False)
    np.testing.assert_array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("A,masked", [(8200, False), (8200, True), (16600, False)])
def test_many_antennas(context, command_queue, A, masked):
    """More antennas than one 32-bit accumulation run (8192): all-255 uint8 samples, both pols summed, so 16600
    antennas give a per-sample sum of 260100 * 16600 > 2^32; with a mask the antenna list is rebuilt per run."""
    B, C, T, tint = 1, 1, 16, 16
    raw = np.full((B, A, C, T, 2, 2), 255, np.uint8)
    mask = None
    if masked:
        mask = (np.random.default_rng(A).random(A) < 0.7).astype(np.uint8)
        mask[[0, 8191, 8192, A - 1]] = 1, 0, 1, 1
    n = A if mask is None else int(mask.sum())
    got = run(context, command_queue, raw, tint, False, True, scale=1.0, mask=mask)
    ref = R.scale_sums(np.full((B, 1, C, 1), 260100 * n * tint, np.int64), 1.0)
    np.testing.assert_array_equal(bits(got), bits(ref))


MASK_SHAPE = (2, 130, 3, 48, 16)


@pytest.mark.parametrize("kind", ["random", "none", "single", "all"])
@pytest.mark.parametrize("signed,sum_pols", [(False, False), (True, True)], ids=["u8-pols", "i8-sum"])
def test_antenna_mask(context, command_queue, kind, signed, sum_pols):
    B, A, C, T, tint = MASK_SHAPE
    raw = voltages((B, A, C, T))
    mask = {"random": (np.random.default_rng(9).random(A) < 0.5).astype(np.uint8), "none": np.zeros(A, np.uint8),
            "single": (np.arange(A) == 77).astype(np.uint8), "all": np.full(A, 200, np.uint8)}[kind]
    got = run(context, command_queue, raw, tint, signed, sum_pols, mask=mask)
    ref = R.incoherent_beam(raw, tint, signed, sum_pols, SCALE, mask=mask)
    np.testing.assert_array_equal(bits(got), bits(ref))
    if kind == "none":
        assert not bits(got).any()  # exact (positive) zeros
    if kind == "all":
        np.testing.assert_array_equal(bits(got), bits(R.incoherent_beam(raw, tint, signed, sum_pols, SCALE)))


def test_set_antenna_mask_between_launches(context, command_queue):
    """A new mask applies from the next launch on: the first result (read back before the change) is the all-ones
    default's, the second the new mask's, a third launch without a change repeats the second."""
    B, A, C, T, tint = MASK_SHAPE
    raw = voltages((B, A, C, T))
    op = IncoherentBeamTemplate(context, B, C, T, A, integration=tint, scale=SCALE,
                                antenna_mask=True).instantiate(command_queue)
    op.ensure_all_bound()
    op.buffer("inSamples").set(command_queue, raw)
    op()
    first = op.buffer("outData").get(command_queue)
    mask = (np.arange(A) % 3 == 0).astype(np.uint8)
    op.set_antenna_mask(mask)
    np.testing.assert_array_equal(op.antenna_mask(), mask)
    op()
    second = op.buffer("outData").get(command_queue)
    op()
    third = op.buffer("outData").get(command_queue)
    np.testing.assert_array_equal(bits(first), bits(R.incoherent_beam(raw, tint, False, False, SCALE)))
    np.testing.assert_array_equal(bits(second), bits(R.incoherent_beam(raw, tint, False, False, SCALE, mask=mask)))
    np.testing.assert_array_equal(bits(third), bits(second))
    assert (bits(first) != bits(second)).any()


@pytest.mark.parametrize("shape,flags", [((2, 130, 3, 48, 16), 0), ((1, 3, 3, 16, 1), 1), ((1, 3, 5, 48, 2), 2),
                                         ((1, 3, 2, 8224, 4112), 3), ((2, 3, 5, 1040, 16), 1),
                                         ((1, 2, 5, 1040, 4), 0)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"flags{v}")
def test_writes_stay_in_bounds(context, command_queue, shape, flags):
    """The C entry point into an output array longer than the result, the whole array prefilled with a NaN pattern
    (the kernel assumes no zeroed output): the result is exact, the tail untouched, the input cube unchanged."""
    B, A, C, T, tint = shape
    signed, sum_pols = bool(flags & _lib.INCOH_SIGNED), bool(flags & _lib.INCOH_SUM_POLS)
    raw = voltages((B, A, C, T))
    n = B * (1 if sum_pols else 2) * C * (T // tint)
    tail = 4096
    sentinel = np.full(n + tail, 0x7fc0beef, np.uint32)
    d_raw = accel.DeviceArray(context, raw.shape, np.uint8)
    d_out = accel.DeviceArray(context, (n + tail,), np.uint32)
    d_raw.set(command_queue, raw)
    d_out.set(command_queue, sentinel)
    _lib.call("bf_incoherent_beam", d_raw.ptr, None, d_out.ptr, B, C, T, A, tint, flags, SCALE, command_queue.handle)
    out = d_out.get(command_queue)
    ref = R.incoherent_beam(raw, tint, signed, sum_pols, SCALE)
    np.testing.assert_array_equal(out[:n], bits(ref).ravel())
    np.testing.assert_array_equal(out[n:], sentinel[n:])
    np.testing.assert_array_equal(d_raw.get(command_queue), raw)


def test_stream_order_with_the_beamformer(context, command_queue):
    """One inSamples buffer bound to a FusedBeamformer (int8 beams) and an IncoherentBeam, both launched on one queue:
    the beams equal the oracle's integer contract, the incoherent beam the restatement, and a second pair of launches
    gives identical bytes."""
    B, A, M, C, Ctot, T, tint = 2, 64, 16, 4, 4096, 256, 16
    rng = np.random.default_rng(21)
    d1 = np.zeros((1, M, A, 4), np.float32)
    d1[..., 0] = rng.uniform(0, 10 * O.TS_MEERKAT, (M, A))
    d1[..., 2] = rng.uniform(-np.pi, np.pi, (M, A))
    raw8 = voltages((B, A, C, T)).view(np.int8)
    fused = FusedBeamformerTemplate(context, B, C, Ctot, T, A, M, delay_channels=1, sample_signed=True, out_int8=True,
                                    out_scale=1 / 64).instantiate(command_queue)
    incoh = IncoherentBeamTemplate(context, B, C, T, A, integration=tint, sample_signed=True,
                                   scale=SCALE).instantiate(command_queue)
    fused.ensure_all_bound()
    incoh.bind(inSamples=fused.buffer("inSamples"))
    incoh.ensure_all_bound()
    assert incoh.buffer("inSamples") is fused.buffer("inSamples")
    fused.buffer("inSamples").set(command_queue, raw8)
    fused.buffer("delay_vals").set(command_queue, d1)
    runs = []
    for _ in range(2):
        fused()
        incoh()
        runs.append((fused.buffer("outData").get(command_queue), incoh.buffer("outData").get(command_queue)))
        fused.buffer("outData").zero(command_queue)
        incoh.buffer("outData").zero(command_queue)
    q, p = runs[0]
    np.testing.assert_array_equal(q, O.fused_beamform_int8(raw8, d1, Ctot, scale=1 / 64, signed=True))
    np.testing.assert_array_equal(bits(p), bits(R.incoherent_beam(raw8, tint, True, False, SCALE)))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    np.testing.assert_array_equal(fused.buffer("inSamples").get(command_queue), raw8)
