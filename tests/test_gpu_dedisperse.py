"""GPU: the dedisperser (bf_dedisperse, csrc/bf_dedisperse.hip; beamforming.dedisperse) against the NumPy restatement
of its contract (dedisperse_ref.py): bit for bit on integer-valued power, within the derived float64 bound
(dedisperse_ref.tolerance) on Gaussian power, and the ring after the call bit for bit.

The C entry point takes the ring and `head` explicitly, so one call on a random prefilled ring exercises wrapping: every
shape runs at head = 0 (reads wrap to the ring's end) and head = R - N, with two lag tables: "mixed" (random lags in
[0, R - N], row 0 all 0 and row 1 all R - N where D >= 3) and "alternating" (rows of all 0 and all R - N in turn).

Shapes are (B, S, plane, K, J, M, D, R).  A workgroup owns 64 positions e = n*M + m and 8 trials; its 16 waves take the
channels in chunks of 4, chunk q to wave q % 16, two chunks per turn of the loop, and add their partial sums at the end.
Beyond the issue's list:
  one full position tile                    (1,1,0, 3,16,4,3, 64): N*M = 64 exactly, one chunk: fifteen waves have nothing
  a partial second tile, two trial tiles    (1,1,0, 3,65,1,9, 130): N*M = 65, D = 9, element accesses in the append
  three chunks per wave                     (1,1,0, 192,8,5,3, 24): an odd number of chunks per wave (the loop's second half
                                            is skipped in the last turn)
  uneven waves, a partial last chunk        (1,1,0, 197,8,5,9, 24): 50 chunks, waves 0 and 1 walk four, the others three;
                                            the last chunk holds one channel"""
import functools

import numpy as np
import pytest

import dedisperse_ref as R
import detect_ref
import oracle as O
from dpdk_dc_sand_amd import _lib, accel
from dpdk_dc_sand_amd.beamforming import BeamDetectorTemplate, DedisperserTemplate, FusedBeamformerTemplate

pytestmark = pytest.mark.gpu

SCALE = 1 / 3  # not a power of two: the float64 product's rounding matters

GRID = [(1, 1, 0, 1, 1, 1, 1, 1), (1, 1, 0, 3, 4, 1, 2, 12), (2, 4, 2, 5, 8, 3, 3, 48), (1, 1, 0, 64, 16, 16, 8, 64),
        (1, 1, 0, 7, 16, 17, 5, 160), (1, 1, 0, 4, 2, 65, 2, 8), (1, 1, 0, 8, 16, 1024, 2, 32),
        (1, 1, 0, 16, 256, 16, 33, 1024), (2, 1, 0, 512, 16, 4, 4, 96), (1, 1, 0, 4, 32, 4, 8, 4128),
        # beyond the issue's list (module docstring)
        (1, 1, 0, 3, 16, 4, 3, 64), (1, 1, 0, 3, 65, 1, 9, 130), (1, 1, 0, 192, 8, 5, 3, 24),
        (1, 1, 0, 197, 8, 5, 9, 24)]


def ident(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def inputs(shape, integer):
    """(power, prefilled ring) of a shape, never modified: integers below 2^12 (the sums stay below 2^24), or Gaussian
    f32 of rms 1000."""
    B, S, plane, K, J, M, D, Rn = shape
    rng = np.random.default_rng(sum(shape) + integer)
    if integer:
        power = rng.integers(0, 1 << 12, (B, S, K, J, M)).astype(np.float32)
        ring = rng.integers(0, 1 << 12, (K, Rn, M)).astype(np.float32)
    else:
        power = (1000 * rng.standard_normal((B, S, K, J, M))).astype(np.float32)
        ring = (1000 * rng.standard_normal((K, Rn, M))).astype(np.float32)
    power.setflags(write=False)
    ring.setflags(write=False)
    return power, ring


@functools.lru_cache(maxsize=None)
def table(shape, kind):
    B, S, plane, K, J, M, D, Rn = shape
    top = Rn - B * J
    if kind == "alternating":
        lags = np.where(np.arange(D)[:, None] % 2 == 0, 0, top) * np.ones((1, K), np.int64)
    else:
        lags = np.random.default_rng(sum(shape)).integers(0, top + 1, (D, K))
        if D >= 3:
            lags[0], lags[1] = 0, top
    lags = lags.astype(np.int32)
    lags.setflags(write=False)
    return lags


@functools.lru_cache(maxsize=None)
def reference(shape, integer, kind, head):
    """(out, |x| sums, ring after) of one call; shared, never modified."""
    B, S, plane, K, J, M, D, Rn = shape
    power, ring = inputs(shape, integer)
    new = R.append(power, ring, head, plane)
    acc, absacc = R.channel_sums(new, table(shape, kind), head, B * J)
    out = R.scale_sums(acc, SCALE)
    for a in (out, absacc, new):
        a.setflags(write=False)
    return out, absacc, new


def launch(context, queue, power, ring, lags, head, plane, scale=SCALE, tail=0, sentinel=0x7fc0beef):
    """bf_dedisperse on device copies: (the whole out array as uint32, ring, power, lags read back)."""
    B, S, K, J, M = power.shape
    D, Rn = lags.shape[0], ring.shape[1]
    n = M * D * B * J
    d_power = accel.DeviceArray(context, power.shape, np.float32)
    d_ring = accel.DeviceArray(context, ring.shape, np.float32)
    d_lags = accel.DeviceArray(context, lags.shape, np.int32)
    d_out = accel.DeviceArray(context, (n + tail,), np.uint32)
    d_power.set(queue, power)
    d_ring.set(queue, ring)
    d_lags.set(queue, lags)
    d_out.set(queue, np.full(n + tail, sentinel, np.uint32))  # the kernel assumes no zeroed output
    _lib.call("bf_dedisperse", d_power.ptr, d_ring.ptr, d_lags.ptr, d_out.ptr, B, S, plane, K, J, M, D, Rn, head,
              scale, queue.handle)
    return d_out.get(queue), d_ring.get(queue), d_power.get(queue), d_lags.get(queue)


def check(got, ref, absacc, K, integer, scale=SCALE):
    """Every element: bit for bit (integer-valued power), or within the derived bound."""
    got = got.view(np.float32).reshape(ref.shape)
    if integer:
        np.testing.assert_array_equal(bits(got), bits(ref))
    else:
        tol = R.tolerance(ref, absacc, K, scale)
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        assert np.isfinite(got).all() and (err <= tol).all(), (float((err / tol).max()), int((err > tol).sum()))


@pytest.mark.parametrize("shape", GRID, ids=ident)
@pytest.mark.parametrize("integer", [True, False], ids=["int", "gauss"])
@pytest.mark.parametrize("kind", ["mixed", "alternating"])
@pytest.mark.parametrize("at", ["head0", "headlast"])
def test_shape_grid(context, command_queue, shape, integer, kind, at):
    B, S, plane, K, J, M, D, Rn = shape
    head = 0 if at == "head0" else Rn - B * J
    power, ring = inputs(shape, integer)
    ref, absacc, ring_ref = reference(shape, integer, kind, head)
    assert ref.any()
    out, ring_got, _, _ = launch(context, command_queue, power, ring, table(shape, kind), head, plane)
    check(out, ref, absacc, K, integer)
    np.testing.assert_array_equal(bits(ring_got), bits(ring_ref))


def test_lags_out_of_range_are_clamped(context, command_queue):
    """A device table with -1, R - N + 1 and 2^31 - 1 (and -2^31) at (2,4,2, 5,8,3,3, 48) gives the reference's result
    for the clamped table: the ring is K*R*M floats and every index is reduced into it."""
    shape = (2, 4, 2, 5, 8, 3, 3, 48)
    B, S, plane, K, J, M, D, Rn = shape
    lags = table(shape, "mixed").copy()
    lags[0, 1], lags[1, 2], lags[2, 0], lags[2, 4], lags[0, 3] = -1, Rn - B * J + 1, 2 ** 31 - 1, -2 ** 31, 2 ** 30
    clamped = R.clamp_lags(lags, Rn, B * J).astype(np.int32)
    assert (clamped != lags).sum() == 5
    power, ring = inputs(shape, True)
    ref, ring_ref = R.dedisperse(power, ring, clamped, 16, plane, SCALE)
    out, ring_got, _, lags_got = launch(context, command_queue, power, ring, lags, 16, plane)
    np.testing.assert_array_equal(bits(out.view(np.float32).reshape(ref.shape)), bits(ref))
    np.testing.assert_array_equal(bits(ring_got), bits(ring_ref))
    np.testing.assert_array_equal(lags_got, lags)


@pytest.mark.parametrize("shape", [(2, 4, 2, 5, 8, 3, 3, 48), (1, 1, 0, 7, 16, 17, 5, 160),
                                   (1, 1, 0, 3, 65, 1, 9, 130)], ids=ident)
def test_writes_stay_in_bounds(context, command_queue, shape):
    """The C entry point into an output array longer than the result, the whole array prefilled with a NaN pattern: the
    result is correct and the tail untouched; ring slots outside [head, head + N) are unchanged; power and lags are
    unchanged."""
    B, S, plane, K, J, M, D, Rn = shape
    N, tail = B * J, 4096
    head = N * ((Rn // N) // 2)
    power, ring = inputs(shape, True)
    lags = table(shape, "mixed")
    ref, ring_ref = R.dedisperse(power, ring, lags, head, plane, SCALE)
    out, ring_got, power_got, lags_got = launch(context, command_queue, power, ring, lags, head, plane, tail=tail)
    np.testing.assert_array_equal(bits(out[:ref.size].view(np.float32).reshape(ref.shape)), bits(ref))
    assert (out[ref.size:] == 0x7fc0beef).all()
    outside = np.ones(Rn, bool)
    outside[head:head + N] = False
    np.testing.assert_array_equal(bits(ring_got[:, outside]), bits(ring[:, outside]))
    np.testing.assert_array_equal(bits(ring_got), bits(ring_ref))
    np.testing.assert_array_equal(bits(power_got), bits(power))
    np.testing.assert_array_equal(lags_got, lags)


@pytest.mark.parametrize("signed", [False, True], ids=["positive", "signed"])
def test_float_accumulation(context, command_queue, signed):
    """(2,1,0, 512,16,4,4, 96), Gaussian fill, signed and squared (positive power): the 512-channel sums meet the
    tolerance that a float32 accumulation breaks for most elements (test_dedisperse_host.py)."""
    shape = (2, 1, 0, 512, 16, 4, 4, 96)
    B, S, plane, K, J, M, D, Rn = shape
    power, ring = inputs(shape, False)
    if not signed:
        power, ring = (power * power).astype(np.float32), (ring * ring).astype(np.float32)
    lags = table(shape, "mixed")
    new = R.append(power, ring, 64, plane)
    acc, absacc = R.channel_sums(new, lags, 64, B * J)
    out, ring_got, _, _ = launch(context, command_queue, power, ring, lags, 64, plane)
    check(out, R.scale_sums(acc, SCALE), absacc, K, False)
    np.testing.assert_array_equal(bits(ring_got), bits(new))


def test_operator_over_calls(context, command_queue):
    """Dedisperser called 7 times at (1,1,0, 6,8,4,4, 32): the calls wrap the ring, the concatenated output equals the
    one-shot reference of the concatenated input, and after reset() a second run reproduces the first run's bytes."""
    B, K, J, M, D, Rn, calls = 1, 6, 8, 4, 4, 32, 7
    N = B * J
    rng = np.random.default_rng(11)
    lags = rng.integers(0, Rn - N + 1, (D, K)).astype(np.int32)
    lags[0], lags[1] = 0, Rn - N
    power = rng.integers(0, 1 << 12, (calls, B, 1, K, J, M)).astype(np.float32)
    tmpl = DedisperserTemplate(context, B, K, J, M, lags, ring_length=Rn, scale=SCALE)
    op = tmpl.instantiate(command_queue)
    op.ensure_all_bound()
    runs = []
    for _ in range(2):
        outs = []
        for c in range(calls):
            assert op.head == c * N % Rn and op.samples_seen == c * N
            op.buffer("inPower").set(command_queue, power[c])
            op()
            outs.append(op.buffer("outData").get(command_queue))
        runs.append(np.concatenate(outs, axis=2))
        assert op.samples_seen == calls * N > Rn
        op.reset()
        assert op.head == 0 and op.samples_seen == 0
    stream = power[:, :, 0].transpose(2, 0, 1, 3, 4).reshape(K, calls * N, M)
    ref = R.one_shot(stream, lags, SCALE)
    np.testing.assert_array_equal(bits(runs[0]), bits(ref))
    assert runs[0].tobytes() == runs[1].tobytes()


def test_bound_to_the_chain(context, command_queue):
    """FusedBeamformer(out_int8) -> BeamDetector(tint 16, fint 2, IQUV, scale 1) -> Dedisperser(plane 0) at A = 64,
    M = 16, C = 4, T = 256, B = 2 on one queue, the slots bound, not copied.  Two calls on two voltage cubes: the output
    equals dedisperse_ref of detect_ref of the oracle's int8 beams, bit for bit; after reset() the pair of calls gives
    identical bytes."""
    B, A, M, C, Ctot, T, tint, fint, D = 2, 64, 16, 4, 4096, 256, 16, 2, 5
    K, J = C // fint, T // tint
    N = B * J
    rng = np.random.default_rng(23)
    d1 = np.zeros((1, M, A, 4), np.float32)
    d1[..., 0] = rng.uniform(0, 10 * O.TS_MEERKAT, (M, A))
    d1[..., 2] = rng.uniform(-np.pi, np.pi, (M, A))
    raw = rng.integers(-128, 128, (2, B, A, C, T, 2, 2), dtype=np.int8)
    lags = rng.integers(0, N + 1, (D, K)).astype(np.int32)
    lags[0], lags[1] = 0, N
    fused = FusedBeamformerTemplate(context, B, C, Ctot, T, A, M, delay_channels=1, sample_signed=True, out_int8=True,
                                    out_scale=1 / 64).instantiate(command_queue)
    det = BeamDetectorTemplate(context, B, C, T, M, time_integration=tint, channel_integration=fint, stokes="IQUV",
                               in_int8=True, scale=1.0).instantiate(command_queue)
    tmpl = DedisperserTemplate(context, B, K, J, M, lags, n_stokes=4, plane=0, scale=SCALE)
    assert tmpl.ring_length == 2 * N
    ded = tmpl.instantiate(command_queue)
    fused.ensure_all_bound()
    det.bind(inBeams=fused.buffer("outData"))
    det.ensure_all_bound()
    ded.bind(inPower=det.buffer("outData"))
    ded.ensure_all_bound()
    assert det.buffer("inBeams") is fused.buffer("outData") and ded.buffer("inPower") is det.buffer("outData")
    fused.buffer("delay_vals").set(command_queue, d1)
    runs = []
    for _ in range(2):
        outs = []
        for c in range(2):
            fused.buffer("inSamples").set(command_queue, raw[c])
            fused()
            det()
            ded()
            outs.append(ded.buffer("outData").get(command_queue))
            ded.buffer("outData").zero(command_queue)
        runs.append(outs)
        ded.reset()
    ring, head = np.zeros(tmpl.ring_shape, np.float32), 0
    for c in range(2):
        y = O.fused_beamform_int8(raw[c], d1, Ctot, scale=1 / 64, signed=True)
        power = detect_ref.beam_detect(y, tint, fint, iquv=True, scale=1.0)
        assert power.shape == tmpl.input_shape and power[:, 0].any() and power[:, 0].max() < 2 ** 23
        ref, ring = R.dedisperse(power, ring, lags, head, 0, SCALE)
        head = (head + N) % tmpl.ring_length
        np.testing.assert_array_equal(bits(runs[0][c]), bits(ref))
    for c in range(2):
        assert runs[0][c].tobytes() == runs[1][c].tobytes()
