"""GPU: the beam detector (bf_beam_detect, csrc/bf_detect.hip; beamforming.detect) against the NumPy restatement of its
contract (detect_ref.py): bit for bit with int8 beams, within the derived float64 bound (detect_ref.tolerance) with f32
beams.

Shapes are (B, C, T, M, tint, fint), the smallest at which each mechanism of the kernels can break.  A step is 256
lanes x 16 bytes = 512 complex f32 or 2048 complex int8.  Beyond the issue's list:
  partial pieces                       (1, 2, 48, 1, 16, 2): a run of 48 positions in a step of 512 / 2048
  more windows per piece than threads  (1, 1, 4096, 1, 2, 1): 256 (f32) / 1024 (int8) windows in one step
  windows across waves                 (1, 4, 256, 16, 256, 4) (issue): 4096 positions = every wave of 2 / 8 steps
  windows across workgroup steps       (1, 1, 4096, 2, 512, 1): f32 windows of two steps, int8 two windows per step
  a load straddling two windows        (1, 1, 16, 1, 1, 1), (1, 2, 32, 2, 2, 1) (issue), (1, 1, 48, 4, 3, 1)
  M above a step, power of two         (1, 1, 16, 1024, 2, 1) f32, (1, 1, 16, 4096, 4, 1) int8 too: column blocks,
                                       steps of whole rows
  period walk (M or tint no power of two, lcm(M, E) within a step): (2, 3, 48, 3, 3, 3), (2, 6, 48, 17, 16, 2),
      (1, 2, 1024, 3, 64, 1), (1, 5, 64, 65, 4, 5) (issue: windows open over several periods, a partial last period),
      (1, 1, 32, 300, 8, 1) (one row per period f32, six int8), (1, 1, 48, 512, 3, 1) (M = the f32 step)
  rows walk (lcm(M, E) above a step)   (1, 1, 16, 1025, 4, 1): rows that start inside a load, three beam blocks, fewer
      rows than row classes (int8); (1, 2, 16, 513, 16, 2): several rows per class and two channels
  short runs side by side in one step (2, 9, 64, 1, 16, 1): 8 (f32) / 32 (int8) channel groups per step, 9 groups, so
      a partial last block; (1, 40, 16, 2, 4, 2): the same with channel integration
  64-bit LDS slots (int8, more than 2048 loads per lane) (1, 4128, 16, 1, 16, 2064), summed across two lanes
  32-bit runs of the int8 sums         test_long_channel_run_int8: 16400 loads per lane, past the 2^14-load flush."""
import functools

import numpy as np
import pytest

import detect_ref as R
import oracle as O
from dpdk_dc_sand_amd import _lib, accel
from dpdk_dc_sand_amd.beamforming import BeamDetectorTemplate, FusedBeamformerTemplate

pytestmark = pytest.mark.gpu

SCALE = 1 / 3  # not a power of two: the float64 product's rounding matters

GRID = [(1, 1, 16, 1, 1, 1), (1, 1, 16, 1, 16, 1), (2, 3, 48, 3, 3, 3), (1, 2, 32, 2, 2, 1), (2, 6, 48, 17, 16, 2),
        (1, 4, 256, 16, 256, 4), (1, 2, 1024, 3, 64, 1), (1, 5, 64, 65, 4, 5), (1, 3, 4096, 1, 4096, 3),
        (1, 2, 2048, 1, 8, 2), (2, 1, 16, 64, 1, 1),
        # beyond the issue's list (module docstring)
        (1, 2, 48, 1, 16, 2), (1, 1, 4096, 1, 2, 1), (1, 1, 4096, 2, 512, 1), (1, 1, 48, 4, 3, 1),
        (1, 1, 16, 1024, 2, 1), (1, 1, 16, 4096, 4, 1), (1, 1, 32, 300, 8, 1), (1, 1, 48, 512, 3, 1),
        (1, 1, 16, 1025, 4, 1), (1, 2, 16, 513, 16, 2), (2, 9, 64, 1, 16, 1), (1, 40, 16, 2, 4, 2),
        (1, 4128, 16, 1, 16, 2064)]


def ident(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


@functools.lru_cache(maxsize=None)
def beams(shape, int8):
    """One cube per (B, C, T, M) and dtype, never modified: random full-range bytes, or Gaussian f32 of rms 1000."""
    B, C, T, M = shape
    rng = np.random.default_rng(sum(shape) + int8)
    full = (B, 2, C, T // 16, 16, 2 * M)
    y = rng.integers(-128, 128, full, dtype=np.int8) if int8 else (1000 * rng.standard_normal(full)).astype(np.float32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def reference(shape, int8, tint, fint):
    """(float64 or int64 IQUV sums, scaled float32 output) of beams(shape, int8); shared, never modified."""
    S = R.stokes_sums(beams(shape, int8), tint, fint)
    out = R.scale_sums(S, SCALE)
    S.setflags(write=False)
    out.setflags(write=False)
    return S, out


def run(context, queue, y, tint, fint, iquv, scale=SCALE):
    B, _, C, nb, _, M2 = y.shape
    tmpl = BeamDetectorTemplate(context, B, C, nb * 16, M2 // 2, time_integration=tint, channel_integration=fint,
                                stokes="IQUV" if iquv else "I", in_int8=y.dtype == np.int8, scale=scale)
    op = tmpl.instantiate(queue)
    op.ensure_all_bound()
    op.buffer("inBeams").set(queue, y)
    op()
    out = op.buffer("outData").get(queue)
    assert out.shape == tmpl.output_shape and out.dtype == np.float32
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(got, S, ref, int8, tint, fint, iquv, scale=SCALE):
    """Every element: bit for bit (int8), or within the derived bound (f32)."""
    ns = 4 if iquv else 1
    if int8:
        np.testing.assert_array_equal(bits(got), bits(ref[:, :ns]))
    else:
        tol = R.tolerance(ref, S, tint, fint, scale)[:, :ns]
        err = np.abs(got.astype(np.float64) - ref[:, :ns].astype(np.float64))
        assert np.isfinite(got).all() and (err <= tol).all(), (float((err / tol).max()), int((err > tol).sum()))


@pytest.mark.parametrize("shape", GRID, ids=ident)
@pytest.mark.parametrize("int8", [True, False], ids=["i8", "f32"])
@pytest.mark.parametrize("iquv", [False, True], ids=["I", "IQUV"])
def test_shape_grid(context, command_queue, shape, int8, iquv):
    B, C, T, M, tint, fint = shape
    y = beams((B, C, T, M), int8)
    S, ref = reference((B, C, T, M), int8, tint, fint)
    assert ref.any()
    got = run(context, command_queue, y, tint, fint, iquv)
    check(got, S, ref, int8, tint, fint, iquv)


FULL_SCALE = {  # (Xr, Xi, Yr, Yi) -> the Stokes term whose window sum reaches 2^31 (I: 2^32), and its sign
    "I": ((-128, -128, -128, -128), 0, 1), "+Q": ((-128, -128, 0, 0), 1, 1), "-Q": ((0, 0, -128, -128), 1, -1),
    "+U": ((-128, -128, -128, -128), 2, 1), "-U": ((-128, -128, 127, 127), 2, -1),
    "+V": ((-128, -128, -128, 127), 3, 1), "-V": ((-128, -128, 127, -128), 3, -1)}


@pytest.mark.parametrize("case", list(FULL_SCALE))
def test_full_scale_int8(context, command_queue, case):
    """Constant int8 beams at (1, 16, 4096, 1, 4096, 16): 2^16 samples per window, so the named term's window sum has
    magnitude >= 2^31 (I: 2^32) and a 32-bit sum anywhere in the kernel fails."""
    B, C, T, M, tint, fint = 1, 16, 4096, 1, 4096, 16
    (xr, xi, yr, yi), s, sign = FULL_SCALE[case]
    y = np.empty((B, 2, C, T // 16, 16, M, 2), np.int8)
    y[:, 0, ..., 0], y[:, 0, ..., 1], y[:, 1, ..., 0], y[:, 1, ..., 1] = xr, xi, yr, yi
    y = y.reshape(B, 2, C, T // 16, 16, 2 * M)
    S = R.stokes_sums(y, tint, fint)
    assert S.shape == (1, 4, 1, 1, 1)
    assert sign * int(S[0, s, 0, 0, 0]) >= (2 ** 32 if case == "I" else 2 ** 31)
    ref = R.scale_sums(S, SCALE)
    got = run(context, command_queue, y, tint, fint, True)
    np.testing.assert_array_equal(bits(got), bits(ref))
    np.testing.assert_array_equal(bits(run(context, command_queue, y, tint, fint, False)), bits(ref[:, :1]))


def test_long_channel_run_int8(context, command_queue):
    """All -128 at (1, 16400, 16, 1, 16, 16400): a lane adds 16400 loads, more than one 32-bit run (2^14 loads), and
    the window sums I = U = 65536 * 16 * 16400 > 2^34, Q = V = 0."""
    B, C, T, M, tint, fint = 1, 16400, 16, 1, 16, 16400
    y = np.full((B, 2, C, T // 16, 16, 2 * M), -128, np.int8)
    n = 65536 * tint * fint
    ref = R.scale_sums(np.array([n, 0, n, 0], np.int64).reshape(1, 4, 1, 1, 1), SCALE)
    got = run(context, command_queue, y, tint, fint, True)
    np.testing.assert_array_equal(bits(got), bits(ref))
    np.testing.assert_array_equal(bits(run(context, command_queue, y, tint, fint, False)), bits(ref[:, :1]))


def test_scaling_is_one_float64_multiply(context, command_queue):
    """Random int8 beams at (1, 4, 256, 16, 256, 4): the I sums exceed 2^24, so float32(S) * float32(scale) gives other
    bits than the contract somewhere (checked on the CPU first) and a kernel that scales in float32 fails."""
    shape, tint, fint = (1, 4, 256, 16), 256, 4
    y = beams(shape, True)
    S, ref = reference(shape, True, tint, fint)
    assert S[:, 0].min() > 2 ** 24
    assert (bits(S.astype(np.float32) * np.float32(SCALE)) != bits(ref)).any()
    got = run(context, command_queue, y, tint, fint, True)
    np.testing.assert_array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("shape", [(1, 4, 256, 16, 256, 4), (1, 2, 1024, 3, 64, 1)], ids=ident)
def test_float_accumulation_is_float64(context, command_queue, shape):
    """f32 beams: a float32 accumulation of the same (float64-exact) terms violates the tolerance for a large share of
    the Q, U and V elements -- checked on the CPU first -- while a float64 sum in another order violates it for none;
    then the GPU result meets the tolerance."""
    B, C, T, M, tint, fint = shape
    y = beams((B, C, T, M), False)
    S, ref = reference((B, C, T, M), False, tint, fint)
    tol = R.tolerance(ref, S, tint, fint, SCALE)
    v = y.reshape(B, 2, C // fint, fint, T // tint, tint, M, 2).astype(np.float64)
    xr, xi, yr, yi = v[:, 0, ..., 0], v[:, 0, ..., 1], v[:, 1, ..., 0], v[:, 1, ..., 1]
    terms = np.stack([xr * xr + xi * xi + yr * yr + yi * yi, xr * xr + xi * xi - yr * yr - yi * yi,
                      2 * (xr * yr + xi * yi), 2 * (xi * yr - xr * yi)], axis=1)  # (B, 4, K, fint, J, tint, M)
    acc32 = np.zeros((B, 4, C // fint, T // tint, M), np.float32)
    for f in range(fint):
        for t in range(tint):
            acc32 += terms[:, :, :, f, :, t].astype(np.float32)
    out32 = (acc32.astype(np.float64) * np.float64(np.float32(SCALE))).astype(np.float32)
    bad = np.abs(out32.astype(np.float64) - ref) > tol
    assert bad[:, 1:].mean() > 0.4 and bad[:, 0].mean() > 0.1, (bad[:, 1:].mean(), bad[:, 0].mean())
    other = terms[:, :, :, ::-1, :, ::-1].sum(axis=(3, 5))  # float64, reversed order
    out64 = (other * np.float64(np.float32(SCALE))).astype(np.float32)
    assert not (np.abs(out64.astype(np.float64) - ref) > tol).any()
    got = run(context, command_queue, y, tint, fint, True)
    check(got, S, ref, False, tint, fint, True)


@pytest.mark.parametrize("shape", [(2, 6, 48, 17, 16, 2), (1, 5, 64, 65, 4, 5)], ids=ident)
@pytest.mark.parametrize("int8", [True, False], ids=["i8", "f32"])
def test_writes_stay_in_bounds(context, command_queue, shape, int8):
    """The C entry point into an output array longer than the result, the whole array prefilled with a NaN pattern
    (the kernel assumes no zeroed output): the result is correct, the tail untouched, the input cube unchanged."""
    B, C, T, M, tint, fint = shape
    y = beams((B, C, T, M), int8)
    S, ref = reference((B, C, T, M), int8, tint, fint)
    n, tail = ref.size, 4096
    sentinel = np.full(n + tail, 0x7fc0beef, np.uint32)
    d_in = accel.DeviceArray(context, y.shape, y.dtype)
    d_out = accel.DeviceArray(context, (n + tail,), np.uint32)
    d_in.set(command_queue, y)
    d_out.set(command_queue, sentinel)
    flags = _lib.DETECT_STOKES_IQUV | (_lib.DETECT_IN_INT8 if int8 else 0)
    _lib.call("bf_beam_detect", d_in.ptr, d_out.ptr, B, C, T, M, tint, fint, flags, SCALE, command_queue.handle)
    out = d_out.get(command_queue)
    check(out[:n].view(np.float32).reshape(ref.shape), S, ref, int8, tint, fint, True)
    np.testing.assert_array_equal(out[n:], sentinel[n:])
    np.testing.assert_array_equal(d_in.get(command_queue), y)


@pytest.mark.parametrize("int8", [True, False], ids=["i8", "f32"])
def test_bound_to_the_beamformer(context, command_queue, int8):
    """A FusedBeamformer's outData bound to a BeamDetector (tint 16, fint 2, IQUV), both launched on one queue.  int8
    beams: the detector output equals detect_ref of the oracle's integer contract, bit for bit; f32 beams: detect_ref of
    the beams read back, within the tolerance.  A second pair of launches gives identical bytes."""
    B, A, M, C, Ctot, T, tint, fint = 2, 64, 16, 4, 4096, 256, 16, 2
    rng = np.random.default_rng(21)
    d1 = np.zeros((1, M, A, 4), np.float32)
    d1[..., 0] = rng.uniform(0, 10 * O.TS_MEERKAT, (M, A))
    d1[..., 2] = rng.uniform(-np.pi, np.pi, (M, A))
    raw8 = rng.integers(-128, 128, (B, A, C, T, 2, 2), dtype=np.int8)
    fused = FusedBeamformerTemplate(context, B, C, Ctot, T, A, M, delay_channels=1, sample_signed=True, out_int8=int8,
                                    out_scale=1 / 64 if int8 else 1.0).instantiate(command_queue)
    det = BeamDetectorTemplate(context, B, C, T, M, time_integration=tint, channel_integration=fint, stokes="IQUV",
                               in_int8=int8, scale=SCALE).instantiate(command_queue)
    fused.ensure_all_bound()
    det.bind(inBeams=fused.buffer("outData"))
    det.ensure_all_bound()
    assert det.buffer("inBeams") is fused.buffer("outData")
    fused.buffer("inSamples").set(command_queue, raw8)
    fused.buffer("delay_vals").set(command_queue, d1)
    runs = []
    for _ in range(2):
        fused()
        det()
        runs.append((fused.buffer("outData").get(command_queue), det.buffer("outData").get(command_queue)))
        fused.buffer("outData").zero(command_queue)
        det.buffer("outData").zero(command_queue)
    y, got = runs[0]
    if int8:
        np.testing.assert_array_equal(y, O.fused_beamform_int8(raw8, d1, Ctot, scale=1 / 64, signed=True))
    assert y.any()
    S = R.stokes_sums(y, tint, fint)
    check(got, S, R.scale_sums(S, SCALE), int8, tint, fint, True)
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
