"""Beam detector without a GPU: the feature query, bf_beam_detect's argument validation (fake pointers, as test_abi.py:
validation fails before anything touches a device), the template, the slots, the byte count, and the NumPy restatement
of the contract (detect_ref.py) on inputs with closed-form answers."""
import numpy as np
import pytest

import detect_ref as R
from dpdk_dc_sand_amd import _lib
from dpdk_dc_sand_amd.beamforming import BeamDetectorTemplate, FusedBeamformerTemplate

FAKE = 1 << 20  # 16-byte aligned, never dereferenced


def test_has_feature():
    lib = _lib.load()
    assert lib.bf_has_feature(b"beam_detect") == 1
    assert lib.bf_has_feature(b"incoherent_beam") == 1
    assert lib.bf_has_feature(b"stokes") == 0
    assert lib.bf_has_feature(b"incoherent") == 0
    assert lib.bf_has_feature(b"detect") == 0
    assert lib.bf_has_feature(None) == 0
    assert lib.bf_abi_version() == 302


def call(beams=FAKE, out=FAKE, B=1, C=4, T=16, M=4, tint=16, fint=1, flags=0, scale=1.0):
    return _lib.call("bf_beam_detect", beams, out, B, C, T, M, tint, fint, flags, scale, None)


@pytest.mark.parametrize("kw,match", [
    (dict(beams=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(B=0), "bad shape"),
    (dict(C=0, fint=1), "bad shape"),
    (dict(T=0), "bad shape"),
    (dict(M=0), "bad shape"),
    (dict(T=17, tint=1), "multiple of 16"),
    (dict(T=1 << 21), "above 2\\^20"),
    (dict(M=4097), "above 4096"),
    (dict(tint=0), "time integration"),
    (dict(T=48, tint=5), "time integration"),
    (dict(T=48, tint=32), "time integration"),
    (dict(fint=0), "channel integration"),
    (dict(fint=3), "channel integration"),
    (dict(B=1, C=1 << 12, T=1 << 20, tint=1 << 20, fint=1 << 12), "exceeds 2\\^31"),
    (dict(flags=4), "unknown flags"),
    (dict(flags=-1), "unknown flags"),
    (dict(scale=0.0), "scale"),
    (dict(scale=float("nan")), "scale"),
    (dict(scale=float("inf")), "scale"),
    (dict(scale=-1.0), "scale"),
    (dict(beams=FAKE + 8), "misaligned"),
    (dict(out=FAKE + 2), "misaligned"),
])
def test_argument_validation_without_gpu(kw, match):
    with pytest.raises(_lib.BeamformerError, match=match) as e:
        call(**kw)
    assert e.value.status == -1  # BF_ERR_ARG


def test_template_errors():
    T = BeamDetectorTemplate
    with pytest.raises(ValueError, match="multiple of 16"):
        T(None, 1, 4, 17, 4)
    with pytest.raises(ValueError, match="n_samples_per_channel"):
        T(None, 1, 4, 1 << 21, 4)
    for name, args in (("n_batches", (0, 4, 16, 4)), ("n_channels_per_stream", (1, 0, 16, 4)),
                       ("n_samples_per_channel", (1, 4, 0, 4)), ("n_beams", (1, 4, 16, 0)),
                       ("n_beams", (1, 4, 16, 4097))):
        with pytest.raises(ValueError, match=name):
            T(None, *args)
    for tint in (0, -16, 5, 32):
        with pytest.raises(ValueError, match="time_integration"):
            T(None, 1, 4, 48, 4, time_integration=tint)
    for fint in (0, -1, 3, 8):
        with pytest.raises(ValueError, match="channel_integration"):
            T(None, 1, 4, 48, 4, channel_integration=fint)
    with pytest.raises(ValueError, match="at most"):
        T(None, 1, 1 << 12, 1 << 20, 1, time_integration=1 << 20, channel_integration=1 << 12)
    with pytest.raises(ValueError, match="stokes"):
        T(None, 1, 4, 16, 4, stokes="IQ")
    for scale in (0.0, -2.0, float("nan"), float("inf"), 1e-60):  # 1e-60 is 0 as float32
        with pytest.raises(ValueError, match="scale"):
            T(None, 1, 4, 16, 4, scale=scale)
    for tint in (1, 2, 3, 4, 6, 8, 12, 16, 24, 48):  # any divisor, odd ones included
        T(None, 1, 4, 48, 5, time_integration=tint)
    T(None, 1, 1 << 11, 1 << 20, 4096, time_integration=1 << 20, channel_integration=1 << 11)


def test_template_shapes_and_flags():
    B, C, T, M = 3, 6, 64, 7
    t = BeamDetectorTemplate(None, B, C, T, M)
    assert t.time_integration == 16 and t.channel_integration == 1 and t.stokes == "I" and t.flags == 0
    assert t.input_shape == (B, 2, C, T // 16, 16, 2 * M) and t.output_shape == (B, 1, C, 4, M)
    # the fused operator's output buffer binds to the detector
    assert t.input_shape == FusedBeamformerTemplate(None, B, C, 1024, T, 5, M).output_shape
    t = BeamDetectorTemplate(None, B, C, T, M, time_integration=64, channel_integration=3, stokes="IQUV", in_int8=True,
                             scale=1 / 3)
    assert t.output_shape == (B, 4, 2, 1, M) and t.flags == _lib.DETECT_IN_INT8 | _lib.DETECT_STOKES_IQUV == 3
    assert t.scale == float(np.float32(1 / 3)) and t.n_stokes == 4
    assert BeamDetectorTemplate(None, B, C, T, M, in_int8=True).flags == 1
    assert BeamDetectorTemplate(None, B, C, T, M, stokes="IQUV").flags == 2


def test_operator_slots():
    B, C, T, M = 2, 4, 32, 5
    op = BeamDetectorTemplate(None, B, C, T, M, time_integration=8, channel_integration=2).instantiate(None)
    assert list(op.slots) == ["inBeams", "outData"]
    assert op.slots["inBeams"].dtype == np.float32 and op.slots["inBeams"].shape == (B, 2, C, 2, 16, 2 * M)
    assert op.slots["outData"].dtype == np.float32 and op.slots["outData"].shape == (B, 1, 2, 4, M)
    op = BeamDetectorTemplate(None, B, C, T, M, stokes="IQUV", in_int8=True).instantiate(None)
    assert op.slots["inBeams"].dtype == np.int8 and op.slots["outData"].shape == (B, 4, C, 2, M)
    fused = FusedBeamformerTemplate(None, B, C, 1024, T, 3, M, out_int8=True).instantiate(None)
    assert fused.slots["outData"].shape == op.slots["inBeams"].shape
    assert fused.slots["outData"].dtype == op.slots["inBeams"].dtype


@pytest.mark.parametrize("B,C,T,M,tint,fint", [(8, 4096, 256, 16, 16, 1), (8, 4096, 256, 16, 256, 16),
                                               (2, 3, 48, 17, 3, 3)])
def test_algorithmic_bytes(B, C, T, M, tint, fint):
    lib = _lib.load()
    values, cells = B * 2 * C * T * 2 * M, B * (C // fint) * (T // tint) * M
    assert lib.bf_detect_algorithmic_bytes(B, C, T, M, tint, fint, 0) == 4 * values + 4 * cells
    assert lib.bf_detect_algorithmic_bytes(B, C, T, M, tint, fint, 1) == values + 4 * cells
    assert lib.bf_detect_algorithmic_bytes(B, C, T, M, tint, fint, 2) == 4 * values + 16 * cells
    assert lib.bf_detect_algorithmic_bytes(B, C, T, M, tint, fint, 3) == values + 16 * cells
    for bad in ((0, C, T, M, tint, fint), (B, C, T, -1, tint, fint), (B, C, T, M, 0, fint), (B, C, T, M, tint, 0)):
        assert lib.bf_detect_algorithmic_bytes(*bad, 0) == 0
    t = BeamDetectorTemplate(None, B, C, T, M, time_integration=tint, channel_integration=fint, stokes="IQUV",
                             in_int8=True)
    assert t.algorithmic_bytes() == values + 16 * cells


@pytest.mark.parametrize("M,tint,fint", [(1, 1, 1), (3, 3, 3), (16, 16, 1), (5, 48, 6)])
def test_reference_closed_forms(M, tint, fint):
    """X = 3+4i, Y = 1+2i: I, Q, U, V = 30, 20, 22, -4 per sample."""
    B, C, T = 2, 6, 48
    for dtype in (np.int8, np.float32):
        y = np.empty((B, 2, C, T // 16, 16, M, 2), dtype)
        y[:, 0, ..., 0], y[:, 0, ..., 1], y[:, 1, ..., 0], y[:, 1, ..., 1] = 3, 4, 1, 2
        y = y.reshape(B, 2, C, T // 16, 16, 2 * M)
        S = R.stokes_sums(y, tint, fint)
        assert S.shape == (B, 4, C // fint, T // tint, M) and S.dtype == (np.int64 if dtype == np.int8 else np.float64)
        n = tint * fint
        for s, per_sample in enumerate((30, 20, 22, -4)):
            assert (S[:, s] == per_sample * n).all()
        S1 = R.stokes_sums(y, tint, fint, iquv=False)
        assert S1.shape == (B, 1, C // fint, T // tint, M) and (S1 == 30 * n).all()
        out = R.beam_detect(y, tint, fint, True, 0.5)
        assert out.dtype == np.float32 and (out[:, 3] == -2 * n).all()
    full = np.full((1, 2, 2, 1, 16, 2), -128, np.int8)
    assert (R.stokes_sums(full, 16, 2)[:, 0] == 65536 * 32).all() and (R.stokes_sums(full, 16, 2)[:, 1] == 0).all()


@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_reference_hand_summed_elements(dtype):
    rng = np.random.default_rng(11)
    B, C, T, M, tint, fint = 2, 6, 32, 3, 8, 2
    if dtype == np.int8:
        y = rng.integers(-128, 128, (B, 2, C, T // 16, 16, 2 * M), dtype=np.int8)
    else:
        y = rng.standard_normal((B, 2, C, T // 16, 16, 2 * M)).astype(np.float32)
    S = R.stokes_sums(y, tint, fint)
    v = y.reshape(B, 2, C, T, M, 2)
    b, k, j, m = 1, 2, 3, 1
    want = [0, 0, 0, 0]
    for c in range(k * fint, (k + 1) * fint):
        for t in range(j * tint, (j + 1) * tint):
            xr, xi, yr, yi = (int(q) if dtype == np.int8 else float(q)
                              for q in (v[b, 0, c, t, m, 0], v[b, 0, c, t, m, 1], v[b, 1, c, t, m, 0], v[b, 1, c, t, m, 1]))
            want[0] += xr * xr + xi * xi + yr * yr + yi * yi
            want[1] += xr * xr + xi * xi - yr * yr - yi * yi
            want[2] += 2 * (xr * yr + xi * yi)
            want[3] += 2 * (xi * yr - xr * yi)
    for s in range(4):
        if dtype == np.int8:
            assert S[b, s, k, j, m] == want[s]
        else:
            assert abs(S[b, s, k, j, m] - want[s]) <= 4 * tint * fint * 2.0 ** -53 * want[0]
    np.testing.assert_array_equal(R.stokes_sums(y, tint, fint, iquv=False)[:, 0], S[:, 0])


def test_reference_scale_and_tolerance():
    # one float64 multiply by float32(scale), one rounding
    S = np.array([[[[[65536 * 4096 * 16 + 1]]]]], np.int64)
    out = R.scale_sums(S, 1 / 3)
    assert out.dtype == np.float32
    assert out.flat[0] == np.float32(float(S.flat[0]) * float(np.float32(1 / 3)))
    # the bound: half an ulp of the output plus N * 2^-51 * scale * I
    sums = np.array([100.0, -40.0, 7.0, 0.0]).reshape(1, 4, 1, 1, 1)
    ref = R.scale_sums(sums, 0.5)
    tol = R.tolerance(ref, sums, 16, 2, 0.5)
    assert tol.shape == ref.shape
    np.testing.assert_allclose(tol.ravel(), 2.0 ** -23 * np.abs(ref.ravel().astype(np.float64)) + 128 * 2.0 ** -51 * 50)
