"""The correlator without a GPU: the feature query, bf_correlate's argument validation (fake pointers, as test_abi.py:
validation fails before anything touches a device), the byte count, the template, the baseline helpers, the accumulate
counter, and the NumPy restatement of the contract (correlate_ref.py) on inputs with closed-form answers, its Hermitian
property, and its autos against the incoherent beam's and the voltage statistics' restatements."""
import numpy as np
import pytest

import correlate_ref as R
import incoherent_ref as IR
import vstats_ref as VR
from dpdk_dc_sand_amd import _lib
from dpdk_dc_sand_amd.beamforming import (CorrelatorTemplate, FusedBeamformerTemplate, baseline_index, n_baselines,
                                          visibility_matrix)

FAKE = 1 << 20  # 16-byte aligned, never dereferenced
SIGNED, ACC = 1, 2


def test_has_feature():
    lib = _lib.load()
    assert lib.bf_has_feature(b"correlate") == 1
    assert lib.bf_has_feature(b"correlator") == 0
    assert lib.bf_has_feature(b"voltage_stats") == 1
    assert lib.bf_abi_version() == 302
    assert (_lib.CORR_SIGNED, _lib.CORR_ACCUMULATE) == (SIGNED, ACC)


def call(raw=FAKE, out=FAKE, B=1, C=4, T=16, A=4, tint=16, bint=1, flags=0):
    return _lib.call("bf_correlate", raw, out, B, C, T, A, tint, bint, flags, None)


REFUSALS = [
    (dict(raw=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(B=0), "bad shape"),
    (dict(C=0), "bad shape"),
    (dict(T=0), "bad shape"),
    (dict(A=0), "antennas"),
    (dict(A=2049), "antennas"),
    (dict(T=17), "multiple of 16"),
    (dict(T=1 << 21, tint=16), "bad shape"),
    (dict(T=48, tint=8), "integration"),       # not a multiple of 16
    (dict(T=48, tint=24), "integration"),
    (dict(T=48, tint=32), "integration"),      # does not divide T
    (dict(tint=0), "integration"),
    (dict(tint=-16), "integration"),
    (dict(bint=0), "batch integration"),
    (dict(B=4, bint=3), "batch integration"),  # does not divide B
    (dict(B=4, T=32, tint=16, bint=2), "batch integration above 1"),
    (dict(flags=4), "unknown flags"),
    (dict(flags=8 | SIGNED), "unknown flags"),
    (dict(flags=-1), "unknown flags"),
    # the int32 bounds, at n + 16 (n itself is accepted: test_int32_bounds_at_n)
    (dict(B=3, T=21840, tint=21840, bint=3, flags=SIGNED), None),                      # n = 65520: accepted
    (dict(B=1, T=65536, tint=65536, flags=SIGNED), "int32 bound"),                     # 65520 + 16
    (dict(B=4, T=16384, tint=16384, bint=4, flags=SIGNED), "int32 bound"),             # the same through bint
    (dict(T=16512, tint=16512), None),                                                 # n = 16512: accepted
    (dict(T=16528, tint=16528), "int32 bound"),
    (dict(B=3, T=5520, tint=5520, bint=3), "int32 bound"),                             # 16560 through bint
    (dict(T=16528, tint=16528, flags=ACC), "int32 bound"),
    (dict(raw=FAKE + 8), "misaligned"),
    (dict(raw=FAKE + 1), "misaligned"),
    (dict(out=FAKE + 2), "misaligned"),
    (dict(out=FAKE + 1), "misaligned"),
    (dict(B=1 << 20, C=1 << 20, T=16, A=1), "grid limit"),
    (dict(B=1, C=1 << 14, T=1 << 20, tint=16, A=2048), "grid limit"),
]


@pytest.mark.parametrize("kw,match", [r for r in REFUSALS if r[1]], ids=lambda v: None if isinstance(v, dict) else v)
def test_argument_validation_without_gpu(kw, match):
    lib = _lib.load()
    before = lib.bf_last_kernel()
    with pytest.raises(_lib.BeamformerError, match=match) as e:
        call(**kw)
    assert e.value.status == -1  # BF_ERR_ARG
    assert lib.bf_last_kernel() == before  # refused before any launch
    assert "bf_correlate" in _lib.last_error()
    args = {**dict(B=1, C=4, T=16, A=4, tint=16, bint=1, flags=0), **{k: v for k, v in kw.items() if k not in
                                                                       ("raw", "out")}}
    if "raw" not in kw and "out" not in kw:  # what the entry point refuses for its shape, the byte count calls 0
        assert lib.bf_correlate_algorithmic_bytes(*(args[k] for k in ("B", "C", "T", "A", "tint", "bint",
                                                                      "flags"))) == 0


@pytest.mark.parametrize("kw", [r[0] for r in REFUSALS if r[1] is None], ids=["int8-65520", "uint8-16512"])
def test_int32_bounds_at_n(kw):
    """The largest windows of the two conventions pass every shape check: the byte count (0 for anything the entry
    point would refuse) is positive, and with a misaligned output, the check that follows the shape, that is what the
    call reports."""
    lib = _lib.load()
    args = {**dict(B=1, C=4, T=16, A=4, tint=16, bint=1, flags=0), **kw}
    assert lib.bf_correlate_algorithmic_bytes(*(args[k] for k in ("B", "C", "T", "A", "tint", "bint", "flags"))) > 0
    with pytest.raises(_lib.BeamformerError, match="misaligned"):
        call(out=FAKE + 2, **kw)
    assert CorrelatorTemplate(None, args["B"], args["C"], args["T"], args["A"], integration=args["tint"],
                              batch_integration=args["bint"], sample_signed=bool(args["flags"] & SIGNED))


def test_int8_bound_is_65535_samples():
    """n is a multiple of 16, so the largest int8 window is 65520 = 3 * 21840 samples; 65535 itself is the bound the
    message states, and 2 * 128^2 * 65535 < 2^31 <= 2 * 128^2 * 65536; for uint8 2 * 255^2 * 16512 < 2^31."""
    assert 2 * 128 ** 2 * 65535 < 2 ** 31 <= 2 * 128 ** 2 * 65536
    assert 2 * 255 ** 2 * 16512 < 2 ** 31 <= 2 * 255 ** 2 * 16513
    with pytest.raises(_lib.BeamformerError, match="65535 for int8, 16512 for uint8"):
        call(T=65536, tint=65536, flags=SIGNED)


@pytest.mark.parametrize("B,C,T,A,tint,bint", [(8, 4096, 256, 64, 256, 8), (1, 4096, 256, 256, 256, 1),
                                               (8, 4096, 256, 64, 16, 1), (6, 3, 48, 130, 48, 3)])
def test_algorithmic_bytes(B, C, T, A, tint, bint):
    lib = _lib.load()
    volts = 4 * B * A * C * T
    outb = 32 * (A * (A + 1) // 2) * (B // bint) * C * (T // tint)
    for flags in (0, SIGNED):
        assert lib.bf_correlate_algorithmic_bytes(B, C, T, A, tint, bint, flags) == volts + outb
        assert lib.bf_correlate_algorithmic_bytes(B, C, T, A, tint, bint, flags | ACC) == volts + 2 * outb
    assert lib.bf_correlate_algorithmic_bytes(B, C, T, A, tint, bint, 4) == 0
    for bad in ((0, C, T, A, tint, bint), (B, -1, T, A, tint, bint), (B, C, 0, A, tint, bint), (B, C, T, 0, tint, bint),
                (B, C, T, A, 0, bint), (B, C, T, A, tint, 0), (B, C, T, 2049, tint, bint), (B, C, T, A, 8, bint)):
        assert lib.bf_correlate_algorithmic_bytes(*bad, 0) == 0
    t = CorrelatorTemplate(None, B, C, T, A, integration=tint, batch_integration=bint)
    assert t.algorithmic_bytes() == volts + outb and t.algorithmic_bytes(accumulating=True) == volts + 2 * outb


def test_cfg4_output_size():
    """The physics of a short integration: 256 antennas, tint = T = 256, a 1 GiB cube -> 4.3 GB out."""
    t = CorrelatorTemplate(None, 1, 4096, 256, 256)
    assert int(np.prod(t.input_shape)) == 1 << 30
    assert int(np.prod(t.output_shape)) * 4 == 32 * 32896 * 4096 == 4311744512


def test_template_errors():
    T = CorrelatorTemplate
    with pytest.raises(ValueError, match="multiple of 16"):
        T(None, 1, 4, 17, 4)
    for tint in (8, 24, 32, 0, -16):
        with pytest.raises(ValueError, match="integration"):
            T(None, 1, 4, 48, 4, integration=tint)
    with pytest.raises(ValueError, match="n_ants"):
        T(None, 1, 4, 16, 0)
    with pytest.raises(ValueError, match="n_ants"):
        T(None, 1, 4, 16, 2049)
    with pytest.raises(ValueError, match="n_batches"):
        T(None, 0, 4, 16, 4)
    with pytest.raises(ValueError, match="n_channels_per_stream"):
        T(None, 1, 0, 16, 4)
    with pytest.raises(ValueError, match="n_samples_per_channel"):
        T(None, 1, 4, 1 << 21, 4, integration=16)
    with pytest.raises(ValueError, match="batch_integration"):
        T(None, 4, 4, 16, 4, batch_integration=3)
    with pytest.raises(ValueError, match="batch_integration"):
        T(None, 4, 4, 16, 4, batch_integration=0)
    with pytest.raises(ValueError, match="batch_integration above 1"):
        T(None, 4, 4, 32, 4, integration=16, batch_integration=2)
    with pytest.raises(ValueError, match="int32 bound"):
        T(None, 1, 1, 16528, 4)
    with pytest.raises(ValueError, match="int32 bound"):
        T(None, 1, 1, 65536, 4, sample_signed=True)
    with pytest.raises(ValueError, match="int32 bound"):
        T(None, 3, 1, 5520, 4, batch_integration=3)
    with pytest.raises(ValueError, match="workgroups"):
        T(None, 1 << 20, 1 << 20, 16, 1)
    T(None, 1, 1, 16512, 4)
    T(None, 3, 1, 21840, 2, batch_integration=3, sample_signed=True)
    T(None, 1, 1, 16, 2048)


def test_template_shapes_and_slots():
    B, C, T, A = 6, 5, 512, 7
    t = CorrelatorTemplate(None, B, C, T, A)
    assert t.integration == T and t.batch_integration == 1 and t.flags == 0 and not t.accumulate
    assert t.input_shape == (B, A, C, T, 2, 2) and t.output_shape == (B, C, 1, 28, 2, 2, 2)
    assert t.input_shape == FusedBeamformerTemplate(None, B, C, 1024, T, A, 2).input_shape
    op = t.instantiate(None)
    assert list(op.slots) == ["inSamples", "outVisibilities"]
    assert op.slots["inSamples"].dtype == np.uint8 and op.slots["inSamples"].shape == t.input_shape
    assert op.slots["outVisibilities"].dtype == np.int32 and op.slots["outVisibilities"].shape == t.output_shape
    t = CorrelatorTemplate(None, B, C, T, A, integration=64, sample_signed=True)
    assert t.output_shape == (B, C, 8, 28, 2, 2, 2) and t.flags == SIGNED
    assert t.instantiate(None).slots["inSamples"].dtype == np.int8
    t = CorrelatorTemplate(None, B, C, T, A, batch_integration=3)
    assert t.output_shape == (2, C, 1, 28, 2, 2, 2)


def test_accumulate_counter():
    """The first launch after reset() overwrites, later ones accumulate, and the launch that would take the samples
    per window past the int32 bound raises before anything is counted."""
    op = CorrelatorTemplate(None, 1, 2, 4096, 3, accumulate=True).instantiate(None)
    assert op.samples_accumulated == 0
    assert op._next_flags() == 0 and op.samples_accumulated == 4096
    for k in (2, 3, 4):
        assert op._next_flags() == ACC and op.samples_accumulated == 4096 * k
    with pytest.raises(OverflowError, match="int32 bound"):  # 5 * 4096 > 16512
        op._next_flags()
    assert op.samples_accumulated == 4 * 4096
    op.reset()
    assert op.samples_accumulated == 0 and op._next_flags() == 0 and op._next_flags() == ACC
    op = CorrelatorTemplate(None, 2, 2, 4096, 3, batch_integration=2, sample_signed=True,
                            accumulate=True).instantiate(None)
    assert [op._next_flags() for _ in range(7)] == [SIGNED] + [SIGNED | ACC] * 6  # 7 * 8192 = 57344 <= 65535
    with pytest.raises(OverflowError):
        op._next_flags()
    plain = CorrelatorTemplate(None, 1, 2, 4096, 3).instantiate(None)
    assert [plain._next_flags() for _ in range(9)] == [0] * 9 and plain.samples_accumulated == 4096


def test_baseline_index():
    assert [n_baselines(a) for a in (1, 2, 3, 64, 256, 2048)] == [1, 3, 6, 2080, 32896, 2098176]
    assert baseline_index(0, 0) == (0, False) and baseline_index(1, 0) == (1, False)
    assert baseline_index(0, 1) == (1, True) and baseline_index(1, 1) == (2, False)
    A = 9
    seen = [baseline_index(a1, a2)[0] for a1 in range(A) for a2 in range(a1 + 1)]
    assert seen == list(range(n_baselines(A)))  # row-major in the lower triangle
    for a1 in range(A):
        for a2 in range(A):
            i, conj = baseline_index(a1, a2)
            assert i == baseline_index(a2, a1)[0] and conj == (a1 < a2)
    assert n_baselines(A) == R.n_baselines(A)
    with pytest.raises(ValueError):
        baseline_index(-1, 0)


def brute_force(raw, signed, k, c, j, tint, bint, a1, p1, a2, p2):
    x = raw.view(np.int8 if signed else np.uint8)
    s = 0
    for b in range(k * bint, (k + 1) * bint):
        for t in range(j * tint, (j + 1) * tint):
            u = complex(int(x[b, a1, c, t, p1, 0]), int(x[b, a1, c, t, p1, 1]))
            v = complex(int(x[b, a2, c, t, p2, 0]), int(x[b, a2, c, t, p2, 1]))
            s += u * v.conjugate()
    return int(s.real), int(s.imag)


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
def test_reference_against_brute_force_and_visibility_matrix(signed):
    B, A, C, T, tint = 2, 5, 2, 32, 16
    raw = R.random_voltages((B, A, C, T))
    vis = R.visibilities(raw, tint, 1, signed)
    assert vis.shape == (B, C, 2, 15, 2, 2, 2) and vis.dtype == np.int32
    full = visibility_matrix(vis)
    assert full.shape == (B, C, 2, A, 2, A, 2) and full.dtype == np.complex128
    for (k, c, j, a1, p1, a2, p2) in [(0, 0, 0, 0, 0, 0, 0), (1, 1, 1, 4, 1, 2, 0), (0, 1, 0, 3, 0, 3, 1),
                                      (1, 0, 1, 2, 1, 2, 0), (1, 1, 0, 1, 0, 4, 1), (0, 0, 1, 0, 1, 3, 0)]:
        re, im = brute_force(raw, signed, k, c, j, tint, 1, a1, p1, a2, p2)
        assert full[k, c, j, a1, p1, a2, p2] == complex(re, im)
        i, conj = baseline_index(a1, a2)
        stored = vis[k, c, j, i, p2, p1] if conj else vis[k, c, j, i, p1, p2]
        assert (int(stored[0]), int(stored[1]) * (-1 if conj else 1)) == (re, im)
    # Hermitian: V[a1, p1, a2, p2] = conj(V[a2, p2, a1, p1]), autos real on the pol diagonal
    flat = full.reshape(B, C, 2, 2 * A, 2 * A)
    np.testing.assert_array_equal(flat, np.conj(np.swapaxes(flat, -1, -2)))
    assert (np.diagonal(flat, axis1=-2, axis2=-1).imag == 0).all()
    with pytest.raises(ValueError, match="shape"):
        visibility_matrix(vis[..., 0])
    with pytest.raises(ValueError, match="baselines"):
        visibility_matrix(vis[:, :, :, :14])


def test_reference_batch_integration_and_accumulate():
    B, A, C, T = 6, 3, 2, 32
    raw = R.random_voltages((B, A, C, T))
    per_batch = R.visibilities(raw, T, 1, True).astype(np.int64)       # (6, C, 1, ...)
    np.testing.assert_array_equal(R.visibilities(raw, T, 3, True),
                                  per_batch.reshape(2, 3, *per_batch.shape[1:]).sum(axis=1))
    re, im = brute_force(raw, True, 1, 1, 0, T, 3, 2, 0, 1, 1)
    assert tuple(R.visibilities(raw, T, 3, True)[1, 1, 0, baseline_index(2, 1)[0], 0, 1]) == (re, im)
    cubes = [raw[0:2], raw[2:4], raw[4:6]]
    np.testing.assert_array_equal(R.accumulate(cubes, T, 1, True),
                                  per_batch[0:2] + per_batch[2:4] + per_batch[4:6])
    # sub-windows add up to the window
    np.testing.assert_array_equal(R.visibilities(raw, 16, 1, False).astype(np.int64).sum(axis=2, keepdims=True),
                                  R.visibilities(raw, 32, 1, False))


@pytest.mark.parametrize("n", [16, 48, 256])
def test_reference_closed_forms(n):
    """x[a, 0] = 3+4i, x[a, 1] = 1+2i: every baseline is (0,0) = 25, (0,1) = (3+4i) conj(1+2i) = 11-2i, (1,0) = 11+2i,
    (1,1) = 5 per sample, in both conventions (im = i1*r2 - r1*i2 = 4*1 - 3*2 for (0,1))."""
    B, A, C, T = 2, 3, 2, 2 * n
    x = np.empty((B, A, C, T, 2, 2), np.int8)
    x[..., 0, 0], x[..., 0, 1], x[..., 1, 0], x[..., 1, 1] = 3, 4, 1, 2
    want = np.array([[[25, 0], [11, -2]], [[11, 2], [5, 0]]]) * n
    for signed in (False, True):
        vis = R.visibilities(x.view(np.uint8), n, 1, signed)
        assert vis.shape == (B, C, 2, 6, 2, 2, 2)
        assert (vis == want).all()
    assert (R.visibilities(x.view(np.uint8), T, 2, True) == 4 * want).all()
    # the same bytes of -1-1i read as uint8 are 255+255i
    m1 = np.full((1, 2, 1, n, 2, 2), -1, np.int8)
    assert (R.visibilities(m1, n, 1, True)[..., 0] == 2 * n).all() and not R.visibilities(m1, n, 1, True)[..., 1].any()
    assert (R.visibilities(m1, n, 1, False)[..., 0] == 130050 * n).all()


def test_reference_full_scale_at_the_bounds():
    lo = np.full((3, 2, 1, 21840, 2, 2), -128, np.int8)
    vis = R.visibilities(lo, 21840, 3, True)
    assert (vis[..., 0] == 2 * 128 * 128 * 65520).all() and vis.max() == 2146959360 and not vis[..., 1].any()
    hi = np.full((1, 2, 1, 16512, 2, 2), 255, np.uint8)
    vis = R.visibilities(hi, 16512, 1, False)
    assert (vis[..., 0] == 130050 * 16512).all() and vis.max() == 2147385600 and not vis[..., 1].any()
    # the largest imaginary parts: x1 = -128 + 127i against x2 = 127 - 128i and the like stay inside int32 too
    z = np.empty((1, 2, 1, 65520, 2, 2), np.int8)
    z[:, 0, ..., 0], z[:, 0, ..., 1] = -128, -128
    z[:, 1, ..., 0], z[:, 1, ..., 1] = -128, 127
    vis = R.visibilities(z, 65520, 1, True)
    assert vis[0, 0, 0, 1, 0, 0, 1] == (127 * -128 - -128 * -128) * 65520  # i1 r2 - r1 i2, a1 = 1, a2 = 0


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "i8"])
def test_autos_are_the_power_sums(signed):
    """On one random cube: Re auto(p, p) per antenna is the voltage statistics' S1, and its sum over the antennas is
    the incoherent beam's S."""
    B, A, C, T, tint = 2, 5, 3, 64, 16
    raw = R.random_voltages((B, A, C, T))
    vis = R.visibilities(raw, tint, 1, signed)                          # (B, C, J, NBL, 2, 2, 2)
    autos = np.stack([vis[:, :, :, baseline_index(a, a)[0]] for a in range(A)], axis=1)  # (B, A, C, J, 2, 2, 2)
    assert not autos[..., 0, 0, 1].any() and not autos[..., 1, 1, 1].any()
    np.testing.assert_array_equal(autos[..., 0, 1, :] * [1, -1], autos[..., 1, 0, :])
    power = np.stack([autos[..., 0, 0, 0], autos[..., 1, 1, 0]], axis=2)                 # (B, A, 2, C, J)
    S1, _ = VR.moments(raw, tint, signed)
    np.testing.assert_array_equal(power, S1)
    np.testing.assert_array_equal(power.sum(axis=1), IR.power_sums(raw, tint, signed))
