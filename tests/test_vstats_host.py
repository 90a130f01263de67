"""Voltage statistics without a GPU: the feature query, bf_voltage_stats' argument validation (fake pointers, as
test_abi.py: validation fails before anything touches a device), the template, the byte count, the flags-to-mask
helper, and the NumPy restatement of the contract (vstats_ref.py) on inputs with closed-form answers and on the
four-behaviour cube (noise, carrier, dead input, pulsed interference)."""
import numpy as np
import pytest

import vstats_ref as R
from dpdk_dc_sand_amd import _lib
from dpdk_dc_sand_amd.beamforming import (FusedBeamformerTemplate, IncoherentBeamTemplate, VoltageStatsTemplate,
                                          antenna_mask_from_flags)

FAKE = 1 << 20  # 16-byte aligned, never dereferenced


def test_has_feature():
    lib = _lib.load()
    assert lib.bf_has_feature(b"voltage_stats") == 1
    assert lib.bf_has_feature(b"voltage") == 0
    assert lib.bf_has_feature(b"incoherent_beam") == 1 and lib.bf_has_feature(b"beam_detect") == 1
    assert lib.bf_abi_version() == 302
    assert _lib.VSTATS_SIGNED == 1


def call(raw=FAKE, power=FAKE, sk=FAKE, flg=FAKE, B=1, C=4, T=16, A=4, tint=16, flags=0, scale=1.0, lo=0.5, hi=1.5):
    return _lib.call("bf_voltage_stats", raw, power, sk, flg, B, C, T, A, tint, flags, scale, lo, hi, None)


@pytest.mark.parametrize("kw,match", [
    (dict(raw=None), "null pointer"),
    (dict(power=None, sk=None, flg=None), "null pointer"),
    (dict(T=17), "multiple of 16"),
    (dict(T=48, tint=8), "integration"),       # not a multiple of 16
    (dict(T=48, tint=24), "integration"),
    (dict(T=48, tint=32), "integration"),      # does not divide T
    (dict(tint=0), "integration"),
    (dict(T=1 << 20, tint=1 << 19), "integration"),  # above 2^18
    (dict(T=1 << 21, tint=16), "bad shape"),
    (dict(B=0), "bad shape"),
    (dict(A=0), "antennas"),
    (dict(A=32769), "antennas"),
    (dict(flags=2), "unknown flags"),
    (dict(raw=FAKE + 1), "misaligned"),
    (dict(power=FAKE + 2), "misaligned"),
    (dict(sk=FAKE + 1), "misaligned"),
    (dict(scale=0.0), "scale"),
    (dict(scale=float("nan")), "scale"),
    (dict(scale=float("inf")), "scale"),
    (dict(scale=-1.0), "scale"),
    (dict(lo=1.0, hi=1.0), "sk limits"),
    (dict(lo=1.5, hi=0.5), "sk limits"),
    (dict(lo=-0.1, hi=1.0), "sk limits"),
    (dict(lo=0.5, hi=float("inf")), "sk limits"),
    (dict(lo=float("nan"), hi=1.0), "sk limits"),
])
def test_argument_validation_without_gpu(kw, match):
    with pytest.raises(_lib.BeamformerError, match=match) as e:
        call(**kw)
    assert e.value.status == -1  # BF_ERR_ARG


def test_sk_limits_are_ignored_without_flags():
    """The same bad limits with out_flags NULL pass validation as far as it goes: the call reaches the one check that
    follows the limits, the grid limit (nothing is launched: 2^15 windows per run in pieces of 1024, times B * A = 2^30
    runs, is more than 2^31 - 1 workgroups), while with out_flags the limits are what is reported."""
    big = dict(B=32768, C=32768, T=16, A=32768, tint=16)
    for lo, hi in ((1.0, 1.0), (1.5, 0.5), (-0.1, 1.0), (float("nan"), float("inf"))):
        with pytest.raises(_lib.BeamformerError, match="grid limit"):
            call(flg=None, lo=lo, hi=hi, **big)
        with pytest.raises(_lib.BeamformerError, match="sk limits"):
            call(lo=lo, hi=hi, **big)


def test_template_errors():
    T = VoltageStatsTemplate
    with pytest.raises(ValueError, match="multiple of 16"):
        T(None, 1, 4, 17, 4, integration=16)
    for tint in (8, 24, 32, 0, -16):
        with pytest.raises(ValueError, match="integration"):
            T(None, 1, 4, 48, 4, integration=tint)
    with pytest.raises(ValueError, match="integration"):
        T(None, 1, 1, 1 << 20, 4, integration=1 << 19)
    with pytest.raises(ValueError, match="integration"):
        T(None, 1, 4, 48, 4)  # the default of 256 does not divide 48
    with pytest.raises(ValueError, match="n_ants"):
        T(None, 1, 4, 16, 0, integration=16)
    with pytest.raises(ValueError, match="n_ants"):
        T(None, 1, 4, 16, 32769, integration=16)
    with pytest.raises(ValueError, match="n_batches"):
        T(None, 0, 4, 16, 4, integration=16)
    with pytest.raises(ValueError, match="n_samples_per_channel"):
        T(None, 1, 4, 1 << 21, 4)
    for scale in (0.0, -2.0, float("nan"), float("inf"), 1e-60):  # 1e-60 is 0 as float32
        with pytest.raises(ValueError, match="scale"):
            T(None, 1, 4, 16, 4, integration=16, scale=scale)
    for limits in ((1.0, 1.0), (1.5, 0.5), (-0.1, 1.0), (0.5, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="sk_limits"):
            T(None, 1, 4, 16, 4, integration=16, sk_limits=limits)
    with pytest.raises(ValueError, match="no output"):
        T(None, 1, 4, 16, 4, integration=16, power=False, sk=False)
    for tint in (16, 48):
        T(None, 1, 4, 48, 4, integration=tint)
    T(None, 1, 1, 1 << 20, 32768, integration=1 << 18)
    T(None, 1, 4, 16, 4, integration=16, power=False, sk=False, sk_limits=(0.0, 1.0))


def test_template_shapes_and_slots():
    B, C, T, A = 3, 5, 512, 7
    t = VoltageStatsTemplate(None, B, C, T, A)
    assert t.integration == 256 and t.flags == 0 and t.outputs == 3 and t.sk_limits is None
    assert t.input_shape == (B, A, C, T, 2, 2) and t.output_shape == (B, A, 2, C, 2)
    # one device buffer binds to all three operators
    assert t.input_shape == FusedBeamformerTemplate(None, B, C, 1024, T, A, 2).input_shape
    assert t.input_shape == IncoherentBeamTemplate(None, B, C, T, A).input_shape
    op = t.instantiate(None)
    assert set(op.slots) == {"inSamples", "outPower", "outSK"}
    assert op.slots["inSamples"].dtype == np.uint8 and op.slots["inSamples"].shape == t.input_shape
    assert op.slots["outPower"].dtype == np.float32 and op.slots["outSK"].shape == t.output_shape

    t = VoltageStatsTemplate(None, B, C, T, A, integration=64, sample_signed=True, scale=1 / 3, power=False,
                             sk_limits=(0.75, 1.25))
    assert t.output_shape == (B, A, 2, C, 8) and t.flags == _lib.VSTATS_SIGNED and t.outputs == 6
    assert t.scale == float(np.float32(1 / 3)) and t.sk_limits == (0.75, 1.25)
    op = t.instantiate(None)
    assert set(op.slots) == {"inSamples", "outSK", "outFlags"}
    assert op.slots["inSamples"].dtype == np.int8
    assert op.slots["outFlags"].dtype == np.uint8 and op.slots["outFlags"].shape == t.output_shape
    t = VoltageStatsTemplate(None, B, C, T, A, sk=False, sk_limits=(0.1, 0.2))
    assert set(t.instantiate(None).slots) == {"inSamples", "outPower", "outFlags"} and t.outputs == 5
    assert t.sk_limits == (float(np.float32(0.1)), float(np.float32(0.2)))  # the float32 values the library compares


@pytest.mark.parametrize("B,C,T,A,tint", [(8, 4096, 256, 64, 256), (8, 4096, 256, 64, 16), (1, 4096, 256, 256, 256),
                                          (2, 3, 48, 130, 48)])
def test_algorithmic_bytes(B, C, T, A, tint):
    lib = _lib.load()
    volts, win = 4 * B * A * C * T, B * A * 2 * C * (T // tint)
    for outputs in range(1, 8):
        per = 4 * (outputs & 1) + 4 * (outputs >> 1 & 1) + (outputs >> 2 & 1)
        assert lib.bf_vstats_algorithmic_bytes(B, C, T, A, tint, outputs) == volts + win * per
    assert lib.bf_vstats_algorithmic_bytes(B, C, T, A, tint, 0) == 0
    assert lib.bf_vstats_algorithmic_bytes(B, C, T, A, tint, 8) == 0
    for bad in ((0, C, T, A, tint), (B, -1, T, A, tint), (B, C, 0, A, tint), (B, C, T, 0, tint), (B, C, T, A, 0)):
        assert lib.bf_vstats_algorithmic_bytes(*bad, 7) == 0
    t = VoltageStatsTemplate(None, B, C, T, A, integration=tint, sk_limits=(0.5, 1.5))
    assert t.algorithmic_bytes() == volts + 9 * win
    t = VoltageStatsTemplate(None, B, C, T, A, integration=tint, sk=False)
    assert t.algorithmic_bytes() == volts + 4 * win


def test_antenna_mask_from_flags():
    B, A, C, J = 2, 5, 3, 4
    flags = np.zeros((B, A, 2, C, J), np.uint8)
    n = B * 2 * C * J  # 48 windows per antenna
    flags[:, 1] = 1                                   # all flagged
    flags[0, 2, 0, 0, :3] = 1                         # 3 / 48
    flags[1, 3, 1, 2, 0] = 7                          # 1 / 48, any non-zero value counts once
    flags.reshape(B, A, -1)[:, 4, :12] = 1            # 24 / 48
    np.testing.assert_array_equal(antenna_mask_from_flags(flags, 0.0), [1, 0, 0, 0, 0])
    np.testing.assert_array_equal(antenna_mask_from_flags(flags, 1 / 48), [1, 0, 0, 1, 0])
    np.testing.assert_array_equal(antenna_mask_from_flags(flags, 3 / 48), [1, 0, 1, 1, 0])  # at most: equality counts
    np.testing.assert_array_equal(antenna_mask_from_flags(flags, 0.5), [1, 0, 1, 1, 1])
    np.testing.assert_array_equal(antenna_mask_from_flags(flags, 1.0), [1, 1, 1, 1, 1])
    m = antenna_mask_from_flags(flags, 0.2)
    assert m.dtype == np.uint8 and m.shape == (A,)
    op = IncoherentBeamTemplate(None, B, C, 64, A, antenna_mask=True).instantiate(None)
    op.set_antenna_mask(m)
    np.testing.assert_array_equal(op.antenna_mask(), [1, 0, 1, 1, 0])
    with pytest.raises(ValueError, match="shape"):
        antenna_mask_from_flags(flags[0], 0.2)
    with pytest.raises(ValueError, match="max_fraction"):
        antenna_mask_from_flags(flags, 1.5)


@pytest.mark.parametrize("n", [16, 48, 256, 4096])
def test_reference_closed_forms(n):
    B, A, C, T = 2, 3, 2, 2 * n
    shape = (B, A, C, T, 2, 2)
    out_shape = (B, A, 2, C, 2)
    limits = (0.5, 1.5)
    # every sample 3+4i: S1 = 25 n, S2 = 625 n, n S2 / S1^2 = 1 exactly, SK exactly 0 (flagged: below the lower limit)
    x = np.empty(shape, np.int8)
    x[..., 0], x[..., 1] = 3, 4
    for signed in (False, True):
        raw = x if signed else x.view(np.uint8)
        S1, S2 = R.moments(raw, n, signed)
        assert S1.shape == out_shape and S1.dtype == np.int64 and (S1 == 25 * n).all() and (S2 == 625 * n).all()
        power, sk, flags = R.voltage_stats(raw, n, signed, 0.5, limits)
        assert power.dtype == sk.dtype == np.float32 and flags.dtype == np.uint8
        assert (power == 12.5 * n).all() and (sk.view(np.uint32) == 0).all() and (flags == 1).all()
    # unsigned samples alternating 255+255i and 0: n S2 / S1^2 = 2, SK = float32((n + 1) / (n - 1))
    x = np.zeros(shape, np.uint8)
    x[:, :, :, 0::2] = 255
    S1, S2 = R.moments(x, n, False)
    assert (S1 == 130050 * n // 2).all() and (S2 == 130050 ** 2 * n // 2).all()
    power, sk, flags = R.voltage_stats(x, n, False, 1.0, limits)
    assert (sk == np.float32((n + 1) / (n - 1))).all() and (sk > 1).all()
    assert (flags == (1 if (n + 1) / (n - 1) > 1.5 else 0)).all()
    # the same bytes read as int8 are -1-1i and 0: pw = 2
    assert (R.moments(x, n, True)[0] == n).all()
    # all zeros: SK 0, flag 1, whatever the limits
    power, sk, flags = R.voltage_stats(np.zeros(shape, np.uint8), n, False, 1.0, (0.0, 1e30))
    assert (power.view(np.uint32) == 0).all() and (sk.view(np.uint32) == 0).all() and (flags == 1).all()
    # full scale
    assert (R.moments(np.full(shape, -128, np.int8), n, True)[1] == 2 ** 30 * n).all()
    assert (R.moments(np.full(shape, 255, np.uint8), n, False)[1] == 130050 ** 2 * n).all()


def test_reference_windows_and_flag_limits():
    rng = np.random.default_rng(5)
    B, A, C, T, tint = 2, 3, 2, 64, 16
    x = rng.integers(-128, 128, (B, A, C, T, 2, 2), dtype=np.int8)
    S1, S2 = R.moments(x, tint, True)
    v = x.astype(np.int64)
    b, a, p, c, j = 1, 2, 1, 1, 3
    pw = [int(v[b, a, c, t, p, 0]) ** 2 + int(v[b, a, c, t, p, 1]) ** 2 for t in range(j * tint, (j + 1) * tint)]
    assert S1[b, a, p, c, j] == sum(pw) and S2[b, a, p, c, j] == sum(q * q for q in pw)
    sk = R.spectral_kurtosis(S1, S2, tint)
    want = np.float32((17 / 15) * ((16.0 * float(S2[b, a, p, c, j])) / (float(sum(pw)) * float(sum(pw))) - 1.0))
    assert sk[b, a, p, c, j] == want
    # a value equal to a limit is not flagged; the compares are on the stored float32
    lo, hi = np.sort(sk.ravel())[[5, -5]]  # 5 values below lo, 4 above hi (random data: no ties)
    flags = R.flag(S1, sk, (lo, hi))
    assert flags.sum() == 9 and not flags[sk == lo].any() and not flags[sk == hi].any()
    assert R.flag(S1, sk, (np.nextafter(lo, np.float32(9)), hi)).sum() == 10


def test_four_behaviours():
    """Noise, a carrier, a dead input and pulsed interference at (1, 4, 2, 8192, 4096), int8, limits (0.75, 1.25):
    the noise antenna is unflagged in every window, the other three are flagged in every window."""
    B, A, C, T, tint = R.FOUR_SHAPE
    raw = R.four_behaviours()
    assert raw.shape == (B, A, C, T, 2, 2) and raw.dtype == np.int8
    power, sk, flags = R.voltage_stats(raw, tint, True, 1.0, R.FOUR_LIMITS)
    assert flags.shape == (B, A, 2, C, T // tint)
    assert 0.898 <= sk[:, 0].min() and sk[:, 0].max() <= 1.129 and not flags[:, 0].any()
    assert (sk[:, 1] == 0).all() and (power[:, 1] == 25 * tint).all() and flags[:, 1].all()
    assert (sk[:, 2] == 0).all() and (power[:, 2] == 0).all() and flags[:, 2].all()
    assert sk[:, 3].min() > 7 and flags[:, 3].all()
    np.testing.assert_array_equal(antenna_mask_from_flags(flags, 0.2), [1, 0, 0, 0])


def test_scaling_is_one_float64_multiply():
    """The sums of the GPU scaling test (random uint8, tint 1024: more than 24 significant bits): float32(S1) *
    float32(scale), and a float32 conversion of S1 before the float64 multiply, give other bits than the contract, so a
    kernel that scales in float32 fails there."""
    B, A, C, T, tint = R.SCALING_SHAPE
    S1, _ = R.moments(R.random_voltages((B, A, C, T)), tint, False)
    assert S1.min() > 2 ** 24
    ref = R.scale_power(S1, 1 / 3)
    f32_product = S1.astype(np.float32) * np.float32(1 / 3)
    f32_sum_first = (S1.astype(np.float32).astype(np.float64) * np.float64(np.float32(1 / 3))).astype(np.float32)
    assert (f32_product.view(np.uint32) != ref.view(np.uint32)).any()
    assert (f32_sum_first.view(np.uint32) != ref.view(np.uint32)).any()
    assert ref.flat[0] == np.float32(float(S1.flat[0]) * float(np.float32(1 / 3)))
