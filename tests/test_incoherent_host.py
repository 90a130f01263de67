"""Incoherent beam without a GPU: the feature query, bf_incoherent_beam's argument validation (fake pointers, as
test_abi.py: validation fails before anything touches a device), the template, the byte count, and the NumPy
restatement of the contract (incoherent_ref.py) on inputs with closed-form answers."""
import numpy as np
import pytest

import incoherent_ref as R
from dpdk_dc_sand_amd import _lib
from dpdk_dc_sand_amd.beamforming import FusedBeamformerTemplate, IncoherentBeamTemplate

FAKE = 1 << 20  # 16-byte aligned, never dereferenced


def test_has_feature():
    lib = _lib.load()
    assert lib.bf_has_feature(b"incoherent_beam") == 1
    assert lib.bf_has_feature(b"incoherent") == 0
    assert lib.bf_has_feature(b"stokes") == 0
    assert lib.bf_has_feature(None) == 0
    assert lib.bf_abi_version() == 302


def call(raw=FAKE, mask=None, out=FAKE, B=1, C=4, T=16, A=4, tint=16, flags=0, scale=1.0):
    return _lib.call("bf_incoherent_beam", raw, mask, out, B, C, T, A, tint, flags, scale, None)


@pytest.mark.parametrize("kw,match", [
    (dict(raw=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(T=17, tint=1), "multiple of 16"),
    (dict(T=48, tint=3), "integration"),
    (dict(T=48, tint=24), "integration"),
    (dict(T=48, tint=32), "integration"),
    (dict(tint=0), "integration"),
    (dict(A=0), "antennas"),
    (dict(A=32769), "antennas"),
    (dict(flags=4), "unknown flags"),
    (dict(raw=FAKE + 1), "misaligned"),
    (dict(out=FAKE + 2), "misaligned"),
    (dict(scale=0.0), "scale"),
    (dict(scale=float("nan")), "scale"),
    (dict(scale=float("inf")), "scale"),
    (dict(scale=-1.0), "scale"),
    (dict(B=0), "bad shape"),
    (dict(T=1 << 21, tint=16), "bad shape"),
])
def test_argument_validation_without_gpu(kw, match):
    with pytest.raises(_lib.BeamformerError, match=match) as e:
        call(**kw)
    assert e.value.status == -1  # BF_ERR_ARG


def test_template_errors():
    T = IncoherentBeamTemplate
    with pytest.raises(ValueError, match="multiple of 16"):
        T(None, 1, 4, 17, 4)
    for tint in (3, 24, 32, 0, -16):
        with pytest.raises(ValueError, match="integration"):
            T(None, 1, 4, 48, 4, integration=tint)
    with pytest.raises(ValueError, match="n_ants"):
        T(None, 1, 4, 16, 0)
    with pytest.raises(ValueError, match="n_ants"):
        T(None, 1, 4, 16, 32769)
    with pytest.raises(ValueError, match="n_batches"):
        T(None, 0, 4, 16, 4)
    with pytest.raises(ValueError, match="n_samples_per_channel"):
        T(None, 1, 4, 1 << 21, 4)
    for scale in (0.0, -2.0, float("nan"), float("inf"), 1e-60):  # 1e-60 is 0 as float32
        with pytest.raises(ValueError, match="scale"):
            T(None, 1, 4, 16, 4, scale=scale)
    for tint in (1, 2, 4, 8, 16, 48):
        T(None, 1, 4, 48, 4, integration=tint)
    T(None, 1, 1, 1 << 20, 32768, integration=1 << 20)


def test_template_shapes_and_flags():
    B, C, T, A = 3, 5, 64, 7
    t = IncoherentBeamTemplate(None, B, C, T, A)
    assert t.integration == 16 and t.flags == 0
    assert t.input_shape == (B, A, C, T, 2, 2) and t.output_shape == (B, 2, C, 4)
    # one device buffer binds to both operators
    assert t.input_shape == FusedBeamformerTemplate(None, B, C, 1024, T, A, 2).input_shape
    t = IncoherentBeamTemplate(None, B, C, T, A, integration=64, sample_signed=True, sum_pols=True, scale=1 / 3,
                               antenna_mask=True)
    assert t.output_shape == (B, 1, C, 1) and t.flags == _lib.INCOH_SIGNED | _lib.INCOH_SUM_POLS == 3
    assert t.scale == float(np.float32(1 / 3)) and t.mask_shape == (A,)


def test_operator_slots_and_mask_host_copy():
    B, C, T, A = 2, 3, 32, 5
    op = IncoherentBeamTemplate(None, B, C, T, A, sample_signed=True).instantiate(None)
    assert set(op.slots) == {"inSamples", "outData"}
    assert op.slots["inSamples"].dtype == np.int8 and op.slots["outData"].shape == (B, 2, C, 2)
    assert op.antenna_mask() is None
    with pytest.raises(ValueError, match="antenna_mask=True"):
        op.set_antenna_mask(np.ones(A))
    op = IncoherentBeamTemplate(None, B, C, T, A, antenna_mask=True).instantiate(None)
    assert op.slots["inSamples"].dtype == np.uint8
    assert op.slots["antennaMask"].shape == (A,) and op.slots["antennaMask"].dtype == np.uint8
    np.testing.assert_array_equal(op.antenna_mask(), np.ones(A, np.uint8))
    op.set_antenna_mask([1, 0, 7, 0, True])
    np.testing.assert_array_equal(op.antenna_mask(), [1, 0, 1, 0, 1])
    op.antenna_mask()[0] = 0  # a copy
    assert op.antenna_mask()[0] == 1
    with pytest.raises(ValueError, match="expected 5"):
        op.set_antenna_mask(np.ones(A + 1))


@pytest.mark.parametrize("B,C,T,A,tint", [(8, 4096, 256, 64, 256), (8, 4096, 256, 64, 16), (1, 4096, 256, 256, 1),
                                          (2, 3, 48, 130, 48)])
def test_algorithmic_bytes(B, C, T, A, tint):
    lib = _lib.load()
    volts, win = 4 * B * A * C * T, B * C * T // tint
    assert lib.bf_incoherent_algorithmic_bytes(B, C, T, A, tint, 0, 0) == volts + 4 * 2 * win
    assert lib.bf_incoherent_algorithmic_bytes(B, C, T, A, tint, 1, 1) == volts + A + 4 * 2 * win
    assert lib.bf_incoherent_algorithmic_bytes(B, C, T, A, tint, 2, 0) == volts + 4 * win
    assert lib.bf_incoherent_algorithmic_bytes(B, C, T, A, tint, 3, 5) == volts + A + 4 * win
    t = IncoherentBeamTemplate(None, B, C, T, A, integration=tint, sum_pols=True, antenna_mask=True)
    assert t.algorithmic_bytes() == volts + A + 4 * win


@pytest.mark.parametrize("A,tint", [(1, 1), (3, 16), (64, 256)])
def test_reference_closed_forms(A, tint):
    B, C, T = 2, 3, 256
    shape = (B, A, C, T, 2, 2)
    x = np.empty(shape, np.int8)
    x[..., 0], x[..., 1] = 3, 4
    for signed in (False, True):
        S = R.power_sums(x if signed else x.view(np.uint8), tint, signed)
        assert S.shape == (B, 2, C, T // tint) and S.dtype == np.int64
        assert (S == 25 * A * tint).all()
        S = R.power_sums(x if signed else x.view(np.uint8), tint, signed, sum_pols=True)
        assert S.shape == (B, 1, C, T // tint) and (S == 50 * A * tint).all()
    assert (R.power_sums(np.full(shape, -128, np.int8), tint, True) == 32768 * A * tint).all()
    assert (R.power_sums(np.full(shape, 255, np.uint8), tint, False) == 130050 * A * tint).all()
    # the same bytes read the other way
    assert (R.power_sums(np.full(shape, 255, np.uint8), tint, True) == 2 * A * tint).all()


def test_reference_mask_windows_and_scale():
    rng = np.random.default_rng(5)
    B, A, C, T, tint = 2, 6, 3, 32, 8
    x = rng.integers(-128, 128, (B, A, C, T, 2, 2), dtype=np.int8)
    mask = np.array([1, 0, 0, 2, 0, 1], np.uint8)
    S = R.power_sums(x, tint, True, mask=mask)
    v = x.astype(np.int64)
    b, p, c, j = 1, 1, 2, 3
    want = sum(int(v[b, a, c, t, p, 0]) ** 2 + int(v[b, a, c, t, p, 1]) ** 2 for a in (0, 3, 5)
               for t in range(j * tint, (j + 1) * tint))
    assert S[b, p, c, j] == want
    assert (R.power_sums(x, tint, True, mask=np.zeros(A, np.uint8)) == 0).all()
    np.testing.assert_array_equal(R.power_sums(x, tint, True, mask=np.ones(A)), R.power_sums(x, tint, True))
    np.testing.assert_array_equal(R.power_sums(x, tint, True, sum_pols=True)[:, 0], R.power_sums(x, tint, True).sum(1))
    # one float64 multiply by float32(scale), one rounding: for a sum above 2^32 this differs from float32 products
    S = np.array([32768 * 256 * 256], np.int64)
    out = R.scale_sums(S, 1 / 3)
    assert out.dtype == np.float32
    assert out[0] == np.float32(float(S[0]) * float(np.float32(1 / 3)))
