"""Beam streams without a GPU: the feature query, bf_beam_streams' argument validation (fake pointers, as test_abi.py:
validation fails before anything touches a device), the byte count, the template, and the NumPy restatement of the
contract (beam_streams_ref.py) against the element-by-element formula and oracle.requantise."""
import numpy as np
import pytest

import beam_streams_ref as R
import oracle as O
from dpdk_dc_sand_amd import _lib
from dpdk_dc_sand_amd.beamforming import BeamStreamsTemplate, FusedBeamformerTemplate, VoltageStatsTemplate

FAKE = 1 << 20  # 16-byte aligned, never dereferenced
I8, Q, LIST = _lib.BSTREAM_IN_INT8, _lib.BSTREAM_REQUANT, _lib.BSTREAM_LIST


def test_has_feature():
    lib = _lib.load()
    assert lib.bf_has_feature(b"beam_streams") == 1
    assert lib.bf_has_feature(b"beam_stream") == 0
    assert lib.bf_abi_version() == 302
    assert (I8, Q, LIST) == (1, 2, 4)


def call(beams=FAKE, index=None, out=FAKE, B=1, C=2, T=16, M=4, K=4, flags=0, scale=1.0):
    return _lib.call("bf_beam_streams", beams, index, out, B, C, T, M, K, flags, scale, None)


@pytest.mark.parametrize("kw,match", [
    (dict(beams=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(B=0), "bad shape"),
    (dict(C=0), "bad shape"),
    (dict(M=0, K=0), "bad shape"),
    (dict(K=0, index=FAKE), "bad shape"),
    (dict(T=24), "multiple of 16"),
    (dict(T=1 << 21), "above 2\\^20"),
    (dict(M=4097, K=4097), "at most 4096"),
    (dict(K=4097, index=FAKE), "at most 4096"),
    (dict(flags=8), "unknown flags"),
    (dict(flags=I8 | Q), "BF_BSTREAM_REQUANT needs f32"),
    (dict(K=3), "no beam list"),
    (dict(K=5, flags=I8), "no beam list"),
    (dict(flags=LIST), "BF_BSTREAM_LIST without"),
    (dict(beams=FAKE + 8), "misaligned"),
    (dict(out=FAKE + 4, flags=I8), "misaligned"),
    (dict(index=FAKE + 2), "misaligned"),
    (dict(flags=Q, scale=0.0), "scale"),
    (dict(flags=Q, scale=-1.0), "scale"),
    (dict(flags=Q, scale=float("nan")), "scale"),
    (dict(flags=Q, scale=float("inf")), "scale"),
    (dict(B=32768, C=32768, T=16, M=4096, K=4096), "grid limit"),
])
def test_argument_validation_without_gpu(kw, match):
    with pytest.raises(_lib.BeamformerError, match=match) as e:
        call(**kw)
    assert e.value.status == -1  # BF_ERR_ARG


@pytest.mark.parametrize("B,C,T,M,K", [(8, 4096, 256, 16, 16), (8, 4096, 256, 1, 1), (1, 4096, 256, 64, 1),
                                       (2, 3, 48, 5, 4), (1, 1, 16, 4096, 4096), (1, 2, 32, 5, 10)])
def test_algorithmic_bytes(B, C, T, M, K):
    f = _lib.load().bf_beam_streams_algorithmic_bytes
    n = B * C * T
    for flags, es_in, es_out in ((I8, 1, 1), (0, 4, 4), (Q, 4, 1)):
        assert f(B, C, T, M, K, flags | LIST) == es_in * n * 2 * 2 * M + es_out * n * K * 4 + 4 * K
        # without the list bit the call is the identity, which needs K == M
        assert f(B, C, T, M, K, flags) == (es_in * n * 2 * 2 * M + es_out * n * K * 4 if K == M else 0)
    # whatever the entry point refuses
    for bad in ((0, C, T, M, K), (B, 0, T, M, K), (B, C, 0, M, K), (B, C, T, 0, K), (B, C, T, M, 0), (B, C, 24, M, K),
                (B, C, 1 << 21, M, K), (B, C, T, 4097, K), (B, C, T, M, 4097)):
        assert f(*bad, LIST) == 0
    assert f(B, C, T, M, K, LIST | 8) == 0 and f(B, C, T, M, K, LIST | I8 | Q) == 0
    assert f(32768, 32768, 16, 4096, 4096, 0) == 0  # the grid limit
    t = BeamStreamsTemplate(None, B, C, T, M, in_int8=True, beams=np.arange(K) % M)
    assert t.algorithmic_bytes() == n * 4 * M + n * K * 4 + 4 * K
    t = BeamStreamsTemplate(None, B, C, T, M, requantise=True, scale=0.5)
    assert t.algorithmic_bytes() == 4 * n * 4 * M + n * M * 4


def test_template_errors():
    T = BeamStreamsTemplate
    for args, match in (((0, 4, 16, 4), "n_batches"), ((1, 0, 16, 4), "n_channels_per_stream"),
                        ((1, 4, 0, 4), "n_samples_per_channel"), ((1, 4, 16, 0), "n_beams"),
                        ((1, 4, 24, 4), "multiple of 16"), ((1, 4, 1 << 21, 4), "at most"),
                        ((1, 4, 16, 4097), "n_beams")):
        with pytest.raises(ValueError, match=match):
            T(None, *args)
    with pytest.raises(ValueError, match="requantise"):
        T(None, 1, 4, 16, 4, in_int8=True, requantise=True)
    for scale in (0.0, -2.0, float("nan"), float("inf"), 1e-60):  # 1e-60 is 0 as float32
        with pytest.raises(ValueError, match="scale"):
            T(None, 1, 4, 16, 4, requantise=True, scale=scale)
    T(None, 1, 4, 16, 4, scale=float("nan"))  # ignored without requantise
    for beams, match in (([], "list of"), ([[0, 1]], "list of"), (np.zeros(4097, int), "list of"), ([0.5], "integers"),
                         ([0, 4], "out of range"), ([-1, 0], "out of range"), ([2 ** 31 - 1], "out of range")):
        with pytest.raises(ValueError, match=match):
            T(None, 1, 4, 16, 4, beams=beams)
    with pytest.raises(ValueError, match="workgroups"):
        T(None, 32768, 32768, 16, 4096)
    T(None, 1, 1, 1 << 20, 4096)
    T(None, 1, 4, 16, 4, beams=np.zeros(4096, int))


def test_template_shapes_slots_and_list():
    B, C, T, M = 3, 5, 32, 7
    t = BeamStreamsTemplate(None, B, C, T, M)
    assert t.flags == 0 and t.n_streams == M and t.beams is None
    assert t.input_shape == (B, 2, C, T // 16, 16, 2 * M) and t.output_shape == (B, M, C, T, 2, 2)
    assert t.input_shape == FusedBeamformerTemplate(None, B, C, 1024, T, 4, M).output_shape
    op = t.instantiate(None)
    assert set(op.slots) == {"inBeams", "outStreams"} and op.beams() is None
    assert op.slots["inBeams"].dtype == np.float32 and op.slots["outStreams"].dtype == np.float32
    with pytest.raises(ValueError, match="without a beam list"):
        op.select_beams([0])

    t = BeamStreamsTemplate(None, B, C, T, M, in_int8=True, beams=[6, 0, 0, 2])
    assert t.flags == I8 | LIST and t.n_streams == 4 and t.output_shape == (B, 4, C, T, 2, 2)
    # the int8 streams are a voltage cube of K antennas
    assert t.output_shape == VoltageStatsTemplate(None, B, C, T, 4, integration=16, sample_signed=True).input_shape
    op = t.instantiate(None)
    assert set(op.slots) == {"inBeams", "outStreams", "beamIndex"}
    assert op.slots["inBeams"].dtype == np.int8 and op.slots["outStreams"].dtype == np.int8
    assert op.slots["beamIndex"].shape == (4,) and op.slots["beamIndex"].dtype == np.int32
    np.testing.assert_array_equal(op.beams(), [6, 0, 0, 2])
    op.select_beams([1, 2, 3, 3])
    assert op.beams().dtype == np.int32 and list(op.beams()) == [1, 2, 3, 3]
    for bad, match in (([1, 2, 3], "expected 4"), ([1, 2, 3, 7], "out of range"), ([1, 2, 3, -1], "out of range")):
        with pytest.raises(ValueError, match=match):
            op.select_beams(bad)
    assert list(op.beams()) == [1, 2, 3, 3]  # a refused list changes nothing

    t = BeamStreamsTemplate(None, B, C, T, M, requantise=True, scale=1 / 3)
    assert t.flags == Q and t.scale == float(np.float32(1 / 3))
    op = t.instantiate(None)
    assert op.slots["inBeams"].dtype == np.float32 and op.slots["outStreams"].dtype == np.int8


@pytest.mark.parametrize("int8", [True, False], ids=["i8", "f32"])
def test_reference_equals_the_element_formula(int8):
    B, C, T, M = 2, 3, 32, 5
    y = R.random_beams(B, C, T, M, int8)
    for index in ([4, 0, 0, 2], None, [-1, 3, M, 2 ** 31 - 1]):
        got = R.beam_streams(y, index)
        assert got.shape == (B, M if index is None else len(index), C, T, 2, 2) and got.dtype == y.dtype
        assert got.flags.c_contiguous
        assert R.as_bytes(got).tobytes() == R.as_bytes(R.by_elements(y, index)).tobytes()
    z = R.beam_streams(y, [-1, 3, M, 2 ** 31 - 1])
    assert not R.as_bytes(z[:, [0, 2, 3]]).any() and R.as_bytes(z[:, 1]).any()


def test_generator_has_the_special_values():
    y = R.random_beams(1, 1, 16, 1, True)
    assert {-128, 127, -127} <= set(y.ravel().tolist())
    y = R.random_beams(1, 1, 16, 2, False)
    u = set(y.view(np.uint32).ravel().tolist())
    assert set(R.F32_SPECIALS.view(np.uint32).tolist()) <= u  # NaN payloads, +-inf, -0.0 bit for bit
    assert np.isnan(y).sum() >= 3 and np.isinf(y).sum() >= 2


def test_requantising_reference_equals_the_oracle():
    B, C, T, M = 2, 3, 32, 5
    y = R.random_beams(B, C, T, M, False)
    index = [4, 0, 0, 2]
    q = R.beam_streams(y, index, scale=R.SCALE)
    assert q.dtype == np.int8 and q.shape == (B, 4, C, T, 2, 2)
    np.testing.assert_array_equal(q, O.requantise(R.beam_streams(y, index), R.SCALE))
    for b, k, c, t, p, z in ((0, 0, 0, 0, 0, 0), (1, 3, 2, 31, 1, 1), (1, 1, 1, 17, 0, 1)):
        assert q[b, k, c, t, p, z] == O.requantise(y[b, p, c, t // 16, t % 16, 2 * index[k] + z], R.SCALE)
    assert (q == 127).any() and (q == -127).any() and not (q == -128).any()
    assert O.requantise(np.float32("nan"), R.SCALE) == -127
    assert not R.as_bytes(R.beam_streams(y, [M, -1], scale=R.SCALE)).any()
