"""GPU: the beam streams (bf_beam_streams, csrc/bf_beam_streams.hip; beamforming.beam_streams) against the NumPy
restatement of the contract (beam_streams_ref.py), byte for byte, no tolerance: every output is prefilled with 0x5A and
compared whole.

Shapes are the smallest at which each mechanism of the kernel can break: one beam (a pure pol interleave), odd M (rows
at every 2-byte alignment), one past a power of two, M = 64 / 65 and 257 / 4096 (whole rows in a tile / column tiles
with rows wider than a tile), a run of C * T = 16 samples (shorter than any tile), 144 (ragged) and 512 (whole tiles
and more than one), several batches."""
import numpy as np
import pytest

import beam_streams_ref as R
import correlate_ref as CR
import guarded as G
import oracle as O
import vstats_ref as VR
from dpdk_dc_sand_amd import _lib
from dpdk_dc_sand_amd import accel
from dpdk_dc_sand_amd.beamforming import (BeamStreamsTemplate, CorrelatorTemplate, FusedBeamformerTemplate,
                                          VoltageStatsTemplate)

pytestmark = pytest.mark.gpu

FLAGS = {"i8": _lib.BSTREAM_IN_INT8, "f32": 0, "f32q": _lib.BSTREAM_REQUANT}


def kernel_name(form, listed):
    return f"beam_streams_kernel:{form}{',list' if listed else ''}"


def out_dtype(form):
    return np.float32 if form == "f32" else np.int8


def reference(y, index, form):
    return R.beam_streams(y, index, scale=R.SCALE if form == "f32q" else None)


def run(context, queue, y, index, form):
    """The C entry point on `y` with `index` (None: no list), into an output prefilled with 0x5A."""
    B, _, C, NB, _, M2 = y.shape
    M, T = M2 // 2, NB * 16
    K = M if index is None else len(index)
    d_y = accel.DeviceArray(context, y.shape, y.dtype)
    d_y.set(queue, y)
    d_out = accel.DeviceArray(context, (B, K, C, T, 2, 2), out_dtype(form))
    _lib.call("bf_memset", d_out.ptr, 0x5A, d_out.nbytes, queue.handle)
    d_idx = None
    if index is not None:
        d_idx = accel.DeviceArray(context, (K,), np.int32)
        d_idx.set(queue, np.asarray(index, np.int64).astype(np.int32))
    _lib.call("bf_beam_streams", d_y.ptr, None if d_idx is None else d_idx.ptr, d_out.ptr, B, C, T, M, K, FLAGS[form],
              R.SCALE, queue.handle)
    assert _lib.load().bf_last_kernel().decode() == kernel_name(form, index is not None)
    out = d_out.get(queue)
    np.testing.assert_array_equal(d_y.get(queue).view(np.uint8), y.view(np.uint8))  # the input is never written
    return out


def check(got, y, index, form):
    ref = reference(y, index, form)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    np.testing.assert_array_equal(R.as_bytes(got), R.as_bytes(ref))


_beams = {}


def beams_of(B, C, T, M, form):
    key = (B, C, T, M, form == "i8")
    if key not in _beams:
        _beams[key] = R.random_beams(B, C, T, M, form == "i8")
        _beams[key].flags.writeable = False
    return _beams[key]


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("CT", [(1, 16), (3, 48), (2, 256)], ids=lambda v: f"C{v[0]}T{v[1]}")
@pytest.mark.parametrize("M", [1, 2, 3, 5, 16, 17, 64, 65])
def test_shape_grid(context, command_queue, M, CT, B, form):
    C, T = CT
    y = beams_of(B, C, T, M, form)
    check(run(context, command_queue, y, None, form), y, None, form)


@pytest.mark.parametrize("form", ["i8", "f32"])
@pytest.mark.parametrize("M,C", [(257, 2), (4096, 1)])
def test_rows_wider_than_a_tile(context, command_queue, M, C, form):
    y = beams_of(1, C, 16, M, form)
    check(run(context, command_queue, y, None, form), y, None, form)


@pytest.mark.parametrize("form", R.FORMS)
def test_long_runs_take_the_xcd_range_order(context, command_queue, form):
    """M = 4 over 4096 samples: 8 (int8) or 16 tiles with stream runs of 1 KiB or more, the shape at which the launch
    deals the tiles to the XCDs in ranges instead of round-robin (a multiple of 8 workgroups)."""
    y = beams_of(1, 16, 256, 4, form)
    check(run(context, command_queue, y, None, form), y, None, form)
    check(run(context, command_queue, y, [3, 0, 9, 1, 1], form), y, [3, 0, 9, 1, 1], form)


def lists(M):
    return {"reversed": list(range(M))[::-1], "repeat": [3, 3, 3], "one": [M - 2],
            "twice": [(7 * k + 1) % M for k in range(2 * M)],
            "outside": [1, -1, 0, M, M - 1, 2 ** 31 - 1, 2]}


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("which", ["reversed", "repeat", "one", "twice", "outside"])
@pytest.mark.parametrize("M", [64, 5])
def test_lists(context, command_queue, M, which, form):
    y = beams_of(2, 3, 48, M, form)
    index = lists(M)[which]
    got = run(context, command_queue, y, index, form)
    check(got, y, index, form)
    if which == "outside":
        assert not R.as_bytes(got[:, [1, 3, 5]]).any()
        for k in (0, 2, 4, 6):  # the neighbours are streams of real beams
            assert R.as_bytes(got[:, k]).any()
            np.testing.assert_array_equal(R.as_bytes(got[:, k]), R.as_bytes(reference(y, [index[k]], form)[:, 0]))


@pytest.mark.parametrize("inverse", [False, True], ids=["one-hot", "one-cold"])
@pytest.mark.parametrize("form", ["i8", "f32"])
@pytest.mark.parametrize("M,hot", [(5, 2), (65, 64), (257, 52)])
def test_isolation(context, command_queue, M, hot, form, inverse):
    """One beam at full scale (-128; for f32 a NaN with a payload) among zero beams, and the inverse: a kernel that
    mixes neighbouring beams or pols shows it in the zero streams."""
    B, C, T = 1, 2, 48
    full = np.int8(-128) if form == "i8" else np.array([0x7fc12345], np.uint32).view(np.float32)[0]
    y = np.zeros((B, 2, C, T // 16, 16, 2 * M), np.int8 if form == "i8" else np.float32)
    cols = y.reshape(B, 2, C, T, M, 2)
    if inverse:
        cols[...] = full
        cols[:, :, :, :, hot] = 0
    else:
        cols[:, 0, :, :, hot, 0] = full  # pol 0, re only: the other pol and im of the same beam stay zero
    got = run(context, command_queue, y, None, form)
    check(got, y, None, form)
    others = [m for m in range(M) if m != hot]
    if inverse:
        assert not R.as_bytes(got[:, hot]).any() and R.as_bytes(got[:, others]).all()
    else:
        assert not R.as_bytes(got[:, others]).any()
        assert R.as_bytes(got[:, hot, :, :, 0, 0]).any() and not R.as_bytes(got[:, hot, :, :, 1]).any()
        assert not R.as_bytes(got[:, hot, :, :, 0, 1]).any()


@pytest.mark.parametrize("listed", [False, True], ids=["identity", "list"])
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("T", [16, 48])
@pytest.mark.parametrize("M", [3, 65])
def test_guard_bands(context, command_queue, M, T, form, listed):
    """REPEAT, ORACLE, GUARD, INPUT and KERNEL of guarded.py, the buffers at their minimum alignment: beams and out at
    offset 16, the list at offset 4."""
    B, C = 2, 3
    y = beams_of(B, C, T, M, form)
    index = [M - 1, 0, -1, 1, 1, M] if listed else None
    K = len(index) if listed else M
    bufs = [G.inp("beams", y, 16), G.out("out", (B, K, C, T, 2, 2), out_dtype(form), 16)]
    if listed:
        bufs.append(G.inp("index", np.asarray(index, np.int32), 4))
    ex = G.DeviceExecutor(context, command_queue)

    def launch(p):
        _lib.call("bf_beam_streams", p["beams"], p.get("index"), p["out"], B, C, T, M, K, FLAGS[form], R.SCALE,
                  command_queue.handle)

    def oracle(outs):
        check(outs["out"], y, index, form)

    G.run_case(ex, bufs, launch, oracle, kernel_name(form, listed))


def test_operator_after_the_fused_beamformer(context, command_queue):
    """FusedBeamformer(out_int8=True).outData bound to BeamStreams.inBeams: the streams equal the restatement applied
    to the fused output (itself the oracle's integer contract); select_beams takes effect on the next launch."""
    B, A, M, C, Ctot, T = 2, 64, 16, 3, 4096, 64
    rng = np.random.default_rng(31)
    d1 = np.zeros((1, M, A, 4), np.float32)
    d1[..., 0] = rng.uniform(0, 10 * O.TS_MEERKAT, (M, A))
    d1[..., 2] = rng.uniform(-np.pi, np.pi, (M, A))
    raw = rng.integers(-128, 128, (B, A, C, T, 2, 2), dtype=np.int8)
    fused = FusedBeamformerTemplate(context, B, C, Ctot, T, A, M, delay_channels=1, sample_signed=True, out_int8=True,
                                    out_scale=1 / 64).instantiate(command_queue)
    first = [5, 0, 15, 5]
    tmpl = BeamStreamsTemplate(context, B, C, T, M, in_int8=True, beams=first)
    streams = tmpl.instantiate(command_queue)
    fused.ensure_all_bound()
    streams.bind(inBeams=fused.buffer("outData"))
    streams.ensure_all_bound()
    assert streams.buffer("inBeams") is fused.buffer("outData")
    fused.buffer("inSamples").set(command_queue, raw)
    fused.buffer("delay_vals").set(command_queue, d1)
    fused()
    streams()
    y = fused.buffer("outData").get(command_queue)
    np.testing.assert_array_equal(y, O.fused_beamform_int8(raw, d1, Ctot, scale=1 / 64, signed=True))
    got = streams.buffer("outStreams").get(command_queue)
    assert got.shape == tmpl.output_shape == (B, 4, C, T, 2, 2) and got.dtype == np.int8
    np.testing.assert_array_equal(got, R.beam_streams(y, first))
    assert _lib.load().bf_last_kernel().decode() == kernel_name("i8", True)
    second = [1, 2, 3, 4]
    streams.select_beams(second)
    np.testing.assert_array_equal(streams.buffer("outStreams").get(command_queue), got)  # nothing until the launch
    streams()
    np.testing.assert_array_equal(streams.buffer("outStreams").get(command_queue), R.beam_streams(y, second))
    np.testing.assert_array_equal(streams.beams(), second)
    # every beam, no list, float32 requantised, through the operator
    y32 = R.random_beams(B, C, T, M, False)
    op = BeamStreamsTemplate(context, B, C, T, M, requantise=True, scale=R.SCALE).instantiate(command_queue)
    op.ensure_all_bound()
    op.buffer("inBeams").set(command_queue, y32)
    op()
    np.testing.assert_array_equal(op.buffer("outStreams").get(command_queue), R.beam_streams(y32, None, R.SCALE))
    assert _lib.load().bf_last_kernel().decode() == kernel_name("f32q", False)


@pytest.fixture(scope="module")
def composed(context, command_queue):
    """B1 K3 C2 T32: int8 streams of beams [4, 0, 4] of 5, left on the device, with their restatement."""
    B, K, C, T, M = 1, 3, 2, 32, 5
    y = beams_of(B, C, T, M, "i8")
    op = BeamStreamsTemplate(context, B, C, T, M, in_int8=True, beams=[4, 0, 4]).instantiate(command_queue)
    op.ensure_all_bound()
    op.buffer("inBeams").set(command_queue, y)
    op()
    ref = R.beam_streams(y, [4, 0, 4])
    np.testing.assert_array_equal(op.buffer("outStreams").get(command_queue), ref)
    return op, ref, (B, K, C, T)


def test_streams_bind_to_the_voltage_statistics(context, command_queue, composed):
    op, ref, (B, K, C, T) = composed
    limits = (0.5, 1.5)
    stats = VoltageStatsTemplate(context, B, C, T, K, integration=16, sample_signed=True, scale=R.SCALE,
                                 sk_limits=limits).instantiate(command_queue)
    stats.bind(inSamples=op.buffer("outStreams"))
    stats.ensure_all_bound()
    assert stats.buffer("inSamples") is op.buffer("outStreams")
    stats()
    power, sk, flags = VR.voltage_stats(ref, 16, True, R.SCALE, limits)
    for name, want in (("outPower", power), ("outSK", sk), ("outFlags", flags)):
        np.testing.assert_array_equal(R.as_bytes(stats.buffer(name).get(command_queue)), R.as_bytes(want), err_msg=name)


def test_streams_bind_to_the_correlator(context, command_queue, composed):
    op, ref, (B, K, C, T) = composed
    corr = CorrelatorTemplate(context, B, C, T, K, integration=16, sample_signed=True).instantiate(command_queue)
    corr.bind(inSamples=op.buffer("outStreams"))
    corr.ensure_all_bound()
    assert corr.buffer("inSamples") is op.buffer("outStreams")
    corr()
    vis = corr.buffer("outVisibilities").get(command_queue)
    want = CR.visibilities(ref, 16, 1, True)
    assert vis.shape == want.shape
    np.testing.assert_array_equal(vis, want)
    # streams 0 and 2 are the same beam: their cross-correlation is that beam's auto-correlation
    np.testing.assert_array_equal(vis[..., 3, :, :, :], vis[..., 0, :, :, :])
