"""The dedisperser without a GPU: the feature query, bf_dedisperse's argument validation (fake pointers, as
test_beam_streams_host.py: validation fails before anything touches a device), the byte count, dispersion_lags, the
template, and the NumPy restatement of the contract (dedisperse_ref.py): chained calls over a ring equal the one-shot
dedispersion of the whole stream, and float32 accumulation is not the contract."""
import numpy as np
import pytest

import dedisperse_ref as R
from dpdk_dc_sand_amd import _lib
from dpdk_dc_sand_amd.beamforming import (BeamDetectorTemplate, DedisperserTemplate, dispersion_lags)

FAKE = 1 << 20  # 16-byte aligned, never dereferenced


def test_has_feature():
    lib = _lib.load()
    assert lib.bf_has_feature(b"dedisperse") == 1
    assert lib.bf_has_feature(b"dedisp") == 0
    assert lib.bf_abi_version() == 302


GOOD = dict(power=FAKE, ring=FAKE, lags=FAKE, out=FAKE, B=2, S=4, plane=1, K=5, J=8, M=3, D=7, R=48, head=16,
            scale=1.0)


def call(**kw):
    a = dict(GOOD, **kw)
    return _lib.call("bf_dedisperse", a["power"], a["ring"], a["lags"], a["out"], a["B"], a["S"], a["plane"], a["K"],
                     a["J"], a["M"], a["D"], a["R"], a["head"], a["scale"], None)


def byte_count(**kw):
    a = dict(GOOD, **kw)
    return _lib.load().bf_dedisperse_algorithmic_bytes(a["B"], a["K"], a["J"], a["M"], a["D"], 11)


REFUSED = [
    (dict(power=None), "null pointer"), (dict(ring=None), "null pointer"), (dict(lags=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(B=0), "bad shape"), (dict(S=0), "bad shape"), (dict(K=0), "bad shape"), (dict(J=0), "bad shape"),
    (dict(M=0), "bad shape"), (dict(D=0), "bad shape"), (dict(B=-1), "bad shape"),
    (dict(plane=-1), "plane"), (dict(plane=4), "plane"),
    (dict(M=4097), "above 4096"), (dict(D=4097), "above 4096"),
    (dict(R=8), "ring length"), (dict(R=40), "ring length"), (dict(R=0), "ring length"),
    (dict(head=-16), "head"), (dict(head=48), "head"), (dict(head=8), "head"),
    (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(scale=float("inf")), "scale"),
    (dict(power=FAKE + 8), "misaligned"), (dict(ring=FAKE + 4), "misaligned"), (dict(out=FAKE + 8), "misaligned"),
    (dict(lags=FAKE + 2), "misaligned"),
]


@pytest.mark.parametrize("kw,match", REFUSED, ids=[f"{'-'.join(k)}={list(k.values())[0]}" for k, _ in REFUSED])
def test_argument_validation_without_gpu(kw, match):
    lib = _lib.load()
    before = lib.bf_last_kernel()
    with pytest.raises(_lib.BeamformerError, match=match) as e:
        call(**kw)
    assert e.value.status == -1  # BF_ERR_ARG
    assert lib.bf_last_kernel() == before  # refused before any launch
    if set(kw) & {"B", "K", "J", "M", "D"}:  # the shapes the byte count can see
        assert byte_count(**kw) == 0


@pytest.mark.parametrize("B,K,J,M,D,span", [(8, 4096, 16, 16, 256, 12345678), (1, 4096, 16, 64, 64, 0),
                                            (2, 5, 8, 3, 7, 11), (1, 1, 1, 1, 1, 0), (1, 2, 3, 4096, 4096, 5)])
def test_algorithmic_bytes(B, K, J, M, D, span):
    f = _lib.load().bf_dedisperse_algorithmic_bytes
    N = B * J
    assert f(B, K, J, M, D, span) == 4 * (2 * K * N * M + (K * N + span) * M + D * N * M)
    assert f(B, K, J, M, D, -1) == 0
    assert f(65536, K, 65536, M, D, span) == 0  # N = B*J beyond int
    lags = np.zeros((D, K), np.int32)
    if D > 1:
        lags[1, 0] = 3
    t = DedisperserTemplate(None, B, K, J, M, lags)
    assert t.span_sum == (3 if D > 1 else 0)
    assert t.algorithmic_bytes() == 4 * (2 * K * N * M + (K * N + t.span_sum) * M + D * N * M)


def test_dispersion_lags_by_hand():
    """Two channels, 1712 and 856 MHz, 76.6 us samples: the delay of the lower channel is
    4.148808e3 * DM * (856^-2 - 1712^-2) / 76.6e-6 = 55.438... samples per unit DM."""
    per_dm = 4.148808e3 * (856.0 ** -2 - 1712.0 ** -2) / 76.6e-6
    assert abs(per_dm - 55.4386) < 1e-3
    lags, latency = dispersion_lags([0.0, 1.0, 10.0], [1712e6, 856e6], 76.6e-6)
    assert lags.dtype == np.int32 and lags.shape == (3, 2)
    assert latency == 554  # rint(554.386)
    np.testing.assert_array_equal(lags, [[554, 554], [554, 554 - 55], [554, 0]])
    # the order of the channels does not matter, the top of the band is the reference
    lags2, latency2 = dispersion_lags([0.0, 1.0, 10.0], [856e6, 1712e6], 76.6e-6)
    assert latency2 == latency
    np.testing.assert_array_equal(lags2, lags[:, ::-1])


def test_dispersion_lags_properties():
    f = np.linspace(856e6, 1712e6, 64, endpoint=False)
    lags, latency = dispersion_lags([0.0], f, 76.6e-6)
    assert latency == 0 and not lags.any()  # DM 0: an all-equal table
    dms = np.arange(64.0)
    lags, latency = dispersion_lags(dms, f, 76.6e-6)
    delay = np.rint(4.148808e3 * dms[:, None] * ((f / 1e6) ** -2 - (f.max() / 1e6) ** -2)[None] / 76.6e-6)
    assert latency == int(delay.max()) and latency == latency - int(lags.min())
    np.testing.assert_array_equal(latency - lags, delay)
    assert (lags[0] == latency).all() and lags.min() == 0 and lags[-1, 0] == 0
    for bad in (dict(dms=[-1.0]), dict(dms=[float("nan")]), dict(freqs_hz=[0.0]), dict(sample_time=0.0), dict(dms=[]),
                dict(dms=[1e30])):
        with pytest.raises(ValueError):
            dispersion_lags(**dict(dict(dms=[1.0], freqs_hz=f, sample_time=76.6e-6), **bad))


def test_reference_chained_equals_one_shot():
    """K = 5, N = 8, R = 48, 9 calls (the ring wraps), random lags in [0, R - N]: chaining dedisperse_ref over a zeroed
    ring equals the one-shot dedispersion of the concatenated stream with zero prehistory, bit for bit on
    integer-valued input."""
    B, S, plane, K, J, M, D, Rn, calls = 2, 3, 1, 5, 4, 3, 6, 48, 9
    N = B * J
    rng = np.random.default_rng(5)
    lags = rng.integers(0, Rn - N + 1, (D, K)).astype(np.int32)
    lags[0], lags[1] = 0, Rn - N
    power = rng.integers(0, 1 << 20, (calls, B, S, K, J, M)).astype(np.float32)
    ring, head, outs = np.zeros((K, Rn, M), np.float32), 0, []
    for c in range(calls):
        out, ring = R.dedisperse(power[c], ring, lags, head, plane, scale=1 / 3)
        assert out.shape == (M, D, N) and out.dtype == np.float32
        outs.append(out)
        head = (head + N) % Rn
    assert head == calls * N % Rn and calls * N > Rn
    stream = power[:, :, plane].transpose(2, 0, 1, 3, 4).reshape(K, calls * N, M)  # (c, b, k, j, m) -> (k, n, m)
    ref = R.one_shot(stream, lags, scale=1 / 3)
    got = np.concatenate(outs, axis=2)
    assert got.view(np.uint32).tobytes() == ref.view(np.uint32).tobytes() and got.any()


def test_reference_against_the_element_formula():
    B, S, plane, K, J, M, D, Rn, head = 2, 2, 1, 3, 2, 2, 3, 12, 8
    N = B * J
    rng = np.random.default_rng(6)
    lags = np.array([[0, 8, 3], [-5, 9, 2 ** 31 - 1], [1, 2, 3]], np.int32)  # out-of-range entries are clamped
    power = rng.standard_normal((B, S, K, J, M)).astype(np.float32)
    ring0 = rng.standard_normal((K, Rn, M)).astype(np.float32)
    out, ring = R.dedisperse(power, ring0, lags, head, plane, scale=0.7)
    for b in range(B):
        for j in range(J):
            assert (ring[:, head + b * J + j] == power[b, plane, :, j]).all()
    untouched = np.ones(Rn, bool)
    untouched[head:head + N] = False
    assert (ring[:, untouched] == ring0[:, untouched]).all()
    for m in range(M):
        for d in range(D):
            for n in range(N):
                acc = 0.0
                for k in range(K):
                    lag = min(max(int(lags[d, k]), 0), Rn - N)
                    acc += float(ring[k, (head + n - lag) % Rn, m])
                assert out[m, d, n] == np.float32(acc * np.float64(np.float32(0.7)))


@pytest.mark.parametrize("signed", [False, True], ids=["positive", "signed"])
def test_accumulation_is_float64(signed):
    """K = 512, D = 4, N = 32, M = 4, R = 96, random lags: a float64 sum in reversed channel order violates the
    tolerance nowhere, a float32 accumulation violates it for more than 40 % of the elements."""
    K, D, N, M, Rn, head, scale = 512, 4, 32, 4, 96, 64, 1 / 3
    rng = np.random.default_rng(7 + signed)
    ring = (1000 * rng.standard_normal((K, Rn, M))).astype(np.float32)
    if not signed:
        ring = (ring * ring).astype(np.float32)
    lags = rng.integers(0, Rn - N + 1, (D, K)).astype(np.int32)
    acc, absacc = R.channel_sums(ring, lags, head, N)
    ref = R.scale_sums(acc, scale)
    tol = R.tolerance(ref, absacc, K, scale)
    slot = (head + np.arange(N)[None, None, :] - lags[:, :, None].astype(np.int64)) % Rn
    x = ring[np.arange(K)[None, :, None], slot]                                        # (D, K, N, M) f32
    rev = x[:, ::-1].astype(np.float64).sum(axis=1).transpose(2, 0, 1)
    assert not (np.abs(R.scale_sums(rev, scale).astype(np.float64) - ref) > tol).any()
    acc32 = np.zeros((D, N, M), np.float32)
    for k in range(K):
        acc32 += x[:, k]
    out32 = R.scale_sums(acc32.transpose(2, 0, 1), scale)
    bad = np.abs(out32.astype(np.float64) - ref) > tol
    assert bad.mean() > 0.4, bad.mean()


def test_template_errors():
    T = DedisperserTemplate
    lags = np.zeros((3, 5), np.int32)
    for args, match in (((0, 5, 8, 3), "n_batches"), ((2, 0, 8, 3), "n_channels"), ((2, 5, 0, 3), "n_windows"),
                        ((2, 5, 8, 0), "n_beams"), ((2, 5, 8, 4097), "n_beams")):
        with pytest.raises(ValueError, match=match):
            T(None, *args, lags)
    for kw, match in ((dict(n_stokes=0), "n_stokes"), (dict(plane=1), "plane"), (dict(n_stokes=4, plane=4), "plane"),
                      (dict(plane=-1), "plane"), (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"),
                      (dict(scale=1e-60), "scale"),
                      (dict(ring_length=40), "multiple of N"), (dict(ring_length=8), "multiple of N"),
                      (dict(ring_length=0), "multiple of N")):
        with pytest.raises(ValueError, match=match):
            T(None, 2, 5, 8, 3, lags, **kw)
    for bad, match in ((np.zeros((3, 4), np.int32), "shape"), (np.zeros(5, np.int32), "shape"),
                       (np.zeros((0, 5), np.int32), "shape"), (np.zeros((3, 5)), "integers"),
                       (np.zeros((4097, 5), np.int32), "trials")):
        with pytest.raises(ValueError, match=match):
            T(None, 2, 5, 8, 3, bad)
    # a lag outside [0, R - N]
    low, high = lags.copy(), lags.copy()
    low[1, 2], high[2, 4] = -1, 33
    with pytest.raises(ValueError, match="lag -1 outside"):
        T(None, 2, 5, 8, 3, low, ring_length=48)
    with pytest.raises(ValueError, match="lag 33 outside"):
        T(None, 2, 5, 8, 3, high, ring_length=48)
    high[2, 4] = 32
    T(None, 2, 5, 8, 3, high, ring_length=48)


def test_template_shapes_slots_and_ring_length():
    B, K, J, M, D = 2, 5, 8, 3, 4
    lags = np.zeros((D, K), np.int64)
    for hi, want in ((0, 16), (1, 32), (16, 32), (17, 48)):  # the smallest multiple of N that is >= N + max lag
        lags[1, 1] = hi
        assert DedisperserTemplate(None, B, K, J, M, lags).ring_length == want
    t = DedisperserTemplate(None, B, K, J, M, lags, n_stokes=4, plane=2, scale=1 / 3)
    assert t.lags.dtype == np.int32 and t.n_trials == D and t.n_samples == 16
    assert t.input_shape == (B, 4, K, J, M) and t.output_shape == (M, D, 16) and t.ring_shape == (K, 48, M)
    assert t.scale == float(np.float32(1 / 3))
    # inPower is BeamDetector.outData
    det = BeamDetectorTemplate(None, B, 2 * K, 16 * J, M, time_integration=16, channel_integration=2, stokes="IQUV")
    assert det.output_shape == t.input_shape
    op = t.instantiate(None)
    assert set(op.slots) == {"inPower", "outData"}
    assert op.slots["inPower"].dtype == np.float32 and op.slots["outData"].dtype == np.float32
    assert op.slots["inPower"].shape == t.input_shape and op.slots["outData"].shape == t.output_shape
    assert op.head == 0 and op.samples_seen == 0
    op.reset()
    assert op.head == 0 and op.samples_seen == 0
