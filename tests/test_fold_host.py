"""The folder without a GPU: the feature query, bf_fold's argument validation (fake device pointers, as
test_dedisperse_host.py: validation fails before anything touches a device), the byte count, the two phase helpers, the
template, and the NumPy restatement of the contract (fold_ref.py): its bins against exact integer arithmetic, chained
calls equal one fold of the whole stream, a planted dispersed pulse lands in its bin in every channel, and float32
accumulation is not the contract."""
import ctypes
import math

import numpy as np
import pytest

import fold_ref as R
from dpdk_dc_sand_amd import _lib
from dpdk_dc_sand_amd.beamforming import (BeamDetectorTemplate, Folder, FolderTemplate, fold_channel_phases,
                                          fold_phase_step, mean_profile)

FAKE = 1 << 20  # 16-byte aligned, never dereferenced
T = 1 << 64     # one turn


def test_has_feature():
    lib = _lib.load()
    assert lib.bf_has_feature(b"fold") == 1
    assert lib.bf_has_feature(b"fol") == 0
    assert lib.bf_abi_version() == 302


def host(ctype, values):
    return (ctype * len(values))(*values)


GOOD = dict(power=FAKE, beam=host(ctypes.c_int32, [2, 0, 2]), phase0=host(ctypes.c_uint64, [0, 1, T - 1]),
            dphase=host(ctypes.c_uint64, [5, 0, T // 2]), chan=FAKE, profile=FAKE, hits=FAKE, B=2, S=4, K=5, J=8, M=3,
            F=3, nbin=16)
WIDE = dict(beam=host(ctypes.c_int32, [0] * 65), phase0=host(ctypes.c_uint64, [0] * 65),
            dphase=host(ctypes.c_uint64, [1] * 65))


def call(**kw):
    a = dict(GOOD, **kw)
    return _lib.call("bf_fold", a["power"], a["beam"], a["phase0"], a["dphase"], a["chan"], a["profile"], a["hits"],
                     a["B"], a["S"], a["K"], a["J"], a["M"], a["F"], a["nbin"], None)


def byte_count(**kw):
    a = dict(GOOD, **kw)
    return _lib.load().bf_fold_algorithmic_bytes(a["B"], a["S"], a["K"], a["J"], a["M"], a["F"], 11)


REFUSED = [
    (dict(power=None), "null pointer"), (dict(beam=None), "null pointer"), (dict(phase0=None), "null pointer"),
    (dict(dphase=None), "null pointer"), (dict(chan=None), "null pointer"), (dict(profile=None), "null pointer"),
    (dict(hits=None), "null pointer"),
    (dict(B=0), "bad shape"), (dict(S=0), "bad shape"), (dict(K=0), "bad shape"), (dict(J=0), "bad shape"),
    (dict(M=0), "bad shape"), (dict(F=0), "bad shape"), (dict(nbin=0), "bad shape"), (dict(B=-1), "bad shape"),
    (dict(nbin=-3), "bad shape"),
    (dict(S=5), "above 4"), (dict(M=4097), "above 4096"), (dict(F=65, **WIDE), "above 64"),
    (dict(nbin=4097), "above 4096"), (dict(B=65536, J=32768), "above 2\\^31"), (dict(B=65536, J=65536), "above 2\\^31"),
    (dict(beam=host(ctypes.c_int32, [2, -1, 2])), "beam\\[1\\] = -1"),
    (dict(beam=host(ctypes.c_int32, [2, 0, 3])), "beam\\[2\\] = 3"),
    (dict(power=FAKE + 8), "misaligned"), (dict(chan=FAKE + 4), "misaligned"), (dict(profile=FAKE + 4), "misaligned"),
    (dict(hits=FAKE + 2), "misaligned"),
]


def refusal_id(kw):
    k, v = next(iter(kw.items()))
    return f"{k}={v if isinstance(v, int) or v is None else list(v)[:3]}" + ("" if len(kw) == 1 else "+")


@pytest.mark.parametrize("kw,match", REFUSED, ids=[refusal_id(k) for k, _ in REFUSED])
def test_argument_validation_without_gpu(kw, match):
    lib = _lib.load()
    before = lib.bf_last_kernel()
    with pytest.raises(_lib.BeamformerError, match=match) as e:
        call(**kw)
    assert e.value.status == -1  # BF_ERR_ARG
    assert lib.bf_last_kernel() == before  # refused before any launch
    if set(kw) & {"B", "S", "K", "J", "M", "F"}:  # the shapes the byte count can see
        assert byte_count(**kw) == 0


def test_the_largest_legal_sample_count_passes_the_shape_checks():
    """N = 2^31 - 1 is legal: the call gets as far as the alignment check."""
    with pytest.raises(_lib.BeamformerError, match="misaligned"):
        call(B=1, J=2 ** 31 - 1, hits=FAKE + 2)


@pytest.mark.parametrize("B,S,K,J,M,F,touched", [(8, 1, 4096, 16, 16, 16, 16 * 4096 * 128), (1, 4, 4096, 16, 64, 64, 5),
                                                 (2, 4, 5, 8, 3, 3, 11), (1, 1, 1, 1, 1, 1, 0),
                                                 (1, 4, 4096, 1, 4096, 64, 64 * 4096 * 1024)])
def test_algorithmic_bytes(B, S, K, J, M, F, touched):
    f = _lib.load().bf_fold_algorithmic_bytes
    assert f(B, S, K, J, M, F, touched) == 4 * B * S * K * J * M + 8 * F * K + touched * (16 * S + 8)
    assert f(B, S, K, J, M, F, -1) == 0
    assert f(65536, S, K, 65536, M, F, touched) == 0  # N = B*J beyond 2^31 - 1
    t = FolderTemplate(None, B, K, J, M, 8, [(0, 100.0, 1.0)] * F, np.linspace(1e9, 2e9, K), 1e-4, n_stokes=S)
    assert t.algorithmic_bytes(touched) == f(B, S, K, J, M, F, touched)


def test_algorithmic_bytes_by_hand():
    """(2, 4, 5, 8, 3) floats are 960 * 4 bytes, the channel phases of 3 folds 120 bytes, and each of 11 touched
    (fold, channel, bin) is 4 float64 and one uint32 read and written: 72 bytes."""
    assert byte_count() == 3840 + 120 + 11 * 72


def test_bins_against_exact_integers():
    """2000 random (phase0, dphase, chan, nbin <= 4096), 8 samples each: the wrapping uint64 arithmetic equals Python's
    exact integers reduced mod 2^64, and every bin is below nbin."""
    rng = np.random.default_rng(1)
    words = rng.integers(0, 1 << 32, (2000, 3, 2), dtype=np.uint64)
    nbins = rng.integers(1, 4097, 2000)
    nbins[:4] = 1, 4096, 4095, 2
    for (p, d, c), nbin in zip(words.tolist(), nbins.tolist()):
        p, d, c = ((hi << 32) | lo for hi, lo in (p, d, c))
        got = R.bins(R.u64([p]), R.u64([d]), R.u64([[c]]), 8, nbin)[0, 0]
        want = [((((p - c + n * d) % T) >> 32) * nbin) >> 32 for n in range(8)]
        assert got.tolist() == want and max(want) < nbin and min(want) >= 0


def test_bins_at_the_edge_of_a_turn():
    """phase0 - chan = 2^64 - 1 with a step of 1: the last bin, then bin 0, never bin nbin."""
    for nbin in (1, 2, 5, 1000, 4096):
        got = R.bins(R.u64([5]), R.u64([1]), R.u64([[6]]), 3, nbin)[0, 0]
        assert got.tolist() == [nbin - 1, 0, 0]


def test_reference_chained_equals_one_fold():
    """9 calls of (B 2, S 3, K 5, J 4, M 3) with 4 folds, the phase advanced as the operator does (phase += N * dphase
    mod 2^64): profile and hits equal one fold of the concatenated stream, bit for bit on integer-valued power."""
    B, S, K, J, M, F, nbin, calls = 2, 3, 5, 4, 3, 4, 7, 9
    N = B * J
    rng = np.random.default_rng(5)
    power = rng.integers(0, 1 << 20, (calls, B, S, K, J, M)).astype(np.float32)
    beam = [1, 1, 0, 2]
    phase0 = [int(x) for x in rng.integers(0, 1 << 62, F)]
    dphase = [T // 7 + 1, T // 2, 12345678901234567, T - T // 50]
    chan = R.u64(rng.integers(0, 1 << 63, (F, K)).tolist())
    profile, hits = np.zeros((F, S, K, nbin)), np.zeros((F, K, nbin), np.uint32)
    phase = list(phase0)
    for c in range(calls):
        profile, hits = R.fold(power[c], beam, R.u64(phase), R.u64(dphase), chan, nbin, profile, hits)[:2]
        phase = [(p + N * d) % T for p, d in zip(phase, dphase)]
    whole = power.reshape(calls * B, S, K, J, M)  # the batches follow one another in time
    one = R.fold(whole, beam, R.u64(phase0), R.u64(dphase), chan, nbin, np.zeros_like(profile), np.zeros_like(hits))
    assert profile.tobytes() == one[0].tobytes() and hits.tobytes() == one[1].tobytes()
    assert hits.sum() == F * K * calls * N and profile.any()


def test_reference_against_the_element_formula():
    B, S, K, J, M, F, nbin = 2, 2, 3, 3, 2, 2, 4
    rng = np.random.default_rng(6)
    power = rng.integers(0, 100, (B, S, K, J, M)).astype(np.float32)
    beam, phase0, dphase = [1, 0], [T - 3, 1 << 63], [T // 3, T // 5]
    chan = R.u64(rng.integers(0, 1 << 63, (F, K)).tolist())
    pre = rng.integers(0, 100, (F, S, K, nbin)).astype(np.float64)
    pre_hits = rng.integers(0, 100, (F, K, nbin)).astype(np.uint32)
    profile, hits, _, _, count = R.fold(power, beam, R.u64(phase0), R.u64(dphase), chan, nbin, pre, pre_hits)
    want, want_hits = pre.copy(), pre_hits.astype(np.int64)
    for f in range(F):
        for k in range(K):
            for b in range(B):
                for j in range(J):
                    phi = (phase0[f] - int(chan[f, k]) + (b * J + j) * dphase[f]) % T
                    bin_ = ((phi >> 32) * nbin) >> 32
                    want_hits[f, k, bin_] += 1
                    for s in range(S):
                        want[f, s, k, bin_] += float(power[b, s, k, j, beam[f]])
    np.testing.assert_array_equal(profile, want)
    np.testing.assert_array_equal(hits, want_hits)
    np.testing.assert_array_equal(count, want_hits - pre_hits)


def test_fold_phase_step():
    assert fold_phase_step(1.0, 0.5) == 1 << 63 and fold_phase_step(2.0, 0.125) == 1 << 62
    step = fold_phase_step(218.8, 76.6e-6)
    assert isinstance(step, int) and step == int(math.ldexp(218.8 * 76.6e-6, 64))
    assert abs(step / T - 218.8 * 76.6e-6) < 2.0 ** -60
    assert fold_phase_step(1.0, 2.0 ** -64) == 1
    for spin, ts in ((0.0, 1.0), (-1.0, 0.1), (1.0, 0.6), (float("nan"), 0.1), (float("inf"), 0.1), (1.0, 0.0)):
        with pytest.raises(ValueError, match="spin_hz \\* sample_time"):
            fold_phase_step(spin, ts)


def test_fold_channel_phases_by_hand():
    """Two channels, 1712 and 856 MHz, DM 10: the lower channel is 4.148808e3 * 10 * (856^-2 - 1712^-2) = 42.46558 ms
    late, at 100 Hz that is 4.246558 turns: the offset is 0.246558 turns."""
    delay = 4.148808e3 * 10 * (856.0 ** -2 - 1712.0 ** -2)
    assert abs(delay - 42.46558e-3) < 1e-8
    chan = fold_channel_phases(100.0, 10.0, [1712e6, 856e6])
    assert chan.dtype == np.uint64 and chan.shape == (2,)
    assert int(chan[0]) == 0 and int(chan[1]) == int(math.ldexp(math.fmod(100.0 * delay, 1.0), 64))
    assert abs(int(chan[1]) / T - 0.246558) < 1e-6
    # the order of the channels does not matter, the top of the band is the reference
    np.testing.assert_array_equal(fold_channel_phases(100.0, 10.0, [856e6, 1712e6]), chan[::-1])


def test_fold_channel_phases_properties():
    f = np.linspace(856e6, 1712e6, 64, endpoint=False)
    assert not fold_channel_phases(218.8, 0.0, f).any()  # DM 0: no offsets
    chan = fold_channel_phases(218.8, 40.0, f)
    turns = 218.8 * 4.148808e3 * 40.0 * ((f / 1e6) ** -2 - (f.max() / 1e6) ** -2)
    assert turns.max() > 30  # many turns across the band: only the fraction is kept
    err = np.abs(chan.astype(np.float64) / T - turns % 1.0)
    assert np.minimum(err, 1 - err).max() < 1e-9
    assert int(chan[np.argmax(f)]) == 0
    for bad in (dict(dm=-1.0), dict(dm=float("nan")), dict(freqs_hz=[0.0]), dict(freqs_hz=[]), dict(spin_hz=0.0),
                dict(spin_hz=float("inf")), dict(freqs_hz=[[1e9]]), dict(dm=float("inf"))):
        with pytest.raises(ValueError):
            fold_channel_phases(**dict(dict(spin_hz=1.0, dm=1.0, freqs_hz=f), **bad))


def test_mean_profile():
    profile = np.arange(24, dtype=np.float64).reshape(1, 2, 3, 4)
    hits = np.array([[[0, 1, 2, 4], [1, 1, 0, 2], [3, 0, 0, 1]]], np.uint32)
    mean = mean_profile(profile, hits)
    assert mean.shape == profile.shape and not mean[0, :, hits[0] == 0].any()
    assert mean[0, 1, 0, 3] == 15 / 4 and mean[0, 0, 2, 0] == 8 / 3 and Folder.mean_profile is mean_profile
    with pytest.raises(ValueError, match="belong together"):
        mean_profile(profile, hits[:, :2])


def test_template_errors():
    f = np.linspace(856e6, 1712e6, 5)
    folds = [(1, 218.8, 40.0), (2, 10.0, 5.0, 1e-9, 0.25)]
    for args, match in (((0, 5, 8, 3, 16), "n_batches"), ((2, 0, 8, 3, 16), "n_channels"),
                        ((2, 5, 0, 3, 16), "n_windows"),
                        ((2, 5, 8, 0, 16), "n_beams"), ((2, 5, 8, 4097, 16), "n_beams"), ((2, 5, 8, 3, 0), "n_bins"),
                        ((2, 5, 8, 3, 4097), "n_bins")):
        with pytest.raises(ValueError, match=match):
            FolderTemplate(None, *args, folds, f, 76.6e-6)
    for kw, match in ((dict(n_stokes=0), "n_stokes"), (dict(n_stokes=5), "n_stokes"),
                      (dict(sample_time=0.0), "sample_time"),
                      (dict(sample_time=float("nan")), "sample_time"), (dict(freqs_hz=f[:4]), "freqs_hz"),
                      (dict(folds=[]), "1 to 64"), (dict(folds=folds * 33), "1 to 64"),
                      (dict(folds=[(1, 218.8)]), "fold 0 must be"), (dict(folds=[(3, 218.8, 40.0)]), "beam 3 outside"),
                      (dict(folds=[(-1, 218.8, 40.0)]), "beam -1 outside"), (dict(folds=[(0.5, 218.8, 40.0)]), "beam"),
                      (dict(folds=[(1, 1e4, 40.0)]), "spin_hz \\* sample_time"),
                      (dict(folds=[(1, 0.0, 40.0)]), "spin_hz \\* sample_time"),
                      (dict(folds=[(1, 218.8, -1.0)]), "dispersion measure"),
                      (dict(folds=[(1, 218.8, 40.0, float("nan"), 0.0)]), "finite"),
                      (dict(folds=[(1, 218.8, 40.0, 0.0, float("inf"))]), "finite")):
        a = dict(dict(folds=folds, freqs_hz=f, sample_time=76.6e-6), **kw)
        with pytest.raises(ValueError, match=match):
            FolderTemplate(None, 2, 5, 8, 3, 16, a.pop("folds"), a.pop("freqs_hz"), a.pop("sample_time"), **a)
    with pytest.raises(ValueError, match="2\\^31"):
        FolderTemplate(None, 65536, 5, 65536, 3, 16, folds, f, 76.6e-6)
    FolderTemplate(None, 2, 5, 8, 3, 16, folds * 32, f, 76.6e-6, n_stokes=4)


def test_template_shapes_slots_and_state():
    B, K, J, M, nbin = 2, 5, 8, 3, 16
    f = np.linspace(856e6, 1712e6, K)
    t = FolderTemplate(None, B, K, J, M, nbin, [(1, 218.8, 40.0), (1, 300.0, 10.0, 1e-3, 0.25)], f, 76.6e-6, n_stokes=4)
    assert t.n_folds == 2 and t.n_samples == 16
    assert t.input_shape == (B, 4, K, J, M) and t.profile_shape == (2, 4, K, nbin) and t.hits_shape == (2, K, nbin)
    # inPower is BeamDetector.outData
    det = BeamDetectorTemplate(None, B, 2 * K, 16 * J, M, time_integration=16, channel_integration=2, stokes="IQUV")
    assert det.output_shape == t.input_shape
    op = t.instantiate(None)
    assert set(op.slots) == {"inPower"} and op.slots["inPower"].dtype == np.float32
    assert op.slots["inPower"].shape == t.input_shape
    assert op.phase == [0, 1 << 62] and op.samples_seen == 0
    np.testing.assert_array_equal(op.chan[1], fold_channel_phases(300.0, 10.0, f))
    # the phase step of a call is that of its mid-time
    steps = op.phase_steps()
    assert steps == [fold_phase_step(218.8, 76.6e-6), fold_phase_step(300.0 + 1e-3 * 8 * 76.6e-6, 76.6e-6)]
    # set_spin keeps the phase and re-derives the channel phases; reset goes back to the template's folds
    op.set_spin(0, 100.0, 2.0)
    assert op.phase == [0, 1 << 62]
    np.testing.assert_array_equal(op.chan[0], fold_channel_phases(100.0, 40.0, f))
    assert op.phase_steps()[0] == fold_phase_step(100.0 + 2.0 * 8 * 76.6e-6, 76.6e-6)
    for bad in ((2, 100.0), (0, 1e4), (0, 100.0, float("nan"))):
        with pytest.raises(ValueError):
            op.set_spin(*bad)
    op.reset()
    assert op.phase == [0, 1 << 62] and op.samples_seen == 0 and op.phase_steps() == steps
    np.testing.assert_array_equal(op.chan[0], fold_channel_phases(218.8, 40.0, f))


# ---- the planted pulse: shared with test_gpu_fold.py ----------------------------------------------------------------
PULSE = dict(K=64, M=3, nbin=32, J=128, calls=40, spin=218.8, dm=40.0, ts=76.6e-6, beam=1, width=0.03, amp=50.0,
             at=8.5 / 32)


def pulse_freqs():
    return np.linspace(856e6, 1712e6, PULSE["K"], endpoint=False)


def pulse_stream():
    """power (calls, 1, 1, K, J, M) f32, integer-valued: Poisson(100) noise in every beam; in beam 1 a Gaussian pulse
    of 0.03 turns and amplitude 50 emitted at phase 8.5/32, arriving in channel k its dispersive delay later."""
    P = PULSE
    rng = np.random.default_rng(40)
    K, J, M, calls = P["K"], P["J"], P["M"], P["calls"]
    power = rng.poisson(100.0, (calls, 1, 1, K, J, M)).astype(np.float64)
    f = pulse_freqs() / 1e6
    delay = 4.148808e3 * P["dm"] * (f ** -2 - f.max() ** -2)
    t = np.arange(calls * J) * P["ts"]
    emitted = P["spin"] * (t[None, :] - delay[:, None])           # the phase of what arrives in channel k at t
    d = (emitted - P["at"] + 0.5) % 1.0 - 0.5
    pulse = P["amp"] * np.exp(-0.5 * (d / P["width"]) ** 2)       # (K, calls * J)
    power[:, 0, 0, :, :, P["beam"]] += pulse.reshape(K, calls, J).transpose(1, 0, 2)
    return np.rint(power).astype(np.float32)


def check_pulse(profile, hits):
    """Folds (beam 1, corrected), (beam 1, chan zeroed), (beam 0, corrected): what the issue asks of the profiles.  The
    thresholds follow from the pulse: a bin is 1.04 sigma wide, so the peak bin's mean excess is about 48 and a
    neighbour's about 29; a channel's bin has 160 hits, noise 10 / sqrt(160) = 0.8 per channel and 0.1 over the 64."""
    P = PULSE
    K, nbin = P["K"], P["nbin"]
    assert (hits.sum(axis=(1, 2)) == K * P["J"] * P["calls"]).all()
    mean = mean_profile(profile, hits)[:, 0]                      # (3, K, nbin)
    assert (mean[0].argmax(axis=1) == 8).all()
    top = np.sort(mean[0], axis=1)
    assert (top[:, -1] - top[:, -2]).min() > 5
    assert len(set(mean[1].argmax(axis=1).tolist())) > 8
    band = mean.mean(axis=1)                                      # (3, nbin)
    over = band.max(axis=1) - np.median(band, axis=1)
    assert over[0] > 40 and over[2] < 1, over


def test_planted_pulse():
    P = PULSE
    power = pulse_stream()
    K, J, nbin = P["K"], P["J"], P["nbin"]
    chan = fold_channel_phases(P["spin"], P["dm"], pulse_freqs())
    chan = np.stack([chan, np.zeros_like(chan), chan])
    beam = [1, 1, 0]
    step = fold_phase_step(P["spin"], P["ts"])
    profile, hits, phase = np.zeros((3, 1, K, nbin)), np.zeros((3, K, nbin), np.uint32), 0
    for c in range(P["calls"]):
        profile, hits = R.fold(power[c], beam, R.u64([phase] * 3), R.u64([step] * 3), chan, nbin, profile, hits)[:2]
        phase = (phase + J * step) % T
    check_pulse(profile, hits)


@pytest.mark.parametrize("signed", [False, True], ids=["positive", "signed"])
def test_accumulation_is_float64(signed):
    """K 64, N 4096, nbin 4, Gaussian power of rms 1000, a prior of rms 1e6: a float64 sum in reversed order, or with
    the prior first, breaks the bound nowhere; a float32 partial sum breaks it for more than half of the elements."""
    K, N, nbin = 64, 4096, 4
    rng = np.random.default_rng(7 + signed)
    power = (1000 * rng.standard_normal((1, 1, K, N, 1))).astype(np.float32)
    if not signed:
        power = np.abs(power)
    pre = 1e6 * rng.standard_normal((1, 1, K, nbin))
    phase0, dphase = R.u64([123456789 << 20]), R.u64([T // 7 + 1])
    chan = R.u64(rng.integers(0, 1 << 63, (1, K)).tolist())
    ref, _, _, absx, count = R.fold(power, [0], phase0, dphase, chan, nbin, pre, np.zeros((1, K, nbin), np.uint32))
    tol = R.tolerance(pre, absx, count)
    b = R.bins(phase0, dphase, chan, N, nbin)[0]
    rev, first, f32 = (np.empty((1, 1, K, nbin)) for _ in range(3))
    for k in range(K):
        for i in range(nbin):
            x = power[0, 0, k, b[k] == i, 0]
            assert x.size == count[0, k, i] > 500
            rev[0, 0, k, i] = pre[0, 0, k, i] + np.cumsum(x[::-1].astype(np.float64))[-1]
            first[0, 0, k, i] = np.cumsum(np.concatenate([pre[0, 0, k, i:i + 1], x.astype(np.float64)]))[-1]
            f32[0, 0, k, i] = pre[0, 0, k, i] + np.float64(np.cumsum(x, dtype=np.float32)[-1])
    assert not (np.abs(rev - ref) > tol).any() and not (np.abs(first - ref) > tol).any()
    assert (np.abs(f32 - ref) > tol).mean() > 0.5
