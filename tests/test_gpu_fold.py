"""GPU: the folder (bf_fold, csrc/bf_fold.hip; beamforming.fold) against the NumPy restatement of its contract
(fold_ref.py): bit for bit on integer-valued power, within the derived float64 bound (fold_ref.tolerance) on Gaussian
power, `hits` always exact, untouched accumulator elements and the memory behind the accumulators unchanged, the
inputs unchanged, two launches identical.

Shapes are (B, S, K, J, M, F, nbin).  A workgroup owns a channel and stages its (S, samples, M) tile in LDS, in chunks
where S * N * M floats exceed 8192; a row (f, k) belongs to 16, 32 or 64 lanes of one wave, which walk it in passes.
Beyond the issue's list, because none of its shapes needs more than one chunk:
  ten chunks of 4 samples, 16-byte staging     (1,4,2,40,512,3,8)
  chunks of one sample, element staging         (1,4,2,5,1025,2,4): J*M odd
  chunks of one sample, element staging         (1,4,2,2,1026,2,4): J*M a multiple of 4, the chunk's offsets not
  three chunks of four, four and two passes     (1,1,2,600,32,3,16): a bin recurs across passes and across chunks
  a batch boundary inside a chunk               (2,2,3,100,48,5,9): chunks of 64 samples, batches of 100
  the largest tile, 64 KiB                      (1,4,1,2,4096,2,4): one sample of 4 planes of 4096 beams per chunk
Every shape runs with every phase table (T = 2^64, one turn): random; still (dphase 0: one bin per row); half (T/2: two
bins alternate); slow (T // (5 nbin): runs of five); msp (T // 7 + 1: a wrap every seven samples, the same bins again
in every pass); back (T - T // (3 nbin): phase decreasing); edge (phase0 - chan = T - 1, dphase 1: the last bin, then
bin 0)."""
import ctypes
import functools

import numpy as np
import pytest

import detect_ref
import fold_ref as R
import oracle as O
from dpdk_dc_sand_amd import _lib, accel
from dpdk_dc_sand_amd.beamforming import (BeamDetectorTemplate, FolderTemplate, FusedBeamformerTemplate,
                                          fold_channel_phases, fold_phase_step)
from test_fold_host import PULSE, check_pulse, pulse_freqs, pulse_stream

pytestmark = pytest.mark.gpu

T = 1 << 64
TAIL = 1024
SENTINEL64, SENTINEL32 = 0x7ff8beefbeefbeef, 0x7fc0beef

GRID = [(1, 1, 1, 1, 1, 1, 1), (1, 1, 3, 4, 1, 2, 3), (2, 4, 5, 8, 3, 5, 16), (1, 1, 4, 64, 16, 16, 64),
        (1, 1, 3, 65, 1, 1, 7), (2, 1, 2, 65, 17, 3, 1000), (1, 4, 2, 16, 64, 64, 32), (1, 1, 2, 128, 16, 16, 4096),
        (1, 1, 130, 16, 4, 4, 8), (1, 1, 2, 300, 2, 2, 5), (1, 1, 1, 2, 4096, 2, 4),
        # beyond the issue's list (module docstring)
        (1, 4, 2, 40, 512, 3, 8), (1, 4, 2, 5, 1025, 2, 4), (1, 4, 2, 2, 1026, 2, 4), (1, 1, 2, 600, 32, 3, 16),
        (2, 2, 3, 100, 48, 5, 9), (1, 4, 1, 2, 4096, 2, 4)]
TABLES = ["random", "still", "half", "slow", "msp", "back", "edge"]


def ident(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


@functools.lru_cache(maxsize=None)
def inputs(shape, integer):
    """power of a shape, never modified: integers in [0, 2^12), or Gaussian f32 of rms 1000."""
    B, S, K, J, M, F, nbin = shape
    rng = np.random.default_rng(sum(shape) + integer)
    if integer:
        power = rng.integers(0, 1 << 12, (B, S, K, J, M)).astype(np.float32)
    else:
        power = (1000 * rng.standard_normal((B, S, K, J, M))).astype(np.float32)
    power.setflags(write=False)
    return power


@functools.lru_cache(maxsize=None)
def prior(shape):
    """(profile: random integers below 2^40, hits: random counts), never modified."""
    B, S, K, J, M, F, nbin = shape
    rng = np.random.default_rng(sum(shape) + 2)
    profile = rng.integers(0, 1 << 40, (F, S, K, nbin)).astype(np.float64)
    hits = rng.integers(0, 1 << 31, (F, K, nbin), dtype=np.uint32)
    profile.setflags(write=False)
    hits.setflags(write=False)
    return profile, hits


def rand64(rng, shape):
    return rng.integers(0, 1 << 64, shape, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def table(shape, kind):
    """(beam list, phase0 (F), dphase (F), chan (F, K)) as read-only arrays; the beams repeat where F >= 2."""
    B, S, K, J, M, F, nbin = shape
    rng = np.random.default_rng(sum(shape) + 3)
    beam = rng.integers(0, M, F).tolist()
    if F >= 2:
        beam[1] = beam[0]
    phase0, dphase, chan = rand64(rng, F), rand64(rng, F), rand64(rng, (F, K))
    step = dict(still=0, half=T // 2, slow=T // (5 * nbin), msp=T // 7 + 1, back=T - T // (3 * nbin), edge=1).get(kind)
    if step is not None:
        dphase = R.u64([step] * F)
    if kind == "edge":
        chan = np.repeat(chan[:, :1], K, axis=1)
        phase0 = R.u64([(int(c) - 1) % T for c in chan[:, 0]])
    for a in (phase0, dphase, chan):
        a.setflags(write=False)
    return tuple(beam), phase0, dphase, chan


@functools.lru_cache(maxsize=None)
def reference(shape, integer, kind):
    """fold_ref.fold over the prior; shared, never modified."""
    B, S, K, J, M, F, nbin = shape
    beam, phase0, dphase, chan = table(shape, kind)
    out = R.fold(inputs(shape, integer), beam, phase0, dphase, chan, nbin, *prior(shape))
    for a in out:
        a.setflags(write=False)
    return out


def launch(context, queue, power, beam, phase0, dphase, chan, nbin, profile, hits):
    """bf_fold on device copies with a sentinel tail behind both accumulators: (profile bits with the tail, hits with
    the tail, power and chan read back)."""
    B, S, K, J, M = power.shape
    F = len(beam)
    d_power = accel.DeviceArray(context, power.shape, np.float32)
    d_chan = accel.DeviceArray(context, chan.shape, np.uint64)
    d_profile = accel.DeviceArray(context, (profile.size + TAIL,), np.uint64)
    d_hits = accel.DeviceArray(context, (hits.size + TAIL,), np.uint32)
    d_power.set(queue, power)
    d_chan.set(queue, chan)
    d_profile.set(queue, np.concatenate([np.ascontiguousarray(profile).view(np.uint64).ravel(),
                                         np.full(TAIL, SENTINEL64, np.uint64)]))
    d_hits.set(queue, np.concatenate([np.ascontiguousarray(hits).ravel(), np.full(TAIL, SENTINEL32, np.uint32)]))
    _lib.call("bf_fold", d_power.ptr, (_lib.c_int * F)(*beam), (ctypes.c_uint64 * F)(*phase0.tolist()),
              (ctypes.c_uint64 * F)(*dphase.tolist()), d_chan.ptr, d_profile.ptr, d_hits.ptr, B, S, K, J, M, F, nbin,
              queue.handle)
    assert _lib.load().bf_last_kernel().startswith(b"fold_kernel")
    return d_profile.get(queue), d_hits.get(queue), d_power.get(queue), d_chan.get(queue)


def run(context, queue, shape, integer, kind, profile, hits):
    beam, phase0, dphase, chan = table(shape, kind)
    power = inputs(shape, integer)
    got_p, got_h, got_power, got_chan = launch(context, queue, power, beam, phase0, dphase, chan, shape[6], profile,
                                               hits)
    assert (got_p[profile.size:] == SENTINEL64).all() and (got_h[hits.size:] == SENTINEL32).all()  # the tails
    assert got_power.tobytes() == power.tobytes() and got_chan.tobytes() == chan.tobytes()         # the inputs
    return got_p[:profile.size].reshape(profile.shape), got_h[:hits.size].reshape(hits.shape)


@pytest.mark.parametrize("shape", GRID, ids=ident)
@pytest.mark.parametrize("kind", TABLES)
def test_integer_power_is_bit_exact(context, command_queue, shape, kind):
    """Integer-valued power in [0, 2^12) over a prior of integers below 2^40: profile and hits bit for bit (untouched
    elements included: the reference leaves them at the prior's bits), tails and inputs unchanged, and a second launch
    on equal inputs gives equal bytes."""
    ref_p, ref_h, _, _, count = reference(shape, True, kind)
    assert count.sum() == shape[5] * shape[2] * shape[0] * shape[3]
    got_p, got_h = run(context, command_queue, shape, True, kind, *prior(shape))
    np.testing.assert_array_equal(got_p, ref_p.view(np.uint64))
    np.testing.assert_array_equal(got_h, ref_h)
    again_p, again_h = run(context, command_queue, shape, True, kind, *prior(shape))
    assert again_p.tobytes() == got_p.tobytes() and again_h.tobytes() == got_h.tobytes()


@pytest.mark.parametrize("shape", GRID, ids=ident)
@pytest.mark.parametrize("kind", TABLES)
def test_gaussian_power_is_within_the_bound(context, command_queue, shape, kind):
    """Gaussian power of rms 1000: every element within t * 2^-52 * (|pre| + sum|x|), untouched elements bit for bit,
    hits exact, and two launches identical."""
    ref_p, ref_h, _, absx, count = reference(shape, False, kind)
    pre, pre_h = prior(shape)
    got_bits, got_h = run(context, command_queue, shape, False, kind, pre, pre_h)
    got_p = got_bits.view(np.float64)
    tol = R.tolerance(pre, absx, count)
    err = np.abs(got_p - ref_p)
    assert np.isfinite(got_p).all() and (err <= tol).all(), (float((err / np.maximum(tol, 1e-300)).max()),
                                                             int((err > tol).sum()))
    untouched = np.broadcast_to((count == 0)[:, None], pre.shape)
    np.testing.assert_array_equal(got_bits[untouched], pre.view(np.uint64)[untouched])
    np.testing.assert_array_equal(got_h, ref_h)
    again_bits, again_h = run(context, command_queue, shape, False, kind, pre, pre_h)
    assert again_bits.tobytes() == got_bits.tobytes() and again_h.tobytes() == got_h.tobytes()


@pytest.mark.parametrize("shape", GRID, ids=ident)
@pytest.mark.parametrize("kind", TABLES)
def test_untouched_elements_keep_their_bits(context, command_queue, shape, kind):
    """Accumulators filled with the byte 0x5A: an element that receives no sample still holds it, a touched hit count
    grew by its samples."""
    _, _, _, _, count = reference(shape, True, kind)
    pre, pre_h = prior(shape)
    fill_p = np.full(pre.shape, 0x5A5A5A5A5A5A5A5A, np.uint64).view(np.float64)
    fill_h = np.full(pre_h.shape, 0x5A5A5A5A, np.uint32)
    got_bits, got_h = run(context, command_queue, shape, True, kind, fill_p, fill_h)
    untouched = np.broadcast_to((count == 0)[:, None], pre.shape)
    assert (got_bits[untouched] == 0x5A5A5A5A5A5A5A5A).all()
    np.testing.assert_array_equal(got_h, (0x5A5A5A5A + count).astype(np.uint32))


def reference_phases(folds, seen, N, ts):
    """The operator's phase step of a call that starts at stream position `seen`, restated: the spin at mid-time."""
    return [fold_phase_step(spin + dot * (seen + N / 2) * ts, ts) for _, spin, _, dot, _ in folds]


def test_bound_to_the_chain(context, command_queue):
    """FusedBeamformer(out_int8) -> BeamDetector(tint 16, fint 2, IQUV, scale 1) -> Folder at A = 64, M = 16, C = 8,
    T = 256, B = 2 on one queue, the slots bound, not copied.  Three calls on three voltage cubes: the dumped profile
    and hits equal fold_ref of detect_ref of the oracle's int8 beams with the phase advanced call by call, bit for bit;
    after reset() the calls give identical bytes."""
    B, A, M, C, Ctot, Tn, tint, fint, nbin, calls, ts = 2, 64, 16, 8, 4096, 256, 16, 2, 16, 3, 76.6e-6
    K, J = C // fint, Tn // tint
    N = B * J
    rng = np.random.default_rng(23)
    d1 = np.zeros((1, M, A, 4), np.float32)
    d1[..., 0] = rng.uniform(0, 10 * O.TS_MEERKAT, (M, A))
    d1[..., 2] = rng.uniform(-np.pi, np.pi, (M, A))
    raw = rng.integers(-128, 128, (calls, B, A, C, Tn, 2, 2), dtype=np.int8)
    freqs = np.linspace(856e6, 1712e6, K, endpoint=False)
    folds = [(3, 218.8, 40.0, 0.0, 0.0), (3, 1234.5, 12.0, 2.5, 0.3), (0, 2.0, 100.0, 0.0, 0.75),
             (15, 6000.0, 3.0, 0.0, 0.5)]
    fused = FusedBeamformerTemplate(context, B, C, Ctot, Tn, A, M, delay_channels=1, sample_signed=True, out_int8=True,
                                    out_scale=1 / 64).instantiate(command_queue)
    det = BeamDetectorTemplate(context, B, C, Tn, M, time_integration=tint, channel_integration=fint, stokes="IQUV",
                               in_int8=True, scale=1.0).instantiate(command_queue)
    tmpl = FolderTemplate(context, B, K, J, M, nbin, folds, freqs, ts, n_stokes=4)
    fold = tmpl.instantiate(command_queue)
    fused.ensure_all_bound()
    det.bind(inBeams=fused.buffer("outData"))
    det.ensure_all_bound()
    fold.bind(inPower=det.buffer("outData"))
    fold.ensure_all_bound()
    assert det.buffer("inBeams") is fused.buffer("outData") and fold.buffer("inPower") is det.buffer("outData")
    fused.buffer("delay_vals").set(command_queue, d1)
    runs = []
    for _ in range(2):
        for c in range(calls):
            assert fold.samples_seen == c * N
            fused.buffer("inSamples").set(command_queue, raw[c])
            fused()
            det()
            fold()
        runs.append(fold.dump())
        fold.reset()
        assert fold.samples_seen == 0
    chan = np.stack([fold_channel_phases(f[1], f[2], freqs) for f in folds])
    phase = [int(np.ldexp(f[4], 64)) for f in folds]
    profile, hits = np.zeros(tmpl.profile_shape), np.zeros(tmpl.hits_shape, np.uint32)
    for c in range(calls):
        y = O.fused_beamform_int8(raw[c], d1, Ctot, scale=1 / 64, signed=True)
        power = detect_ref.beam_detect(y, tint, fint, iquv=True, scale=1.0)
        assert power.shape == tmpl.input_shape and power[:, 0].any() and power[:, 0].max() < 2 ** 23
        steps = reference_phases(folds, c * N, N, ts)
        profile, hits = R.fold(power, [f[0] for f in folds], R.u64(phase), R.u64(steps), chan, nbin, profile, hits)[:2]
        phase = [(p + N * s) % T for p, s in zip(phase, steps)]
    assert fold.phase == [int(np.ldexp(f[4], 64)) for f in folds]  # reset
    assert runs[0][0].tobytes() == profile.tobytes() and runs[0][1].tobytes() == hits.tobytes()
    assert hits.sum() == len(folds) * K * calls * N and profile.any()
    assert runs[1][0].tobytes() == runs[0][0].tobytes() and runs[1][1].tobytes() == runs[0][1].tobytes()


def test_set_spin_and_dump(context, command_queue):
    """Two calls, dump, set_spin on fold 0, two calls, dump: the first dump equals the reference of two calls; dump
    zeroes the accumulators and set_spin keeps the phase, so the second dump equals the reference of the next two calls
    from zeroed accumulators, the phases carried on and fold 0 at its new spin and channel phases."""
    B, S, K, J, M, nbin, ts = 2, 2, 6, 24, 4, 12, 1e-4
    N = B * J
    rng = np.random.default_rng(31)
    power = rng.integers(0, 1 << 12, (4, B, S, K, J, M)).astype(np.float32)
    freqs = np.linspace(1e9, 1.5e9, K)
    folds = [(2, 700.0, 30.0, 0.0, 0.1), (2, 33.0, 5.0, 0.5, 0.0), (1, 4999.0, 1.0, 0.0, 0.9)]
    op = FolderTemplate(context, B, K, J, M, nbin, folds, freqs, ts, n_stokes=S).instantiate(command_queue)
    op.ensure_all_bound()
    beam = [f[0] for f in folds]
    chan = np.stack([fold_channel_phases(f[1], f[2], freqs) for f in folds])
    phase = [int(np.ldexp(f[4], 64)) for f in folds]
    spins = [[f[1], f[3], 0] for f in folds]  # spin, derivative, epoch
    for half in range(2):
        ref_p, ref_h = np.zeros(op.template.profile_shape), np.zeros(op.template.hits_shape, np.uint32)
        for c in (2 * half, 2 * half + 1):
            op.buffer("inPower").set(command_queue, power[c])
            op()
            steps = [fold_phase_step(s + d * (c * N + N / 2 - e) * ts, ts) for s, d, e in spins]
            ref_p, ref_h = R.fold(power[c], beam, R.u64(phase), R.u64(steps), chan, nbin, ref_p, ref_h)[:2]
            phase = [(p + N * s) % T for p, s in zip(phase, steps)]
        assert op.phase == phase and op.samples_seen == (2 * half + 2) * N
        got_p, got_h = op.dump()
        assert got_p.tobytes() == ref_p.tobytes() and got_h.tobytes() == ref_h.tobytes() and ref_h.any()
        if half == 0:
            op.set_spin(0, 650.0, 100.0)
            assert op.phase == phase  # kept
            spins[0] = [650.0, 100.0, 2 * N]
            chan[0] = fold_channel_phases(650.0, 30.0, freqs)
    empty_p, empty_h = op.dump()  # nothing since the last dump
    assert not empty_p.any() and not empty_h.any()


def test_planted_pulse_through_the_operator(context, command_queue):
    """test_fold_host.py's stream (a dispersed Gaussian pulse in beam 1 over Poisson noise, 40 calls) through Folder
    with the folds (beam 1), (beam 1, DM 0: no correction), (beam 0): every channel of the first peaks in bin 8, the
    second smears over the bins, the third shows nothing."""
    P = PULSE
    power = pulse_stream()
    folds = [(1, P["spin"], P["dm"]), (1, P["spin"], 0.0), (0, P["spin"], P["dm"])]
    op = FolderTemplate(context, 1, P["K"], P["J"], P["M"], P["nbin"], folds, pulse_freqs(),
                        P["ts"]).instantiate(command_queue)
    op.ensure_all_bound()
    for c in range(P["calls"]):
        op.buffer("inPower").set(command_queue, power[c])
        op()
    profile, hits = op.dump()
    check_pulse(profile, hits)
