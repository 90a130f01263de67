"""Folder: pulsar profiles of the detected beams, phase-binned (MI355X-native operator, no reference counterpart).

The other consumer of `BeamDetector.outData`, beside the search chain Dedisperser -> PulseSearch: a pulsar whose period
and dispersion measure are known (timing, a globular cluster with many pulsars in one beam, a candidate to confirm).
Every sample of every channel is added into the phase bin its rotational phase falls in, with the channel's dispersive
delay taken out; `Folder.inPower` has the shape of `BeamDetector.outData`, so the detector's output buffer binds to it
directly.  The operator owns the accumulators `profile` (n_folds, n_stokes, n_channels, n_bins) float64 and `hits`
(n_folds, n_channels, n_bins) uint32 on the device, the device table of per-channel phase offsets, and one phase per
fold, which every call advances; `dump()` reads the accumulators back and zeroes them (a sub-integration).

Contract (bf_fold, include/bf.h): the phase is fixed-point, one turn = 2^64:
    phi = phase0[f] - chan[f][k] + n * dphase[f]  (mod 2^64),  bin = ((phi >> 32) * n_bins) >> 32
    profile[f][s][k][bin] += float64(power[b][s][k][j][beam[f]]),  hits[f][k][bin] += 1
Exact integer binning (NumPy's uint64 arithmetic gives the same bins), deterministic, no atomics, bit-exact for
integer-valued power while the accumulators stay below 2^53, and an element that receives no sample is not written.
"""
import ctypes
import math

import numpy as np

from .. import _lib, accel
from .dedisperse import DISPERSION_CONSTANT_S

TURN = 1 << 64


def fold_phase_step(spin_hz, sample_time):
    """The phase step per sample of a spin frequency, in turns * 2^64, as a Python int: int(ldexp(spin_hz *
    sample_time, 64)).  0 < spin_hz * sample_time <= 0.5: at least two samples per turn."""
    x = float(spin_hz) * float(sample_time)
    if not (math.isfinite(x) and 0.0 < x <= 0.5):
        raise ValueError(f"spin_hz * sample_time must be in (0, 0.5], got {x}")
    return int(math.ldexp(x, 64))


def fold_channel_phases(spin_hz, dm, freqs_hz):
    """The per-channel phase offsets of a pulsar, uint64 (K): int(ldexp(frac(spin_hz * delay_k), 64)) mod 2^64 with
    delay_k = 4.148808e3 s * dm * (f_k,MHz^-2 - f_max,MHz^-2), the delay behind the top of the band (dispersion_lags'
    constant and reference).  bf_fold subtracts them: a pulse emitted at phase p lands in the bin of p in every channel."""
    f = np.atleast_1d(np.asarray(freqs_hz, np.float64)) / 1e6
    if f.ndim != 1 or f.size == 0:
        raise ValueError("freqs_hz must be one-dimensional and not empty")
    if not (math.isfinite(dm) and dm >= 0):
        raise ValueError("the dispersion measure must be finite and >= 0")
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError("frequencies must be finite and > 0")
    if not (math.isfinite(spin_hz) and spin_hz > 0):
        raise ValueError("spin_hz must be finite and > 0")
    turns = float(spin_hz) * (DISPERSION_CONSTANT_S * float(dm) * (f ** -2 - f.max() ** -2))
    if not np.isfinite(turns).all():
        raise ValueError("the dispersive delays are not finite")
    return np.array([int(math.ldexp(math.fmod(t, 1.0), 64)) % TURN for t in turns.tolist()], np.uint64)


def mean_profile(profile, hits):
    """profile (F, S, K, nbin) / hits (F, K, nbin), 0 where a bin has no hit."""
    profile, hits = np.asarray(profile, np.float64), np.asarray(hits)
    if profile.ndim != 4 or hits.shape != profile.shape[:1] + profile.shape[2:]:
        raise ValueError(f"profile {profile.shape} and hits {hits.shape} do not belong together")
    h = hits[:, None].astype(np.float64)
    return np.divide(profile, h, out=np.zeros_like(profile), where=h > 0)


class FolderTemplate:
    """Template for the folder.

    Parameters
    ----------
    context: as the other templates.
    n_batches, n_channels, n_windows, n_beams: B, K, J, M of BeamDetector.outData (B, n_stokes, K, J, M); a call brings
        N = B * J samples.
    n_bins: phase bins of a profile (1..4096).
    folds: 1 to 64 of (beam, spin_hz, dm) or (beam, spin_hz, dm, spin_hz_dot, phase): the beam that is folded (repeats
        allowed: several pulsars in one beam), the spin frequency at the first sample and its derivative, the dispersion
        measure, the phase of the first sample at the top of the band in turns.
    freqs_hz: the centre frequencies of the K channels.
    sample_time: seconds per sample of the detector's output.
    n_stokes: the Stokes planes of the input (1..4); all are folded.
    """

    MAX_BEAMS = 4096
    MAX_BINS = 4096
    MAX_FOLDS = 64
    MAX_STOKES = 4

    def __init__(self, context, n_batches: int, n_channels: int, n_windows: int, n_beams: int, n_bins: int, folds,
                 freqs_hz, sample_time: float, n_stokes: int = 1) -> None:
        for name, v in dict(n_batches=n_batches, n_channels=n_channels, n_windows=n_windows, n_beams=n_beams,
                            n_bins=n_bins, n_stokes=n_stokes).items():
            if int(v) <= 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if n_beams > self.MAX_BEAMS:
            raise ValueError(f"n_beams must be at most {self.MAX_BEAMS}, got {n_beams}")
        if n_bins > self.MAX_BINS:
            raise ValueError(f"n_bins must be at most {self.MAX_BINS}, got {n_bins}")
        if n_stokes > self.MAX_STOKES:
            raise ValueError(f"n_stokes must be at most {self.MAX_STOKES}, got {n_stokes}")
        N = int(n_batches) * int(n_windows)
        if N > 2 ** 31 - 1:
            raise ValueError("n_batches * n_windows exceeds 2^31 - 1")
        if not (np.isfinite(sample_time) and sample_time > 0):
            raise ValueError("sample_time must be finite and > 0")
        f = np.asarray(freqs_hz, np.float64)
        if f.shape != (n_channels,):
            raise ValueError(f"freqs_hz must have the shape ({n_channels},), got {f.shape}")
        folds = list(folds)
        if not 1 <= len(folds) <= self.MAX_FOLDS:
            raise ValueError(f"folds must be a list of 1 to {self.MAX_FOLDS} entries, got {len(folds)}")
        self.folds = []
        for i, fold in enumerate(folds):
            fold = tuple(fold)
            if len(fold) not in (3, 5):
                raise ValueError(f"fold {i} must be (beam, spin_hz, dm) or (beam, spin_hz, dm, spin_hz_dot, phase)")
            beam, spin, dm = fold[:3]
            dot, phase = fold[3:] if len(fold) == 5 else (0.0, 0.0)
            if int(beam) != beam or not 0 <= int(beam) < n_beams:
                raise ValueError(f"fold {i}: beam {beam} outside [0, {n_beams})")
            if not (math.isfinite(dot) and math.isfinite(phase)):
                raise ValueError(f"fold {i}: spin_hz_dot and phase must be finite")
            fold_phase_step(spin, sample_time)                      # raises outside (0, 0.5]
            fold_channel_phases(spin, dm, f)                        # raises on a bad dm or band
            self.folds.append((int(beam), float(spin), float(dm), float(dot), float(phase)))
        self.context = context
        self.n_batches, self.n_channels, self.n_windows, self.n_beams = n_batches, n_channels, n_windows, n_beams
        self.n_bins, self.n_stokes, self.n_folds = int(n_bins), int(n_stokes), len(self.folds)
        self.n_samples = N
        self.freqs_hz = f.copy()
        self.freqs_hz.setflags(write=False)
        self.sample_time = float(sample_time)
        self.input_shape = (n_batches, n_stokes, n_channels, n_windows, n_beams)
        self.profile_shape = (self.n_folds, self.n_stokes, n_channels, self.n_bins)
        self.hits_shape = (self.n_folds, n_channels, self.n_bins)
        self.chan_shape = (self.n_folds, n_channels)

    def algorithmic_bytes(self, touched):
        """HBM bytes one call must move when it touches `touched` distinct (fold, channel, bin): the block once, the
        channel phases, the touched accumulators read and written."""
        return _lib.load().bf_fold_algorithmic_bytes(self.n_batches, self.n_stokes, self.n_channels, self.n_windows,
                                                     self.n_beams, self.n_folds, int(touched))

    def instantiate(self, command_queue):
        return Folder(self, command_queue)


class Folder(accel.Operation):
    """.. rubric:: Slots
    inPower: (n_batches, n_stokes, n_channels, n_windows, n_beams), float32 -- BeamDetector.outData

    `profile`, `hits` and the device table of channel phases are allocated (and the accumulators zeroed) at the first
    call, stream-ordered.  `phase[f]` is the phase of the next call's first sample (a Python int, turns * 2^64),
    `samples_seen` the stream position.  A call folds with the phase step of its mid-time,
    spin_hz + spin_hz_dot * (t_mid - t_epoch), t_epoch the stream position at which the fold's spin was set (0, or the
    call before which set_spin was made), and then advances phase += N * dphase mod 2^64: calls continue each other
    exactly.  The channel phases are those of spin_hz at the epoch.
    """

    def __init__(self, template: FolderTemplate, command_queue):
        super().__init__(command_queue)
        self.template = t = template
        self.slots["inPower"] = accel.IOSlot(t.input_shape, np.float32)
        self.profile = self.hits = self._chan = None
        self._beam = (_lib.c_int * t.n_folds)(*[f[0] for f in t.folds])
        self._phase0 = (ctypes.c_uint64 * t.n_folds)()
        self._dphase = (ctypes.c_uint64 * t.n_folds)()
        self.chan = np.stack([fold_channel_phases(f[1], f[2], t.freqs_hz) for f in t.folds])  # the host copy
        self._uploads = []
        self.spin = None
        self.reset()

    def _state(self):
        if self.profile is None:
            t, q = self.template, self.command_queue
            self.profile = accel.DeviceArray(q.context, t.profile_shape, np.float64)
            self.hits = accel.DeviceArray(q.context, t.hits_shape, np.uint32)
            self.profile.zero(q)
            self.hits.zero(q)
            self._chan = accel.DeviceArray(q.context, t.chan_shape, np.uint64)
            self._chan.set_async(q, self.chan.copy())  # stream-ordered before the first launch

    def reset(self):
        """Forget everything: zero the accumulators (stream-ordered), the spins and phases go back to the template's
        folds, samples_seen = 0."""
        t = self.template
        if self.profile is not None:
            self.profile.zero(self.command_queue)
            self.hits.zero(self.command_queue)
        for f, fold in enumerate(t.folds):
            if self.spin is not None and self.spin[f][0] != fold[1]:
                self._set_chan(f, fold[1])
        self.spin = [(fold[1], fold[3], 0) for fold in t.folds]  # (spin_hz, spin_hz_dot, epoch in samples)
        self.phase = [int(math.ldexp(fold[4] % 1.0, 64)) % TURN for fold in t.folds]
        self.samples_seen = 0

    def _set_chan(self, f, spin_hz):
        t = self.template
        self.chan[f] = fold_channel_phases(spin_hz, t.folds[f][2], t.freqs_hz)
        if self._chan is not None:
            row = accel.DeviceArray(self.command_queue.context, (t.n_channels,), np.uint64,
                                    ptr=self._chan.ptr + f * t.n_channels * 8, owner=False)
            row.set_async(self.command_queue, self.chan[f].copy())
            self._uploads.append(row)  # keeps the host row alive until the queue is next synchronised (dump)

    def set_spin(self, f, spin_hz, spin_hz_dot=0.0):
        """A new spin frequency (at the next call's first sample) and derivative for fold f, from the next call on; the
        phase is kept.  The fold's channel phases are re-derived and uploaded in stream order."""
        t = self.template
        if not 0 <= int(f) < t.n_folds:
            raise ValueError(f"fold {f} outside [0, {t.n_folds})")
        if not math.isfinite(spin_hz_dot):
            raise ValueError("spin_hz_dot must be finite")
        fold_phase_step(spin_hz, t.sample_time)
        self._set_chan(int(f), float(spin_hz))
        self.spin[int(f)] = (float(spin_hz), float(spin_hz_dot), self.samples_seen)

    def phase_steps(self):
        """The phase step per sample of every fold for the next call (Python ints), evaluated at the call's mid-time."""
        t = self.template
        mid = self.samples_seen + t.n_samples / 2
        return [fold_phase_step(spin + dot * (mid - epoch) * t.sample_time, t.sample_time)
                for spin, dot, epoch in self.spin]

    def dump(self):
        """(profile, hits) as host arrays; the accumulators are zeroed in stream order (a sub-integration ends).  The
        phases run on."""
        self._state()
        q = self.command_queue
        profile = self.profile.get_async(q)
        hits = self.hits.get(q)  # synchronises the queue
        self._uploads.clear()
        self.profile.zero(q)
        self.hits.zero(q)
        return profile, hits

    mean_profile = staticmethod(mean_profile)

    def _run(self):
        t = self.template
        self._state()
        steps = self.phase_steps()
        for f in range(t.n_folds):
            self._phase0[f] = self.phase[f]
            self._dphase[f] = steps[f]
        _lib.call("bf_fold", self.buffer("inPower").ptr, self._beam, self._phase0, self._dphase, self._chan.ptr,
                  self.profile.ptr, self.hits.ptr, t.n_batches, t.n_stokes, t.n_channels, t.n_windows, t.n_beams,
                  t.n_folds, t.n_bins, self.command_queue.handle)
        self.phase = [(p + t.n_samples * s) % TURN for p, s in zip(self.phase, steps)]
        self.samples_seen += t.n_samples
