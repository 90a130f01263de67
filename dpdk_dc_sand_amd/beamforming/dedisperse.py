"""Dedisperser: DM-trial time series of the detected beams (MI355X-native operator, no reference counterpart).

A dispersed pulse arrives later at the bottom of the band than at the top; summing the channels of
`BeamDetector.outData` without undoing that sweep smears it away.  `Dedisperser.inPower` has the shape of
`BeamDetector.outData`, so the detector's output buffer binds to it directly; `outData` is (n_beams, n_trials, N), one
contiguous time series per beam and trial dispersion measure, N = n_batches * n_windows new samples per call.  The
operator owns a ring of the recent past of the power stream on the device, the device copy of the lag table and the
ring's head, which every call advances.

Contract (bf_dedisperse, include/bf.h): out[m][d][n] = float32(float64(scale) * sum over k of the ring sample of
channel k that lies lags[d][k] samples before sample n), a float64 sum of the f32 values in the kernel's fixed order:
bit-exact for integer-valued power below 2^24, within K * 2^-53 * sum|x| otherwise.
"""
import numpy as np

from .. import _lib, accel

DISPERSION_CONSTANT_S = 4.148808e3  # s MHz^2 pc^-1 cm^3


def dispersion_lags(dms, freqs_hz, sample_time):
    """The lag table of a set of trial dispersion measures: (lags int32 (D, K), latency).

    delay[d][k] = rint(4.148808e3 s * DM_d * (f_k,MHz^-2 - f_max,MHz^-2) / sample_time) samples (float64), latency the
    largest delay of the table, lags = latency - delay: every trial has the same latency, and output sample tau of the
    stream is emission time tau - latency at the top of the band.
    """
    dms = np.atleast_1d(np.asarray(dms, np.float64))
    f = np.atleast_1d(np.asarray(freqs_hz, np.float64)) / 1e6
    if dms.ndim != 1 or f.ndim != 1 or dms.size == 0 or f.size == 0:
        raise ValueError("dms and freqs_hz must be one-dimensional and not empty")
    if not (np.isfinite(dms).all() and (dms >= 0).all()):
        raise ValueError("dispersion measures must be finite and >= 0")
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError("frequencies must be finite and > 0")
    if not (np.isfinite(sample_time) and sample_time > 0):
        raise ValueError("sample_time must be finite and > 0")
    delay = np.rint(DISPERSION_CONSTANT_S * dms[:, None] * (f[None, :] ** -2 - f.max() ** -2) / float(sample_time))
    if delay.max() > 2 ** 31 - 1:
        raise ValueError("delays exceed 2^31 - 1 samples")
    latency = int(delay.max())
    return (latency - delay).astype(np.int32), latency


class DedisperserTemplate:
    """Template for the dedisperser.

    Parameters
    ----------
    context: as the other templates.
    n_batches, n_channels, n_windows, n_beams: B, K, J, M of BeamDetector.outData (B, n_stokes, K, J, M); a call brings
        N = B * J samples.
    lags: host integer (D, K) table, every entry in [0, ring_length - N] (dispersion_lags makes one).
    ring_length: slots of the ring, a multiple of N; default the smallest multiple of N that is at least N + max lag.
    n_stokes, plane: the Stokes planes of the input and the one that is dedispersed.
    scale: finite and > 0; applied once, in float64, to the channel sum.
    """

    MAX_BEAMS = 4096
    MAX_TRIALS = 4096

    def __init__(self, context, n_batches: int, n_channels: int, n_windows: int, n_beams: int, lags,
                 ring_length=None, n_stokes: int = 1, plane: int = 0, scale: float = 1.0) -> None:
        for name, v in dict(n_batches=n_batches, n_channels=n_channels, n_windows=n_windows, n_beams=n_beams,
                            n_stokes=n_stokes).items():
            if int(v) <= 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if n_beams > self.MAX_BEAMS:
            raise ValueError(f"n_beams must be at most {self.MAX_BEAMS}, got {n_beams}")
        if not 0 <= int(plane) < n_stokes:
            raise ValueError(f"plane {plane} outside [0, {n_stokes})")
        if not (np.isfinite(np.float32(scale)) and np.float32(scale) > 0):
            raise ValueError("scale must be finite and > 0")
        table = np.asarray(lags)
        if table.ndim != 2 or table.shape[1] != n_channels or table.shape[0] == 0:
            raise ValueError(f"lags must have the shape (n_trials, {n_channels}), got {table.shape}")
        if not np.issubdtype(table.dtype, np.integer):
            raise ValueError(f"lags must be integers, got {table.dtype}")
        if table.shape[0] > self.MAX_TRIALS:
            raise ValueError(f"at most {self.MAX_TRIALS} trials, got {table.shape[0]}")
        N = int(n_batches) * int(n_windows)
        if N > 2 ** 31 - 1:
            raise ValueError("n_batches * n_windows exceeds 2^31 - 1")
        lo, hi = int(table.min()), int(table.max())
        if ring_length is None:
            ring_length = N * (1 + -(-max(hi, 0) // N))
        ring_length = int(ring_length)
        if ring_length < N or ring_length % N or ring_length > 2 ** 31 - 1:
            raise ValueError(f"ring_length {ring_length} must be a multiple of N = {N} below 2^31")
        if lo < 0 or hi > ring_length - N:
            raise ValueError(f"lag {lo if lo < 0 else hi} outside [0, ring_length - N = {ring_length - N}]")
        self.context = context
        self.n_batches, self.n_channels, self.n_windows, self.n_beams = n_batches, n_channels, n_windows, n_beams
        self.n_stokes, self.plane = n_stokes, int(plane)
        self.n_samples = N
        self.lags = np.ascontiguousarray(table, np.int32)
        self.lags.setflags(write=False)
        self.n_trials = table.shape[0]
        self.ring_length = ring_length
        self.scale = float(np.float32(scale))
        self.span_sum = int((table.max(axis=0).astype(np.int64) - table.min(axis=0)).sum())
        self.input_shape = (n_batches, n_stokes, n_channels, n_windows, n_beams)
        self.output_shape = (n_beams, self.n_trials, N)
        self.ring_shape = (n_channels, ring_length, n_beams)

    def algorithmic_bytes(self):
        """HBM bytes one launch must move: the block read and appended, every ring sample that some trial needs read
        once, the output once."""
        return _lib.load().bf_dedisperse_algorithmic_bytes(self.n_batches, self.n_channels, self.n_windows,
                                                           self.n_beams, self.n_trials, self.span_sum)

    def instantiate(self, command_queue):
        return Dedisperser(self, command_queue)


class Dedisperser(accel.Operation):
    """.. rubric:: Slots
    inPower: (n_batches, n_stokes, n_channels, n_windows, n_beams), float32 -- BeamDetector.outData
    outData: (n_beams, n_trials, n_batches * n_windows), float32

    The ring (n_channels, ring_length, n_beams) and the device lag table are allocated at the first call; `head` is the
    ring slot of the next call's first sample, `samples_seen` the stream position (samples per channel taken so far).
    """

    def __init__(self, template: DedisperserTemplate, command_queue):
        super().__init__(command_queue)
        self.template = t = template
        self.slots["inPower"] = accel.IOSlot(t.input_shape, np.float32)
        self.slots["outData"] = accel.IOSlot(t.output_shape, np.float32)
        self.ring = None
        self._lags = None
        self.head = 0
        self.samples_seen = 0

    def _state(self):
        if self.ring is None:
            t, q = self.template, self.command_queue
            self.ring = accel.DeviceArray(q.context, t.ring_shape, np.float32)
            self.ring.zero(q)
            self._lags = accel.DeviceArray(q.context, t.lags.shape, np.int32)
            self._lags.set_async(q, t.lags)  # stream-ordered before the first launch; the template keeps the host copy

    def reset(self):
        """Forget the past: zero the ring (stream-ordered), head and samples_seen."""
        if self.ring is not None:
            self.ring.zero(self.command_queue)
        self.head = 0
        self.samples_seen = 0

    def _run(self):
        t = self.template
        self._state()
        _lib.call("bf_dedisperse", self.buffer("inPower").ptr, self.ring.ptr, self._lags.ptr,
                  self.buffer("outData").ptr, t.n_batches, t.n_stokes, t.plane, t.n_channels, t.n_windows, t.n_beams,
                  t.n_trials, t.ring_length, self.head, t.scale, self.command_queue.handle)
        self.head = (self.head + t.n_samples) % t.ring_length
        self.samples_seen += t.n_samples
