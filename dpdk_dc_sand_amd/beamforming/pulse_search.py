"""Pulse search: boxcar S/N and peak candidates of the DM trials (MI355X-native operator, no reference counterpart).

The last stage of FusedBeamformer -> BeamDetector -> Dedisperser -> PulseSearch.  `PulseSearch.inSeries` has the shape
of `Dedisperser.outData`, so the dedisperser's output buffer binds to it directly.  Every (beam, trial) row is matched
against boxcars of a list of widths, normalised by a running baseline (mean and variance of the last `baseline_blocks`
calls, the current one included); `outPeaks` (n_beams, n_trials, 4) holds one record per row, `outBest` (n_beams, 4) one
per beam: 16 bytes per (beam, trial) and 16 bytes per beam leave the GPU per call, not the time series.  The operator
owns the ring of the recent past of the series, the block moments of the baseline and their state, which every call
advances.

Contract (bf_pulse_search, include/bf.h): snr_w[n] = float32((cnt * s_w[n] - w * S1) / sqrt(w * (cnt * S2 - S1^2))), 0
where the denominator is not positive; s_w[n] the float64 sum of the w samples that END at sample n -- the centre of a
pulse found at (n, w) is at n - (w - 1) / 2 -- and S1, S2, cnt the baseline's sum, sum of squares and sample count.  Per
sample the best width (ties to the smaller width index), per row the peak {snr bits, n, width index, count of samples at
or above the threshold}, per beam the best row {snr bits, trial, n, width index}.  Bit-exact for integer-valued series
whose sums stay below 2^53.
"""
import numpy as np

from .. import _lib, accel

CANDIDATE_DTYPE = np.dtype([("snr", np.float32), ("beam", np.int32), ("trial", np.int32), ("sample", np.int64),
                            ("width_index", np.int32), ("count", np.int32)])


def candidates(peaks, threshold, samples_seen_before=0):
    """Decode a read-back `outPeaks` (n_beams, n_trials, 4) int32: a structured array (snr, beam, trial, sample,
    width_index, count) of the records with snr >= threshold, beam-major.  `sample` is the stream position
    samples_seen_before + n of the sample at which the boxcar ends."""
    peaks = np.ascontiguousarray(peaks, np.int32)
    if peaks.ndim != 3 or peaks.shape[2] != 4:
        raise ValueError(f"peaks must have the shape (n_beams, n_trials, 4), got {peaks.shape}")
    snr = peaks[..., 0].copy().view(np.float32)
    beam, trial = np.nonzero(snr >= np.float32(threshold))
    out = np.zeros(beam.size, CANDIDATE_DTYPE)
    out["snr"] = snr[beam, trial]
    out["beam"], out["trial"] = beam, trial
    out["sample"] = int(samples_seen_before) + peaks[beam, trial, 1].astype(np.int64)
    out["width_index"] = peaks[beam, trial, 2]
    out["count"] = peaks[beam, trial, 3]
    return out


class PulseSearchTemplate:
    """Template for the pulse search.

    Parameters
    ----------
    context: as the other templates.
    n_beams, n_trials, n_samples: M, D, N of Dedisperser.outData (M, D, N).
    widths: boxcar widths in samples: 1 to 16 of them, strictly ascending, each in 1..1024.
    baseline_blocks: P, the calls the baseline spans (1..64); default min(64, ceil(4096 / N)).
    threshold: finite; a row's record counts its samples at or above it.
    ring_length: slots of the ring, a multiple of N; default the smallest multiple of N that is at least
        N + max width - 1.
    series: also write the per-sample best S/N and width index (outSnr, outWidth).
    """

    MAX_BEAMS = 4096
    MAX_TRIALS = 4096
    MAX_WIDTHS = 16
    MAX_WIDTH = 1024
    MAX_BLOCKS = 64

    def __init__(self, context, n_beams: int, n_trials: int, n_samples: int, widths=(1, 2, 4, 8, 16, 32, 64, 128),
                 baseline_blocks=None, threshold: float = 6.0, ring_length=None, series: bool = False) -> None:
        for name, v in dict(n_beams=n_beams, n_trials=n_trials, n_samples=n_samples).items():
            if int(v) <= 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if n_beams > self.MAX_BEAMS:
            raise ValueError(f"n_beams must be at most {self.MAX_BEAMS}, got {n_beams}")
        if n_trials > self.MAX_TRIALS:
            raise ValueError(f"n_trials must be at most {self.MAX_TRIALS}, got {n_trials}")
        N = int(n_samples)
        if N > 2 ** 31 - 1:
            raise ValueError("n_samples exceeds 2^31 - 1")
        w = np.asarray(widths)
        if w.ndim != 1 or not 1 <= w.size <= self.MAX_WIDTHS:
            raise ValueError(f"widths must be a list of 1 to {self.MAX_WIDTHS} values, got the shape {w.shape}")
        if not np.issubdtype(w.dtype, np.integer):
            raise ValueError(f"widths must be integers, got {w.dtype}")
        if w.min() < 1 or w.max() > self.MAX_WIDTH or (np.diff(w.astype(np.int64)) <= 0).any():
            raise ValueError(f"widths must be strictly ascending in 1..{self.MAX_WIDTH}, got {w.tolist()}")
        wmax = int(w[-1])
        if baseline_blocks is None:
            baseline_blocks = min(self.MAX_BLOCKS, -(-4096 // N))
        baseline_blocks = int(baseline_blocks)
        if not 1 <= baseline_blocks <= self.MAX_BLOCKS:
            raise ValueError(f"baseline_blocks {baseline_blocks} outside 1..{self.MAX_BLOCKS}")
        if baseline_blocks * N >= 2 ** 31:
            raise ValueError(f"baseline_blocks * n_samples = {baseline_blocks * N} at or above 2^31")
        if not np.isfinite(np.float32(threshold)):
            raise ValueError("threshold must be finite")
        if ring_length is None:
            ring_length = N * -(-(N + wmax - 1) // N)
        ring_length = int(ring_length)
        if ring_length % N or ring_length < N + wmax - 1 or ring_length > 2 ** 31 - 1:
            raise ValueError(f"ring_length {ring_length} must be a multiple of N = {N} that is at least "
                             f"N + max width - 1 = {N + wmax - 1}, below 2^31")
        self.context = context
        self.n_beams, self.n_trials, self.n_samples = int(n_beams), int(n_trials), N
        self.widths = np.ascontiguousarray(w, np.int32)
        self.widths.setflags(write=False)
        self.max_width = wmax
        self.baseline_blocks = baseline_blocks
        self.threshold = float(np.float32(threshold))
        self.ring_length = ring_length
        self.series = bool(series)
        self.flags = _lib.PSEARCH_SERIES if series else 0
        self.input_shape = (self.n_beams, self.n_trials, N)
        self.peaks_shape = (self.n_beams, self.n_trials, 4)
        self.best_shape = (self.n_beams, 4)
        self.ring_shape = (self.n_beams, self.n_trials, ring_length)
        self.moments_shape = (self.n_beams, self.n_trials, baseline_blocks, 2)

    def algorithmic_bytes(self):
        """HBM bytes one call must move: the block read and appended, the history read once, the moment slots, the
        peak and best records, the optional series."""
        return _lib.load().bf_pulse_search_algorithmic_bytes(self.n_beams, self.n_trials, self.n_samples,
                                                             self.widths.size, self.max_width, self.baseline_blocks,
                                                             self.flags)

    def instantiate(self, command_queue):
        return PulseSearch(self, command_queue)


class PulseSearch(accel.Operation):
    """.. rubric:: Slots
    inSeries: (n_beams, n_trials, n_samples), float32 -- Dedisperser.outData
    outPeaks: (n_beams, n_trials, 4), int32 -- {snr bits, n, width index, count at or above the threshold} per row
    outBest: (n_beams, 4), int32 -- {snr bits, trial, n, width index} per beam
    with series=True only: outSnr (n_beams, n_trials, n_samples) float32 and outWidth, the same shape, uint8

    A boxcar of width w ENDS at the sample n a record names: the centre of the pulse is at n - (w - 1) / 2.  The ring
    (n_beams, n_trials, ring_length) and the block moments (n_beams, n_trials, baseline_blocks, 2) are allocated and
    zeroed at the first call, stream-ordered; `head` is the ring slot of the next call's first sample, `slot` the moment
    slot the next call writes, `n_blocks` how many slots are filled, `samples_seen` the stream position.
    """

    def __init__(self, template: PulseSearchTemplate, command_queue):
        super().__init__(command_queue)
        self.template = t = template
        self.slots["inSeries"] = accel.IOSlot(t.input_shape, np.float32)
        self.slots["outPeaks"] = accel.IOSlot(t.peaks_shape, np.int32)
        self.slots["outBest"] = accel.IOSlot(t.best_shape, np.int32)
        if t.series:
            self.slots["outSnr"] = accel.IOSlot(t.input_shape, np.float32)
            self.slots["outWidth"] = accel.IOSlot(t.input_shape, np.uint8)
        self.ring = None
        self.moments = None
        self._widths = (_lib.c_int * t.widths.size)(*t.widths.tolist())
        self.head = self.slot = self.n_blocks = self.samples_seen = 0

    def _state(self):
        if self.ring is None:
            t, q = self.template, self.command_queue
            self.ring = accel.DeviceArray(q.context, t.ring_shape, np.float32)
            self.ring.zero(q)
            self.moments = accel.DeviceArray(q.context, t.moments_shape, np.float64)
            self.moments.zero(q)

    def reset(self):
        """Forget the past: zero the ring and the moments (stream-ordered), head, slot, n_blocks and samples_seen."""
        if self.ring is not None:
            self.ring.zero(self.command_queue)
            self.moments.zero(self.command_queue)
        self.head = self.slot = self.n_blocks = self.samples_seen = 0

    def _run(self):
        t = self.template
        self._state()
        n_blocks = min(self.n_blocks + 1, t.baseline_blocks)  # the current block included
        _lib.call("bf_pulse_search", self.buffer("inSeries").ptr, self.ring.ptr, self.moments.ptr, self._widths,
                  self.buffer("outSnr").ptr if t.series else None, self.buffer("outWidth").ptr if t.series else None,
                  self.buffer("outPeaks").ptr, self.buffer("outBest").ptr, t.n_beams, t.n_trials, t.n_samples,
                  t.ring_length, self.head, t.baseline_blocks, self.slot, n_blocks, t.widths.size, t.threshold, t.flags,
                  self.command_queue.handle)
        self.head = (self.head + t.n_samples) % t.ring_length
        self.slot = (self.slot + 1) % t.baseline_blocks
        self.n_blocks = n_blocks
        self.samples_seen += t.n_samples
