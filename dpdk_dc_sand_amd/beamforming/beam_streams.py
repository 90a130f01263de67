"""Beam streams: the beams as per-beam voltage streams, any subset (MI355X-native operator, no reference counterpart:
the reference has a PreBeamformReorder before the contraction and nothing after it).

The fused operator writes the reference's MatrixMultiply layout (B, 2, C, T/16, 16, 2M): the beam index is the fastest
axis and the two pols are separate planes.  A consumer of beam m -- one subscriber, one recorder, one multicast group
per beam -- needs (channel, time, pol) of that beam contiguous.  `BeamStreams.inBeams` has the shape and dtype of
`FusedBeamformer.outData`; `outStreams` is (B, K, C, T, 2, 2), K streams in the order of the beam list, each with the
shape and sample order of one antenna of the voltage cube.  The int8 streams therefore bind directly to
`VoltageStats(sample_signed=True, n_ants=K).inSamples` (spectral kurtosis of a beam), `Correlator(sample_signed=True)`
(cross-correlation of beams) and `IncoherentBeam(sample_signed=True)`.

Contract (bf_beam_streams, include/bf.h): out[b, k, c, t, p, z] = beams[b, p, c, t/16, t%16, 2 m + z], m = the k-th
entry of the list; a copy of bits (NaN payloads, -0.0, -128 unchanged), or with requantise=True
clamp(rne(f32 * scale), -127, 127) as `Requant`, bit-exact.
"""
import numpy as np

from .. import _lib, accel


class BeamStreamsTemplate:
    """Template for the beam streams.

    Parameters
    ----------
    context, n_batches, n_channels_per_stream, n_samples_per_channel, n_beams -- as FusedBeamformerTemplate.
    in_int8: the beams are int8 (FusedBeamformer(out_int8=True)), else float32.
    requantise: float32 beams, int8 streams: clamp(rne(y * scale), -127, 127).  Not with in_int8.
    scale: finite and > 0 when requantising; ignored otherwise.
    beams: the list of beams to stream, K entries in [0, n_beams): repeats, any order and K > n_beams are allowed.
        None = every beam in order (no list on the device; select_beams is not available).
    """

    MAX_BEAMS = 4096
    MAX_SAMPLES = 1 << 20

    def __init__(self, context, n_batches: int, n_channels_per_stream: int, n_samples_per_channel: int, n_beams: int,
                 in_int8: bool = False, requantise: bool = False, scale: float = 1.0, beams=None) -> None:
        for name, v in dict(n_batches=n_batches, n_channels_per_stream=n_channels_per_stream,
                            n_samples_per_channel=n_samples_per_channel, n_beams=n_beams).items():
            if int(v) <= 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if n_samples_per_channel % 16:
            raise ValueError("n_samples_per_channel must be a multiple of 16")
        if n_samples_per_channel > self.MAX_SAMPLES:
            raise ValueError(f"n_samples_per_channel must be at most {self.MAX_SAMPLES}")
        if n_beams > self.MAX_BEAMS:
            raise ValueError(f"n_beams must be at most {self.MAX_BEAMS}, got {n_beams}")
        if requantise and in_int8:
            raise ValueError("requantise needs float32 beams, not in_int8")
        if requantise and not (np.isfinite(np.float32(scale)) and np.float32(scale) > 0):
            raise ValueError("scale must be finite and > 0")
        self.context = context
        self.n_batches = n_batches
        self.n_channels_per_stream = n_channels_per_stream
        self.n_samples_per_channel = n_samples_per_channel
        self.n_beams = n_beams
        self.in_int8 = bool(in_int8)
        self.requantise = bool(requantise)
        self.scale = float(np.float32(scale)) if requantise else 1.0
        self.beams = None if beams is None else self.check_beams(beams)
        self.n_streams = n_beams if self.beams is None else self.beams.size
        self.flags = ((_lib.BSTREAM_IN_INT8 if self.in_int8 else 0) | (_lib.BSTREAM_REQUANT if self.requantise else 0) |
                      (_lib.BSTREAM_LIST if self.beams is not None else 0))
        B, C, T, M, K = n_batches, n_channels_per_stream, n_samples_per_channel, n_beams, self.n_streams
        self.input_shape = (B, 2, C, T // 16, 16, 2 * M)
        self.output_shape = (B, K, C, T, 2, 2)
        self.input_dtype = np.int8 if self.in_int8 else np.float32
        self.output_dtype = np.int8 if self.in_int8 or self.requantise else np.float32
        if _lib.load().bf_beam_streams_algorithmic_bytes(B, C, T, M, K, self.flags) == 0:
            raise ValueError(f"shape B={B} C={C} T={T} M={M} K={K} needs more than 2^31 - 1 workgroups")

    def check_beams(self, beams, length=None):
        """The list as an int32 array, or ValueError: one dimension, 1 .. 4096 integer entries in [0, n_beams), and
        `length` entries when given."""
        a = np.asarray(beams)
        if a.ndim != 1 or a.size == 0 or a.size > self.MAX_BEAMS:
            raise ValueError(f"beams must be a list of 1 .. {self.MAX_BEAMS} beam indices")
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"beams must be integers, got {a.dtype}")
        if length is not None and a.size != length:
            raise ValueError(f"{a.size} beams received, expected {length}")
        if a.min() < 0 or a.max() >= self.n_beams:
            raise ValueError(f"beam {int(a.min() if a.min() < 0 else a.max())} out of range [0, {self.n_beams})")
        return a.astype(np.int32)

    def algorithmic_bytes(self):
        """HBM bytes one launch must move: the whole beam cube once (a dense read, whatever the list), every stream
        once, the list once."""
        return _lib.load().bf_beam_streams_algorithmic_bytes(self.n_batches, self.n_channels_per_stream,
                                                             self.n_samples_per_channel, self.n_beams, self.n_streams,
                                                             self.flags)

    def instantiate(self, command_queue):
        return BeamStreams(self, command_queue)


class BeamStreams(accel.Operation):
    """.. rubric:: Slots
    inBeams: (n_batches, 2, n_channels_per_stream, n_samples_per_channel // 16, 16, 2 * n_beams), float32 (int8 with
        in_int8) -- FusedBeamformer.outData
    outStreams: (n_batches, n_streams, n_channels_per_stream, n_samples_per_channel, 2, 2), the dtype of inBeams (int8
        with requantise)
    beamIndex: (n_streams,), int32 -- with a beam list
    """

    def __init__(self, template: BeamStreamsTemplate, command_queue):
        super().__init__(command_queue)
        self.template = t = template
        self.slots["inBeams"] = accel.IOSlot(t.input_shape, t.input_dtype)
        self.slots["outStreams"] = accel.IOSlot(t.output_shape, t.output_dtype)
        self._beams = None
        if t.beams is not None:
            self.slots["beamIndex"] = accel.IOSlot((t.n_streams,), np.int32)
            self._beams = t.beams.copy()
            self._beams_dirty = True

    def select_beams(self, beams):
        """Replace the beam list by one of the same length.  Takes effect from the next launch (stream-ordered
        upload)."""
        if self._beams is None:
            raise ValueError("operator was built without a beam list")
        self._beams = self.template.check_beams(beams, self.template.n_streams)
        self._beams_dirty = True

    def beams(self):
        """The current beam list (host copy); None without a list (every beam in order)."""
        return None if self._beams is None else self._beams.copy()

    def _run(self):
        t = self.template
        index = None
        if self._beams is not None:
            buf = self.buffer("beamIndex")
            if self._beams_dirty:
                buf.set_async(self.command_queue, self._beams)
                self._beams_dirty = False
            index = buf.ptr
        _lib.call("bf_beam_streams", self.buffer("inBeams").ptr, index, self.buffer("outStreams").ptr, t.n_batches,
                  t.n_channels_per_stream, t.n_samples_per_channel, t.n_beams, t.n_streams, t.flags, t.scale,
                  self.command_queue.handle)
