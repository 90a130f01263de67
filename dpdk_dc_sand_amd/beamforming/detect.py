"""Beam detector: Stokes power of the beams, integrated in time and frequency (MI355X-native operator, no reference
counterpart).

What pulsar and transient searches, filterbank recorders and beam monitors take from a B-engine is the detected beam:
|X|^2 + |Y|^2 per beam (Stokes I), or I, Q, U, V, summed over `time_integration` samples and `channel_integration`
channels.  `BeamDetector.inBeams` has the shape and dtype of `FusedBeamformer.outData` (float32, or int8 with
`in_int8`), so the beamformer's output buffer binds to it directly and the beams never leave the device.

Contract (bf_beam_detect, include/bf.h): out = float32(float64(acc) * float64(float32(scale))).  With int8 beams acc is
the exact integer sum (bit-exact, whatever the order); with float32 beams it is a float64 sum of exact float64 products
in the kernel's fixed order.
"""
import numpy as np

from .. import _lib, accel


class BeamDetectorTemplate:
    """Template for the beam detector.

    Parameters
    ----------
    context, n_batches, n_channels_per_stream, n_samples_per_channel, n_beams -- as FusedBeamformerTemplate.
    time_integration: samples per output window; divides n_samples_per_channel.
    channel_integration: channels per output channel; divides n_channels_per_stream.
    stokes: "I" (one output) or "IQUV" (four).
    in_int8: the beams are int8 (FusedBeamformerTemplate(out_int8=True)) instead of float32.
    scale: finite and > 0; applied once, in float64, to the window sum.
    """

    MAX_BEAMS = 4096
    MAX_SAMPLES = 1 << 20
    MAX_WINDOW = 1 << 31

    def __init__(self, context, n_batches: int, n_channels_per_stream: int, n_samples_per_channel: int, n_beams: int,
                 time_integration: int = 16, channel_integration: int = 1, stokes: str = "I", in_int8: bool = False,
                 scale: float = 1.0) -> None:
        for name, v in dict(n_batches=n_batches, n_channels_per_stream=n_channels_per_stream,
                            n_samples_per_channel=n_samples_per_channel, n_beams=n_beams,
                            time_integration=time_integration, channel_integration=channel_integration).items():
            if int(v) <= 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if n_samples_per_channel % 16:
            raise ValueError("n_samples_per_channel must be a multiple of 16")
        if n_samples_per_channel > self.MAX_SAMPLES:
            raise ValueError(f"n_samples_per_channel must be at most {self.MAX_SAMPLES}")
        if n_beams > self.MAX_BEAMS:
            raise ValueError(f"n_beams must be at most {self.MAX_BEAMS}, got {n_beams}")
        tint, fint = int(time_integration), int(channel_integration)
        if n_samples_per_channel % tint:
            raise ValueError(f"time_integration {tint} must divide n_samples_per_channel")
        if n_channels_per_stream % fint:
            raise ValueError(f"channel_integration {fint} must divide n_channels_per_stream")
        if tint * fint > self.MAX_WINDOW:
            raise ValueError(f"time_integration * channel_integration must be at most {self.MAX_WINDOW}")
        if stokes not in ("I", "IQUV"):
            raise ValueError(f"stokes must be 'I' or 'IQUV', got {stokes!r}")
        if not (np.isfinite(np.float32(scale)) and np.float32(scale) > 0):
            raise ValueError("scale must be finite and > 0")
        self.context = context
        self.n_batches = n_batches
        self.n_channels_per_stream = n_channels_per_stream
        self.n_samples_per_channel = n_samples_per_channel
        self.n_beams = n_beams
        self.time_integration = tint
        self.channel_integration = fint
        self.stokes = stokes
        self.n_stokes = len(stokes)
        self.in_int8 = bool(in_int8)
        self.scale = float(np.float32(scale))
        self.flags = (_lib.DETECT_IN_INT8 if self.in_int8 else 0) | (_lib.DETECT_STOKES_IQUV if stokes == "IQUV" else 0)
        B, C, T, M = n_batches, n_channels_per_stream, n_samples_per_channel, n_beams
        self.input_shape = (B, 2, C, T // 16, 16, 2 * M)
        self.output_shape = (B, self.n_stokes, C // fint, T // tint, M)

    def algorithmic_bytes(self):
        """HBM bytes one launch must move: the beams once, the output once."""
        return _lib.load().bf_detect_algorithmic_bytes(self.n_batches, self.n_channels_per_stream,
                                                       self.n_samples_per_channel, self.n_beams,
                                                       self.time_integration, self.channel_integration, self.flags)

    def instantiate(self, command_queue):
        return BeamDetector(self, command_queue)


class BeamDetector(accel.Operation):
    """.. rubric:: Slots
    inBeams: (n_batches, 2, n_channels_per_stream, n_samples_per_channel // 16, 16, 2 * n_beams), float32 (int8 with
        in_int8) -- FusedBeamformer.outData
    outData: (n_batches, n_stokes, n_channels_per_stream // channel_integration,
        n_samples_per_channel // time_integration, n_beams), float32
    """

    def __init__(self, template: BeamDetectorTemplate, command_queue):
        super().__init__(command_queue)
        self.template = t = template
        self.slots["inBeams"] = accel.IOSlot(t.input_shape, np.int8 if t.in_int8 else np.float32)
        self.slots["outData"] = accel.IOSlot(t.output_shape, np.float32)

    def _run(self):
        t = self.template
        _lib.call("bf_beam_detect", self.buffer("inBeams").ptr, self.buffer("outData").ptr, t.n_batches,
                  t.n_channels_per_stream, t.n_samples_per_channel, t.n_beams, t.time_integration,
                  t.channel_integration, t.flags, t.scale, self.command_queue.handle)
