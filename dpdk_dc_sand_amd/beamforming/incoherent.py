"""Incoherent beam: masked antenna power sums of the raw voltages (MI355X-native operator, no reference counterpart).

The second standard product of a B-engine's voltages next to the tied-array beams: the power re^2 + im^2 of every
antenna, summed over a chosen set of antennas and integrated over windows of `integration` samples, per polarisation
and channel.  It is the wide-field beam, the reference level for choosing `out_scale` of the int8 beams, and a
total-power monitor with flagged antennas left out.  `IncoherentBeam.inSamples` has the shape and dtype of
`FusedBeamformer.inSamples`, so one device buffer binds to both.

Contract (bf_incoherent_beam, include/bf.h): S = the exact integer sum, out = float32(float64(S) * float64(float32(
scale))) -- deterministic and bit-exact, whatever the order of summation.
"""
import numpy as np

from .. import _lib, accel


class IncoherentBeamTemplate:
    """Template for the incoherent beam.

    Parameters
    ----------
    context, n_batches, n_channels_per_stream, n_samples_per_channel, n_ants -- as FusedBeamformerTemplate.
    integration: samples per output window; divides n_samples_per_channel and is a power of two <= 16 or a multiple
        of 16 (the 16-sample block is the time granule).
    sample_signed: read voltages as int8 instead of uint8.
    sum_pols: add the two polarisations before scaling (output has one pol).
    scale: finite and > 0; applied once, in float64, to the exact integer sum.
    antenna_mask: carry a per-antenna uint8 mask (slot antennaMask, set with set_antenna_mask; all ones initially);
        an antenna counts when its entry is non-zero, and a masked antenna's voltages are not read.
    """

    MAX_ANTS = 32768
    MAX_SAMPLES = 1 << 20

    def __init__(self, context, n_batches: int, n_channels_per_stream: int, n_samples_per_channel: int, n_ants: int,
                 integration: int = 16, sample_signed: bool = False, sum_pols: bool = False, scale: float = 1.0,
                 antenna_mask: bool = False) -> None:
        for name, v in dict(n_batches=n_batches, n_channels_per_stream=n_channels_per_stream,
                            n_samples_per_channel=n_samples_per_channel, n_ants=n_ants,
                            integration=integration).items():
            if int(v) <= 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if n_samples_per_channel % 16:
            raise ValueError("n_samples_per_channel must be a multiple of 16")
        if n_samples_per_channel > self.MAX_SAMPLES:
            raise ValueError(f"n_samples_per_channel must be at most {self.MAX_SAMPLES}")
        if n_ants > self.MAX_ANTS:
            raise ValueError(f"n_ants must be at most {self.MAX_ANTS}, got {n_ants}")
        tint = int(integration)
        if n_samples_per_channel % tint or not (tint % 16 == 0 or (tint < 16 and tint & (tint - 1) == 0)):
            raise ValueError(f"integration {tint} must divide n_samples_per_channel and be a power of two <= 16 or a "
                             "multiple of 16")
        if not (np.isfinite(np.float32(scale)) and np.float32(scale) > 0):
            raise ValueError("scale must be finite and > 0")
        self.context = context
        self.n_batches = n_batches
        self.n_pols = 1 if sum_pols else 2
        self.n_channels_per_stream = n_channels_per_stream
        self.n_samples_per_channel = n_samples_per_channel
        self.n_ants = n_ants
        self.integration = tint
        self.sample_signed = bool(sample_signed)
        self.sum_pols = bool(sum_pols)
        self.scale = float(np.float32(scale))
        self.antenna_mask = bool(antenna_mask)
        self.flags = (_lib.INCOH_SIGNED if self.sample_signed else 0) | (_lib.INCOH_SUM_POLS if self.sum_pols else 0)
        B, C, T, A = n_batches, n_channels_per_stream, n_samples_per_channel, n_ants
        self.input_shape = (B, A, C, T, 2, 2)
        self.output_shape = (B, self.n_pols, C, T // tint)
        self.mask_shape = (A,)

    def algorithmic_bytes(self):
        """HBM bytes one launch must move: voltages once, the mask once, the output once."""
        return _lib.load().bf_incoherent_algorithmic_bytes(self.n_batches, self.n_channels_per_stream,
                                                           self.n_samples_per_channel, self.n_ants, self.integration,
                                                           self.flags, int(self.antenna_mask))

    def instantiate(self, command_queue):
        return IncoherentBeam(self, command_queue)


class IncoherentBeam(accel.Operation):
    """.. rubric:: Slots
    inSamples: (n_batches, n_ants, n_channels_per_stream, n_samples_per_channel, 2, 2), uint8 (int8 if signed)
    outData: (n_batches, n_pols, n_channels_per_stream, n_samples_per_channel // integration), float32
    antennaMask: (n_ants,), uint8 -- with antenna_mask=True
    """

    def __init__(self, template: IncoherentBeamTemplate, command_queue):
        super().__init__(command_queue)
        self.template = t = template
        self.slots["inSamples"] = accel.IOSlot(t.input_shape, np.int8 if t.sample_signed else np.uint8)
        self.slots["outData"] = accel.IOSlot(t.output_shape, np.float32)
        self._mask = None
        if t.antenna_mask:
            self.slots["antennaMask"] = accel.IOSlot(t.mask_shape, np.uint8)
            self._mask = np.ones(t.mask_shape, np.uint8)
            self._mask_dirty = True

    def set_antenna_mask(self, mask):
        """Set which antennas count (non-zero = counted).  The length must equal n_ants.  Takes effect from the next
        launch (stream-ordered upload)."""
        if self._mask is None:
            raise ValueError("operator was built without antenna_mask=True")
        m = np.asarray(mask)
        if m.shape != self.template.mask_shape:
            raise ValueError(f"{m.size} mask entries received, expected {self.template.n_ants}")
        self._mask = (m != 0).astype(np.uint8)
        self._mask_dirty = True

    def antenna_mask(self):
        """The current (A,) mask (host copy)."""
        return None if self._mask is None else self._mask.copy()

    def _run(self):
        t = self.template
        mask = None
        if self._mask is not None:
            buf = self.buffer("antennaMask")
            if self._mask_dirty:
                buf.set_async(self.command_queue, self._mask)
                self._mask_dirty = False
            mask = buf.ptr
        _lib.call("bf_incoherent_beam", self.buffer("inSamples").ptr, mask, self.buffer("outData").ptr, t.n_batches,
                  t.n_channels_per_stream, t.n_samples_per_channel, t.n_ants, t.integration, t.flags, t.scale,
                  self.command_queue.handle)
