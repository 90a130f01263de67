"""Voltage statistics: per-antenna power, spectral kurtosis and RFI flags of the raw voltages (MI355X-native operator,
no reference counterpart).

The operator that judges the voltages themselves: for every antenna, polarisation, channel and window of `integration`
samples it takes the first two moments S1, S2 of the sample power re^2 + im^2.  S1 is the level monitor; the ratio of
the moments is the spectral-kurtosis estimator (Nita & Gary 2010), 1 for Gaussian noise whatever its level, 0 for a
constant-amplitude carrier, far above 1 for pulsed interference, and undefined (stored as 0, always flagged) for a dead
input.  `VoltageStats.inSamples` has the shape and dtype of `FusedBeamformer.inSamples`, so one device buffer binds to
both; `antenna_mask_from_flags` turns the flags into the mask `IncoherentBeam.set_antenna_mask` takes.

Contract (bf_voltage_stats, include/bf.h): S1, S2 exact integers, power = float32(float64(S1) * float64(float32(
scale))), sk = float32(k * ((n * float64(S2)) / (float64(S1) * float64(S1)) - 1)) with k = (n + 1) / (n - 1), flag =
S1 == 0 or sk < lo or sk > hi on the stored float32 -- deterministic and bit-exact.
"""
import numpy as np

from .. import _lib, accel


class VoltageStatsTemplate:
    """Template for the voltage statistics.

    Parameters
    ----------
    context, n_batches, n_channels_per_stream, n_samples_per_channel, n_ants -- as FusedBeamformerTemplate.
    integration: samples per window; a multiple of 16 (the 16-sample block is the time granule) that divides
        n_samples_per_channel, at most 2^18 (the second moment stays exact in float64).
    sample_signed: read voltages as int8 instead of uint8.
    scale: finite and > 0; applied once, in float64, to the exact integer S1 (slot outPower).
    power, sk: which of the two float32 outputs to produce (slots outPower, outSK).
    sk_limits: (lo, hi) with 0 <= lo < hi, both finite, adds the flags output (slot outFlags): 1 where the window is
        dead (S1 == 0) or its float32 sk lies outside [lo, hi].
    At least one of the three outputs must be asked for.
    """

    MAX_ANTS = 32768
    MAX_SAMPLES = 1 << 20
    MAX_INTEGRATION = 1 << 18

    def __init__(self, context, n_batches: int, n_channels_per_stream: int, n_samples_per_channel: int, n_ants: int,
                 integration: int = 256, sample_signed: bool = False, scale: float = 1.0, power: bool = True,
                 sk: bool = True, sk_limits=None) -> None:
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
        if tint % 16 or n_samples_per_channel % tint or tint > self.MAX_INTEGRATION:
            raise ValueError(f"integration {tint} must be a multiple of 16 that divides n_samples_per_channel, at most "
                             f"{self.MAX_INTEGRATION}")
        if not (np.isfinite(np.float32(scale)) and np.float32(scale) > 0):
            raise ValueError("scale must be finite and > 0")
        if sk_limits is not None:
            lo, hi = (float(np.float32(v)) for v in sk_limits)
            if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo < hi):
                raise ValueError(f"sk_limits must be finite with 0 <= lo < hi, got {tuple(sk_limits)}")
            sk_limits = (lo, hi)
        if not (power or sk or sk_limits is not None):
            raise ValueError("no output: set power, sk or sk_limits")
        self.context = context
        self.n_batches = n_batches
        self.n_channels_per_stream = n_channels_per_stream
        self.n_samples_per_channel = n_samples_per_channel
        self.n_ants = n_ants
        self.integration = tint
        self.sample_signed = bool(sample_signed)
        self.scale = float(np.float32(scale))
        self.power = bool(power)
        self.sk = bool(sk)
        self.sk_limits = sk_limits
        self.flags = _lib.VSTATS_SIGNED if self.sample_signed else 0
        self.outputs = ((_lib.VSTATS_POWER if self.power else 0) | (_lib.VSTATS_SK if self.sk else 0) |
                        (_lib.VSTATS_FLAGS if sk_limits is not None else 0))
        B, C, T, A = n_batches, n_channels_per_stream, n_samples_per_channel, n_ants
        self.input_shape = (B, A, C, T, 2, 2)
        self.output_shape = (B, A, 2, C, T // tint)

    def algorithmic_bytes(self):
        """HBM bytes one launch must move: the voltages once, each requested output once."""
        return _lib.load().bf_vstats_algorithmic_bytes(self.n_batches, self.n_channels_per_stream,
                                                       self.n_samples_per_channel, self.n_ants, self.integration,
                                                       self.outputs)

    def instantiate(self, command_queue):
        return VoltageStats(self, command_queue)


class VoltageStats(accel.Operation):
    """.. rubric:: Slots
    inSamples: (n_batches, n_ants, n_channels_per_stream, n_samples_per_channel, 2, 2), uint8 (int8 if signed)
    outPower: (n_batches, n_ants, 2, n_channels_per_stream, n_samples_per_channel // integration), float32 -- with power
    outSK: the same shape, float32 -- with sk
    outFlags: the same shape, uint8 -- with sk_limits
    """

    def __init__(self, template: VoltageStatsTemplate, command_queue):
        super().__init__(command_queue)
        self.template = t = template
        self.slots["inSamples"] = accel.IOSlot(t.input_shape, np.int8 if t.sample_signed else np.uint8)
        if t.power:
            self.slots["outPower"] = accel.IOSlot(t.output_shape, np.float32)
        if t.sk:
            self.slots["outSK"] = accel.IOSlot(t.output_shape, np.float32)
        if t.sk_limits is not None:
            self.slots["outFlags"] = accel.IOSlot(t.output_shape, np.uint8)

    def _run(self):
        t = self.template
        lo, hi = t.sk_limits if t.sk_limits is not None else (0.0, 0.0)
        _lib.call("bf_voltage_stats", self.buffer("inSamples").ptr,
                  self.buffer("outPower").ptr if t.power else None, self.buffer("outSK").ptr if t.sk else None,
                  self.buffer("outFlags").ptr if t.sk_limits is not None else None, t.n_batches,
                  t.n_channels_per_stream, t.n_samples_per_channel, t.n_ants, t.integration, t.flags, t.scale, lo, hi,
                  self.command_queue.handle)


def antenna_mask_from_flags(flags, max_fraction):
    """(A,) uint8 mask from an outFlags cube (B, A, 2, C, J): 1 where the fraction of flagged windows of that antenna,
    over batch, pol, channel and window, is at most `max_fraction`.  Pure NumPy; the result is what
    IncoherentBeam.set_antenna_mask takes."""
    f = np.asarray(flags)
    if f.ndim != 5 or f.shape[2] != 2:
        raise ValueError(f"flags must have shape (B, A, 2, C, J), got {f.shape}")
    if not 0 <= max_fraction <= 1:
        raise ValueError(f"max_fraction must lie in [0, 1], got {max_fraction}")
    fraction = (f != 0).mean(axis=(0, 2, 3, 4))
    return (fraction <= max_fraction).astype(np.uint8)
