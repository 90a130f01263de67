"""The correlator: integer visibilities of the raw voltages (MI355X-native operator, no reference counterpart).

The other half of an X/B-engine: for every antenna pair, pol pair, channel and window of `integration` samples (and
`batch_integration` batches) the sum of x[a1, p1] * conj(x[a2, p2]) over the window, as exact int32 (re, im).  Delay
and phase models, per-antenna beam weights and dead-antenna decisions are solved from these.  `Correlator.inSamples`
has the shape and dtype of `FusedBeamformer.inSamples`, so one device buffer binds to both.

Contract (bf_correlate, include/bf.h): out is (B / bint, C, T / tint, NBL, 2, 2, 2) int32 with NBL = A (A + 1) / 2, the
baseline of (a1, a2), a1 >= a2, at a1 (a1 + 1) / 2 + a2 (autos included), the last axes (p1, p2, (re, im));
re = sum r1*r2 + i1*i2, im = sum i1*r2 - r1*i2 -- exact integers, deterministic and bit-exact.
"""
import numpy as np

from .. import _lib, accel


def n_baselines(n_ants):
    """Stored baselines of n_ants antennas, autos included."""
    return n_ants * (n_ants + 1) // 2


def baseline_index(a1, a2):
    """(index, conjugate) of the antenna pair in either order: the stored value is x[max] * conj(x[min]), so for
    a1 < a2 the visibility of (a1, a2) is the conjugate of the stored one with its pol axes swapped."""
    if a1 < 0 or a2 < 0:
        raise ValueError(f"antenna indices must be non-negative, got {(a1, a2)}")
    hi, lo = max(a1, a2), min(a1, a2)
    return hi * (hi + 1) // 2 + lo, a1 < a2


def visibility_matrix(vis):
    """(..., NBL, 2, 2, 2) integer visibilities -> the full Hermitian complex128 (..., A, 2, A, 2) with
    V[..., a1, p1, a2, p2] = sum x[a1, p1] * conj(x[a2, p2]).  Pure NumPy."""
    v = np.asarray(vis)
    if v.ndim < 4 or v.shape[-3:] != (2, 2, 2):
        raise ValueError(f"visibilities must have shape (..., NBL, 2, 2, 2), got {v.shape}")
    nbl = v.shape[-4]
    A = (int(np.sqrt(8 * nbl + 1)) - 1) // 2
    if n_baselines(A) != nbl:
        raise ValueError(f"{nbl} is not a number of baselines A (A + 1) / 2")
    z = v[..., 0].astype(np.float64) + 1j * v[..., 1].astype(np.float64)  # (..., NBL, p1, p2)
    a1, a2 = np.tril_indices(A)  # row-major lower triangle: index a1 (a1 + 1) / 2 + a2
    full = np.zeros(v.shape[:-4] + (A, A, 2, 2), np.complex128)  # (..., a1, a2, p1, p2)
    full[..., a2, a1, :, :] = np.conj(np.swapaxes(z, -1, -2))
    full[..., a1, a2, :, :] = z  # after the conjugates: an auto keeps its stored four pol products
    return np.ascontiguousarray(np.swapaxes(full, -3, -2))


class CorrelatorTemplate:
    """Template for the correlator.

    Parameters
    ----------
    context, n_batches, n_channels_per_stream, n_samples_per_channel, n_ants -- as FusedBeamformerTemplate
        (n_ants at most 2048).
    integration: samples per window; a multiple of 16 that divides n_samples_per_channel.  None: all of them.
    batch_integration: batches per window; divides n_batches, and above 1 needs integration == n_samples_per_channel.
    sample_signed: read voltages as int8 instead of uint8.
    accumulate: the Correlator adds successive calls into outVisibilities (see Correlator).
    The samples per window, integration * batch_integration, must keep every sum in int32: at most 65535 for int8
    samples, 16512 for uint8.
    """

    MAX_ANTS = 2048
    MAX_SAMPLES = 1 << 20
    MAX_WINDOW = {True: 65535, False: 16512}  # by sample_signed

    def __init__(self, context, n_batches: int, n_channels_per_stream: int, n_samples_per_channel: int, n_ants: int,
                 integration=None, batch_integration: int = 1, sample_signed: bool = False,
                 accumulate: bool = False) -> None:
        tint = n_samples_per_channel if integration is None else int(integration)
        bint = int(batch_integration)
        for name, v in dict(n_batches=n_batches, n_channels_per_stream=n_channels_per_stream,
                            n_samples_per_channel=n_samples_per_channel, n_ants=n_ants, integration=tint,
                            batch_integration=bint).items():
            if int(v) <= 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if n_samples_per_channel % 16:
            raise ValueError("n_samples_per_channel must be a multiple of 16")
        if n_samples_per_channel > self.MAX_SAMPLES:
            raise ValueError(f"n_samples_per_channel must be at most {self.MAX_SAMPLES}")
        if n_ants > self.MAX_ANTS:
            raise ValueError(f"n_ants must be at most {self.MAX_ANTS}, got {n_ants}")
        if tint % 16 or n_samples_per_channel % tint:
            raise ValueError(f"integration {tint} must be a multiple of 16 that divides n_samples_per_channel")
        if n_batches % bint:
            raise ValueError(f"batch_integration {bint} must divide n_batches")
        if bint > 1 and tint != n_samples_per_channel:
            raise ValueError("batch_integration above 1 needs integration == n_samples_per_channel")
        self.sample_signed = bool(sample_signed)
        self.window_bound = self.MAX_WINDOW[self.sample_signed]
        if tint * bint > self.window_bound:
            raise ValueError(f"{tint * bint} samples per window pass the int32 bound, {self.window_bound} for "
                             f"{'int8' if self.sample_signed else 'uint8'} samples")
        self.context = context
        self.n_batches = n_batches
        self.n_channels_per_stream = n_channels_per_stream
        self.n_samples_per_channel = n_samples_per_channel
        self.n_ants = n_ants
        self.integration = tint
        self.batch_integration = bint
        self.accumulate = bool(accumulate)
        self.flags = _lib.CORR_SIGNED if self.sample_signed else 0
        B, C, T, A = n_batches, n_channels_per_stream, n_samples_per_channel, n_ants
        self.input_shape = (B, A, C, T, 2, 2)
        self.output_shape = (B // bint, C, T // tint, n_baselines(A), 2, 2, 2)
        if self.algorithmic_bytes() == 0:  # what only the library judges: the grid limit
            raise ValueError("shape refused by bf_correlate: too many workgroups")

    def algorithmic_bytes(self, accumulating=False):
        """HBM bytes one launch must move: the voltages once, the visibilities once (read and written when the launch
        accumulates)."""
        flags = self.flags | (_lib.CORR_ACCUMULATE if accumulating else 0)
        return _lib.load().bf_correlate_algorithmic_bytes(self.n_batches, self.n_channels_per_stream,
                                                          self.n_samples_per_channel, self.n_ants, self.integration,
                                                          self.batch_integration, flags)

    def instantiate(self, command_queue):
        return Correlator(self, command_queue)


class Correlator(accel.Operation):
    """.. rubric:: Slots
    inSamples: (n_batches, n_ants, n_channels_per_stream, n_samples_per_channel, 2, 2), uint8 (int8 if signed)
    outVisibilities: (n_batches // batch_integration, n_channels_per_stream, n_samples_per_channel // integration,
        n_baselines, 2, 2, 2), int32

    With the template's accumulate=True the first call after reset() (or after creation) overwrites outVisibilities and
    every later call adds to it; `samples_accumulated` counts the samples per window summed so far, and a call that
    would take it past the int32 bound raises OverflowError before anything is launched.
    """

    def __init__(self, template: CorrelatorTemplate, command_queue):
        super().__init__(command_queue)
        self.template = t = template
        self.slots["inSamples"] = accel.IOSlot(t.input_shape, np.int8 if t.sample_signed else np.uint8)
        self.slots["outVisibilities"] = accel.IOSlot(t.output_shape, np.int32)
        self.samples_accumulated = 0

    def reset(self):
        """The next call overwrites outVisibilities."""
        self.samples_accumulated = 0

    def _next_flags(self):
        """The flags of the next launch; counts its samples."""
        t = self.template
        n = t.integration * t.batch_integration
        if not t.accumulate:
            self.samples_accumulated = n
            return t.flags
        if self.samples_accumulated + n > t.window_bound:
            raise OverflowError(f"{self.samples_accumulated} + {n} samples per window pass the int32 bound "
                                f"{t.window_bound}: reset() first")
        flags = t.flags | (_lib.CORR_ACCUMULATE if self.samples_accumulated else 0)
        self.samples_accumulated += n
        return flags

    def _run(self):
        t = self.template
        _lib.call("bf_correlate", self.buffer("inSamples").ptr, self.buffer("outVisibilities").ptr, t.n_batches,
                  t.n_channels_per_stream, t.n_samples_per_channel, t.n_ants, t.integration, t.batch_integration,
                  self._next_flags(), self.command_queue.handle)
