"""Drop-in for the reference package `beamformer/beamforming` (magnate3/dpdk_dc_sand), on HIP/gfx950.

Reference module -> here:
    beamforming.prebeamform_reorder   -> PreBeamformReorderTemplate / PreBeamformReorder
    beamforming.coeff_generator       -> CoeffGeneratorTemplate / CoeffGenerator
    beamforming.matrix_multiply       -> MatrixMultiplyTemplate / MatrixMultiply
    beamforming.complex_mult_kernel   -> ComplexMultKernel
    beamforming.beamform_op_sequence  -> OpSequenceTemplate / OpSequence
New (MI355X-native): beamforming.fused -> FusedBeamformerTemplate / FusedBeamformer (one-pass reorder +
coefficient regeneration + multiply, optional ?beam-weights gains), beamforming.requant -> RequantTemplate /
Requant, beamforming.streaming -> StreamingBeamformerTemplate / StreamingBeamformer (host -> GPU -> host frames
with H2D, compute and D2H overlapped), beamforming.incoherent -> IncoherentBeamTemplate / IncoherentBeam (masked
antenna power sums of the same raw voltages, integrated in time; bit-exact integer contract), beamforming.detect ->
BeamDetectorTemplate / BeamDetector (Stokes I or IQUV power of the beams, integrated in time and frequency, bound to
FusedBeamformer.outData), beamforming.vstats -> VoltageStatsTemplate / VoltageStats (per-antenna power, spectral
kurtosis and RFI flags of the same raw voltages; antenna_mask_from_flags turns the flags into an antenna mask),
beamforming.correlate -> CorrelatorTemplate / Correlator (integer visibilities of every antenna pair of the same raw
voltages; n_baselines, baseline_index and visibility_matrix read the triangular output), beamforming.beam_streams ->
BeamStreamsTemplate / BeamStreams (the beams of FusedBeamformer.outData as per-beam voltage streams (B, K, C, T, 2, 2),
any subset; the int8 streams bind to VoltageStats, Correlator and IncoherentBeam as K antennas),
beamforming.dedisperse -> DedisperserTemplate / Dedisperser (DM-trial time series (M, D, N) of one Stokes plane of
BeamDetector.outData over a device ring of the recent past; dispersion_lags makes the lag table),
beamforming.pulse_search -> PulseSearchTemplate / PulseSearch (boxcar S/N of Dedisperser.outData against a running
baseline: one peak record per (beam, trial) and one best record per beam; candidates decodes the read-back peaks),
beamforming.fold -> FolderTemplate / Folder (pulsar profiles (fold, Stokes, channel, bin) of BeamDetector.outData for
known periods and dispersion measures, accumulated on the device in fixed-point phase; fold_phase_step and
fold_channel_phases make the phase step and the per-channel phase offsets, mean_profile divides by the hits).
The CPU reference helpers the reference tests import (beamforming/reorder.py, unit_test/*_cpu.py) live in the
repository's `oracle/` package, which the product path never imports.
"""
from .beam_streams import BeamStreams, BeamStreamsTemplate  # noqa: F401
from .beamform_op_sequence import OpSequence, OpSequenceTemplate  # noqa: F401
from .coeff_generator import CoeffGenerator, CoeffGeneratorTemplate  # noqa: F401
from .complex_mult_kernel import ComplexMultKernel  # noqa: F401
from .correlate import (Correlator, CorrelatorTemplate, baseline_index, n_baselines,  # noqa: F401
                        visibility_matrix)
from .dedisperse import Dedisperser, DedisperserTemplate, dispersion_lags  # noqa: F401
from .detect import BeamDetector, BeamDetectorTemplate  # noqa: F401
from .fold import (Folder, FolderTemplate, fold_channel_phases, fold_phase_step,  # noqa: F401
                   mean_profile)
from .fused import FusedBeamformer, FusedBeamformerTemplate  # noqa: F401
from .incoherent import IncoherentBeam, IncoherentBeamTemplate  # noqa: F401
from .matrix_multiply import MatrixMultiply, MatrixMultiplyTemplate  # noqa: F401
from .pulse_search import PulseSearch, PulseSearchTemplate, candidates  # noqa: F401
from .prebeamform_reorder import PreBeamformReorder, PreBeamformReorderTemplate  # noqa: F401
from .requant import Requant, RequantTemplate  # noqa: F401
from .streaming import StreamingBeamformer, StreamingBeamformerTemplate  # noqa: F401
from .vstats import VoltageStats, VoltageStatsTemplate, antenna_mask_from_flags  # noqa: F401
