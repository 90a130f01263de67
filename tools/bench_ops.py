"""Per-operator timing on the GPU: the reference's three-pass chain (reorder, coefficient generator, table multiply,
OpSequence) next to the fused operator, at the SURVEY §8d configurations.  HIP-event averages on the launch
stream, random inputs, algorithmic bytes per launch and the achieved fraction of 8 TB/s.

    python tools/bench_ops.py [--reps 10] [--only cfg3,cfg4]     -> one JSON line per measurement
At cfg2, cfg3 and cfg4 the incoherent beam follows (integration = T and 16, unmasked), each line with the box's stream
ceiling for the same read and write bytes (build/libbf_stream.so, `make stream`) measured in the same process;
`--incoherent` runs only these.  The beam detector follows at the same configurations (f32 and int8 beams of the
configuration's shape, (tint, fint) = (16, 1) and (T, 16), Stokes I and IQUV), each line with the stream ceiling in the
same way; `--detect` runs only these.  `--vstats` runs the voltage statistics alone, at cfg3 and cfg4: integration 256
and 16, all three outputs and the power alone, each line with the stream ceiling for its own bytes, and the incoherent
beam on the same cube at the same integration, all in one process.  `--correlate` runs the correlator alone, at cfg3
(integration T over all 8 batches) and cfg4 (integration T), each line with the stream ceiling for its own bytes and the
useful int8 operation rate (NBL * 4 * 8 operations per channel-sample), then the incoherent beam on the same cube in
the same process; its lines also go to `--out` (profiles/correlate_ops.jsonl).  `--beam-streams` runs the beam streams
alone, at cfg2, cfg3 and cfg4: int8, f32 and f32 requantised beams of the configuration's shape, every beam and one beam
of M, medians of `--reps` launches, each line with the stream ceiling for its own bytes and bf_reorder on a voltage cube
of the same byte count, in the same process; its lines also go to `--out` (profiles/beam_streams_ops.jsonl).
`--dedisperse` runs the dedisperser alone, at cfg3 and cfg4: the detector-shaped power of the configuration at
(tint, fint) = (16, 1), dispersion_lags over 856-1712 MHz at the 76.6 us sample time, 64 and 256 trials 1 pc cm^-3
apart, medians of `--reps` launches; each line with the K*D*N*M additions per second, the stream ceiling for its own
bytes, the telescope time one call covers (B*T / 208984 s) and the naive one-thread-per-output kernel
(build/libbf_dedisperse_naive.so, `make dedisperse-naive`; step 2 only, no append) on the same ring in the same process;
its lines also go to `--out` (profiles/dedisperse_ops.jsonl).
`--pulse-search` runs the pulse search alone on the dedisperser's four lines (cfg3 and cfg4, 64 and 256 trials): a
series of the dedisperser's output shape (chi-squared noise of 4096 degrees of freedom, as a sum of K channel powers
is), the default widths 1 .. 128 and the default baseline, medians of `--reps` launches with head, slot and n_blocks
advancing as in use; each line with the stream ceiling for its own bytes, the telescope time one call covers and,
beside them, the dedisperser's time of the same line from `--dedisperse-profile` (profiles/dedisperse_ops.jsonl) and
whether the two together stay under the telescope time; its lines also go to `--out` (profiles/pulse_search_ops.jsonl).
`--fold` runs the folder alone on detector-shaped power at cfg3 and cfg4, one fold per beam, 1024 bins, Stokes I and
IQUV, a 4.57 ms and a 0.5 s pulsar at DM 40: each line with the algorithmic bytes for the counted touched accumulators,
the stream ceiling for those bytes in the same process, the telescope time one call covers and the naive
one-thread-per-row kernel (build/libbf_fold_naive.so, `make fold-naive`) on the same buffers; its lines also go to
`--out` (profiles/fold_ops.jsonl).
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from dpdk_dc_sand_amd import _lib, accel  # noqa: E402
from dpdk_dc_sand_amd.beamforming import (BeamDetectorTemplate, BeamStreamsTemplate, CoeffGeneratorTemplate,  # noqa: E402
                                          DedisperserTemplate, dispersion_lags, FolderTemplate, PulseSearchTemplate,
                                          FusedBeamformerTemplate, IncoherentBeamTemplate, MatrixMultiplyTemplate, OpSequenceTemplate,
                                          PreBeamformReorderTemplate, VoltageStatsTemplate, CorrelatorTemplate)

TS = 1 / 1712e6
HBM = 8.0e12
CONFIGS = {
    "cfg1": dict(A=4, M=1, C=64, Ctot=1024, T=1024, B=1),
    "cfg2": dict(A=64, M=1, C=4096, Ctot=4096, T=256, B=8),
    "cfg3": dict(A=64, M=16, C=4096, Ctot=4096, T=256, B=8),
    "cfg4": dict(A=256, M=64, C=4096, Ctot=32768, T=256, B=1),
}
INCOHERENT_CONFIGS = ("cfg2", "cfg3", "cfg4")
VSTATS_CONFIGS = ("cfg3", "cfg4")
CORRELATE_CONFIGS = {"cfg3": dict(bint=8), "cfg4": dict(bint=1)}  # integration = T
INT8_MFMA_PEAK = 5.0e15  # dense int8 MFMA operations per second: twice the 2.5 PFLOP/s dense BF16 rate


def timeit(queue, fn, reps, settle_s=0.2):
    # untimed clock settle first: the first ~30 ms of load run up to 35 % slower (profiles/r1_v6_clock_ramp.txt)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle_s:
        for _ in range(4):
            fn()
        queue.finish()
    e0, e1 = accel.Event(), accel.Event()
    e0.record(queue)
    for _ in range(reps):
        fn()
    e1.record(queue)
    queue.finish()
    return e1.time_since(e0) / reps


EMIT_FILE = None  # --correlate: an open file that receives every line as well


def emit(cfg, op, seconds, alg_bytes, **extra):
    line = {"config": cfg, "op": op, "us": round(seconds * 1e6, 2), "alg_bytes": int(alg_bytes),
            "achieved_GBps": round(alg_bytes / seconds / 1e9, 1), "frac_8TBps": round(alg_bytes / seconds / HBM, 4)}
    line.update(extra)
    print(json.dumps(line), flush=True)
    if EMIT_FILE is not None:
        EMIT_FILE.write(json.dumps(line) + "\n")
        EMIT_FILE.flush()


def delays(C, M, A, rng):
    d = np.zeros((C, M, A, 4), np.float32)
    d[..., 0] = rng.uniform(0, 10 * TS, d.shape[:-1])
    d[..., 2] = rng.uniform(-np.pi, np.pi, d.shape[:-1])
    return d


def run_config(ctx, q, name, c, reps, rng, fused_only=False, tag=""):
    A, M, C, Ctot, T, B = c["A"], c["M"], c["C"], c["Ctot"], c["T"], c["B"]
    samples = A * 2 * C * T * B
    vbytes = 2 * samples
    raw = rng.integers(0, 256, (B, A, C, T, 2, 2), dtype=np.uint8)

    if fused_only:
        return run_fused(ctx, q, name, c, reps, rng, raw, samples, tag)
    # the reference's three-pass chain, op by op and as the OpSequence
    seq = OpSequenceTemplate(ctx, B, 2, C, Ctot, T // 16, 16, A, M, 0, TS, T).instantiate(q)
    seq.ensure_all_bound()
    seq.beamform_coeff.buffer("delay_vals").set(q, delays(C, M, A, rng))
    seq.prebeamform_reorder.buffer("inSamples").set(q, raw)
    table = B * 2 * C * 2 * A * 2 * M * 4
    out_f32 = 8 * M * 2 * C * T * B
    emit(name, "reorder", timeit(q, seq.prebeamform_reorder, reps), 2 * vbytes)
    emit(name, "coeff_gen", timeit(q, seq.beamform_coeff, reps), table + C * M * A * 16)
    emit(name, "matrix_multiply", timeit(q, seq.beamform_mult, reps), vbytes + table + out_f32)
    t_seq = timeit(q, seq, reps)
    emit(name, "op_sequence", t_seq, 3 * vbytes + 2 * table + out_f32 + C * M * A * 16,
         gsamples_per_s=round(samples / t_seq / 1e9, 2))
    del seq
    run_fused(ctx, q, name, c, reps, rng, raw, samples, tag)


def run_fused(ctx, q, name, c, reps, rng, raw, samples, tag):
    A, M, C, Ctot, T, B = c["A"], c["M"], c["C"], c["Ctot"], c["T"], c["B"]
    d1 = delays(1, M, A, rng)
    for label, kw in (("fused_f32_fast", {}), ("fused_f32_exact", dict(exact_coeffs=True)),
                      ("fused_int8", dict(out_int8=True, out_scale=1 / 64))):
        tmpl = FusedBeamformerTemplate(ctx, B, C, Ctot, T, A, M, sample_period=TS, delay_channels=1, t0=0.0,
                                       batch_dt=T * 2 * Ctot * TS, **kw)
        op = tmpl.instantiate(q)
        op.ensure_all_bound()
        op.buffer("inSamples").set(q, raw)
        op.buffer("delay_vals").set(q, d1)
        t = timeit(q, op, reps)
        emit(name, label + tag, t, tmpl.algorithmic_bytes(), gsamples_per_s=round(samples / t / 1e9, 2))
        del op


def stream_ceiling(ctx, q, in_bytes, out_bytes, reps):
    """The box's best plain stream over `in_bytes` read and `out_bytes` written (bf_stream_ceiling of
    build/libbf_stream.so; the grids and codes bench.py tries), timed like the operators.  Every call's return value
    (the launch's hipError_t) is checked."""
    path = os.path.join(ROOT, "build", "libbf_stream.so")
    if not os.path.exists(path):
        raise OSError(f"{path} not found: build it with `make stream`")
    lib = ctypes.CDLL(path)
    V, S, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.bf_stream_ceiling.restype, lib.bf_stream_ceiling.argtypes = I, [V, V, S, S, I, I, V]
    src = accel.DeviceArray(ctx, (in_bytes,), np.uint8)
    dst = accel.DeviceArray(ctx, (max(out_bytes, 16),), np.uint8)
    src.zero(q)
    best = None
    for grid in (1024, 2048):
        for code in (1, 101, 102, 103) + ((200, 201) if out_bytes * 4 == in_bytes else ()):
            def fn():
                st = lib.bf_stream_ceiling(src.ptr, dst.ptr, in_bytes, out_bytes, grid, code, q.handle)
                if st != 0:
                    raise RuntimeError(f"bf_stream_ceiling grid {grid} code {code} failed: hipError_t {st}")
            t = timeit(q, fn, reps, settle_s=0.05)
            if best is None or t < best[0]:
                best = (t, grid, code)
    return best


def run_incoherent(ctx, q, name, c, reps, rng):
    """The incoherent beam over the configuration's voltage cube, unmasked, per pol: integration = T (one window per
    channel) and 16, each with the stream ceiling for its own read and write bytes."""
    A, C, T, B = c["A"], c["C"], c["T"], c["B"]
    raw = accel.DeviceArray(ctx, (B, A, C, T, 2, 2), np.uint8)
    raw.set(q, rng.integers(0, 256, raw.shape, dtype=np.uint8))
    for tint in (T, 16):
        tmpl = IncoherentBeamTemplate(ctx, B, C, T, A, integration=tint)
        op = tmpl.instantiate(q)
        op.bind(inSamples=raw)
        op.ensure_all_bound()
        t = timeit(q, op, reps)
        read_bytes, write_bytes = raw.nbytes, op.buffer("outData").nbytes
        assert tmpl.algorithmic_bytes() == read_bytes + write_bytes
        ct, grid, code = stream_ceiling(ctx, q, read_bytes, write_bytes, reps)
        emit(name, f"incoherent_tint{tint}", t, tmpl.algorithmic_bytes(), integration=tint, read_bytes=read_bytes,
             write_bytes=write_bytes, ceiling_us=round(ct * 1e6, 2),
             ceiling_GBps=round((read_bytes + write_bytes) / ct / 1e9, 1),
             ceiling_kernel=f"bf_stream_ceiling grid {grid} mode {code}", frac_of_ceiling=round(ct / t, 4))
        del op


def run_detect(ctx, q, name, c, reps, rng):
    """The beam detector over beams of the configuration's shape (random bytes read as int8, Gaussian f32 of rms
    1000): (tint, fint) = (16, 1) and (T, 16), Stokes I and IQUV, each with the stream ceiling for its own read and
    write bytes (measured once per distinct byte pair)."""
    M, C, T, B = c["M"], c["C"], c["T"], c["B"]
    shape = (B, 2, C, T // 16, 16, 2 * M)
    ceilings = {}
    for in_int8 in (False, True):
        beams = accel.DeviceArray(ctx, shape, np.int8 if in_int8 else np.float32)
        host = np.empty(shape, beams.dtype)
        flat = host.reshape(-1)
        for i in range(0, flat.size, 1 << 24):  # chunked: no whole-cube float64 temporary
            n = min(1 << 24, flat.size - i)
            flat[i:i + n] = (rng.integers(-128, 128, n, dtype=np.int8) if in_int8
                             else 1000 * rng.standard_normal(n, dtype=np.float32))
        beams.set(q, host)
        del host, flat
        for tint, fint in ((16, 1), (T, 16)):
            for stokes in ("I", "IQUV"):
                tmpl = BeamDetectorTemplate(ctx, B, C, T, M, time_integration=tint, channel_integration=fint,
                                            stokes=stokes, in_int8=in_int8)
                op = tmpl.instantiate(q)
                op.bind(inBeams=beams)
                op.ensure_all_bound()
                t = timeit(q, op, reps)
                read_bytes, write_bytes = beams.nbytes, op.buffer("outData").nbytes
                assert tmpl.algorithmic_bytes() == read_bytes + write_bytes
                if (read_bytes, write_bytes) not in ceilings:
                    ceilings[read_bytes, write_bytes] = stream_ceiling(ctx, q, read_bytes, write_bytes, reps)
                ct, grid, code = ceilings[read_bytes, write_bytes]
                emit(name, f"detect_{'int8' if in_int8 else 'f32'}_{stokes}_t{tint}_f{fint}", t,
                     tmpl.algorithmic_bytes(), time_integration=tint, channel_integration=fint, stokes=stokes,
                     beams="int8" if in_int8 else "f32", read_bytes=read_bytes, write_bytes=write_bytes,
                     ceiling_us=round(ct * 1e6, 2), ceiling_GBps=round((read_bytes + write_bytes) / ct / 1e9, 1),
                     ceiling_kernel=f"bf_stream_ceiling grid {grid} mode {code}", frac_of_ceiling=round(ct / t, 4))
                del op
        del beams


def run_vstats(ctx, q, name, c, reps, rng):
    """The voltage statistics over the configuration's voltage cube: integration 256 and 16, all three outputs and the
    power alone, each with the stream ceiling for its own read and write bytes; then the incoherent beam (unmasked, per
    pol) on the same cube at the same integration with its own ceiling, in the same process."""
    A, C, T, B = c["A"], c["C"], c["T"], c["B"]
    raw = accel.DeviceArray(ctx, (B, A, C, T, 2, 2), np.uint8)
    raw.set(q, rng.integers(0, 256, raw.shape, dtype=np.uint8))

    def measure(label, tmpl, out_names, tint, **extra):
        op = tmpl.instantiate(q)
        op.bind(inSamples=raw)
        op.ensure_all_bound()
        t = timeit(q, op, reps)
        read_bytes, write_bytes = raw.nbytes, sum(op.buffer(n).nbytes for n in out_names)
        assert tmpl.algorithmic_bytes() == read_bytes + write_bytes
        ct, grid, code = stream_ceiling(ctx, q, read_bytes, write_bytes, reps)
        emit(name, label, t, tmpl.algorithmic_bytes(), integration=tint, read_bytes=read_bytes,
             write_bytes=write_bytes, ceiling_us=round(ct * 1e6, 2),
             ceiling_GBps=round((read_bytes + write_bytes) / ct / 1e9, 1),
             ceiling_kernel=f"bf_stream_ceiling grid {grid} mode {code}", frac_of_ceiling=round(ct / t, 4), **extra)

    for tint in (256, 16):
        measure(f"vstats_all_tint{tint}", VoltageStatsTemplate(ctx, B, C, T, A, integration=tint,
                                                               sk_limits=(0.25, 0.55)),
                ("outPower", "outSK", "outFlags"), tint, outputs="power,sk,flags")
        measure(f"vstats_power_tint{tint}", VoltageStatsTemplate(ctx, B, C, T, A, integration=tint, sk=False),
                ("outPower",), tint, outputs="power")
        measure(f"incoherent_tint{tint}", IncoherentBeamTemplate(ctx, B, C, T, A, integration=tint), ("outData",), tint)


def run_correlate(ctx, q, name, c, reps, rng, bint):
    """The correlator over the configuration's voltage cube, uint8, integration T over `bint` batches, with the stream
    ceiling for its own read and write bytes and the useful int8 operation rate; then the incoherent beam (integration
    T, per pol) on the same cube with its own ceiling, in the same process."""
    A, C, T, B = c["A"], c["C"], c["T"], c["B"]
    raw = accel.DeviceArray(ctx, (B, A, C, T, 2, 2), np.uint8)
    raw.set(q, rng.integers(0, 256, raw.shape, dtype=np.uint8))

    def measure(label, tmpl, out_name, **extra):
        op = tmpl.instantiate(q)
        op.bind(inSamples=raw)
        op.ensure_all_bound()
        t = timeit(q, op, reps)
        read_bytes, write_bytes = raw.nbytes, op.buffer(out_name).nbytes
        assert tmpl.algorithmic_bytes() == read_bytes + write_bytes
        kernel = _lib.load().bf_last_kernel().decode()
        del op
        ct, grid, code = stream_ceiling(ctx, q, read_bytes, write_bytes, reps)
        emit(name, label, t, tmpl.algorithmic_bytes(), integration=T, read_bytes=read_bytes, write_bytes=write_bytes,
             kernel=kernel, ceiling_us=round(ct * 1e6, 2), ceiling_GBps=round((read_bytes + write_bytes) / ct / 1e9, 1),
             ceiling_kernel=f"bf_stream_ceiling grid {grid} mode {code}", frac_of_ceiling=round(ct / t, 4),
             **{k: (v(t) if callable(v) else v) for k, v in extra.items()})

    ops = (A * (A + 1) // 2) * 4 * 8 * B * C * T  # useful int8 operations: NBL * 4 * 8 per channel-sample
    measure(f"correlate_tint{T}_bint{bint}", CorrelatorTemplate(ctx, B, C, T, A, integration=T, batch_integration=bint),
            "outVisibilities", batch_integration=bint, n_baselines=A * (A + 1) // 2, useful_int8_ops=ops,
            useful_int8_Tops=lambda t: round(ops / t / 1e12, 2),
            frac_int8_mfma_peak=lambda t: round(ops / t / INT8_MFMA_PEAK, 4))
    measure(f"incoherent_tint{T}", IncoherentBeamTemplate(ctx, B, C, T, A, integration=T), "outData")


def median_time(queue, fn, reps, settle_s=0.2):
    """Per-launch HIP-event times of `reps` launches after the clock settle: (median, min, max) seconds."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle_s:
        for _ in range(4):
            fn()
        queue.finish()
    events = [(accel.Event(), accel.Event()) for _ in range(reps)]
    for e0, e1 in events:
        e0.record(queue)
        fn()
        e1.record(queue)
    queue.finish()
    times = sorted(e1.time_since(e0) for e0, e1 in events)
    return float(np.median(times)), times[0], times[-1]


def run_beam_streams(ctx, q, name, c, reps):
    """The beam streams over beams of the configuration's shape (device-made random bytes): int8, f32 and f32
    requantised, every beam (no list) and one beam of M (a list of one), medians of `reps` launches.  Each line carries
    the stream ceiling for its own read and write bytes, and the drop-in bf_reorder on a voltage cube of the same byte
    count as the beams (A = M for int8 beams, 4 M for f32: the project's other transpose, moving the same bytes as
    the every-beam copy), all in one process."""
    M, C, T, B = c["M"], c["C"], c["T"], c["B"]
    shape = (B, 2, C, T // 16, 16, 2 * M)
    for form, in_int8, requant in (("i8", True, False), ("f32", False, False), ("f32q", False, True)):
        beams = accel.DeviceArray(ctx, shape, np.int8 if in_int8 else np.float32)
        _lib.call("bf_fill_random", beams.ptr, beams.nbytes, 7, q.handle)
        reorder = None
        if not requant:  # bf_reorder on (B, A, C, T, 2, 2) of beams.nbytes, into a cube of the same size
            A = M if in_int8 else 4 * M
            assert B * A * C * T * 4 == beams.nbytes
            dst = accel.DeviceArray(ctx, (beams.nbytes,), np.uint8)

            def fn():
                _lib.call("bf_reorder", beams.ptr, dst.ptr, B, A, C, T, q.handle)
            reorder = median_time(q, fn, reps) + (A, _lib.load().bf_last_kernel().decode())
            del dst
        for label, index in (("all", None), ("one", [M // 2])):
            tmpl = BeamStreamsTemplate(ctx, B, C, T, M, in_int8=in_int8, requantise=requant, scale=1 / 64, beams=index)
            op = tmpl.instantiate(q)
            op.bind(inBeams=beams)
            op.ensure_all_bound()
            t, t_min, t_max = median_time(q, op, reps)
            kernel = _lib.load().bf_last_kernel().decode()
            read_bytes = beams.nbytes + (4 * len(index) if index else 0)
            write_bytes = op.buffer("outStreams").nbytes
            assert tmpl.algorithmic_bytes() == read_bytes + write_bytes
            del op
            ct, grid, code = stream_ceiling(ctx, q, read_bytes, write_bytes, reps)
            extra = {}
            if reorder is not None and index is None:
                extra = dict(reorder_us=round(reorder[0] * 1e6, 2), reorder_min_us=round(reorder[1] * 1e6, 2),
                             reorder_max_us=round(reorder[2] * 1e6, 2), reorder_ants=reorder[3],
                             reorder_kernel=reorder[4], time_over_reorder=round(t / reorder[0], 4))
            emit(name, f"beam_streams_{form}_{label}", t, tmpl.algorithmic_bytes(), form=form, beams=label,
                 n_streams=tmpl.n_streams, reps=reps, min_us=round(t_min * 1e6, 2), max_us=round(t_max * 1e6, 2),
                 read_bytes=read_bytes, write_bytes=write_bytes, kernel=kernel, ceiling_us=round(ct * 1e6, 2),
                 ceiling_GBps=round((read_bytes + write_bytes) / ct / 1e9, 1),
                 ceiling_kernel=f"bf_stream_ceiling grid {grid} mode {code}", frac_of_ceiling=round(ct / t, 4), **extra)
        del beams


DEDISPERSE_CONFIGS = ("cfg3", "cfg4")
SAMPLE_RATE = 208984.0  # channel samples per second: one call covers B * T / SAMPLE_RATE seconds


def run_dedisperse(ctx, q, name, c, reps):
    """The dedisperser over detector-shaped power of the configuration ((tint, fint) = (16, 1): K = C, J = T / 16), 64
    and 256 trials 1 pc cm^-3 apart over 856-1712 MHz at 76.6 us samples, constant power and ring (0.747, the byte 0x3f
    repeated).  Medians of `reps` launches; head advances from launch to launch as in use.  Each line carries the
    additions per second, the stream ceiling for the algorithmic bytes, the telescope time of one call and the naive
    kernel (step 2 only) on the same ring and lag table."""
    M, C, T, B = c["M"], c["C"], c["T"], c["B"]
    K, J = C, T // 16
    N = B * J
    path = os.path.join(ROOT, "build", "libbf_dedisperse_naive.so")
    if not os.path.exists(path):
        raise OSError(f"{path} not found: build it with `make dedisperse-naive`")
    naive = ctypes.CDLL(path)
    V, I = ctypes.c_void_p, ctypes.c_int
    naive.bf_dedisperse_naive.restype = I
    naive.bf_dedisperse_naive.argtypes = [V, V, V, I, I, I, I, I, I, ctypes.c_float, V]
    freqs = 856e6 + 856e6 * np.arange(K) / K
    power = accel.DeviceArray(ctx, (B, 1, K, J, M), np.float32)
    _lib.call("bf_memset", power.ptr, 0x3f, power.nbytes, q.handle)
    for D in (64, 256):
        lags, latency = dispersion_lags(np.arange(D, dtype=np.float64), freqs, 76.6e-6)
        tmpl = DedisperserTemplate(ctx, B, K, J, M, lags)
        op = tmpl.instantiate(q)
        op.bind(inPower=power)
        op.ensure_all_bound()
        op()  # allocates the ring and uploads the table
        _lib.call("bf_memset", op.ring.ptr, 0x3f, op.ring.nbytes, q.handle)
        t, t_min, t_max = median_time(q, op, reps)
        kernel = _lib.load().bf_last_kernel().decode()
        out = op.buffer("outData")

        def fn():
            st = naive.bf_dedisperse_naive(op.ring.ptr, op._lags.ptr, out.ptr, K, M, D, N, tmpl.ring_length, op.head,
                                           1.0, q.handle)
            if st != 0:
                raise RuntimeError(f"bf_dedisperse_naive failed: hipError_t {st}")
        tn, tn_min, tn_max = median_time(q, fn, reps)
        alg = tmpl.algorithmic_bytes()
        read_bytes = 4 * (K * N * M + (K * N + tmpl.span_sum) * M)
        write_bytes = 4 * (K * N * M + D * N * M)
        assert alg == read_bytes + write_bytes
        ring_bytes = op.ring.nbytes
        del op
        ct, grid, code = stream_ceiling(ctx, q, read_bytes, write_bytes, reps)
        adds = K * D * N * M
        telescope = B * T / SAMPLE_RATE
        emit(name, f"dedisperse_D{D}", t, alg, n_trials=D, n_channels=K, n_samples=N, n_beams=M, latency=latency,
             ring_length=tmpl.ring_length, ring_bytes=ring_bytes, span_sum=tmpl.span_sum, reps=reps,
             min_us=round(t_min * 1e6, 2), max_us=round(t_max * 1e6, 2), kernel=kernel, adds=adds,
             Gadds_per_s=round(adds / t / 1e9, 1), read_bytes=read_bytes, write_bytes=write_bytes,
             ceiling_us=round(ct * 1e6, 2), ceiling_GBps=round((read_bytes + write_bytes) / ct / 1e9, 1),
             ceiling_kernel=f"bf_stream_ceiling grid {grid} mode {code}", frac_of_ceiling=round(ct / t, 4),
             telescope_us=round(telescope * 1e6, 1), times_real_time=round(telescope / t, 1),
             naive_us=round(tn * 1e6, 2), naive_min_us=round(tn_min * 1e6, 2), naive_max_us=round(tn_max * 1e6, 2),
             naive_Gadds_per_s=round(adds / tn / 1e9, 1), naive_includes_append=False,
             naive_times_real_time=round(telescope / tn, 1), naive_over_tiled=round(tn / t, 3))
    del power


def run_pulse_search(ctx, q, name, c, reps, dedisperse_profile):
    """The pulse search over a series of the dedisperser's output shape at the configuration ((tint, fint) = (16, 1):
    N = B * T / 16 samples per call, M beams), 64 and 256 trials, the default widths and baseline, threshold 6.  The
    series is noise with the statistics of a sum of 4096 channel powers (mean 4096, variance 8192), so every S/N takes
    the whole arithmetic path.  Medians of `reps` launches; the state advances from launch to launch as in use (the
    first `baseline_blocks` launches, which fill the baseline, fall in the clock settle).  Each line carries the stream
    ceiling for the algorithmic bytes, the telescope time of one call and the dedisperser's time of the same line."""
    M, T, B = c["M"], c["T"], c["B"]
    N = B * (T // 16)
    dedisp = {}
    if os.path.exists(dedisperse_profile):
        for ln in open(dedisperse_profile):
            if ln.strip():
                d = json.loads(ln)
                dedisp[(d["config"], d["op"])] = d["us"]
    rng = np.random.default_rng(3)
    for D in (64, 256):
        tmpl = PulseSearchTemplate(ctx, M, D, N)
        op = tmpl.instantiate(q)
        op.ensure_all_bound()
        op.buffer("inSeries").set(q, (4096 + np.sqrt(8192) * rng.standard_normal(tmpl.input_shape)).astype(np.float32))
        t, t_min, t_max = median_time(q, op, reps)
        assert op.n_blocks == tmpl.baseline_blocks  # the baseline was full while the launches were timed
        kernel = _lib.load().bf_last_kernel().decode()
        above = int(op.buffer("outPeaks").get(q)[..., 3].sum())
        alg = int(tmpl.algorithmic_bytes())
        rows = M * D
        write_bytes = rows * (4 * N + 16 + 16) + 16 * M
        read_bytes = alg - write_bytes
        ring_bytes, moment_bytes = op.ring.nbytes, op.moments.nbytes
        del op
        ct, grid, code = stream_ceiling(ctx, q, read_bytes, write_bytes, reps)
        telescope = B * T / SAMPLE_RATE
        extra = {}
        d_us = dedisp.get((name, f"dedisperse_D{D}"))
        if d_us is not None:
            both = d_us + t * 1e6
            extra = dict(dedisperse_us=d_us, chain_us=round(both, 2),
                         chain_over_telescope=round(both / telescope / 1e6, 4),
                         chain_under_telescope=bool(both < telescope * 1e6))
        emit(name, f"pulse_search_D{D}", t, alg, n_trials=D, n_samples=N, n_beams=M, widths=tmpl.widths.tolist(),
             baseline_blocks=tmpl.baseline_blocks, ring_length=tmpl.ring_length, ring_bytes=ring_bytes,
             moment_bytes=moment_bytes, threshold=tmpl.threshold, samples_above_threshold=above, reps=reps,
             min_us=round(t_min * 1e6, 2), max_us=round(t_max * 1e6, 2), kernel=kernel, read_bytes=read_bytes,
             write_bytes=write_bytes, readback_bytes=16 * rows + 16 * M, ceiling_us=round(ct * 1e6, 2),
             ceiling_GBps=round((read_bytes + write_bytes) / ct / 1e9, 1),
             ceiling_kernel=f"bf_stream_ceiling grid {grid} mode {code}", frac_of_ceiling=round(ct / t, 4),
             telescope_us=round(telescope * 1e6, 1), times_real_time=round(telescope / t, 1), **extra)


def run_fold(ctx, q, name, c, reps):
    """The folder over detector-shaped power of the configuration ((tint, fint) = (16, 1): K = C, J = T / 16), one fold
    per beam (F = M), 1024 bins, 1 and 4 Stokes planes, a 4.57 ms and a 0.5 s pulsar at DM 40 over 856-1712 MHz at
    76.6 us samples, constant power (0.747, the byte 0x3f repeated).  Medians of `reps` launches; the phases advance from
    launch to launch as in use and the accumulators keep accumulating.  `touched`, the distinct (fold, channel, bin) of
    a call, is counted on the host for the first timed call (it barely depends on the starting phase).  Each line
    carries the stream ceiling for the algorithmic bytes, the telescope time of one call and the naive kernel on the
    same buffers."""
    M, C, T, B = c["M"], c["C"], c["T"], c["B"]
    K, J, F, nbin, ts = C, T // 16, M, 1024, 76.6e-6
    N = B * J
    path = os.path.join(ROOT, "build", "libbf_fold_naive.so")
    if not os.path.exists(path):
        raise OSError(f"{path} not found: build it with `make fold-naive`")
    naive = ctypes.CDLL(path)
    V, I = ctypes.c_void_p, ctypes.c_int
    naive.bf_fold_naive.restype = I
    naive.bf_fold_naive.argtypes = [V] * 7 + [I] * 7 + [V]
    freqs = 856e6 + 856e6 * np.arange(K) / K
    for S in (1, 4):
        power = accel.DeviceArray(ctx, (B, S, K, J, M), np.float32)
        _lib.call("bf_memset", power.ptr, 0x3f, power.nbytes, q.handle)
        for label, period in (("4.57ms", 4.57e-3), ("0.5s", 0.5)):
            tmpl = FolderTemplate(ctx, B, K, J, M, nbin, [(m, 1.0 / period, 40.0) for m in range(M)], freqs, ts,
                                  n_stokes=S)
            op = tmpl.instantiate(q)
            op.bind(inPower=power)
            op()  # allocates and zeroes the accumulators, uploads the channel phases
            q.finish()
            with np.errstate(over="ignore"):
                phase0 = np.array(op.phase, np.uint64)[:, None, None] - op.chan[:, :, None]
                phi = phase0 + np.arange(N, dtype=np.uint64) * np.array(op.phase_steps(), np.uint64)[:, None, None]
            bins = ((phi >> np.uint64(32)) * np.uint64(nbin)) >> np.uint64(32)
            touched = int((np.diff(np.sort(bins, axis=2), axis=2) != 0).sum()) + F * K
            del phi, bins
            t, t_min, t_max = median_time(q, op, reps)
            kernel = _lib.load().bf_last_kernel().decode()

            def fn():
                steps = op.phase_steps()
                for f in range(F):
                    op._phase0[f], op._dphase[f] = op.phase[f], steps[f]
                st = naive.bf_fold_naive(power.ptr, op._beam, op._phase0, op._dphase, op._chan.ptr, op.profile.ptr,
                                         op.hits.ptr, B, S, K, J, M, F, nbin, q.handle)
                if st != 0:
                    raise RuntimeError(f"bf_fold_naive failed: hipError_t {st}")
                op.phase = [(p + N * d) % (1 << 64) for p, d in zip(op.phase, steps)]
                op.samples_seen += N
            tn, tn_min, tn_max = median_time(q, fn, reps)
            alg = int(tmpl.algorithmic_bytes(touched))
            write_bytes = touched * (8 * S + 4)
            read_bytes = alg - write_bytes
            accumulator_bytes = op.profile.nbytes + op.hits.nbytes
            del op
            ct, grid, code = stream_ceiling(ctx, q, read_bytes, write_bytes, reps)
            telescope = B * T / SAMPLE_RATE
            emit(name, f"fold_S{S}_{label}", t, alg, n_stokes=S, period_s=period, dm=40.0, n_channels=K, n_samples=N,
                 n_beams=M, n_folds=F, n_bins=nbin, touched=touched, samples=F * K * N,
                 accumulator_bytes=accumulator_bytes, reps=reps, min_us=round(t_min * 1e6, 2),
                 max_us=round(t_max * 1e6, 2), kernel=kernel, read_bytes=read_bytes, write_bytes=write_bytes,
                 ceiling_us=round(ct * 1e6, 2), ceiling_GBps=round((read_bytes + write_bytes) / ct / 1e9, 1),
                 ceiling_kernel=f"bf_stream_ceiling grid {grid} mode {code}", frac_of_ceiling=round(ct / t, 4),
                 telescope_us=round(telescope * 1e6, 1), times_real_time=round(telescope / t, 1),
                 under_telescope=bool(t < telescope), naive_us=round(tn * 1e6, 2), naive_min_us=round(tn_min * 1e6, 2),
                 naive_max_us=round(tn_max * 1e6, 2), naive_times_real_time=round(telescope / tn, 1),
                 naive_over_product=round(tn / t, 3))
        del power


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--only", default=",".join(CONFIGS))
    p.add_argument("--fused-only", action="store_true")
    p.add_argument("--incoherent", action="store_true", help="only the incoherent beam and its stream ceiling")
    p.add_argument("--detect", action="store_true", help="only the beam detector and its stream ceiling")
    p.add_argument("--vstats", action="store_true", help="only the voltage statistics, their stream ceiling and the "
                   "incoherent beam on the same cube")
    p.add_argument("--correlate", action="store_true", help="only the correlator, its stream ceiling and the "
                   "incoherent beam on the same cube")
    p.add_argument("--beam-streams", action="store_true", help="only the beam streams, their stream ceiling and "
                   "bf_reorder on a cube of the same byte count")
    p.add_argument("--dedisperse", action="store_true", help="only the dedisperser, its stream ceiling and the naive "
                   "kernel on the same ring")
    p.add_argument("--pulse-search", action="store_true", help="only the pulse search, its stream ceiling and the "
                   "dedisperser's recorded time of the same line")
    p.add_argument("--fold", action="store_true", help="only the folder, its stream ceiling and the naive kernel on the "
                   "same buffers")
    p.add_argument("--dedisperse-profile", default=os.path.join(ROOT, "profiles", "dedisperse_ops.jsonl"),
                   help="--pulse-search: the dedisperser's lines (the output of --dedisperse)")
    p.add_argument("--out", default=None, help="--correlate, --beam-streams, --dedisperse, --pulse-search, --fold: the "
                   "file that receives the lines as well (profiles/correlate_ops.jsonl, profiles/beam_streams_ops.jsonl, "
                   "profiles/dedisperse_ops.jsonl, profiles/pulse_search_ops.jsonl, profiles/fold_ops.jsonl)")
    p.add_argument("--tag", default="", help="suffix for the op names (e.g. the env variant under test)")
    args = p.parse_args()
    ctx = accel.create_some_context()
    q = ctx.create_command_queue()
    rng = np.random.default_rng(0)
    if args.correlate or args.beam_streams or args.dedisperse or args.pulse_search or args.fold:
        global EMIT_FILE
        default = ("correlate_ops.jsonl" if args.correlate else
                   "beam_streams_ops.jsonl" if args.beam_streams else
                   "dedisperse_ops.jsonl" if args.dedisperse else
                   "pulse_search_ops.jsonl" if args.pulse_search else "fold_ops.jsonl")
        EMIT_FILE = open(args.out or os.path.join(ROOT, "profiles", default), "w")
    for name in args.only.split(","):
        if (args.incoherent or args.detect or args.vstats or args.correlate or args.beam_streams or args.dedisperse or
                args.pulse_search or args.fold):
            if name in DEDISPERSE_CONFIGS and args.fold:
                run_fold(ctx, q, name, CONFIGS[name], args.reps)
            if name in DEDISPERSE_CONFIGS and args.dedisperse:
                run_dedisperse(ctx, q, name, CONFIGS[name], args.reps)
            if name in DEDISPERSE_CONFIGS and args.pulse_search:
                run_pulse_search(ctx, q, name, CONFIGS[name], args.reps, args.dedisperse_profile)
            if name in INCOHERENT_CONFIGS and args.beam_streams:
                run_beam_streams(ctx, q, name, CONFIGS[name], args.reps)
            if name in CORRELATE_CONFIGS and args.correlate:
                run_correlate(ctx, q, name, CONFIGS[name], args.reps, rng, **CORRELATE_CONFIGS[name])
            if name in VSTATS_CONFIGS and args.vstats:
                run_vstats(ctx, q, name, CONFIGS[name], args.reps, rng)
            if name in INCOHERENT_CONFIGS and args.incoherent:
                run_incoherent(ctx, q, name, CONFIGS[name], args.reps, rng)
            if name in INCOHERENT_CONFIGS and args.detect:
                run_detect(ctx, q, name, CONFIGS[name], args.reps, rng)
            continue
        run_config(ctx, q, name, CONFIGS[name], args.reps, rng, args.fused_only, args.tag)
        if name in INCOHERENT_CONFIGS and not args.fused_only:
            run_incoherent(ctx, q, name, CONFIGS[name], args.reps, rng)
            run_detect(ctx, q, name, CONFIGS[name], args.reps, rng)


if __name__ == "__main__":
    main()
