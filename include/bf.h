/*
 * bf.h -- C ABI of libbf.so, the MI355X-native (gfx950) beamformer hot path.
 *
 * Drop-in boundary for the reference's operator package `beamformer/beamforming` (magnate3/dpdk_dc_sand).
 * Every entry point below states the reference interface it replaces (file:line, relative to the reference
 * repository root).  Conventions:
 *   - every function returns int: 0 = OK, negative = error; bf_last_error() gives a thread-local message;
 *   - compute entry points take caller-owned DEVICE pointers plus a stream (hipStream_t passed as void*,
 *     NULL = the default stream), never allocate, are asynchronous and stream-ordered, and are reentrant
 *     across streams;
 *   - shapes are the reference's (B = batches, P = pols = 2, C = channels on this engine, Ctot = channels
 *     in the band, A = antennas, M = beams, T = samples per channel, NB = T / 16);
 *   - 8-bit voltages are complex (re, im) byte pairs; sample_signed = 0 reads them as uint8 (the reference
 *     slots' dtype, matrix_multiply.py:145-147), 1 as int8 (the C++ study's char2, BeamformerKernels.cu:196).
 */
#ifndef DPDK_DC_SAND_AMD_BF_H
#define DPDK_DC_SAND_AMD_BF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ------------------------------------------------------------------------------------------- */
#define BF_OK 0
#define BF_ERR_ARG (-1)     /* invalid shape / argument (reference: template ValueError, prebeamform_reorder.py:62-65) */
#define BF_ERR_HIP (-2)     /* HIP runtime error (reference: GPU_ERRCHK, common/Utils.hpp:8, common/Utils.cpp:8-16) */
#define BF_ERR_NODEV (-3)   /* no GPU visible */
#define BF_ERR_COMM (-4)    /* RCCL unavailable or a collective failed (multi-GPU channel scatter) */

/* Thread-local message of the last failing call on this thread (replaces GPU_ERRCHK's stderr print). */
const char* bf_last_error(void);
/* ABI version: major * 100 + minor.  300: ABI 3.0 -- 0x0500 (BF_FUSED_PATH_WIDE16, accepted by 2.0) is rejected as an
 * unknown path, and bf_coeff_gen_time_study, bf_comm_stats, bf_comm_load and bf_checksum were added.  301: ABI 3.1 --
 * bf_scatter_plan added (the channel scatter's operation list as a pure host function).  302: ABI 3.2 --
 * bf_beamform_study_single_channel added (the C++ study's fused kernel in its own semantics).  Later 3.2 libraries add
 * entry points without a new number; bf_has_feature (itself one of them: look it up with dlsym) tells a caller whether
 * the 3.2 library it loaded has them: "incoherent_beam" = bf_incoherent_beam and bf_incoherent_algorithmic_bytes,
 * "beam_detect" = bf_beam_detect and bf_detect_algorithmic_bytes, "voltage_stats" = bf_voltage_stats and
 * bf_vstats_algorithmic_bytes, "last_kernel" = bf_last_kernel, "fused_plan" = bf_fused_plan, "correlate" =
 * bf_correlate and bf_correlate_algorithmic_bytes, "check_gains" = bf_check_gains, "beam_streams" = bf_beam_streams and
 * bf_beam_streams_algorithmic_bytes, "dedisperse" = bf_dedisperse and bf_dedisperse_algorithmic_bytes, "pulse_search" =
 * bf_pulse_search and bf_pulse_search_algorithmic_bytes, "fold" = bf_fold and bf_fold_algorithmic_bytes. */
int bf_abi_version(void);
/* 1 when this library has the named feature ("incoherent_beam", "beam_detect", "voltage_stats", "last_kernel",
 * "fused_plan", "correlate", "check_gains", "beam_streams", "dedisperse", "pulse_search", "fold"), 0 for any other name
 * (and for NULL). */
int bf_has_feature(const char* name);
/* Thread-local name of the kernel that the last successful compute entry point on this thread launched, "" before any
 * launch; a failing call leaves it unchanged.  Where the library picks among several forms of a kernel at run time the
 * name carries the choice after a colon ("beamform_fused_i8_item_kernel:nts2,full,a64,pow2",
 * "beamform_table_ring_kernel:nts4,r16,w16"): tests and measurements use it to know which device code a call ran.  An
 * entry point that launches two kernels (bf_beamform_fused_ws with a workspace: the table generator, then the
 * contraction) reports the last.  The spelling of names and tags is not part of the ABI. */
const char* bf_last_kernel(void);

/* Pointer alignment.  Every compute entry point checks the alignment of its device pointers before it launches and
 * returns BF_ERR_ARG ("misaligned" / "aligned" in bf_last_error) otherwise; hipMalloc'd buffers satisfy all of them.
 * Bytes:
 *   bf_coeff_gen                      delay_vals 16, out 8 (16 selects the faster block form)
 *   bf_coeff_gen_time                 delay_vals 16, out 8 (float2) or 4 (half2, out_fp16)
 *   bf_coeff_gen_time_study           delay_vals 16, out 8 (float2) or 4 (half2, out_fp16)
 *   bf_beamform_study_single_channel  delay_vals 16, x 4, out 8
 *   bf_reorder                        in 16, out 16
 *   bf_beamform                       x 8, w 4, y 16 (x and w at 16 select the faster forms)
 *   bf_beamform_fused*                raw 16, delay_vals 16, y 16, gains 4 (or NULL), workspace 16 (or NULL)
 *   bf_q14_coeffs                     delay_vals 16, gains 4 (or NULL), out 4
 *   bf_requant                        y 16, q 4
 *   bf_incoherent_beam                raw 16, ant_mask 1 (none), out 4
 *   bf_beam_detect                    beams 16, out 4
 *   bf_voltage_stats                  raw 16, out_power 4, out_sk 4, out_flags 1 (none)
 *   bf_correlate                      raw 16, out 4
 *   bf_beam_streams                   beams 16, beam_index 4 (or NULL), out 16
 *   bf_dedisperse                     power 16, ring 16, lags 4, out 16
 *   bf_pulse_search                   series 16, ring 16, moments 16, snr 16 and width_index 4 (or both NULL), peaks 16,
 *                                     best 16; widths is host memory (none)
 *   bf_fold                           power 16, chan 8, profile 8, hits 4; beam, phase0 and dphase are host memory (none)
 *   bf_fill_random                    dst 16 */

/* ---- runtime helpers (device memory, streams, events) -------------------------------------------------
 * The reference gets these from katsdpsigproc.accel / PyCUDA (accel.create_some_context,
 * ctx.create_command_queue, DeviceArray.set/get: beamform_op_sequence_test.py:105-163) and, in the C++
 * harness, from the CUDA runtime (common/UnitTest.cpp:28-111).  Thin HIP wrappers so the Python shim needs
 * no other GPU runtime. */
int bf_device_count(int* count);
int bf_set_device(int device);
int bf_get_device(int* device);
int bf_device_name(int device, char* buf, size_t len);
int bf_malloc(void** ptr, size_t bytes);
int bf_free(void* ptr);
int bf_host_alloc(void** ptr, size_t bytes);   /* pinned host memory (streaming ring, cudaPcieRateTest.cpp:63-123) */
int bf_host_free(void* ptr);
int bf_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int bf_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int bf_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int bf_memset(void* dst, int value, size_t bytes, void* stream);
int bf_stream_create(void** stream);
int bf_stream_destroy(void* stream);
int bf_stream_synchronize(void* stream);
int bf_stream_wait_event(void* stream, void* event);
int bf_device_synchronize(void);
int bf_event_create(void** event);
int bf_event_destroy(void* event);
int bf_event_record(void* event, void* stream);
int bf_event_synchronize(void* event);
int bf_event_elapsed_ms(float* ms, void* start, void* stop);
/* Launch one empty kernel (`bf_trace_mark_kernel`) on `stream`: its dispatches delimit a region of a profiler's
 * kernel trace (bench.py brackets its timed steps with two of them; tools/kernel_stats.py reads the region). */
int bf_trace_mark(int tag, void* stream);

/* ---- hot path ----------------------------------------------------------------------------------------- */

/* Steering coefficients, Python layout.
 * Replaces CoeffGenerator._run -> run_coeff_gen (beamformer/beamforming/coeff_generator.py:12-103, 209-250),
 * with the CPU oracle's (c, m, a) mapping (beamformer/unit_test/coeff_generator_cpu.py:120-186).
 *   delay_vals : f32 (C, M, A, 4) = (delay_s, delay_rate, phase_rad, phase_rate); only [0] and [2] are read
 *   out        : f32 (B, P, C, 2A, 2M), block [[cos, sin], [-sin, cos]] per (a, m), replicated over (b, p)
 * The phase is evaluated in float64 in the reference's operation order, so the output is bit-exact to the
 * oracle.  `out` must be 8-byte aligned (a 16-byte aligned table takes the faster 16-byte-store block form). */
int bf_coeff_gen(const float* delay_vals, float* out, int B, int P, int C, int Ctot, int A, int M,
                 int xeng_id, double sample_period, void* stream);

/* Time-dependent compact coefficients (C++ study's steering kernels, BeamformerKernels.cu:7-189, with the
 * Python sign convention):
 *   rot(t, c, m, a) = (phi + phi_rate*dt) - pi*(tau + tau_rate*dt)*(ch - Ctot/2)/(Ctot*Ts),
 *   dt = t0 + t*dt_step for t in [0, n_times)
 *   delay_vals : f32 (Cd, M, A, 4) with Cd = C (per channel) or 1 (one model for every channel)
 *   out        : (n_times, C, A, M) complex: out_fp16 = 0 -> float2 (re, im); 1 -> half2 (b16BitOutput,
 *                BeamformerKernels.cu:111-116) */
int bf_coeff_gen_time(const float* delay_vals, int delay_channels, void* out, int out_fp16, int n_times,
                      int C, int Ctot, int A, int M, int xeng_id, double sample_period, double t0,
                      double dt_step, void* stream);

/* Time-dependent coefficients in the C++ study's OWN convention (replaces
 * calculate_beamweights_grouped_channels_and_timestamps, BeamformerKernels.cu:121-189, formula :155-170):
 *   dt = t*Ts*fft_size, dd = delay_rate*dt,
 *   rot = (delay_rate + dd)*c*pi/(Ts*C) + phase - (delay + dd)*(C/2)*pi/(Ts*C) + phase_rate*dt   (float32),
 * i.e. the delay rate in the channel term and the sign opposite to the Python path -- kept so that a
 * caller of the study's kernel gets its numbers; pinned by the study's own golden (BeamformerCoefficientTest.cu:
 * 294-337, tolerance 1e-4) restated in oracle/.
 *   delay_vals : f32 (A*M, 4), index a*M + m (the study's antenna-major struct delay_vals array)
 *   out        : (n_times, C, A, M) complex: out_fp16 = 0 -> float2 (cos, sin); 1 -> half2 */
int bf_coeff_gen_time_study(const float* delay_vals, void* out, int out_fp16, int n_times, int C, int A, int M,
                            float sample_period, int fft_size, void* stream);

/* The C++ study's fused coefficient + beamform kernel in the study's OWN semantics (replaces
 * calculate_beamweights_and_beamform_single_channel, BeamformerKernels.cu:192-367, as its harness's golden checks it,
 * BeamformerCoefficientTest.cu:356-400): per channel c, time t and beam m
 *   y_re = sum_a cos(rot) x_re,  y_im = sum_a sin(rot) x_im    (NOT a complex product: the study's semantics)
 * with rot bf_coeff_gen_time_study's expression at (t, c, a, m), antennas summed in order in float32.  The kernel's
 * shadowed prefetch (:277-282: every chunk after the first re-uses the first chunk's voltages) is not reproduced.
 *   delay_vals : f32 (M*A, 4), index m*A + a (the combined kernel's beam-major order)
 *   x          : int8 [C][T/16][A][16][2]  (char2 [channels][time/16][station][16]);  T % 16 == 0, A <= 2048
 *   out        : f32  [C][T/16][M][16][2] */
int bf_beamform_study_single_channel(const float* delay_vals, const int8_t* x, float* out, int C, int T, int A, int M,
                                     float sample_period, int fft_size, void* stream);

/* Pre-beamform reorder, bit-exact.
 * Replaces PreBeamformReorder._run / prebeamform_reorder kernel (beamformer/beamforming/prebeamform_reorder.py:
 * 171-186, kernels/prebeamform_reorder_kernel.mako:37-93):
 *   in  : u8 (B, A, C, T, 2, 2)   out : u8 (B, 2, C, T/16, 16, A, 2).   T % 16 == 0. */
int bf_reorder(const uint8_t* in, uint8_t* out, int B, int A, int C, int T, void* stream);

/* Beamform complex multiply (MFMA batched GEMM, f16 hi/lo coefficient split, f32 accumulation).
 * Replaces MatrixMultiply._run -> ComplexMultKernel.complex_mult -> run_complex_mult
 * (beamformer/beamforming/matrix_multiply.py:155-163, complex_mult_kernel.py:11-100, 106-162):
 *   x : 8-bit (B, P, C, NB, 16, A, 2)   w : f32 (B, P, C, 2A, 2M)   y : f32 (B, P, C, NB, 16, 2M)
 *   y[..., col] = sum_k x[..., k] * w[k, col] with x[2a] = re, x[2a+1] = im.
 * Float coefficient domain and floor (this entry point's table, and the float beams of bf_beamform_fused* -- float
 * output and BF_FUSED_INT8_VIA_F32 -- whose coefficients are g * (cos, sin)): every coefficient enters the MFMA as
 * hi = f16(w), lo = f16(w - hi).  The domain is |w| <= 65504: from 65520 on f16(w) is infinite and the beams are inf or
 * NaN (this call, which reads its table on the device, does not check; bf_check_gains and the Python wrapper do for
 * weights).  The pair carries w with an error of at most 2^-22 |w| + 2^-25, the second term an absolute floor from
 * f16's subnormal spacing: weights near 1 are f32-class (about 5e-9 of sum |x w| over 256 antennas), but weights far
 * below 1 lose accuracy relative to their own size -- 1e-6 at 2^-8 (a table normalised by 1 / 256 antennas), 1.6e-5
 * at 2^-12, 2e-4 at 2^-16, 4e-3 at 2^-20.  Normalise weights and tables to a maximum of about 1 and fold the common
 * factor into out_scale or a later stage. */
int bf_beamform(const uint8_t* x, const float* w, float* y, int B, int P, int C, int NB, int A, int M,
                int sample_signed, void* stream);

/* Fused pre-beamform reorder + per-batch coefficient regeneration + beamform (one pass over the voltages).
 * Replaces the OpSequence chain (beamformer/beamforming/beamform_op_sequence.py:117-157: reorder ->
 * coeff gen -> multiply) and the C++ fused study kernel calculate_beamweights_and_beamform_single_channel
 * (beamformer_coefficient_generator/BeamformerKernels.cu:192-367, correct complex multiply):
 *   raw        : 8-bit (B, A, C, T, 2, 2), the reorder's input layout, read directly
 *   delay_vals : f32 (Cd, M, A, 4), Cd = C or 1; batch b uses dt_b = t0 + b*batch_dt (regeneration per
 *                block of T samples, BeamformerParameters.h:17); with zero rates/dt it equals OpSequence
 *   y          : f32 (B, 2, C, T/16, 16, 2M), or int8 = sat127(rne(y * out_scale)) with BF_FUSED_OUT_INT8
 *   flags      : BF_FUSED_SIGNED (int8 samples), BF_FUSED_OUT_INT8, BF_FUSED_EXACT_COEFF (float64 phasors
 *                bit-exact to bf_coeff_gen; default is the ~1-ulp float32 fast phasor).
 * int8 beams have two contracts:
 *   default               : the Q14 integer contract (oracle fused_beamform_int8): W = rne(2^14 * f32 phasor), exact
 *                           int32 sums, q = sat127(rne(f32(y) * out_scale * 2^-14)); integer MFMA, bit-exact;
 *   BF_FUSED_INT8_VIA_F32 : q = sat127(rne(y_f32 * out_scale)) of the float32 beams (the reference's float32
 *                           coefficient arithmetic, requantised in-kernel == bf_requant of the float output).
 * The steering argument's domain.  With tau' = tau + tau_rate*dt_b and phi' = phi + phi_rate*dt_b (float64) the phase
 * of channel ch is rot = phi' + tau' * (ch - Ctot/2) * K, K = -pi / (Ctot * sample_period); Ctot may be odd, and the
 * call's channels may lie anywhere in the band, the centre channel (where the delay term vanishes) included.
 *   int8 beams (Q14 contract): the bits are the contract's for every finite model.  A coefficient is evaluated by the
 *     fast phasor while mag = |f32(tau')| * f32((ch + Ctot/2) * |K|) + |f32(phi')| < 2e5 -- at the top of the band that
 *     is |tau'| < 4.2e4 samples less |phi'| / 4.7, at its bottom 1.3e5 samples, and |phi'| < 2e5 rad (a model 2.8 hours
 *     old at a fringe rate of 20 rad/s) -- and otherwise, or where the fast value lies within 5e-10 of a rounding
 *     decision, exactly (float64 in the reference's operation order): the same bits, slower (a wave runs as many exact
 *     passes as its most-flagged lane needs).  An 8 km array at L-band (+-4.6e4 samples) keeps most of the band
 *     on the fast phasor; beyond mag = 2e5 every coefficient is exact.
 *   float beams, BF_FUSED_EXACT_COEFF: bit-exact to bf_coeff_gen / bf_coeff_gen_time at any finite argument.
 *   float beams, fast phasor (default): rot is reduced to revolutions in float64 and rounded once to float32, so the
 *     phasor's error is <= 2^-22 (argument rounding 2^-26 rev plus the hardware sin / cos) + 4 * 2^-53 * |rot|: flat
 *     in |rot| up to about 1e8 rad (measured flat from |rot| < 1e2 to 5e6, tests/test_gpu_phase_domain.py), far beyond
 *     any delay a telescope tracks.
 *   A model with a NaN or an infinity in any field has no contract: no output is defined for it (the int8 path's
 *     range check sends it to the exact path, which returns whatever float64 arithmetic gives).
 * Kernel-path and workgroup-order overrides (BF_FUSED_PATH_*, BF_FUSED_ORDER_*) exist for tests and measurement:
 * every path computes the same contract, a path that does not fit the shape falls through to one that does, and
 * 0 (automatic) picks the fastest path for the shape.  The library never reads the environment. */
#define BF_FUSED_SIGNED 1
#define BF_FUSED_OUT_INT8 2
#define BF_FUSED_EXACT_COEFF 4
#define BF_FUSED_INT8_VIA_F32 8
#define BF_FUSED_PATH_MASK 0x0f00
#define BF_FUSED_PATH_ITEM 0x0100    /* one workgroup per (batch, channel) item (A <= 64, T <= 256), else generic */
#define BF_FUSED_PATH_GENERIC 0x0300 /* any A, any T: groups of 64 antennas */
#define BF_FUSED_PATH_WIDE 0x0400    /* many antennas x beams: multi-wave beam slabs (config 4) */
/* (0x0200 and 0x0600 named two measured-slower kernels of ABI 1.x, and 0x0500 (WIDE16) the 16-beam int8 wide kernel
 * of ABI 2.0, removed from the product in ABI 3.0 (0x0500: the 16-beam float slabs are what WIDE picks for M <= 16; the
 * int8 kernel is gone with the diagnostic build): all three are rejected as unknown.) */
#define BF_FUSED_ORDER_MASK 0x3000
#define BF_FUSED_ORDER_CHANNEL 0x1000 /* plain channel-fastest workgroup order (the persistent config-4 float
                                         kernel walks channel runs and has none: this flag takes the slab kernel) */
#define BF_FUSED_ORDER_XCD 0x2000     /* XCD-range order (XCD x streams channels [x C/8, (x+1) C/8)) */
int bf_beamform_fused(const uint8_t* raw, const float* delay_vals, int delay_channels, void* y, int B, int C,
                      int T, int A, int M, int Ctot, int xeng_id, double sample_period, double t0,
                      double batch_dt, int flags, float out_scale, void* stream);

/* bf_beamform_fused with per-input beam weights folded into the phasors (control-plane hook: the
 * `?beam-weights <beam> w_0 .. w_{A-1}` request, ngkcs/ngkcs/corr3_servlet.py:140-153, forwarded to the
 * B-engines).  gains: f32 (M, A) real weight of antenna a in beam m on the device, or NULL (= all ones, exactly
 * bf_beamform_fused).  Coefficient (a, m) becomes (g*cos, g*sin), one float32 rounding per component.  With
 * BF_FUSED_OUT_INT8 the Q14 integer path needs |g| <= 1.992 (the high limb stays int8) and
 * A*max|x|*(sqrt(2)*max|g|*2^14 + 1) < 2^31 (no int32 overflow; max|x| = 128 signed, 255 unsigned); the Python
 * wrapper, which owns the host copy of the weights, checks both.  Without gains the library checks the unit-gain
 * bound itself (A <= 363 unsigned, A <= 724 signed) and returns BF_ERR_ARG beyond it.  Float beams (float output and
 * BF_FUSED_INT8_VIA_F32) need |g| <= 65504 and are f32-class only for weights of order 1: the float coefficient
 * domain and floor at bf_beamform.  bf_check_gains checks a host copy of the table against whichever bound applies. */
int bf_beamform_fused_weighted(const uint8_t* raw, const float* delay_vals, int delay_channels, const float* gains,
                               void* y, int B, int C, int T, int A, int M, int Ctot, int xeng_id,
                               double sample_period, double t0, double batch_dt, int flags, float out_scale,
                               void* stream);
/* The weight bounds of bf_beamform_fused_weighted for the contract `flags` selects, checked on a HOST copy of the
 * (M, A) table (pure host code, no device): every weight finite; the Q14 integer contract's two conditions above; for
 * float beams max|g| <= 65504.  BF_ERR_ARG with the reason in bf_last_error otherwise.  bf_pipeline_set_gains applies
 * it; a caller of the device-pointer entry points, which cannot read the table, calls it before uploading. */
int bf_check_gains(const float* host_gains, int M, int A, int flags);

/* bf_beamform_fused_weighted with a caller-owned device workspace (the fused call itself never allocates).  With at
 * least bf_fused_workspace_bytes(...) bytes, the int8 beams of many antennas x beams (config 4: the 32-beam integer
 * kernel) take their Q14 coefficients from a table that bf_q14_coeffs' kernel writes into the workspace just before,
 * on `stream` -- the wavefront-parallel phasor generator of the reference's two-kernel structure (coeff_generator.py
 * then matrix_multiply.py; BeamformerKernels.cu:7-189), one float64 complex multiply per coefficient along the
 * channels -- instead of evaluating every phasor inside the contraction kernel.  Same contract, same bits; workspace
 * NULL (or too small) = bf_beamform_fused_weighted.  bf_fused_workspace_bytes gives 0 for shapes and flags that use
 * no workspace.  The workspace must be 16-byte aligned and must not be shared by calls in flight on other streams. */
int bf_fused_workspace_bytes(int B, int C, int T, int A, int M, int flags, size_t* bytes);
int bf_beamform_fused_ws(const uint8_t* raw, const float* delay_vals, int delay_channels, const float* gains, void* y,
                         int B, int C, int T, int A, int M, int Ctot, int xeng_id, double sample_period, double t0,
                         double batch_dt, int flags, float out_scale, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The launch bf_beamform_fused_ws would make for a call, as a pure host function (no device, no launch; like
 * bf_scatter_plan): which kernel a shape takes is decided in one place, and this asks it.  The arguments are the
 * call's: has_gains = gains != NULL, workspace_bytes = what the call would offer (0: none), cus = the device's compute
 * units (sizes the persistent kernel's grid only; 0 = the current device's, 256 when there is none).  T must be a
 * multiple of 16, delay_channels 1 or C.
 *   kernel          : the name bf_last_kernel reports after the call
 *   uses_table      : 1 when the Q14 table is generated into the workspace first (bf_q14_coeffs' kernel)
 *   workspace_bytes : what the table occupies there (0 without); bf_fused_workspace_bytes is this value for an
 *                     unlimited workspace
 *   grid, block, lds_bytes, nslabs, xcd_order, ch_run : the launch configuration of the contraction kernel
 * A call that bf_beamform_fused_ws would refuse for its shape (too many antennas for any kernel's LDS, a grid beyond
 * 2^31, the int32 bound of the Q14 contract) returns BF_ERR_ARG with the same message in bf_last_error. */
typedef struct bf_fused_plan_info {
  char kernel[96];
  int uses_table, nslabs, xcd_order, ch_run;
  unsigned grid, block;
  size_t lds_bytes, workspace_bytes;
} bf_fused_plan_info;
int bf_fused_plan(int B, int C, int T, int A, int M, int delay_channels, int has_gains, int flags, float out_scale,
                  size_t workspace_bytes, int cus, bf_fused_plan_info* out);

/* The int8 path's steering coefficients (the Q14 integer contract, oracle quantise_coeffs of fused_tables):
 *   out[b][c][m][a] = (uint16)Wc | (uint32)Ws << 16, Wc = rne(2^14 * RN32(g * RN32(cos rot))), Ws the same for sin,
 *   rot the reference's float64 phase (coeff_generator_cpu.py:145-164) of channel c + C * xeng_id at
 *   dt = t0 + b * batch_dt (SURVEY A3 time extension), g = gains[m][a] (NULL = 1).  delay_vals f32 (Cd, M, A, 4).
 *   The generator addresses a run of min(C, 64) channel blocks with 32-bit offsets: 4 * M * A * min(C, 64) >= 2^31
 *   returns BF_ERR_ARG. */
int bf_q14_coeffs(const float* delay_vals, int delay_channels, const float* gains, uint32_t* out, int B, int C, int A,
                  int M, int Ctot, int xeng_id, double sample_period, double t0, double batch_dt, void* stream);

/* 8-bit requantiser (no reference counterpart; SURVEY §7 build step 7): q = clamp(rne(y*scale), -127, 127), the product
 * one float32 rounding.  +-inf saturate to +-127.  A NaN (a NaN input, or inf * 0) gives -127: the clamp is
 * min(max(r, -127), 127) with IEEE maxNum / minNum, which drop the NaN operand.  y 16-byte, q 4-byte aligned. */
int bf_requant(const float* y, int8_t* q, size_t n, float scale, void* stream);

/* Incoherent beam (no reference counterpart): the power re^2 + im^2 of every antenna, summed over a set of antennas
 * and integrated over windows of `tint` samples, per pol and channel, from the fused operator's own input cube:
 *   raw      : 8-bit (B, A, C, T, 2, 2), uint8, or int8 with BF_INCOH_SIGNED (the sample_signed convention)
 *   ant_mask : u8 (A,) on the device, antenna a counts when ant_mask[a] != 0; NULL = every antenna
 *   out      : f32 (B, 2, C, T/tint), or (B, 1, C, T/tint) with BF_INCOH_SUM_POLS (the two pols added before scaling)
 *   S[b][p][c][j] = sum over counted a, t in [j*tint, (j+1)*tint) of re^2 + im^2          (exact integer)
 *   out           = float32(float64(S) * float64(scale))      (one float64 multiply, one round-to-nearest-even)
 * S does not depend on the order of summation and every output element is written once (no atomics: `out` need not
 * be zeroed), so the result is deterministic and bit-exact.  T % 16 == 0, T <= 2^20; tint divides T and is a power of
 * two <= 16 or a multiple of 16; 1 <= A <= 32768 (so S < 2^53); scale finite and > 0; raw 16-byte, out 4-byte
 * aligned.  A standalone pass over the voltages (bf_incoherent_algorithmic_bytes: 4*B*A*C*T voltage bytes, A mask
 * bytes when masked != 0, 4*B*(2 or 1)*C*T/tint output bytes). */
#define BF_INCOH_SIGNED 1
#define BF_INCOH_SUM_POLS 2
int bf_incoherent_beam(const uint8_t* raw, const uint8_t* ant_mask, float* out, int B, int C, int T, int A, int tint,
                       int flags, float scale, void* stream);
double bf_incoherent_algorithmic_bytes(int B, int C, int T, int A, int tint, int flags, int masked);

/* Beam detector (no reference counterpart): Stokes power of the beams, integrated over windows of `tint` samples and
 * `fint` channels, straight from the fused operator's output:
 *   beams : (B, 2, C, T/16, 16, 2M), f32, or int8 with BF_DETECT_IN_INT8 (the BF_FUSED_OUT_INT8 output); the last axis
 *           is (re, im) per beam, column 2m = re, 2m+1 = im
 *   out   : f32 (B, S, C/fint, T/tint, M), S = 1 (I), or 4 (I, Q, U, V) with BF_DETECT_STOKES_IQUV
 * With X = pol 0 and Y = pol 1 of (b, c, t, m):
 *   I = Xr^2+Xi^2+Yr^2+Yi^2   Q = Xr^2+Xi^2-Yr^2-Yi^2   U = 2(XrYr+XiYi)   V = 2(XiYr-XrYi)   (V = 2 Im(X conj Y))
 *   acc[b][s][k][j][m] = sum over c in [k*fint, (k+1)*fint), t in [j*tint, (j+1)*tint) of the term s
 *   out                = float32(float64(acc) * float64(scale))      (one multiply, one round-to-nearest-even)
 * X = 3+4i, Y = 1+2i gives I, Q, U, V = 30, 20, 22, -4 per sample.  int8 beams (-128 is legal, |term| <= 2^16): acc is
 * the exact integer sum, so the output is order-independent and bit-exact.  f32 beams: acc is a float64 sum of float64
 * products of the f32 values (the products are exact); the order of the additions is the kernel's own, fixed, so the
 * result is deterministic and within N * 2^-53 * (the window's I) of the exact sum, N = 4 * tint * fint, before the
 * scaling and the float32 rounding.  Every output element is written once (no atomics: `out` need not be zeroed) and
 * the input is never written.  B, C, T, M >= 1; T % 16 == 0, T <= 2^20; M <= 4096; tint >= 1 divides T; fint >= 1
 * divides C; tint * fint <= 2^31 (int8 sums stay below 2^53); scale finite and > 0; beams 16-byte, out 4-byte aligned.
 * bf_detect_algorithmic_bytes: (1 or 4) * B*2*C*T*2M input bytes + 4 * B*S*(C/fint)*(T/tint)*M output bytes; 0 for a
 * non-positive argument. */
#define BF_DETECT_IN_INT8 1      /* beams are int8 (the fused operator's BF_FUSED_OUT_INT8 output), else f32 */
#define BF_DETECT_STOKES_IQUV 2  /* four outputs I, Q, U, V; else I only */
int bf_beam_detect(const void* beams, float* out, int B, int C, int T, int M, int tint, int fint, int flags,
                   float scale, void* stream);
double bf_detect_algorithmic_bytes(int B, int C, int T, int M, int tint, int fint, int flags);

/* Voltage statistics (no reference counterpart): the first two moments of the sample power of every antenna, pol and
 * channel over windows of `tint` samples, from the fused operator's own input cube -- the level monitor and the
 * spectral-kurtosis estimator (Nita & Gary 2010) that tell a caller which inputs to mask or down-weight:
 *   raw       : 8-bit (B, A, C, T, 2, 2), uint8, or int8 with BF_VSTATS_SIGNED (the sample_signed convention)
 *   out_power : f32 (B, A, 2, C, T/tint)   out_sk : f32, same shape   out_flags : u8, same shape
 * Each output may be NULL; at least one must not be.  With n = tint and pw = re^2 + im^2 of one sample of one pol, for
 * the window t in [j*tint, (j+1)*tint) of (b, a, pol, c):
 *   S1 = sum pw          S2 = sum pw^2                                                           (exact integers)
 *   out_power = float32(float64(S1) * float64(scale))                (one float64 multiply, one round-to-nearest-even)
 *   out_sk    = S1 == 0 ? 0.0f : float32(k * ((nd * float64(S2)) / (float64(S1) * float64(S1)) - 1.0)),
 *               nd = float64(n), k = (nd + 1) / (nd - 1) computed once on the host in double
 *   out_flags = (S1 == 0 || out_sk < sk_lo || out_sk > sk_hi) ? 1 : 0    (float32 compares of the stored out_sk; a
 *               value equal to a limit is not flagged)
 * Every float64 operation is a separate IEEE operation in exactly that order (no multiply feeds an add), so all three
 * outputs are bit-exact, independent of the order of summation and deterministic.  out_sk is 1 for Gaussian noise
 * whatever its level, 0 for a constant-amplitude carrier, far above 1 for pulsed interference, and 0 with the flag set
 * for a dead input.  B, C, A >= 1, A <= 32768; T % 16 == 0, T <= 2^20; tint is a multiple of 16 that divides T, at
 * most 2^18 (S2 < 2^52 even for uint8, pw <= 130050: every integer is exact in float64); scale finite and > 0; with
 * out_flags, 0 <= sk_lo < sk_hi, both finite (ignored without); raw 16-byte, the f32 outputs 4-byte aligned.  Every
 * output element is written once (no atomics: the outputs need not be zeroed) and the input is never written.
 * bf_vstats_algorithmic_bytes: `outputs` is a bit mask (1 = power, 2 = sk, 4 = flags); 4*B*A*C*T voltage bytes plus
 * B*A*2*C*(T/tint) * (4 [power] + 4 [sk] + 1 [flags]) output bytes; 0 for a non-positive argument or an empty mask. */
#define BF_VSTATS_SIGNED 1
int bf_voltage_stats(const uint8_t* raw, float* out_power, float* out_sk, uint8_t* out_flags, int B, int C, int T,
                     int A, int tint, int flags, float scale, float sk_lo, float sk_hi, void* stream);
double bf_vstats_algorithmic_bytes(int B, int C, int T, int A, int tint, int outputs);

/* The correlator (no reference counterpart; the X-engine half of the engine the reference belongs to): the integer
 * visibilities of every antenna pair, from the fused operator's own input cube -- what delay and phase models, beam
 * weights and dead-antenna decisions are solved from:
 *   raw : 8-bit (B, A, C, T, 2, 2), uint8, or int8 with BF_CORR_SIGNED (the sample_signed convention)
 *   out : int32 (B/bint, C, T/tint, NBL, 2, 2, 2), NBL = A (A + 1) / 2; the baseline of (a1, a2), a1 >= a2, has index
 *         a1 (a1 + 1) / 2 + a2 (autos included); the last three axes are (p1, p2, (re, im))
 * With x[a,p] = re + i*im of one sample, for the window b in [k*bint, (k+1)*bint), t in [j*tint, (j+1)*tint):
 *   S[k][c][j][bl(a1,a2)][p1][p2] = sum over the window of x[a1,p1] * conj(x[a2,p2])
 *      re = sum r1*r2 + i1*i2        im = sum i1*r2 - r1*i2                                       (exact integers)
 * (x[a,0] = 3+4i, x[a,1] = 1+2i: the auto is (0,0) = 25, (0,1) = 11-2i, (1,0) = 11+2i, (1,1) = 5 per sample).  All
 * four pol products of an auto are stored: (1,0) is the conjugate of (0,1), redundant, but the layout stays one.
 * Without BF_CORR_ACCUMULATE every output element is written once by one thread (no atomics: out need not be zeroed);
 * with it the same thread reads the old value, adds and stores, in uint32 arithmetic (wrap-around is defined), and
 * keeping the sum of several calls inside int32 is the caller's business.  The input is never written; the result does
 * not depend on the order of summation.  B, C, A >= 1, A <= 2048; T % 16 == 0, T <= 2^20; tint is a multiple of 16
 * that divides T; bint >= 1 divides B, and bint > 1 needs tint == T; the samples per window n = bint * tint keep every
 * sum in int32: n <= 65535 for int8 (|term| <= 2 * 128^2), n <= 16512 for uint8 (term <= 2 * 255^2); unknown flag bits
 * are refused; raw 16-byte, out 4-byte aligned; a launch beyond 2^31 - 1 workgroups is refused.  Every refusal is
 * BF_ERR_ARG before any launch.
 * bf_correlate_algorithmic_bytes: 4*B*A*C*T voltage bytes plus 32 * NBL * (B/bint) * C * (T/tint) output bytes (twice
 * with BF_CORR_ACCUMULATE: read and written); 0 for any argument bf_correlate would refuse. */
#define BF_CORR_SIGNED 1       /* int8 samples (the sample_signed convention), else uint8 */
#define BF_CORR_ACCUMULATE 2   /* out += S instead of out = S */
int bf_correlate(const uint8_t* raw, int32_t* out, int B, int C, int T, int A, int tint, int bint, int flags,
                 void* stream);
double bf_correlate_algorithmic_bytes(int B, int C, int T, int A, int tint, int bint, int flags);

/* Beam streams (no reference counterpart: the reference has a PreBeamformReorder and nothing after the contraction):
 * the beams as per-beam voltage streams, any subset, each with the shape and sample order of one antenna of the voltage
 * cube -- what one subscriber, recorder or multicast group of a beam consumes, and what bf_voltage_stats, bf_correlate
 * and bf_incoherent_beam (int8, their signed flags) read directly with A = K:
 *   beams      : (B, 2, C, T/16, 16, 2M), f32, or int8 with BF_BSTREAM_IN_INT8 (the fused operator's output; column
 *                2m = re, 2m+1 = im)
 *   beam_index : int32 (K,) on the device, or NULL = the identity (then K must equal M)
 *   out        : (B, K, C, T, 2, 2), last axes (pol, (re, im)); the dtype of `beams`, or int8 with BF_BSTREAM_REQUANT
 *                (f32 beams only)
 *   m = beam_index[k]  (k, when NULL)
 *   out[b][k][c][t][p][z] = beams[b][p][c][t/16][t%16][2m + z]     if 0 <= m < M
 *                         = 0 (all bits zero)                      otherwise
 *   with BF_BSTREAM_REQUANT: out = clamp(rne(f32(beam value) * scale), -127, 127), bf_requant's formula (NaN -> -127).
 * A copy moves bits and nothing else: a NaN payload, -0.0 and -128 arrive unchanged.  The list may repeat beams, be in
 * any order and be longer than M; an index outside [0, M) is defined (the entry point cannot see a device list): its
 * stream is zero and nothing outside `beams` is read.  Every output element is written once by one thread (no atomics:
 * `out` need not be zeroed), the input is never written, two launches give identical bytes.  B, C, T, M, K >= 1;
 * T % 16 == 0, T <= 2^20; M <= 4096, K <= 4096; scale finite and > 0 with BF_BSTREAM_REQUANT (ignored without); beams
 * and out 16-byte, beam_index 4-byte aligned.  Refused with BF_ERR_ARG before any launch: unknown flag bits,
 * BF_BSTREAM_REQUANT with BF_BSTREAM_IN_INT8, beam_index NULL with K != M (or with BF_BSTREAM_LIST), misalignment, a
 * grid above 2^31 - 1 workgroups.
 * bf_beam_streams_algorithmic_bytes: es_in * B*2*C*T*2M input bytes -- the whole cube once for any list: the cost of a
 * dense read, a sparse list could read less -- plus es_out * B*K*C*T*4 output bytes, plus 4K list bytes with
 * BF_BSTREAM_LIST (this function sees no pointer: the bit says that a list is given; without it K must equal M);
 * es = 1 for int8, 4 for f32.  0 for any shape or flags bf_beam_streams refuses. */
#define BF_BSTREAM_IN_INT8 1  /* beams are int8 (the fused operator's BF_FUSED_OUT_INT8 output), else f32 */
#define BF_BSTREAM_REQUANT 2  /* f32 beams, int8 streams */
#define BF_BSTREAM_LIST 4     /* a beam list is given: optional for bf_beam_streams (beam_index says it), the byte
                                 count's only way to know */
int bf_beam_streams(const void* beams, const int32_t* beam_index, void* out, int B, int C, int T, int M, int K,
                    int flags, float scale, void* stream);
double bf_beam_streams_algorithmic_bytes(int B, int C, int T, int M, int K, int flags);

/* Dedisperser (no reference counterpart): incoherent dedispersion of one Stokes plane of bf_beam_detect's output into
 * one time series per beam and trial dispersion measure, over a caller-owned ring of the recent past:
 *   power : f32 (B, S, K, J, M), exactly bf_beam_detect's out (K = C/fint, J = T/tint); only plane `plane` is read.  The
 *           batches follow one another in time (as in bf_beamform_fused), so the call brings N = B*J new samples per
 *           channel and beam, time index n = b*J + j
 *   ring  : f32 (K, R, M), one slot per sample, beam fastest (the detector's own order); R a multiple of N; `head`, a
 *           multiple of N in [0, R), is the slot of this call's first sample.  The caller zeroes the ring before the
 *           first call and advances head' = (head + N) % R; the library keeps no state
 *   lags  : int32 (D, K) on the device, lags[d][k] = how many samples back channel k is read for trial d.  Legal values
 *           are 0 .. R - N; the entry point cannot see a device table, so the kernel clamps any other value into that
 *           range and never reads outside the ring.  Any table in range is legal (monotone or not)
 *   out   : f32 (M, D, N): one contiguous time series per beam and trial
 * In stream order:
 *   1. ring[k][(head + n) % R][m] = power[b][plane][k][j][m]              (bits copied; nothing else in ring changes)
 *   2. acc[m][d][n] = sum over k = 0 .. K-1 of ring[k][(head + n - lags[d][k]) mod R][m]  (float64 sum of the f32 values)
 *      out[m][d][n] = float32(acc * float64(scale))                       (one multiply, one round-to-nearest-even)
 * The order of the float64 additions is the kernel's own and fixed: two launches give identical
 * bytes; no atomics, `out` need not be zeroed, every element of `out` is written once by one thread; `power` and `lags`
 * are never written.  If the ring holds integer-valued f32 below 2^24 (a detector fed int8 beams at scale 1 with
 * tint * fint < 256), acc is exact in any order and out is bit-exact; for general f32 the result is within
 * K * 2^-53 * sum|x| of the exact sum before the scaling and the float32 rounding.
 * B, S, K, J, M, D >= 1; 0 <= plane < S; M <= 4096, D <= 4096; R >= N and R % N == 0; 0 <= head < R and head % N == 0;
 * scale finite and > 0; power, ring and out 16-byte, lags 4-byte aligned; all element offsets are 64-bit (a ring of
 * several GiB is normal).  Every refusal is BF_ERR_ARG before any launch.
 * bf_dedisperse_algorithmic_bytes: span_sum = sum over k of (max over d of lags[d][k] - min over d of lags[d][k]), from
 * the caller's host copy of the table; 4 * (2*K*N*M [the block read and appended] + (K*N + span_sum)*M [every ring
 * sample some trial needs, once] + D*N*M [the output]); 0 for any shape bf_dedisperse refuses and for span_sum < 0. */
int bf_dedisperse(const float* power, float* ring, const int32_t* lags, float* out, int B, int S, int plane, int K,
                  int J, int M, int D, int R, int head, float scale, void* stream);
double bf_dedisperse_algorithmic_bytes(int B, int K, int J, int M, int D, long long span_sum);

/* Pulse search (no reference counterpart): the matched filter of bf_dedisperse's output -- boxcar signal-to-noise of
 * every (beam, trial) time series at a list of widths against a running baseline, the best width per sample, one peak
 * record per (beam, trial) and one best record per beam.  What leaves the GPU is 16 bytes per (beam, trial) and 16 bytes
 * per beam per call.
 *   series  : f32 (M, D, N), exactly bf_dedisperse's out: N new samples of every (beam, trial) row
 *   ring    : f32 (M, D, R), the caller-owned past of the series, zeroed before the first call; R a multiple of N with
 *             R >= N + Wmax - 1; `head`, a multiple of N in [0, R), is the slot of this call's first sample
 *   moments : f64 (M, D, P, 2), the caller-owned block moments (sum x, sum x*x) of the last P calls, zeroed before the
 *             first call; `slot` in [0, P) is the one this call writes, `n_blocks` in [1, P] how many slots are filled
 *             once it has (the current one included)
 *   widths  : int32 (L) on the HOST, read before the call returns: 1 <= L <= 16, strictly ascending, 1 <= w <= 1024;
 *             Wmax = widths[L-1]
 *   snr, width_index : f32 and uint8 (M, D, N), written only with BF_PSEARCH_SERIES; both NULL without it
 *   peaks   : int32 (M, D, 4);  best : int32 (M, 4)
 * In stream order, per row (m, d):
 *   1. ring[m][d][(head + n) % R] = series[m][d][n]                        (bits copied; nothing else in ring changes)
 *   2. moments[m][d][slot] = (sum_n x, sum_n x*x) of the N new samples, float64 sums of the f32 values (nothing else in
 *      moments changes); S1, S2 = the sums over all P slots of the two moments (unfilled slots are the caller's zeros);
 *      cnt = n_blocks * N
 *   3. s_w[n] = sum over i < w of ring[m][d][(head + n - i) mod R]                                          (float64)
 *      num = cnt * s_w[n] - w * S1;  den = w * (cnt * S2 - S1 * S1)
 *      snr_w[n] = den > 0 ? float32(num / sqrt(den)) : 0     (float64 sqrt and division, one round-to-nearest-even)
 *      = (s_w - w * mean) / (sqrt(w) * sigma) over the last n_blocks blocks, the current one included.  The boxcar of
 *      width w ENDS at sample n: the centre of the pulse is at n - (w - 1) / 2.
 *   4. per sample the best width: the largest snr_w[n], ties to the smallest width index; the search starts from
 *      (-inf, index 0) and compares strictly, so a NaN never wins  -> snr[m][d][n], width_index[m][d][n]
 *   5. peaks[m][d] = { bits of the row's best snr, its n, its width index, count of n whose step-4 snr >= threshold };
 *      larger snr wins, then the smaller width index, then the smaller n; the search starts from (-inf, n 0, index 0)
 *      and compares strictly
 *   6. best[m] = { bits of the beam's best snr over its D peak records, that record's d, n, width index }; ties go to
 *      the smaller d; the search starts from (-inf, d 0, n 0, index 0)
 * The library keeps no state: the caller advances head' = (head + N) % R, slot' = (slot + 1) % P and
 * n_blocks' = min(n_blocks + 1, P).  Every output element is written once by one thread: no atomics, no output needs
 * zeroing, two launches give identical bytes; `series` is never written.  A row that holds a NaN has den > 0 false, so
 * its snr is 0 for as long as the NaN sits in its moments; other rows are unaffected.  For integer-valued series with
 * |num| and den below 2^53 every product and sum is exact in any order and what remains is one float64 sqrt, one float64
 * division and one conversion: the result is bit-exact.  For general f32 the float64 sums (of at most N + Wmax - 1
 * terms) are within (terms) * 2^-53 * sum|x| each.  There is no scale argument: a scale of the series cancels.
 * Refused with BF_ERR_ARG before any launch: a null pointer (snr and width_index: both NULL without
 * BF_PSEARCH_SERIES, both non-NULL with it); unknown flag bits; M, D, N or R not positive; M or D above 4096; L
 * outside 1..16; widths not strictly ascending or outside 1..1024; R % N != 0 or R < N + Wmax - 1; head not a multiple
 * of N in [0, R); P outside 1..64; slot outside [0, P); n_blocks outside [1, P]; n_blocks * N at or above 2^31; a
 * threshold that is not finite; series, ring, moments, snr, peaks or best not 16-byte aligned, width_index not 4-byte
 * aligned.  All element offsets are 64-bit.
 * bf_pulse_search_algorithmic_bytes: M*D * (4 * (2N + Wmax - 1) [the block read and appended, the history read once] +
 * 16 * P [the moment slots] + 16 [the peak record]) + 16 * M [the best records] + 5 * M*D*N with BF_PSEARCH_SERIES; 0
 * for any shape or flags bf_pulse_search refuses (L outside 1..16, Wmax outside L..1024, P outside 1..64 included). */
#define BF_PSEARCH_SERIES 1  /* write snr and width_index (M, D, N) */
int bf_pulse_search(const float* series, float* ring, double* moments, const int32_t* widths, float* snr,
                    uint8_t* width_index, int32_t* peaks, int32_t* best, int M, int D, int N, int R, int head, int P,
                    int slot, int n_blocks, int L, float threshold, int flags, void* stream);
double bf_pulse_search_algorithmic_bytes(int M, int D, int N, int L, int Wmax, int P, int flags);

/* Folder (no reference counterpart): pulsar profiles of bf_beam_detect's output.  For a pulsar of known period and
 * dispersion measure every sample of every channel is added into the phase bin its rotational phase falls in, with the
 * channel's dispersive delay taken out; what accumulates is a (plane, channel, bin) profile per fold.  A fold is a beam,
 * a phase and a phase step; several folds may name the same beam (several pulsars in one beam).
 *   power   : f32 (B, S, K, J, M), exactly bf_beam_detect's out; all S planes are folded.  N = B*J samples per channel
 *             and beam, time index n = b*J + j
 *   beam    : int32 (F) on the HOST, read before the call returns: 0 <= beam[f] < M, repeats and any order allowed
 *   phase0  : uint64 (F) on the HOST: the phase of sample n = 0, in turns * 2^64
 *   dphase  : uint64 (F) on the HOST: the phase step per sample, in turns * 2^64
 *   chan    : uint64 (F, K) on the device: the per-channel phase offset (the dispersive delay in turns), subtracted
 *   profile : f64 (F, S, K, nbin) on the device, caller-owned accumulators, zeroed by the caller before the first call
 *   hits    : uint32 (F, K, nbin) on the device, caller-owned, zeroed likewise
 *   phi(f,k,n) = phase0[f] - chan[f][k] + n * dphase[f]                     (uint64, wraps mod 2^64)
 *   bin        = ((phi >> 32) * nbin) >> 32                                 (integers only; always < nbin)
 *   profile[f][s][k][bin] += float64(power[b][s][k][j][beam[f]])            for every s
 *   hits[f][k][bin]       += 1
 * The phase is fixed-point so that the binning is exact and modular: it is what NumPy's uint64 arithmetic gives, no
 * floating-point contraction can move a sample to another bin, and a caller that advances phase0' = phase0 + N * dphase
 * (mod 2^64) continues the fold exactly.  The library keeps no state.
 *   1. Deterministic: two launches on equal inputs give equal bytes; no atomics; the updates of an accumulator element
 *      are ordered, and the order of the float64 additions is the kernel's own and fixed.
 *   2. If the power is integer-valued f32 and the accumulators stay below 2^53, profile is bit-exact; hits is always
 *      exact (mod 2^32).
 *   3. For general f32 an element is within t * 2^-53 * (|pre| + sum|x|) of the exact value: t its hit count in this call,
 *      pre its value before the call, sum|x| the sum of the magnitudes of the samples that fall into it.
 *   4. An element of profile or hits that receives no sample in a call is not written: the traffic follows the samples,
 *      not nbin.
 * power and chan are never written.
 * Refused with BF_ERR_ARG before any launch: a null pointer; any of B, S, K, J, M, F, nbin not positive; S > 4, M > 4096,
 * F > 64 or nbin > 4096; N = B*J above 2^31 - 1; a beam[f] outside [0, M); power not 16-byte, chan or profile not
 * 8-byte, hits not 4-byte aligned.  All element offsets are 64-bit (profile at F 64, S 4, K 4096, nbin 1024 is 8 GiB).
 * bf_fold_algorithmic_bytes: touched = the number of distinct (f, k, bin) that receive a sample in the call, counted by
 * the caller; 4*B*S*K*J*M [the block, once] + 8*F*K [chan] + touched * (16*S + 8) [the touched accumulators read and
 * written]; 0 for any shape bf_fold refuses and for touched < 0. */
int bf_fold(const float* power, const int32_t* beam, const uint64_t* phase0, const uint64_t* dphase,
            const uint64_t* chan, double* profile, uint32_t* hits, int B, int S, int K, int J, int M, int F, int nbin,
            void* stream);
double bf_fold_algorithmic_bytes(int B, int S, int K, int J, int M, int F, long long touched);

/* ---- streaming ingest --------------------------------------------------------
 * Pinned host frames -> H2D stream -> bf_beamform_fused_weighted on a compute stream -> D2H stream, over a ring of
 * `depth` device slots; the phases of successive frames overlap.  Replaces the back-to-back HtoD / kernel / DtoH
 * phases of the reference harness (common/UnitTest.cpp:28-57) and the event-chained PCIe loop
 * (utilities/pcie_bandwidth_tests/cudaPcieRateTest.cpp:63-123).  Frames have the fused operator's shapes: in
 * (B, A, C, T, 2, 2) 8-bit, out (B, 2, C, T/16, 16, 2M) f32 or int8.  Host buffers should be pinned
 * (bf_host_alloc) for the copies to overlap; they must stay untouched until bf_pipeline_wait(ticket, 0) (input)
 * / (ticket, 1) (output).  The pipeline lives on the device current at creation; calls restore the caller's device.
 * Delay-model and weight updates apply to every frame submitted after them (stream-ordered uploads). */
typedef struct bf_pipeline bf_pipeline;
int bf_pipeline_create(bf_pipeline** out, int B, int C, int T, int A, int M, int Ctot, int xeng_id,
                       double sample_period, int flags, float out_scale, int delay_channels, int depth);
int bf_pipeline_destroy(bf_pipeline* p);
int bf_pipeline_frame_bytes(const bf_pipeline* p, size_t* in_bytes, size_t* out_bytes);
int bf_pipeline_set_delays(bf_pipeline* p, const float* host_delay_vals);  /* host f32 (Cd, M, A, 4) */
/* host f32 (M, A); NULL = unit.  Refuses (BF_ERR_ARG) what bf_check_gains refuses for the pipeline's flags: for float
 * pipelines max|g| > 65504 (the float coefficient domain and floor at bf_beamform). */
int bf_pipeline_set_gains(bf_pipeline* p, const float* host_gains);
int bf_pipeline_submit(bf_pipeline* p, const void* host_in, void* host_out, double t0, double batch_dt,
                       long long* ticket);
int bf_pipeline_wait(bf_pipeline* p, long long ticket, int stage);         /* stage 0 input, 1 output */
int bf_pipeline_query(bf_pipeline* p, long long ticket, int stage, int* done);
int bf_pipeline_flush(bf_pipeline* p);
int bf_pipeline_stage_ms(bf_pipeline* p, long long ticket, float* h2d_ms, float* compute_ms, float* d2h_ms);

/* ---- multi-GPU channel scatter --------------------------------------------------------------
 * One process per GPU, rank r = X-engine r owning channels [C r, C (r+1)) of a C*N-channel band (the reference's
 * absolute-channel convention, beamformer/beamforming/coeff_generator.py:49-53; its only multi-device pattern is a
 * host thread per device, utilities/pcie_bandwidth_tests/main.cpp:193-224, which this replaces).  The hot path
 * needs no collective; the root hands each rank its channel slice of a full-band cube once, device to device over
 * RCCL/xGMI.  RCCL (/opt/rocm librccl.so.1) is loaded at the first bf_comm_* call.
 *   bf_comm_unique_id : rank 0 makes the communicator id (BF_COMM_ID_BYTES); the caller hands it to every rank
 *   bf_comm_create    : collective over all ranks, on the device current at the call
 *   bf_channel_scatter: band (B, A, C*N, T, 2, 2) 8-bit on `root` (ignored elsewhere) -> slice (B, A, C, T, 2, 2) on
 *                       every rank; stream-ordered on `stream`, in pieces of at most 256 MiB (whole (b, a) rows,
 *                       or segments of a longer row), one RCCL group per piece.  Root: each peer's slice 2-D packed
 *                       into a staging buffer of N - 1 slices (grown on demand) and sent with ncclSend, its own slice
 *                       one 2-D copy; at one rank the root's slice is packed and moved by a self ncclSend/ncclRecv
 *                       instead, so one rank runs the point-to-point path of N.  Peers: ncclRecv per piece.
 *   bf_comm_allreduce_max: host value -> max over ranks (blocking; timing brackets and agreement checks)
 *   bf_comm_stats     : bytes this rank has handed to ncclSend / ncclRecv so far (the scatter's RCCL traffic)
 *   bf_comm_load      : BF_OK when RCCL can be loaded (a local precondition each rank checks before the collective
 *                       bf_comm_create, so that no rank waits in it for a rank that already failed) */
#define BF_COMM_ID_BYTES 128
typedef struct bf_comm bf_comm;
int bf_comm_unique_id(void* id, size_t len);
int bf_comm_create(bf_comm** out, const void* id, size_t len, int nranks, int rank);
int bf_comm_destroy(bf_comm* comm);
int bf_comm_allreduce_max(bf_comm* comm, double* value);
int bf_channel_scatter(bf_comm* comm, const uint8_t* band, uint8_t* slice, int B, int A, int C, int T, int root,
                       void* stream);
int bf_comm_stats(const bf_comm* comm, unsigned long long* sent, unsigned long long* received);
int bf_comm_load(void);

/* The scatter's plan for one rank: pure host arithmetic (no device, no RCCL), the exact operation list
 * bf_channel_scatter executes, so the piece / staging-slot / send-receive pairing logic is testable on a CPU for any
 * N and root (tests/test_multi_rank.py replays the N ranks' plans on host buffers).  Ops in execution order:
 *   BF_SCATTER_COPY2D: `height` rows of `width` bytes, (src_space, src_off, src_pitch) -> (dst_space, dst_off,
 *                      dst_pitch); `peer` = the rank whose slice the rows belong to (root only)
 *   BF_SCATTER_SEND  : `width` bytes at (src_space, src_off) to rank `peer` (ncclSend)
 *   BF_SCATTER_RECV  : `width` bytes into (dst_space, dst_off) from rank `peer` (ncclRecv)
 * `group` numbers the pieces: one RCCL group per piece, its COPY2D ops first.  Spaces: the root's band, the root's
 * staging buffer (`*staging_bytes` long), this rank's slice.  chunk = the piece size in bytes (0: the product's
 * 256 MiB).  ops == NULL only counts; a capacity below the count fails with BF_ERR_ARG (`*n_ops` holds the count). */
#define BF_SCATTER_COPY2D 1
#define BF_SCATTER_SEND 2
#define BF_SCATTER_RECV 3
#define BF_SPACE_BAND 1
#define BF_SPACE_STAGING 2
#define BF_SPACE_SLICE 3
typedef struct bf_scatter_op {
  int kind, peer, group, src_space, dst_space, reserved;
  unsigned long long src_off, src_pitch, dst_off, dst_pitch, width, height;
} bf_scatter_op;
int bf_scatter_plan(int nranks, int rank, int root, int B, int A, int C, int T, size_t chunk, bf_scatter_op* ops,
                    size_t capacity, size_t* n_ops, size_t* staging_bytes);

/* Position-weighted 64-bit checksum of a 2-D device region (`rows` runs of `run_bytes`, `pitch_bytes` apart; 4-byte
 * words): sum over packed word index i of splitmix64(splitmix64(i) ^ word_i), mod 2^64 -- equal for a packed slice
 * and the strided band region it came from.  Blocking (synchronises `stream`); verification, not the hot path. */
int bf_checksum(const void* src, size_t run_bytes, size_t pitch_bytes, size_t rows, unsigned long long* out,
                void* stream);

/* Fill `bytes` of device memory with a deterministic pseudo-random byte stream (splitmix64 of seed and position):
 * synthetic voltages made in HBM (bench.py's full-band cube at N GPUs), no host staging. */
int bf_fill_random(void* dst, size_t bytes, unsigned long long seed, void* stream);

/* Algorithmic HBM bytes of one bf_beamform_fused launch (bench / roofline bookkeeping). */
double bf_fused_algorithmic_bytes(int B, int C, int T, int A, int M, int delay_channels, int out_int8);

#ifdef __cplusplus
}
#endif
#endif /* DPDK_DC_SAND_AMD_BF_H */
