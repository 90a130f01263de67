// Beam detector: Stokes power of the fused operator's beams, integrated over windows of tint samples and fint
// channels (no reference counterpart).  For beams y[b][p][c][t][m] (complex; f32 or int8, the fused output layout
// (B, 2, C, T/16, 16, 2M)), X = pol 0, Y = pol 1:
//   I = |X|^2 + |Y|^2   Q = |X|^2 - |Y|^2   U = 2 Re(X conj Y)   V = 2 Im(X conj Y)
//   acc[b][s][k][j][m] = sum over c in [k*fint, (k+1)*fint), t in [j*tint, (j+1)*tint) of the term s
//   out                = float32(float64(acc) * float64(scale))
// X = 3+4i, Y = 1+2i gives I, Q, U, V = 30, 20, 22, -4 per sample.  int8 beams: acc is the exact integer sum (bit-exact
// output); f32 beams: float64 products (exact) and float64 sums in the fixed order below.
//
// A pure HBM read stream.  One (b, p, c) run is N = T*M complex values, time and beam flattened: position e = t*M + m.
// Every lane takes X and Y of the same positions with two 16-byte non-temporal loads at the same offset of the two
// pol planes (E = 2 complex f32 or 8 complex int8 per load), a workgroup of 256 threads takes S = 256*E contiguous
// positions per step (1 KiB per wave-load), and walks so that a lane meets the same output cells (j, m) in every
// load between two flushes: its E * (1 or 4) sums stay in registers over the fint channels and over the steps
// (kUnroll loads of X and of Y in flight).  int8 terms (|PX|, |PY|, |U/2|, |V/2 parts| <= 2^15 per sample, I alone
// <= 2^16) are summed in 32 bits for at most 2^14 loads, then added into 64 bits; f32 values are converted to float64
// once each and enter float64 FMAs (the products are exact: 24-bit factors).
// A flush adds the lane's elements that share a cell, writes the rest to LDS, and the thread that owns an output
// element adds the slots of its cell in ascending order, scales and stores: every element is written once by one
// thread, no atomics, no zeroed output, deterministic.  LDS rows are padded by one slot against bank conflicts.  A
// workgroup owns whole windows.  Three walks:
//   * M and tint powers of two (detect_pow2_kernel): position bits [a, a+w) (M = 2^a, tint = 2^w) are the ones summed
//     over.  A window of at least a step (R = tint*M >= S) is one piece (per S-wide column block when M > S) walked in
//     steps and flushed once; smaller windows make one-step pieces of S/R whole windows; runs shorter than a step put
//     S/N channel groups side by side in one step.  int8 walks of at most 2048 loads keep 32-bit lane sums and slots.
//   * any other M or tint, lcm(M, E) <= S: the step is cut to P, the largest multiple of lcm(M, E) in S, so a lane
//     keeps its beams from period to period; a period (all fint channels) is flushed at once, the thread holding the
//     first slot of a beam adds that beam's rows of the period and carries the open window in registers.  A workgroup
//     takes lcm(tint, P/M) rows: whole windows.
//   * lcm(M, E) > S (M > 256, not a power of two, or tint not one): see detect_rows_kernel.
// Lanes past the end of a run load nothing and store nothing.
#include <cmath>
#include <type_traits>

#include "bf_common.hpp"

namespace bf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kUnroll = 4;       // loads of X and of Y in flight per lane
constexpr int kNarrowLoads = 2048;  // int8: 2048 loads * 8 elements * 2^16 = 2^30
constexpr int kRun32 = 1 << 14;  // int8: loads summed in 32 bits before the 64-bit add (2^14 * 2^16 = 2^30)
constexpr int kSlotValues = 16;  // values per thread of one LDS pass: 16 rows of kRow 8-byte slots, 32 KiB
constexpr int kRow = kThreads + 1;  // slot (value, thread) is [value * kRow + thread]: the owners of neighbouring cells
                                    // read neighbouring values of one thread, which rows of 256 put on one LDS bank

// The loads of one lane between two flushes: n_out x n_in, strides in complex values.
struct Walk {
  unsigned n_in, n_out;
  unsigned long long stride_in, stride_out;
};

struct DetectArgs {
  const uint8_t* beams;
  float* out;
  unsigned long long N;      // T * M: complex values of one (b, p, c) run
  unsigned long long plane;  // C * N: complex values between the two pol planes
  unsigned long long J;      // T / tint
  int M, T, tint, fint, K;   // K = C / fint
  double scale;
  unsigned pieces;  // workgroups per (b, k)
  Walk walk;        // Pow2 and period walks
  // Pow2 walk
  int a, w;                          // M = 2^a, tint = 2^w
  unsigned colblocks;                // S-wide column blocks per window (M > S), else 1
  unsigned kspan, kblocks, nlog;     // channel groups per step (N < S), blocks of them, log2 N
  unsigned long long piece_stride;   // positions between pieces of one column block
  // general walk
  unsigned P, rowsP, gper, nper;  // period (complex), its rows (or the row classes), periods per piece, periods
};

template <bool Int8>
struct Num {
  using Acc = double;
  static constexpr int E = 2, CB = 8;  // complex per 16-byte load, bytes per complex
};
template <>
struct Num<true> {
  using Acc = long long;
  static constexpr int E = 8, CB = 2;
};

__device__ __forceinline__ u32x4 load16(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot4(static_cast<int>(a), static_cast<int>(b), c, false);
}

__device__ __forceinline__ double f64(uint32_t f32_bits) { return static_cast<double>(__uint_as_float(f32_bits)); }

// One load of X and of Y, f32: element e is words 2e (re), 2e+1 (im).  v[e] = PX, PY, U/2, V/2 (or I alone).
template <bool Iquv>
__device__ __forceinline__ void terms_f32(const u32x4 x, const u32x4 y, double (&v)[2][Iquv ? 4 : 1]) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const double xr = f64(x[2 * e]), xi = f64(x[2 * e + 1]), yr = f64(y[2 * e]), yi = f64(y[2 * e + 1]);
    if constexpr (Iquv) {
      v[e][0] = fma(xi, xi, fma(xr, xr, v[e][0]));
      v[e][1] = fma(yi, yi, fma(yr, yr, v[e][1]));
      v[e][2] = fma(xi, yi, fma(xr, yr, v[e][2]));
      v[e][3] = fma(-xr, yi, fma(xi, yr, v[e][3]));
    } else {
      v[e][0] = fma(yi, yi, fma(yr, yr, fma(xi, xi, fma(xr, xr, v[e][0]))));
    }
  }
}

// One load of X and of Y, int8: dword d holds elements 2d (bytes 0, 1 = re, im) and 2d+1 (bytes 2, 3).
// part[e] = PX, PY, U/2, Xi*Yr, Xr*Yi (or I alone, read as unsigned: at most 2^16 per sample).
template <bool Iquv>
__device__ __forceinline__ void terms_i8(const u32x4 x, const u32x4 y, int (&part)[8][Iquv ? 5 : 1]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t xs = x[d], ys = y[d];
    const uint32_t ysw = ((ys & 0x00ff00ffu) << 8) | ((ys >> 8) & 0x00ff00ffu);  // (im, re) of both elements
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t both = 0xffffu << (16 * h), re = 0xffu << (16 * h), im = 0xff00u << (16 * h);
      int(&p)[Iquv ? 5 : 1] = part[2 * d + h];
      if constexpr (Iquv) {
        p[0] = dot4(xs, xs & both, p[0]);
        p[1] = dot4(ys, ys & both, p[1]);
        p[2] = dot4(xs, ys & both, p[2]);
        p[3] = dot4(xs & im, ysw, p[3]);  // Xi * Yr
        p[4] = dot4(xs & re, ysw, p[4]);  // Xr * Yi
      } else {
        p[0] = dot4(ys, ys & both, dot4(xs, xs & both, p[0]));
      }
    }
  }
}

// The lane's sums over its n_out x n_in loads, as I, Q, U, V (or I) per element.  AccT is Num<Int8>::Acc, or int for
// int8 walks of at most kNarrowLoads loads (a lane's sums, its 8 elements added, then stay below 2^31).
template <bool Int8, bool Iquv, typename AccT>
__device__ __forceinline__ void accumulate(const Walk& P, const uint8_t* px, size_t y_off, bool live,
                                           AccT (&v)[Num<Int8>::E][Iquv ? 4 : 1]) {
  constexpr int E = Num<Int8>::E, CB = Num<Int8>::CB, NS = Iquv ? 4 : 1;
#pragma unroll
  for (int e = 0; e < E; ++e)
#pragma unroll
    for (int s = 0; s < NS; ++s) v[e][s] = 0;
  if (!live) return;
  const size_t step_in = static_cast<size_t>(P.stride_in) * CB, step_out = static_cast<size_t>(P.stride_out) * CB;
  for (unsigned o = 0; o < P.n_out; ++o) {
    const uint8_t* p = px + o * step_out;
    for (unsigned i0 = 0; i0 < P.n_in; i0 += kRun32) {
      const unsigned n = P.n_in - i0 < static_cast<unsigned>(kRun32) ? P.n_in - i0 : kRun32;
      int part[Int8 ? E : 1][Iquv ? 5 : 1] = {};
      auto add = [&](const u32x4 x, const u32x4 y) {
        if constexpr (Int8)
          terms_i8<Iquv>(x, y, part);
        else
          terms_f32<Iquv>(x, y, v);
      };
      unsigned i = 0;
      for (; i + kUnroll <= n; i += kUnroll) {
        u32x4 x[kUnroll], y[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          x[u] = load16(p + u * step_in);
          y[u] = load16(p + u * step_in + y_off);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) add(x[u], y[u]);
        p += kUnroll * step_in;
      }
      for (; i < n; ++i) {
        const u32x4 x = load16(p), y = load16(p + y_off);
        add(x, y);
        p += step_in;
      }
      if constexpr (Int8) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if constexpr (Iquv) {
            v[e][0] += static_cast<AccT>(part[e][0]) + part[e][1];
            v[e][1] += static_cast<AccT>(part[e][0]) - part[e][1];
            v[e][2] += 2 * static_cast<AccT>(part[e][2]);
            v[e][3] += 2 * (static_cast<AccT>(part[e][3]) - part[e][4]);
          } else {
            v[e][0] += static_cast<AccT>(static_cast<uint32_t>(part[e][0]));
          }
        }
      }
    }
  }
  if constexpr (!Int8 && Iquv) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double px2 = v[e][0], py2 = v[e][1];
      v[e][0] = px2 + py2;
      v[e][1] = px2 - py2;
      v[e][2] *= 2.0;
      v[e][3] *= 2.0;
    }
  }
}

template <typename Acc>
__device__ __forceinline__ float scaled(Acc s, double scale) {
  return static_cast<float>(static_cast<double>(s) * scale);  // int8: |s| < 2^53, exact; then one RNE conversion
}

// M = 2^a, tint = 2^w.  Position bits of a step: element (LB bits), thread (8 bits).  A run shorter than a step
// (N < S, N a power of two) puts kspan = S / N channel groups side by side in one step: position bits above log2 N
// then count channel groups.
// Narrow (int8 walks of at most kNarrowLoads loads): the lane's sums and the slots are 32 bits wide, all Stokes terms
// in one pass; the owner still adds in 64 bits.
template <bool Int8, bool Iquv, bool Narrow>
__global__ __launch_bounds__(kThreads) void detect_pow2_kernel(DetectArgs P) {
  using Acc = typename Num<Int8>::Acc;
  using Lane = std::conditional_t<Narrow, int, Acc>;
  constexpr int E = Num<Int8>::E, CB = Num<Int8>::CB, NS = Iquv ? 4 : 1;
  constexpr int LB = Int8 ? 3 : 1, SB = LB + 8, S = kThreads * E;
  constexpr int NSP = Narrow || E * NS <= kSlotValues ? NS : kSlotValues / E;  // Stokes terms per pass
  static_assert(NSP * E * sizeof(Lane) <= kSlotValues * 8, "one pass fits the slot rows");
  __shared__ Lane slot[NSP * E * kRow];

  const int tid = threadIdx.x;
  const unsigned piece = blockIdx.x % P.pieces, bk = blockIdx.x / P.pieces;
  const unsigned k0 = bk % P.kblocks * P.kspan, b = bk / P.kblocks;
  const unsigned long long base = static_cast<unsigned long long>(piece / P.colblocks) * P.piece_stride +
                                  static_cast<unsigned long long>(piece % P.colblocks) * S;
  const unsigned long long at = base + static_cast<unsigned long long>(tid) * E;
  const unsigned kk = P.kspan > 1 ? static_cast<unsigned>(at >> P.nlog) : 0;  // the lane's channel group: k0 + kk
  const unsigned long long e0 = P.kspan > 1 ? at & (P.N - 1) : at;
  const unsigned long long run =
      (static_cast<unsigned long long>(b) * 2 * P.K * P.fint + static_cast<unsigned long long>(k0 + kk) * P.fint) * P.N;

  Lane v[E][NS];
  accumulate<Int8, Iquv>(P.walk, P.beams + (run + e0) * CB, static_cast<size_t>(P.plane) * CB,
                         k0 + kk < static_cast<unsigned>(P.K) && e0 < P.N, v);

  // the lane's elements that differ only in summed bits
  const int lo = P.a, hi = P.a + P.w;
#pragma unroll
  for (int bit = 0; bit < LB; ++bit) {
    if (bit >= lo && bit < hi) {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (!(e >> bit & 1)) {
#pragma unroll
          for (int s = 0; s < NS; ++s) v[e][s] += v[e | 1 << bit][s];
        }
    }
  }
  const int al = lo < SB ? lo : SB, ah = hi < SB ? hi : SB;  // summed bits of the step: [al, ah)
  const int lane_sum = (ah < LB ? ah : LB) - (al < LB ? al : LB);
  const unsigned dead = ((1u << lane_sum) - 1) << (al < LB ? al : LB);  // element bits already added
  const int tlo = (al > LB ? al : LB) - LB, tn = ah > LB ? ah - (al > LB ? al : LB) : 0;  // thread bits still to add
  const unsigned ncell = static_cast<unsigned>(S) >> (ah - al);

#pragma unroll
  for (int s0 = 0; s0 < NS; s0 += NSP) {
    if (s0) __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (!(e & dead)) {
#pragma unroll
        for (int s = 0; s < NSP; ++s) slot[(s * E + e) * kRow + tid] = v[e][s0 + s];
      }
    __syncthreads();
    // the owner of an output element adds its cell's slots in ascending thread order
    for (unsigned q = tid; q < NSP * ncell; q += kThreads) {
      const unsigned s = q / ncell, c = q % ncell;
      const unsigned full = (c & ((1u << al) - 1)) | ((c >> al) << ah);  // the cell's first position of the step
      unsigned long long e = base + full;
      unsigned k = k0;
      if (P.kspan > 1) {
        k += static_cast<unsigned>(e >> P.nlog);
        e &= P.N - 1;
      }
      if (e >= P.N || k >= static_cast<unsigned>(P.K)) continue;
      const Lane* src = slot + (s * E + (full & (E - 1))) * kRow + (full >> LB);
      Acc sum = src[0];
      for (unsigned r = 1; r < (1u << tn); ++r) sum += src[r << tlo];
      const unsigned long long j = e >> (P.a + P.w), m = e & (P.M - 1);
      P.out[(((static_cast<unsigned long long>(b) * NS + s0 + s) * P.K + k) * P.J + j) * P.M + m] =
          scaled(sum, P.scale);
    }
  }
}

// Any M and tint with lcm(M, E) <= S.  Offset x of the period is row x / M, beam x % M.
template <bool Int8, bool Iquv>
__global__ __launch_bounds__(kThreads) void detect_period_kernel(DetectArgs P) {
  using Acc = typename Num<Int8>::Acc;
  constexpr int E = Num<Int8>::E, CB = Num<Int8>::CB, NS = Iquv ? 4 : 1;
  constexpr int NSP = E * NS <= kSlotValues ? NS : kSlotValues / E;
  __shared__ Acc slot[NSP * E * kRow];

  const int tid = threadIdx.x;
  const unsigned seg = blockIdx.x % P.pieces, bk = blockIdx.x / P.pieces;
  const unsigned k = bk % P.K, b = bk / P.K;
  const unsigned xt = tid * E;  // the lane's first offset in the period
  const unsigned long long run =
      (static_cast<unsigned long long>(b) * 2 * P.K * P.fint + static_cast<unsigned long long>(k) * P.fint) * P.N;
  const unsigned n_first = seg * P.gper, n_last = n_first + P.gper < P.nper ? n_first + P.gper : P.nper;

  Acc open[E][NS] = {};  // the open window of the beams this thread owns
  for (unsigned n = n_first; n < n_last; ++n) {
    const unsigned long long e0 = static_cast<unsigned long long>(n) * P.P + xt;
    Acc v[E][NS];
    accumulate<Int8, Iquv>(P.walk, P.beams + (run + e0) * CB, static_cast<size_t>(P.plane) * CB, xt < P.P && e0 < P.N,
                           v);
#pragma unroll
    for (int s0 = 0; s0 < NS; s0 += NSP) {
      if (s0 || n > n_first) __syncthreads();
#pragma unroll
      for (int e = 0; e < E; ++e)
#pragma unroll
        for (int s = 0; s < NSP; ++s) slot[(s * E + e) * kRow + tid] = v[e][s0 + s];
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned m = xt + e;  // the first slot of beam m in the period is offset m
        if (m >= static_cast<unsigned>(P.M)) continue;
        unsigned long long t = static_cast<unsigned long long>(n) * P.rowsP;
        for (unsigned xx = m; xx < P.P && t < static_cast<unsigned long long>(P.T); xx += P.M, ++t) {
#pragma unroll
          for (int s = 0; s < NSP; ++s) open[e][s0 + s] += slot[(s * E + xx % E) * kRow + xx / E];
          if ((t + 1) % P.tint == 0) {
#pragma unroll
            for (int s = 0; s < NSP; ++s) {
              P.out[(((static_cast<unsigned long long>(b) * NS + s0 + s) * P.K + k) * P.J + t / P.tint) * P.M + m] =
                  scaled(open[e][s0 + s], P.scale);
              open[e][s0 + s] = 0;
            }
          }
        }
      }
    }
  }
}

// Any tint, M with lcm(M, E) > S (so M > 256): a workgroup owns one window of a block of S - E beams.  The rows of the
// window whose first position has the same offset in its 16 bytes (row classes, rowsP = E / gcd(M, E) of them) give a
// lane the same beams, so each class is summed in registers and flushed once; the 16 bytes that hold a block's edge
// are loaded by both neighbours, each taking its own beams of them.
template <bool Int8, bool Iquv>
__global__ __launch_bounds__(kThreads) void detect_rows_kernel(DetectArgs P) {
  using Acc = typename Num<Int8>::Acc;
  constexpr int E = Num<Int8>::E, CB = Num<Int8>::CB, NS = Iquv ? 4 : 1;
  constexpr unsigned W = kThreads * E - E;
  constexpr int NSP = E * NS <= kSlotValues ? NS : kSlotValues / E;
  __shared__ Acc slot[NSP * E * kRow];

  const int tid = threadIdx.x;
  const unsigned piece = blockIdx.x % P.pieces, bk = blockIdx.x / P.pieces;
  const unsigned k = bk % P.K, b = bk / P.K;
  const unsigned long long j = piece / P.colblocks;
  const unsigned m0 = piece % P.colblocks * W, wc = P.M - m0 < W ? P.M - m0 : W;
  const unsigned long long run =
      (static_cast<unsigned long long>(b) * 2 * P.K * P.fint + static_cast<unsigned long long>(k) * P.fint) * P.N;

  Acc open[E][NS] = {};  // beams m0 + tid * E + e of the window
  for (unsigned rho = 0; rho < P.rowsP && rho < static_cast<unsigned>(P.tint); ++rho) {
    const unsigned long long first = (j * P.tint + rho) * P.M + m0;  // the block's start in the class's first row
    const unsigned delta = static_cast<unsigned>(first % E);
    const unsigned long long e0 = first - delta + static_cast<unsigned long long>(tid) * E;
    const unsigned rows = (P.tint - rho + P.rowsP - 1) / P.rowsP;
    const unsigned long long row_stride = static_cast<unsigned long long>(P.rowsP) * P.M;
    const unsigned fint = P.fint;
    const Walk walk = fint >= rows ? Walk{fint, rows, P.N, row_stride} : Walk{rows, fint, row_stride, P.N};
    Acc v[E][NS];
    accumulate<Int8, Iquv>(walk, P.beams + (run + e0) * CB, static_cast<size_t>(P.plane) * CB, e0 < first + wc, v);
#pragma unroll
    for (int s0 = 0; s0 < NS; s0 += NSP) {
      if (s0 || rho) __syncthreads();
#pragma unroll
      for (int e = 0; e < E; ++e)
#pragma unroll
        for (int s = 0; s < NSP; ++s) slot[(s * E + e) * kRow + tid] = v[e][s0 + s];
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned off = tid * E + e + delta;
        if (tid * E + e < wc) {
#pragma unroll
          for (int s = 0; s < NSP; ++s) open[e][s0 + s] += slot[(s * E + off % E) * kRow + off / E];
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (tid * E + e < wc) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
        P.out[(((static_cast<unsigned long long>(b) * NS + s) * P.K + k) * P.J + j) * P.M + m0 + tid * E + e] =
            scaled(open[e][s], P.scale);
    }
}

enum class Path { kPow2, kPow2Narrow, kPeriod, kRows };

template <bool Int8, bool Iquv>
void launch(const DetectArgs& P, Path path, unsigned grid, hipStream_t st) {
  if (path == Path::kPow2)
    hipLaunchKernelGGL((detect_pow2_kernel<Int8, Iquv, false>), dim3(grid), dim3(kThreads), 0, st, P);
  else if (path == Path::kPow2Narrow)
    hipLaunchKernelGGL((detect_pow2_kernel<Int8, Iquv, Int8>), dim3(grid), dim3(kThreads), 0, st, P);
  else if (path == Path::kPeriod)
    hipLaunchKernelGGL((detect_period_kernel<Int8, Iquv>), dim3(grid), dim3(kThreads), 0, st, P);
  else
    hipLaunchKernelGGL((detect_rows_kernel<Int8, Iquv>), dim3(grid), dim3(kThreads), 0, st, P);
}

int log2_exact(unsigned v) {  // v a power of two
  int n = 0;
  while ((1u << n) < v) ++n;
  return n;
}

unsigned long long gcd(unsigned long long x, unsigned long long y) {
  while (y) {
    const unsigned long long r = x % y;
    x = y;
    y = r;
  }
  return x;
}

}  // namespace
}  // namespace bf

extern "C" int bf_beam_detect(const void* beams, float* out, int B, int C, int T, int M, int tint, int fint, int flags,
                              float scale, void* stream) {
  BF_REQUIRE(beams && out, "bf_beam_detect: null pointer");
  BF_REQUIRE(B > 0 && C > 0 && T > 0 && M > 0, "bf_beam_detect: bad shape B=%d C=%d T=%d M=%d", B, C, T, M);
  BF_REQUIRE(T % bf::kSamplesPerBlock == 0, "bf_beam_detect: T=%d must be a multiple of 16", T);
  BF_REQUIRE(T <= (1 << 20), "bf_beam_detect: bad shape, T=%d above 2^20", T);
  BF_REQUIRE(M <= 4096, "bf_beam_detect: bad shape, M=%d above 4096", M);
  BF_REQUIRE(tint > 0 && T % tint == 0, "bf_beam_detect: time integration %d must divide T=%d", tint, T);
  BF_REQUIRE(fint > 0 && C % fint == 0, "bf_beam_detect: channel integration %d must divide C=%d", fint, C);
  BF_REQUIRE(static_cast<long long>(tint) * fint <= (1ll << 31),
             "bf_beam_detect: integration %d x %d samples exceeds 2^31", tint, fint);
  BF_REQUIRE((flags & ~(BF_DETECT_IN_INT8 | BF_DETECT_STOKES_IQUV)) == 0, "bf_beam_detect: unknown flags 0x%x", flags);
  BF_REQUIRE(std::isfinite(scale) && scale > 0.0f, "bf_beam_detect: scale must be finite and > 0");
  BF_REQUIRE((reinterpret_cast<uintptr_t>(beams) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
             "bf_beam_detect: misaligned buffer");

  const bool int8 = flags & BF_DETECT_IN_INT8;
  const unsigned E = int8 ? 8 : 2, S = bf::kThreads * E;
  bf::DetectArgs P = {};
  P.beams = static_cast<const uint8_t*>(beams);
  P.out = out;
  P.N = static_cast<unsigned long long>(T) * M;
  P.plane = static_cast<unsigned long long>(C) * P.N;
  P.J = T / tint;
  P.M = M;
  P.T = T;
  P.tint = tint;
  P.fint = fint;
  P.K = C / fint;
  P.scale = static_cast<double>(scale);
  const bool pow2 = (M & (M - 1)) == 0 && (tint & (tint - 1)) == 0;
  unsigned long long pieces;
  bf::Path path = bf::Path::kPow2;
  if (pow2) {
    P.a = bf::log2_exact(M);
    P.w = bf::log2_exact(tint);
    const unsigned long long R = static_cast<unsigned long long>(tint) * M;  // positions of one window
    unsigned long long steps = 1, step_stride = S;
    P.colblocks = 1;
    P.kspan = 1;
    if (R >= S) {  // one piece per window (and S-wide column block): steps of S positions, or of whole rows when M > S
      P.colblocks = static_cast<unsigned>(M) > S ? M / S : 1;
      step_stride = static_cast<unsigned>(M) > S ? M : S;
      steps = R / step_stride;
      P.piece_stride = R;
      pieces = P.N / R * P.colblocks;
    } else {  // one-step pieces of S / R whole windows
      P.piece_stride = S;
      pieces = (P.N + S - 1) / S;
      if (P.N < S && S % P.N == 0) {  // short runs: S / N channel groups per step
        P.kspan = static_cast<unsigned>(S / P.N);
        P.nlog = bf::log2_exact(static_cast<unsigned>(P.N));
      }
    }
    P.kblocks = (P.K + P.kspan - 1) / P.kspan;
    if (int8 && steps * fint <= bf::kNarrowLoads) path = bf::Path::kPow2Narrow;
    if (static_cast<unsigned long long>(fint) >= steps) {  // the longer axis is the inner one (kUnroll loads in flight)
      P.walk = {static_cast<unsigned>(fint), static_cast<unsigned>(steps), P.N, step_stride};
    } else {
      P.walk = {static_cast<unsigned>(steps), static_cast<unsigned>(fint), step_stride, P.N};
    }
  } else {
    const unsigned long long L = static_cast<unsigned long long>(M) / bf::gcd(M, E) * E;  // lcm(M, E) <= 32768
    if (L <= S) {
      path = bf::Path::kPeriod;
      P.P = static_cast<unsigned>(S / L * L);
      P.rowsP = P.P / M;
      P.nper = (T + P.rowsP - 1) / P.rowsP;
      P.gper = static_cast<unsigned>(tint / bf::gcd(tint, P.rowsP));  // lcm(tint, rowsP) rows: whole windows
      P.walk = {static_cast<unsigned>(fint), 1u, P.N, 0ull};
      pieces = (P.nper + P.gper - 1) / P.gper;
    } else {
      path = bf::Path::kRows;
      P.rowsP = static_cast<unsigned>(L / M);  // row classes
      P.colblocks = (M + (S - E) - 1) / (S - E);
      pieces = P.J * P.colblocks;
    }
  }
  const unsigned long long grid = pieces * (pow2 ? P.kblocks : P.K) * B;
  BF_REQUIRE(grid <= 0x7fffffffull, "bf_beam_detect: bad shape, %llu workgroups exceed the grid limit", grid);
  P.pieces = static_cast<unsigned>(pieces);
  hipStream_t st = bf::as_stream(stream);
  switch (flags) {
    case 0: bf::launch<false, false>(P, path, static_cast<unsigned>(grid), st); break;
    case BF_DETECT_IN_INT8: bf::launch<true, false>(P, path, static_cast<unsigned>(grid), st); break;
    case BF_DETECT_STOKES_IQUV: bf::launch<false, true>(P, path, static_cast<unsigned>(grid), st); break;
    default: bf::launch<true, true>(P, path, static_cast<unsigned>(grid), st); break;
  }
  BF_LAUNCHED("detect_kernel");
}

extern "C" double bf_detect_algorithmic_bytes(int B, int C, int T, int M, int tint, int fint, int flags) {
  if (B <= 0 || C <= 0 || T <= 0 || M <= 0 || tint <= 0 || fint <= 0) return 0.0;
  const double values = static_cast<double>(B) * 2 * C * T * 2 * M;
  const int stokes = (flags & BF_DETECT_STOKES_IQUV) ? 4 : 1;
  const double outputs = static_cast<double>(B) * stokes * (C / fint) * (T / tint) * M;
  return ((flags & BF_DETECT_IN_INT8) ? 1.0 : 4.0) * values + 4.0 * outputs;
}
