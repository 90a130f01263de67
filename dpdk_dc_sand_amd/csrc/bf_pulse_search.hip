// Pulse search: boxcar S/N and peak candidates of the DM-trial time series (no reference counterpart).  The matched
// filter of bf_dedisperse's output over a caller-owned ring of its recent past and a caller-owned baseline of block
// moments (include/bf.h, bf_pulse_search), per row (m, d):
//   1. ring[(head + n) % R] = series[n]                                                            (bits copied)
//   2. moments[slot] = (sum x, sum x*x) of the N new samples (float64); S1, S2 = the sums of all P slots;
//      cnt = n_blocks * N
//   3. s_w[n] = sum of the w ring samples that end at n (float64); num = cnt*s_w - w*S1; den = w*(cnt*S2 - S1*S1);
//      snr_w[n] = den > 0 ? float32(num / sqrt(den)) : 0
//   4. per sample the best width (largest snr, then smallest width index)
//   5. per row the peak record {snr bits, n, width index, count of n at or above the threshold}
//   6. per beam the best of its D peak records (second launch)
// Every output element is written once by one thread, no atomics, nothing zeroed beforehand, two launches give
// identical bytes.
//
// Two kernels, in stream order.
//   * pulse_search_kernel: the unit of work is a row, and rows are short (16 new samples behind 127 of history at
//     config 4, 128 behind 127 at config 3), so a row belongs to a *group* of G = 16, 32 or 64 consecutive lanes of one
//     wave (the launcher takes the smallest G that is at least min(N, 64)) and a workgroup of 4 waves owns 256 / G
//     whole rows: steps 1 to 5 need nothing from another workgroup.  Pass A walks the N new samples once: appends
//     them, sums x and x*x in float64 (a lane's partial sums, then a butterfly over the group), stores the slot's
//     moments as one 16-byte store, adds the other P - 1 slots from memory and leaves sqrt(den_i) of width i in lane
//     i of the group (L <= 16 <= G).  Pass B walks the row in tiles of T outputs: the tile's window (its outputs and
//     the Wmax - 1 samples before them: history from the ring, contiguous apart from one wrap, the rest from
//     `series`) is scanned once, in chunks of G, into a float64 exclusive prefix E in the group's own LDS, so that
//     s_w[n] = E[p + 1] - E[p + 1 - w]: L subtractions per sample instead of sum(w) additions.  A lane then takes the
//     outputs n0 + lane, n0 + lane + G, ..., keeps its own peak and count in the order of step 5, and the group
//     reduces them by a butterfly in the same order; lane 0 of the group stores the record as one 16-byte store.
//     The widths travel by value in the kernel arguments: one kernel for every shape and width list.  All loops have
//     the same trip counts in every wave of a workgroup (rows past the end load nothing and store nothing, but walk
//     along), so the barriers between the scan and its readers are uniform.
//   * pulse_best_kernel: one wave per beam walks the D records in ascending d.
#include <cmath>

#include "bf_common.hpp"

namespace bf {
namespace {

constexpr int kThreads = 256;     // 4 waves; 256 / G rows per workgroup
constexpr int kMaxWidths = 16;
constexpr int kMaxTile = 256;     // outputs per tile: the group's LDS holds kMaxTile + Wmax float64 at the most
constexpr int kLdsBudget = 48 * 1024;

struct Widths {
  int w[kMaxWidths];
};

struct SearchArgs {
  const float* series;
  float* ring;
  double* moments;
  float* snr;              // NULL without BF_PSEARCH_SERIES
  unsigned char* width_index;
  int32_t* peaks;
  long long rows;          // M * D
  int N, R, head, P, slot, L, Wmax, G, T;
  double cnt;              // n_blocks * N
  float threshold;
  Widths widths;
};

struct Peak {
  float snr;
  int n, idx;
};

// The order of step 5: larger snr, then smaller width index, then smaller n.  Strict: a NaN never wins.
__device__ inline bool beats(const Peak& a, const Peak& b) {
  return a.snr > b.snr || (a.snr == b.snr && (a.idx < b.idx || (a.idx == b.idx && a.n < b.n)));
}

__device__ inline double group_sum(double v, int G) {
  for (int s = 1; s < G; s <<= 1) v += __shfl_xor(v, s, G);  // a butterfly: every lane ends with the same sum
  return v;
}

__global__ __launch_bounds__(kThreads) void pulse_search_kernel(SearchArgs A) {
  extern __shared__ double lds[];

  const int G = A.G;
  const int gl = threadIdx.x % G;                   // lane within the group
  const int grp = threadIdx.x / G;                  // group within the workgroup
  const long long row = static_cast<long long>(blockIdx.x) * (kThreads / G) + grp;
  const bool live = row < A.rows;
  const long long r = live ? row : 0;               // a dead group walks along on row 0 and stores nothing
  const float* series = A.series + r * A.N;
  float* ring = A.ring + r * A.R;
  double* E = lds + static_cast<long long>(grp) * (A.T + A.Wmax);
  const int hist = A.Wmax - 1;

  // Pass A: append, the block's moments, the baseline.
  double m1 = 0.0, m2 = 0.0;
  for (int n = gl; n < A.N; n += G) {
    const float x = series[n];
    if (live) ring[A.head + n] = x;                 // head + N <= R: no wrap inside the block
    const double xd = static_cast<double>(x);
    m1 += xd;
    m2 += xd * xd;
  }
  m1 = group_sum(m1, G);
  m2 = group_sum(m2, G);
  double2* mom = reinterpret_cast<double2*>(A.moments) + r * A.P;
  if (live && gl == 0) mom[A.slot] = make_double2(m1, m2);
  double s1 = 0.0, s2 = 0.0;
  for (int p = gl; p < A.P; p += G) {
    if (p != A.slot) {
      const double2 v = mom[p];
      s1 += v.x;
      s2 += v.y;
    }
  }
  const double S1 = group_sum(s1, G) + m1, S2 = group_sum(s2, G) + m2;
  // lane i < L of the group: sqrt(den_i), or 0 where den_i > 0 is false (a NaN included)
  double root = 0.0;
  for (int i = 0; i < A.L; ++i) {  // a uniform index: the widths stay in the kernel arguments
    if (gl == i) {
      const double den = static_cast<double>(A.widths.w[i]) * (A.cnt * S2 - S1 * S1);
      root = den > 0.0 ? sqrt(den) : 0.0;
    }
  }

  // Pass B: the row in tiles of T outputs.
  Peak mine = {-INFINITY, 0, 0};
  int count = 0;
  for (int n0 = 0; n0 < A.N; n0 += A.T) {
    const int len = A.N - n0 < A.T ? A.N - n0 : A.T;  // outputs of this tile
    const int win = len + hist;                       // window sample j is stream offset q = n0 - hist + j
    if (n0 > 0) __syncthreads();                      // the previous tile's readers are done with E
    double carry = 0.0;
    if (gl == 0) E[0] = 0.0;
    for (int j0 = 0; j0 < win; j0 += G) {
      const int j = j0 + gl;
      const int q = n0 - hist + j;
      float x = 0.0f;
      if (j < win) {
        if (q >= 0) {
          x = series[q];
        } else {
          int s = A.head + q;                         // in (-R, R): R >= N + Wmax - 1
          if (s < 0) s += A.R;
          x = ring[s];                                // never a slot of this call's block: those are [head, head + N)
        }
      }
      double v = static_cast<double>(x);
      for (int s = 1; s < G; s <<= 1) {               // inclusive scan over the group
        const double up = __shfl_up(v, s, G);
        if (gl >= s) v += up;
      }
      v += carry;
      if (j < win) E[j + 1] = v;
      carry = __shfl(v, G - 1, G);
    }
    __syncthreads();
    for (int t0 = 0; t0 < len; t0 += G) {
      const int t = t0 + gl;
      const bool has = t < len;
      const int p1 = hist + (has ? t : 0) + 1;        // E[p1] = the window up to and including output t
      const double top = E[p1];
      float best = -INFINITY;
      int bi = 0;
      for (int i = 0; i < A.L; ++i) {
        const int w = A.widths.w[i];
        const double sq = __shfl(root, i, G);
        const double s = top - E[p1 - w];
        const double num = A.cnt * s - static_cast<double>(w) * S1;
        const float v = sq > 0.0 ? static_cast<float>(num / sq) : 0.0f;
        if (v > best) {
          best = v;
          bi = i;
        }
      }
      if (has) {
        const int n = n0 + t;
        if (live && A.snr) {
          A.snr[r * A.N + n] = best;
          A.width_index[r * A.N + n] = static_cast<unsigned char>(bi);
        }
        const Peak c = {best, n, bi};
        if (beats(c, mine)) mine = c;
        count += best >= A.threshold ? 1 : 0;
      }
    }
  }

  for (int s = 1; s < G; s <<= 1) {
    Peak o;
    o.snr = __shfl_xor(mine.snr, s, G);
    o.n = __shfl_xor(mine.n, s, G);
    o.idx = __shfl_xor(mine.idx, s, G);
    count += __shfl_xor(count, s, G);
    if (beats(o, mine)) mine = o;
  }
  if (live && gl == 0)
    reinterpret_cast<int4*>(A.peaks)[r] = make_int4(__float_as_int(mine.snr), mine.n, mine.idx, count);
}

// Step 6: one wave per beam; lane l walks d = l, l + 64, ... in ascending order, then the lanes meet.  Larger snr wins,
// ties go to the smaller d; the search starts from (-inf, d 0, n 0, index 0).
__global__ __launch_bounds__(64) void pulse_best_kernel(const int32_t* peaks, int32_t* best, int D) {
  const int4* rec = reinterpret_cast<const int4*>(peaks) + static_cast<long long>(blockIdx.x) * D;
  float snr = -INFINITY;
  int d = 0, n = 0, idx = 0;
  for (int i = threadIdx.x; i < D; i += 64) {
    const int4 v = rec[i];
    const float s = __int_as_float(v.x);
    if (s > snr) {
      snr = s;
      d = i;
      n = v.y;
      idx = v.z;
    }
  }
  for (int s = 1; s < 64; s <<= 1) {
    const float os = __shfl_xor(snr, s);
    const int od = __shfl_xor(d, s), on = __shfl_xor(n, s), oi = __shfl_xor(idx, s);
    if (os > snr || (os == snr && od < d)) {
      snr = os;
      d = od;
      n = on;
      idx = oi;
    }
  }
  if (threadIdx.x == 0) reinterpret_cast<int4*>(best)[blockIdx.x] = make_int4(__float_as_int(snr), d, n, idx);
}

// The widths of a call: 1 <= L <= 16, strictly ascending, 1 <= w <= 1024.  Returns Wmax, or 0.
inline int check_widths(const int32_t* widths, int L) {
  if (!widths || L < 1 || L > kMaxWidths) return 0;
  for (int i = 0; i < L; ++i)
    if (widths[i] < 1 || widths[i] > 1024 || (i > 0 && widths[i] <= widths[i - 1])) return 0;
  return widths[L - 1];
}

}  // namespace
}  // namespace bf

extern "C" int bf_pulse_search(const float* series, float* ring, double* moments, const int32_t* widths, float* snr,
                               uint8_t* width_index, int32_t* peaks, int32_t* best, int M, int D, int N, int R,
                               int head, int P, int slot, int n_blocks, int L, float threshold, int flags,
                               void* stream) {
  BF_REQUIRE(series && ring && moments && widths && peaks && best, "bf_pulse_search: null pointer");
  BF_REQUIRE((flags & ~BF_PSEARCH_SERIES) == 0, "bf_pulse_search: unknown flags 0x%x", flags);
  if (flags & BF_PSEARCH_SERIES)
    BF_REQUIRE(snr && width_index, "bf_pulse_search: null pointer (snr and width_index with BF_PSEARCH_SERIES)");
  else
    BF_REQUIRE(!snr && !width_index, "bf_pulse_search: snr and width_index must be NULL without BF_PSEARCH_SERIES");
  BF_REQUIRE(M > 0 && D > 0 && N > 0 && R > 0, "bf_pulse_search: bad shape M=%d D=%d N=%d R=%d", M, D, N, R);
  BF_REQUIRE(M <= 4096, "bf_pulse_search: bad shape, M=%d above 4096", M);
  BF_REQUIRE(D <= 4096, "bf_pulse_search: bad shape, D=%d above 4096", D);
  BF_REQUIRE(L >= 1 && L <= bf::kMaxWidths, "bf_pulse_search: %d widths outside 1..16", L);
  const int Wmax = bf::check_widths(widths, L);
  BF_REQUIRE(Wmax > 0, "bf_pulse_search: widths must be strictly ascending in 1..1024");
  BF_REQUIRE(R % N == 0 && static_cast<long long>(R) >= static_cast<long long>(N) + Wmax - 1,
             "bf_pulse_search: ring length %d must be a multiple of N = %d that is at least N + Wmax - 1 = %lld", R, N,
             static_cast<long long>(N) + Wmax - 1);
  BF_REQUIRE(head >= 0 && head < R && head % N == 0, "bf_pulse_search: head %d must be a multiple of N = %d in [0, %d)",
             head, N, R);
  BF_REQUIRE(P >= 1 && P <= 64, "bf_pulse_search: %d baseline blocks outside 1..64", P);
  BF_REQUIRE(slot >= 0 && slot < P, "bf_pulse_search: slot %d outside [0, %d)", slot, P);
  BF_REQUIRE(n_blocks >= 1 && n_blocks <= P, "bf_pulse_search: n_blocks %d outside [1, %d]", n_blocks, P);
  BF_REQUIRE(static_cast<long long>(n_blocks) * N < (1ll << 31),
             "bf_pulse_search: n_blocks * N = %lld at or above 2^31", static_cast<long long>(n_blocks) * N);
  BF_REQUIRE(std::isfinite(threshold), "bf_pulse_search: threshold must be finite");
  BF_REQUIRE((reinterpret_cast<uintptr_t>(series) & 15) == 0 && (reinterpret_cast<uintptr_t>(ring) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(moments) & 15) == 0 && (reinterpret_cast<uintptr_t>(snr) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(peaks) & 15) == 0 && (reinterpret_cast<uintptr_t>(best) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(width_index) & 3) == 0,
             "bf_pulse_search: misaligned buffer");

  bf::SearchArgs A = {};
  A.series = series;
  A.ring = ring;
  A.moments = moments;
  A.snr = snr;
  A.width_index = width_index;
  A.peaks = peaks;
  A.rows = static_cast<long long>(M) * D;
  A.N = N;
  A.R = R;
  A.head = head;
  A.P = P;
  A.slot = slot;
  A.L = L;
  A.Wmax = Wmax;
  A.cnt = static_cast<double>(n_blocks) * N;
  A.threshold = threshold;
  for (int i = 0; i < bf::kMaxWidths; ++i) A.widths.w[i] = i < L ? widths[i] : 1;
  // The group: the smallest of 16, 32, 64 lanes that is at least min(N, 64); wider while the workgroup's prefix
  // arrays ((256 / G) * (T + Wmax) float64) would not fit the LDS budget.
  int G = N <= 16 ? 16 : (N <= 32 ? 32 : 64);
  int T = 0;
  for (;; G *= 2) {
    const int whole = (N + G - 1) / G * G;
    T = whole < bf::kMaxTile ? whole : bf::kMaxTile;
    if (G == 64 || static_cast<size_t>(bf::kThreads / G) * (T + Wmax) * sizeof(double) <= bf::kLdsBudget) break;
  }
  A.G = G;
  A.T = T;
  const size_t lds = static_cast<size_t>(bf::kThreads / G) * (T + Wmax) * sizeof(double);
  const int per_wg = bf::kThreads / G;
  const unsigned grid = static_cast<unsigned>((A.rows + per_wg - 1) / per_wg);  // M * D <= 2^24

  hipStream_t st = bf::as_stream(stream);
  hipLaunchKernelGGL(bf::pulse_search_kernel, dim3(grid), dim3(bf::kThreads), lds, st, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bf::hip_fail(e, "pulse_search_kernel");
  hipLaunchKernelGGL(bf::pulse_best_kernel, dim3(M), dim3(64), 0, st, peaks, best, D);
  BF_LAUNCHED_TAG("pulse_search_kernel", "g%d,t%d", G, T);  // the filter kernel names the call
}

extern "C" double bf_pulse_search_algorithmic_bytes(int M, int D, int N, int L, int Wmax, int P, int flags) {
  if (M <= 0 || D <= 0 || N <= 0 || M > 4096 || D > 4096 || L < 1 || L > bf::kMaxWidths || Wmax < L || Wmax > 1024 ||
      P < 1 || P > 64 || (flags & ~BF_PSEARCH_SERIES))
    return 0.0;
  const double rows = static_cast<double>(M) * D;
  return rows * (4.0 * (2.0 * N + Wmax - 1) + 16.0 * P + 16.0) + 16.0 * M +
         ((flags & BF_PSEARCH_SERIES) ? 5.0 * rows * N : 0.0);
}
