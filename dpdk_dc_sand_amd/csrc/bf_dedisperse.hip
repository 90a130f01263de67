// Dedisperser: DM-trial time series of the detected beams (no reference counterpart).  Incoherent dedispersion of one
// Stokes plane of the beam detector's output over a caller-owned ring of the recent past (include/bf.h):
//   1. ring[k][(head + n) % R][m] = power[b][plane][k][j][m], n = b*J + j                         (bits copied)
//   2. out[m][d][n] = float32(float64(scale) * sum over k of ring[k][(head + n - lag[d][k]) mod R][m])
// the sum in float64, one value per addition, in the fixed order described below: every output element is written once
// by one thread, no atomics, no zeroed output, two launches give identical bytes.
//
// Two kernels, in stream order.
//   * append_kernel: B*K runs of J*M floats; 16-byte accesses when J*M is a multiple of 4 (every run of the block and
//     of the ring then starts on 16 bytes: R, head and the batch offsets are multiples of N = B*J), else element accesses.
//   * dedisperse_kernel: time and beam flattened, position e = n*M + m, which is contiguous in the ring (beam fastest):
//     with x = head*M + e, trial d of channel k reads ring_k[(x - lag*M) mod R*M], so a wave's 64 lanes read 256
//     contiguous bytes per trial.  A workgroup of 16 waves owns 64 positions (one per lane) and kDt = 8 trials; a lane
//     keeps its 8 float64 sums in registers.  The call is a read stream with almost no arithmetic, and at the shapes of
//     use (N*M of one or two thousand positions) what bounds it is how many loads are in flight, not reuse: a
//     workgroup that walks all K channels alone waits K/4 memory latencies in a row (measured: 5.5 ms at K = 4096,
//     whatever the trial count, with the window staged in LDS; profiles/dedisperse_ops_lds_staged.jsonl).  So the
//     channels are dealt to the 16 waves in chunks of kKc = 4 consecutive channels, chunk q to wave q % 16: every wave
//     walks K/16 channels in ascending order, the loads of its next chunk (kKc * kDt = 32 per lane, all in flight) issued
//     before the adds of this one, and at the end the 16 partial sums of an output element meet in LDS, where the thread
//     that owns the element adds them in ascending wave order, scales and stores.  The order of the additions is
//     therefore fixed: ((chunks of wave 0, ascending) + (chunks of wave 1) + ...), no second pass, no atomics.  The lags
//     of a chunk are uniform over the wave (scalar loads of 4 consecutive table entries per trial).  Trials whose runs
//     overlap (the top of the band, neighbouring DMs) meet in the L1 / L2 caches; there is no LDS window and hence no
//     fallback path: any lag table takes the same code.
//     Lags outside [0, R - N] are clamped (the table is device memory the entry point cannot check): every ring index
//     is reduced into [0, R*M), so nothing outside the ring is read whatever the table holds.
// The output (1/K of the traffic) is stored strided, one float per thread.
#include <cmath>

#include "bf_common.hpp"

namespace bf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;          // append
constexpr int kLanes = 64;             // positions per workgroup: one wave wide
constexpr int kDt = 8;                 // trials per workgroup: float64 sums per lane
constexpr int kWaves = 16;             // waves per workgroup: each walks every 16th chunk of channels
constexpr int kKc = 4;                 // channels per chunk: kKc * kDt loads in flight per lane and chunk
static_assert(kWaves >= kDt, "the epilogue gives wave w < kDt the trial d0 + w");

struct AppendArgs {
  const float* power;
  float* ring;
  unsigned long long run;       // J * M floats (or 16-byte units) of one (b, k) run
  unsigned long long total;     // B * K runs
  unsigned long long src_b, src_k, src_0;  // strides and offset of power, in the same units
  unsigned long long dst_b, dst_k, dst_0;  // of the ring
  int K;
};

// Unit = float or u32x4: bits are moved, nothing else.
template <typename Unit>
__global__ __launch_bounds__(kThreads) void append_kernel(AppendArgs P) {
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= P.total) return;
  const unsigned long long r = i / P.run, off = i % P.run;
  const unsigned long long b = r / P.K, k = r % P.K;
  const Unit* src = reinterpret_cast<const Unit*>(P.power) + P.src_0 + b * P.src_b + k * P.src_k + off;
  Unit* dst = reinterpret_cast<Unit*>(P.ring) + P.dst_0 + b * P.dst_b + k * P.dst_k + off;
  *dst = __builtin_nontemporal_load(src);
}

struct DedispArgs {
  const float* ring;
  const int32_t* lags;
  float* out;
  long long RM, NM, headM;  // floats: one channel's ring, one channel's block, the block's first slot
  int K, M, D, N, lag_max;  // lag_max = R - N
  double scale;
};

__global__ __launch_bounds__(kLanes * kWaves) void dedisperse_kernel(DedispArgs P) {
  __shared__ double part[kWaves][kDt][kLanes];

  const int lane = threadIdx.x % kLanes;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const long long e = static_cast<long long>(blockIdx.x) * kLanes + lane;
  const bool live = e < P.NM;
  const long long x = P.headM + e;  // < R*M for a live lane
  const int d0 = blockIdx.y * kDt;
  const int chunks = (P.K + kKc - 1) / kKc;

  // The loads of chunk q: channel 4q + c, trial d0 + i -> v[c][i] (0 past K and for a lane past the end).
  auto issue = [&](int q, float(&v)[kKc][kDt]) {
#pragma unroll
    for (int c = 0; c < kKc; ++c) {
      const int k = q * kKc + c;
      if (k < P.K) {
        const float* src = P.ring + static_cast<long long>(k) * P.RM;
        int lag[kDt];
#pragma unroll
        for (int i = 0; i < kDt; ++i) {
          const int d = d0 + i < P.D ? d0 + i : P.D - 1;  // a partial trial tile repeats the last trial (never stored)
          const int t = P.lags[static_cast<long long>(d) * P.K + k];
          lag[i] = t < 0 ? 0 : (t > P.lag_max ? P.lag_max : t);
        }
#pragma unroll
        for (int i = 0; i < kDt; ++i) {
          long long idx = x - static_cast<long long>(lag[i]) * P.M;  // in (-R*M, R*M) for a live lane
          if (idx < 0) idx += P.RM;
          v[c][i] = live ? src[idx] : 0.0f;
        }
      } else {
#pragma unroll
        for (int i = 0; i < kDt; ++i) v[c][i] = 0.0f;
      }
    }
  };

  double acc[kDt] = {};
  auto add = [&](const float(&v)[kKc][kDt]) {
#pragma unroll
    for (int c = 0; c < kKc; ++c)
#pragma unroll
      for (int i = 0; i < kDt; ++i) acc[i] += static_cast<double>(v[c][i]);
  };

  float a[kKc][kDt], b[kKc][kDt];
  int q = w;
  if (q < chunks) issue(q, a);
#pragma unroll 1
  for (; q < chunks; q += 2 * kWaves) {
    const bool more = q + kWaves < chunks;
    if (more) issue(q + kWaves, b);
    add(a);
    if (more) {
      if (q + 2 * kWaves < chunks) issue(q + 2 * kWaves, a);
      add(b);
    }
  }

#pragma unroll
  for (int i = 0; i < kDt; ++i) part[w][i][lane] = acc[i];
  __syncthreads();
  // thread (w, lane), w < kDt, owns trial d0 + w of its position: the 16 waves' sums in ascending wave order
  if (!live || w >= kDt || d0 + w >= P.D) return;
  double sum = part[0][w][lane];
#pragma unroll
  for (int g = 1; g < kWaves; ++g) sum += part[g][w][lane];
  const long long n = e / P.M, m = e % P.M;
  P.out[(m * P.D + d0 + w) * P.N + n] = static_cast<float>(sum * P.scale);  // one multiply, one RNE
}

}  // namespace
}  // namespace bf

extern "C" int bf_dedisperse(const float* power, float* ring, const int32_t* lags, float* out, int B, int S, int plane,
                             int K, int J, int M, int D, int R, int head, float scale, void* stream) {
  BF_REQUIRE(power && ring && lags && out, "bf_dedisperse: null pointer");
  BF_REQUIRE(B > 0 && S > 0 && K > 0 && J > 0 && M > 0 && D > 0, "bf_dedisperse: bad shape B=%d S=%d K=%d J=%d M=%d D=%d",
             B, S, K, J, M, D);
  BF_REQUIRE(plane >= 0 && plane < S, "bf_dedisperse: plane %d outside [0, %d)", plane, S);
  BF_REQUIRE(M <= 4096, "bf_dedisperse: bad shape, M=%d above 4096", M);
  BF_REQUIRE(D <= 4096, "bf_dedisperse: bad shape, D=%d above 4096", D);
  const long long N = static_cast<long long>(B) * J;
  BF_REQUIRE(R >= N && R % N == 0, "bf_dedisperse: ring length %d must be a positive multiple of N = B*J = %lld", R, N);
  BF_REQUIRE(head >= 0 && head < R && head % N == 0, "bf_dedisperse: head %d must be a multiple of N = %lld in [0, %d)",
             head, N, R);
  BF_REQUIRE(std::isfinite(scale) && scale > 0.0f, "bf_dedisperse: scale must be finite and > 0");
  BF_REQUIRE((reinterpret_cast<uintptr_t>(power) & 15) == 0 && (reinterpret_cast<uintptr_t>(ring) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(lags) & 3) == 0,
             "bf_dedisperse: misaligned buffer");

  const unsigned long long JM = static_cast<unsigned long long>(J) * M, uK = K, uR = R;
  const bool wide = JM % 4 == 0;  // then every offset below is a multiple of 4 floats
  const unsigned long long u = wide ? 4 : 1;
  bf::AppendArgs A = {};
  A.power = power;
  A.ring = ring;
  A.run = JM / u;
  A.total = static_cast<unsigned long long>(B) * uK * A.run;
  A.src_k = JM / u;
  A.src_b = static_cast<unsigned long long>(S) * uK * JM / u;
  A.src_0 = static_cast<unsigned long long>(plane) * uK * JM / u;
  A.dst_k = uR * M / u;
  A.dst_b = JM / u;
  A.dst_0 = static_cast<unsigned long long>(head) * M / u;
  A.K = K;
  const unsigned long long grid_a = (A.total + bf::kThreads - 1) / bf::kThreads;

  bf::DedispArgs P = {};
  P.ring = ring;
  P.lags = lags;
  P.out = out;
  P.RM = static_cast<long long>(R) * M;
  P.NM = N * M;
  P.headM = static_cast<long long>(head) * M;
  P.K = K;
  P.M = M;
  P.D = D;
  P.N = static_cast<int>(N);
  P.lag_max = static_cast<int>(R - N);
  P.scale = static_cast<double>(scale);
  const unsigned long long grid_x = (static_cast<unsigned long long>(P.NM) + bf::kLanes - 1) / bf::kLanes;
  BF_REQUIRE(grid_a <= 0x7fffffffull && grid_x <= 0x7fffffffull,
             "bf_dedisperse: bad shape, %llu workgroups exceed the grid limit", grid_a > grid_x ? grid_a : grid_x);

  hipStream_t st = bf::as_stream(stream);
  if (wide)
    hipLaunchKernelGGL(bf::append_kernel<bf::u32x4>, dim3(static_cast<unsigned>(grid_a)), dim3(bf::kThreads), 0, st, A);
  else
    hipLaunchKernelGGL(bf::append_kernel<float>, dim3(static_cast<unsigned>(grid_a)), dim3(bf::kThreads), 0, st, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bf::hip_fail(e, "dedisperse_append_kernel");
  hipLaunchKernelGGL(bf::dedisperse_kernel, dim3(static_cast<unsigned>(grid_x), (D + bf::kDt - 1) / bf::kDt),
                     dim3(bf::kLanes * bf::kWaves), 0, st, P);
  BF_LAUNCHED("dedisperse_kernel");
}

extern "C" double bf_dedisperse_algorithmic_bytes(int B, int K, int J, int M, int D, long long span_sum) {
  if (B <= 0 || K <= 0 || J <= 0 || M <= 0 || D <= 0 || M > 4096 || D > 4096 || span_sum < 0) return 0.0;
  const double N = static_cast<double>(B) * J;
  if (N > 2147483647.0) return 0.0;
  const double KN = static_cast<double>(K) * N;
  return 4.0 * (2.0 * KN * M + (KN + static_cast<double>(span_sum)) * M + static_cast<double>(D) * N * M);
}
