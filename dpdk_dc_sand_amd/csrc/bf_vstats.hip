// Voltage statistics: the first two moments of the sample power of the raw voltages, per antenna, pol, channel and
// time window (no reference counterpart; the level monitor and the spectral-kurtosis estimator of Nita & Gary 2010,
// the statistic a B-engine uses to decide which inputs to mask).  For the fused operator's input cube
// x[b][a][c][t][p][z] (8-bit, z = re, im), with pw = re^2 + im^2 of one sample of one pol and n = tint:
//   S1[b][a][p][c][j] = sum over t in [j*tint, (j+1)*tint) of pw      S2 = the same sum of pw^2      (exact integers)
//   power = float32(float64(S1) * float64(scale))
//   sk    = S1 == 0 ? 0 : float32(k * ((n * float64(S2)) / (float64(S1) * float64(S1)) - 1)),   k = (n + 1) / (n - 1)
//   flags = S1 == 0 || sk < sk_lo || sk > sk_hi                                       (float32 compares of the stored sk)
// Every float64 operation is a separate IEEE operation (contraction is off in sk_value), so the three outputs are
// bit-exact against the NumPy restatement and do not depend on the order of summation.
//
// The simpler sibling of bf_incoherent.hip: the same flattening and no antenna walk.  For fixed (b, a) the (c, t) plane
// is one run of C*T dwords (one dword = one time sample: pol0 re, im, pol1 re, im), tint divides T, so the run is cut
// into C*T/tint consecutive windows and window w of pol p goes to out[((b*A + a)*2 + p) * C*T/tint + w].
//
// A workgroup (512 threads) owns a piece of whole windows of one run (16384 samples when tint divides 16384) and walks
// it in steps of 4096 samples = 16 KiB: two 16-byte non-temporal loads per lane, 8 KiB apart, 1 KiB contiguous per
// wave-load, the next step's loads issued before this step's arithmetic.  Per step:
//   1. per sample and pol, pw = the int8 dot product of the dword with itself masked to one half (v_dot4), S1 += pw in
//      32 bits (4 * 130050 per load), S2 += pw * pw in 64 bits (pw^2 passes 2^32 for uint8: v_mad_u64_u32);
//   2. the lane's sums per load go to LDS in sample order; 256 threads per pol add four consecutive entries (tint is
//      a multiple of 16 samples = 4 lanes), then the aligned group of r / 4 lanes that lies inside one window (r = the
//      largest power of two dividing tint / 4, at most a wave) by DPP row shifts, in registers: one set per four
//      lane-loads;
//   3. group sums go to LDS; the thread that owns a window adds the groups of its window and carries them over the
//      steps in registers, then computes the three values and stores them.
// Every output element is written once by one thread: no atomics, no zeroed output, deterministic.  The input is never
// written.
#include <cmath>

#include "bf_common.hpp"

namespace bf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kThreads = 512;
constexpr int kLoads = 2;                     // 16-byte loads per lane and step, kThreads * 16 bytes apart
constexpr int kEntries = kLoads * kThreads;   // lane-loads (4 samples each) of one step, in sample order
constexpr int kStep = 4 * kEntries;           // samples per workgroup step
constexpr int kPieceSteps = 4;                // steps per piece when windows are shorter than that
constexpr int kQuads = kEntries / 4;          // sums of four entries: one per thread and pol
constexpr int kOwned = 2;                     // windows a thread may own: tint = 16 has 2 * kThreads windows per piece
constexpr int kMaxTint = 1 << 18;
static_assert(kThreads == 2 * kQuads, "one thread per pol and quad");
static_assert(kQuads % 16 == 0, "a group of at most 64 / 4 quads lies inside one row of 16 lanes");
static_assert(kStep * kPieceSteps / 16 <= kOwned * kThreads, "every window of a piece has an owner");

struct VstatsArgs {
  const uint8_t* raw;
  float* power;
  float* sk;
  uint8_t* flags;
  u64 N;            // C * T: samples of one (b, a) run
  u64 windows;      // N / tint: output windows per (b, a, pol)
  unsigned pieces;  // workgroups per run
  int tint, wpp, r;  // wpp windows per piece, r lanes per reduction group
  double scale, nd, k;
  float sk_lo, sk_hi;
};

template <bool Signed>
__device__ __forceinline__ uint32_t power_of(uint32_t v, uint32_t half) {
  if constexpr (Signed)
    return static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(v), static_cast<int>(v & half), 0, false));
  else
    return __builtin_amdgcn_udot4(v, v & half, 0u, false);
}

// The value of the lane N below in the same row of 16 lanes (0 where there is none): DPP row_shr, registers only.
template <int N>
__device__ __forceinline__ uint32_t row_shr(uint32_t v) {
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x110 + N, 0xf, 0xf, true));
}
template <int N>
__device__ __forceinline__ void row_shr_add(uint32_t& s1, u64& s2) {
  const uint32_t lo = row_shr<N>(static_cast<uint32_t>(s2)), hi = row_shr<N>(static_cast<uint32_t>(s2 >> 32));
  s1 += row_shr<N>(s1);
  s2 += (static_cast<u64>(hi) << 32) | lo;
}

// S1 > 0.  Integers below 2^53 convert exactly; each operation below is one IEEE float64 operation, in this order.
__device__ __forceinline__ float sk_value(u64 S1, u64 S2, double nd, double k) {
#pragma clang fp contract(off)
  const double s1 = static_cast<double>(S1);
  const double num = nd * static_cast<double>(S2);
  const double den = s1 * s1;
  const double ratio = num / den;
  const double excess = ratio - 1.0;
  return static_cast<float>(k * excess);
}

template <bool Signed>
__global__ __launch_bounds__(kThreads, 8) void vstats_kernel(VstatsArgs P) {  // 8 waves per SIMD: 4 workgroups per CU
  __shared__ alignas(16) uint32_t part1[2][kEntries];
  __shared__ alignas(16) u64 part2[2][kEntries];
  __shared__ uint32_t group1[2][kQuads];
  __shared__ u64 group2[2][kQuads];

  const int tid = threadIdx.x;
  const unsigned run = blockIdx.x / P.pieces, piece = blockIdx.x % P.pieces;  // run = b * A + a
  const u64 win0 = static_cast<u64>(piece) * P.wpp;                           // first window of the piece
  const u64 s0 = win0 * P.tint;                                               // first sample of the piece
  // samples of the piece: at most max(kStep * kPieceSteps, tint) <= 2^18, so positions inside it are 32-bit
  const unsigned piece_len =
      static_cast<unsigned>(P.windows - win0 < static_cast<u64>(P.wpp) ? P.windows - win0 : P.wpp) * P.tint;
  const int steps = static_cast<int>((piece_len + kStep - 1) / kStep);
  const uint8_t* src = P.raw + (static_cast<size_t>(run) * P.N + s0) * 4;

  // Lanes past the piece read its last 16 bytes instead (unconditional loads) and are never stored: a reduction group
  // lies inside one window, and the piece ends on a window boundary.
  auto load = [&](int step, u32x4 (&v)[kLoads]) {
#pragma unroll
    for (int l = 0; l < kLoads; ++l) {
      const unsigned pos = static_cast<unsigned>(step) * kStep + 4u * (l * kThreads + tid);
      v[l] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4*>(src + (pos < piece_len ? pos : piece_len - 4) * 4u));
    }
  };

  const int r4 = P.r / 4;                 // lanes per group of the quad sums (r >= 4: tint is a multiple of 16)
  const int groups = kEntries / P.r;      // group sums of one step, in sample order
  const int k = P.tint / (4 * P.r);       // groups per window
  const int pol = tid / kQuads, quad = tid % kQuads;

  u64 win1[kOwned][2] = {}, win2[kOwned][2] = {};  // this thread owns windows win0 + tid + o * kThreads
  u32x4 next[kLoads];
  load(0, next);
  for (int step = 0; step < steps; ++step) {
    u32x4 v[kLoads];
#pragma unroll
    for (int l = 0; l < kLoads; ++l) v[l] = next[l];
    if (step + 1 < steps) load(step + 1, next);

    // the lane's sums per load and pol (the previous step's entries were last read before its second barrier)
#pragma unroll
    for (int l = 0; l < kLoads; ++l)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const uint32_t half = p ? 0xffff0000u : 0x0000ffffu;
        uint32_t s1 = 0;
        u64 s2 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t pw = power_of<Signed>(v[l][j], half);
          s1 += pw;
          s2 += static_cast<u64>(pw) * pw;
        }
        part1[p][l * kThreads + tid] = s1;
        part2[p][l * kThreads + tid] = s2;
      }
    __syncthreads();

    // four consecutive entries, then the aligned group of r4 lanes (inside one wave, inside one window)
    {
      const u32x4 a = *reinterpret_cast<const u32x4*>(&part1[pol][4 * quad]);
      const u64* b = &part2[pol][4 * quad];
      uint32_t s1 = a[0] + a[1] + a[2] + a[3];
      u64 s2 = b[0] + b[1] + b[2] + b[3];
      // r4 <= 16 lanes, aligned: inside one DPP row; after shifts by 1, 2, .. r4 / 2 the group's last lane holds its sum
      if (r4 > 1) row_shr_add<1>(s1, s2);
      if (r4 > 2) row_shr_add<2>(s1, s2);
      if (r4 > 4) row_shr_add<4>(s1, s2);
      if (r4 > 8) row_shr_add<8>(s1, s2);
      if ((quad & (r4 - 1)) == r4 - 1) {
        group1[pol][quad / r4] = s1;
        group2[pol][quad / r4] = s2;
      }
    }
    __syncthreads();  // the next step's barrier after its entries keeps these sums until every owner has read them

    // window w of the piece = groups [w * k, (w + 1) * k) of the piece; this step holds [step * groups, + groups)
#pragma unroll
    for (int o = 0; o < kOwned; ++o) {
      const int w = tid + o * kThreads;
      if (w < P.wpp) {
        const int first = w * k - step * groups;  // both products count groups of the piece: at most 2^14
        const int lo = first > 0 ? first : 0;
        const int hi = first + k < groups ? first + k : groups;
        for (int g = lo; g < hi; ++g) {
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            win1[o][p] += group1[p][g];
            win2[o][p] += group2[p][g];
          }
        }
      }
    }
  }

#pragma unroll
  for (int o = 0; o < kOwned; ++o) {
    const u64 w = win0 + tid + o * kThreads;
    if (tid + o * kThreads < P.wpp && w < P.windows) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const size_t at = (static_cast<size_t>(run) * 2 + p) * P.windows + w;
        const u64 S1 = win1[o][p], S2 = win2[o][p];
        if (P.power) P.power[at] = static_cast<float>(static_cast<double>(S1) * P.scale);
        if (P.sk || P.flags) {
          const float sk = S1 == 0 ? 0.0f : sk_value(S1, S2, P.nd, P.k);
          if (P.sk) P.sk[at] = sk;
          if (P.flags) P.flags[at] = (S1 == 0 || sk < P.sk_lo || sk > P.sk_hi) ? 1 : 0;
        }
      }
    }
  }
}

}  // namespace
}  // namespace bf

extern "C" int bf_voltage_stats(const uint8_t* raw, float* out_power, float* out_sk, uint8_t* out_flags, int B, int C,
                                int T, int A, int tint, int flags, float scale, float sk_lo, float sk_hi,
                                void* stream) {
  BF_REQUIRE(raw, "bf_voltage_stats: null pointer");
  BF_REQUIRE(out_power || out_sk || out_flags, "bf_voltage_stats: null pointer, at least one output is needed");
  BF_REQUIRE(B > 0 && C > 0 && T > 0, "bf_voltage_stats: bad shape B=%d C=%d T=%d", B, C, T);
  BF_REQUIRE(T % bf::kSamplesPerBlock == 0, "bf_voltage_stats: T=%d must be a multiple of 16", T);
  BF_REQUIRE(T <= (1 << 20), "bf_voltage_stats: bad shape, T=%d above 2^20", T);
  BF_REQUIRE(tint > 0 && tint % 16 == 0 && T % tint == 0 && tint <= bf::kMaxTint,
             "bf_voltage_stats: integration %d must be a multiple of 16 that divides T=%d, at most 2^18", tint, T);
  BF_REQUIRE(A >= 1 && A <= 32768, "bf_voltage_stats: %d antennas, need 1 .. 32768", A);
  BF_REQUIRE((flags & ~BF_VSTATS_SIGNED) == 0, "bf_voltage_stats: unknown flags 0x%x", flags);
  BF_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 15) == 0 && (reinterpret_cast<uintptr_t>(out_power) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(out_sk) & 3) == 0,
             "bf_voltage_stats: misaligned buffer");
  BF_REQUIRE(std::isfinite(scale) && scale > 0.0f, "bf_voltage_stats: scale must be finite and > 0");
  if (out_flags)
    BF_REQUIRE(std::isfinite(sk_lo) && std::isfinite(sk_hi) && sk_lo >= 0.0f && sk_lo < sk_hi,
               "bf_voltage_stats: sk limits must be finite with 0 <= sk_lo < sk_hi");

  bf::VstatsArgs P;
  P.raw = raw;
  P.power = out_power;
  P.sk = out_sk;
  P.flags = out_flags;
  P.N = static_cast<unsigned long long>(C) * T;
  P.windows = P.N / tint;
  P.tint = tint;
  const int piece = bf::kStep * bf::kPieceSteps;
  P.wpp = tint >= piece ? 1 : piece / tint;  // whole windows, about kPieceSteps steps of samples
  int r = 4;  // lanes per reduction group: the largest power of two dividing tint / 4, at most one wave
  while (r < 64 && (tint / 4) % (2 * r) == 0) r *= 2;
  P.r = r;
  P.scale = static_cast<double>(scale);
  P.nd = static_cast<double>(tint);
  P.k = (P.nd + 1.0) / (P.nd - 1.0);
  P.sk_lo = sk_lo;
  P.sk_hi = sk_hi;
  const unsigned long long pieces = (P.windows + P.wpp - 1) / P.wpp;
  const unsigned long long total = pieces * B * A;
  BF_REQUIRE(total <= 0x7fffffffull, "bf_voltage_stats: bad shape, %llu workgroups exceed the grid limit", total);
  P.pieces = static_cast<unsigned>(pieces);
  hipStream_t st = bf::as_stream(stream);
  if (flags & BF_VSTATS_SIGNED)
    hipLaunchKernelGGL((bf::vstats_kernel<true>), dim3(static_cast<unsigned>(total)), dim3(bf::kThreads), 0, st, P);
  else
    hipLaunchKernelGGL((bf::vstats_kernel<false>), dim3(static_cast<unsigned>(total)), dim3(bf::kThreads), 0, st, P);
  BF_LAUNCHED("vstats_kernel");
}

extern "C" double bf_vstats_algorithmic_bytes(int B, int C, int T, int A, int tint, int outputs) {
  if (B <= 0 || C <= 0 || T <= 0 || A <= 0 || tint <= 0 || (outputs & 7) == 0) return 0.0;
  const double samples = static_cast<double>(B) * A * C * T;
  const int per_window = ((outputs & 1) ? 4 : 0) + ((outputs & 2) ? 4 : 0) + ((outputs & 4) ? 1 : 0);
  return 4.0 * samples + 2.0 * (samples / tint) * per_window;
}
