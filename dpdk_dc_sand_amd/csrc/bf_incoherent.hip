// Incoherent beam: antenna power sums of the raw voltages (no reference counterpart; the second standard product of a
// B-engine next to the tied-array beams).  For the fused operator's input cube x[b][a][c][t][p][z] (8-bit, z = re, im):
//   S[b][p][c][j]   = sum over unmasked antennas a, sum over t in [j*tint, (j+1)*tint) of re^2 + im^2   (exact integer)
//   out[b][p][c][j] = float32(float64(S) * float64(scale))                    (one multiply, one RNE conversion)
// A pure HBM read stream.  For fixed (b, a) the (c, t) plane is one run of C*T dwords (one dword = one time sample:
// pol0 re, im, pol1 re, im) and tint divides T, so channel and time flatten into one axis cut into windows of tint.
//
// A workgroup (512 threads) owns a piece of whole windows of that axis (4096 samples when tint divides 4096), for one
// batch, and walks it in steps of 4096 samples = 16 KiB contiguous per antenna: two 16-byte loads per lane, 8 KiB
// apart, 1 KiB contiguous per wave-load, the non-temporal loads of the item kernels of bf_fused.hip.  (Measured,
// tools/probes/incoherent_read_path.hip: the contiguous run per workgroup and antenna is what sets the rate of this
// antenna-strided stream; 4 KiB runs reach 0.75 of the plain read stream, 16 KiB runs 0.95.)  Per step:
//   1. antenna walk (stride C*T*4 bytes), 4 antennas x 2 loads in flight per lane; the per-pol power of a sample is
//      the int8 dot product of its dword with itself masked to one half (v_dot4), accumulated per sample in 32 bits:
//      A * 2 * 255^2 < 2^32 for A <= 32768.  The sum-pols form takes the unmasked dot product (both pols at once) and
//      is flushed into 64 bits every 8192 antennas (8192 * 4 * 255^2 < 2^32);
//   2. time integration inside the lane (the 4 samples of a load, 64-bit), then across the aligned lane group that
//      lies inside one window (r = the largest power of two dividing tint / 4, at most a wave), then through LDS: the
//      thread that owns a window adds the group sums of its window and carries them over the steps in registers.
// Every output element is written once by one thread: no atomics, no zeroed output, deterministic.  The antenna mask
// is read once per workgroup (per 8192-antenna chunk) and compacted into a list of antennas in LDS: a masked
// antenna's loads are never issued.
#include <cmath>

#include "bf_common.hpp"

namespace bf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;
constexpr int kLoads = 2;                     // 16-byte loads per lane, antenna and step, kThreads * 16 bytes apart
constexpr int kStep = 4 * kThreads * kLoads;  // samples per workgroup step
constexpr int kAntChunk = 8192;               // antennas per list / per 32-bit run of the sum-pols form
constexpr int kUnroll = 4;                    // antennas in flight per lane (kUnroll * kLoads loads)
constexpr int kOwned = 2;                     // windows a thread may own: tint = 4 has 2 * kThreads windows per piece

struct IncohArgs {
  const uint8_t* raw;
  const uint8_t* mask;
  float* out;
  unsigned long long N;        // C * T: samples of one (b, a) run
  unsigned long long windows;  // N / tint: output windows per batch and pol
  unsigned pieces;             // workgroups per batch
  int A, tint, wpp, steps, r;  // wpp windows per piece, `steps` steps per piece, r lanes per reduction group
  double scale;
};

template <bool Signed>
__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) {
  if constexpr (Signed)
    return static_cast<uint32_t>(
        __builtin_amdgcn_sdot4(static_cast<int>(a), static_cast<int>(b), static_cast<int>(c), false));
  else
    return __builtin_amdgcn_udot4(a, b, c, false);
}

template <bool Signed, bool SumPols>
__device__ __forceinline__ void detect(const u32x4 v, uint32_t (&acc)[4][SumPols ? 1 : 2]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (SumPols) {
      acc[j][0] = dot4<Signed>(v[j], v[j], acc[j][0]);
    } else {
      acc[j][0] = dot4<Signed>(v[j], v[j] & 0x0000ffffu, acc[j][0]);
      acc[j][1] = dot4<Signed>(v[j], v[j] & 0xffff0000u, acc[j][1]);
    }
  }
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), m, 64);
  const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), m, 64);
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

__device__ __forceinline__ float scaled(unsigned long long s, double scale) {
  return static_cast<float>(static_cast<double>(s) * scale);  // S < 2^53: exact, then one RNE conversion
}

template <bool Signed, bool SumPols, bool Masked>
__global__ __launch_bounds__(kThreads) void incoherent_kernel(IncohArgs P) {
  constexpr int NP = SumPols ? 1 : 2;
  __shared__ unsigned long long group_sum[NP][kLoads * kThreads];
  __shared__ uint16_t ant_list[Masked ? kAntChunk : 1];
  __shared__ int ant_count;

  const int tid = threadIdx.x;
  const unsigned b = blockIdx.x / P.pieces, piece = blockIdx.x % P.pieces;
  const unsigned long long win0 = static_cast<unsigned long long>(piece) * P.wpp;  // first window of the piece
  const unsigned long long s0 = win0 * P.tint;                                     // first sample of the piece
  const unsigned long long piece_len =
      (P.windows - win0 < static_cast<unsigned long long>(P.wpp) ? P.windows - win0 : P.wpp) * P.tint;
  const size_t ant_stride = static_cast<size_t>(P.N) * 4;
  const uint8_t* batch = P.raw + static_cast<size_t>(b) * P.A * ant_stride;
  float* out = P.out + static_cast<size_t>(b) * NP * P.windows;
  const int n_chunks = (P.A + kAntChunk - 1) / kAntChunk;

  unsigned long long win_sum[kOwned][NP] = {};  // tint >= 4: this thread owns windows win0 + tid + o * kThreads
  for (int step = 0; step < P.steps; ++step) {
    // Lanes past the piece read its last 16 bytes instead (unconditional loads) and are never stored: a reduction
    // group lies inside one window, and the piece ends on a window boundary.
    unsigned long long pos[kLoads];
    bool live[kLoads];
    const uint8_t* src[kLoads];
#pragma unroll
    for (int l = 0; l < kLoads; ++l) {
      pos[l] = static_cast<unsigned long long>(step) * kStep + 4u * (l * kThreads + tid);
      live[l] = pos[l] < piece_len;
      src[l] = batch + (s0 + (live[l] ? pos[l] : piece_len - 4)) * 4;
    }

    // per-sample antenna sums: 32 bits hold one pol of every antenna; both pols at once are flushed per chunk
    uint32_t acc[kLoads][4][NP] = {};
    unsigned long long tot[SumPols ? kLoads : 1][4] = {};
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
      const int a0 = chunk * kAntChunk;
      int n = P.A - a0 < kAntChunk ? P.A - a0 : kAntChunk;
      if constexpr (Masked) {
        if (n_chunks > 1 || step == 0) {  // the list of unmasked antennas of this chunk (any order: integer sums)
          __syncthreads();
          if (tid == 0) ant_count = 0;
          __syncthreads();
          for (int i = tid; i < n; i += kThreads)
            if (P.mask[a0 + i]) ant_list[atomicAdd(&ant_count, 1)] = static_cast<uint16_t>(i);
          __syncthreads();
        }
        n = ant_count;
      }
      auto offset = [&](int i) -> size_t {
        int a = i;
        if constexpr (Masked) a = __builtin_amdgcn_readfirstlane(static_cast<int>(ant_list[i]));
        return static_cast<size_t>(a0 + a) * ant_stride;
      };
      int i = 0;
      for (; i + kUnroll <= n; i += kUnroll) {
        u32x4 v[kUnroll][kLoads];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const size_t off = offset(i + u);
#pragma unroll
          for (int l = 0; l < kLoads; ++l)
            v[u][l] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src[l] + off));
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
#pragma unroll
          for (int l = 0; l < kLoads; ++l) detect<Signed, SumPols>(v[u][l], acc[l]);
      }
      for (; i < n; ++i) {
        const size_t off = offset(i);
        u32x4 v[kLoads];
#pragma unroll
        for (int l = 0; l < kLoads; ++l) v[l] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src[l] + off));
#pragma unroll
        for (int l = 0; l < kLoads; ++l) detect<Signed, SumPols>(v[l], acc[l]);
      }
      if constexpr (SumPols) {
#pragma unroll
        for (int l = 0; l < kLoads; ++l)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            tot[l][j] += acc[l][j][0];
            acc[l][j][0] = 0;
          }
      }
    }
    auto sample = [&](int l, int j, int p) -> unsigned long long {
      if constexpr (SumPols) return tot[l][j];
      return acc[l][j][p];
    };

    if (P.tint < 4) {  // 4 or 2 windows per load: no cross-lane sum
#pragma unroll
      for (int l = 0; l < kLoads; ++l) {
        if (!live[l]) continue;
        const unsigned long long w = (s0 + pos[l]) / P.tint;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          float* o = out + p * P.windows + w;
          if (P.tint == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = scaled(sample(l, j, p), P.scale);
          } else {
            o[0] = scaled(sample(l, 0, p) + sample(l, 1, p), P.scale);
            o[1] = scaled(sample(l, 2, p) + sample(l, 3, p), P.scale);
          }
        }
      }
      continue;
    }

    // the 4 samples of each load, then the aligned group of r lanes (inside one wave, inside one window)
    const int per_load = kThreads / P.r, groups = kLoads * per_load;  // group sums of this step, in sample order
    if (step > 0) __syncthreads();                                    // the previous step's sums have been consumed
#pragma unroll
    for (int l = 0; l < kLoads; ++l)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        unsigned long long s = sample(l, 0, p) + sample(l, 1, p) + sample(l, 2, p) + sample(l, 3, p);
        for (int m = 1; m < P.r; m <<= 1) s += shfl_xor_u64(s, m);
        if ((tid & (P.r - 1)) == 0) group_sum[p][l * per_load + tid / P.r] = s;
      }
    __syncthreads();
    // window w of the piece = groups [w * k, (w + 1) * k) of the piece; this step holds [step * groups, + groups)
    const int k = P.tint / (4 * P.r);
#pragma unroll
    for (int o = 0; o < kOwned; ++o) {
      const int w = tid + o * kThreads;
      if (w < P.wpp) {
        const long long first = static_cast<long long>(w) * k - static_cast<long long>(step) * groups;
        const int lo = first > 0 ? static_cast<int>(first) : 0;
        const int hi = first + k < groups ? static_cast<int>(first + k) : groups;
        for (int g = lo; g < hi; ++g) {
#pragma unroll
          for (int p = 0; p < NP; ++p) win_sum[o][p] += group_sum[p][g];
        }
      }
    }
  }

  if (P.tint >= 4) {
#pragma unroll
    for (int o = 0; o < kOwned; ++o) {
      const unsigned long long w = win0 + tid + o * kThreads;
      if (tid + o * kThreads < P.wpp && w < P.windows) {
#pragma unroll
        for (int p = 0; p < NP; ++p) out[p * P.windows + w] = scaled(win_sum[o][p], P.scale);
      }
    }
  }
}

template <bool Signed, bool SumPols>
void launch(const IncohArgs& P, unsigned grid, hipStream_t st) {
  if (P.mask)
    hipLaunchKernelGGL((incoherent_kernel<Signed, SumPols, true>), dim3(grid), dim3(kThreads), 0, st, P);
  else
    hipLaunchKernelGGL((incoherent_kernel<Signed, SumPols, false>), dim3(grid), dim3(kThreads), 0, st, P);
}

}  // namespace
}  // namespace bf

extern "C" int bf_incoherent_beam(const uint8_t* raw, const uint8_t* ant_mask, float* out, int B, int C, int T, int A,
                                  int tint, int flags, float scale, void* stream) {
  BF_REQUIRE(raw && out, "bf_incoherent_beam: null pointer");
  BF_REQUIRE(B > 0 && C > 0 && T > 0, "bf_incoherent_beam: bad shape B=%d C=%d T=%d", B, C, T);
  BF_REQUIRE(T % bf::kSamplesPerBlock == 0, "bf_incoherent_beam: T=%d must be a multiple of 16", T);
  BF_REQUIRE(T <= (1 << 20), "bf_incoherent_beam: bad shape, T=%d above 2^20", T);
  BF_REQUIRE(tint > 0 && T % tint == 0 && (tint % 16 == 0 || (tint < 16 && (tint & (tint - 1)) == 0)),
             "bf_incoherent_beam: integration %d must divide T=%d and be a power of two <= 16 or a multiple of 16",
             tint, T);
  BF_REQUIRE(A >= 1 && A <= 32768, "bf_incoherent_beam: %d antennas, need 1 .. 32768", A);
  BF_REQUIRE((flags & ~(BF_INCOH_SIGNED | BF_INCOH_SUM_POLS)) == 0, "bf_incoherent_beam: unknown flags 0x%x", flags);
  BF_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
             "bf_incoherent_beam: misaligned buffer");
  BF_REQUIRE(std::isfinite(scale) && scale > 0.0f, "bf_incoherent_beam: scale must be finite and > 0");

  bf::IncohArgs P;
  P.raw = raw;
  P.mask = ant_mask;
  P.out = out;
  P.N = static_cast<unsigned long long>(C) * T;
  P.windows = P.N / tint;
  P.A = A;
  P.tint = tint;
  P.wpp = tint >= bf::kStep ? 1 : bf::kStep / tint;  // whole windows, about one step of samples
  P.steps = static_cast<int>((static_cast<long long>(P.wpp) * tint + bf::kStep - 1) / bf::kStep);
  int r = 1;  // lanes per reduction group: the largest power of two dividing tint / 4, at most one wave
  while (tint >= 4 && r < 64 && (tint / 4) % (2 * r) == 0) r *= 2;
  P.r = r;
  P.scale = static_cast<double>(scale);
  const unsigned long long pieces = (P.windows + P.wpp - 1) / P.wpp;
  BF_REQUIRE(pieces * B <= 0x7fffffffull, "bf_incoherent_beam: bad shape, %llu workgroups exceed the grid limit",
             pieces * B);
  P.pieces = static_cast<unsigned>(pieces);
  const unsigned grid = static_cast<unsigned>(pieces * B);
  hipStream_t st = bf::as_stream(stream);
  switch (flags) {
    case 0: bf::launch<false, false>(P, grid, st); break;
    case BF_INCOH_SIGNED: bf::launch<true, false>(P, grid, st); break;
    case BF_INCOH_SUM_POLS: bf::launch<false, true>(P, grid, st); break;
    default: bf::launch<true, true>(P, grid, st); break;
  }
  BF_LAUNCHED("incoherent_kernel");
}

extern "C" double bf_incoherent_algorithmic_bytes(int B, int C, int T, int A, int tint, int flags, int masked) {
  if (B <= 0 || C <= 0 || T <= 0 || A <= 0 || tint <= 0) return 0.0;
  const double samples = static_cast<double>(B) * C * T;
  return 4.0 * samples * A + (masked ? A : 0) + 4.0 * ((flags & BF_INCOH_SUM_POLS) ? 1 : 2) * (samples / tint);
}
