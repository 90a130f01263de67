// Folder: pulsar profiles of the detected beams, phase-binned (no reference counterpart).  Every sample of every
// channel of the beam detector's output is added into the phase bin its rotational phase falls in (include/bf.h,
// bf_fold), per fold f (a beam, a phase and a phase step), channel k and sample n = b*J + j:
//   phi = phase0[f] - chan[f][k] + n * dphase[f]            (uint64, wraps mod 2^64: one turn is 2^64)
//   bin = ((phi >> 32) * nbin) >> 32                         (integers only, always < nbin)
//   profile[f][s][k][bin] += float64(power[b][s][k][j][beam[f]]) for every Stokes plane s;  hits[f][k][bin] += 1
// A scatter with collisions, without atomics: every accumulator row (f, k) belongs to one group of lanes of one wave
// for the whole launch, two launches give identical bytes, and an element that receives no sample is never written.
//
// One kernel.  A workgroup of 4 waves owns a channel k.  The folds of a channel read the same (J, M) tiles of `power`
// (one per batch and plane), so the workgroup stages them once in LDS, plane-major, in chunks of `nc` samples where
// S * N * M floats exceed the budget (16-byte loads when J*M and the chunk's offsets are multiples of 4 floats, element
// loads otherwise), and deals the folds to its waves.  A row (f, k) belongs to a *group* of G = 16, 32 or 64
// consecutive lanes of one wave (the smallest G that is at least min(N, 64), as in bf_pulse_search.hip): group g of the
// workgroup takes the folds g, g + 256/G, ...  A *pass* gives every lane of a group one sample, consecutive lanes
// consecutive n, so that the accumulator addresses of a group are equal or (for a slow pulsar) consecutive.
//   * Collisions inside a pass, in two steps.  (1) Runs: consecutive lanes of equal bin (every pulsar slower than
//     nbin samples per turn) are summed into the run's first lane by a suffix scan over the run, log2(G) shuffle steps.
//     (2) Runs of equal (group, bin) key that are not adjacent (a bin that recurs inside the pass) are merged into the
//     first of them, in ascending lane order: the wave walks the distinct keys of its run starts (ballot, first set
//     bit, v_readlane at a uniform index); a key with a single run, the common case, costs a few scalar instructions.
//     The first lane of the first run of a key is its leader and alone reads, adds to and writes the S profile elements
//     and the hit count of that bin.  (Walking all 64 lanes per pass instead, one v_readlane per lane and plane, was
//     the first version: 2.4 to 3.5 times slower on the slow-pulsar lines, profiles/fold_ops_allpairs.jsonl.)
//   * A bin that recurs in a later pass of the same row (any period shorter than a pass: every millisecond pulsar) is
//     then updated by another lane of the same wave.  The passes of a row are ordered explicitly: a workgroup-scope
//     fence between the stores of a pass and the loads of the next, so the next pass sees them.  The same group walks
//     the row in every chunk, and the chunks are separated by barriers.
// The order of the float64 additions is therefore fixed: ((prior + pass 0's partial) + pass 1's partial) + ..., each
// partial its runs' scan trees, added in ascending n.  There is no work per bin: the cost follows the samples, not nbin.
// beam, phase0 and dphase travel by value in the kernel arguments (F <= 64) and are read at wave-uniform indices.
#include "bf_common.hpp"

namespace bf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;          // 4 waves; 256 / G rows at a time
constexpr int kMaxFolds = 64;
constexpr int kLdsFloats = 8192;       // 32 KiB: the staged chunk; one sample (S * M floats) may need up to 64 KiB

struct FoldArgs {
  const float* power;
  const unsigned long long* chan;
  double* profile;
  uint32_t* hits;
  long long JM;                        // floats of one (b, s, k) run
  int B, S, K, J, M, F, nbin, N;
  int nc;                              // samples per chunk
  int plane;                           // floats of one staged Stokes plane: nc * M rounded up to 4
  int G;                               // lanes per row
  int wide;                            // 16-byte staging
  int beam[kMaxFolds];
  unsigned long long phase0[kMaxFolds], dphase[kMaxFolds];
};

__global__ __launch_bounds__(kThreads) void fold_kernel(FoldArgs A) {
  extern __shared__ __attribute__((aligned(16))) float tile[];

  const int k = blockIdx.x;
  const int lane = threadIdx.x % 64;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int G = A.G;
  const int gl = lane % G;             // lane within the group
  const int gw = lane / G;             // group within the wave
  const int per_wave = 64 / G, per_wg = kThreads / G;
  const long long KJM = static_cast<long long>(A.K) * A.JM;

  for (int c0 = 0; c0 < A.N; c0 += A.nc) {
    const int clen = A.N - c0 < A.nc ? A.N - c0 : A.nc;
    if (c0 > 0) __syncthreads();       // the previous chunk's readers are done with the tile

    // Stage (S, clen, M): position p = n*M + m of the channel's stream lies in batch p / JM at offset p % JM.
    const long long p0 = static_cast<long long>(c0) * A.M;
    const int cfloats = clen * A.M;    // <= max(kLdsFloats, M)
    if (A.wide) {
      const int units = cfloats / 4;
      for (int s = 0; s < A.S; ++s) {
        for (int u = threadIdx.x; u < units; u += kThreads) {
          const long long p = p0 + 4ll * u;
          const long long b = p / A.JM, off = p % A.JM;
          const float* src = A.power + (b * A.S + s) * KJM + k * A.JM + off;
          *reinterpret_cast<u32x4*>(tile + s * A.plane + 4 * u) =
              __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src));
        }
      }
    } else {
      for (int s = 0; s < A.S; ++s) {
        for (int u = threadIdx.x; u < cfloats; u += kThreads) {
          const long long p = p0 + u;
          const long long b = p / A.JM, off = p % A.JM;
          tile[s * A.plane + u] = __builtin_nontemporal_load(A.power + (b * A.S + s) * KJM + k * A.JM + off);
        }
      }
    }
    __syncthreads();

    const int passes = (clen + G - 1) / G;
    for (int f0 = 0; f0 < A.F; f0 += per_wg) {
      // The fold of this lane's group: f0 + wave * per_wave + gw.  The tables are read at wave-uniform indices.
      const int fw = f0 + wave * per_wave;
      const int f = fw + gw;
      int beam = 0;
      unsigned long long base = 0, step = 0;
      for (int q = 0; q < per_wave; ++q) {
        if (fw + q < A.F && gw == q) {
          beam = A.beam[fw + q];
          base = A.phase0[fw + q];
          step = A.dphase[fw + q];
        }
      }
      const bool row = f < A.F;
      const long long fk = static_cast<long long>(row ? f : 0) * A.K + k;
      if (row) base -= A.chan[fk];
      double* prof = A.profile + (static_cast<long long>(row ? f : 0) * A.S * A.K + k) * A.nbin;
      uint32_t* hits = A.hits + fk * A.nbin;
      const long long sstride = static_cast<long long>(A.K) * A.nbin;  // one Stokes plane of a fold's profile

      for (int p = 0; p < passes; ++p) {
        const int i = p * G + gl;      // sample within the chunk
        const bool has = row && i < clen;
        int bin = 0, key = -1;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (has) {
          const unsigned long long phi = base + static_cast<unsigned long long>(c0 + i) * step;
          bin = static_cast<int>(((phi >> 32) * static_cast<unsigned long long>(A.nbin)) >> 32);
          key = gw * 4096 + bin;       // nbin <= 4096
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (s < A.S) x[s] = tile[s * A.plane + i * A.M + beam];
        }
        // Runs: consecutive lanes of equal key.  run = the index of the lane's run in the wave; a lane without a
        // sample is a run of its own and adds nothing.
        const int below = __shfl_up(key, 1);
        const bool start = has && (gl == 0 || below != key);
        const unsigned long long starts = __ballot(start);
        const int run = has ? __popcll(starts & (~0ull >> (63 - lane))) : 64 + lane;
        // A run's sums and count meet in its first lane: a suffix scan over the run, log2(G) steps.
        double acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = static_cast<double>(x[s]);
        uint32_t count = has ? 1u : 0u;
        for (int d = 1; d < G; d <<= 1) {
          const int above = __shfl_down(run, d);  // by every lane: a cross-lane read must not sit behind the `&&`
          const bool take = lane + d < 64 && above == run;
          const uint32_t c = __shfl_down(count, d);
          if (take) count += c;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (s < A.S) {
              const double v = __shfl_down(acc[s], d);
              if (take) acc[s] += v;
            }
          }
        }
        // Runs of equal key (a bin that recurs inside the pass: a period shorter than the pass) meet in the first of
        // them, in ascending lane order.  The walk is over the distinct keys of the run starts, uniform for the wave;
        // a key with one run, the common case, costs a handful of scalar instructions.
        bool leader = start;
        unsigned long long rest = starts;
        while (rest) {
          const int l = __builtin_ctzll(rest);
          const int kl = __builtin_amdgcn_readlane(key, l);
          unsigned long long m = __ballot(start && key == kl);
          rest &= ~m;
          m &= m - 1;                  // the runs of this key after the first
          if (m == 0) continue;
          if (start && key == kl && lane != l) leader = false;
          while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t c = __builtin_amdgcn_readlane(count, j);
            if (lane == l) count += c;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              if (s < A.S) {
                const double v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(acc[s]), j),
                                                  __builtin_amdgcn_readlane(__double2loint(acc[s]), j));
                if (lane == l) acc[s] += v;
              }
            }
          }
        }
        if (leader) {                  // all loads, then all stores: the compiler cannot see that the planes differ
          double old[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (s < A.S) old[s] = prof[s * sstride + bin];
          const uint32_t h = hits[bin];
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (s < A.S) prof[s * sstride + bin] = old[s] + acc[s];
          hits[bin] = h + count;
        }
        // The next pass of this row may update the same elements from other lanes of this wave: order them.  (The
        // rows of the next f0 are other elements, and the barrier orders the chunks.)
        if (p + 1 < passes) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      }
    }
  }
}

}  // namespace
}  // namespace bf

extern "C" int bf_fold(const float* power, const int32_t* beam, const uint64_t* phase0, const uint64_t* dphase,
                       const uint64_t* chan, double* profile, uint32_t* hits, int B, int S, int K, int J, int M, int F,
                       int nbin, void* stream) {
  BF_REQUIRE(power && beam && phase0 && dphase && chan && profile && hits, "bf_fold: null pointer");
  BF_REQUIRE(B > 0 && S > 0 && K > 0 && J > 0 && M > 0 && F > 0 && nbin > 0,
             "bf_fold: bad shape B=%d S=%d K=%d J=%d M=%d F=%d nbin=%d", B, S, K, J, M, F, nbin);
  BF_REQUIRE(S <= 4, "bf_fold: bad shape, S=%d above 4", S);
  BF_REQUIRE(M <= 4096, "bf_fold: bad shape, M=%d above 4096", M);
  BF_REQUIRE(F <= bf::kMaxFolds, "bf_fold: bad shape, F=%d above 64", F);
  BF_REQUIRE(nbin <= 4096, "bf_fold: bad shape, nbin=%d above 4096", nbin);
  const long long N = static_cast<long long>(B) * J;
  BF_REQUIRE(N <= 2147483647ll, "bf_fold: bad shape, N = B*J = %lld above 2^31 - 1", N);
  for (int f = 0; f < F; ++f)
    BF_REQUIRE(beam[f] >= 0 && beam[f] < M, "bf_fold: beam[%d] = %d outside [0, %d)", f, beam[f], M);
  BF_REQUIRE((reinterpret_cast<uintptr_t>(power) & 15) == 0 && (reinterpret_cast<uintptr_t>(chan) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(profile) & 7) == 0 && (reinterpret_cast<uintptr_t>(hits) & 3) == 0,
             "bf_fold: misaligned buffer");

  bf::FoldArgs A = {};
  A.power = power;
  A.chan = reinterpret_cast<const unsigned long long*>(chan);
  A.profile = profile;
  A.hits = hits;
  A.JM = static_cast<long long>(J) * M;
  A.B = B;
  A.S = S;
  A.K = K;
  A.J = J;
  A.M = M;
  A.F = F;
  A.nbin = nbin;
  A.N = static_cast<int>(N);
  for (int f = 0; f < bf::kMaxFolds; ++f) {
    A.beam[f] = f < F ? beam[f] : 0;
    A.phase0[f] = f < F ? phase0[f] : 0;
    A.dphase[f] = f < F ? dphase[f] : 0;
  }
  A.G = N <= 16 ? 16 : (N <= 32 ? 32 : 64);
  // The chunk: as many samples as the budget holds, whole passes of 64 where it holds that many, one at the least.
  long long nc = bf::kLdsFloats / (static_cast<long long>(S) * M);
  if (nc >= 64) nc -= nc % 64;
  if (nc < 1) nc = 1;
  if (nc > N) nc = N;
  A.nc = static_cast<int>(nc);
  // 16-byte staging: every run of the block and every chunk then starts on 4 floats, in memory and in the tile.
  A.wide = A.JM % 4 == 0 && (nc == N || nc * M % 4 == 0);
  A.plane = static_cast<int>((nc * M + 3) / 4 * 4);
  const size_t lds = static_cast<size_t>(S) * A.plane * sizeof(float);  // <= 64 KiB: S * M <= 16384

  hipLaunchKernelGGL(bf::fold_kernel, dim3(static_cast<unsigned>(K)), dim3(bf::kThreads), lds, bf::as_stream(stream),
                     A);
  BF_LAUNCHED_TAG("fold_kernel", "g%d,c%d,%s", A.G, A.nc, A.wide ? "wide" : "element");
}

extern "C" double bf_fold_algorithmic_bytes(int B, int S, int K, int J, int M, int F, long long touched) {
  if (B <= 0 || S <= 0 || K <= 0 || J <= 0 || M <= 0 || F <= 0 || S > 4 || M > 4096 || F > bf::kMaxFolds ||
      static_cast<long long>(B) * J > 2147483647ll || touched < 0)
    return 0.0;
  return 4.0 * B * S * K * J * M + 8.0 * F * K + static_cast<double>(touched) * (16.0 * S + 8.0);
}
