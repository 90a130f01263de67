// Beam streams: the beams as per-beam voltage streams, any subset (no reference counterpart: the reference reorders
// before the contraction, prebeamform_reorder.py, and has nothing after it).  From the fused operator's output
//   beams[b][p][c][t/16][t%16][2m + z]     f32, or int8 (BF_BSTREAM_IN_INT8)
// to one antenna-shaped stream per selected beam,
//   out[b][k][c][t][p][z] = beams[b][p][c][t/16][t%16][2 beam_index[k] + z]      (0 where the index is outside [0, M))
// a copy of bits (f32 in, int8 out with BF_BSTREAM_REQUANT: bf_requant's formula).  DESIGN §3e.
//
// Channel and time flatten on both sides: with n = c * T + t and N = C * T the input is in[b][p][n][m] and the output
// out[b][k][n][p], complex elements of E = 2 (int8) or 8 (f32) bytes, so the kernel never sees C or T.  A workgroup
// owns a tile of nt <= NT samples by mt <= MT beams of one batch:
//   1. load: the tile's rows of both pol planes, as the aligned 16-byte chunks that cover them, non-temporal, the two
//      planes at the same offset.  When the tile spans all beams (M <= 64) its rows are one contiguous run of
//      nt * M * E bytes (16-byte aligned: 16 | NT), so a wave-load is 1 KiB contiguous; wider M is cut into column
//      tiles whose rows are mt * E bytes, M * E apart and at any 2- or 8-byte alignment: a chunk may begin before the
//      row or end past it, inside the plane (a plane is a multiple of 16 bytes at a 16-byte boundary), and elements
//      outside the row are dropped, not stored;
//   2. every element goes to LDS as the output's unit [Xre, Xim, Yre, Yim] of one (beam, sample) -- one dword for int8
//      (v_perm_b32 of the two pols' dwords), 16 bytes for f32 -- at [beam][sample], the transpose: a beam's samples
//      are consecutive, the column pitch NT + 4 dwords (int8: columns stay 16-byte aligned) or NT + 1 units (f32);
//   3. store: each lane reads 16 consecutive bytes of one beam's column (ds_read_b128) and stores them, non-temporal,
//      the lanes of a wave along the samples of one stream: 4 * nt contiguous bytes per stream for int8 (256 B at
//      64 beams, NT = 64; 512 B at 16 beams; 1 KiB per wave-store from NT = 256), 16 * nt for f32 (512 B at 64 beams,
//      NT = 32; 1 KiB at 16 beams).  The requantising form reads four units per lane and stores their 16 int8.
// The tile (plan(), below) is about 2048 (int8) or 1024 (f32) elements and its order over the XCDs depends on the run
// length; both were measured.
// Plain LDS, not the transposed read (ds_read_b64_tr_b16): that instruction transposes 4 x 16 blocks of 16-bit elements
// of ONE image, but here the two pols must interleave as well, the row length M is arbitrary (odd, 1, 4096), and the
// gather needs EXEC all ones, which the ragged tiles cannot give.  Transposing on the LDS write costs 8 ds_write_b32
// per 32 loaded bytes, far below what the HBM stream needs, and leaves the reads conflict-free.
// With a list the loop of step 3 runs over k in [0, K): stream k takes column beam_index[k] when it lies in the
// tile (unsigned compare), the first column tile writes zeros for an index outside [0, M).  Every output element is
// written once by one thread; the input is never written.
#include <cmath>

#include "bf_common.hpp"

namespace bf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kBatch = 4;          // chunks per pol a thread has in flight
constexpr unsigned kMaxMT = 64;    // beams per tile
constexpr unsigned kMaxNT = 1024;  // samples per tile
enum Form { kI8 = 0, kF32 = 1, kF32Q = 2 };

struct BstreamArgs {
  const uint8_t* beams;
  const int32_t* index;  // nullptr: the identity
  uint8_t* out;
  u64 N;                 // C * T
  unsigned M, K;
  unsigned Minv;         // ceil(2^32 / M), M > 1: e / M = umulhi(e, Minv) for e < 2^16
  unsigned MT, NT, NTP;  // tile: beams, samples, LDS column pitch in units
  unsigned nmt, nnt;     // tiles across the beams, along the samples
  unsigned xcd;          // XCD-range order of the tiles
  float scale;
};

__device__ __forceinline__ uint32_t requant1(float v, float scale) {  // bf_requant's formula
  float r = __builtin_rintf(v * scale);
  r = fminf(fmaxf(r, -127.0f), 127.0f);
  return static_cast<uint32_t>(static_cast<int>(r)) & 0xffu;
}
__device__ __forceinline__ uint32_t requant_unit(u32x4 u, float scale) {
  const uint32_t xr = u[0], xi = u[1], yr = u[2], yi = u[3];  // (a bit_cast of u[i] itself reads element 0 four times)
  return requant1(__uint_as_float(xr), scale) | requant1(__uint_as_float(xi), scale) << 8 |
         requant1(__uint_as_float(yr), scale) << 16 | requant1(__uint_as_float(yi), scale) << 24;
}

template <int F>
__global__ __launch_bounds__(kThreads) void beam_streams_kernel(BstreamArgs P) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr unsigned E = F == kI8 ? 2 : 8;    // bytes of one complex input element
  constexpr unsigned UD = F == kI8 ? 1 : 4;   // dwords of one LDS unit
  constexpr unsigned EPC = 16 / E;            // elements per chunk
  const unsigned tid = threadIdx.x;
  const unsigned bid = P.xcd ? (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const unsigned mtile = bid % P.nmt;
  const unsigned ntile = (bid / P.nmt) % P.nnt;
  const unsigned b = bid / P.nmt / P.nnt;
  const unsigned m0 = mtile * P.MT;
  const unsigned mt = min(P.MT, P.M - m0);
  const u64 n0 = static_cast<u64>(ntile) * P.NT;
  const unsigned nt = static_cast<unsigned>(min(static_cast<u64>(P.NT), P.N - n0));  // a multiple of 16

  // The store phase's share of this thread, and the list entry of its first stream: loaded here, beside the tile's
  // loads, not after the barrier where a workgroup would wait for it alone.
  constexpr unsigned SPL = F == kF32 ? 1 : 4;  // samples per lane
  const unsigned per = nt / SPL;               // lanes per stream
  const unsigned streams = P.index ? P.K : mt;
  const unsigned work = streams * per;
  unsigned m_first = 0;
  if (P.index && tid < work) m_first = static_cast<unsigned>(P.index[tid / per]);

  // 1. rows -> registers -> LDS.  All beams in the tile: one row, the whole contiguous run.
  {
    const bool flat = mt == P.M;
    const unsigned R = flat ? 1 : nt;
    const unsigned Lel = flat ? nt * P.M : mt;    // elements per row (a few thousand: far below 2^16, Minv)
    const unsigned CPR = (Lel * E + 15) / 16 + 1;  // chunks that can touch a row at any alignment
    const unsigned items = R * CPR;
    const u64 plane = P.N * P.M * E;
    const uint8_t* src = P.beams + static_cast<u64>(b) * 2 * plane;
    const u64 S0 = (n0 * P.M + m0) * E;  // the tile's first row in its plane
    for (unsigned base = 0; base < items; base += kBatch * kThreads) {
      u32x4 x0[kBatch], x1[kBatch];
      unsigned row[kBatch];
      int first[kBatch];  // the chunk's first element, relative to its row's first (negative: before the row)
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        const unsigned it = base + k * kThreads + tid;
        const unsigned r = flat ? 0 : it / CPR, c = it - r * CPR;
        const u64 S = S0 + static_cast<u64>(r) * P.M * E;
        const unsigned lead = static_cast<unsigned>(S) & 15u;
        const int d = static_cast<int>(16 * c) - static_cast<int>(lead);  // chunk's byte offset from the row's start
        row[k] = r;
        first[k] = d / static_cast<int>(E);  // exact: lead is a multiple of E
        x0[k] = x1[k] = u32x4{0, 0, 0, 0};
        if (it < items && d < static_cast<int>(Lel * E)) {  // lanes past the tile's rows load nothing
          const uint8_t* at = src + (S - lead) + 16 * static_cast<u64>(c);
          x0[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(at));
          x1[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(at + plane));
        } else {
          first[k] = static_cast<int>(Lel);  // no element of this chunk is in range
        }
      }
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        const int e0 = first[k];
        // samples down from the row (flat rows only): e0 / M as a multiply, exact for e0 < 2^16 (Minv, M <= 2^12)
        unsigned q = e0 <= 0 ? 0 : P.M == 1 ? static_cast<unsigned>(e0) : __umulhi(static_cast<unsigned>(e0), P.Minv);
        int rem = e0 - static_cast<int>(q * P.M);                   // beam within the tile
#pragma unroll
        for (unsigned j = 0; j < EPC; ++j) {
          if (static_cast<unsigned>(e0 + static_cast<int>(j)) < Lel) {
            const unsigned unit = static_cast<unsigned>(rem) * P.NTP + row[k] + q;
            if constexpr (F == kI8) {
              lds[unit] = __builtin_amdgcn_perm(x1[k][j / 2], x0[k][j / 2], (j & 1) ? 0x07060302u : 0x05040100u);
            } else {
              *reinterpret_cast<u32x4*>(lds + unit * UD) =
                  u32x4{x0[k][2 * j], x0[k][2 * j + 1], x1[k][2 * j], x1[k][2 * j + 1]};
            }
          }
          if (++rem == static_cast<int>(P.M)) {
            rem = 0;
            ++q;
          }
        }
      }
    }
  }
  __syncthreads();

  // 2. LDS columns -> streams, 16 bytes per lane, lanes along the samples of one stream.
  for (unsigned it = tid; it < work; it += kThreads) {
    const unsigned kk = it / per, n = (it - kk * per) * SPL;
    unsigned k = m0 + kk, col = kk;
    bool zero = false;
    if (P.index) {
      const unsigned m = it == tid ? m_first : static_cast<unsigned>(P.index[kk]);
      k = kk;
      col = m - m0;
      zero = m >= P.M;
      if (zero ? mtile != 0 : col >= mt) continue;  // another tile's beam; zero streams belong to the first tile
    }
    u32x4 v = {0, 0, 0, 0};
    if (!zero) {
      const uint32_t* at = lds + (col * P.NTP + n) * UD;
      if constexpr (F == kF32Q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = requant_unit(*reinterpret_cast<const u32x4*>(at + 4 * j), P.scale);
      } else {
        v = *reinterpret_cast<const u32x4*>(at);
      }
    }
    const u64 sample = (static_cast<u64>(b) * P.K + k) * P.N + n0 + n;
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(P.out + sample * (F == kF32 ? 16 : 4)));
  }
}

// The launch of a shape, or what is wrong with it (nullptr when valid): the one place both entry points ask.
const char* plan(int B, int C, int T, int M, int K, int flags, BstreamArgs& P, u64& grid, size_t& lds_bytes) {
  if (B <= 0 || C <= 0 || T <= 0 || M <= 0 || K <= 0) return "bad shape";
  if (T % kSamplesPerBlock != 0) return "T must be a multiple of 16";
  if (T > (1 << 20)) return "bad shape, T above 2^20";
  if (M > 4096 || K > 4096) return "bad shape, M and K are at most 4096";
  if (flags & ~(BF_BSTREAM_IN_INT8 | BF_BSTREAM_REQUANT | BF_BSTREAM_LIST)) return "unknown flags";
  if ((flags & BF_BSTREAM_REQUANT) && (flags & BF_BSTREAM_IN_INT8))
    return "BF_BSTREAM_REQUANT needs f32 beams, not BF_BSTREAM_IN_INT8";
  const bool i8 = flags & BF_BSTREAM_IN_INT8;
  P.N = static_cast<u64>(C) * T;
  P.M = M;
  P.K = K;
  P.Minv = M == 1 ? 0u : static_cast<unsigned>(((1ull << 32) + M - 1) / M);
  P.nmt = (M + kMaxMT - 1) / kMaxMT;
  P.MT = (M + P.nmt - 1) / P.nmt;
  P.nmt = (M + P.MT - 1) / P.MT;
  // Samples per tile, measured at cfg3 and cfg4: about 2048 (int8) or 1024 (f32) elements, 8 or 16 KiB of
  // streams, but never runs below 256 B (int8: 64 samples) or 512 B (f32: 32); twice the elements for a list of at
  // most M / 2 beams, whose workgroups write little (cfg3 int8, one beam: 141 -> 93 us); at most 34 KiB of LDS
  const unsigned big = (flags & BF_BSTREAM_LIST) && 2 * K <= M ? 2 : 1;
  unsigned NT = (big * (i8 ? 2048u : 1024u) / P.MT + 15) / 16 * 16;
  if (NT < (i8 ? 64u : 32u)) NT = i8 ? 64u : 32u;
  if (NT > kMaxNT) NT = kMaxNT;
  if (NT > P.N) NT = static_cast<unsigned>(P.N);
  P.NT = NT;
  P.NTP = i8 ? NT + 4 : NT + 1;
  const u64 nnt = (P.N + NT - 1) / NT;
  grid = nnt * P.nmt * B;
  if (grid > 0x7fffffffull) return "bad shape, the workgroups exceed the grid limit of 2^31 - 1";
  P.nnt = static_cast<unsigned>(nnt);
  // Tiles with stream runs of 1 KiB or more go to the XCDs in ranges (XCD x takes tiles [x grid/8, (x+1) grid/8), as
  // bf_reorder): cfg3 f32 910 -> 721 us; shorter runs were 3-4 % faster in plain order (cfg4)
  P.xcd = grid % 8 == 0 && NT * ((flags & (BF_BSTREAM_IN_INT8 | BF_BSTREAM_REQUANT)) ? 4u : 16u) >= 1024u;
  lds_bytes = static_cast<size_t>(P.MT) * P.NTP * (i8 ? 4 : 16);
  return nullptr;
}

}  // namespace
}  // namespace bf

extern "C" int bf_beam_streams(const void* beams, const int32_t* beam_index, void* out, int B, int C, int T, int M,
                               int K, int flags, float scale, void* stream) {
  BF_REQUIRE(beams && out, "bf_beam_streams: null pointer");
  bf::BstreamArgs P;
  bf::u64 grid = 0;
  size_t lds_bytes = 0;
  const char* why = bf::plan(B, C, T, M, K, flags | (beam_index ? BF_BSTREAM_LIST : 0), P, grid, lds_bytes);
  BF_REQUIRE(!why, "bf_beam_streams: %s (B=%d C=%d T=%d M=%d K=%d flags=0x%x)", why, B, C, T, M, K, flags);
  BF_REQUIRE(beam_index || K == M, "bf_beam_streams: no beam list (the identity) needs K=%d equal to M=%d", K, M);
  BF_REQUIRE(beam_index || !(flags & BF_BSTREAM_LIST), "bf_beam_streams: BF_BSTREAM_LIST without a beam list");
  BF_REQUIRE((reinterpret_cast<uintptr_t>(beams) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(beam_index) & 3) == 0,
             "bf_beam_streams: misaligned buffer");
  if (flags & BF_BSTREAM_REQUANT)
    BF_REQUIRE(std::isfinite(scale) && scale > 0.0f, "bf_beam_streams: scale must be finite and > 0");
  P.beams = static_cast<const uint8_t*>(beams);
  P.index = beam_index;
  P.out = static_cast<uint8_t*>(out);
  P.scale = scale;
  const dim3 g(static_cast<unsigned>(grid)), t(bf::kThreads);
  hipStream_t st = bf::as_stream(stream);
  const char* form;
  if (flags & BF_BSTREAM_IN_INT8) {
    form = "i8";
    hipLaunchKernelGGL((bf::beam_streams_kernel<bf::kI8>), g, t, lds_bytes, st, P);
  } else if (flags & BF_BSTREAM_REQUANT) {
    form = "f32q";
    hipLaunchKernelGGL((bf::beam_streams_kernel<bf::kF32Q>), g, t, lds_bytes, st, P);
  } else {
    form = "f32";
    hipLaunchKernelGGL((bf::beam_streams_kernel<bf::kF32>), g, t, lds_bytes, st, P);
  }
  BF_LAUNCHED_TAG("beam_streams_kernel", "%s%s", form, beam_index ? ",list" : "");
}

extern "C" double bf_beam_streams_algorithmic_bytes(int B, int C, int T, int M, int K, int flags) {
  bf::BstreamArgs P;
  bf::u64 grid = 0;
  size_t lds_bytes = 0;
  if (bf::plan(B, C, T, M, K, flags, P, grid, lds_bytes)) return 0.0;
  const bool list = flags & BF_BSTREAM_LIST;
  if (!list && K != M) return 0.0;
  const double es_in = (flags & BF_BSTREAM_IN_INT8) ? 1.0 : 4.0;
  const double es_out = (flags & (BF_BSTREAM_IN_INT8 | BF_BSTREAM_REQUANT)) ? 1.0 : 4.0;
  const double n = static_cast<double>(B) * C * T;
  return es_in * n * 2.0 * 2.0 * M + es_out * n * K * 4.0 + (list ? 4.0 * K : 0.0);
}
