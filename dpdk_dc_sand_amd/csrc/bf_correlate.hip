// The correlator: integer visibilities of the raw voltages (no reference counterpart; the X-engine half of the engine
// this project imitates).  For the fused operator's input cube x[b][a][c][t][p][z] (8-bit, z = re, im), the window
// b in [k*bint, (k+1)*bint), t in [j*tint, (j+1)*tint) and the baseline bl(a1, a2) = a1 (a1 + 1) / 2 + a2, a1 >= a2:
//   S[k][c][j][bl][p1][p2] = sum over the window of x[a1,p1] * conj(x[a2,p2])
//      re = sum r1*r2 + i1*i2        im = sum i1*r2 - r1*i2                      (exact integers, int32)
// out is int32 (B/bint, C, T/tint, NBL, 2, 2, 2): one baseline is 8 consecutive words (p1, p2, (re, im)).
//
// A Hermitian rank-n update per (window, channel) on v_mfma_i32_16x16x64_i8 (mfma_i8, bf_fused.hpp: lane l holds
// A[row l & 15][k-slot (l >> 4, byte j)], B[k-slot (l >> 4, j)][col l & 15] and D[rows 4 (l >> 4) ..+3][col l & 15]).
//   * An operand row is one antenna of one pol, a tile is 16 antennas, and the K axis is time: 64 bytes = 32 samples
//     x (re, im).  For fixed (b, a, c) the T samples are 4T contiguous bytes, one dword [p0re, p0im, p1re, p1im] per
//     sample, so lane (row, h) of a fragment is the 32 bytes of samples 8h .. 8h+7 of the step, and one v_perm per
//     dword pair and pol gives its 16 K-bytes of pol 0 and of pol 1.  Both operands are cut the same way, so any
//     assignment of window samples to K slots is as good as any other: the window's 8-sample slices are dealt in
//     order, slice s = 4 step + h, over the batches of the window (slice s lies in batch s / (tint / 8)).  Slices past
//     the window are zero operands whose loads re-read the window's last slice: tint = 16 fills half a K step and
//     never reads its neighbour.
//   * Tile pair (ti, tj), tj <= ti: Re[p1][p2] = X1[p1] . X2[p2]^T over the (t, re/im) bytes, Im[p1][p2] =
//     X1[p1] . X2'[p2]^T with X2' = [~im, re]: ~x = -x - 1 is an int8 for every x (-(-128) is not), so
//     sum r1 * ~i2 + i1 * r2 = Im - sum r1, and the row sum of re comes from v_dot4 on the fragment.  8 MFMAs per
//     step.  The lane of D holds 4 antennas a1 x 1 antenna a2 x all (p1, p2, re/im): the 32 output bytes of a baseline
//     are one lane's two 16-byte stores, and the 16 lanes of a row group write 512 contiguous bytes.
//   * Only tile pairs with tj <= ti exist; a diagonal pair computes the full 16 x 16 and stores a1 >= a2.
//   * uint8 samples run as s = u ^ 0x80 with the exact correction per component product
//     sum u1*u2 = sum s1*s2 + 128 (sum s1 + sum s2) + 16384 n; the constants cancel in Im.  Intermediate sums wrap
//     modulo 2^32 (uint32 arithmetic); the entry point bounds n so that the final value is an int32.
//   * Antennas past A (A % 16 != 0) re-read antenna A - 1; a row or column of D depends on its own operand row only,
//     so they need no zeroing, and they are never stored.
// A workgroup owns one block of 4 x 4 tile pairs (64 x 64 antennas) of the triangle, for one (window, channel) and
// the whole window: at most 8 tiles (4 on a diagonal block) and 16 pairs (10).  A <= 64 is one block, so the voltages
// leave HBM once; A = 256 is 10 blocks reading 64 tiles in all, each tile four times, and the workgroups of one
// (window, channel) are given block indices that agree modulo 8, which the dispatcher has been seen to place on one
// XCD (speed only; nothing depends on it), so the re-reads can meet in that L2.  Per K step, 128 staging threads per
// tile load the tile's 2 KiB once (8 threads read 128 contiguous bytes of one antenna; the next step's load is in
// flight), form the two pol fragments and their share of the row sums once per tile, and write the fragments to LDS in
// lane order (double-buffered, one barrier per step, as coef8_byte does for the coefficients); then one wave per pair
// reads four fragments (ds_read_b128), derives X2' (a v_perm and a v_xor per dword) and issues the 8 MFMAs.  The row
// sums are added up in LDS at the end (integer atomics on LDS: any order gives the same sum).  No global atomics:
// every output element is written once by one thread (with BF_CORR_ACCUMULATE that thread reads, adds and stores),
// and the input is never written.
#include "bf_fused.hpp"

namespace bf {
namespace {

constexpr int kTile = 16;         // antennas per tile
constexpr int kBlockTiles = 4;    // a workgroup owns a block of 4 x 4 tile pairs: at most 8 tiles, 16 pairs
constexpr int kCorrThreads = 1024;  // 16 waves: one per pair; 128 staging threads per tile
constexpr uint32_t kSelSwap = 0x02030001u;  // v_perm: [b1, b0, b3, b2]

typedef int i32x4_u __attribute__((ext_vector_type(4), aligned(4)));  // out is 4-byte aligned

struct CorrArgs {
  const uint8_t* raw;
  int32_t* out;
  int A, C, T, J;           // J = T / tint windows per (b, c)
  int tint, bint;
  int spb, slices, steps;   // 8-sample slices per batch of the window, per window; K steps of 4 slices
  int tiles, nblk, threads;  // 16-antenna tiles, workgroups per (window, channel), threads per workgroup
  unsigned ncw;             // (B / bint) * C * J
  unsigned nbl, n;          // baselines; samples per window
};

// Row i of the element p of a row-major lower triangle: i (i + 1) / 2 <= p < (i + 1)(i + 2) / 2.
__device__ __forceinline__ int tri_row(int p) {
  int i = static_cast<int>((__builtin_sqrtf(8.0f * static_cast<float>(p) + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > p) --i;
  while ((i + 1) * (i + 2) / 2 <= p) ++i;
  return i;
}

// One staging thread's 16 bytes (4 samples, both pols) -> its 8 bytes of the pol 0 and of the pol 1 fragment.
template <bool Signed>
__device__ __forceinline__ void fragments(const u32x4_t& v, uint32_t mask, u32x2_t (&x)[2]) {
  uint32_t d[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    d[i] = v[i];
    if constexpr (!Signed) d[i] ^= 0x80808080u;
    d[i] &= mask;
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint32_t sel = p ? kSelP1 : kSelP0;
    x[p][0] = __builtin_amdgcn_perm(d[1], d[0], sel);
    x[p][1] = __builtin_amdgcn_perm(d[3], d[2], sel);
  }
}

template <bool Signed, bool Accumulate>
__global__ __launch_bounds__(kCorrThreads) void correlate_kernel(CorrArgs P) {
  // [buffer][tile of the block][pol][lane] x 16 bytes: the operand fragments of one K step, in lane order
  __shared__ u32x4_t frag[2][kBlockTiles * 2][2][64];
  __shared__ int sums[kBlockTiles * 2][kTile][4];  // per antenna of a tile: sum re, sum im of pol 0, of pol 1

  const int tid = threadIdx.x, lane = tid & 63, row = lane & 15, h = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned cw, blk;
  if (P.nblk == 1) {
    cw = blockIdx.x;
    blk = 0;
  } else {  // the workgroups of one (window, channel) agree in blockIdx.x % 8
    const unsigned q = blockIdx.x >> 3;
    blk = q % P.nblk;
    cw = (q / P.nblk) * 8 + (blockIdx.x & 7);
  }
  if (cw >= P.ncw) return;  // the whole workgroup

  // the block (bi, bj), bj <= bi, of kBlockTiles x kBlockTiles tile pairs; its tiles: the rows, then (off the
  // diagonal) the columns
  const int bi = tri_row(static_cast<int>(blk)), bj = static_cast<int>(blk) - bi * (bi + 1) / 2;
  const int r0 = kBlockTiles * bi, c0 = kBlockTiles * bj;
  const int nr = min(kBlockTiles, P.tiles - r0), nc = min(kBlockTiles, P.tiles - c0);
  const bool dblock = bi == bj;
  const int nt = dblock ? nr : nr + nc;
  const int npairs = dblock ? nr * (nr + 1) / 2 : nr * nc;

  // this wave's pair: local tile indices t1, t2 into the block's tile list, global tile indices g1 >= g2
  const bool computes = wave < npairs;
  int t1 = 0, t2 = 0, g1 = 0, g2 = 0;
  if (computes) {
    if (dblock) {
      t1 = tri_row(wave);
      t2 = wave - t1 * (t1 + 1) / 2;
      g1 = r0 + t1;
      g2 = r0 + t2;
    } else {
      t1 = wave / nc;
      t2 = nr + (wave - t1 * nc);
      g1 = r0 + t1;
      g2 = c0 + (t2 - nr);
    }
  }

  // staging: thread (tile st, antenna srow, slice sh, half) loads 16 of the lane's 32 bytes; 8 threads read 128
  // contiguous bytes of one antenna
  const bool stages = tid < nt * 128;  // whole waves
  const int st = tid >> 7, srow = (tid >> 3) & 15, sh = (tid >> 1) & 3, half = tid & 1;
  const unsigned j = cw % P.J, kc = cw / P.J, c = kc % P.C, k = kc / P.C;
  const size_t run = static_cast<size_t>(P.T) * 4;           // bytes of one (b, a, c)
  const size_t batch = static_cast<size_t>(P.A) * P.C * run;  // bytes of one b
  const int sg = st < nr ? r0 + st : c0 + (st - nr);
  const int ant = min(kTile * sg + srow, P.A - 1);
  const uint8_t* src = P.raw + static_cast<size_t>(k) * P.bint * batch + (static_cast<size_t>(ant) * P.C + c) * run +
                       static_cast<size_t>(j) * P.tint * 4 + half * 16;

  // slice s of the window: batch s / spb of the window, samples 8 (s % spb) ..+7; past the window, the last slice
  auto load = [&](int step) {
    const int s = min(4 * step + sh, P.slices - 1);
    const int bo = P.bint > 1 ? s / P.spb : 0;
    return *reinterpret_cast<const u32x4_t*>(src + bo * batch + static_cast<size_t>(s - bo * P.spb) * 32);
  };

  if (tid < kBlockTiles * 2 * kTile * 4) (&sums[0][0][0])[tid] = 0;  // ordered before the adds by the loop's barriers

  i32x4_t re[2][2], im[2][2];
#pragma unroll
  for (int p1 = 0; p1 < 2; ++p1)
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) re[p1][p2] = im[p1][p2] = i32x4_t{0, 0, 0, 0};
  int sr[2] = {0, 0}, si[2] = {0, 0};  // staging thread: its samples' share of the row sums

  u32x4_t next = {};
  if (stages) next = load(0);
  for (int step = 0; step < P.steps; ++step) {
    const int buf = step & 1;
    if (stages) {
      const u32x4_t v = next;
      if (step + 1 < P.steps) next = load(step + 1);
      const uint32_t mask = 4 * step + sh < P.slices ? 0xffffffffu : 0u;
      u32x2_t x[2];
      fragments<Signed>(v, mask, x);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        reinterpret_cast<u32x2_t*>(&frag[buf][st][p][srow + 16 * sh])[half] = x[p];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          sr[p] = __builtin_amdgcn_sdot4(static_cast<int>(x[p][m]), 0x00010001, sr[p], false);
          si[p] = __builtin_amdgcn_sdot4(static_cast<int>(x[p][m]), 0x01000100, si[p], false);
        }
      }
    }
    // One barrier per step: buffer `buf` was last read in step - 2, and every wave has passed the barrier of
    // step - 1 since, which it reaches only with those reads done.
    lds_barrier();
    if (computes) {
      i32x4_t x1[2], x2[2], xc[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        x1[p] = __builtin_bit_cast(i32x4_t, frag[buf][t1][p][lane]);
        x2[p] = __builtin_bit_cast(i32x4_t, frag[buf][t2][p][lane]);
#pragma unroll
        for (int m = 0; m < 4; ++m)  // [~im, re]: where the slice is masked this is -1 against a zero row of X1
          xc[p][m] = static_cast<int>(__builtin_amdgcn_perm(x2[p][m], x2[p][m], kSelSwap) ^ 0x00ff00ffu);
      }
#pragma unroll
      for (int p1 = 0; p1 < 2; ++p1)
#pragma unroll
        for (int p2 = 0; p2 < 2; ++p2) {
          re[p1][p2] = mfma_i8(x1[p1], x2[p2], re[p1][p2]);
          im[p1][p2] = mfma_i8(x1[p1], xc[p2], im[p1][p2]);
        }
    }
  }

  // row sums of the window: integer adds, so their order does not matter
  if (stages) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      atomicAdd(&sums[st][srow][2 * p], sr[p]);
      atomicAdd(&sums[st][srow][2 * p + 1], si[p]);
    }
  }
  __syncthreads();
  if (!computes) return;

  int32_t* out = P.out + static_cast<size_t>(cw) * P.nbl * 8;
  const int c2 = kTile * g2 + row;
  uint32_t br[2], bi2[2];  // sums of column c2 of the second tile, per pol
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    br[p] = static_cast<uint32_t>(sums[t2][row][2 * p]);
    bi2[p] = static_cast<uint32_t>(sums[t2][row][2 * p + 1]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int r1 = kTile * g1 + 4 * h + r;
    uint32_t ar[2], ai[2];  // sums of row r1 of the first tile, per pol
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      ar[p] = static_cast<uint32_t>(sums[t1][4 * h + r][2 * p]);
      ai[p] = static_cast<uint32_t>(sums[t1][4 * h + r][2 * p + 1]);
    }
    uint32_t w[8];
#pragma unroll
    for (int p1 = 0; p1 < 2; ++p1)
#pragma unroll
      for (int p2 = 0; p2 < 2; ++p2) {
        uint32_t vr = static_cast<uint32_t>(re[p1][p2][r]);
        uint32_t vi = static_cast<uint32_t>(im[p1][p2][r]) + ar[p1];  // sum r1 * ~i2 = sum r1 * -i2 - sum r1
        if constexpr (!Signed) {
          vr += 128u * (ar[p1] + ai[p1] + br[p2] + bi2[p2]) + 32768u * P.n;
          vi += 128u * (ai[p1] - ar[p1] + br[p2] - bi2[p2]);
        }
        w[(p1 * 2 + p2) * 2] = vr;
        w[(p1 * 2 + p2) * 2 + 1] = vi;
      }
    if (r1 < P.A && c2 <= r1) {  // c2 <= r1 < A
      i32x4_u* o = reinterpret_cast<i32x4_u*>(out + (static_cast<size_t>(r1) * (r1 + 1) / 2 + c2) * 8);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if constexpr (Accumulate) {
          const i32x4_u old = o[q];
#pragma unroll
          for (int e = 0; e < 4; ++e) w[4 * q + e] += static_cast<uint32_t>(old[e]);
        }
        o[q] = i32x4_u{static_cast<int>(w[4 * q]), static_cast<int>(w[4 * q + 1]), static_cast<int>(w[4 * q + 2]),
                       static_cast<int>(w[4 * q + 3])};
      }
    }
  }
}

// nullptr when bf_correlate accepts the shape, else what is wrong with it.
const char* corr_shape_error(int B, int C, int T, int A, int tint, int bint, int flags) {
  if (B < 1 || C < 1 || T < 1) return "bad shape, B, C, T must be positive";
  if (A < 1 || A > 2048) return "antennas, need 1 .. 2048";
  if (T % kSamplesPerBlock != 0 || T > (1 << 20)) return "bad shape, T must be a multiple of 16, at most 2^20";
  if (tint < 16 || tint % 16 != 0 || T % tint != 0) return "integration must be a multiple of 16 that divides T";
  if (bint < 1 || B % bint != 0) return "batch integration must be positive and divide B";
  if (bint > 1 && tint != T) return "batch integration above 1 needs integration == T";
  if (flags & ~(BF_CORR_SIGNED | BF_CORR_ACCUMULATE)) return "unknown flags";
  const long long n = static_cast<long long>(bint) * tint;
  if (n > ((flags & BF_CORR_SIGNED) ? 65535 : 16512))
    return "samples per window above the int32 bound (65535 for int8, 16512 for uint8)";
  return nullptr;
}

// The launch of an accepted shape: (window, channel) items, tiles, workgroups per item (the blocks of the triangle
// of kBlockTiles x kBlockTiles tile pairs), threads per workgroup (a wave per pair and 128 staging threads per tile
// of the largest block).  Returns the grid (items padded to a multiple of 8 where an item has several workgroups).
unsigned long long corr_grid(int B, int C, int T, int A, int tint, int bint, unsigned long long* ncw, int* tiles,
                             int* nblk, int* threads) {
  *ncw = static_cast<unsigned long long>(B / bint) * C * (T / tint);
  *tiles = (A + kTile - 1) / kTile;
  const int side = (*tiles + kBlockTiles - 1) / kBlockTiles;
  *nblk = side * (side + 1) / 2;
  const int pairs = *tiles * (*tiles + 1) / 2, stagers = 2 * *tiles;  // waves of either kind, one block
  *threads = side > 1 ? kCorrThreads : 64 * (pairs > stagers ? pairs : stagers);
  return *nblk == 1 ? *ncw : (*ncw + 7) / 8 * 8 * *nblk;
}

}  // namespace
}  // namespace bf

extern "C" int bf_correlate(const uint8_t* raw, int32_t* out, int B, int C, int T, int A, int tint, int bint, int flags,
                            void* stream) {
  BF_REQUIRE(raw && out, "bf_correlate: null pointer");
  const char* why = bf::corr_shape_error(B, C, T, A, tint, bint, flags);
  BF_REQUIRE(!why, "bf_correlate: %s (B=%d C=%d T=%d A=%d integration=%d batch integration=%d flags=0x%x)", why, B, C,
             T, A, tint, bint, flags);
  BF_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
             "bf_correlate: misaligned buffer");

  bf::CorrArgs P;
  P.raw = raw;
  P.out = out;
  P.A = A;
  P.C = C;
  P.T = T;
  P.J = T / tint;
  P.tint = tint;
  P.bint = bint;
  P.spb = tint / 8;
  P.slices = bint * P.spb;
  P.steps = (P.slices + 3) / 4;
  P.nbl = static_cast<unsigned>(A) * (A + 1) / 2;
  P.n = static_cast<unsigned>(bint) * tint;
  unsigned long long ncw;
  const unsigned long long total = bf::corr_grid(B, C, T, A, tint, bint, &ncw, &P.tiles, &P.nblk, &P.threads);
  BF_REQUIRE(total <= 0x7fffffffull, "bf_correlate: bad shape, %llu workgroups exceed the grid limit", total);
  P.ncw = static_cast<unsigned>(ncw);
  hipStream_t st = bf::as_stream(stream);
  const bool sgn = flags & BF_CORR_SIGNED, acc = flags & BF_CORR_ACCUMULATE;
  const dim3 grid(static_cast<unsigned>(total)), block(P.threads);
  if (sgn && acc)
    hipLaunchKernelGGL((bf::correlate_kernel<true, true>), grid, block, 0, st, P);
  else if (sgn)
    hipLaunchKernelGGL((bf::correlate_kernel<true, false>), grid, block, 0, st, P);
  else if (acc)
    hipLaunchKernelGGL((bf::correlate_kernel<false, true>), grid, block, 0, st, P);
  else
    hipLaunchKernelGGL((bf::correlate_kernel<false, false>), grid, block, 0, st, P);
  BF_LAUNCHED_TAG("correlate_kernel", "%s%s", sgn ? "i8" : "u8", acc ? ",acc" : "");
}

extern "C" double bf_correlate_algorithmic_bytes(int B, int C, int T, int A, int tint, int bint, int flags) {
  if (bf::corr_shape_error(B, C, T, A, tint, bint, flags)) return 0.0;
  unsigned long long ncw;
  int tiles, nblk, threads;
  if (bf::corr_grid(B, C, T, A, tint, bint, &ncw, &tiles, &nblk, &threads) > 0x7fffffffull) return 0.0;
  const double nbl = static_cast<double>(A) * (A + 1) / 2;
  const double outb = 32.0 * nbl * static_cast<double>(ncw);
  return 4.0 * B * static_cast<double>(A) * C * T + ((flags & BF_CORR_ACCUMULATE) ? 2.0 : 1.0) * outb;
}
