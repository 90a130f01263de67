// Sizes that the fused kernels and their host-side launch plan (bf_fused_plan.cpp) must agree on.  Plain C++: no HIP
// include, so the planner compiles with any host compiler.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define BF_HD __host__ __device__
#else
#define BF_HD
#endif

namespace bf {

constexpr size_t kMaxLds = 160 * 1024;

// f16 hi/lo coefficient fragments of S k-steps x nts tiles (bf_mfma.hpp coef_elem)
inline size_t coef_lds_bytes(int S, int nts) { return static_cast<size_t>(S) * nts * 2 * 64 * 16; }

constexpr int kGroup = 4;  // k-steps per register-resident load group (64 antennas)

// Staged float-beam stores (the item kernel's StagedF32 form): each wave's 8 KiB (64 rows x 128 B, one slab = the
// whole row) staged through a padded wave-private LDS image and written as 1 KiB contiguous pieces per store
// instruction.
constexpr int kF32StageRow = 36;                        // floats per staged row (32 + 4: 4-way write conflicts)
constexpr size_t kF32StageBytes = 4 * 64 * kF32StageRow * 4;  // 4 waves x 64 rows

// ---- float wide kernels (bf_wide.hip)
constexpr int kWideGroup = 2;  // k-steps (16 antennas each) per register-resident load group
// k-steps of 16 antennas, padded to a whole number of ping-pong pairs of groups (see the kernel).
BF_HD inline int wide_padded_steps(int A) {
  return 2 * kWideGroup * ((((A + 15) >> 4) + 2 * kWideGroup - 1) / (2 * kWideGroup));
}
constexpr int kWidePSteps = 16;  // the persistent form's k-steps of 16 antennas: A = 256

// ---- integer wide kernels (bf_wide_i8.hip)
constexpr int kW32Beams = 32;      // beams of a workgroup slab
constexpr int kW32TChannels = 4;   // channels a table-driven workgroup walks (8 in its straight-line form)
constexpr int kW32RChannels = 8;   // channels an LDS-DMA ring workgroup walks
// k-steps of 32 antennas of the 32-beam int8 kernel, padded to a multiple of 4 (its four-buffer rotation); padded
// steps have zero table rows
BF_HD inline int w32_table_steps(int A) { return 4 * ((((A + 31) >> 5) + 3) / 4); }
// The table-driven 32-beam kernel stages at most 4 units of 8 words per thread: Sp <= 8 (A <= 256).
BF_HD inline bool w32_table_fits(int A) { return w32_table_steps(A) <= 8; }
// Bytes of the int8 wide path's coefficient table of one launch (kLayoutW32): 1024 Sp words per (b, c, 32-beam slab).
inline size_t w32_table_bytes(int B, int C, int A, int M) {
  return static_cast<size_t>(B) * C * ((M + 31) / 32) * 1024 * w32_table_steps(A) * 4;
}
// LDS: the Q14 limb image (Sp steps x 4 tiles x 2 limbs x 64 lanes x 16 B) + the unsigned correction's partial
// column sums (4 waves x 64 columns)
BF_HD inline size_t w32_lds_bytes(int A) {
  return static_cast<size_t>(w32_table_steps(A)) * 4 * 2 * 64 * 16 + 4 * 64 * 4;
}

// Whether s is a power of two (a normal float with an all-zero mantissa): requant_bits<true> is then exact.
inline bool scale_is_pow2(float s) {
  uint32_t u;
  memcpy(&u, &s, 4);
  const uint32_t e = (u >> 23) & 255;
  return (u & 0x7fffffu) == 0 && e > 0 && e < 255;
}

}  // namespace bf
