// The launch plan of bf_beamform_fused*: which kernel a call takes and with what launch configuration, decided in
// one place on the host (bf_fused_plan.cpp).  Pure: no device query (the CU count is an input), no allocation, no
// HIP include -- any host compiler builds it, and bf_fused_plan() answers "which kernel will this shape take?"
// without a GPU.  The launchers in bf_fused.hip, bf_wide.hip and bf_wide_i8.hip only map a plan to a template
// instantiation and launch it.
#pragma once

#include "../../include/bf.h"
#include "bf_fused_dims.hpp"

namespace bf {

enum class FusedFamily {
  Item,       // beamform_fused_item_kernel      float contraction, A <= 64 and T <= 256, a workgroup per (slab, b, c)
  Generic,    // beamform_fused_kernel           float contraction, any A, any T
  Wide,       // beamform_fused_wide_kernel      float beams of many antennas x beams, 16 tw beams per workgroup
  WideP2,     // beamform_fused_wide_p2_kernel   its persistent form (config 4's shape)
  I8Item,     // beamform_fused_i8_item_kernel   Q14 contract, A <= 64 and T <= 256
  I8Generic,  // beamform_fused_i8_kernel        Q14 contract, any A, any T
  W32,        // beamform_fused_i8_w32_kernel    Q14 contract, 32-beam slabs, phasors evaluated in the kernel
  W32T,       // beamform_fused_i8_w32t_kernel   ... coefficients from the Q14 table in the workspace
  W32R,       // beamform_fused_i8_w32r_kernel   ... and voltages through the LDS-DMA ring (config 4's shape)
};

struct FusedShape {
  int B, C, T, A, M, delay_channels;
  bool gains;              // a per-input weight table is given
  int flags;               // BF_FUSED_* (valid: fused_flags_error)
  float out_scale;
  size_t workspace_bytes;  // offered by the caller (0: none)
  int cus;                 // compute units of the device (sizes the persistent grid only)
};

struct FusedPlan {
  int status;       // BF_OK, or BF_ERR_ARG with `error`: the call is refused, nothing else is set
  char error[200];
  FusedFamily family;
  // the variant: what the launcher turns into template arguments (and fused_plan_name into the tag)
  bool sgn, i8out, exact;  // of the flags: int8 samples, int8 beams, float64 phasors
  int nts;                 // 16-column tiles per workgroup slab (the wide kernel's TW)
  bool full, staged;       // item kernels: every slab complete; float beams staged through LDS
  bool a64, pow2;          // exactly 64 antennas with 32-bit offsets; a power-of-two requantisation scale
  bool buf, gain;          // buffer-resource voltage loads; the weighted instantiation
  bool straight;           // W32T: the straight-line form of config 4's shape
  bool table;              // the Q14 table is generated into the workspace first
  size_t table_bytes;      // what it needs there (0 without table)
  int nslabs, xcd_order, ch_run;  // FusedArgs fields of the launch
  size_t lds;                     // dynamic LDS bytes
  unsigned grid, block;
};

FusedPlan plan_fused(const FusedShape& s);

const char* fused_family_name(FusedFamily f);
// bf_last_kernel's name of a plan: "family" or "family:tag".
void fused_plan_name(const FusedPlan& p, char* out, size_t len);

}  // namespace bf
