// The fused beamformer's launch plan: every shape predicate, LDS size and grid of bf_beamform_fused*, once.
// Measurements behind the thresholds are cited where the kernels are defined.
#include "bf_fused_plan.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

namespace bf {
namespace {

FusedPlan refuse(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
FusedPlan refuse(const char* fmt, ...) {
  FusedPlan p{};
  p.status = BF_ERR_ARG;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p.error, sizeof(p.error), fmt, ap);
  va_end(ap);
  return p;
}

FusedPlan with_grid(FusedPlan p, long long grid, const char* too_large = "grid too large") {
  if (grid >= (1LL << 31)) return refuse("bf_beamform_fused: %s", too_large);
  p.grid = static_cast<unsigned>(grid);
  return p;
}

// What a shape is, beyond its numbers.
struct Shape : FusedShape {
  explicit Shape(const FusedShape& s) : FusedShape(s) {}
  int path() const { return flags & BF_FUSED_PATH_MASK; }
  int order() const { return flags & BF_FUSED_ORDER_MASK; }
  int S() const { return (2 * A + 31) / 32; }   // f16 k-steps of 16 antennas
  int S8() const { return (2 * A + 63) / 64; }  // i8 k-steps of 32 antennas
  int NT() const { return (2 * M + 15) / 16; }  // 16-column tiles of the 2M beam components
  long long items() const { return static_cast<long long>(B) * C; }
  // The item kernels' shape: one register-resident group of 64 antennas, one 64-sample chunk per wave.
  bool small() const { return A <= 64 && T <= 256; }
  // Every voltage offset inside one batch below 2^31: buffer-resource loads (SGPR row offsets) can address it.
  bool offsets31() const { return static_cast<unsigned long long>(A) * C * T * 4 < (1ull << 31); }
  // A lane's 32-bit offset over `rows` antenna rows plus one time run stays below 2^32.
  bool lane_offsets32(int rows) const {
    return static_cast<size_t>(rows) * C * T * 4 + static_cast<size_t>(T) * 4 < (1ull << 32);
  }
  // Workgroup order of the slab kernels: the slabs of an item back to back on one XCD (they share its L2).
  bool slab_xcd_order(int nslabs) const { return nslabs > 1 && order() != BF_FUSED_ORDER_CHANNEL; }
  long long slab_grid(long long columns, int nslabs, bool xcd) const {
    return xcd ? (columns + 7) / 8 * 8 * nslabs : columns * nslabs;
  }
  // Workgroup order of the item kernels: XCD-range when C % 8 == 0 and the beams are at least 8; channel-fastest for
  // one or two beams, whose read-dominated traffic measured no better that way.  BF_FUSED_ORDER_XCD / _CHANNEL force.
  bool item_xcd_order() const {
    if (order() == BF_FUSED_ORDER_CHANNEL) return false;
    if (order() == BF_FUSED_ORDER_XCD) return (C & 7) == 0;
    return (C & 7) == 0 && M >= 8;
  }
  // The float wide kernel: at least one k-step of real antennas, and 16-beam slabs of its (R, -I) table fit LDS
  // (A <= 1280).
  bool wide_fits() const {
    return A >= 16 && lane_offsets32(12) && coef_lds_bytes(wide_padded_steps(A), 1) <= kMaxLds;
  }
  // Its persistent form (beamform_fused_wide_p2_kernel).
  bool wide_p2_fits() const {
    return A == 256 && T == 256 && M % 32 == 0 && delay_channels == 1 && !gains && offsets31();
  }
  // The 32-beam integer kernels: their Q14 limb image in LDS (A <= 512).
  bool i8_w32_fits() const { return A >= 32 && (T & 1) == 0 && lane_offsets32(24) && w32_lds_bytes(A) <= kMaxLds; }
  // The LDS-DMA ring contraction: 8 k-steps, T = 256, whole 32-beam slabs, the beams below 2^31 bytes too.
  bool w32r_fits() const {
    return w32_table_steps(A) == 8 && A > 224 && T == 256 && M % kW32Beams == 0 && offsets31() &&
           static_cast<unsigned long long>(B) * 2 * C * T * 2 * M < (1ull << 31);
  }
};

// Slab width and completeness of the two item kernels: two tiles when there are two, full when every slab is.
void item_slabs(const Shape& s, FusedPlan& p) {
  p.nts = s.NT() >= 2 ? 2 : 1;
  p.full = p.nts == 2 ? (2 * s.M) % 32 == 0 : 2 * s.M == 16;
  p.nslabs = (s.NT() + p.nts - 1) / p.nts;
  p.xcd_order = s.item_xcd_order();
}

FusedPlan plan_item(const Shape& s, FusedPlan p) {
  p.family = FusedFamily::Item;
  item_slabs(s, p);
  p.staged = !p.i8out && s.M == 16;  // float beams of 16 beams (config 3): 1 KiB stores staged through LDS
  p.pow2 = p.i8out && scale_is_pow2(s.out_scale);
  p.lds = coef_lds_bytes(s.S(), p.nts) + (p.staged ? kF32StageBytes : 0);
  return with_grid(p, p.nslabs * s.items(), "too many (batch, channel) items");
}

FusedPlan plan_generic(const Shape& s, FusedPlan p) {
  p.family = FusedFamily::Generic;
  p.nts = s.NT() >= 2 && coef_lds_bytes(s.S(), 2) <= kMaxLds ? 2 : 1;
  p.nslabs = (s.NT() + p.nts - 1) / p.nts;
  p.lds = coef_lds_bytes(s.S(), p.nts);
  if (p.lds > kMaxLds) return refuse("bf_beamform_fused: n_ants=%d too large", s.A);
  p.xcd_order = s.slab_xcd_order(p.nslabs);
  return with_grid(p, s.slab_grid(s.items(), p.nslabs, p.xcd_order));
}

FusedPlan plan_wide(const Shape& s, FusedPlan p) {
  if (!p.exact && s.wide_p2_fits() && s.order() != BF_FUSED_ORDER_CHANNEL) {
    // config 4's shape.  Its channel-run walk has no plain channel-fastest mapping: an explicit
    // BF_FUSED_ORDER_CHANNEL takes the slab kernel below, which honours it.
    p.family = FusedFamily::WideP2;
    p.nts = 2;
    p.nslabs = s.M / 32;
    const long long units = static_cast<long long>(s.B) * p.nslabs;
    const int cus = std::max(1, s.cus);
    p.ch_run = static_cast<int>(std::min<long long>(s.C, std::max<long long>(1, (s.C * units + cus - 1) / cus)));
    const long long groups = static_cast<long long>(s.B) * ((s.C + p.ch_run - 1) / p.ch_run);
    p.lds = 2 * coef_lds_bytes(kWidePSteps, 2);  // two 64 KiB tables
    p.block = 512;
    return with_grid(p, s.slab_grid(groups, p.nslabs, true));
  }
  p.family = FusedFamily::Wide;
  const int Sp = wide_padded_steps(s.A);
  // 32-beam slabs (two workgroups per CU while the table is <= 80 KiB, A <= 320); 16-beam slabs for more antennas
  // or few beams.
  p.nts = s.M > 16 && coef_lds_bytes(Sp, 2) <= kMaxLds ? 2 : 1;
  p.buf = s.offsets31();
  p.lds = coef_lds_bytes(Sp, p.nts);
  p.nslabs = (s.M + 16 * p.nts - 1) / (16 * p.nts);
  p.xcd_order = s.slab_xcd_order(p.nslabs);
  return with_grid(p, s.slab_grid(s.items(), p.nslabs, p.xcd_order));
}

FusedPlan plan_i8_item(const Shape& s, FusedPlan p) {
  p.family = FusedFamily::I8Item;
  item_slabs(s, p);
  p.a64 = s.A == 64 && s.lane_offsets32(24);  // no antenna is clamped, every in-item offset is 32-bit
  p.pow2 = scale_is_pow2(s.out_scale * 0x1p-14f);
  p.lds = static_cast<size_t>(2) * p.nts * 2 * 64 * 16 + 4 * 32 * 4;  // limb image of 2 k-steps + 4 waves' column sums
  return with_grid(p, p.nslabs * s.items(), "too many items");
}

FusedPlan plan_i8_generic(const Shape& s, FusedPlan p) {
  p.family = FusedFamily::I8Generic;
  auto lds_bytes = [&](int nts) { return static_cast<size_t>(s.S8()) * nts * 2 * 64 * 16 + nts * 16 * 4; };
  p.nts = s.NT() >= 2 && lds_bytes(2) <= kMaxLds ? 2 : 1;
  p.lds = lds_bytes(p.nts);
  if (p.lds > kMaxLds) return refuse("bf_beamform_fused: n_ants=%d too large", s.A);
  p.nslabs = (s.NT() + p.nts - 1) / p.nts;
  return with_grid(p, s.items() * p.nslabs);
}

FusedPlan plan_w32(const Shape& s, FusedPlan p) {
  p.family = FusedFamily::W32;
  p.nslabs = (s.M + kW32Beams - 1) / kW32Beams;
  p.xcd_order = s.slab_xcd_order(p.nslabs);
  p.lds = w32_lds_bytes(s.A);
  // a workgroup per (item, slab): the kernel that evaluates its phasors itself, and the table generator's bound
  p = with_grid(p, s.slab_grid(s.items(), p.nslabs, p.xcd_order));
  const size_t need = w32_table_bytes(s.B, s.C, s.A, s.M);
  if (p.status != BF_OK || !w32_table_fits(s.A) || s.workspace_bytes < need) return p;
  p.table = true;
  p.table_bytes = need;
  p.pow2 = scale_is_pow2(s.out_scale * 0x1p-14f);
  int channels;  // a workgroup walks this many consecutive channels of its slab
  if (p.sgn && s.w32r_fits()) {  // config 4's shape: the LDS-DMA voltage ring (static LDS)
    p.family = FusedFamily::W32R;
    p.lds = 0;
    channels = kW32RChannels;
  } else {
    p.family = FusedFamily::W32T;
    const int npasses = ((((s.T >> 1) + 15) >> 4) + 3) >> 2;
    p.buf = s.offsets31();
    // config 4's shape: straight-line code over 8 steps x 2 passes, 8 channels per workgroup (buffer loads only)
    p.straight = w32_table_steps(s.A) == 8 && npasses == 2 && p.buf;
    p.pow2 = p.pow2 && p.straight;  // the general forms have no power-of-two instantiation
    channels = p.straight ? 8 : kW32TChannels;
  }
  const long long groups = static_cast<long long>(s.B) * ((s.C + channels - 1) / channels);
  return with_grid(p, s.slab_grid(groups, p.nslabs, p.xcd_order));
}

}  // namespace

FusedPlan plan_fused(const FusedShape& shape) {
  const Shape s(shape);
  FusedPlan p{};
  p.sgn = s.flags & BF_FUSED_SIGNED;
  p.i8out = s.flags & BF_FUSED_OUT_INT8;
  p.exact = s.flags & BF_FUSED_EXACT_COEFF;
  p.gain = s.gains;
  p.block = 256;
  const int path = s.path();
  const bool item = s.small() && path != BF_FUSED_PATH_GENERIC;
  // int8 beams: the Q14 integer contract (default), or requantised float beams (BF_FUSED_INT8_VIA_F32)
  if (p.i8out && !(s.flags & BF_FUSED_INT8_VIA_F32)) {
    // The contract's int32 sum: |y| <= A * max|x| * (|Wc| + |Ws|) with |Wc| + |Ws| <= sqrt(2) * 2^14 + 1 = 23171 at
    // unit gain.  Beyond that the int32 accumulators would wrap (the oracle sums in int64): refuse.  With gains the
    // caller, which owns the weights, checks the bound (FusedBeamformerTemplate.check_weights).
    if (!s.gains && static_cast<double>(s.A) * (p.sgn ? 128 : 255) * 23171.0 >= 2147483648.0)
      return refuse("bf_beamform_fused: n_ants=%d overflows the int8 path's int32 beam sums (%s samples); use float "
                    "beams or BF_FUSED_INT8_VIA_F32", s.A, p.sgn ? "int8" : "uint8");
    // the 32-beam slab kernels up to A = 512; beyond, the generic kernel (groups of 64 antennas)
    if ((path == BF_FUSED_PATH_WIDE || (path == 0 && !s.small())) && s.i8_w32_fits()) return plan_w32(s, p);
    return item ? plan_i8_item(s, p) : plan_i8_generic(s, p);
  }
  // float beams of many antennas x beams (config 4): the wide kernel keeps every beam of the item in one workgroup
  if (!p.i8out && (path == BF_FUSED_PATH_WIDE || (path == 0 && s.M >= 24 && (!s.small() || s.M > 32))) && s.wide_fits())
    return plan_wide(s, p);
  return item ? plan_item(s, p) : plan_generic(s, p);
}

const char* fused_family_name(FusedFamily f) {
  static const char* const names[] = {  // in FusedFamily's order
      "beamform_fused_item_kernel",    "beamform_fused_kernel",        "beamform_fused_wide_kernel",
      "beamform_fused_wide_p2_kernel", "beamform_fused_i8_item_kernel", "beamform_fused_i8_kernel",
      "beamform_fused_i8_w32_kernel",  "beamform_fused_i8_w32t_kernel", "beamform_fused_i8_w32r_kernel"};
  return names[static_cast<int>(f)];
}

void fused_plan_name(const FusedPlan& p, char* out, size_t len) {
  const char* fam = fused_family_name(p.family);
  const char *io = p.i8out ? "i8" : "f32", *full = p.full ? "full" : "partial", *ex = p.exact ? "exact" : "fast";
  const char* scale = p.pow2 ? "pow2" : "anyscale";
  switch (p.family) {
    case FusedFamily::Item:
      snprintf(out, len, "%s:%s,nts%d,%s,%s%s%s%s", fam, io, p.nts, full, ex, p.staged ? ",staged" : "",
               p.i8out ? "," : "", p.i8out ? scale : "");
      break;
    case FusedFamily::Generic: snprintf(out, len, "%s:%s,nts%d,%s", fam, io, p.nts, ex); break;
    case FusedFamily::Wide:
      snprintf(out, len, "%s:tw%d,%s,%s,%s", fam, p.nts, ex, p.gain ? "gain" : "unit", p.buf ? "buf" : "ptr");
      break;
    case FusedFamily::WideP2: snprintf(out, len, "%s", fam); break;
    case FusedFamily::I8Item:
      snprintf(out, len, "%s:nts%d,%s,%s,%s", fam, p.nts, full, p.a64 ? "a64" : "aany", scale);
      break;
    case FusedFamily::I8Generic: snprintf(out, len, "%s:nts%d", fam, p.nts); break;
    case FusedFamily::W32: snprintf(out, len, "%s:%s", fam, p.gain ? "gain" : "unit"); break;
    case FusedFamily::W32T:
      if (p.straight) snprintf(out, len, "%s:straight,%s", fam, scale);
      else snprintf(out, len, "%s:general,%s", fam, p.buf ? "buf" : "ptr");
      break;
    case FusedFamily::W32R: snprintf(out, len, "%s:%s", fam, scale); break;
  }
}

}  // namespace bf
