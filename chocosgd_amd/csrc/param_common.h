// Helpers shared by the kernels that walk a table of parameter tensors in the kernel
// arguments (params.hip: pack / unpack; sgd.hip: the SGD update fused with the pack):
// the tile geometry, the 16-bit conversions and the 16-byte non-temporal store.
#pragma once

#include "choco_common.h"

namespace choco {

constexpr int kPbThreads = 256;
constexpr int kPbGroup = 8;                                          // elements per group
constexpr int64_t kPbTile = (int64_t)kPbThreads * 4 * kPbGroup;      // 8192 flat elements per workgroup

typedef unsigned short choco_u16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------- conversions
CHOCO_DEV float bf16_widen(unsigned short h) { return __uint_as_float((uint32_t)h << 16); }
// round-to-nearest-even on the upper 16 bits; NaN -> quiet NaN (the carry of the
// rounding add would otherwise turn some NaNs into inf)
CHOCO_DEV unsigned short bf16_narrow(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)0x7fc0u;
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
CHOCO_DEV float f16_widen(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }
// v_cvt_f16_f32: round-to-nearest-even, overflow -> inf, subnormal results kept
CHOCO_DEV unsigned short f16_narrow(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }

template <int DT>
CHOCO_DEV float widen16(unsigned short h) {
  return DT == CHOCO_DT_BF16 ? bf16_widen(h) : f16_widen(h);
}
template <int DT>
CHOCO_DEV unsigned short narrow16(float f) {
  return DT == CHOCO_DT_BF16 ? bf16_narrow(f) : f16_narrow(f);
}

CHOCO_DEV void st_nt4(float* p, float4 v) {
  choco_f32x4 f;
  f.x = v.x; f.y = v.y; f.z = v.z; f.w = v.w;
  __builtin_nontemporal_store(f, reinterpret_cast<choco_f32x4*>(p));
}

CHOCO_DEV int64_t i64max(int64_t x, int64_t y) { return x > y ? x : y; }
CHOCO_DEV int64_t i64min(int64_t x, int64_t y) { return x < y ? x : y; }

}  // namespace choco
