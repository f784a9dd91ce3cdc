// Helpers shared by the kernels that walk a table of parameter tensors in the kernel
// arguments (params.hip: pack / unpack; sgd.hip: the SGD update fused with the pack;
// gradnorm.hip: the gradient norms beside it; mix.hip: the neighbour-weighted model mix): the
// tile geometry, the SGD table's flag bits, the 16-bit conversions, the 16-byte
// non-temporal store, the element / group moves and the tile walk's search.
#pragma once

#include "choco_common.h"

namespace choco {

constexpr int kPbThreads = 256;
constexpr int kPbGroup = 8;                                          // elements per group
constexpr int64_t kPbTile = (int64_t)kPbThreads * 4 * kPbGroup;      // 8192 flat elements per workgroup

// flags of the SGD and norm tables (sgd.hip, gradnorm.hip): the ABI's three CHOCO_SGD_F_* bits,
// then what the host derives from the doubles
constexpr uint32_t kSgdHasWd = 8u, kSgdHasMom = 16u;

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

// The value as the storage dtype holds it.  v is the fp32 result of its line and is narrowed
// from there (two roundings, as a torch op on a 16-bit tensor has): the empty asm keeps the
// compiler from merging an fma and the conversion into one v_fma_mixlo_f16, which rounds the
// exact sum straight to fp16.
template <int DT>
CHOCO_DEV float rnd(float v) {
  if (DT == CHOCO_DT_F32) return v;
  asm("" : "+v"(v));
  return widen16<DT>(narrow16<DT>(v));
}

CHOCO_DEV void st_nt4(float* p, float4 v) {
  choco_f32x4 f;
  f.x = v.x; f.y = v.y; f.z = v.z; f.w = v.w;
  __builtin_nontemporal_store(f, reinterpret_cast<choco_f32x4*>(p));
}

CHOCO_DEV int64_t i64max(int64_t x, int64_t y) { return x > y ? x : y; }
CHOCO_DEV int64_t i64min(int64_t x, int64_t y) { return x < y ? x : y; }

// ---------------------------------------------------------------- one element / one group of a tensor
template <int DT>
CHOCO_DEV float ld1(const void* base, int64_t j) {
  if (DT == CHOCO_DT_F32) return reinterpret_cast<const float*>(base)[j];
  return widen16<DT>(reinterpret_cast<const unsigned short*>(base)[j]);
}
template <int DT>
CHOCO_DEV void st1(void* base, int64_t j, float v) {
  if (DT == CHOCO_DT_F32) reinterpret_cast<float*>(base)[j] = v;
  else reinterpret_cast<unsigned short*>(base)[j] = narrow16<DT>(v);
}

// a group of 8 elements as loaded: two float4 (fp32) or one 16-byte vector of halves
struct Raw8 {
  float4 lo, hi;
  choco_u16x8 h;
};
template <int DT>
CHOCO_DEV void ld8(Raw8& r, const void* base, int64_t j) {
  if (DT == CHOCO_DT_F32) {
    const float* s = reinterpret_cast<const float*>(base) + j;
    r.lo = ld_nt4(s);
    r.hi = ld_nt4(s + 4);
  } else {
    r.h = __builtin_nontemporal_load(
        reinterpret_cast<const choco_u16x8*>(reinterpret_cast<const unsigned short*>(base) + j));
  }
}
template <int DT>
CHOCO_DEV void widen8(const Raw8& r, float (&v)[8]) {
  if (DT == CHOCO_DT_F32) {
    v[0] = r.lo.x; v[1] = r.lo.y; v[2] = r.lo.z; v[3] = r.lo.w;
    v[4] = r.hi.x; v[5] = r.hi.y; v[6] = r.hi.z; v[7] = r.hi.w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = widen16<DT>(r.h[k]);
  }
}
template <int DT>
CHOCO_DEV void st8(void* base, int64_t j, const float (&v)[8]) {
  if (DT == CHOCO_DT_F32) {
    float* s = reinterpret_cast<float*>(base) + j;
    st_nt4(s, make_float4(v[0], v[1], v[2], v[3]));
    st_nt4(s + 4, make_float4(v[4], v[5], v[6], v[7]));
  } else {
    choco_u16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = narrow16<DT>(v[k]);
    __builtin_nontemporal_store(o, reinterpret_cast<choco_u16x8*>(reinterpret_cast<unsigned short*>(base) + j));
  }
}

// ---------------------------------------------------------------- the tile walk
// Workgroup `tile` owns flat elements [tile * kPbTile, (tile + 1) * kPbTile) cut to the chunk
// [off[0], off[nt]) of a launch's table: [tlo, thi).  Returns the first tensor that can hold
// an element of it, found by a uniform upper-bound search (the first s in [1, nt] with
// off[s] > tlo, off[nt] >= thi > tlo: tensor s - 1 holds tlo; zero-length tensors give equal
// offsets and are passed over), or -1 for an empty range.  The caller walks s upwards until
// off[s] >= thi.
CHOCO_DEV int tile_first_tensor(const int64_t* off, int nt, int64_t tile, int64_t& tlo, int64_t& thi) {
  tlo = i64max(tile * kPbTile, off[0]);
  thi = i64min((tile + 1) * kPbTile, off[nt]);
  if (tlo >= thi) return -1;
  int lo = 1, hi = nt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] > tlo) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

}  // namespace choco
