// Device helpers shared by the two QSGD quantizers: the per-tensor L2-norm one (qsgd.hip) and
// the bucketed max-norm one (qsgd_bucket.hip).  Both write the same level and sign planes
// (one CW-bit container per element, one sign bit per element, 8-element groups), divide with
// the same correctly rounded quotient and draw the same uniform stream per element.
#pragma once

#include "choco_common.h"

namespace choco {

constexpr int kQThreads = 256;
constexpr int kQPer = 8;                         // elements per thread in the quantize/decode passes
constexpr int kQTile = kQThreads * kQPer;        // 2048
constexpr int kQMaxMsg = kMaxMsg;

static int container_bits(int q) {
  int cw = 1;
  while (cw < q) cw <<= 1;
  return cw;
}

static int64_t plane_bytes(int64_t n, int cw) { return (int64_t)align_up((size_t)((n + 7) / 8) * cw, 16); }

template <int CW>
CHOCO_DEV void store_levels(uint8_t* __restrict__ plane, int64_t t, const uint32_t (&lv)[kQPer]) {
  if (CW == 16) {
    uint4 v;
    v.x = lv[0] | (lv[1] << 16);
    v.y = lv[2] | (lv[3] << 16);
    v.z = lv[4] | (lv[5] << 16);
    v.w = lv[6] | (lv[7] << 16);
    reinterpret_cast<uint4*>(plane)[t] = v;
  } else {
    uint64_t acc = 0;
#pragma unroll
    for (int c = 0; c < kQPer; ++c) acc |= (uint64_t)lv[c] << (c * CW);
    if (CW == 8) reinterpret_cast<uint64_t*>(plane)[t] = acc;
    if (CW == 4) reinterpret_cast<uint32_t*>(plane)[t] = (uint32_t)acc;
    if (CW == 2) reinterpret_cast<uint16_t*>(plane)[t] = (uint16_t)acc;
    if (CW == 1) plane[t] = (uint8_t)acc;
  }
}

// A group's packed levels as loaded (CW * 8 bits: 1 to 4 words) and one level of them: the
// fused receive keeps the packed form in registers (8 unpacked levels per message and group
// did not fit).
template <int CW>
struct LevelWords {
  uint32_t w[CW == 16 ? 4 : (CW == 8 ? 2 : 1)];
};
template <int CW>
CHOCO_DEV LevelWords<CW> load_level_words(const uint8_t* __restrict__ plane, int64_t t) {
  LevelWords<CW> r;
  if (CW == 16) {
    const uint4 v = reinterpret_cast<const uint4*>(plane)[t];
    r.w[0] = v.x; r.w[CW == 16 ? 1 : 0] = v.y; r.w[CW == 16 ? 2 : 0] = v.z; r.w[CW == 16 ? 3 : 0] = v.w;
  } else if (CW == 8) {
    const uint2 v = reinterpret_cast<const uint2*>(plane)[t];
    r.w[0] = v.x; r.w[CW == 8 ? 1 : 0] = v.y;
  } else if (CW == 4) {
    r.w[0] = reinterpret_cast<const uint32_t*>(plane)[t];
  } else if (CW == 2) {
    r.w[0] = reinterpret_cast<const uint16_t*>(plane)[t];
  } else {
    r.w[0] = plane[t];
  }
  return r;
}
template <int CW>
CHOCO_DEV uint32_t level_of(const LevelWords<CW>& r, int c) {
  const int bit = c * CW;
  return (r.w[bit >> 5] >> (bit & 31)) & ((CW == 16 ? 0x10000u : (1u << CW)) - 1u);
}

template <int CW>
CHOCO_DEV void load_levels(const uint8_t* __restrict__ plane, int64_t t, uint32_t (&lv)[kQPer]) {
  if (CW == 16) {
    const uint4 v = reinterpret_cast<const uint4*>(plane)[t];
    lv[0] = v.x & 0xFFFFu; lv[1] = v.x >> 16;
    lv[2] = v.y & 0xFFFFu; lv[3] = v.y >> 16;
    lv[4] = v.z & 0xFFFFu; lv[5] = v.z >> 16;
    lv[6] = v.w & 0xFFFFu; lv[7] = v.w >> 16;
  } else {
    uint64_t acc = 0;
    if (CW == 8) acc = reinterpret_cast<const uint64_t*>(plane)[t];
    if (CW == 4) acc = reinterpret_cast<const uint32_t*>(plane)[t];
    if (CW == 2) acc = reinterpret_cast<const uint16_t*>(plane)[t];
    if (CW == 1) acc = plane[t];
    const uint32_t mask = (1u << CW) - 1u;
#pragma unroll
    for (int c = 0; c < kQPer; ++c) lv[c] = (uint32_t)(acc >> (c * CW)) & mask;
  }
}

// s * |d| / norm, correctly rounded, without the IEEE division expansion per
// element.  With y = RN(1/norm) (one real division per thread) and q0 = RN(t * y)
// (within one ulp of t / norm), r = fma(-q0, norm, t) is exact and
// RN(q0 + r * y) is RN(t / norm) (Markstein's theorem) as long as nothing
// underflows or overflows: the fast form is taken for norm in [2^-30, 2^96] and
// q0 in [2^-60, 2^7] (then t >= 2^-90 and r stays normal), zeros give +0 as
// 0/norm does, and everything else (tiny quotients, NaN/inf, extreme norms, a
// pinned norm below |d|) takes the real division.  Checked against fp32 division on 3e9 (t, norm) pairs (random over
// the guarded range + exhaustive t for 12 norm mantissas) and bit-exact against
// the oracle in the GPU tests.
struct QDiv {
  float norm, y;
  bool fast;
  uint32_t tlo_m1;  // bits(T_lo) - 1, T_lo = 2^-60 norm (1 + 2^-20): t >= T_lo implies q0 >= 2^-60
  CHOCO_DEV void init(float nrm) {
    norm = nrm;
    y = 1.0f / nrm;
    fast = nrm >= 0x1p-30f && nrm <= 0x1p96f;
    tlo_m1 = __float_as_uint(nrm * 0x1.00001p-60f) - 1u;
  }
  // The guard, per 8-element group: instead of testing every element's q0
  // against [2^-60, 2^7] (three compares and four scalar mask operations per element),
  // the group keeps min(bits(t) - 1) and max(bits(q0)) in two VALU ops per element and
  // tests them once.  Conservative: t != 0 with t < T_lo covers every q0 < 2^-60 (and
  // some above it), bits(q0) > bits(2^7) covers q0 > 2^7, inf and NaN; a flagged group
  // takes the IEEE division for all its elements, so the result is the same as a per-element
  // guard's (q0 in [2^-60, 2^7] or t == 0, norm in range).
  CHOCO_DEV float quot_nocheck(float t, uint32_t& tmin_m1, uint32_t& qmax) const {
    const float q0 = t * y;
    const float r = fmaf(-q0, norm, t);
    tmin_m1 = min(tmin_m1, __float_as_uint(t) - 1u);
    qmax = max(qmax, __float_as_uint(q0));
    return fmaf(r, y, q0);
  }
  CHOCO_DEV bool group_slow(uint32_t tmin_m1, uint32_t qmax) const {
    return !fast || tmin_m1 < tlo_m1 || qmax > 0x43000000u;
  }
};

// The container value of a level: NaN -> 0, levels >= s -> s (a pinned norm below
// |d|), as one branch-free clamp (fmaxf(NaN, 0) = 0); levels are >= 0 and integral.
CHOCO_DEV uint32_t level_code(float lvl, float sf) { return (uint32_t)fminf(fmaxf(lvl, 0.0f), sf); }

// One quantized element: level (clamped container value, 0 for NaN), sign bit.
CHOCO_DEV float qlevel(float lf, float u) {
  const float pl = floorf(lf);                                // previous_level
  return pl + ((u < (lf - pl)) ? 1.0f : 0.0f);                // + is_next_level
}

// A thread's 8-element group as two 16-byte accesses (the bucketed and the MX kernels).
CHOCO_DEV void unpack8(const float4& a, const float4& b, float (&v)[kQPer]) {
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
CHOCO_DEV void load8(const float* p, float (&v)[kQPer]) {
  unpack8(*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4), v);
}
CHOCO_DEV void store8(float* p, const float (&v)[kQPer]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

constexpr int kQG = 4;                                  // groups per thread
// The uniform stream of thread slot t's groups g, g + 1 (g even) of a tile: 16 uniforms
// each, two streams per slot (choco_common.h Xoro128; oracle qsgd_uniforms_at).
CHOCO_DEV uint64_t qstream_id(int64_t tile, int g, uint32_t t) {
  return ((uint64_t)tile << 9) | ((uint64_t)(g >> 1) << 8) | t;
}
constexpr int kQStreamTile = kQThreads * kQPer * kQG;   // 8192 elements per workgroup
static_assert(kQStreamTile == 8192, "the uniform-stream mapping (choco_common.h) assumes 8192-element tiles");

}  // namespace choco
