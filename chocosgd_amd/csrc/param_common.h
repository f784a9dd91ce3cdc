// Helpers shared by the kernels that walk a table of parameter tensors in the kernel arguments
// (params.hip: pack / unpack / the scaled pack; sgd.hip: the SGD updates; gradnorm.hip: the
// gradient norms beside them; ef.hip: the error-feedback lines; mix.hip: the neighbour-weighted
// model mix; consensus.hip: the averaged model and the distance to it; mask.hip: DGC's masking,
// which walks the slot space the same way).
//   device  the tile geometry, the SGD table's flag bits, the 16-bit conversions (the stochastic
//           bf16 rounding among them), the 16-byte non-temporal store, the element / group moves
//           and their stochastically rounded stores; the tile walk and its search
//           (tile_walk), the dtype switch (for_dtype), the 16-byte congruence rule (mis16,
//           on_grid16) and the one-group-in-flight span walk (span_walk)
//   host    the layout's argument check (layout_check), the chunk loop with the table's offsets
//           and the launch geometry (for_chunks), the launch count (chunk_launches)
// span_walk's bodies: sgd.hip SgdBody (the master and flat-gradient updates), mix.hip MixBody.
// Deliberately not on it: the loads-ahead span walks (params.hip param_span, sgd.hip plain_span,
// gradnorm.hip norm_vector), consensus.hip's thread-owned groups (cons_span) and ef.hip's
// ef_span, which measured slower on it in one of its three modes; each says why.
#pragma once

#include <algorithm>

#include "choco_common.h"
#include "dispatch.h"

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
// Stochastic rounding of v to bf16 with the 16 random bits r16 (< 65536): the add carries into
// the kept half with probability low16 / 65536.
//   * a value already representable in bf16 (low16 == 0) is unchanged for every r16
//   * the result is always the truncation or its successor in magnitude (the sign bit is not
//     touched: bf16 is sign-magnitude)
//   * P(successor) = low16 / 65536, also across a binade boundary, where the carry runs from
//     the mantissa into the exponent and lands on the next binade's first value
//   * +-0 and subnormals need no special case: the bit pattern is monotone in the magnitude
//   * a finite value above the largest finite bf16 may round to inf, as rounding up past it does
// inf and NaN go through bf16_narrow (inf kept, quiet NaN): the add would walk off them.
CHOCO_DEV unsigned short bf16_narrow_sr(float v, uint32_t r16) {
  const uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) >= 0x7f800000u) return bf16_narrow(v);
  return (unsigned short)((u + r16) >> 16);
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

// The stochastically rounded stores of a bf16 tensor (choco_common.h sr_word): element j of the
// tensor is flat element i; a whole group starts at a flat index e that is a multiple of 8 and
// costs two mixes, a single element one.
CHOCO_DEV void st1_sr(void* base, int64_t j, float v, uint64_t key, int64_t i) {
  reinterpret_cast<unsigned short*>(base)[j] = bf16_narrow_sr(v, sr_bits16(sr_word(key, i), i));
}
CHOCO_DEV void st8_sr(void* base, int64_t j, const float (&v)[8], uint64_t key, int64_t e) {
  const uint64_t w0 = sr_word(key, e), w1 = sr_word(key, e + 4);
  choco_u16x8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = bf16_narrow_sr(v[k], sr_bits16(k < 4 ? w0 : w1, k));
  __builtin_nontemporal_store(o, reinterpret_cast<choco_u16x8*>(reinterpret_cast<unsigned short*>(base) + j));
}

// ---------------------------------------------------------------- the dtype switch
// a CHOCO_DT_* code's element size
__host__ __device__ inline uintptr_t dtype_size(int dt) { return dt == CHOCO_DT_F32 ? 4u : 2u; }

// f(int_c<DT>) for the dtype code dt
template <typename F>
CHOCO_DEV void for_dtype(int dt, F&& f) {
  if (dt == CHOCO_DT_F32) f(int_c<CHOCO_DT_F32>{});
  else if (dt == CHOCO_DT_BF16) f(int_c<CHOCO_DT_BF16>{});
  else f(int_c<CHOCO_DT_F16>{});
}

// ---------------------------------------------------------------- the tile walk
// Workgroup `tile` owns flat elements [tile * tlen, (tile + 1) * tlen) cut to the chunk
// [off[0], off[nt]) of a launch's table: [tlo, thi).  Returns the first tensor that can hold
// an element of it, found by a uniform upper-bound search (the first s in [1, nt] with
// off[s] > tlo, off[nt] >= thi > tlo: tensor s - 1 holds tlo; zero-length tensors give equal
// offsets and are passed over), or -1 for an empty range.
CHOCO_DEV int tile_first_tensor(const int64_t* off, int nt, int64_t tile, int64_t& tlo, int64_t& thi,
                                int64_t tlen = kPbTile) {
  tlo = i64max(tile * tlen, off[0]);
  thi = i64min((tile + 1) * tlen, off[nt]);
  if (tlo >= thi) return -1;
  int lo = 1, hi = nt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] > tlo) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

// f(s, a, b) for every tensor s of the table that has elements [a, b), a < b, in workgroup
// `tile`'s share of the chunk, in ascending s.  s is workgroup-uniform, so f reads its table
// with scalar loads; f may hold barriers.
template <typename F>
CHOCO_DEV void tile_walk(const int64_t* off, int nt, int64_t tile, F&& f, int64_t tlen = kPbTile) {
  int64_t tlo, thi;
  const int s0 = tile_first_tensor(off, nt, tile, tlo, thi, tlen);
  if (s0 < 0) return;
  for (int s = s0; s < nt; ++s) {
    const int64_t o0 = off[s];
    if (o0 >= thi) break;
    const int64_t a = i64max(o0, tlo), b = i64min(off[s + 1], thi);
    if (a < b) f(s, a, b);  // a zero-length tensor is passed over
  }
}

// ---------------------------------------------------------------- the 16-byte rule
// Is every whole group's start 16-byte aligned on a side of a tensor at flat offset o0?  Groups
// start at flat indices e that are multiples of 8.  A flat side, base + 4 e, is aligned at every
// one when the base is: the kernel's own test, made once on the host.  A tensor's side,
// q + esz (e - o0), is when q - esz o0 is, esz e being a multiple of 16 -- esz the side's own
// element size.  mis16 is that difference; a kernel ors the sides it touches and takes the
// 16-byte path when the low four bits of all of them are clear (on_grid16).
CHOCO_DEV uintptr_t mis16(const void* q, uintptr_t esz, int64_t o0) {
  return reinterpret_cast<uintptr_t>(q) - esz * (uintptr_t)o0;
}
CHOCO_DEV bool on_grid16(uintptr_t mis) { return (mis & 15u) == 0; }

// ---------------------------------------------------------------- the span walk
// Flat elements [a, b) of a tensor, a < b inside this workgroup's tile.  vec: every side the
// body touches is 16-byte aligned at every whole group's start.  One 8-element group in flight
// per thread; the body supplies elem(i), one element at flat index i, and group(e), one whole
// group at flat index e, every load issued before the first store.  A group's loads and its
// update stand under ONE test, so that the group path and the element path exclude each other:
// with the loads in a phase of their own, ahead of the element path, the SGD kernels take 8 to 16
// VGPRs more and lose a wave of occupancy.
template <typename BODY>
CHOCO_DEV void span_walk(const BODY& body, int64_t a, int64_t b, bool vec) {
  const int tid = threadIdx.x;
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) body.elem(i);
    return;
  }
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += kPbThreads) {
    const int64_t e = (gb + tid) * kPbGroup;
    if (e >= a && e + kPbGroup <= b) {
      body.group(e);
    } else {
      // a group cut by the tensor's start or end (or past the span): its own elements only
      const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
      for (int64_t i = ea; i < eb; ++i) body.elem(i);
    }
  }
}

// ---------------------------------------------------------------- the host side
// The layout of a call: nseg tensors of lens[s] elements and dtype code dtypes[s], n elements in
// all.  Checked in this order: nseg and n; own(), the caller's other arguments; per tensor its
// length, dtype code and the running sum against n, then per_tensor(s, esz), the caller's
// pointer and flag checks for tensor s of element size esz; the sum against n.  A failing call
// reports the first check that fails in that order.  Within per_tensor the order of a null test
// and an alignment test of the same pointer is free: a null pointer is aligned and a misaligned
// one is not null, so the two cannot both fire.  `lengths` is how the two sum messages name lens
// (the consensus entry point's say "lengths (lens)", and its host test asks for that).
inline int layout_head(int32_t nseg, int64_t n) {
  CHOCO_REQUIRE(nseg > 0, "nseg must be positive, got %d", (int)nseg);
  CHOCO_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "n must be in [0, 2^31), got %lld", (long long)n);
  return CHOCO_OK;
}
template <typename OWN, typename F>
int layout_check(const int64_t* lens, const int32_t* dtypes, int32_t nseg, int64_t n, OWN&& own, F&& per_tensor,
                 const char* lengths = "lengths") {
  CHOCO_TRY(layout_head(nseg, n));
  CHOCO_TRY(own());
  int64_t sum = 0;
  for (int32_t s = 0; s < nseg; ++s) {
    CHOCO_REQUIRE(lens[s] >= 0, "tensor %d: negative length", (int)s);
    CHOCO_REQUIRE(dtypes[s] >= CHOCO_DT_F32 && dtypes[s] <= CHOCO_DT_F16, "tensor %d: unknown dtype code %d", (int)s,
                  (int)dtypes[s]);
    CHOCO_REQUIRE(lens[s] <= n - sum, "the %s add up to more than n = %lld", lengths, (long long)n);
    sum += lens[s];
    CHOCO_TRY(per_tensor(s, dtype_size(dtypes[s])));
  }
  CHOCO_REQUIRE(sum == n, "the %s add up to %lld, n is %lld", lengths, (long long)sum, (long long)n);
  return CHOCO_OK;
}

// One launch's share of a layout: tensors [s0, s0 + nt), whose first element is at `base` of the
// space the grid walks; workgroups tile0 .. tile0 + tiles - 1.
struct Chunk {
  int32_t s0;
  int nt;
  int64_t base, tile0, tiles;
};

// off[0 .. CAP] = the absolute offsets of the chunk's tensors, from `base` (the rows past nt
// repeat the end); returns the next chunk's base
template <int CAP>
int64_t chunk_offsets(const int64_t* lens, int32_t s0, int nt, int64_t base, int64_t (&off)[CAP + 1]) {
  off[0] = base;
  for (int i = 0; i < CAP; ++i) {
    base += i < nt ? lens[s0 + i] : 0;
    off[i + 1] = base;
  }
  return base;
}

// f(chunk) for every CAP tensors of the layout, with the table's offsets filled in: off is the
// array the kernel's tile walk runs over, tlen its tile.  The caller fills the other rows.  A
// chunk takes the tiles [off[0], off[nt]) touches; an empty chunk still takes its launch, of one
// workgroup that finds nothing.
template <int CAP, typename F>
int for_chunks(const int64_t* lens, int32_t nseg, int64_t (&off)[CAP + 1], F&& f, int64_t tlen = kPbTile) {
  int64_t base = 0;
  for (int32_t s0 = 0; s0 < nseg; s0 += CAP) {
    Chunk c;
    c.s0 = s0;
    c.nt = std::min<int32_t>(CAP, nseg - s0);
    c.base = base;
    base = chunk_offsets<CAP>(lens, s0, c.nt, base, off);
    c.tile0 = off[0] / tlen;
    c.tiles = off[c.nt] > off[0] ? (off[c.nt] - 1) / tlen - c.tile0 + 1 : 1;
    CHOCO_TRY(f(c));
  }
  return CHOCO_OK;
}

inline int chunk_launches(int32_t nseg, int cap) { return nseg <= 0 ? 0 : (nseg + cap - 1) / cap; }

}  // namespace choco
