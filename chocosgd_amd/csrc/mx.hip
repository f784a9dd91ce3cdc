// Block-scaled FP4 / FP8 wire (OCP microscaling, MX) for the CHOCO gossip step on gfx950.
//
// The flat delta d = x - x_hat is cut into blocks of 32 consecutive elements; a block carries
// one E8M0 scale byte (a power of two) and 32 E2M1 (q = 4) or E4M3 (q = 8) codes.  The scale
// exponent is integer arithmetic on the bits of the block maximum, and the rest of a
// quantizer -- the division by the scale, the rounding (nearest even, or stochastic from a
// random operand), the code, its place in a dword -- is ONE v_cvt_scalef32_* instruction per
// two elements (per element for stochastic E4M3).  No quotient, no guard, no clamp, no uniform
// compare, no plane pack: what is left per element is the subtraction and the maximum.
//
// Work split: bucketed QSGD's (qsgd_bucket.hip).  A 256-thread workgroup owns an 8192-element
// tile, thread t the 8-element groups g * 2048 + 8 t (g = 0..3), so the 16-byte loads and the
// per-slot random stream carry over.  A block is then the four lanes of a quad: its maximum is
// two quad_perm DPP steps, with no LDS and no ds_bpermute.  A group's codes are one dword
// (E2M1) or two (E4M3), written by four conversions that each fill one byte or half of a dword,
// and leave as one 4- or 8-byte store.  The tile's 256 scale bytes go through 256 bytes of LDS
// (quad leaders write one byte per row; one barrier per tile) and leave as sixteen 16-byte
// stores: rows are 64 bytes apart on the wire while a wave holds 16 bytes of each, so a gather
// through lane moves would need the same sixteen stores after a chain of DPP / permute steps
// per row, where the LDS stage costs four ds_write_b8 and one barrier that nothing waits at
// for long (every wave reaches it with its loads long consumed).
//
// What the hardware does was pinned on an MI355X ("MX wire"): the scale
// operand divides on the way to FP4 / FP8 and multiplies on the way back, only its exponent
// field counts (field 0 is 2^-127, field 255 decodes every code to NaN); the packed FP4
// conversion puts its first source into the LOW nibble; signs of zeros are kept; fp32
// denormals are neither flushed on input nor on output; E2M1 saturates, E4M3 does not (a
// quotient of 480 or more becomes the NaN code), which the scale rule never lets happen.
//
// Wire: [scale bytes: ceil(n / 32), padded to 16 B | codes: ceil(n q / 8) bytes, padded to 16 B].
// The contract is in include/choco_codec.h.
#include "choco_common.h"
#include "dispatch.h"
#include "qsgd_common.h"

namespace choco {

typedef float mx_f32x2 __attribute__((ext_vector_type(2)));
typedef short mx_i16x2 __attribute__((ext_vector_type(2)));

constexpr int kMxBlock = 32;

// e = E - kBias + (mantissa > kThr) is the smallest exponent with amax <= vmax 2^e:
// vmax = 6 = 1.5 * 2^2 (E2M1), 448 = 1.75 * 2^8 (E4M3).  kWords: dwords of a group's 8 codes.
template <int Q>
struct MxFmt;
template <>
struct MxFmt<4> {
  static constexpr int kBias = 2, kWords = 1;
  static constexpr uint32_t kThr = 0x400000u;
};
template <>
struct MxFmt<8> {
  static constexpr int kBias = 8, kWords = 2;
  static constexpr uint32_t kThr = 0x600000u;
};

// The quantizer half of a kernel: where the message goes and the stream key.
struct MxQuant {
  int64_t n;
  uint64_t seed, offset;
  uint8_t* scales;
  uint8_t* codes;
  float* dense;  // nullable
};

// The messages of a receive.
struct MxMsgs {
  const uint8_t* scales[kQMaxMsg];
  const uint8_t* codes[kQMaxMsg];
  float w[kQMaxMsg];
  int nmsg;
  int self_slot;
};

// The scale byte of a block whose largest key (bits of |d|; NaN and inf sort on top) is kmax:
// e + 127 clamped at 0 (the upper clamp cannot bind: a finite maximum gives at most 253),
// 0xFF for a block that holds an inf or a NaN.
template <int Q>
CHOCO_DEV uint32_t mx_scale_byte(uint32_t kmax) {
  const int t = (int)(kmax >> 23) - MxFmt<Q>::kBias + ((kmax & 0x7FFFFFu) > MxFmt<Q>::kThr ? 1 : 0);
  return kmax >= 0x7F800000u ? 0xFFu : (uint32_t)max(t, 0);
}
CHOCO_DEV float mx_scale(uint32_t byte) { return __uint_as_float(byte << 23); }

// A group's 8 codes of d / scale.  r: the random operands of the conversions (SR), conversion c
// of the group taking half c & 1 (0: high) of word c >> 1 -- four conversions of two elements
// (E2M1), eight of one (E4M3).
template <int Q, bool SR>
CHOCO_DEV void mx_encode(const float (&d)[kQPer], float sc, const uint64_t (&r)[Q / 2], uint32_t (&w)[MxFmt<Q>::kWords]) {
  if constexpr (Q == 4) {
    uint32_t v = 0u;
    if constexpr (SR) {
      // every stochastic conversion writes byte 0 of a zero dword and the bytes are joined by shifts:
      // on the device the SR forms did not keep the other bytes of their destination as the
      // nearest forms do ("MX wire")
      const uint32_t c0 = __builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, mx_f32x2{d[0], d[1]}, (uint32_t)(r[0] >> 32), sc, 0);
      const uint32_t c1 = __builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, mx_f32x2{d[2], d[3]}, (uint32_t)r[0], sc, 0);
      const uint32_t c2 = __builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, mx_f32x2{d[4], d[5]}, (uint32_t)(r[1] >> 32), sc, 0);
      const uint32_t c3 = __builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, mx_f32x2{d[6], d[7]}, (uint32_t)r[1], sc, 0);
      v = (c0 & 0xFFu) | ((c1 & 0xFFu) << 8) | ((c2 & 0xFFu) << 16) | (c3 << 24);
    } else {
      v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, d[0], d[1], sc, 0);
      v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, d[2], d[3], sc, 1);
      v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, d[4], d[5], sc, 2);
      v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, d[6], d[7], sc, 3);
    }
    w[0] = v;
  } else if constexpr (SR) {
    uint32_t c[kQPer];
#pragma unroll
    for (int k = 0; k < kQPer; ++k)
      c[k] = (uint32_t)__builtin_amdgcn_cvt_scalef32_sr_fp8_f32(0, d[k], (uint32_t)(k & 1 ? r[k >> 1] : r[k >> 1] >> 32), sc, 0) & 0xFFu;
    const uint32_t lo = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    const uint32_t hi = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
    w[0] = lo;
    w[MxFmt<Q>::kWords - 1] = hi;
  } else {
    mx_i16x2 lo = {0, 0}, hi = {0, 0};
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(lo, d[0], d[1], sc, false);
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(lo, d[2], d[3], sc, true);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(hi, d[4], d[5], sc, false);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(hi, d[6], d[7], sc, true);
    w[0] = __builtin_bit_cast(uint32_t, lo);
    w[MxFmt<Q>::kWords - 1] = __builtin_bit_cast(uint32_t, hi);
  }
}

// grid[code] * scale of a group's 8 codes: four packed conversions, no table.  Scale field 255
// gives NaN for every code.
template <int Q>
CHOCO_DEV void mx_decode8(const uint32_t (&w)[MxFmt<Q>::kWords], float sc, float (&v)[kQPer]) {
  mx_f32x2 p[4];
  if constexpr (Q == 4) {
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], sc, 0);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], sc, 1);
    p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], sc, 2);
    p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], sc, 3);
  } else {
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], sc, false);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], sc, true);
    p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[MxFmt<Q>::kWords - 1], sc, false);
    p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[MxFmt<Q>::kWords - 1], sc, true);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = p[j].x;
    v[2 * j + 1] = p[j].y;
  }
}

// A group's code words: one 4-byte (E2M1) or 8-byte (E4M3) access at group index t.
template <int Q>
CHOCO_DEV void mx_load_words(const uint8_t* __restrict__ codes, int64_t t, uint32_t (&w)[MxFmt<Q>::kWords]) {
  if constexpr (Q == 4) {
    w[0] = reinterpret_cast<const uint32_t*>(codes)[t];
  } else {
    const uint2 v = reinterpret_cast<const uint2*>(codes)[t];
    w[0] = v.x;
    w[MxFmt<Q>::kWords - 1] = v.y;
  }
}
template <int Q>
CHOCO_DEV void mx_store_words(uint8_t* __restrict__ codes, int64_t t, const uint32_t (&w)[MxFmt<Q>::kWords]) {
  if constexpr (Q == 4)
    reinterpret_cast<uint32_t*>(codes)[t] = w[0];
  else
    reinterpret_cast<uint2*>(codes)[t] = make_uint2(w[0], w[MxFmt<Q>::kWords - 1]);
}

// The elements [e0, e0 + 8) of a buffer of n; FULL: all of them exist (two 16-byte accesses),
// else those past n read as 0 and are not written.
template <bool FULL>
CHOCO_DEV void mx_load8(const float* p, int64_t e0, int64_t n, float (&v)[kQPer]) {
  if constexpr (FULL) {
    load8(p + e0, v);
  } else {
#pragma unroll
    for (int c = 0; c < kQPer; ++c) v[c] = e0 + c < n ? p[e0 + c] : 0.f;
  }
}
template <bool FULL>
CHOCO_DEV void mx_store8(float* p, int64_t e0, int64_t n, const float (&v)[kQPer]) {
  if constexpr (FULL) {
    store8(p + e0, v);
  } else {
#pragma unroll
    for (int c = 0; c < kQPer; ++c)
      if (e0 + c < n) p[e0 + c] = v[c];
  }
}

// The accumulate of one group: for each message in order, x_hat_self += v (self_slot),
// memory += (float)w * v (two roundings).  The messages stay packed until their turn.
template <int Q, int NM>
CHOCO_DEV void mx_recv_group(const MxMsgs& M, const uint32_t (&mw)[NM][MxFmt<Q>::kWords], const uint32_t (&sb)[NM],
                             float (&hv)[kQPer], float (&mv)[kQPer]) {
#pragma unroll
  for (int q = 0; q < NM; ++q) {
    float v[kQPer];
    mx_decode8<Q>(mw[q], mx_scale(sb[q]), v);
#pragma unroll
    for (int c = 0; c < kQPer; ++c) {
      if (q == M.self_slot) hv[c] = hv[c] + v[c];
      const float wv = M.w[q] * v[c];
      mv[c] = mv[c] + wv;
    }
  }
}

// Rows g0 .. g0 + NG - 1 of a tile, everything a kernel does to them: NM messages received into
// x_hat (self) and memory, the consensus step (GS), d = x - x_hat (x alone without XH), the
// block scales into s_sc (the tile's 256 bytes of LDS; mx_flush_scales writes them out), the
// codes and the dense decode.  All of a row's loads are issued before its arithmetic.  Every
// lane of the workgroup runs the quad reduction; with !FULL (the tile that ends the buffer)
// elements past n count as zeros and nothing past n is touched.  g0 is even: a random stream
// spans rows g, g + 1.
template <int Q, bool SR, int NM, int NG, bool XH, bool GS, bool FULL>
CHOCO_DEV void mx_rows(const MxMsgs& M, float* __restrict__ x, float* __restrict__ hat, float* __restrict__ mem,
                       float gamma, const MxQuant& A, int64_t tile, int g0, uint8_t* s_sc) {
  constexpr int RS = kQThreads * kQPer;  // 2048
  constexpr int W = MxFmt<Q>::kWords, NMA = NM > 0 ? NM : 1;
  constexpr bool MEM = GS || NM > 0;
  const int tid = (int)threadIdx.x;
  const int64_t n = A.n;
  const int64_t eb = tile * kQStreamTile + (int64_t)tid * kQPer + (int64_t)g0 * RS;
  float xv[NG][kQPer], hv[XH ? NG : 1][kQPer], mv[MEM ? NG : 1][kQPer];
  uint32_t mw[NG][NMA][W], sb[NG][NMA];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t e0 = eb + g * RS;
    mx_load8<FULL>(x, e0, n, xv[g]);
    if constexpr (XH) mx_load8<FULL>(hat, e0, n, hv[g]);
    if constexpr (MEM) mx_load8<FULL>(mem, e0, n, mv[g]);
#pragma unroll
    for (int q = 0; q < NM; ++q) {
      sb[g][q] = 0u;
#pragma unroll
      for (int k = 0; k < W; ++k) mw[g][q][k] = 0u;
      if (FULL || e0 < n) {
        mx_load_words<Q>(M.codes[q], e0 / kQPer, mw[g][q]);
        sb[g][q] = M.scales[q][e0 / kMxBlock];
      }
    }
  }
  Xoro128 rng;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t e0 = eb + g * RS;
    const bool some = FULL || e0 < n;
    if constexpr (NM > 0) {
      mx_recv_group<Q, NM>(M, mw[g], sb[g], hv[g], mv[g]);
      mx_store8<FULL>(mem, e0, n, mv[g]);
      if (M.self_slot >= 0) mx_store8<FULL>(hat, e0, n, hv[g]);
    }
    float d[kQPer];
    uint32_t kmax = 0u;
#pragma unroll
    for (int c = 0; c < kQPer; ++c) {
      if constexpr (GS) xv[g][c] = gossip1(xv[g][c], mv[g][c], hv[g][c], gamma);
      if constexpr (XH) d[c] = xv[g][c] - hv[g][c]; else d[c] = xv[g][c];
      if (!FULL && e0 + c >= n) d[c] = 0.f;
      kmax = max(kmax, fkey(d[c]));
    }
    if constexpr (GS) mx_store8<FULL>(x, e0, n, xv[g]);
    kmax = max(kmax, dpp_u32<0xB1>(kmax));  // quad_perm [1, 0, 3, 2]
    kmax = max(kmax, dpp_u32<0x4E>(kmax));  // quad_perm [2, 3, 0, 1]: the block's four lanes
    const uint32_t byte = mx_scale_byte<Q>(kmax);
    if ((tid & 3) == 0) s_sc[(g0 + g) * (RS / kMxBlock) + (tid >> 2)] = (uint8_t)byte;
    uint64_t r[Q / 2];
    if constexpr (SR) {
      if (((g0 + g) & 1) == 0) rng.seed(qrng_key(A.seed, A.offset), qstream_id(tile, g0 + g, tid));
#pragma unroll
      for (int k = 0; k < Q / 2; ++k) r[k] = rng.next();
    }
    const float sc = mx_scale(byte);
    uint32_t w[W];
    mx_encode<Q, SR>(d, sc, r, w);
    // a zero block (and one below 2^-127's reach) and a non-finite one send zero codes
    const bool live = byte != 0u && byte != 0xFFu;
#pragma unroll
    for (int k = 0; k < W; ++k) w[k] = live ? w[k] : 0u;
    if (some) mx_store_words<Q>(A.codes, e0 / kQPer, w);
    if (A.dense) {
      float o[kQPer];
      mx_decode8<Q>(w, sc, o);
      mx_store8<FULL>(A.dense, e0, n, o);
    }
  }
}

// The tile's scale bytes out of LDS: sixteen 16-byte stores.  The last tile of a ragged buffer
// stops at the scales' padded end (the bytes of blocks past n are zeros) and also zeroes the
// padding behind the codes.
template <int Q, bool FULL>
CHOCO_DEV void mx_flush_scales(const MxQuant& A, int64_t tile, const uint8_t* s_sc) {
  constexpr int TB = kQStreamTile / kMxBlock;  // 256 bytes
  const int tid = (int)threadIdx.x;
  __syncthreads();
  if (tid < TB / 16) {
    const int64_t off = tile * TB + tid * 16;
    const int64_t end = FULL ? off + 16 : ((A.n + kMxBlock - 1) / kMxBlock + 15) / 16 * 16;
    if (off < end) *reinterpret_cast<uint4*>(A.scales + off) = reinterpret_cast<const uint4*>(s_sc)[tid];
  }
  if constexpr (!FULL) {
    const int64_t used = (A.n + kQPer - 1) / kQPer * Q, padded = ((A.n * Q + 7) / 8 + 15) / 16 * 16;
    for (int64_t b = used + tid; b < padded; b += kQThreads) A.codes[b] = 0;
  }
}

// ---------------------------------------------------------------- 1: the one-pass compressor
// MODE 0: d = x; 1: d = x - x_hat; 2: the consensus step first (x written back).  All four
// rows' loads are in flight before any arithmetic.
template <int Q, bool SR, int MODE>
__global__ __launch_bounds__(kQThreads) void mx_quant_kernel(float* __restrict__ x, const float* __restrict__ xh,
                                                             Gossip gs, MxQuant A) {
  __shared__ __attribute__((aligned(16))) uint8_t s_sc[kQStreamTile / kMxBlock];
  const int64_t tile = blockIdx.x;
  MxMsgs none{};
  none.self_slot = -1;
  float* hat = const_cast<float*>(xh);
  float* mem = const_cast<float*>(gs.mem);
  if (__builtin_expect((tile + 1) * kQStreamTile > A.n, 0)) {
    mx_rows<Q, SR, 0, kQG, (MODE >= 1), (MODE == 2), false>(none, x, hat, mem, gs.gamma, A, tile, 0, s_sc);
    mx_flush_scales<Q, false>(A, tile, s_sc);
    return;
  }
  mx_rows<Q, SR, 0, kQG, (MODE >= 1), (MODE == 2), true>(none, x, hat, mem, gs.gamma, A, tile, 0, s_sc);
  mx_flush_scales<Q, true>(A, tile, s_sc);
}

// ---------------------------------------------------------------- 2: the receiver
// A workgroup takes 2048 elements, a thread one 8-element group: one code access and one scale
// byte per message (the same byte for the four lanes of a block).
template <int Q>
__global__ __launch_bounds__(kQThreads) void mx_decode_kernel(const uint8_t* __restrict__ scales,
                                                              const uint8_t* __restrict__ codes, int64_t n,
                                                              float* __restrict__ out) {
  const int64_t e0 = (int64_t)blockIdx.x * kQTile + (int64_t)threadIdx.x * kQPer;
  if (e0 >= n) return;
  uint32_t w[MxFmt<Q>::kWords];
  mx_load_words<Q>(codes, e0 / kQPer, w);
  float v[kQPer];
  mx_decode8<Q>(w, mx_scale(scales[e0 / kMxBlock]), v);
  if (e0 + kQPer <= n) mx_store8<true>(out, e0, n, v); else mx_store8<false>(out, e0, n, v);
}

template <int Q, int NM>
__global__ __launch_bounds__(kQThreads) void mx_accumulate_kernel(MxMsgs M, int64_t n, float* __restrict__ hat,
                                                                  float* __restrict__ mem) {
  const int64_t e0 = (int64_t)blockIdx.x * kQTile + (int64_t)threadIdx.x * kQPer;
  if (e0 >= n) return;
  const bool full = e0 + kQPer <= n, has_self = M.self_slot >= 0;
  float mv[kQPer], hv[kQPer];
#pragma unroll
  for (int c = 0; c < kQPer; ++c) hv[c] = 0.f;
  if (full) mx_load8<true>(mem, e0, n, mv); else mx_load8<false>(mem, e0, n, mv);
  if (has_self) {
    if (full) mx_load8<true>(hat, e0, n, hv); else mx_load8<false>(hat, e0, n, hv);
  }
  uint32_t mw[NM][MxFmt<Q>::kWords], sb[NM];
#pragma unroll
  for (int q = 0; q < NM; ++q) {
    mx_load_words<Q>(M.codes[q], e0 / kQPer, mw[q]);
    sb[q] = M.scales[q][e0 / kMxBlock];
  }
  mx_recv_group<Q, NM>(M, mw, sb, hv, mv);
  if (full) mx_store8<true>(mem, e0, n, mv); else mx_store8<false>(mem, e0, n, mv);
  if (has_self) {
    if (full) mx_store8<true>(hat, e0, n, hv); else mx_store8<false>(hat, e0, n, hv);
  }
}

// ---------------------------------------------------------------- 3: the whole CHOCO step
// Per element: the accumulate of (2) for the previous step's NM messages, x += gamma (memory -
// x_hat) on the updated values, then (1) on x_new - x_hat_new: the same mx_rows, two rows at a
// time (x, x_hat, memory and NM messages' words are live per row), the scale bytes of both
// halves flushed behind one barrier.
template <int Q, bool SR, int NM>
__global__ __launch_bounds__(kQThreads) void mx_recv_gossip_quant_kernel(MxMsgs M, float* __restrict__ x,
                                                                         float* __restrict__ hat,
                                                                         float* __restrict__ mem, float gamma,
                                                                         MxQuant A) {
  __shared__ __attribute__((aligned(16))) uint8_t s_sc[kQStreamTile / kMxBlock];
  constexpr int NG = 2;
  const int64_t tile = blockIdx.x;
  if (__builtin_expect((tile + 1) * kQStreamTile > A.n, 0)) {
    for (int g0 = 0; g0 < kQG; g0 += NG) mx_rows<Q, SR, NM, NG, true, true, false>(M, x, hat, mem, gamma, A, tile, g0, s_sc);
    mx_flush_scales<Q, false>(A, tile, s_sc);
    return;
  }
#pragma unroll
  for (int g0 = 0; g0 < kQG; g0 += NG) mx_rows<Q, SR, NM, NG, true, true, true>(M, x, hat, mem, gamma, A, tile, g0, s_sc);
  mx_flush_scales<Q, true>(A, tile, s_sc);
}

// ---------------------------------------------------------------- host side
static int64_t mx_scale_bytes(int64_t n) { return (int64_t)align_up((size_t)((n + kMxBlock - 1) / kMxBlock), 16); }
static int64_t mx_code_bytes(int64_t n, int q) { return (int64_t)align_up((size_t)((n * q + 7) / 8), 16); }
static int64_t mx_message_bytes(int64_t n, int q) { return mx_scale_bytes(n) + mx_code_bytes(n, q); }

static int check_mx(int64_t n, int32_t q) {
  CHOCO_REQUIRE(n > 0 && n < (int64_t)INT32_MAX, "n out of range");
  CHOCO_REQUIRE(q == 4 || q == 8, "MX quantize level q must be 4 (E2M1) or 8 (E4M3), got %d", q);
  return CHOCO_OK;
}

template <typename F>
static int dispatch_mx(int32_t q, int32_t sr, F&& f) {
  return dispatch_list<4, 8>(q, "MX quantize level", [&](auto Q) {
    return dispatch_bool(sr != 0, [&](auto SR) { return f(Q, SR); });
  });
}

static int make_mx_quant(MxQuant& A, int64_t n, int32_t q, uint64_t seed, uint64_t offset, uint8_t* message,
                         float* dense_out, const float* x, const float* xhat, const float* mem) {
  CHOCO_REQUIRE(message, "null pointer argument");
  CHOCO_REQUIRE(aligned16(message) && aligned16(dense_out), "buffers must be 16-byte aligned");
  const int64_t mb = mx_message_bytes(n, q);
  CHOCO_REQUIRE(!overlaps(message, mb, x, 4 * n) && !overlaps(message, mb, xhat, 4 * n) &&
                    !overlaps(message, mb, mem, 4 * n),
                "the message aliases (overlaps) x, x_hat or memory");
  A.n = n;
  A.seed = seed;
  A.offset = offset;
  A.scales = message;
  A.codes = message + mx_scale_bytes(n);
  A.dense = dense_out;
  return CHOCO_OK;
}

static int make_mx_msgs(MxMsgs& M, const uint8_t* const* messages, const float* weights, int32_t nmsg,
                        int32_t self_slot, int64_t n) {
  for (int m = 0; m < nmsg; ++m) {
    CHOCO_REQUIRE(messages[m], "null message pointer");
    CHOCO_REQUIRE(aligned16(messages[m]), "messages must be 16-byte aligned");
    M.scales[m] = messages[m];
    M.codes[m] = messages[m] + mx_scale_bytes(n);
    M.w[m] = weights[m];
  }
  M.nmsg = nmsg;
  M.self_slot = self_slot;
  return CHOCO_OK;
}

static int mx_compress(float* x, const float* xhat, int64_t n, int32_t q, int32_t sr, uint64_t seed, uint64_t offset,
                       uint8_t* message, float* dense_out, hipStream_t st, Gossip gs) {
  CHOCO_REQUIRE(x, "null pointer argument");
  CHOCO_TRY(check_mx(n, q));
  CHOCO_REQUIRE(aligned16(x) && aligned16(xhat) && aligned16(gs.mem), "buffers must be 16-byte aligned");
  MxQuant A{};
  CHOCO_TRY(make_mx_quant(A, n, q, seed, offset, message, dense_out, x, xhat, gs.mem));
  const unsigned grid = (unsigned)((n + kQStreamTile - 1) / kQStreamTile);
  const int mode = gs.mem ? 2 : (xhat ? 1 : 0);
  return dispatch_mx(q, sr, [&](auto Q, auto SR) {
    return dispatch_list<0, 1, 2>(mode, "input form", [&](auto MD) {
      return CHOCO_LAUNCH("mx_quantize", "mx_quant_kernel", (mx_quant_kernel<Q, SR, decltype(MD)::value>), dim3(grid),
                          dim3(kQThreads), st, x, xhat, gs, A);
    });
  });
}

}  // namespace choco

using namespace choco;

CHOCO_API int64_t choco_mx_packed_bytes(int64_t n, int32_t q) {
  if (n <= 0 || n >= (int64_t)INT32_MAX || (q != 4 && q != 8)) return 0;
  return mx_message_bytes(n, q);
}

CHOCO_API int choco_mx_compress(const float* x, const float* xhat, int64_t n, int32_t q, int32_t sr, uint64_t seed,
                                uint64_t offset, uint8_t* message, float* dense_out, void* stream) {
  return mx_compress(const_cast<float*>(x), xhat, n, q, sr, seed, offset, message, dense_out, as_stream(stream),
                     Gossip{nullptr, 0.f});
}

CHOCO_API int choco_gossip_mx_compress(float* x, const float* memory, const float* xhat, float gamma, int64_t n,
                                       int32_t q, int32_t sr, uint64_t seed, uint64_t offset, uint8_t* message,
                                       float* dense_out, void* stream) {
  CHOCO_REQUIRE(memory != nullptr && xhat != nullptr, "the gossip step needs memory and x_hat (null pointer)");
  return mx_compress(x, xhat, n, q, sr, seed, offset, message, dense_out, as_stream(stream), Gossip{memory, gamma});
}

CHOCO_API int choco_mx_decode(const uint8_t* message, int64_t n, int32_t q, float* out, void* stream) {
  CHOCO_REQUIRE(message && out, "null pointer argument");
  CHOCO_TRY(check_mx(n, q));
  CHOCO_REQUIRE(aligned16(message) && aligned16(out), "buffers must be 16-byte aligned");
  const unsigned grid = (unsigned)((n + kQTile - 1) / kQTile);
  return dispatch_list<4, 8>(q, "MX quantize level", [&](auto Q) {
    return CHOCO_LAUNCH(nullptr, "mx_decode_kernel", (mx_decode_kernel<Q>), dim3(grid), dim3(kQThreads),
                        as_stream(stream), message, message + mx_scale_bytes(n), n, out);
  });
}

CHOCO_API int choco_mx_decompress_accumulate(const uint8_t* const* messages, const float* weights, int32_t nmsg,
                                             int32_t self_slot, int64_t n, int32_t q, float* xhat_self,
                                             float* memory, void* stream) {
  CHOCO_REQUIRE(messages && weights && memory, "null pointer argument");
  CHOCO_TRY(check_msgs(nmsg, self_slot));
  CHOCO_TRY(check_mx(n, q));
  CHOCO_REQUIRE(aligned16(memory) && aligned16(xhat_self), "buffers must be 16-byte aligned");
  if (!xhat_self) self_slot = -1;
  MxMsgs M{};
  CHOCO_TRY(make_mx_msgs(M, messages, weights, nmsg, self_slot, n));
  const unsigned grid = (unsigned)((n + kQTile - 1) / kQTile);
  return dispatch_list<4, 8>(q, "MX quantize level", [&](auto Q) {
    return dispatch_nmsg(nmsg, [&](auto NM) {
      return CHOCO_LAUNCH("mx_accumulate", "mx_accumulate_kernel", (mx_accumulate_kernel<Q, NM>), dim3(grid),
                          dim3(kQThreads), as_stream(stream), M, n, xhat_self, memory);
    });
  });
}

CHOCO_API int choco_mx_recv_gossip_compress(const uint8_t* const* messages, const float* weights, int32_t nmsg,
                                            int32_t self_slot, float* x, float* memory, float* xhat, float gamma,
                                            int64_t n, int32_t q, int32_t sr, uint64_t seed, uint64_t offset,
                                            uint8_t* message_out, void* stream) {
  CHOCO_REQUIRE(messages && weights && x && memory && xhat, "null pointer argument");
  CHOCO_TRY(check_msgs(nmsg, self_slot));
  CHOCO_TRY(check_mx(n, q));
  CHOCO_REQUIRE(aligned16(x) && aligned16(memory) && aligned16(xhat), "buffers must be 16-byte aligned");
  MxMsgs M{};
  CHOCO_TRY(make_mx_msgs(M, messages, weights, nmsg, self_slot, n));
  MxQuant A{};
  CHOCO_TRY(make_mx_quant(A, n, q, seed, offset, message_out, nullptr, x, xhat, memory));
  const int64_t mb = mx_message_bytes(n, q);
  for (int m = 0; m < nmsg; ++m)
    CHOCO_REQUIRE(!overlaps(message_out, mb, messages[m], mb), "the output message aliases (overlaps) message %d", m);
  const unsigned grid = (unsigned)((n + kQStreamTile - 1) / kQStreamTile);
  return dispatch_mx(q, sr, [&](auto Q, auto SR) {
    return dispatch_nmsg(nmsg, [&](auto NM) {
      return CHOCO_LAUNCH("mx_step", "mx_recv_gossip_quant_kernel", (mx_recv_gossip_quant_kernel<Q, SR, NM>),
                          dim3(grid), dim3(kQThreads), as_stream(stream), M, x, xhat, memory, gamma, A);
    });
  });
}
