// Bucketed QSGD for the CHOCO gossip step on MI355X: the practical variant of the QSGD paper
// (Alistarh et al. 2017, section 4 and the experiments): the flat buffer is cut into buckets
// of B = 128 .. 2048 elements and every bucket is scaled by its own MAXIMUM |d|.
//
// A bucket's scale is known as soon as the wave(s) that loaded it have reduced it, so the
// compressor is ONE pass (the per-tensor quantizer of qsgd.hip needs the tensor's L2 norm
// first: a norm pass, then a quantize pass that reads everything again), and with it the whole
// CHOCO step -- the previous step's receive, the consensus step, this step's message -- is one
// kernel that reads x, x_hat and memory once.  No workspace, no atomics in global memory, no
// last-workgroup ticket; buckets tile the flat buffer, so there is no per-tensor segment code.
//
// Work split: a 256-thread workgroup owns an 8192-element tile, thread t the 8-element groups
// g * 2048 + 8 t (g = 0..3): the planes' groups and the uniform stream of qsgd_quant_kernel,
// unchanged.  Every bucket size divides a 2048-element row, so a bucket is 16 (B = 128), 32,
// 64 (one wave), 128 or 256 consecutive lanes of one row and never straddles a row or a tile:
//   16 lanes   four DPP steps inside the row (quad_perm, quad_perm, row_half_mirror, row_mirror)
//   32, 64     + one / two ds_bpermute butterflies (__shfl_xor 16, 32)
//   128, 256   + the row's four wave maxima through 16 floats of LDS and one barrier
// B is a kernel argument (log2), not a template parameter: the depth of the reduction is a
// scalar branch, and the kernels are instantiated once per container width (and message count)
// as qsgd.hip's are, not five times that.
//
// Wire: [scales: nb fp32, padded to 16 B | level plane | sign plane], the planes exactly those
// of choco_qsgd_packed_bytes(n, q).  The contract is in include/choco_codec.h.
#include "choco_common.h"
#include "dispatch.h"
#include "qsgd_common.h"

#include <algorithm>
#include <math.h>

namespace choco {

// What the quantizer half of every kernel takes.
struct BQuant {
  int64_t n;
  int logb;       // log2 B: 7 .. 11
  int s_levels;   // s = 2^q - 1
  float c;        // 1, or the biased scale 1 / (min(B / s^2, sqrt(B) / s) + 1)
  const float* u_in;
  uint64_t seed, offset;
  float* scales;
  uint8_t* lvl;
  uint8_t* sgn;
  float* dense;   // nullable
};

// The messages of a receive: scales and planes of each, its weight.
struct BMsgs {
  const float* scales[kQMaxMsg];
  const uint8_t* lvl[kQMaxMsg];
  const uint8_t* sgn[kQMaxMsg];
  float w[kQMaxMsg];
  int nmsg;
  int self_slot;
};

// v = +-((c * m_b) * level) / s, left to right, one rounding per operation (cm = c * m_b).
CHOCO_DEV float bdecode(uint32_t level, bool neg, float cm, float sf) {
  const float t = (cm * (float)level) / sf;
  return neg ? -t : t;
}

template <int CTRL>
CHOCO_DEV float dpp_max(float v) {
  return fmaxf(v, __uint_as_float(dpp_u32<CTRL>(__float_as_uint(v))));
}

// The maximum over the min(B, 512) / 8 consecutive lanes of this lane's bucket (every lane of
// the wave active; m is not NaN).  max is idempotent, so mirrored lanes serve as a butterfly.
CHOCO_DEV float bucket_wave_max(float m, int logb) {
  m = dpp_max<0xB1>(m);    // quad_perm [1, 0, 3, 2]
  m = dpp_max<0x4E>(m);    // quad_perm [2, 3, 0, 1]
  m = dpp_max<0x141>(m);   // row_half_mirror: 8 lanes
  m = dpp_max<0x140>(m);   // row_mirror: 16 lanes = 128 elements
  if (logb >= 8) m = fmaxf(m, __shfl_xor(m, 16));
  if (logb >= 9) m = fmaxf(m, __shfl_xor(m, 32));
  return m;
}

// max |d| of a thread's group, NaN elements left out (fmaxf), 0 if there is nothing else
CHOCO_DEV float group_absmax(const float (&d)[kQPer]) {
  float m = 0.0f;
#pragma unroll
  for (int c = 0; c < kQPer; ++c) m = fmaxf(m, fabsf(d[c]));
  return m;
}

// Rows g0 .. g0 + NG - 1 of a FULL tile whose deltas d are in registers: bucket maxima, the
// scale stores, then levels, signs and the dense decode as qsgd.hip's quant_tile_math does
// them (one QDiv::init per bucket and thread).  s_w: NG * 4 floats of LDS that nothing else
// touches during the call (B >= 1024 only; one barrier).  g0 is even: a uniform stream spans
// rows g, g + 1.
template <int CW, int NG, bool UIN>
CHOCO_DEV void bucket_quant_rows(const float (&d)[NG][kQPer], int64_t tile, int g0, const BQuant& A, float* s_w) {
  constexpr int GS = kQThreads * kQPer;  // 2048
  const int tid = (int)threadIdx.x, w = tid >> 6;
  const float sf = (float)A.s_levels;
  float m[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) m[g] = bucket_wave_max(group_absmax(d[g]), A.logb);
  if (A.logb >= 10) {  // workgroup-uniform
    if (lane_id() == 0) {
#pragma unroll
      for (int g = 0; g < NG; ++g) s_w[g * 4 + w] = m[g];
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const float* r = s_w + g * 4;
      m[g] = A.logb == 10 ? fmaxf(r[w & 2], r[(w & 2) + 1]) : fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
    }
  }
  const int64_t eb = tile * kQStreamTile + (int64_t)tid * kQPer + (int64_t)g0 * GS;
  const bool first = ((tid * kQPer) & ((1 << A.logb) - 1)) == 0;  // this lane holds its bucket's first element
  Xoro128 rng;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if constexpr (!UIN) {
      if (((g0 + g) & 1) == 0) rng.seed(qrng_key(A.seed, A.offset), qstream_id(tile, g0 + g, tid));
    }
    const int64_t e0 = eb + g * GS;
    if (first) A.scales[e0 >> A.logb] = m[g];
    QDiv D;
    D.init(m[g]);
    float lf[kQPer];
    uint32_t tmin_m1 = 0xFFFFFFFFu, qmax = 0u;
#pragma unroll
    for (int c = 0; c < kQPer; ++c) lf[c] = D.quot_nocheck(sf * fabsf(d[g][c]), tmin_m1, qmax);  // s * |d| / m_b
    const bool gslow = D.group_slow(tmin_m1, qmax);
    if (__builtin_expect(__ballot(gslow) != 0, 0)) {
#pragma unroll
      for (int c = 0; c < kQPer; ++c)
        if (gslow) lf[c] = (sf * fabsf(d[g][c])) / m[g];
    }
    float u[kQPer];
    if constexpr (UIN) {
      const float4 u0 = *reinterpret_cast<const float4*>(A.u_in + e0);
      const float4 u1 = *reinterpret_cast<const float4*>(A.u_in + e0 + 4);
      u[0] = u0.x; u[1] = u0.y; u[2] = u0.z; u[3] = u0.w;
      u[4] = u1.x; u[5] = u1.y; u[6] = u1.z; u[7] = u1.w;
    } else {
#pragma unroll
      for (int c = 0; c < kQPer; c += 2) rng.next2(u[c], u[c + 1]);
    }
    uint32_t lv[kQPer];
    uint32_t sbits = 0;
#pragma unroll
    for (int c = 0; c < kQPer; ++c) {
      lv[c] = level_code(qlevel(lf[c], u[c]), sf);
      sbits |= d[g][c] < 0.f ? (1u << c) : 0u;
    }
    const int64_t t = e0 / kQPer;
    store_levels<CW>(A.lvl, t, lv);
    A.sgn[t] = (uint8_t)sbits;
    if (A.dense) {  // one branch per group
      const float cm = A.c * m[g];
      float o[kQPer];
#pragma unroll
      for (int c = 0; c < kQPer; ++c) o[c] = bdecode(lv[c], (sbits >> c) & 1u, cm, sf);
      *reinterpret_cast<float4*>(A.dense + e0) = make_float4(o[0], o[1], o[2], o[3]);
      *reinterpret_cast<float4*>(A.dense + e0 + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
  }
}

// The accumulate of one 8-element group: for each message in order, x_hat_self += v
// (self_slot), memory += (float)w * v (two roundings).
template <int CW, int NM>
CHOCO_DEV void recv_group(const BMsgs& M, const LevelWords<CW> (&lw)[NM], const uint32_t (&sb)[NM],
                          const float (&cm)[NM], float sf, float (&hv)[kQPer], float (&mv)[kQPer]) {
#pragma unroll
  for (int q = 0; q < NM; ++q) {
#pragma unroll
    for (int c = 0; c < kQPer; ++c) {
      const float v = bdecode(level_of<CW>(lw[q], c), (sb[q] >> c) & 1u, cm[q], sf);
      if (q == M.self_slot) hv[c] = hv[c] + v;
      const float wv = M.w[q] * v;
      mv[c] = mv[c] + wv;
    }
  }
}

// The tile that ends the buffer (n is no multiple of 8192): a last bucket shorter than B, a
// last 8-group shorter than 8.  Element by element in stream order with the real division,
// whatever the kernel does before the quantizer (NM messages received, the consensus step)
// included; the bucket maxima meet through LDS atomics on the bits of |d| (non-NaN floats
// order as their bits).  It also zeroes the 16-byte padding of the scales and of both planes.
// Cold: one workgroup per launch.  hat == nullptr: d = x; mem is read when NM > 0 or gossip.
template <int CW, int NM>
CHOCO_DEV void bucket_tile_slow(const BMsgs& M, float* x, float* hat, float* mem, float gamma, bool gossip,
                                const BQuant& A, int64_t tile, uint32_t* s_bmax) {
  constexpr int GS = kQThreads * kQPer;
  const int tid = (int)threadIdx.x;
  const int64_t n = A.n;
  const float sf = (float)A.s_levels;
  const int64_t eb = tile * kQStreamTile + (int64_t)tid * kQPer;
  for (int i = tid; i < (kQStreamTile >> A.logb); i += kQThreads) s_bmax[i] = 0u;
  {
    const int64_t groups = (n + kQPer - 1) / kQPer, nb = (n + (1 << A.logb) - 1) >> A.logb;
    for (int64_t b = groups * CW + tid; b < (groups * CW + 15) / 16 * 16; b += kQThreads) A.lvl[b] = 0;
    for (int64_t b = groups + tid; b < (groups + 15) / 16 * 16; b += kQThreads) A.sgn[b] = 0;
    for (int64_t b = nb + tid; b < (nb + 3) / 4 * 4; b += kQThreads) A.scales[b] = 0.0f;
  }
  __syncthreads();
  float d[kQG][kQPer];
#pragma unroll
  for (int g = 0; g < kQG; ++g) {
    const int64_t e0 = eb + (int64_t)g * GS;
    float xv[kQPer], hv[kQPer], mv[kQPer];
#pragma unroll
    for (int c = 0; c < kQPer; ++c) {
      const bool in = e0 + c < n;
      xv[c] = in ? x[e0 + c] : 0.f;
      hv[c] = in && hat ? hat[e0 + c] : 0.f;
      mv[c] = in && (NM > 0 || gossip) ? mem[e0 + c] : 0.f;
    }
    if constexpr (NM > 0) {
      if (e0 < n) {
        LevelWords<CW> lw[NM];
        uint32_t sb[NM];
        float cm[NM];
#pragma unroll
        for (int q = 0; q < NM; ++q) {
          lw[q] = load_level_words<CW>(M.lvl[q], e0 / kQPer);
          sb[q] = M.sgn[q][e0 / kQPer];
          cm[q] = A.c * M.scales[q][e0 >> A.logb];
        }
        recv_group<CW, NM>(M, lw, sb, cm, sf, hv, mv);
      }
    }
    uint32_t key = 0u;
#pragma unroll
    for (int c = 0; c < kQPer; ++c) {
      const bool in = e0 + c < n;
      if (gossip) xv[c] = gossip1(xv[c], mv[c], hv[c], gamma);
      d[g][c] = in ? (hat ? xv[c] - hv[c] : xv[c]) : 0.f;
      if (in) {
        if (gossip) x[e0 + c] = xv[c];
        if (NM > 0) {
          mem[e0 + c] = mv[c];
          if (M.self_slot >= 0) hat[e0 + c] = hv[c];
        }
        const float a = fabsf(d[g][c]);
        if (a == a) key = max(key, __float_as_uint(a));
      }
    }
    if (key) atomicMax(&s_bmax[(g * GS + tid * kQPer) >> A.logb], key);
  }
  __syncthreads();
  Xoro128 rng;
#pragma unroll
  for (int g = 0; g < kQG; ++g) {
    if (!A.u_in && (g & 1) == 0) rng.seed(qrng_key(A.seed, A.offset), qstream_id(tile, g, tid));
    const int64_t e0 = eb + (int64_t)g * GS;
    float u[kQPer];
#pragma unroll
    for (int c = 0; c < kQPer; c += 2) {
      if (!A.u_in) rng.next2(u[c], u[c + 1]);
    }
    if (e0 >= n) continue;
    const float m = __uint_as_float(s_bmax[(g * GS + tid * kQPer) >> A.logb]);
    if (((tid * kQPer) & ((1 << A.logb) - 1)) == 0) A.scales[e0 >> A.logb] = m;
    const float cm = A.c * m;
    uint32_t lv[kQPer];
    uint32_t sbits = 0;
#pragma unroll
    for (int c = 0; c < kQPer; ++c) {
      lv[c] = 0u;
      if (e0 + c >= n) continue;
      if (A.u_in) u[c] = A.u_in[e0 + c];
      lv[c] = level_code(qlevel((sf * fabsf(d[g][c])) / m, u[c]), sf);
      sbits |= d[g][c] < 0.f ? (1u << c) : 0u;
      if (A.dense) A.dense[e0 + c] = bdecode(lv[c], (sbits >> c) & 1u, cm, sf);
    }
    store_levels<CW>(A.lvl, e0 / kQPer, lv);
    A.sgn[e0 / kQPer] = (uint8_t)sbits;
  }
}

// ---------------------------------------------------------------- 1: the one-pass compressor
// XH: d = x - x_hat; GS: the consensus step first (x_new = x + gamma (memory - x_hat) written
// back, d = x_new - x_hat).  All four rows' loads are in flight before any arithmetic.
template <int CW, bool XH, bool GS, bool UIN>
__global__ __launch_bounds__(kQThreads) void qsgd_bucket_quant_kernel(float* __restrict__ x,
                                                                      const float* __restrict__ xh, Gossip gs,
                                                                      BQuant A) {
  static_assert(!GS || XH, "the gossip step needs x_hat");
  __shared__ float s_w[kQG * 4];
  __shared__ uint32_t s_bmax[kQStreamTile / 128];
  constexpr int RS = kQThreads * kQPer;  // 2048
  const int64_t tile = blockIdx.x;
  if (__builtin_expect((tile + 1) * kQStreamTile > A.n, 0)) {
    BMsgs none{};
    none.self_slot = -1;
    bucket_tile_slow<CW, 0>(none, x, const_cast<float*>(xh), const_cast<float*>(gs.mem), gs.gamma, GS, A, tile,
                            s_bmax);
    return;
  }
  const int64_t eb = tile * kQStreamTile + (int64_t)threadIdx.x * kQPer;
  float4 a[kQG][2], h[XH ? kQG : 1][2], mm[GS ? kQG : 1][2];
#pragma unroll
  for (int g = 0; g < kQG; ++g) {
    a[g][0] = *reinterpret_cast<const float4*>(x + eb + g * RS);
    a[g][1] = *reinterpret_cast<const float4*>(x + eb + g * RS + 4);
  }
  if constexpr (XH) {
#pragma unroll
    for (int g = 0; g < kQG; ++g) {
      h[g][0] = *reinterpret_cast<const float4*>(xh + eb + g * RS);
      h[g][1] = *reinterpret_cast<const float4*>(xh + eb + g * RS + 4);
    }
  }
  if constexpr (GS) {
#pragma unroll
    for (int g = 0; g < kQG; ++g) {
      mm[g][0] = *reinterpret_cast<const float4*>(gs.mem + eb + g * RS);
      mm[g][1] = *reinterpret_cast<const float4*>(gs.mem + eb + g * RS + 4);
    }
  }
  float d[kQG][kQPer];
#pragma unroll
  for (int g = 0; g < kQG; ++g) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if constexpr (GS) {
        a[g][k] = gossip4(a[g][k], mm[g][k], h[g][k], gs.gamma);
        *reinterpret_cast<float4*>(x + eb + g * RS + 4 * k) = a[g][k];
      }
      if constexpr (XH) a[g][k] = sub4(a[g][k], h[g][k]);
    }
    unpack8(a[g][0], a[g][1], d[g]);
  }
  bucket_quant_rows<CW, kQG, UIN>(d, tile, 0, A, s_w);
}

// ---------------------------------------------------------------- 2: the receiver
// MODE 0: out (= mem) = decode(message 0); MODE 1: the accumulate of all messages.  A
// workgroup decodes 2048 elements, a thread one 8-element group; the group's scale is one
// load per message (the same address for the 16 .. 64 lanes of a bucket: no segment walk).
template <int CW, int NM, int MODE>
__global__ __launch_bounds__(kQThreads) void qsgd_bucket_decode_kernel(BMsgs M, int64_t n, int logb, int s_levels,
                                                                       float c, float* __restrict__ hat,
                                                                       float* __restrict__ mem) {
  const int64_t e0 = (int64_t)blockIdx.x * kQTile + (int64_t)threadIdx.x * kQPer;
  if (e0 >= n) return;
  const float sf = (float)s_levels;
  const bool full = e0 + kQPer <= n;
  const bool has_self = MODE == 1 && M.self_slot >= 0;
  float mv[kQPer], hv[kQPer];
#pragma unroll
  for (int k = 0; k < kQPer; ++k) mv[k] = hv[k] = 0.f;
  if (MODE == 1) {
    if (full) {
      load8(mem + e0, mv);
      if (has_self) load8(hat + e0, hv);
    } else {
      for (int k = 0; k < kQPer && e0 + k < n; ++k) {
        mv[k] = mem[e0 + k];
        if (has_self) hv[k] = hat[e0 + k];
      }
    }
  }
  LevelWords<CW> lw[NM];
  uint32_t sb[NM];
  float cm[NM];
#pragma unroll
  for (int q = 0; q < NM; ++q) {
    lw[q] = load_level_words<CW>(M.lvl[q], e0 / kQPer);
    sb[q] = M.sgn[q][e0 / kQPer];
    cm[q] = c * M.scales[q][e0 >> logb];
  }
  if (MODE == 0) {
#pragma unroll
    for (int k = 0; k < kQPer; ++k) mv[k] = bdecode(level_of<CW>(lw[0], k), (sb[0] >> k) & 1u, cm[0], sf);
  } else {
    recv_group<CW, NM>(M, lw, sb, cm, sf, hv, mv);
  }
  if (full) {
    store8(mem + e0, mv);
    if (has_self) store8(hat + e0, hv);
  } else {
    for (int k = 0; k < kQPer && e0 + k < n; ++k) {
      mem[e0 + k] = mv[k];
      if (has_self) hat[e0 + k] = hv[k];
    }
  }
}

// ---------------------------------------------------------------- 3: the whole CHOCO step
// Per element: the accumulate of (2) for the previous step's NM messages, x += gamma (memory -
// x_hat) on the updated values, then (1) on x_new - x_hat_new.  Every step is elementwise but
// the bucket maxima, which only the quantizer needs, so the results are those of the three
// calls in sequence.  Two rows at a time (x, x_hat, memory and NM messages' words are live per
// row: four rows did not leave room for resident waves); each half has its own LDS slots.
template <int CW, int NM, bool UIN>
__global__ __launch_bounds__(kQThreads) void qsgd_bucket_recv_gossip_quant_kernel(BMsgs M, float* __restrict__ x,
                                                                                  float* __restrict__ hat,
                                                                                  float* __restrict__ mem,
                                                                                  float gamma, BQuant A) {
  __shared__ float s_w[kQG * 4];
  __shared__ uint32_t s_bmax[kQStreamTile / 128];
  constexpr int RS = kQThreads * kQPer;  // 2048
  constexpr int NG = 2;
  const int64_t tile = blockIdx.x;
  if (__builtin_expect((tile + 1) * kQStreamTile > A.n, 0)) {
    bucket_tile_slow<CW, NM>(M, x, hat, mem, gamma, true, A, tile, s_bmax);
    return;
  }
  const float sf = (float)A.s_levels;
  const bool has_self = M.self_slot >= 0;
#pragma unroll
  for (int g0 = 0; g0 < kQG; g0 += NG) {
    const int64_t eb = tile * kQStreamTile + (int64_t)threadIdx.x * kQPer + (int64_t)g0 * RS;
    float xv[NG][kQPer], hv[NG][kQPer], mv[NG][kQPer];
    LevelWords<CW> lw[NG][NM];
    uint32_t sb[NG][NM];
    float cm[NG][NM];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int64_t e0 = eb + g * RS;
      load8(x + e0, xv[g]);
      load8(hat + e0, hv[g]);
      load8(mem + e0, mv[g]);
#pragma unroll
      for (int q = 0; q < NM; ++q) {
        lw[g][q] = load_level_words<CW>(M.lvl[q], e0 / kQPer);
        sb[g][q] = M.sgn[q][e0 / kQPer];
        cm[g][q] = M.scales[q][e0 >> A.logb];
      }
    }
    float d[NG][kQPer];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int64_t e0 = eb + g * RS;
#pragma unroll
      for (int q = 0; q < NM; ++q) cm[g][q] = A.c * cm[g][q];
      recv_group<CW, NM>(M, lw[g], sb[g], cm[g], sf, hv[g], mv[g]);
#pragma unroll
      for (int c = 0; c < kQPer; ++c) {
        xv[g][c] = gossip1(xv[g][c], mv[g][c], hv[g][c], gamma);
        d[g][c] = xv[g][c] - hv[g][c];
      }
      store8(x + e0, xv[g]);
      store8(mem + e0, mv[g]);
      if (has_self) store8(hat + e0, hv[g]);
    }
    bucket_quant_rows<CW, NG, UIN>(d, tile, g0, A, s_w + g0 * 4);
  }
}

// ---------------------------------------------------------------- host side
static int bucket_log2(int32_t bucket) {
  for (int l = 7; l <= 11; ++l)
    if (bucket == (1 << l)) return l;
  return -1;
}
static int64_t scale_bytes(int64_t n, int logb) {
  return (int64_t)align_up((size_t)((n + (1 << logb) - 1) >> logb) * sizeof(float), 16);
}
static int64_t message_bytes(int64_t n, int cw, int logb) {
  return scale_bytes(n, logb) + plane_bytes(n, cw) + plane_bytes(n, 1);
}

static int check_qb(int64_t n, int32_t q, int32_t bucket) {
  CHOCO_REQUIRE(n > 0 && n < (int64_t)INT32_MAX, "n out of range");
  CHOCO_REQUIRE(q >= 1 && q <= 16, "quantize level q must be in [1, 16], got %d", q);
  CHOCO_REQUIRE(bucket_log2(bucket) > 0, "bucket must be one of 128, 256, 512, 1024, 2048, got %d", bucket);
  return CHOCO_OK;
}

// c: 1, or 1.0 / (min(B / s**2, sqrt(B) / s) + 1.0) in doubles -- sparsification.py:96-97 with the
// bucket size for the tensor's; the same constant for every bucket, a short last one included.
static float biased_scale(int32_t q, int32_t bucket, int32_t is_biased) {
  const double s = (double)((1 << q) - 1), B = (double)bucket;
  return is_biased ? (float)(1.0 / (fmin(B / (s * s), sqrt(B) / s) + 1.0)) : 1.0f;
}

// The quantizer's arguments of a checked call; message: [scales | level plane | sign plane].
static int make_quant(BQuant& A, int64_t n, int32_t q, int32_t bucket, int32_t is_biased, const float* u_in,
                      uint64_t seed, uint64_t offset, uint8_t* message, float* dense_out) {
  CHOCO_REQUIRE(message, "null pointer argument");
  CHOCO_REQUIRE(aligned16(message) && aligned16(u_in) && aligned16(dense_out), "buffers must be 16-byte aligned");
  const int logb = bucket_log2(bucket), cw = container_bits(q);
  A.n = n;
  A.logb = logb;
  A.s_levels = (1 << q) - 1;
  A.c = biased_scale(q, bucket, is_biased);
  A.u_in = u_in;
  A.seed = seed;
  A.offset = offset;
  A.scales = reinterpret_cast<float*>(message);
  A.lvl = message + scale_bytes(n, logb);
  A.sgn = A.lvl + plane_bytes(n, cw);
  A.dense = dense_out;
  return CHOCO_OK;
}

static int make_msgs(BMsgs& M, const uint8_t* const* messages, const float* weights, int32_t nmsg,
                     int32_t self_slot, int64_t n, int cw, int logb) {
  for (int m = 0; m < nmsg; ++m) {
    CHOCO_REQUIRE(messages[m], "null message pointer");
    CHOCO_REQUIRE(aligned16(messages[m]), "messages must be 16-byte aligned");
    M.scales[m] = reinterpret_cast<const float*>(messages[m]);
    M.lvl[m] = messages[m] + scale_bytes(n, logb);
    M.sgn[m] = M.lvl[m] + plane_bytes(n, cw);
    M.w[m] = weights[m];
  }
  M.nmsg = nmsg;
  M.self_slot = self_slot;
  return CHOCO_OK;
}

static int bucket_compress(float* x, const float* xhat, int64_t n, int32_t q, int32_t bucket, int32_t is_biased,
                           const float* u_in, uint64_t seed, uint64_t offset, uint8_t* message, float* dense_out,
                           hipStream_t st, Gossip gs) {
  CHOCO_REQUIRE(x, "null pointer argument");
  CHOCO_TRY(check_qb(n, q, bucket));
  CHOCO_REQUIRE(aligned16(x) && aligned16(xhat) && aligned16(gs.mem), "buffers must be 16-byte aligned");
  BQuant A{};
  CHOCO_TRY(make_quant(A, n, q, bucket, is_biased, u_in, seed, offset, message, dense_out));
  const int64_t mb = message_bytes(n, container_bits(q), A.logb);
  CHOCO_REQUIRE(!overlaps(message, mb, x, 4 * n) && !overlaps(message, mb, xhat, 4 * n) &&
                    !overlaps(message, mb, gs.mem, 4 * n),
                "the message aliases (overlaps) x, x_hat or memory");
  const unsigned grid = (unsigned)((n + kQStreamTile - 1) / kQStreamTile);
  const int mode = gs.mem ? 2 : (xhat ? 1 : 0);
  return dispatch_width(container_bits(q), [&](auto CW) {
    return dispatch_bool(u_in != nullptr, [&](auto UIN) {
      return dispatch_list<0, 1, 2>(mode, "input form", [&](auto MD) {
        return CHOCO_LAUNCH("qsgd_bucket_quantize", "qsgd_bucket_quant_kernel",
                            (qsgd_bucket_quant_kernel<CW, (decltype(MD)::value >= 1), (decltype(MD)::value == 2), UIN>), dim3(grid), dim3(kQThreads), st,
                            x, xhat, gs, A);
      });
    });
  });
}

template <int MODE>
static int bucket_decode_launch(const BMsgs& M, int64_t n, int32_t q, int logb, float c, float* hat, float* mem,
                                hipStream_t st) {
  const unsigned grid = (unsigned)((n + kQTile - 1) / kQTile);
  return dispatch_width(container_bits(q), [&](auto CW) {
    return dispatch_nmsg(M.nmsg, [&](auto NM) {
      return CHOCO_LAUNCH(MODE ? "qsgd_bucket_accumulate" : nullptr, "qsgd_bucket_decode_kernel",
                          (qsgd_bucket_decode_kernel<CW, NM, MODE>), dim3(grid), dim3(kQThreads), st, M, n, logb,
                          (1 << q) - 1, c, hat, mem);
    });
  });
}

}  // namespace choco

using namespace choco;

CHOCO_API int64_t choco_qsgd_bucket_packed_bytes(int64_t n, int32_t q, int32_t bucket) {
  if (n <= 0 || q < 1 || q > 16 || bucket_log2(bucket) < 0) return 0;
  return message_bytes(n, container_bits(q), bucket_log2(bucket));
}

CHOCO_API int choco_qsgd_bucket_compress(const float* x, const float* xhat, int64_t n, int32_t q, int32_t bucket,
                                         int32_t is_biased, const float* u_in, uint64_t seed, uint64_t offset,
                                         uint8_t* message, float* dense_out, void* stream) {
  return bucket_compress(const_cast<float*>(x), xhat, n, q, bucket, is_biased, u_in, seed, offset, message, dense_out,
                         as_stream(stream), Gossip{nullptr, 0.f});
}

CHOCO_API int choco_gossip_qsgd_bucket_compress(float* x, const float* memory, const float* xhat, float gamma,
                                                int64_t n, int32_t q, int32_t bucket, int32_t is_biased,
                                                const float* u_in, uint64_t seed, uint64_t offset, uint8_t* message,
                                                float* dense_out, void* stream) {
  CHOCO_REQUIRE(memory != nullptr && xhat != nullptr, "the gossip step needs memory and x_hat (null pointer)");
  return bucket_compress(x, xhat, n, q, bucket, is_biased, u_in, seed, offset, message, dense_out, as_stream(stream),
                         Gossip{memory, gamma});
}

CHOCO_API int choco_qsgd_bucket_decode(const uint8_t* message, int64_t n, int32_t q, int32_t bucket,
                                       int32_t is_biased, float* out, void* stream) {
  CHOCO_REQUIRE(message && out, "null pointer argument");
  CHOCO_TRY(check_qb(n, q, bucket));
  CHOCO_REQUIRE(aligned16(out), "buffers must be 16-byte aligned");
  const float w = 1.0f;
  BMsgs M{};
  CHOCO_TRY(make_msgs(M, &message, &w, 1, -1, n, container_bits(q), bucket_log2(bucket)));
  return bucket_decode_launch<0>(M, n, q, bucket_log2(bucket), biased_scale(q, bucket, is_biased), nullptr, out,
                                 as_stream(stream));
}

CHOCO_API int choco_qsgd_bucket_decompress_accumulate(const uint8_t* const* messages, const float* weights,
                                                      int32_t nmsg, int32_t self_slot, int64_t n, int32_t q,
                                                      int32_t bucket, int32_t is_biased, float* xhat_self,
                                                      float* memory, void* stream) {
  CHOCO_REQUIRE(messages && weights && memory, "null pointer argument");
  CHOCO_TRY(check_msgs(nmsg, self_slot));
  CHOCO_TRY(check_qb(n, q, bucket));
  CHOCO_REQUIRE(aligned16(memory) && aligned16(xhat_self), "buffers must be 16-byte aligned");
  if (!xhat_self) self_slot = -1;
  BMsgs M{};
  CHOCO_TRY(make_msgs(M, messages, weights, nmsg, self_slot, n, container_bits(q), bucket_log2(bucket)));
  return bucket_decode_launch<1>(M, n, q, bucket_log2(bucket), biased_scale(q, bucket, is_biased), xhat_self, memory,
                                 as_stream(stream));
}

CHOCO_API int choco_qsgd_bucket_recv_gossip_compress(const uint8_t* const* messages, const float* weights,
                                                     int32_t nmsg, int32_t self_slot, float* x, float* memory,
                                                     float* xhat, float gamma, int64_t n, int32_t q, int32_t bucket,
                                                     int32_t is_biased, const float* u_in, uint64_t seed,
                                                     uint64_t offset, uint8_t* message_out, void* stream) {
  CHOCO_REQUIRE(messages && weights && x && memory && xhat, "null pointer argument");
  CHOCO_TRY(check_msgs(nmsg, self_slot));
  CHOCO_TRY(check_qb(n, q, bucket));
  CHOCO_REQUIRE(aligned16(x) && aligned16(memory) && aligned16(xhat), "buffers must be 16-byte aligned");
  const int cw = container_bits(q), logb = bucket_log2(bucket);
  BMsgs M{};
  CHOCO_TRY(make_msgs(M, messages, weights, nmsg, self_slot, n, cw, logb));
  BQuant A{};
  CHOCO_TRY(make_quant(A, n, q, bucket, is_biased, u_in, seed, offset, message_out, nullptr));
  const int64_t mb = message_bytes(n, cw, logb);
  CHOCO_REQUIRE(!overlaps(message_out, mb, x, 4 * n) && !overlaps(message_out, mb, xhat, 4 * n) &&
                    !overlaps(message_out, mb, memory, 4 * n),
                "the output message aliases (overlaps) x, x_hat or memory");
  for (int m = 0; m < nmsg; ++m)
    CHOCO_REQUIRE(!overlaps(message_out, mb, messages[m], mb), "the output message aliases (overlaps) message %d", m);
  const unsigned grid = (unsigned)((n + kQStreamTile - 1) / kQStreamTile);
  return dispatch_width(cw, [&](auto CW) {
    return dispatch_nmsg(nmsg, [&](auto NM) {
      return dispatch_bool(u_in != nullptr, [&](auto UIN) {
        return CHOCO_LAUNCH("qsgd_bucket_step", "qsgd_bucket_recv_gossip_quant_kernel",
                            (qsgd_bucket_recv_gossip_quant_kernel<CW, NM, UIN>), dim3(grid), dim3(kQThreads),
                            as_stream(stream), M, x, xhat, memory, gamma, A);
      });
    });
  });
}
