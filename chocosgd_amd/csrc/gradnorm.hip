// The gradient norms beside the SGD update (sgd.hip): the per-tensor norms DGC clips by, the global
// gradient norm with its clip coefficient, and the dynamic loss-scale state machine on the same
// sum.  The tile geometry, the table walk and the flag bits are the update's (param_common.h).
#include "param_common.h"

#include <cmath>

namespace choco {

// ------------------------------------------------------------------ per-tensor gradient norms
// ||d_s||_2 of every tensor, d = g or rnd(fma(wd, p, g)) (the first line of sgd_math): what
// DGC._clip_gradient takes of d_p after the weight decay (dl_code/pcode/optim/dgc.py:254-265,
// :304-310).  Same shape as the update: 8192-element tiles at absolute flat offsets, the chunk's
// table in the kernel arguments, the same uniform search, 16-byte loads where p and g are
// congruent with the group grid.  Squares and sums are fp64 (the square of an fp32 value is
// exact there and the sum cannot overflow).  No atomics: every (tile, tensor) pair stores ONE
// fp64 partial at slot tile + s -- the pairs are strictly ordered, so the slot is unique and a
// tensor's slots are contiguous -- and the finish kernel adds a tensor's slots in ascending
// order.  Every slot and meta word the finish reads is written by the same call.  Spans of up to
// kNormWaveMax elements are reduced by ONE wave of the workgroup, the waves taking them in turn,
// with no barrier (a tile of the 3000 x 100 layout holds ~80 tensors); longer spans by the
// whole workgroup through LDS.
constexpr int kNormCap = 112;             // tensors per launch
constexpr int kNormU = 2;                 // 8-element groups in flight per thread
constexpr int64_t kNormWaveMax = 1024;
#ifndef CHOCO_SQNORM_NT
#define CHOCO_SQNORM_NT 0                 // 1: non-temporal loads.  Default-policy loads leave p and g in the
                                          // Infinity Cache for the update that follows
#endif

struct NormTable {
  const void* p[kNormCap];
  const void* g[kNormCap];
  int64_t off[kNormCap + 1];
  float wd[kNormCap];
  uint8_t dt[kNormCap];
  uint8_t fl[kNormCap];  // CHOCO_SGD_F_NOGRAD | kSgdHasWd
  int32_t nt;
};
static_assert(sizeof(NormTable) + 32 <= 4096 - 256, "NormTable must fit in the kernel arguments");

template <int DT>
CHOCO_DEV void ld8n(Raw8& r, const void* base, int64_t j) {
  if (CHOCO_SQNORM_NT) {
    ld8<DT>(r, base, j);
  } else if (DT == CHOCO_DT_F32) {
    const float4* s = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + j);
    r.lo = s[0];
    r.hi = s[1];
  } else {
    r.h = *reinterpret_cast<const choco_u16x8*>(reinterpret_cast<const unsigned short*>(base) + j);
  }
}

template <int DT>
CHOCO_DEV double norm_sq(bool has_wd, float wd, float p, float g) {
  float d = g;
  if (has_wd) d = rnd<DT>(fmaf(wd, p, d));
  return (double)d * (double)d;
}

template <int DT>
CHOCO_DEV double norm_elem(const void* p, const void* g, bool has_wd, float wd, int64_t j) {
  return norm_sq<DT>(has_wd, wd, has_wd ? ld1<DT>(p, j) : 0.0f, ld1<DT>(g, j));
}

// this thread's share of flat elements [a, b) of a tensor at flat offset o0, `stride` threads
// (a wave or the workgroup) taking it elementwise, `me` this thread's place among them
template <int DT>
CHOCO_DEV double norm_scalar(const void* p, const void* g, bool has_wd, float wd, int64_t o0, int64_t a, int64_t b,
                             int me, int stride) {
  double acc = 0.0;
  for (int64_t i = a + me; i < b; i += stride) acc += norm_elem<DT>(p, g, has_wd, wd, i - o0);
  return acc;
}

// ... the workgroup taking whole groups as 16-byte vectors, kNormU groups in flight per thread.
// A loop of its own, not param_common.h's span_walk: there is nothing to store, the loads are
// default-policy (ld8n) and all of a round's are issued ahead of the first square.
template <int DT>
CHOCO_DEV double norm_vector(const void* p, const void* g, bool has_wd, float wd, int64_t o0, int64_t a, int64_t b) {
  const int tid = threadIdx.x;
  double acc = 0.0;
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;
  for (int64_t gb = g0; gb <= g1; gb += (int64_t)kPbThreads * kNormU) {
    bool full[kNormU];
    Raw8 rp[kNormU], rg[kNormU];
#pragma unroll
    for (int u = 0; u < kNormU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      full[u] = e >= a && e + kPbGroup <= b;
      if (full[u]) {
        if (has_wd) ld8n<DT>(rp[u], p, e - o0);
        ld8n<DT>(rg[u], g, e - o0);
      }
    }
#pragma unroll
    for (int u = 0; u < kNormU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      if (full[u]) {
        float pv[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gv[8];
        if (has_wd) widen8<DT>(rp[u], pv);
        widen8<DT>(rg[u], gv);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += norm_sq<DT>(has_wd, wd, pv[k], gv[k]);
      } else {
        const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
        for (int64_t i = ea; i < eb; ++i) acc += norm_elem<DT>(p, g, has_wd, wd, i - o0);
      }
    }
  }
  return acc;
}

// meta: two words per tensor of the chunk, {first slot, slots | dtype << 24}
__global__ __launch_bounds__(kPbThreads) void param_sqnorm_kernel(const NormTable tb, double* slots, int32_t* meta,
                                                                  int64_t tile0, int32_t seg0) {
  __shared__ double red[kPbThreads / 64];
  const int nt = tb.nt;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    for (int s = 0; s < nt; ++s) {  // s is uniform: the table is read with scalar loads
      const int64_t o0 = tb.off[s], o1 = tb.off[s + 1];
      const bool any = o1 > o0 && !(tb.fl[s] & CHOCO_SGD_F_NOGRAD);
      const int32_t cnt = any ? (int32_t)((o1 - 1) / kPbTile - o0 / kPbTile + 1) : 0;
      if (tid == (s & (kPbThreads - 1))) {
        meta[2 * s] = (int32_t)(o0 / kPbTile) + seg0 + s;
        meta[2 * s + 1] = cnt | ((int32_t)tb.dt[s] << 24);
      }
    }
  }
  const int64_t tile = tile0 + blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  int nshort = 0;
  tile_walk(tb.off, nt, tile, [&](int s, int64_t a, int64_t b) {
    const uint32_t fl = tb.fl[s];
    if (fl & CHOCO_SGD_F_NOGRAD) return;
    const int dt = tb.dt[s];
    const int64_t o0 = tb.off[s];
    const bool has_wd = (fl & kSgdHasWd) != 0;
    const float wd = tb.wd[s];
    const void* p = tb.p[s];
    const void* g = tb.g[s];
    double* slot = slots + (tile + seg0 + s);
    double acc;
    if (b - a <= kNormWaveMax) {
      const bool mine = (nshort & 3) == wave;
      ++nshort;
      if (!mine) return;
      for_dtype(dt, [&](auto DT) { acc = norm_scalar<DT>(p, g, has_wd, wd, o0, a, b, lane, 64); });
      acc = wave_sum(acc);
      if (lane == 0) *slot = acc;
      return;
    }
    const uintptr_t esz = dtype_size(dt);
    uintptr_t mis = mis16(g, esz, o0);
    if (has_wd) mis |= mis16(p, esz, o0);
    const bool vec = on_grid16(mis);
    for_dtype(dt, [&](auto DT) {
      acc = vec ? norm_vector<DT>(p, g, has_wd, wd, o0, a, b)
                : norm_scalar<DT>(p, g, has_wd, wd, o0, a, b, tid, kPbThreads);
    });
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) *slot = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();  // red is reused by the next long span
  });
}

// v as dtype dt (a CHOCO_DT_* code) holds it
CHOCO_DEV float rnd_as(float v, int dt) {
  for_dtype(dt, [&](auto DT) { v = rnd<DT>(v); });
  return v;
}

// one wave per tensor: its slots added in ascending order (64 at a time are loaded by the lanes
// side by side, then added one after the other, so the order does not depend on the lane count),
// sqrt in fp64, rounded to fp32 and, for a 16-bit tensor, again to its dtype (grad.norm()
// returns the gradient's dtype)
constexpr int kNormFinishWaves = kPbThreads / 64;

__global__ __launch_bounds__(kPbThreads) void param_sqnorm_finish_kernel(const double* slots, const int32_t* meta,
                                                                         float* norms, int32_t nseg) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * kNormFinishWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= nseg) return;
  const int32_t slot0 = meta[2 * s], cd = meta[2 * s + 1];
  const int32_t cnt = cd & 0xffffff, dt = cd >> 24;
  double acc = 0.0;
  for (int32_t base = 0; base < cnt; base += 64) {
    const int32_t i = base + lane;
    const double v = i < cnt ? slots[slot0 + i] : 0.0;
    const int32_t m = cnt - base < 64 ? cnt - base : 64;
    for (int32_t l = 0; l < m; ++l) acc += __shfl(v, l);
  }
  if (lane == 0) norms[s] = rnd_as((float)sqrt(acc), dt);
}

// ------------------------------------------------------------------ the global gradient norm and its clip coefficient
// torch.nn.utils.clip_grad_norm_(parameters, max_norm) (distributed_running_nlp.py:96) up to the
// coefficient, on the device (choco_params_gradnorm): after param_sqnorm_kernel on the raw
// gradients, ONE workgroup adds every tensor's partials as the finish kernel above does (its
// waves take the tensors in turn; sums[s] keeps the fp64 sum, norms[s] the per-tensor norm), then
// its first wave adds sums[0 .. nseg) in ascending order, takes the square root in fp64 and
// evaluates, with CD = the coefficient's dtype,
//     total = rnd_CD((float)sqrt(sum))      or rnd_CD(*total_in): the pinned total, no norm pass
//     t = rnd_CD(total + 1e-6f);  r = rnd_CD(1.0f / t);  c = rnd_CD(r * max_norm);  c = c > 1 ? 1 : c
// -- torch's `max_norm / (total_norm + 1e-6)` is total.reciprocal() * max_norm, clamped with
// max = 1.0: a NaN stays NaN, an inf total gives 0.  out[0] = total, out[1] = c.  No atomics: the
// order of every addition is fixed.  One workgroup means latency, not bandwidth, is the cost: the
// slots, the meta words and the per-tensor sums of a layout that fits (ResNet-50: 3281 slots) are
// staged in LDS by one coalesced pass, and a lane's value reaches the sum through v_readlane
// (the lane index is uniform), not through the LDS crossbar.  A larger layout reads the workspace
// in place, with the same additions in the same order.

// v[0] + v[1] + ... + v[cnt - 1], added in that order by one wave as the finish kernel above adds a
// tensor's slots (cnt uniform); every lane gets the sum
CHOCO_DEV double wave_ordered_sum(const double* v, int32_t cnt, int lane) {
  double acc = 0.0;
  for (int32_t base = 0; base < cnt; base += 64) {
    const int32_t i = base + lane;
    const double x = i < cnt ? v[i] : 0.0;
    const int hi = __double2hiint(x), lo = __double2loint(x);
    const int32_t m = cnt - base < 64 ? cnt - base : 64;
    for (int32_t l = 0; l < m; ++l)
      acc += __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l));
  }
  return acc;
}

//
// The scaled variant (choco_params_gradnorm_scaled, "param_gradnorm_scaled_total_kernel"): dynamic
// loss scaling on the same sum.  The gradients are still multiplied by the loss scale, so with
// scale = *ls.scale and inv = (float)(1.0 / (double)scale)
//     found = !isfinite(sum)                          the fp64 sum, not the fp32 total: squares are
//                                                     non-negative and their fp64 sum cannot overflow
//     total = rnd_CD((float)sqrt(sum) * inv)          the norm of the unscaled gradient
//     c     = the lines above (has_clip), or 1
//     gc    = c * inv                                 fp32, not narrowed
//     out   = [total, gc, found ? 1 : 0, scale]
// and then torch's _amp_update_scale_ on the device state, by the lane that writes out[]:
//     found:  scale = (float)((double)scale * backoff), tracker = 0
//     else:   tracker + 1 == interval ? (s = (float)((double)scale * growth), kept if finite; tracker = 0)
//                                     : tracker += 1
// Same staging, same additions in the same order; the host never reads any of it.
struct LossScale {
  float* scale;      // device, the fp32 loss scale
  int32_t* tracker;  // device, steps since the scale last changed
  double growth, backoff;
  int32_t interval, has_clip;
};

// torch's _amp_update_scale_ on the device state, from the scale the step ran with: plain stores
// by one lane.  loss_scale_update_kernel's copy of the lines scaled_out<true> ends with: that
// instantiation keeps the instruction stream it had.
CHOCO_DEV void amp_update_scale(float scale, bool found, const LossScale& ls) {
  if (found) {
    *ls.scale = (float)((double)scale * ls.backoff);
    *ls.tracker = 0;
  } else {
    const int32_t ok = *ls.tracker + 1;
    if (ok == ls.interval) {
      const float s = (float)((double)scale * ls.growth);
      if (__builtin_isfinite(s)) *ls.scale = s;
      *ls.tracker = 0;
    } else {
      *ls.tracker = ok;
    }
  }
}

// the one lane that writes out[]: sum = the fp64 sum of squares, root = (float)sqrt(sum).
// UPDATE false (choco_params_gradnorm_scaled_local): the state is read, never written -- the
// ranks of an all-reduce step agree on `found` first (choco_loss_scale_update).
template <bool UPDATE>
CHOCO_DEV void scaled_out(double sum, float root, float max_norm, int32_t cd, float* out, const LossScale& ls) {
  const float scale = *ls.scale;
  const float inv = (float)(1.0 / (double)scale);
  const bool found = !__builtin_isfinite(sum);
  const float total = rnd_as(__fmul_rn(root, inv), cd);
  float c = 1.0f;
  if (ls.has_clip) {
    const float t = rnd_as(__fadd_rn(total, 1e-6f), cd);
    const float r = rnd_as(__fdiv_rn(1.0f, t), cd);
    c = rnd_as(__fmul_rn(r, max_norm), cd);
    c = c > 1.0f ? 1.0f : c;
  }
  out[0] = total;
  out[1] = __fmul_rn(c, inv);
  out[2] = found ? 1.0f : 0.0f;
  out[3] = scale;
  if (!UPDATE) return;
  if (found) {
    *ls.scale = (float)((double)scale * ls.backoff);
    *ls.tracker = 0;
  } else {
    const int32_t ok = *ls.tracker + 1;
    if (ok == ls.interval) {
      const float s = (float)((double)scale * ls.growth);
      if (__builtin_isfinite(s)) *ls.scale = s;
      *ls.tracker = 0;
    } else {
      *ls.tracker = ok;
    }
  }
}

struct LossScaleLocal {
  LossScale ls;
};
CHOCO_DEV void scaled_finish(double sum, float root, float max_norm, int32_t cd, float* out, const LossScale& ls) {
  scaled_out<true>(sum, root, max_norm, cd, out, ls);
}
CHOCO_DEV void scaled_finish(double sum, float root, float max_norm, int32_t cd, float* out, const LossScaleLocal& l) {
  scaled_out<false>(sum, root, max_norm, cd, out, l.ls);
}

// choco_loss_scale_update: the state update alone, from the all-reduced flag.  One lane of one
// small workgroup; out is choco_params_gradnorm_scaled_local's, whose third float becomes the
// ranks' common flag.
__global__ __launch_bounds__(64) void loss_scale_update_kernel(const float* found_sum, const LossScale ls, float* out) {
  if (threadIdx.x != 0) return;
  const bool found = *found_sum != 0.0f;
  out[2] = found ? 1.0f : 0.0f;
  amp_update_scale(*ls.scale, found, ls);
}

constexpr int kTotalThreads = 1024;
constexpr int kTotalStageSlots = 5120;  // 40 KB of fp64 slots, 8 KB of meta words and 8 KB of sums in LDS
constexpr int kTotalStageSegs = 1024;
// LS: no argument at all (param_gradnorm_total_kernel, the argument list it always had), or one
// LossScale ("param_gradnorm_scaled_total_kernel"; total_in is then null: a pinned total has no
// norm pass to detect an overflow from), or one LossScaleLocal
// ("param_gradnorm_scaled_local_total_kernel": the same without the state update).
template <typename... LS>
__global__ __launch_bounds__(kTotalThreads) void param_gradnorm_total_kernel(const double* slots, int32_t nslots,
                                                                             const int32_t* meta, double* sums,
                                                                             float* norms, int32_t nseg,
                                                                             const float* total_in, float max_norm,
                                                                             int32_t cd, float* out, const LS... ls) {
  constexpr bool SC = sizeof...(LS) != 0;
  __shared__ double s_slots[kTotalStageSlots];
  __shared__ int32_t s_meta[2 * kTotalStageSegs];
  __shared__ double s_sums[kTotalStageSegs];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float total;
  double sum = 0.0;  // the fp64 sum of squares: what the scaled variant tests for an overflow
  if (total_in != nullptr) {
    total = *total_in;
  } else {
    if (nslots <= kTotalStageSlots && nseg <= kTotalStageSegs) {
      // slots no (tile, tensor) pair wrote hold whatever the workspace held: moved, never added
      for (int32_t i = tid; i < nslots; i += kTotalThreads) s_slots[i] = slots[i];
      for (int32_t i = tid; i < 2 * nseg; i += kTotalThreads) s_meta[i] = meta[i];
      __syncthreads();
      slots = s_slots;
      meta = s_meta;
      sums = s_sums;
    }
    for (int32_t s = wave; s < nseg; s += kTotalThreads / 64) {
      const int32_t slot0 = __builtin_amdgcn_readfirstlane(meta[2 * s]);
      const int32_t w = __builtin_amdgcn_readfirstlane(meta[2 * s + 1]);
      const double acc = wave_ordered_sum(slots + slot0, w & 0xffffff, lane);
      if (lane == 0) {
        sums[s] = acc;
        if (norms != nullptr) norms[s] = rnd_as((float)sqrt(acc), w >> 24);
      }
    }
    __syncthreads();  // sums[] of every wave, written above, is read by the first one
    if (wave != 0) return;
    sum = wave_ordered_sum(sums, nseg, lane);
    total = (float)sqrt(sum);
  }
  if (tid != 0) return;
  if constexpr (SC) {
    (scaled_finish(sum, total, max_norm, cd, out, ls), ...);
    return;
  }
  total = rnd_as(total, cd);
  const float t = rnd_as(__fadd_rn(total, 1e-6f), cd);
  const float r = rnd_as(__fdiv_rn(1.0f, t), cd);
  float c = rnd_as(__fmul_rn(r, max_norm), cd);
  c = c > 1.0f ? 1.0f : c;
  out[0] = total;
  out[1] = c;
}


static int norm_launches(int32_t nseg) { return nseg <= 0 ? 0 : chunk_launches(nseg, kNormCap) + 1; }
static size_t norm_slots(int32_t nseg, int64_t n) { return (size_t)(n / kPbTile + 1) + (size_t)nseg; }
static size_t norm_ws_bytes(int32_t nseg, int64_t n) {
  if (nseg <= 0 || n < 0) return 0;
  return align_up(norm_slots(nseg, n) * sizeof(double) + (size_t)nseg * 2 * sizeof(int32_t), 256);
}

struct NormArgs {
  const void* const* params;
  const void* const* grads;
  const int64_t* lens;
  const int32_t* dtypes;
  const double* wd;
  const int32_t* flags;
  int32_t nseg;
  int64_t n;
  float* norms;
  void* ws;
  size_t ws_bytes;
};

// tensor s of a norm call (params / wd null: choco_params_gradnorm, the raw gradients alone)
static int norm_tensor_check(const void* const* params, const void* const* grads, const int64_t* lens,
                             const double* wd, const int32_t* flags, int32_t s, uintptr_t esz) {
  const int i = (int)s;
  constexpr int32_t kFlags = CHOCO_SGD_F_NESTEROV | CHOCO_SGD_F_FIRST | CHOCO_SGD_F_NOGRAD;
  CHOCO_REQUIRE((flags[s] & ~kFlags) == 0, "tensor %d: unknown flag bits 0x%x", i, (unsigned)flags[s]);
  CHOCO_REQUIRE((!params || elem_aligned(params[s], esz)) && elem_aligned(grads[s], esz),
                "tensor %d: pointer not aligned to its element size", i);
  if (lens[s] == 0 || (flags[s] & CHOCO_SGD_F_NOGRAD)) return CHOCO_OK;
  CHOCO_REQUIRE(grads[s], "tensor %d: null grad pointer without the no-grad flag", i);
  CHOCO_REQUIRE(!params || params[s] || wd[s] == 0.0, "tensor %d: null param pointer with weight decay != 0", i);
  return CHOCO_OK;
}

static int norm_check(const NormArgs& a) {
  CHOCO_REQUIRE(a.params && a.grads && a.lens && a.dtypes && a.wd && a.flags, "null table argument");
  return layout_check(
      a.lens, a.dtypes, a.nseg, a.n,
      [&]() -> int {
        CHOCO_REQUIRE(a.norms && aligned4(a.norms), "norms must be a 4-byte aligned device pointer");
        CHOCO_REQUIRE(a.ws && (reinterpret_cast<uintptr_t>(a.ws) & 7u) == 0, "the workspace must be 8-byte aligned");
        if (a.ws_bytes < norm_ws_bytes(a.nseg, a.n))
          return fail(CHOCO_ERR_WORKSPACE, "workspace too small: %zu bytes, need %zu", a.ws_bytes,
                      norm_ws_bytes(a.nseg, a.n));
        return CHOCO_OK;
      },
      [&](int32_t s, uintptr_t esz) -> int { return norm_tensor_check(a.params, a.grads, a.lens, a.wd, a.flags, s, esz); });
}

// the norm pass: one param_sqnorm_kernel launch per chunk (a.params / a.wd null: raw gradients)
static int norm_pass(const NormArgs& a, double* slots, int32_t* meta, hipStream_t st) {
  NormTable tb;
  return for_chunks<kNormCap>(a.lens, a.nseg, tb.off, [&](const Chunk& c) -> int {
    tb.nt = c.nt;
    for (int i = 0; i < kNormCap; ++i) {
      const bool in = i < c.nt;
      const int32_t s = c.s0 + i;
      const bool upd = in && !(a.flags[s] & CHOCO_SGD_F_NOGRAD);
      tb.p[i] = upd && a.params ? a.params[s] : nullptr;
      tb.g[i] = upd ? a.grads[s] : nullptr;
      tb.wd[i] = upd && a.wd ? (float)a.wd[s] : 0.0f;
      tb.dt[i] = in ? (uint8_t)a.dtypes[s] : (uint8_t)0;
      uint32_t fl = in ? (uint32_t)(a.flags[s] & CHOCO_SGD_F_NOGRAD) : 0u;
      if (upd && a.wd && a.wd[s] != 0.0) fl |= kSgdHasWd;
      tb.fl[i] = (uint8_t)fl;
    }
    return CHOCO_LAUNCH("param_sqnorm_kernel", "param_sqnorm_kernel", param_sqnorm_kernel, dim3((unsigned)c.tiles),
                        dim3(kPbThreads), st, tb, slots, meta + 2 * (size_t)c.s0, c.tile0, c.s0);
  });
}

static int norm_run(const NormArgs& a, hipStream_t st) {
  const int rc = norm_check(a);
  if (rc) return rc;
  double* slots = reinterpret_cast<double*>(a.ws);
  int32_t* meta = reinterpret_cast<int32_t*>(slots + norm_slots(a.nseg, a.n));
  CHOCO_TRY(norm_pass(a, slots, meta, st));
  const unsigned blocks = (unsigned)((a.nseg + kNormFinishWaves - 1) / kNormFinishWaves);
  CHOCO_TRY(CHOCO_LAUNCH("param_sqnorm_finish_kernel", "param_sqnorm_finish_kernel", param_sqnorm_finish_kernel,
                         dim3(blocks), dim3(kPbThreads), st, (const double*)slots, (const int32_t*)meta, a.norms,
                         a.nseg));
  return CHOCO_OK;
}

// choco_params_gradnorm: the norm pass and param_gradnorm_total_kernel, or that launch alone from
// a pinned total.  Workspace: the sqnorm slots, one fp64 sum per tensor, the meta words.
static int gradnorm_launches(int32_t nseg, int32_t pinned) {
  return nseg <= 0 ? 0 : pinned ? 1 : chunk_launches(nseg, kNormCap) + 1;
}
static size_t gradnorm_ws_bytes(int32_t nseg, int64_t n) {
  if (nseg <= 0 || n < 0) return 0;
  return align_up((norm_slots(nseg, n) + (size_t)nseg) * sizeof(double) + (size_t)nseg * 2 * sizeof(int32_t), 256);
}

struct GradnormArgs {
  const void* const* grads;
  const int64_t* lens;
  const int32_t* dtypes;
  const int32_t* flags;
  int32_t nseg;
  int64_t n;
  double max_norm;
  int32_t coef_dtype;
  const float* total_in;
  float* out;
  float* norms;
  void* ws;
  size_t ws_bytes;
  bool scaled;   // choco_params_gradnorm_scaled: out holds four floats and ls is the loss-scale state
  LossScale ls;
  bool local;    // choco_params_gradnorm_scaled_local: the state is not updated
};

// the loss-scale state arguments (choco_params_gradnorm_scaled[_local], choco_loss_scale_update)
static int loss_scale_check(const LossScale& ls) {
  CHOCO_REQUIRE(ls.scale && aligned4(ls.scale), "scale_state must be a 4-byte aligned device pointer");
  CHOCO_REQUIRE(ls.tracker && aligned4(ls.tracker), "growth_tracker must be a 4-byte aligned device pointer");
  CHOCO_REQUIRE(ls.growth > 1.0 && std::isfinite(ls.growth), "growth must be finite and > 1, got %g", ls.growth);
  CHOCO_REQUIRE(ls.backoff > 0.0 && ls.backoff < 1.0, "backoff must be in (0, 1), got %g", ls.backoff);
  CHOCO_REQUIRE(ls.interval >= 1, "interval must be >= 1, got %d", (int)ls.interval);
  return CHOCO_OK;
}

static int gradnorm_check(const GradnormArgs& a) {
  // the arguments beside the layout; a pinned total (parity mode) reads nothing of the layout
  const auto own = [&]() -> int {
    // tested as the kernel uses it: the fp32 value (a scaled call without a clip does not use it)
    if (!a.scaled || a.ls.has_clip)
      CHOCO_REQUIRE(a.max_norm >= 0.0 && a.max_norm <= 3.4028234663852886e38,
                    "max_norm must be >= 0 and finite as an fp32 value, got %g", a.max_norm);
    if (a.scaled) {
      CHOCO_TRY(loss_scale_check(a.ls));
      CHOCO_REQUIRE(a.ls.has_clip == 0 || a.ls.has_clip == 1, "has_clip must be 0 or 1, got %d", (int)a.ls.has_clip);
    }
    CHOCO_REQUIRE(a.coef_dtype >= CHOCO_DT_F32 && a.coef_dtype <= CHOCO_DT_F16, "unknown coef_dtype code %d",
                  (int)a.coef_dtype);
    CHOCO_REQUIRE(a.out && aligned4(a.out), "out must be a 4-byte aligned device pointer");
    CHOCO_REQUIRE(aligned4(a.norms), "norms must be 4-byte aligned");
    if (a.total_in) {
      CHOCO_REQUIRE(aligned4(a.total_in), "total_in must be 4-byte aligned");
      CHOCO_REQUIRE(!a.norms, "norms with a pinned total: there is no norm pass to take them from");
      return CHOCO_OK;
    }
    CHOCO_REQUIRE(a.grads && a.lens && a.dtypes && a.flags, "null table argument");
    CHOCO_REQUIRE(a.ws && (reinterpret_cast<uintptr_t>(a.ws) & 7u) == 0, "the workspace must be 8-byte aligned");
    if (a.ws_bytes < gradnorm_ws_bytes(a.nseg, a.n))
      return fail(CHOCO_ERR_WORKSPACE, "workspace too small: %zu bytes, need %zu", a.ws_bytes,
                  gradnorm_ws_bytes(a.nseg, a.n));
    return CHOCO_OK;
  };
  if (a.total_in) {
    CHOCO_TRY(layout_head(a.nseg, a.n));
    return own();
  }
  return layout_check(a.lens, a.dtypes, a.nseg, a.n, own, [&](int32_t s, uintptr_t esz) -> int {
    return norm_tensor_check(nullptr, a.grads, a.lens, nullptr, a.flags, s, esz);
  });
}

static int gradnorm_run(const GradnormArgs& a, hipStream_t st) {
  const int rc = gradnorm_check(a);
  if (rc) return rc;
  double* slots = nullptr;
  double* sums = nullptr;
  int32_t* meta = nullptr;
  if (!a.total_in) {
    slots = reinterpret_cast<double*>(a.ws);
    sums = slots + norm_slots(a.nseg, a.n);
    meta = reinterpret_cast<int32_t*>(sums + a.nseg);
    const NormArgs pass{nullptr, a.grads, a.lens, a.dtypes, nullptr, a.flags, a.nseg, a.n, nullptr, a.ws, a.ws_bytes};
    CHOCO_TRY(norm_pass(pass, slots, meta, st));
  }
  if (a.scaled && a.local) {
    CHOCO_TRY(CHOCO_LAUNCH("param_gradnorm_scaled_local_total_kernel", "param_gradnorm_scaled_local_total_kernel",
                           param_gradnorm_total_kernel<LossScaleLocal>, dim3(1), dim3(kTotalThreads), st,
                           (const double*)slots, (int32_t)norm_slots(a.nseg, a.n), (const int32_t*)meta, sums, a.norms,
                           a.nseg, (const float*)nullptr, (float)(a.ls.has_clip ? a.max_norm : 0.0), a.coef_dtype,
                           a.out, LossScaleLocal{a.ls}));
    return CHOCO_OK;
  }
  if (a.scaled) {
    CHOCO_TRY(CHOCO_LAUNCH("param_gradnorm_scaled_total_kernel", "param_gradnorm_scaled_total_kernel",
                           param_gradnorm_total_kernel<LossScale>, dim3(1), dim3(kTotalThreads), st,
                           (const double*)slots, (int32_t)norm_slots(a.nseg, a.n), (const int32_t*)meta, sums, a.norms,
                           a.nseg, (const float*)nullptr, (float)(a.ls.has_clip ? a.max_norm : 0.0), a.coef_dtype,
                           a.out, a.ls));
    return CHOCO_OK;
  }
  CHOCO_TRY(CHOCO_LAUNCH("param_gradnorm_total_kernel", "param_gradnorm_total_kernel", param_gradnorm_total_kernel<>,
                         dim3(1), dim3(kTotalThreads), st, (const double*)slots,
                         (int32_t)(a.total_in ? 0 : norm_slots(a.nseg, a.n)), (const int32_t*)meta, sums, a.norms,
                         a.nseg, a.total_in, (float)a.max_norm, a.coef_dtype, a.out));
  return CHOCO_OK;
}

}  // namespace choco

using namespace choco;

CHOCO_API size_t choco_params_sqnorm_workspace_size(int32_t nseg, int64_t n) { return norm_ws_bytes(nseg, n); }
CHOCO_API int choco_params_sqnorm_launches(int32_t nseg) { return norm_launches(nseg); }

CHOCO_API int choco_params_sqnorm(const void* const* params, const void* const* grads, const int64_t* lens,
                                  const int32_t* dtypes, const double* weight_decay, const int32_t* flags, int32_t nseg,
                                  int64_t n, float* norms, void* ws, size_t ws_bytes, void* stream) {
  const NormArgs a{params, grads, lens, dtypes, weight_decay, flags, nseg, n, norms, ws, ws_bytes};
  return norm_run(a, as_stream(stream));
}

CHOCO_API size_t choco_params_gradnorm_workspace_size(int32_t nseg, int64_t n) { return gradnorm_ws_bytes(nseg, n); }
CHOCO_API int choco_params_gradnorm_launches(int32_t nseg, int32_t pinned) { return gradnorm_launches(nseg, pinned); }

CHOCO_API int choco_params_gradnorm(const void* const* grads, const int64_t* lens, const int32_t* dtypes,
                                    const int32_t* flags, int32_t nseg, int64_t n, double max_norm,
                                    int32_t coef_dtype, const float* total_in, float* out, float* norms, void* ws,
                                    size_t ws_bytes, void* stream) {
  const GradnormArgs a{grads, lens, dtypes, flags, nseg, n, max_norm, coef_dtype, total_in, out, norms, ws, ws_bytes};
  return gradnorm_run(a, as_stream(stream));
}

CHOCO_API int choco_params_gradnorm_scaled(const void* const* grads, const int64_t* lens, const int32_t* dtypes,
                                           const int32_t* flags, int32_t nseg, int64_t n, double max_norm,
                                           int32_t coef_dtype, float* scale_state, int32_t* growth_tracker,
                                           double growth, double backoff, int32_t interval, int32_t has_clip,
                                           float* out, float* norms, void* ws, size_t ws_bytes, void* stream) {
  const GradnormArgs a{grads, lens, dtypes, flags, nseg, n, max_norm, coef_dtype, nullptr, out, norms, ws, ws_bytes,
                       true, LossScale{scale_state, growth_tracker, growth, backoff, interval, has_clip}};
  return gradnorm_run(a, as_stream(stream));
}

CHOCO_API int choco_params_gradnorm_scaled_local(const void* const* grads, const int64_t* lens, const int32_t* dtypes,
                                                 const int32_t* flags, int32_t nseg, int64_t n, double max_norm,
                                                 int32_t coef_dtype, const float* scale_state,
                                                 const int32_t* growth_tracker, double growth, double backoff,
                                                 int32_t interval, int32_t has_clip, float* out, float* norms,
                                                 void* ws, size_t ws_bytes, void* stream) {
  const GradnormArgs a{grads, lens, dtypes, flags, nseg, n, max_norm, coef_dtype, nullptr, out, norms, ws, ws_bytes,
                       true,
                       LossScale{const_cast<float*>(scale_state), const_cast<int32_t*>(growth_tracker), growth, backoff,
                                 interval, has_clip},
                       true};
  return gradnorm_run(a, as_stream(stream));
}

CHOCO_API int choco_loss_scale_update(const float* found_sum, float* scale_state, int32_t* growth_tracker,
                                      double growth, double backoff, int32_t interval, float* out, void* stream) {
  const LossScale ls{scale_state, growth_tracker, growth, backoff, interval, 0};
  CHOCO_REQUIRE(found_sum && aligned4(found_sum), "found_sum must be a 4-byte aligned device pointer");
  const int rc = loss_scale_check(ls);
  if (rc) return rc;
  CHOCO_REQUIRE(out && aligned4(out), "out must be a 4-byte aligned device pointer");
  CHOCO_TRY(CHOCO_LAUNCH("loss_scale_update_kernel", "loss_scale_update_kernel", loss_scale_update_kernel, dim3(1),
                         dim3(64), as_stream(stream), found_sum, ls, out));
  return CHOCO_OK;
}
