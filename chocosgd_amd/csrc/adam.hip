// The Adam / AdamW update (torch.optim.adam._single_tensor_adam; the reference's command line
// carries --adam_beta_1 / --adam_beta_2 / --adam_eps) for a whole list of parameter tensors in
// one batched launch per chunk, fused with the pack into the flat fp32 buffer that follows it in
// a CHOCO step, with the global-norm clip coefficient and the fp32 master copy in the same pass.
//
// The hyperparameters of tensor s are computed on the host in doubles, as torch computes them
// from Python floats, and each is narrowed once to fp32 (`step` is the count after the increment):
//     bc1 = 1 - beta1**step;  bc2 = 1 - beta2**step
//     nss = f32(-(lr / bc1));  bs = f32(bc2 ** 0.5);  dec = f32(1 - lr * wd)
//     w = f32(1 - beta1);  b2 = f32(beta2);  omb2 = f32(1 - beta2);  e = f32(eps)
// Per element, each line one rounding (adam_math); rnd is param_common.h's rnd<DT>:
//     g' = g                       (with a clip coefficient c:  g' = rnd(c * g), as sgd.hip's kGradCoef)
//     if wd != 0:  decoupled:  p  = rnd(p * dec)                   param.mul_(1 - lr * wd)
//                  coupled:    g' = rnd(fma(wd, p, g'))            grad.add(param, alpha=wd)
//     d = g' - m                                                   (fp32, not narrowed: inside lerp)
//     m = w < 0.5 ? rnd(fma(w, d, m)) : rnd(fma(-(1 - w), d, g'))  exp_avg.lerp_(grad, 1 - beta1)
//     v = rnd(v * b2);  t = omb2 * g';  v = rnd(fma(t, g', v))     exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
//     den = rnd(sqrt(v));  den = rnd(den / bs);  den = rnd(den + e)   a true division, never a reciprocal multiply
//     q = m / den;  p_new = rnd(fma(nss, q, p))                    param.addcdiv_(exp_avg, denom, value=-step_size)
// FIRST: the tensor has no state yet; m = v = +0 and the moments are written, never read (no
// memset launch).  A skipped op (wd == 0) is skipped, not run with a neutral coefficient.  The
// library is built with -ffp-contract=off: fma stands where the lines say fma, __fmul_rn /
// __fadd_rn / __fsub_rn elsewhere, __fdiv_rn for both divisions, and sqrtf for the square root
// (the correctly rounded one; __fsqrt_rn compiles to a bare v_sqrt_f32 behind a range scale,
// 1 ulp off on some inputs).
//
// The launch is sgd.hip's: workgroups own 8192-element tiles at absolute flat offsets, the table
// of a chunk of tensors travels in the kernel arguments, tile_walk finds a tile's tensors, and
// span_walk moves whole 8-element groups as 16-byte non-temporal vectors -- every load of a group
// issued before its first store, one group in flight per thread: its four operands are 32 values
// already -- and cut groups and incongruent tensors element by element (AdamBody).  Three
// parameter sides:
//     plain   param_adam_kernel: p, g, m and v in the tensor's own dtype, every line narrowed;
//             an optional flat fp32 output receives p_new (the CHOCO pack), the parameters are
//             written with WRITE_PARAMS, and a NOGRAD tensor is pack-only (flat = p).
//     master  param_adam_master_kernel: p is master[i], in place, in fp32; m and v are fp32
//             whatever the tensor's dtype; nothing is narrowed between the lines, and the 16-bit
//             parameter, where written, is the new master value narrowed once.  A NOGRAD tensor
//             is passed over.
//     sr      param_adam_sr_kernel (choco_params_adam_sr): the plain kernel's sides -- p, g, m
//             and v in the tensor's own dtype, the optional flat output, NOGRAD pack-only -- with
//             the master kernel's arithmetic on a bf16 tensor: the lines run in fp32 on the
//             widened operands, nothing is narrowed between them, and the three stores that
//             leave the registers round stochastically (param_common.h st8_sr / st1_sr), each
//             with a bit field of its own: p with lane 0, m with lane 1, v with lane 2 of
//             (seed, step, flat index).  flat receives p_new unrounded.  An fp32 tensor of the
//             same model is the plain kernel's update and draws no bits; the host refuses fp16.
//             The launch carries lane 0's key; the other two are two uniform mixes a workgroup.
// All take `coef`, gradnorm's clip coefficient on the device or null: one uniform load per
// workgroup, the multiply on the load the update does anyway (narrowed in the plain kernel, not
// in front of master or sr arithmetic); WRITE_CLIPPED stores the narrowed product back into g.
// A launch writes only the bytes of its own elements; distinct tensors must not overlap, which
// is not checked.
#include "param_common.h"

#include <cmath>

namespace choco {

// the three kernels' sides (above)
enum AdamSide { kAdamPlain, kAdamMaster, kAdamSr };

constexpr uint32_t kAdamHasWd = 8u;  // derived on the host from the double, beside the ABI's three CHOCO_ADAM_F_* bits

// tensors per launch: four pointers, the offset, seven floats and two bytes a tensor -- the most
// the assert below lets through (ResNet-50's 161: three launches)
constexpr int kAdamCap = 54;

struct AdamTable {
  void* p[kAdamCap];
  void* g[kAdamCap];
  void* m[kAdamCap];
  void* v[kAdamCap];
  int64_t off[kAdamCap + 1];  // absolute flat offsets; off[nt] = end of the chunk
  float nss[kAdamCap], bs[kAdamCap], wdc[kAdamCap];  // -(lr / bc1), sqrt(bc2); decoupled: 1 - lr wd, coupled: wd
  float w[kAdamCap], b2[kAdamCap], omb2[kAdamCap], e[kAdamCap];  // 1 - beta1, beta2, 1 - beta2, eps
  uint8_t dt[kAdamCap];       // CHOCO_DT_*
  uint8_t fl[kAdamCap];       // CHOCO_ADAM_F_* | kAdamHasWd
  int32_t nt;
};
// the table, the flat / master and coef pointers, four words and (sr) ONE 8-byte key -- 40 of
// the 48 bytes: a launch carries at most 4 KB of arguments, and three keys would not fit
static_assert(sizeof(AdamTable) + 48 <= 4096 - 256, "AdamTable must fit in the kernel arguments");

// what one tensor's update needs (workgroup-uniform)
struct AdamTensor {
  void* p;
  void* g;
  void* m;
  void* v;
  int64_t o0;              // the tensor's flat offset
  float nss, bs, wdc, b2, omb2, e;
  float lw;                // lerp's coefficient: w, or -(1 - w) where w >= 0.5 (torch's second branch)
  bool lerp_small;         // w < 0.5: the base of the lerp is m, else g'
  int dt;
  bool has_wd, decoupled, first;
  bool pack_only;          // the plain kernel's NOGRAD tensor: flat = p, nothing else
  float* flat;             // plain: the flat output or null; master: the fp32 copy
  bool wr_p;               // the parameter tensor is written
  bool clip, wr_c;         // g' = c * g on the load; the product goes back into g (WRITE_CLIPPED)
  float gc;
  uint64_t key[3];         // param_adam_sr_kernel: the keys of the step's bit fields for p, m and v (lanes 0, 1, 2)
};

CHOCO_DEV AdamTensor adam_decode(const AdamTable& tb, int s) {
  const uint32_t fl = tb.fl[s];
  AdamTensor t = {};
  t.p = tb.p[s]; t.g = tb.g[s]; t.m = tb.m[s]; t.v = tb.v[s]; t.o0 = tb.off[s];
  t.nss = tb.nss[s]; t.bs = tb.bs[s]; t.wdc = tb.wdc[s]; t.b2 = tb.b2[s]; t.omb2 = tb.omb2[s]; t.e = tb.e[s];
  const float w = tb.w[s];
  t.lerp_small = w < 0.5f;
  t.lw = t.lerp_small ? w : -__fsub_rn(1.0f, w);
  t.dt = tb.dt[s];
  t.has_wd = (fl & kAdamHasWd) != 0;
  t.decoupled = (fl & CHOCO_ADAM_F_DECOUPLED) != 0;
  t.first = (fl & CHOCO_ADAM_F_FIRST) != 0;
  t.gc = 1.0f;
  return t;
}

// one element: the lines above after g' = c * g; DT the dtype every line is narrowed to
template <int DT>
CHOCO_DEV void adam_math(const AdamTensor& t, float p, float g, float& m, float& v, float& out) {
  if (t.has_wd) {
    if (t.decoupled) p = rnd<DT>(__fmul_rn(p, t.wdc));
    else g = rnd<DT>(fmaf(t.wdc, p, g));
  }
  const float d = __fsub_rn(g, m);
  m = rnd<DT>(fmaf(t.lw, d, t.lerp_small ? m : g));
  v = rnd<DT>(__fmul_rn(v, t.b2));
  const float tt = __fmul_rn(t.omb2, g);
  v = rnd<DT>(fmaf(tt, g, v));
  float den = rnd<DT>(sqrtf(v));
  den = rnd<DT>(__fdiv_rn(den, t.bs));
  den = rnd<DT>(__fadd_rn(den, t.e));
  const float q = __fdiv_rn(m, den);
  out = rnd<DT>(fmaf(t.nss, q, p));
}

// The update of one element and of one group (span_walk's body, param_common.h).
template <int DT, int SIDE>
struct AdamBody {
  static constexpr bool MASTER = SIDE == kAdamMaster;
  static constexpr bool SR = SIDE == kAdamSr && DT == CHOCO_DT_BF16;  // an fp32 tensor's sr update is the plain one
  static constexpr int MDT = MASTER ? CHOCO_DT_F32 : DT;              // the moments' dtype
  static constexpr int ADT = MASTER || SR ? CHOCO_DT_F32 : DT;        // the dtype every line is narrowed to
  const AdamTensor& t;

  // the gradient as the lines take it, from the loaded value
  CHOCO_DEV float grad(float g) const {
    if (!t.clip) return g;
    g = __fmul_rn(t.gc, g);
    if (!MASTER && !SR) return rnd<DT>(g);
    if (DT != CHOCO_DT_F32) asm("" : "+v"(g));  // a narrowing below starts from the rounded fp32 (see rnd)
    return g;
  }

  CHOCO_DEV void elem(int64_t i) const {
    const int64_t j = i - t.o0;
    const float p = MASTER ? t.flat[i] : ld1<DT>(t.p, j);
    if (!MASTER && t.pack_only) {
      t.flat[i] = p;  // the host has refused a pack-only launch without a flat side
      return;
    }
    const float g = grad(ld1<DT>(t.g, j));
    float m = t.first ? 0.0f : ld1<MDT>(t.m, j);
    float v = t.first ? 0.0f : ld1<MDT>(t.v, j);
    float out;
    if (t.wr_c) st1<DT>(t.g, j, g);
    adam_math<ADT>(t, p, g, m, v, out);
    if (MASTER && DT != CHOCO_DT_F32) asm("" : "+v"(out));  // the narrowing below starts from the rounded fp32
    if constexpr (SR) {
      st1_sr(t.m, j, m, t.key[1], i);
      st1_sr(t.v, j, v, t.key[2], i);
    } else {
      st1<MDT>(t.m, j, m);
      st1<MDT>(t.v, j, v);
    }
    if (MASTER || t.flat) t.flat[i] = out;
    if (!t.wr_p) return;
    if constexpr (SR) st1_sr(t.p, j, out, t.key[0], i);
    else st1<DT>(t.p, j, out);
  }

  CHOCO_DEV void group(int64_t e) const {
    const int64_t j = e - t.o0;
    Raw8 rp, rg, rm, rv;
    if (MASTER) ld8<CHOCO_DT_F32>(rp, t.flat, e);
    else ld8<DT>(rp, t.p, j);
    float p[8];
    if (!MASTER && t.pack_only) {
      widen8<DT>(rp, p);
      st8<CHOCO_DT_F32>(t.flat, e, p);
      return;
    }
    ld8<DT>(rg, t.g, j);
    if (!t.first) {
      ld8<MDT>(rm, t.m, j);
      ld8<MDT>(rv, t.v, j);
    }
    float g[8], m[8] = {0, 0, 0, 0, 0, 0, 0, 0}, v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, out[8];
    widen8<MDT>(rp, p);
    widen8<DT>(rg, g);
    if (!t.first) {
      widen8<MDT>(rm, m);
      widen8<MDT>(rv, v);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      g[k] = grad(g[k]);
      adam_math<ADT>(t, p[k], g[k], m[k], v[k], out[k]);
      if (MASTER && DT != CHOCO_DT_F32) asm("" : "+v"(out[k]));
    }
    if (t.wr_c) st8<DT>(t.g, j, g);
    if constexpr (SR) {
      st8_sr(t.m, j, m, t.key[1], e);
      st8_sr(t.v, j, v, t.key[2], e);
    } else {
      st8<MDT>(t.m, j, m);
      st8<MDT>(t.v, j, v);
    }
    if (MASTER || t.flat) st8<CHOCO_DT_F32>(t.flat, e, out);
    if (!t.wr_p) return;
    if constexpr (SR) st8_sr(t.p, j, out, t.key[0], e);
    else st8<DT>(t.p, j, out);
  }
};

// Is every whole group's start 16-byte aligned on every side the tensor touches (param_common.h's
// rule; the flat side is the caller's test)?  The element size is the tensor's own, but 4 for a
// master update's moments.
template <bool MASTER>
CHOCO_DEV bool adam_congruent(const AdamTensor& t) {
  const uintptr_t esz = dtype_size(t.dt);
  uintptr_t mis = 0;
  if (!MASTER || t.wr_p) mis |= mis16(t.p, esz, t.o0);
  if (MASTER || !t.pack_only) {
    mis |= mis16(t.g, esz, t.o0);
    mis |= mis16(t.m, MASTER ? 4u : esz, t.o0);
    mis |= mis16(t.v, MASTER ? 4u : esz, t.o0);
  }
  return on_grid16(mis);
}

// workgroup tile0 + blockIdx.x of a kernel; flat: the plain and sr kernels' flat output (or
// null), the master kernel's fp32 copy; flat16: it is 16-byte aligned (or absent); key0: the sr
// kernel's qrng_key(seed, step)
template <int SIDE>
CHOCO_DEV void adam_tile(const AdamTable& tb, float* flat, int64_t tile0, int32_t flat16, int32_t mode,
                         const float* coef, uint64_t key0 = 0) {
  constexpr bool MASTER = SIDE == kAdamMaster;
  const bool clip = coef != nullptr;
  const float gc = clip ? *coef : 1.0f;  // a uniform load
  // the moments' keys: two uniform mixes a workgroup (three keys do not fit the arguments)
  const uint64_t key1 = SIDE == kAdamSr ? sr_lane_key(key0, 1) : 0, key2 = SIDE == kAdamSr ? sr_lane_key(key0, 2) : 0;
  tile_walk(tb.off, tb.nt, tile0 + blockIdx.x, [&](int s, int64_t a, int64_t b) {
    AdamTensor t = adam_decode(tb, s);
    const bool nograd = (tb.fl[s] & CHOCO_ADAM_F_NOGRAD) != 0;
    if (nograd && (MASTER || flat == nullptr)) return;  // passed over: nothing of it is read or written
    t.pack_only = nograd;
    t.flat = flat;
    t.wr_p = !nograd && (mode & CHOCO_SGD_MODE_WRITE_PARAMS) != 0;
    t.clip = clip && !nograd;
    t.wr_c = t.clip && (mode & CHOCO_SGD_MODE_WRITE_CLIPPED) != 0;
    t.gc = gc;
    const bool vec = flat16 != 0 && adam_congruent<MASTER>(t);
    if constexpr (SIDE == kAdamSr) {
      t.key[0] = key0; t.key[1] = key1; t.key[2] = key2;
      // the host has refused fp16
      if (t.dt == CHOCO_DT_BF16) span_walk(AdamBody<CHOCO_DT_BF16, SIDE>{t}, a, b, vec);
      else span_walk(AdamBody<CHOCO_DT_F32, SIDE>{t}, a, b, vec);
    } else {
      for_dtype(t.dt, [&](auto DT) { span_walk(AdamBody<DT, SIDE>{t}, a, b, vec); });
    }
  });
}

__global__ __launch_bounds__(kPbThreads) void param_adam_kernel(const AdamTable tb, float* flat, int64_t tile0,
                                                                int32_t flat16, int32_t mode, const float* coef) {
  adam_tile<kAdamPlain>(tb, flat, tile0, flat16, mode, coef);
}

__global__ __launch_bounds__(kPbThreads) void param_adam_master_kernel(const AdamTable tb, float* master,
                                                                       int64_t tile0, int32_t master16, int32_t mode,
                                                                       const float* coef) {
  adam_tile<kAdamMaster>(tb, master, tile0, master16, mode, coef);
}

__global__ __launch_bounds__(kPbThreads) void param_adam_sr_kernel(const AdamTable tb, float* flat, int64_t tile0,
                                                                   int32_t flat16, int32_t mode, const float* coef,
                                                                   uint64_t key0) {
  adam_tile<kAdamSr>(tb, flat, tile0, flat16, mode, coef, key0);
}

// ------------------------------------------------------------------ the host side
struct AdamArgs {
  void* const* params;
  const void* const* grads;
  void* const* exp_avg;
  void* const* exp_avg_sq;
  const int64_t* lens;
  const int32_t* dtypes;
  const double* lr;
  const double* beta1;
  const double* beta2;
  const double* eps;
  const double* wd;
  const double* step;
  const int32_t* flags;
  int32_t nseg;
  float* flat;        // the flat output or null; master: the master copy
  int64_t n;
  int32_t mode;
  const float* coef;  // device, the global-norm clip coefficient (choco_params_gradnorm's out + 1), or null
  bool master;
  bool sr = false;       // choco_params_adam_sr
  uint64_t sr_key = 0;   // sr: qrng_key(seed, step), lane 0's key
};

// the mode bits, the flat side and the coefficient
static int adam_own_check(const AdamArgs& a) {
  const int32_t clipped = a.coef ? CHOCO_SGD_MODE_WRITE_CLIPPED : 0;
  CHOCO_REQUIRE(!((a.mode & CHOCO_SGD_MODE_WRITE_CLIPPED) && !a.coef), "WRITE_CLIPPED needs coef");
  CHOCO_REQUIRE((a.mode & ~(CHOCO_SGD_MODE_WRITE_PARAMS | clipped)) == 0,
                "the Adam update runs in apply mode, optionally | WRITE_PARAMS | WRITE_CLIPPED: unknown mode bits 0x%x",
                (unsigned)a.mode);
  if (a.master) CHOCO_REQUIRE(a.flat, "master is null");
  CHOCO_REQUIRE(a.flat || (a.mode & (CHOCO_SGD_MODE_WRITE_PARAMS | clipped)),
                "nothing to write: flat is null and the mode does not write the params");
  CHOCO_REQUIRE(aligned4(a.flat), "the %s buffer must be 4-byte aligned", a.master ? "master" : "flat");
  CHOCO_REQUIRE(aligned4(a.coef), "coef must be a 4-byte aligned device pointer");
  return CHOCO_OK;
}

// Every argument is checked before the first launch, with no HIP call.
static int adam_check(const AdamArgs& a) {
  CHOCO_REQUIRE(a.params && a.grads && a.exp_avg && a.exp_avg_sq && a.lens && a.dtypes && a.lr && a.beta1 && a.beta2 &&
                    a.eps && a.wd && a.step && a.flags,
                "null table argument");
  return layout_check(
      a.lens, a.dtypes, a.nseg, a.n, [&]() -> int { return adam_own_check(a); },
      [&](int32_t s, uintptr_t esz) -> int {
        const int i = (int)s;
        constexpr int32_t kFlags = CHOCO_ADAM_F_DECOUPLED | CHOCO_ADAM_F_FIRST | CHOCO_ADAM_F_NOGRAD;
        CHOCO_REQUIRE((a.flags[s] & ~kFlags) == 0, "tensor %d: unknown flag bits 0x%x", i, (unsigned)a.flags[s]);
        if (a.sr)
          CHOCO_REQUIRE(a.dtypes[s] != CHOCO_DT_F16,
                        "tensor %d: fp16 has no stochastic rounding (bf16 and fp32 tensors only)", i);
        const uintptr_t msz = a.master ? 4u : esz;  // a master update's moments are fp32
        CHOCO_REQUIRE(elem_aligned(a.params[s], esz) && elem_aligned(a.grads[s], esz) &&
                          elem_aligned(a.exp_avg[s], msz) && elem_aligned(a.exp_avg_sq[s], msz),
                      "tensor %d: pointer not aligned to its element size", i);
        if (a.lens[s] == 0) return CHOCO_OK;
        CHOCO_REQUIRE(a.params[s], "tensor %d: null param pointer", i);
        if (a.flags[s] & CHOCO_ADAM_F_NOGRAD) return CHOCO_OK;
        CHOCO_REQUIRE(a.grads[s], "tensor %d: null grad pointer without the no-grad flag", i);
        // FIRST: the moments are not read, but they are written
        CHOCO_REQUIRE(a.exp_avg[s] && a.exp_avg_sq[s], "tensor %d: null exp_avg or exp_avg_sq", i);
        // torch.optim.Adam's constructor refuses these
        CHOCO_REQUIRE(a.lr[s] >= 0.0 && std::isfinite(a.lr[s]), "tensor %d: lr must be finite and >= 0, got %g", i,
                      a.lr[s]);
        CHOCO_REQUIRE(a.beta1[s] >= 0.0 && a.beta1[s] < 1.0 && a.beta2[s] >= 0.0 && a.beta2[s] < 1.0,
                      "tensor %d: the betas must be in [0, 1), got %g and %g", i, a.beta1[s], a.beta2[s]);
        CHOCO_REQUIRE(a.eps[s] >= 0.0 && std::isfinite(a.eps[s]), "tensor %d: eps must be finite and >= 0, got %g", i,
                      a.eps[s]);
        CHOCO_REQUIRE(a.wd[s] >= 0.0 && std::isfinite(a.wd[s]), "tensor %d: weight_decay must be finite and >= 0, got %g",
                      i, a.wd[s]);
        CHOCO_REQUIRE(a.step[s] >= 1.0 && std::isfinite(a.step[s]),
                      "tensor %d: step (the count after the increment) must be >= 1, got %g", i, a.step[s]);
        return CHOCO_OK;
      });
}

static int adam_launches(int32_t nseg) { return chunk_launches(nseg, kAdamCap); }

static int adam_run(const AdamArgs& a, hipStream_t st) {
  CHOCO_TRY(adam_check(a));
  const int32_t flat16 = aligned16(a.flat) ? 1 : 0;  // a null flat side is aligned
  AdamTable tb;
  return for_chunks<kAdamCap>(a.lens, a.nseg, tb.off, [&](const Chunk& c) -> int {
    tb.nt = c.nt;
    for (int i = 0; i < kAdamCap; ++i) {
      const bool in = i < c.nt;
      const int32_t s = c.s0 + i;
      const bool upd = in && !(a.flags[s] & CHOCO_ADAM_F_NOGRAD);
      tb.p[i] = in ? a.params[s] : nullptr;
      tb.g[i] = upd ? const_cast<void*>(a.grads[s]) : nullptr;
      tb.m[i] = upd ? a.exp_avg[s] : nullptr;
      tb.v[i] = upd ? a.exp_avg_sq[s] : nullptr;
      tb.dt[i] = in ? (uint8_t)a.dtypes[s] : (uint8_t)0;
      uint32_t fl = in ? (uint32_t)a.flags[s] : 0u;
      float nss = 0, bs = 0, wdc = 0, w = 0, b2 = 0, omb2 = 0, e = 0;
      if (upd) {
        // torch.optim.adam._single_tensor_adam's Python doubles, each narrowed once as torch
        // narrows a Python scalar for an fp32 op
        const double bc1 = 1.0 - std::pow(a.beta1[s], a.step[s]);
        const double bc2 = 1.0 - std::pow(a.beta2[s], a.step[s]);
        const bool decoupled = (fl & CHOCO_ADAM_F_DECOUPLED) != 0;
        nss = (float)(-(a.lr[s] / bc1));
        bs = (float)std::pow(bc2, 0.5);
        wdc = decoupled ? (float)(1.0 - a.lr[s] * a.wd[s]) : (float)a.wd[s];
        w = (float)(1.0 - a.beta1[s]);
        b2 = (float)a.beta2[s];
        omb2 = (float)(1.0 - a.beta2[s]);
        e = (float)a.eps[s];
        if (a.wd[s] != 0.0) fl |= kAdamHasWd;
      }
      tb.nss[i] = nss; tb.bs[i] = bs; tb.wdc[i] = wdc; tb.w[i] = w; tb.b2[i] = b2; tb.omb2[i] = omb2; tb.e[i] = e;
      tb.fl[i] = (uint8_t)fl;
    }
    if (a.sr)
      return CHOCO_LAUNCH("param_adam_sr_kernel", "param_adam_sr_kernel", param_adam_sr_kernel,
                          dim3((unsigned)c.tiles), dim3(kPbThreads), st, tb, a.flat, c.tile0, flat16, a.mode, a.coef,
                          a.sr_key);
    return a.master ? CHOCO_LAUNCH("param_adam_master_kernel", "param_adam_master_kernel", param_adam_master_kernel,
                                   dim3((unsigned)c.tiles), dim3(kPbThreads), st, tb, a.flat, c.tile0, flat16, a.mode,
                                   a.coef)
                    : CHOCO_LAUNCH("param_adam_kernel", "param_adam_kernel", param_adam_kernel,
                                   dim3((unsigned)c.tiles), dim3(kPbThreads), st, tb, a.flat, c.tile0, flat16, a.mode,
                                   a.coef);
  });
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_adam_launches(int32_t nseg) { return adam_launches(nseg); }

CHOCO_API int choco_params_adam(void* const* params, const void* const* grads, void* const* exp_avg,
                                void* const* exp_avg_sq, const int64_t* lens, const int32_t* dtypes, const double* lr,
                                const double* beta1, const double* beta2, const double* eps,
                                const double* weight_decay, const double* step, const int32_t* flags, int32_t nseg,
                                float* flat, int64_t n, int32_t mode, const float* coef_or_null, void* stream) {
  const AdamArgs a{params, grads, exp_avg, exp_avg_sq, lens, dtypes, lr, beta1, beta2, eps,
                   weight_decay, step, flags, nseg,flat, n, mode, coef_or_null, false};
  return adam_run(a, as_stream(stream));
}

CHOCO_API int choco_params_adam_master(void* const* params, const void* const* grads, void* const* exp_avg,
                                       void* const* exp_avg_sq, const int64_t* lens, const int32_t* dtypes,
                                       const double* lr, const double* beta1, const double* beta2, const double* eps,
                                       const double* weight_decay, const double* step, const int32_t* flags,
                                       int32_t nseg, float* master, int64_t n, int32_t mode, const float* coef_or_null,
                                       void* stream) {
  const AdamArgs a{params, grads, exp_avg, exp_avg_sq, lens, dtypes, lr, beta1, beta2, eps,
                   weight_decay, step, flags, nseg,master, n, mode, coef_or_null, true};
  return adam_run(a, as_stream(stream));
}

CHOCO_API int choco_params_adam_sr(void* const* params, const void* const* grads, void* const* exp_avg,
                                   void* const* exp_avg_sq, const int64_t* lens, const int32_t* dtypes,
                                   const double* lr, const double* beta1, const double* beta2, const double* eps,
                                   const double* weight_decay, const double* step, const int32_t* flags, int32_t nseg,
                                   float* flat, int64_t n, int32_t mode, const float* coef_or_null, uint64_t sr_seed,
                                   uint64_t sr_step, void* stream) {
  AdamArgs a{params, grads, exp_avg, exp_avg_sq, lens, dtypes, lr, beta1, beta2, eps,
             weight_decay, step, flags, nseg, flat, n, mode, coef_or_null, false};
  a.sr = true;
  a.sr_key = qrng_key(sr_seed, sr_step);
  return adam_run(a, as_stream(stream));
}
