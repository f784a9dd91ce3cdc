// apply_gradient (dl_code/pcode/optim/utils.py:13-47), the SGD update every optimizer of the
// reference starts its step with, for a whole list of parameter tensors in one batched launch
// per chunk, fused with the pack into the flat fp32 buffer (flatten(),
// dl_code/pcode/utils/communication.py:58-76) that follows it in a CHOCO step.
//
// Per tensor s, element j, each line one reference op with one rounding (sgd_math):
//     d = g
//     if wd  != 0:  d   = fma(wd, p, d)                         d_p.add_(p, alpha=wd)
//     if mom != 0:  t   = buf_in * mom                          buf.mul_(momentum)
//                   buf = first ? fma(1, d, 0 * mom) : fma(1 - damp, d, t)
//                   d   = nesterov ? fma(mom, buf, d) : buf
//     apply mode:   p_new = fma(-lr, d, p)   -> params (optional), flat (optional)
//     grad mode:    d                        -> grads (optional),  flat (optional)
// `first`: the tensor has no momentum buffer yet; the reference builds it as
// zeros.mul_(mom).add_(d_p), so buf_in is never read.  A skipped op (wd == 0, mom == 0) is
// skipped, not run with a zero coefficient.  The arithmetic is written with fmaf / __fmul_rn:
// no contraction can merge the rounded buf * mom into its neighbour.
//
// Shared by the three kernel templates, written once:
//   the launch  the parameter bridge's shape (params.hip): workgroups own 8192-element tiles at
//               absolute flat offsets, the table of a chunk of tensors travels in the kernel
//               arguments (scalar loads), the first tensor of a tile is found by the same uniform
//               upper-bound search, zero-length tensors are skipped (tile_walk, param_common.h); row s of the
//               table becomes an SgdTensor (sgd_decode), and a kernel sets only what is its own.
//   the test    a tensor takes the 16-byte path when the kernel's flat buffers are 16-byte aligned
//               and every side the update touches is congruent with the group grid at that
//               side's own element size (sgd_congruent, on param_common.h's rule); the dtype switch (for_dtype).
//   the lines   sgd_math, and the host side: one check, one table build, one launch switch.
// Whole groups then move as 16-byte vectors, non-temporal, every load of a group issued before
// its first store; cut groups and every other tensor move element by element, coalesced.  The
// master and the flat-gradient kernels do that through the shared span walk (span_walk) and one element /
// group body (SgdBody), compiled for the tensor's dtype, the parameter side and the gradient
// source:
//     parameter side  the tensor itself: bf16 / fp16 lines are computed in fp32 from the widened
//                     operands and narrowed round-to-nearest-even to the storage dtype after each
//                     line (the scalars stay fp32).  Or MASTER, a persistent flat fp32 copy of a
//                     bf16 / fp16 model: p is master[i], the momentum buffer is fp32 whatever the
//                     tensor's dtype, nothing is narrowed between the lines, and the 16-bit
//                     parameter, where the mode writes it, is the new master value narrowed once,
//                     as param_unpack_kernel would narrow it.
//     gradient source the tensor's own g; or that times a coefficient, one fp32 multiply on the
//                     load the update does anyway (not narrowed in front of master arithmetic;
//                     WRITE_CLIPPED stores it, narrowed, back into g); or __fdiv_rn(gsum[i], div),
//                     the flat all-reduced sum over the world size, a correctly rounded division
//                     and never a reciprocal multiply (narrowed to the tensor's dtype except in
//                     front of master arithmetic; WRITE_GRADS stores it, narrowed, into g).
// param_sgd_kernel keeps a span walk and a body of its own (plain_span, plain_elem: optional
// sides, the flat output, kSgdU groups in flight with their loads ahead of a cut group's element
// path); on the shared walk it measured 11 to 14 % slower (see there).  Its stochastic-rounding
// instantiations ("param_sgd_sr_kernel", choco_params_sgd_sr; apply mode, bf16 and fp32 tensors)
// leave the parameter line in fp32 and round the one store that writes a bf16 parameter with 16
// bits that are a function of (seed, step, flat index) alone.  A launch writes only the
// bytes of its own elements.  g and buf of one tensor may be the same memory (the update is
// elementwise; where both are written, d is stored last); distinct tensors must not overlap,
// which is not checked.  The gradient norms these updates clip by: gradnorm.hip.
#include "param_common.h"

#include <cmath>

namespace choco {

constexpr int kSgdCap = 72;  // tensors per launch (ResNet-50's 161: three launches)
constexpr int kSgdU = 1;     // 8-element groups in flight per thread: three operands each, and more
                             // would take the fp32 build below the pack kernel's occupancy

struct SgdTable {
  void* p[kSgdCap];
  void* g[kSgdCap];
  void* buf[kSgdCap];
  int64_t off[kSgdCap + 1];  // absolute flat offsets; off[nt] = end of the chunk
  float wd[kSgdCap], mom[kSgdCap], omd[kSgdCap], nlr[kSgdCap];  // (float)wd, mom, 1 - damp, -lr
  uint8_t dt[kSgdCap];       // CHOCO_DT_*
  uint8_t fl[kSgdCap];       // CHOCO_SGD_F_* | kSgdHas* (param_common.h)
  int32_t nt;
};
// the table, the flat and norms pointers, four words and the stochastic-rounding key: a launch
// carries at most 4 KB of arguments
static_assert(sizeof(SgdTable) + 48 <= 4096 - 256, "SgdTable must fit in the kernel arguments");

// what one tensor's update needs (workgroup-uniform)
struct SgdTensor {
  // row s of the table (sgd_decode)
  void* p;
  void* g;
  void* buf;
  int64_t o0;              // the tensor's flat offset
  float wd, mom, omd, nlr;
  int dt;
  bool has_wd, has_mom, nesterov, first, nograd;
  bool rd_b, wr_b;         // the momentum buffer is read (not the first time) and written
  // the kernel's own; sgd_decode leaves "none" (null, false, coefficients of 1)
  float* flat;             // the plain kernels' flat side
  float* master;           // MASTER: the fp32 copy, read and written at flat indices
  const float* gsum;       // kGradFlat: the summed gradient at flat indices ...
  float div;               // ... and what it is divided by
  bool rd_p, rd_g;         // sides read: param_sgd_kernel's loads; everywhere, what sgd_congruent tests
  bool wr_p, wr_g;         // tensors written; wr_g stores `out`, in a kGradFlat kernel the averaged gradient
  bool grad_mode, pack_only;  // param_sgd_kernel's alone, as the four below
  bool clip, add_flat;     // choco_params_sgd_clip: d = c * d after the weight decay; flat += out
  float c;                 // the tensor's clip coefficient
  bool wr_c;               // kGradCoef: the clipped gradient goes back into g (WRITE_CLIPPED)
  float gc;                // ... and the coefficient
  uint64_t sr_key;         // param_sgd_sr_kernel: the key of the step's stochastic-rounding bits
};

CHOCO_DEV SgdTensor sgd_decode(const SgdTable& tb, int s) {
  const uint32_t fl = tb.fl[s];
  SgdTensor t = {};
  t.p = tb.p[s]; t.g = tb.g[s]; t.buf = tb.buf[s]; t.o0 = tb.off[s];
  t.wd = tb.wd[s]; t.mom = tb.mom[s]; t.omd = tb.omd[s]; t.nlr = tb.nlr[s];
  t.dt = tb.dt[s];
  t.has_wd = (fl & kSgdHasWd) != 0;
  t.has_mom = (fl & kSgdHasMom) != 0;
  t.nesterov = (fl & CHOCO_SGD_F_NESTEROV) != 0;
  t.first = (fl & CHOCO_SGD_F_FIRST) != 0;
  t.nograd = (fl & CHOCO_SGD_F_NOGRAD) != 0;
  t.rd_b = t.has_mom && !t.first;
  t.wr_b = t.has_mom;
  t.c = t.gc = 1.0f;
  return t;
}

// Is every whole group's start 16-byte aligned on every side the tensor touches (param_common.h's
// rule; the flat sides are the caller's test)?  The element size is the tensor's own, but 4 for a
// master update's momentum buffer.
template <bool MASTER>
CHOCO_DEV bool sgd_congruent(const SgdTensor& t) {
  const uintptr_t esz = dtype_size(t.dt);
  uintptr_t mis = 0;
  if (MASTER ? t.wr_p : t.rd_p || t.wr_p) mis |= mis16(t.p, esz, t.o0);
  if (t.rd_g || t.wr_g) mis |= mis16(t.g, esz, t.o0);
  if (t.rd_b || t.wr_b) mis |= mis16(t.buf, MASTER ? 4u : esz, t.o0);
  return on_grid16(mis);
}

// rnd<DT>(v), the value as the storage dtype holds it: param_common.h

// one element; out = what goes to params / grads and to flat.  SR (param_sgd_sr_kernel, apply
// mode): the parameter line is left in fp32, p_new = fma(-lr, d, p) unrounded -- flat takes it as
// it is and the parameter's store rounds it stochastically.
template <int DT, bool SR = false>
CHOCO_DEV void sgd_math(const SgdTensor& t, float p, float g, float b, float& buf_out, float& out) {
  if (t.pack_only) {
    out = p;
    return;
  }
  float d = g;
  if (t.has_wd) d = rnd<DT>(fmaf(t.wd, p, d));
  if (t.clip) d = rnd<DT>(__fmul_rn(t.c, d));
  if (t.has_mom) {
    float nb;
    if (t.first) {
      nb = rnd<DT>(fmaf(1.0f, d, __fmul_rn(0.0f, t.mom)));
    } else {
      const float m = rnd<DT>(__fmul_rn(b, t.mom));
      nb = rnd<DT>(fmaf(t.omd, d, m));
    }
    buf_out = nb;
    d = t.nesterov ? rnd<DT>(fmaf(t.mom, nb, d)) : nb;
  }
  if (SR) out = fmaf(t.nlr, d, p);
  else out = t.grad_mode ? d : rnd<DT>(fmaf(t.nlr, d, p));
}

enum SgdGrad { kGradOwn, kGradCoef, kGradFlat };  // the gradient source

// The update of one element and of one group, for the master and the flat-gradient kernels
// (span_walk's body, param_common.h).
template <int DT, bool MASTER, int GS>
struct SgdBody {
  static constexpr int MDT = MASTER ? CHOCO_DT_F32 : DT;  // the arithmetic's and the momentum buffer's dtype
  const SgdTensor& t;

  // the gradient as the lines take it, from the loaded value
  CHOCO_DEV float grad(float g) const {
    if (GS == kGradOwn) return g;
    g = GS == kGradCoef ? __fmul_rn(t.gc, g) : __fdiv_rn(g, t.div);
    if (!MASTER) return rnd<DT>(g);
    if (DT != CHOCO_DT_F32) asm("" : "+v"(g));  // a narrowing below starts from the rounded fp32 (see rnd)
    return g;
  }

  CHOCO_DEV void elem(int64_t i) const {
    const int64_t j = i - t.o0;
    const float p = MASTER ? t.master[i] : ld1<DT>(t.p, j);
    const float g = grad(GS == kGradFlat ? t.gsum[i] : ld1<DT>(t.g, j));
    const float b = t.rd_b ? ld1<MDT>(t.buf, j) : 0.0f;
    float nb = 0.0f, out;
    if (GS == kGradCoef && t.wr_c) st1<DT>(t.g, j, g);
    sgd_math<MDT>(t, p, g, b, nb, out);
    if (MASTER && DT != CHOCO_DT_F32) asm("" : "+v"(out));  // the narrowing below starts from the rounded fp32
    if (t.wr_b) st1<MDT>(t.buf, j, nb);
    if (MASTER) t.master[i] = out;
    if (t.wr_p) st1<DT>(t.p, j, out);
    if (GS == kGradFlat && t.wr_g) st1<DT>(t.g, j, g);
  }

  CHOCO_DEV void group(int64_t e) const {
    const int64_t j = e - t.o0;
    Raw8 rp, rg, rb;
    if (MASTER) ld8<CHOCO_DT_F32>(rp, t.master, e);
    else ld8<DT>(rp, t.p, j);
    if (GS == kGradFlat) ld8<CHOCO_DT_F32>(rg, t.gsum, e);
    else ld8<DT>(rg, t.g, j);
    if (t.rd_b) ld8<MDT>(rb, t.buf, j);
    float p[8], g[8], bi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float nb[8] = {0, 0, 0, 0, 0, 0, 0, 0}, out[8];
    widen8<MDT>(rp, p);
    widen8<GS == kGradFlat ? CHOCO_DT_F32 : DT>(rg, g);
    if (t.rd_b) widen8<MDT>(rb, bi);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      g[k] = grad(g[k]);
      sgd_math<MDT>(t, p[k], g[k], bi[k], nb[k], out[k]);
      if (MASTER && DT != CHOCO_DT_F32) asm("" : "+v"(out[k]));
    }
    if (GS == kGradCoef && t.wr_c) st8<DT>(t.g, j, g);
    if (t.wr_b) st8<MDT>(t.buf, j, nb);
    if (MASTER) st8<CHOCO_DT_F32>(t.master, e, out);
    if (t.wr_p) st8<DT>(t.p, j, out);
    if (GS == kGradFlat && t.wr_g) st8<DT>(t.g, j, g);
  }
};

// flat elements [a, b) of tensor t; flat16: the kernel's flat buffers are 16-byte aligned
template <bool MASTER, int GS>
CHOCO_DEV void sgd_span(const SgdTensor& t, int64_t a, int64_t b, bool flat16) {
  const bool vec = flat16 && sgd_congruent<MASTER>(t);
  for_dtype(t.dt, [&](auto DT) { span_walk(SgdBody<DT, MASTER, GS>{t}, a, b, vec); });
}

// ------------------------------------------------------------------ the update fused with the pack
// choco_params_sgd: the tensor's own arithmetic and gradient, with what only this kernel has: a
// flat output, grad mode, and pack-only (no-grad) tensors, whose parameter goes to flat as it is.
//
// EXT: the instantiation choco_params_sgd_clip launches (clip coefficients from norms[s] when
// norms != nullptr, ADD_FLAT); choco_params_sgd's own has neither compiled in.
// GC: the instantiation choco_params_sgd_gclip launches ("param_sgd_gclip_kernel"): `norms` is
// then coef, ONE float, the global-norm clip coefficient every gradient is scaled by, and thr is
// not used; the multiply is compiled into neither of the other two, whose argument list this is.
//
// SC ("param_sgd_scaled_kernel", choco_params_sgd_scaled; GC with it): `norms` is then the
// four floats choco_params_gradnorm_scaled leaves, the coefficient is norms[1] (the clip
// coefficient times 1 / loss scale) and norms[2] != 0 says the raw gradients held an inf or a NaN:
// the step is skipped on the device -- every tensor is a pack_only one (flat = p, nothing else
// written), and with no flat side the workgroup returns.  Both are uniform loads, one each per
// workgroup.  The test is compiled into that instantiation only.
//
// This family keeps a span walk and a body of its own under the shared launch, decode and test:
// its sides are optional (a pack-only tensor reads p alone, grad mode may not read p at all), it
// has the flat output with ADD_FLAT and the per-tensor clip, and its walk issues the loads of a
// thread's kSgdU groups in a phase of their own, ahead of a cut group's element path.  With
// plain_elem / plain_span written as a body for span_walk (the same lines behind load / update,
// loads ahead) the bf16 ResNet-50 update took 124.2 to 125.3 us against the 111.9 to 112.8 of
// the code before, the gclip instantiation 120.1 to 121.8 against 104.2 to 104.7, the clip one
// 133.4 to 133.5 against 118.7 to 119.8, in one visit; as below it took 108.0 to 111.8, 104.4 to
// 106.8 and 117.1 to 120.5.

// flat index i, element j of the tensor.  GC (the gclip kernel's instantiations): the gradient
// is clipped as it is loaded, g = rnd(gc * g), one fp32 multiply narrowed to the tensor's dtype.
// SR (the stochastic-rounding kernel's instantiations): sgd_math leaves p_new in fp32, and a
// bf16 parameter's store rounds it with the bits of flat index i (param_common.h st1_sr / st8_sr).
template <int DT, bool GC = false, bool SR = false>
CHOCO_DEV void plain_elem(const SgdTensor& t, int64_t i, int64_t j) {
  const float p = t.rd_p ? ld1<DT>(t.p, j) : 0.0f;
  float g = t.rd_g ? ld1<DT>(t.g, j) : 0.0f;
  const float b = t.rd_b ? ld1<DT>(t.buf, j) : 0.0f;
  float nb = 0.0f, out;
  if (GC) {
    g = rnd<DT>(__fmul_rn(t.gc, g));
    if (t.wr_c) st1<DT>(t.g, j, g);
  }
  sgd_math<DT, SR>(t, p, g, b, nb, out);
  if (t.wr_b) st1<DT>(t.buf, j, nb);
  if (t.wr_p) {
    if constexpr (SR && DT == CHOCO_DT_BF16) st1_sr(t.p, j, out, t.sr_key, i);
    else st1<DT>(t.p, j, out);
  }
  if (t.wr_g) st1<DT>(t.g, j, out);
  if (t.flat) t.flat[i] = t.add_flat ? t.flat[i] + out : out;
}

// Flat elements [a, b) of a tensor at flat offset o0, a < b inside this workgroup's tile.
// vec: every side the update touches is 16-byte aligned at every whole group's start.
template <int DT, bool GC = false, bool SR = false>
CHOCO_DEV void plain_span(const SgdTensor& t, int64_t o0, int64_t a, int64_t b, bool vec) {
  const int tid = threadIdx.x;
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) plain_elem<DT, GC, SR>(t, i, i - o0);
    return;
  }
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += (int64_t)kPbThreads * kSgdU) {
    bool full[kSgdU];
    Raw8 rp[kSgdU], rg[kSgdU], rb[kSgdU], rf[kSgdU];
    // every load of the thread's kSgdU groups is issued before the first store
#pragma unroll
    for (int u = 0; u < kSgdU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      full[u] = e >= a && e + kPbGroup <= b;
      if (full[u]) {
        if (t.rd_p) ld8<DT>(rp[u], t.p, e - o0);
        if (t.rd_g) ld8<DT>(rg[u], t.g, e - o0);
        if (t.rd_b) ld8<DT>(rb[u], t.buf, e - o0);
        if (t.add_flat) ld8<CHOCO_DT_F32>(rf[u], t.flat, e);
      }
    }
#pragma unroll
    for (int u = 0; u < kSgdU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      if (full[u]) {
        float p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, g[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        float nb[8] = {0, 0, 0, 0, 0, 0, 0, 0}, out[8];
        if (t.rd_p) widen8<DT>(rp[u], p);
        if (t.rd_g) widen8<DT>(rg[u], g);
        if (t.rd_b) widen8<DT>(rb[u], bi);
        if (GC) {
#pragma unroll
          for (int k = 0; k < 8; ++k) g[k] = rnd<DT>(__fmul_rn(t.gc, g[k]));
          if (t.wr_c) st8<DT>(t.g, e - o0, g);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) sgd_math<DT, SR>(t, p[k], g[k], bi[k], nb[k], out[k]);
        if (t.wr_b) st8<DT>(t.buf, e - o0, nb);
        if (t.wr_p) {
          if constexpr (SR && DT == CHOCO_DT_BF16) st8_sr(t.p, e - o0, out, t.sr_key, e);
          else st8<DT>(t.p, e - o0, out);
        }
        if (t.wr_g) st8<DT>(t.g, e - o0, out);
        if (t.add_flat) {
          float f[8];
          widen8<CHOCO_DT_F32>(rf[u], f);
#pragma unroll
          for (int k = 0; k < 8; ++k) out[k] = f[k] + out[k];
        }
        if (t.flat) st8<CHOCO_DT_F32>(t.flat, e, out);
      } else {
        // a group cut by the tensor's start or end (or past the span): its own elements only
        const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
        for (int64_t i = ea; i < eb; ++i) plain_elem<DT, GC, SR>(t, i, i - o0);
      }
    }
  }
}

// KEY: no argument at all (the argument lists above), or one SrKey ("param_sgd_sr_kernel",
// choco_params_sgd_sr; with GC where it is given a clip coefficient): the key of the step's
// stochastic-rounding bits.  The host has refused grad mode, ADD_FLAT and fp16 tensors.
struct SrKey {
  uint64_t key;
};

template <bool EXT, bool GC = false, bool SC = false, typename... KEY>
__global__ __launch_bounds__(kPbThreads) void param_sgd_kernel(const SgdTable tb, float* flat, int64_t tile0,
                                                               int32_t flat16, int32_t mode, const float* norms,
                                                               float thr, KEY... sr) {
  constexpr bool SR = sizeof...(KEY) != 0;
  uint64_t sr_key = 0;
  ((sr_key = sr.key), ...);
  const bool grad_mode = (mode & CHOCO_SGD_MODE_GRAD) != 0;
  const float gc = GC ? norms[SC ? 1 : 0] : 1.0f;  // a uniform load
  const bool found = SC && norms[2] != 0.0f;       // ... and another
  if (SC && found && flat == nullptr) return;
  tile_walk(tb.off, tb.nt, tile0 + blockIdx.x, [&](int s, int64_t a, int64_t b) {
    SgdTensor t = sgd_decode(tb, s);
    t.flat = flat;
    t.pack_only = t.nograd || (SC && found);
    t.grad_mode = grad_mode;
    t.clip = EXT && norms != nullptr && !t.pack_only;
    t.add_flat = EXT && (mode & CHOCO_SGD_MODE_ADD_FLAT) != 0;
    if (t.clip) {
      // threshold / grad_norm as torch computes it: grad_norm.reciprocal() * threshold, after an
      // fp32 comparison (a NaN norm compares false; an inf norm gives 0)
      const float nrm = norms[s];
      if (nrm >= thr) t.c = __fmul_rn(1.0f / nrm, thr);
    }
    t.rd_p = t.pack_only || t.has_wd || !grad_mode;
    t.rd_g = !t.pack_only;
    t.rd_b = !t.pack_only && t.rd_b;
    t.wr_b = !t.pack_only && t.wr_b;
    t.wr_p = !t.pack_only && !grad_mode && (mode & CHOCO_SGD_MODE_WRITE_PARAMS) != 0;
    t.wr_g = !t.pack_only && grad_mode && (mode & CHOCO_SGD_MODE_WRITE_GRADS) != 0;
    t.wr_c = GC && !t.pack_only && (mode & CHOCO_SGD_MODE_WRITE_CLIPPED) != 0;  // apply mode (the host's check)
    t.gc = gc;
    t.sr_key = sr_key;
    const bool vec = (flat == nullptr || flat16) && sgd_congruent<false>(t);
    for_dtype(t.dt, [&](auto DT) { plain_span<DT, GC, SR>(t, t.o0, a, b, vec); });
  });
}

// ------------------------------------------------------------------ fp32 master weights
// choco_params_sgd_master: the MASTER parameter side with the tensor's own gradient, widened
// (exact).  A NOGRAD tensor is passed over: neither its master slice nor its parameter is read
// or written.
//
// COEF: no argument at all (param_sgd_master_kernel, the argument list it always had), or one
// `const float*`, the global-norm clip coefficient ("param_sgd_master_gclip_kernel").
// Or one ScaledOut ("param_sgd_master_scaled_kernel", choco_params_sgd_master_scaled):
// choco_params_gradnorm_scaled's four floats -- the coefficient is out[1], and out[2] != 0 (an inf
// or a NaN among the raw gradients) makes the workgroup return before it touches anything.
struct ScaledOut {
  const float* out;
};
CHOCO_DEV float coef_of(const float* coef) { return *coef; }
CHOCO_DEV float coef_of(ScaledOut s) { return s.out[1]; }
CHOCO_DEV bool found_of(const float*) { return false; }
CHOCO_DEV bool found_of(ScaledOut s) { return s.out[2] != 0.0f; }

template <typename... COEF>
__global__ __launch_bounds__(kPbThreads) void param_sgd_master_kernel(const SgdTable tb, float* master, int64_t tile0,
                                                                      int32_t master16, int32_t mode, COEF... coef) {
  constexpr bool GC = sizeof...(COEF) != 0;
  float gc = 1.0f;
  ((gc = coef_of(coef)), ...);  // a uniform load
  if ((found_of(coef) || ...)) return;  // ... and, in the scaled instantiation alone, another
  tile_walk(tb.off, tb.nt, tile0 + blockIdx.x, [&](int s, int64_t a, int64_t b) {
    SgdTensor t = sgd_decode(tb, s);
    if (t.nograd) return;  // no gradient: passed over
    t.master = master;
    t.rd_g = true;
    t.wr_p = (mode & CHOCO_SGD_MODE_WRITE_PARAMS) != 0;
    t.wr_c = GC && (mode & CHOCO_SGD_MODE_WRITE_CLIPPED) != 0;
    t.gc = gc;
    sgd_span<true, GC ? kGradCoef : kGradOwn>(t, a, b, master16 != 0);
  });
}

// ------------------------------------------------------------------ all-reduce SGD: the flat summed gradient
// The centralized branch of SGD.step (dl_code/pcode/optim/sgd.py:68-92) after the all-reduce
// (choco_params_sgd_flatgrad, choco_params_sgd_master_flatgrad): the kGradFlat gradient source,
// gsum the flat fp32 buffer holding the all-reduced SUM with the `/ world_size` of
// _agg(op="avg") (communication.py:186-187) folded in, on either parameter side, in apply mode.
// WRITE_GRADS: grad[j] = the average narrowed, as flatten_grads.unpack(grads) narrows into the
// grad's dtype.  Every tensor has a gradient here (the flat buffer has no slot to skip: the host
// refuses NOGRAD).
//
// al16: bit 0 gsum, bit 1 master 16-byte aligned
// SLOT: no argument at all (param_sgd_flatgrad_kernel / param_sgd_master_flatgrad_kernel, the
// argument list they always had), or one FoundSlot ("param_sgd_flatgrad_scaled_kernel" /
// "param_sgd_master_flatgrad_scaled_kernel", choco_params_sgd[_master]_flatgrad_scaled): the
// address of gsum[n], the all-reduced sum of the ranks' overflow flags -- one uniform load per
// workgroup, and anything but zero (a NaN included) makes the workgroup return before it touches
// a parameter, a momentum buffer, a gradient or the master copy.
struct FoundSlot {
  const float* p;
};
CHOCO_DEV bool found_of(FoundSlot f) { return *f.p != 0.0f; }

template <bool MASTER, typename... SLOT>
__global__ __launch_bounds__(kPbThreads) void param_sgd_flatgrad_kernel(const SgdTable tb, const float* gsum,
                                                                        float* master, int64_t tile0, float div,
                                                                        int32_t al16, int32_t mode, SLOT... slot) {
  if ((found_of(slot) || ...)) return;  // in the scaled instantiations alone
  tile_walk(tb.off, tb.nt, tile0 + blockIdx.x, [&](int s, int64_t a, int64_t b) {
    SgdTensor t = sgd_decode(tb, s);
    t.gsum = gsum;
    t.master = master;
    t.div = div;
    t.rd_p = true;
    t.wr_p = (mode & CHOCO_SGD_MODE_WRITE_PARAMS) != 0;
    t.wr_g = (mode & CHOCO_SGD_MODE_WRITE_GRADS) != 0;
    sgd_span<MASTER, kGradFlat>(t, a, b, al16 == (MASTER ? 3 : 1));
  });
}

// ------------------------------------------------------------------ the host side
static int sgd_launches(int32_t nseg) { return chunk_launches(nseg, kSgdCap); }

// The gradient side of an entry point; with `master`, the parameter side, that names the kernel.
enum class SgdKind {
  Plain,           // choco_params_sgd[_master]
  Clip,            // choco_params_sgd_clip: the ADD_FLAT bit, norms and clip_threshold
  Gclip,           // choco_params_sgd[_master]_gclip: the WRITE_CLIPPED bit and coef
  Scaled,          // choco_params_sgd[_master]_scaled: Gclip whose coef is choco_params_gradnorm_scaled's out,
                   // four floats; the step is skipped on the device where out[2] != 0
  Flatgrad,        // choco_params_sgd[_master]_flatgrad: gsum and divisor
  FlatgradScaled,  // choco_params_sgd[_master]_flatgrad_scaled: gsum holds n + 1 elements, the last the flag
  Sr,              // choco_params_sgd_sr: apply mode, the parameter's store rounded stochastically; coef (or
                   // null) as Gclip's
};

struct SgdArgs {
  void* const* params;
  const void* const* grads;
  void* const* bufs;
  const int64_t* lens;
  const int32_t* dtypes;
  const double* lr;
  const double* wd;
  const double* mom;
  const double* damp;
  const int32_t* flags;
  int32_t nseg;
  float* flat;           // the flat buffer; master: the master copy (a flat-gradient update without: nullptr)
  int64_t n;
  int32_t mode;
  SgdKind kind;
  bool master;           // flat is the master copy, bufs are fp32
  // the kind's own operands
  const float* norms = nullptr;  // Clip: device, nseg per-tensor norms; nullptr: no clipping
  double clip_threshold = 0.0;
  const float* coef = nullptr;   // Gclip: device, the global-norm clip coefficient (choco_params_gradnorm's out + 1);
                                 // Scaled: choco_params_gradnorm_scaled's out
  const float* gsum = nullptr;   // Flatgrad*: the all-reduced sum, n fp32
  double divisor = 0.0;          // ... and what it is divided by
  uint64_t sr_key = 0;           // Sr: qrng_key(seed, step)

  bool gclip() const { return kind == SgdKind::Gclip || kind == SgdKind::Scaled || (kind == SgdKind::Sr && coef); }
  bool flatgrad() const { return kind == SgdKind::Flatgrad || kind == SgdKind::FlatgradScaled; }
};

// the fourteen arguments every entry point has
static SgdArgs sgd_args(SgdKind kind, bool master, void* const* params, const void* const* grads, void* const* bufs,
                        const int64_t* lens, const int32_t* dtypes, const double* lr, const double* wd,
                        const double* mom, const double* damp, const int32_t* flags, int32_t nseg, float* flat,
                        int64_t n, int32_t mode) {
  return SgdArgs{params, grads, bufs, lens, dtypes, lr, wd, mom, damp, flags, nseg, flat, n, mode, kind, master};
}

// the mode bits and the operands of a flat-gradient update (a.flat is the master copy or nullptr;
// a.grads, the table, may be null without WRITE_GRADS)
static int flatgrad_mode_check(const SgdArgs& a) {
  CHOCO_REQUIRE(!(a.mode & CHOCO_SGD_MODE_GRAD), "the flat-gradient update runs in apply mode: mode bits 0x%x",
                (unsigned)a.mode);
  CHOCO_REQUIRE((a.mode & ~(CHOCO_SGD_MODE_WRITE_PARAMS | CHOCO_SGD_MODE_WRITE_GRADS)) == 0, "unknown mode bits 0x%x",
                (unsigned)a.mode);
  CHOCO_REQUIRE(a.grads || !(a.mode & CHOCO_SGD_MODE_WRITE_GRADS), "WRITE_GRADS with a null grads table");
  CHOCO_REQUIRE(aligned4(a.gsum), "gsum must be 4-byte aligned");
  if (a.master) CHOCO_REQUIRE(a.flat && aligned4(a.flat), "master must be a 4-byte aligned device pointer");
  // tested as the kernel divides: by the fp32 value
  CHOCO_REQUIRE(std::isfinite(a.divisor) && (float)a.divisor != 0.0f && std::isfinite((float)a.divisor),
                "divisor must be finite and nonzero as an fp32 value, got %g", a.divisor);
  return CHOCO_OK;
}

// ... and of every other update
static int own_grad_mode_check(const SgdArgs& a) {
  const int32_t clipped = a.gclip() ? CHOCO_SGD_MODE_WRITE_CLIPPED : 0;
  const bool scaled = a.kind == SgdKind::Scaled;
  if (a.kind == SgdKind::Sr) {
    CHOCO_REQUIRE(!(a.mode & CHOCO_SGD_MODE_GRAD),
                  "the stochastic-rounding update runs in apply mode (grad mode stores no parameter): mode bits 0x%x",
                  (unsigned)a.mode);
    CHOCO_REQUIRE(!(a.mode & CHOCO_SGD_MODE_ADD_FLAT),
                  "ADD_FLAT and the per-tensor clip have no stochastic-rounding variant: mode bits 0x%x",
                  (unsigned)a.mode);
  }
  if (a.master) {
    CHOCO_REQUIRE((a.mode & ~(CHOCO_SGD_MODE_WRITE_PARAMS | clipped)) == 0,
                  "the master update runs in apply mode, optionally | WRITE_PARAMS%s: mode bits 0x%x",
                  a.gclip() ? " | WRITE_CLIPPED" : "", (unsigned)a.mode);
    CHOCO_REQUIRE(a.flat, "master is null");
  }
  constexpr int32_t kModes = CHOCO_SGD_MODE_GRAD | CHOCO_SGD_MODE_WRITE_PARAMS | CHOCO_SGD_MODE_WRITE_GRADS;
  if (a.gclip())
    CHOCO_REQUIRE(!(a.mode & CHOCO_SGD_MODE_ADD_FLAT), "ADD_FLAT has no %s variant",
                  scaled ? "loss-scaled" : "global-norm clipped");
  CHOCO_REQUIRE((a.mode & ~(kModes | (a.kind == SgdKind::Clip ? CHOCO_SGD_MODE_ADD_FLAT : 0) | clipped)) == 0,
                "unknown mode bits 0x%x", (unsigned)a.mode);
  const bool grad_mode = (a.mode & CHOCO_SGD_MODE_GRAD) != 0;
  if (scaled) {
    CHOCO_REQUIRE(a.coef && aligned4(a.coef), "out must be a 4-byte aligned device pointer");
    CHOCO_REQUIRE(!grad_mode, "the loss-scaled update runs in apply mode: mode bits 0x%x", (unsigned)a.mode);
  } else if (a.gclip()) {
    CHOCO_REQUIRE(a.coef && aligned4(a.coef), "coef must be a 4-byte aligned device pointer");
    CHOCO_REQUIRE(!(grad_mode && (a.mode & CHOCO_SGD_MODE_WRITE_CLIPPED)),
                  "WRITE_CLIPPED is for apply mode: grad mode writes d_p into the grads");
  }
  if (a.mode & CHOCO_SGD_MODE_ADD_FLAT)
    CHOCO_REQUIRE(grad_mode && a.flat, "ADD_FLAT needs grad mode and a flat buffer");
  if (a.norms) {
    CHOCO_REQUIRE(aligned4(a.norms), "norms must be 4-byte aligned");
    // tested as the kernel uses it: a positive double below fp32's range would clip against 0
    CHOCO_REQUIRE(a.clip_threshold <= 3.4028234663852886e38 && (float)a.clip_threshold > 0.0f,
                  "the clip threshold must be finite and > 0 as an fp32 value, got %g", a.clip_threshold);
  }
  CHOCO_REQUIRE(!(grad_mode && (a.mode & CHOCO_SGD_MODE_WRITE_PARAMS)), "grad mode does not write the params");
  CHOCO_REQUIRE(!(!grad_mode && (a.mode & CHOCO_SGD_MODE_WRITE_GRADS)), "apply mode does not write the grads");
  CHOCO_REQUIRE(a.flat || (a.mode & (CHOCO_SGD_MODE_WRITE_PARAMS | CHOCO_SGD_MODE_WRITE_GRADS | clipped)),
                "nothing to write: flat is null and the mode writes neither params nor grads");
  CHOCO_REQUIRE(aligned4(a.flat), "the %s buffer must be 4-byte aligned", a.master ? "master" : "flat");
  return CHOCO_OK;
}

// Every argument is checked before the first launch, with no HIP call.
static int sgd_check(const SgdArgs& a) {
  const bool fg = a.flatgrad();
  CHOCO_REQUIRE(a.params && (a.grads || fg) && a.bufs && a.lens && a.dtypes && a.lr && a.wd && a.mom && a.damp &&
                    a.flags,
                "null table argument");
  const bool grad_mode = (a.mode & CHOCO_SGD_MODE_GRAD) != 0;
  CHOCO_TRY(layout_check(
      a.lens, a.dtypes, a.nseg, a.n, [&]() -> int { return fg ? flatgrad_mode_check(a) : own_grad_mode_check(a); },
      [&](int32_t s, uintptr_t esz) -> int {
        const int i = (int)s;
        constexpr int32_t kFlags = CHOCO_SGD_F_NESTEROV | CHOCO_SGD_F_FIRST | CHOCO_SGD_F_NOGRAD;
        CHOCO_REQUIRE((a.flags[s] & ~kFlags) == 0, "tensor %d: unknown flag bits 0x%x", i, (unsigned)a.flags[s]);
        const bool nograd = (a.flags[s] & CHOCO_SGD_F_NOGRAD) != 0;
        if (a.kind == SgdKind::Sr)
          CHOCO_REQUIRE(a.dtypes[s] != CHOCO_DT_F16,
                        "tensor %d: fp16 has no stochastic rounding (bf16 and fp32 tensors only)", i);
        if (fg) CHOCO_REQUIRE(!nograd, "tensor %d: a no-grad tensor has no slot to skip in the flat gradient", i);
        CHOCO_REQUIRE(!(nograd && grad_mode), "tensor %d: a no-grad tensor in grad mode", i);
        CHOCO_REQUIRE(elem_aligned(a.params[s], esz) && (!a.grads || elem_aligned(a.grads[s], esz)) &&
                          elem_aligned(a.bufs[s], a.master ? 4u : esz),  // a master update's buffers are fp32
                      "tensor %d: pointer not aligned to its element size", i);
        if (!nograd) {
          // the reference's constructors refuse these (torch.optim.SGD's rule)
          CHOCO_REQUIRE(!((a.flags[s] & CHOCO_SGD_F_NESTEROV) && (!(a.mom[s] > 0.0) || a.damp[s] != 0.0)),
                        "tensor %d: nesterov needs momentum > 0 and dampening == 0", i);
        }
        if (a.lens[s] == 0) return CHOCO_OK;
        CHOCO_REQUIRE(a.params[s], "tensor %d: null param pointer", i);
        if (nograd) return CHOCO_OK;
        if (fg)
          CHOCO_REQUIRE(!(a.mode & CHOCO_SGD_MODE_WRITE_GRADS) || a.grads[s],
                        "tensor %d: null grad pointer with WRITE_GRADS", i);
        else
          CHOCO_REQUIRE(a.grads[s], "tensor %d: null grad pointer without the no-grad flag", i);
        CHOCO_REQUIRE(a.bufs[s] || a.mom[s] == 0.0, "tensor %d: null momentum buffer with momentum != 0", i);
        return CHOCO_OK;
      }));
  if (fg) CHOCO_REQUIRE((a.n == 0 && a.kind != SgdKind::FlatgradScaled) || a.gsum, "gsum is null");
  return CHOCO_OK;
}

// one launch of a chunk: KERNEL counts and is timed under `name`
template <auto KERNEL, typename... A>
static int sgd_launch(const char* name, int64_t tiles, hipStream_t st, const A&... args) {
  return CHOCO_LAUNCH(name, name, KERNEL, dim3((unsigned)tiles), dim3(kPbThreads), st, args...);
}

static int sgd_run(const SgdArgs& a, hipStream_t st) {
  CHOCO_TRY(sgd_check(a));
  const int32_t flat16 = aligned16(a.flat) ? 1 : 0;
  const int32_t al16 = (aligned16(a.gsum) ? 1 : 0) | (a.master ? 2 * flat16 : 0);
  const float div = (float)a.divisor;
  const float* const none = nullptr;
  SgdTable tb;
  return for_chunks<kSgdCap>(a.lens, a.nseg, tb.off, [&](const Chunk& c) -> int {
    const int32_t s0 = c.s0;
    const int64_t tile0 = c.tile0, tiles = c.tiles;
    tb.nt = c.nt;
    for (int i = 0; i < kSgdCap; ++i) {
      const bool in = i < c.nt;
      const int32_t s = s0 + i;
      const bool upd = in && !(a.flags[s] & CHOCO_SGD_F_NOGRAD);
      tb.p[i] = in ? a.params[s] : nullptr;
      tb.g[i] = upd && a.grads ? const_cast<void*>(a.grads[s]) : nullptr;
      tb.buf[i] = upd ? a.bufs[s] : nullptr;
      // torch's conversion of a Python scalar for an fp32 tensor
      tb.wd[i] = upd ? (float)a.wd[s] : 0.0f;
      tb.mom[i] = upd ? (float)a.mom[s] : 0.0f;
      tb.omd[i] = upd ? (float)(1.0 - a.damp[s]) : 0.0f;
      tb.nlr[i] = upd ? (float)(-a.lr[s]) : 0.0f;
      tb.dt[i] = in ? (uint8_t)a.dtypes[s] : (uint8_t)0;
      uint32_t fl = in ? (uint32_t)a.flags[s] : 0u;
      if (upd && a.wd[s] != 0.0) fl |= kSgdHasWd;
      if (upd && a.mom[s] != 0.0) fl |= kSgdHasMom;
      tb.fl[i] = (uint8_t)fl;
    }
    // the kernel of (kind, master) under its profile name, with its own argument list; a.flat is
    // the master copy where there is one, and null in a flat-gradient update without
    int rc = CHOCO_OK;
    switch (a.kind) {
      case SgdKind::Plain:
        rc = a.master ? sgd_launch<param_sgd_master_kernel<>>("param_sgd_master_kernel", tiles, st, tb, a.flat, tile0,
                                                              flat16, a.mode)
                      : sgd_launch<param_sgd_kernel<false>>("param_sgd_kernel", tiles, st, tb, a.flat, tile0, flat16,
                                                            a.mode, none, 0.0f);
        break;
      case SgdKind::Clip:  // counted with the plain kernel
        rc = CHOCO_LAUNCH("param_sgd_kernel", "param_sgd_kernel<clip>", param_sgd_kernel<true>, dim3((unsigned)tiles),
                          dim3(kPbThreads), st, tb, a.flat, tile0, flat16, a.mode, a.norms ? a.norms + s0 : none,
                          (float)a.clip_threshold);
        break;
      case SgdKind::Gclip:
        rc = a.master ? sgd_launch<param_sgd_master_kernel<const float*>>("param_sgd_master_gclip_kernel", tiles, st,
                                                                          tb, a.flat, tile0, flat16, a.mode, a.coef)
                      : sgd_launch<param_sgd_kernel<false, true>>("param_sgd_gclip_kernel", tiles, st, tb, a.flat,
                                                                  tile0, flat16, a.mode, a.coef, 0.0f);
        break;
      case SgdKind::Scaled:
        rc = a.master ? sgd_launch<param_sgd_master_kernel<ScaledOut>>("param_sgd_master_scaled_kernel", tiles, st, tb,
                                                                       a.flat, tile0, flat16, a.mode, ScaledOut{a.coef})
                      : sgd_launch<param_sgd_kernel<false, true, true>>("param_sgd_scaled_kernel", tiles, st, tb,
                                                                        a.flat, tile0, flat16, a.mode, a.coef, 0.0f);
        break;
      case SgdKind::Flatgrad:
        rc = a.master ? sgd_launch<param_sgd_flatgrad_kernel<true>>("param_sgd_master_flatgrad_kernel", tiles, st, tb,
                                                                    a.gsum, a.flat, tile0, div, al16, a.mode)
                      : sgd_launch<param_sgd_flatgrad_kernel<false>>("param_sgd_flatgrad_kernel", tiles, st, tb, a.gsum,
                                                                     a.flat, tile0, div, al16, a.mode);
        break;
      case SgdKind::FlatgradScaled:
        rc = a.master ? sgd_launch<param_sgd_flatgrad_kernel<true, FoundSlot>>(
                            "param_sgd_master_flatgrad_scaled_kernel", tiles, st, tb, a.gsum, a.flat, tile0, div, al16,
                            a.mode, FoundSlot{a.gsum + a.n})
                      : sgd_launch<param_sgd_flatgrad_kernel<false, FoundSlot>>(
                            "param_sgd_flatgrad_scaled_kernel", tiles, st, tb, a.gsum, a.flat, tile0, div, al16, a.mode,
                            FoundSlot{a.gsum + a.n});
        break;
      case SgdKind::Sr:  // both under one name
        rc = a.coef ? sgd_launch<param_sgd_kernel<false, true, false, SrKey>>("param_sgd_sr_kernel", tiles, st, tb,
                                                                             a.flat, tile0, flat16, a.mode, a.coef,
                                                                             0.0f, SrKey{a.sr_key})
                    : sgd_launch<param_sgd_kernel<false, false, false, SrKey>>("param_sgd_sr_kernel", tiles, st, tb,
                                                                              a.flat, tile0, flat16, a.mode, none,
                                                                              0.0f, SrKey{a.sr_key});
        break;
    }
    return rc;
  });
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_sgd_launches(int32_t nseg) { return sgd_launches(nseg); }
CHOCO_API int choco_params_sgd_master_launches(int32_t nseg) { return sgd_launches(nseg); }
CHOCO_API int choco_params_sgd_flatgrad_launches(int32_t nseg) { return sgd_launches(nseg); }

CHOCO_API int choco_params_sgd(void* const* params, const void* const* grads, void* const* bufs, const int64_t* lens,
                               const int32_t* dtypes, const double* lr, const double* weight_decay,
                               const double* momentum, const double* dampening, const int32_t* flags, int32_t nseg,
                               float* flat, int64_t n, int32_t mode, void* stream) {
  SgdArgs a = sgd_args(SgdKind::Plain, false, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, flat, n, mode);
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master(void* const* params, const void* const* grads, void* const* bufs,
                                      const int64_t* lens, const int32_t* dtypes, const double* lr,
                                      const double* weight_decay, const double* momentum, const double* dampening,
                                      const int32_t* flags, int32_t nseg, float* master, int64_t n, int32_t mode,
                                      void* stream) {
  SgdArgs a = sgd_args(SgdKind::Plain, true, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, master, n, mode);
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_clip(void* const* params, const void* const* grads, void* const* bufs,
                                    const int64_t* lens, const int32_t* dtypes, const double* lr,
                                    const double* weight_decay, const double* momentum, const double* dampening,
                                    const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                                    const float* norms, double clip_threshold, void* stream) {
  SgdArgs a = sgd_args(SgdKind::Clip, false, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, flat, n, mode);
  a.norms = norms;
  a.clip_threshold = clip_threshold;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_gclip(void* const* params, const void* const* grads, void* const* bufs,
                                     const int64_t* lens, const int32_t* dtypes, const double* lr,
                                     const double* weight_decay, const double* momentum, const double* dampening,
                                     const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                                     const float* coef, void* stream) {
  SgdArgs a = sgd_args(SgdKind::Gclip, false, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, flat, n, mode);
  a.coef = coef;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_sr(void* const* params, const void* const* grads, void* const* bufs,
                                  const int64_t* lens, const int32_t* dtypes, const double* lr,
                                  const double* weight_decay, const double* momentum, const double* dampening,
                                  const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                                  const float* coef_or_null, uint64_t seed, uint64_t step, void* stream) {
  SgdArgs a = sgd_args(SgdKind::Sr, false, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening,
                       flags, nseg, flat, n, mode);
  a.coef = coef_or_null;
  a.sr_key = qrng_key(seed, step);
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_gclip(void* const* params, const void* const* grads, void* const* bufs,
                                            const int64_t* lens, const int32_t* dtypes, const double* lr,
                                            const double* weight_decay, const double* momentum, const double* dampening,
                                            const int32_t* flags, int32_t nseg, float* master, int64_t n, int32_t mode,
                                            const float* coef, void* stream) {
  SgdArgs a = sgd_args(SgdKind::Gclip, true, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, master, n, mode);
  a.coef = coef;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_scaled(void* const* params, const void* const* grads, void* const* bufs,
                                      const int64_t* lens, const int32_t* dtypes, const double* lr,
                                      const double* weight_decay, const double* momentum, const double* dampening,
                                      const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                                      const float* out, void* stream) {
  SgdArgs a = sgd_args(SgdKind::Scaled, false, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, flat, n, mode);
  a.coef = out;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_scaled(void* const* params, const void* const* grads, void* const* bufs,
                                             const int64_t* lens, const int32_t* dtypes, const double* lr,
                                             const double* weight_decay, const double* momentum,
                                             const double* dampening, const int32_t* flags, int32_t nseg, float* master,
                                             int64_t n, int32_t mode, const float* out, void* stream) {
  SgdArgs a = sgd_args(SgdKind::Scaled, true, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, master, n, mode);
  a.coef = out;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_flatgrad(void* const* params, void* const* grads, void* const* bufs, const int64_t* lens,
                                        const int32_t* dtypes, const double* lr, const double* weight_decay,
                                        const double* momentum, const double* dampening, const int32_t* flags,
                                        int32_t nseg, const float* gsum, int64_t n, double divisor, int32_t mode,
                                        void* stream) {
  SgdArgs a = sgd_args(SgdKind::Flatgrad, false, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, nullptr, n, mode);
  a.gsum = gsum;
  a.divisor = divisor;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_flatgrad(void* const* params, void* const* grads, void* const* bufs,
                                               const int64_t* lens, const int32_t* dtypes, const double* lr,
                                               const double* weight_decay, const double* momentum,
                                               const double* dampening, const int32_t* flags, int32_t nseg,
                                               const float* gsum, float* master, int64_t n, double divisor,
                                               int32_t mode, void* stream) {
  SgdArgs a = sgd_args(SgdKind::Flatgrad, true, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, master, n, mode);
  a.gsum = gsum;
  a.divisor = divisor;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_flatgrad_scaled(void* const* params, void* const* grads, void* const* bufs,
                                               const int64_t* lens, const int32_t* dtypes, const double* lr,
                                               const double* weight_decay, const double* momentum,
                                               const double* dampening, const int32_t* flags, int32_t nseg,
                                               const float* gsum, int64_t n, double divisor, int32_t mode,
                                               void* stream) {
  SgdArgs a = sgd_args(SgdKind::FlatgradScaled, false, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, nullptr, n, mode);
  a.gsum = gsum;
  a.divisor = divisor;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_flatgrad_scaled(void* const* params, void* const* grads, void* const* bufs,
                                                      const int64_t* lens, const int32_t* dtypes, const double* lr,
                                                      const double* weight_decay, const double* momentum,
                                                      const double* dampening, const int32_t* flags, int32_t nseg,
                                                      const float* gsum, float* master, int64_t n, double divisor,
                                                      int32_t mode, void* stream) {
  SgdArgs a = sgd_args(SgdKind::FlatgradScaled, true, params, grads, bufs, lens, dtypes, lr, weight_decay, momentum,
                       dampening, flags, nseg, master, n, mode);
  a.gsum = gsum;
  a.divisor = divisor;
  return sgd_run(a, as_stream(stream));
}
