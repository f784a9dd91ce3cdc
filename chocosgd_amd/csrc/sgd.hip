// apply_gradient (dl_code/pcode/optim/utils.py:13-47), the SGD update every optimizer of the
// reference starts its step with, for a whole list of parameter tensors in one batched launch
// per chunk, fused with the pack into the flat fp32 buffer (flatten(),
// dl_code/pcode/utils/communication.py:58-76) that follows it in a CHOCO step.
//
// Per tensor s, element j, each line one reference op with one rounding:
//     d = g
//     if wd  != 0:  d   = fma(wd, p, d)                         d_p.add_(p, alpha=wd)
//     if mom != 0:  t   = buf_in * mom                          buf.mul_(momentum)
//                   buf = first ? fma(1, d, 0 * mom) : fma(1 - damp, d, t)
//                   d   = nesterov ? fma(mom, buf, d) : buf
//     apply mode:   p_new = fma(-lr, d, p)   -> params (optional), flat (optional)
//     grad mode:    d                        -> grads (optional),  flat (optional)
// `first`: the tensor has no momentum buffer yet; the reference builds it as
// zeros.mul_(mom).add_(d_p), so buf_in is never read.  A skipped op (wd == 0, mom == 0) is
// skipped, not run with a zero coefficient.  bf16 / fp16 tensors: every line is computed in
// fp32 from the widened operands and narrowed round-to-nearest-even to the storage dtype after
// that line (the scalars stay fp32); the flat value is the narrowed result widened again.
// The arithmetic is written with fmaf / __fmul_rn: no contraction can merge the rounded
// buf * mom into its neighbour.
//
// The launch has the parameter bridge's shape (params.hip): workgroups own 8192-element tiles
// at absolute flat offsets, the table of a chunk of tensors travels in the kernel arguments
// (scalar loads), the first tensor of a tile is found by the same uniform upper-bound search,
// zero-length tensors are skipped.  A tensor whose p, g, buf and flat sides (those the update
// touches) are all 16-byte aligned at group starts moves its whole groups as 16-byte vectors,
// kSgdU groups in flight per thread, non-temporal, every load issued before the first store;
// cut groups and every other tensor move element by element, coalesced.  A launch writes only
// the bytes of its own elements.  g and buf of one tensor may be the same memory (the update
// is elementwise; where both are written, d is stored last); distinct tensors must not
// overlap, which is not checked.
#include "param_common.h"

#include <algorithm>

namespace choco {

constexpr int kSgdCap = 72;  // tensors per launch (ResNet-50's 161: three launches)
constexpr int kSgdU = 1;     // 8-element groups in flight per thread: three operands each, and more
                             // would take the fp32 build below the pack kernel's occupancy

// flags of the table: the ABI's three bits, then what the host derives from the doubles
constexpr uint32_t kSgdHasWd = 8u, kSgdHasMom = 16u;

struct SgdTable {
  void* p[kSgdCap];
  void* g[kSgdCap];
  void* buf[kSgdCap];
  int64_t off[kSgdCap + 1];  // absolute flat offsets; off[nt] = end of the chunk
  float wd[kSgdCap], mom[kSgdCap], omd[kSgdCap], nlr[kSgdCap];  // (float)wd, mom, 1 - damp, -lr
  uint8_t dt[kSgdCap];       // CHOCO_DT_*
  uint8_t fl[kSgdCap];       // CHOCO_SGD_F_* | kSgdHas*
  int32_t nt;
};
// the table, the flat and norms pointers and four words: a launch carries at most 4 KB of arguments
static_assert(sizeof(SgdTable) + 40 <= 4096 - 256, "SgdTable must fit in the kernel arguments");

// what one tensor's update needs (workgroup-uniform)
struct SgdTensor {
  void* p;
  void* g;
  void* buf;
  float* flat;        // nullptr: no flat side
  float wd, mom, omd, nlr;
  bool has_wd, has_mom, nesterov, first;
  bool rd_p, rd_g, rd_b;   // operands read
  bool wr_p, wr_g, wr_b;   // tensors written (flat: flat != nullptr)
  bool grad_mode, pack_only;
  bool clip, add_flat;     // choco_params_sgd_clip: d = c * d after the weight decay; flat += out
  float c;                 // the tensor's clip coefficient
  bool wr_c;               // the gclip kernels: the clipped gradient goes back into g (WRITE_CLIPPED)
  float gc;                // ... and the global clip coefficient, *coef
};

// rnd<DT>(v), the value as the storage dtype holds it: param_common.h

// one element; out = what goes to params / grads and to flat
template <int DT>
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
  out = t.grad_mode ? d : rnd<DT>(fmaf(t.nlr, d, p));
}

// flat index i, element j of the tensor.  GC (the gclip kernel's instantiations): the gradient
// is clipped as it is loaded, g = rnd(gc * g), one fp32 multiply narrowed to the tensor's dtype.
template <int DT, bool GC = false>
CHOCO_DEV void sgd_elem(const SgdTensor& t, int64_t i, int64_t j) {
  const float p = t.rd_p ? ld1<DT>(t.p, j) : 0.0f;
  float g = t.rd_g ? ld1<DT>(t.g, j) : 0.0f;
  const float b = t.rd_b ? ld1<DT>(t.buf, j) : 0.0f;
  float nb = 0.0f, out;
  if (GC) {
    g = rnd<DT>(__fmul_rn(t.gc, g));
    if (t.wr_c) st1<DT>(t.g, j, g);
  }
  sgd_math<DT>(t, p, g, b, nb, out);
  if (t.wr_b) st1<DT>(t.buf, j, nb);
  if (t.wr_p) st1<DT>(t.p, j, out);
  if (t.wr_g) st1<DT>(t.g, j, out);
  if (t.flat) t.flat[i] = t.add_flat ? t.flat[i] + out : out;
}

// Flat elements [a, b) of a tensor at flat offset o0, a < b inside this workgroup's tile.
// vec: every side the update touches is 16-byte aligned at every whole group's start.
template <int DT, bool GC = false>
CHOCO_DEV void sgd_span(const SgdTensor& t, int64_t o0, int64_t a, int64_t b, bool vec) {
  const int tid = threadIdx.x;
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) sgd_elem<DT, GC>(t, i, i - o0);
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
        for (int k = 0; k < 8; ++k) sgd_math<DT>(t, p[k], g[k], bi[k], nb[k], out[k]);
        if (t.wr_b) st8<DT>(t.buf, e - o0, nb);
        if (t.wr_p) st8<DT>(t.p, e - o0, out);
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
        for (int64_t i = ea; i < eb; ++i) sgd_elem<DT, GC>(t, i, i - o0);
      }
    }
  }
}

// EXT: the instantiation choco_params_sgd_clip launches (clip coefficients from norms[s] when
// norms != nullptr, ADD_FLAT); choco_params_sgd's own has neither compiled in.
// GC: the instantiation choco_params_sgd_gclip launches ("param_sgd_gclip_kernel"): `norms` is
// then coef, ONE float, the global-norm clip coefficient every gradient is scaled by on the load
// the update does anyway, and thr is not used; the multiply is compiled into neither of the
// other two, whose argument list this is.
//
// SC ("param_sgd_scaled_kernel", choco_params_sgd_scaled; GC with it): `norms` is then the
// four floats choco_params_gradnorm_scaled leaves, the coefficient is norms[1] (the clip
// coefficient times 1 / loss scale) and norms[2] != 0 says the raw gradients held an inf or a NaN:
// the step is skipped on the device -- every tensor is a pack_only one (flat = p, nothing else
// written), and with no flat side the workgroup returns.  Both are uniform loads, one each per
// workgroup.  The test is compiled into that instantiation only.
template <bool EXT, bool GC = false, bool SC = false>
__global__ __launch_bounds__(kPbThreads) void param_sgd_kernel(const SgdTable tb, float* flat, int64_t tile0,
                                                               int32_t flat16, int32_t mode, const float* norms,
                                                               float thr) {
  const int nt = tb.nt;
  int64_t tlo, thi;
  const int s0 = tile_first_tensor(tb.off, nt, tile0 + blockIdx.x, tlo, thi);
  if (s0 < 0) return;
  const bool grad_mode = (mode & CHOCO_SGD_MODE_GRAD) != 0;
  const float gc = GC ? norms[SC ? 1 : 0] : 1.0f;  // a uniform load
  const bool found = SC && norms[2] != 0.0f;       // ... and another
  if (SC && found && flat == nullptr) return;
  for (int s = s0; s < nt; ++s) {
    const int64_t o0 = tb.off[s];
    if (o0 >= thi) break;
    const int64_t a = i64max(o0, tlo), b = i64min(tb.off[s + 1], thi);
    if (a >= b) continue;  // zero-length tensor
    const uint32_t fl = tb.fl[s];
    const int dt = tb.dt[s];
    SgdTensor t;
    t.p = tb.p[s]; t.g = tb.g[s]; t.buf = tb.buf[s]; t.flat = flat;
    t.wd = tb.wd[s]; t.mom = tb.mom[s]; t.omd = tb.omd[s]; t.nlr = tb.nlr[s];
    t.pack_only = (fl & CHOCO_SGD_F_NOGRAD) != 0 || (SC && found);
    t.has_wd = (fl & kSgdHasWd) != 0;
    t.has_mom = (fl & kSgdHasMom) != 0;
    t.nesterov = (fl & CHOCO_SGD_F_NESTEROV) != 0;
    t.first = (fl & CHOCO_SGD_F_FIRST) != 0;
    t.grad_mode = grad_mode;
    t.clip = EXT && norms != nullptr && !t.pack_only;
    t.add_flat = EXT && (mode & CHOCO_SGD_MODE_ADD_FLAT) != 0;
    t.c = 1.0f;
    if (t.clip) {
      // threshold / grad_norm as torch computes it: grad_norm.reciprocal() * threshold, after an
      // fp32 comparison (a NaN norm compares false; an inf norm gives 0)
      const float nrm = norms[s];
      if (nrm >= thr) t.c = __fmul_rn(1.0f / nrm, thr);
    }
    t.rd_p = t.pack_only || t.has_wd || !grad_mode;
    t.rd_g = !t.pack_only;
    t.rd_b = !t.pack_only && t.has_mom && !t.first;
    t.wr_b = !t.pack_only && t.has_mom;
    t.wr_p = !t.pack_only && !grad_mode && (mode & CHOCO_SGD_MODE_WRITE_PARAMS) != 0;
    t.wr_g = !t.pack_only && grad_mode && (mode & CHOCO_SGD_MODE_WRITE_GRADS) != 0;
    t.wr_c = GC && !t.pack_only && (mode & CHOCO_SGD_MODE_WRITE_CLIPPED) != 0;  // apply mode (the host's check)
    t.gc = gc;
    // flat + 4 e is 16-byte aligned at every group start e (a multiple of 8) when flat is; a
    // tensor's side q + esz (e - o0) is when q - esz o0 is, esz e being a multiple of 16
    const uintptr_t esz = dt == CHOCO_DT_F32 ? 4u : 2u, back = esz * (uintptr_t)o0;
    uintptr_t mis = 0;
    if (t.rd_p || t.wr_p) mis |= reinterpret_cast<uintptr_t>(t.p) - back;
    if (t.rd_g || t.wr_g) mis |= reinterpret_cast<uintptr_t>(t.g) - back;
    if (t.rd_b || t.wr_b) mis |= reinterpret_cast<uintptr_t>(t.buf) - back;
    const bool vec = (flat == nullptr || flat16) && (mis & 15u) == 0;
    if (dt == CHOCO_DT_F32) sgd_span<CHOCO_DT_F32, GC>(t, o0, a, b, vec);
    else if (dt == CHOCO_DT_BF16) sgd_span<CHOCO_DT_BF16, GC>(t, o0, a, b, vec);
    else sgd_span<CHOCO_DT_F16, GC>(t, o0, a, b, vec);
  }
}

// ------------------------------------------------------------------ fp32 master weights
// The same update on a persistent flat fp32 copy of a bf16 / fp16 model (choco_params_sgd_master):
// p is master[i], the momentum buffer is fp32 whatever the tensor's dtype, g is the tensor's own
// gradient widened (exact), the arithmetic is sgd_math<CHOCO_DT_F32> -- nothing is narrowed
// between the lines -- and the 16-bit parameter, where the mode writes it, is the new master value
// narrowed once, as param_unpack_kernel would narrow it.  A NOGRAD tensor is passed over: neither
// its master slice nor its parameter is read or written.  The launch has param_sgd_kernel's shape
// (same table, tiles and search).  The sides of one tensor have different element sizes here: a
// tensor takes the 16-byte path when master is 16-byte aligned and each side it touches is
// congruent with the group grid at that side's own element size -- g and p at the tensor's, buf
// at 4 bytes.

// flat index i, element j of the tensor
// GC (the gclip kernel's instantiations): g = gc * g in fp32, not narrowed, in front of the
// lines; WRITE_CLIPPED stores that product narrowed to the gradient's dtype.
template <int DT, bool GC = false>
CHOCO_DEV void master_elem(const SgdTensor& t, float* master, int64_t i, int64_t j) {
  const float p = master[i];
  float g = ld1<DT>(t.g, j);
  const float b = t.rd_b ? ld1<CHOCO_DT_F32>(t.buf, j) : 0.0f;
  float nb = 0.0f, out;
  if (GC) {
    g = __fmul_rn(t.gc, g);
    if (DT != CHOCO_DT_F32) asm("" : "+v"(g));  // the narrowing below starts from the rounded fp32 (see rnd)
    if (t.wr_c) st1<DT>(t.g, j, g);
  }
  sgd_math<CHOCO_DT_F32>(t, p, g, b, nb, out);
  if (DT != CHOCO_DT_F32) asm("" : "+v"(out));  // the narrowing below starts from the rounded fp32 (see rnd)
  if (t.wr_b) st1<CHOCO_DT_F32>(t.buf, j, nb);
  master[i] = out;
  if (t.wr_p) st1<DT>(t.p, j, out);
}

// Flat elements [a, b) of a tensor at flat offset o0, a < b inside this workgroup's tile; one
// 8-element group in flight per thread, every load issued before the first store.
template <int DT, bool GC = false>
CHOCO_DEV void master_span(const SgdTensor& t, float* master, int64_t o0, int64_t a, int64_t b, bool vec) {
  const int tid = threadIdx.x;
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) master_elem<DT, GC>(t, master, i, i - o0);
    return;
  }
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += kPbThreads) {
    const int64_t e = (gb + tid) * kPbGroup;
    if (e >= a && e + kPbGroup <= b) {
      Raw8 rp, rg, rb;
      ld8<CHOCO_DT_F32>(rp, master, e);
      ld8<DT>(rg, t.g, e - o0);
      if (t.rd_b) ld8<CHOCO_DT_F32>(rb, t.buf, e - o0);
      float p[8], g[8], bi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      float nb[8] = {0, 0, 0, 0, 0, 0, 0, 0}, out[8];
      widen8<CHOCO_DT_F32>(rp, p);
      widen8<DT>(rg, g);
      if (t.rd_b) widen8<CHOCO_DT_F32>(rb, bi);
      if (GC) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          g[k] = __fmul_rn(t.gc, g[k]);
          if (DT != CHOCO_DT_F32) asm("" : "+v"(g[k]));
        }
        if (t.wr_c) st8<DT>(t.g, e - o0, g);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        sgd_math<CHOCO_DT_F32>(t, p[k], g[k], bi[k], nb[k], out[k]);
        if (DT != CHOCO_DT_F32) asm("" : "+v"(out[k]));
      }
      if (t.wr_b) st8<CHOCO_DT_F32>(t.buf, e - o0, nb);
      st8<CHOCO_DT_F32>(master, e, out);
      if (t.wr_p) st8<DT>(t.p, e - o0, out);
    } else {
      // a group cut by the tensor's start or end (or past the span): its own elements only
      const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
      for (int64_t i = ea; i < eb; ++i) master_elem<DT, GC>(t, master, i, i - o0);
    }
  }
}

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
  const int nt = tb.nt;
  int64_t tlo, thi;
  const int s0 = tile_first_tensor(tb.off, nt, tile0 + blockIdx.x, tlo, thi);
  if (s0 < 0) return;
  float gc = 1.0f;
  ((gc = coef_of(coef)), ...);  // a uniform load
  if ((found_of(coef) || ...)) return;  // ... and, in the scaled instantiation alone, another
  for (int s = s0; s < nt; ++s) {
    const int64_t o0 = tb.off[s];
    if (o0 >= thi) break;
    const int64_t a = i64max(o0, tlo), b = i64min(tb.off[s + 1], thi);
    const uint32_t fl = tb.fl[s];
    if (a >= b || (fl & CHOCO_SGD_F_NOGRAD)) continue;  // zero-length, or no gradient: passed over
    const int dt = tb.dt[s];
    SgdTensor t;
    t.p = tb.p[s]; t.g = tb.g[s]; t.buf = tb.buf[s]; t.flat = nullptr;
    t.wd = tb.wd[s]; t.mom = tb.mom[s]; t.omd = tb.omd[s]; t.nlr = tb.nlr[s];
    t.pack_only = false;
    t.has_wd = (fl & kSgdHasWd) != 0;
    t.has_mom = (fl & kSgdHasMom) != 0;
    t.nesterov = (fl & CHOCO_SGD_F_NESTEROV) != 0;
    t.first = (fl & CHOCO_SGD_F_FIRST) != 0;
    t.grad_mode = false;
    t.clip = false; t.add_flat = false;
    t.c = 1.0f;
    t.rd_p = true; t.rd_g = true;
    t.rd_b = t.has_mom && !t.first;
    t.wr_b = t.has_mom;
    t.wr_p = (mode & CHOCO_SGD_MODE_WRITE_PARAMS) != 0;
    t.wr_g = false;
    t.wr_c = GC && (mode & CHOCO_SGD_MODE_WRITE_CLIPPED) != 0;
    t.gc = gc;
    // master + 4 e is 16-byte aligned at every group start e (a multiple of 8) when master is; a
    // side q + esz (e - o0) is when q - esz o0 is -- esz the tensor's for g and p, 4 for buf
    const uintptr_t esz = dt == CHOCO_DT_F32 ? 4u : 2u, o = (uintptr_t)o0;
    uintptr_t mis = reinterpret_cast<uintptr_t>(t.g) - esz * o;
    if (t.wr_p) mis |= reinterpret_cast<uintptr_t>(t.p) - esz * o;
    if (t.wr_b) mis |= reinterpret_cast<uintptr_t>(t.buf) - 4u * o;
    const bool vec = master16 && (mis & 15u) == 0;
    if (dt == CHOCO_DT_F32) master_span<CHOCO_DT_F32, GC>(t, master, o0, a, b, vec);
    else if (dt == CHOCO_DT_BF16) master_span<CHOCO_DT_BF16, GC>(t, master, o0, a, b, vec);
    else master_span<CHOCO_DT_F16, GC>(t, master, o0, a, b, vec);
  }
}



// ------------------------------------------------------------------ all-reduce SGD: the flat summed gradient
// The centralized branch of SGD.step (dl_code/pcode/optim/sgd.py:68-92) after the all-reduce
// (choco_params_sgd_flatgrad, choco_params_sgd_master_flatgrad): the gradient side of the update
// is gsum, the flat fp32 buffer holding the all-reduced SUM, and the `/ world_size` of
// _agg(op="avg") (communication.py:186-187) is folded in.  Per flat index i, element j:
//     a = __fdiv_rn(gsum[i], div)                a correctly rounded division, never a reciprocal multiply
//     16-bit / fp32 step:  g = rnd<DT>(a)        flatten_grads.unpack(grads) narrows into the grad's dtype
//                          sgd_math<DT>(p[j], g, buf[j]) in apply mode; WRITE_GRADS: grad[j] = g
//     master step:         g = a, not narrowed   sgd_math<F32>(master[i], g, buf32[j]); master[i] = p_new;
//                          WRITE_PARAMS: p[j] = narrow16(p_new); WRITE_GRADS: grad[j] = narrow16(a)
// Kernels of their own: param_sgd_kernel and param_sgd_master_kernel are not touched.  Same
// table, tiles and search; one 8-element group in flight per thread, every load issued before
// the first store.  A tensor takes the 16-byte path when gsum (and master) is 16-byte aligned
// and every side it touches is congruent with the group grid at that side's own element size:
// p, g and buf at the tensor's in the plain step; p and g at the tensor's, buf at 4 bytes in the
// master step.  Every tensor has a gradient here (the flat buffer has no slot to skip: the host
// refuses NOGRAD).

// flat index i, element j of the tensor
template <int DT, bool MASTER>
CHOCO_DEV void flatgrad_elem(const SgdTensor& t, const float* gsum, float* master, float div, int64_t i, int64_t j) {
  float a = __fdiv_rn(gsum[i], div);
  float nb = 0.0f, out;
  if (MASTER) {
    const float p = master[i];
    const float b = t.rd_b ? ld1<CHOCO_DT_F32>(t.buf, j) : 0.0f;
    sgd_math<CHOCO_DT_F32>(t, p, a, b, nb, out);
    if (DT != CHOCO_DT_F32) {  // the narrowings below start from the rounded fp32 values (see rnd)
      asm("" : "+v"(out));
      asm("" : "+v"(a));
    }
    if (t.wr_b) st1<CHOCO_DT_F32>(t.buf, j, nb);
    master[i] = out;
    if (t.wr_p) st1<DT>(t.p, j, out);
    if (t.wr_g) st1<DT>(t.g, j, a);
  } else {
    const float p = ld1<DT>(t.p, j);
    const float b = t.rd_b ? ld1<DT>(t.buf, j) : 0.0f;
    const float g = rnd<DT>(a);
    sgd_math<DT>(t, p, g, b, nb, out);
    if (t.wr_b) st1<DT>(t.buf, j, nb);
    if (t.wr_p) st1<DT>(t.p, j, out);
    if (t.wr_g) st1<DT>(t.g, j, g);
  }
}

// Flat elements [a, b) of a tensor at flat offset o0, a < b inside this workgroup's tile.
template <int DT, bool MASTER>
CHOCO_DEV void flatgrad_span(const SgdTensor& t, const float* gsum, float* master, float div, int64_t o0, int64_t a,
                             int64_t b, bool vec) {
  constexpr int BDT = MASTER ? CHOCO_DT_F32 : DT;  // the momentum buffer's dtype
  const int tid = threadIdx.x;
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) flatgrad_elem<DT, MASTER>(t, gsum, master, div, i, i - o0);
    return;
  }
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += kPbThreads) {
    const int64_t e = (gb + tid) * kPbGroup;
    if (e >= a && e + kPbGroup <= b) {
      Raw8 rs, rp, rb;
      ld8<CHOCO_DT_F32>(rs, gsum, e);
      if (MASTER) ld8<CHOCO_DT_F32>(rp, master, e);
      else ld8<DT>(rp, t.p, e - o0);
      if (t.rd_b) ld8<BDT>(rb, t.buf, e - o0);
      float g[8], p[8], bi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      float nb[8] = {0, 0, 0, 0, 0, 0, 0, 0}, out[8];
      widen8<CHOCO_DT_F32>(rs, g);
      widen8<MASTER ? CHOCO_DT_F32 : DT>(rp, p);
      if (t.rd_b) widen8<BDT>(rb, bi);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        g[k] = __fdiv_rn(g[k], div);
        if (MASTER) {
          sgd_math<CHOCO_DT_F32>(t, p[k], g[k], bi[k], nb[k], out[k]);
          if (DT != CHOCO_DT_F32) {
            asm("" : "+v"(out[k]));
            asm("" : "+v"(g[k]));
          }
        } else {
          g[k] = rnd<DT>(g[k]);
          sgd_math<DT>(t, p[k], g[k], bi[k], nb[k], out[k]);
        }
      }
      if (t.wr_b) st8<BDT>(t.buf, e - o0, nb);
      if (MASTER) st8<CHOCO_DT_F32>(master, e, out);
      if (t.wr_p) st8<DT>(t.p, e - o0, out);
      if (t.wr_g) st8<DT>(t.g, e - o0, g);
    } else {
      // a group cut by the tensor's start or end (or past the span): its own elements only
      const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
      for (int64_t i = ea; i < eb; ++i) flatgrad_elem<DT, MASTER>(t, gsum, master, div, i, i - o0);
    }
  }
}

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
  const int nt = tb.nt;
  int64_t tlo, thi;
  const int s0 = tile_first_tensor(tb.off, nt, tile0 + blockIdx.x, tlo, thi);
  if (s0 < 0) return;
  if ((found_of(slot) || ...)) return;  // in the scaled instantiations alone
  for (int s = s0; s < nt; ++s) {
    const int64_t o0 = tb.off[s];
    if (o0 >= thi) break;
    const int64_t a = i64max(o0, tlo), b = i64min(tb.off[s + 1], thi);
    if (a >= b) continue;  // zero-length tensor
    const uint32_t fl = tb.fl[s];
    const int dt = tb.dt[s];
    SgdTensor t;
    t.p = tb.p[s]; t.g = tb.g[s]; t.buf = tb.buf[s]; t.flat = nullptr;
    t.wd = tb.wd[s]; t.mom = tb.mom[s]; t.omd = tb.omd[s]; t.nlr = tb.nlr[s];
    t.pack_only = false;
    t.has_wd = (fl & kSgdHasWd) != 0;
    t.has_mom = (fl & kSgdHasMom) != 0;
    t.nesterov = (fl & CHOCO_SGD_F_NESTEROV) != 0;
    t.first = (fl & CHOCO_SGD_F_FIRST) != 0;
    t.grad_mode = false;
    t.clip = false; t.add_flat = false;
    t.c = 1.0f;
    t.rd_p = true; t.rd_g = false;
    t.rd_b = t.has_mom && !t.first;
    t.wr_b = t.has_mom;
    t.wr_p = (mode & CHOCO_SGD_MODE_WRITE_PARAMS) != 0;
    t.wr_g = (mode & CHOCO_SGD_MODE_WRITE_GRADS) != 0;
    // gsum + 4 e (and master + 4 e) is 16-byte aligned at every group start e (a multiple of 8)
    // when gsum is; a side q + esz (e - o0) is when q - esz o0 is -- esz the tensor's, but 4 for
    // the master step's buf
    const uintptr_t esz = dt == CHOCO_DT_F32 ? 4u : 2u, o = (uintptr_t)o0;
    uintptr_t mis = 0;
    if (!MASTER || t.wr_p) mis |= reinterpret_cast<uintptr_t>(t.p) - esz * o;
    if (t.wr_g) mis |= reinterpret_cast<uintptr_t>(t.g) - esz * o;
    if (t.wr_b) mis |= reinterpret_cast<uintptr_t>(t.buf) - (MASTER ? 4u : esz) * o;
    const bool vec = al16 == (MASTER ? 3 : 1) && (mis & 15u) == 0;
    if (dt == CHOCO_DT_F32) flatgrad_span<CHOCO_DT_F32, MASTER>(t, gsum, master, div, o0, a, b, vec);
    else if (dt == CHOCO_DT_BF16) flatgrad_span<CHOCO_DT_BF16, MASTER>(t, gsum, master, div, o0, a, b, vec);
    else flatgrad_span<CHOCO_DT_F16, MASTER>(t, gsum, master, div, o0, a, b, vec);
  }
}

static int sgd_launches(int32_t nseg) { return nseg <= 0 ? 0 : (nseg + kSgdCap - 1) / kSgdCap; }

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
  float* flat;
  int64_t n;
  int32_t mode;
  bool ext;              // choco_params_sgd_clip: the ADD_FLAT bit and the two arguments below
  const float* norms;    // device, nseg per-tensor norms; nullptr: no clipping
  double clip_threshold;
  bool master;           // choco_params_sgd_master: flat is the master copy, bufs are fp32
  const float* gsum;     // choco_params_sgd[_master]_flatgrad: the all-reduced sum, n fp32 (else nullptr)
  double divisor;        // ... and what it is divided by
  bool flatgrad;         // one of those two entry points
  bool gclip;            // choco_params_sgd[_master]_gclip: the WRITE_CLIPPED bit and the argument below
  const float* coef;     // device, the global-norm clip coefficient (choco_params_gradnorm's out + 1)
  bool scaled;           // choco_params_sgd[_master]_scaled (gclip with it): coef is choco_params_gradnorm_scaled's
                         // out, four floats, and the step is skipped on the device where out[2] != 0
  bool found_slot;       // choco_params_sgd[_master]_flatgrad_scaled: gsum holds n + 1 elements, the last the flag
};

static bool elem_aligned(const void* p, uintptr_t esz) { return (reinterpret_cast<uintptr_t>(p) & (esz - 1)) == 0; }

// choco_params_sgd_flatgrad / choco_params_sgd_master_flatgrad (a.flat is the
// master copy or nullptr; a.grads, the table, may be null without WRITE_GRADS)
static int flatgrad_check(const SgdArgs& a) {
  const bool wr_g = (a.mode & CHOCO_SGD_MODE_WRITE_GRADS) != 0;
  CHOCO_REQUIRE(a.params && a.bufs && a.lens && a.dtypes && a.lr && a.wd && a.mom && a.damp && a.flags,
                "null table argument");
  CHOCO_REQUIRE(a.nseg > 0, "nseg must be positive, got %d", (int)a.nseg);
  CHOCO_REQUIRE(a.n >= 0 && a.n <= (int64_t)INT32_MAX, "n must be in [0, 2^31), got %lld", (long long)a.n);
  CHOCO_REQUIRE(!(a.mode & CHOCO_SGD_MODE_GRAD), "the flat-gradient update runs in apply mode: mode bits 0x%x",
                (unsigned)a.mode);
  CHOCO_REQUIRE((a.mode & ~(CHOCO_SGD_MODE_WRITE_PARAMS | CHOCO_SGD_MODE_WRITE_GRADS)) == 0, "unknown mode bits 0x%x",
                (unsigned)a.mode);
  CHOCO_REQUIRE(a.grads || !wr_g, "WRITE_GRADS with a null grads table");
  CHOCO_REQUIRE(aligned4(a.gsum), "gsum must be 4-byte aligned");
  if (a.master) CHOCO_REQUIRE(a.flat && aligned4(a.flat), "master must be a 4-byte aligned device pointer");
  // tested as the kernel divides: by the fp32 value
  CHOCO_REQUIRE(std::isfinite(a.divisor) && (float)a.divisor != 0.0f && std::isfinite((float)a.divisor),
                "divisor must be finite and nonzero as an fp32 value, got %g", a.divisor);
  int64_t sum = 0;
  for (int32_t s = 0; s < a.nseg; ++s) {
    const int i = (int)s;
    CHOCO_REQUIRE(a.lens[s] >= 0, "tensor %d: negative length", i);
    CHOCO_REQUIRE(a.dtypes[s] >= CHOCO_DT_F32 && a.dtypes[s] <= CHOCO_DT_F16, "tensor %d: unknown dtype code %d", i,
                  (int)a.dtypes[s]);
    CHOCO_REQUIRE(a.lens[s] <= a.n - sum, "the lengths add up to more than n = %lld", (long long)a.n);
    sum += a.lens[s];
    constexpr int32_t kFlags = CHOCO_SGD_F_NESTEROV | CHOCO_SGD_F_FIRST | CHOCO_SGD_F_NOGRAD;
    CHOCO_REQUIRE((a.flags[s] & ~kFlags) == 0, "tensor %d: unknown flag bits 0x%x", i, (unsigned)a.flags[s]);
    CHOCO_REQUIRE(!(a.flags[s] & CHOCO_SGD_F_NOGRAD),
                  "tensor %d: a no-grad tensor has no slot to skip in the flat gradient", i);
    const uintptr_t esz = a.dtypes[s] == CHOCO_DT_F32 ? 4u : 2u;
    CHOCO_REQUIRE(elem_aligned(a.params[s], esz) && (!a.grads || elem_aligned(a.grads[s], esz)) &&
                      elem_aligned(a.bufs[s], a.master ? 4u : esz),  // a master update's buffers are fp32
                  "tensor %d: pointer not aligned to its element size", i);
    CHOCO_REQUIRE(!((a.flags[s] & CHOCO_SGD_F_NESTEROV) && (!(a.mom[s] > 0.0) || a.damp[s] != 0.0)),
                  "tensor %d: nesterov needs momentum > 0 and dampening == 0", i);
    if (a.lens[s] == 0) continue;
    CHOCO_REQUIRE(a.params[s], "tensor %d: null param pointer", i);
    CHOCO_REQUIRE(!wr_g || a.grads[s], "tensor %d: null grad pointer with WRITE_GRADS", i);
    CHOCO_REQUIRE(a.bufs[s] || a.mom[s] == 0.0, "tensor %d: null momentum buffer with momentum != 0", i);
  }
  CHOCO_REQUIRE(sum == a.n, "the lengths add up to %lld, n is %lld", (long long)sum, (long long)a.n);
  CHOCO_REQUIRE((a.n == 0 && !a.found_slot) || a.gsum, "gsum is null");
  return CHOCO_OK;
}

// Every argument is checked before the first launch, with no HIP call.
static int sgd_check(const SgdArgs& a) {
  CHOCO_REQUIRE(a.params && a.grads && a.bufs && a.lens && a.dtypes && a.lr && a.wd && a.mom && a.damp && a.flags,
                "null table argument");
  CHOCO_REQUIRE(a.nseg > 0, "nseg must be positive, got %d", (int)a.nseg);
  CHOCO_REQUIRE(a.n >= 0 && a.n <= (int64_t)INT32_MAX, "n must be in [0, 2^31), got %lld", (long long)a.n);
  const int32_t clipped = a.gclip ? CHOCO_SGD_MODE_WRITE_CLIPPED : 0;
  if (a.master) {
    CHOCO_REQUIRE((a.mode & ~(CHOCO_SGD_MODE_WRITE_PARAMS | clipped)) == 0,
                  "the master update runs in apply mode, optionally | WRITE_PARAMS%s: mode bits 0x%x",
                  a.gclip ? " | WRITE_CLIPPED" : "", (unsigned)a.mode);
    CHOCO_REQUIRE(a.flat, "master is null");
  }
  constexpr int32_t kModes = CHOCO_SGD_MODE_GRAD | CHOCO_SGD_MODE_WRITE_PARAMS | CHOCO_SGD_MODE_WRITE_GRADS;
  if (a.gclip)
    CHOCO_REQUIRE(!(a.mode & CHOCO_SGD_MODE_ADD_FLAT), "ADD_FLAT has no %s variant",
                  a.scaled ? "loss-scaled" : "global-norm clipped");
  CHOCO_REQUIRE((a.mode & ~(kModes | (a.ext ? CHOCO_SGD_MODE_ADD_FLAT : 0) | clipped)) == 0, "unknown mode bits 0x%x",
                (unsigned)a.mode);
  const bool grad_mode = (a.mode & CHOCO_SGD_MODE_GRAD) != 0;
  if (a.scaled) {
    CHOCO_REQUIRE(a.coef && aligned4(a.coef), "out must be a 4-byte aligned device pointer");
    CHOCO_REQUIRE(!grad_mode, "the loss-scaled update runs in apply mode: mode bits 0x%x", (unsigned)a.mode);
  } else if (a.gclip) {
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
  int64_t sum = 0;
  for (int32_t s = 0; s < a.nseg; ++s) {
    const int i = (int)s;
    CHOCO_REQUIRE(a.lens[s] >= 0, "tensor %d: negative length", i);
    CHOCO_REQUIRE(a.dtypes[s] >= CHOCO_DT_F32 && a.dtypes[s] <= CHOCO_DT_F16, "tensor %d: unknown dtype code %d", i,
                  (int)a.dtypes[s]);
    CHOCO_REQUIRE(a.lens[s] <= a.n - sum, "the lengths add up to more than n = %lld", (long long)a.n);
    sum += a.lens[s];
    constexpr int32_t kFlags = CHOCO_SGD_F_NESTEROV | CHOCO_SGD_F_FIRST | CHOCO_SGD_F_NOGRAD;
    CHOCO_REQUIRE((a.flags[s] & ~kFlags) == 0, "tensor %d: unknown flag bits 0x%x", i, (unsigned)a.flags[s]);
    const bool nograd = (a.flags[s] & CHOCO_SGD_F_NOGRAD) != 0;
    CHOCO_REQUIRE(!(nograd && grad_mode), "tensor %d: a no-grad tensor in grad mode", i);
    const uintptr_t esz = a.dtypes[s] == CHOCO_DT_F32 ? 4u : 2u;
    CHOCO_REQUIRE(elem_aligned(a.params[s], esz) && elem_aligned(a.grads[s], esz) &&
                      elem_aligned(a.bufs[s], a.master ? 4u : esz),  // a master update's buffers are fp32
                  "tensor %d: pointer not aligned to its element size", i);
    if (!nograd) {
      // the reference's constructors refuse these (torch.optim.SGD's rule)
      CHOCO_REQUIRE(!((a.flags[s] & CHOCO_SGD_F_NESTEROV) && (!(a.mom[s] > 0.0) || a.damp[s] != 0.0)),
                    "tensor %d: nesterov needs momentum > 0 and dampening == 0", i);
    }
    if (a.lens[s] == 0) continue;
    CHOCO_REQUIRE(a.params[s], "tensor %d: null param pointer", i);
    if (nograd) continue;
    CHOCO_REQUIRE(a.grads[s], "tensor %d: null grad pointer without the no-grad flag", i);
    CHOCO_REQUIRE(a.bufs[s] || a.mom[s] == 0.0, "tensor %d: null momentum buffer with momentum != 0", i);
  }
  CHOCO_REQUIRE(sum == a.n, "the lengths add up to %lld, n is %lld", (long long)sum, (long long)a.n);
  return CHOCO_OK;
}

static int sgd_run(const SgdArgs& a, hipStream_t st) {
  const int rc = a.flatgrad ? flatgrad_check(a) : sgd_check(a);
  if (rc) return rc;
  const int32_t flat16 = aligned16(a.flat) ? 1 : 0;
  SgdTable tb;
  int64_t base = 0;
  for (int32_t s0 = 0; s0 < a.nseg; s0 += kSgdCap) {
    const int nt = std::min<int32_t>(kSgdCap, a.nseg - s0);
    tb.nt = nt;
    tb.off[0] = base;
    for (int i = 0; i < kSgdCap; ++i) {
      const bool in = i < nt;
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
      base += in ? a.lens[s] : 0;
      tb.off[i + 1] = base;
    }
    // the tiles the chunk [off[0], off[nt]) touches; an empty chunk still takes its launch
    const int64_t tile0 = tb.off[0] / kPbTile;
    const int64_t tiles = tb.off[nt] > tb.off[0] ? (tb.off[nt] - 1) / kPbTile - tile0 + 1 : 1;
    const float* norms = a.norms ? a.norms + s0 : nullptr;
    const float thr = (float)a.clip_threshold;
    const int32_t al16 = (aligned16(a.gsum) ? 1 : 0) | (a.master ? 2 * flat16 : 0);
    if (a.flatgrad && a.found_slot && a.master)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_master_flatgrad_scaled_kernel", "param_sgd_master_flatgrad_scaled_kernel",
                             param_sgd_flatgrad_kernel<true, FoundSlot>, dim3((unsigned)tiles), dim3(kPbThreads), st,
                             tb, a.gsum, a.flat, tile0, (float)a.divisor, al16, a.mode, FoundSlot{a.gsum + a.n}));
    else if (a.flatgrad && a.found_slot)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_flatgrad_scaled_kernel", "param_sgd_flatgrad_scaled_kernel",
                             param_sgd_flatgrad_kernel<false, FoundSlot>, dim3((unsigned)tiles), dim3(kPbThreads), st,
                             tb, a.gsum, (float*)nullptr, tile0, (float)a.divisor, al16, a.mode,
                             FoundSlot{a.gsum + a.n}));
    else if (a.flatgrad && a.master)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_master_flatgrad_kernel", "param_sgd_master_flatgrad_kernel",
                             param_sgd_flatgrad_kernel<true>, dim3((unsigned)tiles), dim3(kPbThreads), st, tb, a.gsum,
                             a.flat, tile0, (float)a.divisor, al16, a.mode));
    else if (a.flatgrad)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_flatgrad_kernel", "param_sgd_flatgrad_kernel", param_sgd_flatgrad_kernel<false>,
                             dim3((unsigned)tiles), dim3(kPbThreads), st, tb, a.gsum, (float*)nullptr, tile0,
                             (float)a.divisor, al16, a.mode));
    else if (a.scaled && a.master)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_master_scaled_kernel", "param_sgd_master_scaled_kernel",
                             param_sgd_master_kernel<ScaledOut>, dim3((unsigned)tiles), dim3(kPbThreads), st, tb,
                             a.flat, tile0, flat16, a.mode, ScaledOut{a.coef}));
    else if (a.scaled)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_scaled_kernel", "param_sgd_scaled_kernel", param_sgd_kernel<false, true, true>,
                             dim3((unsigned)tiles), dim3(kPbThreads), st, tb, a.flat, tile0, flat16, a.mode, a.coef,
                             0.0f));
    else if (a.gclip && a.master)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_master_gclip_kernel", "param_sgd_master_gclip_kernel",
                             param_sgd_master_kernel<const float*>, dim3((unsigned)tiles), dim3(kPbThreads), st, tb,
                             a.flat, tile0, flat16, a.mode, a.coef));
    else if (a.gclip)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_gclip_kernel", "param_sgd_gclip_kernel", param_sgd_kernel<false, true>,
                             dim3((unsigned)tiles), dim3(kPbThreads), st, tb, a.flat, tile0, flat16, a.mode, a.coef,
                             0.0f));
    else if (a.master)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_master_kernel", "param_sgd_master_kernel", param_sgd_master_kernel<>,
                             dim3((unsigned)tiles), dim3(kPbThreads), st, tb, a.flat, tile0, flat16, a.mode));
    else if (a.ext)
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_kernel", "param_sgd_kernel<clip>", param_sgd_kernel<true>,
                             dim3((unsigned)tiles), dim3(kPbThreads), st, tb, a.flat, tile0, flat16, a.mode, norms,
                             thr));
    else
      CHOCO_TRY(CHOCO_LAUNCH("param_sgd_kernel", "param_sgd_kernel", param_sgd_kernel<false>, dim3((unsigned)tiles),
                             dim3(kPbThreads), st, tb, a.flat, tile0, flat16, a.mode, norms, thr));
  }
  return CHOCO_OK;
}

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

// ... the workgroup taking whole groups as 16-byte vectors
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
  int64_t tlo, thi;
  const int s0 = tile_first_tensor(tb.off, nt, tile, tlo, thi);
  if (s0 < 0) return;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  int nshort = 0;
  for (int s = s0; s < nt; ++s) {
    const int64_t o0 = tb.off[s];
    if (o0 >= thi) break;
    const int64_t a = i64max(o0, tlo), b = i64min(tb.off[s + 1], thi);
    const uint32_t fl = tb.fl[s];
    if (a >= b || (fl & CHOCO_SGD_F_NOGRAD)) continue;
    const int dt = tb.dt[s];
    const bool has_wd = (fl & kSgdHasWd) != 0;
    const float wd = tb.wd[s];
    const void* p = tb.p[s];
    const void* g = tb.g[s];
    double* slot = slots + (tile + seg0 + s);
    if (b - a <= kNormWaveMax) {
      const bool mine = (nshort & 3) == wave;
      ++nshort;
      if (!mine) continue;
      double acc;
      if (dt == CHOCO_DT_F32) acc = norm_scalar<CHOCO_DT_F32>(p, g, has_wd, wd, o0, a, b, lane, 64);
      else if (dt == CHOCO_DT_BF16) acc = norm_scalar<CHOCO_DT_BF16>(p, g, has_wd, wd, o0, a, b, lane, 64);
      else acc = norm_scalar<CHOCO_DT_F16>(p, g, has_wd, wd, o0, a, b, lane, 64);
      acc = wave_sum(acc);
      if (lane == 0) *slot = acc;
      continue;
    }
    const uintptr_t esz = dt == CHOCO_DT_F32 ? 4u : 2u, back = esz * (uintptr_t)o0;
    uintptr_t mis = reinterpret_cast<uintptr_t>(g) - back;
    if (has_wd) mis |= reinterpret_cast<uintptr_t>(p) - back;
    const bool vec = (mis & 15u) == 0;
    double acc;
    if (dt == CHOCO_DT_F32)
      acc = vec ? norm_vector<CHOCO_DT_F32>(p, g, has_wd, wd, o0, a, b)
                : norm_scalar<CHOCO_DT_F32>(p, g, has_wd, wd, o0, a, b, tid, kPbThreads);
    else if (dt == CHOCO_DT_BF16)
      acc = vec ? norm_vector<CHOCO_DT_BF16>(p, g, has_wd, wd, o0, a, b)
                : norm_scalar<CHOCO_DT_BF16>(p, g, has_wd, wd, o0, a, b, tid, kPbThreads);
    else
      acc = vec ? norm_vector<CHOCO_DT_F16>(p, g, has_wd, wd, o0, a, b)
                : norm_scalar<CHOCO_DT_F16>(p, g, has_wd, wd, o0, a, b, tid, kPbThreads);
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) *slot = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();  // red is reused by the next long span
  }
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
  float r = (float)sqrt(acc);
  if (dt == CHOCO_DT_BF16) r = rnd<CHOCO_DT_BF16>(r);
  else if (dt == CHOCO_DT_F16) r = rnd<CHOCO_DT_F16>(r);
  if (lane == 0) norms[s] = r;
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

// v as dtype dt (a CHOCO_DT_* code) holds it
CHOCO_DEV float rnd_as(float v, int dt) {
  if (dt == CHOCO_DT_BF16) return rnd<CHOCO_DT_BF16>(v);
  if (dt == CHOCO_DT_F16) return rnd<CHOCO_DT_F16>(v);
  return v;
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


static int norm_launches(int32_t nseg) { return nseg <= 0 ? 0 : (nseg + kNormCap - 1) / kNormCap + 1; }
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

static int norm_check(const NormArgs& a) {
  CHOCO_REQUIRE(a.params && a.grads && a.lens && a.dtypes && a.wd && a.flags, "null table argument");
  CHOCO_REQUIRE(a.nseg > 0, "nseg must be positive, got %d", (int)a.nseg);
  CHOCO_REQUIRE(a.n >= 0 && a.n <= (int64_t)INT32_MAX, "n must be in [0, 2^31), got %lld", (long long)a.n);
  CHOCO_REQUIRE(a.norms && aligned4(a.norms), "norms must be a 4-byte aligned device pointer");
  CHOCO_REQUIRE(a.ws && (reinterpret_cast<uintptr_t>(a.ws) & 7u) == 0, "the workspace must be 8-byte aligned");
  if (a.ws_bytes < norm_ws_bytes(a.nseg, a.n))
    return fail(CHOCO_ERR_WORKSPACE, "workspace too small: %zu bytes, need %zu", a.ws_bytes,
                norm_ws_bytes(a.nseg, a.n));
  int64_t sum = 0;
  for (int32_t s = 0; s < a.nseg; ++s) {
    const int i = (int)s;
    CHOCO_REQUIRE(a.lens[s] >= 0, "tensor %d: negative length", i);
    CHOCO_REQUIRE(a.dtypes[s] >= CHOCO_DT_F32 && a.dtypes[s] <= CHOCO_DT_F16, "tensor %d: unknown dtype code %d", i,
                  (int)a.dtypes[s]);
    CHOCO_REQUIRE(a.lens[s] <= a.n - sum, "the lengths add up to more than n = %lld", (long long)a.n);
    sum += a.lens[s];
    constexpr int32_t kFlags = CHOCO_SGD_F_NESTEROV | CHOCO_SGD_F_FIRST | CHOCO_SGD_F_NOGRAD;
    CHOCO_REQUIRE((a.flags[s] & ~kFlags) == 0, "tensor %d: unknown flag bits 0x%x", i, (unsigned)a.flags[s]);
    const uintptr_t esz = a.dtypes[s] == CHOCO_DT_F32 ? 4u : 2u;
    CHOCO_REQUIRE(elem_aligned(a.params[s], esz) && elem_aligned(a.grads[s], esz),
                  "tensor %d: pointer not aligned to its element size", i);
    if (a.lens[s] == 0 || (a.flags[s] & CHOCO_SGD_F_NOGRAD)) continue;
    CHOCO_REQUIRE(a.grads[s], "tensor %d: null grad pointer without the no-grad flag", i);
    CHOCO_REQUIRE(a.params[s] || a.wd[s] == 0.0, "tensor %d: null param pointer with weight decay != 0", i);
  }
  CHOCO_REQUIRE(sum == a.n, "the lengths add up to %lld, n is %lld", (long long)sum, (long long)a.n);
  return CHOCO_OK;
}

// the norm pass: one param_sqnorm_kernel launch per chunk (a.params / a.wd null: raw gradients)
static int norm_pass(const NormArgs& a, double* slots, int32_t* meta, hipStream_t st) {
  NormTable tb;
  int64_t base = 0;
  for (int32_t s0 = 0; s0 < a.nseg; s0 += kNormCap) {
    const int nt = std::min<int32_t>(kNormCap, a.nseg - s0);
    tb.nt = nt;
    tb.off[0] = base;
    for (int i = 0; i < kNormCap; ++i) {
      const bool in = i < nt;
      const int32_t s = s0 + i;
      const bool upd = in && !(a.flags[s] & CHOCO_SGD_F_NOGRAD);
      tb.p[i] = upd && a.params ? a.params[s] : nullptr;
      tb.g[i] = upd ? a.grads[s] : nullptr;
      tb.wd[i] = upd && a.wd ? (float)a.wd[s] : 0.0f;
      tb.dt[i] = in ? (uint8_t)a.dtypes[s] : (uint8_t)0;
      uint32_t fl = in ? (uint32_t)(a.flags[s] & CHOCO_SGD_F_NOGRAD) : 0u;
      if (upd && a.wd && a.wd[s] != 0.0) fl |= kSgdHasWd;
      tb.fl[i] = (uint8_t)fl;
      base += in ? a.lens[s] : 0;
      tb.off[i + 1] = base;
    }
    const int64_t tile0 = tb.off[0] / kPbTile;
    const int64_t tiles = tb.off[nt] > tb.off[0] ? (tb.off[nt] - 1) / kPbTile - tile0 + 1 : 1;
    CHOCO_TRY(CHOCO_LAUNCH("param_sqnorm_kernel", "param_sqnorm_kernel", param_sqnorm_kernel, dim3((unsigned)tiles),
                           dim3(kPbThreads), st, tb, slots, meta + 2 * (size_t)s0, tile0, s0));
  }
  return CHOCO_OK;
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
  return nseg <= 0 ? 0 : pinned ? 1 : (nseg + kNormCap - 1) / kNormCap + 1;
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
  CHOCO_REQUIRE(a.nseg > 0, "nseg must be positive, got %d", (int)a.nseg);
  CHOCO_REQUIRE(a.n >= 0 && a.n <= (int64_t)INT32_MAX, "n must be in [0, 2^31), got %lld", (long long)a.n);
  // tested as the kernel uses it: the fp32 value (a scaled call without a clip does not use it)
  if (!a.scaled || a.ls.has_clip)
    CHOCO_REQUIRE(a.max_norm >= 0.0 && a.max_norm <= 3.4028234663852886e38,
                  "max_norm must be >= 0 and finite as an fp32 value, got %g", a.max_norm);
  if (a.scaled) {
    const int rc = loss_scale_check(a.ls);
    if (rc) return rc;
    CHOCO_REQUIRE(a.ls.has_clip == 0 || a.ls.has_clip == 1, "has_clip must be 0 or 1, got %d", (int)a.ls.has_clip);
  }
  CHOCO_REQUIRE(a.coef_dtype >= CHOCO_DT_F32 && a.coef_dtype <= CHOCO_DT_F16, "unknown coef_dtype code %d",
                (int)a.coef_dtype);
  CHOCO_REQUIRE(a.out && aligned4(a.out), "out must be a 4-byte aligned device pointer");
  CHOCO_REQUIRE(aligned4(a.norms), "norms must be 4-byte aligned");
  if (a.total_in) {  // parity mode: nothing of the layout is read
    CHOCO_REQUIRE(aligned4(a.total_in), "total_in must be 4-byte aligned");
    CHOCO_REQUIRE(!a.norms, "norms with a pinned total: there is no norm pass to take them from");
    return CHOCO_OK;
  }
  CHOCO_REQUIRE(a.grads && a.lens && a.dtypes && a.flags, "null table argument");
  CHOCO_REQUIRE(a.ws && (reinterpret_cast<uintptr_t>(a.ws) & 7u) == 0, "the workspace must be 8-byte aligned");
  if (a.ws_bytes < gradnorm_ws_bytes(a.nseg, a.n))
    return fail(CHOCO_ERR_WORKSPACE, "workspace too small: %zu bytes, need %zu", a.ws_bytes,
                gradnorm_ws_bytes(a.nseg, a.n));
  int64_t sum = 0;
  for (int32_t s = 0; s < a.nseg; ++s) {
    const int i = (int)s;
    CHOCO_REQUIRE(a.lens[s] >= 0, "tensor %d: negative length", i);
    CHOCO_REQUIRE(a.dtypes[s] >= CHOCO_DT_F32 && a.dtypes[s] <= CHOCO_DT_F16, "tensor %d: unknown dtype code %d", i,
                  (int)a.dtypes[s]);
    CHOCO_REQUIRE(a.lens[s] <= a.n - sum, "the lengths add up to more than n = %lld", (long long)a.n);
    sum += a.lens[s];
    constexpr int32_t kFlags = CHOCO_SGD_F_NESTEROV | CHOCO_SGD_F_FIRST | CHOCO_SGD_F_NOGRAD;
    CHOCO_REQUIRE((a.flags[s] & ~kFlags) == 0, "tensor %d: unknown flag bits 0x%x", i, (unsigned)a.flags[s]);
    CHOCO_REQUIRE(elem_aligned(a.grads[s], a.dtypes[s] == CHOCO_DT_F32 ? 4u : 2u),
                  "tensor %d: pointer not aligned to its element size", i);
    if (a.lens[s] == 0 || (a.flags[s] & CHOCO_SGD_F_NOGRAD)) continue;
    CHOCO_REQUIRE(a.grads[s], "tensor %d: null grad pointer without the no-grad flag", i);
  }
  CHOCO_REQUIRE(sum == a.n, "the lengths add up to %lld, n is %lld", (long long)sum, (long long)a.n);
  return CHOCO_OK;
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

CHOCO_API int choco_params_sgd_launches(int32_t nseg) { return sgd_launches(nseg); }

CHOCO_API int choco_params_sgd(void* const* params, const void* const* grads, void* const* bufs, const int64_t* lens,
                               const int32_t* dtypes, const double* lr, const double* weight_decay,
                               const double* momentum, const double* dampening, const int32_t* flags, int32_t nseg,
                               float* flat, int64_t n, int32_t mode, void* stream) {
  const SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, flat, n, mode,
                  false, nullptr, 0.0, false};
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_launches(int32_t nseg) { return sgd_launches(nseg); }

CHOCO_API int choco_params_sgd_master(void* const* params, const void* const* grads, void* const* bufs,
                                      const int64_t* lens, const int32_t* dtypes, const double* lr,
                                      const double* weight_decay, const double* momentum, const double* dampening,
                                      const int32_t* flags, int32_t nseg, float* master, int64_t n, int32_t mode,
                                      void* stream) {
  const SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, master, n,
                  mode, false, nullptr, 0.0, true};
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_flatgrad_launches(int32_t nseg) { return sgd_launches(nseg); }

CHOCO_API int choco_params_sgd_flatgrad(void* const* params, void* const* grads, void* const* bufs,
                                        const int64_t* lens, const int32_t* dtypes, const double* lr,
                                        const double* weight_decay, const double* momentum, const double* dampening,
                                        const int32_t* flags, int32_t nseg, const float* gsum, int64_t n,
                                        double divisor, int32_t mode, void* stream) {
  SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, nullptr, n, mode,
            false, nullptr, 0.0, false};
  a.gsum = gsum;
  a.divisor = divisor;
  a.flatgrad = true;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_flatgrad(void* const* params, void* const* grads, void* const* bufs,
                                               const int64_t* lens, const int32_t* dtypes, const double* lr,
                                               const double* weight_decay, const double* momentum,
                                               const double* dampening, const int32_t* flags, int32_t nseg,
                                               const float* gsum, float* master, int64_t n, double divisor,
                                               int32_t mode, void* stream) {
  SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, master, n, mode,
            false, nullptr, 0.0, true};
  a.gsum = gsum;
  a.divisor = divisor;
  a.flatgrad = true;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_clip(void* const* params, const void* const* grads, void* const* bufs,
                                    const int64_t* lens, const int32_t* dtypes, const double* lr,
                                    const double* weight_decay, const double* momentum, const double* dampening,
                                    const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                                    const float* norms, double clip_threshold, void* stream) {
  const SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, flat, n, mode,
                  true, norms, clip_threshold, false};
  return sgd_run(a, as_stream(stream));
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

CHOCO_API int choco_params_sgd_flatgrad_scaled(void* const* params, void* const* grads, void* const* bufs,
                                               const int64_t* lens, const int32_t* dtypes, const double* lr,
                                               const double* weight_decay, const double* momentum,
                                               const double* dampening, const int32_t* flags, int32_t nseg,
                                               const float* gsum, int64_t n, double divisor, int32_t mode,
                                               void* stream) {
  SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, nullptr, n, mode,
            false, nullptr, 0.0, false};
  a.gsum = gsum;
  a.divisor = divisor;
  a.flatgrad = a.found_slot = true;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_flatgrad_scaled(void* const* params, void* const* grads, void* const* bufs,
                                                      const int64_t* lens, const int32_t* dtypes, const double* lr,
                                                      const double* weight_decay, const double* momentum,
                                                      const double* dampening, const int32_t* flags, int32_t nseg,
                                                      const float* gsum, float* master, int64_t n, double divisor,
                                                      int32_t mode, void* stream) {
  SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, master, n, mode,
            false, nullptr, 0.0, true};
  a.gsum = gsum;
  a.divisor = divisor;
  a.flatgrad = a.found_slot = true;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_gclip(void* const* params, const void* const* grads, void* const* bufs,
                                     const int64_t* lens, const int32_t* dtypes, const double* lr,
                                     const double* weight_decay, const double* momentum, const double* dampening,
                                     const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                                     const float* coef, void* stream) {
  SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, flat, n, mode,
            false, nullptr, 0.0, false};
  a.gclip = true;
  a.coef = coef;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_gclip(void* const* params, const void* const* grads, void* const* bufs,
                                            const int64_t* lens, const int32_t* dtypes, const double* lr,
                                            const double* weight_decay, const double* momentum,
                                            const double* dampening, const int32_t* flags, int32_t nseg,
                                            float* master, int64_t n, int32_t mode, const float* coef,
                                            void* stream) {
  SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, master, n, mode,
            false, nullptr, 0.0, true};
  a.gclip = true;
  a.coef = coef;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API size_t choco_params_sqnorm_workspace_size(int32_t nseg, int64_t n) { return norm_ws_bytes(nseg, n); }
CHOCO_API int choco_params_sqnorm_launches(int32_t nseg) { return norm_launches(nseg); }

CHOCO_API int choco_params_sqnorm(const void* const* params, const void* const* grads, const int64_t* lens,
                                  const int32_t* dtypes, const double* weight_decay, const int32_t* flags, int32_t nseg,
                                  int64_t n, float* norms, void* ws, size_t ws_bytes, void* stream) {
  const NormArgs a{params, grads, lens, dtypes, weight_decay, flags, nseg, n, norms, ws, ws_bytes};
  return norm_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_scaled(void* const* params, const void* const* grads, void* const* bufs,
                                      const int64_t* lens, const int32_t* dtypes, const double* lr,
                                      const double* weight_decay, const double* momentum, const double* dampening,
                                      const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                                      const float* out, void* stream) {
  SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, flat, n, mode,
            false, nullptr, 0.0, false};
  a.gclip = a.scaled = true;
  a.coef = out;
  return sgd_run(a, as_stream(stream));
}

CHOCO_API int choco_params_sgd_master_scaled(void* const* params, const void* const* grads, void* const* bufs,
                                             const int64_t* lens, const int32_t* dtypes, const double* lr,
                                             const double* weight_decay, const double* momentum,
                                             const double* dampening, const int32_t* flags, int32_t nseg,
                                             float* master, int64_t n, int32_t mode, const float* out,
                                             void* stream) {
  SgdArgs a{params, grads, bufs, lens, dtypes, lr, weight_decay, momentum, dampening, flags, nseg, master, n, mode,
            false, nullptr, 0.0, true};
  a.gclip = a.scaled = true;
  a.coef = out;
  return sgd_run(a, as_stream(stream));
}
