// The neighbour-weighted model mix sum([hat_r.buffer * neighbors_info[r] for r ...]) that the
// dense half of three decentralized optimizers of the reference is built around, with what
// follows it in each of them, as ONE batched launch per chunk of tensors:
//   * DCD-PSGD  (dl_code/pcode/optim/dcd_psgd.py:114-125)   mix - lr * grads, two roundings,
//               with the params packed beside it for the compressor (:104-107)
//   * ECD-PSGD  (dl_code/pcode/optim/ecd_psgd.py:118-140)   mix.add_(grads, alpha=-lr) (fused),
//               unpack(params), then the extrapolation (1 - 0.5 t) x + 0.5 t y against the
//               packed OLD params
//   * D-PSGD    (dl_code/pcode/optim/sgd.py:94-121 with _agg(op="weighted"),
//               dl_code/pcode/utils/communication.py:271-277)   the mix, then unpack(params)
//
// Sources: nsrc flat fp32 buffers of n elements, weights (float)w[r].  Flat index i, element j
// of tensor s, each line one reference op with one rounding:
//     m = 0.0f + rn(src[0] * w[0])               Python's sum() starts at int 0: -0 becomes +0
//     m = rn(m + rn(src[r] * w[r]))              r = 1 .. nsrc - 1, in the given order
//     GRAD_SUB:     m = rn(m - rn((float)lr * g))           g = grads[s][j] widened
//     GRAD_FMA:     m = fmaf((float)(-lr), g, m)
//     x = params[s][j] widened                   (EXTRAPOLATE or x_out), read before the store
//     WRITE_PARAMS: params[s][j] = narrow_rne(m)             TensorBuffer.unpack
//     EXTRAPOLATE:  z = rn(rn(a * x) + rn(b * m))            the un-narrowed m
//     flat_out[i] = EXTRAPOLATE ? z : m          (if not NULL)
//     x_out[i]    = x                            (if not NULL)
// A zero weight is multiplied, not skipped (inf * 0 = NaN, as torch); NaN and inf propagate.
// Every op is written as __fmul_rn / __fadd_rn / __fsub_rn / fmaf: nothing can be contracted.
//
// More than kMixSrc sources: successive launches of kMixSrc.  The earlier ones run over the
// flat buffer alone (a one-tensor table), leave the running sum in flat_out and apply no
// tail; the next launch takes flat_out[i] as its first term, unweighted and without the
// 0.0f +, so the chain is the one-launch definition bit for bit.
//
// The launch has the parameter bridge's shape (params.hip, sgd.hip): workgroups own
// 8192-element tiles at absolute flat offsets, the chunk's table travels in the kernel
// arguments, the first tensor of a tile comes from the shared uniform search, zero-length
// tensors are skipped.  Where every source, flat_out and x_out are 16-byte aligned and the
// tensor's touched sides (params, grads) are congruent with the group grid, whole groups of 8
// move as 16-byte vectors, non-temporal, one group in flight per thread with all of its loads
// (up to 2 * kMixSrc + 6 of them) issued before the first store; cut groups and every other
// tensor move element by element, coalesced.  Only the layout's own bytes are written.
#include "param_common.h"

#include <algorithm>
#include <cmath>

namespace choco {

constexpr int kMixCap = 128;  // tensors per launch (ResNet-50's 161: two launches)
constexpr int kMixSrc = 8;    // sources per launch
constexpr int kMixMaxSrc = 64;

struct MixTable {
  void* p[kMixCap];
  const void* g[kMixCap];
  int64_t off[kMixCap + 1];  // absolute flat offsets; off[nt] = end of the chunk
  uint8_t dt[kMixCap];       // CHOCO_DT_*
  int32_t nt;
};
struct MixSrcs {
  const float* src[kMixSrc];
  float w[kMixSrc];
  int32_t nsrc;
  int32_t chained;  // the first term is flat_out's running sum
};
// the two tables, two pointers, tile0 and six words: a launch carries at most 4 KB of arguments
static_assert(sizeof(MixTable) + sizeof(MixSrcs) + 48 <= 4096 - 256, "the mix tables must fit in the kernel arguments");

// what one tensor's tail needs (workgroup-uniform)
struct MixTensor {
  void* p;
  const void* g;
  float* flat_out;
  float* x_out;
  float lr, nlr, a, b;
  bool sub, fma, rd_p, wr_p, extrap;
};

// the weighted sum of one element: v[r] = src[r][i], run = flat_out[i] of a chained launch
CHOCO_DEV float mix_sum(const MixSrcs& sr, const float (&v)[kMixSrc], float run) {
  float m = run;
#pragma unroll
  for (int r = 0; r < kMixSrc; ++r) {
    if (r < sr.nsrc) {
      const float t = __fmul_rn(v[r], sr.w[r]);
      m = (r == 0 && !sr.chained) ? __fadd_rn(0.0f, t) : __fadd_rn(m, t);
    }
  }
  return m;
}

// the tail of one element: m the sum, g and x widened.  `m` is what goes to params (narrowed by
// the store), `out` to flat_out.
CHOCO_DEV void mix_tail(const MixTensor& t, float& m, float g, float x, float& out) {
  if (t.sub) m = __fsub_rn(m, __fmul_rn(t.lr, g));
  if (t.fma) m = fmaf(t.nlr, g, m);
  // the empty asm keeps the fma and a 16-bit store's conversion apart (one v_fma_mixlo_f16
  // would round the exact sum straight to fp16; sgd.hip rnd)
  asm("" : "+v"(m));
  out = t.extrap ? __fadd_rn(__fmul_rn(t.a, x), __fmul_rn(t.b, m)) : m;
}

// One element at flat index i and one whole group at flat index e of a tensor of dtype DT at
// flat offset o0 (span_walk's body); every load of a group is issued before its first store.
template <int DT>
struct MixBody {
  const MixSrcs& sr;
  const MixTensor& t;
  int64_t o0;

  CHOCO_DEV void elem(int64_t i) const {
    const int64_t j = i - o0;
    float v[kMixSrc];
#pragma unroll
    for (int r = 0; r < kMixSrc; ++r) v[r] = r < sr.nsrc ? sr.src[r][i] : 0.0f;
    const float run = sr.chained ? t.flat_out[i] : 0.0f;
    const float g = (t.sub || t.fma) ? ld1<DT>(t.g, j) : 0.0f;
    const float x = t.rd_p ? ld1<DT>(t.p, j) : 0.0f;
    float m = mix_sum(sr, v, run), out;
    mix_tail(t, m, g, x, out);
    if (t.wr_p) st1<DT>(t.p, j, m);
    if (t.flat_out) t.flat_out[i] = out;
    if (t.x_out) t.x_out[i] = x;
  }

  CHOCO_DEV void group(int64_t e) const {
    const bool rd_g = t.sub || t.fma;
    Raw8 rs[kMixSrc], rr, rg, rp;
#pragma unroll
    for (int r = 0; r < kMixSrc; ++r)
      if (r < sr.nsrc) ld8<CHOCO_DT_F32>(rs[r], sr.src[r], e);
    if (sr.chained) ld8<CHOCO_DT_F32>(rr, t.flat_out, e);
    if (rd_g) ld8<DT>(rg, t.g, e - o0);
    if (t.rd_p) ld8<DT>(rp, t.p, e - o0);
    float m[8] = {0, 0, 0, 0, 0, 0, 0, 0}, g[8] = {0, 0, 0, 0, 0, 0, 0, 0}, x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float out[8], w8[8];
    if (sr.chained) widen8<CHOCO_DT_F32>(rr, m);
#pragma unroll
    for (int r = 0; r < kMixSrc; ++r) {
      if (r < sr.nsrc) {
        widen8<CHOCO_DT_F32>(rs[r], w8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float tt = __fmul_rn(w8[k], sr.w[r]);
          m[k] = (r == 0 && !sr.chained) ? __fadd_rn(0.0f, tt) : __fadd_rn(m[k], tt);
        }
      }
    }
    if (rd_g) widen8<DT>(rg, g);
    if (t.rd_p) widen8<DT>(rp, x);
#pragma unroll
    for (int k = 0; k < 8; ++k) mix_tail(t, m[k], g[k], x[k], out[k]);
    if (t.wr_p) st8<DT>(t.p, e - o0, m);
    if (t.flat_out) st8<CHOCO_DT_F32>(t.flat_out, e, out);
    if (t.x_out) st8<CHOCO_DT_F32>(t.x_out, e, x);
  }
};

// all16: every source, flat_out and x_out (those not NULL) are 16-byte aligned
__global__ __launch_bounds__(kPbThreads) void param_mix_kernel(const MixTable tb, const MixSrcs sr, float* flat_out,
                                                               float* x_out, int64_t tile0, float lr, float nlr,
                                                               float ext_a, float ext_b, int32_t mode, int32_t all16) {
  MixTensor t;
  t.flat_out = flat_out; t.x_out = x_out;
  t.lr = lr; t.nlr = nlr; t.a = ext_a; t.b = ext_b;
  t.sub = (mode & CHOCO_MIX_GRAD_SUB) != 0;
  t.fma = (mode & CHOCO_MIX_GRAD_FMA) != 0;
  t.wr_p = (mode & CHOCO_MIX_WRITE_PARAMS) != 0;
  t.extrap = (mode & CHOCO_MIX_EXTRAPOLATE) != 0;
  t.rd_p = t.extrap || x_out != nullptr;
  tile_walk(tb.off, tb.nt, tile0 + blockIdx.x, [&](int s, int64_t a, int64_t b) {
    const int dt = tb.dt[s];
    const int64_t o0 = tb.off[s];
    t.p = tb.p[s]; t.g = tb.g[s];
    const uintptr_t esz = dtype_size(dt);
    uintptr_t mis = 0;
    if (t.rd_p || t.wr_p) mis |= mis16(t.p, esz, o0);
    if (t.sub || t.fma) mis |= mis16(t.g, esz, o0);
    const bool vec = all16 && on_grid16(mis);
    for_dtype(dt, [&](auto DT) { span_walk(MixBody<DT>{sr, t, o0}, a, b, vec); });
  });
}

static int mix_launches(int32_t nseg, int32_t nsrc) {
  if (nseg <= 0 || nsrc < 1 || nsrc > kMixMaxSrc) return 0;
  return (nsrc - 1) / kMixSrc + chunk_launches(nseg, kMixCap);
}

struct MixArgs {
  const float* const* srcs;
  const double* weights;
  int32_t nsrc;
  void* const* params;
  const void* const* grads;
  const int64_t* lens;
  const int32_t* dtypes;
  int32_t nseg;
  double lr, ext_a, ext_b;
  int32_t mode;
  float* flat_out;
  float* x_out;
  int64_t n;
};

// Every argument is checked before the first launch, with no HIP call.
static int mix_check(const MixArgs& a) {
  CHOCO_REQUIRE(a.srcs && a.weights && a.lens && a.dtypes, "null table argument");
  CHOCO_REQUIRE(a.nsrc >= 1 && a.nsrc <= kMixMaxSrc, "nsrc must be in [1, %d], got %d", kMixMaxSrc, (int)a.nsrc);
  constexpr int32_t kGrad = CHOCO_MIX_GRAD_SUB | CHOCO_MIX_GRAD_FMA;
  const bool grad = (a.mode & kGrad) != 0;
  const bool use_p = (a.mode & (CHOCO_MIX_WRITE_PARAMS | CHOCO_MIX_EXTRAPOLATE)) != 0 || a.x_out != nullptr;
  return layout_check(
      a.lens, a.dtypes, a.nseg, a.n,
      [&]() -> int {
        constexpr int32_t kModes = kGrad | CHOCO_MIX_WRITE_PARAMS | CHOCO_MIX_EXTRAPOLATE;
        CHOCO_REQUIRE((a.mode & ~kModes) == 0, "unknown mode bits 0x%x", (unsigned)a.mode);
        CHOCO_REQUIRE((a.mode & kGrad) != kGrad, "GRAD_SUB and GRAD_FMA are two gradient terms: one of them at most");
        CHOCO_REQUIRE(!grad || a.grads, "a GRAD mode needs the grads table");
        CHOCO_REQUIRE(!use_p || a.params, "WRITE_PARAMS, EXTRAPOLATE and x_out need the params table");
        CHOCO_REQUIRE(a.flat_out || a.x_out || (a.mode & CHOCO_MIX_WRITE_PARAMS),
                      "nothing to write: flat_out and x_out are null and the mode does not write the params");
        CHOCO_REQUIRE(a.flat_out || !(a.mode & CHOCO_MIX_EXTRAPOLATE), "EXTRAPOLATE writes flat_out, which is null");
        CHOCO_REQUIRE(a.nsrc <= kMixSrc || a.flat_out, "more than %d sources need flat_out for the running sum",
                      kMixSrc);
        CHOCO_REQUIRE(aligned4(a.flat_out) && aligned4(a.x_out), "flat_out and x_out must be 4-byte aligned");
        CHOCO_REQUIRE(!grad || std::isfinite(a.lr), "lr must be finite, got %g", a.lr);
        for (int32_t r = 0; r < a.nsrc; ++r) {
          CHOCO_REQUIRE(a.srcs[r] || a.n == 0, "source %d: null pointer", (int)r);
          CHOCO_REQUIRE(aligned4(a.srcs[r]), "source %d: pointer must be 4-byte aligned", (int)r);
        }
        return CHOCO_OK;
      },
      [&](int32_t s, uintptr_t esz) -> int {
        const int i = (int)s;
        CHOCO_REQUIRE((!use_p || elem_aligned(a.params[s], esz)) && (!grad || elem_aligned(a.grads[s], esz)),
                      "tensor %d: pointer not aligned to its element size", i);
        if (a.lens[s] == 0) return CHOCO_OK;
        CHOCO_REQUIRE(!use_p || a.params[s], "tensor %d: null param pointer", i);
        CHOCO_REQUIRE(!grad || a.grads[s], "tensor %d: null grad pointer in a GRAD mode", i);
        return CHOCO_OK;
      });
}

static int mix_run(const MixArgs& a, hipStream_t st) {
  const int rc = mix_check(a);
  if (rc) return rc;
  const bool grad = (a.mode & (CHOCO_MIX_GRAD_SUB | CHOCO_MIX_GRAD_FMA)) != 0;
  const bool use_p = (a.mode & (CHOCO_MIX_WRITE_PARAMS | CHOCO_MIX_EXTRAPOLATE)) != 0 || a.x_out != nullptr;
  bool all16 = aligned16(a.flat_out) && aligned16(a.x_out);
  for (int32_t r = 0; r < a.nsrc; ++r) all16 = all16 && aligned16(a.srcs[r]);
  // torch's conversion of a Python scalar for an fp32 tensor
  const float lr = (float)a.lr, nlr = (float)(-a.lr), ea = (float)a.ext_a, eb = (float)a.ext_b;
  MixTable tb;
  MixSrcs sr;
  for (int32_t r0 = 0; r0 < a.nsrc; r0 += kMixSrc) {
    sr.nsrc = std::min<int32_t>(kMixSrc, a.nsrc - r0);
    sr.chained = r0 > 0 ? 1 : 0;
    for (int r = 0; r < kMixSrc; ++r) {
      sr.src[r] = r < sr.nsrc ? a.srcs[r0 + r] : nullptr;
      sr.w[r] = r < sr.nsrc ? (float)a.weights[r0 + r] : 0.0f;
    }
    if (r0 + kMixSrc < a.nsrc) {
      // not the last group of sources: the running sum over the flat buffer as one fp32 tensor
      tb.nt = 1;
      for (int i = 0; i < kMixCap; ++i) {
        tb.p[i] = nullptr; tb.g[i] = nullptr; tb.dt[i] = (uint8_t)CHOCO_DT_F32;
        tb.off[i + 1] = a.n;
      }
      tb.off[0] = 0;
      const int64_t tiles = a.n > 0 ? (a.n - 1) / kPbTile + 1 : 1;
      CHOCO_TRY(CHOCO_LAUNCH("param_mix_kernel", "param_mix_kernel<sum>", param_mix_kernel, dim3((unsigned)tiles),
                             dim3(kPbThreads), st, tb, sr, a.flat_out, (float*)nullptr, (int64_t)0, 0.0f, 0.0f, 0.0f,
                             0.0f, (int32_t)0, (int32_t)(all16 ? 1 : 0)));
      continue;
    }
    CHOCO_TRY(for_chunks<kMixCap>(a.lens, a.nseg, tb.off, [&](const Chunk& c) -> int {
      tb.nt = c.nt;
      for (int i = 0; i < kMixCap; ++i) {
        const bool in = i < c.nt;
        tb.p[i] = in && use_p ? a.params[c.s0 + i] : nullptr;
        tb.g[i] = in && grad ? a.grads[c.s0 + i] : nullptr;
        tb.dt[i] = in ? (uint8_t)a.dtypes[c.s0 + i] : (uint8_t)0;
      }
      return CHOCO_LAUNCH("param_mix_kernel", "param_mix_kernel", param_mix_kernel, dim3((unsigned)c.tiles),
                          dim3(kPbThreads), st, tb, sr, a.flat_out, a.x_out, c.tile0, lr, nlr, ea, eb, a.mode,
                          (int32_t)(all16 ? 1 : 0));
    }));
  }
  return CHOCO_OK;
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_mix_launches(int32_t nseg, int32_t nsrc) { return mix_launches(nseg, nsrc); }

CHOCO_API int choco_params_mix(const float* const* srcs, const double* weights, int32_t nsrc, void* const* params,
                               const void* const* grads, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                               double lr, double ext_a, double ext_b, int32_t mode, float* flat_out, float* x_out,
                               int64_t n, void* stream) {
  const MixArgs a{srcs, weights, nsrc, params, grads, lens, dtypes, nseg, lr, ext_a, ext_b, mode, flat_out, x_out, n};
  return mix_run(a, as_stream(stream));
}
