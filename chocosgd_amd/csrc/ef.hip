// The dense lines around the compressors of the reference's two error-feedback optimizers, as
// ONE batched launch per chunk of tensors straight between the parameter tensors and a flat
// fp32 buffer (no pack, no unpack, no temporary):
//   * DeepSqueeze (dl_code/pcode/optim/deep_squeeze.py:101-108)   the pack of the params and
//               memory.buffer += params_tb.buffer                         -> ACCUM
//               (:125-126)  params_tb.buffer += agg, unpack(params)       -> APPLY, flat = agg
//   * EF-signSGD (dl_code/pcode/optim/ef_sign_sgd.py:218, :113-122)  synced /= world_size,
//               the pack of the params, add_(-lr * synced), unpack(params)
//                                                    -> APPLY | DIV | SCALE, flat = synced_grads
//
// Flat index i, element j of tensor s, x = params[s][j] widened, each line one reference op
// with one rounding:
//     ACCUM:  flat[i] = rn(flat[i] + x)                       the params are read only
//     APPLY:  a = flat[i]
//       DIV:    a = rn(a / (float)divisor), flat[i] = a       a correctly rounded IEEE division
//       SCALE:  a = rn((float)(-lr) * a)                      not written back
//             params[s][j] = narrow_rne(rn(x + a))            the add in fp32, ONE narrowing
// Every op is written as __fadd_rn / __fmul_rn / __fdiv_rn: nothing can be contracted.  NaN and
// inf propagate; -0 + +0 = +0.
//
// The launch has the parameter bridge's shape (params.hip, sgd.hip, mix.hip): workgroups own
// 8192-element tiles at absolute flat offsets, the chunk's table travels in the kernel
// arguments, the first tensor of a tile comes from the shared uniform search, zero-length
// tensors are skipped.  Where flat is 16-byte aligned and the tensor's side is congruent with
// the group grid, whole groups of 8 move as 16-byte vectors, non-temporal, both loads of a
// group issued before its first store; cut groups and every other tensor move element by
// element, coalesced.  Each thread reads before it writes.  Only the layout's own bytes are
// written.
#include "param_common.h"

#include <cmath>

namespace choco {

constexpr int kEfCap = 128;  // tensors per launch (ResNet-50's 161: two launches)

struct EfTable {
  void* p[kEfCap];
  int64_t off[kEfCap + 1];  // absolute flat offsets; off[nt] = end of the chunk
  uint8_t dt[kEfCap];       // CHOCO_DT_*
  int32_t nt;
};
// the table, one pointer, tile0 and four words: a launch carries at most 4 KB of arguments
static_assert(sizeof(EfTable) + 32 <= 4096 - 256, "the table must fit in the kernel arguments");

// what one element's arithmetic needs (workgroup-uniform)
struct EfOp {
  float* flat;
  float nlr, div;
  bool accum, do_div, scale;
};

// a = flat[i], x the widened param.  ACCUM: `fl` is what goes to flat.  APPLY: `fl` is what goes
// to flat under DIV, `px` to the param (narrowed by the store).
CHOCO_DEV void ef_op(const EfOp& o, float a, float x, float& fl, float& px) {
  if (o.accum) {
    fl = __fadd_rn(a, x);
    px = x;
    return;
  }
  if (o.do_div) a = __fdiv_rn(a, o.div);
  fl = a;
  if (o.scale) a = __fmul_rn(o.nlr, a);
  px = __fadd_rn(x, a);
  // the empty asm keeps the fp32 add and a 16-bit store's conversion apart (one mixed-precision
  // instruction would round the exact sum straight to fp16; mix.hip mix_tail, sgd.hip rnd)
  asm("" : "+v"(px));
}

// flat index i, element j of the tensor
template <int DT>
CHOCO_DEV void ef_elem(const EfOp& o, void* p, int64_t i, int64_t j) {
  const float a = o.flat[i];
  const float x = ld1<DT>(p, j);
  float fl, px;
  ef_op(o, a, x, fl, px);
  if (o.accum || o.do_div) o.flat[i] = fl;
  if (!o.accum) st1<DT>(p, j, px);
}

// Flat elements [a, b) of a tensor at flat offset o0, a < b inside this workgroup's tile.
// vec: flat and the tensor's side are 16-byte aligned at every whole group's start.
// The lines of param_common.h's span_walk, kept as a function of this kernel's own: with
// ef_elem and the group step as a body for span_walk (the same loads, stores and arithmetic in
// another schedule) the fp32 ResNet-50 APPLY launch took 82.4 to 83.9 us against the 75.9 to
// 78.3 of this form, alternated in one visit -- and ACCUM 68.9 to 70.5 against 76.3 to 76.6,
// APPLY | DIV | SCALE 102.7 to 109.5 against 112.0 to 118.2; bf16 the same either way.  One
// kernel holds the three modes, so the form that slows none of them stays.
template <int DT>
CHOCO_DEV void ef_span(const EfOp& o, void* p, int64_t o0, int64_t a, int64_t b, bool vec) {
  const int tid = threadIdx.x;
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) ef_elem<DT>(o, p, i, i - o0);
    return;
  }
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += kPbThreads) {
    const int64_t e = (gb + tid) * kPbGroup;
    if (e >= a && e + kPbGroup <= b) {
      // both loads of the group are issued before the first store
      Raw8 rf, rp;
      ld8<CHOCO_DT_F32>(rf, o.flat, e);
      ld8<DT>(rp, p, e - o0);
      float av[8], x[8], fl[8], px[8];
      widen8<CHOCO_DT_F32>(rf, av);
      widen8<DT>(rp, x);
#pragma unroll
      for (int k = 0; k < 8; ++k) ef_op(o, av[k], x[k], fl[k], px[k]);
      if (o.accum || o.do_div) st8<CHOCO_DT_F32>(o.flat, e, fl);
      if (!o.accum) st8<DT>(p, e - o0, px);
    } else {
      // a group cut by the tensor's start or end (or past the span): its own elements only
      const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
      for (int64_t i = ea; i < eb; ++i) ef_elem<DT>(o, p, i, i - o0);
    }
  }
}

// flat16: flat is 16-byte aligned
__global__ __launch_bounds__(kPbThreads) void param_ef_kernel(const EfTable tb, float* flat, int64_t tile0, float nlr,
                                                              float div, int32_t mode, int32_t flat16) {
  EfOp o;
  o.flat = flat; o.nlr = nlr; o.div = div;
  o.accum = (mode & CHOCO_EF_ACCUM) != 0;
  o.do_div = (mode & CHOCO_EF_DIV) != 0;
  o.scale = (mode & CHOCO_EF_SCALE) != 0;
  tile_walk(tb.off, tb.nt, tile0 + blockIdx.x, [&](int s, int64_t a, int64_t b) {
    const int dt = tb.dt[s];
    void* p = tb.p[s];
    const int64_t o0 = tb.off[s];
    const bool vec = flat16 && on_grid16(mis16(p, dtype_size(dt), o0));
    for_dtype(dt, [&](auto DT) { ef_span<DT>(o, p, o0, a, b, vec); });
  });
}

struct EfArgs {
  void* const* params;
  const int64_t* lens;
  const int32_t* dtypes;
  int32_t nseg;
  float* flat;
  int64_t n;
  int32_t mode;
  double lr, divisor;
};

// Every argument is checked before the first launch, with no HIP call.
static int ef_check(const EfArgs& a) {
  CHOCO_REQUIRE(a.params && a.lens && a.dtypes, "null table argument");
  return layout_check(
      a.lens, a.dtypes, a.nseg, a.n,
      [&]() -> int {
        constexpr int32_t kModes = CHOCO_EF_ACCUM | CHOCO_EF_APPLY | CHOCO_EF_DIV | CHOCO_EF_SCALE;
        CHOCO_REQUIRE((a.mode & ~kModes) == 0, "unknown mode bits 0x%x", (unsigned)a.mode);
        const bool accum = (a.mode & CHOCO_EF_ACCUM) != 0, apply = (a.mode & CHOCO_EF_APPLY) != 0;
        CHOCO_REQUIRE(accum != apply, "exactly one of ACCUM and APPLY, got mode 0x%x", (unsigned)a.mode);
        CHOCO_REQUIRE(apply || !(a.mode & (CHOCO_EF_DIV | CHOCO_EF_SCALE)), "DIV and SCALE belong to APPLY");
        CHOCO_REQUIRE(a.flat, "flat is null");
        CHOCO_REQUIRE(aligned4(a.flat), "flat must be 4-byte aligned");
        if (a.mode & CHOCO_EF_DIV)
          CHOCO_REQUIRE(std::isfinite(a.divisor) && (float)a.divisor != 0.0f && std::isfinite((float)a.divisor),
                        "divisor must be finite and nonzero, got %g", a.divisor);
        if (a.mode & CHOCO_EF_SCALE) CHOCO_REQUIRE(std::isfinite(a.lr), "lr must be finite, got %g", a.lr);
        return CHOCO_OK;
      },
      [&](int32_t s, uintptr_t esz) -> int {
        CHOCO_REQUIRE(elem_aligned(a.params[s], esz), "tensor %d: pointer not aligned to its element size", (int)s);
        CHOCO_REQUIRE(a.lens[s] == 0 || a.params[s], "tensor %d: null param pointer", (int)s);
        return CHOCO_OK;
      });
}

static int ef_run(const EfArgs& a, hipStream_t st) {
  const int rc = ef_check(a);
  if (rc) return rc;
  // torch's conversion of a Python scalar for an fp32 tensor
  const float nlr = (float)(-a.lr), div = (float)a.divisor;
  const int32_t flat16 = aligned16(a.flat) ? 1 : 0;
  EfTable tb;
  return for_chunks<kEfCap>(a.lens, a.nseg, tb.off, [&](const Chunk& c) -> int {
    tb.nt = c.nt;
    for (int i = 0; i < kEfCap; ++i) {
      const bool in = i < c.nt;
      tb.p[i] = in ? a.params[c.s0 + i] : nullptr;
      tb.dt[i] = in ? (uint8_t)a.dtypes[c.s0 + i] : (uint8_t)0;
    }
    return CHOCO_LAUNCH("param_ef_kernel", "param_ef_kernel", param_ef_kernel, dim3((unsigned)c.tiles),
                        dim3(kPbThreads), st, tb, a.flat, c.tile0, nlr, div, a.mode, flat16);
  });
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_ef_launches(int32_t nseg) { return chunk_launches(nseg, kEfCap); }

CHOCO_API int choco_params_ef(void* const* params, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                              float* flat, int64_t n, int32_t mode, double lr, double divisor, void* stream) {
  const EfArgs a{params, lens, dtypes, nseg, flat, n, mode, lr, divisor};
  return ef_run(a, as_stream(stream));
}
