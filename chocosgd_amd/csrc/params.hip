// The bridge between a model's parameter tensors and the flat fp32 buffer every
// codec kernel works on, one batched launch per direction:
//   * pack     flat[off[s] + j] = (float)tensor_s[j]
//              (reference flatten(), dl_code/pcode/utils/communication.py:58-76: the
//              flat buffer is the default fp32 whatever the model's dtype; widening
//              bf16 / fp16 is exact)
//   * unpack   tensor_s[j] = (dtype_s)flat[off[s] + j]
//              (TensorBuffer.unpack, dl_code/pcode/utils/tensor_buffer.py:38-40: the
//              converting copy narrows round-to-nearest-even; +-0, +-inf and NaN are
//              kept, fp16 overflow gives inf, fp16 subnormals are produced)
//   * unpack, stochastically rounded ("param_unpack_sr_kernel"): a bf16 tensor receives
//              bf16_narrow_sr(flat[i], the 16 bits of flat element i), an fp32 tensor the copy
// in the manner of torch's multi_tensor_apply: the table of a chunk of tensors (device
// pointers, int64 flat offsets, one dtype code each) travels in the kernel arguments, so
// there is no device-side table, no allocation and no synchronisation.
//
// Workgroups own tiles of the FLAT buffer at absolute flat offsets (tile t is flat
// elements [t * kTile, (t + 1) * kTile) whatever chunk is being copied), so the flat
// side of every 8-element group is 32-byte aligned when the flat pointer is.  A
// workgroup finds the first tensor of its tile by a uniform binary search over off[]
// (upper bound: zero-length tensors give equal offsets and are skipped), then walks the
// tensors that cross the tile.  A tensor whose address is congruent with the flat side
// modulo 16 bytes (uniform per tensor) moves its whole groups as 16-byte vectors, kU
// groups in flight per thread, non-temporal; its edge groups, and every tensor that is
// not congruent (odd offsets, views at element alignment, a flat pointer that is only
// 4-byte aligned), move element by element, coalesced.  A launch writes only the bytes
// of its own elements: no vector store reaches past a tensor's end or before its start.
#include "param_common.h"

namespace choco {

constexpr int kParamCap = 192;      // tensors per launch (ResNet-50: 161)
constexpr int kPbU = 4;             // 8-element groups in flight per thread
static_assert(kPbTile == (int64_t)kPbThreads * kPbU * kPbGroup, "a tile is one round of the workgroup");

struct ParamTable {
  void* ptr[kParamCap];
  int64_t off[kParamCap + 1];  // absolute flat offsets; off[nt] = end of the chunk
  uint8_t dt[kParamCap];       // CHOCO_DT_*
  int32_t nt;
};
// the table, the flat pointer and three words: a launch carries at most 4 KB of arguments
static_assert(sizeof(ParamTable) + 32 <= 4096, "ParamTable must fit in the kernel arguments");

// What the copy does to one widened value of a tensor of dtype DT on its way across: nothing
// (pack, unpack: widening and the store's round-to-nearest-even narrowing are the moves' own) ...
struct CopyOp {
  static constexpr bool kSr = false;
  template <int DT>
  CHOCO_DEV float apply(float v) const { return v; }
};
// ... nothing either, but the store into a bf16 tensor rounds stochastically with the bits of the
// element's flat index (param_common.h st1_sr / st8_sr): compiled into param_unpack_sr_kernel alone
struct SrOp {
  static constexpr bool kSr = true;
  uint64_t key;
  template <int DT>
  CHOCO_DEV float apply(float v) const { return v; }
};

// Flat elements [a, b) of a tensor, a < b inside this workgroup's tile: element i - so of src
// (dtype SDT) goes, through op for the tensor's dtype DT, to element i - d_o of dst (dtype DDT).
// vec: both sides of every whole group are 16-byte aligned.  kPbU groups in flight per thread,
// every load of them issued in a phase of its own ahead of the first store: the bridge has one
// operand, so the registers of four groups cost no occupancy (the shared span_walk keeps one
// group under one test, which is what the three-operand updates need).
template <int SDT, int DDT, int DT, typename OP>
CHOCO_DEV void param_span(const void* src, int64_t so, void* dst, int64_t d_o, const OP& op, int64_t a, int64_t b,
                          bool vec) {
  const int tid = threadIdx.x;
  constexpr bool kSr = OP::kSr && DDT == CHOCO_DT_BF16;
  const auto elem = [&](int64_t i) {
    if constexpr (kSr) st1_sr(dst, i - d_o, op.template apply<DT>(ld1<SDT>(src, i - so)), op.key, i);
    else st1<DDT>(dst, i - d_o, op.template apply<DT>(ld1<SDT>(src, i - so)));
  };
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) elem(i);
    return;
  }
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += (int64_t)kPbThreads * kPbU) {
    bool full[kPbU];
    Raw8 r[kPbU];
#pragma unroll
    for (int u = 0; u < kPbU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      full[u] = e >= a && e + kPbGroup <= b;
      if (full[u]) ld8<SDT>(r[u], src, e - so);
    }
#pragma unroll
    for (int u = 0; u < kPbU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      if (full[u]) {
        float v[8];
        widen8<SDT>(r[u], v);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = op.template apply<DT>(v[k]);
        if constexpr (kSr) st8_sr(dst, e - d_o, v, op.key, e);
        else st8<DDT>(dst, e - d_o, v);
      } else {
        // a group cut by the tensor's start or end (or past the span): its own elements only
        const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
        for (int64_t i = ea; i < eb; ++i) elem(i);
      }
    }
  }
}

// this workgroup's tile of the chunk; flat16: flat is 16-byte aligned
template <bool PACK, typename OP>
CHOCO_DEV void param_tile(const ParamTable& tb, float* flat, int64_t tile0, int flat16, const OP& op) {
  tile_walk(tb.off, tb.nt, tile0 + blockIdx.x, [&](int s, int64_t a, int64_t b) {
    void* p = tb.ptr[s];
    const int dt = tb.dt[s];
    const int64_t o0 = tb.off[s];
    const bool vec = flat16 && on_grid16(mis16(p, dtype_size(dt), o0));
    for_dtype(dt, [&](auto DT) {
      if constexpr (PACK) param_span<DT, CHOCO_DT_F32, DT>(p, o0, flat, 0, op, a, b, vec);
      else param_span<CHOCO_DT_F32, DT, DT>(flat, 0, p, o0, op, a, b, vec);
    });
  });
}

__global__ __launch_bounds__(kPbThreads) void param_pack_kernel(const ParamTable tb, float* flat, int64_t tile0,
                                                                int flat16) {
  param_tile<true>(tb, flat, tile0, flat16, CopyOp{});
}

__global__ __launch_bounds__(kPbThreads) void param_unpack_kernel(const ParamTable tb, float* flat, int64_t tile0,
                                                                  int flat16) {
  param_tile<false>(tb, flat, tile0, flat16, CopyOp{});
}

__global__ __launch_bounds__(kPbThreads) void param_unpack_sr_kernel(const ParamTable tb, float* flat, int64_t tile0,
                                                                     int flat16, uint64_t key) {
  param_tile<false>(tb, flat, tile0, flat16, SrOp{key});
}

// ------------------------------------------------------------------ the scaled pack
// choco_params_pack_scaled ("param_pack_scaled_kernel"): the pack of the all-reduce SGD step with
// the global-norm clip coefficient and 1 / loss scale on the load it does anyway,
//     RND:   flat[i] = (float)rnd_DT(c * g)   the product the gclip / scaled update kernels form
//     !RND:  flat[i] = c * (float)g           fp32, not narrowed: the master path
// c = *coef, one uniform load per workgroup.  The tiles, walk and span of param_pack_kernel, which
// carries none of this.  found != nullptr (the FIRST launch of a layout alone gets it): thread 0
// of workgroup 0 stores flat[n] = (*found != 0) ? 1 : 0, the slot that rides through the
// all-reduce behind the gradient.
template <int DT, bool RND>
CHOCO_DEV float pack_scaled1(float c, float g) {
  const float v = __fmul_rn(c, g);
  return RND ? rnd<DT>(v) : v;
}

// ... or that product
template <bool RND>
struct ScaleOp {
  static constexpr bool kSr = false;
  float c;
  template <int DT>
  CHOCO_DEV float apply(float v) const { return pack_scaled1<DT, RND>(c, v); }
};

template <bool RND>
__global__ __launch_bounds__(kPbThreads) void param_pack_scaled_kernel(const ParamTable tb, float* flat, int64_t tile0,
                                                                       int flat16, const float* coef,
                                                                       const float* found, int64_t n) {
  const float c = *coef;  // a uniform load
  if (found != nullptr && blockIdx.x == 0 && threadIdx.x == 0) flat[n] = *found != 0.0f ? 1.0f : 0.0f;
  param_tile<true>(tb, flat, tile0, flat16, ScaleOp<RND>{c});
}

// Every argument is checked before the first launch, with no HIP call.
// sr: the stochastically rounded unpack, which has no fp16 form.
static int params_check(const void* const* ptrs, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                        const float* flat, int64_t n, bool sr = false) {
  CHOCO_REQUIRE(ptrs && lens && dtypes, "null table argument");
  return layout_check(
      lens, dtypes, nseg, n,
      [&]() -> int {
        CHOCO_REQUIRE(flat || n == 0, "null flat buffer");
        CHOCO_REQUIRE(aligned4(flat), "the flat buffer must be 4-byte aligned");
        return CHOCO_OK;
      },
      [&](int32_t s, uintptr_t esz) -> int {
        CHOCO_REQUIRE(!(sr && dtypes[s] == CHOCO_DT_F16),
                      "tensor %d: fp16 has no stochastic rounding (bf16 and fp32 tensors only)", (int)s);
        CHOCO_REQUIRE(ptrs[s] || lens[s] == 0, "tensor %d: null pointer", (int)s);
        CHOCO_REQUIRE(elem_aligned(ptrs[s], esz), "tensor %d: pointer not aligned to its element size", (int)s);
        return CHOCO_OK;
      });
}

// choco_params_pack_scaled's three arguments; found: flat holds n + 1 elements
struct PackScale {
  const float* coef;
  const float* found;
  int32_t round;
};

template <bool PACK>
static int params_run(const void* const* ptrs, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                      float* flat, int64_t n, hipStream_t st, const PackScale* sc = nullptr,
                      const uint64_t* sr_key = nullptr) {
  const int rc = params_check(ptrs, lens, dtypes, nseg, flat, n, sr_key != nullptr);
  if (rc) return rc;
  if (sc) {
    CHOCO_REQUIRE(sc->coef && aligned4(sc->coef), "coef must be a 4-byte aligned device pointer");
    CHOCO_REQUIRE(aligned4(sc->found), "found must be 4-byte aligned");
    CHOCO_REQUIRE(sc->round == 0 || sc->round == 1, "round must be 0 or 1, got %d", (int)sc->round);
    CHOCO_REQUIRE(flat || !sc->found, "null flat buffer with a found slot to write");
  }
  const char* name = PACK ? "param_pack_kernel" : "param_unpack_kernel";
  const int flat16 = aligned16(flat) ? 1 : 0;
  ParamTable tb;
  return for_chunks<kParamCap>(lens, nseg, tb.off, [&](const Chunk& c) -> int {
    tb.nt = c.nt;
    for (int i = 0; i < kParamCap; ++i) {
      const bool in = i < c.nt;
      tb.ptr[i] = in ? const_cast<void*>(ptrs[c.s0 + i]) : nullptr;
      tb.dt[i] = in ? (uint8_t)dtypes[c.s0 + i] : (uint8_t)0;
    }
    if (sc) {
      // the slot behind the gradient is the first launch's: written once however many chunks follow
      const float* found = c.s0 == 0 ? sc->found : nullptr;
      return CHOCO_LAUNCH("param_pack_scaled_kernel", "param_pack_scaled_kernel",
                          sc->round ? param_pack_scaled_kernel<true> : param_pack_scaled_kernel<false>,
                          dim3((unsigned)c.tiles), dim3(kPbThreads), st, tb, flat, c.tile0, flat16, sc->coef, found, n);
    }
    if (sr_key)
      return CHOCO_LAUNCH("param_unpack_sr_kernel", "param_unpack_sr_kernel", param_unpack_sr_kernel,
                          dim3((unsigned)c.tiles), dim3(kPbThreads), st, tb, flat, c.tile0, flat16, *sr_key);
    return CHOCO_LAUNCH(name, name, PACK ? param_pack_kernel : param_unpack_kernel, dim3((unsigned)c.tiles),
                        dim3(kPbThreads), st, tb, flat, c.tile0, flat16);
  });
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_launches(int32_t nseg) { return chunk_launches(nseg, kParamCap); }

CHOCO_API int choco_params_pack(const void* const* ptrs, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                                float* flat, int64_t n, void* stream) {
  return params_run<true>(ptrs, lens, dtypes, nseg, flat, n, as_stream(stream));
}

CHOCO_API int choco_params_pack_scaled(const void* const* ptrs, const int64_t* lens, const int32_t* dtypes,
                                       int32_t nseg, float* flat, int64_t n, const float* coef,
                                       const float* found_or_null, int32_t round, void* stream) {
  const PackScale sc{coef, found_or_null, round};
  return params_run<true>(ptrs, lens, dtypes, nseg, flat, n, as_stream(stream), &sc);
}

CHOCO_API int choco_params_unpack(void* const* ptrs, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                                  const float* flat, int64_t n, void* stream) {
  return params_run<false>(const_cast<const void* const*>(ptrs), lens, dtypes, nseg, const_cast<float*>(flat), n,
                           as_stream(stream));
}

CHOCO_API int choco_params_unpack_sr(void* const* ptrs, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                                     const float* flat, int64_t n, uint64_t seed, uint64_t step, void* stream) {
  const uint64_t key = qrng_key(seed, step);
  return params_run<false>(const_cast<const void* const*>(ptrs), lens, dtypes, nseg, const_cast<float*>(flat), n,
                           as_stream(stream), nullptr, &key);
}
