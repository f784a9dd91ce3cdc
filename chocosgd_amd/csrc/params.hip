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

#include <algorithm>

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
// the table, the flat pointer and two words: a launch carries at most 4 KB of arguments
static_assert(sizeof(ParamTable) + 24 <= 4096, "ParamTable must fit in the kernel arguments");

// one element: flat index i, element j = i - off[s] of a tensor of dtype DT
template <bool PACK, int DT>
CHOCO_DEV void param_elem(void* p, float* flat, int64_t i, int64_t j) {
  if (DT == CHOCO_DT_F32) {
    float* t = reinterpret_cast<float*>(p);
    if (PACK) flat[i] = t[j]; else t[j] = flat[i];
  } else {
    unsigned short* t = reinterpret_cast<unsigned short*>(p);
    if (PACK) flat[i] = widen16<DT>(t[j]); else t[j] = narrow16<DT>(flat[i]);
  }
}

// Flat elements [a, b) of tensor s (flat offset o0, base p), a < b inside this
// workgroup's tile.  vec: both sides of every whole group are 16-byte aligned.
template <bool PACK, int DT>
CHOCO_DEV void param_span(void* p, float* flat, int64_t o0, int64_t a, int64_t b, bool vec) {
  const int tid = threadIdx.x;
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) param_elem<PACK, DT>(p, flat, i, i - o0);
    return;
  }
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += (int64_t)kPbThreads * kPbU) {
    bool full[kPbU];
    float4 lo[kPbU], hi[kPbU];
    choco_u16x8 hv[kPbU];
    // every load of the thread's kPbU groups is issued before the first store
#pragma unroll
    for (int u = 0; u < kPbU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      full[u] = e >= a && e + kPbGroup <= b;
      if (full[u]) {
        if (PACK) {
          if (DT == CHOCO_DT_F32) {
            const float* t = reinterpret_cast<const float*>(p) + (e - o0);
            lo[u] = ld_nt4(t);
            hi[u] = ld_nt4(t + 4);
          } else {
            hv[u] = __builtin_nontemporal_load(
                reinterpret_cast<const choco_u16x8*>(reinterpret_cast<const unsigned short*>(p) + (e - o0)));
          }
        } else {
          lo[u] = ld_nt4(flat + e);
          hi[u] = ld_nt4(flat + e + 4);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kPbU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      if (full[u]) {
        if (PACK) {
          if (DT != CHOCO_DT_F32) {
            lo[u] = make_float4(widen16<DT>(hv[u][0]), widen16<DT>(hv[u][1]), widen16<DT>(hv[u][2]),
                                widen16<DT>(hv[u][3]));
            hi[u] = make_float4(widen16<DT>(hv[u][4]), widen16<DT>(hv[u][5]), widen16<DT>(hv[u][6]),
                                widen16<DT>(hv[u][7]));
          }
          st_nt4(flat + e, lo[u]);
          st_nt4(flat + e + 4, hi[u]);
        } else if (DT == CHOCO_DT_F32) {
          float* t = reinterpret_cast<float*>(p) + (e - o0);
          st_nt4(t, lo[u]);
          st_nt4(t + 4, hi[u]);
        } else {
          choco_u16x8 o;
          o[0] = narrow16<DT>(lo[u].x); o[1] = narrow16<DT>(lo[u].y);
          o[2] = narrow16<DT>(lo[u].z); o[3] = narrow16<DT>(lo[u].w);
          o[4] = narrow16<DT>(hi[u].x); o[5] = narrow16<DT>(hi[u].y);
          o[6] = narrow16<DT>(hi[u].z); o[7] = narrow16<DT>(hi[u].w);
          __builtin_nontemporal_store(
              o, reinterpret_cast<choco_u16x8*>(reinterpret_cast<unsigned short*>(p) + (e - o0)));
        }
      } else {
        // a group cut by the tensor's start or end (or past the span): its own elements only
        const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
        for (int64_t i = ea; i < eb; ++i) param_elem<PACK, DT>(p, flat, i, i - o0);
      }
    }
  }
}

template <bool PACK>
CHOCO_DEV void param_tile(const ParamTable& tb, float* flat, int64_t tile0, int flat16) {
  const int nt = tb.nt;
  int64_t tlo, thi;
  const int s0 = tile_first_tensor(tb.off, nt, tile0 + blockIdx.x, tlo, thi);
  if (s0 < 0) return;
  for (int s = s0; s < nt; ++s) {
    const int64_t o0 = tb.off[s];
    if (o0 >= thi) break;
    const int64_t a = i64max(o0, tlo), b = i64min(tb.off[s + 1], thi);
    if (a >= b) continue;  // zero-length tensor
    void* p = tb.ptr[s];
    const int dt = tb.dt[s];
    // flat + 4 e is 16-byte aligned at every group start e (a multiple of 8); the tensor's
    // side p + esz (e - o0) is when p - esz o0 is, esz e being a multiple of 16
    const uintptr_t esz = dt == CHOCO_DT_F32 ? 4u : 2u;
    const bool vec = flat16 && ((reinterpret_cast<uintptr_t>(p) - esz * (uintptr_t)o0) & 15u) == 0;
    if (dt == CHOCO_DT_F32) param_span<PACK, CHOCO_DT_F32>(p, flat, o0, a, b, vec);
    else if (dt == CHOCO_DT_BF16) param_span<PACK, CHOCO_DT_BF16>(p, flat, o0, a, b, vec);
    else param_span<PACK, CHOCO_DT_F16>(p, flat, o0, a, b, vec);
  }
}

__global__ __launch_bounds__(kPbThreads) void param_pack_kernel(const ParamTable tb, float* flat, int64_t tile0,
                                                                int flat16) {
  param_tile<true>(tb, flat, tile0, flat16);
}

__global__ __launch_bounds__(kPbThreads) void param_unpack_kernel(const ParamTable tb, float* flat, int64_t tile0,
                                                                  int flat16) {
  param_tile<false>(tb, flat, tile0, flat16);
}

// ------------------------------------------------------------------ the scaled pack
// choco_params_pack_scaled ("param_pack_scaled_kernel"): the pack of the all-reduce SGD step with
// the global-norm clip coefficient and 1 / loss scale on the load it does anyway,
//     RND:   flat[i] = (float)rnd_DT(c * g)   the product the gclip / scaled update kernels form
//     !RND:  flat[i] = c * (float)g           fp32, not narrowed: the master path
// c = *coef, one uniform load per workgroup.  Same tiles, search and alignment rule as
// param_pack_kernel, which carries none of this.  found != nullptr (the FIRST launch of a layout
// alone gets it): thread 0 of workgroup 0 stores flat[n] = (*found != 0) ? 1 : 0, the slot that
// rides through the all-reduce behind the gradient.
template <int DT, bool RND>
CHOCO_DEV float pack_scaled1(float c, float g) {
  const float v = __fmul_rn(c, g);
  return RND ? rnd<DT>(v) : v;
}

// Flat elements [a, b) of tensor s (flat offset o0, base p), a < b inside this workgroup's tile.
template <int DT, bool RND>
CHOCO_DEV void pack_scaled_span(const void* p, float* flat, float c, int64_t o0, int64_t a, int64_t b, bool vec) {
  const int tid = threadIdx.x;
  if (!vec) {
    for (int64_t i = a + tid; i < b; i += kPbThreads) flat[i] = pack_scaled1<DT, RND>(c, ld1<DT>(p, i - o0));
    return;
  }
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += (int64_t)kPbThreads * kPbU) {
    bool full[kPbU];
    Raw8 r[kPbU];
    // every load of the thread's kPbU groups is issued before the first store
#pragma unroll
    for (int u = 0; u < kPbU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      full[u] = e >= a && e + kPbGroup <= b;
      if (full[u]) ld8<DT>(r[u], p, e - o0);
    }
#pragma unroll
    for (int u = 0; u < kPbU; ++u) {
      const int64_t e = (gb + u * kPbThreads + tid) * kPbGroup;
      if (full[u]) {
        float v[8];
        widen8<DT>(r[u], v);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = pack_scaled1<DT, RND>(c, v[k]);
        st8<CHOCO_DT_F32>(flat, e, v);
      } else {
        // a group cut by the tensor's start or end (or past the span): its own elements only
        const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
        for (int64_t i = ea; i < eb; ++i) flat[i] = pack_scaled1<DT, RND>(c, ld1<DT>(p, i - o0));
      }
    }
  }
}

template <bool RND>
__global__ __launch_bounds__(kPbThreads) void param_pack_scaled_kernel(const ParamTable tb, float* flat, int64_t tile0,
                                                                       int flat16, const float* coef,
                                                                       const float* found, int64_t n) {
  const float c = *coef;  // a uniform load
  if (found != nullptr && blockIdx.x == 0 && threadIdx.x == 0) flat[n] = *found != 0.0f ? 1.0f : 0.0f;
  const int nt = tb.nt;
  int64_t tlo, thi;
  const int s0 = tile_first_tensor(tb.off, nt, tile0 + blockIdx.x, tlo, thi);
  if (s0 < 0) return;
  for (int s = s0; s < nt; ++s) {
    const int64_t o0 = tb.off[s];
    if (o0 >= thi) break;
    const int64_t a = i64max(o0, tlo), b = i64min(tb.off[s + 1], thi);
    if (a >= b) continue;  // zero-length tensor
    const void* p = tb.ptr[s];
    const int dt = tb.dt[s];
    // the alignment rule of param_tile
    const uintptr_t esz = dt == CHOCO_DT_F32 ? 4u : 2u;
    const bool vec = flat16 && ((reinterpret_cast<uintptr_t>(p) - esz * (uintptr_t)o0) & 15u) == 0;
    if (dt == CHOCO_DT_F32) pack_scaled_span<CHOCO_DT_F32, RND>(p, flat, c, o0, a, b, vec);
    else if (dt == CHOCO_DT_BF16) pack_scaled_span<CHOCO_DT_BF16, RND>(p, flat, c, o0, a, b, vec);
    else pack_scaled_span<CHOCO_DT_F16, RND>(p, flat, c, o0, a, b, vec);
  }
}

static int params_launches(int32_t nseg) { return nseg <= 0 ? 0 : (nseg + kParamCap - 1) / kParamCap; }

// Every argument is checked before the first launch, with no HIP call.
static int params_check(const void* const* ptrs, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                        const float* flat, int64_t n) {
  CHOCO_REQUIRE(ptrs && lens && dtypes, "null table argument");
  CHOCO_REQUIRE(nseg > 0, "nseg must be positive, got %d", (int)nseg);
  CHOCO_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "n must be in [0, 2^31), got %lld", (long long)n);
  CHOCO_REQUIRE(flat || n == 0, "null flat buffer");
  CHOCO_REQUIRE(aligned4(flat), "the flat buffer must be 4-byte aligned");
  int64_t sum = 0;
  for (int32_t s = 0; s < nseg; ++s) {
    CHOCO_REQUIRE(lens[s] >= 0, "tensor %d: negative length", (int)s);
    CHOCO_REQUIRE(dtypes[s] >= CHOCO_DT_F32 && dtypes[s] <= CHOCO_DT_F16, "tensor %d: unknown dtype code %d", (int)s,
                  (int)dtypes[s]);
    CHOCO_REQUIRE(lens[s] <= n - sum, "the lengths add up to more than n = %lld", (long long)n);
    sum += lens[s];
    CHOCO_REQUIRE(ptrs[s] || lens[s] == 0, "tensor %d: null pointer", (int)s);
    const uintptr_t esz = dtypes[s] == CHOCO_DT_F32 ? 4u : 2u;
    CHOCO_REQUIRE((reinterpret_cast<uintptr_t>(ptrs[s]) & (esz - 1)) == 0,
                  "tensor %d: pointer not aligned to its element size", (int)s);
  }
  CHOCO_REQUIRE(sum == n, "the lengths add up to %lld, n is %lld", (long long)sum, (long long)n);
  return CHOCO_OK;
}

// choco_params_pack_scaled's three arguments; found: flat holds n + 1 elements
struct PackScale {
  const float* coef;
  const float* found;
  int32_t round;
};

template <bool PACK>
static int params_run(const void* const* ptrs, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                      float* flat, int64_t n, hipStream_t st, const PackScale* sc = nullptr) {
  const int rc = params_check(ptrs, lens, dtypes, nseg, flat, n);
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
  int64_t base = 0;
  for (int32_t s0 = 0; s0 < nseg; s0 += kParamCap) {
    const int nt = std::min<int32_t>(kParamCap, nseg - s0);
    tb.nt = nt;
    tb.off[0] = base;
    for (int i = 0; i < kParamCap; ++i) {
      const bool in = i < nt;
      tb.ptr[i] = in ? const_cast<void*>(ptrs[s0 + i]) : nullptr;
      tb.dt[i] = in ? (uint8_t)dtypes[s0 + i] : (uint8_t)0;
      base += in ? lens[s0 + i] : 0;
      tb.off[i + 1] = base;
    }
    // the tiles the chunk [off[0], off[nt]) touches; an empty chunk still takes its launch
    const int64_t tile0 = tb.off[0] / kPbTile;
    const int64_t tiles = tb.off[nt] > tb.off[0] ? (tb.off[nt] - 1) / kPbTile - tile0 + 1 : 1;
    if (sc) {
      // the slot behind the gradient is the first launch's: written once however many chunks follow
      const float* found = s0 == 0 ? sc->found : nullptr;
      CHOCO_TRY(CHOCO_LAUNCH("param_pack_scaled_kernel", "param_pack_scaled_kernel",
                             sc->round ? param_pack_scaled_kernel<true> : param_pack_scaled_kernel<false>,
                             dim3((unsigned)tiles), dim3(kPbThreads), st, tb, flat, tile0, flat16, sc->coef, found, n));
      continue;
    }
    CHOCO_TRY(CHOCO_LAUNCH(name, name, PACK ? param_pack_kernel : param_unpack_kernel, dim3((unsigned)tiles),
                           dim3(kPbThreads), st, tb, flat, tile0, flat16));
  }
  return CHOCO_OK;
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_launches(int32_t nseg) { return params_launches(nseg); }

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
