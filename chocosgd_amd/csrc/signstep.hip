// signSGD's update from a packed verdict (Bernstein et al. 2019: p -= lr * sign, the sign voted
// by csrc/vote.hip) straight into the parameter tensors: one bit per element in, no dense decode.
// Flat element i < n, N' = ceil(n / 32), element j of tensor s:
//     bit = (verdict[i mod N'] >> (i div N')) & 1        the (32, N') layout of sign_pack, DESIGN 3
//     params[s][j] = narrow_rne(rn(widen(params[s][j]) + (bit ? +lr_s : -lr_s)))
// with lr_s = (float)lr[s], for a 16-bit tensor rounded on to the tensor's dtype: torch converts
// alpha to the dtype of the tensors it adds.  That is torch's p.add_(sign, alpha=-lr) on a CPU
// tensor of p's dtype with sign = 1 - 2 bit, bit for bit: one __fadd_rn, one narrowing, the
// empty asm between them (ef.hip ef_op).  NaN and inf
// propagate.  Elements >= n (the padding bits), zero-length tensors and bytes outside the layout
// are neither read nor written.
//
// The launch has the shape of the sign receivers (sign.hip sign_accumulate_kernel), not of the
// flat-tile kernels: a flat 8192-element tile would load 8192 verdict words to use one bit of
// each.  A 256-thread workgroup owns 1024 consecutive words and 8 of the 32 rows; the row blocks
// of one column block run on one XCD (linear ids congruent mod 8), so their word loads meet in
// that XCD's L2.  A wave owns 256 words; for row r its elements are the contiguous flat run
// [r N' + j0, + 256).  A thread holds its words twice, in the two arrangements of the two access
// paths (8 words against 32 x 4 elements):
//     vector   words j0 + 4 lane + c: elements run + 4 lane + c, one 16-byte (fp32) or 8-byte
//              (bf16 / fp16) non-temporal access per lane at the run's own alignment (gfx950
//              serves element-aligned wide accesses directly), taken where the whole run lies in
//              one tensor
//     element  words j0 + 64 c + lane: elements run + 64 c + lane, four fully coalesced element
//              accesses, each guarded: cut runs
// The tensors come per row, not per element: the first tensor of each row's run from a uniform
// upper-bound search over the table's offsets in the kernel arguments (tile_first_tensor's), the
// rows of a load group searched in lock step so that a step's scalar loads are independent.  A
// group whose runs each lie in one tensor, all of one dtype, loads all its rows before its first
// store; any other group goes row by row, a cut run piece by piece.  Every thread reads before it
// writes, and no two threads share an element.
//
// The table (pointer, absolute flat offset, dtype code, fp32 lr per tensor) travels in the kernel
// arguments, 176 tensors a launch (ResNet-50's 161: one launch); for_chunks covers more, and a
// chunk's launch covers only the column blocks and rows its flat range [off[0], off[nt]) touches.
#include "param_common.h"

#include <cmath>
#include <cstring>

namespace choco {

constexpr int kStepThreads = 256;
constexpr int kStepCols = 1024;  // words per workgroup (sign.hip kSignCols)
constexpr int kStepRows = 8;     // rows per workgroup (sign.hip kSAccRows)
constexpr int kStepRU = 4;       // rows whose loads are in flight together
constexpr int kStepCap = 176;    // tensors per launch
static_assert(32 % kStepRows == 0 && kStepRows % kStepRU == 0, "row blocking");

struct StepTable {
  void* p[kStepCap];
  int64_t off[kStepCap + 1];  // absolute flat offsets; off[nt] = end of the chunk
  float lr[kStepCap];
  uint8_t dt[kStepCap];       // CHOCO_DT_*
  int32_t nt;
};
// what a launch covers: column blocks [cb0, cb0 + ncb), rows [r0, r1) in nrb row blocks
struct StepGeom {
  int64_t n, Np;
  int32_t cb0, ncb, r0, r1, nrb;
};
static_assert(sizeof(StepTable) + sizeof(StepGeom) + 8 <= 4096 - 256, "the table must fit in the kernel arguments");

// CHOCO_SIGNSTEP_ALIGNED (a measuring variant, tools/build_variants.py signstep_aligned): only a
// whole run that starts on a 16-byte (8-byte) boundary on the tensor's side takes the vector
// path, every other one the element path.  It measured 4 % slower on ResNet-50's layout, where
// N' = 2 mod 4 leaves every other row off the boundary; DESIGN.md section 4 has both numbers.
#ifndef CHOCO_SIGNSTEP_ALIGNED
typedef uint32_t step_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t step_u32x2 __attribute__((ext_vector_type(2), aligned(2)));
#else
typedef uint32_t step_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t step_u32x2 __attribute__((ext_vector_type(2)));
#endif

// A wave's run of row r starts at flat s; [a, b) is the part of it inside one tensor (pointer p,
// flat offset o0).  The vector path: the whole 256-element run.
template <int DT>
CHOCO_DEV bool piece_vec(const void* p, int64_t o0, int64_t s, int64_t a, int64_t b) {
  constexpr uintptr_t esz = DT == CHOCO_DT_F32 ? 4u : 2u;
  const bool whole = a == s && b == s + 256;
#ifndef CHOCO_SIGNSTEP_ALIGNED
  return whole;
#else
  return whole && ((reinterpret_cast<uintptr_t>(p) + esz * (uintptr_t)(s - o0)) & (4u * esz - 1u)) == 0;
#endif
}

// the thread's four elements as stored: vector path -- 4 dwords (fp32) or 2 dwords of two halves
// each; element path -- one element per word (zero where the thread has none)
template <int DT>
CHOCO_DEV void piece_load(const void* p, int64_t o0, int64_t s, int64_t a, int64_t b, bool vec, int lane,
                          uint32_t (&raw)[4]) {
  if (vec) {
    const int64_t j = s - o0 + 4 * lane;
    if (DT == CHOCO_DT_F32) {
      const step_u32x4 v = __builtin_nontemporal_load(
          reinterpret_cast<const step_u32x4*>(reinterpret_cast<const uint32_t*>(p) + j));
      raw[0] = v.x; raw[1] = v.y; raw[2] = v.z; raw[3] = v.w;
    } else {
      const step_u32x2 v = __builtin_nontemporal_load(
          reinterpret_cast<const step_u32x2*>(reinterpret_cast<const unsigned short*>(p) + j));
      raw[0] = v.x; raw[1] = v.y; raw[2] = 0u; raw[3] = 0u;
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t e = s + 64 * c + lane;
    raw[c] = 0u;
    if (e >= a && e < b)
      raw[c] = DT == CHOCO_DT_F32 ? reinterpret_cast<const uint32_t*>(p)[e - o0]
                                  : (uint32_t) reinterpret_cast<const unsigned short*>(p)[e - o0];
  }
}

// one element as stored -> the updated element as stored
template <int DT>
CHOCO_DEV uint32_t step_elem(uint32_t stored, uint32_t bit, float lr) {
  const float x = DT == CHOCO_DT_F32 ? __uint_as_float(stored) : widen16<DT>((unsigned short)stored);
  float px = __fadd_rn(x, bit ? lr : -lr);
  // the empty asm keeps the fp32 add and a 16-bit store's conversion apart (ef.hip ef_op)
  asm("" : "+v"(px));
  return DT == CHOCO_DT_F32 ? __float_as_uint(px) : (uint32_t)narrow16<DT>(px);
}

// wv / we: the thread's words in the vector and the element arrangement; r the row
template <int DT>
CHOCO_DEV void piece_store(void* p, int64_t o0, float lr, int64_t s, int64_t a, int64_t b, bool vec, int lane, int r,
                           const uint32_t (&wv)[4], const uint32_t (&we)[4], const uint32_t (&raw)[4]) {
  if (vec) {
    const int64_t j = s - o0 + 4 * lane;
    uint32_t o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t stored = DT == CHOCO_DT_F32 ? raw[c] : (raw[c >> 1] >> (16 * (c & 1))) & 0xffffu;
      o[c] = step_elem<DT>(stored, (wv[c] >> r) & 1u, lr);
    }
    if (DT == CHOCO_DT_F32) {
      step_u32x4 v;
      v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
      __builtin_nontemporal_store(v, reinterpret_cast<step_u32x4*>(reinterpret_cast<uint32_t*>(p) + j));
    } else {
      step_u32x2 v;
      v.x = o[0] | (o[1] << 16); v.y = o[2] | (o[3] << 16);
      __builtin_nontemporal_store(v, reinterpret_cast<step_u32x2*>(reinterpret_cast<unsigned short*>(p) + j));
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t e = s + 64 * c + lane;
    if (e >= a && e < b) {
      const uint32_t v = step_elem<DT>(raw[c], (we[c] >> r) & 1u, lr);
      if (DT == CHOCO_DT_F32) reinterpret_cast<uint32_t*>(p)[e - o0] = v;
      else reinterpret_cast<unsigned short*>(p)[e - o0] = (unsigned short)v;
    }
  }
}

__global__ __launch_bounds__(kStepThreads) void param_sign_step_kernel(const StepTable tb,
                                                                      const uint32_t* __restrict__ verdict,
                                                                      const StepGeom G) {
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // block -> (column block, row block): the row blocks of a column block on one XCD
  const uint32_t rest = blockIdx.x / 8;
  const int cbi = (int)(blockIdx.x % 8 + 8 * (rest / (uint32_t)G.nrb));
  if (cbi >= G.ncb) return;  // (the grid is padded to a multiple of 8 column blocks)
  const int rbase = G.r0 + (int)(rest % (uint32_t)G.nrb) * kStepRows;
  const int64_t j0 = (int64_t)(G.cb0 + cbi) * kStepCols + 256 * w;
  if (j0 >= G.Np) return;
  const int ncol = (int)i64min(256, G.Np - j0);
  uint32_t wv[4], we[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t jv = j0 + 4 * lane + c, je = j0 + 64 * c + lane;
    wv[c] = jv < G.Np ? verdict[jv] : 0u;
    we[c] = je < G.Np ? verdict[je] : 0u;
  }
  const int nt = tb.nt;
  const int64_t clo = tb.off[0], chi = tb.off[nt];
  for (int g = 0; g < kStepRows; g += kStepRU) {
    // the rows' runs cut to n and to the chunk: [a, b), empty where a >= b
    int64_t s[kStepRU], a[kStepRU], b[kStepRU];
    int lo[kStepRU], hi[kStepRU];
#pragma unroll
    for (int u = 0; u < kStepRU; ++u) {
      const int r = rbase + g + u;
      s[u] = (int64_t)r * G.Np + j0;
      a[u] = i64max(s[u], clo);
      b[u] = r < G.r1 ? i64min(i64min(s[u] + ncol, G.n), chi) : a[u];
      lo[u] = 1;
      hi[u] = a[u] < b[u] ? nt : 1;
    }
    // the first s in [1, nt] with off[s] > a: tensor s - 1 holds a (zero-length tensors are
    // passed over); the rows in lock step, every round's loads independent
    for (int span = nt - 1; span > 0; span >>= 1) {
#pragma unroll
      for (int u = 0; u < kStepRU; ++u) {
        if (lo[u] < hi[u]) {
          const int mid = (lo[u] + hi[u]) >> 1;
          if (tb.off[mid] > a[u]) hi[u] = mid; else lo[u] = mid + 1;
        }
      }
    }
    // one tensor per run and one dtype in the group?
    bool single = true;
    int dt = -1;
#pragma unroll
    for (int u = 0; u < kStepRU; ++u) {
      if (a[u] < b[u]) {
        const int t = lo[u] - 1;
        single = single && tb.off[t + 1] >= b[u] && (dt < 0 || dt == (int)tb.dt[t]);
        dt = tb.dt[t];
      }
    }
    if (dt < 0) continue;  // nothing in this group
    if (single) {
      for_dtype(dt, [&](auto DT) {
        uint32_t raw[kStepRU][4];
        bool vec[kStepRU];
#pragma unroll
        for (int u = 0; u < kStepRU; ++u) {
          vec[u] = false;
          if (a[u] < b[u]) {
            const int t = lo[u] - 1;
            vec[u] = piece_vec<DT>(tb.p[t], tb.off[t], s[u], a[u], b[u]);
            piece_load<DT>(tb.p[t], tb.off[t], s[u], a[u], b[u], vec[u], lane, raw[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < kStepRU; ++u) {
          if (a[u] < b[u]) {
            const int t = lo[u] - 1;
            piece_store<DT>(tb.p[t], tb.off[t], tb.lr[t], s[u], a[u], b[u], vec[u], lane, rbase + g + u, wv, we,
                            raw[u]);
          }
        }
      });
      continue;
    }
    // runs cut by tensor boundaries, or a group of mixed dtypes: row by row, piece by piece
#pragma unroll
    for (int u = 0; u < kStepRU; ++u) {
      if (a[u] >= b[u]) continue;
      for (int t = lo[u] - 1; t < nt && tb.off[t] < b[u]; ++t) {
        const int64_t pa = i64max(a[u], tb.off[t]), pb = i64min(b[u], tb.off[t + 1]);
        if (pa >= pb) continue;  // a zero-length tensor
        for_dtype(tb.dt[t], [&](auto DT) {
          uint32_t raw[4];
          const bool vec = piece_vec<DT>(tb.p[t], tb.off[t], s[u], pa, pb);
          piece_load<DT>(tb.p[t], tb.off[t], s[u], pa, pb, vec, lane, raw);
          piece_store<DT>(tb.p[t], tb.off[t], tb.lr[t], s[u], pa, pb, vec, lane, rbase + g + u, wv, we, raw);
        });
      }
    }
  }
}

struct StepArgs {
  void* const* params;
  const int64_t* lens;
  const int32_t* dtypes;
  const double* lr;
  int32_t nseg;
  const int32_t* verdict;
  int64_t n;
};

// torch's conversion of the Python scalar alpha for an add_ on a tensor of this dtype: to fp32 and,
// for a 16-bit tensor, on to that dtype (round-to-nearest-even), then widened for the op's fp32 math
static float lr_as(int dt, double lr) {
  const float f = (float)lr;
  if (dt == CHOCO_DT_F32 || !std::isfinite(f)) return f;
  if (dt == CHOCO_DT_F16) return (float)(_Float16)f;
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
  float r;
  std::memcpy(&r, &u, 4);
  return r;
}

// Every argument is checked before the first launch, with no HIP call.
static int step_check(const StepArgs& a) {
  CHOCO_REQUIRE(a.params && a.lens && a.dtypes && a.lr, "null table argument");
  return layout_check(
      a.lens, a.dtypes, a.nseg, a.n,
      [&]() -> int {
        CHOCO_REQUIRE(a.verdict, "verdict is null");
        CHOCO_REQUIRE(aligned4(a.verdict), "verdict must be 4-byte aligned");
        return CHOCO_OK;
      },
      [&](int32_t s, uintptr_t esz) -> int {
        CHOCO_REQUIRE(elem_aligned(a.params[s], esz), "tensor %d: pointer not aligned to its element size", (int)s);
        CHOCO_REQUIRE(a.lens[s] == 0 || a.params[s], "tensor %d: null param pointer", (int)s);
        CHOCO_REQUIRE(std::isfinite(a.lr[s]) && std::isfinite(lr_as(a.dtypes[s], a.lr[s])),
                      "tensor %d: lr must be finite (in the tensor's dtype), got %g", (int)s, a.lr[s]);
        return CHOCO_OK;
      });
}

static int step_run(const StepArgs& a, hipStream_t st) {
  CHOCO_TRY(step_check(a));
  StepGeom G;
  G.n = a.n;
  G.Np = (a.n + 31) / 32;
  const uint32_t* verdict = reinterpret_cast<const uint32_t*>(a.verdict);
  StepTable tb;
  return for_chunks<kStepCap>(a.lens, a.nseg, tb.off, [&](const Chunk& c) -> int {
    tb.nt = c.nt;
    for (int i = 0; i < kStepCap; ++i) {
      const bool in = i < c.nt;
      tb.p[i] = in ? a.params[c.s0 + i] : nullptr;
      tb.lr[i] = in ? lr_as(a.dtypes[c.s0 + i], a.lr[c.s0 + i]) : 0.f;
      tb.dt[i] = in ? (uint8_t)a.dtypes[c.s0 + i] : (uint8_t)0;
    }
    // the rows and column blocks the chunk's flat range touches (an empty chunk: one workgroup
    // that finds nothing)
    const int64_t lo = tb.off[0], hi = tb.off[c.nt];
    G.cb0 = 0; G.ncb = 1; G.r0 = 0; G.r1 = 1;
    if (hi > lo) {
      const int64_t rlo = lo / G.Np, rhi = (hi - 1) / G.Np;
      G.r0 = (int32_t)rlo;
      G.r1 = (int32_t)rhi + 1;
      // one row: its columns; more: a row's end and the next row's start, every column block
      const int64_t c0 = rlo == rhi ? (lo - rlo * G.Np) / kStepCols : 0;
      const int64_t c1 = rlo == rhi ? (hi - 1 - rlo * G.Np) / kStepCols : (G.Np - 1) / kStepCols;
      G.cb0 = (int32_t)c0;
      G.ncb = (int32_t)(c1 - c0 + 1);
    }
    G.nrb = (G.r1 - G.r0 + kStepRows - 1) / kStepRows;
    const unsigned grid = (unsigned)((G.ncb + 7) / 8 * 8 * G.nrb);
    return CHOCO_LAUNCH("param_sign_step_kernel", "param_sign_step_kernel", param_sign_step_kernel, dim3(grid),
                        dim3(kStepThreads), st, tb, verdict, G);
  });
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_sign_step_launches(int32_t nseg) { return chunk_launches(nseg, kStepCap); }

CHOCO_API int choco_params_sign_step(void* const* params, const int64_t* lens, const int32_t* dtypes, const double* lr,
                                     int32_t nseg, const int32_t* verdict, int64_t n, void* stream) {
  const StepArgs a{params, lens, dtypes, lr, nseg, verdict, n};
  return step_run(a, as_stream(stream));
}
