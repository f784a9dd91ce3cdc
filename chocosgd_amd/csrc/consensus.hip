// Consensus evaluation (--evaluate_consensus of the reference: distributed_running_cv.py:110-115,
// :239-243; agg_model, communication.py:114-122; get_model_difference, auxiliary.py:18-34): the
// model averaged over the workers and the L2 distance of this worker's model to that average, for
// a whole list of parameter tensors in ONE batched launch per chunk, straight from the flat fp32
// buffer the all-reduce SUM left (no copy of the model, no per-tensor division, subtraction,
// concatenation or norm).
//
// Flat index i, element j of tensor s, each line with exactly one rounding:
//     a = __fdiv_rn(xsum[i], div)                     a correctly rounded division, never a reciprocal multiply
//     x = master ? master[i] : (float)params[s][j]    widening is exact
//     d = __fsub_rn(a, x)                             weights2 - weights1 (auxiliary.py:32)
//     DIST:       ssd_s += (double)d * d,  ssa_s += (double)a * a
//     WRITE_AVG:  avg_out[s][j] = narrow_rne(a)
// avg_out[s] may be params[s]: each element is read before the same thread writes it.
//
// The sums are fp64 (the square of an fp32 value is exact there and the sum cannot overflow) and
// are taken in ONE fixed order that depends on the layout alone -- not on the pointers'
// alignment, not on how the tensors fall into launches, and there are no floating-point atomics:
//   * the span [lo, hi) of a tensor inside an 8192-element tile of at most kConsWaveMax elements:
//     one wave; lane l adds elements lo + l, lo + l + 64, ... in ascending order; the 64 lane sums
//     are joined by the xor butterfly (32, 16, 8, 4, 2, 1);
//   * a longer span: group g = i >> 3 (groups sit at absolute flat offsets) belongs to thread
//     (g - (lo >> 3)) mod 256, which adds its groups in ascending order and a group's elements in
//     ascending order; the butterfly per wave, then ((w0 + w1) + w2) + w3;
//   * every (tile, tensor) pair stores its two partials in slots of its own (param_sqnorm_kernel's
//     layout: slot tile + s, a tensor's slots contiguous); param_consensus_total_kernel adds a
//     tensor's slots in ascending order, then the tensors' sums in ascending order.
// Because the order must not depend on alignment, the thread that owns a group also takes it where
// the 16-byte path is not available (element by element, 32 bytes per lane); the 16-byte path
// (whole groups, non-temporal, every load of a group issued before its store) is taken by a
// tensor when xsum (and master) is 16-byte aligned and every side it touches is congruent with
// the group grid at that side's element size.
//
// The launch has the parameter bridge's shape (params.hip, sgd.hip, ef.hip): workgroups own
// 8192-element tiles at absolute flat offsets, the chunk's table travels in the kernel arguments,
// the first tensor of a tile comes from the shared uniform search, zero-length tensors are passed
// over.  Only the layout's own bytes of avg_out are written; xsum, master and (unless aliased)
// the parameters are read only.
#include "param_common.h"

#include <cmath>

namespace choco {

constexpr int kConsCap = 128;  // tensors per launch (ResNet-50's 161: two launches)
constexpr int64_t kConsWaveMax = 1024;

struct ConsTable {
  const void* p[kConsCap];   // the parameters (read under DIST without a master copy)
  void* q[kConsCap];         // avg_out (written under WRITE_AVG)
  int64_t off[kConsCap + 1]; // absolute flat offsets; off[nt] = end of the chunk
  uint8_t dt[kConsCap];      // CHOCO_DT_*
  int32_t nt;
};
// the table, five pointers, tile0 and four words: a launch carries at most 4 KB of arguments
static_assert(sizeof(ConsTable) + 64 <= 4096 - 256, "the table must fit in the kernel arguments");

// what one tensor's elements need (workgroup-uniform)
struct ConsOp {
  const float* xsum;
  const float* master;  // nullptr: x is the parameter
  const void* p;
  void* q;
  float div;
  bool wr;
};

// a = xsum[i] / div, x the widened parameter or the master value
template <bool DIST>
CHOCO_DEV void cons_acc(float a, float x, double& sd, double& sa) {
  if (!DIST) return;
  const float d = __fsub_rn(a, x);
  sd += (double)d * (double)d;
  sa += (double)a * (double)a;
}

// flat index i, element j of the tensor
template <int DT, bool DIST>
CHOCO_DEV void cons_elem(const ConsOp& o, int64_t i, int64_t j, double& sd, double& sa) {
  float a = __fdiv_rn(o.xsum[i], o.div);
  if (DIST) cons_acc<DIST>(a, o.master ? o.master[i] : ld1<DT>(o.p, j), sd, sa);
  if (o.wr) {
    if (DT != CHOCO_DT_F32) asm("" : "+v"(a));  // the narrowing starts from the rounded fp32 quotient (see rnd)
    st1<DT>(o.q, j, a);
  }
}

// Flat elements [a, b) of a tensor at flat offset o0, a < b inside this workgroup's tile, by the
// whole workgroup: thread tid owns groups (a >> 3) + tid, + 256, ...
// vec: every side the tensor touches is 16-byte aligned at every whole group's start.
// Not the shared span_walk: off the 16-byte grid that walk hands a thread elements a + tid,
// a + tid + 256, ..., so which values a thread adds, and in what order, would depend on the
// pointers' alignment; here the group's owner takes it either way and the fp64 order stays fixed.
template <int DT, bool DIST>
CHOCO_DEV void cons_span(const ConsOp& o, int64_t o0, int64_t a, int64_t b, bool vec, double& sd, double& sa) {
  const int tid = threadIdx.x;
  const int64_t g0 = a >> 3, g1 = (b - 1) >> 3;  // groups at absolute flat offsets, inclusive
  for (int64_t gb = g0; gb <= g1; gb += kPbThreads) {
    const int64_t e = (gb + tid) * kPbGroup;
    if (vec && e >= a && e + kPbGroup <= b) {
      // every load of the group is issued before its store
      Raw8 rs, rx;
      ld8<CHOCO_DT_F32>(rs, o.xsum, e);
      if (DIST) {
        if (o.master) ld8<CHOCO_DT_F32>(rx, o.master, e);
        else ld8<DT>(rx, o.p, e - o0);
      }
      float av[8], x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      widen8<CHOCO_DT_F32>(rs, av);
      if (DIST) {
        if (o.master) widen8<CHOCO_DT_F32>(rx, x);
        else widen8<DT>(rx, x);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        av[k] = __fdiv_rn(av[k], o.div);
        cons_acc<DIST>(av[k], x[k], sd, sa);
        if (DT != CHOCO_DT_F32) asm("" : "+v"(av[k]));
      }
      if (o.wr) st8<DT>(o.q, e - o0, av);
    } else {
      // a group cut by the span's start or end (or past it), or a tensor off the 16-byte grid:
      // the group's own elements, by the thread that owns the group
      const int64_t ea = e > a ? e : a, eb = e + kPbGroup < b ? e + kPbGroup : b;
      for (int64_t i = ea; i < eb; ++i) cons_elem<DT, DIST>(o, i, i - o0, sd, sa);
    }
  }
}

// ... by one wave, lane `lane` taking elements a + lane, a + lane + 64, ...
template <int DT, bool DIST>
CHOCO_DEV void cons_wave(const ConsOp& o, int64_t o0, int64_t a, int64_t b, int lane, double& sd, double& sa) {
  for (int64_t i = a + lane; i < b; i += 64) cons_elem<DT, DIST>(o, i, i - o0, sd, sa);
}

// meta: two words per tensor of the chunk, {first slot, slots}; slots_d / slots_a: the partial
// sums of d^2 and a^2, one per (tile, tensor) pair at slot tile + seg0 + s.
// al16: bit 0 xsum, bit 1 master 16-byte aligned (bit 1 set when there is no master)
template <bool DIST>
__global__ __launch_bounds__(kPbThreads) void param_consensus_kernel(const ConsTable tb, const float* xsum,
                                                                     const float* master, double* slots_d,
                                                                     double* slots_a, int32_t* meta, int64_t tile0,
                                                                     int32_t seg0, float div, int32_t mode,
                                                                     int32_t al16) {
  __shared__ double red[2 * (kPbThreads / 64)];
  const int nt = tb.nt;
  const int tid = threadIdx.x;
  if (DIST && blockIdx.x == 0) {
    for (int s = 0; s < nt; ++s) {  // s is uniform: the table is read with scalar loads
      const int64_t o0 = tb.off[s], o1 = tb.off[s + 1];
      const int32_t cnt = o1 > o0 ? (int32_t)((o1 - 1) / kPbTile - o0 / kPbTile + 1) : 0;
      if (tid == (s & (kPbThreads - 1))) {
        meta[2 * s] = (int32_t)(o0 / kPbTile) + seg0 + s;
        meta[2 * s + 1] = cnt;
      }
    }
  }
  const int64_t tile = tile0 + blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  ConsOp o;
  o.xsum = xsum; o.master = master; o.div = div;
  o.wr = (mode & CHOCO_CONS_WRITE_AVG) != 0;
  const bool rd_p = DIST && master == nullptr;
  int nshort = 0;
  tile_walk(tb.off, nt, tile, [&](int s, int64_t a, int64_t b) {
    const int dt = tb.dt[s];
    const int64_t o0 = tb.off[s];
    o.p = tb.p[s];
    o.q = tb.q[s];
    double sd = 0.0, sa = 0.0;
    if (DIST && b - a <= kConsWaveMax) {
      // short spans are taken by the waves in turn, with no barrier
      const bool mine = (nshort & 3) == wave;
      ++nshort;
      if (!mine) return;
      for_dtype(dt, [&](auto DT) { cons_wave<DT, DIST>(o, o0, a, b, lane, sd, sa); });
      sd = wave_sum(sd);
      sa = wave_sum(sa);
      if (lane == 0) {
        slots_d[tile + seg0 + s] = sd;
        slots_a[tile + seg0 + s] = sa;
      }
      return;
    }
    const uintptr_t esz = dtype_size(dt);
    uintptr_t mis = 0;
    if (rd_p) mis |= mis16(o.p, esz, o0);
    if (o.wr) mis |= mis16(o.q, esz, o0);
    const bool vec = al16 == 3 && on_grid16(mis);
    for_dtype(dt, [&](auto DT) { cons_span<DT, DIST>(o, o0, a, b, vec, sd, sa); });
    if (DIST) {
      sd = wave_sum(sd);
      sa = wave_sum(sa);
      if (lane == 0) {
        red[wave] = sd;
        red[4 + wave] = sa;
      }
      __syncthreads();
      if (tid == 0) {
        slots_d[tile + seg0 + s] = ((red[0] + red[1]) + red[2]) + red[3];
        slots_a[tile + seg0 + s] = ((red[4] + red[5]) + red[6]) + red[7];
      }
      __syncthreads();  // red is reused by the next long span
    }
  });
}

// d = vd[0] + vd[1] + ... + vd[cnt - 1] and a = va[0] + ... + va[cnt - 1], each added in that order
// by one wave (cnt uniform): 64 at a time are loaded by the lanes side by side, then added one
// after the other through v_readlane; the two chains are independent and share the loop, so one
// fills the other's add latency.  Every lane gets both sums.
CHOCO_DEV void cons_ordered_sum2(const double* vd, const double* va, int32_t cnt, int lane, double& d, double& a) {
  d = 0.0;
  a = 0.0;
  for (int32_t base = 0; base < cnt; base += 64) {
    const int32_t i = base + lane;
    const double xd = i < cnt ? vd[i] : 0.0, xa = i < cnt ? va[i] : 0.0;
    const int dhi = __double2hiint(xd), dlo = __double2loint(xd);
    const int ahi = __double2hiint(xa), alo = __double2loint(xa);
    const int32_t m = cnt - base < 64 ? cnt - base : 64;
    for (int32_t l = 0; l < m; ++l) {
      d += __hiloint2double(__builtin_amdgcn_readlane(dhi, l), __builtin_amdgcn_readlane(dlo, l));
      a += __hiloint2double(__builtin_amdgcn_readlane(ahi, l), __builtin_amdgcn_readlane(alo, l));
    }
  }
}

// ONE workgroup: its waves take the tensors in turn and add a tensor's slots in ascending order
// (sums_d[s], sums_a[s]; dists[s] = (float)sqrt(sums_d[s])), then the first wave adds the tensors'
// sums in ascending order: out[0] = (float)sqrt(sum ssd), out[1] = (float)sqrt(sum ssa).
// One workgroup means latency, not bandwidth, is the cost: the slots, the meta words and the
// per-tensor sums of a layout that fits (ResNet-50: 3281 slots of each kind) are staged in LDS by
// one coalesced pass, as param_gradnorm_total_kernel stages them; a larger layout reads the
// workspace in place, with the same additions in the same order.
constexpr int kConsTotalThreads = 1024;
constexpr int kConsStageSlots = 4096;  // 2 x 32 KB of fp64 slots, 8 KB of meta words and 2 x 8 KB of sums in LDS
constexpr int kConsStageSegs = 1024;

__global__ __launch_bounds__(kConsTotalThreads) void param_consensus_total_kernel(const double* slots_d,
                                                                                  const double* slots_a,
                                                                                  int32_t nslots, const int32_t* meta,
                                                                                  double* sums_d, double* sums_a,
                                                                                  int32_t nseg, float* out,
                                                                                  float* dists) {
  __shared__ double s_slots_d[kConsStageSlots];
  __shared__ double s_slots_a[kConsStageSlots];
  __shared__ int32_t s_meta[2 * kConsStageSegs];
  __shared__ double s_sums_d[kConsStageSegs];
  __shared__ double s_sums_a[kConsStageSegs];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (nslots <= kConsStageSlots && nseg <= kConsStageSegs) {
    // slots no (tile, tensor) pair wrote hold whatever the workspace held: moved, never added
    for (int32_t i = tid; i < nslots; i += kConsTotalThreads) {
      s_slots_d[i] = slots_d[i];
      s_slots_a[i] = slots_a[i];
    }
    for (int32_t i = tid; i < 2 * nseg; i += kConsTotalThreads) s_meta[i] = meta[i];
    __syncthreads();
    slots_d = s_slots_d;
    slots_a = s_slots_a;
    meta = s_meta;
    sums_d = s_sums_d;
    sums_a = s_sums_a;
  }
  for (int32_t s = wave; s < nseg; s += kConsTotalThreads / 64) {
    const int32_t slot0 = __builtin_amdgcn_readfirstlane(meta[2 * s]);
    const int32_t cnt = __builtin_amdgcn_readfirstlane(meta[2 * s + 1]);
    double d, a;
    cons_ordered_sum2(slots_d + slot0, slots_a + slot0, cnt, lane, d, a);
    if (lane == 0) {
      sums_d[s] = d;
      sums_a[s] = a;
      if (dists != nullptr) dists[s] = (float)sqrt(d);
    }
  }
  __syncthreads();  // the sums of every wave, written above, are read by the first one
  if (wave != 0) return;
  double d, a;
  cons_ordered_sum2(sums_d, sums_a, nseg, lane, d, a);
  if (tid != 0) return;
  out[0] = (float)sqrt(d);
  out[1] = (float)sqrt(a);
}

constexpr int32_t kConsModes = CHOCO_CONS_DIST | CHOCO_CONS_WRITE_AVG;

static int cons_launches(int32_t nseg, int32_t mode) {
  if (nseg <= 0 || (mode & ~kConsModes) != 0 || (mode & kConsModes) == 0) return 0;
  return chunk_launches(nseg, kConsCap) + ((mode & CHOCO_CONS_DIST) ? 1 : 0);
}
// two partials per (tile, tensor) pair, two fp64 sums per tensor, the meta words
static size_t cons_slots(int32_t nseg, int64_t n) { return (size_t)(n / kPbTile + 1) + (size_t)nseg; }
static size_t cons_ws_bytes(int32_t nseg, int64_t n) {
  if (nseg <= 0 || n < 0) return 0;
  return align_up((2 * cons_slots(nseg, n) + 2 * (size_t)nseg) * sizeof(double) + (size_t)nseg * 2 * sizeof(int32_t),
                  256);
}

struct ConsArgs {
  const void* const* params;
  void* const* avg_out;
  const int64_t* lens;
  const int32_t* dtypes;
  int32_t nseg;
  const float* xsum;
  const float* master;
  int64_t n;
  double divisor;
  int32_t mode;
  float* out;
  float* dists;
  void* ws;
  size_t ws_bytes;
};

// Every argument is checked before the first launch, with no HIP call.
static int cons_check(const ConsArgs& a) {
  CHOCO_REQUIRE((a.mode & ~kConsModes) == 0, "unknown mode bits 0x%x", (unsigned)a.mode);
  CHOCO_REQUIRE((a.mode & kConsModes) != 0, "mode needs CHOCO_CONS_DIST or CHOCO_CONS_WRITE_AVG, got 0");
  const bool dist = (a.mode & CHOCO_CONS_DIST) != 0, wr = (a.mode & CHOCO_CONS_WRITE_AVG) != 0;
  const bool rd_p = dist && !a.master;
  CHOCO_REQUIRE(a.lens && a.dtypes, "null table argument: lens / dtypes");
  return layout_check(
      a.lens, a.dtypes, a.nseg, a.n,
      [&]() -> int {
        CHOCO_REQUIRE(a.params || !rd_p, "DIST without a master copy needs the params table");
        CHOCO_REQUIRE(a.avg_out || !wr, "WRITE_AVG with a null avg_out table");
        // tested as the kernel divides: by the fp32 value
        CHOCO_REQUIRE(std::isfinite(a.divisor) && (float)a.divisor != 0.0f && std::isfinite((float)a.divisor),
                      "divisor must be finite and nonzero as an fp32 value, got %g", a.divisor);
        CHOCO_REQUIRE(a.xsum || a.n == 0, "xsum is null");
        CHOCO_REQUIRE(aligned4(a.xsum), "xsum must be 4-byte aligned");
        CHOCO_REQUIRE(aligned4(a.master), "master must be 4-byte aligned");
        CHOCO_REQUIRE(aligned4(a.dists), "dists must be 4-byte aligned");
        if (dist) {
          CHOCO_REQUIRE(a.out && aligned4(a.out), "out must be a 4-byte aligned device pointer");
          CHOCO_REQUIRE(a.ws && (reinterpret_cast<uintptr_t>(a.ws) & 7u) == 0,
                        "the workspace (ws) must be an 8-byte aligned device pointer");
          CHOCO_REQUIRE(a.ws_bytes >= cons_ws_bytes(a.nseg, a.n), "workspace (ws) too small: %zu bytes, need %zu",
                        a.ws_bytes, cons_ws_bytes(a.nseg, a.n));
        } else {
          CHOCO_REQUIRE(!a.dists, "dists without CHOCO_CONS_DIST");
        }
        return CHOCO_OK;
      },
      [&](int32_t s, uintptr_t esz) -> int {
        const int i = (int)s;
        CHOCO_REQUIRE(!a.params || elem_aligned(a.params[s], esz),
                      "tensor %d: params pointer not aligned to its element size", i);
        CHOCO_REQUIRE(!a.avg_out || elem_aligned(a.avg_out[s], esz),
                      "tensor %d: avg_out pointer not aligned to its element size", i);
        if (a.lens[s] == 0) return CHOCO_OK;
        CHOCO_REQUIRE(!rd_p || a.params[s], "tensor %d: null params pointer", i);
        CHOCO_REQUIRE(!wr || a.avg_out[s], "tensor %d: null avg_out pointer with WRITE_AVG", i);
        return CHOCO_OK;
      },
      "lengths (lens)");
}

static int cons_run(const ConsArgs& a, hipStream_t st) {
  const int rc = cons_check(a);
  if (rc) return rc;
  const bool dist = (a.mode & CHOCO_CONS_DIST) != 0, wr = (a.mode & CHOCO_CONS_WRITE_AVG) != 0;
  const bool rd_p = dist && !a.master;
  double* slots_d = nullptr;
  double* slots_a = nullptr;
  double* sums_d = nullptr;
  double* sums_a = nullptr;
  int32_t* meta = nullptr;
  if (dist) {
    const size_t ns = cons_slots(a.nseg, a.n);
    slots_d = reinterpret_cast<double*>(a.ws);
    slots_a = slots_d + ns;
    sums_d = slots_a + ns;
    sums_a = sums_d + a.nseg;
    meta = reinterpret_cast<int32_t*>(sums_a + a.nseg);
  }
  const float div = (float)a.divisor;
  const int32_t al16 = (aligned16(a.xsum) ? 1 : 0) | (!a.master || !dist || aligned16(a.master) ? 2 : 0);
  const float* master = dist ? a.master : nullptr;  // WRITE_AVG alone reads neither master nor params
  ConsTable tb;
  CHOCO_TRY(for_chunks<kConsCap>(a.lens, a.nseg, tb.off, [&](const Chunk& c) -> int {
    tb.nt = c.nt;
    for (int i = 0; i < kConsCap; ++i) {
      const bool in = i < c.nt;
      tb.p[i] = in && rd_p ? a.params[c.s0 + i] : nullptr;
      tb.q[i] = in && wr ? a.avg_out[c.s0 + i] : nullptr;
      tb.dt[i] = in ? (uint8_t)a.dtypes[c.s0 + i] : (uint8_t)0;
    }
    if (dist)
      return CHOCO_LAUNCH("param_consensus_kernel", "param_consensus_kernel", param_consensus_kernel<true>,
                          dim3((unsigned)c.tiles), dim3(kPbThreads), st, tb, a.xsum, master, slots_d, slots_a,
                          meta + 2 * (size_t)c.s0, c.tile0, c.s0, div, a.mode, al16);
    return CHOCO_LAUNCH("param_consensus_kernel", "param_consensus_kernel<write>", param_consensus_kernel<false>,
                        dim3((unsigned)c.tiles), dim3(kPbThreads), st, tb, a.xsum, master, slots_d, slots_a, meta,
                        c.tile0, c.s0, div, a.mode, al16);
  }));
  if (dist)
    CHOCO_TRY(CHOCO_LAUNCH("param_consensus_total_kernel", "param_consensus_total_kernel",
                           param_consensus_total_kernel, dim3(1), dim3(kConsTotalThreads), st,
                           (const double*)slots_d, (const double*)slots_a, (int32_t)cons_slots(a.nseg, a.n),
                           (const int32_t*)meta, sums_d, sums_a, a.nseg, a.out, a.dists));
  return CHOCO_OK;
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_consensus_launches(int32_t nseg, int32_t mode) { return cons_launches(nseg, mode); }
CHOCO_API size_t choco_params_consensus_workspace_size(int32_t nseg, int64_t n) { return cons_ws_bytes(nseg, n); }

CHOCO_API int choco_params_consensus(const void* const* params, void* const* avg_out, const int64_t* lens,
                                     const int32_t* dtypes, int32_t nseg, const float* xsum, const float* master,
                                     int64_t n, double divisor, int32_t mode, float* out, float* dists, void* ws,
                                     size_t ws_bytes, void* stream) {
  const ConsArgs a{params, avg_out, lens, dtypes, nseg, xsum, master, n, divisor, mode, out, dists, ws, ws_bytes};
  return cons_run(a, as_stream(stream));
}
