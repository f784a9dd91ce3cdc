// Exact single-workgroup selection, shared by the flat pipeline (topk.hip: small n
// and the segmented fallback) and the batched segmented select (topk_seg.hip: a
// segment whose warm window missed).  Semantics as in topk.hip's header:
//   T = k-th largest key, out = {key > T} U {the lowest-index ties at T}, ascending.
#pragma once

#include "choco_common.h"

namespace choco {

// ----------------------------------------------------------------------------
// key / value sources
// ----------------------------------------------------------------------------
template <int MODE, bool XH>
struct Src {
  const float* __restrict__ x;
  const float* __restrict__ xh;
  uint64_t seed;
  CHOCO_DEV float val(int64_t i) const { return XH ? x[i] - xh[i] : x[i]; }
  // the fused gossip step on one element: x[i] <- x_new, returns x_new - xh[i]
  CHOCO_DEV float val_gossip(int64_t i, const Gossip& g) const {
    const float xn = gossip1(x[i], g.mem[i], xh[i], g.gamma);
    const_cast<float*>(x)[i] = xn;
    return xn - xh[i];
  }
  CHOCO_DEV uint32_t key_of(int64_t i, float v) const {
    if (MODE == kHash) return rank_hash(seed, (uint32_t)i) >> 1;
    return fkey(v);
  }
  CHOCO_DEV uint32_t key(int64_t i) const {
    if (MODE == kHash) return rank_hash(seed, (uint32_t)i) >> 1;
    return fkey(val(i));
  }
};

// ----------------------------------------------------------------------------
// block-wide rank search over a histogram
// ----------------------------------------------------------------------------
// Every thread of the workgroup holds PER consecutive bins of a histogram in ascending key
// order: hv[j] = bin PER * tid + j.  All threads call these; `scratch` as block_excl_scan.
struct BinScan {
  uint32_t local;  // the sum of this thread's bins
  uint32_t pre;    // the sum of the bins below them
  uint32_t total;  // the sum of all bins
};
template <int PER>
CHOCO_DEV BinScan block_bin_scan(const uint32_t (&hv)[PER], uint32_t* scratch) {
  BinScan s;
  s.local = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) s.local += hv[j];
  s.pre = block_excl_scan(s.local, scratch, &s.total);
  return s;
}

// The bin holding the rank-th largest entry and the rank inside it -> out[2q], out[2q + 1] for
// each of the NR ranks; a rank of 0, or one above the total, writes nothing.  TOTAL (one rank
// only): the histogram total -> out[2].  Ends with a barrier.
// (With two ranks the zero test is written out although `above < 0` is never true: without
// it seg_emit_w_kernel<true>, at its 72-VGPR budget, took 8 bytes of scratch.)
template <bool TOTAL = false, int PER, int NR>
CHOCO_DEV void block_find_ranks(const uint32_t (&hv)[PER], const uint32_t (&ranks)[NR], uint32_t* scratch,
                                uint32_t* out) {
  static_assert(!TOTAL || NR == 1, "out[2] is the second rank's bin");
  const int tid = threadIdx.x;
  const BinScan s = block_bin_scan(hv, scratch);
  const uint32_t above = s.total - s.pre - s.local;  // entries in bins above mine
  if (TOTAL && tid == 0) out[2] = s.total;
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    const uint32_t r = ranks[q];
    if ((NR == 1 || r != 0u) && above < r && r <= above + s.local) {
      uint32_t acc = above;
#pragma unroll
      for (int j = PER - 1; j >= 0; --j) {
        if (acc < r && r <= acc + hv[j]) { out[2 * q] = (uint32_t)(PER * tid + j); out[2 * q + 1] = r - acc; }
        acc += hv[j];
      }
    }
  }
  __syncthreads();
}
template <bool TOTAL = false, int PER>
CHOCO_DEV void block_find_rank(const uint32_t (&hv)[PER], uint32_t rank, uint32_t* scratch, uint32_t* out) {
  const uint32_t ranks[1] = {rank};
  block_find_ranks<TOTAL>(hv, ranks, scratch, out);
}

// ... over a histogram in LDS or global memory: this thread's PER bins
template <int PER>
CHOCO_DEV void load_bins(const uint32_t* hist, uint32_t (&hv)[PER]) {
#pragma unroll
  for (int j = 0; j < PER; ++j) hv[j] = hist[PER * threadIdx.x + j];
}
template <int PER, bool TOTAL = false>
CHOCO_DEV void block_find_rank_in(const uint32_t* hist, uint32_t rank, uint32_t* scratch, uint32_t* out) {
  uint32_t hv[PER];
  load_bins(hist, hv);
  block_find_rank<TOTAL>(hv, rank, scratch, out);
}
// hist[2048] and an NT-thread workgroup, two ranks -> out[0..1], out[2..3]
template <int NT = 1024>
CHOCO_DEV void block_find_two(const uint32_t* hist, uint32_t r0, uint32_t r1, uint32_t* scratch, uint32_t* out) {
  static_assert(2048 % NT == 0, "whole bins per thread");
  uint32_t hv[2048 / NT];
  load_bins(hist, hv);
  const uint32_t ranks[2] = {r0, r1};
  block_find_ranks(hv, ranks, scratch, out);
}

// ----------------------------------------------------------------------------
// exact single-workgroup select (small n, segments, fallback)
// ----------------------------------------------------------------------------
struct ExactSmem {
  uint32_t hist[2048];
  uint32_t scratch[40];  // block_excl_scan2: 2 words per wave
  uint32_t bc[4];
};

// Returns T (k-th largest key) and the tie quota r via bc[0], bc[1]; bc[2] = #ties at T.
// NT: the workgroup's threads.
template <int NT, class S>
CHOCO_DEV void block_select_T(const S& src, int64_t n, int64_t k, ExactSmem& sm) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0, maskhi = 0;
  uint32_t krem = (uint32_t)k;
  const int shs[3] = {20, 9, 0};
  const int wds[3] = {11, 11, 9};
  for (int rd = 0; rd < 3; ++rd) {
    const int sh = shs[rd];
    const uint32_t dmask = (1u << wds[rd]) - 1u;
    for (int i = tid; i < 2048; i += NT) sm.hist[i] = 0;
    __syncthreads();
    for (int64_t i = tid; i < n; i += NT) {
      uint32_t key = src.key(i);
      if ((key & maskhi) == prefix) atomicAdd(&sm.hist[(key >> sh) & dmask], 1u);
    }
    __syncthreads();
    block_find_two<NT>(sm.hist, krem, 0u, sm.scratch, sm.bc);  // (the bins past a 9-bit digit are zero)
    prefix |= sm.bc[0] << sh;
    maskhi |= dmask << sh;
    krem = sm.bc[1];
    if (rd == 2 && tid == 0) sm.bc[2] = sm.hist[sm.bc[0]];  // entries of the last digit's bin: keys equal to T
    __syncthreads();
  }
  if (tid == 0) { sm.bc[0] = prefix; sm.bc[1] = krem; }
  __syncthreads();
}

// Ordered compaction of the selection defined by (T, r) over [0, n).
template <class S>
CHOCO_DEV void block_emit(const S& src, int64_t n, uint32_t T, uint32_t r, uint32_t ties_total,
                          float scale, float* __restrict__ out_val, int32_t* __restrict__ out_idx,
                          int64_t idx_base, ExactSmem& sm) {
  const int tid = threadIdx.x, B = blockDim.x;
  const bool all_ties = (r == ties_total);
  uint32_t out = 0, tie_run = 0;
  for (int64_t base = 0; base < n; base += B) {
    const int64_t i = base + tid;
    const bool valid = i < n;
    float v = 0.f;
    uint32_t key = 0;
    if (valid) { v = src.val(i); key = src.key_of(i, v); }
    const bool gt = valid && key > T;
    const bool eq = valid && key == T;
    bool sel;
    if (all_ties) {
      sel = gt || eq;
    } else {
      uint32_t ntie;
      uint32_t trank = tie_run + block_excl_scan(eq ? 1u : 0u, sm.scratch, &ntie);
      sel = gt || (eq && trank < r);
      tie_run += ntie;
    }
    uint32_t nsel;
    uint32_t pos = out + block_excl_scan(sel ? 1u : 0u, sm.scratch, &nsel);
    if (sel) {
      out_val[pos] = v * scale;
      out_idx[pos] = (int32_t)(i + idx_base);
    }
    out += nsel;
  }
}

template <int NT, class S>
CHOCO_DEV void block_topk_exact(const S& src, int64_t n, int64_t k, float scale,
                                float* out_val, int32_t* out_idx, int64_t idx_base, ExactSmem& sm) {
  if (k >= n) {
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      out_val[i] = src.val(i) * scale;
      out_idx[i] = (int32_t)(i + idx_base);
    }
    return;
  }
  block_select_T<NT>(src, n, k, sm);
  const uint32_t T = sm.bc[0], r = sm.bc[1], ties = sm.bc[2];
  __syncthreads();
  block_emit(src, n, T, r, ties, scale, out_val, out_idx, idx_base, sm);
}

}  // namespace choco
