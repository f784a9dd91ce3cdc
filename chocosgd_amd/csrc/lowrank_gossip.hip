// PowerGossip (Vogels, Karimireddy, Jaggi, NeurIPS 2020): the low-rank kernels of a decentralized
// worker, batched over its E edges (include/choco_codec.h, "low-rank gossip").
//
// Edge e = (me, j_e) runs a warm-started power iteration on X_me - X_j without either end forming
// the difference: both ends multiply their own X by the edge's shared Q_e and swap the thin
// products.  A worker with E neighbours holds E different Qs against the SAME X, so every pass
// over X here serves all edges at once, K = E r columns wide (K <= 8):
//     project        P_e = X Q_e for every e                      reads X:            4 B / element
//     orthogonalise  P^_e = MGS(P_e(lo end) - P_e(hi end))       one workgroup per (edge, matrix)
//     back-project   Q'_e = X^T P^_e for every e                  reads X:            4 B / element
//     diff           dQ_e = Q'_e(lo end) - Q'_e(hi end); the edge's next Q unless it is all zero
//     apply          X += sum_e c_e P^_e dQ_e^T                   reads and writes X: 8 B / element
// against PowerSGD's 12 + 4 + 12 B / element per Q (lowrank.hip), which a per-edge loop would pay E
// times.  The kernels read codec.LowRankPlan's tile table at rank r unchanged (lowrank.h: row items,
// back-project items, slab-sum items); the E edges' buffers are contiguous [E][msg1_len],
// [E][msg2_len] and [E][P_total] arrays, and the slab workspace is E times PowerSGD's.
//
// Templated on (ES, R): ES = E rounded up to 1, 2, 4 or 8 edge slots, R the rank, K = ES R <= 8
// planes / accumulators.  A padded slot's planes are zeros in LDS and nothing of it is ever stored.
//   * project: PowerSGD's project on K planes (lowrank.h, lr_project_rows: the wave-per-row walk with
//     16-byte loads on the flat buffer's 16-byte grid, scalar head and tail, a fixed butterfly, the
//     column blocks' sums added in ascending order) with all E Qs' column blocks in LDS; the block is
//     2048 columns up to K = 4 and 1024 at K = 8 (K planes x block x 4 B = 32 KB beside the 8 KB of row
//     sums).
//   * back-project: PowerSGD's kernel and slab-sum kernel themselves (lowrank.h,
//     lowrank_backproject_kernel<ES, R>; PowerSGD is its one-edge instance): 64 columns x one 256-row slab
//     an item, the slab's P^ rows of all edges in LDS, K accumulators a lane, slab partials summed in
//     ascending slab order by a grid of (items, E).
//   * apply: K planes of dQ through LDS in the same column blocks and the same walk (lr_row_walk), the
//     item's P^ rows of all edges in LDS; per element each edge's product is lr_chain, decode's, then
//     u = c_0 o_0, u = u + c_e o_e in ascending e (a multiply and an add, not fused), x = x + u.
//     c_e = -w_e at the edge's low end and +w_e at its high end: with bit-identical P^_e and dQ_e at
//     both ends (orthogonalise and diff see the same operands in the same order) the two ends'
//     updates are exact negations.  Tail items mix the uncompressed tensors plainly.
// No atomics: every output is a fixed-order function of its inputs, the same bits every call.
#include "lowrank.h"

#include <cmath>

namespace choco {

constexpr int kLgMaxK = 8;
constexpr int lg_colblock(int K) { return K <= 4 ? kLrColBlock : 1024; }
constexpr int lg_slots(int E) { return E <= 1 ? 1 : E <= 2 ? 2 : E <= 4 ? 4 : 8; }

// the signed weights of apply's matrix items (c) and the plain ones of its tail items (w)
struct LgWeights {
  float c[kLgMaxK], w[kLgMaxK];
};

// ---------------------------------------------------------------- project
template <int ES, int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_gossip_project_kernel(const float* __restrict__ x,
                                                                            const float* __restrict__ q,
                                                                            float* __restrict__ msg1, int E,
                                                                            const int64_t* __restrict__ plan) {
  constexpr int K = ES * R, CB = lg_colblock(K);
  __shared__ __attribute__((aligned(16))) float Qs[K * CB];
  __shared__ float psum[kLrRowCap * K];
  const int64_t m1 = plan[kLrMsg1], m2 = plan[kLrMsg2];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) {  // a piece of an uncompressed tensor: into every edge's message tail
    const int64_t off = it[1], tail = it[3];
    const int cnt = (int)it[2];
    for (int i = threadIdx.x; i < cnt; i += kLrThreads) {
      const float v = x[off + i];
      for (int e = 0; e < E; ++e) msg1[e * m1 + tail + i] = v;
    }
    return;
  }
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t row0 = it[1];
  const int nrows = (int)it[2];
  for (int i = E * R * CB + threadIdx.x; i < K * CB; i += kLrThreads) Qs[i] = 0.0f;  // the padded slots' planes
  lr_project_rows<R, K, CB>(
      Qs, psum, q, m2, E, M, row0, nrows, [&](int64_t i) LR_INLINE { return x[i]; },
      [&](int64_t i) LR_INLINE { return *reinterpret_cast<const float4*>(x + i); });
  for (int i = threadIdx.x; i < nrows * K; i += kLrThreads) {
    const int rl = i / K, k = i % K, e = k / R;
    if (e < E) msg1[e * m1 + M.poff + (row0 + rl) * R + k % R] = psum[i];
  }
}

// ---------------------------------------------------------------- orthogonalise
// one workgroup per (matrix, edge): dP = P(lo end) - P(hi end), one fp32 subtraction per element
// formed by the thread that owns the row in lr_mgs, then lowrank_orth_kernel's sweep; like it, with
// kLrHiOrthStage staged rows at ranks 8, 16 and 32 (the wide family, lowrank_gossip_mfma.hip)
template <int R, int STAGE = kLrOrthStage>
__global__ __launch_bounds__(kLrThreads) void lowrank_gossip_orth_kernel(const float* __restrict__ own,
                                                                         const float* __restrict__ recv,
                                                                         float* __restrict__ phat, uint32_t lo_mask,
                                                                         const int64_t* __restrict__ plan) {
  __shared__ float Ps[STAGE * R];
  __shared__ double red[kLrWaves][R];
  const LrMat M = lr_mat(plan, blockIdx.x);
  const int e = blockIdx.y;
  const bool lo = (lo_mask >> e) & 1u;
  const int64_t at1 = e * plan[kLrMsg1] + M.poff;
  const float* __restrict__ a = (lo ? own : recv) + at1;
  const float* __restrict__ b = (lo ? recv : own) + at1;
  float* P = phat + e * plan[kLrPTotal] + M.poff;
  for (int64_t i = threadIdx.x; i < M.rows; i += kLrThreads) {
    float* r = i < STAGE ? Ps + i * R : P + i * R;
#pragma unroll
    for (int c = 0; c < R; ++c) r[c] = a[i * R + c] - b[i * R + c];
  }
  __syncthreads();
  lr_mgs<R, STAGE>(P, M.rows, Ps, red);
  __syncthreads();
  const int ns = (int)(M.rows < STAGE ? M.rows : STAGE);
  for (int i = threadIdx.x; i < ns * R; i += kLrThreads) P[i] = Ps[i];
}

// ---------------------------------------------------------------- diff
// one workgroup per (matrix, edge): dQ = Q'(lo end) - Q'(hi end) into dq; the edge's Q state takes
// it unless every element is zero (an edge that once agrees exactly would otherwise be dead for good)
template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_gossip_diff_kernel(const float* __restrict__ own,
                                                                         const float* __restrict__ recv,
                                                                         float* __restrict__ q, float* __restrict__ dq,
                                                                         uint32_t lo_mask,
                                                                         const int64_t* __restrict__ plan) {
  const LrMat M = lr_mat(plan, blockIdx.x);
  const int e = blockIdx.y;
  const bool lo = (lo_mask >> e) & 1u;
  const int64_t at2 = e * plan[kLrMsg2] + M.qoff, ne = M.cols * R;
  const float* __restrict__ a = (lo ? own : recv) + at2;
  const float* __restrict__ b = (lo ? recv : own) + at2;
  int nz = 0;
  for (int64_t i = threadIdx.x; i < ne; i += kLrThreads) {
    const float d = a[i] - b[i];
    dq[at2 + i] = d;
    nz |= d != 0.0f;
  }
  if (!__syncthreads_or(nz)) return;
  for (int64_t i = threadIdx.x; i < ne; i += kLrThreads) q[at2 + i] = a[i] - b[i];
}

// ---------------------------------------------------------------- apply
// u = sum_e c_e (p_e . dq_e): each edge's product in column order, the edges in ascending order
template <int ES, int R>
CHOCO_DEV float lg_update(const float (&p)[ES * R], const float (&qc)[ES * R], const LgWeights& W, int E) {
  float u = 0.0f;
#pragma unroll
  for (int e = 0; e < ES; ++e) {
    if (e < E) {
      const float t = W.c[e] * lr_chain<R>(p + e * R, qc + e * R);
      u = e == 0 ? t : u + t;
    }
  }
  return u;
}

template <int ES, int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_gossip_apply_kernel(float* __restrict__ x,
                                                                          const float* __restrict__ phat,
                                                                          const float* __restrict__ dq,
                                                                          const float* __restrict__ recv1, LgWeights W,
                                                                          int E, const int64_t* __restrict__ plan) {
  constexpr int K = ES * R, CB = lg_colblock(K);
  __shared__ __attribute__((aligned(16))) float Qs[K * CB];
  __shared__ float Ps[kLrRowCap * K];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) {  // an uncompressed tensor: x + sum_e w_e (x_received,e - x) from the received tails
    const int64_t off = it[1], tail = it[3], m1 = plan[kLrMsg1];
    const int cnt = (int)it[2];
    for (int i = threadIdx.x; i < cnt; i += kLrThreads) {
      const float xv = x[off + i];
      float u = W.w[0] * (recv1[tail + i] - xv);
#pragma unroll
      for (int e = 1; e < ES; ++e)
        if (e < E) u = u + W.w[e] * (recv1[e * m1 + tail + i] - xv);
      x[off + i] = xv + u;
    }
    return;
  }
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t row0 = it[1];
  const int nrows = (int)it[2];
  const int w = threadIdx.x >> 6;
  for (int i = E * R * CB + threadIdx.x; i < K * CB; i += kLrThreads) Qs[i] = 0.0f;  // the padded slots' planes
  lr_stage_rows<ES, R>(Ps, phat, plan[kLrPTotal], M, row0, nrows, E);
  for (int64_t cb0 = 0; cb0 < M.cols; cb0 += CB) {
    const int nb = (int)(M.cols - cb0 < CB ? M.cols - cb0 : CB);
    __syncthreads();
    lr_stage<R, CB>(Qs, dq + M.qoff + cb0 * R, plan[kLrMsg2], E, nb);
    __syncthreads();
    for (int rl = w; rl < nrows; rl += kLrWaves) {
      float p[K];
#pragma unroll
      for (int k = 0; k < K; ++k) p[k] = Ps[rl * K + k];
      lr_row_walk(
          M.off + (row0 + rl) * M.cols + cb0, nb,
          [&](int64_t i, int j) LR_INLINE {
            float qc[K];
#pragma unroll
            for (int k = 0; k < K; ++k) qc[k] = Qs[k * CB + j];
            x[i] = x[i] + lg_update<ES, R>(p, qc, W, E);
          },
          [&](int64_t i, int j, bool al) LR_INLINE {
            const float4 m = *reinterpret_cast<const float4*>(x + i);
            float qq[K][4], qc[K], o[4];
            lr_q4<K, CB>(Qs, j, al, qq);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
              for (int k = 0; k < K; ++k) qc[k] = qq[k][u];
              o[u] = lg_update<ES, R>(p, qc, W, E);
            }
            *reinterpret_cast<float4*>(x + i) = make_float4(m.x + o[0], m.y + o[1], m.z + o[2], m.w + o[3]);
          });
    }
  }
}

// ---------------------------------------------------------------- launches
// (edge slots, rank) -> the kernel's instance, f(int_c<ES>, int_c<R>): the nine pairs with ES R <= 8
template <typename F>
int lg_dispatch(int32_t rank, int E, F&& f) {
  return dispatch_list<1, 2, 4, 8>(lg_slots(E), "edge slots", [&](auto ES) {
    return lr_dispatch_lo(rank, [&](auto R) {
      if constexpr (ES * R <= kLgMaxK)
        return f(ES, R);
      else
        return fail(CHOCO_ERR_INVALID, "no instance for %d edges at rank %d", (int)E, (int)rank);
    });
  });
}

// what every gossip launch checks first: lr_check, then the width
static int lg_check(const int64_t* plan_host, const void* plan_dev, int64_t n, int32_t rank, int32_t n_edges,
                    int64_t msg1_len, int64_t msg2_len) {
  CHOCO_TRY(lr_check(plan_host, plan_dev, n, rank, msg1_len, msg2_len));
  CHOCO_REQUIRE(n_edges >= 1, "n_edges must be at least 1, got %d", (int)n_edges);
  CHOCO_REQUIRE(rank <= 4 && (int64_t)n_edges * rank <= kLgMaxK,
                "n_edges * rank must be at most %d at rank 1, 2 or 4, got %d edges at rank %d", kLgMaxK, (int)n_edges,
                (int)rank);
  return CHOCO_OK;
}

// orthogonalise and diff are per (matrix, edge) at rank r, whatever the width: both families launch these
int lg_orth(int32_t rank, dim3 grid, hipStream_t st, const float* own, const float* recv, float* phat, uint32_t lo_mask,
            const int64_t* plan) {
  if (lr_rank_hi(rank))
    return lr_dispatch_hi(rank, [&](auto R) {
      return CHOCO_LAUNCH("lowrank_gossip_orth_kernel", "lowrank_gossip_orth_kernel",
                          (lowrank_gossip_orth_kernel<R, kLrHiOrthStage>), grid, dim3(kLrThreads), st, own, recv, phat,
                          lo_mask, plan);
    });
  return lr_dispatch_lo(rank, [&](auto R) {
    return CHOCO_LAUNCH("lowrank_gossip_orth_kernel", "lowrank_gossip_orth_kernel", lowrank_gossip_orth_kernel<R>, grid,
                        dim3(kLrThreads), st, own, recv, phat, lo_mask, plan);
  });
}

int lg_diff(int32_t rank, dim3 grid, hipStream_t st, const float* own, const float* recv, float* q, float* dq,
            uint32_t lo_mask, const int64_t* plan) {
  return dispatch_list<1, 2, 4, 8, 16, 32>(rank, "rank", [&](auto R) {
    return CHOCO_LAUNCH("lowrank_gossip_diff_kernel", "lowrank_gossip_diff_kernel", lowrank_gossip_diff_kernel<R>, grid,
                        dim3(kLrThreads), st, own, recv, q, dq, lo_mask, plan);
  });
}

}  // namespace choco

using namespace choco;

CHOCO_API size_t choco_lowrank_gossip_workspace_size(const int64_t* plan_host, int32_t n_edges) {
  if (!plan_host || plan_host[kLrMagic] != kLrMagicValue || n_edges < 1 || n_edges > kLgMaxK) return 0;
  return align_up((size_t)n_edges * (size_t)plan_host[kLrWsFloats] * sizeof(float), 256) + 256;
}

CHOCO_API int choco_lowrank_gossip_project(const float* x, const float* q, float* msg1, int64_t msg1_len,
                                           int64_t msg2_len, const int64_t* plan_host, const int64_t* plan_dev,
                                           int64_t n, int32_t rank, int32_t n_edges, void* stream) {
  CHOCO_REQUIRE(x && msg1, "null pointer");
  CHOCO_TRY(lg_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  CHOCO_REQUIRE(q || plan_host[kLrMsg2] == 0, "null pointer");
  CHOCO_REQUIRE(aligned16(x), "x must be 16-byte aligned");
  CHOCO_REQUIRE(aligned4(q) && aligned4(msg1), "q and msg1 must be 4-byte aligned");
  return lg_dispatch(rank, n_edges, [&](auto ES, auto R) {
    return CHOCO_LAUNCH("lowrank_gossip_project_kernel", "lowrank_gossip_project_kernel",
                        (lowrank_gossip_project_kernel<ES, R>), dim3((unsigned)plan_host[kLrNRow]), dim3(kLrThreads),
                        as_stream(stream), x, q, msg1, n_edges, plan_dev);
  });
}

CHOCO_API int choco_lowrank_gossip_orthogonalize(const float* msg1_own, const float* msg1_recv, int64_t msg1_len,
                                                 float* phat, uint32_t lo_mask, const int64_t* plan_host,
                                                 const int64_t* plan_dev, int64_t n, int32_t rank, int32_t n_edges,
                                                 void* stream) {
  CHOCO_REQUIRE(msg1_own && msg1_recv, "null pointer");
  CHOCO_TRY(lg_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, -1));
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  CHOCO_REQUIRE(phat, "null pointer");
  CHOCO_REQUIRE(aligned4(msg1_own) && aligned4(msg1_recv) && aligned4(phat), "misaligned pointer");
  return lg_orth(rank, dim3((unsigned)plan_host[kLrNcomp], (unsigned)n_edges), as_stream(stream), msg1_own, msg1_recv,
                 phat, lo_mask, plan_dev);
}

CHOCO_API int choco_lowrank_gossip_backproject(const float* x, const float* phat, int64_t msg1_len, float* msg2,
                                               int64_t msg2_len, void* ws, size_t ws_bytes, const int64_t* plan_host,
                                               const int64_t* plan_dev, int64_t n, int32_t rank, int32_t n_edges,
                                               void* stream) {
  CHOCO_REQUIRE(x, "null pointer");
  CHOCO_TRY(lg_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  CHOCO_REQUIRE(phat && msg2 && ws, "null pointer");
  CHOCO_REQUIRE(ws_bytes >= choco_lowrank_gossip_workspace_size(plan_host, n_edges),
                "workspace too small: %zu bytes, need %zu", ws_bytes,
                choco_lowrank_gossip_workspace_size(plan_host, n_edges));
  CHOCO_REQUIRE(aligned4(x) && aligned4(phat) && aligned4(msg2) && aligned16(ws), "misaligned pointer");
  const hipStream_t st = as_stream(stream);
  float* wsf = reinterpret_cast<float*>(ws);
  CHOCO_TRY(lg_dispatch(rank, n_edges, [&](auto ES, auto R) {
    return CHOCO_LAUNCH("lowrank_gossip_backproject_kernel", "lowrank_gossip_backproject_kernel",
                        (lowrank_backproject_kernel<ES, R>), dim3((unsigned)plan_host[kLrNBp]), dim3(kLrThreads), st, x,
                        phat, msg2, wsf, n_edges, plan_dev);
  }));
  if (plan_host[kLrNSum] == 0) return CHOCO_OK;
  return CHOCO_LAUNCH("lowrank_gossip_slabsum_kernel", "lowrank_gossip_slabsum_kernel", lowrank_slabsum_kernel,
                      dim3((unsigned)plan_host[kLrNSum], (unsigned)n_edges), dim3(kLrThreads), st, (const float*)wsf,
                      msg2, plan_dev);
}

CHOCO_API int choco_lowrank_gossip_diff(const float* msg2_own, const float* msg2_recv, int64_t msg1_len,
                                        int64_t msg2_len, float* q, float* dq, uint32_t lo_mask,
                                        const int64_t* plan_host, const int64_t* plan_dev, int64_t n, int32_t rank,
                                        int32_t n_edges, void* stream) {
  CHOCO_TRY(lg_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  CHOCO_REQUIRE(msg2_own && msg2_recv && q && dq, "null pointer");
  CHOCO_REQUIRE(aligned4(msg2_own) && aligned4(msg2_recv) && aligned4(q) && aligned4(dq), "misaligned pointer");
  return lg_diff(rank, dim3((unsigned)plan_host[kLrNcomp], (unsigned)n_edges), as_stream(stream), msg2_own, msg2_recv, q,
                 dq, lo_mask, plan_dev);
}

CHOCO_API int choco_lowrank_gossip_apply(float* x, const float* phat, const float* dq, const float* msg1_recv,
                                         int64_t msg1_len, int64_t msg2_len, const double* weights, uint32_t lo_mask,
                                         const int64_t* plan_host, const int64_t* plan_dev, int64_t n, int32_t rank,
                                         int32_t n_edges, void* stream) {
  CHOCO_REQUIRE(x && msg1_recv && weights, "null pointer");
  CHOCO_TRY(lg_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  CHOCO_REQUIRE((phat && dq) || plan_host[kLrNcomp] == 0, "null pointer");
  CHOCO_REQUIRE(aligned16(x), "x must be 16-byte aligned");
  CHOCO_REQUIRE(aligned4(phat) && aligned4(dq) && aligned4(msg1_recv), "misaligned pointer");
  LgWeights W = {};
  for (int e = 0; e < n_edges; ++e) {
    CHOCO_REQUIRE(std::isfinite((float)weights[e]), "weight %d is not finite as an fp32 value", e);
    W.w[e] = (float)weights[e];
    W.c[e] = (lo_mask >> e) & 1u ? -W.w[e] : W.w[e];
  }
  return lg_dispatch(rank, n_edges, [&](auto ES, auto R) {
    return CHOCO_LAUNCH("lowrank_gossip_apply_kernel", "lowrank_gossip_apply_kernel", (lowrank_gossip_apply_kernel<ES, R>),
                        dim3((unsigned)plan_host[kLrNRow]), dim3(kLrThreads), as_stream(stream), x, phat, dq, msg1_recv, W,
                        n_edges, plan_dev);
  });
}
