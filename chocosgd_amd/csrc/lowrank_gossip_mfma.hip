// PowerGossip beyond E r = 8: the wide family, project, back-project and apply batched over a worker's E
// edges on v_mfma_f32_16x16x4_f32 (include/choco_codec.h, "low-rank gossip, wide").
//
// A worker's E thin factors Q_e (cols x r) are one concatenated cols x K factor, K = E r, and its P^_e one
// rows x K factor: column k = e r + c belongs to edge e = k / r.  K is padded to KW = 16 (K <= 16) or 32; a
// padded column is fed zeros and never stored (lowrank_mfma.hip's rank-8 instance does the same to the upper
// half of its tile).  Any rank of the list with E r <= 32 fits; what lowrank_gossip.hip serves (r <= 4 and
// E r <= 8) stays there.  Templated on KW alone: E and r are run-time values that only the staging and the
// stores see, the tile loops are lowrank_mfma.hip's with KW for the rank.
//     project        P_e = X Q_e for every e                    reads X:            4 B / element
//     back-project   Q'_e = X^T P^_e for every e                reads X:            4 B / element
//     apply          X += sum_e c_e P^_e dQ_e^T                 reads and writes X: 8 B / element
// whatever E is, against 2 KW flop per element.  The kernels read codec.LowRankPlan's table at rank r
// unchanged: a row item at r <= 4 is not whole 16-row tiles, so an item is ceil(nrows / 16) tiles, the last
// one guarded.  Per-edge buffers keep lowrank_gossip.hip's edge-major layout: [E][msg1_len], [E][msg2_len],
// [E][P_total], and E slab workspaces plan[kLrWsFloats] apart.
//   * project: the column blocks of all E factors in LDS as kLrHiColBlock rows of KW + 4 words, a 16-row x KW
//     accumulator tile in registers across all columns, the four waves interleaved over 64-column chunks and
//     joined through LDS in wave order; result column e r + c goes to msg1[e] at rank r.
//   * back-project: lowrank_mfma.hip's item (64 columns x one 256-row slab), the slab's P^ rows of all edges in
//     LDS as [row][KW] with the bank-spreading stride, four result tiles a 16-byte load, the waves joined in
//     wave order; then lowrank_slabsum_kernel on a grid of (items, E).
//   * apply: decode's transposed tile, D'[col][row] = sum_k dQ[col][k] B[row][k] with B[row][e r + c] =
//     c_e P^_e[row][c] formed once per row tile (one fp32 multiply); a lane's four results are four
//     consecutive columns of one row: one 16-byte load and one 16-byte store of X, x = x + d.  The
//     accumulator starts at zero and the two ends of an edge feed exactly negated B (c_e = -w_e at the low end,
//     +w_e at the high end), so their updates d are exact negations.  Tail items mix the uncompressed tensors
//     plainly, in lowrank_gossip_apply_kernel's op order, for up to 32 edges.
// Every kernel has the 16-byte and the guarded scalar instantiation, chosen per matrix (lr_rows_aligned).
// orthogonalise and diff are per (matrix, edge) at rank r and do not depend on the width: lowrank_gossip.hip's
// kernels on a grid of (matrices, E) (lg_orth, lg_diff).
// No atomics: every sum's order is fixed by the table, E and r, the same bits every call.
#include "lowrank.h"

#include <cmath>

namespace choco {

constexpr int kLwMaxK = 32;      // E r served; also the most edges (lo_mask is 32 bits)
constexpr int kLwNarrowK = 8;    // up to here, at r <= 4, lowrank_gossip.hip serves

template <int KW>
struct LwTile {
  static constexpr int NT = KW / 16;               // 16-wide result tiles along K
  static constexpr int QS = KW + 4;                // LDS row stride of Q / dQ: the lanes of a read on 64 banks
  static constexpr int PS = KW == 32 ? 48 : KW;    // LDS row stride of P^ in back-project
};

// E edges at rank r = 1 << rs; K = E r.  Column k of the concatenated factor: edge k >> rs, column k & (r - 1).
struct LwEdges {
  int E, rs;
};

// the signed weights of apply's matrix items (c) and the plain ones of its tail items (w)
struct LwWeights {
  float c[kLwMaxK], w[kLwMaxK];
};

// the workgroup stages columns [cb0, cb0 + nb) of every edge's (cols x r) row-major factor at `src + e * stride`
// as kLrHiColBlock rows of QS words, row c = [edge 0's r columns | edge 1's | .. | zeros up to KW]; the rows
// past nb are zeros (a zero of X times them must stay zero)
template <int KW>
CHOCO_DEV void lw_stage_q(float* Qs, const float* __restrict__ src, int64_t stride, LwEdges G, int nb) {
  const int r = 1 << G.rs, K = G.E << G.rs;
  for (int i = threadIdx.x; i < kLrHiColBlock * KW; i += kLrThreads) {
    const int c = i / KW, k = i % KW;
    Qs[c * LwTile<KW>::QS + k] = (c < nb && k < K) ? src[(k >> G.rs) * stride + c * r + (k & (r - 1))] : 0.0f;
  }
}

// ---------------------------------------------------------------- project
// lowrank_mfma.hip's project tile on the concatenated factor: lane (i, kq) loads row i's 16-byte groups at
// columns c0 + 16 t + 4 kq, sixteen k steps a 64-column chunk, B = Q[col][k] from LDS.
template <int KW, bool AL>
CHOCO_DEV void lw_project_item(const float* __restrict__ x, const float* __restrict__ q, float* __restrict__ msg1,
                               LwEdges G, int64_t m1, int64_t m2, const LrMat& M, int64_t row0, int nrows, float* Qs,
                               float* red) {
  constexpr int NT = LwTile<KW>::NT, QS = LwTile<KW>::QS;
  const int lane = lane_id(), w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const int r = 1 << G.rs, K = G.E << G.rs;
  const int ntile = (nrows + kLrTile - 1) / kLrTile;
  const bool one_block = M.cols <= kLrHiColBlock;
  for (int t = 0; t < ntile; ++t) {
    const int rl = kLrTile * t + i;
    const bool row_ok = rl < nrows;
    const int64_t a0 = M.off + (row0 + rl) * M.cols;
    lr_f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = lr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t cb0 = 0; cb0 < M.cols; cb0 += kLrHiColBlock) {
      const int nb = (int)(M.cols - cb0 < kLrHiColBlock ? M.cols - cb0 : kLrHiColBlock);
      if (t == 0 || !one_block) {  // a matrix of one block stages Q once for all its tiles
        __syncthreads();
        lw_stage_q<KW>(Qs, q + M.qoff + cb0 * r, m2, G, nb);
        __syncthreads();
      }
      const int nch = (nb + 63) >> 6;
      for (int ch = w; ch < nch; ch += kLrWaves) {
        const int cl = 64 * ch + 4 * kq;
        float4 m[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const int64_t col = cb0 + cl + 16 * tt;
          m[tt] = lr_ld4<AL, false>(x + a0 + col, lr_nv(row_ok, M.cols, col));
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float* qr = Qs + (cl + 16 * tt + u) * QS + i;
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = lr_mfma(lr_comp(m[tt], u), qr[16 * n], acc[n]);
          }
        }
      }
    }
    __syncthreads();  // the last tile's sums have been read
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int v = 0; v < 4; ++v) red[(w * kLrTile + 4 * kq + v) * KW + 16 * n + i] = acc[n][v];
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kLrTile * KW; s += kLrThreads) {
      const int ri = s / KW, k = s % KW;
      if (kLrTile * t + ri < nrows && k < K)
        msg1[(k >> G.rs) * m1 + M.poff + (row0 + kLrTile * t + ri) * r + (k & (r - 1))] =
            ((red[s] + red[kLrTile * KW + s]) + red[2 * kLrTile * KW + s]) + red[3 * kLrTile * KW + s];
    }
  }
}

template <int KW>
__global__ __launch_bounds__(kLrThreads) void lowrank_gossip_project_mfma_kernel(const float* __restrict__ x,
                                                                                 const float* __restrict__ q,
                                                                                 float* __restrict__ msg1, LwEdges G,
                                                                                 const int64_t* __restrict__ plan) {
  __shared__ float Qs[kLrHiColBlock * LwTile<KW>::QS];
  __shared__ float red[kLrWaves * kLrTile * KW];
  const int64_t m1 = plan[kLrMsg1], m2 = plan[kLrMsg2];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) {  // a piece of an uncompressed tensor: into every edge's message tail
    const int64_t off = it[1], tail = it[3];
    const int cnt = (int)it[2];
    for (int i = threadIdx.x; i < cnt; i += kLrThreads) {
      const float v = x[off + i];
      for (int e = 0; e < G.E; ++e) msg1[e * m1 + tail + i] = v;
    }
    return;
  }
  const LrMat M = lr_mat(plan, it[0]);
  if (lr_rows_aligned(x, M))
    lw_project_item<KW, true>(x, q, msg1, G, m1, m2, M, it[1], (int)it[2], Qs, red);
  else
    lw_project_item<KW, false>(x, q, msg1, G, m1, m2, M, it[1], (int)it[2], Qs, red);
}

// ---------------------------------------------------------------- back-project
// lowrank_mfma.hip's item on the concatenated P^: lane (i, kq) loads the group at row 4 s + kq, columns
// col0 + 4 i .. + 4; component u feeds result tile u, whose 16 "rows" are the columns col0 + 4 i + u, and the
// four MFMAs of a load share B = P^[row][k] from LDS.
template <int KW, bool AL>
CHOCO_DEV void lw_backproject_item(const float* __restrict__ x, const float* __restrict__ phat, float* __restrict__ msg2,
                                   float* __restrict__ ws, LwEdges G, const int64_t* __restrict__ plan, const LrMat& M,
                                   int64_t col0, int64_t slab, float* smem) {
  constexpr int NT = LwTile<KW>::NT, PS = LwTile<KW>::PS;
  const int lane = lane_id(), w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const int r = 1 << G.rs, K = G.E << G.rs;
  const int64_t row0 = slab * kLrSlab;
  const int nrows = (int)(M.rows - row0 < kLrSlab ? M.rows - row0 : kLrSlab);
  for (int s = threadIdx.x; s < kLrSlab * KW; s += kLrThreads) {
    const int rr = s / KW, k = s % KW;
    smem[rr * PS + k] =
        (rr < nrows && k < K) ? phat[(k >> G.rs) * plan[kLrPTotal] + M.poff + (row0 + rr) * r + (k & (r - 1))] : 0.0f;
  }
  __syncthreads();
  lr_f32x4 acc[4][NT];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[u][n] = lr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const int64_t col = col0 + 4 * i;
  const int nstep = (nrows + 3) >> 2;
  for (int s = w; s < nstep; s += kLrWaves) {
    const int rl = 4 * s + kq;
    const float4 m = lr_ld4<AL, false>(x + M.off + (row0 + rl) * M.cols + col, lr_nv(rl < nrows, M.cols, col));
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const float b = smem[rl * PS + 16 * n + i];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u][n] = lr_mfma(lr_comp(m, u), b, acc[u][n]);
    }
  }
  __syncthreads();  // P^ has been read: its LDS takes the waves' partial tiles, [wave][column][k]
#pragma unroll
  for (int u = 0; u < 4; ++u) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int v = 0; v < 4; ++v) smem[(w * kLrStrip + 4 * (4 * kq + v) + u) * KW + 16 * n + i] = acc[u][n][v];
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kLrStrip * KW; s += kLrThreads) {
    const int c = s / KW, k = s % KW;
    if (col0 + c >= M.cols || k >= K) continue;
    const int e = k >> G.rs;
    float* dst = M.nslab == 1 ? msg2 + e * plan[kLrMsg2] + M.qoff + (col0 + c) * r
                              : ws + e * plan[kLrWsFloats] + M.wsoff + (slab * M.cols + col0 + c) * r;
    dst[k & (r - 1)] = ((smem[s] + smem[kLrStrip * KW + s]) + smem[2 * kLrStrip * KW + s]) + smem[3 * kLrStrip * KW + s];
  }
}

template <int KW>
__global__ __launch_bounds__(kLrThreads) void lowrank_gossip_backproject_mfma_kernel(const float* __restrict__ x,
                                                                                     const float* __restrict__ phat,
                                                                                     float* __restrict__ msg2,
                                                                                     float* __restrict__ ws, LwEdges G,
                                                                                     const int64_t* __restrict__ plan) {
  constexpr int kP = kLrSlab * LwTile<KW>::PS, kRed = kLrWaves * kLrStrip * KW;
  __shared__ float smem[kP > kRed ? kP : kRed];
  const int64_t* it = plan + plan[kLrOffBp] + kLrItemRow * (int64_t)blockIdx.x;
  const LrMat M = lr_mat(plan, it[0]);
  if (lr_rows_aligned(x, M))
    lw_backproject_item<KW, true>(x, phat, msg2, ws, G, plan, M, it[1], it[2], smem);
  else
    lw_backproject_item<KW, false>(x, phat, msg2, ws, G, plan, M, it[1], it[2], smem);
}

// ---------------------------------------------------------------- apply
// decode's transposed tile: A = dQ[col][k] from LDS, B = c_e P^_e[row = l % 16][k] in KW / 4 registers for the
// row tile, four column tiles back to back.
template <int KW, bool AL>
CHOCO_DEV void lw_apply_item(float* __restrict__ x, const float* __restrict__ phat, const float* __restrict__ dq,
                             const LwWeights& W, LwEdges G, const int64_t* __restrict__ plan, const LrMat& M,
                             int64_t row0, int nrows, float* Qs) {
  constexpr int QS = LwTile<KW>::QS, KS = KW / 4;
  const int lane = lane_id(), w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const int r = 1 << G.rs, K = G.E << G.rs;
  const int ntile = (nrows + kLrTile - 1) / kLrTile;
  for (int64_t cb0 = 0; cb0 < M.cols; cb0 += kLrHiColBlock) {
    const int nb = (int)(M.cols - cb0 < kLrHiColBlock ? M.cols - cb0 : kLrHiColBlock);
    __syncthreads();
    lw_stage_q<KW>(Qs, dq + M.qoff + cb0 * r, plan[kLrMsg2], G, nb);
    __syncthreads();
    const int nch = (nb + 63) >> 6;
    for (int t = 0; t < ntile; ++t) {
      const int rl = kLrTile * t + i;
      const bool row_ok = rl < nrows;
      const int64_t a0 = M.off + (row0 + rl) * M.cols;
      float b[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = 4 * s + kq, e = k >> G.rs;
        b[s] = (row_ok && k < K) ? W.c[e] * phat[e * plan[kLrPTotal] + M.poff + (row0 + rl) * r + (k & (r - 1))] : 0.0f;
      }
      for (int ch = w; ch < nch; ch += kLrWaves) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float* qr = Qs + (64 * ch + 16 * ct + i) * QS + kq;
          lr_f32x4 d = lr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int s = 0; s < KS; ++s) d = lr_mfma(qr[4 * s], b[s], d);
          const int64_t col = cb0 + 64 * ch + 16 * ct + 4 * kq;
          const int nv = lr_nv(row_ok, M.cols, col);
          const float4 m = lr_ld4<AL, false>(x + a0 + col, nv);
          lr_st4<AL>(x + a0 + col, nv, make_float4(m.x + d[0], m.y + d[1], m.z + d[2], m.w + d[3]));
        }
      }
    }
  }
}

template <int KW>
__global__ __launch_bounds__(kLrThreads) void lowrank_gossip_apply_mfma_kernel(float* __restrict__ x,
                                                                               const float* __restrict__ phat,
                                                                               const float* __restrict__ dq,
                                                                               const float* __restrict__ recv1,
                                                                               LwWeights W, LwEdges G,
                                                                               const int64_t* __restrict__ plan) {
  __shared__ float Qs[kLrHiColBlock * LwTile<KW>::QS];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) {  // an uncompressed tensor: x + sum_e w_e (x_received,e - x) from the received tails
    const int64_t off = it[1], tail = it[3], m1 = plan[kLrMsg1];
    const int cnt = (int)it[2];
    for (int i = threadIdx.x; i < cnt; i += kLrThreads) {
      const float xv = x[off + i];
      float u = W.w[0] * (recv1[tail + i] - xv);
      for (int e = 1; e < G.E; ++e) u = u + W.w[e] * (recv1[e * m1 + tail + i] - xv);
      x[off + i] = xv + u;
    }
    return;
  }
  const LrMat M = lr_mat(plan, it[0]);
  if (lr_rows_aligned(x, M))
    lw_apply_item<KW, true>(x, phat, dq, W, G, plan, M, it[1], (int)it[2], Qs);
  else
    lw_apply_item<KW, false>(x, phat, dq, W, G, plan, M, it[1], (int)it[2], Qs);
}

// ---------------------------------------------------------------- launches
static LwEdges lw_edges(int32_t rank, int32_t n_edges) {
  int rs = 0;
  while ((1 << rs) < rank) ++rs;
  return LwEdges{n_edges, rs};
}

// E r -> the kernel's instance, f(int_c<KW>)
template <typename F>
int lw_dispatch(int32_t rank, int32_t n_edges, F&& f) {
  return dispatch_list<16, 32>(n_edges * rank <= 16 ? 16 : 32, "padded width", f);
}

// what every wide launch checks first: lr_check, then the range this family serves
static int lw_check(const int64_t* plan_host, const void* plan_dev, int64_t n, int32_t rank, int32_t n_edges,
                    int64_t msg1_len, int64_t msg2_len) {
  CHOCO_TRY(lr_check(plan_host, plan_dev, n, rank, msg1_len, msg2_len));
  const int64_t K = (int64_t)n_edges * rank;
  CHOCO_REQUIRE(n_edges >= 1 && K <= kLwMaxK && (K > kLwNarrowK || rank >= 8),
                "n_edges must be at least 1 and n_edges * rank in (%d, %d], or in [8, %d] at rank 8 and up; got %d edges "
                "at rank %d",
                kLwNarrowK, kLwMaxK, kLwMaxK, (int)n_edges, (int)rank);
  return CHOCO_OK;
}

}  // namespace choco

using namespace choco;

CHOCO_API size_t choco_lowrank_gossip_wide_workspace_size(const int64_t* plan_host, int32_t n_edges) {
  if (!plan_host || plan_host[kLrMagic] != kLrMagicValue || n_edges < 1 || n_edges > kLwMaxK) return 0;
  return align_up((size_t)n_edges * (size_t)plan_host[kLrWsFloats] * sizeof(float), 256) + 256;
}

CHOCO_API int choco_lowrank_gossip_wide_project(const float* x, const float* q, float* msg1, int64_t msg1_len,
                                                int64_t msg2_len, const int64_t* plan_host, const int64_t* plan_dev,
                                                int64_t n, int32_t rank, int32_t n_edges, void* stream) {
  CHOCO_REQUIRE(x && msg1, "null pointer");
  CHOCO_TRY(lw_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  CHOCO_REQUIRE(q || plan_host[kLrMsg2] == 0, "null pointer");
  CHOCO_REQUIRE(aligned16(x), "x must be 16-byte aligned");
  CHOCO_REQUIRE(aligned4(q) && aligned4(msg1), "q and msg1 must be 4-byte aligned");
  return lw_dispatch(rank, n_edges, [&](auto KW) {
    return CHOCO_LAUNCH("lowrank_gossip_project_mfma_kernel", "lowrank_gossip_project_mfma_kernel",
                        lowrank_gossip_project_mfma_kernel<KW>, dim3((unsigned)plan_host[kLrNRow]), dim3(kLrThreads),
                        as_stream(stream), x, q, msg1, lw_edges(rank, n_edges), plan_dev);
  });
}

CHOCO_API int choco_lowrank_gossip_wide_orthogonalize(const float* msg1_own, const float* msg1_recv, int64_t msg1_len,
                                                      float* phat, uint32_t lo_mask, const int64_t* plan_host,
                                                      const int64_t* plan_dev, int64_t n, int32_t rank,
                                                      int32_t n_edges, void* stream) {
  CHOCO_REQUIRE(msg1_own && msg1_recv, "null pointer");
  CHOCO_TRY(lw_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, -1));
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  CHOCO_REQUIRE(phat, "null pointer");
  CHOCO_REQUIRE(aligned4(msg1_own) && aligned4(msg1_recv) && aligned4(phat), "misaligned pointer");
  return lg_orth(rank, dim3((unsigned)plan_host[kLrNcomp], (unsigned)n_edges), as_stream(stream), msg1_own, msg1_recv,
                 phat, lo_mask, plan_dev);
}

CHOCO_API int choco_lowrank_gossip_wide_backproject(const float* x, const float* phat, int64_t msg1_len, float* msg2,
                                                    int64_t msg2_len, void* ws, size_t ws_bytes,
                                                    const int64_t* plan_host, const int64_t* plan_dev, int64_t n,
                                                    int32_t rank, int32_t n_edges, void* stream) {
  CHOCO_REQUIRE(x, "null pointer");
  CHOCO_TRY(lw_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  CHOCO_REQUIRE(phat && msg2 && ws, "null pointer");
  CHOCO_REQUIRE(ws_bytes >= choco_lowrank_gossip_wide_workspace_size(plan_host, n_edges),
                "workspace too small: %zu bytes, need %zu", ws_bytes,
                choco_lowrank_gossip_wide_workspace_size(plan_host, n_edges));
  CHOCO_REQUIRE(aligned4(x) && aligned4(phat) && aligned4(msg2) && aligned16(ws), "misaligned pointer");
  const hipStream_t st = as_stream(stream);
  float* wsf = reinterpret_cast<float*>(ws);
  CHOCO_TRY(lw_dispatch(rank, n_edges, [&](auto KW) {
    return CHOCO_LAUNCH("lowrank_gossip_backproject_mfma_kernel", "lowrank_gossip_backproject_mfma_kernel",
                        lowrank_gossip_backproject_mfma_kernel<KW>, dim3((unsigned)plan_host[kLrNBp]), dim3(kLrThreads),
                        st, x, phat, msg2, wsf, lw_edges(rank, n_edges), plan_dev);
  }));
  if (plan_host[kLrNSum] == 0) return CHOCO_OK;
  return CHOCO_LAUNCH("lowrank_gossip_slabsum_kernel", "lowrank_gossip_slabsum_kernel", lowrank_slabsum_kernel,
                      dim3((unsigned)plan_host[kLrNSum], (unsigned)n_edges), dim3(kLrThreads), st, (const float*)wsf,
                      msg2, plan_dev);
}

CHOCO_API int choco_lowrank_gossip_wide_diff(const float* msg2_own, const float* msg2_recv, int64_t msg1_len,
                                             int64_t msg2_len, float* q, float* dq, uint32_t lo_mask,
                                             const int64_t* plan_host, const int64_t* plan_dev, int64_t n, int32_t rank,
                                             int32_t n_edges, void* stream) {
  CHOCO_TRY(lw_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  CHOCO_REQUIRE(msg2_own && msg2_recv && q && dq, "null pointer");
  CHOCO_REQUIRE(aligned4(msg2_own) && aligned4(msg2_recv) && aligned4(q) && aligned4(dq), "misaligned pointer");
  return lg_diff(rank, dim3((unsigned)plan_host[kLrNcomp], (unsigned)n_edges), as_stream(stream), msg2_own, msg2_recv, q,
                 dq, lo_mask, plan_dev);
}

CHOCO_API int choco_lowrank_gossip_wide_apply(float* x, const float* phat, const float* dq, const float* msg1_recv,
                                              int64_t msg1_len, int64_t msg2_len, const double* weights,
                                              uint32_t lo_mask, const int64_t* plan_host, const int64_t* plan_dev,
                                              int64_t n, int32_t rank, int32_t n_edges, void* stream) {
  CHOCO_REQUIRE(x && msg1_recv && weights, "null pointer");
  CHOCO_TRY(lw_check(plan_host, plan_dev, n, rank, n_edges, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  CHOCO_REQUIRE((phat && dq) || plan_host[kLrNcomp] == 0, "null pointer");
  CHOCO_REQUIRE(aligned16(x), "x must be 16-byte aligned");
  CHOCO_REQUIRE(aligned4(phat) && aligned4(dq) && aligned4(msg1_recv), "misaligned pointer");
  LwWeights W = {};
  for (int e = 0; e < n_edges; ++e) {
    CHOCO_REQUIRE(std::isfinite((float)weights[e]), "weight %d is not finite as an fp32 value", e);
    W.w[e] = (float)weights[e];
    W.c[e] = (lo_mask >> e) & 1u ? -W.w[e] : W.w[e];
  }
  return lw_dispatch(rank, n_edges, [&](auto KW) {
    return CHOCO_LAUNCH("lowrank_gossip_apply_mfma_kernel", "lowrank_gossip_apply_mfma_kernel",
                        lowrank_gossip_apply_mfma_kernel<KW>, dim3((unsigned)plan_host[kLrNRow]), dim3(kLrThreads),
                        as_stream(stream), x, phat, dq, msg1_recv, W, lw_edges(rank, n_edges), plan_dev);
  });
}
