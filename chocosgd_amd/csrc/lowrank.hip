// Rank-r PowerSGD (Vogels, Karimireddy, Jaggi, NeurIPS 2019): the four batched kernels between the
// gradient pack and the flat-gradient update (include/choco_codec.h, "low-rank compression").
//
// Every 2-D tensor of the layout whose rank-r factors are smaller than itself is a row-major
// matrix M_t (rows x cols) in place in the flat buffer; the other tensors travel as they are.
//     project        M = g + e (stored over e),  P = M Q            reads g, e, writes e: 12 B / element
//     orthogonalise  modified Gram-Schmidt on the columns of the summed P, fp64 dots
//     back-project   Q = M^T P^                                       reads M: 4 B / element
//     decode         out = P^ Q^T,  e = M - out / W                   reads M, writes out, e: 12 B / element
// The products are 2 r flop per 4 to 12 bytes at r <= 4: memory-bound loops on the vector ALUs,
// no MFMA (a 4 x 4 x 1 MFMA would only re-shape them).
//
// The tile table (choco_lowrank_plan, built once per layout on the host, uploaded once) holds
// header | tensor rows | matrix rows | row items | back-project items | slab-sum items, all
// int64; a workgroup reads its item and its matrix row from it -- no search.
//   * project and decode share the ROW ITEMS: kLrRowCap or fewer whole rows of one matrix, about
//     kLrItemElems elements, or a piece of an uncompressed tensor (copied into / out of message
//     1's tail by the same launch).  The r-column factor (Q) goes through LDS in blocks of
//     kLrColBlock columns, ascending, transposed to r planes so that a lane's four columns are
//     one 16-byte LDS read; a wave owns a row at a time, its lanes stride over the block's
//     columns with 16-byte loads (a scalar head up to the next 16-byte boundary, a scalar tail),
//     r accumulators a lane, a fixed butterfly across the wave, and the blocks' sums are added
//     in ascending order.
//   * back-project reduces down the strided dimension: an item is kLrStrip adjacent columns
//     (one lane each: coalesced row segments) x one slab of kLrSlab rows, the slab's P^ rows in
//     LDS (a broadcast read), the four waves interleaved over the slab's rows and joined in wave
//     order.  A matrix of one slab writes Q itself; otherwise the slab partials go to the
//     workspace and lowrank_slabsum_kernel adds them in ascending slab order.
//   * orthogonalise is one workgroup per matrix, the first kLrOrthStage rows of P in LDS, the rest
//     in place in global memory; a thread keeps to its own rows, so only the fp64 reductions
//     (butterfly, then the waves in order) need barriers.
// No atomics anywhere: every output is a function of the inputs in an order the table fixes.
// The table's layout, its builder and the launch check are in lowrank.h, shared with lowrank_mfma.hip:
// ranks 8, 16 and 32 run project, back-project and decode there on the fp32 matrix instruction, behind
// the entry points below, and orthogonalise here with kLrHiOrthStage staged rows.
#include "lowrank.h"

#include <cmath>

namespace choco {

// a row of up to four columns' factors from the LDS planes: one 16-byte read where j is on the
// 16-byte grid, else four words
template <int R>
CHOCO_DEV void lr_q4(const float* Qs, int j, bool al, float (&q)[R][4]) {
#pragma unroll
  for (int c = 0; c < R; ++c) {
    if (al) {
      const float4 t = *reinterpret_cast<const float4*>(Qs + c * kLrColBlock + j);
      q[c][0] = t.x; q[c][1] = t.y; q[c][2] = t.z; q[c][3] = t.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) q[c][u] = Qs[c * kLrColBlock + j + u];
    }
  }
}

// the workgroup stages columns [cb0, cb0 + nb) of a (cols x R) row-major factor as R planes
template <int R>
CHOCO_DEV void lr_stage(float* Qs, const float* __restrict__ src, int nb) {
  for (int i = threadIdx.x; i < nb * R; i += kLrThreads) Qs[(i % R) * kLrColBlock + i / R] = src[i];
}

// ---------------------------------------------------------------- project
template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_project_kernel(const float* __restrict__ g, float* __restrict__ e,
                                                                     const float* __restrict__ q,
                                                                     float* __restrict__ msg1,
                                                                     const int64_t* __restrict__ plan) {
  __shared__ __attribute__((aligned(16))) float Qs[R * kLrColBlock];
  __shared__ float psum[kLrRowCap * R];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) {  // a piece of an uncompressed tensor: into the message tail
    const int64_t off = it[1], tail = it[3];
    const int cnt = (int)it[2];
    for (int i = threadIdx.x; i < cnt; i += kLrThreads) msg1[tail + i] = g[off + i];
    return;
  }
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t row0 = it[1];
  const int nrows = (int)it[2];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nrows * R; i += kLrThreads) psum[i] = 0.0f;
  for (int64_t cb0 = 0; cb0 < M.cols; cb0 += kLrColBlock) {
    const int nb = (int)(M.cols - cb0 < kLrColBlock ? M.cols - cb0 : kLrColBlock);
    __syncthreads();
    lr_stage<R>(Qs, q + M.qoff + cb0 * R, nb);
    __syncthreads();
    for (int rl = w; rl < nrows; rl += kLrWaves) {
      const int64_t a = M.off + (row0 + rl) * M.cols + cb0;
      const int head0 = (int)((4 - (a & 3)) & 3), head = head0 < nb ? head0 : nb;
      float acc[R];
#pragma unroll
      for (int c = 0; c < R; ++c) acc[c] = 0.0f;
      if (lane < head) {
        const float m = g[a + lane] + e[a + lane];
        e[a + lane] = m;
#pragma unroll
        for (int c = 0; c < R; ++c) acc[c] = fmaf(m, Qs[c * kLrColBlock + lane], acc[c]);
      }
      const int nvec = (nb - head) >> 2;
      const bool al = head == 0;
#pragma unroll 2
      for (int v = lane; v < nvec; v += 64) {
        const int j = head + 4 * v;
        const float4 gv = ld_nt4(g + a + j);
        const float4 ev = *reinterpret_cast<const float4*>(e + a + j);
        const float4 m = make_float4(gv.x + ev.x, gv.y + ev.y, gv.z + ev.z, gv.w + ev.w);
        *reinterpret_cast<float4*>(e + a + j) = m;
        float qq[R][4];
        lr_q4<R>(Qs, j, al, qq);
#pragma unroll
        for (int c = 0; c < R; ++c)
          acc[c] = fmaf(m.w, qq[c][3], fmaf(m.z, qq[c][2], fmaf(m.y, qq[c][1], fmaf(m.x, qq[c][0], acc[c]))));
      }
      const int j0 = head + 4 * nvec;
      if (lane < nb - j0) {
        const float m = g[a + j0 + lane] + e[a + j0 + lane];
        e[a + j0 + lane] = m;
#pragma unroll
        for (int c = 0; c < R; ++c) acc[c] = fmaf(m, Qs[c * kLrColBlock + j0 + lane], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < R; ++c) acc[c] = wave_sum(acc[c]);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < R; ++c) psum[rl * R + c] += acc[c];
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nrows * R; i += kLrThreads) msg1[M.poff + row0 * R + i] = psum[i];
}

// ---------------------------------------------------------------- decode
template <int R>
CHOCO_DEV float lr_dec1(float* __restrict__ e, float* __restrict__ out, int64_t i, const float (&p)[R], const float* Qs,
                        int j, float div) {
  float o = p[0] * Qs[j];
#pragma unroll
  for (int c = 1; c < R; ++c) o = fmaf(p[c], Qs[c * kLrColBlock + j], o);
  out[i] = o;
  const float avg = o / div;
  e[i] = e[i] - avg;
  return o;
}

template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_decode_kernel(float* __restrict__ e,
                                                                    const float* __restrict__ msg1,
                                                                    const float* __restrict__ msg2,
                                                                    float* __restrict__ out, float div,
                                                                    const int64_t* __restrict__ plan) {
  __shared__ __attribute__((aligned(16))) float Qs[R * kLrColBlock];
  __shared__ float Ps[kLrRowCap * R];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) {  // the summed elements of an uncompressed tensor, back from the tail
    const int64_t off = it[1], tail = it[3];
    const int cnt = (int)it[2];
    for (int i = threadIdx.x; i < cnt; i += kLrThreads) out[off + i] = msg1[tail + i];
    return;
  }
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t row0 = it[1];
  const int nrows = (int)it[2];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nrows * R; i += kLrThreads) Ps[i] = msg1[M.poff + row0 * R + i];
  for (int64_t cb0 = 0; cb0 < M.cols; cb0 += kLrColBlock) {
    const int nb = (int)(M.cols - cb0 < kLrColBlock ? M.cols - cb0 : kLrColBlock);
    __syncthreads();
    lr_stage<R>(Qs, msg2 + M.qoff + cb0 * R, nb);
    __syncthreads();
    for (int rl = w; rl < nrows; rl += kLrWaves) {
      const int64_t a = M.off + (row0 + rl) * M.cols + cb0;
      const int head0 = (int)((4 - (a & 3)) & 3), head = head0 < nb ? head0 : nb;
      float p[R];
#pragma unroll
      for (int c = 0; c < R; ++c) p[c] = Ps[rl * R + c];
      if (lane < head) lr_dec1<R>(e, out, a + lane, p, Qs, lane, div);
      const int nvec = (nb - head) >> 2;
      const bool al = head == 0;
#pragma unroll 2
      for (int v = lane; v < nvec; v += 64) {
        const int j = head + 4 * v;
        const float4 m = *reinterpret_cast<const float4*>(e + a + j);
        float qq[R][4], o[4];
        lr_q4<R>(Qs, j, al, qq);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          o[u] = p[0] * qq[0][u];
#pragma unroll
          for (int c = 1; c < R; ++c) o[u] = fmaf(p[c], qq[c][u], o[u]);
        }
        *reinterpret_cast<float4*>(out + a + j) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(e + a + j) =
            make_float4(m.x - o[0] / div, m.y - o[1] / div, m.z - o[2] / div, m.w - o[3] / div);
      }
      const int j0 = head + 4 * nvec;
      if (lane < nb - j0) lr_dec1<R>(e, out, a + j0 + lane, p, Qs, j0 + lane, div);
    }
  }
}

// ---------------------------------------------------------------- back-project
template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_backproject_kernel(const float* __restrict__ Mflat,
                                                                         const float* __restrict__ msg1,
                                                                         float* __restrict__ msg2,
                                                                         float* __restrict__ ws,
                                                                         const int64_t* __restrict__ plan) {
  __shared__ __attribute__((aligned(16))) float Ps[kLrSlab * R];
  __shared__ float red[kLrWaves][kLrStrip][R];
  const int64_t* it = plan + plan[kLrOffBp] + kLrItemRow * (int64_t)blockIdx.x;
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t col0 = it[1], slab = it[2];
  const int64_t row0 = slab * kLrSlab;
  const int nrows = (int)(M.rows - row0 < kLrSlab ? M.rows - row0 : kLrSlab);
  const int lane = lane_id(), w = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nrows * R; i += kLrThreads) Ps[i] = msg1[M.poff + row0 * R + i];
  __syncthreads();
  const int64_t col = col0 + lane;
  const bool active = col < M.cols;
  float acc[R];
#pragma unroll
  for (int c = 0; c < R; ++c) acc[c] = 0.0f;
  if (active) {
    const float* __restrict__ p = Mflat + M.off + row0 * M.cols + col;
#pragma unroll 4
    for (int rl = w; rl < nrows; rl += kLrWaves) {
      const float m = p[rl * M.cols];
#pragma unroll
      for (int c = 0; c < R; ++c) acc[c] = fmaf(m, Ps[rl * R + c], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < R; ++c) red[w][lane][c] = acc[c];
  __syncthreads();
  if (w == 0 && active) {
    float* dst = M.nslab == 1 ? msg2 + M.qoff + col * R : ws + M.wsoff + (slab * M.cols + col) * R;
#pragma unroll
    for (int c = 0; c < R; ++c) dst[c] = ((red[0][lane][c] + red[1][lane][c]) + red[2][lane][c]) + red[3][lane][c];
  }
}

// Q of the matrices of more than one slab: the slab partials in ascending slab order
__global__ __launch_bounds__(kLrThreads) void lowrank_slabsum_kernel(const float* __restrict__ ws,
                                                                     float* __restrict__ msg2,
                                                                     const int64_t* __restrict__ plan) {
  const int64_t* it = plan + plan[kLrOffSum] + kLrItemRow * (int64_t)blockIdx.x;
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t ne = M.cols * plan[kLrRank], i = it[1] + threadIdx.x;
  if ((int)threadIdx.x >= (int)it[2]) return;
  float s = ws[M.wsoff + i];
  for (int64_t sl = 1; sl < M.nslab; ++sl) s += ws[M.wsoff + sl * ne + i];
  msg2[M.qoff + i] = s;
}

// ---------------------------------------------------------------- orthogonalise
// the Gram-Schmidt sweep itself (lr_mgs) is in lowrank.h, shared with lowrank_gossip.hip
template <int R, int STAGE = kLrOrthStage>
__global__ __launch_bounds__(kLrThreads) void lowrank_orth_kernel(float* __restrict__ msg1,
                                                                  const int64_t* __restrict__ plan) {
  __shared__ float Ps[STAGE * R];
  __shared__ double red[kLrWaves][R];
  const LrMat M = lr_mat(plan, blockIdx.x);
  float* P = msg1 + M.poff;
  const int ns = (int)(M.rows < STAGE ? M.rows : STAGE);
  for (int i = threadIdx.x; i < ns * R; i += kLrThreads) Ps[i] = P[i];
  __syncthreads();
  lr_mgs<R, STAGE>(P, M.rows, Ps, red);
  __syncthreads();
  for (int i = threadIdx.x; i < ns * R; i += kLrThreads) P[i] = Ps[i];
}

// rank -> the kernel's instance
#define LR_BY_RANK(rank, KERNEL, ...)                                                                             \
  ((rank) == 1 ? CHOCO_LAUNCH(#KERNEL, #KERNEL, KERNEL<1>, __VA_ARGS__)                                           \
               : (rank) == 2 ? CHOCO_LAUNCH(#KERNEL, #KERNEL, KERNEL<2>, __VA_ARGS__)                             \
                             : CHOCO_LAUNCH(#KERNEL, #KERNEL, KERNEL<4>, __VA_ARGS__))
// Diagnostic build only (tools/build_variants.py "lowrank_vector8"): rank 8 on the vector templates,
// whose 64 KB Q stage still fits -- the A/B against the matrix-instruction kernels.
#ifdef CHOCO_LOWRANK_VECTOR8
#define LR_VECTOR8(rank, KERNEL, ...) \
  if ((rank) == 8) return CHOCO_LAUNCH(#KERNEL, #KERNEL, KERNEL<8>, __VA_ARGS__)
#else
#define LR_VECTOR8(rank, KERNEL, ...)
#endif
// orthogonalise is the one kernel both families share: the same structure with fewer staged rows
#define LR_ORTH_HI(rank, ...)                                                                                     \
  ((rank) == 8 ? CHOCO_LAUNCH("lowrank_orth_kernel", "lowrank_orth_kernel", (lowrank_orth_kernel<8, kLrHiOrthStage>), \
                              __VA_ARGS__)                                                                        \
               : (rank) == 16 ? CHOCO_LAUNCH("lowrank_orth_kernel", "lowrank_orth_kernel",                        \
                                             (lowrank_orth_kernel<16, kLrHiOrthStage>), __VA_ARGS__)              \
                              : CHOCO_LAUNCH("lowrank_orth_kernel", "lowrank_orth_kernel",                        \
                                             (lowrank_orth_kernel<32, kLrHiOrthStage>), __VA_ARGS__))

}  // namespace choco

using namespace choco;

CHOCO_API int64_t choco_lowrank_plan_len(const int64_t* rows, const int64_t* lens, int32_t nseg, int32_t rank) {
  return lr_build(rows, lens, nseg, rank, nullptr);
}

CHOCO_API int64_t choco_lowrank_plan(const int64_t* rows, const int64_t* lens, int32_t nseg, int32_t rank,
                                     int64_t* plan) {
  if (!plan) return fail(CHOCO_ERR_INVALID, "null pointer");
  return lr_build(rows, lens, nseg, rank, plan);
}

CHOCO_API size_t choco_lowrank_workspace_size(const int64_t* plan_host) {
  if (!plan_host || plan_host[kLrMagic] != kLrMagicValue) return 0;
  return align_up((size_t)plan_host[kLrWsFloats] * sizeof(float), 256) + 256;
}

CHOCO_API int choco_lowrank_project(const float* g, float* e, const float* q, float* msg1, int64_t msg1_len,
                                    int64_t msg2_len, const int64_t* plan_host, const int64_t* plan_dev, int64_t n,
                                    int32_t rank, void* stream) {
  CHOCO_REQUIRE(g && e && msg1, "null pointer");
  CHOCO_TRY(lr_check(plan_host, plan_dev, n, rank, msg1_len, msg2_len));
  CHOCO_REQUIRE(q || plan_host[kLrMsg2] == 0, "null pointer");
  CHOCO_REQUIRE(aligned16(g) && aligned16(e), "g and e must be 16-byte aligned");
  CHOCO_REQUIRE(aligned4(q) && aligned4(msg1), "q and msg1 must be 4-byte aligned");
  const dim3 grid((unsigned)plan_host[kLrNRow]), block(kLrThreads);
  LR_VECTOR8(rank, lowrank_project_kernel, grid, block, as_stream(stream), g, e, q, msg1, plan_dev);
  if (lr_rank_hi(rank)) return lr_hi_project(rank, grid, as_stream(stream), g, e, q, msg1, plan_dev);
  return LR_BY_RANK(rank, lowrank_project_kernel, grid, block, as_stream(stream), g, e, q, msg1, plan_dev);
}

CHOCO_API int choco_lowrank_orthogonalize(float* msg1, int64_t msg1_len, const int64_t* plan_host,
                                          const int64_t* plan_dev, int64_t n, int32_t rank, void* stream) {
  CHOCO_REQUIRE(msg1, "null pointer");
  CHOCO_TRY(lr_check(plan_host, plan_dev, n, rank, msg1_len, -1));
  CHOCO_REQUIRE(aligned4(msg1), "msg1 must be 4-byte aligned");
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  const dim3 grid((unsigned)plan_host[kLrNcomp]), block(kLrThreads);
  if (lr_rank_hi(rank)) return LR_ORTH_HI(rank, grid, block, as_stream(stream), msg1, plan_dev);
  return LR_BY_RANK(rank, lowrank_orth_kernel, grid, block, as_stream(stream), msg1, plan_dev);
}

CHOCO_API int choco_lowrank_backproject(const float* e, const float* msg1, int64_t msg1_len, float* msg2,
                                        int64_t msg2_len, void* ws, size_t ws_bytes, const int64_t* plan_host,
                                        const int64_t* plan_dev, int64_t n, int32_t rank, void* stream) {
  CHOCO_REQUIRE(e && msg1, "null pointer");
  CHOCO_TRY(lr_check(plan_host, plan_dev, n, rank, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  CHOCO_REQUIRE(msg2 && ws, "null pointer");
  CHOCO_REQUIRE(ws_bytes >= choco_lowrank_workspace_size(plan_host), "workspace too small: %zu bytes, need %zu",
                ws_bytes, choco_lowrank_workspace_size(plan_host));
  CHOCO_REQUIRE(aligned4(e) && aligned4(msg1) && aligned4(msg2) && aligned16(ws), "misaligned pointer");
  const hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)plan_host[kLrNBp]), block(kLrThreads);
  float* wsf = reinterpret_cast<float*>(ws);
#ifdef CHOCO_LOWRANK_VECTOR8
  if (rank == 8)
    CHOCO_TRY(CHOCO_LAUNCH("lowrank_backproject_kernel", "lowrank_backproject_kernel", lowrank_backproject_kernel<8>, grid,
                           block, st, e, msg1, msg2, wsf, plan_dev));
  else
#endif
  if (lr_rank_hi(rank))
    CHOCO_TRY(lr_hi_backproject(rank, grid, st, e, msg1, msg2, wsf, plan_dev));
  else
    CHOCO_TRY(LR_BY_RANK(rank, lowrank_backproject_kernel, grid, block, st, e, msg1, msg2, wsf, plan_dev));
  if (plan_host[kLrNSum] == 0) return CHOCO_OK;
  return CHOCO_LAUNCH("lowrank_slabsum_kernel", "lowrank_slabsum_kernel", lowrank_slabsum_kernel,
                      dim3((unsigned)plan_host[kLrNSum]), block, st, (const float*)wsf, msg2, plan_dev);
}

CHOCO_API int choco_lowrank_decode(float* e, const float* msg1, int64_t msg1_len, const float* msg2, int64_t msg2_len,
                                   float* flat_out, double divisor, const int64_t* plan_host, const int64_t* plan_dev,
                                   int64_t n, int32_t rank, void* stream) {
  CHOCO_REQUIRE(e && msg1 && flat_out, "null pointer");
  CHOCO_TRY(lr_check(plan_host, plan_dev, n, rank, msg1_len, msg2_len));
  CHOCO_REQUIRE(msg2_len >= 0, "message 2 needs its length");
  CHOCO_REQUIRE(msg2 || plan_host[kLrMsg2] == 0, "null pointer");
  CHOCO_REQUIRE(divisor > 0.0 && std::isfinite((float)divisor) && (float)divisor > 0.0f,
                "divisor must be positive and finite as an fp32 value, got %g", divisor);
  CHOCO_REQUIRE(aligned16(e) && aligned16(flat_out), "e and flat_out must be 16-byte aligned");
  CHOCO_REQUIRE(aligned4(msg1) && aligned4(msg2), "msg1 and msg2 must be 4-byte aligned");
  const dim3 grid((unsigned)plan_host[kLrNRow]), block(kLrThreads);
  LR_VECTOR8(rank, lowrank_decode_kernel, grid, block, as_stream(stream), e, msg1, msg2, flat_out, (float)divisor, plan_dev);
  if (lr_rank_hi(rank))
    return lr_hi_decode(rank, grid, as_stream(stream), e, msg1, msg2, flat_out, (float)divisor, plan_dev);
  return LR_BY_RANK(rank, lowrank_decode_kernel, grid, block, as_stream(stream), e, msg1, msg2, flat_out,
                    (float)divisor, plan_dev);
}
