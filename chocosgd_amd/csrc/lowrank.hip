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
// The table's layout and the launch check are in lowrank.h, and so is every loop these kernels have in
// common with lowrank_gossip.hip's: the LDS staging, the row walk (lr_row_walk), project's matrix item
// (lr_project_rows), the product chain (lr_chain), the Gram-Schmidt sweep (lr_mgs) and the back-project
// kernel itself; this file keeps what is PowerSGD's own per element.  The slab-sum kernel (which
// lowrank_gossip.hip launches too) and the table's builder are here.  Ranks 8, 16 and 32 run project,
// back-project and decode in lowrank_mfma.hip on the fp32 matrix instruction, behind the entry points
// below, and orthogonalise here with kLrHiOrthStage staged rows.
#include "lowrank.h"

#include <cmath>

namespace choco {

// ---------------------------------------------------------------- project
template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_project_kernel(const float* __restrict__ g, float* __restrict__ e,
                                                                     const float* __restrict__ q,
                                                                     float* __restrict__ msg1,
                                                                     const int64_t* __restrict__ plan) {
  __shared__ __attribute__((aligned(16))) float Qs[R * kLrColBlock];
  __shared__ float psum[kLrRowCap * R];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) return lr_copy_item(msg1, it[3], g, it[1], (int)it[2]);
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t row0 = it[1];
  const int nrows = (int)it[2];
  lr_project_rows<R, R, kLrColBlock>(
      Qs, psum, q, 0, 1, M, row0, nrows,
      [&](int64_t i) LR_INLINE {
        const float m = g[i] + e[i];
        e[i] = m;
        return m;
      },
      [&](int64_t i) LR_INLINE {
        const float4 gv = ld_nt4(g + i);
        const float4 ev = *reinterpret_cast<const float4*>(e + i);
        const float4 m = make_float4(gv.x + ev.x, gv.y + ev.y, gv.z + ev.z, gv.w + ev.w);
        *reinterpret_cast<float4*>(e + i) = m;
        return m;
      });
  for (int i = threadIdx.x; i < nrows * R; i += kLrThreads) msg1[M.poff + row0 * R + i] = psum[i];
}

// ---------------------------------------------------------------- decode
template <int R>
CHOCO_DEV void lr_dec1(float* __restrict__ e, float* __restrict__ out, int64_t i, const float (&p)[R], const float* Qs,
                       int j, float div) {
  const float o = lr_chain<R, kLrColBlock>(p, Qs + j);
  out[i] = o;
  const float avg = o / div;
  e[i] = e[i] - avg;
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
  if (it[0] < 0) return lr_copy_item(out, it[1], msg1, it[3], (int)it[2]);
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t row0 = it[1];
  const int nrows = (int)it[2];
  const int w = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nrows * R; i += kLrThreads) Ps[i] = msg1[M.poff + row0 * R + i];
  for (int64_t cb0 = 0; cb0 < M.cols; cb0 += kLrColBlock) {
    const int nb = (int)(M.cols - cb0 < kLrColBlock ? M.cols - cb0 : kLrColBlock);
    __syncthreads();
    lr_stage<R, kLrColBlock>(Qs, msg2 + M.qoff + cb0 * R, 0, 1, nb);
    __syncthreads();
    for (int rl = w; rl < nrows; rl += kLrWaves) {
      float p[R];
#pragma unroll
      for (int c = 0; c < R; ++c) p[c] = Ps[rl * R + c];
      lr_row_walk(
          M.off + (row0 + rl) * M.cols + cb0, nb,
          [&](int64_t i, int j) LR_INLINE { lr_dec1<R>(e, out, i, p, Qs, j, div); },
          [&](int64_t i, int j, bool al) LR_INLINE {
            const float4 m = *reinterpret_cast<const float4*>(e + i);
            float qq[R][4], o[4];
            lr_q4<R, kLrColBlock>(Qs, j, al, qq);
#pragma unroll
            for (int u = 0; u < 4; ++u) o[u] = lr_chain<R, 4>(p, &qq[0][u]);
            *reinterpret_cast<float4*>(out + i) = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<float4*>(e + i) =
                make_float4(m.x - o[0] / div, m.y - o[1] / div, m.z - o[2] / div, m.w - o[3] / div);
          });
    }
  }
}

// ---------------------------------------------------------------- slab-sum
// Q of the matrices of more than one slab, per edge (blockIdx.y; PowerSGD: one): the slab partials in
// ascending slab order
__global__ __launch_bounds__(kLrThreads) void lowrank_slabsum_kernel(const float* __restrict__ ws,
                                                                     float* __restrict__ msg2,
                                                                     const int64_t* __restrict__ plan) {
  const int64_t* it = plan + plan[kLrOffSum] + kLrItemRow * (int64_t)blockIdx.x;
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t ne = M.cols * plan[kLrRank], i = it[1] + threadIdx.x;
  if ((int)threadIdx.x >= (int)it[2]) return;
  const float* __restrict__ src = ws + blockIdx.y * plan[kLrWsFloats] + M.wsoff;
  float s = src[i];
  for (int64_t sl = 1; sl < M.nslab; ++sl) s += src[sl * ne + i];
  msg2[blockIdx.y * plan[kLrMsg2] + M.qoff + i] = s;
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

// The ranks whose project, back-project and decode are the vector kernels (the others' are
// lowrank_mfma.hip's), and rank -> the kernel's instance among them.  The diagnostic build
// (tools/build_variants.py "lowrank_vector8") adds rank 8, whose 64 KB Q stage still fits: the A/B against
// the matrix-instruction kernels.
template <int... Rs>
struct LrRanks {
  static bool has(int rank) { return ((rank == Rs) || ...); }
  template <typename F>
  static int dispatch(int rank, F&& f) {
    return dispatch_list<Rs...>(rank, "rank", f);
  }
};
#ifdef CHOCO_LOWRANK_VECTOR8
using LrVector = LrRanks<1, 2, 4, 8>;
#else
using LrVector = LrRanks<1, 2, 4>;
#endif

// ---------------------------------------------------------------- the table (host)
// Counts (plan == nullptr) or writes the table; returns its length, or a negative status.
static int64_t lr_build(const int64_t* rows, const int64_t* lens, int32_t nseg, int32_t rank, int64_t* plan) {
  CHOCO_REQUIRE(rows && lens, "null pointer");
  CHOCO_REQUIRE(nseg >= 1, "nseg must be at least 1");
  CHOCO_REQUIRE(lr_rank_ok(rank), LR_RANKS_TEXT, (int)rank);
  int64_t n = 0;
  for (int32_t t = 0; t < nseg; ++t) {
    CHOCO_REQUIRE(rows[t] >= 0 && lens[t] >= 0, "tensor %d: negative size", (int)t);
    CHOCO_REQUIRE(rows[t] == 0 || lens[t] % rows[t] == 0, "tensor %d: %lld elements are not whole rows of %lld",
                  (int)t, (long long)lens[t], (long long)rows[t]);
    n += lens[t];
    CHOCO_REQUIRE(n < (int64_t)INT32_MAX, "n out of range");
  }
  CHOCO_REQUIRE(n > 0, "n out of range");
  const int64_t R = rank;
  auto compressed = [&](int32_t t) {
    if (rows[t] == 0 || lens[t] == 0) return false;
    const int64_t c = lens[t] / rows[t];
    return rows[t] * c > R * (rows[t] + c);
  };
  auto item_rows = [&](int64_t c) {
    const int64_t want = kLrItemElems / c;
    if (lr_rank_hi(rank)) {  // whole 16-row tiles
      const int64_t tiles = want / kLrTile;
      return tiles < 1 ? (int64_t)kLrTile : tiles * kLrTile > kLrRowCap ? (int64_t)kLrRowCap : tiles * kLrTile;
    }
    return want < kLrWaves ? (int64_t)kLrWaves : want > kLrRowCap ? (int64_t)kLrRowCap : want;
  };
  int64_t ncomp = 0, nrow = 0, nbp = 0, nsum = 0;
  for (int32_t t = 0; t < nseg; ++t) {
    if (!compressed(t)) {
      nrow += (lens[t] + kLrCopyChunk - 1) / kLrCopyChunk;
      continue;
    }
    const int64_t r = rows[t], c = lens[t] / r, nslab = (r + kLrSlab - 1) / kLrSlab;
    ++ncomp;
    nrow += (r + item_rows(c) - 1) / item_rows(c);
    nbp += nslab * ((c + kLrStrip - 1) / kLrStrip);
    if (nslab > 1) nsum += (c * R + kLrThreads - 1) / kLrThreads;
  }
  const int64_t off_tensor = kLrHdrLen, off_mat = off_tensor + 4 * (int64_t)nseg, off_row = off_mat + kLrMatRow * ncomp,
                off_bp = off_row + kLrItemRow * nrow, off_sum = off_bp + kLrItemRow * nbp,
                total = off_sum + kLrItemRow * nsum;
  if (!plan) return total;
  int64_t p_total = 0;
  for (int32_t t = 0; t < nseg; ++t)
    if (compressed(t)) p_total += rows[t] * R;
  int64_t *tr = plan + off_tensor, *mr = plan + off_mat, *ri = plan + off_row, *bi = plan + off_bp, *si = plan + off_sum;
  int64_t off = 0, poff = 0, qoff = 0, tail = p_total, wsoff = 0, m = 0;
  for (int32_t t = 0; t < nseg; ++t, tr += 4) {
    if (!compressed(t)) {
      tr[0] = 0; tr[1] = tail; tr[2] = -1; tr[3] = off;
      for (int64_t o = 0; o < lens[t]; o += kLrCopyChunk, ri += kLrItemRow) {
        ri[0] = -1; ri[1] = off + o; ri[2] = lens[t] - o < kLrCopyChunk ? lens[t] - o : kLrCopyChunk; ri[3] = tail + o;
      }
      tail += lens[t];
      off += lens[t];
      continue;
    }
    const int64_t r = rows[t], c = lens[t] / r, nslab = (r + kLrSlab - 1) / kLrSlab, ir = item_rows(c);
    tr[0] = 1; tr[1] = poff; tr[2] = qoff; tr[3] = off;
    mr[0] = off; mr[1] = r; mr[2] = c; mr[3] = poff; mr[4] = qoff; mr[5] = nslab; mr[6] = nslab > 1 ? wsoff : 0;
    mr[7] = t;
    mr += kLrMatRow;
    for (int64_t r0 = 0; r0 < r; r0 += ir, ri += kLrItemRow) {
      ri[0] = m; ri[1] = r0; ri[2] = r - r0 < ir ? r - r0 : ir; ri[3] = 0;
    }
    for (int64_t sl = 0; sl < nslab; ++sl)
      for (int64_t c0 = 0; c0 < c; c0 += kLrStrip, bi += kLrItemRow) {
        bi[0] = m; bi[1] = c0; bi[2] = sl; bi[3] = 0;
      }
    if (nslab > 1) {
      for (int64_t e0 = 0; e0 < c * R; e0 += kLrThreads, si += kLrItemRow) {
        si[0] = m; si[1] = e0; si[2] = c * R - e0 < kLrThreads ? c * R - e0 : kLrThreads; si[3] = 0;
      }
      wsoff += nslab * c * R;
    }
    poff += r * R;
    qoff += c * R;
    off += lens[t];
    ++m;
  }
  int64_t* h = plan;
  h[kLrMagic] = kLrMagicValue; h[kLrN] = n; h[kLrNseg] = nseg; h[kLrRank] = rank; h[kLrNcomp] = ncomp;
  h[kLrMsg1] = tail; h[kLrMsg2] = qoff; h[kLrPTotal] = p_total; h[kLrNRow] = nrow; h[kLrNBp] = nbp; h[kLrNSum] = nsum;
  h[kLrWsFloats] = wsoff; h[kLrOffMat] = off_mat; h[kLrOffRow] = off_row; h[kLrOffBp] = off_bp; h[kLrOffSum] = off_sum;
  return total;
}

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
  if (!LrVector::has(rank)) return lr_hi_project(rank, grid, as_stream(stream), g, e, q, msg1, plan_dev);
  return LrVector::dispatch(rank, [&](auto R) {
    return CHOCO_LAUNCH("lowrank_project_kernel", "lowrank_project_kernel", lowrank_project_kernel<R>, grid, block,
                        as_stream(stream), g, e, q, msg1, plan_dev);
  });
}

CHOCO_API int choco_lowrank_orthogonalize(float* msg1, int64_t msg1_len, const int64_t* plan_host,
                                          const int64_t* plan_dev, int64_t n, int32_t rank, void* stream) {
  CHOCO_REQUIRE(msg1, "null pointer");
  CHOCO_TRY(lr_check(plan_host, plan_dev, n, rank, msg1_len, -1));
  CHOCO_REQUIRE(aligned4(msg1), "msg1 must be 4-byte aligned");
  if (plan_host[kLrNcomp] == 0) return CHOCO_OK;
  const dim3 grid((unsigned)plan_host[kLrNcomp]), block(kLrThreads);
  // the one kernel every rank shares, with fewer staged rows at ranks 8, 16 and 32
  if (lr_rank_hi(rank))
    return lr_dispatch_hi(rank, [&](auto R) {
      return CHOCO_LAUNCH("lowrank_orth_kernel", "lowrank_orth_kernel", (lowrank_orth_kernel<R, kLrHiOrthStage>), grid,
                          block, as_stream(stream), msg1, plan_dev);
    });
  return lr_dispatch_lo(rank, [&](auto R) {
    return CHOCO_LAUNCH("lowrank_orth_kernel", "lowrank_orth_kernel", lowrank_orth_kernel<R>, grid, block,
                        as_stream(stream), msg1, plan_dev);
  });
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
  if (!LrVector::has(rank))
    CHOCO_TRY(lr_hi_backproject(rank, grid, st, e, msg1, msg2, wsf, plan_dev));
  else  // one edge, whose P^ is the head of message 1
    CHOCO_TRY(LrVector::dispatch(rank, [&](auto R) {
      return CHOCO_LAUNCH("lowrank_backproject_kernel", "lowrank_backproject_kernel", (lowrank_backproject_kernel<1, R>),
                          grid, block, st, e, msg1, msg2, wsf, 1, plan_dev);
    }));
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
  if (!LrVector::has(rank))
    return lr_hi_decode(rank, grid, as_stream(stream), e, msg1, msg2, flat_out, (float)divisor, plan_dev);
  return LrVector::dispatch(rank, [&](auto R) {
    return CHOCO_LAUNCH("lowrank_decode_kernel", "lowrank_decode_kernel", lowrank_decode_kernel<R>, grid, block,
                        as_stream(stream), e, msg1, msg2, flat_out, (float)divisor, plan_dev);
  });
}
