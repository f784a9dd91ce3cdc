// Cholesky-QR orthogonalisation of PowerSGD's summed P at ranks 8, 16 and 32, on v_mfma_f64_16x16x4_f64
// (include/choco_codec.h, choco_lowrank_orthogonalize_cholqr).  The thin QR
// factorisation with a positive diagonal is unique, so this computes what lowrank_orth_kernel's modified
// Gram-Schmidt computes, in three launches whose work is parallel over every 256-row block of every matrix
// instead of 3 R dependent passes on one workgroup a matrix:
//     gram       G = P^T P per (matrix, block of kLrSlab rows), fp64, one partial per block
//     chol       the partials in ascending block order, G = L L^T with the pivot rule, T = L^-T D
//     orthapply  P^ = P T in fp64, each element rounded to fp32 once, in place
// All arithmetic is fp64 (P's fp32 words widen exactly; the one narrowing is the final store), so the file
// has no fp32 arithmetic for the packed fp32 instructions to touch.
//
// The instruction, lane l of the wave:  A[i = l % 16][k = l / 16],  B[k = l / 16][j = l % 16], four
// results v: D[i = 4 v + l / 16][j = l % 16] (the fp64 instruction interleaves its result rows; the fp32
// one of lowrank_mfma.hip holds four consecutive rows).  k is summed inside, so any assignment of the real
// reduction index to (step, k) is valid as long as A and B use the same one.
//
// A workgroup finds its (matrix, block) with no search: the grid is (the most blocks of any matrix) x
// (matrices) and a surplus workgroup exits at once.  Block b of matrix m owns the workspace slot
// poff / (kLrSlab R) + m + b: poff is the R-fold sum of the earlier matrices' rows, so the slots of
// successive matrices cannot overlap (floor(rows / 256) + 1 >= the matrix's blocks) and there are at most
// p_total / (kLrSlab R) + ncomp of them.  T of matrix m follows the slots, R x R row-major.
// No atomics: every sum's order is fixed by the table and the rank.
#include "lowrank.h"

#include <cmath>

namespace choco {

typedef double lr_f64x4 __attribute__((ext_vector_type(4)));
CHOCO_DEV lr_f64x4 lr_dmfma(double a, double b, lr_f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

constexpr double kLrPivotTau = 0x1p-30;  // a pivot at or under tau G_kk drops its column
constexpr double kLrOrthEps = 1e-8;      // Gram-Schmidt's col /= ||col|| + 1e-8

static int64_t lr_cq_slots(const int64_t* plan_host) {
  return plan_host[kLrPTotal] / (kLrSlab * plan_host[kLrRank]) + plan_host[kLrNcomp];
}
CHOCO_DEV int64_t lr_cq_slot(const LrMat& M, int64_t m, int R) { return M.poff / (kLrSlab * R) + m; }

// ---------------------------------------------------------------- gram
// A wave takes 64 of the block's rows in sixteen k steps of four rows: lane (i, kq) loads
// P[row0 + 4 s + kq][16 c + i], at R = 16 one 256-byte segment a step, and that word is both A and B of a
// diagonal tile.  R = 32 runs tiles (0, 0), (0, 1), (1, 1); R = 8 one tile whose upper eight columns are
// fed zeros.  The waves are joined through LDS in wave order.
template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_gram_kernel(const float* __restrict__ msg1, double* __restrict__ ws,
                                                                  const int64_t* __restrict__ plan) {
  constexpr int NC = R > 16 ? 2 : 1, NTL = NC * (NC + 1) / 2, KS = 64 / 4;
  __shared__ double red[kLrWaves][NTL][kLrTile * kLrTile];
  const int64_t m = blockIdx.y;
  const LrMat M = lr_mat(plan, m);
  if ((int64_t)blockIdx.x >= M.nslab) return;
  const int lane = lane_id(), w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const float* P = msg1 + M.poff;
  const int64_t row0 = (int64_t)blockIdx.x * kLrSlab + 64 * w;
  float a[KS][NC];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int64_t row = row0 + 4 * s + kq;
    const bool ok = row < M.rows && (R >= 16 || i < R);
#pragma unroll
    for (int c = 0; c < NC; ++c) a[s][c] = ok ? P[row * R + 16 * c + i] : 0.0f;
  }
  lr_f64x4 acc[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t) acc[t] = lr_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const double a0 = (double)a[s][0];
    acc[0] = lr_dmfma(a0, a0, acc[0]);
    if constexpr (NC == 2) {
      const double a1 = (double)a[s][1];
      acc[1] = lr_dmfma(a0, a1, acc[1]);
      acc[2] = lr_dmfma(a1, a1, acc[2]);
    }
  }
#pragma unroll
  for (int t = 0; t < NTL; ++t) {
#pragma unroll
    for (int v = 0; v < 4; ++v) red[w][t][(4 * v + kq) * kLrTile + i] = acc[t][v];
  }
  __syncthreads();
  double* out = ws + (lr_cq_slot(M, m, R) + blockIdx.x) * (R * R);
  for (int x = threadIdx.x; x < R * R; x += kLrThreads) {
    const int gi = x / R, gj = x % R, ti = gi >> 4, tj = gj >> 4;
    // the lower tile of R = 32 is the transpose of tile (0, 1)
    const int t = ti + tj, e = ti <= tj ? (gi & 15) * kLrTile + (gj & 15) : (gj & 15) * kLrTile + (gi & 15);
    out[x] = ((red[0][t][e] + red[1][t][e]) + red[2][t][e]) + red[3][t][e];
  }
}

// ---------------------------------------------------------------- chol
// One workgroup a matrix.  G's entries are summed over the blocks coalesced; thread i then owns row i of
// L: column k's pivot d_k = G_kk - sum_{j<k} L_kj^2 is dropped at d_k <= tau G_kk (L_kk = 0, L_ik = 0),
// X = L^-1 by forward substitution (thread c its column c, kept in G's upper triangle; a dropped row is
// zero), and T[k][j] = X[j][k] D_j with D_j = L_jj / (L_jj + 1e-8), upper triangular.
template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_chol_kernel(double* __restrict__ ws, int64_t t_off,
                                                                  const int64_t* __restrict__ plan) {
  constexpr int RS = R + 1;  // the row stride: thread i walks row i, and R doubles apart is one bank
  __shared__ double Gs[R * RS];
  __shared__ double Ld[R];
  const int64_t m = blockIdx.x;
  const LrMat M = lr_mat(plan, m);
  const double* part = ws + lr_cq_slot(M, m, R) * (R * R);
  for (int x = threadIdx.x; x < R * R; x += kLrThreads) {
    double s = part[x];
    for (int64_t b = 1; b < M.nslab; ++b) s += part[b * (R * R) + x];
    Gs[x / R * RS + x % R] = s;
  }
  __syncthreads();
  const int i = threadIdx.x;
  for (int k = 0; k < R; ++k) {
    double s = 0.0;
    if (i >= k && i < R) {
      s = Gs[i * RS + k];
      for (int j = 0; j < k; ++j) s -= Gs[i * RS + j] * Gs[k * RS + j];
    }
    if (i == k) Ld[k] = s <= kLrPivotTau * Gs[k * RS + k] ? 0.0 : sqrt(s);
    __syncthreads();
    if (i > k && i < R) Gs[i * RS + k] = Ld[k] > 0.0 ? s / Ld[k] : 0.0;
    __syncthreads();
  }
  if (i < R) {  // X[r][i], r >= i, into Gs[i][r]: the strictly lower triangle (L) is only read
    for (int r = i; r < R; ++r) {
      double s = r == i ? 1.0 : 0.0;
      for (int j = i; j < r; ++j) s -= Gs[r * RS + j] * Gs[i * RS + j];
      Gs[i * RS + r] = Ld[r] > 0.0 ? s / Ld[r] : 0.0;
    }
  }
  __syncthreads();
  double* T = ws + t_off + m * (R * R);
  for (int x = threadIdx.x; x < R * R; x += kLrThreads) {
    const int k = x / R, j = x % R;
    T[x] = j >= k && Ld[j] > 0.0 ? Gs[k * RS + j] * (Ld[j] / (Ld[j] + kLrOrthEps)) : 0.0;
  }
}

// ---------------------------------------------------------------- orthapply
// gram's items; a wave takes every fourth 16-row tile of the block.  Lane (i, kq) loads KV consecutive
// words of row i from each 16-column group of P -- a tile is one contiguous 64 R bytes, read with 16-byte
// (R = 8: 8-byte) loads -- and component s of group g is the k step whose real index is 16 g + KV kq + s;
// B = T[that k][16 n + j] sits in registers for the whole block.  The tile's rows are read whole before
// the wave's stores (the stores wait for the instructions that consumed every lane's loads).
template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_orthapply_kernel(float* msg1, const double* __restrict__ tmat,
                                                                       const int64_t* __restrict__ plan) {
  constexpr int NT = R > 16 ? 2 : 1, NG = NT, KV = R >= 16 ? 4 : 2;
  typedef float lr_ldv __attribute__((ext_vector_type(KV)));
  const int64_t m = blockIdx.y;
  const LrMat M = lr_mat(plan, m);
  if ((int64_t)blockIdx.x >= M.nslab) return;
  const int lane = lane_id(), w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const double* T = tmat + m * (R * R);
  double b[NG * KV][NT];
#pragma unroll
  for (int gs = 0; gs < NG * KV; ++gs) {
    const int k = 16 * (gs / KV) + KV * kq + gs % KV;
#pragma unroll
    for (int n = 0; n < NT; ++n) b[gs][n] = 16 * n + i < R ? T[k * R + 16 * n + i] : 0.0;
  }
  float* P = msg1 + M.poff;
  for (int t = w; t < kLrSlab / kLrTile; t += kLrWaves) {
    const int64_t r0 = (int64_t)blockIdx.x * kLrSlab + kLrTile * t;
    if (r0 >= M.rows) break;
    lr_ldv a[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      a[g] = lr_ldv(0.0f);
      if (r0 + i < M.rows) a[g] = *reinterpret_cast<const lr_ldv*>(P + (r0 + i) * R + 16 * g + KV * kq);
    }
    lr_f64x4 d[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) d[n] = lr_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int gs = 0; gs < NG * KV; ++gs) {
#pragma unroll
      for (int n = 0; n < NT; ++n) d[n] = lr_dmfma((double)a[gs / KV][gs % KV], b[gs][n], d[n]);
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t row = r0 + 4 * v + kq;
        if (row < M.rows && 16 * n + i < R) P[row * R + 16 * n + i] = (float)d[n][v];
      }
    }
  }
}

}  // namespace choco

using namespace choco;

CHOCO_API size_t choco_lowrank_orth_workspace_size(const int64_t* plan_host) {
  if (!plan_host || plan_host[kLrMagic] != kLrMagicValue || !lr_rank_hi((int32_t)plan_host[kLrRank])) return 0;
  const size_t rr = (size_t)(plan_host[kLrRank] * plan_host[kLrRank]);
  return align_up((size_t)(lr_cq_slots(plan_host) + plan_host[kLrNcomp]) * rr * sizeof(double), 256) + 256;
}

CHOCO_API int choco_lowrank_orthogonalize_cholqr(float* msg1, int64_t msg1_len, void* ws, size_t ws_bytes,
                                                 const int64_t* plan_host, const int64_t* plan_dev, int64_t n,
                                                 int32_t rank, void* stream) {
  CHOCO_TRY(lr_check(plan_host, plan_dev, n, rank, msg1_len, -1));
  CHOCO_REQUIRE(lr_rank_hi(rank), "Cholesky-QR orthogonalisation is built for ranks 8, 16 and 32, got %d (ranks 1, 2 and "
                "4 run choco_lowrank_orthogonalize)", (int)rank);
  CHOCO_REQUIRE(msg1, "null msg1");
  CHOCO_REQUIRE(ws, "null workspace");
  CHOCO_REQUIRE(ws_bytes >= choco_lowrank_orth_workspace_size(plan_host), "workspace too small: %zu bytes, need %zu",
                ws_bytes, choco_lowrank_orth_workspace_size(plan_host));
  CHOCO_REQUIRE(aligned16(msg1) && aligned16(ws), "msg1 and the workspace must be 16-byte aligned");
  const int64_t ncomp = plan_host[kLrNcomp];
  if (ncomp == 0) return CHOCO_OK;
  CHOCO_REQUIRE(ncomp <= 65535, "%lld compressed matrices: more than a grid's 65535 rows", (long long)ncomp);
  int64_t maxslab = 1;
  for (int64_t m = 0; m < ncomp; ++m) {
    const int64_t nslab = plan_host[plan_host[kLrOffMat] + kLrMatRow * m + 5];
    maxslab = nslab > maxslab ? nslab : maxslab;
  }
  const hipStream_t st = as_stream(stream);
  const dim3 items((unsigned)maxslab, (unsigned)ncomp), block(kLrThreads);
  double* wsd = reinterpret_cast<double*>(ws);
  const int64_t t_off = lr_cq_slots(plan_host) * rank * rank;
  return lr_dispatch_hi(rank, [&](auto R) {
    CHOCO_TRY(CHOCO_LAUNCH("lowrank_gram_kernel", "lowrank_gram_kernel", lowrank_gram_kernel<R>, items, block, st,
                           (const float*)msg1, wsd, plan_dev));
    CHOCO_TRY(CHOCO_LAUNCH("lowrank_chol_kernel", "lowrank_chol_kernel", lowrank_chol_kernel<R>, dim3((unsigned)ncomp),
                           block, st, wsd, t_off, plan_dev));
    return CHOCO_LAUNCH("lowrank_orthapply_kernel", "lowrank_orthapply_kernel", lowrank_orthapply_kernel<R>, items, block,
                        st, msg1, (const double*)(wsd + t_off), plan_dev);
  });
}
