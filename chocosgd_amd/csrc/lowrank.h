// What the low-rank files share.  All of them (lowrank.hip: PowerSGD at ranks 1, 2 and 4 on the vector ALUs;
// lowrank_mfma.hip: ranks 8, 16 and 32 on the fp32 matrix instruction; lowrank_cholqr.hip: Cholesky-QR
// orthogonalisation at ranks 8, 16 and 32; lowrank_gossip.hip: PowerGossip, batched over a worker's edges up to
// E r = 8; lowrank_gossip_mfma.hip: the same up to E r = 32 on the matrix instruction) read one tile table: its layout, the check every launch makes first and the rank lists are here.
// lowrank.hip and lowrank_gossip.hip are one kernel family, and what they have in common stands here once:
// the Gram-Schmidt sweep, the LDS staging, the wave-per-row walk over a column block, project's matrix item,
// the per-element product chain, and the back-project kernel, which both launch (as they do lowrank.hip's
// slab-sum kernel).
#pragma once

#include "choco_common.h"
#include "dispatch.h"

namespace choco {

constexpr int kLrThreads = 256;
constexpr int kLrWaves = kLrThreads / 64;
constexpr int kLrColBlock = 2048;      // columns of the r-column factor staged in LDS at a time
constexpr int kLrRowCap = 256;         // rows of a row item
constexpr int64_t kLrItemElems = 32768;  // elements a row item aims at
constexpr int64_t kLrCopyChunk = 8192;   // elements of an uncompressed tensor per item
constexpr int kLrStrip = 64;           // back-project: columns of an item
constexpr int kLrSlab = 256;           // back-project: rows of an item
constexpr int kLrOrthStage = 2048;     // orthogonalise: rows of P held in LDS
// ranks 8, 16 and 32 (lowrank_mfma.hip): 16 x 16 x 4 fp32 matrix-instruction tiles
constexpr int kLrTile = 16;            // rows of a project / decode tile; a row item is whole tiles
constexpr int kLrHiColBlock = 256;     // columns of Q staged in LDS at a time, in the message's own [col][r] layout
constexpr int kLrHiOrthStage = 256;    // orthogonalise: rows of P held in LDS

// the table's header words
enum LrHdr {
  kLrMagic = 0, kLrN, kLrNseg, kLrRank, kLrNcomp, kLrMsg1, kLrMsg2, kLrPTotal, kLrNRow, kLrNBp, kLrNSum, kLrWsFloats,
  kLrOffMat, kLrOffRow, kLrOffBp, kLrOffSum, kLrHdrLen
};
constexpr int64_t kLrMagicValue = 0x4c52504c414eLL;  // "LRPLAN"
// a matrix row: {flat offset, rows, cols, P offset in message 1, Q offset in message 2, slabs,
// workspace offset, tensor}
constexpr int kLrMatRow = 8;
constexpr int kLrItemRow = 4;

struct LrMat {
  int64_t off, rows, cols, poff, qoff, nslab, wsoff;
};
CHOCO_DEV LrMat lr_mat(const int64_t* __restrict__ plan, int64_t m) {
  const int64_t* r = plan + plan[kLrOffMat] + kLrMatRow * m;
  return LrMat{r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
}

// A row item that is a piece of an uncompressed tensor (it[0] < 0): project copies it into message 1's
// tail, decode copies the summed elements back -- at every rank, so lowrank_mfma.hip calls this too.
CHOCO_DEV void lr_copy_item(float* __restrict__ dst, int64_t doff, const float* __restrict__ src, int64_t soff,
                            int cnt) {
  for (int i = threadIdx.x; i < cnt; i += kLrThreads) dst[doff + i] = src[soff + i];
}

// ---------------------------------------------------------------- orthogonalise (device)
// the sum of K doubles per thread over the workgroup, in every thread: a butterfly in the wave,
// then the waves in order
template <int K>
CHOCO_DEV void lr_block_sum(double (&v)[K], double (*red)[K]) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();  // red is free again
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[w][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// Modified Gram-Schmidt on the columns of one P (rows x R) by one workgroup: rows [0, STAGE) are in
// Ps (LDS, already loaded and barriered), the others in place in P.  Thread t owns rows t, t + 256,
// ...: only the fp64 reductions need barriers.  lowrank_orth_kernel and lowrank_gossip_orth_kernel
// both run exactly this.
template <int R, int STAGE>
CHOCO_DEV void lr_mgs(float* __restrict__ P, int64_t rows, float* Ps, double (*red)[R]) {
  auto at = [&](int64_t i) -> float* { return i < STAGE ? Ps + i * R : P + i * R; };
#pragma unroll
  for (int k = 0; k < R; ++k) {
    double s[1] = {0.0};
    for (int64_t i = threadIdx.x; i < rows; i += kLrThreads) {
      const double v = (double)at(i)[k];
      s[0] += v * v;
    }
    lr_block_sum<1>(s, reinterpret_cast<double(*)[1]>(&red[0][0]));
    const double den = sqrt(s[0]) + 1e-8;
    double dot[R];
#pragma unroll
    for (int l = 0; l < R; ++l) dot[l] = 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += kLrThreads) {
      float* r = at(i);
      const float v = (float)((double)r[k] / den);
      r[k] = v;
#pragma unroll
      for (int l = 0; l < R; ++l)  // l > k as a predicate: dot[] keeps constant indices where k is not unrolled
        if (l > k) dot[l] += (double)v * (double)r[l];
    }
    if (k + 1 < R) {
      lr_block_sum<R>(dot, red);
      for (int64_t i = threadIdx.x; i < rows; i += kLrThreads) {
        float* r = at(i);
#pragma unroll
        for (int l = 0; l < R; ++l)
          if (l > k) r[l] = (float)((double)r[l] - dot[l] * (double)r[k]);
      }
    }
  }
}

// ---------------------------------------------------------------- ranks 1, 2 and 4 (device)
// lowrank.hip and lowrank_gossip.hip: K planes of an r-column factor in LDS, CB columns at a time.  PowerSGD
// has one factor (E = 1, K = R, CB = kLrColBlock); PowerGossip has one per edge (K = ES R, lowrank_gossip.hip).

// up to four columns of all K planes: one 16-byte LDS read a plane where j is on the 16-byte grid, else
// four words
template <int K, int CB>
CHOCO_DEV void lr_q4(const float* Qs, int j, bool al, float (&q)[K][4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (al) {
      const float4 t = *reinterpret_cast<const float4*>(Qs + k * CB + j);
      q[k][0] = t.x; q[k][1] = t.y; q[k][2] = t.z; q[k][3] = t.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) q[k][u] = Qs[k * CB + j + u];
    }
  }
}

// the workgroup stages columns [cb0, cb0 + nb) of every edge's (cols x R) row-major factor at
// `src + e * stride` as planes e R .. e R + R - 1
template <int R, int CB>
CHOCO_DEV void lr_stage(float* Qs, const float* __restrict__ src, int64_t stride, int E, int nb) {
  for (int e = 0; e < E; ++e) {
    const float* __restrict__ s = src + e * stride;
    for (int i = threadIdx.x; i < nb * R; i += kLrThreads) Qs[(e * R + i % R) * CB + i / R] = s[i];
  }
}

// rows [row0, row0 + nrows) of every edge's P^ of matrix M (at `phat + e * stride`) as Ps[row][K]; a padded
// slot's are zeros
template <int ES, int R>
CHOCO_DEV void lr_stage_rows(float* Ps, const float* __restrict__ phat, int64_t stride, const LrMat& M, int64_t row0,
                             int nrows, int E) {
  constexpr int K = ES * R;
  for (int i = threadIdx.x; i < nrows * K; i += kLrThreads) {
    const int rl = i / K, k = i % K, e = k / R;
    Ps[i] = e < E ? phat[e * stride + M.poff + (row0 + rl) * R + k % R] : 0.0f;
  }
}

// A wave walks the nb elements of a row from flat address a on, LDS columns 0 .. nb - 1: a scalar head up to
// the flat buffer's 16-byte grid, 16-byte groups, a scalar tail.  one(flat index, LDS column) takes a single
// element; group(flat index, LDS column, al) takes four on the grid and fetches their K x 4 factors itself,
// lr_q4<K, CB>(Qs, column, al, ..), AFTER it has issued its global load (the LDS reads ahead of the load cost
// PowerGossip's project 6 to 10 %).  The lane that gets an element depends on a and nb alone, which is what
// fixes the order of every sum built on this walk.  The callables are lambdas marked LR_INLINE: inlined with
// the CHOCO_DEV functions around them, before the loops are optimised, as when the walk was written out.
#define LR_INLINE __attribute__((always_inline))
template <typename One, typename Group>
CHOCO_DEV void lr_row_walk(int64_t a, int nb, One one, Group group) {
  const int lane = lane_id();
  const int head0 = (int)((4 - (a & 3)) & 3), head = head0 < nb ? head0 : nb;
  if (lane < head) one(a + lane, lane);
  const int nvec = (nb - head) >> 2;
  const bool al = head == 0;
#pragma unroll 2
  for (int v = lane; v < nvec; v += 64) {
    const int j = head + 4 * v;
    group(a + j, j, al);
  }
  const int j0 = head + 4 * nvec;
  if (lane < nb - j0) one(a + j0 + lane, j0 + lane);
}

// Project's matrix item: psum[row][K] = M Q_e for the item's rows and every edge's Q (at `q + e * stride`).
// The column blocks go through LDS in ascending order; a wave owns a row at a time, K accumulators a lane, a
// fixed butterfly across the wave, and the blocks' sums are added in ascending order.  ld1(flat index) and
// ld4(flat index) give one and four elements of M.  Ends on a barrier: psum is ready to be stored.
template <int R, int K, int CB, typename Ld1, typename Ld4>
CHOCO_DEV void lr_project_rows(float* Qs, float* psum, const float* __restrict__ q, int64_t stride, int E,
                               const LrMat& M, int64_t row0, int nrows, Ld1 ld1, Ld4 ld4) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nrows * K; i += kLrThreads) psum[i] = 0.0f;
  for (int64_t cb0 = 0; cb0 < M.cols; cb0 += CB) {
    const int nb = (int)(M.cols - cb0 < CB ? M.cols - cb0 : CB);
    __syncthreads();
    lr_stage<R, CB>(Qs, q + M.qoff + cb0 * R, stride, E, nb);
    __syncthreads();
    for (int rl = w; rl < nrows; rl += kLrWaves) {
      float acc[K];
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = 0.0f;
      lr_row_walk(
          M.off + (row0 + rl) * M.cols + cb0, nb,
          [&](int64_t i, int j) LR_INLINE {
            const float m = ld1(i);
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = fmaf(m, Qs[k * CB + j], acc[k]);
          },
          [&](int64_t i, int j, bool al) LR_INLINE {
            const float4 m = ld4(i);
            float qq[K][4];
            lr_q4<K, CB>(Qs, j, al, qq);
#pragma unroll
            for (int k = 0; k < K; ++k)
              acc[k] = fmaf(m.w, qq[k][3], fmaf(m.z, qq[k][2], fmaf(m.y, qq[k][1], fmaf(m.x, qq[k][0], acc[k]))));
          });
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) psum[rl * K + k] += acc[k];
      }
    }
  }
  __syncthreads();
}

// One element of P^ Q^T: the product of column 0, then one fmaf per column in ascending order -- the rounding
// order of the contract.  q's columns are QS words apart.
template <int R, int QS = 1>
CHOCO_DEV float lr_chain(const float* p, const float* q) {
  float o = p[0] * q[0];
#pragma unroll
  for (int c = 1; c < R; ++c) o = fmaf(p[c], q[c * QS], o);
  return o;
}

// ---------------------------------------------------------------- back-project (ranks 1, 2 and 4)
// Q_e = M^T P^_e for every edge, down the strided dimension: an item is kLrStrip adjacent columns (one lane
// each: coalesced row segments) x one slab of kLrSlab rows, the slab's P^ rows of all edges in LDS (a
// broadcast read), K = ES R accumulators a lane, the four waves interleaved over the slab's rows and joined in
// wave order through red ([wave][k][lane]: a wave's store has no bank conflict).  A matrix of one slab writes
// Q itself; otherwise the slab partials go to the workspace for lowrank_slabsum_kernel.  The edges' P^, Q and
// workspaces are plan[kLrPTotal], plan[kLrMsg2] and plan[kLrWsFloats] apart; PowerSGD is the one edge whose
// P^ is the head of message 1.
template <int ES, int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_backproject_kernel(const float* __restrict__ x,
                                                                         const float* __restrict__ phat,
                                                                         float* __restrict__ msg2,
                                                                         float* __restrict__ ws, int E,
                                                                         const int64_t* __restrict__ plan) {
  constexpr int K = ES * R;
  __shared__ __attribute__((aligned(16))) float Ps[kLrSlab * K];
  __shared__ float red[kLrWaves][K][kLrStrip];
  const int64_t* it = plan + plan[kLrOffBp] + kLrItemRow * (int64_t)blockIdx.x;
  const LrMat M = lr_mat(plan, it[0]);
  const int64_t col0 = it[1], slab = it[2];
  const int64_t row0 = slab * kLrSlab;
  const int nrows = (int)(M.rows - row0 < kLrSlab ? M.rows - row0 : kLrSlab);
  const int lane = lane_id(), w = threadIdx.x >> 6;
  lr_stage_rows<ES, R>(Ps, phat, plan[kLrPTotal], M, row0, nrows, E);
  __syncthreads();
  const int64_t col = col0 + lane;
  const bool active = col < M.cols;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0f;
  if (active) {
    const float* __restrict__ p = x + M.off + row0 * M.cols + col;
#pragma unroll 4
    for (int rl = w; rl < nrows; rl += kLrWaves) {
      const float m = p[rl * M.cols];
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = fmaf(m, Ps[rl * K + k], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) red[w][k][lane] = acc[k];
  __syncthreads();
  if (w == 0 && active) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = k / R;
      if (e >= E) continue;
      float* dst = M.nslab == 1 ? msg2 + e * plan[kLrMsg2] + M.qoff + col * R
                                : ws + e * plan[kLrWsFloats] + M.wsoff + (slab * M.cols + col) * R;
      dst[k % R] = ((red[0][k][lane] + red[1][k][lane]) + red[2][k][lane]) + red[3][k][lane];
    }
  }
}

// Q of the matrices of more than one slab, per edge (blockIdx.y): the slab partials in ascending slab order.
// Defined in lowrank.hip; lowrank_gossip.hip launches the same kernel with one grid row an edge.
__global__ void lowrank_slabsum_kernel(const float* __restrict__ ws, float* __restrict__ msg2,
                                       const int64_t* __restrict__ plan);

// ---------------------------------------------------------------- matrix-instruction tiles (device)
// lowrank_mfma.hip and lowrank_gossip_mfma.hip: v_mfma_f32_16x16x4_f32 and the 16-byte groups its lanes touch.
typedef float lr_f32x4 __attribute__((ext_vector_type(4)));
CHOCO_DEV lr_f32x4 lr_mfma(float a, float b, lr_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Four consecutive elements at p of which the first nv exist (nv = 0: none, and no access).  AL:
// p is 16-byte aligned and nv is 0 or 4.
template <bool AL, bool NT>
CHOCO_DEV float4 lr_ld4(const float* p, int nv) {
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (AL) {
    if (nv > 0) v = NT ? ld_nt4(p) : *reinterpret_cast<const float4*>(p);
  } else {
    if (nv > 0) v.x = NT ? __builtin_nontemporal_load(p) : p[0];
    if (nv > 1) v.y = NT ? __builtin_nontemporal_load(p + 1) : p[1];
    if (nv > 2) v.z = NT ? __builtin_nontemporal_load(p + 2) : p[2];
    if (nv > 3) v.w = NT ? __builtin_nontemporal_load(p + 3) : p[3];
  }
  return v;
}
template <bool AL>
CHOCO_DEV void lr_st4(float* p, int nv, float4 v) {
  if (AL) {
    if (nv > 0) *reinterpret_cast<float4*>(p) = v;
  } else {
    if (nv > 0) p[0] = v.x;
    if (nv > 1) p[1] = v.y;
    if (nv > 2) p[2] = v.z;
    if (nv > 3) p[3] = v.w;
  }
}
// how many of the four columns from col on exist in a row of `cols`, none for a row that does not
CHOCO_DEV int lr_nv(bool row_ok, int64_t cols, int64_t col) {
  const int64_t left = cols - col;
  return !row_ok || left <= 0 ? 0 : left < 4 ? (int)left : 4;
}
CHOCO_DEV float lr_comp(const float4& v, int u) { return u == 0 ? v.x : u == 1 ? v.y : u == 2 ? v.z : v.w; }

// whether every row of the matrix starts on the 16-byte grid of `base`
CHOCO_DEV bool lr_rows_aligned(const float* base, const LrMat& M) {
  return ((reinterpret_cast<uintptr_t>(base + M.off) & 15u) == 0) && (M.cols & 3) == 0;
}

// ---------------------------------------------------------------- ranks and the launch check (host)
static bool lr_rank_hi(int32_t r) { return r == 8 || r == 16 || r == 32; }
static bool lr_rank_ok(int32_t r) { return r == 1 || r == 2 || r == 4 || lr_rank_hi(r); }
#define LR_RANKS_TEXT "rank must be 1, 2, 4, 8, 16 or 32, got %d"

// rank -> the kernel's instance: f(int_c<rank>) launches it (dispatch.h)
template <typename F>
int lr_dispatch_lo(int rank, F&& f) {
  return dispatch_list<1, 2, 4>(rank, "rank", f);
}
template <typename F>
int lr_dispatch_hi(int rank, F&& f) {
  return dispatch_list<8, 16, 32>(rank, "rank", f);
}

// What every launch checks first, with no HIP call: the host copy of the table against the
// call's n, rank and message lengths (a null or zero length is a message the call does not use).
static int lr_check(const int64_t* plan_host, const void* plan_dev, int64_t n, int32_t rank, int64_t msg1_len,
                    int64_t msg2_len) {
  CHOCO_REQUIRE(plan_host && plan_dev, "null table");
  CHOCO_REQUIRE(lr_rank_ok(rank), LR_RANKS_TEXT, (int)rank);
  CHOCO_REQUIRE(plan_host[kLrMagic] == kLrMagicValue, "plan_host is not a choco_lowrank_plan table");
  CHOCO_REQUIRE(plan_host[kLrN] == n && n > 0 && n < (int64_t)INT32_MAX, "the table was built for n = %lld, got %lld",
                (long long)plan_host[kLrN], (long long)n);
  CHOCO_REQUIRE(plan_host[kLrRank] == rank, "the table was built for rank %lld, got %d", (long long)plan_host[kLrRank],
                (int)rank);
  CHOCO_REQUIRE(msg1_len == plan_host[kLrMsg1], "message 1 holds %lld elements in the table, got %lld",
                (long long)plan_host[kLrMsg1], (long long)msg1_len);
  CHOCO_REQUIRE(msg2_len < 0 || msg2_len == plan_host[kLrMsg2], "message 2 holds %lld elements in the table, got %lld",
                (long long)plan_host[kLrMsg2], (long long)msg2_len);
  CHOCO_REQUIRE(aligned16(plan_dev), "the device table must be 16-byte aligned");
  return CHOCO_OK;
}

// The launches of ranks 8, 16 and 32 (lowrank_mfma.hip), behind the same entry points and checks.
int lr_hi_project(int32_t rank, dim3 grid, hipStream_t st, const float* g, float* e, const float* q, float* msg1,
                  const int64_t* plan);
int lr_hi_backproject(int32_t rank, dim3 grid, hipStream_t st, const float* e, const float* msg1, float* msg2, float* ws,
                      const int64_t* plan);
int lr_hi_decode(int32_t rank, dim3 grid, hipStream_t st, float* e, const float* msg1, const float* msg2, float* out,
                 float div, const int64_t* plan);


// PowerGossip's orthogonalise and diff, one workgroup per (matrix, edge) of `grid` at any rank of the list
// (lowrank_gossip.hip): lowrank_gossip_mfma.hip's entry points launch them too.
int lg_orth(int32_t rank, dim3 grid, hipStream_t st, const float* own, const float* recv, float* phat, uint32_t lo_mask,
            const int64_t* plan);
int lg_diff(int32_t rank, dim3 grid, hipStream_t st, const float* own, const float* recv, float* q, float* dq,
            uint32_t lo_mask, const int64_t* plan);

}  // namespace choco
