// What the two low-rank kernel families share (lowrank.hip: ranks 1, 2 and 4 on the vector ALUs;
// lowrank_mfma.hip: ranks 8, 16 and 32 on the fp32 matrix instruction): the tile table's layout,
// its builder, the check every launch makes first, and the high-rank launches' declarations.
// lowrank_cholqr.hip (Cholesky-QR orthogonalisation at ranks 8, 16 and 32) reads the same table, and so
// does lowrank_gossip.hip (PowerGossip, batched over a worker's edges), which also shares the
// Gram-Schmidt sweep below with lowrank.hip.
#pragma once

#include "choco_common.h"

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

// ---------------------------------------------------------------- the table (host)
static bool lr_rank_hi(int32_t r) { return r == 8 || r == 16 || r == 32; }
static bool lr_rank_ok(int32_t r) { return r == 1 || r == 2 || r == 4 || lr_rank_hi(r); }
#define LR_RANKS_TEXT "rank must be 1, 2, 4, 8, 16 or 32, got %d"

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

}  // namespace choco
