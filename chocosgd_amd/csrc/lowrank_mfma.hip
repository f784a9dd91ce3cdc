// Rank-8, 16 and 32 PowerSGD: project, back-project and decode on v_mfma_f32_16x16x4_f32 -- the
// one place in this library where a matrix instruction pays.  The vector
// kernels of lowrank.hip read R LDS words and run R fmaf per element and need a 6 R-step
// butterfly per row; here a lane hands the instruction one value of M and one of the factor for
// 1024 multiply-adds, and the reduction over k happens inside it.  The products stay fp32 (no
// bf16 / fp16 inputs), memory-bound: 2 r flop per 4 to 12 bytes.
//
// The instruction, lane l of the wave:  A[i = l % 16][k = l / 16],  B[k = l / 16][j = l % 16],
// four results v: D[i = 4 (l / 16) + v][j = l % 16].  k is summed inside, so any assignment of the
// real reduction index to (step, k) is valid as long as A and B use the same one.  Rank 32 is two
// 16-wide result tiles; rank 8 is one whose upper eight rank columns are fed zeros (free in a
// loop that waits for memory).
//
// The table, the messages, the slab scheme, lowrank_slabsum_kernel, orthogonalise and the copy of an
// uncompressed tensor's piece (lr_copy_item) are lowrank.hip's and lowrank.h's; a row item is whole
// 16-row tiles here.  Q goes through LDS in blocks of
// kLrHiColBlock columns in the message's own [col][r] layout, the row stride padded by 4 words so
// that the lanes of a read fall on 64 different banks.  A lane (i, kq) always touches M in
// 16-byte groups of four consecutive columns, a row's 64 columns (project, decode) or a row's 64
// columns of the strip (back-project) being one 256-byte segment.  A matrix whose rows are all
// on the 16-byte grid (its start is, and cols % 4 == 0) runs the 16-byte instantiation; any other
// the guarded scalar one (the rows of a tile then differ in alignment).
// No atomics: every sum's order is fixed by the table and the rank.  The instruction's wrapper and the guarded
// 16-byte accesses (lr_mfma, lr_ld4, lr_st4, lr_nv, lr_rows_aligned) are in lowrank.h, shared with
// lowrank_gossip_mfma.hip.
#include "lowrank.h"

namespace choco {

template <int R>
struct LrHi {
  static constexpr int NT = R > 16 ? R / 16 : 1;  // 16-wide result tiles along the rank
  static constexpr int RN = 16 * NT;              // rank columns of the result tiles
  static constexpr int QS = R + 4;                // LDS row stride of Q: 4 QS = 16 (mod 32), QS = 4 (mod 8)
  static constexpr int PS = R == 32 ? 48 : R;     // LDS row stride of P^ in back-project: the four k rows 16 banks apart
};

// the workgroup stages columns [cb0, cb0 + nb) of a (cols x R) row-major factor at src as
// kLrHiColBlock rows of QS words, the rows past nb zero (a zero of M times them must stay zero)
template <int R>
CHOCO_DEV void lr_stage_q(float* Qs, const float* __restrict__ src, int nb) {
  for (int i = threadIdx.x; i < kLrHiColBlock * R; i += kLrThreads) {
    const int c = i / R, r = i % R;
    Qs[c * LrHi<R>::QS + r] = c < nb ? src[i] : 0.0f;
  }
}

// ---------------------------------------------------------------- project
// A tile is 16 rows x R ranks of P, accumulated in registers across all columns.  Lane (i, kq)
// loads row i's groups at columns c0 + 16 t + 4 kq, t = 0..3: sixteen k steps a 64-column chunk,
// B = Q[col][j] from LDS.  The four waves take the chunks of the tile interleaved and are joined
// through LDS in wave order.
template <int R, bool AL>
CHOCO_DEV void lr_project_item(const float* __restrict__ g, float* __restrict__ e, const float* __restrict__ q,
                               float* __restrict__ msg1, const LrMat& M, int64_t row0, int nrows, float* Qs, float* red) {
  constexpr int NT = LrHi<R>::NT, RN = LrHi<R>::RN, QS = LrHi<R>::QS;
  const int lane = lane_id(), w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
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
        lr_stage_q<R>(Qs, q + M.qoff + cb0 * R, nb);
        __syncthreads();
      }
      const int nch = (nb + 63) >> 6;
      for (int ch = w; ch < nch; ch += kLrWaves) {
        const int cl = 64 * ch + 4 * kq;
        float4 m[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const int64_t col = cb0 + cl + 16 * tt;
          const int nv = lr_nv(row_ok, M.cols, col);
          const float4 gv = lr_ld4<AL, true>(g + a0 + col, nv), ev = lr_ld4<AL, false>(e + a0 + col, nv);
          m[tt] = make_float4(gv.x + ev.x, gv.y + ev.y, gv.z + ev.z, gv.w + ev.w);
          lr_st4<AL>(e + a0 + col, nv, m[tt]);
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float* qr = Qs + (cl + 16 * tt + u) * QS + i;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
              const float b = (R >= 16 || i < R) ? qr[16 * n] : 0.0f;
              acc[n] = lr_mfma(lr_comp(m[tt], u), b, acc[n]);
            }
          }
        }
      }
    }
    __syncthreads();  // the last tile's sums have been read
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int v = 0; v < 4; ++v) red[(w * kLrTile + 4 * kq + v) * RN + 16 * n + i] = acc[n][v];
    }
    __syncthreads();
    for (int x = threadIdx.x; x < kLrTile * RN; x += kLrThreads) {
      const int ri = x / RN, j = x % RN;
      if (kLrTile * t + ri < nrows && j < R)
        msg1[M.poff + (row0 + kLrTile * t + ri) * R + j] =
            ((red[x] + red[kLrTile * RN + x]) + red[2 * kLrTile * RN + x]) + red[3 * kLrTile * RN + x];
    }
  }
}

template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_project_mfma_kernel(const float* __restrict__ g,
                                                                          float* __restrict__ e,
                                                                          const float* __restrict__ q,
                                                                          float* __restrict__ msg1,
                                                                          const int64_t* __restrict__ plan) {
  __shared__ float Qs[kLrHiColBlock * LrHi<R>::QS];
  __shared__ float red[kLrWaves * kLrTile * LrHi<R>::RN];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) return lr_copy_item(msg1, it[3], g, it[1], (int)it[2]);
  const LrMat M = lr_mat(plan, it[0]);
  if (lr_rows_aligned(g, M) && lr_rows_aligned(e, M))
    lr_project_item<R, true>(g, e, q, msg1, M, it[1], (int)it[2], Qs, red);
  else
    lr_project_item<R, false>(g, e, q, msg1, M, it[1], (int)it[2], Qs, red);
}

// ---------------------------------------------------------------- decode
// The tile transposed: D'[col][row] = sum_k Q[col][k] P^[row][k], k the rank in R / 4 steps.  A is
// Q[col][k] from LDS, B = P^[row = l % 16][k] sits in R / 4 registers for the row tile, and a
// lane's four results are four consecutive columns of one row: one 16-byte load of e, one 16-byte
// store each of out and e, four column tiles back to back.
template <int R, bool AL>
CHOCO_DEV void lr_decode_item(float* __restrict__ e, const float* __restrict__ msg1, const float* __restrict__ msg2,
                              float* __restrict__ out, float div, const LrMat& M, int64_t row0, int nrows, float* Qs) {
  constexpr int QS = LrHi<R>::QS, KS = R / 4;
  const int lane = lane_id(), w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const int ntile = (nrows + kLrTile - 1) / kLrTile;
  for (int64_t cb0 = 0; cb0 < M.cols; cb0 += kLrHiColBlock) {
    const int nb = (int)(M.cols - cb0 < kLrHiColBlock ? M.cols - cb0 : kLrHiColBlock);
    __syncthreads();
    lr_stage_q<R>(Qs, msg2 + M.qoff + cb0 * R, nb);
    __syncthreads();
    const int nch = (nb + 63) >> 6;
    for (int t = 0; t < ntile; ++t) {
      const int rl = kLrTile * t + i;
      const bool row_ok = rl < nrows;
      const int64_t a0 = M.off + (row0 + rl) * M.cols;
      float p[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) p[s] = row_ok ? msg1[M.poff + (row0 + rl) * R + 4 * s + kq] : 0.0f;
      for (int ch = w; ch < nch; ch += kLrWaves) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float* qr = Qs + (64 * ch + 16 * ct + i) * QS + kq;
          lr_f32x4 d = lr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int s = 0; s < KS; ++s) d = lr_mfma(qr[4 * s], p[s], d);
          const int64_t col = cb0 + 64 * ch + 16 * ct + 4 * kq;
          const int nv = lr_nv(row_ok, M.cols, col);
          const float4 m = lr_ld4<AL, false>(e + a0 + col, nv);
          lr_st4<AL>(out + a0 + col, nv, make_float4(d[0], d[1], d[2], d[3]));
          lr_st4<AL>(e + a0 + col, nv, make_float4(m.x - d[0] / div, m.y - d[1] / div, m.z - d[2] / div, m.w - d[3] / div));
        }
      }
    }
  }
}

template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_decode_mfma_kernel(float* __restrict__ e,
                                                                         const float* __restrict__ msg1,
                                                                         const float* __restrict__ msg2,
                                                                         float* __restrict__ out, float div,
                                                                         const int64_t* __restrict__ plan) {
  __shared__ float Qs[kLrHiColBlock * LrHi<R>::QS];
  const int64_t* it = plan + plan[kLrOffRow] + kLrItemRow * (int64_t)blockIdx.x;
  if (it[0] < 0) return lr_copy_item(out, it[1], msg1, it[3], (int)it[2]);
  const LrMat M = lr_mat(plan, it[0]);
  if (lr_rows_aligned(e, M) && lr_rows_aligned(out, M))
    lr_decode_item<R, true>(e, msg1, msg2, out, div, M, it[1], (int)it[2], Qs);
  else
    lr_decode_item<R, false>(e, msg1, msg2, out, div, M, it[1], (int)it[2], Qs);
}

// ---------------------------------------------------------------- back-project
// An item is lowrank.hip's: kLrStrip columns x one slab of kLrSlab rows.  Lane (i, kq) loads the
// group at row 4 s + kq, columns col0 + 4 i .. + 4: four rows of 256 bytes an instruction.
// Component u feeds result tile u, whose 16 "rows" are the columns col0 + 4 i + u; the four
// MFMAs of a load share B = P^[row][j] from the slab's P^ rows in LDS.  The waves interleave
// over the slab's rows and are joined in wave order through the LDS that held P^.
template <int R, bool AL>
CHOCO_DEV void lr_backproject_item(const float* __restrict__ Mflat, const float* __restrict__ msg1,
                                   float* __restrict__ msg2, float* __restrict__ ws, const LrMat& M, int64_t col0,
                                   int64_t slab, float* smem) {
  constexpr int NT = LrHi<R>::NT, RN = LrHi<R>::RN, PS = LrHi<R>::PS;
  const int lane = lane_id(), w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const int64_t row0 = slab * kLrSlab;
  const int nrows = (int)(M.rows - row0 < kLrSlab ? M.rows - row0 : kLrSlab);
  for (int x = threadIdx.x; x < kLrSlab * R; x += kLrThreads) {
    const int rr = x / R, j = x % R;
    smem[rr * PS + j] = rr < nrows ? msg1[M.poff + row0 * R + x] : 0.0f;
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
    const float4 m = lr_ld4<AL, false>(Mflat + M.off + (row0 + rl) * M.cols + col, lr_nv(rl < nrows, M.cols, col));
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const float b = (R >= 16 || i < R) ? smem[rl * PS + 16 * n + i] : 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u][n] = lr_mfma(lr_comp(m, u), b, acc[u][n]);
    }
  }
  __syncthreads();  // P^ has been read: its LDS takes the waves' partial tiles, [wave][column][rank]
#pragma unroll
  for (int u = 0; u < 4; ++u) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int v = 0; v < 4; ++v) smem[(w * kLrStrip + 4 * (4 * kq + v) + u) * RN + 16 * n + i] = acc[u][n][v];
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < kLrStrip * R; x += kLrThreads) {
    const int c = x / R, j = x % R;
    if (col0 + c >= M.cols) continue;
    float* dst = M.nslab == 1 ? msg2 + M.qoff + (col0 + c) * R : ws + M.wsoff + (slab * M.cols + col0 + c) * R;
    const float* r0 = smem + c * RN + j;
    dst[j] = ((r0[0] + r0[kLrStrip * RN]) + r0[2 * kLrStrip * RN]) + r0[3 * kLrStrip * RN];
  }
}

template <int R>
__global__ __launch_bounds__(kLrThreads) void lowrank_backproject_mfma_kernel(const float* __restrict__ Mflat,
                                                                              const float* __restrict__ msg1,
                                                                              float* __restrict__ msg2,
                                                                              float* __restrict__ ws,
                                                                              const int64_t* __restrict__ plan) {
  constexpr int kP = kLrSlab * LrHi<R>::PS, kRed = kLrWaves * kLrStrip * LrHi<R>::RN;
  __shared__ float smem[kP > kRed ? kP : kRed];
  const int64_t* it = plan + plan[kLrOffBp] + kLrItemRow * (int64_t)blockIdx.x;
  const LrMat M = lr_mat(plan, it[0]);
  if (lr_rows_aligned(Mflat, M))
    lr_backproject_item<R, true>(Mflat, msg1, msg2, ws, M, it[1], it[2], smem);
  else
    lr_backproject_item<R, false>(Mflat, msg1, msg2, ws, M, it[1], it[2], smem);
}

// ---------------------------------------------------------------- the launches
int lr_hi_project(int32_t rank, dim3 grid, hipStream_t st, const float* g, float* e, const float* q, float* msg1,
                  const int64_t* plan) {
  return lr_dispatch_hi(rank, [&](auto R) {
    return CHOCO_LAUNCH("lowrank_project_mfma_kernel", "lowrank_project_mfma_kernel", lowrank_project_mfma_kernel<R>, grid,
                        dim3(kLrThreads), st, g, e, q, msg1, plan);
  });
}

int lr_hi_backproject(int32_t rank, dim3 grid, hipStream_t st, const float* e, const float* msg1, float* msg2, float* ws,
                      const int64_t* plan) {
  return lr_dispatch_hi(rank, [&](auto R) {
    return CHOCO_LAUNCH("lowrank_backproject_mfma_kernel", "lowrank_backproject_mfma_kernel",
                        lowrank_backproject_mfma_kernel<R>, grid, dim3(kLrThreads), st, e, msg1, msg2, ws, plan);
  });
}

int lr_hi_decode(int32_t rank, dim3 grid, hipStream_t st, float* e, const float* msg1, const float* msg2, float* out,
                 float div, const int64_t* plan) {
  return lr_dispatch_hi(rank, [&](auto R) {
    return CHOCO_LAUNCH("lowrank_decode_mfma_kernel", "lowrank_decode_mfma_kernel", lowrank_decode_mfma_kernel<R>, grid,
                        dim3(kLrThreads), st, e, msg1, msg2, out, div, plan);
  });
}

}  // namespace choco
