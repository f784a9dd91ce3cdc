/*
 * choco_codec.h -- C ABI of the MI355X (gfx950) CHOCO compressor codec.
 *
 * This is the drop-in boundary for ChocoSGD's compressor operator path
 * (reference: epfml/ChocoSGD, dl_code/pcode).  Each entry point names the
 * reference interface it replaces (file:line relative to the reference's
 * dl_code/ directory).  All pointers are DEVICE pointers owned by the caller
 * unless documented as host arrays; all work is enqueued on `stream`
 * (a hipStream_t passed as void*), nothing allocates, nothing synchronises.
 *
 * Return value of every function: CHOCO_OK (0) or a negative CHOCO_ERR_*;
 * choco_last_error() returns the per-thread message of the last failure.
 *
 * Workspaces (`ws`, sized by the matching *_workspace_size): device memory the
 * caller zero-fills ONCE before first use; every call leaves it ready for the
 * next (self-resetting tickets and histograms).  A workspace carries state
 * between the kernels of one call, so calls that may run concurrently need
 * separate workspaces (one per stream).
 *
 * Element/index conventions:
 *   - n counts fp32 elements; every n must be < 2^31 (indices are int32 on the
 *     wire; the reference sends fp32 indices and is inexact above 2^24,
 *     pcode/utils/communication.py:69-72 + pcode/utils/sparsification.py:76).
 *   - "delta" inputs: if xhat != NULL the op works on d = x - xhat computed in
 *     fp32 (pcode/optim/parallel_choco_v.py:236,382,482), else on d = x.
 *   - segment tables `seg_off` are int64[nseg+1], seg_off[0] = 0,
 *     seg_off[nseg] = n (the per-tensor layout of create_optimizer.py:15-24).
 */
#ifndef CHOCO_CODEC_H_
#define CHOCO_CODEC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHOCO_OK 0
#define CHOCO_ERR_INVALID (-1)   /* bad argument / shape / alignment          */
#define CHOCO_ERR_HIP (-2)       /* HIP runtime error                          */
#define CHOCO_ERR_WORKSPACE (-3) /* workspace too small                        */

/* ---------------------------------------------------------------- library */
int choco_version(void);                          /* ABI version, currently 1 */
int choco_last_error(char* buf, size_t len);      /* copies message, returns its length */

/* k = max(1, int(n * (1 - ratio))) evaluated in IEEE double exactly as
 * SparsificationCompressor.get_top_k / get_random_k do
 * (pcode/utils/sparsification.py:22,45). */
int64_t choco_topk_k(int64_t n, double ratio);

/* --------------------------------------------------------------- top-k
 * Replaces SparsificationCompressor.get_top_k (pcode/utils/sparsification.py:18-31)
 * and the per-tensor loop of CHOCOSparsificationCompressor.compress
 * (pcode/optim/parallel_choco_v.py:229-260).
 * Output: exactly k (value, index) pairs of the largest |d|, SIGNED values,
 * in ascending index order.  Ties at the k-th magnitude are broken towards the
 * lowest index (the reference's k==1 path, torch.max, does the same; its
 * torch.topk order is implementation-defined). */
size_t choco_topk_workspace_size(int64_t n);
/* Warm start.  A top-k workspace keeps the previous call's exact threshold and
 * bucket counts, and the library keeps (host side, per workspace pointer) the
 * (n, k) and the call count of the last call made on it.  A call with the same
 * (n, k) as the previous call on the same workspace skips the sampling kernel
 * and selects inside a candidate window around the previous threshold (its
 * margin follows the drift observed between calls); a call whose window misses
 * takes the exact fallback, and leaves a fresh window for the next call.  The
 * output is identical on every path.  Calls on one workspace must be issued in
 * stream order (one stream per workspace, as above).
 * choco_topk_workspace_reset forgets every workspace inside [ws, ws + ws_bytes)
 * (call it whenever a top-k / random-k / segmented workspace is allocated or
 * zero-filled again: its next call is cold); choco_topk_set_warm_start(0) turns
 * the warm path off library-wide (every call samples). */
int choco_topk_workspace_reset(const void* ws, size_t ws_bytes);
int choco_topk_set_warm_start(int32_t enable);
/* Byte offset, in every top-k / random-k / segmented workspace, of a sticky uint32
 * status word.  Bit 0: a bounded wait inside the exact fallback gave up, so the
 * output of that call is invalid (never expected; the wait is bounded so that a
 * stuck producer cannot hang the GPU).  The device raises the same bits in a
 * pinned host mirror of the word with a system-scope store, so
 * choco_topk_host_status(ws, clear, stream) reads them with NO copy and NO
 * synchronisation: a call issued after the failing call has run on the GPU sees
 * them (the Python wrapper checks before every call and raises RuntimeError, the
 * exception the reference's pipelines catch, parallel_choco_v.py:226-227).  It
 * returns the bits (0: nothing raised); clear != 0 zeroes the mirror and queues a
 * zero of the device word on `stream`.  The mirror is released with the workspace
 * (choco_topk_workspace_reset). */
#define CHOCO_TOPK_STATUS_OFFSET 0
int choco_topk_host_status(const void* ws, int32_t clear, void* stream);
/* Byte offset of a uint32 counter of calls (flat: the exact fallback; segmented: segments
 * whose warm window missed) in the same workspaces: diagnostics, never reset by the codec. */
#define CHOCO_TOPK_FALLBACKS_OFFSET 4
/* Flat workspaces only, diagnostics: the uint32 cold-run length (calls left that take a
 * sampled window after a warm window missed) and a uint32 counter of calls whose stream
 * kernel took that sample itself (never with the fused consensus step, whose x changes
 * under the stream: the host then runs the separate sample kernel first). */
#define CHOCO_TOPK_COLD_LEFT_OFFSET 8
#define CHOCO_TOPK_K2_SAMPLES_OFFSET 16
/* Flat workspaces only, diagnostics (byte offsets of uint32 words unless noted; read them
 * after the call has completed, never written by the host): the rest of the warm-start
 * controller's state, as the finish kernel of the last call left it.
 *   BACKOFF   the length of the last cold run, as warm hits have halved it since (not below
 *             64): the next warm miss doubles it (64 on a fresh workspace, at most 4096) and
 *             starts a cold run of that many calls;
 *   T_PREV    the last call's exact k-th key (|v| bits; 0 after a fallback), D_PREV its move
 *             against the call before (int32 bits; 0 when there is none for this (n, k));
 *   SH_LO / SH_HI / SH_NK  the window the last call prepared for the next one and a tag of
 *             the (n, k) it was made for; SH_HITS the cold-run calls in a row whose k-th key
 *             that carried window would have held (2 end the cold run early);
 *   D_CAND    the drift the last call proposed (int32 bits), D_TRUST the calls in a row whose
 *             proposed drift predicted the k-th key better than the previous key did (from 2
 *             on the prepared window is moved by the drift);
 *   OVERFLOW + 4 par  per call parity (call count on the workspace & 1): bit 0 a side list
 *             overflowed, bit 1 the sample was degenerate; either means the exact fallback.
 *             Call c's word stays as it was until call c + 1's stream kernel clears it;
 *   BOUNDS + CHOCO_TOPK_DIAG_BOUNDS_STRIDE par  the window call c used (par = c & 1) and, at
 *             the other parity, the one it prepared: uint32 S_LO, S_HI, SHIFT, M1024 (the
 *             margin in 1/1024 of k; 0: a sampled or fallback window), int64 N, K and uint32
 *             VALID at the CHOCO_TOPK_DIAG_BOUNDS_* offsets inside the entry. */
#define CHOCO_TOPK_DIAG_BACKOFF_OFFSET 12
#define CHOCO_TOPK_DIAG_T_PREV_OFFSET 20
#define CHOCO_TOPK_DIAG_D_PREV_OFFSET 24
#define CHOCO_TOPK_DIAG_SH_LO_OFFSET 28
#define CHOCO_TOPK_DIAG_SH_HI_OFFSET 32
#define CHOCO_TOPK_DIAG_SH_NK_OFFSET 36
#define CHOCO_TOPK_DIAG_SH_HITS_OFFSET 40
#define CHOCO_TOPK_DIAG_D_CAND_OFFSET 44
#define CHOCO_TOPK_DIAG_D_TRUST_OFFSET 48
#define CHOCO_TOPK_DIAG_OVERFLOW_OFFSET 64
#define CHOCO_TOPK_DIAG_BOUNDS_OFFSET 128
#define CHOCO_TOPK_DIAG_BOUNDS_STRIDE 40
#define CHOCO_TOPK_DIAG_BOUNDS_S_LO 0
#define CHOCO_TOPK_DIAG_BOUNDS_S_HI 4
#define CHOCO_TOPK_DIAG_BOUNDS_SHIFT 8
#define CHOCO_TOPK_DIAG_BOUNDS_M1024 12
#define CHOCO_TOPK_DIAG_BOUNDS_N 16
#define CHOCO_TOPK_DIAG_BOUNDS_K 24
#define CHOCO_TOPK_DIAG_BOUNDS_VALID 32
#define CHOCO_TOPK_STATUS_POLL_TIMEOUT 1
int choco_topk_compress(const float* x, const float* xhat, int64_t n, int64_t k,
                        float* out_val, int32_t* out_idx,
                        void* ws, size_t ws_bytes, void* stream);

/* choco_topk_compress followed by the SELF message's part of
 * CHOCOSparsificationCompressor.uncompress (parallel_choco_v.py:307-310), folded into
 * the emission of the message (no second launch, no re-read of the message):
 *   if hat_self != NULL:  hat_self[idx] += val
 *   if memory   != NULL:  memory[idx]   += (float)weight * val
 * with the arithmetic of choco_sparse_accumulate (at least one target non-NULL).
 * hat_self may be xhat itself (the CHOCO case): it is written only after this call's
 * last read of it.  The reference applies the messages to memory in ascending rank
 * order (topology.py:161-162 get_neighborhood), so memory may be folded bit-identically
 * only when the self rank comes first among the neighbours (rank 0 of a ring, or a
 * single worker); pass memory = NULL otherwise and apply the self message to memory
 * with choco_sparse_accumulate in its turn. */
int choco_topk_compress_accumulate(const float* x, const float* xhat, int64_t n, int64_t k,
                                   float* out_val, int32_t* out_idx, float* hat_self, float* memory,
                                   float weight,
                                   void* ws, size_t ws_bytes, void* stream);

/* Per-segment top-k (one tensor per segment, as the reference loops over
 * parameter tensors): k_s = choco_topk_k(len_s, ratio), outputs concatenated in
 * segment order, indices GLOBAL (segment offset added in integer arithmetic --
 * the reference adds it in fp32, sparsification.py:76).  Every segment of up to
 * 16M elements is cut into 16K-element tiles and ALL of them are selected in the
 * same launches (topk_seg.hip): five on a cold call, which reads the input twice (a
 * workspace's first call, and the calls of a cold run), three on a warm call, which reads
 * it once inside the windows the previous call left; longer segments run the flat pipeline.
 * choco_topk_segmented_plan fills a HOST int64 plan of
 * choco_topk_segmented_plan_len(seg_off, nseg) entries from the HOST table
 * seg_off[nseg+1]: nseg rows of 8 {off, len, k_s, out_off, first tile, tiles, ., .}
 * (row 0's last two = total tiles, batched segments), then the tile -> segment
 * map, then the batched segment ids, the random-k tile table (randk.hip) and the
 * collect launch's tile order (single-tile segments first).  It returns K = sum k_s (the reference's
 * selected_shapes are the k_s, parallel_choco_v.py:245); ratio must be in [0, 1).
 * The caller keeps a DEVICE copy of the whole plan (plan_dev) and passes both on
 * every call.  x / xhat need only 4-byte alignment.  The workspace
 * (choco_topk_segmented_workspace_size) is bound to ONE plan: its per-segment
 * histograms are left zeroed for the next call of that plan, so a workspace that
 * served another plan or call must be zero-filled again first. */
int64_t choco_topk_segmented_plan_len(const int64_t* seg_off_host, int32_t nseg);
int64_t choco_topk_segmented_plan(const int64_t* seg_off_host, int32_t nseg, double ratio,
                                  int64_t* plan_host);
size_t choco_topk_segmented_workspace_size(const int64_t* plan_host, int32_t nseg);
int choco_topk_compress_segmented(const float* x, const float* xhat, const int64_t* plan_dev,
                                  const int64_t* plan_host, int32_t nseg,
                                  float* out_val, int32_t* out_idx,
                                  void* ws, size_t ws_bytes, void* stream);
/* Segmented workspaces, diagnostics (read-only; nothing here is on the hot path).  Each
 * multi-tile batched segment s carries a warm window of CHOCO_SEG_WIN_STRIDE bytes at
 * win_off + CHOCO_SEG_WIN_STRIDE s, uint32 words at the CHOCO_SEG_WIN_* byte offsets:
 *   LO / SH   next call's candidates are the keys >= LO, binned by (key - LO) >> SH (SH <= 9);
 *   VALID     0 until a call has written the window;
 *   T_PREV    the exact k_s-th key of the call that wrote it (0 after a take-all call), D_PREV
 *             its move against the call before (int32 bits);
 *   CAND      the drift that call proposed (int32 bits), TRUST the calls in a row whose proposed
 *             drift predicted the k-th key better than the previous key did (at most 15; from
 *             2 on the window is moved by the drift).
 * and a row of CHOCO_SEG_INFO_STRIDE bytes at info_off + CHOCO_SEG_INFO_STRIDE s, uint32 words:
 * after a warm call, word CHOCO_SEG_INFO_LO / _SH hold the window the call used and word
 * CHOCO_SEG_INFO_MODE how it went (0 selected inside the window, 1 the k-th key was below
 * the window, 3 above it -- both selected exactly and counted at CHOCO_TOPK_FALLBACKS_OFFSET --
 * 2 every element taken).  CHOCO_SEG_SHADOW_OFFSET: a uint64 in the workspace header, added
 * to by every cold call, per multi-tile segment, (1 << 32 if the window the previous call
 * left would not have held this call's k-th key) + 1.
 * choco_topk_segmented_diag_layout returns win_off and info_off of the plan's workspace.
 * choco_topk_segmented_host_state copies the host's warm / cold bookkeeping of the
 * workspace `ws` (the base pointer passed to the compress calls) into out[8]: calls made,
 * the call at which the miss flag was last seen, cold calls left in the run, the backoff
 * (length of the last cold run as exits have halved it), clean (cold calls' checks without
 * a miss), the shadow counter's checks and misses when last read, and the pinned miss-flag
 * word as it stands (1: a warm call's window missed and no later call has seen it yet).
 * All zeros for a workspace no call was made on; it creates no record and touches no GPU. */
#define CHOCO_SEG_WIN_STRIDE 32
#define CHOCO_SEG_WIN_LO 0
#define CHOCO_SEG_WIN_SH 4
#define CHOCO_SEG_WIN_VALID 8
#define CHOCO_SEG_WIN_T_PREV 16
#define CHOCO_SEG_WIN_D_PREV 20
#define CHOCO_SEG_WIN_CAND 24
#define CHOCO_SEG_WIN_TRUST 28
#define CHOCO_SEG_INFO_STRIDE 32
#define CHOCO_SEG_INFO_LO 0
#define CHOCO_SEG_INFO_SH 1
#define CHOCO_SEG_INFO_MODE 6
#define CHOCO_SEG_SHADOW_OFFSET 64
int choco_topk_segmented_diag_layout(const int64_t* plan_host, int32_t nseg, int64_t* win_off,
                                     int64_t* info_off);
int choco_topk_segmented_host_state(const void* ws, const int64_t* plan_host, int32_t nseg,
                                    uint64_t out[8]);

/* ------------------------------------------------------------- random-k
 * Replaces SparsificationCompressor.get_random_k (sparsification.py:40-54).
 * The reference draws np.random.choice(n, k, replace=False) on the host (legacy
 * RandomState); here a uniform k-subset of [0, n) is drawn on the device, and
 * only the k selected elements are read (randk.hip):
 *   derive(K, i) = splitmix64_mix(K + (i + 1) * 0x9E3779B97F4A7C15);
 *   K = derive(key, 0), key = splitmix64_mix(seed + (offset + 1) * 0xD1B54A32D192ED03);
 *   pi_N(j; K): on B bits (2^B >= N, h = (B + 1) / 2), four rounds of
 *     x = (x + a_r) & mask; x = (x * m_r) & mask; x ^= x >> h,
 *     a_r = (u32)derive(K, 2r) & mask, m_r = ((u32)derive(K, 2r + 1) | 1) & mask,
 *     repeated while x >= N (cycle walking: a bijection of [0, N));
 *   tiles of 2^18 elements; tile t holds c_t = #{ j < k : pi_n(j; K) >> 18 == t }
 *     of the selected indices (one tile: c_0 = k; k >= n: every index);
 *   its positions are pi_{L_t}(j; derive(K, 8 + t)), j < c_t (L_t = the tile length).
 * Output in ascending index order.  `offset` selects an independent stream for the
 * same seed (e.g. the step number).  is_biased = 0 scales values by
 * (float)(n / k) like the reference's unbiased branch (sparsification.py:54).
 * Workspace: choco_randk_workspace_size(n) (zero-filled once; see the top-k
 * workspace rules; choco_topk_workspace_reset also resets it). */
size_t choco_randk_workspace_size(int64_t n);
int choco_randk_compress(const float* x, const float* xhat, int64_t n, int64_t k,
                         uint64_t seed, uint64_t offset, int32_t is_biased,
                         float* out_val, int32_t* out_idx,
                         void* ws, size_t ws_bytes, void* stream);

/* Gather at caller-given int64 indices (the reference's x_data[selected_indices],
 * sparsification.py:31,52); scale = 1 for the biased path, (float)(n/k) otherwise. */
int choco_gather(const float* x, const float* xhat, const int64_t* idx, int64_t k,
                 float scale, float* out_val, void* stream);

/* Per-segment random-k (CHOCOSparsificationCompressor.compress with
 * comm_op "random_k", parallel_choco_v.py:229-260 -> sparsification.py:40-54 per
 * tensor): the plan of choco_topk_segmented_plan (k_s = max(1, int(len_s*(1-ratio))),
 * which also carries the random-k tile table), segment s drawn as above with
 * K_s = derive(key, s), outputs concatenated in segment order with GLOBAL
 * indices.  Any 4-byte alignment; workspace: choco_topk_segmented_workspace_size. */
int choco_randk_compress_segmented(const float* x, const float* xhat, const int64_t* plan_dev,
                                   const int64_t* plan_host, int32_t nseg,
                                   uint64_t seed, uint64_t offset, int32_t is_biased,
                                   float* out_val, int32_t* out_idx,
                                   void* ws, size_t ws_bytes, void* stream);

/* Receiver side of CHOCOSparsificationCompressor.uncompress
 * (parallel_choco_v.py:307-310): for one message (val, idx) of k pairs,
 *   if xhat_self != NULL:  xhat_self[idx] += val
 *   memory[idx] += (float)weight * val        (two roundings, as torch does)
 * Indices within one message must be unique (true for top-k / random-k).
 * n = length of xhat_self / memory: an index outside [0, n) is skipped and
 * counted into *bad_count (device uint32, nullable) -- the reference's
 * index_put raises IndexError there. */
int choco_sparse_accumulate(const float* val, const int32_t* idx, int64_t k,
                            float* xhat_self, float* memory, int64_t n, float weight,
                            uint32_t* bad_count, void* stream);

/* Every neighbour's message of a receive step in ONE call: the per-neighbour loop of
 * CHOCOSparsificationCompressor.uncompress (parallel_choco_v.py:291-310) --
 *   for m in 0 .. nmsg-1 (neighbors_info order):
 *     if m == self_slot and xhat_self != NULL:  xhat_self[idx_m] += val_m
 *     memory[idx_m] += (float)weights[m] * val_m
 * bit-identical to nmsg choco_sparse_accumulate calls in that order (which is how it runs:
 * a merged sweep that applies all messages to each touched line of memory once measured
 * slower).  vals / idxs / ks / weights are HOST arrays of nmsg (1..8) entries
 * (device pointers inside).  Workspace: choco_sparse_accumulate_multi_workspace_size(n,
 * nmsg) bytes (0: none).  Out-of-range / non-ascending indices are counted into
 * *bad_count (nullable), as by choco_sparse_accumulate. */
size_t choco_sparse_accumulate_multi_workspace_size(int64_t n, int32_t nmsg);
int choco_sparse_accumulate_multi(const float* const* vals, const int32_t* const* idxs, const int64_t* ks,
                                  const float* weights, int32_t nmsg, int32_t self_slot, float* xhat_self,
                                  float* memory, int64_t n, void* ws, size_t ws_bytes, uint32_t* bad_count,
                                  void* stream);

/* ECDSparsificationCompressor.uncompress (ecd_psgd.py:287-303) for one message:
 * target[idx] = fmaf(b, val, target[idx] * a)   (hat[idx].mul(a).add(b, q_values),
 * a = 1 - 2/t, b = 2/t); out-of-range indices are skipped and counted as above. */
int choco_sparse_extrapolate(const float* val, const int32_t* idx, int64_t k, float* target,
                             int64_t n, float a, float b, uint32_t* bad_count, void* stream);

/* --------------------------------------------------------------- sign
 * Replaces SignCompressor.packing (sparsification.py:129-145, incl. the external
 * bit2byte.packing) and the per-tensor L1 norms of CHOCOSignCompressor.compress
 * (parallel_choco_v.py:476-499).  Layout = the reference's (32, N') view of the
 * zero-padded flat buffer, N' = ceil(n/32): word j holds elements j + r*N',
 * r = 0..31, element r at bit r (LSB first: this repo's documented convention,
 * the unvendored bit2byte's bit order is unpinned); bit set <=> d < 0
 * (sign(0), -0.0, NaN and padding encode as "+").
 * l1_norms (nullable) receives per-segment sum|d| accumulated in fp64 and
 * rounded once to fp32.  seg_off is a DEVICE int64[nseg+1] (may be NULL when
 * nseg == 1).  Workspace: choco_sign_workspace_size(nseg). */
int64_t choco_sign_words(int64_t n);
size_t choco_sign_workspace_size(int32_t nseg);
int choco_sign_compress(const float* x, const float* xhat, int64_t n,
                        const int64_t* seg_off, int32_t nseg,
                        int32_t* packed, float* l1_norms,
                        void* ws, size_t ws_bytes, void* stream);

/* Chunked sign pack (the exchange pipelined with compress, SURVEY.md §8(e);
 * parallel_choco.py exchange_chunks): choco_sign_compress over the words [w0, w1) of the
 * SAME layout (packed is the whole word array; w0 a multiple of 1024, w1 one too or N'),
 * so each range's words can be sent as soon as its launch is queued.  The per-segment L1
 * sums stay in the workspace's fp64 accumulators between calls; the call with finish = 1,
 * issued LAST on the same stream and workspace, writes l1_norms and clears them.  A
 * receiver needs the norms of every segment a range touches, and in the (32, N') layout
 * every range touches every row's segments, so the norms header is sent last and the
 * receiver decodes after the whole message (choco_sign_decompress_accumulate).
 * Words and norms equal the whole-buffer call's (the norms up to fp64 summation order). */
int choco_sign_compress_range(const float* x, const float* xhat, int64_t n, const int64_t* seg_off, int32_t nseg,
                              int64_t w0, int64_t w1, int32_t finish, int32_t* packed, float* l1_norms,
                              void* ws, size_t ws_bytes, void* stream);

/* SignCompressor.unpacking (sparsification.py:147-163): +1.0 / -1.0 floats. */
int choco_sign_unpack(const int32_t* packed, int64_t n, float* out, void* stream);

/* Receiver side of CHOCOSignCompressor.uncompress (parallel_choco_v.py:524-558),
 * fused over all messages in the given order (the reference's neighbors_info
 * order).  For message m with per-segment norms norms[m][s] and packed signs:
 *   upd = (norms[m][s] / (float)numel_s) * sign
 *   if m == self_slot:  xhat_self += upd
 *   memory = fmaf((float)weights[m], upd, memory)     (torch add_(.., alpha=w))
 * packed_list/norms_list/weights are HOST arrays of length nmsg (<= 8) holding
 * device pointers / weights.  self_slot = -1 when no message is the local one. */
int choco_sign_decompress_accumulate(const int32_t* const* packed_list,
                                     const float* const* norms_list,
                                     const float* weights, int32_t nmsg, int32_t self_slot,
                                     int64_t n, const int64_t* seg_off, int32_t nseg,
                                     float* xhat_self, float* memory,
                                     void* ws, size_t ws_bytes, void* stream);

/* Receiver side of the other consumers of the sign codec: for each message m in
 * order, target += weights[m] * decode(m) per element, with the reference's
 * rounding: two_roundings = 0 -> fmaf(w, u, target) (torch add_(u, alpha=w):
 * DCDSignCompressor.uncompress, dcd_psgd.py:442-446, w = 1); 1 -> target + (w * u)
 * (torch add_(w * u): DeepSqueezeSignCompressor.uncompress, deep_squeeze.py:481-488,
 * w = consensus_stepsize * (w_r - [r == self])).  u = (norms[m][s] / numel_s) * sign. */
/* The deferred receive fused into the next step's pass (sign): the previous step's
 * messages applied exactly as choco_sign_decompress_accumulate (x_hat += u_self, memory =
 * fmaf(w, u, memory) in order; CHOCOSignCompressor.uncompress, parallel_choco_v.py:
 * 548-558), then this step's consensus step x += gamma (memory - x_hat) (optim/utils.py:
 * 67-72), then this step's message: packed signs of x - x_hat and l1_norms[s] -- ONE pass
 * over x, x_hat and memory, per-tensor layouts included (n >= 2^30 runs the receive and
 * choco_gossip_sign_compress as two kernels).  Bit-identical x, x_hat, memory and words
 * to that sequence.  packed must not alias a message's words (l1_norms may alias a
 * message's norms: every workgroup reads them before the last one writes).  nmsg 1..8;
 * ws of choco_sign_recv_workspace_size(n, nseg, nmsg) bytes (the pass runs over row runs of
 * the (32, N') view, the messages and the output words as bit planes). */
/* Workspace bytes of choco_sign_recv_gossip_compress for n elements in nseg segments and
 * nmsg messages (the per-segment accumulators plus bit planes of every message and of the
 * output; n >= 2^30: choco_sign_workspace_size(nseg)). */
size_t choco_sign_recv_workspace_size(int64_t n, int32_t nseg, int32_t nmsg);

int choco_sign_recv_gossip_compress(const int32_t* const* packed_list, const float* const* norms_list,
                                    const float* weights, int32_t nmsg, int32_t self_slot, float* x,
                                    float* memory, float* xhat, float gamma, int64_t n,
                                    const int64_t* seg_off, int32_t nseg, int32_t* packed,
                                    float* l1_norms, void* ws, size_t ws_bytes, void* stream);

int choco_sign_decompress_axpy(const int32_t* const* packed_list, const float* const* norms_list,
                               const float* weights, int32_t nmsg, int64_t n,
                               const int64_t* seg_off, int32_t nseg, int32_t two_roundings,
                               float* target, void* stream);

/* ECDSignCompressor.uncompress (ecd_psgd.py:448-454) for one message:
 * target_s = (target_s * a) + ((b * norm_s) / numel_s) * sign   (a = 1 - 2/t, b = 2/t). */
int choco_sign_decompress_extrapolate(const int32_t* packed, const float* norms, int64_t n,
                                      const int64_t* seg_off, int32_t nseg, float a, float b,
                                      float* target, void* stream);

/* DeepSqueezeSignCompressor.compress's local compressed copy (deep_squeeze.py:416-422):
 * out = (norms[s] * torch.sign(x)) / numel_s with torch.sign's values: sign(+-0) = +0 and
 * sign(NaN) = +0 (so out is 0 at a NaN of x), +-1 for infinities and subnormals. */
int choco_sign_local_decode(const float* x, int64_t n, const int64_t* seg_off, int32_t nseg,
                            const float* norms, float* out, void* stream);

/* The local copy with the error feedback that subtracts it, in one pass
 * (deep_squeeze.py:416-422 with :115; ef_sign_sgd.py:153 with :104-106): u is exactly
 * choco_sign_local_decode's value (the same device function), then
 *     resid_out[i] = rn(x[i] - u),   local_out[i] = u   (when local_out != NULL).
 * resid_out may be x itself (each thread reads an element before it writes it); it must
 * not overlap x otherwise, and local_out may overlap neither x nor resid_out: both are
 * checked, with null x / norms / resid_out, n outside [1, 2^31 - 1), nseg < 1, nseg > 1
 * without seg_off and pointers off 4-byte alignment, before the launch and without a
 * HIP call. */
int choco_sign_local_residual(const float* x, int64_t n, const int64_t* seg_off, int32_t nseg,
                              const float* norms, float* local_out, float* resid_out,
                              void* stream);

/* --------------------------------------------------------------- QSGD
 * Replaces QuantizationCompressor.get_qsgd/compress (sparsification.py:87-98,114-120)
 * applied per segment (parallel_choco_v.py:375-397).  s = 2^q - 1 levels.
 *   norm_s  = ||d_s||_2 (fp64 accumulation, rounded once)   or norm_in[s] if given
 *   lf      = ((float)s * |d|) / norm_s
 *   level   = floor(lf) + (u < lf - floor(lf)),  u = u_in[e] if given, else
 *             this codec's stream (the reference draws torch.rand_like,
 *             sparsification.py:91): key = splitmix64_mix(seed + (offset+1) *
 *             0xD1B54A32D192ED03); with g = (e & 8191) >> 11, element e
 *             belongs to stream sid = ((e >> 13) << 9) | ((g >> 1) << 8) |
 *             ((e & 8191) >> 3 & 255) at position p = (g & 1) * 8 + (e & 7)
 *             (16 uniforms per stream); stream sid is xoroshiro128+
 *             (a=24, b=16, c=37) started from (splitmix64_mix(z),
 *             splitmix64_mix(z + 0x9E3779B97F4A7C15)), z = key + (2 sid + 1) *
 *             0x9E3779B97F4A7C15; its output number p / 2, r = s0 + s1, gives
 *             u = (even p: r >> 40, odd p: (r >> 16) & 0xFFFFFF) * 2^-24
 *             (restated in oracle/choco_oracle.py qsgd_uniforms_at)
 * Wire format (packed, choco_qsgd_packed_bytes): level plane (container of
 * cw = 1,2,4,8,16 bits >= q, little-endian within 32-bit words) followed by a
 * sign plane (1 bit/element, bit set <=> d < 0), both padded to 16 bytes.
 * dense_out (nullable) receives the reference's decoded floats
 *   ((scale * sign(d)) * norm_s) * level / (float)s
 * bit-for-bit; norms_out (nullable) the per-segment fp32 norms. q in [1,16]. */
int64_t choco_qsgd_packed_bytes(int64_t n, int32_t q);
size_t choco_qsgd_workspace_size(int32_t nseg);
int choco_qsgd_compress(const float* x, const float* xhat, int64_t n,
                        const int64_t* seg_off, int32_t nseg,
                        int32_t q, int32_t is_biased,
                        const float* norm_in, const float* u_in,
                        uint64_t seed, uint64_t offset,
                        uint8_t* packed, float* norms_out, float* dense_out,
                        void* ws, size_t ws_bytes, void* stream);

/* Decode a packed message to the reference's dense floats (the value that
 * QuantizationCompressor.uncompress, sparsification.py:122-123, passes on). */
int choco_qsgd_decode(const uint8_t* packed, const float* norms, int64_t n,
                      const int64_t* seg_off, int32_t nseg, int32_t q, int32_t is_biased,
                      float* out, void* stream);

/* Receiver side of CHOCOQuantizationCompressor.uncompress (parallel_choco_v.py:415-433)
 * fused over messages:  v = decode(m);  if m == self_slot: xhat_self += v;
 * memory += (float)weights[m] * v   (two roundings). */
int choco_qsgd_decompress_accumulate(const uint8_t* const* packed_list,
                                     const float* const* norms_list,
                                     const float* weights, int32_t nmsg, int32_t self_slot,
                                     int64_t n, const int64_t* seg_off, int32_t nseg,
                                     int32_t q, int32_t is_biased,
                                     float* xhat_self, float* memory, void* stream);

/* The deferred receive fused into the next step's first pass (QSGD): the previous step's
 * messages applied exactly as choco_qsgd_decompress_accumulate (x_hat += q_self, memory +=
 * w * q in order; CHOCOQuantizationCompressor.uncompress, parallel_choco_v.py:430-433),
 * then this step's consensus step x += gamma (memory - x_hat) (optim/utils.py:67-72), then
 * norms_out[s] = ||x - x_hat||_2 per segment (fp64, rounded once) -- ONE pass over x,
 * x_hat and memory instead of the decode, gossip and norm passes; bit-identical x, x_hat
 * and memory.  Quantize this step's message afterwards with choco_qsgd_compress(...,
 * norm_in = norms_out, ...).  Valid wherever the receive of step t-1 and the consensus
 * step of step t are adjacent (ParallelCHOCO_V.step: apply_gradient, then the previous
 * gossip's join, then update_params_from_neighbor).  nmsg 1..8; ws as for
 * choco_qsgd_norms (choco_qsgd_workspace_size(nseg)).  norms_out MAY alias a message's
 * norms (e.g. the pending self message's header, reused as this step's): every workgroup
 * reads the message norms before it takes the last-workgroup ticket, and only the last
 * workgroup writes norms_out.  The level / sign planes must not overlap x, x_hat or memory. */
int choco_qsgd_recv_gossip_norms(const uint8_t* const* packed_list, const float* const* norms_list,
                                 const float* weights, int32_t nmsg, int32_t self_slot, float* x,
                                 float* memory, float* xhat, float gamma, int64_t n,
                                 const int64_t* seg_off, int32_t nseg, int32_t q, int32_t is_biased,
                                 float* norms_out, void* ws, size_t ws_bytes, void* stream);

/* ECDQuantizationCompressor.uncompress (ecd_psgd.py:415-423) for one message:
 * target = fmaf(b, decode(m), target * a)   (hat.mul_(a).add_(q, alpha=b)). */
int choco_qsgd_decompress_extrapolate(const uint8_t* packed, const float* norms, int64_t n,
                                      const int64_t* seg_off, int32_t nseg, int32_t q, int32_t is_biased,
                                      float a, float b, float* target, void* stream);

/* Chunked QSGD wire (the exchange pipelined with compress and decompress, SURVEY.md
 * §8(e); parallel_choco.py exchange_chunks): the norm pass alone, then the quantize
 * pass over element ranges [e0, e1), each range a self-contained message of
 * choco_qsgd_packed_bytes(e1 - e0, q) bytes ([level plane | sign plane] of its own
 * elements), and the receiver over the same ranges.  e0 must be a multiple of 8192
 * (the uniform-stream tile), e1 one too or n.  A range's levels, signs and uniforms
 * are exactly those of choco_qsgd_compress over the whole buffer (element e keeps its
 * stream position), so the decoded values, and memory / xhat_self after all ranges,
 * are bit-identical to the unchunked path; norms come from choco_qsgd_norms (or its
 * gossip form, which also applies the consensus step to x). */
int choco_qsgd_norms(const float* x, const float* xhat, int64_t n, const int64_t* seg_off, int32_t nseg,
                     float* norms_out, void* ws, size_t ws_bytes, void* stream);
int choco_gossip_qsgd_norms(float* x, const float* memory, const float* xhat, float gamma, int64_t n,
                            const int64_t* seg_off, int32_t nseg, float* norms_out, void* ws, size_t ws_bytes,
                            void* stream);
int choco_qsgd_quantize_range(const float* x, const float* xhat, int64_t n, const int64_t* seg_off, int32_t nseg,
                              int32_t q, int32_t is_biased, const float* norms, uint64_t seed, uint64_t offset,
                              int64_t e0, int64_t e1, uint8_t* packed_range, void* stream);
int choco_qsgd_decompress_accumulate_range(const uint8_t* const* packed_list, const float* const* norms_list,
                                           const float* weights, int32_t nmsg, int32_t self_slot, int64_t n,
                                           const int64_t* seg_off, int32_t nseg, int32_t q, int32_t is_biased,
                                           int64_t e0, int64_t e1, float* xhat_self, float* memory,
                                           void* stream);

/* ------------------------------------------------------- gossip step
 * update_params_from_neighbor (pcode/optim/utils.py:67-72):
 *   x += (float)gamma * (memory - xhat)   (three roundings, as torch does). */
int choco_gossip_step(float* x, const float* memory, const float* xhat, float gamma,
                      int64_t n, void* stream);

/* ------------------------------------------- parameter pack / unpack
 * The bridge between a model's parameter tensors and the flat fp32 buffer the
 * entry points above work on: flatten() (pcode/utils/communication.py:58-76, one
 * copy per tensor into a default-dtype -- fp32 -- buffer) and TensorBuffer.unpack
 * (pcode/utils/tensor_buffer.py:38-40, one converting copy per tensor back), each
 * as ONE launch per chunk of tensors.  Tensor s holds lens[s] contiguous elements
 * of dtype dtypes[s] (CHOCO_DT_*) at DEVICE pointer ptrs[s] and owns flat elements
 * [sum(lens[0..s)), + lens[s]); sum(lens) must equal n.  `ptrs`, `lens` and
 * `dtypes` are HOST arrays, copied into the kernel arguments of each launch (no
 * device-side table, nothing allocated, nothing synchronised), so they may be
 * freed as soon as the call returns.
 *   pack:   flat[..] = (float)tensor[..]       widening bf16 / fp16 is exact
 *   unpack: tensor[..] = (dtype)flat[..]       round-to-nearest-even; +-0, +-inf and
 *           NaN are kept, fp16 overflow gives inf, fp16 subnormals are produced
 *           (torch's converting copy)
 * Only the bytes of the layout's own elements are written: tensors may be views
 * packed next to each other in one storage, `flat` may be a slice of a larger
 * buffer.  Pointers need their element's alignment only (16-byte vectors are used
 * where both sides of a group of 8 elements allow them).  Zero-length tensors are
 * allowed (their pointer may be NULL).  Every argument is checked before the first
 * launch without a HIP call; a bad one returns CHOCO_ERR_INVALID and launches
 * nothing.  A layout takes choco_params_launches(nseg) launches of
 * "param_pack_kernel" / "param_unpack_kernel" (choco_launch_count). */
#define CHOCO_DT_F32 0
#define CHOCO_DT_BF16 1
#define CHOCO_DT_F16 2
/* launches a layout of nseg tensors takes (host only); 0 for nseg <= 0 */
int choco_params_launches(int32_t nseg);
int choco_params_pack(const void* const* ptrs, const int64_t* lens, const int32_t* dtypes,
                      int32_t nseg, float* flat, int64_t n, void* stream);
int choco_params_unpack(void* const* ptrs, const int64_t* lens, const int32_t* dtypes,
                        int32_t nseg, const float* flat, int64_t n, void* stream);

/* ------------------------------------------- SGD update fused with the pack
 * apply_gradient (pcode/optim/utils.py:13-47), the update every optimizer of the
 * reference starts its step with, for a whole parameter list as ONE launch per chunk
 * of tensors, optionally writing the flat fp32 buffer flatten() would build next in
 * the same pass.  Tensor s holds lens[s] contiguous elements of dtype dtypes[s] in
 * each of params[s], grads[s] and bufs[s] (its momentum buffer) and owns flat elements
 * [sum(lens[0..s)), + lens[s]); sum(lens) must equal n.  Per element, every line one
 * reference op with one rounding:
 *     d = g
 *     if weight_decay != 0:  d   = fma(wd, p, d)
 *     if momentum != 0:      t   = buf * mom
 *                            buf = FIRST ? fma(1, d, 0 * mom) : fma(1 - damp, d, t)
 *                            d   = NESTEROV ? fma(mom, buf, d) : buf
 *     apply mode:  p_new = fma(-lr, d, p)  -> params (WRITE_PARAMS), flat (if not NULL)
 *     grad mode:   d                       -> grads  (WRITE_GRADS),  flat (if not NULL)
 * with the scalars converted as torch converts a Python scalar for an fp32 tensor:
 * (float)wd, (float)mom, (float)(1.0 - dampening), (float)(-lr).  A skipped op
 * (weight_decay == 0, momentum == 0, tested on the doubles) is skipped, not run with a
 * zero coefficient.  fp32 tensors match the reference bit for bit.  bf16 / fp16
 * tensors: every line is computed in fp32 from the widened operands and narrowed
 * round-to-nearest-even to the tensor's dtype after that line; the scalars stay fp32;
 * the flat value is the narrowed result widened again.  buf is written whenever
 * momentum != 0.
 *   flags[s]: CHOCO_SGD_F_NESTEROV; CHOCO_SGD_F_FIRST: the tensor has no momentum
 *     buffer yet (the reference builds it as zeros.mul_(mom).add_(d_p)): bufs[s] is
 *     written and never read; CHOCO_SGD_F_NOGRAD (p.grad is None): in apply mode a pure
 *     pack, flat = p and nothing else written; grads[s] and bufs[s] are ignored.
 *   mode: CHOCO_SGD_MODE_APPLY or CHOCO_SGD_MODE_GRAD, | CHOCO_SGD_MODE_WRITE_PARAMS
 *     (apply mode only) | CHOCO_SGD_MODE_WRITE_GRADS (grad mode only).
 * All tables are HOST arrays copied into the kernel arguments (nothing allocated or
 * synchronised); the pointers in them are DEVICE pointers.  grads[s] and bufs[s] of one
 * tensor may be the same memory (where both are written, d is stored last).  Distinct
 * tensors, and the flat buffer, must not overlap: this is NOT checked.  Only the bytes
 * of the layout's own elements are written; pointers need their element's alignment
 * only.  Zero-length tensors are allowed (their pointers may be NULL).  Every argument
 * is checked before the first launch without a HIP call -- null tables, nseg <= 0,
 * negative or oversumming lengths, lengths that do not sum to n, unknown dtype, flag or
 * mode bits, misaligned pointers, a NULL param, a NULL grad without NOGRAD, a NULL buf
 * with momentum != 0, NESTEROV with momentum <= 0 or dampening != 0 (the reference's
 * constructors refuse it), NOGRAD in grad mode, flat == NULL with nothing else to
 * write -- and a bad one returns CHOCO_ERR_INVALID and launches nothing.  A layout
 * takes choco_params_sgd_launches(nseg) launches of "param_sgd_kernel". */
#define CHOCO_SGD_F_NESTEROV 1
#define CHOCO_SGD_F_FIRST 2
#define CHOCO_SGD_F_NOGRAD 4
#define CHOCO_SGD_MODE_APPLY 0
#define CHOCO_SGD_MODE_GRAD 1
#define CHOCO_SGD_MODE_WRITE_PARAMS 2
#define CHOCO_SGD_MODE_WRITE_GRADS 4
/* launches an update of nseg tensors takes (pcode/optim/utils.py:13-47 is one loop
 * over them; host only); 0 for nseg <= 0 */
int choco_params_sgd_launches(int32_t nseg);
/* pcode/optim/utils.py:13-47 */
int choco_params_sgd(void* const* params, const void* const* grads, void* const* bufs,
                     const int64_t* lens, const int32_t* dtypes, const double* lr,
                     const double* weight_decay, const double* momentum, const double* dampening,
                     const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                     void* stream);

/* ------------------------------------------- SGD update on fp32 master weights
 * apply_gradient (pcode/optim/utils.py:13-47) for a bf16 / fp16 model that keeps a
 * persistent flat fp32 copy of its parameters (the reference has no 16-bit path; its
 * fp32 path is the yardstick).  The tables are those of choco_params_sgd, except that
 * bufs[s], the momentum buffer, holds lens[s] FP32 elements whatever dtypes[s] is (4-byte
 * aligned); grads[s] has the tensor's dtype.  master (DEVICE, n fp32 elements, never
 * NULL, 4-byte aligned) is laid out as the flat buffer of choco_params_sgd.  The master
 * contract, per element (flat index i, element j of tensor s):
 *     p = master[i]; g = grads[s][j] widened (exact); buf = bufs[s][j]
 *     the lines of choco_params_sgd in apply mode, computed as for an fp32 tensor:
 *     nothing is narrowed between them, a skipped op is skipped, the scalars are
 *     converted as there
 *     master[i] = p_new (in place); bufs[s][j] = buf (fp32, when momentum != 0)
 *     WRITE_PARAMS: params[s][j] = p_new narrowed round-to-nearest-even to dtypes[s],
 *     the narrowing of choco_params_unpack (an fp32 tensor receives p_new itself)
 * so master follows, bit for bit, the trajectory of the fp32 model on the widened
 * gradients, and the 16-bit parameters are its narrowing.  A CHOCO_SGD_F_NOGRAD tensor
 * is passed over: neither its master slice nor its parameter is read or written.
 * Without WRITE_PARAMS the parameters are not touched at all.
 *   mode: CHOCO_SGD_MODE_APPLY, optionally | CHOCO_SGD_MODE_WRITE_PARAMS; GRAD,
 *     WRITE_GRADS and ADD_FLAT are rejected.
 * Only the bytes of the layout's own elements are written.  Every argument is checked
 * before the first launch without a HIP call, as choco_params_sgd checks its own (the
 * NESTEROV rule and sum(lens) == n included), and a bad one returns CHOCO_ERR_INVALID and
 * launches nothing.  A layout takes choco_params_sgd_master_launches(nseg) launches of
 * "param_sgd_master_kernel". */
int choco_params_sgd_master_launches(int32_t nseg);
/* pcode/optim/utils.py:13-47 */
int choco_params_sgd_master(void* const* params, const void* const* grads, void* const* bufs,
                            const int64_t* lens, const int32_t* dtypes, const double* lr,
                            const double* weight_decay, const double* momentum, const double* dampening,
                            const int32_t* flags, int32_t nseg, float* master, int64_t n,
                            int32_t mode, void* stream);

/* ------------------------------------------- all-reduce SGD: the update reads the flat sum
 * The centralized branch of SGD.step (pcode/optim/sgd.py:68-92), plain all-reduce
 * data-parallel SGD, after its all-reduce: unflatten of the averaged gradient and
 * apply_gradient as ONE launch per chunk of tensors.  The tables are those of
 * choco_params_sgd; the gradient side of the update is gsum (DEVICE, n fp32 elements,
 * 4-byte aligned, read only), the flat buffer of the gradients after the all-reduce SUM
 * (sgd.py:78-80), laid out as the flat buffer of choco_params_sgd.  Per element (flat
 * index i, element j of tensor s), every line with exactly one rounding:
 *     a = gsum[i] / (float)divisor      communication.py:186-187, data / world_size: a
 *                                       correctly rounded IEEE division, never a
 *                                       reciprocal multiply; divisor == 1 runs like any other
 *   choco_params_sgd_flatgrad (the fp32 / 16-bit step):
 *     g = a narrowed round-to-nearest-even to dtypes[s]   flatten_grads.unpack(grads), sgd.py:84
 *     the lines of choco_params_sgd in apply mode on params[s][j], g, bufs[s][j]
 *     WRITE_PARAMS: params[s][j] = p_new;  WRITE_GRADS: grads[s][j] = g
 *   choco_params_sgd_master_flatgrad (master, bufs as in choco_params_sgd_master):
 *     g = a, fp32, NOT narrowed (the gain over the 16-bit step)
 *     the lines of choco_params_sgd_master on master[i], g, bufs[s][j] (fp32);
 *     master[i] = p_new
 *     WRITE_PARAMS: params[s][j] = p_new narrowed;  WRITE_GRADS: grads[s][j] = a narrowed
 * bufs[s] is written whenever momentum != 0.  There is no flat output of the new
 * parameters.  grads is an OUTPUT table here: it is read by nobody, may be NULL (as may
 * its entries) without WRITE_GRADS, and the reference's later in-place weight decay on
 * p.grad is not reproduced.  Zero-length tensors are skipped.
 *   mode: CHOCO_SGD_MODE_APPLY | CHOCO_SGD_MODE_WRITE_PARAMS | CHOCO_SGD_MODE_WRITE_GRADS,
 *     the two write bits usable together.
 * Only the bytes of the layout's own elements are written; pointers need their element's
 * alignment only.  Every argument is checked before the first launch without a HIP call,
 * as choco_params_sgd checks its own, and these return CHOCO_ERR_INVALID and launch
 * nothing: CHOCO_SGD_MODE_GRAD; unknown mode bits; a CHOCO_SGD_F_NOGRAD tensor (the flat
 * gradient has no slot to skip); WRITE_GRADS with a NULL grads table or a NULL grad
 * pointer; a divisor that is zero or not finite when cast to float; a NULL or misaligned
 * gsum or master; momentum buffers of the master call that are not 4-byte aligned (16-bit
 * buffers; the Python layer refuses them by dtype); misaligned element pointers.  A layout
 * takes choco_params_sgd_flatgrad_launches(nseg) launches of "param_sgd_flatgrad_kernel"
 * or "param_sgd_master_flatgrad_kernel". */
int choco_params_sgd_flatgrad_launches(int32_t nseg);
/* pcode/optim/sgd.py:68-92 */
int choco_params_sgd_flatgrad(void* const* params, void* const* grads, void* const* bufs,
                              const int64_t* lens, const int32_t* dtypes, const double* lr,
                              const double* weight_decay, const double* momentum,
                              const double* dampening, const int32_t* flags, int32_t nseg,
                              const float* gsum, int64_t n, double divisor, int32_t mode,
                              void* stream);
int choco_params_sgd_master_flatgrad(void* const* params, void* const* grads, void* const* bufs,
                                     const int64_t* lens, const int32_t* dtypes, const double* lr,
                                     const double* weight_decay, const double* momentum,
                                     const double* dampening, const int32_t* flags, int32_t nseg,
                                     const float* gsum, float* master, int64_t n, double divisor,
                                     int32_t mode, void* stream);

/* ------------------------------------------- DGC's optimizer half
 * DGC._apply_gradient (pcode/optim/dgc.py:279-324) is apply_gradient with one more
 * line: after the weight decay and before the momentum, each tensor's d_p is clipped by
 * its own L2 norm (_clip_gradient, dgc.py:254-265, called at :308-310).  _compress then
 * adds d_p to the error-feedback memory (:157) and, with mask_momentum, multiplies the
 * momentum buffers by 1 - mask at the selected positions (:174-182).  Three entry
 * points, each one launch per chunk of tensors, with the tables of choco_params_sgd.
 *
 * choco_params_sqnorm (dgc.py:256, grad.norm(p=2) of the d_p of :302-306):
 *   norms[s] (DEVICE, fp32, nseg of them) = || d_s ||_2 with d = g, or
 *   d = fma((float)wd, p, g) when weight_decay[s] != 0, narrowed for a 16-bit tensor as
 *   choco_params_sgd narrows that line.  NOGRAD and zero-length tensors get 0.  Squares
 *   and sums are fp64 (exact squares, no overflow); the result is sqrt in fp64, rounded
 *   to fp32 and, for a 16-bit tensor, again to that dtype (grad.norm() returns the
 *   gradient's dtype).  The summation order is fixed -- no floating-point atomics: every
 *   (8192-element tile, tensor) pair stores one fp64 partial in the workspace and a
 *   finish launch adds a tensor's partials in ascending order -- so two calls on the
 *   same data give the same bits.  The workspace (choco_params_sqnorm_workspace_size
 *   bytes, 8-byte aligned) needs no initialisation: everything read from it is written
 *   by the same call.  The flags are those of choco_params_sgd (only NOGRAD matters).
 *   Launches: choco_params_sqnorm_launches(nseg), of "param_sqnorm_kernel" per chunk and
 *   one "param_sqnorm_finish_kernel".  Returns CHOCO_ERR_WORKSPACE for a short workspace.
 *
 * choco_params_sgd_clip (dgc.py:279-324): choco_params_sgd with, when norms != NULL,
 *   for every tensor that has a gradient, between the weight decay and the momentum
 *       thr = (float)clip_threshold
 *       c   = norms[s] >= thr ? (1.0f / norms[s]) * thr : 1.0f
 *       d   = c * d
 *   -- torch's `threshold / grad_norm * grad` (dgc.py:263-264): an fp32 comparison, a
 *   correctly rounded reciprocal times the threshold, one fp32 multiply per element
 *   (narrowed for a 16-bit tensor).  A NaN norm compares false (unchanged); an inf norm
 *   gives c = 0.  clip_threshold is clip_grad_val / sqrt(n_nodes), computed by the host
 *   in double (dgc.py:258-262); with norms != NULL it must be finite and > 0 as the
 *   fp32 value the kernel compares with.
 *   CHOCO_SGD_MODE_ADD_FLAT (grad mode only, flat != NULL): flat[i] = flat[i] + d, an
 *   fp32 add -- `_grad = grad + memory` (dgc.py:157) with the error-feedback memory as
 *   the flat buffer.  choco_params_sgd itself rejects the bit.
 *
 * choco_params_mask (dgc.py:174-182): values[k] / indices[k] (DEVICE; global, ascending)
 *   are a segmented selection with k_per_seg[s] (HOST) slots for tensor s; lens, dtypes:
 *   the layout; bufs[s] (HOST table of DEVICE pointers, NULL entries allowed): the
 *   momentum buffer of tensor s, of dtype dtypes[s].  For every slot j of tensor s whose
 *   index i lies in the tensor's flat range:
 *       bufs[s][i - off_s] = buf * 0.0f                  buf.mul_(1 - mask): -3 -> -0,
 *                                                        inf / NaN -> NaN
 *       memory[i] = values[j] + (-values[j])             when memory != NULL (DEVICE, n)
 *   the latter being what choco_sparse_accumulate with -values leaves.  Other indices
 *   are skipped.  Only selected elements are written.  Launches:
 *   choco_params_mask_launches(nseg) of "param_mask_kernel".
 *
 * All three check every argument before the first launch without a HIP call. */
#define CHOCO_SGD_MODE_ADD_FLAT 8
size_t choco_params_sqnorm_workspace_size(int32_t nseg, int64_t n);
int choco_params_sqnorm_launches(int32_t nseg);
/* pcode/optim/dgc.py:254-256, :302-306 */
int choco_params_sqnorm(const void* const* params, const void* const* grads, const int64_t* lens,
                        const int32_t* dtypes, const double* weight_decay, const int32_t* flags,
                        int32_t nseg, int64_t n, float* norms, void* ws, size_t ws_bytes,
                        void* stream);
/* pcode/optim/dgc.py:279-324, :157 */
int choco_params_sgd_clip(void* const* params, const void* const* grads, void* const* bufs,
                          const int64_t* lens, const int32_t* dtypes, const double* lr,
                          const double* weight_decay, const double* momentum,
                          const double* dampening, const int32_t* flags, int32_t nseg, float* flat,
                          int64_t n, int32_t mode, const float* norms, double clip_threshold,
                          void* stream);
int choco_params_mask_launches(int32_t nseg);
/* pcode/optim/dgc.py:174-182 */
int choco_params_mask(void* const* bufs, const int64_t* lens, const int32_t* dtypes,
                      const int64_t* k_per_seg, int32_t nseg, const float* values,
                      const int32_t* indices, int64_t k, float* memory, int64_t n, void* stream);

/* ------------------------------------------- global-norm gradient clipping
 * torch.nn.utils.clip_grad_norm_(model.parameters(), conf.rnn_clip) in front of
 * optimizer.step (pcode/distributed_running_nlp.py:94-97), fused into the batched update:
 * one extra read of the gradients for the norm, a coefficient that never leaves the
 * device, and an update that applies it to g on the load it already does.  Three entry
 * points with the tables of choco_params_sgd.  With CD = coef_dtype, the gradients' common
 * dtype (all bf16 -> bf16, all fp16 -> fp16, any fp32 or any mix -> fp32; the caller says
 * which), every line one torch op with one rounding:
 *     total = the total L2 norm, a value on CD's grid
 *     t = rnd_CD(total + (float)1e-6)
 *     r = rnd_CD(1.0f / t)                 a correctly rounded reciprocal, NOT max_norm / t:
 *                                          torch's `max_norm / tensor` is reciprocal() * max_norm
 *     c = rnd_CD(r * (float)max_norm)
 *     c = c > 1 ? 1 : c                    clamp(max=1.0): a NaN stays NaN
 *     g = rnd_DT(c * g)                    for EVERY element of every tensor with a gradient,
 *                                          also when c == 1: c in fp32 times the widened g,
 *                                          narrowed once to the gradient's dtype DT
 * A NaN total makes every gradient NaN, a +inf total gives c = 0 (signed zeros), a zero
 * total c = 1.  There is no `total >= max_norm` shortcut: a gradient whose norm equals
 * max_norm is still scaled by (1 / (max_norm + 1e-6)) * max_norm < 1.
 *
 * choco_params_gradnorm: out (DEVICE, 2 floats, 4-byte aligned): out[0] = total, out[1] = c.
 *   The total is the one place that differs from torch by design (torch: fp32 per-tensor
 *   norms in its own reduction order, each rounded to the gradient's dtype, then the norm
 *   of the stacked norms): here total = sqrt(sum over all elements of all tensors with a
 *   gradient of g^2), squares and sums in fp64 in a fixed order with no floating-point
 *   atomics, rounded once to fp32 and, for a 16-bit CD, to CD.  CHOCO_SGD_F_NOGRAD and
 *   zero-length tensors contribute 0.  The norm pass is choco_params_sqnorm's
 *   "param_sqnorm_kernel" on the raw gradients (no weight decay), one launch per chunk;
 *   then ONE single-workgroup launch of "param_gradnorm_total_kernel" adds each tensor's
 *   partials in the order choco_params_sqnorm's finish uses, adds the per-tensor fp64 sums
 *   in ascending tensor order, takes the square root in fp64 and evaluates the lines above.
 *   norms (DEVICE, nseg floats, or NULL): norms[s] = the per-tensor norm from the same
 *   partials, bit for bit what choco_params_sqnorm gives at zero weight decay.  Two calls
 *   on the same data give the same bits.  The workspace
 *   (choco_params_gradnorm_workspace_size bytes, 8-byte aligned) needs no initialisation:
 *   everything read from it is written by the same call.  total_in != NULL (DEVICE, one
 *   float) is parity mode: no norm pass, nothing of the layout or the workspace is read
 *   (they may be NULL), total = rnd_CD(*total_in), and norms must be NULL.  The host never
 *   reads the total or the coefficient.  Launches:
 *   choco_params_gradnorm_launches(nseg, pinned) -- chunks of 112 tensors plus one, or 1
 *   when pinned; 0 for nseg <= 0.  Rejected (CHOCO_ERR_INVALID, nothing launched): nseg <= 0;
 *   n outside [0, 2^31); a max_norm that is NaN, negative or not finite as a float; an
 *   unknown coef_dtype; a NULL or misaligned out; a misaligned norms or total_in; norms
 *   with total_in; and, unpinned, null tables, negative or oversumming lengths, lengths
 *   that do not sum to n, unknown dtype or flag bits, misaligned gradient pointers, a NULL
 *   grad without NOGRAD, a NULL or misaligned workspace.  A short workspace returns
 *   CHOCO_ERR_WORKSPACE.
 *
 * choco_params_sgd_gclip: choco_params_sgd with one line in front, g = rnd_DT(c * g) with
 *   c = *coef (DEVICE, one float, 4-byte aligned, e.g. out + 1 of choco_params_gradnorm),
 *   read by the kernel.  Apply mode and grad mode, with or without flat.
 *   CHOCO_SGD_MODE_WRITE_CLIPPED (apply mode only) also stores the clipped g into grads[s]
 *   -- what clip_grad_norm_ leaves in p.grad; without the bit the gradients are not
 *   written in apply mode, as in choco_params_sgd, and flat may then be NULL with the bit
 *   as the only write.  NOGRAD tensors stay a pure pack.  In grad mode with zero weight
 *   decay and momentum and WRITE_GRADS this is the in-place clip itself: g read once,
 *   written once.  Launches: choco_params_sgd_launches(nseg) of "param_sgd_gclip_kernel", an
 *   instantiation of its own: "param_sgd_kernel" carries neither the pointer nor the multiply.
 *
 * choco_params_sgd_master_gclip: choco_params_sgd_master with g = c * g in fp32 in front,
 *   NOT narrowed before the master lines (the caller computes c with CD = fp32: the point
 *   of the master path, and a documented difference from torch for 16-bit models).
 *   WRITE_CLIPPED stores that product narrowed to the gradient's dtype into grads[s].
 *   Launches: choco_params_sgd_master_launches(nseg) of "param_sgd_master_gclip_kernel".
 *
 * Both check every argument before the first launch without a HIP call and reject, in
 * addition to the base function's own list: coef NULL or not 4-byte aligned;
 * WRITE_CLIPPED in grad mode; WRITE_CLIPPED with a NULL grad pointer (a NULL grad without
 * NOGRAD is rejected with or without the bit); CHOCO_SGD_MODE_ADD_FLAT; unknown mode bits. */
#define CHOCO_SGD_MODE_WRITE_CLIPPED 16
size_t choco_params_gradnorm_workspace_size(int32_t nseg, int64_t n);
int choco_params_gradnorm_launches(int32_t nseg, int32_t pinned);
/* pcode/distributed_running_nlp.py:96 */
int choco_params_gradnorm(const void* const* grads, const int64_t* lens, const int32_t* dtypes,
                          const int32_t* flags, int32_t nseg, int64_t n, double max_norm,
                          int32_t coef_dtype, const float* total_in, float* out, float* norms,
                          void* ws, size_t ws_bytes, void* stream);
/* pcode/distributed_running_nlp.py:96-97 */
int choco_params_sgd_gclip(void* const* params, const void* const* grads, void* const* bufs,
                           const int64_t* lens, const int32_t* dtypes, const double* lr,
                           const double* weight_decay, const double* momentum,
                           const double* dampening, const int32_t* flags, int32_t nseg, float* flat,
                           int64_t n, int32_t mode, const float* coef, void* stream);
int choco_params_sgd_master_gclip(void* const* params, const void* const* grads, void* const* bufs,
                                  const int64_t* lens, const int32_t* dtypes, const double* lr,
                                  const double* weight_decay, const double* momentum,
                                  const double* dampening, const int32_t* flags, int32_t nseg,
                                  float* master, int64_t n, int32_t mode, const float* coef,
                                  void* stream);

/* ------------------------------------------- stochastic rounding for bf16 models
 * The third way to train a bf16 model, beside the plain update (every line narrowed
 * round-to-nearest-even: an update below half a bf16 ulp of the parameter is lost, at
 * every step) and fp32 master weights (4 B per parameter more, twice the traffic): the ONE
 * store that writes a bf16 parameter rounds stochastically.  The parameter takes one of its
 * two bf16 neighbours with probabilities that make the expectation exact, so small updates
 * survive in expectation; no extra memory, the plain update's traffic.  The reference has
 * no counterpart.  bf16 only: an fp32 tensor of the same model passes through unchanged, an
 * fp16 tensor is rejected (its subnormal and overflow ranges make the bit trick wrong;
 * fp16 models use loss scaling with master weights).
 *
 * The rounding, with u = the bits of the fp32 value v and r16 in [0, 65536):
 *     (u & 0x7fffffff) >= 0x7f800000 (inf, NaN):  the round-to-nearest narrowing (inf kept,
 *                                                 quiet NaN 0x7fc0)
 *     otherwise:                                  (u + r16) >> 16
 *   A value already representable in bf16 is unchanged for every r16; the result is always
 *   the truncation or its successor in magnitude; P(successor) = low16 / 65536, also across
 *   a binade boundary; +-0 and subnormals need no special case; a finite value above the
 *   largest finite bf16 may round to inf, as rounding up past it does.
 *
 * The bits.  The 16 bits of FLAT element i (its index in the layout, sum(lens[0..s)) + j)
 * are a pure function of (seed, step, i) -- this definition is part of the ABI, and the
 * vector path, the element path, the tile, the chunk of tensors and the tensors' alignment
 * cannot change a result:
 *     mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *              return z ^ (z >> 31)                                  (SplitMix64's output function)
 *     key = mix(seed + (step + 1) * 0xD1B54A32D192ED03)              (the QSGD stream's key rule)
 *     w   = mix(key + ((i >> 2) + 1) * 0x9E3779B97F4A7C15)
 *     r16 = (w >> (16 * (i & 3))) & 0xffff
 *   all in uint64 arithmetic modulo 2^64.  A group of 8 elements at a flat index that is a
 *   multiple of 8 costs two mixes, a cut group's elements one each.  A caller advances
 *   `step` once per optimizer step and keeps `seed`; the same (seed, step) must not round
 *   the same parameter twice.  chocosgd_amd/rounding.py restates both in numpy.
 *
 * Lanes.  A step that rounds more than one value per element (choco_params_adam_sr: the
 * parameter and both moments) draws each from a bit field of its own, lane L of
 * (seed, step, i):
 *     key_0 = key                                                    (the stream above, unchanged)
 *     key_L = mix(key_0 + L * 0xD1B54A32D192ED03)                    L = 1, 2
 *     w, r16 as above with key_L in place of key
 *   Lane 0 is the PARAMETER's lane in every entry point: an update that leaves the
 *   parameters unwritten and a choco_params_unpack_sr of its flat output with the same
 *   (seed, step) agree, and no field is used twice.  rounding.sr_bits(..., lane=) restates it.
 *
 * choco_params_unpack_sr: choco_params_unpack's tables, tiles, walk, 16-byte rule, checks
 *   and launch count; a bf16 tensor receives the stochastic rounding of flat[i] with the
 *   bits of i, an fp32 tensor the copy.  Rejects an fp16 tensor (the message names it) in
 *   addition to choco_params_unpack's list.  Launches: choco_params_launches(nseg) of
 *   "param_unpack_sr_kernel"; "param_pack_kernel" / "param_unpack_kernel" carry none of it.
 *
 * choco_params_sgd_sr: choco_params_sgd in apply mode.  Every line up to d is as there
 *   (fp32 from the widened operands, narrowed round-to-nearest-even after each line), the
 *   momentum buffer is written as there; the parameter line stays fp32,
 *   p_new = fma(-lr, d, p), flat (if not NULL) receives p_new UNROUNDED, and the parameter
 *   (WRITE_PARAMS) receives its stochastic rounding with the bits of its flat index (an
 *   fp32 tensor p_new itself: the same bits as choco_params_sgd).  NOGRAD tensors put p
 *   into flat and are not written.  coef_or_null != NULL is choco_params_sgd_gclip's form,
 *   g = rnd_DT(*coef * g) on the load, with its WRITE_CLIPPED bit; coef is ONE float, so
 *   there is no loss-scaled form.  With WRITE_PARAMS unset and flat given, a later
 *   choco_params_unpack_sr of flat with the same (seed, step) stores what this call would
 *   have: a step that ends in the unpack rounds each parameter once.
 *   Rejects, each with its own message and in addition to choco_params_sgd's list: grad
 *   mode; CHOCO_SGD_MODE_ADD_FLAT (the per-tensor clip's entry point has no such form);
 *   fp16 tensors; a misaligned coef.  Launches: choco_params_sgd_launches(nseg) of
 *   "param_sgd_sr_kernel", instantiations of their own: the kernels above carry neither the
 *   key nor the mixes. */
int choco_params_unpack_sr(void* const* ptrs, const int64_t* lens, const int32_t* dtypes,
                           int32_t nseg, const float* flat, int64_t n, uint64_t seed, uint64_t step,
                           void* stream);
int choco_params_sgd_sr(void* const* params, const void* const* grads, void* const* bufs,
                        const int64_t* lens, const int32_t* dtypes, const double* lr,
                        const double* weight_decay, const double* momentum, const double* dampening,
                        const int32_t* flags, int32_t nseg, float* flat, int64_t n, int32_t mode,
                        const float* coef_or_null, uint64_t seed, uint64_t step, void* stream);

/* ------------------------------------------- dynamic loss scaling
 * torch.amp.GradScaler's unscale_, inf/NaN check, skipped step and scale update for an fp16
 * (or bf16) model, fused into the norm pass and the update above: no pass that rewrites the
 * gradients, no second norm pass for the clip, no host sync.  The gradients the caller
 * hands in are still multiplied by the loss scale.  With scale = *scale_state (DEVICE, one
 * float), CD = coef_dtype as above (fp32 for the master update), every line one rounding:
 *     inv   = (float)(1.0 / (double)scale)
 *     S     = the fp64 sum of squares of the raw gradients, choco_params_gradnorm's own
 *     found = !isfinite(S)                  S is non-finite exactly when a gradient element
 *                                           is: squares are non-negative (no inf - inf) and an
 *                                           fp64 sum of finite fp32 squares cannot overflow.
 *                                           The fp32 total is NOT tested: huge is not overflow
 *     total = rnd_CD((float)sqrt(S) * inv)  the norm of the unscaled gradient
 *     c     = choco_params_gradnorm's lines from total and max_norm;  has_clip == 0: c = 1
 *     gc    = c * inv                       an fp32 product, not narrowed to CD
 *     out   = [total, gc, found ? 1.0f : 0.0f, scale]
 * then torch's _amp_update_scale_ on the device state, in the same launch:
 *     found:  *scale_state = (float)((double)scale * backoff);  *growth_tracker = 0
 *     else:   k = *growth_tracker + 1;  k == interval: s = (float)((double)scale * growth),
 *             stored if finite, and *growth_tracker = 0;  otherwise *growth_tracker = k
 *
 * choco_params_gradnorm_scaled: choco_params_gradnorm's arguments without total_in (a
 *   pinned total has no norm pass to detect an overflow from), and scale_state (DEVICE
 *   float), growth_tracker (DEVICE int32), growth, backoff, interval, has_clip (0: max_norm
 *   is not used), out (DEVICE, FOUR floats).  The same norm pass ("param_sqnorm_kernel")
 *   and ONE launch of "param_gradnorm_scaled_total_kernel", an instantiation of the total
 *   kernel with the same staging and the same ordered additions: workspace and launches
 *   are choco_params_gradnorm_workspace_size(nseg, n) and
 *   choco_params_gradnorm_launches(nseg, 0).  norms (or NULL) receives the per-tensor norms
 *   of the RAW gradients.  Rejected in addition to choco_params_gradnorm's unpinned list: a
 *   NULL or misaligned scale_state or growth_tracker; growth not finite or <= 1; backoff
 *   outside (0, 1); interval < 1; has_clip other than 0 or 1.  max_norm is checked only
 *   with has_clip.
 *
 * choco_params_sgd_scaled / choco_params_sgd_master_scaled: choco_params_sgd_gclip /
 *   choco_params_sgd_master_gclip with out (the four floats above) in place of coef.  The
 *   kernels use gc = out[1] exactly as the gclip kernels use the clip coefficient
 *   (g = rnd_DT(gc * g); master: g = gc * g in fp32, not narrowed; WRITE_CLIPPED stores the
 *   product narrowed: the unscaled, clipped gradient) and read out[2] as one uniform load
 *   per workgroup.  out[2] != 0 skips the step on the device: the master kernel returns
 *   before it touches anything; the plain kernel treats every tensor as a NOGRAD one
 *   (flat = p; no parameter, buffer or gradient is written) and returns at once without a
 *   flat side.  Apply mode only: CHOCO_SGD_MODE_GRAD is rejected, as are ADD_FLAT and a
 *   NULL or misaligned out, on top of the gclip entry points' lists.  Launches:
 *   choco_params_sgd_launches(nseg) of "param_sgd_scaled_kernel" /
 *   "param_sgd_master_scaled_kernel", instantiations of their own: no other kernel
 *   carries the skip test.  CHOCO_SGD_F_FIRST is decided by the host before the launch: a
 *   caller whose step creates momentum buffers reads out[2] first (the one host read) and
 *   does not launch a skipped first step. */
int choco_params_gradnorm_scaled(const void* const* grads, const int64_t* lens,
                                 const int32_t* dtypes, const int32_t* flags, int32_t nseg,
                                 int64_t n, double max_norm, int32_t coef_dtype, float* scale_state,
                                 int32_t* growth_tracker, double growth, double backoff,
                                 int32_t interval, int32_t has_clip, float* out, float* norms,
                                 void* ws, size_t ws_bytes, void* stream);
int choco_params_sgd_scaled(void* const* params, const void* const* grads, void* const* bufs,
                            const int64_t* lens, const int32_t* dtypes, const double* lr,
                            const double* weight_decay, const double* momentum,
                            const double* dampening, const int32_t* flags, int32_t nseg, float* flat,
                            int64_t n, int32_t mode, const float* out, void* stream);
int choco_params_sgd_master_scaled(void* const* params, const void* const* grads, void* const* bufs,
                                   const int64_t* lens, const int32_t* dtypes, const double* lr,
                                   const double* weight_decay, const double* momentum,
                                   const double* dampening, const int32_t* flags, int32_t nseg,
                                   float* master, int64_t n, int32_t mode, const float* out,
                                   void* stream);

/* ------------------------------------------- all-reduce SGD: clip and loss scale in the pack
 * clip_grad_norm_ (pcode/distributed_running_nlp.py:96) and dynamic loss scaling in front of
 * the centralized branch of SGD.step (pcode/optim/sgd.py:68-92), on passes that step does
 * anyway: the pack multiplies by the coefficient on its one load of the gradients, the
 * ranks' overflow flags ride through the all-reduce in ONE extra fp32 slot behind the flat
 * gradient, and the update skips the step on the device where their sum is not zero.  A
 * step is
 *     choco_params_gradnorm_scaled_local      out = [total, gc, found_local, scale]
 *     choco_params_pack_scaled                flat[0..n) = gc * g;  flat[n] = found_local
 *     all-reduce SUM of n + 1 floats          (the caller's)
 *     choco_loss_scale_update                 found = flat[n] != 0; out[2]; the scale update
 *     choco_params_sgd[_master]_flatgrad_scaled   the update, or nothing where found
 * and a clip without loss scaling is choco_params_gradnorm, choco_params_pack_scaled with
 * found_or_null == NULL, the all-reduce of n floats and choco_params_sgd[_master]_flatgrad.
 *
 * choco_params_gradnorm_scaled_local: choco_params_gradnorm_scaled without the
 *   _amp_update_scale_ tail -- the same arguments, checks, norm pass, ordered fp64
 *   additions, workspace and launch count (choco_params_gradnorm_launches(nseg, 0)), the
 *   same four floats in out, every line with the rounding documented there; *scale_state
 *   is read, *growth_tracker is not even read, neither is written: the state must not move
 *   on one rank's local flag, or the ranks would drift apart.  The last launch is
 *   "param_gradnorm_scaled_local_total_kernel", an instantiation of its own.
 *
 * choco_params_pack_scaled: choco_params_pack's arguments, and coef (DEVICE, one float,
 *   4-byte aligned: out + 1 of either gradnorm entry point), found_or_null (DEVICE, one
 *   float, or NULL: out + 2) and round.  c = *coef is one uniform load per workgroup.
 *   Per element, DT the tensor's dtype:
 *     round == 1:  flat[i] = (float)rnd_DT(c * g)   one fp32 multiply of c and the widened g,
 *                                                   narrowed once round-to-nearest-even to DT
 *                                                   and widened: the product the gclip /
 *                                                   scaled update kernels form
 *     round == 0:  flat[i] = c * (float)g           the fp32 product, not narrowed: the
 *                                                   master path (choco_params_sgd_master_gclip)
 *   (for an fp32 tensor the two are the same).  inf and NaN gradients keep their kind (an
 *   inf times c == 0 is a NaN, as in IEEE): a rank that overflowed still packs.  With
 *   found_or_null != NULL flat holds n + 1 floats and exactly one thread of the layout's
 *   FIRST launch stores flat[n] = (*found_or_null != 0) ? 1.0f : 0.0f; with NULL flat holds
 *   n floats and nothing past them is written.  Everything else is choco_params_pack: the
 *   same tiles at absolute flat offsets, 16-byte vectors only where both sides of a group
 *   of 8 elements allow them, zero-length tensors, only the layout's own bytes written, no
 *   device-side table.  Rejected in addition to choco_params_pack's list: coef NULL or
 *   misaligned; a misaligned found_or_null, or one with a NULL flat; round other than 0 or
 *   1.  Launches: choco_params_launches(nseg) of "param_pack_scaled_kernel".
 *
 * choco_loss_scale_update: found_sum (DEVICE, one float: the address of gsum[n] after the
 *   all-reduce), the state arguments of choco_params_gradnorm_scaled, out (DEVICE, four
 *   floats, 4-byte aligned: choco_params_gradnorm_scaled_local's).  ONE launch of one
 *   64-thread workgroup, "loss_scale_update_kernel", one lane of which runs
 *     found  = *found_sum != 0              a NaN counts as found
 *     out[2] = found ? 1.0f : 0.0f          the ranks' common flag
 *     scale  = *scale_state, then the _amp_update_scale_ lines documented above for
 *              choco_params_gradnorm_scaled, bit for bit, with plain stores
 *   Rejected: a NULL or misaligned found_sum, out, scale_state or growth_tracker; growth
 *   not finite or <= 1; backoff outside (0, 1); interval < 1.
 *
 * choco_params_sgd_flatgrad_scaled / choco_params_sgd_master_flatgrad_scaled:
 *   choco_params_sgd_flatgrad / choco_params_sgd_master_flatgrad with gsum of n + 1 floats
 *   (never NULL).  gsum[n] is one uniform load per workgroup; gsum[n] != 0 (a NaN included)
 *   skips the step on the device: the workgroup returns before it touches a parameter, a
 *   momentum buffer, a gradient or the master copy.  Otherwise exactly the lines of the
 *   unscaled entry points on gsum[0..n), with their roundings, their argument checks and
 *   their launch count, choco_params_sgd_flatgrad_launches(nseg), of
 *   "param_sgd_flatgrad_scaled_kernel" / "param_sgd_master_flatgrad_scaled_kernel",
 *   instantiations of their own: the unscaled kernels carry neither the pointer nor the
 *   test.  CHOCO_SGD_F_FIRST stays a host decision: a caller whose step creates momentum
 *   buffers reads gsum[n] after the all-reduce (the one host read) and does not launch a
 *   skipped first step. */
int choco_params_gradnorm_scaled_local(const void* const* grads, const int64_t* lens,
                                       const int32_t* dtypes, const int32_t* flags, int32_t nseg,
                                       int64_t n, double max_norm, int32_t coef_dtype,
                                       const float* scale_state, const int32_t* growth_tracker,
                                       double growth, double backoff, int32_t interval,
                                       int32_t has_clip, float* out, float* norms, void* ws,
                                       size_t ws_bytes, void* stream);
int choco_params_pack_scaled(const void* const* ptrs, const int64_t* lens, const int32_t* dtypes,
                             int32_t nseg, float* flat, int64_t n, const float* coef,
                             const float* found_or_null, int32_t round, void* stream);
int choco_loss_scale_update(const float* found_sum, float* scale_state, int32_t* growth_tracker,
                            double growth, double backoff, int32_t interval, float* out,
                            void* stream);
/* pcode/optim/sgd.py:68-92 behind pcode/distributed_running_nlp.py:96 */
int choco_params_sgd_flatgrad_scaled(void* const* params, void* const* grads, void* const* bufs,
                                     const int64_t* lens, const int32_t* dtypes, const double* lr,
                                     const double* weight_decay, const double* momentum,
                                     const double* dampening, const int32_t* flags, int32_t nseg,
                                     const float* gsum, int64_t n, double divisor, int32_t mode,
                                     void* stream);
int choco_params_sgd_master_flatgrad_scaled(void* const* params, void* const* grads,
                                            void* const* bufs, const int64_t* lens,
                                            const int32_t* dtypes, const double* lr,
                                            const double* weight_decay, const double* momentum,
                                            const double* dampening, const int32_t* flags,
                                            int32_t nseg, const float* gsum, float* master,
                                            int64_t n, double divisor, int32_t mode, void* stream);

/* ------------------------------------------- neighbour-weighted model mix
 * The dense line three decentralized optimizers of the reference share,
 *     sum([hat_r.buffer * neighbors_info[r] for r, hat_r in ...])
 * with what follows it in each, as ONE launch per chunk of tensors:
 *   DCD-PSGD (pcode/optim/dcd_psgd.py:114-125): `- lr * flatten_grads.buffer`, two
 *     roundings; the params are packed beside it for the compressor.
 *       mode GRAD_SUB, flat_out = half params, x_out = packed params
 *   ECD-PSGD (pcode/optim/ecd_psgd.py:118-140): `.add_(grads, alpha=-lr)` (fused),
 *     unpack(params), then (1 - 0.5 t) * old params + 0.5 t * updated.
 *       mode GRAD_FMA | WRITE_PARAMS | EXTRAPOLATE, flat_out = the extrapolated model
 *   D-PSGD (pcode/optim/sgd.py:94-121, _agg(op="weighted") of
 *     pcode/utils/communication.py:271-277), then unpack(params).
 *       mode WRITE_PARAMS (and / or flat_out)
 * srcs[r] (HOST table of nsrc DEVICE pointers): flat fp32 buffers of n elements;
 * weights[r] (HOST doubles) are used as (float)weights[r].  The tensor tables are those
 * of choco_params_sgd: tensor s holds lens[s] elements of dtype dtypes[s] in params[s] and
 * grads[s] and owns flat elements [sum(lens[0..s)), + lens[s]).  Per element (flat index
 * i, element j of tensor s), every line one reference op with one rounding:
 *     m = 0.0f + rn(src[0][i] * w[0])          Python's sum() starts at int 0: -0 -> +0
 *     m = rn(m + rn(src[r][i] * w[r]))         r = 1 .. nsrc - 1, in the given order
 *     GRAD_SUB:     m = rn(m - rn((float)lr * g))       g = grads[s][j] widened
 *     GRAD_FMA:     m = fmaf((float)(-lr), g, m)
 *     WRITE_PARAMS: params[s][j] = m narrowed round-to-nearest-even (the unpack)
 *     EXTRAPOLATE:  x = old params[s][j] widened, read before the store above
 *                   z = rn(rn((float)ext_a * x) + rn((float)ext_b * m))   the un-narrowed m
 *     flat_out[i] = EXTRAPOLATE ? z : m        (if not NULL)
 *     x_out[i]    = old params[s][j] widened   (if not NULL)
 * A zero weight is multiplied, not skipped (inf * 0 = NaN); NaN and inf propagate.
 * flat_out and x_out must not overlap a source or each other: NOT checked.  Each thread
 * reads params before it writes them.  nsrc may be 1 .. 64: more than 8 sources run as
 * successive launches of 8 whose earlier ones leave the running sum in flat_out (then
 * required) and whose last one applies the tail -- the same bits as one sum.  `params`
 * may be NULL when neither the mode nor x_out touches them, `grads` without a GRAD bit;
 * lens = {n}, nseg = 1 is a flat buffer.  Only the bytes of the layout's own elements are
 * written; pointers need their element's alignment only.  Every argument is checked
 * before the first launch without a HIP call -- null srcs / weights / lens / dtypes
 * tables, nsrc outside 1..64, a NULL source, nseg <= 0, negative lengths or lengths that
 * do not sum to n, unknown dtype or mode bits, both GRAD bits, a GRAD bit with a NULL
 * grads table or grad, EXTRAPOLATE / WRITE_PARAMS / x_out with a NULL params table or
 * param, nothing to write, EXTRAPOLATE or nsrc > 8 with flat_out == NULL, misaligned
 * pointers, a non-finite lr with a GRAD bit -- and a bad one returns CHOCO_ERR_INVALID
 * and launches nothing.  A call takes choco_params_mix_launches(nseg, nsrc) launches of
 * "param_mix_kernel" (0 for arguments the call would refuse). */
#define CHOCO_MIX_GRAD_SUB 1
#define CHOCO_MIX_GRAD_FMA 2
#define CHOCO_MIX_WRITE_PARAMS 4
#define CHOCO_MIX_EXTRAPOLATE 8
int choco_params_mix_launches(int32_t nseg, int32_t nsrc);
/* pcode/optim/dcd_psgd.py:114-125, ecd_psgd.py:118-140, sgd.py:94-121 */
int choco_params_mix(const float* const* srcs, const double* weights, int32_t nsrc,
                     void* const* params, const void* const* grads,
                     const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                     double lr, double ext_a, double ext_b, int32_t mode,
                     float* flat_out, float* x_out, int64_t n, void* stream);

/* ------------------------------------------- error-feedback lines
 * The dense lines around the compressors of the reference's two error-feedback
 * optimizers, as ONE launch per chunk of tensors straight between the parameter tensors
 * and a flat fp32 buffer (no pack, no unpack, no temporary):
 *   DeepSqueeze (pcode/optim/deep_squeeze.py:101-108): the pack of the params and
 *     `self.memory.buffer += params_tb.buffer`.
 *       mode ACCUM, flat = memory.buffer
 *   DeepSqueeze (pcode/optim/deep_squeeze.py:125-126): `params_tb.buffer += agg`, unpack.
 *       mode APPLY, flat = the aggregate
 *   EF-signSGD (pcode/optim/ef_sign_sgd.py:218, :113-122): `/= world_size * 1.0`, the pack
 *     of the params, `.add_(-lr * sync_grads_tb.buffer)`, unpack.
 *       mode APPLY | DIV | SCALE, flat = synced_grads
 * The tensor tables are those of choco_params_sgd: tensor s holds lens[s] elements of
 * dtype dtypes[s] in params[s] and owns flat elements [sum(lens[0..s)), + lens[s]).  Per
 * element (flat index i, element j of tensor s, x = params[s][j] widened), every line one
 * reference op with one rounding:
 *     ACCUM:  flat[i] = rn(flat[i] + x)                    the params are read only
 *     APPLY:  a = flat[i]
 *       DIV:    a = rn(a / (float)divisor), flat[i] = a    a correctly rounded IEEE division,
 *                                                          never a reciprocal multiply
 *       SCALE:  a = rn((float)(-lr) * a)                   not written back
 *             params[s][j] = rn(x + a) narrowed round-to-nearest-even: the add is an fp32
 *             add on the widened param, the store narrows once
 * NaN and inf propagate; (-0) + (+0) = +0.  Each thread reads before it writes.  Only the
 * bytes of the layout's own elements are written; pointers need their element's alignment
 * only (16-byte vectors are used where flat and a tensor's side allow them).  Every
 * argument is checked before the first launch without a HIP call -- null params / lens /
 * dtypes tables, nseg <= 0, negative lengths or lengths that do not sum to n, unknown
 * dtype or mode bits, neither or both of ACCUM and APPLY, DIV or SCALE without APPLY,
 * flat == NULL, a NULL param of a non-empty tensor, misaligned pointers, a divisor that is
 * not finite or is zero (as a float) under DIV, a non-finite lr under SCALE -- and a bad
 * one returns CHOCO_ERR_INVALID and launches nothing.  A call takes
 * choco_params_ef_launches(nseg) launches of "param_ef_kernel" (0 for nseg <= 0). */
#define CHOCO_EF_ACCUM 1
#define CHOCO_EF_APPLY 2
#define CHOCO_EF_DIV 4
#define CHOCO_EF_SCALE 8
int choco_params_ef_launches(int32_t nseg);
/* pcode/optim/deep_squeeze.py:101-108, :125-126, ef_sign_sgd.py:113-122, :218 */
int choco_params_ef(void* const* params, const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                    float* flat, int64_t n, int32_t mode, double lr, double divisor, void* stream);

/* ------------------------------------------- consensus evaluation
 * The reference's --evaluate_consensus (pcode/distributed_running_cv.py:110-115, :239-243):
 * the model averaged over the workers (agg_model(copy, op="avg"),
 * pcode/utils/communication.py:114-122) and the L2 distance of this worker's model to it
 * (get_model_difference, pcode/utils/auxiliary.py:18-34), as ONE launch per chunk of tensors
 * plus one total launch, straight from the flat fp32 buffer that the all-reduce SUM of the
 * packed parameters left (no copy of the model, no per-tensor division, subtraction,
 * concatenation or norm).
 * The tensor tables are those of choco_params_sgd: tensor s holds lens[s] elements of dtype
 * dtypes[s] in params[s] (and in avg_out[s]) and owns flat elements [sum(lens[0..s)), +
 * lens[s]).  xsum is laid out as choco_params_pack lays it out and is read only; master, if
 * given, is the flat fp32 master copy of the parameters (choco_params_sgd_master) and is read
 * in their place.  Per element (flat index i, element j of tensor s), every line with exactly
 * one rounding:
 *     a = xsum[i] / (float)divisor                  a correctly rounded IEEE division (the one
 *                                                   of choco_params_sgd_flatgrad), never a
 *                                                   reciprocal multiply
 *     x = master ? master[i] : (float)params[s][j]  widening is exact
 *     d = a - x                                     in fp32: weights2 - weights1
 *     CHOCO_CONS_DIST:       ssd_s += (double)d * d,  ssa += (double)a * a
 *     CHOCO_CONS_WRITE_AVG:  avg_out[s][j] = a narrowed round-to-nearest-even to dtypes[s]
 * avg_out[s] may be params[s] itself (agg_model in place): each element is read before the same
 * thread writes it, so with both bits set the distance is to the values from before the call.
 * The sums are fp64, taken in one fixed order that depends on the layout alone (not on the
 * pointers' alignment nor on how the tensors fall into launches), with no floating-point
 * atomics: per (8192-element tile, tensor) pair one partial -- a span of at most 1024
 * elements by one wave (lane l adds elements l, l + 64, ... of the span, the lanes are joined
 * by the xor butterfly 32, 16, ..., 1), a longer one by the workgroup (the 8-element group at
 * absolute flat offset 8 g belongs to thread (g - first group of the span) mod 256; groups and
 * their elements in ascending order; the butterfly per wave, then ((w0 + w1) + w2) + w3) --
 * then a tensor's partials in ascending tile order, then the tensors in ascending order.
 *     out[0]   = (float)sqrt(sum_s ssd_s)     the distance to the average
 *     out[1]   = (float)sqrt(ssa)             the norm of the average (a relative distance
 *                                             costs nothing more)
 *     dists[s] = (float)sqrt(ssd_s)           if dists != NULL: which layer has drifted
 * A zero-length tensor contributes 0.  NaN and inf propagate.  WRITE_AVG alone reads neither
 * params nor master, needs neither out nor ws and launches no total kernel.  ws holds
 * choco_params_consensus_workspace_size(nseg, n) bytes (0 for nseg <= 0 or n < 0), 8-byte
 * aligned; every word of it that is read is written by the same call.  Nothing is allocated or
 * synchronised.  Pointers need their element's alignment only (16-byte vectors are used where
 * xsum, master and a tensor's sides allow them).  Every argument is checked before the first
 * launch without a HIP call -- unknown mode bits or none, a divisor that is zero or not finite
 * as a float, null lens / dtypes, nseg <= 0, negative lengths or lengths that do not sum to n,
 * unknown dtype codes, a NULL or misaligned xsum, a misaligned master, out or dists, DIST
 * with a NULL out, with a NULL, misaligned or too small ws or, without master, a NULL params
 * table or entry of a non-empty tensor, WRITE_AVG with a NULL avg_out table or entry of a
 * non-empty tensor, dists without DIST, element pointers off their element's alignment --
 * and a bad one returns CHOCO_ERR_INVALID and launches nothing.
 * A call takes choco_params_consensus_launches(nseg, mode) launches (0 for nseg <= 0 or a
 * bad mode): ceil(nseg / 128) of "param_consensus_kernel" -- 128 tensors' table of two
 * pointers, an offset and a dtype each fits the 4 KB of kernel arguments -- and, under
 * DIST, one of "param_consensus_total_kernel". */
#define CHOCO_CONS_DIST 1
#define CHOCO_CONS_WRITE_AVG 2
int choco_params_consensus_launches(int32_t nseg, int32_t mode);
size_t choco_params_consensus_workspace_size(int32_t nseg, int64_t n);
/* pcode/utils/communication.py:114-122, pcode/utils/auxiliary.py:18-34 */
int choco_params_consensus(const void* const* params, void* const* avg_out,
                           const int64_t* lens, const int32_t* dtypes, int32_t nseg,
                           const float* xsum, const float* master /* or NULL */, int64_t n,
                           double divisor, int32_t mode,
                           float* out /* 2 floats */, float* dists /* nseg or NULL */,
                           void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------- Adam / AdamW update fused with the pack
 * torch.optim.Adam.step / AdamW.step (torch.optim.adam._single_tensor_adam; the reference's
 * command line carries --adam_beta_1, --adam_beta_2 and --adam_eps) for nseg parameter
 * tensors as ONE launch per chunk of tensors, with the pack into the flat fp32 buffer, the
 * global-norm clip coefficient and the fp32 master copy in the same pass.  The tables are laid
 * out as those of choco_params_sgd: tensor s holds lens[s] contiguous elements of dtype
 * dtypes[s] in params[s] and grads[s] and owns flat elements [sum(lens[0..s)), + lens[s]);
 * exp_avg[s] and exp_avg_sq[s] are its moments.  step[s] is the tensor's step count AFTER the
 * increment (>= 1).  The hyperparameters are computed in doubles as torch computes them from
 * Python floats, and each is narrowed once to fp32:
 *     bc1 = 1 - beta1**step;  bc2 = 1 - beta2**step
 *     nss = f32(-(lr / bc1));  bs = f32(bc2 ** 0.5);  dec = f32(1 - lr * wd)
 *     w = f32(1 - beta1);  b2 = f32(beta2);  omb2 = f32(1 - beta2);  e = f32(eps)
 * Per element, each line one rounding; rnd is the identity for an fp32 tensor and the
 * round-to-nearest-even narrowing to the tensor's dtype for bf16 / fp16:
 *     g' = g                       (coef given, c = *coef:  g' = rnd(c * g))
 *     if wd != 0:  DECOUPLED:  p  = rnd(p * dec)
 *                  coupled:    g' = rnd(fma(wd, p, g'))
 *     d = g' - m                                     (fp32, not narrowed)
 *     m = w < 0.5 ? rnd(fma(w, d, m)) : rnd(fma(-(1 - w), d, g'))     (both branches of torch's lerp)
 *     v = rnd(v * b2);  t = omb2 * g';  v = rnd(fma(t, g', v))
 *     den = rnd(sqrt(v));  den = rnd(den / bs);  den = rnd(den + e)   (a correctly rounded square
 *                                                    root and division, never a reciprocal multiply)
 *     q = m / den;  p_new = rnd(fma(nss, q, p))
 * A skipped op (weight_decay == 0, tested on the double) is skipped.
 *   choco_params_adam: p, g, m and v have the tensor's dtype.  flat (DEVICE, n fp32 elements,
 *     or NULL) receives p_new; WRITE_PARAMS writes the parameters.  A CHOCO_ADAM_F_NOGRAD tensor
 *     is pack-only: flat = p and nothing else written (passed over without flat).
 *   choco_params_adam_master: p is master[i] (DEVICE, n fp32 elements, never NULL), updated in
 *     place; exp_avg[s] and exp_avg_sq[s] hold FP32 elements whatever dtypes[s] is; g is the
 *     gradient widened (exact); the lines are computed as for an fp32 tensor and nothing is
 *     narrowed between them, the coefficient product included.  WRITE_PARAMS: params[s][j] =
 *     p_new narrowed once to dtypes[s].  A NOGRAD tensor is passed over.
 *   flags[s]: CHOCO_ADAM_F_DECOUPLED (AdamW's weight decay); CHOCO_ADAM_F_FIRST: the tensor has
 *     no state yet, m = v = +0 -- the moments are written and never read;
 *     CHOCO_ADAM_F_NOGRAD (p.grad is None).
 *   mode: CHOCO_SGD_MODE_APPLY, optionally | CHOCO_SGD_MODE_WRITE_PARAMS |
 *     CHOCO_SGD_MODE_WRITE_CLIPPED (needs coef: the product c * g, narrowed, goes back into
 *     grads[s]).
 *   coef_or_null: DEVICE, one float, choco_params_gradnorm's out + 1; one load per workgroup.
 * Only the bytes of the layout's own elements are written.  Distinct tensors, and the flat
 * buffer, must not overlap: this is NOT checked.  Every argument is checked before the first
 * launch without a HIP call, in this order: null tables; nseg and n; the mode bits, a NULL
 * master, nothing to write, the flat / master and coef alignment; then per tensor its length,
 * dtype code and the running sum, unknown flag bits, the pointers' alignment to their element
 * size, a NULL param, a NULL grad without NOGRAD, a NULL moment (FIRST or not: they are
 * written), lr finite and >= 0, the betas in [0, 1), eps finite and >= 0, weight_decay finite
 * and >= 0, step >= 1; last sum(lens) == n.  A bad call returns CHOCO_ERR_INVALID and launches
 * nothing.  A layout takes choco_params_adam_launches(nseg) launches of "param_adam_kernel" /
 * "param_adam_master_kernel" (four pointers a tensor: 54 tensors' table fits the 4 KB of kernel
 * arguments).
 *
 * choco_params_adam_sr: Adam for a bf16 model with stochastic rounding of the parameter AND of
 * both moments (the section "stochastic rounding for bf16 models" above defines the rounding
 * sr(x, r16), the bit stream and its lanes).  Round-to-nearest bf16 moments stall --
 * v * 0.999 is v again -- and a step of lr below half an ulp of p is lost; this keeps both in
 * expectation at choco_params_adam's memory and traffic.  choco_params_adam's arguments,
 * tables, tiles, walk, 16-byte rule, flags, mode bits, coef and launch count, plus
 * (sr_seed, sr_step).  For a BF16 tensor, element j at flat index i:
 *     p, g, m, v are loaded as bf16 and widened to fp32 (FIRST: m = v = +0, not read);
 *     the lines above run as for an fp32 tensor (choco_params_adam_master's arithmetic):
 *       every line fp32, nothing narrowed between the lines, the same host scalars, with
 *       coef g' = c * g not narrowed; den and q use the UNROUNDED v_new and m_new;
 *     exp_avg[s][j]    = sr(m_new, lane 1's r16 of i)
 *     exp_avg_sq[s][j] = sr(v_new, lane 2's r16 of i)
 *     params[s][j]     = sr(p_new, lane 0's r16 of i)        (WRITE_PARAMS only)
 *     flat[i]          = p_new, the unrounded fp32            (flat != NULL)
 *     grads[s][j]      = rnd_bf16(c * g), round-to-nearest    (WRITE_CLIPPED only)
 *   With WRITE_PARAMS unset and flat given, a later choco_params_unpack_sr of flat with the
 *   same (seed, step) stores the parameters this call would have.  For an F32 tensor the
 *   update is choco_params_adam's, bit for bit, and no bits are drawn; a NOGRAD tensor is
 *   pack-only as there.  Rejects, in addition to choco_params_adam's list and at the place
 *   of the per-tensor flag check: an F16 tensor ("fp16 has no stochastic rounding").
 *   Launches: choco_params_adam_launches(nseg) of "param_adam_sr_kernel", an instantiation
 *   of its own: the two kernels above carry neither the key nor the mixes. */
#define CHOCO_ADAM_F_DECOUPLED 1
#define CHOCO_ADAM_F_FIRST 2
#define CHOCO_ADAM_F_NOGRAD 4
int choco_params_adam_launches(int32_t nseg);
/* torch.optim.adam._single_tensor_adam */
int choco_params_adam(void* const* params, const void* const* grads, void* const* exp_avg,
                      void* const* exp_avg_sq, const int64_t* lens, const int32_t* dtypes,
                      const double* lr, const double* beta1, const double* beta2, const double* eps,
                      const double* weight_decay, const double* step, const int32_t* flags,
                      int32_t nseg, float* flat /* or NULL */, int64_t n, int32_t mode,
                      const float* coef_or_null, void* stream);
int choco_params_adam_master(void* const* params, const void* const* grads, void* const* exp_avg,
                             void* const* exp_avg_sq, const int64_t* lens, const int32_t* dtypes,
                             const double* lr, const double* beta1, const double* beta2,
                             const double* eps, const double* weight_decay, const double* step,
                             const int32_t* flags, int32_t nseg, float* master, int64_t n,
                             int32_t mode, const float* coef_or_null, void* stream);
int choco_params_adam_sr(void* const* params, const void* const* grads, void* const* exp_avg,
                         void* const* exp_avg_sq, const int64_t* lens, const int32_t* dtypes,
                         const double* lr, const double* beta1, const double* beta2, const double* eps,
                         const double* weight_decay, const double* step, const int32_t* flags,
                         int32_t nseg, float* flat /* or NULL */, int64_t n, int32_t mode,
                         const float* coef_or_null, uint64_t sr_seed, uint64_t sr_step, void* stream);

/* ------------------------------------------- fused gossip step + compress
 * ParallelCHOCO_V.step's update_params_from_neighbor -> compress sequence
 * (pcode/optim/parallel_choco_v.py:116-142 -> :229-240, optim/utils.py:67-72) in
 * the codec's own passes: the FIRST full pass of the compressor reads x, memory
 * and xhat, writes x_new = x + (float)gamma * (memory - xhat) back into x (bit-
 * identical to choco_gossip_step) and compresses d = x_new - xhat, so the step
 * costs one pass of 12 B read + 4 B written per element less than
 * choco_gossip_step followed by the compressor.  Outputs, workspaces, plans and
 * alignment rules are those of the matching non-gossip entry point.  Paths with
 * no full first pass (random-k, which gathers k elements; pinned-norm QSGD; tiny
 * or k == n top-k) run choco_gossip_step first. */
int choco_gossip_topk_compress(float* x, const float* memory, const float* xhat, float gamma,
                               int64_t n, int64_t k, float* out_val, int32_t* out_idx,
                               void* ws, size_t ws_bytes, void* stream);
/* The fused step + top-k + self-message fold: xhat[idx] += val, and memory[idx] +=
 * (float)weight * val when fold_memory != 0 (the ordering rule of
 * choco_topk_compress_accumulate). */
int choco_gossip_topk_compress_accumulate(float* x, float* memory, float* xhat, float gamma,
                                          int64_t n, int64_t k, float* out_val, int32_t* out_idx,
                                          int32_t fold_memory, float weight,
                                          void* ws, size_t ws_bytes, void* stream);
int choco_gossip_topk_compress_segmented(float* x, const float* memory, const float* xhat, float gamma,
                                         const int64_t* plan_dev, const int64_t* plan_host, int32_t nseg,
                                         float* out_val, int32_t* out_idx,
                                         void* ws, size_t ws_bytes, void* stream);
int choco_gossip_randk_compress_segmented(float* x, const float* memory, const float* xhat, float gamma,
                                          const int64_t* plan_dev, const int64_t* plan_host, int32_t nseg,
                                          uint64_t seed, uint64_t offset, int32_t is_biased,
                                          float* out_val, int32_t* out_idx,
                                          void* ws, size_t ws_bytes, void* stream);
int choco_gossip_sign_compress(float* x, const float* memory, const float* xhat, float gamma,
                               int64_t n, const int64_t* seg_off, int32_t nseg,
                               int32_t* packed, float* l1_norms,
                               void* ws, size_t ws_bytes, void* stream);
int choco_gossip_sign_compress_range(float* x, const float* memory, const float* xhat, float gamma, int64_t n,
                                     const int64_t* seg_off, int32_t nseg, int64_t w0, int64_t w1, int32_t finish,
                                     int32_t* packed, float* l1_norms, void* ws, size_t ws_bytes, void* stream);
int choco_gossip_qsgd_compress(float* x, const float* memory, const float* xhat, float gamma,
                               int64_t n, const int64_t* seg_off, int32_t nseg,
                               int32_t q, int32_t is_biased, uint64_t seed, uint64_t offset,
                               uint8_t* packed, float* norms_out, float* dense_out,
                               void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------- profiling hooks
 * Optional: when enabled, the dominant kernel of each op is launched with a
 * pair of hipEvents attached to the dispatch itself (hipExtLaunchKernelGGL), so
 * the elapsed time is the kernel's own, not the queue ahead of it (the bench's
 * roofline source; agrees with rocprofv3 --kernel-trace). */
int choco_profile_enable(int32_t on);
/* Accumulated (sum of ms, count) of the named kernel since the last reset,
 * after synchronising its events.  Names: "topk_stream", "sign_pack",
 * "qsgd_quantize", "sparse_accumulate", ... */
/* Time only the launches whose name is in the comma-separated list `names`
 * (NULL or "" = all); events are reused. */
int choco_profile_filter(const char* names);
int choco_profile_read(const char* name, double* total_ms, int64_t* count);
int choco_profile_reset(void);
/* Launches of the named kernel since the library was loaded, counted whether or not
 * profiling is enabled (diagnostic: the bench's per-step warm-hit rates, e.g. how many
 * "topk_bounds" sample launches or "topk_seg_hist" cold passes a step took). */
int64_t choco_launch_count(const char* name);

#ifdef __cplusplus
}
#endif

#endif /* CHOCO_CODEC_H_ */
