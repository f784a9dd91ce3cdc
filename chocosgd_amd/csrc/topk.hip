// Top-k / random-k sparsification for the CHOCO gossip step on MI355X.
//
// Replaces SparsificationCompressor.get_top_k / get_random_k
// (reference dl_code/pcode/utils/sparsification.py:18-54) and the per-tensor
// compress loop of CHOCOSparsificationCompressor (parallel_choco_v.py:229-260).
//
// Exact semantics (every path below produces bit-identical results):
//   T  = k-th largest key(d) (key = |d| bits, see choco_common.h)
//   out = { i : key_i > T }  U  { the (k - #{key > T}) lowest i with key_i == T },
//   emitted as (d_i, i) in ascending i.
//
// Fast path for large n ("pipeline"); the delta is read from HBM ONCE, in two
// kernels:
//   K2 topk_stream  : one 16-wave workgroup per tile, one per CU.  Prologue:
//                     every workgroup histograms the same 32K-element strided
//                     sample in LDS (while its first load batch is in flight)
//                     and derives the candidate floor s_lo (#{key >= s_lo} >= k
//                     with a ~6 sigma margin) and the "sure" ceiling s_hi
//                     (#{key >= s_hi} < k); [s_lo, s_hi) is split into 255
//                     key-buckets of width 2^shift.  Stream: per float4 row the
//                     wave ballots candidates (key >= s_lo) and appends them in
//                     index order to an LDS ring flushed to the chunk's slots of
//                     the candidate buffer.  Tile end: the "maybe" keys
//                     (key < s_hi) are bucket-counted and counting-sorted into a
//                     per-tile side list; per-tile bucket suffix counts go to a
//                     [tile][256] table and to kNRep replicated global totals.
//   K34 topk_finish : one workgroup per tile.  Each finds the bucket j* of the
//                     k-th key from the totals, copies every tile's bucket-j*
//                     keys (a few thousand) into LDS, radix-selects T and the tie
//                     quota r exactly, scans all tiles' output offsets, and then
//                     compacts its own tile's candidates into the final
//                     ascending-index output.
//   If the sample's guess was off (too few candidates, T in the "sure" range,
//   bucket j* larger than LDS, or a side list overflowed), every K34 workgroup
//   joins an exact radix select over the full input instead (wide.h: a ticketed
//   queue of per-tile passes; correct, ~5 reads of the input).
// Small n (<= kSmallN) uses an exact radix select (block_topk_exact) in one
// workgroup; per-tensor (segmented) calls are batched in topk_seg.hip.
#include "choco_common.h"
#include "select.h"
#include "wide.h"

#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <unordered_map>

namespace choco {

constexpr int kK2Threads = 1024;          // 16 waves, each a contiguous range of the tile
constexpr int kK2Waves = kK2Threads / 64;
constexpr int kK2Unroll = 8;            // float4 rows per wave per load batch (8 KiB in flight)
constexpr int64_t kK2Target = 256;      // tiles per launch: one workgroup per CU, no two tiles compete on a CU
constexpr int64_t kTileQuant = (int64_t)kK2Waves * kK2Unroll * 256;   // 32768 elements
static_assert(kK2Target <= 1024, "K34 keeps one tile per thread");
// Elements a wave claims at a time (LDS counter): one load batch.
constexpr int64_t kChunk = 256 * kK2Unroll;
static_assert(kTileQuant % kChunk == 0, "chunk geometry");
constexpr int kMaybeCap = 65536;        // side-list capacity per tile (maybe keys)
constexpr int kNBucket = 256;           // 255 "maybe" buckets + 1 "sure"
constexpr int kNMaybe = kNBucket - 1;
// Replicas of the global bucket totals (K2's tile ends add to replica b & 3; every K34
// workgroup reads all of them in its first round trip).  Same-box A/B, round 6
// (profiles/r06_ab_summary.txt item 11): 16 replicas K34 11.48-11.66 us, 4 replicas 11.07-11.38 us.
constexpr int kNRep = 4;
constexpr int kMCap = 16384;            // max keys of bucket j* selected in LDS
constexpr int kK4Threads = 1024;
constexpr int64_t kSmallN = 65536;
constexpr int kExactThreads = 1024;

// Diagnostic phase stamps (tools/stamps.py; never in the product build).
#ifndef CHOCO_STAMPS
#define CHOCO_STAMPS 0
#endif
#if CHOCO_STAMPS
constexpr int kStampSlots = 40960;
__device__ unsigned long long g_stamps[kStampSlots][4];
#define STAMP(slot, j)                                                      \
  do {                                                                      \
    if (threadIdx.x == 0) g_stamps[(slot)][(j)] = wall_clock64();           \
  } while (0)
#define WSTAMP(slot, j)                                                      \
  do {                                                                      \
    if (lane_id() == 0) g_stamps[(slot)][(j)] = wall_clock64();             \
  } while (0)
#else
#define STAMP(slot, j) \
  do {                 \
  } while (0)
#define WSTAMP(slot, j) \
  do {                  \
  } while (0)
#endif

enum TileMode { kTakeNone = 0, kTakeAll = 1, kTakePartial = 2 };

// Candidate window of one call: keys >= s_lo are candidates, [s_lo, s_hi) is
// split into 255 "maybe" buckets of width 2^shift, keys >= s_hi are "sure".
// Written by K1 (cold call: the sample) or by the previous call's K34 (warm
// call: the previous exact threshold and bucket counts, margin m / 1024 of k),
// for the (n, k) it was made for.
struct TopkBounds {
  uint32_t s_lo, s_hi, shift, m1024;  // m1024 = 0: a sample / fallback window (no count targets)
  int64_t n, k;
  uint32_t valid, pad;
};

// The control block at the start of every top-k workspace.  Per-call state is
// double-buffered by call parity `par` (the host keeps the call count of each
// workspace, topk_warm_*): call c reads bounds[par], adds into G[par] and
// overflow[par]; its K2 zeroes G[par ^ 1] / overflow[par ^ 1] for call c + 1
// and its K34 writes bounds[par ^ 1] -- no kernel of call c touches state that
// another kernel of call c still reads.
struct TopkCtrl {
  uint32_t status;                               // sticky error bits (kStatus*), read by the host lazily
  uint32_t fallbacks;                            // calls that took the exact fallback (diagnostic counter)
  uint32_t cold_left;                            // warm-host calls still to sample their window in K2 (backoff)
  uint32_t backoff;                              // the next warm miss doubles it and starts a cold run that long
  uint32_t k2_samples;                           // calls whose K2 took its window from its own sample (diagnostic)
  // drift tracking (K34, workgroup 0): the previous call's exact k-th key, the key drift
  // between the two calls before it, the window the previous call prepared for this one
  // (the "shadow": on a cold run, would it have held this call's k-th key?) and for which
  // (n, k), and the cold-run calls in a row whose k-th key the shadow held
  uint32_t t_prev;
  uint32_t d_prev;                               // int32 bits
  uint32_t sh_lo, sh_hi, sh_nk, sh_hits;
  uint32_t d_cand;                               // the drift window_drift proposed last call (int32 bits)
  uint32_t d_trust;                              // calls in a row whose proposed drift beat the static key
  uint32_t pad0[3];
  uint32_t overflow[2];                          // bit 0: a side list overflowed; bit 1: take the exact fallback
  uint32_t pad1[14];
  TopkBounds bounds[2];
  uint32_t pad2[16];
  uint32_t G[2][kNRep][kNBucket];                // replicated bucket suffix totals
};
static_assert(offsetof(TopkCtrl, status) == CHOCO_TOPK_STATUS_OFFSET, "status word at the documented offset");
static_assert(offsetof(TopkCtrl, fallbacks) == CHOCO_TOPK_FALLBACKS_OFFSET, "fallback counter at the documented offset");
static_assert(offsetof(TopkCtrl, cold_left) == CHOCO_TOPK_COLD_LEFT_OFFSET, "cold-run word at the documented offset");
static_assert(offsetof(TopkCtrl, k2_samples) == CHOCO_TOPK_K2_SAMPLES_OFFSET, "K2 sample counter at the documented offset");
static_assert(offsetof(TopkCtrl, backoff) == CHOCO_TOPK_DIAG_BACKOFF_OFFSET, "backoff at the documented offset");
static_assert(offsetof(TopkCtrl, t_prev) == CHOCO_TOPK_DIAG_T_PREV_OFFSET, "t_prev at the documented offset");
static_assert(offsetof(TopkCtrl, d_prev) == CHOCO_TOPK_DIAG_D_PREV_OFFSET, "d_prev at the documented offset");
static_assert(offsetof(TopkCtrl, sh_lo) == CHOCO_TOPK_DIAG_SH_LO_OFFSET, "sh_lo at the documented offset");
static_assert(offsetof(TopkCtrl, sh_hi) == CHOCO_TOPK_DIAG_SH_HI_OFFSET, "sh_hi at the documented offset");
static_assert(offsetof(TopkCtrl, sh_nk) == CHOCO_TOPK_DIAG_SH_NK_OFFSET, "sh_nk at the documented offset");
static_assert(offsetof(TopkCtrl, sh_hits) == CHOCO_TOPK_DIAG_SH_HITS_OFFSET, "sh_hits at the documented offset");
static_assert(offsetof(TopkCtrl, d_cand) == CHOCO_TOPK_DIAG_D_CAND_OFFSET, "d_cand at the documented offset");
static_assert(offsetof(TopkCtrl, d_trust) == CHOCO_TOPK_DIAG_D_TRUST_OFFSET, "d_trust at the documented offset");
static_assert(offsetof(TopkCtrl, overflow) == CHOCO_TOPK_DIAG_OVERFLOW_OFFSET, "overflow words at the documented offset");
static_assert(offsetof(TopkCtrl, bounds) == CHOCO_TOPK_DIAG_BOUNDS_OFFSET, "windows at the documented offset");
static_assert(sizeof(TopkBounds) == CHOCO_TOPK_DIAG_BOUNDS_STRIDE, "one window per documented stride");
static_assert(offsetof(TopkBounds, s_lo) == CHOCO_TOPK_DIAG_BOUNDS_S_LO && offsetof(TopkBounds, s_hi) == CHOCO_TOPK_DIAG_BOUNDS_S_HI &&
                  offsetof(TopkBounds, shift) == CHOCO_TOPK_DIAG_BOUNDS_SHIFT &&
                  offsetof(TopkBounds, m1024) == CHOCO_TOPK_DIAG_BOUNDS_M1024 && offsetof(TopkBounds, n) == CHOCO_TOPK_DIAG_BOUNDS_N &&
                  offsetof(TopkBounds, k) == CHOCO_TOPK_DIAG_BOUNDS_K && offsetof(TopkBounds, valid) == CHOCO_TOPK_DIAG_BOUNDS_VALID,
              "window fields at the documented offsets");
constexpr uint32_t kNoCandKey = 0x7F800000u;   // window that admits only inf / NaN keys (invalid bounds)

// The self-message part of CHOCOSparsificationCompressor.uncompress (parallel_choco_v.py:
// 307-310) folded into the emission of the message: hat[i] += q (hat != nullptr) and
// mem[i] += w * q (mem != nullptr; two roundings, as choco_sparse_accumulate) for every
// emitted (q, i).  hat may be the x_hat the call compresses against: nothing reads it
// once emission starts (K34 emits from the candidate slots; the exact fallback's emission
// phase starts after every read phase, and each element is read before it is written).
struct Fold {
  float* hat;
  float* mem;
  float w;
  __host__ __device__ bool on() const { return hat != nullptr || mem != nullptr; }
};
CHOCO_DEV void fold_apply(const Fold& f, int64_t i, float q) {
  if (f.hat) f.hat[i] = f.hat[i] + q;
  if (f.mem) f.mem[i] = f.mem[i] + f.w * q;
}

struct TopkLayout {
  int64_t n;
  uint32_t tile, nb, side_cap;
  size_t off_ctrl, off_cum, off_cntw, off_side, off_cval, off_cidx, off_wide, off_gcnt, off_thist, off_tinfo, total;
};

// Tile = ceil(n / kK2Target) rounded up to 32768 elements: one tile per CU, all
// resident at once (few tiles also keep K3's table reads short).  A tile's side
// list holds its "maybe" keys (kMaybeCap, LDS-staged): the sample's margin is
// ~12 sqrt(k/n / 65536) of the elements (0.5 % at k = 1 %, 1.5 % at k = 10 %,
// 3.3 % at k = 50 % -> 13K of a 390K-element tile).
static TopkLayout topk_layout(int64_t n) {
  TopkLayout L{};
  L.n = n;
  int64_t tile = (n + kK2Target - 1) / kK2Target;
  tile = std::max<int64_t>(kTileQuant, (tile + kTileQuant - 1) / kTileQuant * kTileQuant);
  L.tile = (uint32_t)tile;
  L.nb = (uint32_t)((n + tile - 1) / tile);
  L.side_cap = (uint32_t)std::min<int64_t>(kMaybeCap, tile);
  // A fixed header at the start of every top-k workspace (any n): the control block
  // and the exact-fallback queue (WideCtrl), whose counters rely on starting zeroed --
  // calls of different n sharing one workspace must not move them.
  size_t o = 0;
  L.off_ctrl = o;  o += align_up(sizeof(TopkCtrl), 256);
  L.off_wide = o;  o += kWideBytes;
  L.off_cum = o;   o += align_up((size_t)L.nb * kNBucket * 4, 256);
  L.off_cntw = o;  o += align_up((size_t)L.nb * (tile / kChunk) * 4, 256);   // per-chunk candidate counts
  L.off_side = o;  o += align_up((size_t)L.nb * L.side_cap * 4, 256);
  L.off_cval = o;  o += align_up((size_t)L.nb * tile * 4, 256);   // candidate values, chunk slot ranges
  L.off_cidx = o;  o += align_up((size_t)L.nb * tile * 4, 256);   // ... and indices
  L.off_gcnt = o;  o += align_up((size_t)L.nb * 8, 256);              // ... its per-tile (#>T, #==T)
  L.off_thist = o; o += align_up((size_t)L.nb * 512 * 4, 256);        // ... and per-tile last-digit histograms
  L.off_tinfo = o; o += align_up((size_t)L.nb * 4, 256);              // per tile: candidates (compact) or ~0 (spilled)
  L.total = o;
  return L;
}

template <int MODE, bool XH>
__global__ __launch_bounds__(kExactThreads) void topk_exact_kernel(
    const float* __restrict__ x, const float* __restrict__ xh, int64_t n, int64_t k, uint64_t seed,
    float scale, float* __restrict__ out_val, int32_t* __restrict__ out_idx, int64_t idx_base) {
  __shared__ ExactSmem sm;
  Src<MODE, XH> src{x, xh, seed};
  block_topk_exact<kExactThreads>(src, n, k, scale, out_val, out_idx, idx_base, sm);
}

// k >= n (ratio 0): every element, in index order -- a plain multi-workgroup copy.
template <bool XH>
__global__ __launch_bounds__(256) void topk_all_kernel(const float* __restrict__ x, const float* __restrict__ xh,
                                                      int64_t n, float scale, float* __restrict__ out_val,
                                                      int32_t* __restrict__ out_idx, int64_t idx_base) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    out_val[i] = (XH ? x[i] - xh[i] : x[i]) * scale;
    out_idx[i] = (int32_t)(i + idx_base);
  }
}

// ----------------------------------------------------------------------------
// Sample bounds: the prologue of K2, computed identically by every workgroup
//
// 128 runs of 256 contiguous elements (32768 keys, 128 KiB -- after the first
// workgroup of an XCD misses, an L2 hit for the other 31) are histogrammed in
// LDS, two levels: coarse key >> 20 (2048 bins), then bits 19..9 inside the two
// coarse bins that hold the R_lo-th / R_hi-th largest sample keys.  s_lo is
// rounded down and s_hi up to 512 keys.  Every workgroup reads the same sample
// and counts it the same way, so all of them derive the same (s_lo, s_hi)
// without a grid-wide hand-off.  Both bounds are heuristics that K34 verifies
// (G[0] >= k, G[sure] < k); any k/n works.
// ----------------------------------------------------------------------------
constexpr int kSampleRuns = 64;  // runs of 256 contiguous elements
constexpr int kSampleN = kSampleRuns * 256;                  // 16384 at 64 runs
constexpr int kK1Threads = 1024;                              // the bounds kernel: one workgroup
constexpr int kSampleLoads = kSampleRuns * 64 / kK1Threads;  // float4 per thread (4)
static_assert(kSampleLoads * kK1Threads == kSampleRuns * 64, "sample geometry");

struct SampleRanks {
  uint32_t lo, hi;  // 1-based ranks from the top; 0 = none
  uint32_t sub;     // rank in the 1024-key subsample whose bin floors F (below rank lo w.h.p.)
};

// Ranks of the candidate floor / sure ceiling in the sample (~6 sigma margins),
// computed on the host (they depend on n and k only) and passed to K2.
static SampleRanks sample_ranks(int64_t n, int64_t k) {
  const double m = (double)kSampleN;
  const double e = (double)k / (double)n * m;
  const double sd = sqrt(e);
  const double rlo = ceil(e + 6.0 * sd + 4.0);
  const double rhi = floor(e - 6.0 * sd - 4.0);
  SampleRanks r;
  r.lo = rlo <= m ? (uint32_t)rlo : 0u;  // 0: every key is a candidate
  r.hi = rhi >= 1.0 ? (uint32_t)rhi : 0u;  // 0: no key is "sure"
  const double es = (double)r.lo * (1024.0 / m);
  r.sub = (uint32_t)std::min(1024.0, ceil(es + 4.0 * sqrt(es) + 4.0));
  return r;
}

// Per-call bucket geometry: [s_lo, s_hi) is split into 255 "maybe" buckets of
// width 2^shift; keys >= s_hi are "sure" (bucket 255).
struct Buckets {
  int64_t n;
  uint32_t s_lo, s_hi, shift;
  float s_lo_f;  // s_lo as a float: !(|v| < s_lo_f) is a superset test of key >= s_lo
  uint64_t seed;
};

CHOCO_DEV Buckets make_buckets(uint32_t s_lo, uint64_t s_hi_est, uint64_t seed, uint32_t nmaybe = kNMaybe) {
  const uint64_t width = s_hi_est > s_lo ? s_hi_est - s_lo : 1;
  uint32_t shift = 0;
  while (((uint64_t)nmaybe << shift) < width) ++shift;
  uint64_t s_hi = (uint64_t)s_lo + ((uint64_t)nmaybe << shift);
  if (s_hi > 0xFFFFFFFFull) s_hi = 0xFFFFFFFFull;
  Buckets bk;
  bk.n = 0;
  bk.s_lo = s_lo;
  bk.s_hi = (uint32_t)s_hi;
  bk.shift = shift;
  bk.s_lo_f = __uint_as_float(s_lo);  // NaN when s_lo is a NaN key: then every lane is staged
  bk.seed = seed;
  return bk;
}

CHOCO_DEV Buckets make_buckets_from(uint32_t s_lo, uint32_t s_hi, uint32_t shift, uint64_t seed) {
  Buckets bk;
  bk.n = 0;
  bk.s_lo = s_lo;
  bk.s_hi = s_hi;
  bk.shift = shift;
  bk.s_lo_f = __uint_as_float(s_lo);
  bk.seed = seed;
  return bk;
}

template <bool XH, bool GS>
CHOCO_DEV void load_sample(const float* __restrict__ x, const float* __restrict__ xh, const float* __restrict__ mem,
                           int64_t n, float4 (&s)[kSampleLoads], float4 (&h)[kSampleLoads],
                           float4 (&m)[kSampleLoads]) {
  const int64_t stride4 = ((n - 256) / (kSampleRuns - 1)) >> 2;  // float4 between run starts
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // one 1 KiB buffer resource per run (wave-uniform base): dword-aligned 16-B
  // buffer loads, so x / xh need only 4-byte alignment (unaligned segments)
#pragma unroll
  for (int j = 0; j < kSampleLoads; ++j) {
    const int64_t run0 = (int64_t)(w * kSampleLoads + j) * stride4 * 4;  // wave w: runs 4w .. 4w+3
    s[j] = ld_buf4<false>(buf_rsrc(x + run0, 1024u), 16u * (uint32_t)lane);
    if (XH) h[j] = ld_buf4<false>(buf_rsrc(xh + run0, 1024u), 16u * (uint32_t)lane);
    if (GS) m[j] = ld_buf4<false>(buf_rsrc(mem + run0, 1024u), 16u * (uint32_t)lane);
  }
}

// ----------------------------------------------------------------------------
// K2: sample prologue + streaming candidate compaction, one 16-wave workgroup
// per tile, one per CU
//
// Measured (tools/probe_position.hip, probe_balance.hip): when two or more
// workgroups share a CU, the one dispatched first streams first and the last
// ones finish alone with few bytes in flight; with ONE workgroup per CU every
// workgroup finishes within ~10 % of the others.  LDS use (> 80 KiB) enforces
// that placement.  Inside the workgroup the CU's issue arbiter favours older
// waves, so waves claim kChunk-element chunks through an LDS counter.
//
// Each wave keeps its next load batch in flight while it works on the current
// one (two register buffers A/B, 8 KiB each).  The first batch is issued
// before the sample is counted, so the HBM is busy during the prologue.
//
// Candidates stay ON CHIP until the stream is over (tools/probe_wmix.hip: a
// trickle of stores inside a saturated 400 MB read costs ~0.5 us per MB
// written -- 3-4x its byte share, HBM read/write turnaround -- while LDS work
// of the same shape costs nothing measurable):
//   * per float4 row a wave decides which LANES hold a candidate (|v| >= s_lo,
//     one ballot) and appends those lanes' float4 + first index ("entries", ~3
//     of 64 lanes per row at k = 1 %) to a per-wave LDS ring;
//   * every 64 entries are expanded with the exact key test into (value, index)
//     pairs in the wave's region of an LDS pair buffer (chunk order), and the
//     maybe keys (s_lo <= key < s_hi) are counted into the tile's bucket
//     histogram;
//   * a wave whose region is full writes further pairs straight to their
//     chunk's global slots (dense inputs / large k: correct, slower);
//   * at the end of the tile every chunk's LDS pairs leave in one burst to the
//     chunk's global slots, and the maybe keys are counting-sorted into the
//     tile's side list on the way.
// ----------------------------------------------------------------------------
constexpr int kEnt = 128;  // entry ring per wave (flush at 64: <= 63 + 64 pending)
constexpr int kPairsPerWave = 640;  // LDS pair region per wave (~2x the k = 1 % share)
constexpr int kSideLds = kK2Waves * kEnt * 4;  // maybe keys sorted in LDS at tile end (in the dead entry ring)
constexpr int kMaxTileChunks = (int)((int64_t(1) << 31) / kK2Target / kChunk);  // tile <= 2^31 / 256 elements
constexpr int kCPT = kMaxTileChunks / kK4Threads;  // chunk counts per K34 thread
static_assert(kCPT * kK4Threads == kMaxTileChunks, "chunk table");

constexpr int kListPerWave = 256;  // sample keys >= F kept per wave (prologue)
struct SampleHist {
  uint32_t coarse[4][2048];  // 4 copies (lane & 3): same-bin lanes of one atomic instruction serialize
  uint32_t fine[2][2048];
  uint32_t list[kK2Waves][kListPerWave];
};

struct StreamSmem {
  float4 ent_v[kK2Waves][kEnt];   // staged lanes: the float4 row slice
  uint32_t ent_i[kK2Waves][kEnt]; // ... and the index of its first element
  float4 trash_v[64];             // per-lane sink of the branch-free batch writes (shared, never read)
  uint32_t trash_i[64];
  union {
    uint2 pairs[kK2Waves * kPairsPerWave];  // (value bits, index) per candidate, per-wave regions
    SampleHist sh;                          // the prologue's sample window (cold calls only)
  } u;
  uint32_t cmeta[kMaxTileChunks];  // per chunk: LDS start | LDS count << 16
  uint32_t ccnt[kMaxTileChunks + 1];  // per chunk: candidates; at tile end their exclusive prefix
  uint32_t hist[kNBucket];        // maybe-key bucket counts, then counting-sort cursors
  uint32_t cnt[kK2Waves];
  uint32_t scratch[40];
  uint32_t bc[8];
  uint32_t next_chunk;            // the tile's chunk counter (waves claim chunks)
  uint32_t spill;                 // some wave spilled pairs to global (tile end)
};

// Unconditional float4 loads of kK2Unroll rows (no branch around a load: the
// compiler's vmcnt accounting stays exact and all rows are in flight together),
// through buffer resources based at the tile start (tile-relative byte offsets).
// A chunk that does not exist is "loaded" from kNoChunk, out of the resource's
// range: zeros, no memory access -- so the prefetch issued after a wave's last
// chunk does not hold the tile's end for a round trip (the registers it targets
// are reused there, which waits for it).
// The once-read stream uses non-temporal loads: they do not allocate in the
// 256 MB Infinity Cache, so a previous kernel's dirty lines there are not
// evicted (and written back) in the middle of the stream.  Measured in the
// bench step (the previous step's sparse accumulate leaves ~120 MB dirty):
// K2 130 -> 83 us; back to back, cold caches: 89.6 -> 82.9 us.
constexpr uint32_t kNoChunk = 0x80000000u;  // > any tile's bytes (tile <= 2^31 / 256 elements)
struct TileRsrc {
  __amdgpu_buffer_rsrc_t x, xh, m;  // m: the gossip step's memory (GS only)
};

template <bool XH>
CHOCO_DEV void load_rows_full(const TileRsrc& ts, uint32_t boff, int lane, float4 (&r)[kK2Unroll]) {
#pragma unroll
  for (int u = 0; u < kK2Unroll; ++u) r[u] = ld_buf4<true>(ts.x, boff + (u * 256 + 4 * lane) * 4);
  if (XH) {
#pragma unroll
    for (int u = 0; u < kK2Unroll; ++u) {
      const float4 h = ld_buf4<true>(ts.xh, boff + (u * 256 + 4 * lane) * 4);
      r[u].x -= h.x; r[u].y -= h.y; r[u].z -= h.z; r[u].w -= h.w;
    }
  }
}

// The fused gossip step on one load batch (GS): x, memory and xh rows in flight
// together, x_new = x + gamma (memory - xh) stored back in place (a chunk that
// does not exist loads zeros and its stores are dropped: out of the resource's
// range), and r = x_new - xh.  No cross-chunk prefetch: three streams per wave
// keep 24 KiB in flight, 16 waves per CU are plenty to cover the latency.
CHOCO_DEV void gossip_rows(const TileRsrc& ts, uint32_t boff, int lane, float gamma, float4 (&r)[kK2Unroll]) {
  float4 M[kK2Unroll], H[kK2Unroll];
#pragma unroll
  for (int u = 0; u < kK2Unroll; ++u) r[u] = ld_buf4<true>(ts.x, boff + (u * 256 + 4 * lane) * 4);
#pragma unroll
  for (int u = 0; u < kK2Unroll; ++u) M[u] = ld_buf4<true>(ts.m, boff + (u * 256 + 4 * lane) * 4);
#pragma unroll
  for (int u = 0; u < kK2Unroll; ++u) H[u] = ld_buf4<true>(ts.xh, boff + (u * 256 + 4 * lane) * 4);
#pragma unroll
  for (int u = 0; u < kK2Unroll; ++u) {
    const float4 xn = gossip4(r[u], M[u], H[u], gamma);
    st_buf4<1>(ts.x, boff + (u * 256 + 4 * lane) * 4, xn);
    r[u] = sub4(xn, H[u]);
  }
}

CHOCO_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Per-wave state (wave-uniform).
struct WaveAcc {
  uint32_t estaged, eflushed;  // entry ring of the current chunk: appended / expanded
  uint32_t staged;             // candidates of the current chunk
  uint32_t lstart, lcnt;       // the current chunk's pairs kept in LDS: region offset, count
  uint32_t lfill;              // pairs in the wave's LDS region
  uint32_t cand;               // candidates, whole tile
};

// Expand ring entries [eflushed, eflushed + nent) (nent <= 64, one per lane)
// with the exact key test into the current chunk's candidates [staged, ..):
// into the wave's LDS region while it has room, else straight to the chunk's
// global slots (then for the rest of the chunk, so the LDS part stays a prefix
// of the chunk's run).  Maybe keys are counted into the bucket histogram.
template <int MODE, bool XH, class SM>
CHOCO_DEV void flush_entries(const Src<MODE, XH>& src, SM& sm, int w, int lane, WaveAcc& a, uint32_t nent,
                             float* __restrict__ ov, uint32_t* __restrict__ oi, const Buckets& bk) {
  wave_sync();
  const bool have = (uint32_t)lane < nent;
  const uint32_t slot = (a.eflushed + lane) & (kEnt - 1);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  uint32_t i0 = 0;
  if (have) {
    if (MODE == kData) v = sm.ent_v[w][slot];
    i0 = sm.ent_i[w][slot];
  }
  float vv[4] = {v.x, v.y, v.z, v.w};
  bool ok[4];
  uint32_t nc = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t key = MODE == kData ? fkey(vv[q]) : (rank_hash(bk.seed, i0 + q) >> 1);
    ok[q] = have && (int64_t)i0 + q < bk.n && key >= bk.s_lo;
    nc += ok[q] ? 1u : 0u;
    if (ok[q] && key < bk.s_hi) atomicAdd(&sm.hist[(key - bk.s_lo) >> bk.shift], 1u);
  }
  if (MODE == kHash) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (ok[q]) vv[q] = src.val((int64_t)i0 + q);
  }
  const uint64_t b0 = ballot(nc & 1u), b1 = ballot(nc & 2u), b2 = ballot(nc & 4u);
  const uint32_t tot = (uint32_t)(__popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2));
  const uint32_t pre = mask_prefix(b0) + 2 * mask_prefix(b1) + 4 * mask_prefix(b2);
  if (tot != 0u) {  // wave-uniform
    const bool lds = a.lcnt == a.staged && a.lfill + tot <= (uint32_t)kPairsPerWave;  // LDS part still a prefix
    uint32_t p = pre;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (ok[q]) {
        if (lds) {
          sm.u.pairs[w * kPairsPerWave + a.lfill + p] = make_uint2(__float_as_uint(vv[q]), i0 + q);
        } else {
          ov[a.staged + p] = vv[q];
          oi[a.staged + p] = i0 + q;
        }
        ++p;
      }
    }
    if (lds) {
      a.lfill += tot;
      a.lcnt += tot;
    }
    a.staged += tot;
  }
  a.cand += tot;
  a.eflushed += nent;
}

// One float4 row per lane (256 elements per wave): stage the lanes that hold a
// candidate.  The float test !(|v| < s_lo_f) is a superset of key >= s_lo (NaN
// passes); the flush applies the exact test.
template <int MODE, bool XH, bool GUARD, class SM>
CHOCO_DEV void process_row(const Src<MODE, XH>& src, const float4 v4, int64_t i, int64_t cend, SM& sm,
                           int w, int lane, WaveAcc& a, float* __restrict__ ov, uint32_t* __restrict__ oi,
                           const Buckets& bk) {
  bool any = false;
  if (MODE == kData) {
    const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) any |= (!GUARD || i + c < cend) && !(fabsf(vv[c]) < bk.s_lo_f);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) any |= (!GUARD || i + c < cend) && src.key_of(i + c, 0.f) >= bk.s_lo;
  }
  const uint64_t M = ballot(any);
  if (M == 0ull) return;  // wave-uniform: no candidate lane in this row
  if (any) {
    const uint32_t slot = (a.estaged + mask_prefix(M)) & (kEnt - 1);
    if (MODE == kData) sm.ent_v[w][slot] = v4;
    sm.ent_i[w][slot] = (uint32_t)i;
  }
  a.estaged = __builtin_amdgcn_readfirstlane(a.estaged + (uint32_t)__popcll(M));
  if (a.estaged - a.eflushed >= 64u) flush_entries(src, sm, w, lane, a, 64u, ov, oi, bk);
}

// Eight full rows (one load batch) as ONE branch-free block, so the compiler can
// interleave the rows' dependent compare -> ballot -> prefix -> LDS-store chains.
// Lanes without a candidate store to a trash slot.  If the batch could overflow
// the entry ring (dense inputs), rows take the per-row path instead.
// `reload` is called once A is dead (the batch is staged in LDS), BEFORE the ring
// is expanded: the wave's next load batch then flies during the expansion, so
// both of its buffers are in flight for most of the batch's work.
template <bool XH, class SM, class RL>
CHOCO_DEV void process_batch(const Src<kData, XH>& src, const float4 (&A)[kK2Unroll], int64_t base, int64_t cend,
                             SM& sm, int w, int lane, WaveAcc& a, float* __restrict__ ov,
                             uint32_t* __restrict__ oi, const Buckets& bk, RL&& reload) {
  bool any[kK2Unroll];
  uint64_t M[kK2Unroll];
  uint32_t add = 0;
#pragma unroll
  for (int u = 0; u < kK2Unroll; ++u) {
    any[u] = !(fabsf(A[u].x) < bk.s_lo_f) || !(fabsf(A[u].y) < bk.s_lo_f) || !(fabsf(A[u].z) < bk.s_lo_f) ||
             !(fabsf(A[u].w) < bk.s_lo_f);
    M[u] = ballot(any[u]);
    add += (uint32_t)__popcll(M[u]);
  }
  add = __builtin_amdgcn_readfirstlane(add);
  if (add == 0u) {
    reload();
    return;
  }
  if (a.estaged - a.eflushed + add <= (uint32_t)kEnt) {
    uint32_t run = a.estaged;
#pragma unroll
    for (int u = 0; u < kK2Unroll; ++u) {
      const uint32_t slot = (run + mask_prefix(M[u])) & (kEnt - 1);
      float4* pv = any[u] ? &sm.ent_v[w][slot] : &sm.trash_v[lane];
      uint32_t* pi = any[u] ? &sm.ent_i[w][slot] : &sm.trash_i[lane];
      *pv = A[u];
      *pi = (uint32_t)(base + u * 256 + 4 * lane);
      run += (uint32_t)__popcll(M[u]);
    }
    a.estaged = __builtin_amdgcn_readfirstlane(run);
    reload();
#pragma unroll 1
    while (a.estaged - a.eflushed >= 64u) flush_entries(src, sm, w, lane, a, 64u, ov, oi, bk);
  } else {
#pragma unroll
    for (int u = 0; u < kK2Unroll; ++u)
      process_row<kData, XH, false>(src, A[u], base + u * 256 + 4 * lane, cend, sm, w, lane, a, ov, oi, bk);
    reload();
  }
}

template <int MODE, bool XH, class SM>
CHOCO_DEV void process_rows_hash(const Src<MODE, XH>& src, int64_t base, int64_t cend, SM& sm, int w,
                                 int lane, WaveAcc& a, float* __restrict__ ov, uint32_t* __restrict__ oi,
                                 const Buckets& bk) {
#pragma unroll
  for (int u = 0; u < kK2Unroll; ++u)
    process_row<MODE, XH, false>(src, make_float4(0.f, 0.f, 0.f, 0.f), base + u * 256 + 4 * lane, cend, sm, w,
                                 lane, a, ov, oi, bk);
}

template <class SM>
CHOCO_DEV uint32_t claim_chunk(SM& sm, int lane) {
  uint32_t c = 0;
  if (lane == 0) c = atomicAdd(&sm.next_chunk, 1u);
  return __builtin_amdgcn_readfirstlane(c);
}

// The sample's candidate floor s_lo (the R_lo-th largest key, rounded down) and
// sure ceiling s_hi (the R_hi-th largest, rounded up) -- every workgroup, same
// sample, same answer.  LDS atomics cost ~16 cycles per wave instruction however
// few lanes collide (measured: 32 per thread ~3 us per pass), so the fast path
// counts few keys: a 1024-key subsample (one key per thread) in a coarse
// histogram (16 runs spread over the buffer) gives a floor F safely below the R_lo-th largest key, the ~3 % of
// keys >= F are compacted into per-wave LDS lists with ballots, and one fine
// histogram of those (2048 bins over [F, subsample max]) resolves both ranks.
// If a list overflows or fewer than R_lo keys pass F, the full two-level
// histogram of all keys runs instead.
struct BoundsSmem {
  SampleHist sh;
  uint32_t scratch[40];
  uint32_t bc[8];
};

template <class BS>
CHOCO_DEV void sample_bounds_full(const uint32_t (&kk)[kSampleLoads * 4], const SampleRanks& R, int lane,
                                  BS& sm, uint32_t& s_lo, uint64_t& s_hi_est) {
  const int tid = threadIdx.x;
  for (int i = tid; i < 6 * 2048; i += kK1Threads) (&sm.sh.coarse[0][0])[i] = 0u;
  if (tid < 8) sm.bc[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSampleLoads * 4; ++j) atomicAdd(&sm.sh.coarse[lane & 3][kk[j] >> 20], 1u);
  __syncthreads();
  for (int i = tid; i < 2048; i += kK1Threads)
    sm.sh.coarse[0][i] += sm.sh.coarse[1][i] + sm.sh.coarse[2][i] + sm.sh.coarse[3][i];
  __syncthreads();
  block_find_two(sm.sh.coarse[0], R.lo, R.hi, sm.scratch, sm.bc);
  const uint32_t c_lo = sm.bc[0], r_lo = sm.bc[1], c_hi = sm.bc[2], r_hi = sm.bc[3];
#pragma unroll
  for (int j = 0; j < kSampleLoads * 4; ++j) {
    const uint32_t cb = kk[j] >> 20, fb = (kk[j] >> 9) & 2047u;
    if (R.lo && cb == c_lo) atomicAdd(&sm.sh.fine[0][fb], 1u);
    if (R.hi && cb == c_hi) atomicAdd(&sm.sh.fine[1][fb], 1u);
  }
  __syncthreads();
  block_find_two(sm.sh.fine[0], R.lo ? r_lo : 0u, 0u, sm.scratch, sm.bc + 4);
  block_find_two(sm.sh.fine[1], R.hi ? r_hi : 0u, 0u, sm.scratch, sm.bc + 6);
  s_lo = R.lo ? ((c_lo << 20) | (sm.bc[4] << 9)) : 0u;                                  // rounded down
  s_hi_est = R.hi ? (uint64_t)((c_hi << 20) | (sm.bc[6] << 9)) + 512u : 0x80000000ull;  // rounded up
}

template <class BS>
CHOCO_DEV void sample_bounds(const uint32_t (&kk)[kSampleLoads * 4], const SampleRanks& R, int lane, int w,
                             BS& sm, uint32_t& s_lo, uint64_t& s_hi_est) {
  const int tid = threadIdx.x;
  if (R.lo == 0) {  // every key is a candidate
    s_lo = 0u;
    s_hi_est = 0x80000000ull;
    return;
  }
  // ---- stage A: subsample floor F and subsample maximum
  uint32_t* coarse = sm.sh.coarse[0];
  uint32_t* fine = sm.sh.fine[0];
  for (int i = tid; i < 2048; i += kK1Threads) { coarse[i] = 0u; fine[i] = 0u; }
  if (tid < 8) sm.bc[tid] = 0;
  __syncthreads();
  atomicAdd(&coarse[kk[0] >> 20], 1u);  // subsample: every thread's first key (wave w: run 4w)
  __syncthreads();
  STAMP(30001, 0);
  block_find_two(coarse, R.sub, 1u, sm.scratch, sm.bc);
  STAMP(30001, 1);
  const uint32_t F = sm.bc[0] << 20;
  const uint32_t top = (sm.bc[2] + 1u) << 20;          // above the subsample maximum's bin
  const uint32_t width = top - F;                      // >= 2^20
  const int shiftB = max(0, 32 - (int)__clz(width - 1u) - 11);
  // ---- keys >= F -> this wave's list (ballot compaction, no atomics)
  uint32_t cnt = 0;  // wave-uniform
#pragma unroll
  for (int j = 0; j < kSampleLoads * 4; ++j) {
    const bool p = kk[j] >= F;
    const uint64_t M = ballot(p);
    if (M != 0ull) {
      const uint32_t pos = cnt + mask_prefix(M);
      if (p && pos < (uint32_t)kListPerWave) sm.sh.list[w][pos] = kk[j];
      cnt += (uint32_t)__popcll(M);
    }
  }
  STAMP(30001, 2);
  const uint32_t mine = min(cnt, (uint32_t)kListPerWave);
  for (uint32_t i = lane; i < mine; i += 64) {
    const uint32_t key = sm.sh.list[w][i];
    atomicAdd(&fine[min((key - F) >> shiftB, 2047u)], 1u);
  }
  if (lane == 0) {
    atomicAdd(&sm.bc[6], cnt);
    if (cnt > (uint32_t)kListPerWave) atomicOr(&sm.bc[7], 1u);
  }
  __syncthreads();
  STAMP(30001, 3);
  const uint32_t total = sm.bc[6], over = sm.bc[7];
  __syncthreads();
  if (over != 0u || total < R.lo) {  // workgroup-uniform
    sample_bounds_full(kk, R, lane, sm, s_lo, s_hi_est);
    return;
  }
  STAMP(30002, 0);
  block_find_two(fine, R.lo, R.hi, sm.scratch, sm.bc);
  STAMP(30002, 1);
  const uint32_t j_lo = sm.bc[0], j_hi = sm.bc[2];
  s_lo = F + (j_lo << shiftB);                                                     // rounded down
  s_hi_est = (R.hi == 0u || j_hi == 2047u) ? 0x80000000ull : (uint64_t)F + ((uint64_t)(j_hi + 1u) << shiftB);
}


// K1: the sample bounds, ONE 1024-thread workgroup.  Measured: computed inside
// the stream kernel's prologue by every workgroup they cost ~8-13 us of idle
// HBM per call (the first prefetch batch cannot cover them: 255 CUs issuing
// 8 KiB per wave at once block in the load-issue path until the flood
// drains, so the histogram work does not start until it has); as their own
// tiny kernel they take a few us and the stream kernel starts streaming at
// once.
// GS: the sample is of d = (x + gamma (memory - xh)) - xh (K2 writes x_new later).
template <bool XH, bool GS>
__global__ __launch_bounds__(kK1Threads) void topk_bounds_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ xh, int64_t n, int64_t k,
                                                                 uint32_t par, SampleRanks ranks,
                                                                 TopkCtrl* __restrict__ ctrl, Gossip gs) {
  __shared__ BoundsSmem sm;
  STAMP(30000, 0);
  const int lane = lane_id(), w = threadIdx.x >> 6;
  // this call's bucket totals and overflow flag start from zero (K2 adds to them);
  // a cold call makes no assumption about what an earlier call left
  for (int i = threadIdx.x; i < kNRep * kNBucket; i += kK1Threads) (&ctrl->G[par][0][0])[i] = 0u;
  if (threadIdx.x == 0) ctrl->overflow[par] = 0u;
  float4 s[kSampleLoads], sh[kSampleLoads], sm_[kSampleLoads];
  load_sample<XH, GS>(x, xh, gs.mem, n, s, sh, sm_);
  uint32_t kk[kSampleLoads * 4];
#pragma unroll
  for (int j = 0; j < kSampleLoads; ++j) {
    float4 v = s[j];
    if (GS) v = gossip4(v, sm_[j], sh[j], gs.gamma);
    if (XH) { v.x -= sh[j].x; v.y -= sh[j].y; v.z -= sh[j].z; v.w -= sh[j].w; }
    kk[4 * j + 0] = fkey(v.x); kk[4 * j + 1] = fkey(v.y); kk[4 * j + 2] = fkey(v.z); kk[4 * j + 3] = fkey(v.w);
  }
  STAMP(30000, 1);
  uint32_t s_lo;
  uint64_t s_hi_est;
  sample_bounds(kk, ranks, lane, w, sm, s_lo, s_hi_est);
  const Buckets bk = make_buckets(s_lo, s_hi_est, 0);
  // Degenerate input: more than a quarter of the sample lies in the "maybe" range (an
  // all-equal buffer, a huge tie cluster at the k-th magnitude): the bucket select
  // cannot succeed, so flag it (overflow bit 1) -- K2 then skips the candidate stream
  // and K34 goes straight to the exact fallback.
  uint32_t nmaybe = 0;
#pragma unroll
  for (int j = 0; j < kSampleLoads * 4; ++j) nmaybe += (kk[j] >= bk.s_lo && kk[j] < bk.s_hi) ? 1u : 0u;
  uint32_t tot_maybe;
  block_excl_scan(nmaybe, sm.scratch, &tot_maybe);
  if (threadIdx.x == 0) {
    TopkBounds& B = ctrl->bounds[par];
    B.s_lo = bk.s_lo;
    B.s_hi = bk.s_hi;
    B.shift = bk.shift;
    B.m1024 = 0u;  // a sample window: no count targets to measure the next call's drift against
    B.n = n;
    B.k = k;
    B.valid = 1u;
    if (tot_maybe > (uint32_t)(kSampleN / 4)) ctrl->overflow[par] = 2u;
  }
  STAMP(30000, 2);
}

// K1's window computed inside K2's prologue (a warm-host call on a cold run): every
// workgroup takes the same sample and finds the same bounds.  The sample's loads queue
// behind the first prefetch of 255 CUs, so this costs ~10 us against K1's ~7 -- paid
// only on the calls of a cold run, never on a warm call.
struct SampleView {
  SampleHist& sh;
  uint32_t* scratch;
  uint32_t* bc;
};
template <bool XH, bool GS>
CHOCO_DEV Buckets prologue_sample(const float* __restrict__ x, const float* __restrict__ xh, const Gossip& gs,
                                  int64_t n, const SampleRanks& ranks, int lane, int w, SampleView& sv, bool* deg) {
  static_assert(kK2Threads == kK1Threads, "the K1 sample geometry");
  float4 s[kSampleLoads], sh[kSampleLoads], sm_[kSampleLoads];
  load_sample<XH, GS>(x, xh, gs.mem, n, s, sh, sm_);
  uint32_t kk[kSampleLoads * 4];
#pragma unroll
  for (int j = 0; j < kSampleLoads; ++j) {
    float4 v = s[j];
    if (GS) v = gossip4(v, sm_[j], sh[j], gs.gamma);
    if (XH) { v.x -= sh[j].x; v.y -= sh[j].y; v.z -= sh[j].z; v.w -= sh[j].w; }
    kk[4 * j + 0] = fkey(v.x); kk[4 * j + 1] = fkey(v.y); kk[4 * j + 2] = fkey(v.z); kk[4 * j + 3] = fkey(v.w);
  }
  uint32_t s_lo;
  uint64_t s_hi_est;
  sample_bounds(kk, ranks, lane, w, sv, s_lo, s_hi_est);
  const Buckets bk = make_buckets(s_lo, s_hi_est, 0);
  uint32_t nmaybe = 0;
#pragma unroll
  for (int j = 0; j < kSampleLoads * 4; ++j) nmaybe += (kk[j] >= bk.s_lo && kk[j] < bk.s_hi) ? 1u : 0u;
  uint32_t tot_maybe;
  block_excl_scan(nmaybe, sv.scratch, &tot_maybe);
  *deg = tot_maybe > (uint32_t)(kSampleN / 4);
  return bk;
}

// Random-k (MODE kHash): keys are uniform on [0, 2^31) and (s_lo, s_hi) come from
// the binomial tails (host), passed as hs_lo / hs_hi.
// GS (kData, XH): the fused gossip step -- the stream reads x, memory and xh,
// writes x_new back and selects on d = x_new - xh.
template <int MODE, bool XH, bool GS = false>
__global__ __launch_bounds__(kK2Threads, 4) void topk_stream_kernel(
    const float* __restrict__ x, const float* __restrict__ xh, int64_t n, int64_t k, uint32_t tile, uint32_t nb,
    uint32_t par, uint32_t side_cap, uint64_t seed, uint32_t hs_lo, uint64_t hs_hi, TopkCtrl* __restrict__ ctrl,
    uint32_t* __restrict__ cum_tab, uint32_t* __restrict__ cntw, uint32_t* __restrict__ side,
    float* __restrict__ cval, uint32_t* __restrict__ cidx, uint32_t* __restrict__ tinfo, Gossip gs,
    SampleRanks ranks, uint32_t sample_if_cold) {
  static_assert(!GS || (MODE == kData && XH), "the gossip step needs x_hat and data keys");
  __shared__ StreamSmem sm;
  STAMP(1024 + blockIdx.x, 0);
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int w = tid >> 6;
  const int64_t b = blockIdx.x;
  constexpr int64_t kStep = 256 * kK2Unroll;
  static_assert(kChunk == kStep, "a chunk is one load batch");
  constexpr bool kTwoChunks = MODE == kData && !XH;  // A and B hold the next two chunks
  const uint32_t nchunk = tile / (uint32_t)kChunk;
  Src<MODE, XH> src{x, xh, seed};
  // tile-relative byte offset of a full chunk's first / second batch, or kNoChunk
  const int64_t tlen = min((int64_t)tile, n - b * (int64_t)tile);
  const TileRsrc ts{buf_rsrc(x + b * (int64_t)tile, (uint32_t)(tlen * 4)),
                    buf_rsrc((XH ? xh : x) + b * (int64_t)tile, (uint32_t)(tlen * 4)),
                    buf_rsrc((GS ? gs.mem : x) + b * (int64_t)tile, (uint32_t)(tlen * 4))};
  auto batch0 = [&](uint32_t c) -> uint32_t {
    return (c < nchunk && (int64_t)(c + 1) * kChunk <= tlen) ? c * (uint32_t)kChunk * 4u : kNoChunk;
  };

  // ---- prologue: the window words K1 / the previous call left in the control block
  // are read FIRST, then the wave's first chunk w (and with one-batch chunks its second,
  // w + 16) goes out.  vmcnt retires in order: read behind the first batches (~67 MB
  // requested GPU-wide at once), the window arrived after all of them (~10 us) and no
  // wave could start its first chunk or refill its buffers until then.
  uint32_t c = (uint32_t)w;
  float4 A[kK2Unroll], B[kK2Unroll];
  Buckets bk;
  TopkBounds W{};
  uint32_t cold_left = 0, ovf_now = 0;
  if constexpr (MODE == kData) {
    // ONE vector load, lane i <-> word i (bounds words 0..8, cold_left, overflow): issued
    // before the batch, waited for (by the compiler, at the first readlane) behind it.
    // (Separate scalar loads made the batch wait for their lgkmcnt; separate vector loads
    // got a register reused as an address of the batch, which then waited for them.)
    static_assert(offsetof(TopkBounds, valid) == 32, "bounds words 0..8: s_lo, s_hi, shift, m1024, n, k, valid");
    const uint32_t* bw = reinterpret_cast<const uint32_t*>(&ctrl->bounds[par]);
    const uint32_t* wsrc = lane < 9 ? bw + lane : (lane == 9 ? &ctrl->cold_left : &ctrl->overflow[par]);
    const uint32_t wl = __hip_atomic_load(wsrc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::: "memory");  // (the batch's loads stay behind the window load)
    if (!GS) load_rows_full<XH>(ts, batch0(c), lane, A);
    if (kTwoChunks) load_rows_full<XH>(ts, batch0(c + kK2Waves), lane, B);
    asm volatile("" ::: "memory");
    W.s_lo = __builtin_amdgcn_readlane(wl, 0);
    W.s_hi = __builtin_amdgcn_readlane(wl, 1);
    W.shift = __builtin_amdgcn_readlane(wl, 2);
    W.m1024 = __builtin_amdgcn_readlane(wl, 3);
    W.n = (int64_t)(((uint64_t)__builtin_amdgcn_readlane(wl, 5) << 32) | __builtin_amdgcn_readlane(wl, 4));
    W.k = (int64_t)(((uint64_t)__builtin_amdgcn_readlane(wl, 7) << 32) | __builtin_amdgcn_readlane(wl, 6));
    W.valid = __builtin_amdgcn_readlane(wl, 8);
    cold_left = __builtin_amdgcn_readlane(wl, 9);
    ovf_now = __builtin_amdgcn_readlane(wl, 10);
  }
  // the NEXT call's bucket totals and overflow word start from zero (no kernel of
  // this call reads them: this call's are G[par] / overflow[par])
  for (int i = (int)b * kK2Threads + tid; i < kNRep * kNBucket; i += (int)nb * kK2Threads)
    (&ctrl->G[par ^ 1u][0][0])[i] = 0u;
  if (b == 0 && tid == 0) ctrl->overflow[par ^ 1u] = 0u;
  if constexpr (MODE == kData) {
    // this call's window: K1's sample (cold call), the previous call's (warm call), or --
    // when the host skipped K1 but the window is stale or a warm miss put this workspace
    // on a cold run (cold_left, set by K34) -- a sample taken here by every workgroup.
    // Never with the fused gossip step (GS): the workgroups write x_new as they stream, so
    // a workgroup that starts late could sample some x_new and derive other buckets than
    // the rest (a wrong selection, undetected); the host runs K1 instead (launch_topk).
    bool ok = W.valid != 0u && W.n == n && W.k == k && W.shift < 32u;
    bool degenerate = false;
    if (!GS && sample_if_cold && (!ok || cold_left != 0u)) {  // grid-uniform
      SampleView sv{sm.u.sh, sm.scratch, sm.bc};
      bool deg;
      const Buckets sb = prologue_sample<XH, GS>(x, xh, gs, n, ranks, lane, w, sv, &deg);
      __syncthreads();  // the union is the pairs region again
      bk = make_buckets_from(sb.s_lo, sb.s_hi, sb.shift, seed);
      ok = true;
      degenerate = deg;
      if (b == 0 && tid == 0) {  // K34 reads this call's window from the control block
        TopkBounds& B = ctrl->bounds[par];
        B.s_lo = sb.s_lo;
        B.s_hi = sb.s_hi;
        B.shift = sb.shift;
        B.m1024 = 0u;
        B.n = n;
        B.k = k;
        B.valid = 1u;
        if (deg) atomicOr(&ctrl->overflow[par], 2u);
        ctrl->k2_samples += 1u;  // (this call's only writer of the word)
      }
    } else {
      bk = ok ? make_buckets_from(W.s_lo, W.s_hi, W.shift, seed) : make_buckets_from(kNoCandKey, kNoCandKey, 0u, seed);
      degenerate = (ovf_now & 2u) != 0u;
    }
    // no window for this (n, k) (a workspace the host believed warm): the exact fallback
    if (!ok && b == 0 && tid == 0) atomicOr(&ctrl->overflow[par], 2u);
    // a degenerate sample (K1's flag, or this prologue's): K34 will take the exact
    // fallback, which needs nothing from this kernel (with the fused gossip step the
    // stream must still run)
    if (!GS && (!ok || degenerate)) return;
  } else {
    bk = make_buckets(hs_lo, hs_hi, seed);
  }
  if (tid < kNBucket) sm.hist[tid] = 0;
  if (tid == 0) {
    sm.next_chunk = kTwoChunks ? 2 * kK2Waves : kK2Waves;
    sm.spill = 0;
  }
  __syncthreads();
  bk.n = n;
  if (MODE == kHash && b == 0 && tid == 0) {
    TopkBounds& W = ctrl->bounds[par];
    W.s_lo = bk.s_lo;
    W.s_hi = bk.s_hi;
    W.shift = bk.shift;
    W.m1024 = 0u;
    W.n = n;
    W.k = k;
    W.valid = 1u;
  }
  STAMP(1024 + b, 1);

  // ---- stream.  Chunk c's candidates get the global slot range [cbeg, ..) and
  // a count, so the tile's candidates in chunk order are in index order.
  // Invariant at the loop top: A holds (or is loading) chunk c's first batch
  // when c is a full chunk.
  const int64_t tb = b * (int64_t)tile;
  WaveAcc a{};
  // One chunk whose batch (one-batch chunks) is in R, or that loads itself
  // (hash mode, the partial chunk); ends with the chunk's bookkeeping.
  // `reload` refills R (the wave's next chunk) as soon as R is dead.
  auto run_chunk = [&](uint32_t cc, const float4 (&R)[kK2Unroll], auto&& reload) {
    const int64_t cbeg = tb + (int64_t)cc * kChunk;
    const int64_t cend = min(cbeg + kChunk, n);
    float* __restrict__ ov = cval + cbeg;
    uint32_t* __restrict__ oi = cidx + cbeg;
    a.estaged = a.eflushed = a.staged = a.lcnt = 0u;
    a.lstart = a.lfill;
    if (cbeg + kChunk <= n) {
      if constexpr (MODE == kData) {
        process_batch<XH>(src, R, cbeg, cend, sm, w, lane, a, ov, oi, bk, reload);
      } else {
        reload();
        process_rows_hash<MODE, XH>(src, cbeg, cend, sm, w, lane, a, ov, oi, bk);
      }
    } else {
      reload();  // (R unused: the partial chunk loads itself)
      // the buffer's last, partial chunk (or an empty one past n): guarded rows
      for (int64_t base = cbeg; base < cend; base += 256) {
        const int64_t i = base + 4 * lane;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE == kData) {
          float tt[4];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            tt[q] = (i + q < cend) ? (GS ? src.val_gossip(i + q, gs) : src.val(i + q)) : 0.f;
          v = make_float4(tt[0], tt[1], tt[2], tt[3]);
        }
        process_row<MODE, XH, true>(src, v, i, cend, sm, w, lane, a, ov, oi, bk);
      }
    }
    // the chunk's remaining entries (< 64)
    const uint32_t rest = a.estaged - a.eflushed;
    if (rest) flush_entries<MODE, XH>(src, sm, w, lane, a, rest, ov, oi, bk);
    if (lane == 0) {
      sm.ccnt[cc] = a.staged;
      sm.cmeta[cc] = (w * kPairsPerWave + a.lstart) | (a.lcnt << 16);
    }
  };
  if constexpr (kTwoChunks) {
    // A and B hold the wave's next two chunks; a buffer is refilled with the
    // next claimed chunk as soon as it has been processed.  Claims are
    // increasing per wave (cA < cB at the loop top), so the first chunk past
    // the tile ends the wave's stream.
    uint32_t cA = c, cB = c + kK2Waves;
    for (;;) {
      if (cA >= nchunk) break;
      const uint32_t nA = claim_chunk(sm, lane);
      run_chunk(cA, A, [&] {
        if constexpr (MODE == kData) load_rows_full<XH>(ts, batch0(nA), lane, A);
      });
      cA = nA;
      if (cB >= nchunk) break;
      const uint32_t nB = claim_chunk(sm, lane);
      run_chunk(cB, B, [&] {
        if constexpr (MODE == kData) load_rows_full<XH>(ts, batch0(nB), lane, B);
      });
      cB = nB;
    }
  } else {
    // one buffer (two input streams: x - xh is formed at load time; hash mode: no loads)
    while (c < nchunk) {
      const uint32_t nn = claim_chunk(sm, lane);
      if constexpr (GS) gossip_rows(ts, batch0(c), lane, gs.gamma, A);
      run_chunk(c, A, [&] {
        if constexpr (MODE == kData && !GS) load_rows_full<XH>(ts, batch0(nn), lane, A);
      });
      c = nn;
    }
  }
  if (lane == 0) sm.cnt[w] = a.cand;  // wave-uniform
  STAMP(1024 + b, 2);
  WSTAMP(32000 + b * 8 + (w >> 2), w & 3);
  __syncthreads();

  // ---- end of tile: bucket suffix counts and the chunks' candidate prefix;
  // then the LDS pairs leave in one burst and the maybe keys are counting-sorted
  // into the side list.  When no wave spilled (the usual case) the tile's
  // candidates are written COMPACTLY, chunk after chunk from the tile start
  // (full lines; cntw then says "one run": [total, 0, 0, ...]), and the sorted
  // side list is staged in LDS and copied out coalesced.  Scattered partial-line
  // stores while other CUs still stream cost ~0.5 us per MB (HBM turnaround): each wave
  // writing its chunks' pairs as its own stream ends (per-chunk slots) took K2 71 -> 96 us
  // and K34 11 -> 15 us at 100M (same-box A/B, round 5: removed).
  uint32_t hsum, csum;
  bool spilled;
  {
    // thread t <-> maybe bucket jb = 254 - t (t = 255: the "sure" bucket 255);
    // cum[j] = #candidates with bucket >= j, sure included.  And thread t <->
    // chunks kCPT*t .. +kCPT-1 for the chunk prefix.
    const int t = tid;
    const int jb = t < kNMaybe ? kNMaybe - 1 - t : kNMaybe;
    const uint32_t hv = t < kNMaybe ? sm.hist[jb] : 0u;
    uint32_t cc4[kCPT], cs = 0;
    bool sp = false;
#pragma unroll
    for (int q = 0; q < kCPT; ++q) {
      const uint32_t j = kCPT * (uint32_t)t + q;
      cc4[q] = j < nchunk ? sm.ccnt[j] : 0u;
      if (j < nchunk) sp |= cc4[q] != (sm.cmeta[j] >> 16);
      cs += cc4[q];
    }
    if (ballot(sp) != 0ull && lane == 0) atomicOr(&sm.spill, 1u);  // (__syncthreads_or waits on vmcnt(0))
    uint32_t above, cpre;
    block_excl_scan2(hv, cs, sm.scratch, &above, &cpre, &hsum, &csum);  // maybe keys in buckets > jb
#pragma unroll
    for (int q = 0; q < kCPT; ++q) {
      const uint32_t j = kCPT * (uint32_t)t + q;
      if (j < nchunk) sm.ccnt[j] = cpre;
      cpre += cc4[q];
    }
    if (t == 0) sm.ccnt[nchunk] = csum;
    const uint32_t sure = csum - hsum;
    if (t == 0 && hsum > side_cap) atomicOr(&ctrl->overflow[par], 1u);
    if (t < kNBucket) {
      const uint32_t cum = t < kNMaybe ? sure + above + hv : sure;
      cum_tab[b * kNBucket + jb] = cum;
      atomicAdd(&ctrl->G[par][b & (kNRep - 1)][jb], cum);
      if (t < kNMaybe) sm.hist[jb] = above;  // counting-sort cursor of bucket jb (hist is dead now)
    }
    STAMP(22000 + b, 0);
    __syncthreads();
    spilled = sm.spill != 0;
  }
  {
    uint32_t* __restrict__ sd = side + b * side_cap;
    uint32_t* __restrict__ skeys = reinterpret_cast<uint32_t*>(&sm.ent_v[0][0]);  // the ring is dead now
    const bool sort_lds = hsum <= (uint32_t)kSideLds;
    // a half wave per chunk (a chunk holds ~20 candidates at k = 1 %)
    const uint32_t h = (uint32_t)lane & 31u;
    for (uint32_t c0 = 2u * w; c0 < nchunk; c0 += 2u * kK2Waves) {
      const uint32_t cc = c0 + ((uint32_t)lane >> 5);
      const bool have = cc < nchunk;
      const uint32_t meta = have ? sm.cmeta[cc] : 0u;
      const uint32_t cp = have ? sm.ccnt[cc] : 0u, cnt = have ? sm.ccnt[cc + 1] - cp : 0u;
      const uint32_t ls = meta & 0xFFFFu, lc = meta >> 16;
      const int64_t o = tb + (spilled ? (int64_t)cc * kChunk : (int64_t)cp);
      float* __restrict__ ov = cval + o;
      uint32_t* __restrict__ oi = cidx + o;
      auto to_side = [&](uint32_t vb, uint32_t ix) {
        const uint32_t key = MODE == kData ? (vb & 0x7fffffffu) : (rank_hash(seed, ix) >> 1);
        if (key < bk.s_hi) {  // every candidate has key >= s_lo
          const uint32_t p = atomicAdd(&sm.hist[(key - bk.s_lo) >> bk.shift], 1u);
          if (sort_lds) skeys[p] = key;
          else if (p < side_cap) sd[p] = key;
        }
      };
      // Store-only loop: no global load may follow the stores inside it (vmcnt
      // counts stores too, so a load's wait would wait for every store before it).
      for (uint32_t j = h; j < lc; j += 32) {
        const uint2 pr = sm.u.pairs[ls + j];
        ov[j] = __uint_as_float(pr.x);
        oi[j] = pr.y;
        to_side(pr.x, pr.y);
      }
      if (have && h == 0) cntw[(int64_t)b * nchunk + cc] = spilled ? cnt : (cc == 0 ? csum : 0u);
      if (cc == 0 && lane == 0) tinfo[b] = spilled ? 0xFFFFFFFFu : csum;
      // rare (a wave's LDS region overflowed): this tile keeps per-chunk slot
      // ranges; the pairs spilled during the stream are only binned here
      for (uint32_t j = lc + h; j < cnt; j += 32) to_side(__float_as_uint(ov[j]), oi[j]);
    }
    if (sort_lds) {
      __syncthreads();
      for (uint32_t i = (uint32_t)tid; i < hsum; i += kK2Threads) sd[i] = skeys[i];
    }
  }
  WSTAMP(32000 + b * 8 + 4 + (w >> 2), w & 3);
  STAMP(1024 + b, 3);
}

// ----------------------------------------------------------------------------
// K34: exact threshold T, tie quota r, then this tile's ordered output; one
// workgroup per tile
//
// Every workgroup derives (T, r) and ALL tiles' output offsets itself from the
// same inputs (the replicated bucket totals, two table words per tile, the few
// thousand keys of bucket j* copied into LDS), then compacts its own tile.  The
// redundant select is a handful of L2-served round trips; it replaces a
// single-workgroup select kernel and a kernel boundary.
//
// The bucket totals and the overflow flag are zeroed at the START of each call
// (K1, or a memset in hash mode), so K34 needs no last-workgroup ticket: a
// returning atomic here was waited for on the spot (~1.8 us on the critical
// path) because the atomic optimizer consumes its result right away.
// ----------------------------------------------------------------------------
// Wave 0 of a workgroup: over a 256-bin LDS histogram (ascending value order),
// find the bin holding the rank-th largest entry; returns (bin, rank inside bin)
// via out[0], out[1].  Other waves must not call.
CHOCO_DEV void wave_find_bin(const uint32_t* hist, uint32_t rank, uint32_t* out) {
  const int lane = lane_id();
  const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
  const uint32_t loc = h0 + h1 + h2 + h3;
  const uint32_t rv = __shfl(loc, 63 - lane);
  const uint32_t inc = wave_incl_scan(rv);
  const uint32_t suf_incl = __shfl(inc, 63 - lane);  // entries in bins >= 4*lane
  const uint32_t above = suf_incl - loc;
  if (above < rank && rank <= suf_incl) {
    uint32_t acc = above;
    const uint32_t hs[4] = {h0, h1, h2, h3};
    for (int t = 3; t >= 0; --t) {
      if (acc + hs[t] >= rank) { out[0] = 4 * lane + t; out[1] = rank - acc; break; }
      acc += hs[t];
    }
  }
}

// Run starts of a tile's per-chunk candidate runs: counts (kCPT per thread) ->
// exclusive starts, starts[nchunk] = total.  Every thread of the kK4Threads
// workgroup calls it; ends with a barrier.
CHOCO_DEV uint32_t chunk_run_starts(const uint32_t (&cw)[kCPT], uint32_t nchunk, uint32_t* starts,
                                    uint32_t* scratch) {
  const uint32_t j0 = kCPT * threadIdx.x;
  uint32_t s = 0;
#pragma unroll
  for (int q = 0; q < kCPT; ++q) s += cw[q];
  uint32_t tot;
  uint32_t pre = block_excl_scan(s, scratch, &tot);
#pragma unroll
  for (int q = 0; q < kCPT; ++q) {
    if (j0 + q < nchunk) starts[j0 + q] = pre;
    pre += cw[q];
  }
  if (threadIdx.x == 0) starts[nchunk] = tot;
  __syncthreads();
  return tot;
}

constexpr int kEmitR = 8;  // emission batch: kEmitR rows of kK4Threads candidate positions
constexpr int kEmitRows = kEmitR;
constexpr int kSelBits = 13;  // radix-select digit: one round for bucket widths <= 2^13
struct FinSmem {
  uint32_t keys[kMCap];
  uint32_t kbase[kK4Threads];  // per tile: side-list index of its first bucket-j* key - its first slot
  uint32_t ecnt[2][kEmitRows * (kK4Threads / 64) + 1];  // emission: per (row, wave) counts -> bases, total
  uint32_t hist[1 << kSelBits];
  uint32_t G[kNBucket];
  uint32_t run_start[kMaxTileChunks + 1];
  uint32_t scratch[40];
  uint32_t bc[8];
  uint32_t ctl[16];  // this call's window (s_lo, s_hi, shift), overflow word, margin m1024; drift words
};
static_assert(kK2Target <= kK4Threads, "K34 keeps one tile per thread");

// Emission: a batch is kEmitRows rows of kK4Threads candidate positions; in
// row i thread t owns position p0 + i * kK4Threads + t, so every load and
// store instruction is contiguous across the wave.
// Candidate slot of tile position p (positions past the tile's total clamp to
// the tile start: loads stay unconditional).  One run (the compact layout)
// needs no search.
CHOCO_DEV int64_t cand_addr(const uint32_t* run_start, uint32_t nchunk, uint32_t tot, uint32_t p, int64_t tb,
                            bool compact) {
  if (p >= tot) return tb;
  if (compact || run_start[1] >= tot) return tb + p;
  uint32_t lo = 0, hi = nchunk - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (run_start[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return tb + (int64_t)lo * kChunk + (p - run_start[lo]);
}

// Exclusive ranks, in position order, of the flagged slots of one emission
// batch (row-major: row i, then wave, then lane); returns the batch total.
// `cnt` is one of two alternating LDS buffers; two barriers.
CHOCO_DEV uint32_t batch_ranks(const bool (&f)[kEmitRows], uint32_t (&rk)[kEmitRows], uint32_t* cnt,
                               uint32_t nrows = kEmitRows) {
  // rows >= nrows (workgroup-uniform) hold no position: no ballot, a zero count.
  // (r04 A/B: every wave scanning the counts itself after ONE barrier was slower,
  // 1.48 against 1.03 us in K34's stamps: wave 0 scans between two barriers)
  constexpr int kW = kK4Threads / 64;
  const int lane = lane_id(), w = threadIdx.x >> 6;
  uint64_t bm[kEmitRows];
#pragma unroll
  for (int i = 0; i < kEmitRows; ++i) {
    bm[i] = (uint32_t)i < nrows ? ballot(f[i]) : 0ull;
    if (lane == 0) cnt[i * kW + w] = (uint32_t)__popcll(bm[i]);
  }
  __syncthreads();
  if (w == 0) {  // wave 0 scans the kEmitRows * kW = 128 counts, two per lane
    const uint32_t c0 = cnt[2 * lane], c1 = cnt[2 * lane + 1];
    const uint32_t inc = wave_incl_scan(c0 + c1);
    const uint32_t ex = inc - c0 - c1;
    cnt[2 * lane] = ex;
    cnt[2 * lane + 1] = ex + c0;
    if (lane == 63) cnt[kEmitRows * kW] = inc;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kEmitRows; ++i) rk[i] = cnt[i * kW + w] + mask_prefix(bm[i]);
  return cnt[kEmitRows * kW];
}
static_assert(kEmitRows * (kK4Threads / 64) == 128, "batch_ranks: wave 0 scans 2 counts per lane");

// The next call's window after a fallback: keys at count levels k (1 +- 1/8) from the
// complete coarse histogram hist[0] (key >> 20 of every key), bin-rounded outward.
CHOCO_DEV void fallback_window(WideCtrl* W, int64_t n, int64_t k, ExactSmem& es, TopkBounds* next) {
  for (int i = threadIdx.x; i < 2048; i += blockDim.x) es.hist[i] = ld_sc1(&W->hist[0][i]);
  if (threadIdx.x < 4) es.bc[threadIdx.x] = 0u;
  __syncthreads();
  const uint64_t lo_t = std::min<uint64_t>((uint64_t)n, (uint64_t)k + (uint64_t)k / 8);
  const uint64_t hi_t = std::max<uint64_t>(1, (uint64_t)k - (uint64_t)k / 8);
  block_find_two(es.hist, (uint32_t)lo_t, (uint32_t)hi_t, es.scratch, es.bc);
  if (threadIdx.x == 0) {
    const uint64_t x_lo = (uint64_t)es.bc[0] << 20, x_hi = ((uint64_t)es.bc[2] + 1) << 20;
    const uint64_t width = x_hi > x_lo + 255 ? x_hi - x_lo : 255;
    uint32_t sh = 0;
    while (((uint64_t)kNMaybe << sh) < width) ++sh;
    next->s_lo = (uint32_t)x_lo;
    next->s_hi = (uint32_t)std::min<uint64_t>(x_lo + ((uint64_t)kNMaybe << sh), 0xFFFFFFFFull);
    next->shift = sh;
    next->m1024 = 0u;
    next->n = n;
    next->k = k;
    next->valid = 1u;
  }
  __syncthreads();
}

// The exact select over the whole input, shared by every K34 workgroup (wide.h), when
// the sample's guess failed; workgroup 0's item for tile 0 also writes the next window.
template <int MODE, bool XH>
CHOCO_DEV void wide_fallback(const Src<MODE, XH>& src, int64_t n, int64_t k, uint32_t tile, uint32_t nb, const Fold& fold,
                             float scale, WideCtrl* W, uint32_t* __restrict__ gcnt, uint32_t* __restrict__ thist,
                             float* __restrict__ out_val,
                             int32_t* __restrict__ out_idx, int64_t idx_base, ExactSmem& es, uint32_t* s_tk,
                             uint32_t* __restrict__ status, uint32_t* __restrict__ host_status, TopkBounds* next) {
  wide_select<kK4Threads>(
      RangeTiles<kK4Threads, 4, MODE, XH>{src, n, tile},  // 4 float4 rows per stream in flight
      k, nb, W, gcnt, thist, es, s_tk, status, host_status,
      [&](uint32_t) {
        if (next != nullptr) fallback_window(W, n, k, es, next);
      },
      [&](uint32_t pos, int64_t i, float v) {
        out_val[pos] = v * scale;
        out_idx[pos] = (int32_t)(i + idx_base);
        if (fold.on()) fold_apply(fold, i, v * scale);
      });
}

// ----------------------------------------------------------------------------
// Warm start: the NEXT call's window from this call's bucket counts
//
// G[j] = #{key >= s_lo + j 2^shift} (j = 0..255, G[255] = #{key >= s_hi}) is
// this call's key distribution around T.  The next window puts its candidate
// floor where this call had k (1 + m) keys above, and its sure ceiling where it
// had k (1 - m): if the next delta's distribution moved by less than m the next
// call selects inside it.  m (in 1/1024 of k) is twice the miss of the edges
// this call aimed at, decaying by half per call to the floor m0 (warm_m0).  Edges outside the
// window are extrapolated from its density (G[0] - k keys over [s_lo, T]).
// Wave 0 of one workgroup; ~0.3 us, after that workgroup's emission.
// ----------------------------------------------------------------------------
// Cold-run lengths after a warm miss.  A miss costs the exact fallback (~0.6-0.75 ms at
// 100M) against ~10 us saved per warm call, so a retry pays only if warm then holds for
// ~60+ calls: the first run is 64 calls, doubling per consecutive miss.
constexpr uint32_t kColdMin = 64, kColdMax = 4096;
constexpr uint32_t kShadowExit = 2;  // cold-run calls in a row whose k-th key the carried window would have held
CHOCO_DEV uint32_t nk_tag(int64_t n, int64_t k) {
  return ((uint32_t)n * 2654435761u) ^ ((uint32_t)k * 40503u) ^ (uint32_t)((uint64_t)k >> 32) ^ 1u;
}
// (window_drift: choco_common.h)
constexpr uint32_t kWarmM0 = 20;     // ~2 % of k (the bench's randn deltas drift ~0.1 %)
constexpr uint32_t kWarmMMax = 512;  // 50 %
// The margin's floor m0 for a given k (host; a kernel argument of K34).  Between two independent
// draws of the same distribution the number of keys above a fixed key moves by ~sqrt(2 k)
// (one binomial error in the draw that placed the edge, one in the draw that meets it), i.e.
// by sqrt(2 / k) of k: 0.14 % at k = 1M, but 2.8 % at k = 2,621 (n = 262,147 at 1 %), more
// than kWarmM0 -- there a stationary delta missed its carried window every few calls, and the
// rule below, which raises m once an edge comes closer than m / 2, kept moving m.  The floor
// is 8 sigma of that noise (4 sigma for the rule) where this exceeds kWarmM0: k < 335,545.
static uint32_t warm_m0(int64_t k) {
  const double m = ceil(1024.0 * 8.0 * sqrt(2.0 / (double)k));
  return (uint32_t)std::min<double>((double)kWarmMMax, std::max<double>((double)kWarmM0, m));
}
CHOCO_DEV void next_window(const uint32_t* G, uint32_t s_lo, uint32_t s_hi, uint32_t shift, uint32_t m_prev,
                           uint32_t T, int64_t n, int64_t k, int32_t drift, uint32_t m0,
                           TopkBounds* __restrict__ out, uint32_t& w_lo, uint32_t& w_hi) {
  const int lane = lane_id();
  const double kd = (double)k;
  uint32_t m = m0;
  if (m_prev != 0u) {  // this call's window aimed at k (1 + m_prev) / k (1 - m_prev)
    // One-sided: only an edge that moved TOWARD the k-th key is a miss of the aim (fewer
    // candidates above the floor, more keys above the ceiling).  A window wider than
    // aimed -- its edges are rounded outward to the previous window's buckets -- is safe;
    // counting that slack as drift (|.|) doubled m call after call on i.i.d. deltas
    // (20 -> 97 -> 181 -> 512 / 1024 of k, r04) until the bucket of the k-th key no
    // longer fitted the select.
    const double e = fmax(fmax(kd * (1.0 + m_prev / 1024.0) - (double)G[0], 0.0),
                          fmax((double)G[kNMaybe] - kd * (1.0 - m_prev / 1024.0), 0.0));
    const double me = ceil(2.0 * e / kd * 1024.0);
    m = (uint32_t)fmin((double)kWarmMMax, fmax(fmax((double)m0, me), (double)(m_prev / 2)));
  }
  const uint64_t lo_t = (uint64_t)k + (uint64_t)k * m / 1024u;
  const uint64_t hi_t = (uint64_t)k - std::min<uint64_t>((uint64_t)k, (uint64_t)k * m / 1024u);
  uint32_t nlo = 0, nhi = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t g = G[4 * lane + q];
    nlo += (uint64_t)g >= lo_t ? 1u : 0u;  // G is non-increasing: a prefix of the buckets
    nhi += (uint64_t)g > hi_t ? 1u : 0u;
  }
  nlo = wave_sum(nlo);
  nhi = wave_sum(nhi);
  if (lane != 0) return;
  const uint64_t w0 = (uint64_t)s_hi - s_lo;
  uint64_t x_lo, x_hi;
  if (nlo >= 1u) {
    x_lo = (uint64_t)s_lo + ((uint64_t)(nlo - 1u) << shift);
  } else {  // fewer than k (1 + m) keys in the whole window: extend it downwards
    const double D = (double)(T - s_lo), C = (double)G[0] - kd, need = (double)lo_t - (double)G[0];
    const double dl = C >= fmax(kd / 1024.0, 16.0) ? 2.0 * D * need / C + (double)(1u << shift)
                                                   : 2.0 * (double)w0 + D;
    x_lo = dl >= (double)s_lo ? 0ull : (uint64_t)((double)s_lo - dl);
  }
  if (nhi <= (uint32_t)kNMaybe) {
    x_hi = std::min<uint64_t>((uint64_t)s_lo + ((uint64_t)nhi << shift), s_hi);
  } else {  // more than k (1 - m) keys are "sure": extend it upwards
    const double D = (double)(s_hi - T), C = kd - (double)G[kNMaybe], need = (double)G[kNMaybe] - (double)hi_t;
    const double dh = C >= fmax(kd / 1024.0, 16.0) ? 2.0 * D * need / C + (double)(1u << shift)
                                                   : 2.0 * (double)w0 + D;
    x_hi = (uint64_t)fmin((double)s_hi + dh, 2147483648.0);
  }
  // drift-aware: both edges follow the k-th key's steady drift (window_drift)
  if (drift != 0) {
    const int64_t lo2 = (int64_t)x_lo + drift, hi2 = (int64_t)x_hi + drift;
    x_lo = (uint64_t)std::max<int64_t>(0, lo2);
    x_hi = (uint64_t)std::min<int64_t>(2147483648ll, std::max<int64_t>(hi2, (int64_t)x_lo + 1));
  }
  const uint64_t width = x_hi > x_lo + kNMaybe ? x_hi - x_lo : (uint64_t)kNMaybe;
  uint32_t sh = 0;
  while (((uint64_t)kNMaybe << sh) < width) ++sh;
  w_lo = (uint32_t)x_lo;  // (also returned in registers: no read-back on workgroup 0's tail)
  w_hi = (uint32_t)std::min<uint64_t>(x_lo + ((uint64_t)kNMaybe << sh), 0xFFFFFFFFull);
  out->s_lo = w_lo;
  out->s_hi = w_hi;
  out->shift = sh;
  out->m1024 = m;
  out->n = n;
  out->k = k;
  out->valid = 1u;
}

template <int MODE, bool XH>
__global__ __launch_bounds__(kK4Threads) void topk_finish_kernel(
    const float* x, const float* xh, int64_t n, int64_t k, uint32_t tile, uint32_t nb,
    uint32_t side_cap, uint64_t seed, float scale, TopkCtrl* __restrict__ ctrl, const uint32_t* __restrict__ cum_tab,
    const uint32_t* __restrict__ cntw, const uint32_t* __restrict__ side, const float* __restrict__ cval,
    const uint32_t* __restrict__ cidx, float* __restrict__ out_val, int32_t* __restrict__ out_idx,
    int64_t idx_base, WideCtrl* __restrict__ wide, uint32_t* __restrict__ gcnt, uint32_t* __restrict__ thist,
    uint32_t par, uint32_t* __restrict__ status, uint32_t* __restrict__ host_status, const uint32_t* __restrict__ tinfo,
    Fold fold, uint32_t* __restrict__ cold_host, uint32_t m0) {
  __shared__ FinSmem fs;
  __shared__ ExactSmem es;
  __shared__ uint32_t s_tk;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  STAMP(24576 + b, 0);
  // ---- first round trip, every load independent: control words (as vector
  // loads, so they are issued here and not as late scalar loads), the totals,
  // every tile's j*-independent "sure" count, this tile's chunk counts
  const uint32_t ku = (uint32_t)k;
  const uint32_t nchunk = tile / (uint32_t)kChunk;
  // the tile's candidates: one compact run (the usual case) or per-chunk slot runs
  const uint32_t ti = tinfo[b];
  const bool compact = ti != 0xFFFFFFFFu;
  uint32_t cw[kCPT];
#pragma unroll
  for (int q = 0; q < kCPT; ++q) {
    const uint32_t j = kCPT * tid + q;
    cw[q] = (!compact && j < nchunk) ? cntw[b * nchunk + j] : 0u;
  }
  uint32_t cword = 0;
  {
    const TopkBounds& Bw = ctrl->bounds[par];
    const uint32_t* src = tid == 0 ? &Bw.s_lo : tid == 1 ? &Bw.s_hi : tid == 2 ? &Bw.shift
                        : tid == 3 ? &ctrl->overflow[par] : tid == 4 ? &Bw.m1024
                        : tid < 11 ? &ctrl->t_prev + (tid - 5)  // t_prev, d_prev, sh_lo, sh_hi, sh_nk, sh_hits
                        : tid == 11 ? &ctrl->backoff : tid == 12 ? &ctrl->cold_left
                        : tid == 13 ? &ctrl->d_cand : &ctrl->d_trust;
    if (tid < 15) cword = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const bool mine_tile = tid < (int)nb;
  const uint32_t* row = cum_tab + (int64_t)(mine_tile ? tid : 0) * kNBucket;  // clamped: loads unconditional
  const uint32_t sure_t = row[kNMaybe];
  uint32_t g[kNRep];
  if (tid < kNBucket) {
#pragma unroll
    for (int r = 0; r < kNRep; ++r) g[r] = ctrl->G[par][r][tid];
  }
  // s_lo, s_hi, shift, overflow, m1024, t_prev, d_prev, sh_lo, sh_hi, sh_nk, sh_hits, backoff, cold_left,
  // d_cand, d_trust (workgroup 0's tail then issues stores only)
  if (tid < 15) fs.ctl[tid] = cword;
  const uint32_t tot = compact ? ti : chunk_run_starts(cw, nchunk, fs.run_start, fs.scratch);
  if (compact) __syncthreads();  // fs.ctl (chunk_run_starts ends with this barrier)
  const uint32_t s_lo = fs.ctl[0], shift = fs.ctl[2], overflow = fs.ctl[3];
  STAMP(26000 + b, 0);
  // ---- the addresses of the tile's first emission batch (it does not depend on T)
  const int64_t tb = b * (int64_t)tile;
  int64_t addr[kEmitR];
#pragma unroll
  for (int i = 0; i < kEmitR; ++i) addr[i] = cand_addr(fs.run_start, nchunk, tot, (uint32_t)(i * kK4Threads + tid), tb, compact);
  float v[kEmitR];
  uint32_t idx[kEmitR];
  if (tid < kNBucket) {
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < kNRep; ++r) s += g[r];
    fs.G[tid] = s;
  }
  if (tid == 0) fs.bc[4] = 0;
  __syncthreads();
  STAMP(26000 + b, 1);
  // G[j] = #candidates in buckets >= j is non-increasing; j* = the unique
  // j <= 254 with G[j] >= k > G[j+1]
  bool fallback = overflow != 0 || fs.G[0] < ku || fs.G[kNMaybe] >= ku;
  if (!fallback && tid < kNMaybe && fs.G[tid] >= ku && fs.G[tid + 1] < ku) fs.bc[4] = tid;
  __syncthreads();
  const uint32_t jstar = fs.bc[4];
  STAMP(26000 + b, 2);
  if (!fallback && fs.G[jstar] - fs.G[jstar + 1] > (uint32_t)kMCap) fallback = true;
  uint32_t T_exact = 0;  // (workgroup 0's tail: this call's exact k-th key on the select path)
  uint32_t nw_lo = 0, nw_hi = 0;  // ... and the window it prepared for the next call
  uint32_t trust = 0;             // ... and the drift-trust streak
  const uint32_t nk = nk_tag(n, k);
  if (fallback) {
    if (b == 0 && tid == 0) atomicAdd(&ctrl->fallbacks, 1u);
    // the sample's guess was off: the exact radix select over the whole input, shared
    // by every workgroup through the ticketed queue (wide_fallback)
    Src<MODE, XH> src{x, xh, seed};
    wide_fallback(src, n, k, tile, nb, fold, scale, wide, gcnt, thist, out_val, out_idx, idx_base, es, &s_tk, status,
                  host_status, MODE == kData ? &ctrl->bounds[par ^ 1u] : nullptr);
  } else {
    // ---- thread t <-> tile t: bucket-j* key count and side-list offset
    uint32_t above = 0, cb = 0, off = 0;
    {
      const uint32_t a = row[jstar], c = row[jstar + 1], s = sure_t;
      if (mine_tile) {
        above = c;
        cb = a - c;   // keys of bucket j* in this tile
        off = c - s;  // their side-list offset (buckets stored high to low)
      }
    }
    uint32_t M;
    const uint32_t kpos = block_excl_scan(cb, fs.scratch, &M);  // M = G[j*] - G[j*+1]
    STAMP(26000 + b, 3);
#if CHOCO_STAMPS
    if (b == 0 && tid == 0) {
      g_stamps[29000][0] = M; g_stamps[29000][1] = shift; g_stamps[29000][2] = jstar; g_stamps[29000][3] = fs.G[0];
    }
#endif
    {
      // All tiles' bucket-j* keys -> keys[0, M), tile after tile: key slot i
      // belongs to tile tmap[i] (a slot -> tile map each tile writes for its
      // own slots; it lives in the select histogram, which is not in use yet),
      // so consecutive lanes load consecutive side-list words (a tile holds
      // ~M / nb ~ 20 keys): a few lines per load instead of one per lane.
      uint16_t* tmap = reinterpret_cast<uint16_t*>(fs.hist);
      static_assert(sizeof(fs.hist) >= kMCap * sizeof(uint16_t), "tile map fits the histogram");
      fs.kbase[tid] = (uint32_t)(mine_tile ? tid : 0) * side_cap + off - kpos;  // mod 2^32
      for (uint32_t j = 0; j < cb; ++j) tmap[kpos + j] = (uint16_t)tid;
      __syncthreads();
      STAMP(27000 + b, 1);
      constexpr int kG = kMCap / kK4Threads;  // M <= kMCap: at most kG slots per thread
      uint32_t ka[kG];
#pragma unroll
      for (int q = 0; q < kG; ++q) {
        const uint32_t i = min((uint32_t)tid + (uint32_t)q * kK4Threads, M - 1u);
        ka[q] = (uint32_t)q * kK4Threads < M ? fs.kbase[tmap[i]] + i : 0u;  // workgroup-uniform guard
      }
      STAMP(28000 + b, 0);
      uint32_t kv[kG];
#pragma unroll
      for (int q = 0; q < kG; ++q) kv[q] = (uint32_t)q * kK4Threads < M ? side[ka[q]] : 0u;  // clamped slots
      STAMP(28000 + b, 1);
      __syncthreads();  // the tile map (= histogram) is dead before the select clears it
#pragma unroll
      for (int q = 0; q < kG; ++q) {
        const uint32_t i = (uint32_t)tid + (uint32_t)q * kK4Threads;
        if (i < M) fs.keys[i] = kv[q];
      }
      {
        // late prefetch: the first emission batch goes out once the keys are in, so it
        // does not queue in front of other workgroups' key gathers (issued behind the key
        // loads instead, measured slower), and lands while T is being selected
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < kEmitR; ++i) {
          v[i] = cval[addr[i]];
          idx[i] = cidx[addr[i]];
        }
      }
    }
    // ---- radix select inside bucket j*: rel = key - base_j in [0, 2^shift),
    // kSelBits per round (one round for shift <= kSelBits)
    STAMP(27000 + b, 2);
    const uint32_t base_j = s_lo + (jstar << shift);
    uint32_t prefix = 0, krem = ku - fs.G[jstar + 1];  // 1 <= krem <= M
    int sh = (int)shift;
    while (sh > 0) {
      const int dsh = sh > kSelBits ? sh - kSelBits : 0;
      const uint32_t dmask = (1u << (sh - dsh)) - 1u;
      // a digit of <= 10 bits (the warm window's buckets): one bin per thread
      const bool narrow = dmask < (uint32_t)kK4Threads;
      for (int i = tid; i < (narrow ? (int)dmask + 1 : (1 << kSelBits)); i += kK4Threads) fs.hist[i] = 0;
      __syncthreads();  // also: the bucket keys are in LDS
      for (uint32_t j = tid; j < M; j += kK4Threads) {
        const uint32_t rel = fs.keys[j] - base_j;
        if (sh >= 32 || (rel >> sh) == (prefix >> sh)) atomicAdd(&fs.hist[(rel >> dsh) & dmask], 1u);
      }
      __syncthreads();
      STAMP(28000 + b, 2);
      if (narrow) {
        const uint32_t hv[1] = {(uint32_t)tid <= dmask ? fs.hist[tid] : 0u};
        block_find_rank(hv, krem, fs.scratch, fs.bc + 5);
      } else {
        block_find_rank_in<(1 << kSelBits) / kK4Threads>(fs.hist, krem, fs.scratch, fs.bc + 5);
      }
      STAMP(28000 + b, 3);
      prefix |= fs.bc[5] << dsh;
      krem = fs.bc[6];
      sh = dsh;
    }
    if (shift == 0) __syncthreads();  // the bucket keys are in LDS
    STAMP(28000 + b, 3);
    STAMP(27000 + b, 0);
    const uint32_t T = base_j + prefix;
    const uint32_t r = krem;  // ties at T to take (>= 1)
    T_exact = T;
    // ---- per tile: #keys > T (every key above bucket j* is) and #keys == T
    uint32_t gt = above, eq = 0;
    for (uint32_t i0 = 0; i0 < cb; i0 += 8) {  // 8 independent LDS reads per round trip
      uint32_t kk[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) kk[q] = fs.keys[kpos + min(i0 + q, cb - 1)];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        gt += (i0 + q < cb && kk[q] > T) ? 1u : 0u;
        eq += (i0 + q < cb && kk[q] == T) ? 1u : 0u;
      }
    }
    uint32_t gpre, epre, gtot, etot;
    block_excl_scan2(gt, eq, fs.scratch, &gpre, &epre, &gtot, &etot);
    if (tid == (int)b) {
      const uint32_t taken = min(r, epre);  // ties taken by earlier tiles (lowest index first)
      const uint32_t take = min(eq, r - taken);
      fs.bc[4] = gpre + taken;
      fs.bc[5] = epre;
      fs.bc[6] = take == 0 ? kTakeNone : (take == eq ? kTakeAll : kTakePartial);
    }
    __syncthreads();
    STAMP(24576 + b, 1);
    uint32_t out = fs.bc[4];
    uint32_t tie_run = fs.bc[5];
    const uint32_t mode = fs.bc[6];
    // Batches of kEmitRows x kK4Threads candidates (row i, thread t <-> position
    // p0 + i * kK4Threads + t); the ranks of the selected ones place them (the
    // ties' ranks first, only when ties at T are split).
    int eb = 0;  // alternating rank buffer
    for (uint32_t p0 = 0; p0 < tot; p0 += kK4Threads * kEmitR) {
      if (p0 != 0) {  // workgroup-uniform: batches after the prefetched first one
#pragma unroll
        for (int i = 0; i < kEmitR; ++i) addr[i] = cand_addr(fs.run_start, nchunk, tot, p0 + i * kK4Threads + tid, tb, compact);
#pragma unroll
        for (int i = 0; i < kEmitR; ++i) {
          v[i] = cval[addr[i]];
          idx[i] = cidx[addr[i]];
        }
      }
      // rows holding positions (workgroup-uniform): a k = 1 % tile holds ~4,000 candidates,
      // half of the batch's 8 rows
      const uint32_t nrows = min((uint32_t)kEmitR, (tot - p0 + kK4Threads - 1) / kK4Threads);
      bool gtv[kEmitR], eqv[kEmitR];
#pragma unroll
      for (int i = 0; i < kEmitR; ++i) {
        const bool valid = p0 + i * kK4Threads + tid < tot;
        const uint32_t key = MODE == kData ? fkey(v[i]) : (rank_hash(seed, idx[i]) >> 1);
        gtv[i] = valid && key > T;
        eqv[i] = valid && key == T;
      }
      STAMP(30000 + b, 0);
      bool sel[kEmitR];
      uint32_t rk[kEmitR];
      if (mode == kTakePartial) {  // workgroup-uniform
        const uint32_t eq_total = batch_ranks(eqv, rk, fs.ecnt[eb], nrows);
        eb ^= 1;
#pragma unroll
        for (int i = 0; i < kEmitR; ++i) sel[i] = gtv[i] || (eqv[i] && tie_run + rk[i] < r);
        tie_run += eq_total;
      } else {
#pragma unroll
        for (int i = 0; i < kEmitR; ++i) sel[i] = gtv[i] || (eqv[i] && mode == kTakeAll);
      }
      const uint32_t nsel = batch_ranks(sel, rk, fs.ecnt[eb], nrows);
      eb ^= 1;
      STAMP(30000 + b, 1);
#pragma unroll
      for (int i = 0; i < kEmitR; ++i) {
        if ((uint32_t)i >= nrows) continue;  // workgroup-uniform
        if (sel[i] && out + rk[i] < ku) {  // (bounded: an inconsistent select cannot write past k)
          out_val[out + rk[i]] = v[i] * scale;
          out_idx[out + rk[i]] = (int32_t)((int64_t)idx[i] + idx_base);
          if (fold.on()) fold_apply(fold, (int64_t)idx[i], v[i] * scale);
        }
      }
      out += nsel;
    }
    STAMP(30000 + b, 2);
    if (MODE == kData && b == 0 && tid < 64)
      next_window(fs.G, s_lo, fs.ctl[1], shift, fs.ctl[4], T, n, k,
                  (trust = drift_trusted(T, fs.ctl[5], fs.ctl[13], fs.ctl[9] == nk) ? min(fs.ctl[14] + 1u, 15u) : 0u)
                          >= kDriftTrust ? window_drift(T, fs.ctl[5], fs.ctl[6], fs.ctl[9] == nk) : 0,
                  m0, &ctrl->bounds[par ^ 1u], nw_lo, nw_hi);
  }
  // random-k windows come from the host each call: nothing for the next call to reuse
  if (MODE == kHash && b == 0 && tid == 0) ctrl->bounds[par ^ 1u].valid = 0u;
  // Cold backoff: a call that took a carried window (m1024 != 0) and still missed puts
  // the workspace on a run of `backoff` calls that sample their own window (in K1 or in
  // K2's prologue), doubling per consecutive miss; warm hits halve it again.  A delta
  // whose k-th key moves further than the window between calls (x_hat draining the top
  // keys of a fixed x, the bench's fused step) then pays K1's sample instead of the
  // exact fallback every call.
  if (MODE == kData && b == 0 && tid == 0) {
    const bool warm_call = fs.ctl[4] != 0u;
    uint32_t bo = fs.ctl[11], cl = fs.ctl[12], hits = fs.ctl[10];
    // the shadow: would the window the previous call prepared have held this k-th key?
    const bool shadow_hit = !fallback && fs.ctl[9] == nk && fs.ctl[7] <= T_exact && T_exact < fs.ctl[8];
    if (warm_call && fallback) {
      bo = min(max(2u * bo, kColdMin), kColdMax);
      cl = bo;
      hits = 0u;
    } else if (warm_call) {
      bo = max(bo / 2u, kColdMin);
      hits = 0u;
    } else if (cl != 0u) {
      --cl;
      // a cold run ends early once the carried (drift-aware) windows would have held the
      // k-th key kShadowExit calls in a row: the drift that caused the miss is followed now
      hits = shadow_hit ? hits + 1u : 0u;
      if (hits >= kShadowExit) {
        cl = 0u;
        hits = 0u;
      }
    }
    ctrl->backoff = bo;
    ctrl->cold_left = cl;
    ctrl->sh_hits = hits;
    if (!fallback) {  // the drift words and the shadow for the next call
      ctrl->d_prev = (fs.ctl[9] == nk && fs.ctl[5] != 0u) ? T_exact - fs.ctl[5] : 0u;
      ctrl->t_prev = T_exact;
      ctrl->sh_lo = nw_lo;  // (this thread's next_window)
      ctrl->sh_hi = nw_hi;
      ctrl->sh_nk = nk;
      ctrl->d_cand = (uint32_t)window_drift(T_exact, fs.ctl[5], fs.ctl[6], fs.ctl[9] == nk);
      ctrl->d_trust = trust;
    } else {
      ctrl->t_prev = 0u;
      ctrl->d_prev = 0u;
      ctrl->sh_nk = 0u;
      ctrl->d_cand = 0u;
      ctrl->d_trust = 0u;
    }
    // (the host launches K1 for fused-gossip calls on a cold run: launch_topk)
    if (cold_host) __hip_atomic_store(cold_host, cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  STAMP(24576 + b, 2);
}

// ----------------------------------------------------------------------------
// host dispatch
// ----------------------------------------------------------------------------
size_t topk_ws_bytes(int64_t n) {
  if (n <= kSmallN) return 256;
  return topk_layout(n).total;
}

// ---- warm-start bookkeeping (host): per workspace pointer, the (n, k, mode) and
// call count of the last pipeline call made on it.  The call count gives each
// call its parity (TopkCtrl); a data-mode call with the same (n, k) as the
// previous call on the workspace is warm (no K1).  K2 re-checks the window's
// (n, k) on the device, so a stale entry costs one exact fallback, never a
// wrong answer.
struct WarmEntry {
  int64_t n, k;
  uint64_t calls;
  bool data;
};
static std::mutex g_warm_mu;
static std::unordered_map<const void*, WarmEntry> g_warm;
static std::atomic<bool> g_warm_on{true};

struct WarmClaim {
  uint32_t par;
  bool known;  // an earlier pipeline call on this workspace left G[par] / overflow[par] zeroed
  bool warm;   // ... and its window is for this (n, k): skip K1
};
static WarmClaim warm_claim(const void* ws, int64_t n, int64_t k, bool data) {
  std::lock_guard<std::mutex> g(g_warm_mu);
  auto it = g_warm.find(ws);
  if (it == g_warm.end()) {
    g_warm.emplace(ws, WarmEntry{n, k, 1u, data});
    return WarmClaim{0u, false, false};
  }
  WarmEntry& e = it->second;
  WarmClaim c{(uint32_t)(e.calls & 1u), true,
              data && e.data && e.n == n && e.k == k && g_warm_on.load(std::memory_order_relaxed)};
  e.n = n;
  e.k = k;
  e.data = data;
  e.calls += 1;
  return c;
}

// GS: the gossip step fused into K1's sample and K2's stream (x written by K2);
// K34 and its exact fallback then read (x_new, xh).
// status: where the exact fallback flags a bounded wait that gave up (the
// workspace's own status word and host mirror, or the segmented workspace's).
static uint32_t host_cold_left(const void* ws);

template <int MODE, bool XH, bool GS = false>
static int launch_topk(const float* x, const float* xh, int64_t n, int64_t k, uint64_t seed, float scale,
                       float* out_val, int32_t* out_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                       hipStream_t st, Gossip gs = Gossip{nullptr, 0.f}, StatusSink status = StatusSink{nullptr, nullptr},
                       Fold fold = Fold{nullptr, nullptr, 0.f}) {
  // the one-workgroup / copy paths emit without a fold: the self message is then applied
  // by the accumulate kernel after them (same arithmetic)
  auto fold_after = [&]() -> int {
    if (!fold.on()) return CHOCO_OK;
    if (fold.mem) return choco_sparse_accumulate(out_val, out_idx, k, fold.hat, fold.mem, n, fold.w, nullptr, st);
    return choco_sparse_accumulate(out_val, out_idx, k, nullptr, fold.hat, n, 1.0f, nullptr, st);
  };
  if (k >= n) {
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    CHOCO_TRY(CHOCO_LAUNCH("topk_all", "topk_all_kernel", (topk_all_kernel<XH>), dim3(g), dim3(256), st, x, xh, n,
                           scale, out_val, out_idx, idx_base));
    return fold_after();
  }
  if (n <= kSmallN) {
    CHOCO_TRY(CHOCO_LAUNCH("topk_exact", "topk_exact_kernel", (topk_exact_kernel<MODE, XH>), dim3(1),
                           dim3(kExactThreads), st, x, xh, n, k, seed, scale, out_val, out_idx, idx_base));
    return fold_after();
  }
  const TopkLayout L = topk_layout(n);
  CHOCO_REQUIRE(ws != nullptr && ws_bytes >= L.total, "top-k workspace too small: need %zu bytes, got %zu",
                L.total, ws_bytes);
  char* base = static_cast<char*>(ws);
  TopkCtrl* ctrl = reinterpret_cast<TopkCtrl*>(base + L.off_ctrl);
  uint32_t* cum = reinterpret_cast<uint32_t*>(base + L.off_cum);
  uint32_t* cntw = reinterpret_cast<uint32_t*>(base + L.off_cntw);
  uint32_t* side = reinterpret_cast<uint32_t*>(base + L.off_side);
  float* cval = reinterpret_cast<float*>(base + L.off_cval);
  uint32_t* cidx = reinterpret_cast<uint32_t*>(base + L.off_cidx);
  if (status.dev == nullptr) status = StatusSink{&ctrl->status, host_status_dev(ws)};
  CHOCO_REQUIRE(status.host != nullptr,
                "top-k: could not map the pinned host mirror of the workspace status word (hipHostMalloc / "
                "hipHostGetDevicePointer failed), so a failed exact-fallback wait could not be reported");
  uint32_t hs_lo = 0;
  uint64_t hs_hi = 0;
  if (MODE == kHash) {
    // keys uniform on [0, 2^31): P(key >= t) = (2^31 - t) / 2^31
    const double nd = (double)n, kd = (double)k, sd = sqrt(kd);
    const double c_lo = std::min(nd, kd + 6.0 * sd + 16.0);
    const double c_hi = kd - 6.0 * sd - 16.0;
    const double two31 = 2147483648.0;
    hs_lo = (uint32_t)std::max(0.0, floor(two31 * (1.0 - c_lo / nd)));
    hs_hi = c_hi < 1.0 ? 0x80000000ull : (uint64_t)ceil(two31 * (1.0 - c_hi / nd));
    if (hs_hi <= hs_lo) hs_hi = (uint64_t)hs_lo + 1;
  }
  const WarmClaim wc = warm_claim(ws, n, k, MODE == kData);
  const uint32_t par = wc.par;
  // Fused gossip step: K2 cannot sample its own window (x is rewritten while it streams),
  // so a warm call on a cold run (K34's backoff, mirrored to the host) runs K1 first.
  uint32_t* cold_host = nullptr;
  bool warm = wc.warm;
  if (GS && MODE == kData) {
    uint32_t* mir = host_status_dev(ws);
    CHOCO_REQUIRE(mir != nullptr, "top-k: could not map the pinned host mirror of the workspace");
    cold_host = mir + 1;
    if (warm && host_cold_left(ws) != 0u) warm = false;
  }
  if (MODE == kHash && !wc.known) {
    // this call's bucket totals and overflow word start from zero (K1 does it in data mode)
    CHOCO_REQUIRE(hipMemsetAsync(&ctrl->G[par][0][0], 0, sizeof(ctrl->G[par]), st) == hipSuccess &&
                      hipMemsetAsync(&ctrl->overflow[par], 0, sizeof(uint32_t), st) == hipSuccess,
                  "hipMemsetAsync failed");
  }
  if (MODE == kData && !warm)
    CHOCO_TRY(CHOCO_LAUNCH("topk_bounds", "topk_bounds_kernel", (topk_bounds_kernel<XH, GS>), dim3(1),
                           dim3(kK1Threads), st, x, xh, n, k, par, sample_ranks(n, k), ctrl, gs));
  CHOCO_TRY(CHOCO_LAUNCH("topk_stream", "topk_stream_kernel", (topk_stream_kernel<MODE, XH, GS>), dim3(L.nb),
                         dim3(kK2Threads), st, x, xh, n, k, L.tile, L.nb, par, L.side_cap, seed, hs_lo, hs_hi, ctrl,
                         cum, cntw, side, cval, cidx, reinterpret_cast<uint32_t*>(base + L.off_tinfo), gs,
                         sample_ranks(n, k), (uint32_t)(MODE == kData && warm && !GS ? 1 : 0)));
  return CHOCO_LAUNCH("topk_finish", "topk_finish_kernel", (topk_finish_kernel<MODE, XH>), dim3(L.nb),
                      dim3(kK4Threads), st, x, xh, n, k, L.tile, L.nb, L.side_cap, seed, scale, ctrl, cum, cntw, side,
                      cval, cidx, out_val, out_idx, idx_base, reinterpret_cast<WideCtrl*>(base + L.off_wide),
                      reinterpret_cast<uint32_t*>(base + L.off_gcnt), reinterpret_cast<uint32_t*>(base + L.off_thist),
                      par, status.dev, status.host, reinterpret_cast<const uint32_t*>(base + L.off_tinfo), fold,
                      cold_host, warm_m0(k));
}

template <int MODE>
static int dispatch_topk(const float* x, const float* xh, int64_t n, int64_t k, uint64_t seed, float scale,
                         float* out_val, int32_t* out_idx, int64_t idx_base, void* ws, size_t ws_bytes,
                         hipStream_t st, Gossip gs = Gossip{nullptr, 0.f}, StatusSink status = StatusSink{nullptr, nullptr},
                         Fold fold = Fold{nullptr, nullptr, 0.f}) {
  CHOCO_REQUIRE(x != nullptr && out_val != nullptr && out_idx != nullptr, "null pointer argument");
  CHOCO_REQUIRE(n > 0 && n < (int64_t)INT32_MAX, "n must be in [1, 2^31-1), got %lld", (long long)n);
  CHOCO_REQUIRE(k >= 1 && k <= n, "k must be in [1, n], got k=%lld n=%lld", (long long)k, (long long)n);
  CHOCO_REQUIRE(aligned4(x) && (xh == nullptr || aligned4(xh)), "x/xhat must be 4-byte aligned");
  if (gs.mem) {
    CHOCO_REQUIRE(xh != nullptr && aligned4(gs.mem), "the gossip step needs x_hat and a 4-byte aligned memory");
    if (MODE == kData && k < n && n > kSmallN)
      return launch_topk<kData, true, true>(x, xh, n, k, seed, scale, out_val, out_idx, idx_base, ws, ws_bytes, st,
                                            gs, status, fold);
    // no full stream pass to fuse into (random-k gathers k elements; small n and
    // k == n are one-workgroup / copy paths): the standalone step, then the codec
    const int rc = gossip_launch(const_cast<float*>(x), gs.mem, xh, gs.gamma, n, st);
    if (rc) return rc;
  }
  if (xh)
    return launch_topk<MODE, true>(x, xh, n, k, seed, scale, out_val, out_idx, idx_base, ws, ws_bytes, st,
                                   Gossip{nullptr, 0.f}, status, fold);
  return launch_topk<MODE, false>(x, xh, n, k, seed, scale, out_val, out_idx, idx_base, ws, ws_bytes, st,
                                  Gossip{nullptr, 0.f}, status, fold);
}

int topk_pipeline(int mode, const float* x, const float* xh, int64_t n, int64_t k, uint64_t seed, float scale,
                  float* out_val, int32_t* out_idx, int64_t idx_base, void* ws, size_t ws_bytes, hipStream_t st,
                  Gossip gs, StatusSink status) {
  if (mode == kHash)
    return dispatch_topk<kHash>(x, xh, n, k, seed, scale, out_val, out_idx, idx_base, ws, ws_bytes, st, gs, status);
  return dispatch_topk<kData>(x, xh, n, k, seed, scale, out_val, out_idx, idx_base, ws, ws_bytes, st, gs, status);
}

bool topk_warm_enabled() { return g_warm_on.load(std::memory_order_relaxed); }

// ---- pinned host mirrors of the workspaces' status words (choco_topk_host_status)
struct HostStatus {
  uint32_t* host;  // pinned, mapped, coherent
  uint32_t* dev;   // its device address
};
static std::mutex g_hs_mu;
static std::unordered_map<const void*, HostStatus> g_hs;

uint32_t* host_status_dev(const void* ws) {
  std::lock_guard<std::mutex> g(g_hs_mu);
  auto it = g_hs.find(ws);
  if (it != g_hs.end()) return it->second.dev;
  // A failure is not cached: this call fails (the callers raise), the next one retries.
  // (A call that ran without the mirror could not report a bounded wait that gave up.)
  void* h = nullptr;
  if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return nullptr;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || d == nullptr) {
    (void)hipHostFree(h);
    return nullptr;
  }
  HostStatus hs{static_cast<uint32_t*>(h), static_cast<uint32_t*>(d)};
  __atomic_store_n(hs.host + 1, 0u, __ATOMIC_RELEASE);  // word 1: K34's cold-run mirror (fused gossip)
  __atomic_store_n(hs.host, 0u, __ATOMIC_RELEASE);
  g_hs.emplace(ws, hs);
  return hs.dev;
}

// The cold-run length K34 mirrors to host word 1 of the workspace's mirror (fused-gossip
// calls only; as of the last call that has completed).
static uint32_t host_cold_left(const void* ws) {
  std::lock_guard<std::mutex> g(g_hs_mu);
  auto it = g_hs.find(ws);
  if (it == g_hs.end() || it->second.host == nullptr) return 0u;
  return __atomic_load_n(it->second.host + 1, __ATOMIC_ACQUIRE);
}

static uint32_t host_status_read(const void* ws, bool clear) {
  std::lock_guard<std::mutex> g(g_hs_mu);
  auto it = g_hs.find(ws);
  if (it == g_hs.end() || it->second.host == nullptr) return 0u;
  const uint32_t v = __atomic_load_n(it->second.host, __ATOMIC_ACQUIRE);
  if (clear && v != 0u) __atomic_store_n(it->second.host, 0u, __ATOMIC_RELEASE);
  return v;
}

void topk_warm_forget(const void* ws, size_t bytes) {
  const char* lo = static_cast<const char*>(ws);
  auto inside = [&](const void* q) {
    const char* p = static_cast<const char*>(q);
    return p == lo || (p > lo && p < lo + bytes);
  };
  {
    std::lock_guard<std::mutex> g(g_warm_mu);
    for (auto it = g_warm.begin(); it != g_warm.end();) {
      if (inside(it->first)) it = g_warm.erase(it);
      else ++it;
    }
  }
  std::lock_guard<std::mutex> g(g_hs_mu);
  for (auto it = g_hs.begin(); it != g_hs.end();) {
    if (inside(it->first)) {
      if (it->second.host) (void)hipHostFree(it->second.host);  // (callers synchronise before a reset)
      it = g_hs.erase(it);
    } else {
      ++it;
    }
  }
}

}  // namespace choco

using namespace choco;

CHOCO_API int64_t choco_topk_k(int64_t n, double ratio) {
  // identical IEEE-double expression to max(1, int(x_len * (1 - ratio)))
  double v = (double)n * (1.0 - ratio);
  int64_t k = (int64_t)v;  // int() truncates toward zero
  return k < 1 ? 1 : k;
}

CHOCO_API size_t choco_topk_workspace_size(int64_t n) { return topk_ws_bytes(n); }

CHOCO_API int choco_topk_workspace_reset(const void* ws, size_t ws_bytes) {
  topk_warm_forget(ws, ws_bytes);
  seg_forget(ws, ws_bytes);
  randk_forget(ws, ws_bytes);
  return CHOCO_OK;
}

CHOCO_API int choco_topk_host_status(const void* ws, int32_t clear, void* stream) {
  const uint32_t v = host_status_read(ws, clear != 0);
  if (clear != 0 && v != 0u && ws != nullptr) {
    // the device word too (sticky, at CHOCO_TOPK_STATUS_OFFSET), behind the stream's work
    if (hipMemsetAsync(const_cast<void*>(ws), 0, sizeof(uint32_t), as_stream(stream)) != hipSuccess)
      return fail(CHOCO_ERR_HIP, "hipMemsetAsync failed");
  }
  return (int32_t)v;
}

CHOCO_API int choco_topk_set_warm_start(int32_t enable) {
  g_warm_on.store(enable != 0);
  return CHOCO_OK;
}

CHOCO_API int choco_topk_compress(const float* x, const float* xhat, int64_t n, int64_t k, float* out_val,
                                  int32_t* out_idx, void* ws, size_t ws_bytes, void* stream) {
  return dispatch_topk<kData>(x, xhat, n, k, 0, 1.0f, out_val, out_idx, 0, ws, ws_bytes, as_stream(stream));
}

CHOCO_API int choco_topk_compress_accumulate(const float* x, const float* xhat, int64_t n, int64_t k,
                                             float* out_val, int32_t* out_idx, float* hat_self, float* memory,
                                             float weight, void* ws, size_t ws_bytes, void* stream) {
  CHOCO_REQUIRE(hat_self != nullptr || memory != nullptr, "nothing to fold into (hat_self and memory are NULL)");
  CHOCO_REQUIRE((hat_self == nullptr || aligned4(hat_self)) && (memory == nullptr || aligned4(memory)),
                "hat_self / memory must be 4-byte aligned");
  return dispatch_topk<kData>(x, xhat, n, k, 0, 1.0f, out_val, out_idx, 0, ws, ws_bytes, as_stream(stream),
                              Gossip{nullptr, 0.f}, StatusSink{nullptr, nullptr}, Fold{hat_self, memory, weight});
}

CHOCO_API int choco_gossip_topk_compress_accumulate(float* x, float* memory, float* xhat, float gamma, int64_t n,
                                                    int64_t k, float* out_val, int32_t* out_idx, int32_t fold_memory,
                                                    float weight, void* ws, size_t ws_bytes, void* stream) {
  CHOCO_REQUIRE(memory != nullptr && xhat != nullptr, "the gossip step needs memory and x_hat");
  return dispatch_topk<kData>(x, xhat, n, k, 0, 1.0f, out_val, out_idx, 0, ws, ws_bytes, as_stream(stream),
                              Gossip{memory, gamma}, StatusSink{nullptr, nullptr},
                              Fold{xhat, fold_memory ? memory : nullptr, weight});
}

CHOCO_API int choco_gossip_topk_compress(float* x, const float* memory, const float* xhat, float gamma, int64_t n,
                                         int64_t k, float* out_val, int32_t* out_idx, void* ws, size_t ws_bytes,
                                         void* stream) {
  CHOCO_REQUIRE(memory != nullptr && xhat != nullptr, "the gossip step needs memory and x_hat");
  return dispatch_topk<kData>(x, xhat, n, k, 0, 1.0f, out_val, out_idx, 0, ws, ws_bytes, as_stream(stream),
                              Gossip{memory, gamma});
}

#if CHOCO_STAMPS
// Diagnostic builds only: re-launch the stream kernel alone `reps` times back to
// back (after one full choco_topk_compress on the same workspace set its
// thresholds), timed with dispatch-attached events -> *avg_ms.
CHOCO_API int choco_dbg_stream_only(const float* x, int64_t n, int64_t k, void* ws, size_t ws_bytes, int32_t reps,
                                    double* avg_ms, void* stream) {
  hipStream_t st = as_stream(stream);
  const TopkLayout L = topk_layout(n);
  CHOCO_REQUIRE(ws && ws_bytes >= L.total && reps > 0, "bad arguments");
  char* base = static_cast<char*>(ws);
  TopkCtrl* ctrl = reinterpret_cast<TopkCtrl*>(base + L.off_ctrl);
  // the window the next call would use; the totals it accumulates are garbage afterwards,
  // so the workspace is forgotten (its next call is cold: K1 re-zeroes them)
  uint32_t par = 0;
  {
    std::lock_guard<std::mutex> g(g_warm_mu);
    auto it = g_warm.find(ws);
    CHOCO_REQUIRE(it != g_warm.end(), "run choco_topk_compress on this workspace first");
    par = (uint32_t)(it->second.calls & 1u);
  }
  hipEvent_t a, b;
  CHOCO_HIP(hipEventCreate(&a));
  CHOCO_HIP(hipEventCreate(&b));
  CHOCO_HIP(hipEventRecord(a, st));
  for (int r = 0; r < reps; ++r)
    hipLaunchKernelGGL((topk_stream_kernel<kData, false>), dim3(L.nb), dim3(kK2Threads), 0, st, x, nullptr, n, k,
                       L.tile, L.nb, par, L.side_cap, (uint64_t)0, 0u, (uint64_t)0, ctrl,
                       reinterpret_cast<uint32_t*>(base + L.off_cum),
                       reinterpret_cast<uint32_t*>(base + L.off_cntw), reinterpret_cast<uint32_t*>(base + L.off_side),
                       reinterpret_cast<float*>(base + L.off_cval), reinterpret_cast<uint32_t*>(base + L.off_cidx),
                       reinterpret_cast<uint32_t*>(base + L.off_tinfo), Gossip{nullptr, 0.f}, SampleRanks{0u, 0u, 0u},
                       0u);
  CHOCO_HIP(hipEventRecord(b, st));
  CHOCO_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  CHOCO_HIP(hipEventElapsedTime(&ms, a, b));
  *avg_ms = ms / reps;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  topk_warm_forget(ws, 1);
  return CHOCO_OK;
}

// Diagnostic builds only: copy out (and clear) the phase stamps.
CHOCO_API int choco_dbg_stamps(unsigned long long* host, size_t bytes) {
  const size_t all = sizeof(unsigned long long) * kStampSlots * 4;
  if (bytes > all) bytes = all;
  if (host) CHOCO_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), bytes, 0, hipMemcpyDeviceToHost));
  static unsigned long long zeros[kStampSlots * 4];
  CHOCO_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), zeros, all, 0, hipMemcpyHostToDevice));
  return CHOCO_OK;
}
#endif
