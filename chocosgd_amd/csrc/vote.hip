// Majority vote over packed sign words (signSGD with majority vote, Bernstein et al. 2019; the
// reference's SignCompressor.majority_vote, dl_code/pcode/utils/sparsification.py:165-181):
// packed words in, the packed verdict out, no decode.
//     out[j] bit b = 1  <=>  2 * #{q : packed[q][j] bit b} > W
// A tie (even W) gives 0, which decodes as "+": what sign(sum of the decoded +-1) packs to.  All
// 32 bits of every word are voted; the (32, N') layout does not matter here.
//
// The kernel is word-parallel and bit-sliced.  A thread owns 4 consecutive words (one 16-byte
// non-temporal load per voter) and keeps the 32 x 4 running counts as 7 bit planes of 4 words:
// plane k holds bit k of every counter.  Voters go in eights through a carry-save tree (Harley
// and Seal's population count, turned sideways): planes 0 to 2 are the tree's ones, twos and
// fours accumulators, seven carry-save adders (xor3 + majority) take eight words in, and only
// the eights carry ripples through planes 3 to 6 -- 43 bit operations per 8 voters and word
// against 112 for eight ripples.  What is left goes in pairs (one adder, a ripple from plane 1),
// then a single word (a ripple from plane 0).  The eight loads of a block are independent of
// the planes and stand in front of its first adder.
// The comparison is bit-sliced as well and costs nothing per voter: the planes start at
// 64 - T, T = W / 2 + 1 (workgroup-uniform), so that count >= T <=> plane 6 of the sum is set
// (count <= W <= 64 and T >= 1: the sum stays below 128).  The verdict is plane 6.
// No LDS, no atomics, no per-bit loop.  The voter pointers travel in the kernel arguments (64
// pointers, 512 B); the voter loop is uniform, so they are scalar loads.
// `out` may be any one of the inputs: a thread reads all its inputs before it writes, and no
// two threads share a word.
// Pointers that are not all 16-byte aligned take the same kernel with one word per thread
// (chosen once on the host); the nwords mod 4 tail of the vector form is voted word by word by
// one thread of the same launch.
#include "choco_common.h"

namespace choco {

constexpr int kVoteMax = 64;  // voters of one call
constexpr int kVoteThreads = 256;
constexpr int kVotePlanes = 7;                  // counts up to 127
constexpr int64_t kVoteMaxWords = int64_t(1) << 26;  // the sign wire's bound: n < 2^31

struct VoteMsgs {
  const uint32_t* p[kVoteMax];
};

typedef uint32_t choco_u32x4 __attribute__((ext_vector_type(4)));

template <int L>
CHOCO_DEV void vote_ld(const uint32_t* p, int64_t i, uint32_t (&v)[L]) {
  if constexpr (L == 4) {
    const choco_u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const choco_u32x4*>(p + i));
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = __builtin_nontemporal_load(p + i);
  }
}

// acc + x + y = acc' + 2 carry, bit by bit
CHOCO_DEV void vote_csa(uint32_t& acc, uint32_t x, uint32_t y, uint32_t& carry) {
  const uint32_t u = acc ^ x;
  carry = (acc & x) | (u & y);
  acc = u ^ y;
}

// counters += x << K0
template <int K0, int L>
CHOCO_DEV void vote_ripple(uint32_t (&c)[kVotePlanes][L], int l, uint32_t x) {
#pragma unroll
  for (int k = K0; k < kVotePlanes; ++k) {
    const uint32_t t = c[k][l] & x;
    c[k][l] ^= x;
    x = t;
  }
}

// the verdict of words [i, i + L)
template <int L>
CHOCO_DEV void vote_words(const VoteMsgs& M, int W, uint32_t bias, int64_t i, uint32_t* out) {
  uint32_t c[kVotePlanes][L];
#pragma unroll
  for (int k = 0; k < kVotePlanes; ++k)
#pragma unroll
    for (int l = 0; l < L; ++l) c[k][l] = 0u - ((bias >> k) & 1u);
  int q = 0;
#pragma unroll 1
  for (; q + 8 <= W; q += 8) {
    uint32_t x[8][L];
#pragma unroll
    for (int u = 0; u < 8; ++u) vote_ld<L>(M.p[q + u], i, x[u]);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      uint32_t ta, tb, tc, td, fa, fb, e;
      vote_csa(c[0][l], x[0][l], x[1][l], ta);
      vote_csa(c[0][l], x[2][l], x[3][l], tb);
      vote_csa(c[1][l], ta, tb, fa);
      vote_csa(c[0][l], x[4][l], x[5][l], tc);
      vote_csa(c[0][l], x[6][l], x[7][l], td);
      vote_csa(c[1][l], tc, td, fb);
      vote_csa(c[2][l], fa, fb, e);
      vote_ripple<3, L>(c, l, e);
    }
  }
#pragma unroll 1
  for (; q + 2 <= W; q += 2) {
    uint32_t x[2][L];
    vote_ld<L>(M.p[q], i, x[0]);
    vote_ld<L>(M.p[q + 1], i, x[1]);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      uint32_t t;
      vote_csa(c[0][l], x[0][l], x[1][l], t);
      vote_ripple<1, L>(c, l, t);
    }
  }
  if (q < W) {
    uint32_t x[L];
    vote_ld<L>(M.p[q], i, x);
#pragma unroll
    for (int l = 0; l < L; ++l) vote_ripple<0, L>(c, l, x[l]);
  }
  if constexpr (L == 4) {
    choco_u32x4 o;
    o.x = c[6][0]; o.y = c[6][1]; o.z = c[6][2]; o.w = c[6][3];
    *reinterpret_cast<choco_u32x4*>(out + i) = o;
  } else {
    out[i] = c[6][0];
  }
}

// L words per thread: 4 (every pointer 16-byte aligned) or 1.  Thread g < nwords / L owns words
// [g L, g L + L); thread nwords / L votes the nwords mod L tail word by word.
template <int L>
__global__ __launch_bounds__(kVoteThreads) void sign_vote_kernel(const VoteMsgs M, int W, int64_t nwords,
                                                                 uint32_t* out) {
  const uint32_t bias = 64u - (uint32_t)(W / 2 + 1);
  const int64_t g = (int64_t)blockIdx.x * kVoteThreads + threadIdx.x;
  const int64_t nvec = nwords / L;
  if (g < nvec) {
    vote_words<L>(M, W, bias, g * L, out);
  } else if (L > 1 && g == nvec) {
    for (int64_t i = nvec * L; i < nwords; ++i) vote_words<1>(M, W, bias, i, out);
  }
}

// Every argument is checked before the launch, with no HIP call.
static int vote_check(const int32_t* const* packed_list, int32_t nvoters, int64_t nwords, const int32_t* out) {
  CHOCO_REQUIRE(packed_list && out, "null pointer");
  CHOCO_REQUIRE(nvoters >= 1 && nvoters <= kVoteMax, "nvoters must be in [1, %d], got %d", kVoteMax, (int)nvoters);
  CHOCO_REQUIRE(nwords >= 0 && nwords <= kVoteMaxWords, "nwords must be in [0, 2^26], got %lld", (long long)nwords);
  CHOCO_REQUIRE(aligned4(out), "out must be 4-byte aligned");
  for (int32_t q = 0; q < nvoters; ++q) {
    CHOCO_REQUIRE(packed_list[q], "voter %d: null pointer", (int)q);
    CHOCO_REQUIRE(aligned4(packed_list[q]), "voter %d: must be 4-byte aligned", (int)q);
  }
  return CHOCO_OK;
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_sign_vote(const int32_t* const* packed_list, int32_t nvoters, int64_t nwords, int32_t* out,
                              void* stream) {
  CHOCO_TRY(vote_check(packed_list, nvoters, nwords, out));
  if (nwords == 0) return CHOCO_OK;
  VoteMsgs M;
  bool vec = aligned16(out);
  for (int q = 0; q < kVoteMax; ++q) {
    M.p[q] = q < nvoters ? reinterpret_cast<const uint32_t*>(packed_list[q]) : nullptr;
    vec = vec && aligned16(M.p[q]);
  }
  uint32_t* o = reinterpret_cast<uint32_t*>(out);
  const hipStream_t st = as_stream(stream);
  if (!vec) {
    const unsigned grid = (unsigned)((nwords + kVoteThreads - 1) / kVoteThreads);
    return CHOCO_LAUNCH("sign_vote_kernel", "sign_vote_kernel", sign_vote_kernel<1>, dim3(grid), dim3(kVoteThreads),
                        st, M, (int)nvoters, nwords, o);
  }
  const int64_t units = nwords / 4 + (nwords % 4 ? 1 : 0);
  const unsigned grid = (unsigned)((units + kVoteThreads - 1) / kVoteThreads);
  return CHOCO_LAUNCH("sign_vote_kernel", "sign_vote_kernel", sign_vote_kernel<4>, dim3(grid), dim3(kVoteThreads), st,
                      M, (int)nvoters, nwords, o);
}
