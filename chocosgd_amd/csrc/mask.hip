// DGC's momentum-factor masking and the clear of the error-feedback memory at the selected
// positions (dl_code/pcode/optim/dgc.py:174-182), for a whole parameter list in one batched
// launch per chunk of tensors.  The segmented top-k / random-k has produced values[k] and
// ascending GLOBAL indices[k], k_per_seg[s] of them for tensor s (slots koff[s] .. koff[s+1]).
// Per slot j of tensor s, with i = indices[j] inside the tensor's flat range [off[s], off[s+1]):
//     bufs[s][i - off[s]] = rnd(buf * 0.0f)        buf.mul_(nmask), nmask = 1 - mask: a finite
//                                                  value keeps its sign (-3 -> -0), inf / NaN -> NaN
//     memory[i]           = values[j] + (-values[j])   what sparse_accumulate(-values) leaves
// An index outside its tensor's range is skipped, as the sparse receivers skip out-of-range
// indices.  Only the selected elements are written (2-byte stores for 16-bit buffers).
//
// The grid walks the SLOT space the way the parameter bridge walks the flat space: workgroups
// own kMaskTile consecutive slots, the chunk's table (buffer pointers, flat offsets, slot
// offsets, dtype codes) travels in the kernel arguments, the first tensor of a tile is found by
// the uniform upper-bound search over the slot offsets and the walk from there is
// workgroup-uniform, so the table is only ever indexed with a uniform value.  A tensor's slots
// inside a tile are taken by one wave (the waves take the tensors in turn: the 3000 x 100
// layout at ratio 0.9 has 10 slots per tensor) or, past kMaskWaveMax slots, by the workgroup.
#include "param_common.h"

namespace choco {

constexpr int kMaskCap = 128;         // tensors per launch
constexpr int64_t kMaskTile = 2048;   // slots per workgroup
constexpr int64_t kMaskWaveMax = 256;

struct MaskTable {
  void* buf[kMaskCap];
  int64_t off[kMaskCap + 1];   // absolute flat offsets
  int64_t koff[kMaskCap + 1];  // absolute slot offsets
  uint8_t dt[kMaskCap];
  int32_t nt;
};
// the table, three pointers and a word
static_assert(sizeof(MaskTable) + 32 <= 4096 - 256, "MaskTable must fit in the kernel arguments");

CHOCO_DEV void mask_slot(void* buf, int dt, int64_t o0, int64_t o1, const float* __restrict__ values,
                         const int32_t* __restrict__ indices, float* memory, int64_t j) {
  const int64_t i = indices[j];
  if (i < o0 || i >= o1) return;
  if (buf) for_dtype(dt, [&](auto DT) { st1<DT>(buf, i - o0, __fmul_rn(ld1<DT>(buf, i - o0), 0.0f)); });
  if (memory) {
    const float v = values[j];
    memory[i] = v + (-v);
  }
}

__global__ __launch_bounds__(kPbThreads) void param_mask_kernel(const MaskTable tb, const float* values,
                                                                const int32_t* indices, float* memory,
                                                                int64_t tile0) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  int nshort = 0;
  // the shared walk over the slot offsets: [a, b) are tensor s's slots in this workgroup's tile
  tile_walk(tb.koff, tb.nt, tile0 + blockIdx.x, [&](int s, int64_t a, int64_t b) {
    void* buf = tb.buf[s];
    if (!buf && !memory) return;
    const int dt = tb.dt[s];
    const int64_t o0 = tb.off[s], o1 = tb.off[s + 1];
    if (b - a <= kMaskWaveMax) {
      const bool mine = (nshort & 3) == wave;
      ++nshort;
      if (!mine) return;
      for (int64_t j = a + lane; j < b; j += 64) mask_slot(buf, dt, o0, o1, values, indices, memory, j);
    } else {
      for (int64_t j = a + tid; j < b; j += kPbThreads) mask_slot(buf, dt, o0, o1, values, indices, memory, j);
    }
  }, kMaskTile);
}

struct MaskArgs {
  void* const* bufs;
  const int64_t* lens;
  const int32_t* dtypes;
  const int64_t* kseg;
  int32_t nseg;
  const float* values;
  const int32_t* indices;
  int64_t k;
  float* memory;
  int64_t n;
};

// Every argument is checked before the first launch, with no HIP call.
static int mask_check(const MaskArgs& a) {
  CHOCO_REQUIRE(a.bufs && a.lens && a.dtypes && a.kseg, "null table argument");
  int64_t ksum = 0;
  bool any = a.memory != nullptr;
  CHOCO_TRY(layout_check(
      a.lens, a.dtypes, a.nseg, a.n,
      [&]() -> int {
        CHOCO_REQUIRE(a.k >= 0 && a.k <= a.n, "k must be in [0, n], got %lld", (long long)a.k);
        CHOCO_REQUIRE(a.k == 0 || (a.values && a.indices), "null values or indices with k > 0");
        CHOCO_REQUIRE(aligned4(a.values) && aligned4(a.indices) && aligned4(a.memory),
                      "values, indices and memory must be 4-byte aligned");
        return CHOCO_OK;
      },
      [&](int32_t s, uintptr_t esz) -> int {
        CHOCO_REQUIRE(a.kseg[s] >= 0 && a.kseg[s] <= a.lens[s], "tensor %d: k_per_seg outside [0, length]", (int)s);
        ksum += a.kseg[s];
        CHOCO_REQUIRE(elem_aligned(a.bufs[s], esz), "tensor %d: pointer not aligned to its element size", (int)s);
        any = any || a.bufs[s] != nullptr;
        return CHOCO_OK;
      }));
  CHOCO_REQUIRE(ksum == a.k, "k_per_seg adds up to %lld, k is %lld", (long long)ksum, (long long)a.k);
  CHOCO_REQUIRE(any, "nothing to write: memory is null and so is every buffer");
  return CHOCO_OK;
}

static int mask_run(const MaskArgs& a, hipStream_t st) {
  const int rc = mask_check(a);
  if (rc) return rc;
  MaskTable tb;
  int64_t base = 0;
  // the grid walks the slot offsets; a chunk without a slot still takes its launch
  return for_chunks<kMaskCap>(a.kseg, a.nseg, tb.koff, [&](const Chunk& c) -> int {
    tb.nt = c.nt;
    base = chunk_offsets<kMaskCap>(a.lens, c.s0, c.nt, base, tb.off);
    for (int i = 0; i < kMaskCap; ++i) {
      const bool in = i < c.nt;
      tb.buf[i] = in ? a.bufs[c.s0 + i] : nullptr;
      tb.dt[i] = in ? (uint8_t)a.dtypes[c.s0 + i] : (uint8_t)0;
    }
    return CHOCO_LAUNCH("param_mask_kernel", "param_mask_kernel", param_mask_kernel, dim3((unsigned)c.tiles),
                        dim3(kPbThreads), st, tb, a.values, a.indices, a.memory, c.tile0);
  }, kMaskTile);
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_params_mask_launches(int32_t nseg) { return chunk_launches(nseg, kMaskCap); }

CHOCO_API int choco_params_mask(void* const* bufs, const int64_t* lens, const int32_t* dtypes, const int64_t* k_per_seg,
                                int32_t nseg, const float* values, const int32_t* indices, int64_t k, float* memory,
                                int64_t n, void* stream) {
  const MaskArgs a{bufs, lens, dtypes, k_per_seg, nseg, values, indices, k, memory, n};
  return mask_run(a, as_stream(stream));
}
