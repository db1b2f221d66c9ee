// Evaluation: the confusion counts behind mmseg's IoUMetric (configs/base_config.py:19 test_evaluator, which the reference's eval.py runs
// through runner.test() and reports, eval.py:94-95; mmseg intersect_and_union: mask by ignore_index, then three torch.histc over the
// classes -- on the CPU, per image, in the reference).
//   confusion : one pass over (label, truth) pairs -> counts[(K+1)][(K+1)], row = prediction, column = truth, index K = outside [0,K)
// Integers end to end: 32-bit counts in an LDS table per workgroup, folded into the int64 table with one 64-bit add per non-zero bin
// per workgroup.  Integer adds commute, so the table is byte-identical whatever the launch shape or arrival order.
// HBM-bound: 9 B per pixel (int64 label + u8 truth), 16 B with int64 truth; one pass.
#include "common.h"

namespace sg {

constexpr int CF_RUN = 16;                       // consecutive pixels per lane per step: 128 B of labels, one 16-B load of u8 truth
constexpr int CF_MAX_K = 127;                    // (K+1)^2 32-bit counts <= 64 KiB of LDS: two workgroups per CU at the largest K
constexpr int CF_WG_PER_CU = 4;
constexpr int64_t CF_MAX_PIXELS = (int64_t)1 << 40;   // the grid is raised so that a workgroup sees < 2^32 pixels: no 32-bit count wraps

// steps 2-4 of the entry's contract for one pixel: the bin, or -1 for an ignored pixel.  G = int for u8 truth, int64_t otherwise.
template <typename G>
__device__ __forceinline__ int confusion_bin(int64_t p, G g, int K, int ignore_index, int reduce_zero_label) {
  if (reduce_zero_label) g = (g == 0 || g == 255) ? (G)255 : g - 1;          // mmseg LoadAnnotations: 0 -> 255, 255 stays, else g - 1
  if (g == (G)ignore_index) return -1;
  const int pp = (uint64_t)p < (uint64_t)K ? (int)p : K;
  const int gg = (uint64_t)(int64_t)g < (uint64_t)K ? (int)g : K;
  return pp * (K + 1) + gg;
}

// Real masks are flat areas: a whole wave on one bin is the common case, and 64 lanes adding 1 to one LDS address serialise.  So
// (1) a lane takes CF_RUN consecutive pixels and merges equal neighbours in registers into (bin, length) runs;
// (2) run slot by run slot the wave combines by leader match: the lanes whose bin equals the first remaining lane's are found with
//     one ballot, their lengths summed with five more (lengths fit 5 bits), and one lane adds the sum.  After two rounds, once a round
//     matches fewer than 4 lanes (the data is not flat here), the rest go to the LDS atomic unit directly.
// A uniform 1024-pixel stretch costs one LDS add per wave step; slots a wave does not use are skipped on the scalar unit.
template <bool GT64>
__global__ __launch_bounds__(256) void confusion_kernel(const int64_t* __restrict__ labels, const void* __restrict__ gtv, int64_t n,
                                                        int head, int64_t nchunks, int K, int ignore_index, int reduce_zero_label,
                                                        unsigned long long* __restrict__ table) {
  extern __shared__ uint32_t cf_bins[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = (K + 1) * (K + 1);
  const uint8_t* gt8 = reinterpret_cast<const uint8_t*>(gtv);
  const int64_t* gt64 = reinterpret_cast<const int64_t*>(gtv);
  for (int i = tid; i < nb; i += 256) cf_bins[i] = 0u;
  __syncthreads();

  // the unaligned head (pixels before the first 16-byte boundary of the u8 truth) and the tail (< CF_RUN pixels): one pixel per thread.
  // A buffer shorter than the unaligned head (the host clamps head to n, nchunks = 0) is counted entirely here; the loop below then
  // does not run.
  if (blockIdx.x == 0 && tid < 2 * CF_RUN) {
    const int64_t i = tid < CF_RUN ? (tid < head ? (int64_t)tid : -1) : head + nchunks * CF_RUN + (tid - CF_RUN);
    if (i >= 0 && i < n) {
      const int b = GT64 ? confusion_bin<int64_t>(labels[i], gt64[i], K, ignore_index, reduce_zero_label)
                         : confusion_bin<int>(labels[i], (int)gt8[i], K, ignore_index, reduce_zero_label);
      if (b >= 0) atomicAdd(&cf_bins[b], 1u);
    }
  }

  for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 64; base < nchunks; base += (int64_t)gridDim.x * 256) {
    const int64_t c = base + lane;
    int b[CF_RUN];
#pragma unroll
    for (int j = 0; j < CF_RUN; ++j) b[j] = -1;
    if (c < nchunks) {
      const int64_t i0 = head + c * CF_RUN;
      int64_t p[CF_RUN];
      __builtin_memcpy(p, labels + i0, sizeof(p));                       // 8-byte aligned: flush-group offsets are not multiples of 16
      if (GT64) {
        int64_t g[CF_RUN];
        __builtin_memcpy(g, gt64 + i0, sizeof(g));
#pragma unroll
        for (int j = 0; j < CF_RUN; ++j) b[j] = confusion_bin<int64_t>(p[j], g[j], K, ignore_index, reduce_zero_label);
      } else {
        const uint4 q = *reinterpret_cast<const uint4*>(gt8 + i0);       // 16-byte aligned by the choice of `head`
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < CF_RUN; ++j)
          b[j] = confusion_bin<int>(p[j], (int)((w[j >> 2] >> (8 * (j & 3))) & 255u), K, ignore_index, reduce_zero_label);
      }
    }
    // run lengths: len[j] = pixels of the run that starts at j (meaningful where b[j] != b[j-1]); ignored pixels form runs too, never added
    int len[CF_RUN];
    len[CF_RUN - 1] = 1;
#pragma unroll
    for (int j = CF_RUN - 2; j >= 0; --j) len[j] = b[j] == b[j + 1] ? len[j + 1] + 1 : 1;
#pragma unroll
    for (int j = 0; j < CF_RUN; ++j) {
      bool act = b[j] >= 0 && (j == 0 || b[j] != b[j - 1]);
      unsigned long long rem = __ballot(act);
      int rounds = 0;
      while (rem != 0ull) {                                              // wave-uniform
        const int src = __ffsll((long long)rem) - 1;
        const int lb = __builtin_amdgcn_readlane(b[j], src);
        const bool m = act && b[j] == lb;
        const unsigned long long mm = __ballot(m);
        int total = 0;
#pragma unroll
        for (int bit = 0; bit < 5; ++bit) total += __popcll(__ballot(m && ((len[j] >> bit) & 1))) << bit;
        if (lane == src) atomicAdd(&cf_bins[lb], (uint32_t)total);
        act = act && !m;
        rem &= ~mm;
        if (++rounds >= 2 && __popcll(mm) < 4) break;
      }
      if (act) atomicAdd(&cf_bins[b[j]], (uint32_t)len[j]);
    }
  }
  __syncthreads();
  for (int i = tid; i < nb; i += 256) {
    const uint32_t v = cf_bins[i];
    if (v != 0u) atomicAdd(&table[i], (unsigned long long)v);
  }
}

}  // namespace sg

using namespace sg;

extern "C" int sg_confusion_accumulate(const int64_t* labels, const void* gt, int gt_format, int64_t n_pixels, int K, int ignore_index,
                                       int reduce_zero_label, int64_t* table, sg_stream s) {
  SG_REQUIRE(labels && gt && table, "sg_confusion_accumulate: null pointer");
  SG_REQUIRE(gt_format == SG_GT_U8 || gt_format == SG_GT_I64, "sg_confusion_accumulate: unknown ground-truth format %d", gt_format);
  SG_REQUIRE(K >= 1, "sg_confusion_accumulate: K=%d, need at least one class", K);
  SG_REQUIRE(K <= CF_MAX_K, "sg_confusion_accumulate: K=%d exceeds %d (the per-workgroup table of (K+1)^2 32-bit counts must fit 64 KiB of LDS)",
             K, CF_MAX_K);
  SG_REQUIRE(n_pixels >= 0 && n_pixels <= CF_MAX_PIXELS, "sg_confusion_accumulate: n_pixels=%lld outside [0, 2^40]", (long long)n_pixels);
  SG_REQUIRE((((uintptr_t)labels) & 7) == 0 && (gt_format == SG_GT_U8 || (((uintptr_t)gt) & 7) == 0) && (((uintptr_t)table) & 7) == 0,
             "sg_confusion_accumulate: int64 buffers must be 8-byte aligned");
  if (n_pixels == 0) return SG_OK;
  const bool gt64 = gt_format == SG_GT_I64;
  int64_t head = gt64 ? 0 : (int64_t)((16 - (((uintptr_t)gt) & 15)) & 15);
  if (head > n_pixels) head = n_pixels;
  const int64_t nchunks = (n_pixels - head) / CF_RUN;
  const size_t lds = (size_t)(K + 1) * (K + 1) * sizeof(uint32_t);
  auto kern = gt64 ? confusion_kernel<true> : confusion_kernel<false>;
  if (lds > 48 * 1024) SG_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds));
  int64_t blocks = cdiv(nchunks, 256);
  const int64_t cap = (int64_t)device_cu_count() * CF_WG_PER_CU;
  blocks = blocks < 1 ? 1 : (blocks > cap ? cap : blocks);
  if (blocks < cdiv(n_pixels, (int64_t)1 << 31)) blocks = cdiv(n_pixels, (int64_t)1 << 31);     // a workgroup's 32-bit counts stay below 2^32
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, as_stream(s), labels, gt, n_pixels, (int)head, nchunks, K, ignore_index,
                     reduce_zero_label, reinterpret_cast<unsigned long long*>(table));
  SG_LAUNCH_CHECK();
  return SG_OK;
}
