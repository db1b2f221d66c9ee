// area_thd: per-image suppression of small-area classes (the option of that name in the training-free segmenter family; the
// definition is the comment block of these entries in include/segearth_hip.h).  Three small kernels around the heads:
//   class_area   : first-pass labels -> counts int64 [K] per image.  confusion_kernel's scheme (csrc/metric.hip): 32-bit bins in LDS per
//                  workgroup, runs merged in registers, the wave-uniform leader match for flat areas, one 64-bit add per non-zero bin
//                  into the global row.  Integers end to end: byte-identical whatever the launch shape or arrival order.
//   area_keep    : counts -> keep int32 [K] per image, the comparison in double on the device (no count ever visits the host).
//   area_filter  : probs [K,HW] in place (dropped planes zeroed) and the final labels from the first-pass labels; comparisons only.
// The labels-only form with no probability planes (sg_area_relabel) lives in head.hip beside label_head_block, whose gather it repeats.
// HBM-bound: class_area reads 8 B per pixel; area_filter reads 8 B and writes 8 B + 4 B per dropped class per pixel, and reads one plane
// (a pixel whose first label is kept) or the kept planes (a pixel whose first label is dropped).
#include "common.h"

namespace sg {

constexpr int CA_RUN = 16;                         // consecutive pixels per lane per step: 128 B of labels
constexpr int CA_SPAN = 256 * CA_RUN;              // pixels per workgroup step; a block of the multi form owns one span of one image
constexpr int CA_MAX_K = SG_AREA_MAX_K;            // 16 KiB of 32-bit bins: far more than two workgroups per CU fit the 160 KiB of LDS
constexpr int CA_WG_PER_CU = 4;
constexpr int64_t CA_MAX_PIXELS = (int64_t)1 << 40;

// Pixels [lo, hi) of `labels` for one wave step: the lane's CA_RUN consecutive labels starting at i0 (lanes past hi hold nothing) are
// merged into runs and added to the workgroup's bins.  A label outside [0,K) is bin -1 and never added.
__device__ __forceinline__ void class_area_step(const int64_t* __restrict__ labels, int64_t i0, int64_t hi, int K, uint32_t* bins,
                                                int lane) {
  int b[CA_RUN];
  if (i0 + CA_RUN <= hi) {
    int64_t p[CA_RUN];
    __builtin_memcpy(p, labels + i0, sizeof(p));                         // 8-byte aligned: image offsets are not multiples of 16
#pragma unroll
    for (int j = 0; j < CA_RUN; ++j) b[j] = (uint64_t)p[j] < (uint64_t)K ? (int)p[j] : -1;
  } else {
#pragma unroll
    for (int j = 0; j < CA_RUN; ++j) {
      const int64_t p = i0 + j < hi ? labels[i0 + j] : -1;
      b[j] = (uint64_t)p < (uint64_t)K ? (int)p : -1;
    }
  }
  // run lengths: len[j] = pixels of the run that starts at j (meaningful where b[j] != b[j-1])
  int len[CA_RUN];
  len[CA_RUN - 1] = 1;
#pragma unroll
  for (int j = CA_RUN - 2; j >= 0; --j) len[j] = b[j] == b[j + 1] ? len[j + 1] + 1 : 1;
#pragma unroll
  for (int j = 0; j < CA_RUN; ++j) {
    bool act = b[j] >= 0 && (j == 0 || b[j] != b[j - 1]);
    unsigned long long rem = __ballot(act);
    int rounds = 0;
    while (rem != 0ull) {                                                // wave-uniform: leader match, as confusion_kernel
      const int src = __ffsll((long long)rem) - 1;
      const int lb = __builtin_amdgcn_readlane(b[j], src);
      const bool m = act && b[j] == lb;
      const unsigned long long mm = __ballot(m);
      int total = 0;
#pragma unroll
      for (int bit = 0; bit < 5; ++bit) total += __popcll(__ballot(m && ((len[j] >> bit) & 1))) << bit;
      if (lane == src) atomicAdd(&bins[lb], (uint32_t)total);
      act = act && !m;
      rem &= ~mm;
      if (++rounds >= 2 && __popcll(mm) < 4) break;
    }
    if (act) atomicAdd(&bins[b[j]], (uint32_t)len[j]);
  }
}

__device__ __forceinline__ void class_area_flush(const uint32_t* bins, int K, unsigned long long* __restrict__ counts) {
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += 256) {
    const uint32_t v = bins[i];
    if (v != 0u) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

// One image: the grid strides over spans of CA_SPAN pixels.
__global__ __launch_bounds__(256) void class_area_kernel(const int64_t* __restrict__ labels, int64_t n, int K,
                                                         unsigned long long* __restrict__ counts) {
  extern __shared__ uint32_t ca_bins[];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < K; i += 256) ca_bins[i] = 0u;
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * CA_SPAN; base < n; base += (int64_t)gridDim.x * CA_SPAN) {
    const int64_t i0 = base + (int64_t)tid * CA_RUN;
    if (base + (int64_t)(tid - lane) * CA_RUN < n)                       // wave-uniform: the wave holds a pixel
      class_area_step(labels, i0, n, K, ca_bins, lane);
  }
  class_area_flush(ca_bins, K, counts);
}

// N images in one flat label buffer: image n holds image_pixels[n] labels at out_offset[n]; its blocks, one span each, follow
// block_prefix[n].  A block never straddles two images, so its bins fold into one row of counts [N,K].
__global__ __launch_bounds__(256) void class_area_multi_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ image_pixels,
                                                               const int64_t* __restrict__ out_offset,
                                                               const int64_t* __restrict__ block_prefix, int N, int64_t out_pixels, int K,
                                                               unsigned long long* __restrict__ counts) {
  extern __shared__ uint32_t ca_bins[];
  const int tid = threadIdx.x, lane = tid & 63;
  int lo = 0, hi = N;                                                    // largest n with block_prefix[n] <= blockIdx.x (skips empty images)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (block_prefix[mid] <= (int64_t)blockIdx.x) lo = mid; else hi = mid;
  }
  const int n = lo;
  const int64_t np = image_pixels[n], off = out_offset[n];
  if (np <= 0 || off < 0 || off + np > out_pixels) return;               // a descriptor that leaves the buffer: block-uniform, before any barrier
  const int64_t base = ((int64_t)blockIdx.x - block_prefix[n]) * CA_SPAN;
  if (base >= np) return;
  for (int i = tid; i < K; i += 256) ca_bins[i] = 0u;
  __syncthreads();
  if (base + (int64_t)(tid - lane) * CA_RUN < np)                        // wave-uniform
    class_area_step(labels + off, base + (int64_t)tid * CA_RUN, np, K, ca_bins, lane);
  class_area_flush(ca_bins, K, counts + (int64_t)n * K);
}

// One workgroup per image: total = sum of the non-background counts, then keep[c] = c == bg_idx || (double)area[c] > area_thd * (double)total.
// The int64 sum is exact and order-free; both conversions and the product are IEEE double, evaluated once per class.
__global__ __launch_bounds__(256) void area_keep_kernel(const int64_t* __restrict__ counts, int K, int bg_idx, double area_thd,
                                                        int32_t* __restrict__ keep) {
  __shared__ long long s_part[256];
  const int64_t* row = counts + (int64_t)blockIdx.x * K;
  long long part = 0;
  for (int c = threadIdx.x; c < K; c += 256)
    if (c != bg_idx) part += row[c];
  s_part[threadIdx.x] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_part[threadIdx.x] += s_part[threadIdx.x + o];
    __syncthreads();
  }
  const double bound = area_thd * (double)s_part[0];
  for (int c = threadIdx.x; c < K; c += 256) keep[(int64_t)blockIdx.x * K + c] = (c == bg_idx || (double)row[c] > bound) ? 1 : 0;
}

// Pixel i of one image: steps 4 and 5 of the definition.  Comparisons and stores only, no arithmetic.  keep[] is read with a
// wave-uniform index (the scalar unit); a pixel whose first label is kept reads p[l0] alone, one whose first label is dropped takes the
// first maximum over the kept planes (the background is always kept, so there is one).
// labels_in and labels_out may be one buffer: a pixel's thread reads its label before it writes it.
__device__ __forceinline__ void area_filter_pixel(float* __restrict__ probs, const int64_t* labels_in, int64_t* labels_out, const int32_t* __restrict__ keep, int K, int64_t HW,
                                                  int64_t i, float prob_thd, int bg_idx) {
  const int64_t l0 = labels_in[i];
  const bool kept = (uint64_t)l0 < (uint64_t)K && keep[l0] != 0;
  float best = -INFINITY;
  int arg = bg_idx;
  if (kept) { best = probs[l0 * HW + i]; arg = (int)l0; }
  for (int c = 0; c < K; ++c) {
    if (keep[c] == 0) {
      probs[c * HW + i] = 0.f;
    } else if (!kept) {
      const float v = probs[c * HW + i];
      if (v > best) { best = v; arg = c; }                               // first maximum wins
    }
  }
  labels_out[i] = best < prob_thd ? bg_idx : arg;
}

__global__ __launch_bounds__(256) void area_filter_kernel(float* __restrict__ probs, const int64_t* labels_in, int64_t* labels_out,
                                                          const int32_t* __restrict__ keep, int K,
                                                          int64_t HW, float prob_thd, int bg_idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  area_filter_pixel(probs, labels_in, labels_out, keep, K, HW, i, prob_thd, bg_idx);
}

// sg_postprocess_multi's output layout: image n of out_hw[n] pixels has its labels at out_offset[n] and its probs [K,H,W] at
// K * out_offset[n]; 256 pixels per block after block_prefix[n].
__global__ __launch_bounds__(256) void area_filter_multi_kernel(float* __restrict__ probs, const int64_t* labels_in, int64_t* labels_out,
                                                                const int32_t* __restrict__ keep,
                                                                const int32_t* __restrict__ out_hw, const int64_t* __restrict__ out_offset,
                                                                const int64_t* __restrict__ block_prefix, int N, int64_t out_pixels, int K,
                                                                float prob_thd, int bg_idx) {
  int lo = 0, hi = N;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (block_prefix[mid] <= (int64_t)blockIdx.x) lo = mid; else hi = mid;
  }
  const int n = lo;
  const int64_t HW = (int64_t)out_hw[2 * n] * out_hw[2 * n + 1], off = out_offset[n];
  if (HW <= 0 || off < 0 || off + HW > out_pixels) return;
  const int64_t i = ((int64_t)blockIdx.x - block_prefix[n]) * 256 + threadIdx.x;
  if (i >= HW) return;
  area_filter_pixel(probs + (int64_t)K * off, labels_in + off, labels_out + off, keep + (int64_t)n * K, K, HW, i, prob_thd, bg_idx);
}

}  // namespace sg

using namespace sg;

#define SG_AREA_K(name, K) \
  SG_REQUIRE((K) >= 1 && (K) <= CA_MAX_K, name ": K=%d outside [1, %d] (SG_AREA_MAX_K: the per-workgroup table of K 32-bit counts in LDS)", (K), CA_MAX_K)

extern "C" int sg_class_area(const int64_t* labels, int64_t n_pixels, int K, int64_t* counts, sg_stream s) {
  SG_REQUIRE(labels && counts, "sg_class_area: null pointer");
  SG_AREA_K("sg_class_area", K);
  SG_REQUIRE(n_pixels >= 0 && n_pixels <= CA_MAX_PIXELS, "sg_class_area: n_pixels=%lld outside [0, 2^40]", (long long)n_pixels);
  SG_REQUIRE((((uintptr_t)labels) & 7) == 0 && (((uintptr_t)counts) & 7) == 0, "sg_class_area: int64 buffers must be 8-byte aligned");
  if (n_pixels == 0) return SG_OK;
  int64_t blocks = cdiv(n_pixels, CA_SPAN);
  const int64_t cap = (int64_t)device_cu_count() * CA_WG_PER_CU;
  blocks = blocks > cap ? cap : blocks;
  if (blocks < cdiv(n_pixels, (int64_t)1 << 31)) blocks = cdiv(n_pixels, (int64_t)1 << 31);   // a workgroup's 32-bit counts stay below 2^32
  hipLaunchKernelGGL(class_area_kernel, dim3((unsigned)blocks), dim3(256), (size_t)K * sizeof(uint32_t), as_stream(s), labels, n_pixels, K,
                     reinterpret_cast<unsigned long long*>(counts));
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_class_area_multi(const int64_t* labels, const int64_t* image_pixels, const int64_t* out_offset, const int64_t* block_prefix,
                                   int N, int64_t total_blocks, int64_t out_pixels, int K, int64_t* counts, sg_stream s) {
  SG_REQUIRE(labels && image_pixels && out_offset && block_prefix && counts, "sg_class_area_multi: null pointer");
  SG_AREA_K("sg_class_area_multi", K);
  SG_REQUIRE(N > 0, "sg_class_area_multi: N=%d images", N);
  SG_REQUIRE(total_blocks > 0 && total_blocks <= INT32_MAX, "sg_class_area_multi: total_blocks=%lld outside (0, 2^31)", (long long)total_blocks);
  SG_REQUIRE(out_pixels > 0, "sg_class_area_multi: out_pixels=%lld holds no image", (long long)out_pixels);
  SG_REQUIRE((((uintptr_t)labels) & 7) == 0 && (((uintptr_t)counts) & 7) == 0, "sg_class_area_multi: int64 buffers must be 8-byte aligned");
  hipLaunchKernelGGL(class_area_multi_kernel, dim3((unsigned)total_blocks), dim3(256), (size_t)K * sizeof(uint32_t), as_stream(s), labels,
                     image_pixels, out_offset, block_prefix, N, out_pixels, K, reinterpret_cast<unsigned long long*>(counts));
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_area_keep(const int64_t* counts, int N, int K, int bg_idx, double area_thd, int32_t* keep, sg_stream s) {
  SG_REQUIRE(counts && keep, "sg_area_keep: null pointer");
  SG_AREA_K("sg_area_keep", K);
  SG_REQUIRE(N > 0, "sg_area_keep: N=%d images", N);
  SG_REQUIRE(bg_idx >= 0 && bg_idx < K, "sg_area_keep: bg_idx=%d outside [0, K=%d)", bg_idx, K);
  SG_REQUIRE(area_thd >= 0.0, "sg_area_keep: area_thd=%g must be a number >= 0", area_thd);
  hipLaunchKernelGGL(area_keep_kernel, dim3((unsigned)N), dim3(256), 0, as_stream(s), counts, K, bg_idx, area_thd, keep);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_area_filter_probs(float* probs, const int64_t* labels_in, const int32_t* keep, int K, int H, int W, float prob_thd,
                                    int bg_idx, int64_t* labels_out, sg_stream s) {
  SG_REQUIRE(probs && labels_in && keep && labels_out, "sg_area_filter_probs: null pointer");
  SG_AREA_K("sg_area_filter_probs", K);
  SG_REQUIRE(H > 0 && W > 0, "sg_area_filter_probs: H=%d W=%d", H, W);
  SG_REQUIRE(bg_idx >= 0 && bg_idx < K, "sg_area_filter_probs: bg_idx=%d outside [0, K=%d)", bg_idx, K);
  const int64_t HW = (int64_t)H * W;
  SG_REQUIRE(cdiv(HW, 256) <= INT32_MAX, "sg_area_filter_probs: image too large for one launch");
  hipLaunchKernelGGL(area_filter_kernel, dim3((unsigned)cdiv(HW, 256)), dim3(256), 0, as_stream(s), probs, labels_in, labels_out, keep, K, HW,
                     prob_thd, bg_idx);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_area_filter_probs_multi(float* probs, const int64_t* labels_in, const int32_t* keep, const int32_t* out_hw,
                                          const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks,
                                          int64_t out_pixels, int K, float prob_thd, int bg_idx, int64_t* labels_out, sg_stream s) {
  SG_REQUIRE(probs && labels_in && keep && out_hw && out_offset && block_prefix && labels_out, "sg_area_filter_probs_multi: null pointer");
  SG_AREA_K("sg_area_filter_probs_multi", K);
  SG_REQUIRE(N > 0, "sg_area_filter_probs_multi: N=%d images", N);
  SG_REQUIRE(bg_idx >= 0 && bg_idx < K, "sg_area_filter_probs_multi: bg_idx=%d outside [0, K=%d)", bg_idx, K);
  SG_REQUIRE(total_blocks > 0 && total_blocks <= INT32_MAX, "sg_area_filter_probs_multi: total_blocks=%lld outside (0, 2^31)",
             (long long)total_blocks);
  SG_REQUIRE(out_pixels > 0, "sg_area_filter_probs_multi: out_pixels=%lld holds no image", (long long)out_pixels);
  hipLaunchKernelGGL(area_filter_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(s), probs, labels_in, labels_out, keep,
                     out_hw, out_offset, block_prefix, N, out_pixels, K, prob_thd, bg_idx);
  SG_LAUNCH_CHECK();
  return SG_OK;
}
