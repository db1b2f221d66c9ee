// Connected-component labelling shared by sieve.hip (sg_sieve, sg_regions) and objmatch.hip (sg_object_match): the launch-sequence
// descriptors, the union-find helpers and the three labelling kernels sieve_local / sieve_merge / sieve_flatten, whose description stands
// at the head of sieve.hip.  After the three, parent[i] is the root of pixel i's region (its smallest raster index) and area[root] its pixel
// count.  Everything lies in an unnamed namespace: each unit that includes this header compiles its own copy of the kernels.
#pragma once
#include "common.h"

namespace sg {
namespace {

constexpr int SV_TW = 64, SV_TH = 16, SV_TILE = SV_TW * SV_TH;      // the LDS tile: 8 KiB of labels + 4 KiB of parents
constexpr int SV_RUN = 8, SV_PIX = 256 * SV_RUN;                    // pixels per workgroup of the per-pixel kernels: 2048
constexpr int SV_GROUP = SG_SIEVE_GROUP;                            // images per launch sequence: their descriptors are launch arguments
constexpr int64_t SV_MAX_PIXELS = ((int64_t)1 << 31) - 1;           // per image (parent is int32); sg_regions: per call (rows are int32)
constexpr int64_t SV_MAX_GRID = (int64_t)1 << 30;                   // workgroups per launch
constexpr int SV_COPY = -1;                                         // sieve_apply's fill for min_region = 1: the input bytes

// The images of one launch sequence, by value in the kernel arguments (2 KiB): nothing is copied to the device for them.
struct SieveImages {
  int n;
  int h[SV_GROUP], w[SV_GROUP];
  long long off[SV_GROUP];                                          // first label of the image in the flat label buffers
  long long wbase[SV_GROUP];                                        // first pixel of the image in parent / area / best
  int tile_prefix[SV_GROUP + 1];                                    // workgroups of sieve_local / sieve_merge before the image
  int blk_prefix[SV_GROUP + 1];                                     // workgroups of the per-pixel kernels before the image
};

// largest n with prefix[n] <= b (block-uniform: scalar loads from the kernel arguments)
__device__ __forceinline__ int sieve_image_of(const int* prefix, int n_images, int b) {
  int lo = 0, hi = n_images;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- union-find ---------------------------------------------------------------------------------------------------------------------
// Invariant: parent[i] <= i, always, for every entry and at every moment.  It holds after initialisation (parent[i] = i), and every
// write keeps it: unite stores min(parent[hi], lo) with lo < hi, flatten stores find(i) <= i.  An entry therefore only ever decreases,
// and every value an entry has ever held is a pixel of the same region (a link is only made between two pixels of equal label that
// are connected).
// find terminates: it moves from i to parent[i] only while parent[i] != i, i.e. to a strictly smaller index, and indices are >= 0.
// This needs nothing but parent[i] <= i for the value that was read, so it also holds for a stale read (an older value of the entry).
// unite terminates: each retry continues with (old, lo) where old < hi is what the atomicMin found in parent[hi] and lo < hi, so the
// larger of the two indices it works on strictly decreases from one round to the next.
// unite is correct with stale reads: a stale find ends at an entry that WAS a root of the same region, maybe no longer is.  The
// atomicMin acts on the true current value and returns it: when it returns hi the entry was a root and now hangs under lo, a smaller
// pixel of the other region -- the two regions are one; when it returns old != hi the entry was no root (any more), parent[hi] now
// holds min(old, lo), and the round that follows re-unites old with lo, which restores the link to old where lo replaced it.
template <bool GLOBAL> __device__ __forceinline__ int uf_load(int* p, int i) {
  if constexpr (GLOBAL) return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // other workgroups write it in this launch
  else return *reinterpret_cast<volatile int*>(p + i);                                                 // LDS: other waves of the workgroup do
}
template <bool GLOBAL> __device__ __forceinline__ int uf_min(int* p, int i, int v) {
  if constexpr (GLOBAL) return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return atomicMin(p + i, v);
}
template <bool GLOBAL> __device__ __forceinline__ int uf_find(int* p, int i) {
  for (int q = uf_load<GLOBAL>(p, i); q < i; q = uf_load<GLOBAL>(p, i)) i = q;      // q < i: strictly down; q >= i is a root (q == i)
  return i;
}
template <bool GLOBAL> __device__ __forceinline__ void uf_unite(int* p, int a, int b) {
  for (;;) {
    a = uf_find<GLOBAL>(p, a);
    b = uf_find<GLOBAL>(p, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = uf_min<GLOBAL>(p, hi, lo);
    if (old >= hi) return;                                            // hi was a root (old == hi) and now hangs under lo
    a = old; b = lo;                                                  // old < hi and lo < hi: the larger index strictly decreases
  }
}

struct SieveTile { int n, H, W, y0, x0; };
__device__ __forceinline__ SieveTile sieve_tile(const SieveImages& im) {
  SieveTile t;
  t.n = sieve_image_of(im.tile_prefix, im.n, (int)blockIdx.x);
  t.H = im.h[t.n]; t.W = im.w[t.n];
  const int tiles_x = (t.W + SV_TW - 1) / SV_TW, k = (int)blockIdx.x - im.tile_prefix[t.n];
  t.y0 = (k / tiles_x) * SV_TH; t.x0 = (k % tiles_x) * SV_TW;
  return t;
}

// One workgroup per tile, a thread per column and four rows.  Every index below stays inside the tile's 1024 LDS entries and, for
// global memory, inside the image (gx < W and gy < H are checked before any access).
__global__ __launch_bounds__(256) void sieve_local_kernel(const int64_t* __restrict__ labels, const SieveImages im, int conn8,
                                                          int32_t* __restrict__ parent, int32_t* __restrict__ area,
                                                          unsigned long long* __restrict__ best) {
  __shared__ int64_t s_lab[SV_TILE];
  __shared__ int s_par[SV_TILE];
  const SieveTile t = sieve_tile(im);
  const int64_t* lab = labels + im.off[t.n];
  const int64_t wb = im.wbase[t.n];
  const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 4, gx = t.x0 + lx;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + k, gy = t.y0 + ly, l = ly * SV_TW + lx;
    s_lab[l] = (gx < t.W && gy < t.H) ? lab[(int64_t)gy * t.W + gx] : 0;
  }
  __syncthreads();
  // A wave owns whole rows (lane = column): the horizontal runs of a row need no union -- every pixel starts under the first pixel of
  // its run, found by a ballot of the run heads.
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + k, gy = t.y0 + ly, l = ly * SV_TW + lx;
    const bool in = gx < t.W && gy < t.H;
    const bool head = !in || lx == 0 || s_lab[l - 1] != s_lab[l];
    const unsigned long long heads = __ballot(head) & ((2ull << lx) - 1ull);     // lane 63: 2 << 63 wraps to 0, the mask to all ones
    s_par[l] = ly * SV_TW + (63 - __clzll((long long)heads));                      // bit 0 is always set
  }
  __syncthreads();
  // The links between rows.  A pair is skipped where pairs that are not skipped already imply it:
  //   up        when the left pixel and the upper-left pixel hold the label too (the left pixel's own upward link, and the two runs)
  //   up-left   when the upper or the left pixel holds the label (that pixel's link, and a run)
  //   up-right  when the upper pixel holds the label (its link, and the upper run)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + k, gy = t.y0 + ly, l = ly * SV_TW + lx;
    if (gx >= t.W || gy >= t.H || ly == 0) continue;                  // a pixel of the image: its left and upper neighbours in the tile are too
    const int64_t v = s_lab[l];
    const bool up = s_lab[l - SV_TW] == v, left = lx > 0 && s_lab[l - 1] == v, upleft = lx > 0 && s_lab[l - SV_TW - 1] == v;
    if (up && !(left && upleft)) uf_unite<false>(s_par, l, l - SV_TW);
    if (conn8) {
      if (upleft && !up && !left) uf_unite<false>(s_par, l, l - SV_TW - 1);
      if (!up && lx < SV_TW - 1 && gx + 1 < t.W && s_lab[l - SV_TW + 1] == v) uf_unite<false>(s_par, l, l - SV_TW + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + k, gy = t.y0 + ly, l = ly * SV_TW + lx;
    if (gx >= t.W || gy >= t.H) continue;
    const int r = uf_find<false>(s_par, l);                          // the tile's raster order is the image's: the smallest local index is the smallest raster index
    const int64_t i = wb + (int64_t)gy * t.W + gx;
    parent[i] = (int32_t)((int64_t)(t.y0 + (r >> 6)) * t.W + t.x0 + (r & 63));
    area[i] = 0;
    if (best) best[i] = 0ull;
  }
}

// Threads 0..63: the tile's top row; 64..79: its left column; 80..95: its right column (connectivity 8 only).  Each looks at its
// pixel's four BACKWARD neighbours (left, up, up-left, up-right: every pair of the image is seen once, from its later pixel) and
// unites the pair where it straddles a tile border and the labels agree.
// parent entries that other workgroups may be writing in this launch are read with agent-scope atomic loads (a plain load may be
// served from this CU's L1 or this XCD's L2 and be stale) or through the atomicMin's return value; the algorithm does not depend on
// the reads being fresh (see unite above).  labels is not written here.
__global__ __launch_bounds__(128) void sieve_merge_kernel(const int64_t* __restrict__ labels, const SieveImages im, int conn8, int32_t* parent) {
  const SieveTile t = sieve_tile(im);
  const int role = threadIdx.x;
  int lx, ly;
  if (role < 64) { lx = role; ly = 0; }
  else if (role < 80) { lx = 0; ly = role - 64; }
  else if (role < 96 && conn8) { lx = SV_TW - 1; ly = role - 80; }
  else return;
  if (role >= 64 && ly == 0) return;                                   // the corner pixels belong to the top row
  const int gx = t.x0 + lx, gy = t.y0 + ly, W = t.W;
  if (gx >= W || gy >= t.H) return;
  const int64_t* lab = labels + im.off[t.n];
  int* P = parent + im.wbase[t.n];
  const int i = gy * W + gx;                                           // < H * W < 2^31
  const int64_t v = lab[i];
  if (lx == 0 && gx > 0 && lab[i - 1] == v) {                          // the left pair crosses a vertical border
    // skipped when the pair above it (same tile: ly > 0) holds the same labels under the same two entries: that pair's thread unites them
    const bool same = ly > 0 && lab[i - W] == v && lab[i - W - 1] == v && uf_load<true>(P, i - W) == uf_load<true>(P, i) &&
                      uf_load<true>(P, i - W - 1) == uf_load<true>(P, i - 1);
    if (!same) uf_unite<true>(P, i, i - 1);
  }
  if (ly == 0 && gy > 0 && lab[i - W] == v) {                          // the upper pair crosses a horizontal border
    const bool same = lx > 0 && lab[i - 1] == v && lab[i - W - 1] == v && uf_load<true>(P, i - 1) == uf_load<true>(P, i) &&
                      uf_load<true>(P, i - W - 1) == uf_load<true>(P, i - W);
    if (!same) uf_unite<true>(P, i, i - W);
  }
  if (conn8 && gy > 0) {
    // a diagonal pair is implied, as in sieve_local, where the upper pixel (or for up-left the left pixel) holds the label too: that
    // pixel's straight pairs are united there or by the thread of this launch that owns them, and unions commute
    const bool up = lab[i - W] == v;
    if (gx > 0 && (lx == 0 || ly == 0) && !up && lab[i - 1] != v && lab[i - W - 1] == v) uf_unite<true>(P, i, i - W - 1);
    if (gx + 1 < W && (lx == SV_TW - 1 || ly == 0) && !up && lab[i - W + 1] == v) uf_unite<true>(P, i, i - W + 1);
  }
}

struct SievePixel { int n; int64_t np; int64_t base; };            // the workgroup's image, its pixel count, the workgroup's first pixel
__device__ __forceinline__ SievePixel sieve_pixel(const SieveImages& im) {
  SievePixel p;
  p.n = sieve_image_of(im.blk_prefix, im.n, (int)blockIdx.x);
  p.np = (int64_t)im.h[p.n] * im.w[p.n];
  p.base = ((int64_t)blockIdx.x - im.blk_prefix[p.n]) * SV_PIX;
  return p;
}

// parent[i] = find(i); area[root] += the region's pixels.  Other threads of this launch store roots into entries that a find here
// walks through: either value of such an entry is a pixel of the region above it (the invariant), so plain loads do.
// The adds are merged before they reach global memory, as class_area_step of area.hip does: the 64 consecutive pixels of a wave step by
// leader match (a ballot of the lanes that hold the first unserved lane's root), the waves' and steps' sums through a table of 64
// (root, count) pairs in LDS that one wave merges the same way.  A flat map sends ONE add per workgroup of 2048 pixels to its root.
// What does not fit (a wave step that meets many roots, a full table) adds directly: those are distinct roots.
__global__ __launch_bounds__(256) void sieve_flatten_kernel(const SieveImages im, int32_t* parent, int32_t* area) {
  __shared__ int s_root[64], s_cnt[64], s_n;
  const SievePixel p = sieve_pixel(im);
  int* P = parent + im.wbase[p.n];
  int* A = area + im.wbase[p.n];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) s_n = 0;
  __syncthreads();
  int r[SV_RUN], h[SV_RUN];
  // the first two steps of the eight finds as independent loads (a step at a root stays there: parent[root] = root), then the rest
#pragma unroll
  for (int j = 0; j < SV_RUN; ++j) r[j] = p.base + j * 256 + tid < p.np ? P[p.base + j * 256 + tid] : -1;
#pragma unroll
  for (int j = 0; j < SV_RUN; ++j) h[j] = r[j] >= 0 ? P[r[j]] : -1;
#pragma unroll
  for (int j = 0; j < SV_RUN; ++j) {
    bool act = r[j] >= 0;
    if (act) {
      int i = h[j];
      for (int q = P[i]; q < i; q = P[i]) i = q;                       // strictly down (see find)
      r[j] = i;
      P[p.base + j * 256 + tid] = i;
    }
    unsigned long long rem = __ballot(act);
    int rounds = 0;
    while (rem != 0ull) {                                              // wave-uniform
      const int src = __ffsll((long long)rem) - 1;
      const int lr = __builtin_amdgcn_readlane(r[j], src);
      const bool m = act && r[j] == lr;
      const unsigned long long mm = __ballot(m);
      if (lane == src) {
        const int slot = atomicAdd(&s_n, 1);
        if (slot < 64) { s_root[slot] = lr; s_cnt[slot] = __popcll(mm); }
        else atomicAdd(&A[lr], __popcll(mm));
      }
      act = act && !m;
      rem &= ~mm;
      if (++rounds >= 3 && __popcll(mm) < 4) break;
    }
    if (act) atomicAdd(&A[r[j]], 1);
  }
  __syncthreads();
  if (tid < 64) {                                                      // one wave merges the table: at most 64 rounds
    const int n = s_n < 64 ? s_n : 64;
    bool act = tid < n;
    const int rr = act ? s_root[tid] : -1, cc = act ? s_cnt[tid] : 0;
    unsigned long long rem = __ballot(act);
    while (rem != 0ull) {
      const int src = __ffsll((long long)rem) - 1;
      const int lr = __builtin_amdgcn_readlane(rr, src);
      const bool m = act && rr == lr;
      const unsigned long long mm = __ballot(m);
      int total = 0;                                                   // the sum of cc (<= 64: 7 bits) over the matching lanes
      for (int b = 0; b < 7; ++b) total += __popcll(__ballot(m && ((cc >> b) & 1))) << b;
      if (lane == src) atomicAdd(&A[lr], total);
      act = act && !m;
      rem &= ~mm;
    }
  }
}

// The next launch sequence: the images n0 .. n0 + k - 1 (k <= SG_SIEVE_GROUP; fewer only beyond 2^30 workgroups), their descriptors in
// im, their workgroup counts in tiles / blks; wbase moves past their pixels.  Returns k.
static int sieve_group(const int32_t* image_hw, const int64_t* out_offset, int N, int n0, int64_t* wbase, SieveImages* im, int64_t* tiles_out,
                       int64_t* blks_out) {
  memset(im, 0, sizeof(*im));
  int64_t tiles = 0, blks = 0;
  int k = 0;
  for (; k < SV_GROUP && n0 + k < N; ++k) {
    const int64_t h = image_hw[2 * (n0 + k)], w = image_hw[2 * (n0 + k) + 1];
    const int64_t t = cdiv(h, SV_TH) * cdiv(w, SV_TW), b = cdiv(h * w, SV_PIX);
    if (k > 0 && (tiles + t > SV_MAX_GRID || blks + b > SV_MAX_GRID)) break;
    im->h[k] = (int)h; im->w[k] = (int)w;
    im->off[k] = out_offset[n0 + k];
    im->wbase[k] = *wbase;
    im->tile_prefix[k] = (int)tiles; im->blk_prefix[k] = (int)blks;
    tiles += t; blks += b; *wbase += h * w;
  }
  im->n = k;
  for (int j = k; j <= SV_GROUP; ++j) { im->tile_prefix[j] = (int)tiles; im->blk_prefix[j] = (int)blks; }
  *tiles_out = tiles; *blks_out = blks;
  return k;
}

// The three labelling launches over the images of one launch sequence (im, tiles and blks as sieve_group left them), in stream order.
// sieve_local also zeroes best[] of every pixel where best is not null.
static int sieve_label(const int64_t* labels, const SieveImages& im, int64_t tiles, int64_t blks, int conn8, int32_t* parent, int32_t* area,
                       unsigned long long* best, hipStream_t s) {
  const dim3 gt((unsigned)tiles), gp((unsigned)blks);
  hipLaunchKernelGGL(sieve_local_kernel, gt, dim3(256), 0, s, labels, im, conn8, parent, area, best);
  SG_LAUNCH_CHECK();
  hipLaunchKernelGGL(sieve_merge_kernel, gt, dim3(128), 0, s, labels, im, conn8, parent);
  SG_LAUNCH_CHECK();
  hipLaunchKernelGGL(sieve_flatten_kernel, gp, dim3(256), 0, s, im, parent, area);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

}  // namespace
}  // namespace sg
