// min_region: sieve small connected regions out of a label map (the definition is the comment block of sg_sieve in
// include/segearth_hip.h).  Connected-component labelling by union-find, in five kernels whose only ordering is the stream's:
//   sieve_local    : one workgroup per 64 x 16 pixel tile; union-find over the tile in LDS (row runs by ballot, then the links between
//                    rows); parent[i] = the smallest raster index of the pixel's component INSIDE the tile; area and best zeroed.
//                    Reads 8 B, writes 8 (16) B per pixel.
//   sieve_merge    : one thread per pixel on a tile border; union of the pixel pairs that straddle the border (diagonal ones with
//                    connectivity 8) by atomicMin on the larger root.  A pair whose two pixels hang under the same two entries as the pair
//                    before it along the border is skipped, so a flat border costs one union, not 64.
//   sieve_flatten  : parent[i] = find(i), and area[root] += the pixel counts, merged in registers, in the wave (leader match, as
//                    class_area_step of area.hip) and in an LDS table before they reach global memory: a flat map sends one add per
//                    workgroup of 2048 pixels to its root, not one per pixel.
//   sieve_choose   : "neighbour" only: a pixel of a small region that touches a kept region sends (area << 32 | ~root) of the best kept
//                    region among its neighbours to best[its root] with one 64-bit atomicMax -- at most one per pixel, and none
//                    unless the key beats what best[] already shows.
//   sieve_apply    : the new label per pixel.
// No workgroup ever waits for another: there is no flag, spin loop, cooperative launch or grid barrier in this file, and every loop
// runs down a strictly decreasing chain (the argument stands beside find and unite in sieve_label.h,
// which holds the three labelling kernels, shared with objmatch.hip).  Integer atomics only (min, add, max), all
// commutative and exact, so the result is byte-identical whatever the launch shape or the arrival order.
// parent holds raster indices y * W + x inside the pixel's own image (below 2^31); the images of a call share nothing but the launch.
#include "sieve_label.h"

namespace sg {

// "neighbour": the kept region next to a small one.  parent holds roots now and area is complete (kernel boundaries).
__device__ __forceinline__ void sieve_choose_pixel(const int32_t* __restrict__ P, const int32_t* __restrict__ A, unsigned long long* B, int H, int W,
                                                   int conn8, int64_t min_region, int i) {
  const int y = i / W, x = i - y * W;
  const int r = P[i];
  if ((int64_t)A[r] >= min_region) return;
  unsigned long long key = 0ull;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k >= 4 && !conn8) break;
    const int dx = k == 0 ? -1 : k == 1 ? 1 : k < 4 ? 0 : (k & 1 ? 1 : -1);          // left, right, up, down, then the four corners
    const int dy = k < 2 ? 0 : k == 2 ? -1 : k == 3 ? 1 : (k < 6 ? -1 : 1);
    const int xx = x + dx, yy = y + dy;
    if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
    const int q = P[yy * W + xx];
    if (q == r) continue;                                              // another root: another region, hence another label
    const int a = A[q];
    if ((int64_t)a < min_region) continue;                             // a small neighbour never wins
    const unsigned long long cand = ((unsigned long long)(uint32_t)a << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)q);
    key = cand > key ? cand : key;                                     // the larger area, then the smaller root
  }
  // the plain read may be older than what other workgroups have sent: then the atomic is issued needlessly, never wrongly
  if (key != 0ull && key > B[r]) atomicMax(&B[r], key);
}

__global__ __launch_bounds__(256) void sieve_choose_kernel(const SieveImages im, int conn8, int64_t min_region, const int32_t* __restrict__ parent,
                                                           const int32_t* __restrict__ area, unsigned long long* best) {
  const SievePixel p = sieve_pixel(im);
  const int64_t wb = im.wbase[p.n];
  for (int k = 0; k < SV_RUN; ++k) {
    const int64_t i = p.base + k * 256 + threadIdx.x;
    if (i >= p.np) return;                                             // and so is every later pixel of this thread
    sieve_choose_pixel(parent + wb, area + wb, best + wb, im.h[p.n], im.w[p.n], conn8, min_region, (int)i);
  }
}

// The new label of every pixel.  In place (labels_out == labels) this is safe because the only labels read from another pixel are
// those of winner roots, which lie in KEPT regions, and a pixel of a kept region is never rewritten: whichever of the two buffers is
// read there holds the same value at every moment.  A pixel reads its own label before it writes it.
__global__ __launch_bounds__(256) void sieve_apply_kernel(const int64_t* labels, int64_t* labels_out, const SieveImages im, int fill, int64_t min_region,
                                                          int64_t bg_idx, const int32_t* __restrict__ parent, const int32_t* __restrict__ area,
                                                          const unsigned long long* __restrict__ best) {
  const SievePixel p = sieve_pixel(im);
  const int64_t* lab = labels + im.off[p.n];
  int64_t* out = labels_out + im.off[p.n];
  const int64_t wb = im.wbase[p.n];
  for (int k = 0; k < SV_RUN; ++k) {
    const int64_t i = p.base + k * 256 + threadIdx.x;
    if (i >= p.np) return;
    const int64_t v = lab[i];
    int64_t nv = v;
    if (fill != SV_COPY) {
      const int r = parent[wb + i];
      if ((int64_t)area[wb + r] < min_region) {
        if (fill == SG_SIEVE_FILL_BG) {
          nv = bg_idx;                                                 // a small background region keeps its label this way too
        } else {
          const unsigned long long b = best[wb + r];
          nv = b != 0ull ? lab[0xFFFFFFFFu - (uint32_t)b] : bg_idx;
        }
      }
    }
    if (nv != v || out != lab) out[i] = nv;
  }
}

// ---- the region table (sg_regions; the definition is its comment block in include/segearth_hip.h) -----------------------------------------
// After sieve_local / sieve_merge / sieve_flatten (parent holds roots, area[root] the region's pixel count) four more kernels, under the
// same rule as above (stream order only, integer atomics only):
//   regions_count   : blk[b] = the listed roots among the 2048 pixels of per-pixel workgroup b.
//   regions_scan    : ONE workgroup turns blk into exclusive row offsets, SG_REGIONS_SCAN_BLOCKS entries per pass with the carry in a
//                     register, starting from the rows of the launch sequences before it (counts[N], device memory), and writes the
//                     per-image counts.  The workgroups are ordered by (image, first pixel), so the offsets give the (image, root) order.
//   regions_scatter : a listed root's row = blk[b] + its rank in the workgroup (ballot / popcount, per-wave counts in LDS); it writes the
//                     row's IMAGE, ROOT, LABEL, AREA, Y0 (the root's own y: the root is the region's first pixel in raster order) and the
//                     neutral values of what regions_reduce fills, and leaves the row index in area[root] (-1: not listed).  A region
//                     of ONE pixel gets its whole row here and -(row + 2) in area[root]: regions_reduce adds nothing for it.
//   regions_reduce  : one workgroup per tile of 64 x 128 pixels; every pixel of a listed region adds its x / y to the row's box, sums and
//                     score, merged before they reach global memory: the lanes of a wave that hold the same row by leader match (as
//                     sieve_flatten, by scalar arithmetic on the ballot), four rows per wave in registers, the waves in a direct-mapped
//                     LDS table of 64 rows.  A flat map sends five or six atomics per workgroup of 8192 pixels to its one row.
constexpr int RG_SCAN = SG_REGIONS_SCAN_BLOCKS;                      // entries per pass of the scan's single workgroup
constexpr int RG_SLOTS = 64;                                         // the merge table of regions_reduce
constexpr int RG_WAVE = 4;                                           // regions_reduce: rows a wave merges in registers before the table
constexpr int RG_TH = 128;                                           // regions_reduce: a workgroup's tile is 64 x RG_TH pixels, in halves of 64 rows
static_assert(SV_PIX == SG_REGIONS_BLOCK_PIXELS, "the header states the pixels per workgroup of the per-pixel kernels");

struct RegionRule { long long min_area, skip_label; int use_skip; };

// pixel i of the image is a listed root.  i < np is checked before any access; a root's area entry is complete (kernel boundary).
__device__ __forceinline__ bool region_listed(const int32_t* P, const int32_t* A, const int64_t* lab, int64_t i, int64_t np, const RegionRule& ru) {
  if (i >= np || P[i] != (int)i || (long long)A[i] < ru.min_area) return false;
  return !ru.use_skip || lab[i] != ru.skip_label;
}

__global__ __launch_bounds__(256) void regions_count_kernel(const int64_t* __restrict__ labels, const SieveImages im, const RegionRule ru,
                                                            const int32_t* __restrict__ parent, const int32_t* __restrict__ area,
                                                            int32_t* __restrict__ blk) {
  __shared__ int s_w[4];
  const SievePixel p = sieve_pixel(im);
  const int64_t* lab = labels + im.off[p.n];
  const int32_t* P = parent + im.wbase[p.n];
  const int32_t* A = area + im.wbase[p.n];
  int c = 0;                                                           // wave-uniform
#pragma unroll
  for (int j = 0; j < SV_RUN; ++j) c += __popcll(__ballot(region_listed(P, A, lab, p.base + j * 256 + threadIdx.x, p.np, ru)));
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// One workgroup.  blk[0 .. nblk) in: the counts; out: the row of each workgroup's first listed root; blk[nblk] = the rows after this
// launch sequence.  counts[image0 + k] for the sequence's images, counts[N] = the running total (read here unless this is the first
// sequence of the call; written by thread 0 after every thread has read it).  A count is at most 2048 and the total below 2^31.
__global__ __launch_bounds__(RG_SCAN) void regions_scan_kernel(int32_t* blk, int nblk, const SieveImages im, int image0, int first, int N,
                                                               int64_t* counts) {
  __shared__ int s_w[RG_SCAN / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = first ? 0 : (int)counts[N];
  for (int p0 = 0; p0 < nblk; p0 += RG_SCAN) {                        // block-uniform
    const int v = p0 + tid < nblk ? blk[p0 + tid] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RG_SCAN / 64; ++w) {
      const int c = s_w[w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (p0 + tid < nblk) blk[p0 + tid] = carry + before + inc - v;
    carry += all;
    __syncthreads();                                                   // s_w is rewritten by the next pass
  }
  if (tid == 0) blk[nblk] = carry;
  __syncthreads();                                                     // the offsets written above are read below by other threads of this workgroup
  if (tid < im.n) counts[image0 + tid] = (int64_t)(blk[im.blk_prefix[tid + 1]] - blk[im.blk_prefix[tid]]);
  if (tid == 0) counts[N] = carry;
}

// q(c): round-to-nearest-even of clamp(c, 0, 1) * 2^24; a NaN counts 0.  The product is exact in f32 (a power of two).
__device__ __forceinline__ unsigned long long region_q(float c) {
  if (!(c > 0.f)) return 0ull;                                         // NaN, zero and negatives
  return (unsigned long long)__builtin_rintf((c < 1.f ? c : 1.f) * 16777216.f);
}

__global__ __launch_bounds__(256) void regions_scatter_kernel(const int64_t* __restrict__ labels, const float* __restrict__ conf, const SieveImages im,
                                                              const RegionRule ru, int image0, const int32_t* __restrict__ parent, int32_t* area,
                                                              const int32_t* __restrict__ blk, int64_t max_regions, int64_t* __restrict__ table) {
  __shared__ int s_c[SV_RUN * 4];
  const SievePixel p = sieve_pixel(im);
  const int64_t* lab = labels + im.off[p.n];
  const int32_t* P = parent + im.wbase[p.n];
  int32_t* A = area + im.wbase[p.n];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long m[SV_RUN];
#pragma unroll
  for (int j = 0; j < SV_RUN; ++j) {
    m[j] = __ballot(region_listed(P, A, lab, p.base + j * 256 + tid, p.np, ru));
    if (lane == 0) s_c[j * 4 + wave] = __popcll(m[j]);
  }
  __syncthreads();
  const int first_row = blk[blockIdx.x];
#pragma unroll
  for (int j = 0; j < SV_RUN; ++j) {
    const int64_t i = p.base + j * 256 + tid;
    if (i >= p.np || P[i] != (int)i) continue;                         // roots only: area[] means something only there
    if (!((m[j] >> lane) & 1ull)) { A[i] = -1; continue; }
    int before = 0;                                                    // the listed roots of the workgroup before this wave's step j, in pixel order
    for (int q = 0; q < j * 4 + wave; ++q) before += s_c[q];
    const int row = first_row + before + __popcll(m[j] & ((1ull << lane) - 1ull));
    const int a = A[i];
    const bool lone = a == 1;                                          // a region of one pixel: its row is complete here, regions_reduce adds nothing
    if ((int64_t)row < max_regions) {
      int64_t* t = table + (int64_t)row * SG_REGION_FIELDS;
      const int W = im.w[p.n], y = (int)i / W, x = (int)i - y * W;
      t[SG_REGION_IMAGE] = image0 + p.n;
      t[SG_REGION_ROOT] = i;
      t[SG_REGION_LABEL] = lab[i];
      t[SG_REGION_AREA] = a;
      t[SG_REGION_Y0] = y;
      t[SG_REGION_X0] = lone ? x : W;
      t[SG_REGION_Y1] = lone ? y + 1 : 0;
      t[SG_REGION_X1] = lone ? x + 1 : 0;
      t[SG_REGION_SUM_Y] = lone ? y : 0;
      t[SG_REGION_SUM_X] = lone ? x : 0;
      t[SG_REGION_SCORE_Q] = lone && conf ? (int64_t)region_q(conf[im.off[p.n] + i]) : 0;
      t[SG_REGION_FIELDS - 1] = 0;
    }
    A[i] = lone ? -row - 2 : row;                                      // row <= 2^31 - 2: no step of -row - 2 leaves int
  }
}

struct RegionAcc { int xmin, xend, yend; unsigned long long sy, sx, sq; };          // xend / yend: one past
__device__ __forceinline__ void region_add(RegionAcc& a, const RegionAcc& b) {
  a.xmin = b.xmin < a.xmin ? b.xmin : a.xmin; a.xend = b.xend > a.xend ? b.xend : a.xend; a.yend = b.yend > a.yend ? b.yend : a.yend;
  a.sy += b.sy; a.sx += b.sx; a.sq += b.sq;
}

// row < max_regions is checked by the caller
__device__ __forceinline__ void region_send(int64_t* table, int row, const RegionAcc& a, bool scored) {
  long long* t = reinterpret_cast<long long*>(table + (int64_t)row * SG_REGION_FIELDS);
  __hip_atomic_fetch_min(t + SG_REGION_X0, (long long)a.xmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_max(t + SG_REGION_X1, (long long)a.xend, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_max(t + SG_REGION_Y1, (long long)a.yend, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(reinterpret_cast<unsigned long long*>(t + SG_REGION_SUM_Y), a.sy);
  atomicAdd(reinterpret_cast<unsigned long long*>(t + SG_REGION_SUM_X), a.sx);
  if (scored && a.sq != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(t + SG_REGION_SCORE_Q), a.sq);
}

// the sum of v over the 64 lanes, in every lane, on DPP and v_readlane (no LDS-queue round trips; common.h 'sum16_dpp'); all lanes take part
template <int CTRL> __device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += dpp_i32<0xB1>(v); v += dpp_i32<0x4E>(v); v += dpp_i32<0x141>(v); v += dpp_i32<0x140>(v);
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) + (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}
// the sum of the positions of the set bits of mm
__device__ __forceinline__ int lane_sum(unsigned long long mm) {
  return __popcll(mm & 0xAAAAAAAAAAAAAAAAull) + (__popcll(mm & 0xCCCCCCCCCCCCCCCCull) << 1) + (__popcll(mm & 0xF0F0F0F0F0F0F0F0ull) << 2) +
         (__popcll(mm & 0xFF00FF00FF00FF00ull) << 3) + (__popcll(mm & 0xFFFF0000FFFF0000ull) << 4) + (__popcll(mm & 0xFFFFFFFF00000000ull) << 5);
}

// The workgroup's merge table: RG_SLOTS rows, direct-mapped by row & 63 (the rows that meet in a workgroup are neighbours in the table's
// order, so they seldom share a slot).  The first row to come owns the slot; a row that finds its slot taken by another sends directly.
struct RegionSlots {
  int row[RG_SLOTS], xmin[RG_SLOTS], xend[RG_SLOTS], yend[RG_SLOTS];
  unsigned long long sy[RG_SLOTS], sx[RG_SLOTS], sq[RG_SLOTS];
};
__device__ __forceinline__ void region_merge(RegionSlots& t, int64_t* table, int row, const RegionAcc& a, bool scored) {
  const int k = row & (RG_SLOTS - 1);
  const int old = atomicCAS(&t.row[k], -1, row);
  if (old == -1 || old == row) {
    atomicMin(&t.xmin[k], a.xmin); atomicMax(&t.xend[k], a.xend); atomicMax(&t.yend[k], a.yend);
    atomicAdd(&t.sy[k], a.sy); atomicAdd(&t.sx[k], a.sx);
    if (scored) atomicAdd(&t.sq[k], a.sq);
  } else {
    region_send(table, row, a, scored);
  }
}

// regions_reduce runs on tiles of 64 x RG_TH pixels, not on the linear 2048-pixel workgroups of the other per-pixel kernels: a compact
// region then meets few workgroups (a 37 x 37 block one to four, not 37), and each sends its merged share once; and a flat map has 1152
// workgroups, not 4608, that all send to one row (atomics on one address pass one at a time).
struct RegionTiles { int prefix[SV_GROUP + 1]; };                     // workgroups of regions_reduce before the image

// One workgroup per tile; a wave owns whole rows of it (lane = column; wave w the rows w, w + 4, ...), so the 64 pixels of a wave step lie
// in one image row and the merge of the lanes that hold a table row needs no data from other lanes: the ballot of the matching lanes
// gives the count, the first and last x and the sum of the x (lane_sum), y is the step's; only q(conf) is summed across lanes, one
// 32-bit value (64 * 2^24 fits) on DPP.  gx < W and gy < H are checked before any access.
__global__ __launch_bounds__(256) void regions_reduce_kernel(const float* __restrict__ conf, const SieveImages im, const RegionTiles rt,
                                                             const int32_t* __restrict__ parent, const int32_t* __restrict__ rows,
                                                             int64_t max_regions, int64_t* table, int32_t* __restrict__ region_of) {
  __shared__ RegionSlots s_t;
  const int n = sieve_image_of(rt.prefix, im.n, (int)blockIdx.x);
  const int H = im.h[n], W = im.w[n];
  const int tiles_x = (W + SV_TW - 1) / SV_TW, k = (int)blockIdx.x - rt.prefix[n];
  const int y00 = (k / tiles_x) * RG_TH, x0 = (k % tiles_x) * SV_TW;
  const int32_t* P = parent + im.wbase[n];
  const int32_t* R = rows + im.wbase[n];
  const int64_t off = im.off[n];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gx = x0 + lane;
  const bool scored = conf != nullptr;
  if (tid < RG_SLOTS) {
    s_t.row[tid] = -1; s_t.xmin[tid] = 0x7fffffff; s_t.xend[tid] = 0; s_t.yend[tid] = 0;
    s_t.sy[tid] = 0ull; s_t.sx[tid] = 0ull; s_t.sq[tid] = 0ull;
  }
  __syncthreads();
  int crow[RG_WAVE], victim = 0;                                       // the wave's own merge: rows and their sums, wave-uniform
  RegionAcc cacc[RG_WAVE];
#pragma unroll
  for (int e = 0; e < RG_WAVE; ++e) { crow[e] = -1; cacc[e] = RegionAcc{0, 0, 0, 0ull, 0ull, 0ull}; }
  for (int half = 0; half < RG_TH / 64; ++half) {
    const int y0 = y00 + half * 64 + wave;                             // this wave's rows of the half: y0, y0 + 4, ... (wave-uniform)
    if (y0 >= H) break;
    // the loads of the sixteen rows first, independent of each other: the root, then the root's entry, then the confidence
    int v[16], q[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) v[s] = gx < W && y0 + 4 * s < H ? P[(int64_t)(y0 + 4 * s) * W + gx] : -1;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (v[s] < 0) continue;                                          // outside the image
      v[s] = R[v[s]];                                                  // the root's entry: its row; -1: not listed; <= -2: a one-pixel region, complete
      if (region_of) region_of[off + (int64_t)(y0 + 4 * s) * W + gx] = v[s] >= -1 ? v[s] : -(v[s] + 2);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s)
      q[s] = scored && v[s] >= 0 && (int64_t)v[s] < max_regions ? (int)region_q(conf[off + (int64_t)(y0 + 4 * s) * W + gx]) : 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int gy = y0 + 4 * s, row = v[s];
      bool act = row >= 0 && (int64_t)row < max_regions;
      unsigned long long rem = __ballot(act);
      int rounds = 0;
      while (rem != 0ull) {                                            // wave-uniform
        const int src = __ffsll((long long)rem) - 1;
        const int lr = __builtin_amdgcn_readlane(row, src);
        const bool m = act && row == lr;
        const unsigned long long mm = __ballot(m);
        const int cnt = __popcll(mm);
        RegionAcc w;
        w.xmin = x0 + src; w.xend = x0 + 64 - __clzll((long long)mm); w.yend = gy + 1;
        w.sy = (unsigned long long)cnt * (unsigned long long)gy;
        w.sx = (unsigned long long)cnt * (unsigned long long)x0 + (unsigned long long)lane_sum(mm);
        w.sq = scored ? (unsigned long long)wave_sum_i32(m ? q[s] : 0) : 0ull;
        // w and lr are wave-uniform: the wave keeps RG_WAVE rows in registers and merges there; a row that is not among them takes the
        // place of the oldest, which goes to the workgroup's table
        bool hit = false;
#pragma unroll
        for (int e = 0; e < RG_WAVE; ++e) {
          if (!hit && crow[e] == lr) { region_add(cacc[e], w); hit = true; }
        }
        if (!hit) {
#pragma unroll
          for (int e = 0; e < RG_WAVE; ++e) {
            if (victim != e) continue;
            if (crow[e] >= 0 && lane == 0) region_merge(s_t, table, crow[e], cacc[e], scored);
            crow[e] = lr; cacc[e] = w;
          }
          victim = (victim + 1) % RG_WAVE;
        }
        act = act && !m;
        rem &= ~mm;
        if (++rounds >= 3 && cnt < 4) break;
      }
      if (act) {                                                       // many small regions in one row of the tile: distinct rows
        const RegionAcc a = {gx, gx + 1, gy + 1, (unsigned long long)gy, (unsigned long long)gx, (unsigned long long)q[s]};
        region_send(table, row, a, scored);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < RG_WAVE; ++e) {
    if (crow[e] >= 0 && lane == 0) region_merge(s_t, table, crow[e], cacc[e], scored);
  }
  __syncthreads();
  if (tid < RG_SLOTS && s_t.row[tid] >= 0) {
    const RegionAcc a = {s_t.xmin[tid], s_t.xend[tid], s_t.yend[tid], s_t.sy[tid], s_t.sx[tid], s_t.sq[tid]};
    region_send(table, s_t.row[tid], a, scored);
  }
}

}  // namespace sg

using namespace sg;

extern "C" size_t sg_sieve_workspace_bytes(int64_t n_pixels_total, int fill) {
  if (n_pixels_total < 0 || (fill != SG_SIEVE_FILL_BG && fill != SG_SIEVE_FILL_NEIGHBOUR)) return 0;
  return (size_t)n_pixels_total * (fill == SG_SIEVE_FILL_NEIGHBOUR ? 16 : 8);
}

extern "C" int sg_sieve(const int64_t* labels, int64_t* labels_out, const int32_t* image_hw, const int64_t* out_offset, int N, int64_t min_region,
                        int connectivity, int fill, int64_t bg_idx, void* workspace, size_t workspace_bytes, sg_stream stream) {
  SG_REQUIRE(labels && labels_out && image_hw && out_offset && workspace, "sg_sieve: null pointer");
  SG_REQUIRE(min_region >= 1, "sg_sieve: min_region=%lld must be >= 1 (a region is small when its area is below it)", (long long)min_region);
  SG_REQUIRE(connectivity == 4 || connectivity == 8, "sg_sieve: connectivity=%d is neither 4 nor 8", connectivity);
  SG_REQUIRE(fill == SG_SIEVE_FILL_BG || fill == SG_SIEVE_FILL_NEIGHBOUR, "sg_sieve: unknown fill %d (SG_SIEVE_FILL_BG or SG_SIEVE_FILL_NEIGHBOUR)", fill);
  SG_REQUIRE(N >= 1, "sg_sieve: N=%d images", N);
  int64_t total = 0;
  for (int n = 0; n < N; ++n) {
    const int64_t h = image_hw[2 * n], w = image_hw[2 * n + 1];
    SG_REQUIRE(h > 0 && w > 0, "sg_sieve: image %d has non-positive size %lld x %lld", n, (long long)h, (long long)w);
    SG_REQUIRE(h * w <= SV_MAX_PIXELS, "sg_sieve: image %d of %lld x %lld has 2^31 or more pixels (region roots are 32-bit raster indices)", n,
               (long long)h, (long long)w);
    SG_REQUIRE(out_offset[n] >= 0, "sg_sieve: out_offset[%d]=%lld is negative", n, (long long)out_offset[n]);
    total += h * w;
  }
  SG_REQUIRE((((uintptr_t)labels) & 7) == 0 && (((uintptr_t)labels_out) & 7) == 0 && (((uintptr_t)workspace) & 7) == 0,
             "sg_sieve: the label buffers and the workspace must be 8-byte aligned");
  const size_t need = sg_sieve_workspace_bytes(total, fill);
  SG_REQUIRE(workspace_bytes >= need, "sg_sieve: workspace too small: %zu bytes given, %zu needed for %lld pixels", workspace_bytes, need,
             (long long)total);
  // workspace: best u64 [total] ("neighbour" only), parent int32 [total], area int32 [total]
  unsigned long long* best = fill == SG_SIEVE_FILL_NEIGHBOUR ? reinterpret_cast<unsigned long long*>(workspace) : nullptr;
  int32_t* parent = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + (best ? (size_t)total * 8 : 0));
  int32_t* area = parent + total;
  const int conn8 = connectivity == 8;
  hipStream_t s = as_stream(stream);
  int64_t wbase = 0;
  for (int n0 = 0; n0 < N;) {                                          // one launch sequence per SG_SIEVE_GROUP images (fewer only beyond 2^30 workgroups)
    SieveImages im;
    int64_t tiles = 0, blks = 0;
    n0 += sieve_group(image_hw, out_offset, N, n0, &wbase, &im, &tiles, &blks);
    const dim3 gp((unsigned)blks);
    if (min_region > 1) {                                              // min_region = 1: no region is small, the apply kernel copies
      SG_TRY(sieve_label(labels, im, tiles, blks, conn8, parent, area, best, s));
      if (best) {
        hipLaunchKernelGGL(sieve_choose_kernel, gp, dim3(256), 0, s, im, conn8, min_region, parent, area, best);
        SG_LAUNCH_CHECK();
      }
    } else if (labels_out == labels) {
      continue;
    }
    hipLaunchKernelGGL(sieve_apply_kernel, gp, dim3(256), 0, s, labels, labels_out, im, min_region > 1 ? fill : SV_COPY, min_region, bg_idx, parent,
                       area, best);
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}

extern "C" size_t sg_regions_workspace_bytes(int64_t n_pixels_total, int64_t max_regions) {
  if (n_pixels_total < 0 || max_regions < 1) return 0;
  // parent int32 + area / row int32 per pixel, and the scan's block array: one int32 per workgroup of a launch sequence, and its total
  return (size_t)n_pixels_total * 8 + align_up(4 * (size_t)(cdiv(n_pixels_total, SV_PIX) + SV_GROUP + 1), 8);
}

extern "C" int sg_regions(const int64_t* labels, const float* conf, const int32_t* image_hw, const int64_t* out_offset, int N, int connectivity,
                          int64_t min_area, int64_t skip_label, int use_skip, int64_t max_regions, int64_t* table, int32_t* region_of,
                          int64_t* counts, void* workspace, size_t workspace_bytes, sg_stream stream) {
  SG_REQUIRE(labels && image_hw && out_offset && table && counts && workspace, "sg_regions: null pointer");
  SG_REQUIRE(connectivity == 4 || connectivity == 8, "sg_regions: connectivity=%d is neither 4 nor 8", connectivity);
  SG_REQUIRE(min_area >= 1, "sg_regions: min_area=%lld must be >= 1 (a region is listed when its area is at least it)", (long long)min_area);
  SG_REQUIRE(max_regions >= 1, "sg_regions: max_regions=%lld must be >= 1", (long long)max_regions);
  SG_REQUIRE(N >= 1, "sg_regions: N=%d images", N);
  int64_t total = 0;
  for (int n = 0; n < N; ++n) {
    const int64_t h = image_hw[2 * n], w = image_hw[2 * n + 1];
    SG_REQUIRE(h > 0 && w > 0, "sg_regions: image %d has non-positive size %lld x %lld", n, (long long)h, (long long)w);
    SG_REQUIRE(out_offset[n] >= 0, "sg_regions: out_offset[%d]=%lld is negative", n, (long long)out_offset[n]);
    total += h * w;
    SG_REQUIRE(total <= SV_MAX_PIXELS, "sg_regions: the images up to %d hold 2^31 or more pixels (row indices and roots are 32-bit)", n);
  }
  SG_REQUIRE((((uintptr_t)labels) & 7) == 0 && (((uintptr_t)table) & 7) == 0 && (((uintptr_t)counts) & 7) == 0 && (((uintptr_t)workspace) & 7) == 0,
             "sg_regions: labels, table, counts and the workspace must be 8-byte aligned");
  SG_REQUIRE((((uintptr_t)conf) & 3) == 0 && (((uintptr_t)region_of) & 3) == 0, "sg_regions: conf and region_of must be 4-byte aligned");
  const size_t need = sg_regions_workspace_bytes(total, max_regions);
  SG_REQUIRE(workspace_bytes >= need, "sg_regions: workspace too small: %zu bytes given, %zu needed for %lld pixels", workspace_bytes, need,
             (long long)total);
  // workspace: parent int32 [total], area int32 [total] (a root's entry becomes its row), blk int32 [workgroups of a sequence + 1]
  int32_t* parent = reinterpret_cast<int32_t*>(workspace);
  int32_t* area = parent + total;
  int32_t* blk = area + total;
  const int conn8 = connectivity == 8;
  const RegionRule ru = {(long long)min_area, (long long)skip_label, use_skip != 0};
  hipStream_t s = as_stream(stream);
  int64_t wbase = 0;
  for (int n0 = 0; n0 < N;) {                                          // one launch sequence per SG_SIEVE_GROUP images, as sg_sieve
    SieveImages im;
    int64_t tiles = 0, blks = 0;
    const int image0 = n0;
    n0 += sieve_group(image_hw, out_offset, N, n0, &wbase, &im, &tiles, &blks);
    const dim3 gp((unsigned)blks);
    SG_TRY(sieve_label(labels, im, tiles, blks, conn8, parent, area, nullptr, s));
    hipLaunchKernelGGL(regions_count_kernel, gp, dim3(256), 0, s, labels, im, ru, parent, area, blk);
    SG_LAUNCH_CHECK();
    // the rows of the sequences before this one wait in counts[N]: the host never sees them
    hipLaunchKernelGGL(regions_scan_kernel, dim3(1), dim3(RG_SCAN), 0, s, blk, (int)blks, im, image0, image0 == 0 ? 1 : 0, N, counts);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(regions_scatter_kernel, gp, dim3(256), 0, s, labels, conf, im, ru, image0, parent, area, blk, max_regions, table);
    SG_LAUNCH_CHECK();
    RegionTiles rt;                                                    // an eighth of the sieve_local tiles, rounded up per image: below 2^30
    int64_t rtiles = 0;
    for (int k = 0; k <= SV_GROUP; ++k) {
      rt.prefix[k] = (int)rtiles;
      if (k < im.n) rtiles += cdiv(im.h[k], RG_TH) * cdiv(im.w[k], SV_TW);
    }
    hipLaunchKernelGGL(regions_reduce_kernel, dim3((unsigned)rtiles), dim3(256), 0, s, conf, im, rt, parent, area, max_regions, table, region_of);
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}
