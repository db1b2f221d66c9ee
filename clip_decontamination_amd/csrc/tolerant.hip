// Relaxed precision / recall and the boundary F-score: per class, the marked pixels of one label map that have a marked pixel of the same
// class in the other map within a Euclidean tolerance (the definition: include/segearth_hip.h).
// The disk is a stack of row segments: with w(dy) = isqrt(tol_sq - dy*dy), near_L(p,k) holds iff for some |dy| <= r = isqrt(tol_sq) row
// py + dy of L holds a marked pixel of class k within w(dy) columns of px.  Per image, per group of G = min(K, 8) classes [c0, c0 + G),
// and once per direction (target truth / source prediction, then target prediction / source truth):
//   row pass    : over the TARGET map.  One workgroup sweeps a row twice.  Left to right: a block-wide max-scan of "last marked column of
//                 class c" per class of the group (G scans in registers; lanes of a wave by shuffles, the four waves through LDS, the
//                 carry from chunk to chunk), which gives the distance to the nearest marked pixel of class c at or left of every column.
//                 Right to left: the min-scan of "next marked column", and the byte becomes the smaller of the two distances, capped
//                 at 255: hd[c][y][x], one uint8 plane per class of the group.  A lane reads back only bytes it wrote itself.
//                 In contour mode the mark is computed on the fly from the rows above and below.
//   count       : over the SOURCE map, a lane per column, TL_RUN consecutive rows per lane.  A counted, marked source of class k in the
//                 group tests dy = 0 first (hd[k][y][x] <= r; with prediction equal to truth every pixel ends here) and then walks
//                 |dy| = 1 .. r, comparing hd[k][y -+ dy][x] with w(dy) from a table in LDS, TL_WALK rows above and below loaded ahead of
//                 their compares; it stops at the first hit.  The work per searched pixel is at most 2r + 1 bytes: linear in r.
//                 The lane's bins (source: k, matched: K + k) go to 2K 32-bit LDS bins through lm_add_stream (common.h), then one 64-bit add
//                 per non-zero bin per workgroup into the two rows of `counts` the direction owns.
// The planes are reused by every group and direction in stream order: the workspace is G planes whatever K is.
// Integers and integer atomics only; no workgroup waits for another; nothing visits the host; the inputs are only read.
#include "common.h"

namespace sg {

constexpr int TL_MAX_SQ = 254 * 254;
constexpr int TL_MAX_K = LM_MAX_K;
constexpr int TL_GROUP = 8;                      // classes per pass: planes of the workspace
constexpr int TL_ROW_RUN = 8;                    // consecutive pixels per lane per chunk of the row pass
constexpr int TL_ROW_CHUNK = 256 * TL_ROW_RUN;
constexpr int TL_ROW_MAX_BLOCKS = 1 << 16;       // workgroups of the row pass: rows beyond it are looped over
constexpr int TL_RUN = 8;                        // consecutive rows per lane per tile of the count
constexpr int TL_WALK = 8;                       // rows above and below a lane of the count loads ahead
constexpr int TL_WG_PER_CU = 8;
constexpr int TL_NONE_LEFT = -256;               // "no marked column yet": any column minus it is capped
constexpr int TL_NONE_RIGHT = 0x7fffffff;

__device__ __forceinline__ int tl_isqrt(int v) {                          // floor(sqrt(v)), 0 <= v <= 254^2: the float is a first guess only
  int w = (int)sqrtf((float)v);
  while (w * w > v) --w;
  while ((w + 1) * (w + 1) <= v) ++w;
  return w;
}

// class codes of TL_ROW_RUN consecutive pixels from column u0 of row y: c - c0 for a marked pixel of a class of the group, else -1
template <typename T>
__device__ __forceinline__ void tl_row_codes(const T* __restrict__ map, int64_t y, int H, int W, int64_t u0, int rzl, int mode, int c0, int G,
                                             int (&code)[TL_ROW_RUN]) {
  const T* row = map + y * W;
  int64_t v[TL_ROW_RUN];
  bool mk[TL_ROW_RUN];
  lm_load_run<TL_ROW_RUN>(row, u0, W, rzl, v);
  if (mode == SG_TOL_CONTOUR) {
    const bool ha = y > 0, hb = y + 1 < H;
    int64_t up[TL_ROW_RUN], dn[TL_ROW_RUN];
    if (ha) lm_load_run<TL_ROW_RUN>(row - W, u0, W, rzl, up);
    if (hb) lm_load_run<TL_ROW_RUN>(row + W, u0, W, rzl, dn);
    const bool hl = u0 > 0 && u0 < W, hr = u0 + TL_ROW_RUN < W;
    const int64_t prev = hl ? lm_value(row, u0 - 1, rzl) : 0;
    const int64_t next = hr ? lm_value(row, u0 + TL_ROW_RUN, rzl) : 0;
#pragma unroll
    for (int j = 0; j < TL_ROW_RUN; ++j) {
      const bool l = j == 0 ? (hl && v[0] != prev) : v[j] != v[j - 1];
      const bool r = j == TL_ROW_RUN - 1 ? (hr && v[j] != next) : (u0 + j + 1 < W && v[j] != v[j + 1 < TL_ROW_RUN ? j + 1 : j]);
      mk[j] = l || r || (ha && v[j] != up[j]) || (hb && v[j] != dn[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < TL_ROW_RUN; ++j) mk[j] = true;
  }
#pragma unroll
  for (int j = 0; j < TL_ROW_RUN; ++j) {
    const uint64_t c = (uint64_t)v[j] - (uint64_t)c0;
    code[j] = (mk[j] && u0 + j < W && c < (uint64_t)G) ? (int)c : -1;
  }
}

// hd[c][y][x] of one image: `hd` points at the image's first byte of plane 0, the planes lie `plane` bytes apart
template <typename T>
__global__ __launch_bounds__(256) void tl_row_kernel(const T* __restrict__ map, int H, int W, int rzl, int mode, int c0, int G, uint8_t* hd,
                                                     size_t plane) {
  __shared__ int wave_edge[2][4][TL_GROUP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int par = 0;                                                             // LDS slot of the chunk; it keeps alternating
  const int64_t nchunks = ((int64_t)W + TL_ROW_CHUNK - 1) / TL_ROW_CHUNK;
  for (int64_t y = blockIdx.x; y < H; y += gridDim.x) {
    uint8_t* out = hd + y * W;
    int carry[TL_GROUP];
    // ---- left to right: the distance to the nearest marked pixel of class c at or left of the column
#pragma unroll
    for (int c = 0; c < TL_GROUP; ++c) carry[c] = TL_NONE_LEFT;
    for (int64_t ch = 0; ch < nchunks; ++ch, par ^= 1) {                   // block-uniform
      const int64_t u0 = ch * TL_ROW_CHUNK + (int64_t)tid * TL_ROW_RUN;
      int code[TL_ROW_RUN];
      tl_row_codes(map, y, H, W, u0, rzl, mode, c0, G, code);
      int s[TL_GROUP];
#pragma unroll
      for (int c = 0; c < TL_GROUP; ++c) {
        if (c >= G) continue;                                              // uniform
        int inc = TL_NONE_LEFT;
#pragma unroll
        for (int j = 0; j < TL_ROW_RUN; ++j)
          if (code[j] == c) inc = (int)(u0 + j);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(inc, o);
          if (lane >= o && t > inc) inc = t;
        }
        if (lane == 63) wave_edge[par][wave][c] = inc;
        s[c] = __shfl_up(inc, 1);                                          // exclusive: the lanes before this one
        if (lane == 0) s[c] = TL_NONE_LEFT;
      }
      __syncthreads();                                                     // the other parity is written next: one barrier per chunk
#pragma unroll
      for (int c = 0; c < TL_GROUP; ++c) {
        if (c >= G) continue;
        int all = carry[c];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int t = wave_edge[par][w][c];
          if (w < wave && t > s[c]) s[c] = t;
          if (t > all) all = t;
        }
        if (carry[c] > s[c]) s[c] = carry[c];
        carry[c] = all;
        uint8_t b[TL_ROW_RUN];
#pragma unroll
        for (int j = 0; j < TL_ROW_RUN; ++j) {
          if (code[j] == c) s[c] = (int)(u0 + j);
          const int64_t dist = u0 + j - (int64_t)s[c];
          b[j] = (uint8_t)(dist < 255 ? dist : 255);
        }
        uint8_t* o = out + (size_t)c * plane;
        if (u0 + TL_ROW_RUN <= W) {
          __builtin_memcpy(o + u0, b, sizeof(b));
        } else {
#pragma unroll
          for (int j = 0; j < TL_ROW_RUN; ++j)
            if (u0 + j < W) o[u0 + j] = b[j];
        }
      }
    }
    // ---- right to left: the nearest marked pixel at or right of the column; the byte becomes the smaller distance
#pragma unroll
    for (int c = 0; c < TL_GROUP; ++c) carry[c] = TL_NONE_RIGHT;
    for (int64_t ch = nchunks - 1; ch >= 0; --ch, par ^= 1) {
      const int64_t u0 = ch * TL_ROW_CHUNK + (int64_t)tid * TL_ROW_RUN;
      int code[TL_ROW_RUN];
      tl_row_codes(map, y, H, W, u0, rzl, mode, c0, G, code);
      int s[TL_GROUP];
#pragma unroll
      for (int c = 0; c < TL_GROUP; ++c) {
        if (c >= G) continue;
        int inc = TL_NONE_RIGHT;
#pragma unroll
        for (int j = TL_ROW_RUN - 1; j >= 0; --j)
          if (code[j] == c) inc = (int)(u0 + j);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_down(inc, o);
          if (lane + o < 64 && t < inc) inc = t;
        }
        if (lane == 0) wave_edge[par][wave][c] = inc;
        s[c] = __shfl_down(inc, 1);                                        // exclusive: the lanes after this one
        if (lane == 63) s[c] = TL_NONE_RIGHT;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < TL_GROUP; ++c) {
        if (c >= G) continue;
        int all = carry[c];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int t = wave_edge[par][w][c];
          if (w > wave && t < s[c]) s[c] = t;
          if (t < all) all = t;
        }
        if (carry[c] < s[c]) s[c] = carry[c];
        carry[c] = all;
        uint8_t* o = out + (size_t)c * plane;
        const bool whole = u0 + TL_ROW_RUN <= W;
        uint8_t b[TL_ROW_RUN];
        if (whole) {
          __builtin_memcpy(b, o + u0, sizeof(b));
        } else {
#pragma unroll
          for (int j = 0; j < TL_ROW_RUN; ++j) b[j] = u0 + j < W ? o[u0 + j] : (uint8_t)255;
        }
#pragma unroll
        for (int j = TL_ROW_RUN - 1; j >= 0; --j) {
          if (code[j] == c) s[c] = (int)(u0 + j);
          const int64_t dist = (int64_t)s[c] - (u0 + j);                   // >= 0 for every column < W; columns past W are not stored
          if (dist < (int64_t)b[j]) b[j] = (uint8_t)dist;
        }
        if (whole) {
          __builtin_memcpy(o + u0, b, sizeof(b));
        } else {
#pragma unroll
          for (int j = 0; j < TL_ROW_RUN; ++j)
            if (u0 + j < W) o[u0 + j] = b[j];
        }
      }
    }
  }
}

// value of the source map at pixel i: the prediction as it is, the truth after reduce_zero_label
template <bool GT64>
__device__ __forceinline__ int64_t tl_truth(const void* gtv, int64_t i, int rzl) {
  return GT64 ? lm_value(reinterpret_cast<const int64_t*>(gtv), i, rzl) : lm_value(reinterpret_cast<const uint8_t*>(gtv), i, rzl);
}

template <bool GT64>
__device__ __forceinline__ int64_t tl_source(const int64_t* labels, const void* gtv, int src_gt, int64_t i, int rzl) {
  return src_gt ? tl_truth<GT64>(gtv, i, rzl) : labels[i];
}

// One direction of one class group of one image.  Tiles of TL_RUN rows x 256 columns, tile = row band * col_groups + column group.
// counts points at the first of the direction's two rows (source, matched).
template <bool GT64>
__global__ __launch_bounds__(256) void tl_count_kernel(const int64_t* __restrict__ labels, const void* __restrict__ gtv,
                                                       const uint8_t* __restrict__ hd, size_t plane, int H, int W, int tol_sq, int r, int mode,
                                                       int src_gt, int c0, int G, int K, int ignore_index, int rzl, int64_t ntiles,
                                                       int col_groups, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t bins[2 * TL_MAX_K];
  __shared__ uint8_t wtab[256];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < 2 * K; i += 256) bins[i] = 0u;
  wtab[tid] = tid <= r ? (uint8_t)tl_isqrt(tol_sq - tid * tid) : (uint8_t)0;          // w(dy), dy = 0 .. r <= 254
  __syncthreads();

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {      // block-uniform
    const int64_t x = (tile % col_groups) * 256 + tid, y0 = (tile / col_groups) * TL_RUN;
    int bsrc[TL_RUN], bhit[TL_RUN];
#pragma unroll
    for (int j = 0; j < TL_RUN; ++j) bsrc[j] = bhit[j] = -1;
    if (x < W) {
#pragma unroll
      for (int j = 0; j < TL_RUN; ++j) {
        const int64_t y = y0 + j;
        if (y >= H) continue;
        const int64_t i = y * W + x;
        const int64_t g = tl_truth<GT64>(gtv, i, rzl);
        const int64_t v = src_gt ? g : labels[i];
        const uint64_t c = (uint64_t)v - (uint64_t)c0;
        bool in = g != (int64_t)ignore_index && c < (uint64_t)G;
        if (in && mode == SG_TOL_CONTOUR)
          in = (x > 0 && tl_source<GT64>(labels, gtv, src_gt, i - 1, rzl) != v) || (x + 1 < W && tl_source<GT64>(labels, gtv, src_gt, i + 1, rzl) != v) ||
               (y > 0 && tl_source<GT64>(labels, gtv, src_gt, i - W, rzl) != v) || (y + 1 < H && tl_source<GT64>(labels, gtv, src_gt, i + W, rzl) != v);
        if (!in) continue;
        bsrc[j] = (int)v;
        const uint8_t* col = hd + (size_t)c * plane + x;                   // hd[c][.][x]
        bool found = (int)col[y * W] <= r;
        for (int d0 = 1; d0 <= r && !found; d0 += TL_WALK) {
          int a[TL_WALK], b[TL_WALK];
#pragma unroll
          for (int t = 0; t < TL_WALK; ++t) {                              // the loads of a batch before its compares
            const int dy = d0 + t;
            a[t] = (dy <= r && y - dy >= 0) ? (int)col[(y - dy) * W] : 255;
            b[t] = (dy <= r && y + dy < H) ? (int)col[(y + dy) * W] : 255;
          }
#pragma unroll
          for (int t = 0; t < TL_WALK; ++t) {
            const int w = (int)wtab[d0 + t <= r ? d0 + t : r];             // a capped byte (255) is above every w
            found = found || a[t] <= w || b[t] <= w;
          }
        }
        if (found) bhit[j] = K + (int)v;
      }
    }
    lm_add_stream<TL_RUN>(bsrc, bins, lane);
    lm_add_stream<TL_RUN>(bhit, bins, lane);
  }
  __syncthreads();
  for (int i = tid; i < 2 * K; i += 256) {
    const uint32_t v = bins[i];
    if (v != 0u) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

template <typename T>
static int tl_row_pass(const T* map, int H, int W, int rzl, int mode, int c0, int G, uint8_t* hd, size_t plane, hipStream_t st) {
  hipLaunchKernelGGL(tl_row_kernel<T>, dim3((unsigned)(H < TL_ROW_MAX_BLOCKS ? H : TL_ROW_MAX_BLOCKS)), dim3(256), 0, st, map, H, W, rzl, mode, c0, G,
                     hd, plane);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" size_t sg_tolerant_workspace_bytes(int64_t n_pixels_total, int K) {
  if (n_pixels_total < 0 || K < 1 || K > TL_MAX_K) return 0;
  return (size_t)(K < TL_GROUP ? K : TL_GROUP) * lm_plane_bytes(n_pixels_total);
}

extern "C" int sg_tolerant_accumulate(const int64_t* labels, const void* gt, int gt_format, const int32_t* image_hw, const int64_t* offset,
                                      const int32_t* tol_sq, int N, int K, int mode, int ignore_index, int reduce_zero_label, int64_t* counts,
                                      void* workspace, size_t workspace_bytes, sg_stream s) {
  const char* who = "sg_tolerant_accumulate";
  SG_REQUIRE(labels && gt && image_hw && offset && tol_sq && counts && workspace, "%s: null pointer", who);
  SG_REQUIRE(gt_format == SG_GT_U8 || gt_format == SG_GT_I64, "%s: unknown ground-truth format %d", who, gt_format);
  SG_REQUIRE(mode == SG_TOL_REGION || mode == SG_TOL_CONTOUR, "%s: unknown mode %d", who, mode);
  SG_REQUIRE(K >= 1 && K <= TL_MAX_K, "%s: K=%d outside [1, %d] (the cap of sg_confusion_accumulate)", who, K, TL_MAX_K);
  const auto tolerance = [&](int n) -> int {
    SG_REQUIRE(tol_sq[n] >= 0 && tol_sq[n] <= TL_MAX_SQ, "%s: tol_sq[%d]=%d outside [0, %d]", who, n, tol_sq[n], TL_MAX_SQ);
    return SG_OK;
  };
  int64_t total = 0;
  SG_TRY(lm_check_images(who, image_hw, offset, N, false, tolerance, &total));
  SG_REQUIRE(lm_aligned8(labels) && (gt_format == SG_GT_U8 || lm_aligned8(gt)) && lm_aligned8(counts), "%s: int64 buffers must be 8-byte aligned", who);
  const size_t need = sg_tolerant_workspace_bytes(total, K);
  SG_REQUIRE(workspace_bytes >= need, "%s: workspace too small: %zu bytes given, %zu needed for %lld pixels and K=%d", who, workspace_bytes, need,
             (long long)total, K);

  const size_t plane = lm_plane_bytes(total);
  uint8_t* hd = reinterpret_cast<uint8_t*>(workspace);
  const bool gt64 = gt_format == SG_GT_I64;
  const int rzl = reduce_zero_label ? 1 : 0;
  const hipStream_t st = as_stream(s);
  const int64_t cap = (int64_t)device_cu_count() * TL_WG_PER_CU;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  auto count = gt64 ? tl_count_kernel<true> : tl_count_kernel<false>;
  for (int n = 0; n < N; ++n) {
    const int H = image_hw[2 * n], W = image_hw[2 * n + 1];
    const int64_t o = offset[n];
    const int64_t* lab_n = labels + o;
    const void* gt_n = lm_gt_at(gt, gt_format, o);
    int r = 0;
    while ((r + 1) * (r + 1) <= tol_sq[n]) ++r;
    const int64_t col_groups = cdiv(W, 256), ntiles = col_groups * cdiv(H, TL_RUN);
    const int64_t blocks = ntiles < cap ? ntiles : cap;
    for (int c0 = 0; c0 < K; c0 += TL_GROUP) {
      const int G = K - c0 < TL_GROUP ? K - c0 : TL_GROUP;
      for (int src_gt = 0; src_gt < 2; ++src_gt) {                         // 0: targets in the truth, sources in the prediction (rows 0, 1)
        if (src_gt)
          SG_TRY(tl_row_pass(lab_n, H, W, 0, mode, c0, G, hd + o, plane, st));
        else if (gt64)
          SG_TRY(tl_row_pass(reinterpret_cast<const int64_t*>(gt_n), H, W, rzl, mode, c0, G, hd + o, plane, st));
        else
          SG_TRY(tl_row_pass(reinterpret_cast<const uint8_t*>(gt_n), H, W, rzl, mode, c0, G, hd + o, plane, st));
        hipLaunchKernelGGL(count, dim3((unsigned)blocks), dim3(256), 0, st, lab_n, gt_n, (const uint8_t*)(hd + o), plane, H, W, tol_sq[n], r, mode,
                           src_gt, c0, G, K, ignore_index, rzl, ntiles, (int)col_groups, cnt + (size_t)(2 * src_gt) * K);
        SG_LAUNCH_CHECK();
      }
    }
  }
  return SG_OK;
}
