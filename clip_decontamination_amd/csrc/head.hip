// Segmentation head: everything after the vision tower.
//   cosine_logits : segmentor.py:309-336 (CLS normalise, cls_logits, similarity-weighted global debias),
//                   :374-379 (L2 normalise, tokens @ T^T, + lambda * cls_logits)
//   stitch        : segmentor.py:388-391 bilinear upsample of each tile's logits, :436-447 un-pad,
//                   overlap-add, count-normalise -- fused, write-once per canvas pixel (the reference
//                   re-writes the whole canvas once per tile)
//   resize        : F.interpolate(mode='bilinear', align_corners=False) (segmentor.py:449)
//   postprocess   : segmentor.py:475-489
// All HBM-bound; one pass over the data each.
#include "rowops.h"

namespace sg {

// ---- cosine logits -------------------------------------------------------------------------------------------
// 16 lanes per token, four tokens per wave at a time, CL_TPW tokens per wave.  T (Q x E) is staged once per workgroup in LDS.
constexpr int CL_TPW = 8, CL_TPB = 4 * CL_TPW, CL_MAXV = 32;   // E <= 64 * CL_MAXV
template <int NV>      // NV = compile-time bound on E / 64 (features of a token held in NV registers per lane)
__global__ __launch_bounds__(256) void cosine_logits_kernel(const float* __restrict__ tokens, const float* __restrict__ cls,
                                                            const float* __restrict__ text, int n, int E, int Q, float debias,
                                                            float lambda, float* __restrict__ logits) {
  extern __shared__ float sm[];
  float* sT = sm;                    // [Q][E]
  float* sC = sm + (size_t)Q * E;    // [E] unit-norm CLS
  float* sCL = sC + E;               // [Q] cls logits
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool use_cls = cls != nullptr;
  for (int i = tid; i < Q * E; i += 256) sT[i] = text[i];
  if (use_cls) {
    for (int i = tid; i < E; i += 256) sC[i] = cls[(int64_t)b * E + i];
    __syncthreads();
    if (wave == 0) {                                       // cls /= ||cls||  (segmentor.py:310)
      float ss = 0.f;
      for (int i = lane; i < E; i += 64) ss += sC[i] * sC[i];
      const float nrm = sqrtf(wave_sum(ss));
      for (int i = lane; i < E; i += 64) sC[i] = sC[i] / nrm;
    }
    __syncthreads();
    for (int q = wave; q < Q; q += 4) {                    // cls_logits = cls @ T^T  (:311)
      float d = 0.f;
      for (int i = lane; i < E; i += 64) d += sC[i] * sT[q * E + i];
      d = wave_sum(d);
      if (lane == 0) sCL[q] = d;
    }
  }
  __syncthreads();
  // Four tokens per wave at a time (16 lanes each, CL_TPW tokens per wave in all): the staging above is paid once per CL_TPB tokens,
  // a token's features are read from HBM once (one float4 per lane per 64 channels) and kept in registers for the three passes
  // (norm / debias, renormalise, Q dot products), and every reduction is a 4-step shuffle inside the 16-lane group instead of a
  // 6-step wave reduction per token.
  const int sub = lane >> 4, sl = lane & 15;
  auto group_sum = [](float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  const bool deb = use_cls && debias != 0.f;
  for (int tt = 0; tt < CL_TPW; tt += 4) {
    const int t = blockIdx.x * CL_TPB + wave * CL_TPW + tt + sub;
    if (blockIdx.x * CL_TPB + wave * CL_TPW + tt >= n) break;             // wave-uniform: none of the four tokens exists
    const float* f = tokens + ((int64_t)b * n + (t < n ? t : n - 1)) * E;
    float4 x[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i = 4 * sl + 64 * k;
      x[k] = i < E ? *reinterpret_cast<const float4*>(f + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // similarity-weighted debias (:322-336): f' = f - cls * (cos(f, cls) * factor); cls already unit norm,
    // the reference renormalises it once more (a no-op up to rounding) -- reproduced for fidelity.
    float ff = 0.f, fc = 0.f, cc = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i = 4 * sl + 64 * k;
      if (i < E) {
        ff += (x[k].x * x[k].x + x[k].y * x[k].y) + (x[k].z * x[k].z + x[k].w * x[k].w);
        if (use_cls) {
          const float4 c4 = *reinterpret_cast<const float4*>(sC + i);
          fc += (x[k].x * c4.x + x[k].y * c4.y) + (x[k].z * c4.z + x[k].w * c4.w);
          cc += (c4.x * c4.x + c4.y * c4.y) + (c4.z * c4.z + c4.w * c4.w);
        }
      }
    }
    ff = group_sum(ff);
    float w = 0.f;
    if (deb) {
      fc = group_sum(fc); cc = group_sum(cc);
      w = (fc / (sqrtf(ff) * sqrtf(cc))) * debias;
    }
    float nn = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i = 4 * sl + 64 * k;
      if (i < E) {
        if (deb) {
          const float4 c4 = *reinterpret_cast<const float4*>(sC + i);
          x[k].x -= c4.x * w; x[k].y -= c4.y * w; x[k].z -= c4.z * w; x[k].w -= c4.w * w;
        }
        nn += (x[k].x * x[k].x + x[k].y * x[k].y) + (x[k].z * x[k].z + x[k].w * x[k].w);
      }
    }
    const float inv = 1.0f / sqrtf(group_sum(nn));
    for (int q = 0; q < Q; ++q) {
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = 4 * sl + 64 * k;
        if (i < E) {
          const float4 t4 = *reinterpret_cast<const float4*>(sT + q * E + i);
          d += ((x[k].x * inv) * t4.x + (x[k].y * inv) * t4.y) + ((x[k].z * inv) * t4.z + (x[k].w * inv) * t4.w);
        }
      }
      d = group_sum(d);
      if (sl == 0 && t < n) {
        if (use_cls && lambda != 0.f) d += sCL[q] * lambda;
        logits[((int64_t)b * Q + q) * n + t] = d;
      }
    }
  }
}

// Any Q: the text rows pass through LDS in chunks of R rows (as many as fit), inside the kernel.  A wave holds ONE round of four tokens
// (CLW_TPB = 16 tokens per workgroup) so that their debiased features stay in registers across the chunks: read from HBM once, as above.
// Everything per (token, q) is cosine_logits_kernel's, expression for expression: the 16-lane groups, the summation order, the
// debias / renormalise / + lambda * cls_logits steps.  Same expressions are not same bits, though: the compiler fuses the multiply-adds
// of the debias sums (fc, cc) in another order here than there, step by step and differently per instantiation, so with the global
// debias a few outputs are one unit in the last place apart (11 of 2464 at E = 768; equal without it).  The entry therefore sends every
// shape cosine_logits_kernel takes to that kernel and this one only runs with R < Q.
// The price is the staging: Q * E floats per 16 tokens instead of per 32.
constexpr int CLW_TPB = 16;
template <int NV>
__global__ __launch_bounds__(256) void cosine_logits_wide_kernel(const float* __restrict__ tokens, const float* __restrict__ cls,
                                                                 const float* __restrict__ text, int n, int E, int Q, int R, float debias,
                                                                 float lambda, float* __restrict__ logits) {
  extern __shared__ float sm[];
  float* sT = sm;                    // [R][E] the current chunk of text rows
  float* sC = sm + (size_t)R * E;    // [E] unit-norm CLS
  float* sCL = sC + E;               // [R] cls logits of the chunk's rows
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool use_cls = cls != nullptr;
  if (use_cls) {
    for (int i = tid; i < E; i += 256) sC[i] = cls[(int64_t)b * E + i];
    __syncthreads();
    if (wave == 0) {                                       // cls /= ||cls||  (segmentor.py:310)
      float ss = 0.f;
      for (int i = lane; i < E; i += 64) ss += sC[i] * sC[i];
      const float nrm = sqrtf(wave_sum(ss));
      for (int i = lane; i < E; i += 64) sC[i] = sC[i] / nrm;
    }
    __syncthreads();
  }
  const int sub = lane >> 4, sl = lane & 15;
  auto group_sum = [](float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  const bool deb = use_cls && debias != 0.f;
  const int t = blockIdx.x * CLW_TPB + wave * 4 + sub;
  const bool wave_live = blockIdx.x * CLW_TPB + wave * 4 < n;           // wave-uniform; a dead wave still takes part in the barriers below
  const float* f = tokens + ((int64_t)b * n + (t < n ? t : n - 1)) * E;
  float4 x[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = 4 * sl + 64 * k;
    x[k] = (wave_live && i < E) ? *reinterpret_cast<const float4*>(f + i) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float ff = 0.f, fc = 0.f, cc = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = 4 * sl + 64 * k;
    if (i < E) {
      ff += (x[k].x * x[k].x + x[k].y * x[k].y) + (x[k].z * x[k].z + x[k].w * x[k].w);
      if (use_cls) {
        const float4 c4 = *reinterpret_cast<const float4*>(sC + i);
        fc += (x[k].x * c4.x + x[k].y * c4.y) + (x[k].z * c4.z + x[k].w * c4.w);
        cc += (c4.x * c4.x + c4.y * c4.y) + (c4.z * c4.z + c4.w * c4.w);
      }
    }
  }
  ff = group_sum(ff);
  float w = 0.f;
  if (deb) {
    fc = group_sum(fc); cc = group_sum(cc);
    w = (fc / (sqrtf(ff) * sqrtf(cc))) * debias;
  }
  float nn = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = 4 * sl + 64 * k;
    if (i < E) {
      if (deb) {
        const float4 c4 = *reinterpret_cast<const float4*>(sC + i);
        x[k].x -= c4.x * w; x[k].y -= c4.y * w; x[k].z -= c4.z * w; x[k].w -= c4.w * w;
      }
      nn += (x[k].x * x[k].x + x[k].y * x[k].y) + (x[k].z * x[k].z + x[k].w * x[k].w);
    }
  }
  const float inv = 1.0f / sqrtf(group_sum(nn));
  for (int q0 = 0; q0 < Q; q0 += R) {
    const int rq = Q - q0 < R ? Q - q0 : R;
    __syncthreads();                                       // every reader of the previous chunk is done
    const float* src = text + (int64_t)q0 * E;
    for (int i = tid; i < rq * E; i += 256) sT[i] = src[i];
    __syncthreads();
    if (use_cls) {
      for (int q = wave; q < rq; q += 4) {                 // cls_logits = cls @ T^T  (:311)
        float d = 0.f;
        for (int i = lane; i < E; i += 64) d += sC[i] * sT[q * E + i];
        d = wave_sum(d);
        if (lane == 0) sCL[q] = d;
      }
      __syncthreads();
    }
    if (!wave_live) continue;
    for (int q = 0; q < rq; ++q) {
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = 4 * sl + 64 * k;
        if (i < E) {
          const float4 t4 = *reinterpret_cast<const float4*>(sT + q * E + i);
          d += ((x[k].x * inv) * t4.x + (x[k].y * inv) * t4.y) + ((x[k].z * inv) * t4.z + (x[k].w * inv) * t4.w);
        }
      }
      d = group_sum(d);
      if (sl == 0 && t < n) {
        if (use_cls && lambda != 0.f) d += sCL[q] * lambda;
        logits[((int64_t)b * Q + q0 + q) * n + t] = d;
      }
    }
  }
}

// ---- stitch -------------------------------------------------------------------------------------------------------
// Write-once: a pixel's contributions are summed in registers in raster order of the tiles (the reference's `preds[...] += `
// order, so the f32 sum is bit-identical), divided by the count and stored a single time.  The row test of a tile is wave-uniform
// (one canvas row per wave) and runs on the scalar unit; queries go through the registers in chunks of ST_QC.
constexpr int ST_QC = 8, ST_MAXC = 64;
// One 64 x 4 pixel block of one image, the only copy of the gather: every stitch and label-head kernel, single-image or multi-image,
// gets its stitched values here, so they agree bit for bit by construction.  tile_logits / win / tile_image point at the image's first
// tile (tile_image == nullptr: every tile is this image's).  A thread whose row y lies in the image hands each finished chunk to
// sink(x, y, q0, acc, cnt): acc[k] = the sum over the cnt tiles that cover (x, y) for query q0 + k (k < ST_QC, q0 + k < Q), not yet
// divided; x may lie beyond W (cnt = 0 then).
// The gather is in two steps so that a kernel can run the second one several times over one candidate list (the three passes of the
// probability head beyond PP_MAX_Q queries); stitch_block is the two in a row.
struct StitchList { const int* list; int n_cand; };      // more than ST_MAXC candidates: the list is not used, every window is tested
// Step 1, all 256 threads (one barrier): the candidate tiles of the block.
__device__ __forceinline__ StitchList stitch_candidates(const int32_t* __restrict__ win, const int32_t* __restrict__ tile_image, int img,
                                                        int n_tiles, int bx0, int by0) {
  __shared__ int s_list[ST_MAXC];
  __shared__ int s_count;
  // candidate tiles of this block, compacted IN RASTER ORDER by wave 0 (ballot + prefix popcount): the per-pixel loop then visits the
  // handful of overlapping tiles instead of testing all n_tiles windows
  const int lane = threadIdx.x & 63;
  if ((threadIdx.x >> 6) == 0) {
    int base = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 64) {
      const int t = t0 + lane;
      bool hit = false;
      if (t < n_tiles && (tile_image == nullptr || tile_image[t] == img)) {
        const int y1 = win[t * 4 + 0], y2 = win[t * 4 + 1], x1 = win[t * 4 + 2], x2 = win[t * 4 + 3];
        hit = y1 < by0 + 4 && y2 > by0 && x1 < bx0 + 64 && x2 > bx0;
      }
      const unsigned long long m = __ballot(hit);
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      if (hit && pos < ST_MAXC) s_list[pos] = t;
      base += __popcll(m);
    }
    if (lane == 0) s_count = base;
  }
  __syncthreads();
  return {s_list, s_count};
}

// Step 2: the stitched sums of this thread's pixel, chunk by chunk, handed to the sink.  NCHUNK = 0 walks the chunks of the Q queries in
// a run-time loop (every stitch and label-head kernel: their machine code is what it was before the split); NCHUNK > 0 unrolls NCHUNK
// chunks (Q <= NCHUNK * ST_QC) so that q0 is a constant in every call of the sink and a caller can file the values in statically
// indexed registers.
//
// BLEND (sg_stitch_blend, include/segearth_hip.h): every covering tile enters with the weight w = ramp[min(dy, L-1)] * ramp[min(dx, L-1)]
// of the pixel's distance to the tile's own window edges, acc = fma(w, u, acc) with u the unweighted form's value, and the sink gets the
// sum of the weights where the unweighted form hands it the count.  The row weight is wave-uniform (y is, and so is the tile) and is
// read with a scalar index; the column weight is one load per lane.  The table is read through the cache, not staged in LDS: a block
// of 64 x 4 pixels touches at most 68 of its entries per tile, they are shared by every block of the launch (1 KiB at the default
// R = 256, 8 KiB at most), and staging would cost every block a barrier and up to SG_BLEND_MAX_RAMP loads for those few reads.
// With BLEND = false nothing of this is compiled: the unweighted instantiations are what they were.
struct StitchRamp { const float* r = nullptr; int last = 0; };   // the table and L - 1
template <int NCHUNK = 0, bool BLEND = false, class Sink>
__device__ __forceinline__ void stitch_gather(const StitchList& sl, const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                              const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw, int up_h,
                                              int up_w, int pad_t, int pad_l, int H, int W, int bx0, int by0, Sink&& sink,
                                              StitchRamp ramp = {}) {
  const int* s_list = sl.list;
  const int n_cand = sl.n_cand;
  const bool use_list = n_cand <= ST_MAXC;                         // pathological overlap (stride << crop): test every window
  const int n_iter = use_list ? n_cand : n_tiles;
  const int lane = threadIdx.x & 63;
  const int x = bx0 + lane;
  const int y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  if (y >= H) return;
  const int64_t tile_sz = (int64_t)gh * gw;
  constexpr int UNROLL = NCHUNK > 0 ? NCHUNK : 1;                  // 1 = the run-time loop as it always was
#pragma unroll UNROLL
  for (int q0 = 0; NCHUNK > 0 ? q0 < NCHUNK * ST_QC : q0 < Q; q0 += ST_QC) {
    if (NCHUNK > 0 && q0 >= Q) break;
    float acc[ST_QC];
#pragma unroll
    for (int k = 0; k < ST_QC; ++k) acc[k] = 0.f;
    float cnt = 0.f;
    for (int it = 0; it < n_iter; ++it) {                              // raster order = the reference's add order
      const int t = use_list ? s_list[it] : it;
      if (!use_list && tile_image != nullptr && tile_image[t] != img) continue;
      const int y1 = win[t * 4 + 0], y2 = win[t * 4 + 1];
      if (y < y1 || y >= y2) continue;                                 // wave-uniform: the whole wave skips the tile
      const int x1 = win[t * 4 + 2], x2 = win[t * 4 + 3];
      int dy = 0;
      if constexpr (BLEND) dy = __builtin_amdgcn_readfirstlane(min(min(y - y1, y2 - 1 - y), ramp.last));   // 0 <= y - y1 < y2 - y1
      if (x < x1 || x >= x2 || x >= W) continue;
      int ya, yb, xa, xb; float wy0, wy1, wx0, wx1;
      bilinear_tap(y - y1 + pad_t, gh, up_h, ya, yb, wy0, wy1);
      bilinear_tap(x - x1 + pad_l, gw, up_w, xa, xb, wx0, wx1);
      float w = 1.f;
      if constexpr (BLEND) w = ramp.r[dy] * ramp.r[min(min(x - x1, x2 - 1 - x), ramp.last)];                // 0 <= x - x1 < x2 - x1
      const float* base = tile_logits + ((int64_t)t * Q + q0) * tile_sz;
#pragma unroll
      for (int k = 0; k < ST_QC; ++k) {
        if (q0 + k < Q) {
          const float* p = base + (int64_t)k * tile_sz;
          const float top = p[ya * gw + xa] * wx0 + p[ya * gw + xb] * wx1;
          const float bot = p[yb * gw + xa] * wx0 + p[yb * gw + xb] * wx1;
          if constexpr (BLEND) acc[k] = __builtin_fmaf(w, top * wy0 + bot * wy1, acc[k]);
          else acc[k] += top * wy0 + bot * wy1;
        }
      }
      cnt += BLEND ? w : 1.f;                                          // the sum of the weights where the unweighted form counts
    }
    sink(x, y, q0, acc, cnt);
  }
}

template <bool BLEND = false, class Sink>
__device__ __forceinline__ void stitch_block(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                             const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw, int up_h,
                                             int up_w, int pad_t, int pad_l, int H, int W, int bx0, int by0, Sink&& sink,
                                             StitchRamp ramp = {}) {
  const StitchList sl = stitch_candidates(win, tile_image, img, n_tiles, bx0, by0);
  stitch_gather<0, BLEND>(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0, sink, ramp);
}

// The block's stitched values, count-normalised (BLEND: divided by the sum of the weights), into the image's canvas [Q,H,W].
template <bool BLEND = false>
__device__ __forceinline__ void stitch_canvas_block(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                                    const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw,
                                                    int up_h, int up_w, int pad_t, int pad_l, int H, int W, int bx0, int by0,
                                                    float* __restrict__ canvas, StitchRamp ramp = {}) {
  const int64_t plane = (int64_t)H * W;
  stitch_block<BLEND>(tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0,
               [&](int x, int y, int q0, const float (&acc)[ST_QC], float cnt) {
                 if (x >= W) return;
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) canvas[(q0 + k) * plane + (int64_t)y * W + x] = cnt > 0.f ? acc[k] / cnt : 0.f;
               }, ramp);
}

__global__ __launch_bounds__(256) void stitch_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                     int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l,
                                                     int H, int W, float* __restrict__ canvas) {
  stitch_canvas_block(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, blockIdx.x * 64, blockIdx.y * 4, canvas);
}

// stitch_kernel with every tile weighted by the ramp of the distance to its own window edges (stitch_gather's BLEND form).
__global__ __launch_bounds__(256) void stitch_blend_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                           int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l,
                                                           int H, int W, float* __restrict__ canvas, const float* __restrict__ ramp,
                                                           int ramp_len) {
  stitch_canvas_block<true>(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, blockIdx.x * 64, blockIdx.y * 4,
                            canvas, {ramp, ramp_len - 1});
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ src, int C, int h, int w,
                                                              float* __restrict__ dst, int H, int W) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  int ya, yb, xa, xb; float wy0, wy1, wx0, wx1;
  bilinear_tap(y, h, H, ya, yb, wy0, wy1);
  bilinear_tap(x, w, W, xa, xb, wx0, wx1);
  for (int c = 0; c < C; ++c) {
    const float* p = src + (int64_t)c * h * w;
    const float top = p[ya * w + xa] * wx0 + p[ya * w + xb] * wx1;
    const float bot = p[yb * w + xa] * wx0 + p[yb * w + xb] * wx1;
    dst[((int64_t)c * H + y) * W + x] = top * wy0 + bot * wy1;
  }
}

// ---- postprocess ----------------------------------------------------------------------------------------------------
constexpr int PP_MAX_Q = 64;
// Pixel i of an image from its logits to its outputs, the only copy of the tail: sg_postprocess and sg_postprocess_multi differ in how
// logit q is loaded and where the image's outputs start, so they agree bit for bit by construction.  load(q) = logit q of the pixel; the
// image's labels [HW] start at pixel ooff of the flat outputs, its probs [K,HW] (when wanted) at K * ooff.  QMAX is a compile-time
// bound on Q so that v[] lives in registers (a runtime-sized v[64] goes to scratch memory).  The outputs are addressed in here, after
// the exponentials: with the offsets folded into pointers by the caller, postprocess_multi_kernel<64> took 144 VGPRs instead of 85
// (3 waves per SIMD instead of 5).
template <int QMAX, class Load>
__device__ __forceinline__ void class_tail(Load&& load, const int32_t* __restrict__ query_idx, int Q, int K, float logit_scale,
                                           float prob_thd, int bg_idx, float* __restrict__ probs, int64_t* __restrict__ labels,
                                           int64_t ooff, int64_t HW, int64_t i) {
  float v[QMAX];
  float mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < QMAX; ++q)
    if (q < Q) { v[q] = load(q) * logit_scale; mx = fmaxf(mx, v[q]); }
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < QMAX; ++q)
    if (q < Q) { v[q] = expf(v[q] - mx); sum += v[q]; }
  float best = -INFINITY; int arg = 0;
  float* pr = probs ? probs + K * ooff : nullptr;
  for (int c = 0; c < K; ++c) {
    float pc;
    if (K == Q) {
      pc = 0.f;
#pragma unroll
      for (int q = 0; q < QMAX; ++q) if (q == c) pc = v[q] / sum;       // static indexing keeps v[] in registers
    } else {
      // (probabilities * one_hot).max over queries (segmentor.py:484-486): zeros take part in the max
      bool any_other = false;
      float m = -INFINITY;
#pragma unroll
      for (int q = 0; q < QMAX; ++q)
        if (q < Q) { if (query_idx[q] == c) m = fmaxf(m, v[q] / sum); else any_other = true; }
      pc = any_other ? fmaxf(m, 0.f) : m;
    }
    if (pr) pr[c * HW + i] = pc;
    if (pc > best) { best = pc; arg = c; }                                // first maximum wins (torch argmax)
  }
  if (best < prob_thd) arg = bg_idx;
  labels[ooff + i] = arg;
}

template <int QMAX>
__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ logits, const int32_t* __restrict__ query_idx,
                                                          int Q, int K, int64_t HW, float logit_scale, float prob_thd, int bg_idx,
                                                          float* __restrict__ probs, int64_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  class_tail<QMAX>([&](int q) { return logits[q * HW + i]; }, query_idx, Q, K, logit_scale, prob_thd, bg_idx, probs, labels, 0, HW, i);
}

// ---- multi-canvas head: the canvases of N images in one launch ---------------------------------------------------------
// The grid is flattened over (image, block): block_prefix[n] is the first block of image n (an exclusive prefix sum, N + 1
// entries).  The image of a block is found by a wave-uniform binary search; no host loop over images.
__device__ __forceinline__ int image_of_block(const int64_t* __restrict__ block_prefix, int N, int64_t blk) {
  int lo = 0, hi = N;                                              // largest n with block_prefix[n] <= blk (skips empty images)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (block_prefix[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

// The descriptors sg_stitch_multi and sg_label_head_multi share, decoded for this block: image n is (H, W) = image_hw[n], its tiles are
// [t_first, t_first + n_tiles) = image_tiles[n], it owns per_pixel * H * W elements at out_offset[n] of an output of out_elems, and its
// blocks of 64 x 4 pixels follow block_prefix[n] in raster order.
struct ImageBlock { int n, H, W, t_first, n_tiles, bx0, by0; int64_t off; };
// false: a descriptor that would read or write outside the buffers, or a block past the image's last.  The whole block leaves then
// (block-uniform; callers return before any barrier).
__device__ __forceinline__ bool image_block(const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
                                            const int64_t* __restrict__ out_offset, const int64_t* __restrict__ block_prefix, int N, int T,
                                            int64_t per_pixel, int64_t out_elems, ImageBlock& ib) {
  const int n = image_of_block(block_prefix, N, blockIdx.x);
  ib.n = n;
  ib.H = image_hw[2 * n]; ib.W = image_hw[2 * n + 1];
  ib.t_first = image_tiles[2 * n]; ib.n_tiles = image_tiles[2 * n + 1];
  ib.off = out_offset[n];
  if (ib.H <= 0 || ib.W <= 0 || ib.t_first < 0 || ib.n_tiles <= 0 || ib.t_first + ib.n_tiles > T || ib.off < 0 ||
      ib.off + per_pixel * ((int64_t)ib.H * ib.W) > out_elems)
    return false;
  const int64_t local = blockIdx.x - block_prefix[n];
  const int bw = (ib.W + 63) / 64;
  ib.bx0 = (int)(local % bw) * 64; ib.by0 = (int)(local / bw) * 4;
  return local < (int64_t)bw * ((ib.H + 3) / 4);
}

// stitch_kernel for the tiles of many images: tiles [first, first + count) of image n, windows in that image's coordinates,
// its canvas [Q,H,W] at canvas_offset[n].  Both run stitch_canvas_block, so every canvas is bit-identical to sg_stitch on that image
// alone.
__global__ __launch_bounds__(256) void stitch_multi_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                           const int32_t* __restrict__ tile_image, int T, int Q, int gh, int gw,
                                                           int up_h, int up_w, int pad_t, int pad_l, const int32_t* __restrict__ image_hw,
                                                           const int32_t* __restrict__ image_tiles, const int64_t* __restrict__ canvas_offset,
                                                           const int64_t* __restrict__ block_prefix, int N, int64_t canvas_elems,
                                                           float* __restrict__ canvases) {
  ImageBlock ib;
  if (!image_block(image_hw, image_tiles, canvas_offset, block_prefix, N, T, Q, canvas_elems, ib)) return;
  stitch_canvas_block(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first, ib.n,
                      ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, ib.H, ib.W, ib.bx0, ib.by0, canvases + ib.off);
}

// stitch_blend_kernel for the tiles of many images (stitch_multi_kernel's descriptors): every canvas is bit-identical to sg_stitch_blend
// on that image alone.
__global__ __launch_bounds__(256) void stitch_blend_multi_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                                 const int32_t* __restrict__ tile_image, int T, int Q, int gh, int gw,
                                                                 int up_h, int up_w, int pad_t, int pad_l,
                                                                 const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
                                                                 const int64_t* __restrict__ canvas_offset,
                                                                 const int64_t* __restrict__ block_prefix, int N, int64_t canvas_elems,
                                                                 float* __restrict__ canvases, const float* __restrict__ ramp, int ramp_len) {
  ImageBlock ib;
  if (!image_block(image_hw, image_tiles, canvas_offset, block_prefix, N, T, Q, canvas_elems, ib)) return;
  stitch_canvas_block<true>(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first,
                            ib.n, ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, ib.H, ib.W, ib.bx0, ib.by0, canvases + ib.off,
                            {ramp, ramp_len - 1});
}

// postprocess_kernel for N canvases, 256 output pixels per block: canvas n [Q,h,w] at canvas_offset[n]; its outputs are
// labels [H,W] at out_offset[n] and probs [K,H,W] at K * out_offset[n].  When (H,W) != (h,w) the align_corners=False bilinear
// resize of resize_bilinear_kernel is evaluated per output pixel (no resized canvas is written).  Everything after the load is class_tail,
// shared with postprocess_kernel, so the outputs are bit-identical to sg_resize_bilinear + sg_postprocess per image.
template <int QMAX>
__global__ __launch_bounds__(256) void postprocess_multi_kernel(const float* __restrict__ canvases, const int32_t* __restrict__ canvas_hw,
                                                                const int64_t* __restrict__ canvas_offset, const int32_t* __restrict__ out_hw,
                                                                const int64_t* __restrict__ out_offset, const int64_t* __restrict__ block_prefix,
                                                                int N, int64_t canvas_elems, int64_t out_pixels,
                                                                const int32_t* __restrict__ query_idx, int Q, int K, float logit_scale,
                                                                float prob_thd, int bg_idx, float* __restrict__ probs,
                                                                int64_t* __restrict__ labels) {
  const int n = image_of_block(block_prefix, N, blockIdx.x);
  const int h = canvas_hw[2 * n], w = canvas_hw[2 * n + 1], H = out_hw[2 * n], W = out_hw[2 * n + 1];
  const int64_t coff = canvas_offset[n], ooff = out_offset[n];
  const int64_t hw = (int64_t)h * w, HW = (int64_t)H * W;
  if (coff < 0 || coff + Q * hw > canvas_elems || ooff < 0 || ooff + HW > out_pixels) return;
  const int64_t i = (blockIdx.x - block_prefix[n]) * 256 + threadIdx.x;
  if (i >= HW) return;
  const float* logits = canvases + coff;
  const bool resize = h != H || w != W;
  int ya = 0, yb = 0, xa = 0, xb = 0; float wy0 = 0.f, wy1 = 0.f, wx0 = 0.f, wx1 = 0.f;
  if (resize) {
    bilinear_tap((int)(i / W), h, H, ya, yb, wy0, wy1);
    bilinear_tap((int)(i % W), w, W, xa, xb, wx0, wx1);
  }
  class_tail<QMAX>([&](int q) {
    float l;
    if (resize) {
      // resize_bilinear_kernel's arithmetic exactly as it is compiled there, spelled out so that this kernel cannot contract it any
      // other way.  Its channel loop is vectorised two channels at a time (v_pk_fma_f32: first product of each sum fused); an odd
      // last channel runs through the loop's scalar remainder, which fuses the other product of `top` and rounds both products of
      // the final blend.  Mirroring both keeps this bit-identical to sg_resize_bilinear for every Q (pinned by tests/test_gpu_batch.py
      // for even and odd Q; a compiler that vectorised that loop differently would show up there).
#pragma clang fp contract(off)
      const float* p = logits + (int64_t)q * h * w;
      if ((Q & 1) && q == Q - 1) {
        const float top = __builtin_fmaf(p[ya * w + xb], wx1, p[ya * w + xa] * wx0);
        const float bot = __builtin_fmaf(p[yb * w + xa], wx0, p[yb * w + xb] * wx1);
        l = top * wy0 + bot * wy1;
      } else {
        const float top = __builtin_fmaf(p[ya * w + xa], wx0, p[ya * w + xb] * wx1);
        const float bot = __builtin_fmaf(p[yb * w + xa], wx0, p[yb * w + xb] * wx1);
        l = __builtin_fmaf(top, wy0, bot * wy1);
      }
      asm volatile("" : "+v"(l));     // opaque from here on, like a loaded value: the tail compiles as postprocess_kernel's
    } else {
      l = logits[q * hw + i];
    }
    return l;
  }, query_idx, Q, K, logit_scale, prob_thd, bg_idx, probs, labels, ooff, HW, i);
}

// ---- fused label head: stitch -> softmax -> synonym merge -> argmax -> threshold, labels only, any Q ---------------------------
// One 64 x 4 pixel block of one image, shared by the single-image and the multi-image kernel (so the two agree byte for byte).  The
// stitched value of a query is stitch_kernel's because both get it from stitch_block, then divide by the count.  No canvas exists:
// queries pass through the registers in chunks of ST_QC and only a running maximum, the running sum of exp(v - max) and the best (value, class) pair survive a chunk.
//   Online maximum and sum, not a second pass that recomputes the stitched values: the gathers are the cost of this kernel (four loads
//   and seven multiply-adds per covering tile and query, all of it address-dependent), a second pass would double them, while the
//   online form adds one expf per chunk of ST_QC queries (the rescale of the sum when the maximum moves).  The order of every operation
//   is fixed by (pixel, query index), so repeats are byte-identical.
// softmax is monotone, so the class of the largest class probability is the class of the largest scaled logit; among queries that
// share that largest value the lowest class index wins (torch.argmax's first maximum).  Queries whose class lies outside [0,K) only
// take part in the sum, as in postprocess_kernel.  conf = exp(v_best - v_max) / sum = 1 / sum exp(v_q - v_max).
// BLEND (sg_label_head_blend): the stitched value is stitch_blend_kernel's, acc / the sum of the weights, which the sink receives as cnt;
// every statement after it is the same.
template <bool BLEND = false>
__device__ __forceinline__ void label_head_block(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                                 const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw,
                                                 int up_h, int up_w, int pad_t, int pad_l, int H, int W, int bx0, int by0,
                                                 const int32_t* __restrict__ query_idx, int K, float logit_scale, float prob_thd,
                                                 int bg_idx, int64_t* __restrict__ labels, float* __restrict__ conf, StitchRamp ramp = {}) {
  float vmax = -INFINITY, sum = 0.f, best = -INFINITY;
  int best_c = 0;
  stitch_block<BLEND>(tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0,
               [&](int, int, int q0, float (&acc)[ST_QC], float cnt) {
#pragma clang fp contract(off)        // the scaled logit is rounded before the subtraction, as postprocess_kernel compiles it
                 float cm = -INFINITY;
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) { acc[k] = (cnt > 0.f ? acc[k] / cnt : 0.f) * logit_scale; cm = fmaxf(cm, acc[k]); }
                 if (cm > vmax) { sum *= expf(vmax - cm); vmax = cm; }            // the first chunk: sum = 0 * exp(-inf) = 0
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) {
                     sum += expf(acc[k] - vmax);
                     const int c = K == Q ? q0 + k : query_idx[q0 + k];
                     if (c >= 0 && c < K && (acc[k] > best || (acc[k] == best && c < best_c))) { best = acc[k]; best_c = c; }
                   }
               }, ramp);
  const int x = bx0 + (threadIdx.x & 63);
  const int y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  if (y >= H || x >= W) return;
  const float cf = expf(best - vmax) / sum;
  const int64_t o = (int64_t)y * W + x;
  labels[o] = cf < prob_thd ? bg_idx : best_c;
  if (conf) conf[o] = cf;
}

__global__ __launch_bounds__(256) void label_head_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                         int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l, int H,
                                                         int W, const int32_t* __restrict__ query_idx, int K, float logit_scale,
                                                         float prob_thd, int bg_idx, int64_t* __restrict__ labels,
                                                         float* __restrict__ conf) {
  label_head_block(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, blockIdx.x * 64, blockIdx.y * 4,
                   query_idx, K, logit_scale, prob_thd, bg_idx, labels, conf);
}

// The tiles of N images (sg_stitch_multi's descriptors); labels / conf of image n at out_offset[n] pixels of the flat outputs.
__global__ __launch_bounds__(256) void label_head_multi_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                               const int32_t* __restrict__ tile_image, int T, int Q, int gh, int gw,
                                                               int up_h, int up_w, int pad_t, int pad_l,
                                                               const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
                                                               const int64_t* __restrict__ out_offset, const int64_t* __restrict__ block_prefix,
                                                               int N, int64_t out_pixels, const int32_t* __restrict__ query_idx, int K,
                                                               float logit_scale, float prob_thd, int bg_idx, int64_t* __restrict__ labels,
                                                               float* __restrict__ conf) {
  ImageBlock ib;
  if (!image_block(image_hw, image_tiles, out_offset, block_prefix, N, T, 1, out_pixels, ib)) return;
  label_head_block(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first, ib.n,
                   ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, ib.H, ib.W, ib.bx0, ib.by0, query_idx, K, logit_scale, prob_thd, bg_idx,
                   labels + ib.off, conf ? conf + ib.off : nullptr);
}

// label_head_kernel / label_head_multi_kernel over the blended stitch (label_head_block<true>).
__global__ __launch_bounds__(256) void label_head_blend_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                               int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l,
                                                               int H, int W, const int32_t* __restrict__ query_idx, int K,
                                                               float logit_scale, float prob_thd, int bg_idx, int64_t* __restrict__ labels,
                                                               float* __restrict__ conf, const float* __restrict__ ramp, int ramp_len) {
  label_head_block<true>(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, blockIdx.x * 64, blockIdx.y * 4,
                         query_idx, K, logit_scale, prob_thd, bg_idx, labels, conf, {ramp, ramp_len - 1});
}

__global__ __launch_bounds__(256) void label_head_blend_multi_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                                     const int32_t* __restrict__ tile_image, int T, int Q, int gh, int gw,
                                                                     int up_h, int up_w, int pad_t, int pad_l,
                                                                     const int32_t* __restrict__ image_hw,
                                                                     const int32_t* __restrict__ image_tiles,
                                                                     const int64_t* __restrict__ out_offset,
                                                                     const int64_t* __restrict__ block_prefix, int N, int64_t out_pixels,
                                                                     const int32_t* __restrict__ query_idx, int K, float logit_scale,
                                                                     float prob_thd, int bg_idx, int64_t* __restrict__ labels,
                                                                     float* __restrict__ conf, const float* __restrict__ ramp, int ramp_len) {
  ImageBlock ib;
  if (!image_block(image_hw, image_tiles, out_offset, block_prefix, N, T, 1, out_pixels, ib)) return;
  label_head_block<true>(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first, ib.n,
                         ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, ib.H, ib.W, ib.bx0, ib.by0, query_idx, K, logit_scale, prob_thd,
                         bg_idx, labels + ib.off, conf ? conf + ib.off : nullptr, {ramp, ramp_len - 1});
}

// ---- fused top-k head: stitch -> softmax -> synonym merge -> the k best classes with their probabilities, any Q ------------------------
// label_head_block with a sorted list of KTOP (value, class) pairs in place of the single best pair; the per-chunk statements (scaled
// logit, chunk maximum, rescale of the sum, sum of exp) are that function's, copied, so that slot 0 carries sg_label_head's label and
// conf byte for byte.  label_head_block itself is not shared with this one: its machine code stays what it is.
//   The list: larger value first, among equal values the lower class first; an empty slot is (-inf, INT_MAX) and therefore sorts last.
//   Every slot is addressed with a compile-time index in fully unrolled loops (a run-time index would send the arrays to scratch, as
//   class_tail's comment has it).  A query (v, c) with K != Q first looks for a slot that already holds class c and raises it to
//   max(v_slot, v): a class's value is the maximum over its queries, which is the synonym max of the class probabilities because softmax
//   is monotone.  Otherwise it replaces the last slot if it precedes it.  Either way at most one slot is out of place afterwards and it
//   can only have moved up, so one bottom-up pass of KTOP - 1 compare-exchanges restores the order.  With K == Q every class has one
//   query and the search is skipped (block-uniform).
// Outputs are planes [k,H,W] of the image: classes int32 (-1 for a slot no class filled) and probs = expf(v_j - vmax) / sum, the
// expression of label_head_block's conf (0 for an unfilled slot).  No atomics, no LDS beyond the candidate list, nothing proportional
// to Q * H * W; every element is written by its pixel's own thread in an order fixed by (pixel, query index).
constexpr int TOPK_MAX = 8;
template <int KTOP>
__device__ __forceinline__ void topk_head_block(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                                const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw,
                                                int up_h, int up_w, int pad_t, int pad_l, int H, int W, int bx0, int by0,
                                                const int32_t* __restrict__ query_idx, int K, float logit_scale, int k,
                                                int32_t* __restrict__ classes, float* __restrict__ probs) {
  float vmax = -INFINITY, sum = 0.f;
  float tv[KTOP];
  int tc[KTOP];
#pragma unroll
  for (int j = 0; j < KTOP; ++j) { tv[j] = -INFINITY; tc[j] = INT_MAX; }
  const bool merge = K != Q;
  stitch_block(tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0,
               [&](int, int, int q0, float (&acc)[ST_QC], float cnt) {
#pragma clang fp contract(off)        // the scaled logit is rounded before the subtraction, as postprocess_kernel compiles it
                 float cm = -INFINITY;
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) { acc[k] = (cnt > 0.f ? acc[k] / cnt : 0.f) * logit_scale; cm = fmaxf(cm, acc[k]); }
                 if (cm > vmax) { sum *= expf(vmax - cm); vmax = cm; }            // the first chunk: sum = 0 * exp(-inf) = 0
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) {
                     sum += expf(acc[k] - vmax);
                     const float v = acc[k];
                     const int c = merge ? query_idx[q0 + k] : q0 + k;
                     if (c < 0 || c >= K) continue;
                     bool held = false;
                     if (merge) {
#pragma unroll
                       for (int j = 0; j < KTOP; ++j)
                         if (tc[j] == c) { held = true; tv[j] = fmaxf(tv[j], v); }
                     }
                     if (!held && (v > tv[KTOP - 1] || (v == tv[KTOP - 1] && c < tc[KTOP - 1]))) { tv[KTOP - 1] = v; tc[KTOP - 1] = c; }
#pragma unroll
                     for (int j = KTOP - 1; j > 0; --j) {
                       const bool up = tv[j] > tv[j - 1] || (tv[j] == tv[j - 1] && tc[j] < tc[j - 1]);
                       const float fv = tv[j]; const int fc = tc[j];
                       tv[j] = up ? tv[j - 1] : fv; tc[j] = up ? tc[j - 1] : fc;
                       tv[j - 1] = up ? fv : tv[j - 1]; tc[j - 1] = up ? fc : tc[j - 1];
                     }
                   }
               });
  const int x = bx0 + (threadIdx.x & 63);
  const int y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  if (y >= H || x >= W) return;
  const int64_t HW = (int64_t)H * W, o = (int64_t)y * W + x;
#pragma unroll
  for (int j = 0; j < KTOP; ++j)
    if (j < k) {
      const bool filled = tc[j] != INT_MAX;
      const float p = expf(tv[j] - vmax) / sum;
      classes[j * HW + o] = filled ? tc[j] : -1;
      probs[j * HW + o] = filled ? p : 0.f;
    }
}

template <int KTOP>
__global__ __launch_bounds__(256) void topk_head_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows, int T,
                                                        int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l, int H, int W,
                                                        const int32_t* __restrict__ query_idx, int K, float logit_scale, int k,
                                                        int32_t* __restrict__ classes, float* __restrict__ probs) {
  topk_head_block<KTOP>(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, blockIdx.x * 64, blockIdx.y * 4,
                        query_idx, K, logit_scale, k, classes, probs);
}

// The tiles of N images (sg_stitch_multi's descriptors); the planes [k,H,W] of image n at k * out_offset[n] elements of the flat outputs
// (sg_prob_head_multi's layout with k in place of K).
template <int KTOP>
__global__ __launch_bounds__(256) void topk_head_multi_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                              const int32_t* __restrict__ tile_image, int T, int Q, int gh, int gw,
                                                              int up_h, int up_w, int pad_t, int pad_l,
                                                              const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
                                                              const int64_t* __restrict__ out_offset, const int64_t* __restrict__ block_prefix,
                                                              int N, int64_t out_pixels, const int32_t* __restrict__ query_idx, int K,
                                                              float logit_scale, int k, int32_t* __restrict__ classes,
                                                              float* __restrict__ probs) {
  ImageBlock ib;
  if (!image_block(image_hw, image_tiles, out_offset, block_prefix, N, T, 1, out_pixels, ib)) return;   // k * (off + H * W) <= k * out_pixels
  topk_head_block<KTOP>(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first, ib.n,
                        ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, ib.H, ib.W, ib.bx0, ib.by0, query_idx, K, logit_scale, k,
                        classes + k * ib.off, probs + k * ib.off);
}

// ---- the label and top-k heads at another ori_shape: stitch -> bilinear resize -> the same tails, no canvas --------------------------------
// segmentor.py:447-449: preds / count, then F.interpolate(bilinear, align_corners=False) to ori_shape, then the post-process.  An output
// pixel (Y, X) of [OH, OW] over the [h, w] canvas takes the taps of rs_tap(Y, h, OH) and rs_tap(X, w, OW), the STITCHED value of each of
// its four canvas pixels (covering tiles summed in raster order and divided by THAT pixel's count, 0 where no tile covers: neighbouring
// taps can have different counts, so the division comes before the blend), and blends them top row, bottom row, then the two.  The
// blended value goes to the per-chunk statements of label_head_block / topk_head_block with cnt = 1.
//   Two forms get the four values, both from stitched_pixel, and all of it (taps, gather, division, blend) is compiled with fp
//   contraction off, so a value does not depend on the form that asked for it: the two forms agree byte for byte.
//   direct: every thread gathers its own (up to) four canvas pixels; equal taps are gathered once.  Any scale.
//   staged: the block's 64 x 4 output pixels read a canvas footprint of at most rs_span(4, h, OH) x rs_span(64, w, OW) pixels (120 for
//   448 -> 1024 instead of 1024 gathers); the block computes each footprint pixel's chunk of ST_QC queries once into LDS, barrier, every
//   thread blends from LDS, barrier, next chunk.  It runs when the footprint holds at most RS_STAGE_PIX pixels: ST_QC planes of
//   RS_STAGE_PIX floats are the 16 KiB of s_stage.
//   Barriers: in the staged form no thread leaves before the last chunk's second barrier; a thread outside the image only skips its
//   blend and its stores.  The form is chosen per block from block-uniform values, and the multi-image kernels return on a bad
//   descriptor before the first barrier, the whole block at once.
constexpr int RS_STAGE_PIX = 512;
constexpr int RS_AUTO = SG_RESIZED_AUTO, RS_DIRECT = SG_RESIZED_DIRECT, RS_STAGED = SG_RESIZED_STAGED;
// rows (columns) of the canvas that n consecutive output rows (columns) can touch: their source coordinates span (n - 1) in / out, the
// floor and the second tap add one each
__host__ __device__ inline int64_t rs_span(int n, int in, int out) { return ((int64_t)n * in + out - 1) / out + 2; }
__host__ __device__ inline bool rs_fits(int h, int w, int OH, int OW) { return rs_span(4, h, OH) * rs_span(64, w, OW) <= RS_STAGE_PIX; }
// SG_RESIZED_AUTO: the staged form where it fits and the output is larger than the canvas along both axes -- measured 2.1 to 2.8 times
// the direct form's speed at 448 -> 1024 and at 1.5x (a thread of the direct form gathers up to four canvas pixels, the stage holds at
// most two per output pixel).  At the canvas's own size the direct form gathers one pixel per thread and was 5 to 10 % faster
// (0.476 against 0.525 ms), so identity runs direct; so does a mixed up / down scale, which was not measured (profiles/head_resized.jsonl).
__host__ __device__ inline bool rs_want_staged(int flags, int h, int w, int OH, int OW) {
  if (flags == RS_DIRECT || !rs_fits(h, w, OH, OW)) return false;
  return flags == RS_STAGED || (OH > h && OW > w);
}

// bilinear_tap (rowops.h) with every product rounded: the taps of both forms and of the footprint are the same numbers by construction
__device__ __forceinline__ void rs_tap(int dst, int in, int out, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  if (in == out) { i0 = i1 = dst; l0 = 1.f; l1 = 0.f; return; }
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src; i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0; l0 = 1.f - l1;
}

__device__ __forceinline__ float rs_blend(float v00, float v01, float v10, float v11, float wx0, float wx1, float wy0, float wy1) {
#pragma clang fp contract(off)
  const float top = v00 * wx0 + v01 * wx1;
  const float bot = v10 * wx0 + v11 * wx1;
  return top * wy0 + bot * wy1;
}

// The candidate tiles of a canvas rectangle [cx0, cx1] x [cy0, cy1] (stitch_candidates for a footprint that is not 64 x 4), all 256
// threads, one barrier.
__device__ __forceinline__ StitchList rs_candidates(const int32_t* __restrict__ win, const int32_t* __restrict__ tile_image, int img,
                                                    int n_tiles, int cx0, int cy0, int cx1, int cy1) {
  __shared__ int s_list[ST_MAXC];
  __shared__ int s_count;
  const int lane = threadIdx.x & 63;
  if ((threadIdx.x >> 6) == 0) {
    int base = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 64) {
      const int t = t0 + lane;
      bool hit = false;
      if (t < n_tiles && (tile_image == nullptr || tile_image[t] == img)) {
        const int y1 = win[t * 4 + 0], y2 = win[t * 4 + 1], x1 = win[t * 4 + 2], x2 = win[t * 4 + 3];
        hit = y1 <= cy1 && y2 > cy0 && x1 <= cx1 && x2 > cx0;
      }
      const unsigned long long m = __ballot(hit);
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      if (hit && pos < ST_MAXC) s_list[pos] = t;
      base += __popcll(m);
    }
    if (lane == 0) s_count = base;
  }
  __syncthreads();
  return {s_list, s_count};
}

// Canvas pixel (cx, cy), 0 <= cx < w, 0 <= cy < h: out[k] = the stitched value of query q0 + k as stitch_gather defines it -- the tiles
// that cover the pixel in raster order, each tile's bilinear upsample, the sum divided by the count, 0 without a tile.  The only copy.
__device__ __forceinline__ void stitched_pixel(const StitchList& sl, const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                               const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw, int up_h,
                                               int up_w, int pad_t, int pad_l, int cx, int cy, int q0, float (&out)[ST_QC]) {
#pragma clang fp contract(off)
  const bool use_list = sl.n_cand <= ST_MAXC;                      // beyond ST_MAXC candidates: test every window
  const int n_iter = use_list ? sl.n_cand : n_tiles;
  const int64_t tile_sz = (int64_t)gh * gw;
  float acc[ST_QC];
#pragma unroll
  for (int k = 0; k < ST_QC; ++k) acc[k] = 0.f;
  float cnt = 0.f;
  for (int it = 0; it < n_iter; ++it) {                              // raster order = the reference's add order
    const int t = use_list ? sl.list[it] : it;
    if (!use_list && tile_image != nullptr && tile_image[t] != img) continue;
    const int y1 = win[t * 4 + 0], y2 = win[t * 4 + 1];
    if (cy < y1 || cy >= y2) continue;
    const int x1 = win[t * 4 + 2], x2 = win[t * 4 + 3];
    if (cx < x1 || cx >= x2) continue;
    int ya, yb, xa, xb; float wy0, wy1, wx0, wx1;
    rs_tap(cy - y1 + pad_t, gh, up_h, ya, yb, wy0, wy1);
    rs_tap(cx - x1 + pad_l, gw, up_w, xa, xb, wx0, wx1);
    const float* base = tile_logits + ((int64_t)t * Q + q0) * tile_sz;
#pragma unroll
    for (int k = 0; k < ST_QC; ++k) {
      if (q0 + k < Q) {
        const float* p = base + (int64_t)k * tile_sz;
        acc[k] += rs_blend(p[ya * gw + xa], p[ya * gw + xb], p[yb * gw + xa], p[yb * gw + xb], wx0, wx1, wy0, wy1);
      }
    }
    cnt += 1.f;
  }
#pragma unroll
  for (int k = 0; k < ST_QC; ++k) out[k] = cnt > 0.f ? acc[k] / cnt : 0.f;
}

// One 64 x 4 block of OUTPUT pixels of one image: a thread whose pixel (X, Y) lies in the output hands each chunk's resized stitched
// values to sink(q0, acc), acc[k] for query q0 + k.  Returns whether this thread's pixel is in the output.  All 256 threads call it.
// FLIP (sg_tta_head): the instantiation can read the resized canvas mirrored along the width -- with `flip` set the thread of output
// column X takes the taps of column OW - 1 - X and the block's footprint is that of the mirrored columns; what is gathered, divided and
// blended per canvas pixel is the same code.  With FLIP = false nothing of this is compiled and `flip` is not read.
template <bool FLIP = false, class Sink>
__device__ __forceinline__ bool resized_gather(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                               const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw, int up_h,
                                               int up_w, int pad_t, int pad_l, int h, int w, int OH, int OW, int bx0, int by0, int flags,
                                               Sink&& sink, bool flip = false) {
  __shared__ float s_stage[ST_QC * RS_STAGE_PIX];
  int X = bx0 + (threadIdx.x & 63);
  const int Y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  const bool live = Y < OH && X < OW;
  int bxa = bx0, bxb = bx0 + 63 < OW ? bx0 + 63 : OW - 1;            // the block's first and last source column
  if constexpr (FLIP) {
    if (flip) { X = OW - 1 - X; const int t = OW - 1 - bxb; bxb = OW - 1 - bxa; bxa = t; }   // live: 0 <= X < OW either way
  }
  // the block's canvas footprint [fx0, fx1] x [fy0, fy1]: the first tap of its first row / column to the second tap of its last one
  // (taps do not decrease with the output coordinate).  Block-uniform.
  int fy0, fy1, fx0, fx1, unused; float u0, u1;
  rs_tap(by0, h, OH, fy0, unused, u0, u1);
  rs_tap(by0 + 3 < OH ? by0 + 3 : OH - 1, h, OH, unused, fy1, u0, u1);
  rs_tap(bxa, w, OW, fx0, unused, u0, u1);
  rs_tap(bxb, w, OW, unused, fx1, u0, u1);
  const int fw = fx1 - fx0 + 1, npix = (fy1 - fy0 + 1) * fw;
  const StitchList sl = rs_candidates(win, tile_image, img, n_tiles, fx0, fy0, fx1, fy1);
  const bool staged = rs_want_staged(flags, h, w, OH, OW) && npix <= RS_STAGE_PIX;   // block-uniform; npix <= the rs_span product
  int ya = 0, yb = 0, xa = 0, xb = 0; float wy0 = 0.f, wy1 = 0.f, wx0 = 0.f, wx1 = 0.f;
  if (live) {
    rs_tap(Y, h, OH, ya, yb, wy0, wy1);
    rs_tap(X, w, OW, xa, xb, wx0, wx1);
  }
  if (!staged) {
    if (!live) return false;                                         // no barrier below on this path
    for (int q0 = 0; q0 < Q; q0 += ST_QC) {
      float v00[ST_QC], v01[ST_QC], v10[ST_QC], v11[ST_QC], acc[ST_QC];
      stitched_pixel(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, xa, ya, q0, v00);
      if (xb != xa) stitched_pixel(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, xb, ya, q0, v01);
      else {
#pragma unroll
        for (int k = 0; k < ST_QC; ++k) v01[k] = v00[k];
      }
      if (yb != ya) {
        stitched_pixel(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, xa, yb, q0, v10);
        if (xb != xa) stitched_pixel(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, xb, yb, q0, v11);
        else {
#pragma unroll
          for (int k = 0; k < ST_QC; ++k) v11[k] = v10[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < ST_QC; ++k) { v10[k] = v00[k]; v11[k] = v01[k]; }
      }
#pragma unroll
      for (int k = 0; k < ST_QC; ++k) acc[k] = rs_blend(v00[k], v01[k], v10[k], v11[k], wx0, wx1, wy0, wy1);
      sink(q0, acc);
    }
    return true;
  }
  const int i00 = (ya - fy0) * fw + (xa - fx0), i01 = (ya - fy0) * fw + (xb - fx0);
  const int i10 = (yb - fy0) * fw + (xa - fx0), i11 = (yb - fy0) * fw + (xb - fx0);
  for (int q0 = 0; q0 < Q; q0 += ST_QC) {                              // Q is uniform: every thread runs every barrier
    for (int p = threadIdx.x; p < npix; p += 256) {
      float o[ST_QC];
      stitched_pixel(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, fx0 + p % fw, fy0 + p / fw, q0, o);
#pragma unroll
      for (int k = 0; k < ST_QC; ++k) s_stage[k * RS_STAGE_PIX + p] = o[k];
    }
    __syncthreads();
    if (live) {
      float acc[ST_QC];
#pragma unroll
      for (int k = 0; k < ST_QC; ++k) {
        const float* sp = s_stage + k * RS_STAGE_PIX;
        acc[k] = rs_blend(sp[i00], sp[i01], sp[i10], sp[i11], wx0, wx1, wy0, wy1);
      }
      sink(q0, acc);
    }
    __syncthreads();                                                   // the stage is free for the next chunk
  }
  return live;
}

// label_head_block over resized_gather: the per-chunk statements are that function's, copied (its machine code stays what it is); the
// resized value is already count-normalised, so the division by the count is gone.
__device__ __forceinline__ void label_head_resized_block(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                                         const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw,
                                                         int up_h, int up_w, int pad_t, int pad_l, int h, int w, int OH, int OW, int bx0,
                                                         int by0, int flags, const int32_t* __restrict__ query_idx, int K, float logit_scale,
                                                         float prob_thd, int bg_idx, int64_t* __restrict__ labels, float* __restrict__ conf) {
  float vmax = -INFINITY, sum = 0.f, best = -INFINITY;
  int best_c = 0;
  const bool live = resized_gather(tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, h, w, OH, OW, bx0, by0,
                                   flags, [&](int q0, float (&acc)[ST_QC]) {
#pragma clang fp contract(off)        // the scaled logit is rounded before the subtraction, as postprocess_kernel compiles it
                 float cm = -INFINITY;
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) { acc[k] = acc[k] * logit_scale; cm = fmaxf(cm, acc[k]); }
                 if (cm > vmax) { sum *= expf(vmax - cm); vmax = cm; }            // the first chunk: sum = 0 * exp(-inf) = 0
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) {
                     sum += expf(acc[k] - vmax);
                     const int c = K == Q ? q0 + k : query_idx[q0 + k];
                     if (c >= 0 && c < K && (acc[k] > best || (acc[k] == best && c < best_c))) { best = acc[k]; best_c = c; }
                   }
               });
  if (!live) return;
  const int X = bx0 + (threadIdx.x & 63);
  const int Y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  const float cf = expf(best - vmax) / sum;
  const int64_t o = (int64_t)Y * OW + X;
  labels[o] = cf < prob_thd ? bg_idx : best_c;
  if (conf) conf[o] = cf;
}

__global__ __launch_bounds__(256) void label_head_resized_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                                 int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l,
                                                                 int h, int w, int OH, int OW, const int32_t* __restrict__ query_idx, int K,
                                                                 float logit_scale, float prob_thd, int bg_idx,
                                                                 int64_t* __restrict__ labels, float* __restrict__ conf, int flags) {
  label_head_resized_block(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, h, w, OH, OW, blockIdx.x * 64,
                           blockIdx.y * 4, flags, query_idx, K, logit_scale, prob_thd, bg_idx, labels, conf);
}

// The descriptors of the resized multi-image kernels: image_block over the OUTPUT sizes (out_hw, out_offset in output pixels,
// block_prefix over output blocks: every check of image_block holds against the output extents), plus the image's canvas size.
__device__ __forceinline__ bool image_block_resized(const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
                                                    const int32_t* __restrict__ out_hw, const int64_t* __restrict__ out_offset,
                                                    const int64_t* __restrict__ block_prefix, int N, int T, int64_t out_pixels,
                                                    ImageBlock& ib, int& h, int& w) {
  if (!image_block(out_hw, image_tiles, out_offset, block_prefix, N, T, 1, out_pixels, ib)) return false;
  h = image_hw[2 * ib.n]; w = image_hw[2 * ib.n + 1];
  return h > 0 && w > 0;
}

__global__ __launch_bounds__(256) void label_head_resized_multi_kernel(
    const float* __restrict__ tile_logits, const int32_t* __restrict__ windows, const int32_t* __restrict__ tile_image, int T, int Q, int gh,
    int gw, int up_h, int up_w, int pad_t, int pad_l, const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
    const int32_t* __restrict__ out_hw, const int64_t* __restrict__ out_offset, const int64_t* __restrict__ block_prefix, int N,
    int64_t out_pixels, const int32_t* __restrict__ query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
    int64_t* __restrict__ labels, float* __restrict__ conf, int flags) {
  ImageBlock ib; int h, w;
  if (!image_block_resized(image_hw, image_tiles, out_hw, out_offset, block_prefix, N, T, out_pixels, ib, h, w)) return;
  label_head_resized_block(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first, ib.n,
                           ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, h, w, ib.H, ib.W, ib.bx0, ib.by0, flags, query_idx, K,
                           logit_scale, prob_thd, bg_idx, labels + ib.off, conf ? conf + ib.off : nullptr);
}

// topk_head_block over resized_gather, the per-chunk statements copied likewise: plane 0 carries sg_label_head_resized's label and conf.
template <int KTOP>
__device__ __forceinline__ void topk_head_resized_block(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                                        const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw,
                                                        int up_h, int up_w, int pad_t, int pad_l, int h, int w, int OH, int OW, int bx0,
                                                        int by0, int flags, const int32_t* __restrict__ query_idx, int K, float logit_scale,
                                                        int k, int32_t* __restrict__ classes, float* __restrict__ probs) {
  float vmax = -INFINITY, sum = 0.f;
  float tv[KTOP];
  int tc[KTOP];
#pragma unroll
  for (int j = 0; j < KTOP; ++j) { tv[j] = -INFINITY; tc[j] = INT_MAX; }
  const bool merge = K != Q;
  const bool live = resized_gather(tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, h, w, OH, OW, bx0, by0,
                                   flags, [&](int q0, float (&acc)[ST_QC]) {
#pragma clang fp contract(off)        // the scaled logit is rounded before the subtraction, as postprocess_kernel compiles it
                 float cm = -INFINITY;
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) { acc[k] = acc[k] * logit_scale; cm = fmaxf(cm, acc[k]); }
                 if (cm > vmax) { sum *= expf(vmax - cm); vmax = cm; }            // the first chunk: sum = 0 * exp(-inf) = 0
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) {
                     sum += expf(acc[k] - vmax);
                     const float v = acc[k];
                     const int c = merge ? query_idx[q0 + k] : q0 + k;
                     if (c < 0 || c >= K) continue;
                     bool held = false;
                     if (merge) {
#pragma unroll
                       for (int j = 0; j < KTOP; ++j)
                         if (tc[j] == c) { held = true; tv[j] = fmaxf(tv[j], v); }
                     }
                     if (!held && (v > tv[KTOP - 1] || (v == tv[KTOP - 1] && c < tc[KTOP - 1]))) { tv[KTOP - 1] = v; tc[KTOP - 1] = c; }
#pragma unroll
                     for (int j = KTOP - 1; j > 0; --j) {
                       const bool up = tv[j] > tv[j - 1] || (tv[j] == tv[j - 1] && tc[j] < tc[j - 1]);
                       const float fv = tv[j]; const int fc = tc[j];
                       tv[j] = up ? tv[j - 1] : fv; tc[j] = up ? tc[j - 1] : fc;
                       tv[j - 1] = up ? fv : tv[j - 1]; tc[j - 1] = up ? fc : tc[j - 1];
                     }
                   }
               });
  if (!live) return;
  const int X = bx0 + (threadIdx.x & 63);
  const int Y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  const int64_t HW = (int64_t)OH * OW, o = (int64_t)Y * OW + X;
#pragma unroll
  for (int j = 0; j < KTOP; ++j)
    if (j < k) {
      const bool filled = tc[j] != INT_MAX;
      const float p = expf(tv[j] - vmax) / sum;
      classes[j * HW + o] = filled ? tc[j] : -1;
      probs[j * HW + o] = filled ? p : 0.f;
    }
}

template <int KTOP>
__global__ __launch_bounds__(256) void topk_head_resized_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                                int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l,
                                                                int h, int w, int OH, int OW, const int32_t* __restrict__ query_idx, int K,
                                                                float logit_scale, int k, int32_t* __restrict__ classes,
                                                                float* __restrict__ probs, int flags) {
  topk_head_resized_block<KTOP>(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, h, w, OH, OW, blockIdx.x * 64,
                                blockIdx.y * 4, flags, query_idx, K, logit_scale, k, classes, probs);
}

template <int KTOP>
__global__ __launch_bounds__(256) void topk_head_resized_multi_kernel(
    const float* __restrict__ tile_logits, const int32_t* __restrict__ windows, const int32_t* __restrict__ tile_image, int T, int Q, int gh,
    int gw, int up_h, int up_w, int pad_t, int pad_l, const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
    const int32_t* __restrict__ out_hw, const int64_t* __restrict__ out_offset, const int64_t* __restrict__ block_prefix, int N,
    int64_t out_pixels, const int32_t* __restrict__ query_idx, int K, float logit_scale, int k, int32_t* __restrict__ classes,
    float* __restrict__ probs, int flags) {
  ImageBlock ib; int h, w;
  if (!image_block_resized(image_hw, image_tiles, out_hw, out_offset, block_prefix, N, T, out_pixels, ib, h, w)) return;   // k * (off + OH * OW) <= k * out_pixels
  topk_head_resized_block<KTOP>(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first,
                                ib.n, ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, h, w, ib.H, ib.W, ib.bx0, ib.by0, flags, query_idx, K,
                                logit_scale, k, classes + k * ib.off, probs + k * ib.off);
}

// ---- test-time augmentation: the class probabilities of V views merged at the output size (sg_tta_head) ------------------------------
// One 64 x 4 block of output pixels walks the views in ascending order.  Per view resized_gather<FLIP> hands the thread its pixel's
// resized stitched values chunk by chunk (mirrored along the width for a flipped view) and the sink runs label_head_resized_block's
// online softmax in its chunk order -- the running maximum and sum are that kernel's bytes -- while the largest scaled logit of every
// class goes to s_cmax[class][thread]: the class of a query is a run-time value, so this is the one dynamically indexed array and it
// lives in LDS ((K - 1) * 1 KiB, dynamic), each thread reading and writing only its own column (no barrier guards it).  The last class
// is kept in a register instead: at K = 64 the array is then 63 KiB, and with the 16 KiB stage and the candidate list a workgroup stays
// under 80 KiB, so two fit a CU (with all 64 KiB one did, and the head took 54.1 instead of 29.9 ms on the bench's three views).  At the end of the
// view P_v[c] = expf(cmax[c] - vmax) / sum (0 for a class without a query: expf is monotone, so this is the largest probability of the
// class's queries) is added to P[c], QMAX statically indexed registers.  Then P[c] / V, the arg-max (first maximum) and the threshold.
//   With V = 1 and no flip, conf is expf(best - vmax) / sum / 1: sg_label_head_resized's bytes, and so is the label unless two classes'
//   distinct best logits round to one probability (that kernel compares logits, this one the probabilities the definition names).
//   Barriers: resized_gather's own, plus one at the end of every view -- its direct form ends without one, and the next view's candidate
//   list and stage reuse the same LDS.  No thread leaves before the last view's barrier; V and every descriptor are block-uniform.
//   No atomics, nothing proportional to Q * H * W or V * K * H * W; every output element is written by its pixel's thread in an order
//   fixed by (pixel, view, query).
constexpr int TTA_MAX_VIEWS = SG_TTA_MAX_VIEWS;
struct TtaView { int T, t0, gh, gw, up_h, up_w, pad_t, pad_l, h, w, flip; int64_t off; };   // t0: first window; off: first tile-logit element
struct TtaViews { TtaView v[TTA_MAX_VIEWS]; };

template <int QMAX>
__global__ __launch_bounds__(256) void tta_head_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                       const TtaViews views, int V, int Q, int OH, int OW,
                                                       const int32_t* __restrict__ query_idx, int K, float logit_scale, float prob_thd,
                                                       int bg_idx, int64_t* __restrict__ labels, float* __restrict__ conf,
                                                       float* __restrict__ probs, int flags) {
  extern __shared__ float s_cmax[];                                    // [K - 1][256]; class K - 1 lives in a register (clast)
  const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
  float* cm = s_cmax + threadIdx.x;
  float P[QMAX];
#pragma unroll
  for (int c = 0; c < QMAX; ++c) P[c] = 0.f;
  bool live = false;
  for (int v = 0; v < V; ++v) {
    const TtaView& d = views.v[v];
    for (int c = 0; c < K - 1; ++c) cm[c * 256] = -INFINITY;
    float vmax = -INFINITY, sum = 0.f, clast = -INFINITY;
    live = resized_gather<true>(tile_logits + d.off, windows + (int64_t)d.t0 * 4, nullptr, 0, d.T, Q, d.gh, d.gw, d.up_h, d.up_w, d.pad_t,
                                d.pad_l, d.h, d.w, OH, OW, bx0, by0, flags, [&](int q0, float (&acc)[ST_QC]) {
#pragma clang fp contract(off)        // label_head_resized_block's statements: the scaled logit is rounded before the subtraction
                 float m = -INFINITY;
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) { acc[k] = acc[k] * logit_scale; m = fmaxf(m, acc[k]); }
                 if (m > vmax) { sum *= expf(vmax - m); vmax = m; }               // the first chunk: sum = 0 * exp(-inf) = 0
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) {
                     sum += expf(acc[k] - vmax);
                     const int c = K == Q ? q0 + k : query_idx[q0 + k];
                     if (c >= 0 && c < K - 1) cm[c * 256] = fmaxf(cm[c * 256], acc[k]);
                     else if (c == K - 1) clast = fmaxf(clast, acc[k]);
                   }
               }, d.flip != 0);
    if (live) {
#pragma clang fp contract(off)
#pragma unroll
      for (int c = 0; c < QMAX; ++c)
        if (c < K) {
          const float m = c < K - 1 ? cm[c * 256] : clast;
          P[c] += m == -INFINITY ? 0.f : expf(m - vmax) / sum;
        }
    }
    __syncthreads();                                                   // the candidate list and the stage are free for the next view
  }
  if (!live) return;
  const int X = bx0 + (threadIdx.x & 63);
  const int Y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  const int64_t plane = (int64_t)OH * OW, o = (int64_t)Y * OW + X;
  const float fv = (float)V;
  float best = -INFINITY; int arg = 0;
#pragma unroll
  for (int c = 0; c < QMAX; ++c)
    if (c < K) {
      const float p = P[c] / fv;
      if (probs) probs[c * plane + o] = p;
      if (p > best) { best = p; arg = c; }                             // first maximum wins: ties go to the lower class
    }
  labels[o] = best < prob_thd ? bg_idx : arg;
  if (conf) conf[o] = best;
}

// The canvas route of the same merge (any Q, any stitch): every view's [K,OH,OW] probability planes come from the existing tail and are
// added into one accumulator, a flipped view mirrored along the width; sg_tta_finish then divides, takes the arg-max and thresholds with
// tta_head_kernel's statements.  Plain elementwise kernels.
__global__ __launch_bounds__(256) void tta_accumulate_kernel(const float* __restrict__ probs_view, int64_t rows, int OW, int flip, int first,
                                                             float* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * OW) return;
  const int64_t r = i / OW;
  const int x = (int)(i - r * OW);
  const float p = probs_view[r * OW + (flip ? OW - 1 - x : x)];
  acc[i] = first ? p : acc[i] + p;
}

__global__ __launch_bounds__(256) void tta_finish_kernel(const float* acc, int V, int K, int64_t HW, float prob_thd, int bg_idx,
                                                         int64_t* __restrict__ labels, float* __restrict__ conf, float* probs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const float fv = (float)V;
  float best = -INFINITY; int arg = 0;
  for (int c = 0; c < K; ++c) {
    const float p = acc[c * HW + i] / fv;
    if (probs) probs[c * HW + i] = p;                                  // probs may be acc itself: the element is read before it is written
    if (p > best) { best = p; arg = c; }
  }
  labels[i] = best < prob_thd ? bg_idx : arg;
  if (conf) conf[i] = best;
}

// ---- postprocess for any Q: several passes over the canvas, nothing held per query ------------------------------------------------
// Pass 1 the maximum, pass 2 the sum (postprocess_kernel's order), pass 3 the per-class maximum, written through probs[class(q)] by the
// pixel's own thread.  A class starts at what postprocess_kernel's `any_other` rule gives a class without queries: 0 when some query
// belongs to another class (the zeros of probabilities * one_hot take part in the max), -inf when every query is this class's.
// Plain and correct, not tuned: Q > PP_MAX_Q only.
__global__ __launch_bounds__(256) void postprocess_wide_kernel(const float* __restrict__ logits, const int32_t* __restrict__ query_idx,
                                                               int Q, int K, int64_t HW, float logit_scale, float prob_thd, int bg_idx,
                                                               float* probs, int64_t* __restrict__ labels) {
#pragma clang fp contract(off)          // the scaled logit is rounded before the subtraction, as postprocess_kernel compiles it
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const bool ident = K == Q;                                            // postprocess_kernel: class(q) = q, query_idx is not read
  bool all_same = true;
  const int c0 = ident ? 0 : query_idx[0];
  for (int q = 1; q < Q; ++q) all_same = all_same && (ident ? q : query_idx[q]) == c0;
  float mx = -INFINITY;
  for (int q = 0; q < Q; ++q) mx = fmaxf(mx, logits[q * HW + i] * logit_scale);
  float sum = 0.f;
  for (int q = 0; q < Q; ++q) sum += expf(logits[q * HW + i] * logit_scale - mx);
  if (probs)
    for (int c = 0; c < K; ++c) probs[c * HW + i] = (all_same && c == c0) ? -INFINITY : 0.f;
  float best = -INFINITY; int arg = 0;
  for (int q = 0; q < Q; ++q) {
    const int c = ident ? q : query_idx[q];
    if (c < 0 || c >= K) continue;
    const float p = expf(logits[q * HW + i] * logit_scale - mx) / sum;
    if (probs) { float* d = probs + c * HW + i; *d = fmaxf(*d, p); }
    if (p > best || (p == best && c < arg)) { best = p; arg = c; }        // the first maximum over classes wins (torch argmax)
  }
  if (best < prob_thd) arg = bg_idx;
  labels[i] = arg;
}

// ---- fused probability head: stitch -> class probabilities + labels, no canvas, any Q -------------------------------------------------
// One 64 x 4 pixel block of one image, shared by the single-image and the multi-image kernel.  stitch_gather supplies the stitched
// values (sg_stitch's by construction) and the tail is the canvas route's own, so probs and labels carry the bytes of sg_stitch +
// sg_postprocess (QMAX = 16 / PP_MAX_Q, the instantiations sg_postprocess dispatches on) or + sg_postprocess_wide (QMAX = 0, Q > PP_MAX_Q).
// The image's labels [H,W] start at pixel ooff of the flat outputs and its probs [K,H,W] at K * ooff.
//   QMAX > 0: one gather.  The chunk loop is unrolled, so the Q stitched values of the pixel sit in statically indexed registers, and
//   class_tail<QMAX> runs on them with load(q) = the register (made opaque like a loaded value, as in postprocess_multi_kernel).
//   QMAX = 0: postprocess_wide_kernel's three passes with logits[q * HW + i] replaced by the stitched value, i.e. three gathers over
//   one candidate list and nothing held per query.  The tile logits are L2 / MALL resident at these sizes; the gathers are the cost
//   (label_head_block's comment), and this form pays them three times to keep that kernel's summation order: the byte identity.
// No atomics, no buffer proportional to Q * H * W, no LDS beyond the candidate list; every output element is written by its pixel's
// own thread in an order fixed by (pixel, query index), so repeats are byte-identical.
template <int QMAX>
__device__ __forceinline__ void prob_head_block(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                                const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw,
                                                int up_h, int up_w, int pad_t, int pad_l, int H, int W, int bx0, int by0,
                                                const int32_t* __restrict__ query_idx, int K, float logit_scale, float prob_thd,
                                                int bg_idx, float* probs, int64_t* __restrict__ labels, int64_t ooff) {
  const StitchList sl = stitch_candidates(win, tile_image, img, n_tiles, bx0, by0);
  const int x = bx0 + (threadIdx.x & 63);
  const int y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  const bool live = y < H && x < W;
  const int64_t HW = (int64_t)H * W, i = (int64_t)y * W + x;
  if constexpr (QMAX > 0) {
    float v[QMAX];
#pragma unroll
    for (int q = 0; q < QMAX; ++q) v[q] = 0.f;
    stitch_gather<QMAX / ST_QC>(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0,
                                [&](int, int, int q0, const float (&acc)[ST_QC], float cnt) __attribute__((always_inline)) {
#pragma unroll
                                  for (int k = 0; k < ST_QC; ++k)
                                    if (q0 + k < Q) v[q0 + k] = cnt > 0.f ? acc[k] / cnt : 0.f;      // q0 is a constant here
                                });
    if (!live) return;
    class_tail<QMAX>([&](int q) { float l = v[q]; asm volatile("" : "+v"(l)); return l; }, query_idx, Q, K, logit_scale, prob_thd, bg_idx,
                     probs, labels, ooff, HW, i);
  } else {
    const bool ident = K == Q;                                            // postprocess_wide_kernel: class(q) = q, query_idx is not read
    bool all_same = true;
    const int c0 = ident ? 0 : query_idx[0];
    for (int q = 1; q < Q; ++q) all_same = all_same && (ident ? q : query_idx[q]) == c0;
    float mx = -INFINITY;
    stitch_gather(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0,
                  [&](int, int, int q0, const float (&acc)[ST_QC], float cnt) {
#pragma clang fp contract(off)        // the scaled logit is rounded before the subtraction, as postprocess_wide_kernel has it
#pragma unroll
                    for (int k = 0; k < ST_QC; ++k)
                      if (q0 + k < Q) mx = fmaxf(mx, (cnt > 0.f ? acc[k] / cnt : 0.f) * logit_scale);
                  });
    float sum = 0.f;
    stitch_gather(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0,
                  [&](int, int, int q0, const float (&acc)[ST_QC], float cnt) {
#pragma clang fp contract(off)
#pragma unroll
                    for (int k = 0; k < ST_QC; ++k)                       // q ascending
                      if (q0 + k < Q) sum += expf((cnt > 0.f ? acc[k] / cnt : 0.f) * logit_scale - mx);
                  });
    float* pr = probs + K * ooff;
    if (live)
      for (int c = 0; c < K; ++c) pr[c * HW + i] = (all_same && c == c0) ? -INFINITY : 0.f;
    float best = -INFINITY; int arg = 0;
    stitch_gather(sl, tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0,
                  [&](int, int, int q0, const float (&acc)[ST_QC], float cnt) {
#pragma clang fp contract(off)
                    if (!live) return;
#pragma unroll
                    for (int k = 0; k < ST_QC; ++k) {
                      if (q0 + k >= Q) continue;
                      const int c = ident ? q0 + k : query_idx[q0 + k];
                      if (c < 0 || c >= K) continue;
                      const float p = expf((cnt > 0.f ? acc[k] / cnt : 0.f) * logit_scale - mx) / sum;
                      float* d = pr + c * HW + i;
                      *d = fmaxf(*d, p);
                      if (p > best || (p == best && c < arg)) { best = p; arg = c; }   // the first maximum over classes wins (torch argmax)
                    }
                  });
    if (!live) return;
    if (best < prob_thd) arg = bg_idx;
    labels[ooff + i] = arg;
  }
}

// QMAX = PP_MAX_Q is held to at least four waves per SIMD (128 registers): the gathers want waves to hide behind.  With the output
// offset a literal 0 the single-image kernel folded it into the pointers and took 191 registers (class_tail's comment: the same effect),
// and spilled under the bound; with the offset opaque both kernels take 93 and no scratch.
template <int QMAX>
__global__ __launch_bounds__(256, QMAX > 16 ? 4 : 1) void prob_head_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows, int T,
                                                        int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l, int H, int W,
                                                        const int32_t* __restrict__ query_idx, int K, float logit_scale, float prob_thd,
                                                        int bg_idx, float* probs, int64_t* __restrict__ labels) {
  int64_t ooff = 0;
  asm volatile("" : "+s"(ooff));      // not a constant to the compiler: it then addresses the outputs as the multi-image kernel does
  prob_head_block<QMAX>(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, blockIdx.x * 64, blockIdx.y * 4,
                        query_idx, K, logit_scale, prob_thd, bg_idx, probs, labels, ooff);
}

// The tiles of N images (sg_stitch_multi's descriptors); labels of image n at out_offset[n] pixels of the flat outputs, its probs at
// K * out_offset[n] (sg_postprocess_multi's layout).
template <int QMAX>
__global__ __launch_bounds__(256, QMAX > 16 ? 4 : 1) void prob_head_multi_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                              const int32_t* __restrict__ tile_image, int T, int Q, int gh, int gw,
                                                              int up_h, int up_w, int pad_t, int pad_l,
                                                              const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
                                                              const int64_t* __restrict__ out_offset, const int64_t* __restrict__ block_prefix,
                                                              int N, int64_t out_pixels, const int32_t* __restrict__ query_idx, int K,
                                                              float logit_scale, float prob_thd, int bg_idx, float* probs,
                                                              int64_t* __restrict__ labels) {
  ImageBlock ib;
  if (!image_block(image_hw, image_tiles, out_offset, block_prefix, N, T, 1, out_pixels, ib)) return;   // K * (off + H * W) <= K * out_pixels
  prob_head_block<QMAX>(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first, ib.n,
                        ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, ib.H, ib.W, ib.bx0, ib.by0, query_idx, K, logit_scale, prob_thd,
                        bg_idx, probs, labels, ib.off);
}

// ---- area_thd on the labels-only route: the second decision after sg_label_head, no canvas and no probability planes -----------------
// labels [H,W] hold the first-pass labels l0 (sg_label_head with prob_thd = 0), conf its conf, keep [K] the classes that survive
// (sg_area_keep).  A 64 x 4 block in which every first label is kept gathers nothing: l0 is still the best kept class and conf its
// probability, so the block writes conf < prob_thd ? bg_idx : l0.  A block that holds a dropped label repeats label_head_block for all
// its pixels with the best pair restricted to kept classes: the per-chunk statements (scaled logit, chunk maximum, rescale of the sum,
// sum of exp) are that function's, copied -- label_head_block itself is not touched, its machine code stays what it is -- so the block's
// output is sg_label_head's on a query_idx whose dropped queries are -1.  Dropped classes still take part in the softmax sum.
// The vote is one __syncthreads_or per block; which path a block takes depends on its own pixels alone: repeats are byte-identical.
__device__ __forceinline__ void area_relabel_block(const float* __restrict__ tile_logits, const int32_t* __restrict__ win,
                                                   const int32_t* __restrict__ tile_image, int img, int n_tiles, int Q, int gh, int gw,
                                                   int up_h, int up_w, int pad_t, int pad_l, int H, int W, int bx0, int by0,
                                                   const int32_t* __restrict__ query_idx, int K, float logit_scale, float prob_thd,
                                                   int bg_idx, const int32_t* __restrict__ keep, const float* __restrict__ conf,
                                                   int64_t* __restrict__ labels) {
  const int x = bx0 + (threadIdx.x & 63);
  const int y = __builtin_amdgcn_readfirstlane(by0 + (threadIdx.x >> 6));
  const bool inside = y < H && x < W;
  const int64_t o = (int64_t)y * W + x;
  int64_t l0 = 0;
  float cf0 = 0.f;
  bool dropped = false;
  if (inside) {
    l0 = labels[o];
    cf0 = conf[o];
    dropped = !((uint64_t)l0 < (uint64_t)K && keep[l0] != 0);
  }
  if (!__syncthreads_or(dropped)) {                                        // block-uniform
    if (inside) labels[o] = cf0 < prob_thd ? bg_idx : l0;
    return;
  }
  float vmax = -INFINITY, sum = 0.f, best = -INFINITY;
  int best_c = 0;
  stitch_block(tile_logits, win, tile_image, img, n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, bx0, by0,
               [&](int, int, int q0, float (&acc)[ST_QC], float cnt) {
#pragma clang fp contract(off)        // the scaled logit is rounded before the subtraction, as postprocess_kernel compiles it
                 float cm = -INFINITY;
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) { acc[k] = (cnt > 0.f ? acc[k] / cnt : 0.f) * logit_scale; cm = fmaxf(cm, acc[k]); }
                 if (cm > vmax) { sum *= expf(vmax - cm); vmax = cm; }            // the first chunk: sum = 0 * exp(-inf) = 0
#pragma unroll
                 for (int k = 0; k < ST_QC; ++k)
                   if (q0 + k < Q) {
                     sum += expf(acc[k] - vmax);
                     const int c = K == Q ? q0 + k : query_idx[q0 + k];
                     if (c >= 0 && c < K && keep[c] != 0 && (acc[k] > best || (acc[k] == best && c < best_c))) { best = acc[k]; best_c = c; }
                   }
               });
  if (!inside) return;
  const float cf = expf(best - vmax) / sum;
  labels[o] = cf < prob_thd ? bg_idx : best_c;
}

__global__ __launch_bounds__(256) void area_relabel_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                           int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l, int H,
                                                           int W, const int32_t* __restrict__ query_idx, int K, float logit_scale,
                                                           float prob_thd, int bg_idx, const int32_t* __restrict__ keep,
                                                           const float* __restrict__ conf, int64_t* __restrict__ labels) {
  area_relabel_block(tile_logits, windows, nullptr, 0, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, blockIdx.x * 64, blockIdx.y * 4,
                     query_idx, K, logit_scale, prob_thd, bg_idx, keep, conf, labels);
}

// The tiles of N images (sg_label_head_multi's descriptors); keep [N,K], conf and labels of image n at out_offset[n] pixels.
__global__ __launch_bounds__(256) void area_relabel_multi_kernel(const float* __restrict__ tile_logits, const int32_t* __restrict__ windows,
                                                                 const int32_t* __restrict__ tile_image, int T, int Q, int gh, int gw,
                                                                 int up_h, int up_w, int pad_t, int pad_l,
                                                                 const int32_t* __restrict__ image_hw, const int32_t* __restrict__ image_tiles,
                                                                 const int64_t* __restrict__ out_offset, const int64_t* __restrict__ block_prefix,
                                                                 int N, int64_t out_pixels, const int32_t* __restrict__ query_idx, int K,
                                                                 float logit_scale, float prob_thd, int bg_idx,
                                                                 const int32_t* __restrict__ keep, const float* __restrict__ conf,
                                                                 int64_t* __restrict__ labels) {
  ImageBlock ib;
  if (!image_block(image_hw, image_tiles, out_offset, block_prefix, N, T, 1, out_pixels, ib)) return;
  area_relabel_block(tile_logits + (int64_t)ib.t_first * Q * gh * gw, windows + (int64_t)ib.t_first * 4, tile_image + ib.t_first, ib.n,
                     ib.n_tiles, Q, gh, gw, up_h, up_w, pad_t, pad_l, ib.H, ib.W, ib.bx0, ib.by0, query_idx, K, logit_scale, prob_thd, bg_idx,
                     keep + (int64_t)ib.n * K, conf + ib.off, labels + ib.off);
}

// ---- label / confidence images (segmentor.py:501-531, 580-608) ---------------------------------------------------------
// mask  = palette[clip(label, 0, K-1)]                                (_colorize_mask)
// heat  = (g, 0, 255 - g), g = uint8(clip(nan_to_num(max_k probs), 0, 1) * 255)   (_to_colormap, the branch without OpenCV)
__global__ __launch_bounds__(256) void render_maps_kernel(const int64_t* __restrict__ labels, const float* __restrict__ probs,
                                                          const uint8_t* __restrict__ palette, int K, int64_t HW,
                                                          uint8_t* __restrict__ mask_rgb, uint8_t* __restrict__ heat_rgb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  if (mask_rgb) {
    int64_t l = labels[i];
    l = l < 0 ? 0 : (l > K - 1 ? K - 1 : l);
    mask_rgb[3 * i + 0] = palette[3 * l + 0]; mask_rgb[3 * i + 1] = palette[3 * l + 1]; mask_rgb[3 * i + 2] = palette[3 * l + 2];
  }
  if (heat_rgb) {
    float c = -INFINITY;
    for (int k = 0; k < K; ++k) { const float v = probs[(int64_t)k * HW + i]; c = (v > c || v != v) ? v : c; }   // torch.max propagates NaN
    if (c != c) c = 0.f;
    c = fminf(fmaxf(c, 0.f), 1.f);
    const uint8_t g = (uint8_t)(c * 255.0f);
    heat_rgb[3 * i + 0] = g; heat_rgb[3 * i + 1] = 0; heat_rgb[3 * i + 2] = (uint8_t)(255 - g);
  }
}

}  // namespace sg

using namespace sg;

extern "C" int sg_render_maps(const int64_t* labels, const float* probs, const uint8_t* palette, int K, int H, int W, uint8_t* mask_rgb,
                              uint8_t* heat_rgb, sg_stream s) {
  SG_REQUIRE(K > 0 && H > 0 && W > 0, "sg_render_maps: bad shape");
  SG_REQUIRE(!mask_rgb || (labels && palette), "sg_render_maps: the mask needs labels and a palette");
  SG_REQUIRE(!heat_rgb || probs, "sg_render_maps: the heat map needs the class probabilities");
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(render_maps_kernel, dim3((unsigned)cdiv(HW, 256)), dim3(256), 0, as_stream(s), labels, probs, palette, K, HW, mask_rgb, heat_rgb);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

namespace sg {
// Large-n form without the global debias (per-pixel logits behind the upsampler): logits = (x / |x|) . T^T is a [n, E] x [E, 16] GEMM.
// f32-grade on the f16 matrix pipe: T as two f16 planes in LDS, the f32 rows split into hi + lo on the fly, three v_mfma_f32_16x16x32_f16
// per product into one f32 accumulator (the same scheme as SG_PREC_F16X2's GEMMs), |x|^2 in f32 from the loaded values.  A wave owns 64
// consecutive pixels per round; a lane ends with 4 consecutive pixels of one query.  Bound by the read of x (the lane-per-token kernel
// above runs this shape at 1.5 TB/s on the vector pipe: 5.9 ms per 8 tiles of 592 x 592 at E = 768).
constexpr int CLM_ROUNDS = 4;
__global__ __launch_bounds__(256, 2) void cosine_logits_mfma_kernel(const float* __restrict__ tokens, const float* __restrict__ cls,
                                                                    const float* __restrict__ text, int n, int E, int Q, float lambda,
                                                                    float* __restrict__ logits) {
  extern __shared__ __attribute__((aligned(16))) char clm_sm[];
  const int ldt = E + 8;
  uint16_t* sTh = reinterpret_cast<uint16_t*>(clm_sm);                   // [16][E + 8] f16
  uint16_t* sTl = sTh + 16 * ldt;
  float* sN = reinterpret_cast<float*>(sTl + 16 * ldt);                   // [4 waves][64]
  float* sCL = sN + 4 * 64;                                               // [16] lambda * cls logits of this image
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 16 * E; i += 256) {
    const int q = i / E, c = i % E;
    const float v = q < Q ? text[(int64_t)q * E + c] : 0.f;
    const f16_t hi = f2h(v);
    sTh[q * ldt + c] = hi.bits;
    sTl[q * ldt + c] = f2h(v - h2f(hi)).bits;
  }
  if (tid < 16) sCL[tid] = 0.f;
  __syncthreads();
  if (cls != nullptr && lambda != 0.f) {                                   // lambda * (cls / |cls|) . T[q]   (segmentor.py:310-311, 379), f32
    const float* cr = cls + (int64_t)b * E;
    float ss = 0.f;
    for (int i = lane; i < E; i += 64) ss += cr[i] * cr[i];
    const float inv = 1.0f / sqrtf(wave_sum(ss));
    for (int q = wave; q < Q; q += 4) {
      float d = 0.f;
      for (int i = lane; i < E; i += 64) d += cr[i] * text[(int64_t)q * E + i];
      d = wave_sum(d);
      if (lane == 0) sCL[q] = lambda * d * inv;
    }
    __syncthreads();
  }
  const int r = lane & 15, g = lane >> 4;
  float* myN = sN + wave * 64;
  const float* xb = tokens + (int64_t)b * n * E;
  float* lb = logits + (int64_t)b * Q * n;
  for (int round = 0; round < CLM_ROUNDS; ++round) {
    const int pix0 = ((blockIdx.x * CLM_ROUNDS + round) * 4 + wave) * 64;
    if (pix0 >= n) return;                                                // wave-uniform; no workgroup barrier below
    const float* xr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      int pr = pix0 + t * 16 + r;
      pr = pr < n ? pr : n - 1;
      xr[t] = xb + (int64_t)pr * E + 8 * g;
    }
    f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float nx[4] = {0.f, 0.f, 0.f, 0.f};
    float4 cur[4][2], nxt[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) { cur[t][0] = *reinterpret_cast<const float4*>(xr[t]); cur[t][1] = *reinterpret_cast<const float4*>(xr[t] + 4); }
    const int nk = E / 32;
    for (int ks = 0; ks < nk; ++ks) {
      const int kn = ks + 1 < nk ? ks + 1 : ks;
#pragma unroll
      for (int t = 0; t < 4; ++t) { nxt[t][0] = *reinterpret_cast<const float4*>(xr[t] + 32 * kn); nxt[t][1] = *reinterpret_cast<const float4*>(xr[t] + 32 * kn + 4); }
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(sTh + r * ldt + 32 * ks + 8 * g);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(sTl + r * ldt + 32 * ks + 8 * g);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float v[8] = {cur[t][0].x, cur[t][0].y, cur[t][0].z, cur[t][0].w, cur[t][1].x, cur[t][1].y, cur[t][1].z, cur[t][1].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) nx[t] = __builtin_fmaf(v[e], v[e], nx[t]);
        uint4 hi, lo;
        split_h2x8(v, hi, lo);
        const bf16x8 ah = __builtin_bit_cast(bf16x8, hi), al = __builtin_bit_cast(bf16x8, lo);
        acc[t] = mfma_16x16x32<true>(ah, bh, acc[t]);                      // D[pixel i][query j]: lane = j + 16 (i / 4), 4 consecutive pixels
        acc[t] = mfma_16x16x32<true>(al, bh, acc[t]);
        acc[t] = mfma_16x16x32<true>(ah, bl, acc[t]);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) { cur[t][0] = nxt[t][0]; cur[t][1] = nxt[t][1]; }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) { nx[t] += __shfl_xor(nx[t], 16, 64); nx[t] += __shfl_xor(nx[t], 32, 64); }
    if (g == 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t) myN[t * 16 + r] = 1.0f / fmaxf(sqrtf(nx[t]), 1e-12f);   // F.normalize's eps
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (r < Q) {
      const float cl = sCL[r];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int pix = pix0 + t * 16 + 4 * g;
        if (pix >= n) continue;
        const float4 inv = *reinterpret_cast<const float4*>(myN + t * 16 + 4 * g);
        const float o[4] = {acc[t][0] * inv.x + cl, acc[t][1] * inv.y + cl, acc[t][2] * inv.z + cl, acc[t][3] * inv.w + cl};
        float* dst = lb + (int64_t)r * n + pix;
        if (pix + 3 < n && (n & 3) == 0) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        else {
          for (int e = 0; e < 4; ++e) if (pix + e < n) dst[e] = o[e];
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}
}  // namespace sg

extern "C" int sg_cosine_logits(const float* tokens, const float* cls, const float* text, int B, int n, int E, int Q,
                                float global_debias_factor, float cls_token_lambda, float* logits, sg_stream s) {
  SG_REQUIRE(tokens && text && logits, "sg_cosine_logits: null pointer");
  SG_REQUIRE(B > 0 && n > 0 && E > 0 && Q > 0 && B < 65536, "sg_cosine_logits: bad shape B=%d n=%d E=%d Q=%d", B, n, E, Q);
  SG_REQUIRE(cls || (global_debias_factor == 0.f && cls_token_lambda == 0.f), "sg_cosine_logits: cls required for debias / lambda");
  const size_t lds = ((size_t)Q * E + E + Q) * sizeof(float);
  SG_REQUIRE(lds <= 160 * 1024, "sg_cosine_logits: Q*E=%d exceeds LDS", Q * E);
  SG_REQUIRE(E <= 64 * CL_MAXV && E % 4 == 0, "sg_cosine_logits: E=%d must be a multiple of 4 and <= %d", E, 64 * CL_MAXV);
  SG_REQUIRE((((uintptr_t)tokens) & 15) == 0, "sg_cosine_logits: tokens must be 16-byte aligned");
  const int nv = (E + 63) / 64;
  auto kern = nv <= 8 ? cosine_logits_kernel<8> : (nv <= 12 ? cosine_logits_kernel<12> : (nv <= 16 ? cosine_logits_kernel<16> : cosine_logits_kernel<CL_MAXV>));
  if (lds > 48 * 1024) SG_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(n, CL_TPB), (unsigned)B), dim3(256), lds, as_stream(s), tokens, cls, text,
                     n, E, Q, global_debias_factor, cls_token_lambda, logits);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

// The per-pixel logits of the EXACT tower mode (SG_PREC_F16X2): the same contract as sg_cosine_logits without the global debias, on the f16 matrix
// pipe with every operand as two f16 planes (f32-grade; like everything in that mode, magnitudes beyond +-131 008 saturate -- sg_cosine_logits
// itself stays plain f32 arithmetic with no such bound).  Shapes the matrix-pipe form does not take (Q > 16, E % 32 != 0, small n) go to sg_cosine_logits.
extern "C" int sg_cosine_logits_two_plane(const float* tokens, const float* cls, const float* text, int B, int n, int E, int Q,
                                          float cls_token_lambda, float* logits, sg_stream s) {
  SG_REQUIRE(tokens && text && logits, "sg_cosine_logits_two_plane: null pointer");
  SG_REQUIRE(B > 0 && n > 0 && E > 0 && Q > 0 && B < 65536, "sg_cosine_logits_two_plane: bad shape B=%d n=%d E=%d Q=%d", B, n, E, Q);
  SG_REQUIRE(cls || cls_token_lambda == 0.f, "sg_cosine_logits_two_plane: cls required for lambda");
  const size_t ldsm = (size_t)2 * 16 * (E + 8) * 2 + (4 * 64 + 16) * sizeof(float);
  if (!(Q <= 16 && E % 32 == 0 && n >= 4096 && (((uintptr_t)logits) & 15) == 0 && (((uintptr_t)tokens) & 15) == 0 && ldsm <= 160 * 1024))
    return sg_cosine_logits(tokens, cls, text, B, n, E, Q, 0.f, cls_token_lambda, logits, s);
  if (ldsm > 48 * 1024) SG_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(sg::cosine_logits_mfma_kernel), ldsm));
  hipLaunchKernelGGL(sg::cosine_logits_mfma_kernel, dim3((unsigned)cdiv(n, 4 * 64 * sg::CLM_ROUNDS), (unsigned)B), dim3(256), ldsm, as_stream(s), tokens, cls, text,
                     n, E, Q, cls_token_lambda, logits);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

// ---- what the head entries share on the host -----------------------------------------------------------------------------------------------
// The entries sg_stitch .. sg_area_relabel_multi (and sg_tta_head for K, bg_idx and the flags) state each argument check and each launch
// shape once, here.  A check takes the entry's name and says "<entry>: ..."; an entry is its own null-pointer line, these checks under
// SG_TRY in the order its refusals fire, the kernel choice and one of the two launches.  A new head entry composes them the same way.
// The checks of K, k and bg_idx come between the shape and the launch limit (rows, blocks), which is why those two are apart.
static bool head_tiles_ok(int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l) {
  return T > 0 && Q > 0 && gh > 0 && gw > 0 && up_h > 0 && up_w > 0 && pad_t >= 0 && pad_l >= 0;
}
static int head_check_rows(const char* who, const char* what, int rows) {       // blockIdx.y counts rows of 4
  SG_REQUIRE(cdiv(rows, 4) < 65536, "%s: %s too tall for one launch", who, what);
  return SG_OK;
}
static int head_check_stitch(const char* who, int T, int Q, int gh, int gw, int H, int W) {   // bare, and up_h .. pad_l go untested
  SG_REQUIRE(T > 0 && Q > 0 && gh > 0 && gw > 0 && H > 0 && W > 0, "%s: bad shape", who);
  return head_check_rows(who, "canvas", H);
}
static int head_check_image(const char* who, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l, int H, int W) {
  SG_REQUIRE(head_tiles_ok(T, Q, gh, gw, up_h, up_w, pad_t, pad_l) && H > 0 && W > 0, "%s: bad shape T=%d Q=%d gh=%d gw=%d up=%dx%d H=%d W=%d",
             who, T, Q, gh, gw, up_h, up_w, H, W);
  return SG_OK;
}
static int head_check_resized_image(const char* who, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l, int H, int W,
                                    int out_h, int out_w) {
  SG_REQUIRE(head_tiles_ok(T, Q, gh, gw, up_h, up_w, pad_t, pad_l) && H > 0 && W > 0 && out_h > 0 && out_w > 0,
             "%s: bad shape T=%d Q=%d gh=%d gw=%d up=%dx%d H=%d W=%d out=%dx%d", who, T, Q, gh, gw, up_h, up_w, H, W, out_h, out_w);
  return SG_OK;
}
static int head_check_images(const char* who, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t, int pad_l, int N) {
  SG_REQUIRE(head_tiles_ok(T, Q, gh, gw, up_h, up_w, pad_t, pad_l) && N > 0 && N <= T, "%s: bad shape T=%d Q=%d gh=%d gw=%d N=%d", who, T, Q,
             gh, gw, N);
  return SG_OK;
}
// canvas_Q = 0: `size` is out_pixels; the stitch entries pass Q, and `size` is canvas_elems
static int head_check_blocks(const char* who, int64_t total_blocks, int64_t size, int canvas_Q = 0) {
  SG_REQUIRE(total_blocks > 0 && total_blocks <= INT32_MAX, "%s: total_blocks=%lld outside (0, 2^31)", who, (long long)total_blocks);
  if (canvas_Q) SG_REQUIRE(size >= canvas_Q, "%s: canvas_elems=%lld holds no canvas", who, (long long)size);
  else SG_REQUIRE(size > 0, "%s: out_pixels=%lld holds no image", who, (long long)size);
  return SG_OK;
}
static int head_check_K(const char* who, int K, int Q) { SG_REQUIRE(K > 0 && K <= Q, "%s: K=%d must lie in [1, Q=%d]", who, K, Q); return SG_OK; }
static int head_check_topk(const char* who, int k, int K) {
  SG_REQUIRE(k >= 1 && k <= SG_TOPK_MAX && k <= K, "%s: k=%d must lie in [1, min(%d, K=%d)]", who, k, SG_TOPK_MAX, K);
  return SG_OK;
}
static int head_check_area_K(const char* who, int K) {
  SG_REQUIRE(K <= SG_AREA_MAX_K, "%s: K=%d exceeds %d (SG_AREA_MAX_K, the limit of sg_class_area)", who, K, SG_AREA_MAX_K);
  return SG_OK;
}
static int head_check_bg(const char* who, int bg, int K) { SG_REQUIRE(bg >= 0 && bg < K, "%s: bg_idx=%d outside [0, K=%d)", who, bg, K); return SG_OK; }
// The kernels index the table with min(d, ramp_len - 1) and d >= 0, so a table of ramp_len entries is all they read.
static int head_check_ramp(const char* who, const float* ramp, int ramp_len) {
  SG_REQUIRE(ramp, "%s: null ramp", who);
  SG_REQUIRE(ramp_len >= 1 && ramp_len <= SG_BLEND_MAX_RAMP, "%s: ramp_len=%d outside [1, %d]", who, ramp_len, SG_BLEND_MAX_RAMP);
  return SG_OK;
}
static int head_check_flags(const char* who, int flags) {
  SG_REQUIRE(flags == SG_RESIZED_AUTO || flags == SG_RESIZED_DIRECT || flags == SG_RESIZED_STAGED, "%s: flags=%d is no SG_RESIZED_* value", who,
             flags);
  return SG_OK;
}
// SG_RESIZED_STAGED is refused where the footprint of a block does not fit the stage; the multi-image entries cannot see the sizes (they
// are device arrays), so there a block whose image does not fit runs the direct form and the caller checks beforehand (ops.py does).
static int head_check_staged_fit(const char* who, int flags, int H, int W, int out_h, int out_w) {
  SG_REQUIRE(flags != SG_RESIZED_STAGED || rs_fits(H, W, out_h, out_w),
             "%s: the staged form does not fit: a block's footprint of %lld x %lld canvas pixels exceeds the stage of %d", who,
             (long long)rs_span(4, H, out_h), (long long)rs_span(64, W, out_w), RS_STAGE_PIX);
  return SG_OK;
}

// The two launch shapes: one block per 64 x 4 pixels of a [H, W] image, and the blocks of all images counted up front.
template <class Kernel, class... Args>
static int head_launch_image(Kernel kernel, int H, int W, sg_stream s, Args... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(W, 64), (unsigned)cdiv(H, 4)), dim3(256), 0, as_stream(s), args...);
  SG_LAUNCH_CHECK();
  return SG_OK;
}
template <class Kernel, class... Args>
static int head_launch_blocks(Kernel kernel, int64_t total_blocks, sg_stream s, Args... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(s), args...);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_stitch(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w,
                         int pad_t, int pad_l, int H, int W, float* canvas, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && canvas, "sg_stitch: null pointer");
  SG_TRY(head_check_stitch(__func__, T, Q, gh, gw, H, W));
  return head_launch_image(stitch_kernel, H, W, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, canvas);
}

extern "C" int sg_resize_bilinear(const float* src, int C, int h, int w, float* dst, int H, int W, sg_stream s) {
  SG_REQUIRE(src && dst && C > 0 && h > 0 && w > 0 && H > 0 && W > 0, "sg_resize_bilinear: bad arguments");
  SG_REQUIRE(cdiv(H, 4) < 65536, "sg_resize_bilinear: too tall");
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)cdiv(W, 64), (unsigned)cdiv(H, 4)), dim3(256), 0, as_stream(s), src, C, h, w, dst, H, W);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_postprocess(const float* logits, const int32_t* query_idx, int Q, int K, int H, int W, float logit_scale,
                              float prob_thd, int bg_idx, float* probs, int64_t* labels, sg_stream s) {
  SG_REQUIRE(logits && query_idx && labels, "sg_postprocess: null pointer");
  SG_REQUIRE(Q > 0 && Q <= PP_MAX_Q && K > 0 && K <= Q, "sg_postprocess: Q=%d K=%d unsupported (Q <= %d)", Q, K, PP_MAX_Q);
  const int64_t HW = (int64_t)H * W;
  if (Q <= 16)
    hipLaunchKernelGGL(postprocess_kernel<16>, dim3((unsigned)cdiv(HW, 256)), dim3(256), 0, as_stream(s), logits, query_idx, Q, K, HW,
                       logit_scale, prob_thd, bg_idx, probs, labels);
  else
    hipLaunchKernelGGL(postprocess_kernel<PP_MAX_Q>, dim3((unsigned)cdiv(HW, 256)), dim3(256), 0, as_stream(s), logits, query_idx, Q, K, HW,
                       logit_scale, prob_thd, bg_idx, probs, labels);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_stitch_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                               int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                               const int64_t* canvas_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t canvas_elems,
                               float* canvases, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && canvas_offset && block_prefix && canvases,
             "sg_stitch_multi: null pointer");
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_blocks(__func__, total_blocks, canvas_elems, Q));
  return head_launch_blocks(stitch_multi_kernel, total_blocks, s, tile_logits, windows, tile_image, T, Q, gh, gw, up_h, up_w, pad_t, pad_l,
                            image_hw, image_tiles, canvas_offset, block_prefix, N, canvas_elems, canvases);
}

extern "C" int sg_postprocess_multi(const float* canvases, const int32_t* canvas_hw, const int64_t* canvas_offset, const int32_t* out_hw,
                                    const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t canvas_elems,
                                    int64_t out_pixels, const int32_t* query_idx, int Q, int K, float logit_scale, float prob_thd, int bg_idx,
                                    float* probs, int64_t* labels, sg_stream s) {
  SG_REQUIRE(canvases && canvas_hw && canvas_offset && out_hw && out_offset && block_prefix && query_idx && labels,
             "sg_postprocess_multi: null pointer");
  SG_REQUIRE(N > 0 && Q > 0 && Q <= PP_MAX_Q && K > 0 && K <= Q, "sg_postprocess_multi: N=%d Q=%d K=%d unsupported (Q <= %d)", N, Q, K, PP_MAX_Q);
  SG_REQUIRE(total_blocks > 0 && total_blocks <= INT32_MAX, "sg_postprocess_multi: total_blocks=%lld outside (0, 2^31)", (long long)total_blocks);
  SG_REQUIRE(canvas_elems >= Q && out_pixels > 0, "sg_postprocess_multi: canvas_elems=%lld out_pixels=%lld", (long long)canvas_elems,
             (long long)out_pixels);
  auto kern = Q <= 16 ? postprocess_multi_kernel<16> : postprocess_multi_kernel<PP_MAX_Q>;
  hipLaunchKernelGGL(kern, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(s), canvases, canvas_hw, canvas_offset, out_hw, out_offset,
                     block_prefix, N, canvas_elems, out_pixels, query_idx, Q, K, logit_scale, prob_thd, bg_idx, probs, labels);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

// sg_cosine_logits for any Q.  A text matrix that fits in LDS whole is one chunk: that is cosine_logits_kernel itself (32 tokens per
// staging instead of 16, and the same bits as sg_cosine_logits by construction).  Beyond it the rows go through LDS in chunks inside one
// launch of cosine_logits_wide_kernel.
extern "C" int sg_cosine_logits_wide(const float* tokens, const float* cls, const float* text, int B, int n, int E, int Q,
                                     float global_debias_factor, float cls_token_lambda, float* logits, sg_stream s) {
  SG_REQUIRE(tokens && text && logits, "sg_cosine_logits_wide: null pointer");
  SG_REQUIRE(B > 0 && n > 0 && E > 0 && Q > 0 && B < 65536, "sg_cosine_logits_wide: bad shape B=%d n=%d E=%d Q=%d", B, n, E, Q);
  SG_REQUIRE(cls || (global_debias_factor == 0.f && cls_token_lambda == 0.f), "sg_cosine_logits_wide: cls required for debias / lambda");
  SG_REQUIRE(E <= 64 * CL_MAXV && E % 4 == 0, "sg_cosine_logits_wide: E=%d must be a multiple of 4 and <= %d", E, 64 * CL_MAXV);
  SG_REQUIRE((((uintptr_t)tokens) & 15) == 0, "sg_cosine_logits_wide: tokens must be 16-byte aligned");
  SG_REQUIRE((int64_t)Q * n <= INT64_MAX / B, "sg_cosine_logits_wide: output too large");
  if (((size_t)Q * E + E + Q) * sizeof(float) <= 160 * 1024)
    return sg_cosine_logits(tokens, cls, text, B, n, E, Q, global_debias_factor, cls_token_lambda, logits, s);
  const int fit = (160 * 1024 / (int)sizeof(float) - E) / (E + 1);           // rows R with (R * E + E + R) * 4 <= 160 KiB; >= 19 at E = 2048
  const int R = Q < fit ? Q : fit;
  const size_t lds = ((size_t)R * E + E + R) * sizeof(float);
  const int nv = (E + 63) / 64;
  auto kern = nv <= 8 ? cosine_logits_wide_kernel<8>
                      : (nv <= 12 ? cosine_logits_wide_kernel<12> : (nv <= 16 ? cosine_logits_wide_kernel<16> : cosine_logits_wide_kernel<CL_MAXV>));
  if (lds > 48 * 1024) SG_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(n, CLW_TPB), (unsigned)B), dim3(256), lds, as_stream(s), tokens, cls, text, n, E, Q, R,
                     global_debias_factor, cls_token_lambda, logits);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_postprocess_wide(const float* logits, const int32_t* query_idx, int Q, int K, int H, int W, float logit_scale,
                                   float prob_thd, int bg_idx, float* probs, int64_t* labels, sg_stream s) {
  SG_REQUIRE(logits && query_idx && labels, "sg_postprocess_wide: null pointer");
  SG_REQUIRE(Q > 0 && K > 0 && K <= Q && H > 0 && W > 0, "sg_postprocess_wide: Q=%d K=%d H=%d W=%d unsupported", Q, K, H, W);
  const int64_t HW = (int64_t)H * W;
  SG_REQUIRE(cdiv(HW, 256) <= INT32_MAX, "sg_postprocess_wide: image too large for one launch");
  hipLaunchKernelGGL(postprocess_wide_kernel, dim3((unsigned)cdiv(HW, 256)), dim3(256), 0, as_stream(s), logits, query_idx, Q, K, HW,
                     logit_scale, prob_thd, bg_idx, probs, labels);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_label_head(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                             int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                             int64_t* labels, float* conf, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && query_idx && labels, "sg_label_head: null pointer");
  SG_TRY(head_check_image(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_rows(__func__, "canvas", H));
  return head_launch_image(label_head_kernel, H, W, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, query_idx, K,
                           logit_scale, prob_thd, bg_idx, labels, conf);
}

extern "C" int sg_label_head_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                                   int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                                   const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                                   const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, int64_t* labels,
                                   float* conf, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && out_offset && block_prefix && query_idx && labels,
             "sg_label_head_multi: null pointer");
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_blocks(__func__, total_blocks, out_pixels));
  return head_launch_blocks(label_head_multi_kernel, total_blocks, s, tile_logits, windows, tile_image, T, Q, gh, gw, up_h, up_w, pad_t, pad_l,
                            image_hw, image_tiles, out_offset, block_prefix, N, out_pixels, query_idx, K, logit_scale, prob_thd, bg_idx, labels,
                            conf);
}

// ---- weighted window blending: the four entries above with a ramp table (include/segearth_hip.h) ------------------------------------------
// Each checks the table first, then what its counterpart checks.
extern "C" int sg_stitch_blend(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w,
                               int pad_t, int pad_l, int H, int W, float* canvas, const float* ramp, int ramp_len, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && canvas, "sg_stitch_blend: null pointer");
  SG_TRY(head_check_ramp(__func__, ramp, ramp_len));
  SG_TRY(head_check_stitch(__func__, T, Q, gh, gw, H, W));
  return head_launch_image(stitch_blend_kernel, H, W, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, canvas, ramp,
                           ramp_len);
}

extern "C" int sg_stitch_blend_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh,
                                     int gw, int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                                     const int64_t* canvas_offset, const int64_t* block_prefix, int N, int64_t total_blocks,
                                     int64_t canvas_elems, float* canvases, const float* ramp, int ramp_len, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && canvas_offset && block_prefix && canvases,
             "sg_stitch_blend_multi: null pointer");
  SG_TRY(head_check_ramp(__func__, ramp, ramp_len));
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_blocks(__func__, total_blocks, canvas_elems, Q));
  return head_launch_blocks(stitch_blend_multi_kernel, total_blocks, s, tile_logits, windows, tile_image, T, Q, gh, gw, up_h, up_w, pad_t, pad_l,
                            image_hw, image_tiles, canvas_offset, block_prefix, N, canvas_elems, canvases, ramp, ramp_len);
}

extern "C" int sg_label_head_blend(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w,
                                   int pad_t, int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, float prob_thd,
                                   int bg_idx, int64_t* labels, float* conf, const float* ramp, int ramp_len, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && query_idx && labels, "sg_label_head_blend: null pointer");
  SG_TRY(head_check_ramp(__func__, ramp, ramp_len));
  SG_TRY(head_check_image(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_rows(__func__, "canvas", H));
  return head_launch_image(label_head_blend_kernel, H, W, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, query_idx, K,
                           logit_scale, prob_thd, bg_idx, labels, conf, ramp, ramp_len);
}

extern "C" int sg_label_head_blend_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh,
                                         int gw, int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw,
                                         const int32_t* image_tiles, const int64_t* out_offset, const int64_t* block_prefix, int N,
                                         int64_t total_blocks, int64_t out_pixels, const int32_t* query_idx, int K, float logit_scale,
                                         float prob_thd, int bg_idx, int64_t* labels, float* conf, const float* ramp, int ramp_len,
                                         sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && out_offset && block_prefix && query_idx && labels,
             "sg_label_head_blend_multi: null pointer");
  SG_TRY(head_check_ramp(__func__, ramp, ramp_len));
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_blocks(__func__, total_blocks, out_pixels));
  return head_launch_blocks(label_head_blend_multi_kernel, total_blocks, s, tile_logits, windows, tile_image, T, Q, gh, gw, up_h, up_w, pad_t,
                            pad_l, image_hw, image_tiles, out_offset, block_prefix, N, out_pixels, query_idx, K, logit_scale, prob_thd, bg_idx,
                            labels, conf, ramp, ramp_len);
}

// QMAX of the probability head: sg_postprocess's two instantiations up to PP_MAX_Q, the three-pass form (0) beyond.
#define SG_PROB_HEAD_DISPATCH(kernel, Q) ((Q) <= 16 ? kernel<16> : ((Q) <= PP_MAX_Q ? kernel<PP_MAX_Q> : kernel<0>))

extern "C" int sg_prob_head(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                            int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                            float* probs, int64_t* labels, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && query_idx && labels, "sg_prob_head: null pointer");
  SG_REQUIRE(probs, "sg_prob_head: probs is NULL (labels alone: sg_label_head)");
  SG_TRY(head_check_image(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_rows(__func__, "canvas", H));
  return head_launch_image(SG_PROB_HEAD_DISPATCH(prob_head_kernel, Q), H, W, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H,
                           W, query_idx, K, logit_scale, prob_thd, bg_idx, probs, labels);
}

extern "C" int sg_prob_head_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                                  int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                                  const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                                  const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, float* probs,
                                  int64_t* labels, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && out_offset && block_prefix && query_idx && labels,
             "sg_prob_head_multi: null pointer");
  SG_REQUIRE(probs, "sg_prob_head_multi: probs is NULL (labels alone: sg_label_head_multi)");
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_blocks(__func__, total_blocks, out_pixels));
  return head_launch_blocks(SG_PROB_HEAD_DISPATCH(prob_head_multi_kernel, Q), total_blocks, s, tile_logits, windows, tile_image, T, Q, gh, gw,
                            up_h, up_w, pad_t, pad_l, image_hw, image_tiles, out_offset, block_prefix, N, out_pixels, query_idx, K, logit_scale,
                            prob_thd, bg_idx, probs, labels);
}

// KTOP of the top-k head: the next power of two of k; the kernel writes the first k slots.
#define SG_TOPK_HEAD_DISPATCH(kernel, k) ((k) <= 1 ? kernel<1> : ((k) <= 2 ? kernel<2> : ((k) <= 4 ? kernel<4> : kernel<TOPK_MAX>)))
static_assert(TOPK_MAX == SG_TOPK_MAX, "the header's SG_TOPK_MAX is the largest instantiated list");

extern "C" int sg_topk_head(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                            int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, int k, int32_t* classes,
                            float* probs, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && query_idx && classes && probs, "sg_topk_head: null pointer");
  SG_TRY(head_check_image(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_topk(__func__, k, K));
  SG_TRY(head_check_rows(__func__, "canvas", H));
  return head_launch_image(SG_TOPK_HEAD_DISPATCH(topk_head_kernel, k), H, W, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H,
                           W, query_idx, K, logit_scale, k, classes, probs);
}

extern "C" int sg_topk_head_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                                  int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                                  const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                                  const int32_t* query_idx, int K, float logit_scale, int k, int32_t* classes, float* probs, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && out_offset && block_prefix && query_idx && classes && probs,
             "sg_topk_head_multi: null pointer");
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_topk(__func__, k, K));
  SG_TRY(head_check_blocks(__func__, total_blocks, out_pixels));
  return head_launch_blocks(SG_TOPK_HEAD_DISPATCH(topk_head_multi_kernel, k), total_blocks, s, tile_logits, windows, tile_image, T, Q, gh, gw,
                            up_h, up_w, pad_t, pad_l, image_hw, image_tiles, out_offset, block_prefix, N, out_pixels, query_idx, K, logit_scale,
                            k, classes, probs);
}

// ---- the label and top-k heads at another ori_shape (segmentor.py:447-449 fused into the heads) ------------------------------------------
// The launch covers the output, so it is the output that can be too tall.
extern "C" int sg_label_head_resized(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w,
                                     int pad_t, int pad_l, int H, int W, int out_h, int out_w, const int32_t* query_idx, int K,
                                     float logit_scale, float prob_thd, int bg_idx, int64_t* labels, float* conf, int flags, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && query_idx && labels, "sg_label_head_resized: null pointer");
  SG_TRY(head_check_resized_image(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, out_h, out_w));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_rows(__func__, "output", out_h));
  SG_TRY(head_check_flags(__func__, flags));
  SG_TRY(head_check_staged_fit(__func__, flags, H, W, out_h, out_w));
  return head_launch_image(label_head_resized_kernel, out_h, out_w, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W,
                           out_h, out_w, query_idx, K, logit_scale, prob_thd, bg_idx, labels, conf, flags);
}

extern "C" int sg_label_head_resized_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh,
                                           int gw, int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw,
                                           const int32_t* image_tiles, const int32_t* out_hw, const int64_t* out_offset,
                                           const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                                           const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, int64_t* labels,
                                           float* conf, int flags, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && out_hw && out_offset && block_prefix && query_idx && labels,
             "sg_label_head_resized_multi: null pointer");
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_blocks(__func__, total_blocks, out_pixels));
  SG_TRY(head_check_flags(__func__, flags));
  return head_launch_blocks(label_head_resized_multi_kernel, total_blocks, s, tile_logits, windows, tile_image, T, Q, gh, gw, up_h, up_w, pad_t,
                            pad_l, image_hw, image_tiles, out_hw, out_offset, block_prefix, N, out_pixels, query_idx, K, logit_scale, prob_thd,
                            bg_idx, labels, conf, flags);
}

extern "C" int sg_topk_head_resized(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w,
                                    int pad_t, int pad_l, int H, int W, int out_h, int out_w, const int32_t* query_idx, int K,
                                    float logit_scale, int k, int32_t* classes, float* probs, int flags, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && query_idx && classes && probs, "sg_topk_head_resized: null pointer");
  SG_TRY(head_check_resized_image(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, out_h, out_w));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_topk(__func__, k, K));
  SG_TRY(head_check_rows(__func__, "output", out_h));
  SG_TRY(head_check_flags(__func__, flags));
  SG_TRY(head_check_staged_fit(__func__, flags, H, W, out_h, out_w));
  return head_launch_image(SG_TOPK_HEAD_DISPATCH(topk_head_resized_kernel, k), out_h, out_w, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w,
                           pad_t, pad_l, H, W, out_h, out_w, query_idx, K, logit_scale, k, classes, probs, flags);
}

extern "C" int sg_topk_head_resized_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh,
                                          int gw, int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw,
                                          const int32_t* image_tiles, const int32_t* out_hw, const int64_t* out_offset,
                                          const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                                          const int32_t* query_idx, int K, float logit_scale, int k, int32_t* classes, float* probs, int flags,
                                          sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && out_hw && out_offset && block_prefix && query_idx && classes &&
                 probs, "sg_topk_head_resized_multi: null pointer");
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_topk(__func__, k, K));
  SG_TRY(head_check_blocks(__func__, total_blocks, out_pixels));
  SG_TRY(head_check_flags(__func__, flags));
  return head_launch_blocks(SG_TOPK_HEAD_DISPATCH(topk_head_resized_multi_kernel, k), total_blocks, s, tile_logits, windows, tile_image, T, Q,
                            gh, gw, up_h, up_w, pad_t, pad_l, image_hw, image_tiles, out_hw, out_offset, block_prefix, N, out_pixels, query_idx,
                            K, logit_scale, k, classes, probs, flags);
}

// ---- test-time augmentation ---------------------------------------------------------------------------------------------------------------
static_assert(sizeof(TtaViews) <= 1024, "the view table travels as a kernel argument");

extern "C" int sg_tta_head(const float* tile_logits, int64_t logit_elems, const int32_t* windows, int total_tiles, const int32_t* views, int V,
                           int Q, int out_h, int out_w, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                           int64_t* labels, float* conf, float* probs, int flags, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && views && query_idx && labels, "sg_tta_head: null pointer");
  SG_REQUIRE(V >= 1 && V <= SG_TTA_MAX_VIEWS, "sg_tta_head: V=%d views, must lie in [1, %d]", V, SG_TTA_MAX_VIEWS);
  SG_REQUIRE(Q > 0 && Q <= PP_MAX_Q, "sg_tta_head: Q=%d must lie in [1, %d] (more queries: sg_tta_accumulate / sg_tta_finish)", Q, PP_MAX_Q);
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_bg(__func__, bg_idx, K));
  SG_REQUIRE(out_h > 0 && out_w > 0, "sg_tta_head: bad output size %dx%d", out_h, out_w);
  SG_TRY(head_check_rows(__func__, "output", out_h));
  SG_TRY(head_check_flags(__func__, flags));
  TtaViews tv;
  memset(&tv, 0, sizeof(tv));
  int64_t tiles = 0, elems = 0;
  for (int v = 0; v < V; ++v) {
    const int32_t* f = views + (int64_t)v * SG_TTA_VIEW_FIELDS;
    TtaView& d = tv.v[v];
    d.T = f[0]; d.t0 = f[1]; d.gh = f[2]; d.gw = f[3]; d.up_h = f[4]; d.up_w = f[5]; d.pad_t = f[6]; d.pad_l = f[7]; d.h = f[8]; d.w = f[9];
    d.flip = f[10]; d.off = elems;
    SG_REQUIRE(d.T > 0 && d.gh > 0 && d.gw > 0 && d.up_h > 0 && d.up_w > 0 && d.pad_t >= 0 && d.pad_l >= 0 && d.h > 0 && d.w > 0,
               "sg_tta_head: view %d has a bad shape T=%d gh=%d gw=%d up=%dx%d pad=%d,%d H=%d W=%d", v, d.T, d.gh, d.gw, d.up_h, d.up_w, d.pad_t,
               d.pad_l, d.h, d.w);
    SG_REQUIRE(d.flip == 0 || d.flip == 1, "sg_tta_head: view %d has flip=%d, neither 0 nor 1", v, d.flip);
    SG_REQUIRE(d.t0 == tiles, "sg_tta_head: view %d starts at tile %d, but the views before it hold %lld (the views' tiles follow each other)",
               v, d.t0, (long long)tiles);
    tiles += d.T;
    elems += (int64_t)d.T * Q * d.gh * d.gw;
  }
  SG_REQUIRE(tiles == total_tiles && elems == logit_elems,
             "sg_tta_head: the views hold %lld tiles and %lld logits, the buffers %d and %lld", (long long)tiles, (long long)elems, total_tiles,
             (long long)logit_elems);
  auto kern = Q <= 16 ? tta_head_kernel<16> : tta_head_kernel<PP_MAX_Q>;
  const size_t lds = (size_t)(K - 1) * 256 * sizeof(float);        // 63 KiB at K = 64: with the 16 KiB stage two workgroups fit a CU's 160 KiB
  if (lds > 32 * 1024) SG_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), (size_t)PP_MAX_Q * 256 * sizeof(float)));
  hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(out_w, 64), (unsigned)cdiv(out_h, 4)), dim3(256), lds, as_stream(s), tile_logits, windows, tv, V, Q,
                     out_h, out_w, query_idx, K, logit_scale, prob_thd, bg_idx, labels, conf, probs, flags);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_tta_accumulate(const float* probs_view, int K, int out_h, int out_w, int flip, float* acc, int first, sg_stream s) {
  SG_REQUIRE(probs_view && acc && probs_view != acc, "sg_tta_accumulate: null pointer, or the view's planes are the accumulator");
  SG_REQUIRE(K > 0 && out_h > 0 && out_w > 0, "sg_tta_accumulate: bad shape K=%d out=%dx%d", K, out_h, out_w);
  SG_REQUIRE((flip == 0 || flip == 1) && (first == 0 || first == 1), "sg_tta_accumulate: flip=%d first=%d, each 0 or 1", flip, first);
  const int64_t rows = (int64_t)K * out_h, n = rows * out_w;
  SG_REQUIRE(cdiv(n, 256) <= INT32_MAX, "sg_tta_accumulate: too large for one launch");
  hipLaunchKernelGGL(tta_accumulate_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(s), probs_view, rows, out_w, flip, first, acc);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_tta_finish(const float* acc, int V, int K, int out_h, int out_w, float prob_thd, int bg_idx, int64_t* labels, float* conf,
                             float* probs, sg_stream s) {
  SG_REQUIRE(acc && labels, "sg_tta_finish: null pointer");
  SG_REQUIRE(V >= 1 && V <= SG_TTA_MAX_VIEWS, "sg_tta_finish: V=%d views, must lie in [1, %d]", V, SG_TTA_MAX_VIEWS);
  SG_REQUIRE(K > 0 && out_h > 0 && out_w > 0, "sg_tta_finish: bad shape K=%d out=%dx%d", K, out_h, out_w);
  SG_REQUIRE(bg_idx >= 0 && bg_idx < K, "sg_tta_finish: bg_idx=%d outside [0, K=%d)", bg_idx, K);
  const int64_t HW = (int64_t)out_h * out_w;
  SG_REQUIRE(cdiv(HW, 256) <= INT32_MAX, "sg_tta_finish: too large for one launch");
  hipLaunchKernelGGL(tta_finish_kernel, dim3((unsigned)cdiv(HW, 256)), dim3(256), 0, as_stream(s), acc, V, K, HW, prob_thd, bg_idx, labels, conf,
                     probs);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_area_relabel(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                               int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                               const int32_t* keep, const float* conf, int64_t* labels, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && query_idx && keep && conf && labels, "sg_area_relabel: null pointer");
  SG_TRY(head_check_image(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_area_K(__func__, K));
  SG_TRY(head_check_bg(__func__, bg_idx, K));
  SG_TRY(head_check_rows(__func__, "canvas", H));
  return head_launch_image(area_relabel_kernel, H, W, s, tile_logits, windows, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, H, W, query_idx, K,
                           logit_scale, prob_thd, bg_idx, keep, conf, labels);
}

extern "C" int sg_area_relabel_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                                     int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                                     const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                                     const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, const int32_t* keep,
                                     const float* conf, int64_t* labels, sg_stream s) {
  SG_REQUIRE(tile_logits && windows && tile_image && image_hw && image_tiles && out_offset && block_prefix && query_idx && keep && conf && labels,
             "sg_area_relabel_multi: null pointer");
  SG_TRY(head_check_images(__func__, T, Q, gh, gw, up_h, up_w, pad_t, pad_l, N));
  SG_TRY(head_check_K(__func__, K, Q));
  SG_TRY(head_check_area_K(__func__, K));
  SG_TRY(head_check_bg(__func__, bg_idx, K));
  SG_TRY(head_check_blocks(__func__, total_blocks, out_pixels));
  return head_launch_blocks(area_relabel_multi_kernel, total_blocks, s, tile_logits, windows, tile_image, T, Q, gh, gw, up_h, up_w, pad_t, pad_l,
                            image_hw, image_tiles, out_offset, block_prefix, N, out_pixels, query_idx, K, logit_scale, prob_thd, bg_idx, keep,
                            conf, labels);
}
