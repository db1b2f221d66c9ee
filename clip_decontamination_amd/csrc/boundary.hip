// Boundary IoU (Cheng et al., CVPR 2021): the band of a label map and the band-restricted counts (the definition: include/segearth_hip.h).
//   band(y,x) = 1 iff the window [y-d,y+d] x [x-d,x+d] leaves the image or holds a label other than L(y,x)
// The window test decomposes exactly, and neither pass loops over the window: the work per pixel does not grow with d.
//   row pass    : one workgroup sweeps one row left to right with a running maximum s(u) = start of the run of equal labels that holds
//                 column u (a block-wide max-scan of break positions, carried from chunk to chunk).  The segment [x-d, x+d] is inside the
//                 image and uniform iff s(x+d) <= x-d, so the lane at u = x+d writes the byte of x = u-d:
//                   bit 0  ok(y,x)   = u - s(u) >= 2d           (the last d columns of a row get 0: their segment leaves the image)
//                   bit 1  up(y,x)   = ok && y > 0 && L(y,u) == L(y-1,u)
//                 Where ok(y,x) and ok(y-1,x) both hold, both rows are uniform over [x-d, x+d], so the comparison at column u stands for
//                 the one at column x; the column pass reads bit 1 only there.  It then needs no label at all: 1 byte in, 1 byte out.
//   column pass : one lane per column marches down a band of rows with cnt(u) = ok(u) ? (up(u) && cnt(u-1) ? cnt(u-1) + 1 : 1) : 0, clamped
//                 at 2d+1; rows y-d .. y+d are all ok and of one label iff cnt(y+d) >= 2d+1, so row u settles band(u-d).  A band of R output
//                 rows starts its march d rows above its first output row with cnt = 0 (a halo of 2d rows in all); the clamped count is
//                 exact from the first row it is used at.  Reads and writes are coalesced rows of bytes.
//   count       : prediction, truth and the two band maps -> 3K 32-bit bins in LDS per workgroup, one 64-bit add per non-zero bin; the
//                 run merge and the leader match of confusion_kernel (metric.hip), once per bin stream.
// Integers and integer atomics only; no workgroup waits for another; nothing visits the host.
#include "common.h"

namespace sg {

constexpr int BD_MAX_D = 4095;
constexpr int BD_ROW_RUN = 8;                    // consecutive pixels per lane per chunk of the row pass
constexpr int BD_ROW_CHUNK = 256 * BD_ROW_RUN;
constexpr int BD_CNT_RUN = 16;                   // consecutive pixels per lane per step of the count
constexpr int BD_WG_PER_CU = 4;
constexpr int BD_ROW_MAX_BLOCKS = 1 << 20;          // workgroups of the row pass: rows beyond it are looped over
constexpr int BD_COL_BATCH = 16;                 // rows a lane of the column pass loads ahead
constexpr int BD_COL_WAVES_PER_CU = 16;          // the column pass splits the rows until about this many waves per CU march

template <typename T>
__global__ __launch_bounds__(256) void bd_row_kernel(const T* __restrict__ labels, int H, int W, int d, int rzl, uint8_t* __restrict__ rowb) {
  __shared__ int wave_last[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int par = 0;                                                           // LDS slot of the chunk; it keeps alternating from row to row
  // a workgroup takes the rows blockIdx.x, blockIdx.x + gridDim.x, ...: the grid stays below BD_ROW_MAX_BLOCKS whatever H is
  for (int64_t y = blockIdx.x; y < H; y += gridDim.x) {
    const T* row = labels + (int64_t)y * W;
    const T* above = y > 0 ? row - W : nullptr;
    uint8_t* out = rowb + (int64_t)y * W;
    // the last d columns: [x-d, x+d] leaves the image.  No lane below writes them (a lane at u < W writes column u - d < W - d).
    for (int64_t x = (W > d ? W - d : 0) + tid; x < W; x += 256) out[x] = 0;
    int carry = 0;                                                         // start of the run that reaches the chunk's first column (< W)
    for (int64_t c0 = 0; c0 < W; c0 += BD_ROW_CHUNK, par ^= 1) {           // block-uniform
      const int64_t u0 = c0 + (int64_t)tid * BD_ROW_RUN;
      int64_t v[BD_ROW_RUN], up[BD_ROW_RUN];
      lm_load_run<BD_ROW_RUN>(row, u0, W, rzl, v);
      if (above) lm_load_run<BD_ROW_RUN>(above, u0, W, rzl, up);
      const int64_t prev = (u0 > 0 && u0 < W) ? lm_value(row, u0 - 1, rzl) : 0;
      bool brk[BD_ROW_RUN];
      int last = -1;                                                       // the lane's last break column, -1 = none
#pragma unroll
      for (int j = 0; j < BD_ROW_RUN; ++j) {
        brk[j] = j == 0 ? (u0 == 0 || v[0] != prev) : v[j] != v[j - 1];
        if (brk[j] && u0 + j < W) last = (int)(u0 + j);
      }
      // inclusive max-scan of `last` over the workgroup: lanes of a wave by shuffles, the four waves through LDS
      int inc = last;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o && t > inc) inc = t;
      }
      if (lane == 63) wave_last[par][wave] = inc;
      int64_t s = __shfl_up(inc, 1);                                       // exclusive: the lanes before this one (64-bit from here: u0 + j may pass W)
      if (lane == 0) s = -1;
      __syncthreads();                                                     // the other parity is written next: one barrier per chunk
      int all = carry;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int t = wave_last[par][w];
        if (w < wave && t > s) s = t;
        if (t > all) all = t;
      }
      if (carry > s) s = carry;
      carry = all;
      uint8_t b[BD_ROW_RUN];
#pragma unroll
      for (int j = 0; j < BD_ROW_RUN; ++j) {
        if (brk[j]) s = u0 + j;
        const bool ok = u0 + j - s >= 2 * d;
        b[j] = ok ? (uint8_t)(1 | ((above && v[j] == up[j]) ? 2 : 0)) : (uint8_t)0;
      }
      const int64_t x0 = u0 - d;
      if (x0 >= 0 && u0 + BD_ROW_RUN <= W) {
        __builtin_memcpy(out + x0, b, sizeof(b));
      } else {
#pragma unroll
        for (int j = 0; j < BD_ROW_RUN; ++j)
          if (x0 + j >= 0 && u0 + j < W) out[x0 + j] = b[j];
      }
    }
  }
}

// BD_COL_BATCH rows of one column from row u0.  MODE 0: all halo, nothing stored; 1: all stored; 2: rows past u_end and halo rows tested
template <int MODE>
__device__ __forceinline__ void bd_col_step(const uint8_t* __restrict__ rowb, uint8_t* __restrict__ band, uint32_t x, int64_t u0, int64_t u_out, int64_t u_end,
                                            uint32_t W, int d, int full, int& cnt) {
  int b[BD_COL_BATCH];
#pragma unroll
  for (int j = 0; j < BD_COL_BATCH; ++j) b[j] = (MODE != 2 || u0 + j <= u_end) ? (int)rowb[(uint32_t)(u0 + j) * W + x] : 0;   // < 2^31 pixels: 32-bit offsets
#pragma unroll
  for (int j = 0; j < BD_COL_BATCH; ++j) {
    const int64_t u = u0 + j;
    cnt = (b[j] & 1) ? (((b[j] & 2) && cnt) ? (cnt < full ? cnt + 1 : full) : 1) : 0;
    if (MODE == 1 || (MODE == 2 && u >= u_out && u <= u_end)) band[(uint32_t)(u - d) * W + x] = cnt < full ? 1 : 0;
  }
}

// blockIdx.x = row band * column groups + column group; a lane owns one column of the band
__global__ __launch_bounds__(256) void bd_col_kernel(const uint8_t* __restrict__ rowb, int H, int W, int d, int R, int col_groups,
                                                     uint8_t* __restrict__ band) {
  const int cg = blockIdx.x % col_groups, rb = blockIdx.x / col_groups;
  const int64_t x = (int64_t)cg * 256 + threadIdx.x;
  if (x >= W) return;
  const int64_t yb = (int64_t)rb * R, ye = yb + R < H ? yb + R : H;
  const int full = 2 * d + 1;
  const int64_t u_begin = yb > d ? yb - d : 0;                             // 64-bit: H may be close to 2^31 (a one-column image)
  const int64_t u_end = ye - 1 + d < H - 1 ? ye - 1 + d : H - 1;           // inclusive
  uint8_t* dst = band + x;
  int cnt = 0;
  // BD_COL_BATCH rows per step, their loads issued before the first is used: the march is a chain of dependent counts, not of loads.
  // A band that lies in the image's last d rows has nothing to march for.
  const int64_t u_out = yb + d;                                            // the rows above it are the halo: counts only
  for (int64_t u0 = u_begin; u0 <= u_end && yb < H - d; u0 += BD_COL_BATCH) {
    const int64_t u1 = u0 + BD_COL_BATCH - 1;
    if (u1 <= u_end && u1 < u_out) bd_col_step<0>(rowb, band, (uint32_t)x, u0, u_out, u_end, (uint32_t)W, d, full, cnt);
    else if (u1 <= u_end && u0 >= u_out) bd_col_step<1>(rowb, band, (uint32_t)x, u0, u_out, u_end, (uint32_t)W, d, full, cnt);
    else bd_col_step<2>(rowb, band, (uint32_t)x, u0, u_out, u_end, (uint32_t)W, d, full, cnt);
  }
  // rows whose window leaves the image at the bottom
  for (int64_t yy = (H - d > yb ? H - d : yb); yy < ye; ++yy) dst[yy * W] = 1;
}

// the three bins of one pixel (-1 = none): intersection k, prediction band K + k, truth band 2K + k
__device__ __forceinline__ void bd_pixel_bins(int64_t p, int64_t g, int bp, int bg, int K, int ignore_index, int rzl, int& bi, int& bpd, int& bgt) {
  if (rzl) g = lm_reduce_zero(g);
  const bool counted = g != (int64_t)ignore_index;
  const bool pin = counted && bp && (uint64_t)p < (uint64_t)K;
  const bool gin = counted && bg && (uint64_t)g < (uint64_t)K;
  bpd = pin ? K + (int)p : -1;
  bgt = gin ? 2 * K + (int)g : -1;
  bi = (pin && gin && p == g) ? (int)p : -1;
}

template <bool GT64>
__global__ __launch_bounds__(256) void bd_count_kernel(const int64_t* __restrict__ labels, const void* __restrict__ gtv,
                                                       const uint8_t* __restrict__ band_p, const uint8_t* __restrict__ band_g, int64_t n,
                                                       int64_t nchunks, int K, int ignore_index, int rzl, unsigned long long* __restrict__ areas) {
  extern __shared__ uint32_t bd_bins[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = 3 * K;
  const uint8_t* gt8 = reinterpret_cast<const uint8_t*>(gtv);
  const int64_t* gt64 = reinterpret_cast<const int64_t*>(gtv);
  for (int i = tid; i < nb; i += 256) bd_bins[i] = 0u;
  __syncthreads();

  if (blockIdx.x == 0 && tid < BD_CNT_RUN) {                             // the tail (< BD_CNT_RUN pixels): one pixel per thread
    const int64_t i = nchunks * BD_CNT_RUN + tid;
    if (i < n) {
      int bi, bpd, bgt;
      bd_pixel_bins(labels[i], GT64 ? gt64[i] : (int64_t)gt8[i], band_p[i], band_g[i], K, ignore_index, rzl, bi, bpd, bgt);
      if (bi >= 0) atomicAdd(&bd_bins[bi], 1u);
      if (bpd >= 0) atomicAdd(&bd_bins[bpd], 1u);
      if (bgt >= 0) atomicAdd(&bd_bins[bgt], 1u);
    }
  }

  for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 64; base < nchunks; base += (int64_t)gridDim.x * 256) {
    const int64_t c = base + lane;
    int bi[BD_CNT_RUN], bpd[BD_CNT_RUN], bgt[BD_CNT_RUN];
#pragma unroll
    for (int j = 0; j < BD_CNT_RUN; ++j) bi[j] = bpd[j] = bgt[j] = -1;
    if (c < nchunks) {
      const int64_t i0 = c * BD_CNT_RUN;
      int64_t p[BD_CNT_RUN], g[BD_CNT_RUN];
      uint8_t mp[BD_CNT_RUN], mg[BD_CNT_RUN];
      __builtin_memcpy(p, labels + i0, sizeof(p));
      __builtin_memcpy(mp, band_p + i0, sizeof(mp));                     // image offsets are not multiples of 16: byte-aligned copies
      __builtin_memcpy(mg, band_g + i0, sizeof(mg));
      if (GT64) {
        __builtin_memcpy(g, gt64 + i0, sizeof(g));
      } else {
        uint8_t g8[BD_CNT_RUN];
        __builtin_memcpy(g8, gt8 + i0, sizeof(g8));
#pragma unroll
        for (int j = 0; j < BD_CNT_RUN; ++j) g[j] = (int64_t)g8[j];
      }
#pragma unroll
      for (int j = 0; j < BD_CNT_RUN; ++j) bd_pixel_bins(p[j], g[j], mp[j], mg[j], K, ignore_index, rzl, bi[j], bpd[j], bgt[j]);
    }
    lm_add_stream<BD_CNT_RUN>(bi, bd_bins, lane);
    lm_add_stream<BD_CNT_RUN>(bpd, bd_bins, lane);
    lm_add_stream<BD_CNT_RUN>(bgt, bd_bins, lane);
  }
  __syncthreads();
  for (int i = tid; i < nb; i += 256) {
    const uint32_t v = bd_bins[i];
    if (v != 0u) atomicAdd(&areas[i], (unsigned long long)v);
  }
}

// rows of output per workgroup of the column pass.  A lane's march is latency-bound and as long as its band plus the halo of 2d rows,
// so the rows are split until about BD_COL_WAVES_PER_CU waves per CU march (bands of at least 16 rows): more bands re-read more halo,
// but the halo rows of all bands together stay below that many waves times 2d rows, whatever d and the image are.
static inline int bd_band_rows(int H, int W) {
  int64_t bands = (int64_t)device_cu_count() * BD_COL_WAVES_PER_CU / cdiv(W, 64);
  const int64_t most = cdiv(H, 16);
  bands = bands < 1 ? 1 : (bands > most ? most : bands);
  return (int)cdiv(H, bands);
}

template <typename T>
static int bd_band_image(const T* labels, int H, int W, int d, int rzl, uint8_t* rowb, uint8_t* band, hipStream_t st) {
  hipLaunchKernelGGL(bd_row_kernel<T>, dim3((unsigned)(H < BD_ROW_MAX_BLOCKS ? H : BD_ROW_MAX_BLOCKS)), dim3(256), 0, st, labels, H, W, d, rzl, rowb);
  SG_LAUNCH_CHECK();
  const int R = bd_band_rows(H, W);
  const int64_t col_groups = cdiv(W, 256), row_bands = cdiv(H, R);       // H * W < 2^31, so the product fits a grid
  hipLaunchKernelGGL(bd_col_kernel, dim3((unsigned)(col_groups * row_bands)), dim3(256), 0, st, rowb, H, W, d, R, (int)col_groups, band);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

// the checks both entries share: the images (fewer than 2^31 pixels each) and a band width in [1, BD_MAX_D] for every one
static int bd_check_images(const char* who, const int32_t* image_hw, const int64_t* offset, const int32_t* d, int N, int64_t* total_out) {
  const auto width = [&](int n) -> int {
    SG_REQUIRE(d[n] >= 1 && d[n] <= BD_MAX_D, "%s: d[%d]=%d outside [1, %d]", who, n, d[n], BD_MAX_D);
    return SG_OK;
  };
  return lm_check_images(who, image_hw, offset, N, false, width, total_out);
}

}  // namespace sg

using namespace sg;

extern "C" size_t sg_boundary_workspace_bytes(int64_t n_pixels_total) {
  if (n_pixels_total < 0) return 0;
  return 4 * lm_plane_bytes(n_pixels_total);
}

extern "C" int sg_boundary_band(const void* labels, int fmt, const int32_t* image_hw, const int64_t* offset, const int32_t* d, int N,
                                uint8_t* band, void* workspace, size_t workspace_bytes, sg_stream s) {
  SG_REQUIRE(labels && image_hw && offset && d && band && workspace, "sg_boundary_band: null pointer");
  SG_REQUIRE(fmt == SG_GT_U8 || fmt == SG_GT_I64, "sg_boundary_band: unknown label format %d", fmt);
  int64_t total = 0;
  SG_TRY(bd_check_images("sg_boundary_band", image_hw, offset, d, N, &total));
  SG_REQUIRE(fmt == SG_GT_U8 || lm_aligned8(labels), "sg_boundary_band: int64 labels must be 8-byte aligned");
  const size_t need = lm_plane_bytes(total);
  SG_REQUIRE(workspace_bytes >= need, "sg_boundary_band: workspace too small: %zu bytes given, %zu needed for %lld pixels", workspace_bytes,
             need, (long long)total);
  uint8_t* rowb = reinterpret_cast<uint8_t*>(workspace);
  for (int n = 0; n < N; ++n) {
    const int H = image_hw[2 * n], W = image_hw[2 * n + 1];
    if (fmt == SG_GT_U8)
      SG_TRY(bd_band_image(reinterpret_cast<const uint8_t*>(labels) + offset[n], H, W, d[n], 0, rowb + offset[n], band + offset[n], as_stream(s)));
    else
      SG_TRY(bd_band_image(reinterpret_cast<const int64_t*>(labels) + offset[n], H, W, d[n], 0, rowb + offset[n], band + offset[n], as_stream(s)));
  }
  return SG_OK;
}

extern "C" int sg_boundary_accumulate(const int64_t* labels, const void* gt, int gt_format, const int32_t* image_hw, const int64_t* offset,
                                      const int32_t* d, int N, int K, int ignore_index, int reduce_zero_label, int64_t* areas,
                                      void* workspace, size_t workspace_bytes, sg_stream s) {
  SG_REQUIRE(labels && gt && image_hw && offset && d && areas && workspace, "sg_boundary_accumulate: null pointer");
  SG_REQUIRE(gt_format == SG_GT_U8 || gt_format == SG_GT_I64, "sg_boundary_accumulate: unknown ground-truth format %d", gt_format);
  SG_REQUIRE(K >= 1, "sg_boundary_accumulate: K=%d, need at least one class", K);
  SG_REQUIRE(K <= LM_MAX_K, "sg_boundary_accumulate: K=%d exceeds %d (the cap of sg_confusion_accumulate)", K, LM_MAX_K);
  int64_t total = 0;
  SG_TRY(bd_check_images("sg_boundary_accumulate", image_hw, offset, d, N, &total));
  SG_REQUIRE(lm_aligned8(labels) && (gt_format == SG_GT_U8 || lm_aligned8(gt)) && lm_aligned8(areas),
             "sg_boundary_accumulate: int64 buffers must be 8-byte aligned");
  const size_t need = sg_boundary_workspace_bytes(total);
  SG_REQUIRE(workspace_bytes >= need, "sg_boundary_accumulate: workspace too small: %zu bytes given, %zu needed for %lld pixels",
             workspace_bytes, need, (long long)total);
  // workspace: row bytes of the prediction, row bytes of the truth, band of the prediction, band of the truth
  const size_t plane = lm_plane_bytes(total);
  uint8_t* rowb_p = reinterpret_cast<uint8_t*>(workspace);
  uint8_t* rowb_g = rowb_p + plane;
  uint8_t* band_p = rowb_g + plane;
  uint8_t* band_g = band_p + plane;
  const bool gt64 = gt_format == SG_GT_I64;
  const int rzl = reduce_zero_label ? 1 : 0;
  const hipStream_t st = as_stream(s);
  const size_t lds = (size_t)3 * K * sizeof(uint32_t);
  const int64_t cap = (int64_t)device_cu_count() * BD_WG_PER_CU;
  for (int n = 0; n < N; ++n) {
    const int H = image_hw[2 * n], W = image_hw[2 * n + 1];
    const int64_t o = offset[n], px = (int64_t)H * W;
    SG_TRY(bd_band_image(labels + o, H, W, d[n], 0, rowb_p + o, band_p + o, st));
    if (gt64)
      SG_TRY(bd_band_image(reinterpret_cast<const int64_t*>(gt) + o, H, W, d[n], rzl, rowb_g + o, band_g + o, st));
    else
      SG_TRY(bd_band_image(reinterpret_cast<const uint8_t*>(gt) + o, H, W, d[n], rzl, rowb_g + o, band_g + o, st));
    const int64_t nchunks = px / BD_CNT_RUN;
    int64_t blocks = cdiv(nchunks, 256);
    blocks = blocks < 1 ? 1 : (blocks > cap ? cap : blocks);             // an image has < 2^31 pixels: no 32-bit count wraps
    const void* gt_n = lm_gt_at(gt, gt_format, o);
    auto kern = gt64 ? bd_count_kernel<true> : bd_count_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st, labels + o, gt_n, (const uint8_t*)(band_p + o),
                       (const uint8_t*)(band_g + o), px, nchunks, K, ignore_index, rzl, reinterpret_cast<unsigned long long*>(areas));
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}
