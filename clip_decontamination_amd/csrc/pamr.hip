// PAMR (Pixel-Adaptive Mask Refinement, Araslanov & Roth 2020): the optional last stage of the training-free open-vocabulary segmenters
// whose attention variants this library implements.  It snaps the stitched patch-grid logits to image edges.  The definition is stated in
// include/segearth_hip.h (sg_pamr); in short, with D dilations, 8 offsets each, replicate padding:
//   affinity : g [3,H,W] -> w [8D,H,W], w_k(p) = softmax_k of the channel mean of -|g(p) - g(n_k(p))| / (1e-8 + 0.1 sigma(p)), sigma the
//              unbiased standard deviation of the 9D window samples (two passes)
//   step     : m_out[q,p] = sum_k w_k(p) m_in[q, n_k(p)], k ascending
// Both kernels: one pixel per lane over the flat pixel index (coalesced whatever W is), D a template parameter so that the 8D weights and
// the 6D clamped coordinates live in registers, no atomics, fixed trip counts, every coordinate clamped before it addresses anything,
// 64-bit element indices.  A lane's result depends on its own pixel alone, so repeats are byte-identical.
// The step is bound by HBM and L2: per pixel it reads the 8D weights once, then per query 8D neighbours (each element is read by 8D
// different pixels: re-reads are served by L1 / L2) and writes one value: (2Q + 8D) * 4 bytes per pixel from HBM.  Workgroups take the
// pixels in raster order; handing each XCD a contiguous band of the image instead measured 8 to 39 % slower per step.
#include "common.h"

namespace sg {

constexpr int PAMR_MAX_DIL = 8;
constexpr int PAMR_MAX_D = 64;
constexpr int PAMR_MAX_STEPS = 64;
constexpr int64_t PAMR_MAX_PIXELS = (int64_t)1 << 38;      // the grid (pixels / 256) stays below 2^31
constexpr int64_t PAMR_MAX_ELEMS = (int64_t)1 << 60;

struct PamrDil { int d[PAMR_MAX_DIL]; };                       // the dilations, passed to the kernels by value

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Flat pixel index of this lane (256 consecutive pixels per workgroup, raster order), or -1 beyond the image.
__device__ __forceinline__ int64_t pamr_pixel(int64_t HW) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  return p < HW ? p : -1;
}

// Clamped neighbour coordinates of pixel (y, x): row[i][j] = clamp(y + d_i (j - 1)) * W as an element offset, col[i][j] likewise for x.
template <int D>
__device__ __forceinline__ void pamr_coords(const PamrDil& dil, int y, int x, int H, int W, int64_t (&row)[D][3], int (&col)[D][3]) {
#pragma unroll
  for (int i = 0; i < D; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      row[i][j] = (int64_t)clampi(y + dil.d[i] * (j - 1), H - 1) * W;
      col[i][j] = clampi(x + dil.d[i] * (j - 1), W - 1);
    }
  }
}

// the eight offsets in the order of the definition: (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1) as indices into row / col
__host__ __device__ constexpr int pamr_dy(int j) { return j < 3 ? 0 : (j < 5 ? 1 : 2); }
__host__ __device__ constexpr int pamr_dx(int j) { return j < 3 ? j : (j < 5 ? (j == 3 ? 0 : 2) : j - 5); }

template <int D>
__global__ __launch_bounds__(256) void pamr_affinity_kernel(const float* __restrict__ g, int H, int W, PamrDil dil, float* __restrict__ w) {
  const int64_t HW = (int64_t)H * W;
  const int64_t p = pamr_pixel(HW);
  if (p < 0) return;
  const int y = (int)(p / W), x = (int)(p % W);
  int64_t row[D][3];
  int col[D][3];
  pamr_coords<D>(dil, y, x, H, W, row, col);
  constexpr int N = 9 * D;
  float a[8 * D];
#pragma unroll
  for (int k = 0; k < 8 * D; ++k) a[k] = 0.f;
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    const float* gc = g + c * HW;
    const float ctr = gc[p];
    // sigma over the 9D samples in two passes, on differences to the centre (the mean is shift-invariant; a flat window gives exactly 0)
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < 9; ++j) sum += gc[row[i][j / 3] + col[i][j % 3]] - ctr;
    const float mean = sum / (float)N;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const float dv = (gc[row[i][j / 3] + col[i][j % 3]] - ctr) - mean;
        ss = fmaf(dv, dv, ss);
      }
    const float sigma = sqrtf(ss / (float)(N - 1));
    const float den = 1e-8f + 0.1f * sigma;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) a[i * 8 + j] += fabsf(ctr - gc[row[i][pamr_dy(j)] + col[i][pamr_dx(j)]]) / den;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 8 * D; ++k) { a[k] = -a[k] / 3.0f; mx = fmaxf(mx, a[k]); }
  float tot = 0.f;
#pragma unroll
  for (int k = 0; k < 8 * D; ++k) { a[k] = expf(a[k] - mx); tot += a[k]; }
#pragma unroll
  for (int k = 0; k < 8 * D; ++k) w[k * HW + p] = a[k] / tot;
}

template <int D>
__global__ __launch_bounds__(256) void pamr_step_kernel(const float* __restrict__ w, const float* __restrict__ in, float* __restrict__ out,
                                                        int Q, int H, int W, PamrDil dil) {
  const int64_t HW = (int64_t)H * W;
  const int64_t p = pamr_pixel(HW);
  if (p < 0) return;
  const int y = (int)(p / W), x = (int)(p % W);
  int64_t row[D][3];
  int col[D][3];
  pamr_coords<D>(dil, y, x, H, W, row, col);
  float wk[8 * D];
#pragma unroll
  for (int k = 0; k < 8 * D; ++k) wk[k] = w[k * HW + p];
#pragma unroll 1
  for (int q = 0; q < Q; ++q) {
    const float* m = in + q * HW;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = fmaf(wk[i * 8 + j], m[row[i][pamr_dy(j)] + col[i][pamr_dx(j)]], acc);
    out[q * HW + p] = acc;
  }
}

static int pamr_check_dims(const char* who, int Q, int H, int W, const int* dilations, int n_dil) {
  SG_REQUIRE(Q >= 1 && H >= 1 && W >= 1, "%s: Q=%d H=%d W=%d, each must be at least 1", who, Q, H, W);
  SG_REQUIRE((int64_t)H * W <= PAMR_MAX_PIXELS && (int64_t)Q <= PAMR_MAX_ELEMS / ((int64_t)H * W),
             "%s: Q=%d H=%d W=%d is beyond 2^38 pixels or 2^60 elements", who, Q, H, W);
  SG_REQUIRE(dilations, "%s: null pointer (dilations)", who);
  SG_REQUIRE(n_dil >= 1 && n_dil <= PAMR_MAX_DIL, "%s: n_dil=%d outside [1, %d]", who, n_dil, PAMR_MAX_DIL);
  for (int i = 0; i < n_dil; ++i)
    SG_REQUIRE(dilations[i] >= 1 && dilations[i] <= PAMR_MAX_D, "%s: dilation %d is %d, outside [1, %d]", who, i, dilations[i], PAMR_MAX_D);
  return SG_OK;
}

static PamrDil pamr_dil(const int* dilations, int n_dil) {
  PamrDil d;
  for (int i = 0; i < PAMR_MAX_DIL; ++i) d.d[i] = i < n_dil ? dilations[i] : 1;
  return d;
}

static unsigned pamr_grid(int H, int W) { return (unsigned)cdiv((int64_t)H * W, 256); }      // below 2^31: PAMR_MAX_PIXELS

static size_t pamr_weight_bytes(int H, int W, int n_dil) { return align_up((size_t)8 * n_dil * H * W * sizeof(float), 256); }

template <int D>
static int pamr_launch_affinity(const float* g, int H, int W, const PamrDil& dil, float* w, hipStream_t s) {
  hipLaunchKernelGGL(pamr_affinity_kernel<D>, dim3(pamr_grid(H, W)), dim3(256), 0, s, g, H, W, dil, w);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

template <int D>
static int pamr_launch_step(const float* w, const float* in, float* out, int Q, int H, int W, const PamrDil& dil, hipStream_t s) {
  hipLaunchKernelGGL(pamr_step_kernel<D>, dim3(pamr_grid(H, W)), dim3(256), 0, s, w, in, out, Q, H, W, dil);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

static int pamr_affinity(const float* g, int H, int W, const PamrDil& dil, int n_dil, float* w, hipStream_t s) {
#define PAMR_AFF(D) pamr_launch_affinity<D>(g, H, W, dil, w, s)
  switch (n_dil) {
    case 1: return PAMR_AFF(1); case 2: return PAMR_AFF(2); case 3: return PAMR_AFF(3); case 4: return PAMR_AFF(4);
    case 5: return PAMR_AFF(5); case 6: return PAMR_AFF(6); case 7: return PAMR_AFF(7); default: return PAMR_AFF(8);
  }
#undef PAMR_AFF
}

static int pamr_step(const float* w, const float* in, float* out, int Q, int H, int W, const PamrDil& dil, int n_dil, hipStream_t s) {
#define PAMR_STEP(D) pamr_launch_step<D>(w, in, out, Q, H, W, dil, s)
  switch (n_dil) {
    case 1: return PAMR_STEP(1); case 2: return PAMR_STEP(2); case 3: return PAMR_STEP(3); case 4: return PAMR_STEP(4);
    case 5: return PAMR_STEP(5); case 6: return PAMR_STEP(6); case 7: return PAMR_STEP(7); default: return PAMR_STEP(8);
  }
#undef PAMR_STEP
}

}  // namespace sg

using namespace sg;

extern "C" size_t sg_pamr_workspace_bytes(int Q, int H, int W, int n_dil) {
  if (Q < 1 || H < 1 || W < 1 || n_dil < 1 || n_dil > PAMR_MAX_DIL) return 0;
  return pamr_weight_bytes(H, W, n_dil) + (size_t)Q * H * W * sizeof(float);
}

extern "C" int sg_pamr_affinity(const float* guide, int H, int W, const int* dilations, int n_dil, float* weights, sg_stream s) {
  SG_REQUIRE(guide && weights, "sg_pamr_affinity: null pointer");
  SG_TRY(pamr_check_dims("sg_pamr_affinity", 1, H, W, dilations, n_dil));
  return pamr_affinity(guide, H, W, pamr_dil(dilations, n_dil), n_dil, weights, as_stream(s));
}

extern "C" int sg_pamr_step(const float* weights, const float* in, float* out, int Q, int H, int W, const int* dilations, int n_dil,
                            sg_stream s) {
  SG_REQUIRE(weights && in && out, "sg_pamr_step: null pointer");
  SG_REQUIRE(in != out, "sg_pamr_step: in == out (a step reads neighbours that another lane would already have overwritten)");
  SG_TRY(pamr_check_dims("sg_pamr_step", Q, H, W, dilations, n_dil));
  return pamr_step(weights, in, out, Q, H, W, pamr_dil(dilations, n_dil), n_dil, as_stream(s));
}

extern "C" int sg_pamr(const float* guide, float* logits_inout, int Q, int H, int W, const int* dilations, int n_dil, int steps,
                       void* workspace, size_t workspace_bytes, sg_stream s) {
  SG_REQUIRE(guide && logits_inout, "sg_pamr: null pointer");
  SG_TRY(pamr_check_dims("sg_pamr", Q, H, W, dilations, n_dil));
  SG_REQUIRE(steps >= 0 && steps <= PAMR_MAX_STEPS, "sg_pamr: steps=%d outside [0, %d]", steps, PAMR_MAX_STEPS);
  if (steps == 0) return SG_OK;
  const size_t need = sg_pamr_workspace_bytes(Q, H, W, n_dil);
  SG_REQUIRE(workspace, "sg_pamr: null pointer (workspace)");
  SG_REQUIRE((((uintptr_t)workspace) & 255) == 0, "sg_pamr: workspace must be 256-byte aligned");
  if (workspace_bytes < need) return fail(SG_ERR_STATE, "sg_pamr: workspace too small (%zu bytes given, %zu needed)", workspace_bytes, need);
  float* w = reinterpret_cast<float*>(workspace);
  float* tmp = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + pamr_weight_bytes(H, W, n_dil));
  const PamrDil dil = pamr_dil(dilations, n_dil);
  hipStream_t st = as_stream(s);
  SG_TRY(pamr_affinity(guide, H, W, dil, n_dil, w, st));
  float* cur = logits_inout;
  float* nxt = tmp;
  for (int t = 0; t < steps; ++t) {
    SG_TRY(pamr_step(w, cur, nxt, Q, H, W, dil, n_dil, st));
    float* sw = cur; cur = nxt; nxt = sw;
  }
  if (cur != logits_inout)                                              // an odd number of steps ends in the workspace canvas
    SG_HIP(hipMemcpyAsync(logits_inout, cur, (size_t)Q * H * W * sizeof(float), hipMemcpyDeviceToDevice, st));
  return SG_OK;
}
