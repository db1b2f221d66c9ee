// C ABI of libsegearth_hip.so: context / weight packing / the ViT and text forward orchestration.
// Everything here is host code issuing asynchronous launches on the caller's stream.  Device memory is allocated in two places only:
// sg_create / sg_text_create (one arena each, sized from the architecture) and sg_vit_set_tensor (f32 staging copies of the QKV / fc
// weights a LayerNorm will be folded into, freed by sg_vit_finalize or sg_destroy).  No forward allocates.
#include <string>
#include <vector>
#include <mutex>
#include <utility>
#include <math.h>
#include "rowops.h"

namespace sg {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
int fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
  return code;
}

// ---- live kernel timing ------------------------------------------------------------------------------------
struct ProfState {
  bool on = false;
  int cap = 0;
  std::vector<hipEvent_t> start[PROF_NCAT], stop[PROF_NCAT];
  int used[PROF_NCAT] = {};
  double work[PROF_NCAT] = {};
  int64_t dropped[PROF_NCAT] = {};
};
// measurement state belongs to the CALLING THREAD (bench.py enables, launches and reads on one thread): two host threads driving
// two contexts never share it
static thread_local ProfState g_prof;

static std::mutex g_dev_mu;                                        // guards the two per-device caches below
struct LdsOptIn { int dev; const void* kernel; size_t bytes; };
static std::vector<LdsOptIn> g_lds_done;                           // (device, kernel) -> the dynamic-LDS size already opted in to
static std::vector<std::pair<int, int>> g_cu_count;               // (device, compute units)
int ensure_dynamic_lds(const void* kernel, size_t bytes) {
  int dev = 0;
  SG_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_dev_mu);
  LdsOptIn* hit = nullptr;
  for (auto& e : g_lds_done) if (e.dev == dev && e.kernel == kernel) hit = &e;
  if (hit && hit->bytes >= bytes) return SG_OK;                   // a LARGER request than the cached one raises the limit again (jbu_pixel_logits_kernel: size depends on C)
  SG_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (hit) hit->bytes = bytes; else g_lds_done.push_back(LdsOptIn{dev, kernel, bytes});
  return SG_OK;
}
int device_cu_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::lock_guard<std::mutex> lk(g_dev_mu);
  for (const auto& e : g_cu_count) if (e.first == dev) return e.second;
  int n = 256;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) n = prop.multiProcessorCount;
  g_cu_count.emplace_back(dev, n);
  return n;
}
bool prof_on() { return g_prof.on; }
void prof_begin(int cat, double work, hipStream_t s) {
  if (!g_prof.on) return;
  if (g_prof.used[cat] >= g_prof.cap) { g_prof.dropped[cat]++; return; }
  g_prof.work[cat] += work;
  (void)hipEventRecord(g_prof.start[cat][g_prof.used[cat]], s);
}
void prof_end(int cat, hipStream_t s) {
  if (!g_prof.on || g_prof.used[cat] >= g_prof.cap) return;
  (void)hipEventRecord(g_prof.stop[cat][g_prof.used[cat]], s);
  g_prof.used[cat]++;
}

struct LayerW {
  void *w_qkv, *w_out, *w_fc, *w_proj;                 // packed [N_out, K] in the compute dtype
  uint8_t *w_qkv8 = nullptr, *w_fc8 = nullptr, *w_proj8 = nullptr;   // SG_PREC_FP8: e4m3 copies + per-output-channel scales
  float *s_qkv = nullptr, *s_fc = nullptr, *s_proj = nullptr;
  float *b_qkv, *b_out, *b_fc, *b_proj, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  // LayerNorm folded into the GEMMs (2-byte modes without fp8 linears): W' = gamma o W, c = row sums of W', b' = b + W.beta  (rowops.h)
  void *w_qkv_f = nullptr, *w_fc_f = nullptr;
  float *c_qkv = nullptr, *c_fc = nullptr, *bf_qkv = nullptr, *bf_fc = nullptr;
  float *stage_qkv = nullptr, *stage_fc = nullptr;     // f32 copies of the two weights, kept from sg_vit_set_tensor to sg_vit_finalize only
  bool folded = false;
};

// A stack of residual blocks and how it computes: what the vision tower (sg_context) and the text tower (sg_text) both own, and all that
// the block functions (std_block, mlp_block, averaged_attention) see of either.
struct TowerCore {
  int width, heads, mlp_width, n_layers, quick_gelu;
  int device;
  int hk;                                              // HalfKind of the GEMM / attention operands
  bool fp8;                                            // SG_PREC_FP8: bf16 machinery + fp8 linears in the ordinary blocks
  bool ln_fold;                                        // the layers carry folded-LayerNorm operands (vision tower, 2-byte and two-plane modes without fp8)
  size_t esz;                                          // bytes per element of the compute dtype
  void* arena = nullptr; size_t arena_bytes = 0;       // all packed weights
  std::vector<LayerW> layers;
};

static void core_init(TowerCore& c, int device, int width, int heads, int mlp_width, int n_layers, int quick_gelu, int precision, bool ln_fold) {
  c.width = width; c.heads = heads; c.mlp_width = mlp_width; c.n_layers = n_layers; c.quick_gelu = quick_gelu;
  c.device = device; c.hk = hk_of_precision(precision); c.fp8 = precision == SG_PREC_FP8; c.esz = hk_esz(c.hk);
  c.ln_fold = ln_fold && c.hk != HK_F32 && !c.fp8;
}

// the arena layout of the layers (the towers lay their own top-level tensors in front)
static void lay_layers(TowerCore& c, Bump& bb) {
  const size_t e = c.esz; const int D = c.width, M = c.mlp_width;
  c.layers.resize(c.n_layers);
  for (auto& L : c.layers) {
    L.w_qkv = bb.take((size_t)3 * D * D * e); L.w_out = bb.take((size_t)D * D * e);
    L.w_fc = bb.take((size_t)M * D * e); L.w_proj = bb.take((size_t)D * M * e);
    L.b_qkv = bb.get<float>(3 * D); L.b_out = bb.get<float>(D); L.b_fc = bb.get<float>(M); L.b_proj = bb.get<float>(D);
    L.ln1_g = bb.get<float>(D); L.ln1_b = bb.get<float>(D); L.ln2_g = bb.get<float>(D); L.ln2_b = bb.get<float>(D);
    if (c.ln_fold) {
      L.w_qkv_f = bb.take((size_t)3 * D * D * e); L.w_fc_f = bb.take((size_t)M * D * e);
      L.c_qkv = bb.get<float>(3 * D); L.bf_qkv = bb.get<float>(3 * D); L.c_fc = bb.get<float>(M); L.bf_fc = bb.get<float>(M);
    }
    if (c.fp8) {
      L.w_qkv8 = (uint8_t*)bb.take((size_t)3 * D * D); L.w_fc8 = (uint8_t*)bb.take((size_t)M * D); L.w_proj8 = (uint8_t*)bb.take((size_t)D * M);
      L.s_qkv = bb.get<float>(3 * D); L.s_fc = bb.get<float>(M); L.s_proj = bb.get<float>(D);
    }
  }
}

}  // namespace sg

using namespace sg;

struct sg_context {
  sg_vit_desc d;
  TowerCore core;
  int Kpatch, Kpad;
  void* w_patch;                                       // [D, Kpad]
  void* w_projT;                                       // [E, D]
  float *cls_emb, *pos, *lnpre_g, *lnpre_b, *lnpost_g, *lnpost_b;
  std::vector<uint8_t> have;                           // which tensors have arrived: 8 of the tower's own, then 12 per layer
  bool finalized;
};

namespace sg {

// ---- variants of the last-block attention: which (Q,K) terms, summed or not ---------------------------------------
struct Variant { int n_terms, sum_scores, qsel[3], ksel[3]; float scale_mul; int resoftmax; int gauss; };   // sel: 0=q 1=k 2=v; gauss: 1 plain omega, 2 omega*|q||k|*scale
static bool variant_of(int model_type, Variant& v) {
  switch (model_type) {
    case SG_VANILLA:      v = {1, 0, {0, 0, 0}, {1, 0, 0}, 1.f, 0, 0}; return true;
    case SG_CLEARCLIP:    v = {1, 0, {0, 0, 0}, {0, 0, 0}, 1.f, 0, 0}; return true;
    case SG_SCLIP:        v = {2, 0, {0, 1, 0}, {0, 1, 0}, 1.f, 0, 0}; return true;
    case SG_SEGEARTH:     v = {3, 0, {0, 1, 2}, {0, 1, 2}, 1.f, 0, 0}; return true;
    case SG_SFP:          v = {2, 1, {0, 1, 0}, {0, 1, 0}, 0.5f, 0, 0}; return true;
    case SG_EXPERIMENTAL: v = {2, 1, {1, 0, 0}, {1, 0, 0}, 1.f, 1, 0}; return true;
    // Gaussian-window variants (transformer.py:909-932): the similarity map is NOT applied on these paths in the reference
    case SG_NACLIP:       v = {1, 0, {1, 0, 0}, {1, 0, 0}, 1.f, 0, 1}; return true;      // k k^T * scale + omega
    case SG_NONLY:        v = {1, 0, {0, 0, 0}, {1, 0, 0}, 0.f, 0, 2}; return true;      // omega * scale * |q_i| |k_j| only
    case SG_GAV:          v = {1, 0, {0, 0, 0}, {1, 0, 0}, 1.f, 0, 2}; return true;      // q k^T * scale + omega * scale * |q_i| |k_j|
    default: return false;
  }
}

// Generic multi-term attention in either precision.  Element (b, t, h, d) of a Q/K operand lives at
// p + b*sb + t*st + h*dh + d (elements of the compute dtype); V has its own strides.
// f32: materialised scores/probs in `scores`/`probs` ([B*H,N,N] each).  bf16: fused kernel.
struct AttnBuffers { float* scores; float* probs; float* lse; float* lse1; float* omega; float* qnorm; float* knorm; };
struct AttnSpec {
  const void* q[3]; const void* k[3]; int64_t sb, st;
  const void* v; int64_t v_sb, v_st;
  int n_terms, sum_scores, resoftmax, causal;
  float scale; const float* scale_per_image;
  const float* bias; float bias_w; int64_t bias_bstride; const float* bias_rn; const float* bias_cn;
  float out_scale;
  void* ctx; int64_t ctx_sb, ctx_st;
  bool want_lse;
};

static int attn_generic(int hk, const AttnSpec& sp, int B, int N, int H, int dh, const AttnBuffers& buf, hipStream_t s) {
  if (hk != HK_F32) {
    AttnArgs a{};
    for (int t = 0; t < sp.n_terms; ++t) { a.q[t] = (const bf16_t*)sp.q[t]; a.k[t] = (const bf16_t*)sp.k[t]; }
    a.v = (const bf16_t*)sp.v; a.sb = sp.sb; a.st = sp.st; a.v_sb = sp.v_sb; a.v_st = sp.v_st;
    a.n_terms = sp.n_terms; a.sum_scores = sp.sum_scores; a.causal = sp.causal;
    a.B = B; a.N = N; a.H = H; a.dh = dh; a.scale = sp.scale; a.scale_per_image = sp.scale_per_image;
    a.out_scale = sp.out_scale; a.ctx_sb = sp.ctx_sb; a.ctx_st = sp.ctx_st; a.f16 = hk == HK_F16; a.h2 = hk == HK_F16X2;
    if (a.h2) { a.sb *= 2; a.st *= 2; a.v_sb *= 2; a.v_st *= 2; a.ctx_sb *= 2; a.ctx_st *= 2; }   // two-plane f16: the kernel addresses in f16 units
    if (sp.resoftmax) {
      AttnArgs p = a; p.ctx = nullptr; p.bias = nullptr; p.lse_out = buf.lse1; p.resoftmax = 0;
      SG_TRY(attention_bf16(p, s));
      a.resoftmax = 1; a.lse_in = buf.lse1;
    }
    a.bias = sp.bias; a.bias_w = sp.bias_w; a.bias_bstride = sp.bias_bstride; a.bias_rn = sp.bias_rn; a.bias_cn = sp.bias_cn; a.ctx = (bf16_t*)sp.ctx; a.lse_out = sp.want_lse ? buf.lse : nullptr;
    return attention_bf16(a, s);
  }
  const int64_t NN = (int64_t)N * N;
  auto scores_of = [&](int t, bool accumulate) {
    GemmF32Args g{};
    g.A = (const float*)sp.q[t]; g.lda = sp.st; g.sAo = sp.sb; g.sAi = dh;
    g.B = (const float*)sp.k[t]; g.sbk = 1; g.sbn = sp.st; g.sBo = sp.sb; g.sBi = dh;
    g.C = buf.scores; g.ldc = N; g.sCo = (int64_t)H * NN; g.sCi = NN;
    g.residual = accumulate ? buf.scores : nullptr; g.ldr = N;
    g.M = N; g.N = N; g.K = dh; g.batch = B * H; g.inner = H; g.act = 0; g.alpha = 1.f;
    return gemm_f32(g, s);
  };
  const int64_t rows = (int64_t)B * H * N;
  if (sp.sum_scores) {
    for (int t = 0; t < sp.n_terms; ++t) SG_TRY(scores_of(t, t > 0));
    SG_TRY(softmax_rows(buf.scores, N, rows, N, H, sp.scale_per_image, sp.scale, sp.bias, sp.bias_w, sp.bias_bstride, sp.bias_rn, sp.bias_cn, sp.resoftmax ? 1 : 0, 0,
                        buf.probs, sp.want_lse ? buf.lse : nullptr, s));
  } else {
    for (int t = 0; t < sp.n_terms; ++t) {
      SG_TRY(scores_of(t, false));
      SG_TRY(softmax_rows(buf.scores, N, rows, N, H, sp.scale_per_image, sp.scale, sp.bias, sp.bias_w, sp.bias_bstride, sp.bias_rn, sp.bias_cn, 0, t > 0, buf.probs,
                          (sp.want_lse && t == 0) ? buf.lse : nullptr, s, sp.causal));
    }
  }
  GemmF32Args g{};
  g.A = buf.probs; g.lda = N; g.sAo = (int64_t)H * NN; g.sAi = NN;
  g.B = (const float*)sp.v; g.sbk = sp.v_st; g.sbn = 1; g.sBo = sp.v_sb; g.sBi = dh;
  g.C = (float*)sp.ctx; g.ldc = sp.ctx_st; g.sCo = sp.ctx_sb; g.sCi = dh;
  g.M = N; g.N = dh; g.K = N; g.batch = B * H; g.inner = H; g.act = 0; g.alpha = sp.out_scale;
  return gemm_f32(g, s);
}

// Attention over packed qkv [B,N,3D] (compute dtype) -> ctx [B,N,D] (compute dtype).
static int run_attention(int hk, const void* qkv, int B, int N, int D, int H, int model_type, const float* sim, float sim_w,
                         const float* scale_per_image, void* ctx, bool want_lse, const AttnBuffers& buf, hipStream_t s, bool causal = false) {
  const int dh = D / H;
  Variant v;
  if (!variant_of(model_type, v)) return fail(SG_ERR_INVALID, "attention variant %d is not built (NACLIP / NOnly / GAV: SURVEY.md §8f rank 3)", model_type);
  const size_t e = hk_esz(hk);
  AttnSpec sp{};
  for (int t = 0; t < v.n_terms; ++t) { sp.q[t] = (const char*)qkv + (size_t)v.qsel[t] * D * e; sp.k[t] = (const char*)qkv + (size_t)v.ksel[t] * D * e; }
  sp.v = (const char*)qkv + (size_t)2 * D * e;
  sp.st = sp.v_st = 3 * (int64_t)D; sp.sb = sp.v_sb = (int64_t)N * 3 * D;
  sp.n_terms = v.n_terms; sp.sum_scores = v.sum_scores; sp.resoftmax = v.resoftmax; sp.causal = causal ? 1 : 0;
  sp.scale = v.scale_mul / sqrtf((float)dh); sp.scale_per_image = scale_per_image;
  sp.bias = sim; sp.bias_w = sim_w; sp.bias_bstride = (int64_t)(N - 1) * (N - 1); sp.out_scale = 1.f;
  if (v.gauss) {
    const int gside = (int)lroundf(sqrtf((float)(N - 1)));                 // the reference assumes a square grid here (transformer.py:912)
    SG_REQUIRE(gside * gside == N - 1, "Gaussian-window attention needs a square patch grid (N-1 = %d)", N - 1);
    SG_REQUIRE(buf.omega && buf.qnorm && buf.knorm, "Gaussian-window attention: scratch missing");
    SG_TRY(gaussian_bias(gside, gside, 1.0f, buf.omega, s));
    sp.bias = buf.omega; sp.bias_bstride = 0; sp.bias_w = 1.f;
    if (v.gauss == 2) {
      SG_TRY(head_norms(sp.q[0], hk, sp.sb, sp.st, B, N, H, dh, buf.qnorm, s));
      SG_TRY(head_norms(sp.k[0], hk, sp.sb, sp.st, B, N, H, dh, buf.knorm, s));
      sp.bias_rn = buf.qnorm; sp.bias_cn = buf.knorm; sp.bias_w = 1.0f / sqrtf((float)dh);
    }
  }
  sp.ctx = ctx; sp.ctx_sb = (int64_t)N * D; sp.ctx_st = D; sp.want_lse = want_lse;
  return attn_generic(hk, sp, B, N, H, dh, buf, s);
}

// The fields every 2-byte / two-plane / fp8 GEMM call shares: C = act(A . W^T + bias) (+ residual), A [M,K] (ld lda), W [N,K] packed, residual
// on C's leading dimension, alpha = 1, `batch` contiguous problems.  The special forms below add only what is theirs.
static GemmBf16Args gemm_args(int hk, const void* A, int64_t lda, const void* W, const float* bias, const float* residual, void* C, int64_t ldc,
                              bool c_f32, int M, int N, int K, int act, int batch = 1) {
  GemmBf16Args g{};
  g.A = (const bf16_t*)A; g.lda = lda; g.W = (const bf16_t*)W; g.ldw = K; g.bias = bias; g.residual = residual; g.ldr = ldc;
  g.C = C; g.ldc = ldc; g.c_is_bf16 = c_f32 ? 0 : 1; g.M = M; g.N = N; g.K = K; g.batch = batch; g.act = act; g.alpha = 1.f;
  if (batch > 1) { g.strideA = (int64_t)M * lda; g.strideW = (int64_t)N * K; g.strideC = (int64_t)M * ldc; }
  g.f16 = hk == HK_F16; g.h2 = hk == HK_F16X2;
  return g;
}
// y = act(A . W^T + bias) (+ residual) in the context's compute dtype; c_f32 forces an f32 C.
// batch > 1 (2-byte / two-plane only): `batch` contiguous problems, strides M lda / N K / M ldc elements (the residual shares C's).
static int linear(int hk, const void* A, int64_t lda, const void* W, const float* bias, const float* residual, void* C,
                  int64_t ldc, bool c_f32, int M, int N, int K, int act, hipStream_t s, int batch = 1) {
  if (hk != HK_F32) return gemm_bf16(gemm_args(hk, A, lda, W, bias, residual, C, ldc, c_f32, M, N, K, act, batch), s);
  GemmF32Args g{};
  g.A = (const float*)A; g.lda = lda; g.B = (const float*)W; g.sbk = 1; g.sbn = K; g.bias = bias; g.residual = residual; g.ldr = ldc;
  g.C = (float*)C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.batch = 1; g.inner = 1; g.act = act; g.alpha = 1.f;
  return gemm_f32(g, s);
}
// The two GEMM forms a folded LayerNorm is made of (2-byte modes, persistent kernel; GemmBf16Args::copy16 / ln_stats):
//   producer: C (f32) = A.W^T + bias (+ residual), plus its 2-byte copy `copy16` [M, N] and the slice statistics of the finished rows
//   consumer: C (2-byte) = act(rstd (A.W'^T - mean c) + b') with (mean, rstd) per row
static int linear_ln_producer(int hk, const void* A, int64_t lda, const void* W, const float* bias, const float* residual, float* C, int64_t ldc,
                              void* copy16, float* slice_stats, int M, int N, int K, hipStream_t s) {
  GemmBf16Args g = gemm_args(hk, A, lda, W, bias, residual, C, ldc, true, M, N, K, ACT_NONE);
  g.copy16 = copy16; g.ld16 = N; g.row_stats = slice_stats;
  return gemm_bf16(g, s);
}
static int linear_ln_consumer(int hk, const void* A, int64_t lda, const void* Wf, const float* bias_f, const float* c_vec, const float* mean_rstd,
                              void* C, int64_t ldc, int M, int N, int K, int act, hipStream_t s) {
  GemmBf16Args g = gemm_args(hk, A, lda, Wf, bias_f, nullptr, C, ldc, false, M, N, K, act);
  g.ln_stats = mean_rstd; g.ln_c = c_vec;
  return gemm_bf16(g, s);
}

// C = act((A8 . W8^T) * sa[m] * sw[n] + bias) (+ residual): fp8 e4m3 operands, f32 accumulate.
// The MX forms (GemmBf16Args::a_mx / c_mx): A8 with E8M0 block scales a_mx [K/128][M][4] instead of row scales, and / or the output written as
// e4m3 [M,N] + block scales c_mx_scale [N/128][M][4] (then C is unused).
static int linear_fp8_mx(const uint8_t* A8, const float* sa, const uint8_t* a_mx, int64_t lda, const uint8_t* W8, const float* sw, const float* bias,
                         const float* residual, void* C, int64_t ldc, bool c_f32, uint8_t* c_mx, uint8_t* c_mx_scale, int M, int N, int K, int act,
                         hipStream_t s) {
  GemmBf16Args g = gemm_args(HK_BF16, A8, lda, W8, bias, residual, c_mx ? (void*)c_mx : C, ldc, c_f32 && !c_mx, M, N, K, act);
  g.fp8 = 1; g.row_scale = sa; g.col_scale = sw; g.a_mx = a_mx; g.c_mx = c_mx; g.c_mx_scale = c_mx_scale;
  return gemm_bf16(g, s);
}
static int linear_fp8(const uint8_t* A8, const float* sa, int64_t lda, const uint8_t* W8, const float* sw, const float* bias,
                      const float* residual, void* C, int64_t ldc, bool c_f32, int M, int N, int K, int act, hipStream_t s) {
  return linear_fp8_mx(A8, sa, nullptr, lda, W8, sw, bias, residual, C, ldc, c_f32, nullptr, nullptr, M, N, K, act, s);
}

__global__ void zero_diag_kernel(float* sim, int n, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) sim[(i / n) * (int64_t)n * n + (i % n) * (int64_t)(n + 1)] = 0.f;
}
// `kind` = HalfKind of src (two-plane f16: a contiguous buffer whose rows are multiples of 8 elements, so flat index = element index)
__global__ void unpack_bf16_kernel(const bf16_t* src, float* dst, int64_t n, int kind) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = kind == HK_F16X2 ? ld_elem<h2_t>(reinterpret_cast<const h2_t*>(src), i) : kind == HK_F16 ? h2f(f16_t{src[i]}) : bf2f(src[i]);
}

// similarity map from L2-normalised patch rows xhat [B,n,D] (compute dtype) -> sim [B,n,n] f32
static int similarity_from_xhat(int hk, const void* xhat, int B, int n, int D, float temperature, int add_self, float* sim, hipStream_t s) {
  if (hk != HK_F32) {
    GemmBf16Args g = gemm_args(hk, xhat, D, xhat, nullptr, nullptr, sim, n, true, n, n, D, ACT_NONE, B);
    g.alpha = 1.0f / temperature; g.strideA = g.strideW = (int64_t)n * D; g.strideC = (int64_t)n * n;   // strides also for B == 1
    SG_TRY(gemm_bf16(g, s));
  } else {
    GemmF32Args g{};
    g.A = (const float*)xhat; g.lda = D; g.sAo = (int64_t)n * D; g.B = (const float*)xhat; g.sbk = 1; g.sbn = D; g.sBo = (int64_t)n * D;
    g.C = sim; g.ldc = n; g.sCo = (int64_t)n * n; g.M = n; g.N = n; g.K = D; g.batch = B; g.inner = 1; g.act = 0; g.alpha = 1.0f / temperature;
    SG_TRY(gemm_f32(g, s));
  }
  if (!add_self) {
    const int64_t total = (int64_t)B * n;
    hipLaunchKernelGGL(zero_diag_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, sim, n, total);
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}

// ---- workspace of one forward (laid out by the same function for the size query and the forward itself) ------------------------------
// What a residual block touches; either tower's plan holds one and the block functions take nothing else of the workspace.
struct BlockScratch {
  void *xn, *qkv, *ctx, *hbuf;
  float *lse, *lse1, *scores, *probs;
  float *ln_slice, *ln_rows;                              // folded LayerNorm: slice statistics [D/64][R][2] (slice-major) written by the producing GEMM, (mean, rstd) [R][2]
  uint8_t* hmx;                                           // SG_PREC_FP8: MX block scales of h8 ([M/128][R][4] E8M0), written by the fc GEMM's epilogue
  uint8_t *x8, *h8; float *sx8, *sh8;                     // SG_PREC_FP8: quantised LN output / GELU output + per-row scales
  float *attn_cls, *attn_diag;
  float *attn_avg, *sa_tmp, *sa_qk32, *sa_scores, *sa_probs;   // self-attention enhancement, mode='attention'; layer fusion
  float *omega, *qnorm, *knorm;
};
struct Plan {
  BlockScratch blk;
  void *patchA; float* patchOut; float* pos_r; float* x; void* xhat; float* sim;
  float *out_last, *y; int32_t *idx_out, *idx_sa; void* refine_scratch;
  float *lf_acc;                                              // layer fusion: the EMA of the head-averaged attention maps [B,N,N]
  // GEM
  float* x_gem; void* gnorm[3]; void* gatt[3]; float* inv_temp; float* gem_out; void* ctx2;
};

static size_t plan(const sg_context* c, int B, int gh, int gw, const sg_forward_opts* o, void* ws, bool dry, Plan& p) {
  const sg_vit_desc& d = c->d;
  const TowerCore& core = c->core;
  const int n = gh * gw, N = n + 1;
  const int64_t R = (int64_t)B * N;
  const size_t e = core.esz;
  p = Plan{};                                             // what a forward does not need stays null
  BlockScratch& k = p.blk;
  Bump b(ws, 0, dry);
  p.patchA = b.take((size_t)B * n * c->Kpad * e);
  p.patchOut = b.get<float>((size_t)B * n * d.width);
  p.pos_r = b.get<float>((size_t)N * d.width);
  p.x = b.get<float>(R * d.width);
  k.xn = b.take(R * d.width * e);
  k.qkv = b.take(R * 3 * d.width * e);
  k.ctx = b.take(R * d.width * e);
  k.hbuf = b.take(R * d.mlp_width * e);
  if (core.hk != HK_F32 && !core.fp8 && d.width % 64 == 0) { k.ln_slice = b.get<float>(R * (d.width / 64) * 2); k.ln_rows = b.get<float>(R * 2); }
  if (core.fp8) {
    k.x8 = (uint8_t*)b.take(R * d.width); k.sx8 = b.get<float>(R);
    k.h8 = (uint8_t*)b.take(R * d.mlp_width); k.sh8 = b.get<float>(R);
    k.hmx = (uint8_t*)b.take(R * (d.mlp_width / 32 + 4));
  }
  if (o->similarity_enabled) { p.xhat = b.take((size_t)B * n * d.width * e); p.sim = b.get<float>((size_t)B * n * n); }
  k.lse = b.get<float>((size_t)B * d.heads * N);
  k.lse1 = b.get<float>((size_t)B * d.heads * N);
  k.attn_cls = b.get<float>((size_t)B * N);
  k.attn_diag = b.get<float>((size_t)B * N);
  p.out_last = b.get<float>(R * d.width);
  p.y = b.get<float>(R * d.embed_dim);
  const int k_out = o->outlier_enabled ? (o->outlier_top_k < n ? o->outlier_top_k : n) : 0;
  const int k_sa = (o->outlier_enabled && o->selfattn_enabled) ? (o->selfattn_top_k < n ? o->selfattn_top_k : n) : 0;
  p.idx_out = b.get<int32_t>((size_t)B * (k_out > 0 ? k_out : 1));
  p.idx_sa = b.get<int32_t>((size_t)B * (k_sa > 0 ? k_sa : 1));
  const int kmax = k_out > k_sa ? k_out : k_sa;
  p.refine_scratch = b.take(refine_scratch_bytes(B, d.width, kmax > 0 ? kmax : 1));
  if (core.hk == HK_F32) { k.scores = b.get<float>((size_t)B * d.heads * N * N); k.probs = b.get<float>((size_t)B * d.heads * N * N); }
  if (o->layer_fusion_enabled) p.lf_acc = b.get<float>((size_t)B * N * N);
  if (o->layer_fusion_enabled || (o->outlier_enabled && o->selfattn_enabled && o->selfattn_mode == 1)) {
    k.attn_avg = b.get<float>((size_t)B * N * N); k.sa_tmp = b.get<float>(R * d.width);
    if (core.hk != HK_F32) {                            // one image at a time: f32 copies of q|k, scores and probabilities of all heads
      k.sa_qk32 = b.get<float>((size_t)N * 2 * d.width); k.sa_scores = b.get<float>((size_t)d.heads * N * N); k.sa_probs = b.get<float>((size_t)d.heads * N * N);
    }
  }
  if (o->model_type == SG_NACLIP || o->model_type == SG_NONLY || o->model_type == SG_GAV) {
    k.omega = b.get<float>((size_t)n * n); k.qnorm = b.get<float>((size_t)B * d.heads * N); k.knorm = b.get<float>((size_t)B * d.heads * N);
  }
  if (o->model_type == SG_GEM) {
    p.x_gem = b.get<float>(R * d.width);
    p.gem_out = b.get<float>(R * d.width);
    for (int t = 0; t < 3; ++t) { p.gnorm[t] = b.take(R * d.width * e); p.gatt[t] = b.take(R * d.width * e); }
    p.ctx2 = b.take(R * d.width * e);
    p.inv_temp = b.get<float>(B);
  }
  return align_up(b.off, 256);
}

static int find_layer_tensor(const char* rest, int& slot) {
  static const char* names[12] = {"ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                                  "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias",
                                  "mlp.c_proj.weight", "mlp.c_proj.bias"};
  for (int i = 0; i < 12; ++i) if (!strcmp(rest, names[i])) { slot = i; return 1; }
  return 0;
}

// One f32 device tensor on its way into a tower: `api` is the entry point the caller used (error texts name it).
struct TensorSrc { const char* api; const char* name; const float* src; int64_t numel; int hk; hipStream_t s; };
static int copy_f32(const TensorSrc& t, float* dst, int64_t n) {
  SG_REQUIRE(t.numel == n, "%s(%s): expected %lld elements, got %lld", t.api, t.name, (long long)n, (long long)t.numel);
  SG_HIP(hipMemcpyAsync(dst, t.src, (size_t)n * 4, hipMemcpyDeviceToDevice, t.s));
  return SG_OK;
}
static int pack_w(const TensorSrc& t, void* dst, int rows, int cols, int cols_pad) {
  SG_REQUIRE(t.numel == (int64_t)rows * cols, "%s(%s): expected %lld elements, got %lld", t.api, t.name, (long long)rows * cols, (long long)t.numel);
  return pack_rows(t.src, rows, cols, cols, dst, cols_pad, t.hk, t.s);
}
// transformer.resblocks.<i>.<name> of either tower: copy or pack, quantise for the fp8 linears, stage the weights a LayerNorm will be folded
// into (sg_vit_finalize), invalidate the block's folded operands.  slot = 12 i + index of <name>, or -1 when the name is not a layer tensor.
static int set_layer_tensor(TowerCore& c, const TensorSrc& t, int& slot) {
  const int D = c.width, M = c.mlp_width;
  int li = -1, consumed = 0, k;
  slot = -1;
  if (sscanf(t.name, "transformer.resblocks.%d.%n", &li, &consumed) != 1 || consumed <= 0 || li < 0 || li >= c.n_layers ||
      !find_layer_tensor(t.name + consumed, k)) return SG_OK;
  LayerW& L = c.layers[li];
  slot = li * 12 + k;
  auto quant = [&](uint8_t* w8, float* scale, int rows, int cols) -> int {   // SG_PREC_FP8: e4m3 copy + per-output-channel scales
    return c.fp8 ? quantize_rows_fp8(t.src, 0, cols, w8, cols, scale, rows, cols, t.s) : SG_OK;
  };
  auto stage = [&](float*& dst, int64_t n) -> int {        // f32 copy of a weight the LayerNorm in front of it will be folded into
    if (!L.w_qkv_f || t.numel != n) return SG_OK;
    if (!dst) SG_HIP(hipMalloc((void**)&dst, (size_t)n * 4));
    SG_HIP(hipMemcpyAsync(dst, t.src, (size_t)n * 4, hipMemcpyDeviceToDevice, t.s));
    return SG_OK;
  };
  if (k <= 3 || (k >= 6 && k <= 9)) L.folded = false;      // anything the folded operands are made from
  switch (k) {
    case 0: return copy_f32(t, L.ln1_g, D);
    case 1: return copy_f32(t, L.ln1_b, D);
    case 2: SG_TRY(pack_w(t, L.w_qkv, 3 * D, D, D)); SG_TRY(quant(L.w_qkv8, L.s_qkv, 3 * D, D)); return stage(L.stage_qkv, (int64_t)3 * D * D);
    case 3: return copy_f32(t, L.b_qkv, 3 * D);
    case 4: return pack_w(t, L.w_out, D, D, D);
    case 5: return copy_f32(t, L.b_out, D);
    case 6: return copy_f32(t, L.ln2_g, D);
    case 7: return copy_f32(t, L.ln2_b, D);
    case 8: SG_TRY(pack_w(t, L.w_fc, M, D, D)); SG_TRY(quant(L.w_fc8, L.s_fc, M, D)); return stage(L.stage_fc, (int64_t)M * D);
    case 9: return copy_f32(t, L.b_fc, M);
    case 10: SG_TRY(pack_w(t, L.w_proj, D, M, M)); return quant(L.w_proj8, L.s_proj, D, M);
    default: return copy_f32(t, L.b_proj, D);
  }
}

}  // namespace sg

extern "C" const char* sg_last_error(void) { return g_err; }
extern "C" int sg_version(void) { return 100; }

// Live timing for bench.py: HIP events bracket every launch of a kernel family on the stream it is launched on.
extern "C" int sg_profile_enable(int capacity) {
  SG_REQUIRE(capacity > 0 && capacity <= (1 << 20), "sg_profile_enable: bad capacity");
  if (capacity > g_prof.cap) {
    for (int c = 0; c < PROF_NCAT; ++c) {
      g_prof.start[c].resize(capacity); g_prof.stop[c].resize(capacity);
      for (int i = g_prof.cap; i < capacity; ++i) { SG_HIP(hipEventCreate(&g_prof.start[c][i])); SG_HIP(hipEventCreate(&g_prof.stop[c][i])); }
    }
    g_prof.cap = capacity;
  }
  for (int c = 0; c < PROF_NCAT; ++c) { g_prof.used[c] = 0; g_prof.work[c] = 0; g_prof.dropped[c] = 0; }
  g_prof.on = true;
  return SG_OK;
}
// Raw bf16 GEMM on caller-packed operands (A [M,K], W [N,K] bf16, K % 64 == 0): C = act(A.W^T + bias) (+ residual).
extern "C" int sg_gemm_bf16_raw(const void* A, const void* W, const float* bias, const float* residual, void* C, int M, int N, int K,
                                int act, int c_is_bf16, sg_stream st) {
  SG_REQUIRE(A && W && C, "sg_gemm_bf16_raw: null pointer");
  return linear(HK_BF16, A, K, W, bias, residual, C, N, !c_is_bf16, M, N, K, act, as_stream(st));
}
// The same for every 2-byte / two-plane storage (SG_PREC_BF16 / F16 / F16X2: A [batch][M][K], W [batch][N][K] in the precision's operand
// storage, two-plane as common.h's 32-byte groups; K % 64 == 0, two-plane K % 32 == 0), C f32 or (c_packed) that storage, `batch` contiguous problems.
extern "C" int sg_gemm_raw(int precision, const void* A, const void* W, const float* bias, const float* residual, void* C, int M, int N, int K,
                           int batch, int act, int c_packed, sg_stream st) {
  SG_REQUIRE(A && W && C, "sg_gemm_raw: null pointer");
  SG_REQUIRE(precision == SG_PREC_BF16 || precision == SG_PREC_F16 || precision == SG_PREC_F16X2, "sg_gemm_raw: bad precision %d", precision);
  SG_REQUIRE(batch >= 1 && (c_packed == 0 || c_packed == 1), "sg_gemm_raw: bad batch %d / c_packed %d", batch, c_packed);
  return linear(hk_of_precision(precision), A, K, W, bias, residual, C, N, !c_packed, M, N, K, act, as_stream(st), batch);
}
// fp8 (OCP e4m3) GEMM on caller-quantised operands: A8 [M,K] with per-row scales sa [M], W8 [N,K] with per-row scales sw [N], K % 128 == 0.
extern "C" int sg_gemm_fp8_raw(const void* A8, const float* sa, const void* W8, const float* sw, const float* bias, const float* residual,
                               void* C, int M, int N, int K, int act, int c_is_bf16, sg_stream st) {
  SG_REQUIRE(A8 && W8 && sa && sw && C, "sg_gemm_fp8_raw: null pointer");
  return linear_fp8((const uint8_t*)A8, sa, K, (const uint8_t*)W8, sw, bias, residual, C, N, !c_is_bf16, M, N, K, act, as_stream(st));
}
// The MXFP8 forms of the fp8 GEMM (M >= 1024, N >= 256, N % 128 == 0 when c_mx): exactly one of sa (per-row scales) / a_mx (E8M0 block scales,
// [K/128][M][4] bytes) describes A8; when c_mx is given the result is written as e4m3 [M,N] + block scales c_mx_scale [N/128][M][4] and C is unused.
extern "C" int sg_gemm_fp8_mx_raw(const void* A8, const float* sa, const void* a_mx, const void* W8, const float* sw, const float* bias,
                                  const float* residual, void* C, void* c_mx, void* c_mx_scale, int M, int N, int K, int act, int c_is_bf16, sg_stream st) {
  // one of sa / a_mx and c_mx_scale with c_mx: gemm_fp8's own checks, behind the reset of the launch record (a refused call reads "none")
  SG_REQUIRE(A8 && W8 && sw && (C || c_mx), "sg_gemm_fp8_mx_raw: null pointer");
  return linear_fp8_mx((const uint8_t*)A8, sa, (const uint8_t*)a_mx, K, (const uint8_t*)W8, sw, bias, residual, C, N, !c_is_bf16, (uint8_t*)c_mx,
                       (uint8_t*)c_mx_scale, M, N, K, act, as_stream(st));
}
// rows of f32 -> e4m3 + per-row absmax scale (scale[r] = max|x[r,:]| / 448), the quantiser both fp8 operands go through
extern "C" int sg_quantize_rows_fp8(const float* x, int64_t rows, int D, void* y, float* scale, sg_stream st) {
  SG_REQUIRE(x && y && scale && rows > 0 && D > 0, "sg_quantize_rows_fp8: bad arguments");
  return quantize_rows_fp8(x, 0, D, (uint8_t*)y, D, scale, rows, D, as_stream(st));
}
// Tuning hook (-1 = automatic, common.h Tuning for the codes); an unknown code is refused and leaves the setting as it was.
extern "C" int sg_set_gemm_config(int cfg) { return set_gemm_config(cfg); }
extern "C" int sg_profile_disable(void) { g_prof.on = false; return SG_OK; }
// K step in elements (64: gemm_bf16_persist_k64, 32: gemm_bf16_persist) of the calling thread's last persistent bf16 / f16 GEMM launch; 0 = none yet.
extern "C" int sg_gemm_persist_last_kstep(void) { return gemm_persist_last_kstep(); }
// "<family> grid=<x> ngroup=<n>" of the calling thread's last GEMM launch through the 2-byte / two-plane / fp8 GEMM entry (thread-local text).
extern "C" const char* sg_gemm_last_kernel(void) { return gemm_last_kernel(); }
// The fused attention on caller-packed operands: AttnArgs as they are, strides in elements (doubled here for two-plane storage, as
// attn_generic does).  One attention_bf16() call: every check runs before the first HIP call, so a refused call launches nothing.
extern "C" int sg_attention_raw(int precision, const void* q0, const void* q1, const void* q2, const void* k0, const void* k1, const void* k2,
                                int64_t sb, int64_t st, const void* v, int64_t v_sb, int64_t v_st, int B, int N, int H, int dh, int n_terms,
                                int sum_scores, int causal, float scale, const float* scale_per_image, const float* bias, float bias_w,
                                int64_t bias_bstride, const float* bias_rn, const float* bias_cn, int resoftmax, const float* lse_in, float* lse_out,
                                void* ctx, int64_t ctx_sb, int64_t ctx_st, float out_scale, sg_stream st_) {
  SG_REQUIRE(precision == SG_PREC_BF16 || precision == SG_PREC_F16 || precision == SG_PREC_F16X2, "sg_attention_raw: bad precision %d", precision);
  SG_REQUIRE(n_terms >= 1 && n_terms <= 3, "attention: n_terms=%d", n_terms);
  const void* qs[3] = {q0, q1, q2};
  const void* ks[3] = {k0, k1, k2};
  const void* ptrs[7] = {qs[0], ks[0], qs[1], ks[1], qs[2], ks[2], ctx ? v : nullptr};
  for (int i = 0; i < 7; ++i) {
    const bool need = i < 2 * n_terms || (i == 6 && ctx);
    SG_REQUIRE(!need || ptrs[i], "sg_attention_raw: null operand pointer");
    SG_REQUIRE(((uintptr_t)ptrs[i] & 15) == 0, "sg_attention_raw: operands must be 16-byte aligned");
  }
  SG_REQUIRE(((uintptr_t)ctx & 7) == 0 && ctx_sb % 4 == 0 && ctx_st % 4 == 0, "sg_attention_raw: ctx must be 8-byte aligned (strides multiples of 4)");
  AttnArgs a{};
  for (int t = 0; t < n_terms; ++t) { a.q[t] = (const bf16_t*)qs[t]; a.k[t] = (const bf16_t*)ks[t]; }
  a.v = (const bf16_t*)v; a.sb = sb; a.st = st; a.v_sb = v_sb; a.v_st = v_st;
  a.n_terms = n_terms; a.sum_scores = sum_scores; a.causal = causal;
  a.B = B; a.N = N; a.H = H; a.dh = dh; a.scale = scale; a.scale_per_image = scale_per_image;
  a.bias = bias; a.bias_w = bias_w; a.bias_bstride = bias_bstride; a.bias_rn = bias_rn; a.bias_cn = bias_cn;
  a.resoftmax = resoftmax; a.lse_in = lse_in; a.lse_out = lse_out;
  a.ctx = (bf16_t*)ctx; a.ctx_sb = ctx_sb; a.ctx_st = ctx_st; a.out_scale = out_scale;
  a.f16 = precision == SG_PREC_F16; a.h2 = precision == SG_PREC_F16X2;
  if (a.h2) { a.sb *= 2; a.st *= 2; a.v_sb *= 2; a.v_st *= 2; a.ctx_sb *= 2; a.ctx_st *= 2; }
  return attention_bf16(a, as_stream(st_));
}
// attention_stats() on caller-packed q | k rows (k D = H dh elements after q in a row; element strides sb / st) and a given lse [B,H,N].
extern "C" int sg_attention_stats_raw(int precision, const void* qk, int64_t sb, int64_t st, const float* lse, int B, int N, int H, int dh,
                                      float scale, float* attn_cls, float* attn_diag, sg_stream st_) {
  SG_REQUIRE(precision == SG_PREC_BF16 || precision == SG_PREC_F16 || precision == SG_PREC_F16X2, "sg_attention_stats_raw: bad precision %d", precision);
  SG_REQUIRE(qk && lse && attn_cls && attn_diag, "sg_attention_stats_raw: null pointer");
  SG_REQUIRE(B > 0 && B < 65536 && N > 0 && H > 0 && dh > 0, "sg_attention_stats_raw: bad shape");
  return attention_stats(qk, hk_of_precision(precision), sb, st, lse, B, N, H, dh, scale, attn_cls, attn_diag, as_stream(st_));
}
// ---- raw test entries of the row kernels (rowops.hip) and patchify: one host function each, arguments passed one to one ---------------
// `kind` arguments are sg_precision values naming a storage: SG_PREC_F32, SG_PREC_BF16, SG_PREC_F16, SG_PREC_F16X2 (two-plane groups).
static int raw_kind(const char* api, int p, int* hk) {
  SG_REQUIRE(p == SG_PREC_F32 || p == SG_PREC_BF16 || p == SG_PREC_F16 || p == SG_PREC_F16X2, "%s: bad kind %d", api, p);
  *hk = hk_of_precision(p);
  return SG_OK;
}
extern "C" int sg_layernorm_raw(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy, int out_kind,
                                int64_t rows, int D, float eps, sg_stream st) {
  SG_REQUIRE(x && gamma && beta && y, "sg_layernorm_raw: null pointer");
  int hk; SG_TRY(raw_kind("sg_layernorm_raw", out_kind, &hk));
  return layernorm(x, ldx, gamma, beta, y, ldy, hk, rows, D, eps, as_stream(st));
}
extern "C" int sg_layernorm_fp8_raw(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy, float* scale,
                                    int64_t rows, int D, float eps, sg_stream st) {
  SG_REQUIRE(x && gamma && beta && y && scale, "sg_layernorm_fp8_raw: null pointer");
  return layernorm_fp8(x, ldx, gamma, beta, (uint8_t*)y, ldy, scale, rows, D, eps, as_stream(st));
}
extern "C" int sg_quantize_rows_raw(const void* x, int in_kind, int64_t ldx, void* y, int64_t ldy, float* scale, int64_t rows, int D,
                                    sg_stream st) {
  SG_REQUIRE(x && y && scale, "sg_quantize_rows_raw: null pointer");
  SG_REQUIRE(in_kind == SG_PREC_F32 || in_kind == SG_PREC_BF16 || in_kind == SG_PREC_F16, "sg_quantize_rows_raw: bad kind %d", in_kind);
  return quantize_rows_fp8(x, hk_of_precision(in_kind), ldx, (uint8_t*)y, ldy, scale, rows, D, as_stream(st));
}
extern "C" int sg_embed_assemble_raw(const float* patches, int64_t ldp, const float* cls_emb, const float* pos, const float* gamma,
                                     const float* beta, float* x, int B, int N, int D, float eps, sg_stream st) {
  SG_REQUIRE(patches && cls_emb && pos && gamma && beta && x, "sg_embed_assemble_raw: null pointer");
  return embed_assemble(patches, ldp, cls_emb, pos, gamma, beta, x, B, N, D, eps, as_stream(st));
}
extern "C" int sg_posembed_resize_raw(const float* pos, int g0, int D, int gh, int gw, int antialias, float* out, sg_stream st) {
  SG_REQUIRE(pos && out, "sg_posembed_resize_raw: null pointer");
  return posembed_resize(pos, g0, D, gh, gw, antialias, out, as_stream(st));
}
extern "C" int sg_pack_rows_raw(const float* src, int64_t rows, int cols, int64_t ld_src, void* dst, int cols_pad, int kind, sg_stream st) {
  SG_REQUIRE(src && dst, "sg_pack_rows_raw: null pointer");
  int hk; SG_TRY(raw_kind("sg_pack_rows_raw", kind, &hk));
  return pack_rows(src, rows, cols, ld_src, dst, cols_pad, hk, as_stream(st));
}
extern "C" int sg_transpose_pack_raw(const float* src, int rows, int cols, void* dst, int kind, sg_stream st) {
  SG_REQUIRE(src && dst, "sg_transpose_pack_raw: null pointer");
  int hk; SG_TRY(raw_kind("sg_transpose_pack_raw", kind, &hk));
  return transpose_pack(src, rows, cols, dst, hk, as_stream(st));
}
extern "C" int sg_ln_stats_finalize_raw(const float* slice_stats, int64_t rows, int D, float eps, float* mean_rstd, sg_stream st) {
  SG_REQUIRE(slice_stats && mean_rstd, "sg_ln_stats_finalize_raw: null pointer");
  return ln_stats_finalize(slice_stats, rows, D, eps, mean_rstd, as_stream(st));
}
extern "C" int sg_fold_ln_weight_raw(const float* W, int N, int K, const float* gamma, const float* beta, const float* bias, int precision,
                                     void* Wp, float* c, float* bias_f, sg_stream st) {
  SG_REQUIRE(W && gamma && beta && Wp && c && bias_f, "sg_fold_ln_weight_raw: null pointer");
  int hk; SG_TRY(raw_kind("sg_fold_ln_weight_raw", precision, &hk));
  return fold_ln_weight(W, N, K, gamma, beta, bias, hk, Wp, c, bias_f, as_stream(st));
}
extern "C" int sg_l2norm_rows_raw(const void* x, int in_kind, int64_t so, int64_t si, int inner, void* y, int out_kind, int64_t yo, int64_t yi,
                                  int64_t rows, int D, float eps, sg_stream st) {
  SG_REQUIRE(x && y, "sg_l2norm_rows_raw: null pointer");
  SG_REQUIRE(inner >= 1, "sg_l2norm_rows_raw: inner=%d", inner);
  int hx, hy; SG_TRY(raw_kind("sg_l2norm_rows_raw", in_kind, &hx)); SG_TRY(raw_kind("sg_l2norm_rows_raw", out_kind, &hy));
  return l2norm_rows(x, hx, so, si, inner, y, hy, yo, yi, rows, D, eps, as_stream(st));
}
extern "C" int sg_softmax_rows_raw(const float* scores, int64_t ld, int64_t rows, int N, int H, const float* scale_per_image, float scale,
                                   const float* bias, float bias_w, int64_t bias_bstride, const float* bias_rn, const float* bias_cn, int mode,
                                   int accumulate, int causal, float* out, float* lse, sg_stream st) {
  SG_REQUIRE(scores && out, "sg_softmax_rows_raw: null pointer");
  SG_REQUIRE(N >= 1 && H >= 1 && (mode == 0 || mode == 1), "sg_softmax_rows_raw: bad N=%d H=%d mode=%d", N, H, mode);
  return softmax_rows(scores, ld, rows, N, H, scale_per_image, scale, bias, bias_w, bias_bstride, bias_rn, bias_cn, mode, accumulate, out, lse,
                      as_stream(st), causal);
}
extern "C" int sg_gaussian_bias_raw(int gh, int gw, float std, float* omega, sg_stream st) {
  SG_REQUIRE(omega, "sg_gaussian_bias_raw: null pointer");
  SG_REQUIRE(gh >= 1 && gw >= 1, "sg_gaussian_bias_raw: bad grid %d x %d", gh, gw);
  return gaussian_bias(gh, gw, std, omega, as_stream(st));
}
extern "C" int sg_head_norms_raw(const void* x, int kind, int64_t sb, int64_t st, int B, int N, int H, int dh, float* out, sg_stream st_) {
  SG_REQUIRE(x && out, "sg_head_norms_raw: null pointer");
  SG_REQUIRE(B > 0 && B < 65536 && N > 0 && H > 0 && dh > 0, "sg_head_norms_raw: bad shape");
  int hk; SG_TRY(raw_kind("sg_head_norms_raw", kind, &hk));
  return head_norms(x, hk, sb, st, B, N, H, dh, out, as_stream(st_));
}
extern "C" int sg_axpby_raw(float* y, const float* x, float a, float b, int64_t n, sg_stream st) {
  SG_REQUIRE(y && x, "sg_axpby_raw: null pointer");
  return axpby(y, x, a, b, n, as_stream(st));
}
extern "C" int sg_gem_inv_temp_raw(const float* x, int B, int N, int D, float scale, float* out, sg_stream st) {
  SG_REQUIRE(x && out, "sg_gem_inv_temp_raw: null pointer");
  SG_REQUIRE(B > 0 && N > 0 && D > 0, "sg_gem_inv_temp_raw: bad shape");
  return gem_inv_temp(x, B, N, D, scale, out, as_stream(st));
}
extern "C" int sg_patchify_raw(const sg_tile_batch* tiles, int P, int Kpad, void* out, int out_kind, sg_stream st) {
  SG_REQUIRE(tiles && out && tiles->scene && tiles->windows, "sg_patchify_raw: null pointer");
  SG_REQUIRE(P > 0, "sg_patchify_raw: P=%d", P);
  int hk; SG_TRY(raw_kind("sg_patchify_raw", out_kind, &hk));
  return patchify(*tiles, P, out, Kpad, hk, as_stream(st));
}
// "<kernel> ..." of the calling thread's last launch through the fused attention or its statistics (thread-local text).
extern "C" const char* sg_attention_last_kernel(void) { return attention_last_kernel(); }
// which body that launch ran: "dma" / "staged" (the fused attention), "stats", or "none"
extern "C" const char* sg_attention_last_body(void) { return attention_last_body(); }
// category: 0 bf16 GEMM (non-persistent tile variants), 1 fused attention, 2 f32 GEMM, 3 the persistent bf16 GEMM (all instantiations), 4 fp8 GEMM,
// 5 / 6 the persistent GEMM's folded-LayerNorm consumer / producer instantiations alone.  Call after the stream
// has been synchronised.
extern "C" int sg_profile_read(int category, double* total_ms, double* total_flops, int64_t* launches, int64_t* dropped) {
  SG_REQUIRE(category >= 0 && category < PROF_NCAT && total_ms && total_flops && launches, "sg_profile_read: bad argument");
  double ms = 0, work = 0; int64_t n = 0, drop = 0;
  // category 3 = EVERY launch of the persistent kernel: its plain instantiation plus the two folded-LayerNorm ones (5, 6)
  const int members[3] = {category, category == PROF_GEMM_PERSIST ? PROF_GEMM_PERSIST_LN_CONSUMER : -1, category == PROF_GEMM_PERSIST ? PROF_GEMM_PERSIST_LN_PRODUCER : -1};
  for (int c : members) {
    if (c < 0) continue;
    for (int i = 0; i < g_prof.used[c]; ++i) {
      float t = 0.f;
      SG_HIP(hipEventElapsedTime(&t, g_prof.start[c][i], g_prof.stop[c][i]));
      ms += t;
    }
    work += g_prof.work[c]; n += g_prof.used[c]; drop += g_prof.dropped[c];
  }
  *total_ms = ms; *total_flops = work; *launches = n;
  if (dropped) *dropped = drop;
  return SG_OK;
}

extern "C" int sg_create(sg_context** out, int device, const sg_vit_desc* desc) {
  SG_REQUIRE(out && desc, "sg_create: null argument");
  const sg_vit_desc& d = *desc;
  SG_REQUIRE(d.width > 0 && d.layers >= 2 && d.heads > 0 && d.width % d.heads == 0 && d.patch > 0 && d.embed_dim > 0 && d.grid0 > 0 &&
             d.mlp_width > 0, "sg_create: bad descriptor");
  SG_REQUIRE(d.precision == SG_PREC_F32 || d.precision == SG_PREC_BF16 || d.precision == SG_PREC_FP8 || d.precision == SG_PREC_F16 ||
             d.precision == SG_PREC_F16X2, "sg_create: bad precision %d", d.precision);
  SG_REQUIRE(d.width % 4 == 0 && d.embed_dim % 4 == 0, "sg_create: width / embed_dim must be multiples of 4");
  if (d.precision == SG_PREC_FP8)
    SG_REQUIRE(d.width % 128 == 0 && d.mlp_width % 128 == 0, "sg_create: fp8 mode needs width and mlp_width to be multiples of 128");
  if (d.precision != SG_PREC_F32) {
    SG_REQUIRE(d.width % 64 == 0 && d.mlp_width % 64 == 0, "sg_create: bf16 mode needs width and mlp_width to be multiples of 64");
    const int dh = d.width / d.heads;
    SG_REQUIRE(dh == 32 || dh == 64 || dh == 80 || dh == 128, "sg_create: bf16 mode supports head_dim 32/64/80/128, got %d", dh);
  }
  DeviceGuard dg(device);
  sg_context* c = new sg_context();
  TowerCore& core = c->core;
  c->d = d;
  core_init(core, device, d.width, d.heads, d.mlp_width, d.layers, d.quick_gelu, d.precision, /*ln_fold=*/true);
  c->Kpatch = 3 * d.patch * d.patch;
  c->Kpad = (int)align_up(c->Kpatch, 64);
  c->finalized = false;
  c->have.assign(8 + 12 * d.layers, 0);
  auto lay = [&](Bump& bb) {
    const size_t e = core.esz; const int D = d.width;
    c->w_patch = bb.take((size_t)D * c->Kpad * e);
    c->w_projT = bb.take((size_t)d.embed_dim * D * e);
    c->cls_emb = bb.get<float>(D);
    c->pos = bb.get<float>((size_t)(d.grid0 * d.grid0 + 1) * D);
    c->lnpre_g = bb.get<float>(D); c->lnpre_b = bb.get<float>(D); c->lnpost_g = bb.get<float>(D); c->lnpost_b = bb.get<float>(D);
    lay_layers(core, bb);
  };
  Bump dry(nullptr, 0, true); lay(dry);
  core.arena_bytes = align_up(dry.off, 256);
  hipError_t e = hipMalloc(&core.arena, core.arena_bytes);
  if (e != hipSuccess) { const size_t bytes = core.arena_bytes; delete c; return fail(SG_ERR_HIP, "sg_create: hipMalloc(%zu) -> %s", bytes, hipGetErrorString(e)); }
  Bump real(core.arena, core.arena_bytes, false); lay(real);
  *out = c;
  return SG_OK;
}

extern "C" void sg_destroy(sg_context* c) {
  if (!c) return;
  for (auto& L : c->core.layers) { if (L.stage_qkv) (void)hipFree(L.stage_qkv); if (L.stage_fc) (void)hipFree(L.stage_fc); }
  if (c->core.arena) (void)hipFree(c->core.arena);
  delete c;
}

extern "C" int sg_vit_set_tensor(sg_context* c, const char* name, const float* src, int64_t numel, sg_stream st) {
  SG_REQUIRE(c && name && src, "sg_vit_set_tensor: null argument");
  DeviceGuard dg(c->core.device);
  const sg_vit_desc& d = c->d;
  const int D = d.width, E = d.embed_dim;
  const TensorSrc t{"sg_vit_set_tensor", name, src, numel, c->core.hk, as_stream(st)};
  int slot = -1, rc = SG_OK;
  if (!strcmp(name, "conv1.weight")) { slot = 0; rc = pack_w(t, c->w_patch, D, c->Kpatch, c->Kpad); }
  else if (!strcmp(name, "class_embedding")) { slot = 1; rc = copy_f32(t, c->cls_emb, D); }
  else if (!strcmp(name, "positional_embedding")) { slot = 2; rc = copy_f32(t, c->pos, (int64_t)(d.grid0 * d.grid0 + 1) * D); }
  else if (!strcmp(name, "ln_pre.weight")) { slot = 3; rc = copy_f32(t, c->lnpre_g, D); }
  else if (!strcmp(name, "ln_pre.bias")) { slot = 4; rc = copy_f32(t, c->lnpre_b, D); }
  else if (!strcmp(name, "ln_post.weight")) { slot = 5; rc = copy_f32(t, c->lnpost_g, D); }
  else if (!strcmp(name, "ln_post.bias")) { slot = 6; rc = copy_f32(t, c->lnpost_b, D); }
  else if (!strcmp(name, "proj")) {
    slot = 7;
    SG_REQUIRE(numel == (int64_t)D * E, "sg_vit_set_tensor(proj): expected %d x %d", D, E);
    rc = transpose_pack(src, D, E, c->w_projT, t.hk, t.s);
  } else {
    rc = set_layer_tensor(c->core, t, slot);
    if (slot >= 0) slot += 8;
  }
  if (slot < 0) return fail(SG_ERR_INVALID, "sg_vit_set_tensor: unknown tensor name '%s'", name);
  if (rc != SG_OK) return rc;
  c->have[slot] = 1;
  c->finalized = false;
  return SG_OK;
}

extern "C" int sg_vit_finalize(sg_context* c, sg_stream st) {
  SG_REQUIRE(c, "sg_vit_finalize: null context");
  int missing = 0;
  for (uint8_t h : c->have) if (!h) ++missing;
  if (missing) return fail(SG_ERR_STATE, "sg_vit_finalize: %d of %d tensors were never set", missing, (int)c->have.size());
  // fold ln_1 into the QKV weight and ln_2 into the fc weight of every block whose f32 weights are still staged; a block whose LayerNorm
  // parameters were replaced without its weights keeps the explicit LayerNorm pass (folded == false)
  TowerCore& core = c->core;
  DeviceGuard dg(core.device);
  const int D = core.width, M = core.mlp_width;
  for (auto& L : core.layers) {
    if (!L.w_qkv_f || L.folded || !L.stage_qkv || !L.stage_fc) continue;
    SG_TRY(fold_ln_weight(L.stage_qkv, 3 * D, D, L.ln1_g, L.ln1_b, L.b_qkv, core.hk, L.w_qkv_f, L.c_qkv, L.bf_qkv, as_stream(st)));
    SG_TRY(fold_ln_weight(L.stage_fc, M, D, L.ln2_g, L.ln2_b, L.b_fc, core.hk, L.w_fc_f, L.c_fc, L.bf_fc, as_stream(st)));
    L.folded = true;
  }
  SG_HIP(hipStreamSynchronize(as_stream(st)));               // the staged f32 copies are freed below: their last readers (and writers) are on this stream
  for (auto& L : core.layers) {
    if (L.stage_qkv) { (void)hipFree(L.stage_qkv); L.stage_qkv = nullptr; }
    if (L.stage_fc) { (void)hipFree(L.stage_fc); L.stage_fc = nullptr; }
  }
  c->finalized = true;
  return SG_OK;
}

extern "C" size_t sg_vit_workspace_bytes(const sg_context* c, int n_tiles, int gh, int gw, const sg_forward_opts* o) {
  if (!c || !o || n_tiles <= 0 || gh <= 0 || gw <= 0) return 0;
  Plan p;
  return plan(c, n_tiles, gh, gw, o, nullptr, true, p);
}

// stats: leave the head-averaged A[cls,:] / diag(A) in sc.attn_cls / sc.attn_diag; want_avg: leave the head-averaged attention matrix in
// sc.attn_avg; causal: the text tower's mask
struct BlockOpts { bool stats = false, want_avg = false, causal = false; };
// The folded-LayerNorm hand-off between blocks.  x16 == true means exactly this: sc.xn holds the 2-byte copy of the
// CURRENT x and sc.ln_slice its slice statistics, both written by the GEMM that produced x, so the next LayerNorm of x needs no pass of
// its own.  A block function reads it for the x it is given and leaves it describing the x it returns.
struct LnHandoff { bool x16 = false; };

// May a LayerNorm of x [R, D] in front of one of L's GEMMs be folded into it?  2-byte modes, shapes that run on the persistent GEMM;
// TUNE_LN_PASS switches it off (small launches -- a tile or two per call -- run the residual GEMMs on smaller tiles instead, see gemm_bf16.hip few_tiles)
static bool ln_fold_ok(const TowerCore& c, const LayerW& L, const BlockScratch& sc, int64_t R) {
  const int D = c.width;
  return c.hk != HK_F32 && !c.fp8 && L.folded && sc.ln_slice && R < (1ll << 31) && gemm_bf16_ln_fold_ok((int)R, D, D) && D % 256 == 0 &&
         gemm_bf16_prefers_persistent((int)R, D) && get_gemm_config() != TUNE_LN_PASS;
}

// sc.qkv = ln_1(x) . Wqkv^T + b of an ordinary block or of the last block.  allow_fp8: the fp8 linear may be used (fp8 mode; never for the
// last block); x16: the hand-off above holds for x, so ln_1 is folded into the GEMM where ln_fold_ok() allows it.
static int ln1_qkv(const TowerCore& c, const LayerW& L, const float* x, const BlockScratch& sc, int64_t R, bool allow_fp8, bool x16, hipStream_t s) {
  const int D = c.width;
  if (allow_fp8 && c.fp8 && sc.x8 && L.w_qkv8) {
    SG_TRY(layernorm_fp8(x, D, L.ln1_g, L.ln1_b, sc.x8, D, sc.sx8, R, D, 1e-5f, s));
    return linear_fp8(sc.x8, sc.sx8, D, L.w_qkv8, L.s_qkv, L.b_qkv, nullptr, sc.qkv, 3 * D, false, (int)R, 3 * D, D, ACT_NONE, s);
  }
  if (x16 && ln_fold_ok(c, L, sc, R)) {
    SG_TRY(ln_stats_finalize(sc.ln_slice, R, D, 1e-5f, sc.ln_rows, s));
    return linear_ln_consumer(c.hk, sc.xn, D, L.w_qkv_f, L.bf_qkv, L.c_qkv, sc.ln_rows, sc.qkv, 3 * D, (int)R, 3 * D, D, ACT_NONE, s);
  }
  SG_TRY(layernorm(x, D, L.ln1_g, L.ln1_b, sc.xn, D, c.hk, R, D, 1e-5f, s));
  return linear(c.hk, sc.xn, D, L.w_qkv, L.b_qkv, nullptr, sc.qkv, 3 * D, false, (int)R, 3 * D, D, ACT_NONE, s);
}

// x += proj(act(fc(ln_2(x)))).  h.x16 on entry folds ln_2 into the fc GEMM, and the proj GEMM then hands the x it produces on in the same way.
static int mlp_block(const TowerCore& c, const LayerW& L, float* x, const BlockScratch& sc, int64_t R, LnHandoff& h, hipStream_t s) {
  const int D = c.width, M = c.mlp_width;
  const int act = c.quick_gelu ? ACT_QUICK_GELU : ACT_GELU;
  const bool fold = h.x16;
  h.x16 = false;
  if (c.fp8 && sc.x8 && L.w_fc8) {                          // fp8 linears: LN -> e4m3 + row scale; GELU output re-quantised per row
    SG_TRY(layernorm_fp8(x, D, L.ln2_g, L.ln2_b, sc.x8, D, sc.sx8, R, D, 1e-5f, s));
    if (R >= 1024 && M % 128 == 0 && D % 256 == 0) {
      // MXFP8 hand-off: the fc epilogue writes GELU(h) as e4m3 with one power-of-two scale per 32 columns, which the proj GEMM's scaled MFMA
      // consumes directly -- no [R, M] 2-byte intermediate and no separate row-quantisation pass (finer-grained scales than one per row, too)
      SG_TRY(linear_fp8_mx(sc.x8, sc.sx8, nullptr, D, L.w_fc8, L.s_fc, L.b_fc, nullptr, nullptr, M, false, sc.h8, sc.hmx, (int)R, M, D, act, s));
      return linear_fp8_mx(sc.h8, nullptr, sc.hmx, M, L.w_proj8, L.s_proj, L.b_proj, x, x, D, true, nullptr, nullptr, (int)R, D, M, ACT_NONE, s);
    }
    SG_TRY(linear_fp8(sc.x8, sc.sx8, D, L.w_fc8, L.s_fc, L.b_fc, nullptr, sc.hbuf, M, false, (int)R, M, D, act, s));
    SG_TRY(quantize_rows_fp8(sc.hbuf, 1, M, sc.h8, M, sc.sh8, R, M, s));
    return linear_fp8(sc.h8, sc.sh8, M, L.w_proj8, L.s_proj, L.b_proj, x, x, D, true, (int)R, D, M, ACT_NONE, s);
  }
  if (!fold) {
    SG_TRY(layernorm(x, D, L.ln2_g, L.ln2_b, sc.xn, D, c.hk, R, D, 1e-5f, s));
    SG_TRY(linear(c.hk, sc.xn, D, L.w_fc, L.b_fc, nullptr, sc.hbuf, M, false, (int)R, M, D, act, s));
    return linear(c.hk, sc.hbuf, M, L.w_proj, L.b_proj, x, x, D, true, (int)R, D, M, ACT_NONE, s);
  }
  SG_TRY(ln_stats_finalize(sc.ln_slice, R, D, 1e-5f, sc.ln_rows, s));
  SG_TRY(linear_ln_consumer(c.hk, sc.xn, D, L.w_fc_f, L.bf_fc, L.c_fc, sc.ln_rows, sc.hbuf, M, (int)R, M, D, act, s));
  SG_TRY(linear_ln_producer(c.hk, sc.hbuf, M, L.w_proj, L.b_proj, x, x, D, sc.xn, sc.ln_slice, (int)R, D, M, s));
  h.x16 = true;
  return SG_OK;
}

static int averaged_attention(int hk, size_t esz, int D, int H, const void* qkv_or_probs, float* qk32, float* scores, float* probs, float* attn_avg,
                              int B, int N, hipStream_t s);
// the block whose packed qkv (parity mode: whose materialised probabilities) the scratch holds -> sc.attn_avg
static int block_averaged_attention(const TowerCore& c, const BlockScratch& sc, int B, int N, hipStream_t s) {
  return averaged_attention(c.hk, c.esz, c.width, c.heads, c.hk == HK_F32 ? (const void*)sc.probs : sc.qkv, sc.sa_qk32, sc.sa_scores, sc.sa_probs,
                            sc.attn_avg, B, N, s);
}
// One ordinary residual block (reference open_clip/transformer.py:234-254), x updated in place.
static int std_block(const TowerCore& c, const LayerW& L, float* x, const BlockScratch& sc, int B, int N, const BlockOpts& o, LnHandoff& h,
                     hipStream_t s) {
  const int D = c.width, H = c.heads;
  const int64_t R = (int64_t)B * N;
  AttnBuffers ab{sc.scores, sc.probs, sc.lse, sc.lse1, sc.omega, sc.qnorm, sc.knorm};
  const bool fold = ln_fold_ok(c, L, sc, R);
  SG_TRY(ln1_qkv(c, L, x, sc, R, /*allow_fp8=*/true, h.x16, s));
  SG_TRY(run_attention(c.hk, sc.qkv, B, N, D, H, SG_VANILLA, nullptr, 0.f, nullptr, sc.ctx, o.stats, ab, s, o.causal));
  if (o.stats)
    SG_TRY(attention_stats(sc.qkv, c.hk, (int64_t)N * 3 * D, 3 * D, sc.lse, B, N, H, D / H, 1.0f / sqrtf((float)(D / H)), sc.attn_cls,
                           sc.attn_diag, s));
  if (o.want_avg) SG_TRY(block_averaged_attention(c, sc, B, N, s));
  if (fold) SG_TRY(linear_ln_producer(c.hk, sc.ctx, D, L.w_out, L.b_out, x, x, D, sc.xn, sc.ln_slice, (int)R, D, D, s));
  else SG_TRY(linear(c.hk, sc.ctx, D, L.w_out, L.b_out, x, x, D, true, (int)R, D, D, ACT_NONE, s));
  h.x16 = fold;                                                       // the out-projection has just written x
  return mlp_block(c, L, x, sc, R, h, s);
}

__global__ void unpack_qk_kernel(const void* __restrict__ qkv, int N, int D, float* __restrict__ out, int kind) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * 2 * D) return;
  const int t = (int)(i / (2 * D)), c = (int)(i % (2 * D));
  if (kind == HK_F16X2) { out[i] = ld_elem<h2_t>(reinterpret_cast<const h2_t*>(qkv) + (int64_t)t * 3 * D, c); return; }
  const bf16_t v = reinterpret_cast<const bf16_t*>(qkv)[(int64_t)t * 3 * D + c];
  out[i] = kind == HK_F16 ? h2f(f16_t{v}) : bf2f(v);
}
// head-averaged attention matrix [B,N,N] of a block (the tensor the reference gets from nn.MultiheadAttention(need_weights=True),
// transformer.py:609-610).  Only the optional mode='attention' enhancer and layer fusion need it.  Parity mode (HK_F32): `qkv_or_probs` is the
// materialised probabilities [B,H,N,N] and the head mean is the whole stage; otherwise it is the packed qkv [B,N,3D] in the storage `hk`
// (esz bytes per element), rebuilt per image through qk32 [N,2D], scores and probs [H,N,N] (all f32).
static int averaged_attention(int hk, size_t esz, int D, int H, const void* qkv_or_probs, float* qk32, float* scores, float* probs, float* attn_avg,
                              int B, int N, hipStream_t s) {
  const int dh = D / H;
  const float scale = 1.0f / sqrtf((float)dh);
  if (hk == HK_F32) return head_mean((const float*)qkv_or_probs, B, H, N, attn_avg, s);   // parity mode: the probabilities are materialised already
  const int64_t NN = (int64_t)N * N;
  for (int b = 0; b < B; ++b) {
    const void* qkv = (const char*)qkv_or_probs + (size_t)b * N * 3 * D * esz;
    hipLaunchKernelGGL(unpack_qk_kernel, dim3((unsigned)cdiv((int64_t)N * 2 * D, 256)), dim3(256), 0, s, qkv, N, D, qk32, hk);
    SG_LAUNCH_CHECK();
    GemmF32Args g{};
    g.A = qk32; g.lda = 2 * D; g.sAi = dh; g.B = qk32 + D; g.sbk = 1; g.sbn = 2 * D; g.sBi = dh;
    g.C = scores; g.ldc = N; g.sCi = NN; g.M = N; g.N = N; g.K = dh; g.batch = H; g.inner = H; g.act = 0; g.alpha = 1.f;
    SG_TRY(gemm_f32(g, s));
    SG_TRY(softmax_rows(scores, N, (int64_t)H * N, N, H, nullptr, scale, nullptr, 0.f, 0, nullptr, nullptr, 0, 0, probs, nullptr, s));
    SG_TRY(head_mean(probs, 1, H, N, attn_avg + (int64_t)b * NN, s));
  }
  return SG_OK;
}

static int gem_forward_tail(const sg_context* c, const sg_forward_opts* o, const Plan& p, int B, int N, hipStream_t s);

extern "C" int sg_vit_forward(sg_context* c, const sg_tile_batch* tiles, const sg_forward_opts* o, float* out_cls, float* out_tokens,
                              void* workspace, size_t workspace_bytes, sg_stream st) {
  SG_REQUIRE(c && tiles && o && out_tokens && workspace, "sg_vit_forward: null argument");
  if (!c->finalized) return fail(SG_ERR_STATE, "sg_vit_forward: weights not finalized (call sg_vit_finalize)");
  const TowerCore& core = c->core;
  DeviceGuard dg(core.device);                                        // the context's device, whatever the caller's current device is
  hipStream_t s = as_stream(st);
  const sg_vit_desc& d = c->d;
  const int hk = core.hk;
  const int B = tiles->n_tiles, gh = tiles->grid_h, gw = tiles->grid_w, n = gh * gw, N = n + 1;
  const int D = d.width, H = d.heads, L = d.layers, E = d.embed_dim;
  const int64_t R = (int64_t)B * N;
  SG_REQUIRE(B > 0 && gh > 0 && gw > 0, "sg_vit_forward: empty batch");
  SG_REQUIRE(tiles->scene && tiles->windows, "sg_vit_forward: null scene / windows");
  SG_REQUIRE(o->model_type == SG_GEM || out_cls, "sg_vit_forward: out_cls required");
  SG_REQUIRE(R * (int64_t)(d.mlp_width > 3 * D ? d.mlp_width : 3 * D) < (1ll << 40), "sg_vit_forward: batch too large");
  if (o->outlier_enabled || o->selfattn_enabled) SG_REQUIRE(gh == gw, "sg_vit_forward: refiners need a square patch grid (reference transformer.py:583)");
  if (o->outlier_enabled) SG_REQUIRE(o->outlier_top_k >= 1, "sg_vit_forward: outlier_top_k must be >= 1");
  Plan p;
  const size_t need = plan(c, B, gh, gw, o, workspace, false, p);
  if (need > workspace_bytes) return fail(SG_ERR_STATE, "sg_vit_forward: workspace %zu < required %zu bytes", workspace_bytes, need);
  SG_REQUIRE((((uintptr_t)workspace) & 255) == 0, "sg_vit_forward: workspace must be 256-byte aligned");
  const BlockScratch& sc = p.blk;

  // ---- prologue: patch embed, class token, positional embedding, ln_pre (transformer.py:559-576) ----
  const bool gem = o->model_type == SG_GEM;
  SG_TRY(patchify(*tiles, d.patch, p.patchA, c->Kpad, hk, s));
  SG_TRY(linear(hk, p.patchA, c->Kpad, c->w_patch, nullptr, nullptr, p.patchOut, D, true, B * n, D, c->Kpad, ACT_NONE, s));
  const float* pos = c->pos;
  if (gh != d.grid0 || gw != d.grid0) { SG_TRY(posembed_resize(c->pos, d.grid0, D, gh, gw, gem ? 1 : 0, p.pos_r, s)); pos = p.pos_r; }
  SG_TRY(embed_assemble(p.patchOut, D, c->cls_emb, pos, c->lnpre_g, c->lnpre_b, p.x, B, N, D, 1e-5f, s));

  LnHandoff h;                                                        // of p.x, from block to block
  if (gem) {
    const int first = L - (o->gem_depth - 1);
    SG_REQUIRE(o->gem_depth >= 2 && first >= 0, "sg_vit_forward: gem_depth %d does not fit %d layers", o->gem_depth, L);
    // GEM + outlier suppression in ONE forward (BASELINE configs[2]; the reference cannot run it, SURVEY R5 -- DESIGN.md section 7 defines it):
    // detection on the head-averaged attention of the ORDINARY stream of block L-2, suppression on the GEM stream before ln_post.
    // The other refiners have no defined place in the GEM forward: refuse rather than ignore them.
    SG_REQUIRE(!o->selfattn_enabled && !o->similarity_enabled && !o->layer_fusion_enabled,
               "sg_vit_forward: GEM composes with outlier suppression only (self-attention / similarity enhancement and layer fusion are not defined for the GEM forward)");
    const bool gem_out = o->outlier_enabled != 0;
    BlockOpts bo;
    for (int i = 0; i < first; ++i) {
      bo.stats = gem_out && i == L - 2;
      SG_TRY(std_block(core, core.layers[i], p.x, sc, B, N, bo, h, s));
    }
    SG_TRY(gem_forward_tail(c, o, p, B, N, s));
    if (gem_out) {
      const int k = o->outlier_top_k < n ? o->outlier_top_k : n;
      SG_TRY(select_topk(sc.attn_cls, sc.attn_diag, B, N, k, 0, p.idx_out, s));
      SG_TRY(neighbour_refine(p.x_gem, (int64_t)N * D, D, p.idx_out, B, gh, gw, D, k, 1, o->outlier_contamination_temp, p.refine_scratch, s));
    }
    SG_TRY(layernorm(p.x_gem, D, c->lnpost_g, c->lnpost_b, sc.xn, D, hk, R, D, 1e-5f, s));
  } else {
    const int mid = (L - 1) / 2;                                      // transformer.py:593
    const bool fusion = o->layer_fusion_enabled != 0;                 // transformer.py:598: takes precedence over the elif at :609
    const bool want_stats = o->outlier_enabled != 0 && !fusion;       // transformer.py:609 (R6)
    const float lf = o->layer_fusion_lambda;
    const int64_t BNN = (int64_t)B * N * N;
    for (int i = 0; i < L - 1; ++i) {
      if (i == mid && o->similarity_enabled)                          // normalised mid-layer patches (similarity_enhancement.py:49)
        SG_TRY(l2norm_rows(p.x + D, 0, (int64_t)N * D, D, n, p.xhat, hk, (int64_t)n * D, D, (int64_t)B * n, D, 1e-12f, s));
      BlockOpts bo;
      bo.stats = want_stats && i == L - 2;
      bo.want_avg = fusion || (bo.stats && o->selfattn_enabled && o->selfattn_mode == 1);
      SG_TRY(std_block(core, core.layers[i], p.x, sc, B, N, bo, h, s));
      if (fusion) {                                                   // A_acc = lambda * A_acc + (1 - lambda) * A_l   (:601-607)
        if (i == 0) SG_HIP(hipMemcpyAsync(p.lf_acc, sc.attn_avg, (size_t)BNN * 4, hipMemcpyDeviceToDevice, s));
        else SG_TRY(axpby(p.lf_acc, sc.attn_avg, 1.0f - lf, lf, BNN, s));
      }
    }
    if (o->similarity_enabled)
      // the map stays f32 (similarity_enhancement.py computes it in fp32): a 2-byte map halves the attention kernel's bias fetch but was
      // measured no faster (round 2) -- the 'Experimental' kernel is bound by its two exponentials per score, not by the fetch
      SG_TRY(similarity_from_xhat(hk, p.xhat, B, n, D, o->similarity_temperature, o->similarity_add_self, p.sim, s));
    // ---- last block: self-self attention on ln_1(x), no residual / MLP when ignore_residual (transformer.py:627-643) ----
    // Its QKV projection never takes the fp8 linear; ln_1 is folded when block L-2's proj GEMM handed x on.
    const LayerW& LL = core.layers[L - 1];
    AttnBuffers ab{sc.scores, sc.probs, sc.lse1, sc.lse1, sc.omega, sc.qnorm, sc.knorm};
    SG_TRY(ln1_qkv(core, LL, p.x, sc, R, /*allow_fp8=*/false, h.x16, s));
    if (fusion && o->ignore_residual) {                               // :630-637: the last block's own blk(x) attention joins the EMA
      if (hk == HK_F32) {                                             // parity mode: materialise the ordinary attention's probabilities
        AttnBuffers av{sc.scores, sc.probs, sc.lse, sc.lse1, sc.omega, sc.qnorm, sc.knorm};
        SG_TRY(run_attention(hk, sc.qkv, B, N, D, H, SG_VANILLA, nullptr, 0.f, nullptr, sc.ctx, false, av, s));
      }
      SG_TRY(block_averaged_attention(core, sc, B, N, s));
      if (L == 1) SG_HIP(hipMemcpyAsync(p.lf_acc, sc.attn_avg, (size_t)BNN * 4, hipMemcpyDeviceToDevice, s));
      else SG_TRY(axpby(p.lf_acc, sc.attn_avg, 1.0f - lf, lf, BNN, s));
    }
    const void* ctx = sc.ctx; int64_t ctx_ld = D;
    if (o->model_type == SG_MASKCLIP) { ctx = (const char*)sc.qkv + (size_t)2 * D * core.esz; ctx_ld = 3 * D; }   // identity attention: ctx = v
    else SG_TRY(run_attention(hk, sc.qkv, B, N, D, H, o->model_type, (o->similarity_enabled && o->model_type < SG_NACLIP) ? p.sim : nullptr, o->similarity_weight,
                              nullptr, sc.ctx, false, ab, s));
    SG_TRY(linear(hk, ctx, ctx_ld, LL.w_out, LL.b_out, o->ignore_residual ? nullptr : p.x, p.out_last, D, true, (int)R, D, D, ACT_NONE, s));
    LnHandoff none;                                                   // p.out_last comes from a plain GEMM
    if (!o->ignore_residual) SG_TRY(mlp_block(core, LL, p.out_last, sc, R, none, s));
    // ---- attention-map layer fusion: mask the fused map's outlier columns, renormalise, re-weight every token (transformer.py:647-690) ----
    if (fusion && o->outlier_enabled)
      SG_TRY(layer_fusion_apply(p.lf_acc, p.out_last, B, N, D, o->outlier_top_k, sc.attn_cls, sc.attn_diag, p.idx_out, sc.sa_tmp, s));
    // ---- refinements on the last-block output (transformer.py:698-742); need block L-2's attention, which layer fusion does not capture ----
    if (!fusion && o->outlier_enabled && o->selfattn_enabled && o->selfattn_mode == 1) {
      SG_TRY(attn_mode_enhance(p.out_last, (int64_t)N * D, D, sc.attn_avg, B, N, D, o->selfattn_strength, o->selfattn_threshold, sc.sa_tmp, s));
    } else if (!fusion && o->outlier_enabled && o->selfattn_enabled) {   // top-k replacement of the weakest tokens
      const int k = o->selfattn_top_k < n ? o->selfattn_top_k : n;
      SG_TRY(select_topk(sc.attn_cls, sc.attn_diag, B, N, k, 1, p.idx_sa, s));
      SG_TRY(neighbour_refine(p.out_last, (int64_t)N * D, D, p.idx_sa, B, gh, gw, D, k, 0, 0.f, p.refine_scratch, s));
    }
    if (o->outlier_enabled && !fusion) {
      const int k = o->outlier_top_k < n ? o->outlier_top_k : n;
      SG_TRY(select_topk(sc.attn_cls, sc.attn_diag, B, N, k, 0, p.idx_out, s));
      SG_TRY(neighbour_refine(p.out_last, (int64_t)N * D, D, p.idx_out, B, gh, gw, D, k, 1, o->outlier_contamination_temp, p.refine_scratch, s));
    }
    SG_TRY(layernorm(p.out_last, D, c->lnpost_g, c->lnpost_b, sc.xn, D, hk, R, D, 1e-5f, s));
  }
  // ---- epilogue: `@ proj` on every token (transformer.py:765-770) ----
  SG_TRY(linear(hk, sc.xn, D, c->w_projT, nullptr, nullptr, p.y, E, true, (int)R, E, D, ACT_NONE, s));
  if (out_cls && !gem)
    SG_HIP(hipMemcpy2DAsync(out_cls, (size_t)E * 4, p.y, (size_t)N * E * 4, (size_t)E * 4, B, hipMemcpyDeviceToDevice, s));
  SG_HIP(hipMemcpy2DAsync(out_tokens, (size_t)n * E * 4, p.y + E, (size_t)N * E * 4, (size_t)n * E * 4, B, hipMemcpyDeviceToDevice, s));
  return SG_OK;
}

// GEM dual-stream blocks (reference gem/gem_utils.py:60-153).  p.x is the ordinary stream; p.x_gem the GEM stream.
static int gem_forward_tail(const sg_context* c, const sg_forward_opts* o, const Plan& p, int B, int N, hipStream_t s) {
  const TowerCore& core = c->core;
  const BlockScratch& sc = p.blk;
  const int D = core.width, H = core.heads, L = core.n_layers, dh = D / H;
  const int64_t R = (int64_t)B * N;
  const float scale = 1.0f / sqrtf((float)dh);
  const int first = L - (o->gem_depth - 1);
  const int hk = core.hk;
  SG_HIP(hipMemcpyAsync(p.x_gem, p.x, (size_t)R * D * 4, hipMemcpyDeviceToDevice, s));
  AttnBuffers ab{sc.scores, sc.probs, sc.lse, sc.lse1, nullptr, nullptr, nullptr};
  for (int i = first; i < L; ++i) {
    const LayerW& LW = core.layers[i];
    // not ln1_qkv(): the temperature (mean token norm, gem_utils.py:79-81) needs ln_1(x) in f32, so the compute-dtype copy is packed from it
    SG_TRY(layernorm(p.x, D, LW.ln1_g, LW.ln1_b, p.gem_out, D, HK_F32, R, D, 1e-5f, s));
    SG_TRY(gem_inv_temp(p.gem_out, B, N, D, scale, p.inv_temp, s));
    const void* xn = p.gem_out;
    if (hk != HK_F32) { SG_TRY(pack_rows(p.gem_out, R, D, D, sc.xn, D, hk, s)); xn = sc.xn; }
    SG_TRY(linear(hk, xn, D, LW.w_qkv, LW.b_qkv, nullptr, sc.qkv, 3 * D, false, (int)R, 3 * D, D, ACT_NONE, s));
    // ordinary stream attention -> sc.ctx (+ block L-2's head-averaged A[cls,:] / diag(A) when outlier suppression rides on the GEM forward)
    const bool stats = o->outlier_enabled != 0 && i == L - 2;
    SG_TRY(run_attention(hk, sc.qkv, B, N, D, H, SG_VANILLA, nullptr, 0.f, nullptr, sc.ctx, stats, ab, s));
    if (stats)
      SG_TRY(attention_stats(sc.qkv, hk, (int64_t)N * 3 * D, 3 * D, sc.lse, B, N, H, dh, scale, sc.attn_cls, sc.attn_diag, s));
    // GEM streams (v, k, q): normalise per head -> self-attend with values = the normalised vectors -> normalise
    const int64_t st3 = 3 * (int64_t)D;
    for (int t = 0; t < 3; ++t) {
      const char* src = (const char*)sc.qkv + (size_t)(2 - t) * D * core.esz;
      SG_TRY(l2norm_rows(src, hk, st3, dh, H, p.gnorm[t], hk, D, dh, R * H, dh, 1e-12f, s));
      AttnSpec sp{};
      sp.q[0] = sp.k[0] = sp.v = p.gnorm[t]; sp.sb = sp.v_sb = (int64_t)N * D; sp.st = sp.v_st = D;
      sp.n_terms = 1; sp.scale = scale; sp.scale_per_image = p.inv_temp; sp.out_scale = 1.f;
      sp.ctx = p.gatt[t]; sp.ctx_sb = (int64_t)N * D; sp.ctx_st = D;
      SG_TRY(attn_generic(hk, sp, B, N, H, dh, ab, s));
      SG_TRY(l2norm_rows(p.gatt[t], hk, D, dh, H, p.gatt[t], hk, D, dh, R * H, dh, 1e-12f, s));
    }
    // assignment to V: mean of the three softmax(y y^T * inv_temp) . v   (gem_utils.py:101-117)
    AttnSpec sp{};
    for (int t = 0; t < 3; ++t) sp.q[t] = sp.k[t] = p.gatt[t];
    sp.sb = (int64_t)N * D; sp.st = D;
    sp.v = (const char*)sc.qkv + (size_t)2 * D * core.esz; sp.v_sb = (int64_t)N * st3; sp.v_st = st3;
    sp.n_terms = 3; sp.scale = scale; sp.scale_per_image = p.inv_temp; sp.out_scale = 1.0f / 3.0f;
    sp.ctx = p.ctx2; sp.ctx_sb = (int64_t)N * D; sp.ctx_st = D;
    SG_TRY(attn_generic(hk, sp, B, N, H, dh, ab, s));
    // shared out_proj: GEM stream (residual optional, gem_utils.py:149-152), then the ordinary stream + MLP
    SG_TRY(linear(hk, p.ctx2, D, LW.w_out, LW.b_out, o->ignore_residual ? nullptr : p.x_gem, p.x_gem, D, true, (int)R, D, D, ACT_NONE, s));
    SG_TRY(linear(hk, sc.ctx, D, LW.w_out, LW.b_out, p.x, p.x, D, true, (int)R, D, D, ACT_NONE, s));
    LnHandoff none;                                                   // p.x comes from a plain GEMM
    SG_TRY(mlp_block(core, LW, p.x, sc, R, none, s));
  }
  return SG_OK;
}

// ---- CLIP text tower (reference open_clip/model.py:288-306 encode_text; init-time producer of query_features) --------------------
// Same residual blocks as the vision tower (nn.MultiheadAttention + MLP) with the causal mask of build_causal_mask, token +
// positional embedding in front, ln_final + EOT pooling (argmax of the token ids) + text_projection behind.
struct sg_text {
  TowerCore core;
  int context_length, vocab_size, embed_dim;
  float *tok_emb, *pos_emb, *lnf_g, *lnf_b;
  void* w_projT;                   // [E, W]
  std::vector<uint8_t> have_text;  // which tensors have arrived: 5 of the tower's own, then 12 per layer
};

__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ tok_emb,
                                                         const float* __restrict__ pos, int S, int ctx, int W, int vocab, float* __restrict__ x,
                                                         int* __restrict__ bad_id) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)S * ctx * W) return;
  const int c = (int)(i % W);
  const int64_t row = i / W;
  const int t = (int)(row % ctx);
  int id = tokens[row];
  if (id < 0 || id >= vocab) { if (c == 0) atomicMax(bad_id, 1); id = id < 0 ? 0 : vocab - 1; }   // reported by sg_text_encode; clamped only so the gather stays in bounds
  x[i] = tok_emb[(int64_t)id * W + c] + pos[(int64_t)t * W + c];
}
// pooled[s,:] = x[s, argmax_t tokens[s,t], :]   (text_global_pool 'argmax': the EOT token has the highest id; first maximum wins)
__global__ __launch_bounds__(256) void text_pool_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ x, int ctx, int W,
                                                        float* __restrict__ pooled) {
  __shared__ int s_arg;
  const int sidx = blockIdx.x;
  if (threadIdx.x == 0) {
    int best = tokens[(int64_t)sidx * ctx], arg = 0;
    for (int t = 1; t < ctx; ++t) { const int v = tokens[(int64_t)sidx * ctx + t]; if (v > best) { best = v; arg = t; } }
    s_arg = arg;
  }
  __syncthreads();
  const float* src = x + ((int64_t)sidx * ctx + s_arg) * W;
  for (int c = threadIdx.x; c < W; c += 256) pooled[(int64_t)sidx * W + c] = src[c];
}

extern "C" int sg_text_create(sg_text** out, int device, int width, int layers, int heads, int context_length, int vocab_size, int embed_dim,
                              int quick_gelu, int precision) {
  SG_REQUIRE(out && width > 0 && layers > 0 && heads > 0 && width % heads == 0 && context_length > 0 && vocab_size > 0 && embed_dim > 0,
             "sg_text_create: bad arguments");
  SG_REQUIRE(precision == SG_PREC_F32 || precision == SG_PREC_BF16 || precision == SG_PREC_F16 || precision == SG_PREC_F16X2, "sg_text_create: bad precision");
  SG_REQUIRE(width % 4 == 0 && embed_dim % 4 == 0, "sg_text_create: width / embed_dim must be multiples of 4");
  if (precision != SG_PREC_F32) {
    const int dh = width / heads;
    SG_REQUIRE(width % 64 == 0 && (dh == 32 || dh == 64 || dh == 80 || dh == 128), "sg_text_create: bf16 mode needs width %% 64 == 0 and head_dim 32/64/80/128");
  }
  DeviceGuard dg(device);
  sg_text* t = new sg_text();
  TowerCore& c = t->core;
  core_init(c, device, width, heads, 4 * width, layers, quick_gelu, precision, /*ln_fold=*/false);   // no finalize step here: LayerNorm is never folded
  t->context_length = context_length; t->vocab_size = vocab_size; t->embed_dim = embed_dim;
  auto lay = [&](Bump& bb) {
    const int D = width;
    t->tok_emb = bb.get<float>((size_t)vocab_size * D); t->pos_emb = bb.get<float>((size_t)context_length * D);
    t->lnf_g = bb.get<float>(D); t->lnf_b = bb.get<float>(D); t->w_projT = bb.take((size_t)embed_dim * D * c.esz);
    lay_layers(c, bb);
  };
  Bump dry(nullptr, 0, true); lay(dry);
  c.arena_bytes = align_up(dry.off, 256);
  hipError_t e = hipMalloc(&c.arena, c.arena_bytes);
  if (e != hipSuccess) { const size_t bytes = c.arena_bytes; delete t; return fail(SG_ERR_HIP, "sg_text_create: hipMalloc(%zu) -> %s", bytes, hipGetErrorString(e)); }
  Bump real(c.arena, c.arena_bytes, false); lay(real);
  t->have_text.assign(5 + 12 * layers, 0);
  *out = t;
  return SG_OK;
}

extern "C" void sg_text_destroy(sg_text* t) {
  if (!t) return;
  if (t->core.arena) (void)hipFree(t->core.arena);
  delete t;
}

extern "C" int sg_text_set_tensor(sg_text* t, const char* name, const float* src, int64_t numel, sg_stream st) {
  SG_REQUIRE(t && name && src, "sg_text_set_tensor: null argument");
  DeviceGuard dg(t->core.device);
  const int D = t->core.width, E = t->embed_dim;
  const TensorSrc ts{"sg_text_set_tensor", name, src, numel, t->core.hk, as_stream(st)};
  int slot = -1, rc = SG_OK;
  if (!strcmp(name, "token_embedding.weight")) { slot = 0; rc = copy_f32(ts, t->tok_emb, (int64_t)t->vocab_size * D); }
  else if (!strcmp(name, "positional_embedding")) { slot = 1; rc = copy_f32(ts, t->pos_emb, (int64_t)t->context_length * D); }
  else if (!strcmp(name, "ln_final.weight")) { slot = 2; rc = copy_f32(ts, t->lnf_g, D); }
  else if (!strcmp(name, "ln_final.bias")) { slot = 3; rc = copy_f32(ts, t->lnf_b, D); }
  else if (!strcmp(name, "text_projection")) {
    slot = 4;
    SG_REQUIRE(numel == (int64_t)D * E, "sg_text_set_tensor(text_projection): expected %d x %d", D, E);
    rc = transpose_pack(src, D, E, t->w_projT, ts.hk, ts.s);
  } else {
    rc = set_layer_tensor(t->core, ts, slot);
    if (slot >= 0) slot += 5;
  }
  if (slot < 0) return fail(SG_ERR_INVALID, "sg_text_set_tensor: unknown tensor name '%s'", name);
  if (rc != SG_OK) return rc;
  t->have_text[slot] = 1;
  return SG_OK;
}

struct TextPlan { float* x; BlockScratch blk; float* pooled; int32_t* bad_id; };   // bad_id: out-of-vocabulary flag of text_embed_kernel

static size_t text_plan(const sg_text* t, int S, void* ws, bool dry, TextPlan& p) {
  const TowerCore& c = t->core;
  const int N = t->context_length, D = c.width;
  const int64_t R = (int64_t)S * N;
  p = TextPlan{};
  BlockScratch& k = p.blk;
  Bump b(ws, 0, dry);
  p.x = b.get<float>(R * D);
  k.xn = b.take(R * D * c.esz); k.qkv = b.take(R * 3 * D * c.esz); k.ctx = b.take(R * D * c.esz); k.hbuf = b.take(R * c.mlp_width * c.esz);
  k.lse = b.get<float>((size_t)S * c.heads * N); k.lse1 = b.get<float>((size_t)S * c.heads * N);
  if (c.hk == HK_F32) { k.scores = b.get<float>((size_t)S * c.heads * N * N); k.probs = b.get<float>((size_t)S * c.heads * N * N); }
  p.pooled = b.get<float>((size_t)S * D);
  p.bad_id = b.get<int32_t>(1);
  return align_up(b.off, 256);
}

extern "C" size_t sg_text_workspace_bytes(const sg_text* t, int n_seq) {
  if (!t || n_seq <= 0) return 0;
  TextPlan p;
  return text_plan(t, n_seq, nullptr, true, p);
}

// tokens int32 [S, context_length] (device) -> out [S, E] f32 (un-normalised, as encode_text(normalize=False))
extern "C" int sg_text_encode(sg_text* t, const int32_t* tokens, int n_seq, float* out, void* workspace, size_t workspace_bytes, sg_stream st) {
  SG_REQUIRE(t && tokens && out && workspace && n_seq > 0, "sg_text_encode: bad arguments");
  for (size_t i = 0; i < t->have_text.size(); ++i) if (!t->have_text[i]) return fail(SG_ERR_STATE, "sg_text_encode: text weights incomplete");
  const TowerCore& c = t->core;
  DeviceGuard dg(c.device);
  hipStream_t s = as_stream(st);
  const int N = t->context_length, D = c.width, E = t->embed_dim, S = n_seq;
  const int64_t R = (int64_t)S * N;
  TextPlan p;
  const size_t need = text_plan(t, S, workspace, false, p);
  if (need > workspace_bytes) return fail(SG_ERR_STATE, "sg_text_encode: workspace %zu < required %zu", workspace_bytes, need);
  SG_HIP(hipMemsetAsync(p.bad_id, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)cdiv(R * D, 256)), dim3(256), 0, s, tokens, t->tok_emb, t->pos_emb, S, N, D, t->vocab_size, p.x, p.bad_id);
  SG_LAUNCH_CHECK();
  BlockOpts bo;
  bo.causal = true;
  LnHandoff h;                                              // stays false: this tower has no folded operands
  for (const LayerW& L : c.layers) SG_TRY(std_block(c, L, p.x, p.blk, S, N, bo, h, s));
  hipLaunchKernelGGL(text_pool_kernel, dim3(S), dim3(256), 0, s, tokens, p.x, N, D, p.pooled);
  SG_LAUNCH_CHECK();
  SG_TRY(layernorm(p.pooled, D, t->lnf_g, t->lnf_b, p.blk.xn, D, c.hk, S, D, 1e-5f, s));
  SG_TRY(linear(c.hk, p.blk.xn, D, t->w_projT, nullptr, nullptr, out, E, true, S, E, D, ACT_NONE, s));
  // init-time call: the one entry point that synchronises, so that an id outside the vocabulary is an error as in the reference
  // (nn.Embedding raises, open_clip/model.py:292) instead of a silently clamped row
  int32_t bad = 0;
  SG_HIP(hipMemcpyAsync(&bad, p.bad_id, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  SG_HIP(hipStreamSynchronize(s));
  if (bad) return fail(SG_ERR_INVALID, "sg_text_encode: token id outside [0, %d)", t->vocab_size);
  return SG_OK;
}

// ---- stand-alone ops ------------------------------------------------------------------------------------------------------
extern "C" int sg_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, sg_stream s) {
  SG_REQUIRE(x && gamma && beta && y, "sg_op_layernorm: null pointer");
  return layernorm(x, D, gamma, beta, y, D, 0, rows, D, eps, as_stream(s));
}

extern "C" int sg_op_linear(const float* A, const float* W, const float* bias, const float* residual, float* C, int M, int N, int K,
                            int act, int precision, void* scratch, size_t scratch_bytes, sg_stream st) {
  SG_REQUIRE(A && W && C, "sg_op_linear: null pointer");
  SG_REQUIRE(act >= ACT_NONE && act <= ACT_RELU, "sg_op_linear: act %d (0 none, 1 QuickGELU, 2 erf GELU, 3 ReLU)", act);
  hipStream_t s = as_stream(st);
  if (precision == SG_PREC_F32) return linear(HK_F32, A, K, W, bias, residual, C, N, true, M, N, K, act, s);
  const int hk = hk_of_precision(precision);
  const size_t e = hk_esz(hk);
  const int Kp = (int)align_up(K, 64);
  const size_t need = align_up((size_t)M * Kp * e, 256) + (size_t)N * Kp * e;
  if (!scratch || scratch_bytes < need) return fail(SG_ERR_STATE, "sg_op_linear: scratch %zu < %zu", scratch_bytes, need);
  bf16_t* a16 = (bf16_t*)scratch;
  bf16_t* w16 = (bf16_t*)((char*)scratch + align_up((size_t)M * Kp * e, 256));
  SG_TRY(pack_rows(A, M, K, K, a16, Kp, hk, s));
  SG_TRY(pack_rows(W, N, K, K, w16, Kp, hk, s));
  return linear(hk, a16, Kp, w16, bias, residual, C, N, true, M, N, Kp, act, s);
}

// x_new = x + A.W1^T + b1;  y = act(LayerNorm(x_new; gamma, beta).W2^T + b2)  -- the residual GEMM -> LayerNorm -> GEMM chain of a block
// (out-proj -> ln_2 -> fc, proj -> ln_1 -> QKV), either with the LayerNorm as its own pass (fold = 0) or folded into the two GEMMs
// (fold = 1: 2-byte copy + slice statistics out of the first epilogue, (mean, rstd) and the gamma-folded weight in the second).
// 2-byte and two-plane precisions; M >= 1024, D >= 512, D % 64 == 0, N2 >= 512 with fold.  All operands f32 on the device.
extern "C" size_t sg_op_ln_chain_scratch_bytes(int M, int K1, int D, int N2) {
  const size_t K1p = align_up((size_t)K1, 64);
  return align_up((size_t)M * K1p * 4, 256) + align_up((size_t)D * K1p * 4, 256) + align_up((size_t)M * D * 4, 256) + align_up((size_t)N2 * D * 4, 256) +
         align_up((size_t)M * N2 * 4, 256) + align_up((size_t)M * (D / 64 + 1) * 8, 256) + align_up((size_t)M * 8, 256) + 2 * align_up((size_t)N2 * 4, 256) + 4096;
}
extern "C" int sg_op_ln_chain(const float* A, const float* W1, const float* b1, float* x, const float* gamma, const float* beta, const float* W2,
                              const float* b2, float* y, int M, int K1, int D, int N2, int act, int precision, int fold, void* scratch,
                              size_t scratch_bytes, sg_stream st) {
  SG_REQUIRE(A && W1 && x && gamma && beta && W2 && y && scratch, "sg_op_ln_chain: null pointer");
  SG_REQUIRE(precision == SG_PREC_BF16 || precision == SG_PREC_F16 || precision == SG_PREC_F16X2, "sg_op_ln_chain: 2-byte and two-plane precisions only");
  SG_REQUIRE(D % 64 == 0, "sg_op_ln_chain: D %% 64 != 0");
  if (scratch_bytes < sg_op_ln_chain_scratch_bytes(M, K1, D, N2)) return fail(SG_ERR_STATE, "sg_op_ln_chain: scratch too small");
  hipStream_t s = as_stream(st);
  const int hk = hk_of_precision(precision);
  const size_t e = hk_esz(hk);
  const int K1p = (int)align_up(K1, 64);
  Bump b(scratch, 0, false);
  void* a16 = b.take((size_t)M * K1p * e); void* w116 = b.take((size_t)D * K1p * e); void* xn = b.take((size_t)M * D * e);
  void* w216 = b.take((size_t)N2 * D * e); void* y16 = b.take((size_t)M * N2 * e);
  float* slice = b.get<float>((size_t)M * (D / 64) * 2); float* rows = b.get<float>((size_t)M * 2);
  float* cvec = b.get<float>(N2); float* bf = b.get<float>(N2);
  SG_TRY(pack_rows(A, M, K1, K1, a16, K1p, hk, s));
  SG_TRY(pack_rows(W1, D, K1, K1, w116, K1p, hk, s));
  if (fold) {
    SG_TRY(linear_ln_producer(hk, a16, K1p, w116, b1, x, x, D, xn, slice, M, D, K1p, s));
    SG_TRY(ln_stats_finalize(slice, M, D, 1e-5f, rows, s));
    SG_TRY(fold_ln_weight(W2, N2, D, gamma, beta, b2, hk, w216, cvec, bf, s));
    SG_TRY(linear_ln_consumer(hk, xn, D, w216, bf, cvec, rows, y16, N2, M, N2, D, act, s));
  } else {
    SG_TRY(linear(hk, a16, K1p, w116, b1, x, x, D, true, M, D, K1p, ACT_NONE, s));
    SG_TRY(layernorm(x, D, gamma, beta, xn, D, hk, M, D, 1e-5f, s));
    SG_TRY(pack_rows(W2, N2, D, D, w216, D, hk, s));
    SG_TRY(linear(hk, xn, D, w216, b2, nullptr, y16, N2, false, M, N2, D, act, s));
  }
  const int64_t total = (int64_t)M * N2;
  hipLaunchKernelGGL(unpack_bf16_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, (const bf16_t*)y16, y, total, hk);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" size_t sg_op_attention_scratch_bytes(int B, int N, int D, int H, int precision) {
  const size_t R = (size_t)B * N;
  size_t b = 4 * 256 + 2 * align_up((size_t)B * H * N * 4, 256) + align_up((size_t)(N - 1) * (N - 1) * 4, 256) + 2 * align_up((size_t)B * H * N * 4, 256);
  if (precision != SG_PREC_F32) b += align_up(R * 3 * D * hk_esz(hk_of_precision(precision)), 256) + align_up(R * D * hk_esz(hk_of_precision(precision)), 256);
  else b += 2 * align_up((size_t)B * H * N * N * 4, 256);
  return b + 4096;
}

extern "C" int sg_op_attention(const float* qkv, int B, int N, int D, int H, int variant, const float* sim, float sim_weight, float* ctx,
                               float* attn_cls, float* attn_diag, int precision, void* scratch, size_t scratch_bytes, sg_stream st) {
  SG_REQUIRE(qkv && ctx && scratch, "sg_op_attention: null pointer");
  SG_REQUIRE(D % H == 0, "sg_op_attention: D %% H != 0");
  hipStream_t s = as_stream(st);
  const int64_t R = (int64_t)B * N;
  const int hk = hk_of_precision(precision);
  Bump b(scratch, scratch_bytes, false);
  AttnBuffers ab{};
  ab.lse = b.get<float>((size_t)B * H * N); ab.lse1 = b.get<float>((size_t)B * H * N);
  ab.omega = b.get<float>((size_t)(N - 1) * (N - 1)); ab.qnorm = b.get<float>((size_t)B * H * N); ab.knorm = b.get<float>((size_t)B * H * N);
  void* qkv_c = (void*)qkv; void* ctx_c = ctx;
  if (hk != HK_F32) { qkv_c = b.take((size_t)R * 3 * D * hk_esz(hk)); ctx_c = b.take((size_t)R * D * hk_esz(hk)); }
  else { ab.scores = b.get<float>((size_t)B * H * N * N); ab.probs = b.get<float>((size_t)B * H * N * N); }
  if (b.off > scratch_bytes) return fail(SG_ERR_STATE, "sg_op_attention: scratch %zu < %zu", scratch_bytes, b.off);
  if (hk != HK_F32) SG_TRY(pack_rows(qkv, R, 3 * D, 3 * D, qkv_c, 3 * D, hk, s));
  const bool stats = attn_cls && attn_diag;
  if (variant == SG_MASKCLIP) return fail(SG_ERR_INVALID, "sg_op_attention: MaskCLIP is the identity (ctx = v)");
  SG_TRY(run_attention(hk, qkv_c, B, N, D, H, variant, sim, sim_weight, nullptr, ctx_c, stats, ab, s));
  if (stats) SG_TRY(attention_stats(qkv_c, hk, (int64_t)N * 3 * D, 3 * D, ab.lse, B, N, H, D / H, 1.0f / sqrtf((float)(D / H)), attn_cls, attn_diag, s));
  if (hk != HK_F32) {
    hipLaunchKernelGGL(unpack_bf16_kernel, dim3((unsigned)cdiv(R * D, 256)), dim3(256), 0, s, (const bf16_t*)ctx_c, ctx, R * D, hk);
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}

extern "C" int sg_similarity_map(const float* patches, int64_t batch_stride, int ld, int B, int n, int D, float temperature, int add_self,
                                 int precision, float* sim, void* scratch, size_t scratch_bytes, sg_stream st) {
  SG_REQUIRE(patches && sim && scratch, "sg_similarity_map: null pointer");
  hipStream_t s = as_stream(st);
  const int hk = hk_of_precision(precision);
  const size_t need = (size_t)B * n * D * hk_esz(hk);
  if (scratch_bytes < need) return fail(SG_ERR_STATE, "sg_similarity_map: scratch %zu < %zu", scratch_bytes, need);
  if (hk != HK_F32) SG_REQUIRE(D % 64 == 0, "sg_similarity_map: bf16 mode needs D %% 64 == 0");
  SG_TRY(l2norm_rows(patches, 0, batch_stride, ld, n, scratch, hk, (int64_t)n * D, D, (int64_t)B * n, D, 1e-12f, s));
  return similarity_from_xhat(hk, scratch, B, n, D, temperature, add_self, sim, s);
}

// ---- raw test entries of the f32 GEMM and the attention-map stages: one host function each, arguments passed one to one -------------------
extern "C" int sg_gemm_f32_raw(const float* A, int64_t lda, int64_t sAo, int64_t sAi, const float* B, int64_t sbk, int64_t sbn, int64_t sBo,
                               int64_t sBi, const float* bias, const float* residual, int64_t ldr, float* C, int64_t ldc, int64_t sCo, int64_t sCi,
                               int M, int N, int K, int batch, int inner, int act, float alpha, sg_stream st) {
  SG_REQUIRE(A && B && C, "sg_gemm_f32_raw: null pointer");
  GemmF32Args g{};
  g.A = A; g.lda = lda; g.sAo = sAo; g.sAi = sAi; g.B = B; g.sbk = sbk; g.sbn = sbn; g.sBo = sBo; g.sBi = sBi;
  g.bias = bias; g.residual = residual; g.ldr = ldr; g.C = C; g.ldc = ldc; g.sCo = sCo; g.sCi = sCi;
  g.M = M; g.N = N; g.K = K; g.batch = batch; g.inner = inner; g.act = act; g.alpha = alpha;
  return gemm_f32(g, as_stream(st));
}
extern "C" int sg_attn_average_raw(int precision, const void* qkv_or_probs, int B, int N, int D, int H, void* scratch, size_t scratch_bytes,
                                   float* attn_avg, sg_stream st) {
  SG_REQUIRE(qkv_or_probs && attn_avg, "sg_attn_average_raw: null pointer");
  SG_REQUIRE(B > 0 && B < 65536 && N > 0 && D > 0 && H > 0 && D % H == 0, "sg_attn_average_raw: bad shape B=%d N=%d D=%d H=%d", B, N, D, H);
  int hk; SG_TRY(raw_kind("sg_attn_average_raw", precision, &hk));
  float *qk32 = nullptr, *scores = nullptr, *probs = nullptr;
  if (hk != HK_F32) {
    SG_REQUIRE(hk != HK_F16X2 || D % 8 == 0, "sg_attn_average_raw: two-plane rows need D %% 8 == 0");
    SG_REQUIRE(scratch && (((uintptr_t)scratch) & 255) == 0, "sg_attn_average_raw: scratch must be 256-byte aligned");
    Bump b(scratch, scratch_bytes, false);
    qk32 = b.get<float>((size_t)N * 2 * D); scores = b.get<float>((size_t)H * N * N); probs = b.get<float>((size_t)H * N * N);
    if (b.off > scratch_bytes) return fail(SG_ERR_STATE, "sg_attn_average_raw: scratch %zu < %zu", scratch_bytes, b.off);
  }
  return averaged_attention(hk, hk_esz(hk), D, H, qkv_or_probs, qk32, scores, probs, attn_avg, B, N, as_stream(st));
}
extern "C" int sg_attn_enhance_raw(float* tokens, int64_t sb, int64_t st, float* A, int B, int N, int D, float strength, float threshold, float* tmp,
                                   sg_stream st_) {
  SG_REQUIRE(tokens && A && tmp, "sg_attn_enhance_raw: null pointer");
  SG_REQUIRE(B > 0 && B < 65536 && N > 1 && D > 0, "sg_attn_enhance_raw: bad shape B=%d N=%d D=%d", B, N, D);
  SG_REQUIRE(st == D && sb >= (int64_t)N * D, "sg_attn_enhance_raw: the write-back needs dense token rows (st == D) and sb >= N D");
  return attn_mode_enhance(tokens, sb, st, A, B, N, D, strength, threshold, tmp, as_stream(st_));
}
extern "C" int sg_layer_fusion_apply_raw(float* acc, float* tokens, int B, int N, int D, int top_k, float* a_cls, float* a_diag, int32_t* idx_out,
                                         float* tmp, sg_stream st) {
  SG_REQUIRE(acc && tokens && a_cls && a_diag && idx_out && tmp, "sg_layer_fusion_apply_raw: null pointer");
  SG_REQUIRE(B > 0 && B < 65536 && N > 1 && D > 0 && top_k >= 1, "sg_layer_fusion_apply_raw: bad shape B=%d N=%d D=%d top_k=%d", B, N, D, top_k);
  return layer_fusion_apply(acc, tokens, B, N, D, top_k, a_cls, a_diag, idx_out, tmp, as_stream(st));
}

extern "C" size_t sg_outlier_scratch_bytes(int B, int D, int k) { return refine_scratch_bytes(B, D, k); }

extern "C" int sg_outlier_suppress(float* feats, const float* attn_cls, const float* attn_diag, int B, int gh, int gw, int D, int top_k,
                                   float contamination_temp, int32_t* out_idx, void* scratch, sg_stream st) {
  SG_REQUIRE(feats && attn_cls && attn_diag && out_idx && scratch, "sg_outlier_suppress: null pointer");
  hipStream_t s = as_stream(st);
  const int n = gh * gw, N = n + 1, k = top_k < n ? top_k : n;
  SG_TRY(select_topk(attn_cls, attn_diag, B, N, k, 0, out_idx, s));
  // feats is patch-only [B,n,D]: token t of the kernels = 1 + cell, so shift the base by one row
  return neighbour_refine(feats - D, (int64_t)n * D, D, out_idx, B, gh, gw, D, k, 1, contamination_temp, scratch, s);
}

extern "C" int sg_weak_token_replace(float* feats, const float* attn_diag, int B, int gh, int gw, int D, int top_k, int32_t* out_idx,
                                     void* scratch, sg_stream st) {
  SG_REQUIRE(feats && attn_diag && out_idx && scratch, "sg_weak_token_replace: null pointer");
  hipStream_t s = as_stream(st);
  const int n = gh * gw, N = n + 1, k = top_k < n ? top_k : n;
  SG_TRY(select_topk(attn_diag, attn_diag, B, N, k, 1, out_idx, s));
  return neighbour_refine(feats - D, (int64_t)n * D, D, out_idx, B, gh, gw, D, k, 0, 0.f, scratch, s);
}
