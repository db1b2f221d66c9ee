/*
 * segearth_hip.h -- C ABI of libsegearth_hip.so: the MI355X (gfx950) implementation of the
 * sliding-window CLIP dense-feature path of CLIP-Decontamination / SegEarth-OV.
 *
 * This is the drop-in boundary.  Every entry point replaces one seam of the
 * reference's Python hot path; the reference file:line it stands in for is cited on each.
 * Conventions
 *   - plain C types only: device pointers, sizes, a hipStream_t passed as void*;
 *   - the CALLER owns every input, output and workspace buffer (device memory); the library
 *     allocates only in sg_create / sg_vit_set_tensor / sg_jbu_set_tensor (packed weights) and
 *     frees in sg_destroy; no hidden per-call hipMalloc, no host synchronisation in any call
 *     that takes a stream;
 *   - every call returns 0 on success or a negative sg_status; the message of the last
 *     failure on the calling thread is returned by sg_last_error(); nothing aborts or throws;
 *   - calls are asynchronous on the given stream and re-entrant across contexts: the library keeps no mutable per-process
 *     state (per-device launch bookkeeping is keyed by device and thread-safe; the measurement and tuning hooks below act on
 *     the calling thread only); an entry point that takes a context makes the context's device current for its duration, the
 *     context-free ops run on the caller's current device (the one the stream belongs to).
 *   - "tokens" are token-major [B, N, D] row-major (N = 1 + gh*gw, CLS first).
 */
#ifndef SEGEARTH_HIP_H
#define SEGEARTH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sg_context sg_context;
typedef void* sg_stream;            /* hipStream_t */

enum sg_status {
  SG_OK = 0,
  SG_ERR_INVALID = -1,    /* bad argument / unsupported shape */
  SG_ERR_HIP = -2,        /* a HIP runtime call failed */
  SG_ERR_STATE = -3,      /* weights missing, text not set, workspace too small ... */
};

enum sg_precision {       /* arithmetic the ViT GEMMs / attention run in */
  SG_PREC_F32 = 0,        /* parity mode: f32 MFMA (exact fmaf chains), materialised attention */
  SG_PREC_BF16 = 1,       /* throughput mode: bf16 MFMA, f32 accumulate, f32 residual stream + LN */
  SG_PREC_FP8 = 2,        /* bf16 mode whose QKV / fc / proj linears of the ordinary blocks run on fp8 (OCP e4m3) MFMA with per-token and
                             per-output-channel absmax scales; attention, out-proj, the last block and everything else stay bf16 / f32 */
  SG_PREC_F16 = 3,        /* throughput mode on IEEE f16 operands (v_mfma_*_f16: the bf16 rate, 3 more mantissa bits): the reference's own
                             GPU arithmetic (segmentor.py:467 .half(), open_clip/model.py:142 fp32 LayerNorm).  f32 accumulate, f32
                             residual stream / LN / softmax statistics as in bf16 mode; stores saturate at +-65504 */
  SG_PREC_F16X2 = 4,      /* parity AT SPEED: every GEMM / attention operand is held as two f16 planes x = hi + lo (within max(2^-22 |x|,
                             2^-25): 22 significant bits from |x| = 2^-3 up, below that the 2^-25 floor of lo's f16 subnormals) and every
                             product is issued as hi.hi + hi.lo + lo.hi on the f16 matrix pipe into one f32 accumulator -- the error of an f32
                             fmaf chain (tools/h2_probe.hip) at a third of the f16 MFMA rate instead of the 1/16 of the f32 MFMA.  f32 residual
                             stream / LayerNorm / softmax statistics, exact expf / erff activations.  Logits within 1e-3 of the reference's fp32 CPU
                             path with arg-max identical up to fp32 ties, like SG_PREC_F32 (same reference bar: segmentor.py:467 .half() is the
                             reference's own GPU arithmetic; its CPU path, the oracle, is fp32).  Values beyond +-131008 are not representable. */
};

/* last-block attention variants: reference open_clip/transformer.py:858-932 (custom_attn),
 * SG_GEM: reference gem/gem_utils.py:60-199 */
enum sg_model_type {
  SG_VANILLA = 0, SG_MASKCLIP = 1, SG_CLEARCLIP = 2, SG_SCLIP = 3, SG_SEGEARTH = 4, SG_SFP = 5,
  SG_EXPERIMENTAL = 6, SG_NACLIP = 7, SG_NONLY = 8, SG_GAV = 9, SG_GEM = 10,
};

enum sg_image_format {
  SG_IMG_F32_NCHW = 0,    /* normalised float planes: what predict() receives (segmentor.py:453-467) */
  SG_IMG_U8_NHWC = 1,     /* raw RGB bytes; (x-mean)/std of segmentor.py:64-67 fused into the load */
};

/* Architecture of the vision tower: reference open_clip/model_configs/ViT-*.json,
 * open_clip/transformer.py:341-362 */
typedef struct sg_vit_desc {
  int32_t width;          /* D */
  int32_t layers;         /* L */
  int32_t heads;          /* H */
  int32_t patch;          /* P */
  int32_t embed_dim;      /* E */
  int32_t grid0;          /* native positional grid side (image_size / patch) */
  int32_t mlp_width;      /* 4D */
  int32_t quick_gelu;     /* 1: x*sigmoid(1.702x) (transformer.py:35-38), 0: exact erf GELU */
  int32_t precision;      /* enum sg_precision */
} sg_vit_desc;

/* Knobs of one forward: the kwargs of VisionTransformer.forward (transformer.py:538) plus the
 * refiner modules the reference hangs on net.visual (segmentor.py:196-274). */
typedef struct sg_forward_opts {
  int32_t model_type;             /* enum sg_model_type */
  int32_t ignore_residual;        /* transformer.py:627-643 */
  int32_t similarity_enabled;     /* similarity_enhancement.py; 0 = module not installed */
  float   similarity_weight;
  float   similarity_temperature;
  int32_t similarity_add_self;
  int32_t outlier_enabled;        /* outlier_suppression.py; captures block L-2 attention */
  int32_t outlier_top_k;
  float   outlier_contamination_temp;
  int32_t selfattn_enabled;       /* self_attention_enhancement.py (inert unless outlier_enabled, R6) */
  int32_t selfattn_mode;          /* 0 feature, 1 attention */
  int32_t selfattn_top_k;
  float   selfattn_strength;
  float   selfattn_threshold;
  int32_t gem_depth;              /* GEM: blocks -1..-(depth-1) are dual-stream (gem_wrapper.py:24-45) */
  int32_t layer_fusion_enabled;   /* apply_layer_fusion (transformer.py:598-607,630-637,647-690): EMA of the head-averaged attention of every
                                     block; with an outlier suppressor its top_k columns are zeroed, rows L1-renormalised and
                                     output = attn @ output -- the refiners are then skipped, as in the reference.  The reference's
                                     view(N, heads, L, L) only runs for heads == 1; that case pins the semantics. */
  float   layer_fusion_lambda;
} sg_forward_opts;

/* Where the tiles of one launch come from: one scene + a window per tile, so that cropping,
 * zero padding to a patch multiple (segmentor.py:418-431, 534-546) and im2col happen on the
 * device in one pass. */
typedef struct sg_tile_batch {
  const void* scene;              /* device: [C=3,H,W] f32 planes or [H,W,3] u8 */
  int32_t format;                 /* enum sg_image_format */
  int32_t scene_h, scene_w;
  const int32_t* windows;         /* device int32 [n_tiles][4] = y1,y2,x1,x2 */
  const int32_t* scene_index;     /* device int32 [n_tiles] image index of each tile, or NULL (all tiles from image 0) */
  int64_t scene_stride;           /* elements between consecutive images when `scene` holds a batch [B,3,H,W] / [B,H,W,3] */
  int32_t n_tiles;
  int32_t tile_h, tile_w;         /* window size (all tiles of a launch share it) */
  int32_t pad_l, pad_t;           /* compute_padsize(): zeros added left / top */
  int32_t grid_h, grid_w;         /* (tile + pad) / patch */
} sg_tile_batch;

const char* sg_last_error(void);
int sg_version(void);

/* ---- live kernel timing (measurement only; used by bench.py's roofline) -------------------------
 * HIP events bracket every launch of a kernel family on the stream it is launched on.
 * category: 0 = bf16 MFMA GEMM (small-shape tile variants), 1 = fused attention, 2 = f32 MFMA GEMM,
 *           3 = the persistent bf16 GEMM (every large ViT linear; the kernel bench.py's roofline prices: all three instantiations),
 *           4 = fp8 GEMM, 5 / 6 = the persistent GEMM's folded-LayerNorm consumer / producer instantiations alone (subsets of 3).
 *           Read after synchronising.  The state belongs to the calling thread (enable, launch and read on one thread). */
int sg_profile_enable(int capacity);
int sg_profile_disable(void);
int sg_gemm_persist_last_kstep(void);   /* K step in elements of the calling thread's last persistent bf16 / f16 GEMM launch: 64 (gemm_bf16_persist_k64),
                                         * 32 (gemm_bf16_persist: K / 64 < 4 or tuning code 38), 0 = none yet */
const char* sg_gemm_last_kernel(void);   /* the calling thread's last launch through the 2-byte / two-plane / fp8 GEMM: "<family> grid=<x> ngroup=<n>"
                                          * with family persist_k64, persist_k32, h2_persist, fp8_persist, pingpong, h2_pingpong, ring128,
                                          * h2_ring128, fp8_ring128, fp8_ring256x256 or one of the MXFP8 forms fp8_mx_ring256x256_fc1 / _fc2 (MX
                                          * output after QuickGELU / GELU), _proj (MX operand, f32 C + residual, no activation), _mxa (any other MX
                                          * operand form) or _out (any other MX output form); grid = workgroups (persistent) or tiles along x;
                                          * ngroup = the persistent kernel's N-group size (0 = raster order); "none" when its last GEMM call
                                          * launched nothing.  The text stays valid until the thread's next query. */
const char* sg_attention_last_kernel(void);   /* the calling thread's last launch through the fused attention (sg_attention_raw, sg_op_attention,
                                              * the towers): "attn dh=<32|64|80|128> ts=<1|2> gk=<0 lean|1 generic|2 Experimental> multi=<0|1>
                                              * pv=<0 log-sum-exp only|1> kind=<bf16|f16|h2> order=<head|qblock|images> nb=<LDS buffers> grid=<x>", or of
                                              * its statistics kernel: "stats_fast lph=<4|8|16> kind=<bf16|f16> grid=<blocks>" / "stats_generic lph=0
                                              * kind=<bf16|f16|h2> grid=<blocks>"; "none" when its last such call launched nothing.  Valid until the
                                              * thread's next query. */
const char* sg_attention_last_body(void);     /* the body of that same launch: "dma" (the lean and the 'Experimental' dh-64 kernels staging K / V by
                                              * LDS-DMA), "staged" (register-staged K / V: every other fused-attention kernel, the lean dh-64 one
                                              * under tuning code 39 and the 'Experimental' dh-64 one under code 40), "stats" (a statistics kernel)
                                              * or "none". */
int sg_set_gemm_config(int cfg);   /* tuning hook (calling thread only), -1 = automatic; 31 = the fp8 GEMM on its ring kernels at every shape,
                                    * 32 = the fp8 GEMM's persistent kernel from K = 512 on (not only from K = 2048), 34 = LayerNorm as its own
                                    * pass (no folding), 36 = no small-launch dispatch (a few-tile GEMM stays on the persistent kernel), 38 = the
                                    * persistent kernel with 32-element K steps (same results as the default 64-element one), 39 = the fused
                                    * attention's lean dh-64 kernels with register-staged K / V instead of LDS-DMA (the previous body, bit-identical
                                    * results), 40 = the dh-64 'Experimental' last-block attention on its register-staged body (likewise);
                                    * 1000 + v = tile order of the persistent kernel; 2000 + n = at most n workgroups for every persistent
                                    * kernel (2000 = one per CU).  Any other code is refused (SG_ERR_INVALID, the setting unchanged). */
int sg_profile_read(int category, double* total_ms, double* total_flops, int64_t* launches, int64_t* dropped);

/* ---- context and weights ------------------------------------------------------------------
 * sg_create replaces create_model(...) + .eval().to(device) (segmentor.py:69-131) for the
 * vision tower only; weights arrive by their visual.* state-dict names
 * (e.g. "transformer.resblocks.3.attn.in_proj_weight", open_clip/transformer.py:372-442). */
int  sg_create(sg_context** out, int device, const sg_vit_desc* desc);
void sg_destroy(sg_context* ctx);
int  sg_vit_set_tensor(sg_context* ctx, const char* name, const float* dev_f32, int64_t numel, sg_stream s);
int  sg_vit_finalize(sg_context* ctx, sg_stream s);

/* ---- the vision tower -----------------------------------------------------------------------
 * sg_vit_forward replaces net.encode_image(img, model_type, ignore_residual, output_cls_token=True, ...)
 * (open_clip/model.py:265-286 -> open_clip/transformer.py:538-775) and, for SG_GEM,
 * net.visual(img) (gem/gem_utils.py:159-199).
 *   out_cls    [B,E] f32 (untouched for SG_GEM), out_tokens [B,gh*gw,E] f32. */
size_t sg_vit_workspace_bytes(const sg_context* ctx, int n_tiles, int grid_h, int grid_w, const sg_forward_opts* o);
int sg_vit_forward(sg_context* ctx, const sg_tile_batch* tiles, const sg_forward_opts* o,
                   float* out_cls, float* out_tokens, void* workspace, size_t workspace_bytes, sg_stream s);

/* ---- segmentation head ----------------------------------------------------------------------
 * sg_cosine_logits replaces segmentor.py:309-336,374-386: CLS normalise + cls_logits, global
 * debias tokens -= cls * (cos(tokens,cls) * factor), L2 normalise, tokens @ T^T, + lambda*cls_logits.
 *   tokens [B,n,E], cls [B,E] (may be NULL when both factors are 0), text [Q,E] -> logits [B,Q,n]. */
int sg_cosine_logits(const float* tokens, const float* cls, const float* text, int B, int n, int E, int Q,
                     float global_debias_factor, float cls_token_lambda, float* logits, sg_stream s);
/* The per-pixel logits behind the upsampler (segmentor.py:374-379, no global debias: it ran before the upsampler) for the exact tower mode
 * SG_PREC_F16X2: the [n, E] x [E, Q] product on the f16 matrix pipe with both operands as two f16 planes (f32-grade results, three MFMAs per
 * product; magnitudes beyond +-131 008 saturate, as everywhere in that mode).  Same layouts as sg_cosine_logits; shapes it does not take
 * (Q > 16, E % 32 != 0, n < 4096) are forwarded to sg_cosine_logits.
 * Precision: every feature and text element is held as hi + lo with a representation error of max(2^-22 |x|, 2^-25) -- an ABSOLUTE floor
 * of 2^-25 per element, so the kernel is not scale-invariant although the cosine it computes is.  f32-grade for per-element magnitudes of
 * 1e-2 and above; below that the error grows as 1 / scale.  CPU emulation of the split (E = 768, Q = 16, max |err| against float64) by
 * token scale: 1e2 6e-8, 1 7e-8, 1e-2 2.6e-7, 1e-3 2.5e-6, 1e-4 2.5e-5, 1e-5 2.3e-4.  Measured on an MI355X
 * (tests/test_gpu_head_reference.py): 7.5e-7 over row scales 2^-6 .. 2^6 (E = 32 / 96), 7.1e-5 with every row at 2^-13 (E = 96, Q = 13;
 * the per-element bound there is 2.9e-4).  Rescale the rows before the call if they can be smaller than that. */
int sg_cosine_logits_two_plane(const float* tokens, const float* cls, const float* text, int B, int n, int E, int Q,
                               float cls_token_lambda, float* logits, sg_stream s);

/* sg_stitch replaces the bilinear upsample + un-pad + overlap-add + count-normalise of
 * segmentor.py:388-391,436-447 in a write-once form: canvas[q,y,x] = mean over covering tiles
 * (raster order) of bilinear(tile_logits)[y - y1 + pad_t, x - x1 + pad_l].
 *   tile_logits [T,Q,gh,gw] f32, windows int32 [T][4] (y1,y2,x1,x2), canvas [Q,H,W] f32.
 *   up_h/up_w: the size tiles are bilinearly resized to (tile + pad). */
int sg_stitch(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw,
              int up_h, int up_w, int pad_t, int pad_l, int H, int W, float* canvas, sg_stream s);

/* ---- weighted window blending: sg_stitch with every tile feathered towards its own window edges -----------------------------------
 * The ramp is an f32 table r[0 .. L-1] in device memory, L = ramp_len >= 1, every entry finite and > 0.  For a pixel (y, x) inside
 * window t = (y1, y2, x1, x2):
 *     dy = min(y - y1, y2 - 1 - y),  dx = min(x - x1, x2 - 1 - x),  w_t = fl32(r[min(dy, L-1)] * r[min(dx, L-1)]).
 * The distances are taken in the window's own coordinates, so the shifted windows of a canvas band give the weights of the whole
 * canvas.  With u_t the bilinear value sg_stitch takes from tile t (the same taps, the same expression):
 *     acc = sum_t w_t u_t over the covering tiles in raster order, each step one fused multiply-add; wsum = sum_t w_t in that order;
 *     canvas = wsum > 0 ? acc / wsum : 0.
 * A table of the one entry 1.0f is the uniform mean: byte for byte sg_stitch.  No atomics, every pixel is written once by its own
 * thread, repeats are byte-identical.  The host builds r[d] = (d + 0.5) / R ("linear") or sin^2(pi/2 (d + 0.5) / R) ("hann") for
 * d < R and r[R] = 1, L = R + 1, in float64 rounded once; the kernels only read the table.  "hann" with R = crop / 2 at a stride of
 * crop / 2 is a partition of unity away from the image border.
 * The four entries take their counterpart's arguments with (ramp, ramp_len) before the stream and refuse, before any device work, a
 * NULL ramp and a ramp_len outside [1, SG_BLEND_MAX_RAMP].  sg_label_head_blend[_multi]: sg_label_head[_multi] on the blended value
 * (acc / wsum where that one has acc / count), every later statement the same; the multi entries equal the single ones per image. */
#define SG_BLEND_MAX_RAMP 2048
int sg_stitch_blend(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                    int pad_l, int H, int W, float* canvas, const float* ramp, int ramp_len, sg_stream s);
int sg_stitch_blend_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                          int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                          const int64_t* canvas_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t canvas_elems,
                          float* canvases, const float* ramp, int ramp_len, sg_stream s);
int sg_label_head_blend(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                        int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                        int64_t* labels, float* conf, const float* ramp, int ramp_len, sg_stream s);
int sg_label_head_blend_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                              int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                              const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                              const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, int64_t* labels,
                              float* conf, const float* ramp, int ramp_len, sg_stream s);

/* F.interpolate(mode='bilinear', align_corners=False) on [C,h,w] -> [C,H,W] (segmentor.py:389,449) */
int sg_resize_bilinear(const float* src, int C, int h, int w, float* dst, int H, int W, sg_stream s);

/* sg_postprocess replaces postprocess_result (segmentor.py:475-489): x logit_scale, softmax over
 * queries, per-class max over synonyms, argmax, prob_thd -> bg_idx.
 *   logits [Q,H,W]; query_idx int32 [Q]; probs [K,H,W] f32 (may be NULL); labels int64 [H,W]. */
int sg_postprocess(const float* logits, const int32_t* query_idx, int Q, int K, int H, int W, float logit_scale,
                   float prob_thd, int bg_idx, float* probs, int64_t* labels, sg_stream s);
/* ---- multi-canvas head: the images of a packed batch in one launch each ------------------------------------------------------
 * sg_stitch_multi replaces segmentor.py:388-391,436-447 for N images at once: the tiles of image n are [first, first + count) of the
 * call's tile list (image-major), windows are in that image's own coordinates and tile_image[t] names the image of tile t; its canvas
 * [Q,H,W] is written at canvas_offset[n] (elements) of `canvases`.  All tiles of one call share gh, gw, up_h, up_w, pad_t, pad_l (one
 * tile size).  The grid is flattened over (image, 64 x 4 pixel block): block_prefix [N+1] = exclusive prefix sum of
 * ceil(W/64) * ceil(H/4), total_blocks = block_prefix[N].  Each canvas is bit-identical to sg_stitch on that image alone.
 *   tile_logits [T,Q,gh,gw] f32, windows int32 [T][4], tile_image int32 [T], image_hw int32 [N][2] (H,W), image_tiles int32 [N][2]
 *   (first, count), canvas_offset int64 [N], block_prefix int64 [N+1] -- all device memory; canvas_elems = size of `canvases`.
 *   HBM-bound, write-once: reads the tile logits (~1x, overlapping windows re-read through L2) and writes Q*sum(H*W)*4 bytes. */
int sg_stitch_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                    int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                    const int64_t* canvas_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t canvas_elems,
                    float* canvases, sg_stream s);
/* sg_postprocess_multi replaces segmentor.py:449 + 475-489 for N canvases at once: canvas n [Q,h,w] at canvas_offset[n] ->
 * labels int64 [H,W] at out_offset[n] and (probs != NULL) probs f32 [K,H,W] at K * out_offset[n], where (H,W) = out_hw[n] is the
 * image's ori_shape.  When it differs from the canvas the align_corners=False bilinear resize is evaluated per output pixel (no
 * resized canvas is written).  Bit-identical to sg_resize_bilinear + sg_postprocess per image.  block_prefix [N+1] = exclusive prefix
 * sum of ceil(H*W/256); canvas_elems / out_pixels = sizes of `canvases` / `labels`.  Reads Q*h*w*4 B, writes (8 + 4K) B per pixel. */
int sg_postprocess_multi(const float* canvases, const int32_t* canvas_hw, const int64_t* canvas_offset, const int32_t* out_hw,
                         const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t canvas_elems,
                         int64_t out_pixels, const int32_t* query_idx, int Q, int K, float logit_scale, float prob_thd, int bg_idx,
                         float* probs, int64_t* labels, sg_stream s);
/* ---- large vocabularies: any Q --------------------------------------------------------------------------------------------------
 * sg_cosine_logits_wide: the contract and output layout [B,Q,n] of sg_cosine_logits for any Q >= 1.  The text rows pass through LDS
 * in chunks of as many rows as fit, inside one launch; a token's features are read once and stay in registers.  A shape that
 * sg_cosine_logits takes (the whole text matrix fits in LDS) runs its kernel: the same bits.  Beyond it the expressions per (token, q)
 * are the same, but the compiler fuses the debias sums in another order: within an ulp or two of that arithmetic.  E % 4 == 0, E <= 2048. */
int sg_cosine_logits_wide(const float* tokens, const float* cls, const float* text, int B, int n, int E, int Q,
                          float global_debias_factor, float cls_token_lambda, float* logits, sg_stream s);
/* sg_postprocess_wide: the contract of sg_postprocess for any Q (sg_postprocess holds the queries in registers and stops at 64).
 * Three passes over the canvas: maximum, sum, per-class maximum written through probs[class(q)] by the pixel's own thread.  Plain,
 * not tuned: reads the canvas three times. */
int sg_postprocess_wide(const float* logits, const int32_t* query_idx, int Q, int K, int H, int W, float logit_scale,
                        float prob_thd, int bg_idx, float* probs, int64_t* labels, sg_stream s);
/* sg_label_head: sg_stitch + sg_postprocess without the canvas, labels only, any Q >= 1 and 1 <= K <= Q.  Inputs as sg_stitch plus
 * the post-process parameters.  Per pixel and query the stitched value is sg_stitch's (the same taps, covering tiles summed in raster
 * order, divided by the count); the queries pass through registers in chunks with an online maximum and sum of exp.
 *   labels int64 [H,W] = class of the largest scaled logit (lowest class index among equal ones; query_idx need not be sorted; with
 *   K == Q class(q) = q, as in sg_postprocess), bg_idx where conf < prob_thd; conf f32 [H,W] (may be NULL) = the winning class's
 *   probability 1 / sum_q exp(v_q - v_max).  No buffer proportional to Q*H*W, no atomics; repeats are byte-identical.
 * Against sg_stitch + sg_postprocess the label can differ only where two class probabilities are closer than their f32 rounding. */
int sg_label_head(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                  int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                  int64_t* labels, float* conf, sg_stream s);
/* sg_label_head_multi: sg_label_head for the tiles of N images in one launch, descriptors as sg_stitch_multi; labels (and conf) of
 * image n are written at out_offset[n] pixels of the flat outputs (sg_postprocess_multi's label layout), out_pixels = their size.
 * Byte-identical to sg_label_head per image. */
int sg_label_head_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                        int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                        const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                        const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, int64_t* labels,
                        float* conf, sg_stream s);
/* sg_prob_head: sg_stitch + sg_postprocess without the canvas, class probabilities AND labels, any Q >= 1 and 1 <= K <= Q.  Inputs as
 * sg_label_head; probs f32 [K,H,W] must not be NULL (labels alone: sg_label_head), labels int64 [H,W].  Contract: probs and labels are
 * byte-identical to sg_stitch followed by sg_postprocess for Q <= 64 and by sg_postprocess_wide beyond -- the stitched value of a
 * (pixel, query) is sg_stitch's (same taps, covering tiles summed in raster order, divided by the count, 0 where no tile covers) and
 * the tail is that entry's own code -- and repeats are byte-identical.  Q <= 64: one gather, the pixel's Q values stay in registers.
 * Q > 64: three gathers (maximum, sum, per-class maximum), nothing held per query.  No buffer proportional to Q*H*W, no atomics. */
int sg_prob_head(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                 int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                 float* probs, int64_t* labels, sg_stream s);
/* sg_prob_head_multi: sg_prob_head for the tiles of N images in one launch, descriptors as sg_label_head_multi.  The labels of image n
 * are written at out_offset[n] pixels of `labels` and its probs [K,H,W] at K * out_offset[n] elements of `probs` (sg_postprocess_multi's
 * layout); out_pixels = the size of `labels`, `probs` holds K * out_pixels.  Contract: per image byte-identical to sg_prob_head on that
 * image alone, hence to sg_stitch_multi + sg_postprocess_multi (Q <= 64) or + sg_postprocess_wide per image (beyond); repeats are
 * byte-identical. */
int sg_prob_head_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                       int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                       const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                       const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, float* probs,
                       int64_t* labels, sg_stream s);
/* sg_topk_head: the k best classes of every pixel with their probabilities, straight from the tile logits: no [Q,H,W] canvas and no
 * [K,H,W] probability planes.  Inputs as sg_label_head, any Q >= 1, 1 <= K <= Q, 1 <= k <= min(SG_TOPK_MAX, K).  Outputs are planes:
 * classes int32 [k,H,W] and probs f32 [k,H,W]; the 8k bytes per pixel they hold are the call's only writes.  Contract:
 *   - the probability of a class is the one sg_postprocess defines: the softmax over all Q scaled logits, the maximum over the class's
 *     queries (query_idx need not be sorted; with K == Q class(q) = q; a query whose class lies outside [0,K) takes part in the sum only);
 *   - slots are in descending order of that probability, equal values by ascending class; plane 0 is sg_label_head's label before any
 *     threshold and its probability is sg_label_head's conf, byte for byte (thresholding it is the caller's: there is no prob_thd here);
 *   - a class that owns no query never appears -- a deliberate difference from the canvas route, where such a class has probability 0
 *     and would be listed after the others; the slots left unfilled hold class -1 and probability 0;
 *   - a pixel no tile covers has every stitched value 0: classes in ascending index, equal probabilities;
 *   - repeats are byte-identical (no atomics, every element written by its pixel's own thread in an order fixed by pixel and query);
 *   - against sg_stitch + sg_postprocess + a stable descending sort, the order can differ only where two class probabilities are closer
 *     than their f32 rounding.
 * The queries pass through registers in chunks as in sg_label_head; a sorted list of k (value, class) pairs is kept per pixel. */
#define SG_TOPK_MAX 8
int sg_topk_head(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                 int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, int k, int32_t* classes, float* probs,
                 sg_stream s);
/* sg_topk_head_multi: sg_topk_head for the tiles of N images in one launch, descriptors as sg_label_head_multi.  The planes [k,H,W] of
 * image n start at k * out_offset[n] elements of `classes` and of `probs` (sg_prob_head_multi's layout with k for K); out_pixels = the
 * sum of H * W, both outputs hold k * out_pixels.  Byte-identical to sg_topk_head per image. */
int sg_topk_head_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                       int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                       const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                       const int32_t* query_idx, int K, float logit_scale, int k, int32_t* classes, float* probs, sg_stream s);
/* ---- the label and top-k heads at another ori_shape ----------------------------------------------------------------------------------
 * segmentor.py:447-449 (preds / count, then the bilinear resize to ori_shape) fused into sg_label_head / sg_topk_head: the outputs are
 * [out_h, out_w] maps over the [H, W] canvas, and neither the canvas nor the resized canvas exists.  Output pixel (Y, X) takes the
 * align_corners=False taps of sg_resize_bilinear along each axis, the stitched value of each of its four canvas pixels as sg_stitch
 * defines it (covering tiles in raster order, divided by that pixel's own count, 0 where no tile covers -- the division comes BEFORE the
 * blend, neighbouring taps can have different counts), blends them top row, bottom row, then the two, and hands the result to the
 * per-query statements of the unresized head.  Taps, gather and blend are compiled with every product rounded (no fused multiply-add),
 * so against sg_stitch + sg_resize_bilinear + sg_postprocess a value is within a few f32 roundings, not byte-identical; with
 * out = (H, W) the taps are the identity and the same kernel runs (it does not dispatch to the unresized entry).
 * flags picks how a block of 64 x 4 output pixels gets its canvas values; both forms call one device function per canvas pixel and give
 * the same bytes:
 *   SG_RESIZED_DIRECT  every thread gathers its own four canvas pixels; any scale;
 *   SG_RESIZED_STAGED  the block stitches its canvas footprint, (ceil(4 H / out_h) + 2) x (ceil(64 W / out_w) + 2) pixels at most, once
 *                      per chunk of 8 queries into 16 KiB of LDS and every thread blends from there; refused when that product exceeds
 *                      512 pixels;
 *   SG_RESIZED_AUTO    staged where it fits and the output is larger than the canvas along both axes (measured 2.1 to 2.8 times the
 *                      direct form's speed at 448 -> 1024 and at 1.5x), direct otherwise (at the canvas's own size direct was 5 to 10 %
 *                      faster; a mixed up / down scale was not measured). */
#define SG_RESIZED_AUTO 0
#define SG_RESIZED_DIRECT 1
#define SG_RESIZED_STAGED 2
/* sg_label_head_resized: sg_label_head's arguments, outputs and contract with labels int64 [out_h,out_w] and conf f32 [out_h,out_w]. */
int sg_label_head_resized(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                          int pad_l, int H, int W, int out_h, int out_w, const int32_t* query_idx, int K, float logit_scale,
                          float prob_thd, int bg_idx, int64_t* labels, float* conf, int flags, sg_stream s);
/* sg_label_head_resized_multi: the tiles of N images in one launch.  image_hw[n] is the canvas size and image_tiles[n] the tiles as in
 * sg_stitch_multi; out_hw[n] is the image's ori_shape, out_offset[n] its first pixel in the flat outputs, block_prefix [N+1] the
 * exclusive prefix sum of ceil(out_w / 64) * ceil(out_h / 4), out_pixels the size of `labels` (sg_postprocess_multi's layout: canvas
 * size, output size, offsets in output pixels).  A descriptor that would leave the buffers makes its blocks return without writing.
 * Byte-identical to sg_label_head_resized per image.  An image whose footprint does not fit the stage runs the direct form whatever
 * flags says (the sizes are device arrays; a caller that wants the refusal checks them itself). */
int sg_label_head_resized_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                                int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                                const int32_t* out_hw, const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks,
                                int64_t out_pixels, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                                int64_t* labels, float* conf, int flags, sg_stream s);
/* sg_topk_head_resized: sg_topk_head's arguments, outputs and contract with planes [k,out_h,out_w]; plane 0 is
 * sg_label_head_resized's label before the threshold and its conf, byte for byte. */
int sg_topk_head_resized(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                         int pad_l, int H, int W, int out_h, int out_w, const int32_t* query_idx, int K, float logit_scale, int k,
                         int32_t* classes, float* probs, int flags, sg_stream s);
/* sg_topk_head_resized_multi: descriptors as sg_label_head_resized_multi; the planes [k,out_h,out_w] of image n start at
 * k * out_offset[n] elements of `classes` and `probs`, which hold k * out_pixels.  Byte-identical to sg_topk_head_resized per image. */
int sg_topk_head_resized_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                               int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                               const int32_t* out_hw, const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks,
                               int64_t out_pixels, const int32_t* query_idx, int K, float logit_scale, int k, int32_t* classes,
                               float* probs, int flags, sg_stream s);
/* ---- test-time augmentation: V views of one image merged at the output size ----------------------------------------------------------
 * mmseg's SegTTAModel over postprocess_result (segearth_segmentor.py:301-326): every view's seg_logits are class probabilities, the
 * views' probabilities are summed, divided by V, and the arg-max is taken.  A view is the image resized by a scale and possibly
 * mirrored along the width, slid like any image: it has its own tile logits [T_v,Q,gh_v,gw_v], windows, up size, pad and canvas
 * (h_v, w_v).  For output pixel (Y, X) of the (out_h, out_w) map and view v:
 *   X_v    = out_w - 1 - X if the view is flipped, else X;
 *   r_v[q] = the value at (Y, X_v) of the view's stitched canvas resized to (out_h, out_w), exactly as sg_label_head_resized defines
 *            it (every tap divided by its own count, the same taps and blend, every product rounded);
 *   p_v    = softmax_q(logit_scale * r_v), that entry's online recurrence in its chunk order;
 *   P_v[c] = the largest p_v[q] over the queries of class c (query_idx[q] == c; K == Q: class q), 0 for a class without a query;
 *   P[c]   = (P_0[c] + P_1[c] + ... in ascending v) / V;  label = the first c with the largest P[c];  conf = P[label];
 *   label  = bg_idx where conf < prob_thd.
 * sg_tta_head does this in one launch, one block per 64 x 4 output pixels, with no canvas, no per-view planes and no atomics; every
 * output element is written by its pixel's thread in an order fixed by (pixel, view, query), so repeats are byte-identical.  With
 * V = 1 and flip = 0 conf carries sg_label_head_resized's bytes, and so do the labels except where two classes' distinct best logits
 * round to the same probability (this entry compares the probabilities).
 *   tile_logits  the views' tile logits back to back, logit_elems floats = sum of T_v * Q * gh_v * gw_v;
 *   windows      int32 [total_tiles,4], the views' windows back to back, each in its own view's canvas coordinates;
 *   views        HOST array int32 [V][SG_TTA_VIEW_FIELDS]: T_v, first tile (= the sum of the T before it), gh, gw, up_h, up_w, pad_t,
 *                pad_l, h, w, flip (0 / 1).  It is read during the call and travels as a kernel argument;
 *   labels int64 [out_h,out_w]; conf f32 [out_h,out_w] or NULL; probs f32 [K,out_h,out_w] (the mean planes P) or NULL;
 *   flags        SG_RESIZED_*, per view: a view whose footprint does not fit the stage runs the direct form (same bytes).
 * Refused with the outputs untouched: V outside [1, SG_TTA_MAX_VIEWS], a non-positive size, Q > 64, K outside [1, Q], bg_idx outside
 * [0, K), a flip that is neither 0 nor 1, views whose tiles do not follow each other or do not add up to the buffers.
 * LDS: 1 KiB per class but the last (the per-view class maxima, one column per thread) beside the 16 KiB stage. */
#define SG_TTA_MAX_VIEWS 8
#define SG_TTA_VIEW_FIELDS 11
int sg_tta_head(const float* tile_logits, int64_t logit_elems, const int32_t* windows, int total_tiles, const int32_t* views, int V, int Q,
                int out_h, int out_w, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, int64_t* labels,
                float* conf, float* probs, int flags, sg_stream s);
/* The same merge for what the fused entry does not take (Q > 64, a weighted stitch, the JBU upsampler, whole-image inference): every
 * view goes through the existing probability tail at (out_h, out_w), then
 *   sg_tta_accumulate  acc[c,y,x] = (first ? 0 : acc[c,y,x]) + probs_view[c,y, flip ? out_w-1-x : x]   (acc and probs_view f32
 *                      [K,out_h,out_w], distinct buffers), views in ascending order;
 *   sg_tta_finish      P = acc / V, label, conf and threshold as above; probs (NULL, or f32 [K,out_h,out_w], or acc itself) gets P.
 * Plain elementwise kernels; one view's planes and the accumulator are all that is alive. */
int sg_tta_accumulate(const float* probs_view, int K, int out_h, int out_w, int flip, float* acc, int first, sg_stream s);
int sg_tta_finish(const float* acc, int V, int K, int out_h, int out_w, float prob_thd, int bg_idx, int64_t* labels, float* conf,
                  float* probs, sg_stream s);
/* Label / confidence images of postprocess_result (segmentor.py:501-531): mask_rgb [H,W,3] = palette[clip(label)] (_colorize_mask,
 * :580-590); heat_rgb [H,W,3] = (g, 0, 255-g) with g = uint8(clip(max_k probs, 0, 1) * 255) (_to_colormap without OpenCV, :604-608;
 * OpenCV's JET table is not reproduced).  Either output may be NULL. */
int sg_render_maps(const int64_t* labels, const float* probs, const uint8_t* palette, int K, int H, int W, uint8_t* mask_rgb,
                   uint8_t* heat_rgb, sg_stream s);

/* ---- token refinements as stand-alone ops (same arithmetic as inside sg_vit_forward) ----------
 * sg_outlier_suppress replaces OutlierSuppressionModule.forward (outlier_suppression.py:83-214):
 *   feats [B,gh*gw,D] f32 in place; attn_cls [B,N] = head-averaged A[0,:], attn_diag [B,N] = diag(A);
 *   out_idx int32 [B,k] receives the selected tokens; scratch >= sg_outlier_scratch_bytes. */
size_t sg_outlier_scratch_bytes(int B, int D, int k);
int sg_outlier_suppress(float* feats, const float* attn_cls, const float* attn_diag, int B, int gh, int gw, int D,
                        int top_k, float contamination_temp, int32_t* out_idx, void* scratch, sg_stream s);
/* sg_cross_tile_fusion replaces CrossTileFusion.forward applied to every tile of a scene in raster order
 * (cross_tile_fusion.py:290-320; 'weighted' :185-236 adaptive branch, 'attention' :143-183).  The reference never calls the
 * module (dead code); the semantics are those of running it tile by tile with B=1 (oracle/refine.py).
 *   tokens [hg*wg, gh*gw, C] f32 patch tokens of the scene's tiles, updated in place; mode 0 = weighted, 1 = attention. */
size_t sg_cross_tile_scratch_bytes(int T, int gh, int gw, int C, int bw);
int sg_cross_tile_fusion(float* tokens, int hg, int wg, int gh, int gw, int C, int bw, int mode, float strength, void* scratch, sg_stream s);
/* The same fusion for a rank holding tiles [tile0, tile0+n_local) of the raster list: neighbour strips are read
 * from PACKED buffers indexed by the global tile id, which the caller all-gathers between the steps
 *   pack(which=0: original right columns [gh*bw,C]) -> gather -> fuse(pass 0) -> pack(which=1: final bottom rows [bw*gw,C],
 *   columns [0,bw) taken from left_result) -> gather -> fuse(pass 1) -> apply.
 * tokens / out / result / left_result / top_result are local ([n_local, ...]); nbr_strips is global ([hg*wg, S, C]). */
int sg_cross_tile_pack(const float* tokens, const float* left_result, int n_local, int tile0, int wg, int gh, int gw, int C, int bw,
                       int which, float* out, sg_stream s);
int sg_cross_tile_fuse(const float* tokens, const float* nbr_strips, int n_local, int tile0, int wg, int gh, int gw, int C, int bw,
                       int mode, float strength, int pass, float* result, sg_stream s);
int sg_cross_tile_apply(float* tokens, const float* left_result, const float* top_result, int n_local, int tile0, int wg, int gh, int gw,
                        int C, int bw, sg_stream s);
/* SelfAttentionEnhancementModule feature mode (self_attention_enhancement.py:71-150,247-324) */
int sg_weak_token_replace(float* feats, const float* attn_diag, int B, int gh, int gw, int D, int top_k,
                          int32_t* out_idx, void* scratch, sg_stream s);
/* SimilarityEnhancementModule.compute_similarity_map (similarity_enhancement.py:37-66):
 *   patches [B,n,D] f32 (row stride ld) -> sim [B,n,n] f32 */
int sg_similarity_map(const float* patches, int64_t batch_stride, int ld, int B, int n, int D, float temperature,
                      int add_self, int precision, float* sim, void* scratch, size_t scratch_bytes, sg_stream s);

/* ---- building-block ops exported for unit parity tests -----------------------------------------
 * C[M,N] = act(A[M,K] . W[N,K]^T + bias) (+ residual); f32 in/out at the boundary, computed in
 * `precision`.  act: 0 none, 1 QuickGELU, 2 erf GELU, 3 ReLU. */
int sg_op_linear(const float* A, const float* W, const float* bias, const float* residual, float* C,
                 int M, int N, int K, int act, int precision, void* scratch, size_t scratch_bytes, sg_stream s);
/* The residual GEMM -> LayerNorm -> GEMM chain of a transformer block (reference open_clip/transformer.py:234-254: x = x + out_proj(attn);
 * mlp(ln_2(x)), and the next block's attention(ln_1(x))):  x <- x + A.W1^T + b1 (in place),  y = act(LayerNorm(x; gamma, beta).W2^T + b2).
 * fold = 0 runs the LayerNorm as its own pass; fold = 1 is what the towers do in the 2-byte modes: the first GEMM's epilogue also writes the
 * 2-byte copy of x and per-64-column (sum, centred sum of squares), the second GEMM runs on that copy with W' = gamma o W2 and applies
 * rstd (acc - mean c) + b' in its epilogue (c = row sums of W', b' = b2 + W2.beta) -- no pass over x in between.
 * precision: SG_PREC_BF16 / SG_PREC_F16 / SG_PREC_F16X2; fold needs M >= 1024, D >= 512, D % 64 == 0, N2 >= 512.  All pointers are f32 device memory. */
size_t sg_op_ln_chain_scratch_bytes(int M, int K1, int D, int N2);
int sg_op_ln_chain(const float* A, const float* W1, const float* b1, float* x, const float* gamma, const float* beta, const float* W2,
                   const float* b2, float* y, int M, int K1, int D, int N2, int act, int precision, int fold, void* scratch,
                   size_t scratch_bytes, sg_stream s);
/* bf16 GEMM on caller-packed operands: A [M,K], W [N,K] bf16 (K % 64 == 0), C bf16 or f32 */
int sg_gemm_bf16_raw(const void* A, const void* W, const float* bias, const float* residual, void* C, int M, int N, int K,
                     int act, int c_is_bf16, sg_stream s);
/* The same GEMM for SG_PREC_BF16 / SG_PREC_F16 / SG_PREC_F16X2 operands in the precision's own storage (two-plane: groups of 8 elements as
 * [8 hi f16][8 lo f16], 32 bytes): A [batch][M][K], W [batch][N][K] (K % 64 == 0; two-plane K % 32 == 0), C [batch][M][N] f32 or, with
 * c_packed, in that storage; residual f32 [batch][M][N] (f32 C).  C = act(A.W^T + bias) (+ residual) per problem. */
int sg_gemm_raw(int precision, const void* A, const void* W, const float* bias, const float* residual, void* C, int M, int N, int K,
                int batch, int act, int c_packed, sg_stream s);
/* fp8 (OCP e4m3, v_mfma_f32_16x16x128_f8f6f4) GEMM on quantised operands: C = act((A8 . W8^T) * sa[m] * sw[n] + bias) (+ residual);
 * A8 [M,K], W8 [N,K] bytes, K % 128 == 0; sg_quantize_rows_fp8 produces an operand and its per-row scales (absmax / 448). */
int sg_gemm_fp8_raw(const void* A8, const float* sa, const void* W8, const float* sw, const float* bias, const float* residual, void* C,
                    int M, int N, int K, int act, int c_is_bf16, sg_stream s);
/* The MXFP8 forms of the same GEMM (OCP microscaling: one E8M0 power-of-two scale, value 2^(byte - 127), per 32 consecutive K elements,
 * fed to the scale operands of v_mfma_scale_f32_16x16x128_f8f6f4).  Block scales of an [M, K] operand are laid out [K/128][M][4] bytes
 * (the four blocks of one 128-wide K step of a row form one dword).  Exactly one of `sa` (per-row f32 scales) / `a_mx` (block scales)
 * describes A8.  With `c_mx` the result act(..) is written as e4m3 bytes [M,N] with block scales `c_mx_scale` [N/128][M][4] -- the next
 * linear's MX operand straight out of the epilogue (the tower's fc -> proj hand-off in SG_PREC_FP8) -- and C / residual are unused.
 * Needs M >= 1024, N >= 256, N % 8 == 0 (N % 128 == 0 with c_mx), K % 128 == 0. */
int sg_gemm_fp8_mx_raw(const void* A8, const float* sa, const void* a_mx, const void* W8, const float* sw, const float* bias,
                       const float* residual, void* C, void* c_mx, void* c_mx_scale, int M, int N, int K, int act, int c_is_bf16, sg_stream s);
int sg_quantize_rows_fp8(const float* x, int64_t rows, int D, void* y, float* scale, sg_stream s);
int sg_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, sg_stream s);
/* multi-term attention over packed qkv [B,N,3D] (rows q|k|v, nn.MultiheadAttention order);
 * variant = enum sg_model_type (SG_VANILLA = ordinary softmax(q k^T) v). bias: [B,n,n] or NULL.
 * Optional outputs: attn_cls/attn_diag [B,N] head-averaged probabilities (vanilla only). */
/* The fused attention kernel on caller-packed operands, for testing it directly (SG_PREC_BF16 / F16 / F16X2 storage; two-plane as the GEMM's).
 * Term t (t < n_terms) scores Q_t[b, i] . K_t[b, j] per head h, element (b, i, h, d) of a Q / K operand at q + b sb + i st + h dh + d; V its
 * own strides; strides in elements, multiples of 8, operands 16-byte aligned.  sum_scores = 1: the terms form one stream (at most 2);
 * otherwise each term is a separately soft-maxed stream and the streams' contexts are summed.  Score of (i, j) in natural-log units:
 *   s = scale_b sum_t Q_t[i].K_t[j]   (scale_b = scale_per_image[b] when given, else scale)
 *   resoftmax: s <- exp(s - lse_in[b,h,i]);   bias: s += bias_w bias[b bias_bstride + (j-1)(N-1) + (i-1)] (bias_rn[b,h,i] bias_cn[b,h,j])
 *   (bias read as [key][query]: the map must be symmetric; no bias for i = 0 or j = 0);  causal: keys j > i masked.
 * ctx [b, i, h dh + d] (strides ctx_sb / ctx_st, nullable: a log-sum-exp-only pass) = out_scale sum_streams softmax_j(s) V[j, h, d];
 * lse_out [B,H,N] (nullable) = the log-sum-exp of the last stream's scores.  Head dims 32 / 64 / 80 / 128. */
int sg_attention_raw(int precision, const void* q0, const void* q1, const void* q2, const void* k0, const void* k1, const void* k2,
                     int64_t sb, int64_t st, const void* v, int64_t v_sb, int64_t v_st, int B, int N, int H, int dh, int n_terms,
                     int sum_scores, int causal, float scale, const float* scale_per_image, const float* bias, float bias_w,
                     int64_t bias_bstride, const float* bias_rn, const float* bias_cn, int resoftmax, const float* lse_in, float* lse_out,
                     void* ctx, int64_t ctx_sb, int64_t ctx_st, float out_scale, sg_stream s);
/* The head-averaged statistics of an ordinary block on caller-packed rows: q at element 0 and k at element H dh of row (b, j) (strides sb /
 * st in elements) and a given lse [B,H,N]:  attn_cls[b,j] = mean_h exp(scale q_0.k_j - lse[b,h,0]), attn_diag[b,j] = mean_h exp(scale
 * q_j.k_j - lse[b,h,j]).  SG_PREC_BF16 / F16 / F16X2 storage. */
int sg_attention_stats_raw(int precision, const void* qk, int64_t sb, int64_t st, const float* lse, int B, int N, int H, int dh,
                           float scale, float* attn_cls, float* attn_diag, sg_stream s);
/* ---- raw test entries of the row kernels and patchify -----------------------------------------------------------------------------
 * Each passes its arguments one to one to ONE host function of the library (csrc/rowops.h), so a test can hold that kernel alone to a
 * reference at any shape, stride and storage the host function accepts; a refused call (non-zero, sg_last_error) launches nothing.
 * `kind` arguments name a storage by its sg_precision value: SG_PREC_F32 f32, SG_PREC_BF16 bf16, SG_PREC_F16 IEEE f16, SG_PREC_F16X2
 * two-plane groups of 8 elements as [8 hi f16][8 lo f16] (rows then start on multiples of 8 elements).  Strides are in elements. */
/* y[r, :D] = LayerNorm(x[r, :D]) * gamma + beta (biased variance, eps inside the square root), rows of x / y ldx / ldy elements apart,
 * y in the storage `out_kind`.  D % 4 == 0, D <= 2048, strides multiples of 4 (two-plane: D and ldy multiples of 8). */
int sg_layernorm_raw(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy, int out_kind, int64_t rows,
                     int D, float eps, sg_stream s);
/* The same LayerNorm quantised per row to OCP e4m3: scale[r] = max|v[r, :]| / 448 (1 for an all-zero row, never below the smallest normal
 * f32), y[r, :D] = e4m3(v / scale[r]) bytes, rows ldy bytes apart. */
int sg_layernorm_fp8_raw(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy, float* scale, int64_t rows,
                         int D, float eps, sg_stream s);
/* Rows of f32 / bf16 / f16 (`in_kind`, ldx elements apart) -> e4m3 bytes (ldy apart) + per-row scale as above.  D % 4 == 0, ldy % 4 == 0. */
int sg_quantize_rows_raw(const void* x, int in_kind, int64_t ldx, void* y, int64_t ldy, float* scale, int64_t rows, int D, sg_stream s);
/* x[b, t, :] = LayerNorm((t == 0 ? cls_emb : patches[b (N-1) + t - 1, :]) + pos[t, :]); patches rows ldp apart, x [B, N, D] dense. */
int sg_embed_assemble_raw(const float* patches, int64_t ldp, const float* cls_emb, const float* pos, const float* gamma, const float* beta,
                          float* x, int B, int N, int D, float eps, sg_stream s);
/* pos [1 + g0 g0, D] -> out [1 + gh gw, D]: row 0 copied; antialias 0: bicubic (A = -0.75) at scale_factor (g + 0.1) / g0, 1: the
 * antialiased bicubic (A = -0.5) to size (gh, gw); a downscale whose window exceeds 24 taps is refused. */
int sg_posembed_resize_raw(const float* pos, int g0, int D, int gh, int gw, int antialias, float* out, sg_stream s);
/* dst [rows, cols_pad] in the storage `kind` = src [rows, :cols] (rows ld_src apart) rounded once, columns >= cols zero.  Two-plane:
 * cols_pad % 8 == 0. */
int sg_pack_rows_raw(const float* src, int64_t rows, int cols, int64_t ld_src, void* dst, int cols_pad, int kind, sg_stream s);
/* dst [cols, rows] in the storage `kind` = src [rows, cols]^T rounded once.  Two-plane: rows % 8 == 0. */
int sg_transpose_pack_raw(const float* src, int rows, int cols, void* dst, int kind, sg_stream s);
/* slice_stats [D/64][rows][2] = (sum, centred sum of squares) of each 64-wide slice of a row -> mean_rstd [rows][2] by Chan's combination.
 * D % 64 == 0, rows > 0. */
int sg_ln_stats_finalize_raw(const float* slice_stats, int64_t rows, int D, float eps, float* mean_rstd, sg_stream s);
/* LayerNorm folded into a weight W [N, K]: Wp = round(gamma o W) in the storage of `precision` (bf16 / f16 / two-plane, K % 8 == 0 for the
 * last), c[n] = sum_k Wp[n, k] of the rounded values, bias_f[n] = (bias ? bias[n] : 0) + sum_k beta[k] W[n, k]. */
int sg_fold_ln_weight_raw(const float* W, int N, int K, const float* gamma, const float* beta, const float* bias, int precision, void* Wp,
                          float* c, float* bias_f, sg_stream s);
/* y_row = x_row / max(||x_row||, eps) over D contiguous elements; row r of x at (r / inner) so + (r % inner) si, of y at (r / inner) yo +
 * (r % inner) yi; storages `in_kind` / `out_kind` (two-plane rows start on multiples of 8); x == y allowed when the kinds agree. */
int sg_l2norm_rows_raw(const void* x, int in_kind, int64_t so, int64_t si, int inner, void* y, int out_kind, int64_t yo, int64_t yi,
                       int64_t rows, int D, float eps, sg_stream s);
/* The materialised softmax over rows of scores [rows, N] (stride ld; row = (b H + h) N + i), out with the same layout:
 * mode 0 p = softmax(sc s + w bias), mode 1 p = softmax(softmax(sc s) + w bias); sc = scale_per_image ? scale_per_image[b] : scale;
 * the bias term of (i, j) is bias[b bias_bstride + (i-1)(N-1) + j-1] (none at i == 0 or j == 0), w = bias_w (x bias_rn[b,h,i])
 * (x bias_cn[b,h,j]); causal: keys j > i get probability 0; out += p with accumulate; lse [rows] (optional) = log-sum-exp of the first
 * softmax's arguments. */
int sg_softmax_rows_raw(const float* scores, int64_t ld, int64_t rows, int N, int H, const float* scale_per_image, float scale,
                        const float* bias, float bias_w, int64_t bias_bstride, const float* bias_rn, const float* bias_cn, int mode,
                        int accumulate, int causal, float* out, float* lse, sg_stream s);
/* omega [gh gw, gh gw]: exp(-((y - y')^2 + (x - x')^2) / (2 std^2)) over the cells of a gh x gw grid (row-major cell index). */
int sg_gaussian_bias_raw(int gh, int gw, float std, float* omega, sg_stream s);
/* out[b, h, t] = || x[b sb + t st + h dh : + dh] || for x in the storage `kind` (strides in elements). */
int sg_head_norms_raw(const void* x, int kind, int64_t sb, int64_t st, int B, int N, int H, int dh, float* out, sg_stream s);
/* y[i] = a x[i] + b y[i], i < n. */
int sg_axpby_raw(float* y, const float* x, float a, float b, int64_t n, sg_stream s);
/* out[b] = scale * mean_t || x[b, t, :] || for x [B, N, D]. */
int sg_gem_inv_temp_raw(const float* x, int B, int N, int D, float scale, float* out, sg_stream s);
/* The patch matrix [n_tiles grid_h grid_w, Kpad] in the storage `out_kind` of a tile batch: column k = c P P + py P + px holds the
 * (normalised, for u8 scenes) pixel of the window padded by pad_t rows on top and pad_l columns on the left, zero in the padding and in
 * columns >= 3 P P.  Kpad >= 3 P P (two-plane: Kpad % 8 == 0), the grid must cover the padded tile. */
int sg_patchify_raw(const sg_tile_batch* tiles, int P, int Kpad, void* out, int out_kind, sg_stream s);
/* ---- raw test entries of the f32 GEMM and the attention-map stages --------------------------------------------------------------------
 * Same convention: one host function each, arguments one to one, a refused call launches nothing.  Strides in f32 elements. */
/* The parity-mode f32 GEMM in every form it has:  C[z](m, n) = act(alpha sum_k A[z](m, k) B[z](k, n) + bias[n]) + residual[z](m, n)  with
 * A[z](m, k) at A[zo sAo + zi sAi + m lda + k], B[z](k, n) at B[zo sBo + zi sBi + k sbk + n sbn], C[z](m, n) at C[zo sCo + zi sCi + m ldc + n],
 * zo = z / inner, zi = z % inner, z < batch.  bias [N] (nullable) is shared by the batch.  residual (nullable) is batched by C's strides
 * (sCo / sCi) with its own leading dimension: residual[z](m, n) at residual[zo sCo + zi sCi + m ldr + n].  act: 0 none, 1 QuickGELU, 2 erf-GELU,
 * 3 ReLU.  M, N, K, batch, inner > 0 (refused otherwise), batch < 65536.  A == B and residual == C are allowed. */
int sg_gemm_f32_raw(const float* A, int64_t lda, int64_t sAo, int64_t sAi, const float* B, int64_t sbk, int64_t sbn, int64_t sBo, int64_t sBi,
                    const float* bias, const float* residual, int64_t ldr, float* C, int64_t ldc, int64_t sCo, int64_t sCi, int M, int N, int K,
                    int batch, int inner, int act, float alpha, sg_stream s);
/* attn_avg [B,N,N] = the head-averaged attention matrix mean_h softmax_j(q_i.k_j / sqrt(D / H)) of an ordinary block.
 * SG_PREC_F32: qkv_or_probs is the materialised probabilities [B,H,N,N] f32 and the head mean is the whole stage (scratch unused, may be NULL).
 * SG_PREC_BF16 / F16 / F16X2: qkv_or_probs is the packed qkv [B,N,3D] in that storage; q and k are unpacked exactly to f32 and the scores,
 * the softmax and the mean run in f32, image by image.  scratch (256-byte aligned) holds [N,2D] + 2 [H,N,N] f32, each rounded up to 256 bytes. */
int sg_attn_average_raw(int precision, const void* qkv_or_probs, int B, int N, int D, int H, void* scratch, size_t scratch_bytes, float* attn_avg,
                        sg_stream s);
/* Self-attention enhancement, mode 'attention', on tokens [B,N,D] f32 (image b at tokens + b sb, dense rows: st == D, sb >= N D) with the
 * head-averaged map A [B,N,N]:  A'[i,i] += max(threshold - A[i,i], 0) strength for the patch rows i >= 1, every row divided by (its sum +
 * 1e-8), column 0 dropped; tokens[b, 1:, :] = (A'[b] . tokens[b])[1:, :], the CLS row untouched.  A is destroyed; tmp [B,N,D] f32. */
int sg_attn_enhance_raw(float* tokens, int64_t sb, int64_t st, float* A, int B, int N, int D, float strength, float threshold, float* tmp,
                        sg_stream s);
/* Attention-map layer fusion on the fused map acc [B,N,N] (destroyed) and tokens [B,N,D] dense f32 (in / out): a_cls[b, j] = acc[b, 0, j],
 * a_diag[b, j] = acc[b, j, j]; idx_out [B,k], k = min(top_k, N - 1): the k patch tokens with the largest a_cls / (a_diag + 1e-8), descending,
 * ties to the lowest index; columns 1 + idx_out[b, :] of acc[b] zeroed, every row divided by (its sum + 1e-8); tokens[b] = acc[b] . tokens[b].
 * tmp [B,N,D] f32. */
int sg_layer_fusion_apply_raw(float* acc, float* tokens, int B, int N, int D, int top_k, float* a_cls, float* a_diag, int32_t* idx_out, float* tmp,
                              sg_stream s);
size_t sg_op_attention_scratch_bytes(int B, int N, int D, int H, int precision);
int sg_op_attention(const float* qkv, int B, int N, int D, int H, int variant, const float* sim, float sim_weight,
                    float* ctx, float* attn_cls, float* attn_diag, int precision, void* scratch, size_t scratch_bytes,
                    sg_stream s);

/* ---- SimFeatUp joint bilateral upsampler --------------------------------------------------------
 * sg_adaptive_conv mirrors featup.adaptive_conv_cuda AdaptiveConv.apply as called at
 * simfeatup_dev/upsamplers.py:274 (semantics: adaptive_conv_py_simple, :14-25):
 *   input [B,C,h+d-1,w+d-1], filters [B,h,w,d,d] -> out [B,C,h,w], all f32. */
int sg_adaptive_conv(const float* input, const float* filters, int B, int C, int h, int w, int d, float* out, sg_stream s);

/* ---- Cluster-Then-Debias (reference CTD.py as segmentor.py:339-365 drives it) --------------------
 * sg_ctd_debias replaces, for every tile of a launch at once,
 *     _, labels = cluster_patch_tokens_dbscan(feats, grid_hw, {'metric': 'euclidean', 'eps': eps, 'min_samples': m})   CTD.py:147-296
 *     feats     = adaptive_debiasing(items=feats, labels=labels, bias=cls, factor=factor)                              CTD.py:299-366
 * (scikit-learn DBSCAN on the CPU in the reference).  tokens [B,n,C] f32 in/out, cls [B,C] = the CLS features (unit, or raw with
 * normalize_cls = 1: segmentor.py:310 normalises them first), labels_out int32 [B,n] (-1 = noise) or NULL.  n > 8192 leaves the tokens unchanged, as the reference's max_points does. */
size_t sg_ctd_scratch_bytes(int B, int n, int C);
int sg_ctd_debias(float* tokens, const float* cls, int B, int n, int C, double eps, int min_samples, float factor, int normalize_cls,
                  int32_t* labels_out, void* scratch, size_t scratch_bytes, sg_stream s);

/* ---- CLIP text tower (init-time producer of query_features) -------------------------------------
 * sg_text_encode replaces CLIP.encode_text(tokens) (open_clip/model.py:288-306): token + positional embedding, causal
 * residual blocks, ln_final, EOT pooling (argmax of the ids), @ text_projection.  Tensor names = the text part of the CLIP
 * state dict ("token_embedding.weight", "positional_embedding", "transformer.resblocks.N.*", "ln_final.*", "text_projection").
 *   tokens int32 [n_seq, context_length] -> out [n_seq, E] f32 (not normalised).  Init-time call: unlike the rest of the ABI it
 *   synchronises the stream before returning, so that an id outside [0, vocab_size) is SG_ERR_INVALID (the reference's
 *   nn.Embedding raises) instead of a silently clamped row. */
typedef struct sg_text sg_text;
int  sg_text_create(sg_text** out, int device, int width, int layers, int heads, int context_length, int vocab_size, int embed_dim,
                    int quick_gelu, int precision);
void sg_text_destroy(sg_text* t);
int  sg_text_set_tensor(sg_text* t, const char* name, const float* dev_f32, int64_t numel, sg_stream s);
size_t sg_text_workspace_bytes(const sg_text* t, int n_seq);
int  sg_text_encode(sg_text* t, const int32_t* tokens, int n_seq, float* out, void* workspace, size_t workspace_bytes, sg_stream s);

/* JBU context.  sg_jbu_create replaces get_upsampler(name, dim) (upsamplers.py:353-369; kind 0 = 'jbu_one', 1 = 'jbu_stack', 2 = 'bilinear');
 * sg_jbu_set_tensor takes the tensors by their state-dict names ("up.range_temp", "up2.fixup_proj.0.weight",
 * "fixup_proj.1.weight" ...), i.e. load_state_dict (segmentor.py:281-283);
 * sg_jbu_upsample replaces self.upsampler(image_features, img) (segmentor.py:371 -> upsamplers.py:278-325):
 *   source [B, gh*gw, C] patch tokens (pixel-major), guidance [B,3,GH,GW] normalised tile -> out [B, 16gh*16gw, C].
 *   precision: SG_PREC_F32 (parity kernels), SG_PREC_F16X2 (f32-grade: the linears and the low-res adaptive convolution on three f16 MFMAs per
 *   product -- what an exact tower mode is paired with), SG_PREC_BF16 (throughput: low-res convolution on bf16 operands, f16 fixup chain).
 *   Precision, per kernel against f64 on its own operands (tests/jbu_reference.py): under SG_PREC_F16X2 the low-res convolution stays within
 *   (2u 3 KP + 4u D + 2^-21) M + 2^-25 S_win (u = 2^-24, KP = 160 / 128 K slots, D = 2r + 1, M = sum_t |K_t| sum_s |w_s| |src_s|, S_win the
 *   window's sum |src|), a median of <= 2.1e-4 of |out| in the tests; the two-plane fixup and final GEMMs within gemm_bound's two-plane terms. */
/* Kind 2 = 'bilinear' (upsamplers.py:343-350, Bilinear: F.interpolate(feats, (GH, GW), mode='bilinear'), align_corners=False) has no
 * tensors: sg_jbu_set_tensor refuses every name (SG_ERR_INVALID).  sg_jbu_upsample writes the plain resize out [B, GH*GW, C] f32 (the module's
 * own output, for tests); sg_jbu_logits (every precision, C % 4 == 0, Q <= 32) writes logits [B, Q, GH*GW] without that map: by linearity
 * out_q(p) = (sum_k w_k y_kq) / sqrt(sum_kl w_k w_l G_kl) + lambda cls_q over the four corners k of p's cell, from y = tokens . T^T and five
 * Gram terms per token, all in f32 with f32 accumulation whatever the precision argument.  Bound per element against f64 on the same
 * operands (tests/upsampler_alt_reference.py, u = 2^-24, M = sum_k w_k |f_k|, D2 = |f(p)|^2, A_q = sum_k w_k sum_c |f_kc T_qc|):
 *   |err| <= (g_C A_q + g_4 sum_k w_k |y_kq|) / sqrt(D2) + |N_q| / sqrt(D2) * (g_C + g_12) M^2 / (2 D2) + 4u |out_q| + |lambda| g_C' S_cls,
 * g_n = n u / (1 - n u), N_q the numerator, S_cls the CLS logit's own dot bound.  The M^2 / D2 factor is the Gram form's price: neighbours
 * that nearly cancel (|f(p)| << M) lose digits that interpolate-then-normalise keeps. */
/* Kind 3 = 'resize_conv' (upsamplers.py:178-200, LayeredResizeConv(dim, 1); feat_dim % 8 == 0): tensors "conv{1..4}.weight" [C, C+3, 1, 1]
 * and "conv{1..4}.bias" [C]; weights are packed at sg_jbu_set_tensor as [W_src | W_guid | 0] rows of KP = align_up(C + 3, 64).  Four stages of
 * big = bilinear x2 (source), guid = tile resized to big's size (no antialias), out = act([big | guid] . W^T + b) + big (ReLU on stages 1-3);
 * sg_jbu_upsample -> out [B, 16gh*16gw, C].  Each stage's 1x1 conv runs on the precision's GEMM (f32; two-plane f16 for SG_PREC_F16X2; bf16
 * operands otherwise) and is bounded per element as that GEMM (tests/gemm_reference.py terms over K = C + 3); the operand producer's bilinear
 * blends within 4u of sum |w_k||x_k| (tests/upsampler_alt_reference.py).  sg_jbu_logits refuses this kind (SG_ERR_INVALID): the host runs
 * sg_jbu_upsample + sg_cosine_logits[_two_plane]. */
enum { SG_JBU_ONE = 0, SG_JBU_STACK = 1, SG_JBU_BILINEAR = 2, SG_JBU_RESIZE_CONV = 3 };
typedef struct sg_jbu sg_jbu;
int  sg_jbu_create(sg_jbu** out, int device, int kind, int feat_dim);
void sg_jbu_destroy(sg_jbu* j);
int  sg_jbu_set_tensor(sg_jbu* j, const char* name, const float* dev_f32, int64_t numel, sg_stream s);
size_t sg_jbu_workspace_bytes(const sg_jbu* j, int B, int gh, int gw);
int  sg_jbu_upsample(sg_jbu* j, const float* source, const float* guidance, int B, int gh, int gw, int GH, int GW, int precision,
                     float* out, void* workspace, size_t workspace_bytes, sg_stream s);

/* sg_jbu_logits (throughput mode, bf16, C % 64 == 0) replaces segmentor.py:368-379 for a batch of tiles in one call:
 *   feats = upsampler(tokens -> [1,C,g,g], img); feats /= |feats|; logits = feats @ T^T (+ cls_token_lambda * cls_logits)
 * with the JBU tail fused: out = x + 0.1 * fixup_proj(x) is never written -- the C x C 1x1 conv (upsamplers.py:301,325) runs as a GEMM whose
 * epilogue only accumulates |out|^2 per pixel, and out . T^T = x . (T^T + 0.1 Wf^T T^T) + 0.1 bf . T^T is a Q-wide f32 product.
 *   source [B, gh*gw, C] (global debias already applied), guidance [B,3,GH,GW], text [Q,C] (Q <= 32), cls [B,C] or NULL
 *   -> logits [B, Q, 16gh*16gw] f32.  Workspace as sg_jbu_workspace_bytes. */
int  sg_jbu_logits(sg_jbu* j, const float* source, const float* guidance, int B, int gh, int gw, int GH, int GW, int precision,
                   const float* text, int Q, const float* cls, float cls_token_lambda, float* logits, void* workspace, size_t workspace_bytes,
                   sg_stream s);
/* sg_jbu_logits_wide: the contract and output layout [B, Q, 16gh*16gw] of sg_jbu_logits for any Q >= 1, i.e. segmentor.py:368-379 with a class
 * file whose synonyms give more than 32 text rows (segmentor.py:262-276 builds one row per name).  Up to 32 queries it calls sg_jbu_logits: the
 * same kernels, buffer strides and bits.  Beyond, the tail's product x . Geff runs on the matrix pipe with the queries in groups of 16
 * (jbu_pixel_logits_wide_kernel: Geff as two bf16 planes in LDS, as many groups resident as fit, x re-read once per pass over the groups);
 * geff / g0 / clsl then have the query stride Qp = 16 ceil(Q / 16), which is also what the GEFF [C,Qp], G0 [Qp] and CLSL [B,Qp] captures copy.
 * Same conditions as sg_jbu_logits (SG_PREC_BF16, C % 64 == 0, C >= 512, 1024 <= pixels < 2^31, complete weights; resize_conv refused), each
 * refused with its reason; beyond 32 queries also C <= 1216 (two groups' planes must fit the 160 KB of LDS) and Q < 65536.  Kind 2 ('bilinear', upsamplers.py:343-350): one call for any Q, the per-token prologue and the pixel
 * kernel run per 32-query chunk and write their query planes in place -- per (pixel, query) the arithmetic of sg_jbu_logits on that chunk.
 * sg_jbu_workspace_bytes_wide: the workspace of sg_jbu_logits_wide for Q queries (sg_jbu_workspace_bytes up to 32 queries and for kind 2). */
size_t sg_jbu_workspace_bytes_wide(const sg_jbu* j, int B, int gh, int gw, int Q);
int  sg_jbu_logits_wide(sg_jbu* j, const float* source, const float* guidance, int B, int gh, int gw, int GH, int GW, int precision,
                        const float* text, int Q, const float* cls, float cls_token_lambda, float* logits, void* workspace,
                        size_t workspace_bytes, sg_stream s);

/* Test instrumentation of the upsampler (tests/test_gpu_jbu_reference.py).  sg_jbu_set_capture(j, cap) with a non-NULL cap makes every later
 * sg_jbu_upsample / sg_jbu_logits on j copy, on the call's stream, what each kernel of the unchanged kernel sequence read and wrote, in its
 * stored format, into the caller's device buffers: slot.dst (NULL = not captured) must hold slot.cap bytes; the call sets slot.bytes to the
 * bytes copied (0: that buffer did not exist in this dispatch) and fails with SG_ERR_INVALID if a region exceeds slot.cap.  cap must stay valid
 * until capture is switched off with sg_jbu_set_capture(j, NULL).  Per stage (JBULearnedRange), in kernel order:
 *   GS pooled guidance [px,3] f32 | PROJ range_proj [px,32] f32 | X range-kernel rows [px,d2+3] f32 | X16 operand rows [px,KP1] (bf16, f16 or
 *   two-plane) | H1 GELU rows (f32 [px,d2], or [px,NP] 2-byte / two-plane) | KF kernel rows (f32 [px,d2] or [px,NP], f16 [px,NP]) |
 *   SRC the convolution's source as stored, taken just before it (f32, bf16 or two-plane, [B,h,w,C]) | HR the bicubic output (f32 / bf16) |
 *   OUT the stage's f32 output | OUT16 its bf16 / two-plane copy.
 * Tail: FIN_A the final 1x1 GEMM's A operand | FIN_RES its f32 residual | GEFF [C,32] | G0 [32] | CLSL [B,32] | ROWDOT [px, C/64]
 *   (sg_jbu_logits_wide beyond 32 queries: query stride 16 ceil(Q / 16) in place of 32).
 * sg_jbu_last_kernels(): the calling thread's last sg_jbu_upsample / sg_jbu_logits as space-separated key=value tokens: per stage k
 * "sk.range= sk.x16= sk.fixup0= sk.fixup1= sk.kf= sk.src= sk.bicubic= sk.hr= sk.conv= sk.grid= sk.out16=", then "final=" (GEMM family) and
 * "tail=" (comma-separated kernels); "none" before the first call on the thread (a call refused by its argument checks leaves the
 * record as it was). */
enum { SG_JBU_CAP_GS, SG_JBU_CAP_PROJ, SG_JBU_CAP_X, SG_JBU_CAP_X16, SG_JBU_CAP_H1, SG_JBU_CAP_KF, SG_JBU_CAP_SRC, SG_JBU_CAP_HR,
       SG_JBU_CAP_OUT, SG_JBU_CAP_OUT16, SG_JBU_CAP_STAGE_SLOTS };
enum { SG_JBU_CAP_FIN_A, SG_JBU_CAP_FIN_RES, SG_JBU_CAP_GEFF, SG_JBU_CAP_G0, SG_JBU_CAP_CLSL, SG_JBU_CAP_ROWDOT, SG_JBU_CAP_TAIL_SLOTS };
typedef struct sg_jbu_capture_slot { void* dst; size_t cap; size_t bytes; } sg_jbu_capture_slot;
typedef struct sg_jbu_capture {
  sg_jbu_capture_slot stage[4][SG_JBU_CAP_STAGE_SLOTS];
  sg_jbu_capture_slot tail[SG_JBU_CAP_TAIL_SLOTS];
} sg_jbu_capture;
int  sg_jbu_set_capture(sg_jbu* j, sg_jbu_capture* cap);
const char* sg_jbu_last_kernels(void);

/* the normalised, zero-padded tile planes [T,3,up_h,up_w] f32 the reference hands to the upsampler as `img`
 * (segmentor.py:424-431 crop + pad, :371) */
int sg_extract_tiles(const sg_tile_batch* tiles, int up_h, int up_w, float* out, sg_stream s);

/* similarity-weighted global debias as a stand-alone op (segmentor.py:322-336), used ahead of the upsampler:
 *   out = tokens - cls_hat * (cos(tokens, cls_hat) * factor), tokens [B,n,E], cls [B,E] */
int sg_global_debias(const float* tokens, const float* cls, int B, int n, int E, float factor, float* out, sg_stream s);

/* ---- evaluation: confusion counts for mmseg's IoUMetric ---------------------------------------------------------------------
 * sg_confusion_accumulate replaces the counting behind test_evaluator = dict(type='IoUMetric', ...) (configs/base_config.py:19; the
 * reference's eval.py runs it through runner.test() and reports the result, eval.py:94-95): mmseg's intersect_and_union, which per
 * image copies the labels to the host, masks by ignore_index and runs torch.histc three times.  Here one device pass per call:
 *   labels int64 [n_pixels] (what sg_postprocess / sg_postprocess_multi write; any 8-byte aligned start), gt u8 or int64 [n_pixels] (any
 *   start), flat: one image, or the concatenated label buffer of a whole flush group.  Per pixel, in this order: g = raw truth; with
 *   reduce_zero_label mmseg's LoadAnnotations rule (raw 0 -> 255, raw 255 stays 255, every other value -> g - 1; the 255 is literal
 *   whatever ignore_index is); skip the pixel if g == ignore_index; p' = label if in [0,K) else K, g' likewise; table[p'][g'] += 1.
 *   table int64 [(K+1)][(K+1)], row = prediction, column = ground truth, index K = "outside [0,K)"; counts are ADDED to it.
 * The extra row and column reproduce torch.histc(min=0, max=K-1), which drops an out-of-range value from one histogram while the pixel
 * still counts in the others: area_intersect[k] = table[k][k], area_pred_label[k] = sum_g' table[k][g'], area_label[k] = sum_p' table[p'][k].
 * Counts are integers end to end (32-bit per workgroup in LDS, one 64-bit add per non-zero bin per workgroup): byte-identical across
 * repeats and launch shapes.  HBM-bound, one pass: 9 B per pixel (int64 label + u8 truth), 16 B with int64 truth.
 * Refused with SG_ERR_INVALID before any launch: null pointers, an unknown format, K < 1, K > 127 (the per-workgroup table of (K+1)^2
 * 32-bit counts must fit 64 KiB of LDS; there is no slower path for larger K), n_pixels < 0 or > 2^40.  n_pixels == 0 is a valid no-op. */
typedef enum { SG_GT_U8 = 0, SG_GT_I64 = 1 } sg_gt_format;
int sg_confusion_accumulate(const int64_t* labels, const void* gt, int gt_format, int64_t n_pixels, int K, int ignore_index,
                            int reduce_zero_label, int64_t* table, sg_stream s);

/* ---- PAMR: Pixel-Adaptive Mask Refinement of the stitched logits (Araslanov & Roth 2020) ----------------------------------------
 * The optional last stage of the training-free open-vocabulary segmenters (their pamr_steps / pamr_stride options): the [Q,H,W] logits
 * are averaged `steps` times over image-adaptive neighbourhoods, which snaps the patch-grid logits to image edges.  It comes after the
 * resize to ori_shape (the guidance resized to the same size with the same bilinear resize) and before the logit scale and the softmax
 * of the post-process.  The definition:
 *   guide g [3,H,W] f32 (the normalised image: what predict() receives; for a u8 scene (u - mean) / std as the ingest computes it),
 *   logits m_0 [Q,H,W] f32, dilations d_1..d_D, steps.
 *   Offsets o_1..o_8 = (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1) as (dy,dx).  Neighbour k = (i-1)*8 + j of pixel p = (y,x)
 *   is n_k(p) = (clamp(y + d_i dy_j, 0, H-1), clamp(x + d_i dx_j, 0, W-1)): replicate padding; a dilation may exceed H or W.
 *   Weights, once per image:
 *     sigma_c(p) = the unbiased standard deviation (divisor 9D - 1) of the 9D samples g_c(p + d_i (dy,dx)), i = 1..D, dy, dx in {-1,0,1},
 *                  clamped coordinates; the centre is among them D times.  Two passes (the mean, then the deviations), taken on the
 *                  differences to the centre value, so that a flat window gives exactly 0.
 *     a_k(p)     = (1/3) sum_c -|g_c(p) - g_c(n_k(p))| / (1e-8 + 0.1 sigma_c(p))
 *     w_k(p)     = softmax over k = 1..8D of a_k(p), the maximum subtracted.
 *   Steps, `steps` times: m_{t+1}[q,p] = sum_k w_k(p) m_t[q, n_k(p)], k in ascending order.  steps = 0 is the identity.
 * Conditioning: where a float image's local spread is at the rounding level of its own values without being exactly flat, w is
 * ill-conditioned in any f32 evaluation (the differences g(p) - g(n_k) and sigma are then a few units of the inputs' last place, and one
 * such unit moves a_k by O(1)); on normalised u8 images a window is either exactly flat or spread by at least one grey level.
 *   sg_pamr_workspace_bytes : the weights [8D,H,W] f32 (rounded up to 256 bytes) plus one ping-pong canvas [Q,H,W] f32; 0 for sizes
 *                             the entries refuse
 *   sg_pamr_affinity        : guide -> weights [8D,H,W] f32
 *   sg_pamr_step            : one step, weights + in [Q,H,W] -> out [Q,H,W]; in == out is refused
 *   sg_pamr                 : affinity + `steps` steps; the result is in logits_inout for odd and even `steps` alike (workspace 256-byte
 *                             aligned; not read when steps == 0)
 * `dilations` is a HOST array of n_dil ints, passed to the kernels by value.  Limits: 1 <= n_dil <= 8, 1 <= d <= 64, 0 <= steps <= 64,
 * Q, H, W >= 1 (any Q; at most 2^38 pixels).  Every refusal (a null pointer, a limit, in == out, a workspace too small: SG_ERR_STATE)
 * happens before any device work.  No atomics; a pixel's result depends on that pixel's lane alone: repeats are byte-identical.
 * Bound by HBM and L2: a step moves (2Q + 8D) * 4 bytes per pixel from and to HBM, neighbour re-reads are served by the caches. */
size_t sg_pamr_workspace_bytes(int Q, int H, int W, int n_dil);
int sg_pamr_affinity(const float* guide, int H, int W, const int* dilations, int n_dil, float* weights, sg_stream s);
int sg_pamr_step(const float* weights, const float* in, float* out, int Q, int H, int W, const int* dilations, int n_dil, sg_stream s);
int sg_pamr(const float* guide, float* logits_inout, int Q, int H, int W, const int* dilations, int n_dil, int steps, void* workspace,
            size_t workspace_bytes, sg_stream s);

/* ---- area_thd: per-image suppression of small-area classes ---------------------------------------------------------------------
 * The `area_thd` option of the training-free open-vocabulary segmenters: a class that wins only a small share of an image's
 * non-background pixels is removed from that image and its pixels go to the best remaining class.  The definition, for one image:
 *   p [K,H,W] f32 = the class probabilities exactly as the tail produces them (after stitch, the resize to ori_shape, PAMR, logit scale,
 *   softmax and the synonym maximum); area_thd a double >= 0 (the option's range is [0, 1]; above 1 every non-background class goes).
 *   1. l0(x)    = the class of the first maximum of p[:,x] (lowest class index on ties), BEFORE prob_thd.
 *   2. area[c]  = the number of pixels with l0 = c, int64; total = sum over c != bg_idx of area[c].
 *   3. keep[c]  = (c == bg_idx) or (double)area[c] > area_thd * (double)total.  The comparison is strict and is evaluated in double on
 *                 the device (upstream compares in the logits' dtype; counts above 2^24 are not exact in f32).  The background class
 *                 is always kept; total = 0 keeps only the background.
 *   4. p'[c]    = keep[c] ? p[c] : 0: what the probabilities hold afterwards.
 *   5. label(x) = the kept class with the largest p[c,x] (lowest index on ties), or bg_idx if that maximum is < prob_thd.
 * Dropped classes are EXCLUDED from the arg-max of step 5 rather than compared as zeros.  The two readings differ only at a pixel where
 * every kept probability is exactly 0 (the zeros of the dropped planes then tie with them and a dropped class of lower index would win);
 * they never differ for bg_idx = 0, because the background is kept and has the lowest index.
 * The first pass is the existing tail run with prob_thd = 0, whose labels are l0.  No entry synchronises with the host.
 *   sg_class_area[_multi]        labels int64 -> counts int64 [K] / [N,K], ADDED to `counts` (the caller zeroes it).  A label outside [0,K)
 *                                is not counted.  32-bit counts per workgroup in LDS, one 64-bit add per non-zero bin per workgroup:
 *                                integers end to end, byte-identical across repeats and launch shapes.  Multi: image n holds
 *                                image_pixels[n] labels at out_offset[n] of the flat buffer of out_pixels labels; block_prefix [N+1] =
 *                                exclusive prefix sum of ceil(image_pixels[n] / 4096); a block never straddles two images.
 *   sg_area_keep                 counts [N,K], bg_idx, area_thd -> keep int32 [N,K] (1 / 0), step 3, one launch of N workgroups.
 *   sg_area_filter_probs[_multi] steps 4 and 5: probs in place, first-pass labels in, final labels out (labels_in == labels_out is
 *                                allowed).  A pixel whose l0 is kept reads p[l0] only; one whose l0 is dropped (or outside [0,K)) takes
 *                                the first maximum over the kept planes.  Comparisons and stores, no arithmetic: byte-equal to the
 *                                definition on the same inputs.  Multi: sg_postprocess_multi's output layout (labels of image n at
 *                                out_offset[n], probs [K,H,W] at K * out_offset[n], block_prefix of ceil(H*W/256)), keep [N,K].
 *   sg_area_relabel[_multi]      the labels-only route, no canvas and no probability planes: sg_label_head[_multi]'s arguments plus keep,
 *                                the first-pass conf, and labels in/out (the first pass: sg_label_head with prob_thd = 0 and conf).  A
 *                                64 x 4 pixel block in which every first label is kept gathers nothing and writes
 *                                conf < prob_thd ? bg_idx : l0.  A block that holds a dropped label repeats sg_label_head's statements
 *                                with the best (value, class) pair restricted to kept classes.  Contract: every pixel equals
 *                                sg_label_head called with a query_idx in which the queries of dropped classes are -1.
 * Limits: 1 <= K <= SG_AREA_MAX_K (the per-workgroup table of K 32-bit counts: 16 KiB, so far more than two workgroups share a CU's
 * LDS; there is no slower path beyond it), 0 <= bg_idx < K, n_pixels <= 2^40.  Every refusal (a null pointer, a limit, K, a bg_idx out of
 * range) is SG_ERR_INVALID before any device work. */
#define SG_AREA_MAX_K 4096
int sg_class_area(const int64_t* labels, int64_t n_pixels, int K, int64_t* counts, sg_stream s);
int sg_class_area_multi(const int64_t* labels, const int64_t* image_pixels, const int64_t* out_offset, const int64_t* block_prefix, int N,
                        int64_t total_blocks, int64_t out_pixels, int K, int64_t* counts, sg_stream s);
int sg_area_keep(const int64_t* counts, int N, int K, int bg_idx, double area_thd, int32_t* keep, sg_stream s);
int sg_area_filter_probs(float* probs, const int64_t* labels_in, const int32_t* keep, int K, int H, int W, float prob_thd, int bg_idx,
                         int64_t* labels_out, sg_stream s);
int sg_area_filter_probs_multi(float* probs, const int64_t* labels_in, const int32_t* keep, const int32_t* out_hw, const int64_t* out_offset,
                               const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels, int K, float prob_thd,
                               int bg_idx, int64_t* labels_out, sg_stream s);
int sg_area_relabel(const float* tile_logits, const int32_t* windows, int T, int Q, int gh, int gw, int up_h, int up_w, int pad_t,
                    int pad_l, int H, int W, const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx,
                    const int32_t* keep, const float* conf, int64_t* labels, sg_stream s);
int sg_area_relabel_multi(const float* tile_logits, const int32_t* windows, const int32_t* tile_image, int T, int Q, int gh, int gw,
                          int up_h, int up_w, int pad_t, int pad_l, const int32_t* image_hw, const int32_t* image_tiles,
                          const int64_t* out_offset, const int64_t* block_prefix, int N, int64_t total_blocks, int64_t out_pixels,
                          const int32_t* query_idx, int K, float logit_scale, float prob_thd, int bg_idx, const int32_t* keep,
                          const float* conf, int64_t* labels, sg_stream s);

/* ---- min_region: sieve small connected regions out of a label map ---------------------------------------------------------------
 * The spatial clean-up that follows prob_thd and area_thd: skimage's remove_small_objects (fill "bg") and GDAL's sieve (fill
 * "neighbour"), on the final labels.
 * Input.  labels int64 [H,W]; any int64 value is a label.  Two pixels belong to the same *region* when they hold the same label and are
 *   linked by a chain of such pixels under the chosen connectivity: 4 (edge neighbours) or 8 (edge and corner neighbours).  A region's
 *   *area* is its pixel count, its *root* the smallest raster index y*W + x among its pixels.  min_region is an integer >= 1; a region is
 *   *small* when area < min_region and *kept* otherwise.  min_region = 1 changes nothing: the output holds the input bytes.
 * SG_SIEVE_FILL_BG (remove small objects).  Every small region whose label is not bg_idx becomes bg_idx.  Regions labelled bg_idx are
 *   never changed.
 * SG_SIEVE_FILL_NEIGHBOUR (sieve).  Every small region is sieved, background ones included: it takes the label of the kept region
 *   adjacent to it (same connectivity as the regions) that has the largest area; ties on area go to the smaller root.  A small region
 *   with no adjacent kept region becomes bg_idx.  There is ONE pass over the regions of the input and no iteration: a sieved region may
 *   take the label of a kept region next to another kept region of that label, or several small neighbours may fall to bg_idx together,
 *   so the result is not necessarily a fixed point -- sieving it again can change it.
 * The output is int64 [H,W] and may alias the input.  The images of a multi-image call never connect to each other.
 *   sg_sieve_workspace_bytes  scratch for n_pixels_total pixels (the sum over the images): parent int32 + area int32 per pixel, and best
 *                             u64 per pixel for SG_SIEVE_FILL_NEIGHBOUR -- 8 or 16 bytes per pixel.  0 for a negative count or an
 *                             unknown fill.
 *   sg_sieve                  N >= 1 images in one flat int64 buffer (what the multi-image heads write): image n is image_hw[2n] x
 *                             image_hw[2n+1] labels at labels + out_offset[n] and is written to labels_out + out_offset[n].  image_hw
 *                             (int32 [N,2]) and out_offset (int64 [N]) are HOST arrays: they are checked before anything is launched
 *                             and travel to the kernels as launch arguments, SG_SIEVE_GROUP images per launch sequence (local
 *                             labelling, border merge, flatten + areas, neighbour choice, apply), so a group of up to SG_SIEVE_GROUP
 *                             images is served by one sequence, a larger one by one per SG_SIEVE_GROUP, and nothing is copied or
 *                             synchronised.  workspace: 8-byte aligned device memory.
 * Integers and integer atomics only: byte-identical across repeats and launch shapes.  Nothing visits the host.
 * Refused with SG_ERR_INVALID before any device work: a null pointer, min_region < 1, a connectivity other than 4 or 8, an unknown fill,
 * N < 1, an image of non-positive size or of 2^31 or more pixels, a negative out_offset, a misaligned buffer, a workspace that is too
 * small. */
#define SG_SIEVE_FILL_BG 0
#define SG_SIEVE_FILL_NEIGHBOUR 1
#define SG_SIEVE_GROUP 64
size_t sg_sieve_workspace_bytes(int64_t n_pixels_total, int fill);
int sg_sieve(const int64_t* labels, int64_t* labels_out, const int32_t* image_hw, const int64_t* out_offset, int N, int64_t min_region,
             int connectivity, int fill, int64_t bg_idx, void* workspace, size_t workspace_bytes, sg_stream stream);

/* ---- region table: list the connected regions of a label map --------------------------------------------------------------------------
 * The last stage after prob_thd -> area_thd -> min_region, for the object datasets: how many regions, how large, where, how confident.
 * It only reads final labels.  Regions, area, root and connectivity are exactly those of sg_sieve: a region is a set of pixels of equal
 * int64 label, connected under connectivity 4 or 8; its root is its smallest raster index y*W + x.
 * A region is *listed* when area >= min_area (min_area >= 1) and, if use_skip is set, its label is not skip_label.  The listed regions
 * of a call are ordered by (image index, root), ascending; the images of a call never connect to each other.
 * table.  Row r is one region: SG_REGION_FIELDS = 12 int64 columns, 96 bytes:
 *   SG_REGION_IMAGE    the image index            SG_REGION_ROOT   the region's root
 *   SG_REGION_LABEL    its label                  SG_REGION_AREA   its pixel count
 *   SG_REGION_Y0, _X0, _Y1, _X1   the half-open bounding box: Y1 / X1 are one past the last row / column
 *   SG_REGION_SUM_Y, _SUM_X       the integer sums of the pixels' coordinates; centroid = sum / area, in double on the caller's side
 *   SG_REGION_SCORE_Q  the sum over the region's pixels of q(conf); 0 when conf is null
 *   column 11          0
 *   q(c) is round-to-nearest-even of clamp(c, 0, 1) * 2^24 as a 64-bit integer; a NaN counts 0.  The scaling by a power of two is exact
 *   in f32, so the sum is an exact integer, independent of arrival order.  The mean score is SCORE_Q / 2^24 / AREA.
 * counts int64 [N+1]: counts[n] is the true number of listed regions of image n, counts[N] their total; both are uncapped.  Rows
 *   0 .. min(total, max_regions) - 1 are written; rows beyond that are not touched: the caller's bytes stay.
 * region_of (optional) int32, laid out like labels: the row index of the pixel's region in the uncapped order (so it may be >=
 *   max_regions), -1 where the region is not listed.
 * conf (optional) f32 with the labels' layout and offsets.  image_hw / out_offset are HOST arrays, as in sg_sieve.
 *   sg_regions_workspace_bytes  8 * n_pixels_total (parent int32 + area int32 per pixel; a listed root's area entry becomes its row
 *                               index) + 4 * (ceil(n_pixels_total / SG_REGIONS_BLOCK_PIXELS) + SG_SIEVE_GROUP + 1) rounded up to 8 (the
 *                               scan's block array: one int32 per per-pixel workgroup of a launch sequence, and the running total).
 *                               max_regions does not enter it.  0 for a negative count or max_regions < 1.
 *   sg_regions                  per launch sequence of up to SG_SIEVE_GROUP images: the three labelling kernels of sg_sieve, then count
 *                               (listed roots per workgroup of SG_REGIONS_BLOCK_PIXELS pixels), scan (one workgroup, exclusive offsets,
 *                               SG_REGIONS_SCAN_BLOCKS entries per pass; the row offset passes from one sequence to the next in
 *                               counts[N]), scatter (the rows' IMAGE, ROOT, LABEL, AREA and start values; the whole row of a one-pixel
 *                               region) and reduce (box, sums, score and region_of, on tiles of 64 x 128 pixels; merged per wave and
 *                               per workgroup before they reach global memory).  All in stream order; nothing is copied or
 *                               synchronised.
 * Integers and integer atomics only (min, max, add): byte-identical across repeats and launch shapes.
 * Refused with SG_ERR_INVALID before any device work: a null labels / image_hw / out_offset / table / counts / workspace, a connectivity
 * other than 4 or 8, min_area < 1, max_regions < 1, N < 1, an image of non-positive size, a negative out_offset, 2^31 or more pixels in
 * the call (row indices are int32), a buffer that is not 8-byte aligned (region_of / conf: 4-byte), a workspace that is too small. */
#define SG_REGION_IMAGE 0
#define SG_REGION_ROOT 1
#define SG_REGION_LABEL 2
#define SG_REGION_AREA 3
#define SG_REGION_Y0 4
#define SG_REGION_X0 5
#define SG_REGION_Y1 6
#define SG_REGION_X1 7
#define SG_REGION_SUM_Y 8
#define SG_REGION_SUM_X 9
#define SG_REGION_SCORE_Q 10
#define SG_REGION_FIELDS 12
#define SG_REGIONS_BLOCK_PIXELS 2048
#define SG_REGIONS_SCAN_BLOCKS 1024
size_t sg_regions_workspace_bytes(int64_t n_pixels_total, int64_t max_regions);
int sg_regions(const int64_t* labels, const float* conf, const int32_t* image_hw, const int64_t* out_offset, int N, int connectivity,
               int64_t min_area, int64_t skip_label, int use_skip, int64_t max_regions, int64_t* table, int32_t* region_of, int64_t* counts,
               void* workspace, size_t workspace_bytes, sg_stream s);

/* ---- Boundary IoU: boundary bands and band-restricted counts (Cheng et al., CVPR 2021) -------------------------------------------------
 * IoU restricted to the pixels of each mask that lie within d pixels of that mask's contour: the score that moves when an outline moves,
 * which area IoU (sg_confusion_accumulate) barely does.  It only reads final labels.
 * Band.  For a label map L of H x W and a width d >= 1, band(y,x) = 1 iff the square window [y-d, y+d] x [x-d, x+d] either leaves the
 *   image or holds a pixel whose label differs from L(y,x).  This is, for every class c at once, the paper's
 *   mask_c - erode(pad0(mask_c), 3x3 ones, iterations = d) with mask_c = (L == c); every pixel has exactly one label, so one bit per pixel
 *   carries the bands of all classes.  Labels are compared as raw 64-bit values: a value outside [0,K) is a label like any other here.
 * Width from the ratio (host arithmetic in double, per image): d = max(1, int(round(ratio * sqrt(H*H + W*W)))), Python's round; the
 *   paper's default ratio is 0.02.  1 <= d <= 4095.
 * Counts.  Per image, bandP is the band of the prediction as it is; bandG the band of the truth after reduce_zero_label (the rule of
 *   sg_confusion_accumulate: raw 0 -> 255, raw 255 stays, else g - 1).  Ignored truth pixels stay in the map, as a value that belongs to
 *   no class: a class that borders an ignored area has a boundary there, as the per-class binary mask gives.  Then every pixel whose
 *   transformed truth g is not ignore_index is counted, with p its prediction and areas int64 [3][K]:
 *     areas[0][k] += (p == k && g == k && bandP && bandG)      the intersection of the two bands
 *     areas[1][k] += (p == k && bandP)                         the prediction's band
 *     areas[2][k] += (g == k && bandG)                         the truth's band
 *   Values outside [0,K) add to nothing.  BIoU[k] = areas[0][k] / (areas[1][k] + areas[2][k] - areas[0][k]) in float64 on the caller's
 *   side, NaN where the denominator is 0.  With d >= max(H, W) every pixel is in both bands and areas equals (area_intersect,
 *   area_pred_label, area_label) of the confusion table on the same inputs.
 * N >= 1 maps lie back to back in one flat buffer (what the multi-image heads write): image n is image_hw[2n] x image_hw[2n+1] at
 * offset[n] (in pixels), with its own width d[n]; image_hw, offset and d are HOST arrays, checked before anything is launched.  The
 * images lie in ascending order, do not overlap and stay inside the n_pixels_total = sum of H*W pixels of the call (so offset[n] is the
 * sum of the sizes before image n).
 *   sg_boundary_workspace_bytes  4 planes of n_pixels_total bytes, each rounded up to 256: row bytes and band of the prediction and of the
 *                                truth (sg_boundary_accumulate).  sg_boundary_band uses the first plane only and accepts a workspace of
 *                                a quarter of this.  0 for a negative count.
 *   sg_boundary_band             labels u8 (SG_GT_U8) or int64 (SG_GT_I64) -> band u8 [n_pixels_total], 0 / 1, same offsets.  Per image a
 *                                row pass (per row one sweep with a running start-of-run: is [x-d, x+d] inside the image and of one
 *                                label) and a column pass (a march down the columns over the row pass's bytes, in row bands with a halo
 *                                of 2d rows).  No loop over the window: the work per pixel does not grow with d.
 *   sg_boundary_accumulate       the bands of labels and of the transformed truth, then the counts above ADDED to areas (the caller zeroes
 *                                it): 3K 32-bit bins in LDS per workgroup, one 64-bit add per non-zero bin per workgroup.
 * Integers and integer atomics only: byte-identical across repeats.  Nothing is copied or synchronised; no workgroup waits for another.
 * Refused with SG_ERR_INVALID before any launch: a null pointer, an unknown format, N < 1, an image of non-positive size or of 2^31 or
 * more pixels, an offset that puts an image over the one before it or outside the call's pixels, d outside [1, 4095], K < 1, K > 127 (the cap of
 * sg_confusion_accumulate, so that one metric object can hold both tables), a misaligned int64 buffer, a workspace that is too small. */
size_t sg_boundary_workspace_bytes(int64_t n_pixels_total);
int sg_boundary_band(const void* labels, int fmt, const int32_t* image_hw, const int64_t* offset, const int32_t* d, int N, uint8_t* band,
                     void* workspace, size_t workspace_bytes, sg_stream s);
int sg_boundary_accumulate(const int64_t* labels, const void* gt, int gt_format, const int32_t* image_hw, const int64_t* offset,
                           const int32_t* d, int N, int K, int ignore_index, int reduce_zero_label, int64_t* areas, void* workspace,
                           size_t workspace_bytes, sg_stream s);

/* ---- Tolerant matching: relaxed precision / recall (Mnih & Hinton 2010) and the boundary F-score (Martin et al. 2004; Csurka et al. 2013) --
 * Both scores are one count: per class, the marked pixels of one label map that have a marked pixel of the same class in the other map
 * within a Euclidean distance.  Area IoU and Boundary IoU do not give it: a two-pixel-wide road lies wholly inside its own band, so a
 * prediction displaced by two pixels scores about zero BIoU and about one relaxed F.  It only reads final labels.
 * Inputs.  A prediction P and a truth G of H x W, G taken after reduce_zero_label (the rule of sg_confusion_accumulate: raw 0 -> 255, raw
 *   255 stays, else g - 1), an integer tol_sq >= 0 and a mode.
 * Marked pixels M_L of a map L.  SG_TOL_REGION: every pixel.  SG_TOL_CONTOUR: a pixel is marked iff one of its 4-neighbours inside the
 *   image holds another 64-bit value (of G: after the transform).  The image border is not a contour.  An ignored truth value is a value
 *   like any other here: a class that borders an ignored area has a contour there, as in Boundary IoU.
 * Class sets and nearness.  S_L(k) = { q in M_L : L(q) == k } for 0 <= k < K; near_L(p,k) holds iff some q in S_L(k) has
 *   (py-qy)^2 + (px-qx)^2 <= tol_sq, in integer arithmetic: tol_sq = 10 reaches the offset (1,3), tol_sq = 9 does not.
 * Sources and targets.  A source p is counted only where G(p) is not ignore_index; targets are never restricted by that.
 * Counts, ADDED to counts int64 [4][K] (the caller zeroes it):
 *     counts[0][k] += (p in S_P(k), counted)                   predicted pixels of class k
 *     counts[1][k] += (p in S_P(k), counted, near_G(p,k))      ... that are right within the tolerance
 *     counts[2][k] += (p in S_G(k), counted)                   true pixels of class k
 *     counts[3][k] += (p in S_G(k), counted, near_P(p,k))      ... that are found within the tolerance
 *   Values outside [0,K) add to nothing and match nothing.
 * Scores, in float64 on the caller's side, NaN where the denominator is 0: precision = counts[1] / counts[0], recall = counts[3] /
 *   counts[2], F = 2PR / (P + R).
 * Identities.  With tol_sq = 0 in region mode rows 1 and 3 both equal area_intersect, rows 0 and 2 area_pred_label and area_label of the
 *   confusion table on the same inputs.  With tol_sq >= (H-1)^2 + (W-1)^2 a source is matched iff its class is marked anywhere in the
 *   other map.
 * Limits.  0 <= tol_sq <= 254*254, so the radius r = isqrt(tol_sq) <= 254 and a one-byte capped distance suffices; 1 <= K <= 127, as
 *   in the other two tables; an image has fewer than 2^31 pixels.
 * Tolerance from a ratio (host arithmetic in double, per image): r = max(1, ceil(ratio * sqrt(H*H + W*W))), tol_sq = r*r; the default
 *   ratio is 0.0075 (38 px on 2048 x 4608); a radius above 254 is refused.
 * N >= 1 images lie back to back in flat buffers with HOST arrays image_hw, offset and tol_sq[n]; the layout rules are those of
 * sg_boundary_accumulate (ascending, no overlap, inside the n_pixels_total = sum of H*W pixels of the call).
 *   sg_tolerant_workspace_bytes  min(K, 8) planes of n_pixels_total bytes, each rounded up to 256: per class of a group of up to 8 classes
 *                                the distance, capped at 255, to the nearest marked pixel of that class in the same row.  Groups and
 *                                directions reuse the planes, so it does not grow with K beyond 8 planes.  0 for a negative count or a K
 *                                outside [1, 127].
 *   sg_tolerant_accumulate       per image, per class group and per direction a row pass over the target map (two scans per row, no loop
 *                                over the tolerance) and a count over the source map (a walk over at most 2r + 1 rows of those bytes against
 *                                w(dy) = isqrt(tol_sq - dy*dy), stopped at the first hit: linear in r), into 2K 32-bit LDS bins per
 *                                workgroup, then one 64-bit add per non-zero bin per workgroup.
 * Integers and integer atomics only: byte-identical across repeats.  Nothing is copied or synchronised; no workgroup waits for another; the
 * inputs are only read.
 * Refused with SG_ERR_INVALID before any launch, counts untouched: a null pointer, an unknown format or mode, N < 1, an image of
 * non-positive size or of 2^31 or more pixels, an offset that puts an image over the one before it or outside the call's pixels, tol_sq
 * outside [0, 254*254], K outside [1, 127], a misaligned int64 buffer, a workspace that is too small. */
#define SG_TOL_REGION 0
#define SG_TOL_CONTOUR 1
size_t sg_tolerant_workspace_bytes(int64_t n_pixels_total, int K);
int sg_tolerant_accumulate(const int64_t* labels, const void* gt, int gt_format, const int32_t* image_hw, const int64_t* offset,
                           const int32_t* tol_sq, int N, int K, int mode, int ignore_index, int reduce_zero_label, int64_t* counts,
                           void* workspace, size_t workspace_bytes, sg_stream s);

/* ---- Object matching: object-level precision / recall / F1 and panoptic quality (Kirillov et al., "Panoptic Segmentation", CVPR 2019) ----
 * The three tables above are pixel counts: one warehouse of 40 000 pixels outvotes forty missed houses of 400 pixels each.  This one
 * counts objects: per class, which connected region of the prediction overlaps which connected region of the truth with an IoU above a
 * threshold.  It only reads final labels.
 * Inputs.  A prediction P of H x W, int64, and a truth G (SG_GT_U8 or SG_GT_I64) taken after reduce_zero_label (the rule of
 *   sg_confusion_accumulate: raw 0 -> 255, raw 255 stays, else g - 1); call it G'.
 * Objects of a map L.  A region is what sg_sieve calls a region: pixels of equal 64-bit value, connected under connectivity 4 or 8; its
 *   root is its smallest raster index y*W + x.  A region is an *object of class k* when its value is k with 0 <= k < K, use_skip is 0 or
 *   k != skip_label, its area >= min_area (>= 1) and, for the truth, k != ignore_index.  Ignored truth is a value like any other: it
 *   separates regions and is itself no object.  Predicted objects are counted WHEREVER they lie, also on ignored truth (there they find no
 *   partner and count as false positives); dropping predicted objects that lie mostly on ignored truth is a follow-up.
 * Match.  A predicted object p and a true object g of the same class in the same image, I = |p n g|, U = |p| + |g| - I, match iff
 *   I * iou_den > iou_num * U, in 64-bit integers, strictly.  1 <= iou_num < iou_den <= 2^20 and 2 * iou_num >= iou_den: with a threshold
 *   of at least 1/2 and the strict comparison every object has at most one partner (Theorem 1 of the paper), so no ordering or greedy
 *   assignment exists.  At 1/2 a pair at exactly IoU 0.5 is NOT a match: the panoptic-quality rule.
 * Counts, ADDED to counts int64 [4][K] (the caller zeroes it):
 *     counts[0][k]   matched pairs of class k                       TP
 *     counts[1][k]   predicted objects of class k                   TP + FP
 *     counts[2][k]   true objects of class k                        TP + FN
 *     counts[3][k]   the sum over the matched pairs of floor(I * 2^24 / U), 64-bit integer division: an exact integer, independent of
 *                    arrival order, like SG_REGION_SCORE_Q
 * Scores, in float64 on the caller's side, NaN where a denominator is 0: precision = counts[0] / counts[1], recall = counts[0] /
 *   counts[2], F1 = RQ = 2 counts[0] / (counts[1] + counts[2]), SQ = counts[3] / 2^24 / counts[0], PQ = SQ * RQ (connected regions as
 *   the segments).
 * match_map (optional, null allowed) uint8, laid out like labels, WRITTEN for every pixel of the call: a + b with a = 1 where the pixel's
 *   predicted region is a matched object, 2 where it is an unmatched object, else 0; b = 4 where the pixel's true region is a matched
 *   object, 8 where it is an unmatched object, else 0.  It is the TP / FP / FN picture, and a root pixel's byte joins the matches to the
 *   rows of sg_regions.
 * Limits.  1 <= K <= 127, as in the other tables; fewer than 2^31 pixels per call.
 * N >= 1 images lie back to back in flat buffers with HOST arrays image_hw and offset; the layout rules are those of
 * sg_boundary_accumulate (ascending, no overlap, inside the n_pixels_total = sum of H*W pixels of the call).  The images never connect.
 *   sg_object_workspace_bytes  36 * n_pixels_total + 2 * (n_pixels_total rounded up to 256): per pixel G' int64, the candidate word u64,
 *                              parent and area int32 of both maps, the intersection counter u32, and two planes of match marks u8.
 *                              Linear in the pixels whatever the maps hold: there is no cap on the number of objects and no overflow
 *                              case.  0 for a negative count.
 *   sg_object_match            one kernel writes G'; then per launch sequence of up to SG_SIEVE_GROUP images the three labelling
 *                              kernels of sg_sieve on P and on G', and: vote (one word per predicted root, candidate true root : 32 |
 *                              counter : 32, a Boyer-Moore majority summary merged by a 64-bit compare-and-swap loop -- a match needs
 *                              I > |p| / 2, so the partner is the strict majority among the true objects of p's class under p's pixels,
 *                              and the summary finds a strict majority whatever the merge order), verify (I of the candidate, exactly),
 *                              decide (over the root pixels: the integer test, K-wide LDS bins, one 64-bit add per non-zero bin per
 *                              workgroup) and, with match_map, one pass that writes the bytes.  Votes and intersections merge in
 *                              registers, across the wave and in an LDS cache of the workgroup (32 768 pixels) before they reach memory.
 * Integers and integer atomics only: byte-identical across repeats.  Nothing is copied or synchronised; no workgroup waits for another
 * (the compare-and-swap retry is lock-free); the inputs are only read.
 * Refused with SG_ERR_INVALID before any launch, counts and match_map untouched: a null labels / gt / image_hw / offset / counts /
 * workspace, an unknown format, N < 1, an image of non-positive size, 2^31 or more pixels in the call, an offset that puts an image over
 * the one before it or outside the call's pixels, K outside [1, 127], a connectivity other than 4 or 8, min_area < 1, a threshold outside
 * the limits above, a misaligned int64 buffer or workspace, a workspace that is too small. */
size_t sg_object_workspace_bytes(int64_t n_pixels_total);
int sg_object_match(const int64_t* labels, const void* gt, int gt_format, const int32_t* image_hw, const int64_t* offset, int N, int K,
                    int connectivity, int64_t min_area, int64_t skip_label, int use_skip, int iou_num, int iou_den, int ignore_index,
                    int reduce_zero_label, int64_t* counts, uint8_t* match_map, void* workspace, size_t workspace_bytes, sg_stream s);

#ifdef __cplusplus
}
#endif
#endif /* SEGEARTH_HIP_H */
