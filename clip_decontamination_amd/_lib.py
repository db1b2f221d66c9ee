"""ctypes binding of libsegearth_hip.so (the C ABI declared in include/segearth_hip.h).

The product path has NO CPU fallback: if the shared library is missing or fails to load, importing
any op raises immediately with the build command.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SEGEARTH_HIP_LIB: another build of the same library (same-box A/B measurements of a kernel change); the default is the in-tree build
LIB_PATH = os.environ.get("SEGEARTH_HIP_LIB") or os.path.join(HERE, "libsegearth_hip.so")

# enums (include/segearth_hip.h)
PREC_F32, PREC_BF16, PREC_FP8, PREC_F16, PREC_F16X2 = 0, 1, 2, 3, 4
MODEL_TYPES = {"vanilla": 0, "MaskCLIP": 1, "ClearCLIP": 2, "SCLIP": 3, "SegEarth": 4, "SFP": 5, "Experimental": 6,
               "NACLIP": 7, "NOnly": 8, "GAV": 9, "GEM": 10}
IMG_F32_NCHW, IMG_U8_NHWC = 0, 1
GT_U8, GT_I64 = 0, 1
TOL_REGION, TOL_CONTOUR = 0, 1


class VitDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "layers", "heads", "patch", "embed_dim", "grid0", "mlp_width",
                                          "quick_gelu", "precision")]


class ForwardOpts(C.Structure):
    _fields_ = [("model_type", C.c_int32), ("ignore_residual", C.c_int32), ("similarity_enabled", C.c_int32),
                ("similarity_weight", C.c_float), ("similarity_temperature", C.c_float), ("similarity_add_self", C.c_int32),
                ("outlier_enabled", C.c_int32), ("outlier_top_k", C.c_int32), ("outlier_contamination_temp", C.c_float),
                ("selfattn_enabled", C.c_int32), ("selfattn_mode", C.c_int32), ("selfattn_top_k", C.c_int32),
                ("selfattn_strength", C.c_float), ("selfattn_threshold", C.c_float), ("gem_depth", C.c_int32),
                ("layer_fusion_enabled", C.c_int32), ("layer_fusion_lambda", C.c_float)]


class TileBatch(C.Structure):
    _fields_ = [("scene", C.c_void_p), ("format", C.c_int32), ("scene_h", C.c_int32), ("scene_w", C.c_int32),
                ("windows", C.c_void_p), ("scene_index", C.c_void_p), ("scene_stride", C.c_int64), ("n_tiles", C.c_int32), ("tile_h", C.c_int32), ("tile_w", C.c_int32),
                ("pad_l", C.c_int32), ("pad_t", C.c_int32), ("grid_h", C.c_int32), ("grid_w", C.c_int32)]


class JbuCaptureSlot(C.Structure):
    """sg_jbu_capture_slot (include/segearth_hip.h): caller's device buffer, its size, the bytes the last call copied."""
    _fields_ = [("dst", C.c_void_p), ("cap", C.c_size_t), ("bytes", C.c_size_t)]


JBU_CAP_STAGE = ("GS", "PROJ", "X", "X16", "H1", "KF", "SRC", "HR", "OUT", "OUT16")        # SG_JBU_CAP_* per stage, in enum order
JBU_CAP_TAIL = ("FIN_A", "FIN_RES", "GEFF", "G0", "CLSL", "ROWDOT")


class JbuCapture(C.Structure):
    """sg_jbu_capture: per stage and tail slots (test instrumentation of the upsampler, sg_jbu_set_capture)."""
    _fields_ = [("stage", (JbuCaptureSlot * len(JBU_CAP_STAGE)) * 4), ("tail", JbuCaptureSlot * len(JBU_CAP_TAIL))]


P, I, F, Z, L = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64

# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against the header
SIGNATURES = {
    "sg_last_error": (C.c_char_p, []),
    "sg_version": (I, []),
    "sg_profile_enable": (I, [I]),
    "sg_profile_disable": (I, []),
    "sg_gemm_persist_last_kstep": (I, []),
    "sg_gemm_last_kernel": (C.c_char_p, []),
    "sg_attention_last_kernel": (C.c_char_p, []),
    "sg_attention_last_body": (C.c_char_p, []),
    "sg_set_gemm_config": (I, [I]),
    "sg_profile_read": (I, [I, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(L), C.POINTER(L)]),
    "sg_create": (I, [C.POINTER(P), I, C.POINTER(VitDesc)]),
    "sg_destroy": (None, [P]),
    "sg_vit_set_tensor": (I, [P, C.c_char_p, P, L, P]),
    "sg_vit_finalize": (I, [P, P]),
    "sg_vit_workspace_bytes": (Z, [P, I, I, I, C.POINTER(ForwardOpts)]),
    "sg_vit_forward": (I, [P, C.POINTER(TileBatch), C.POINTER(ForwardOpts), P, P, P, Z, P]),
    "sg_cosine_logits": (I, [P, P, P, I, I, I, I, F, F, P, P]),
    "sg_cosine_logits_two_plane": (I, [P, P, P, I, I, I, I, F, P, P]),
    "sg_stitch": (I, [P, P, I, I, I, I, I, I, I, I, I, I, P, P]),
    "sg_resize_bilinear": (I, [P, I, I, I, P, I, I, P]),
    "sg_postprocess": (I, [P, P, I, I, I, I, F, F, I, P, P, P]),
    "sg_stitch_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, I, L, L, P, P]),
    "sg_postprocess_multi": (I, [P, P, P, P, P, P, I, L, L, L, P, I, I, F, F, I, P, P, P]),
    "sg_cosine_logits_wide": (I, [P, P, P, I, I, I, I, F, F, P, P]),
    "sg_postprocess_wide": (I, [P, P, I, I, I, I, F, F, I, P, P, P]),
    "sg_label_head": (I, [P, P, I, I, I, I, I, I, I, I, I, I, P, I, F, F, I, P, P, P]),
    "sg_label_head_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, I, L, L, P, I, F, F, I, P, P, P]),
    "sg_stitch_blend": (I, [P, P, I, I, I, I, I, I, I, I, I, I, P, P, I, P]),
    "sg_stitch_blend_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, I, L, L, P, P, I, P]),
    "sg_label_head_blend": (I, [P, P, I, I, I, I, I, I, I, I, I, I, P, I, F, F, I, P, P, P, I, P]),
    "sg_label_head_blend_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, I, L, L, P, I, F, F, I, P, P, P, I, P]),
    "sg_prob_head": (I, [P, P, I, I, I, I, I, I, I, I, I, I, P, I, F, F, I, P, P, P]),
    "sg_prob_head_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, I, L, L, P, I, F, F, I, P, P, P]),
    "sg_topk_head": (I, [P, P, I, I, I, I, I, I, I, I, I, I, P, I, F, I, P, P, P]),
    "sg_topk_head_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, I, L, L, P, I, F, I, P, P, P]),
    "sg_label_head_resized": (I, [P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, I, F, F, I, P, P, I, P]),
    "sg_label_head_resized_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, P, I, L, L, P, I, F, F, I, P, P, I, P]),
    "sg_topk_head_resized": (I, [P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, I, F, I, P, P, I, P]),
    "sg_topk_head_resized_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, P, I, L, L, P, I, F, I, P, P, I, P]),
    "sg_tta_head": (I, [P, L, P, I, P, I, I, I, I, P, I, F, F, I, P, P, P, I, P]),
    "sg_tta_accumulate": (I, [P, I, I, I, I, P, I, P]),
    "sg_tta_finish": (I, [P, I, I, I, I, F, I, P, P, P, P]),
    "sg_outlier_scratch_bytes": (Z, [I, I, I]),
    "sg_outlier_suppress": (I, [P, P, P, I, I, I, I, I, F, P, P, P]),
    "sg_cross_tile_scratch_bytes": (Z, [I, I, I, I, I]),
    "sg_cross_tile_fusion": (I, [P, I, I, I, I, I, I, I, F, P, P]),
    "sg_cross_tile_pack": (I, [P, P, I, I, I, I, I, I, I, I, P, P]),
    "sg_cross_tile_fuse": (I, [P, P, I, I, I, I, I, I, I, I, F, I, P, P]),
    "sg_cross_tile_apply": (I, [P, P, P, I, I, I, I, I, I, I, P]),
    "sg_weak_token_replace": (I, [P, P, I, I, I, I, I, P, P, P]),
    "sg_similarity_map": (I, [P, L, I, I, I, I, F, I, I, P, P, Z, P]),
    "sg_op_linear": (I, [P, P, P, P, P, I, I, I, I, I, P, Z, P]),
    "sg_gemm_bf16_raw": (I, [P, P, P, P, P, I, I, I, I, I, P]),
    "sg_gemm_raw": (I, [I, P, P, P, P, P, I, I, I, I, I, I, P]),
    "sg_gemm_fp8_raw": (I, [P, P, P, P, P, P, P, I, I, I, I, I, P]),
    "sg_op_ln_chain_scratch_bytes": (Z, [I, I, I, I]),
    "sg_op_ln_chain": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "sg_gemm_fp8_mx_raw": (I, [P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, P]),
    "sg_quantize_rows_fp8": (I, [P, L, I, P, P, P]),
    "sg_op_layernorm": (I, [P, P, P, P, I, I, F, P]),
    "sg_attention_raw": (I, [I, P, P, P, P, P, P, L, L, P, L, L, I, I, I, I, I, I, I, F, P, P, F, L, P, P, I, P, P, P, L, L, F, P]),
    "sg_attention_stats_raw": (I, [I, P, L, L, P, I, I, I, I, F, P, P, P]),
    "sg_layernorm_raw": (I, [P, L, P, P, P, L, I, L, I, F, P]),
    "sg_layernorm_fp8_raw": (I, [P, L, P, P, P, L, P, L, I, F, P]),
    "sg_quantize_rows_raw": (I, [P, I, L, P, L, P, L, I, P]),
    "sg_embed_assemble_raw": (I, [P, L, P, P, P, P, P, I, I, I, F, P]),
    "sg_posembed_resize_raw": (I, [P, I, I, I, I, I, P, P]),
    "sg_pack_rows_raw": (I, [P, L, I, L, P, I, I, P]),
    "sg_transpose_pack_raw": (I, [P, I, I, P, I, P]),
    "sg_ln_stats_finalize_raw": (I, [P, L, I, F, P, P]),
    "sg_fold_ln_weight_raw": (I, [P, I, I, P, P, P, I, P, P, P, P]),
    "sg_l2norm_rows_raw": (I, [P, I, L, L, I, P, I, L, L, L, I, F, P]),
    "sg_softmax_rows_raw": (I, [P, L, L, I, I, P, F, P, F, L, P, P, I, I, I, P, P, P]),
    "sg_gaussian_bias_raw": (I, [I, I, F, P, P]),
    "sg_head_norms_raw": (I, [P, I, L, L, I, I, I, I, P, P]),
    "sg_axpby_raw": (I, [P, P, F, F, L, P]),
    "sg_gem_inv_temp_raw": (I, [P, I, I, I, F, P, P]),
    "sg_patchify_raw": (I, [C.POINTER(TileBatch), I, I, P, I, P]),
    "sg_gemm_f32_raw": (I, [P, L, L, L, P, L, L, L, L, P, P, L, P, L, L, L, I, I, I, I, I, I, F, P]),
    "sg_attn_average_raw": (I, [I, P, I, I, I, I, P, Z, P, P]),
    "sg_attn_enhance_raw": (I, [P, L, L, P, I, I, I, F, F, P, P]),
    "sg_layer_fusion_apply_raw": (I, [P, P, I, I, I, I, P, P, P, P, P]),
    "sg_op_attention_scratch_bytes": (Z, [I, I, I, I, I]),
    "sg_op_attention": (I, [P, I, I, I, I, I, P, F, P, P, P, I, P, Z, P]),
    "sg_adaptive_conv": (I, [P, P, I, I, I, I, I, P, P]),
    "sg_render_maps": (I, [P, P, P, I, I, I, P, P, P]),
    "sg_ctd_scratch_bytes": (Z, [I, I, I]),
    "sg_ctd_debias": (I, [P, P, I, I, I, C.c_double, I, F, I, P, P, Z, P]),
    "sg_text_create": (I, [C.POINTER(P), I, I, I, I, I, I, I, I, I]),
    "sg_text_destroy": (None, [P]),
    "sg_text_set_tensor": (I, [P, C.c_char_p, P, L, P]),
    "sg_text_workspace_bytes": (Z, [P, I]),
    "sg_text_encode": (I, [P, P, I, P, P, Z, P]),
    "sg_jbu_create": (I, [C.POINTER(P), I, I, I]),
    "sg_jbu_destroy": (None, [P]),
    "sg_jbu_set_tensor": (I, [P, C.c_char_p, P, L, P]),
    "sg_jbu_workspace_bytes": (Z, [P, I, I, I]),
    "sg_jbu_upsample": (I, [P, P, P, I, I, I, I, I, I, P, P, Z, P]),
    "sg_jbu_logits": (I, [P, P, P, I, I, I, I, I, I, P, I, P, F, P, P, Z, P]),
    "sg_jbu_workspace_bytes_wide": (Z, [P, I, I, I, I]),
    "sg_jbu_logits_wide": (I, [P, P, P, I, I, I, I, I, I, P, I, P, F, P, P, Z, P]),
    "sg_jbu_set_capture": (I, [P, P]),
    "sg_jbu_last_kernels": (C.c_char_p, []),
    "sg_extract_tiles": (I, [C.POINTER(TileBatch), I, I, P, P]),
    "sg_global_debias": (I, [P, P, I, I, I, F, P, P]),
    "sg_confusion_accumulate": (I, [P, P, I, L, I, I, I, P, P]),
    "sg_pamr_workspace_bytes": (Z, [I, I, I, I]),
    "sg_pamr_affinity": (I, [P, I, I, C.POINTER(I), I, P, P]),
    "sg_pamr_step": (I, [P, P, P, I, I, I, C.POINTER(I), I, P]),
    "sg_pamr": (I, [P, P, I, I, I, C.POINTER(I), I, I, P, Z, P]),
    "sg_class_area": (I, [P, L, I, P, P]),
    "sg_class_area_multi": (I, [P, P, P, P, I, L, L, I, P, P]),
    "sg_area_keep": (I, [P, I, I, I, C.c_double, P, P]),
    "sg_area_filter_probs": (I, [P, P, P, I, I, I, F, I, P, P]),
    "sg_area_filter_probs_multi": (I, [P, P, P, P, P, P, I, L, L, I, F, I, P, P]),
    "sg_area_relabel": (I, [P, P, I, I, I, I, I, I, I, I, I, I, P, I, F, F, I, P, P, P, P]),
    "sg_area_relabel_multi": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P, P, P, I, L, L, P, I, F, F, I, P, P, P, P]),
    "sg_sieve_workspace_bytes": (Z, [L, I]),
    "sg_sieve": (I, [P, P, P, P, I, L, I, I, L, P, Z, P]),
    "sg_regions_workspace_bytes": (Z, [L, L]),
    "sg_regions": (I, [P, P, P, P, I, I, L, L, I, L, P, P, P, P, Z, P]),
    "sg_boundary_workspace_bytes": (Z, [L]),
    "sg_boundary_band": (I, [P, I, P, P, P, I, P, P, Z, P]),
    "sg_boundary_accumulate": (I, [P, P, I, P, P, P, I, I, I, I, P, P, Z, P]),
    "sg_tolerant_workspace_bytes": (Z, [L, I]),
    "sg_tolerant_accumulate": (I, [P, P, I, P, P, P, I, I, I, I, I, P, P, Z, P]),
    "sg_object_workspace_bytes": (Z, [L]),
    "sg_object_match": (I, [P, P, I, P, P, I, I, I, L, L, I, I, I, I, I, P, P, P, Z, P]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP library or fail loudly -- there is no other implementation of the hot path."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch owns device memory and streams, so the library must bind to the SAME HIP runtime instance:
    # import torch first (its bundled libamdhip64 is then the one already loaded when ours resolves).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -m clip_decontamination_amd.build` (needs hipcc, cross-compiles for gfx950). "
            "There is no CPU fallback for the segmentation hot path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().sg_last_error().decode(errors="replace")
        raise RuntimeError(f"libsegearth_hip {what} failed ({rc}): {msg}")
