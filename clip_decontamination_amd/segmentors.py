"""Host-side implementation shared by the two drop-in entry points (repo-root ``segmentor.py`` /
``segearth_segmentor.py``).  Same class names, constructor kwargs, public methods and return types as the
reference (segmentor.py:25-546, segearth_segmentor.py:22-326); the bodies call the HIP library.

What differs, and why (none of it is on the hot path):
  * weights: every pretrained tag of the reference resolves to a download (segmentor.py:69-128), impossible
    offline.  The drop-in takes ``checkpoint=`` (a local state dict holding ``visual.*`` tensors, loaded with
    ``weights_only=True``) or, with ``synthetic_ok=True``, the deterministic synthetic weights used for parity.
  * text features: ``tokenizer=`` (callable: list[str] -> int ids [n, 77]; the BPE vocabulary is a downloaded
    asset) together with a ``checkpoint`` that holds the text tower runs the reference's own route
    (segmentor.py:157-174) on the HIP text tower (``sg_text_encode``).  Alternatives: ``text_features=`` ([Q,E]
    tensor / .npy / .pt path) or ``text_encoder=`` (callable: list[str] -> [n,E] tensor); the 80-template
    prompt ensemble is applied here in every case.
  * ``precision=`` (default ``"f16x2"``): the arithmetic of the tower.  The reference runs ``.half()`` on the GPU (segmentor.py:467) and fp32
    on the CPU; the default here is the most faithful mode that clears the 50 Mpix/s target -- two f16 planes per operand, three MFMAs
    per product: the fp32 path's logits (max |dlogit| 5e-7 on the bench tiles) and labels (identical up to fp32 ties) at ~95 Mpix/s for
    ViT-L/14.  ``"bf16"`` (225 Mpix/s, 5e-3 / 99.4 % labels), ``"f16"``, ``"fp8"`` trade accuracy for speed; ``"f32"`` is the f32-MFMA parity mode.
"""
from __future__ import annotations

import os
import warnings
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn as nn

from . import weights as Wt
from .engine import (HipCLIP, HipVisionTower, OutlierSuppressionModule, SelfAttentionEnhancementModule,
                     SimilarityEnhancementModule, compute_padsize)
from .pipeline import SegPipeline
from .prompts import ensemble_prompts

try:  # the reference's plugin registry, when mmseg is installed
    from mmseg.models.segmentors import BaseSegmentor as _Base
    from mmseg.models.data_preprocessor import SegDataPreProcessor
    from mmseg.registry import MODELS
    from mmengine.structures import PixelData
    HAVE_MMSEG = True
except Exception:  # stand-alone use (tests, bench, serving)
    HAVE_MMSEG = False

    class _Base(nn.Module):
        def __init__(self, data_preprocessor=None, **_):
            super().__init__()
            self.data_preprocessor = data_preprocessor

    class SegDataPreProcessor:
        def __init__(self, mean=None, std=None, bgr_to_rgb=False, **_):
            self.mean, self.std, self.bgr_to_rgb = mean, std, bgr_to_rgb

    class PixelData:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    MODELS = _Registry()


class _RegionSample:
    """The least of a data sample that ``predict`` fills: predict_regions(with_score=True) without data samples, whole-image inference."""

    def __init__(self, metainfo):
        self.metainfo = metainfo

    def set_data(self, data):
        self.__dict__.update(data)


def get_cls_idx(path):
    """One class per line, commas separate synonym queries (reference segmentor.py:611-622)."""
    with open(path, "r") as f:
        name_sets = f.readlines()
    class_names, class_indices = [], []
    for idx, line in enumerate(name_sets):
        names_i = line.split(",")
        class_names += names_i
        class_indices += [idx for _ in range(len(names_i))]
    class_names = [item.replace("\n", "") for item in class_names]
    return class_names, class_indices


def _vit_name(clip_type: str, vit_type: str) -> str:
    """The architecture the reference would have built for (clip_type, vit_type) (segmentor.py:69-128)."""
    if "tiny" in vit_type:
        return vit_type
    if "B" in vit_type:
        return "ViT-B-16" if clip_type in ("CLIP", "OpenCLIP", "MetaCLIP") else "ViT-B-32"
    if "L" in vit_type:
        return "ViT-L-14"
    if "H" in vit_type:
        return "ViT-H-14"
    raise ValueError(f"unsupported vit_type {vit_type!r}")


def _load_full_state(path: str):
    """The whole CLIP state dict (text tower included); loaders that execute nothing from the file."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return {k: torch.from_numpy(z[k]) for k in z.files}
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return sd["state_dict"] if isinstance(sd, dict) and "state_dict" in sd else sd


def _load_state(path: str):
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    elif path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            sd = {k: torch.from_numpy(z[k]) for k in z.files}
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd:
            sd = sd["state_dict"]
    vis = {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}
    return vis if vis else sd


def _to_bool(value):
    if isinstance(value, str):
        return value.strip().lower() in ("1", "true", "yes", "y", "on")
    return bool(value)


class _HipSegmentorBase(_Base):
    """Everything both reference classes share: construction of the tower, text features, slide / feature /
    post-process methods."""

    _to_bool = staticmethod(_to_bool)

    def _setup(self, clip_type, vit_type, model_type, name_path, device, ignore_residual, prob_thd, logit_scale, slide_stride,
               slide_crop, cls_token_lambda, bg_idx, apply_sim_feat_up, sim_feat_up_cfg, global_debias_factor=0.0,
               checkpoint=None, text_features=None, text_encoder: Optional[Callable] = None, precision="f16x2",
               synthetic_ok=False, tiles_per_launch=None, jbu_checkpoint_ok=True, tokenizer: Optional[Callable] = None, tile_group=None,
               label_head="auto", prob_head="auto", pamr_steps=0, pamr_stride=(8, 16), resize_head="canvas", area_thd=None,
               min_region=None, region_connectivity=4, region_fill="neighbour", blend="uniform", blend_ramp=None,
               tta_scales=None, tta_flip=False, tta_head="auto"):
        from . import ops
        from .pipeline import (AREA_TILE_GROUP, LABEL_HEADS, PAMR_TILE_GROUP, PROB_HEADS, RESIZE_HEADS, SIEVE_TILE_GROUP, TTA_AREA, TTA_HEADS,
                               TTA_PAMR, TTA_TILE_GROUP)
        # Test-time augmentation (tta_scales=None and tta_flip=False = off): predict / predict_many / predict_regions / evaluate run every
        # image as the views ops.tta_views lists and average the views' class probabilities at ori_shape before the arg-max (SegPipeline;
        # the definition: include/segearth_hip.h); seg_logits are the mean planes.  forward_slide / forward_feature return the logits of
        # the image as it is.  Refused with tile_group, PAMR, area_thd and predict_topk.
        if tta_head not in TTA_HEADS:
            raise ValueError(f"tta_head must be one of {TTA_HEADS}, got {tta_head!r}")
        self.tta_scales = None if tta_scales is None else tuple(float(v) for v in ([tta_scales] if isinstance(tta_scales, (int, float)) else tta_scales))
        self.tta_flip, self.tta_head = _to_bool(tta_flip), tta_head
        if self.tta_scales is not None or self.tta_flip:
            ops.tta_views((64, 64), self.tta_scales, self.tta_flip)
            for on, why in ((tile_group is not None, TTA_TILE_GROUP), (int(pamr_steps) > 0, TTA_PAMR), (area_thd is not None, TTA_AREA)):
                if on:
                    raise ValueError(why)
        # blend ("uniform" = off) / blend_ramp: overlapping windows combined by a ramp-weighted mean instead of the plain one (SegPipeline;
        # the definition: include/segearth_hip.h).  Whole-image inference (slide_crop <= 0) has no windows and ignores it.
        self.blend, self.blend_ramp = ops.blend_args(blend, blend_ramp)
        # min_region (None = off): the last step on the final labels of predict / predict_many / evaluate -- connected regions of fewer
        # than min_region pixels are sieved out on the device (SegPipeline; the definition: include/segearth_hip.h)
        _, self.region_connectivity, self.region_fill = ops.sieve_args(1 if min_region is None else min_region, region_connectivity, region_fill)
        self.min_region = min_region
        if min_region is not None and tile_group is not None:
            raise ValueError(SIEVE_TILE_GROUP)
        # area_thd (the upstream option name; None = off): per image, a class that wins at most this share of the non-background pixels is
        # removed and its pixels go to the best remaining class (SegPipeline; the definition: include/segearth_hip.h).  The background
        # class is always kept, so 0 <= bg_idx < the number of classes is required (checked below, once the class file is read).
        if area_thd is not None:
            if not float(area_thd) >= 0.0:
                raise ValueError(f"area_thd must be None or a number >= 0 (a share of the non-background pixels), got {area_thd!r}")
            if tile_group is not None:
                raise ValueError(AREA_TILE_GROUP)
        self.area_thd = None if area_thd is None else float(area_thd)
        if resize_head not in RESIZE_HEADS:
            raise ValueError(f"resize_head must be one of {RESIZE_HEADS}, got {resize_head!r}")
        # labels and the k best classes at another ori_shape than the image's: "canvas" = stitch, resize the canvas, post-process; "fused" =
        # sg_label_head_resized / sg_topk_head_resized, the resize inside the head and no canvas (not with PAMR or whole-image inference)
        self.resize_head = resize_head
        if label_head not in LABEL_HEADS:
            raise ValueError(f"label_head must be one of {LABEL_HEADS}, got {label_head!r}")
        if prob_head not in PROB_HEADS:
            raise ValueError(f"prob_head must be one of {PROB_HEADS}, got {prob_head!r}")
        # the tail of ``predict`` / ``predict_many`` with data samples (class probabilities + labels): "canvas" = stitch + post-process,
        # "fused" = sg_prob_head (no canvas, the same bytes), "auto" = SegPipeline.fused_prob_head
        self.prob_head = prob_head
        # the labels-only tail: "canvas" = stitch + post-process through the [Q,H,W] canvas, "fused" = sg_label_head (no canvas, any
        # number of queries), "auto" = the canvas wherever it works (Q <= 64) and the fused head beyond
        self.label_head = label_head
        self.tile_group = tile_group                         # opt-in tile sharding (pipeline.resolve_tile_group); None = off
        # PAMR (the upstream option names): ``pamr_steps`` refinement steps over the dilations ``pamr_stride`` on the stitched logits, after
        # the resize to ori_shape and before the post-process; 0 = off.  With PAMR on every tail that returns labels or probabilities takes
        # the canvas route, whatever label_head / prob_head say (SegPipeline).
        self.pamr_steps, self.pamr_stride = int(pamr_steps), ops.pamr_dilations(pamr_stride)[0]
        if not 0 <= self.pamr_steps <= ops.PAMR_MAX_STEPS:
            raise ValueError(f"pamr_steps must lie in [0, {ops.PAMR_MAX_STEPS}], got {pamr_steps!r}")
        if self.pamr_steps > 0 and tile_group is not None:
            raise ValueError(PAMR_TILE_GROUP)
        if clip_type == "BLIP":
            raise NotImplementedError("clip_type='BLIP' is a different backbone (vendored BLIP) and is out of scope for the HIP path")
        self.clip_type, self.vit_type, self.model_type = clip_type, vit_type, model_type
        dev = torch.device(device) if not isinstance(device, torch.device) else device
        if dev.type != "cuda":
            raise RuntimeError("the drop-in segmentors run on the GPU only (HIP hot path, no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        quick = clip_type in ("CLIP", "MetaCLIP")            # openai / *-quickgelu tags (model.py:116,518)
        cfg = Wt.vit_config(_vit_name(clip_type, vit_type), quick_gelu=None if "tiny" in vit_type else quick)
        checkpoint = checkpoint or os.environ.get("SEGEARTH_CLIP_CHECKPOINT")
        if checkpoint:
            state = _load_state(checkpoint)
        elif synthetic_ok:
            warnings.warn("SegEarth drop-in: using deterministic SYNTHETIC vision weights (no pretrained checkpoint given)")
            state = Wt.make_vit_weights(cfg, seed=0)
        else:
            raise RuntimeError("no vision checkpoint: pass checkpoint=<path to a state dict with visual.* tensors> "
                               "(or set SEGEARTH_CLIP_CHECKPOINT); pretrained tags cannot be downloaded here. "
                               "synthetic_ok=True selects the synthetic parity weights.")
        visual = HipVisionTower(cfg, state, precision=precision, device=dev)
        visual.gem_ignore_residual = ignore_residual
        self.net = HipCLIP(visual)
        self.patch_size = visual.patch_size
        self.cls_token_lambda = cls_token_lambda
        self.global_debias_factor = global_debias_factor
        self.bg_idx = bg_idx
        self.apply_sim_feat_up = apply_sim_feat_up

        query_words, query_idx = get_cls_idx(name_path)
        self.num_queries = len(query_words)
        self.num_classes = max(query_idx) + 1
        if self.area_thd is not None:
            ops.area_args("area_thd", self.num_classes, bg_idx)
        self.query_idx = torch.tensor(query_idx, dtype=torch.int64, device=dev)
        E = cfg.embed_dim
        if text_features is not None:
            tf = text_features
            if isinstance(tf, str):
                tf = torch.from_numpy(np.load(tf, allow_pickle=False)) if tf.endswith(".npy") else torch.load(tf, map_location="cpu", weights_only=True)
            tf = torch.as_tensor(tf).float()
        elif text_encoder is not None:
            feats = []
            with torch.no_grad():
                for qw in query_words:                                   # segmentor.py:159-173
                    f = torch.as_tensor(text_encoder(ensemble_prompts(qw))).float()
                    f = f / f.norm(dim=-1, keepdim=True)
                    f = f.mean(dim=0)
                    feats.append((f / f.norm()).unsqueeze(0))
            tf = torch.cat(feats, 0)
        elif tokenizer is not None:
            # the reference's own route (segmentor.py:157-174): tokenizer -> net.encode_text, here on the HIP text tower
            from .engine import HipTextTower
            full = _load_full_state(checkpoint) if checkpoint else None
            if not full or "token_embedding.weight" not in full:
                raise RuntimeError("tokenizer= given but the checkpoint holds no text tower (token_embedding.weight ...)")
            tcfg = Wt.TEXT_CONFIGS[cfg.name] if cfg.name in Wt.TEXT_CONFIGS else None
            if tcfg is None:
                raise RuntimeError(f"no text configuration known for {cfg.name}")
            if tcfg.quick_gelu != quick:
                tcfg = Wt.TextConfig(**{**tcfg.__dict__, "quick_gelu": quick})
            self.net.text = HipTextTower(tcfg, full, precision="f32", device=dev)
            tf = self.net.text.query_features(tokenizer, query_words).cpu()
        elif synthetic_ok:
            warnings.warn("SegEarth drop-in: using SYNTHETIC text features")
            tf = torch.from_numpy(Wt.make_text_features(self.num_queries, E))
        else:
            raise RuntimeError("no text features: pass text_features=[Q,E], text_encoder=callable, or tokenizer=callable together "
                               "with a checkpoint that holds the text tower")
        if tuple(tf.shape) != (self.num_queries, E):
            raise ValueError(f"text features have shape {tuple(tf.shape)}, expected ({self.num_queries}, {E})")
        self.query_features = tf.to(dev)
        self.dtype = self.query_features.dtype
        self.ignore_residual = ignore_residual
        self.logit_scale, self.prob_thd = logit_scale, prob_thd
        self.slide_stride, self.slide_crop = slide_stride, slide_crop
        self.upsampler = None
        if apply_sim_feat_up:
            from .upsampler import HipJBU
            self.feat_dim = E
            cfgu = sim_feat_up_cfg or {}
            self.upsampler = HipJBU.from_config(cfgu.get("model_name", "jbu_one"), E, cfgu.get("model_path"), dev,
                                                synthetic_ok=synthetic_ok, precision=precision)
        # tiles per tower launch: None = the machine-filling size for this tower and tile (about ten rounds of 256 x 256 GEMM tiles on the 256 CUs:
        # 119 tiles of 512 for ViT-L/14, 95 for ViT-H/14, capped at 128; measured 228 Mpix/s at 119 tiles against 213 at 32)
        if tiles_per_launch is None:
            vc = visual.cfg
            crop = slide_crop if isinstance(slide_crop, int) and slide_crop > 0 else 512
            n_tok = (-(-crop // vc.patch)) ** 2 + 1
            tiles_per_launch = max(1, min(128, (2560 // max(1, -(-vc.width // 256))) * 256 // n_tok))
        self._tiles_per_launch = tiles_per_launch
        self._pipe = None
        return visual

    # -- pipeline object (rebuilt lazily so attribute edits after construction are honoured) ---------------------
    def _pipeline(self) -> SegPipeline:
        return SegPipeline(self.net, self.query_features, self.query_idx, model_type=self.model_type,
                           ignore_residual=self.ignore_residual, cls_token_lambda=self.cls_token_lambda,
                           global_debias_factor=self.global_debias_factor, logit_scale=self.logit_scale, prob_thd=self.prob_thd,
                           bg_idx=self.bg_idx, apply_similarity_enhancement=getattr(self, "apply_similarity_enhancement", False),
                           upsampler=self.upsampler, tiles_per_launch=self._tiles_per_launch,
                           cross_tile_fusion=getattr(self, "cross_tile_fusion_cfg", None), apply_ctd=getattr(self, "apply_ctd", False),
                           tile_group=getattr(self, "tile_group", None), apply_layer_fusion=getattr(self, "apply_layer_fusion", False),
                           layer_fusion_lambda=getattr(self, "layer_fusion_lambda", 0.5), label_head=getattr(self, "label_head", "auto"),
                           prob_head=getattr(self, "prob_head", "auto"), pamr_steps=getattr(self, "pamr_steps", 0),
                           pamr_stride=getattr(self, "pamr_stride", (8, 16)), resize_head=getattr(self, "resize_head", "canvas"),
                           area_thd=getattr(self, "area_thd", None), min_region=getattr(self, "min_region", None),
                           region_connectivity=getattr(self, "region_connectivity", 4), region_fill=getattr(self, "region_fill", "neighbour"),
                           blend=getattr(self, "blend", "uniform"), blend_ramp=getattr(self, "blend_ramp", None),
                           tta_scales=getattr(self, "tta_scales", None), tta_flip=getattr(self, "tta_flip", False),
                           tta_head=getattr(self, "tta_head", "auto"))

    def forward_feature(self, img, logit_size=None, tile_h_idx=None, tile_w_idx=None):
        """Reference segmentor.py:286-392.  img [B,3,H,W] -> logits [B,Q,h,w]."""
        if type(img) == list:
            img = img[0]
        return self._pipeline().forward_feature(img.float(), logit_size)

    def forward_slide(self, img, img_metas, stride=112, crop_size=224):
        """Reference segmentor.py:394-451.  One image [1,3,H,W] (or a list holding one [3,H,W])."""
        if type(img) == list:
            img = img[0].unsqueeze(0)
        pipe = self._pipeline()
        if getattr(self, "pack_images", False) and img.shape[0] > 1:        # opt-in: the windows of all B images in shared launches
            ori = [tuple(m["ori_shape"][:2]) for m in img_metas] if img_metas is not None else None
            return torch.cat(pipe.forward_slide_many(img.float(), stride, crop_size, ori), 0)
        outs = []
        for b in range(img.shape[0]):
            ori = img_metas[b]["ori_shape"][:2] if img_metas is not None else None
            outs.append(pipe.forward_slide(img[b].float(), stride, crop_size, ori))
        return torch.cat(outs, 0)

    @torch.no_grad()
    def predict(self, inputs, data_samples):
        """Reference segmentor.py:453-473.  With PAMR on (``pamr_steps > 0``) the stitched logits of every image are refined under that
        image (resized to ``ori_shape`` where the logits are) before the post-process, on the canvas route whatever label_head /
        prob_head say; whole-image inference (``slide_crop <= 0``) likewise.
        With ``area_thd`` set the tail runs twice over the decision: the first pass with ``prob_thd = 0`` gives the plain arg-max, its
        per-image class areas decide which classes stay (sg_class_area, sg_area_keep: on the device, no host synchronisation), and
        ``seg_logits`` hold the probabilities with the dropped planes zeroed, ``pred_sem_seg`` the best kept class (sg_area_filter_probs).
        Labels alone on the fused label head need no probability planes for it (sg_area_relabel); labels alone on the canvas route
        write the probabilities into a scratch [K,H,W] first -- the fused head is the memory-lean way.
        With ``min_region`` set the connected regions of fewer than ``min_region`` pixels are sieved out of the final labels (sg_sieve,
        after prob_thd and area_thd, at ``ori_shape``, whatever route the tail took): ``pred_sem_seg`` holds the sieved labels,
        ``seg_logits`` are left as they are."""
        if data_samples is not None:
            batch_img_metas = [data_sample.metainfo for data_sample in data_samples]
        else:
            batch_img_metas = [dict(ori_shape=inputs.shape[2:], img_shape=inputs.shape[2:], pad_shape=inputs.shape[2:],
                                    padding_size=[0, 0, 0, 0])] * inputs.shape[0]
        inputs = inputs.float()
        if getattr(self, "tta_scales", None) is not None or getattr(self, "tta_flip", False):
            # test-time augmentation: every image through SegPipeline.tta_image at its ori_shape (sliding windows or whole image)
            pipe = self._pipeline()
            if data_samples is None:
                return pipe.tta_image(inputs[0], self.slide_stride, self.slide_crop)
            for i, ds in enumerate(data_samples):
                probs, labels = pipe.tta_image(inputs[i], self.slide_stride, self.slide_crop, tuple(batch_img_metas[i]["ori_shape"][:2]), True)
                self._fill_sample(ds, probs, labels, i)
            return data_samples
        if data_samples is None and self.slide_crop > 0:
            # labels only, at the image's own size, of the first image (what postprocess_result returns without data samples): the
            # labels-only tail, which needs no canvas with the fused head (``label_head``)
            return self._pipeline().segment_scene(inputs[0], self.slide_stride, self.slide_crop)
        if self.slide_crop > 0 and getattr(self, "tile_group", None) is None and \
                all(tuple(m["ori_shape"][:2]) == tuple(inputs.shape[2:]) for m in batch_img_metas):
            pipe = self._pipeline()
            if pipe.fused_prob_head():
                # tile logits -> probabilities + labels with no canvas (sg_prob_head): the bytes of the canvas route below.  A resize to
                # another ori_shape, tile sharding and whole-image inference keep the canvas.
                if getattr(self, "pack_images", False) and inputs.shape[0] > 1:
                    probs, labels = pipe.segment_scenes(inputs, self.slide_stride, self.slide_crop, want_probs=True)
                else:
                    pl = [pipe.segment_scene(inputs[b], self.slide_stride, self.slide_crop, want_probs=True) for b in range(inputs.shape[0])]
                    probs, labels = [p for p, _ in pl], [l for _, l in pl]
                for i, ds in enumerate(data_samples):
                    self._fill_sample(ds, probs[i], labels[i], i)
                return data_samples
        if self.slide_crop > 0:
            seg_logits = self.forward_slide(inputs, batch_img_metas, self.slide_stride, self.slide_crop)
        else:
            seg_logits = self.forward_feature(inputs, batch_img_metas[0]["ori_shape"])
        if getattr(self, "pamr_steps", 0) > 0:
            pipe = self._pipeline()
            seg_logits = seg_logits.float().contiguous()
            for b in range(seg_logits.shape[0]):                             # in place: each image's logits are a contiguous f32 slice
                pipe.refine(seg_logits[b], inputs[b])
        return self.postprocess_result(seg_logits, data_samples)

    @torch.no_grad()
    def predict_many(self, inputs, data_samples=None, ori_shapes=None):
        """``predict`` for many images with their sliding windows packed into shared tower launches and one stitch + one post-process
        launch per flush group (SegPipeline.segment_scenes).  inputs: a list of [3,H,W] images of any sizes or a [B,3,H,W] batch.
        Fills each data sample exactly as ``predict`` does (seg_logits, pred_sem_seg, result_dir / heatmap_dir PNGs) and returns
        them; with ``data_samples=None`` returns one label map [1,H,W] per image.  In f32 the results equal ``predict`` per image bit
        for bit; in the 2-byte modes a larger launch may take a different GEMM path and differ by 2-byte rounding.  On the canvas route with
        more than 64 queries the one-launch multi-canvas post-process does not apply: data samples are then filled image by image (the
        canvases still come from the packed launches, the probabilities from sg_postprocess_wide per image); ``data_samples=None`` takes the fused
        label head, one launch per flush group.  With the fused probability head selected (``prob_head``) and every ``ori_shape`` equal
        to its image's size, data samples are filled from one sg_prob_head_multi launch per flush group for any number of queries: no
        canvas, and nothing image by image.  With PAMR on (``pamr_steps > 0``) every flush group takes the canvas route and each image's
        canvas is refined before the post-process (SegPipeline.label_groups).
        ``ori_shapes`` (only with ``data_samples=None``; data samples carry their own): one (H, W) or None per image, the size of that
        image's label map.  With ``resize_head="fused"`` the resize runs inside the label head (sg_label_head_resized_multi, one launch
        per flush group, no canvas); otherwise the canvas is stitched, resized and post-processed.
        With ``area_thd`` set every flush group decides twice (``predict``; SegPipeline.label_groups): one launch per step and group,
        labels alone on the fused label head through sg_area_relabel_multi with no probability planes, ``resize_head="fused"`` on the
        canvas route.  With ``min_region`` set the labels of every flush group are sieved by one sg_sieve call (``predict``)."""
        if ori_shapes is not None and data_samples is not None:
            raise ValueError("predict_many: ori_shapes goes with data_samples=None; data samples carry their own ori_shape")
        batch = torch.is_tensor(inputs)
        imgs = inputs.float() if batch else [x[0].float() if x.dim() == 4 else x.float() for x in inputs]
        n = imgs.shape[0] if batch else len(imgs)
        if data_samples is not None and len(data_samples) != n:
            raise ValueError(f"predict_many: {n} images but {len(data_samples)} data samples")
        if ori_shapes is not None and len(ori_shapes) != n:
            raise ValueError(f"predict_many: {n} images but {len(ori_shapes)} ori_shapes")
        if self.slide_crop <= 0 and (getattr(self, "tta_scales", None) is not None or getattr(self, "tta_flip", False)):
            pipe = self._pipeline()                          # whole-image inference under test-time augmentation: image by image
            if data_samples is None:
                return [pipe.tta_image(imgs[i], None, None, None if ori_shapes is None else ori_shapes[i]) for i in range(n)]
            for i, ds in enumerate(data_samples):
                self._fill_sample(ds, *pipe.tta_image(imgs[i], None, None, tuple(ds.metainfo["ori_shape"][:2]), True), i)
            return data_samples
        if self.slide_crop <= 0:                             # whole-image inference (forward_feature) has no windows to pack
            if data_samples is None and ori_shapes is not None:
                pipe = self._pipeline()
                out = []
                for i in range(n):
                    size = tuple(imgs[i].shape[-2:]) if ori_shapes[i] is None else tuple(ori_shapes[i])
                    lg = pipe.refine(pipe.forward_feature(imgs[i][None], size)[0].float().contiguous(), imgs[i])
                    out.append(pipe.sieve(pipe.postprocess(lg, want_probs=False)[1]))
                return out
            if data_samples is None:
                return [self.predict(imgs[i][None], None) for i in range(n)]
            for i in range(n):
                self.predict(imgs[i][None], [data_samples[i]])
            return data_samples
        pipe = self._pipeline()
        if data_samples is None:
            return pipe.segment_scenes(imgs, self.slide_stride, self.slide_crop, want_probs=False, ori_shapes=ori_shapes)
        ori = [tuple(ds.metainfo["ori_shape"][:2]) for ds in data_samples]
        probs, labels = pipe.segment_scenes(imgs, self.slide_stride, self.slide_crop, want_probs=True, ori_shapes=ori)
        for i, ds in enumerate(data_samples):
            self._fill_sample(ds, probs[i], labels[i], i)
        return data_samples

    @torch.no_grad()
    def predict_regions(self, images, data_samples=None, min_area=1, include_bg=False, with_score=False, want_map=False):
        """The label maps of ``predict_many`` and the table of their connected regions (SegPipeline.regions, sg_regions: the definition
        is in include/segearth_hip.h).  images: as ``predict_many``.  The labels come from the calls ``predict_many`` itself makes, every
        option as configured (``area_thd``, ``min_region``, ``blend``, the data samples' ``ori_shape``), so they equal its labels byte
        for byte; the regions are then listed on those final labels by ONE sg_regions call per flush group, on the group's flat label
        buffer (whole-image inference, ``slide_crop <= 0``, has no flush groups: one call per image).  A region is listed when it has
        at least ``min_area`` pixels and, unless ``include_bg``, its label is not ``bg_idx``; connectivity is ``region_connectivity``.
        Returns ``(label_maps, regions)``: one int64 [1,H,W] map and one dict per image (``root``, ``label``, ``area``, ``bbox``,
        ``centroid``, ``score`` / ``score_q``, and ``region_of`` int32 [H,W] with ``want_map``: rows of that image, counted from 0).
        With data samples ``pred_sem_seg`` and ``seg_logits`` are set as ``predict`` sets them -- which means the probability tail runs,
        with or without ``with_score`` -- and the dict is attached as ``pred_regions``.
        ``with_score``: the probability tail that ``predict_many(images, data_samples)`` takes runs instead of the labels-only one
        (without data samples too, at the images' own sizes), and a region's score is the mean probability of its pixels' final label,
        ``probs.gather(0, labels)``; a pixel whose final label is no class plane (a ``bg_idx`` outside [0, K)) scores 0.  This costs
        the K probability planes of every image; the label head's own confidence plane (``conf`` of sg_label_head) is the follow-up
        that needs none.  ``tile_group`` sharding is refused."""
        from . import ops
        from .pipeline import REGIONS_TILE_GROUP
        if getattr(self, "tile_group", None) is not None:
            raise ValueError(REGIONS_TILE_GROUP)
        batch = torch.is_tensor(images)
        imgs = images.float() if batch else [x[0].float() if x.dim() == 4 else x.float() for x in images]
        n = imgs.shape[0] if batch else len(imgs)
        if data_samples is not None and len(data_samples) != n:
            raise ValueError(f"predict_regions: {n} images but {len(data_samples)} data samples")
        ops.regions_args(self.region_connectivity, min_area)                 # before any tower work
        pipe = self._pipeline()
        want_probs = with_score or data_samples is not None
        labels, regions = [None] * n, [None] * n

        def listed(idx, prb, lab, flat):
            """One sg_regions call over the label maps ``lab`` of the images ``idx`` (``flat``: the buffer they are views of)."""
            conf = None
            if with_score:                                                   # the probability of the pixel's final label; no plane: 0
                conf = [ops.label_confidence(p, l).reshape(-1) for p, l in zip(prb, lab)]
                conf = conf[0] if len(conf) == 1 else torch.cat(conf)
            hw = [tuple(l.shape[-2:]) for l in lab]
            table = pipe.regions(flat, image_hw=hw, conf=conf, min_area=min_area, include_bg=include_bg, want_map=want_map)
            r0 = 0
            for k, (i, c) in enumerate(zip(idx, table["counts_host"].tolist())):
                d = {key: (None if table[key] is None else table[key][r0:r0 + c]) for key in ("root", "label", "area", "bbox", "centroid", "score", "score_q")}
                if want_map:
                    m = table["region_of"][k]
                    d["region_of"] = torch.where(m >= 0, m - r0, m)
                labels[i], regions[i] = lab[k], d
                r0 += c

        if self.slide_crop <= 0:                                             # whole-image inference has no windows to pack: image by image
            for i in range(n):
                if not want_probs:
                    lab = self.predict_many(imgs[i][None], None)[0].contiguous()
                    listed([i], [None], [lab], lab.view(-1))
                    continue
                hw = tuple(imgs[i].shape[-2:])
                ds = data_samples[i] if data_samples is not None else _RegionSample(dict(ori_shape=hw, img_shape=hw, pad_shape=hw, padding_size=[0, 0, 0, 0]))
                self.predict_many(imgs[i][None], [ds])
                lab = ds.pred_sem_seg.data.contiguous()
                listed([i], [ds.seg_logits.data], [lab], lab.view(-1))
        else:
            ori = None if data_samples is None else [tuple(ds.metainfo["ori_shape"][:2]) for ds in data_samples]
            for idx, prb, lab, flat in pipe.label_groups(imgs, self.slide_stride, self.slide_crop, want_probs=want_probs, ori_shapes=ori):
                listed(idx, prb, lab, flat)
                if data_samples is not None:
                    for k, i in enumerate(idx):
                        self._fill_sample(data_samples[i], prb[k], lab[k], i)
        if data_samples is not None:
            for ds, d in zip(data_samples, regions):
                ds.set_data({"pred_regions": d})
        return labels, regions

    @torch.no_grad()
    def predict_topk(self, inputs, k, data_samples=None):
        """The ``k`` best classes of every pixel with their probabilities (1 <= k <= min(8, classes)).  inputs: as ``predict_many``.
        Returns one (classes int32 [k,H,W], probs f32 [k,H,W]) per image, slots in descending class probability (equal values by
        ascending class); with data samples each receives ``seg_topk_classes``, ``seg_topk_probs`` and ``pred_sem_seg`` (plane 0 with
        ``prob_thd`` -> ``bg_idx`` applied, int64 [1,H,W]) and no ``seg_logits``, and the samples are returned.
        Sliding-window inference at the images' own sizes without PAMR runs the fused head (sg_topk_head_multi, one launch per flush
        group): neither the [Q,H,W] canvas nor the [K,H,W] probabilities exist, and a class that owns no query is never listed.  With
        PAMR on, an ``ori_shape`` of another size, or whole-image inference (``slide_crop <= 0``) the canvas route of ``predict`` runs
        (stitch, resize, PAMR, post-process) and ``ops.topk_from_probs`` sorts its probabilities -- except that with
        ``resize_head="fused"`` and no PAMR another ``ori_shape`` runs sg_topk_head_resized_multi, one launch per flush group and no
        canvas.  ``tile_group`` sharding is refused."""
        from .pipeline import AREA_TOPK, SIEVE_TOPK, TOPK_TILE_GROUP, TTA_TOPK
        if getattr(self, "tile_group", None) is not None:
            raise ValueError(TOPK_TILE_GROUP)
        if getattr(self, "tta_scales", None) is not None or getattr(self, "tta_flip", False):
            raise ValueError(TTA_TOPK)
        if getattr(self, "area_thd", None) is not None:
            raise ValueError(AREA_TOPK)
        if getattr(self, "min_region", None) is not None:
            raise ValueError(SIEVE_TOPK)
        batch = torch.is_tensor(inputs)
        imgs = inputs.float() if batch else [x[0].float() if x.dim() == 4 else x.float() for x in inputs]
        n = imgs.shape[0] if batch else len(imgs)
        if data_samples is not None and len(data_samples) != n:
            raise ValueError(f"predict_topk: {n} images but {len(data_samples)} data samples")
        pipe = self._pipeline()
        k = pipe.topk_k(k)
        ori = None if data_samples is None else [tuple(ds.metainfo["ori_shape"][:2]) for ds in data_samples]
        if self.slide_crop <= 0:                             # whole-image inference: the logits exist at the output size anyway
            out = []
            for i in range(n):
                size = tuple(imgs[i].shape[-2:]) if ori is None else ori[i]
                out.append(pipe.topk_from_logits(pipe.forward_feature(imgs[i][None], size)[0], k, guide=imgs[i]))
        else:
            out = pipe.segment_scenes(imgs, self.slide_stride, self.slide_crop, ori_shapes=ori, topk=k)
        if data_samples is None:
            return out
        for ds, (cls, prb) in zip(data_samples, out):
            seg_pred = torch.where(prb[0] < self.prob_thd, torch.full_like(cls[0], int(self.bg_idx)), cls[0]).to(torch.int64).unsqueeze(0)
            ds.set_data({"seg_topk_classes": PixelData(**{"data": cls}), "seg_topk_probs": PixelData(**{"data": prb}),
                         "pred_sem_seg": PixelData(**{"data": seg_pred})})
        return data_samples

    def _fill_sample(self, sample, probs, seg_pred, i):
        """What postprocess_result leaves in a data sample: seg_logits, pred_sem_seg and the result_dir / heatmap_dir images."""
        sample.set_data({"seg_logits": PixelData(**{"data": probs}), "pred_sem_seg": PixelData(**{"data": seg_pred})})
        if getattr(self, "result_dir", None) or getattr(self, "heatmap_dir", None):        # segmentor.py:501-531
            self._write_maps(probs, seg_pred, sample, i)

    @torch.no_grad()
    def evaluate(self, inputs, gt_maps, metric=None, reduce_zero_label=False, ignore_index=255, iou_metrics=("mIoU",), at_gt_size=False,
                 boundary_ratio=None, boundary_px=None, relaxed_px=None, relaxed_ratio=None, relaxed_mode="region", object_iou=None,
                 object_min_area=1, object_include_bg=False):
        """Labels to score without leaving the device: what the reference's ``test_evaluator = dict(type='IoUMetric', ...)`` reports.
        inputs: as ``predict_many``; gt_maps: one [H,W] / [1,H,W] uint8 or int64 tensor or numpy array per image, of the image's size.
        Returns ``(metric.compute(), metric)``; pass ``metric`` back in to accumulate over the calls of a dataset loop (its own
        ignore_index / reduce_zero_label / iou_metrics then hold).  The packed labels-only path produces the labels (no probabilities
        are written), the ground truth goes to the device once per call, the counts are taken with ONE sg_confusion_accumulate launch
        per flush group over its flat label buffer, and only the (K+1) x (K+1) table comes back.  Whole-image inference
        (``slide_crop <= 0``) goes image by image through ``predict``.  ``tile_group`` sharding is refused here (counting each rank's
        band against the matching rows of the truth is not built yet: DESIGN.md section 8); score per rank over whole images and call
        ``metric.reduce(group)``.  With PAMR on (``pamr_steps > 0``) the labels come from the refined canvases (SegPipeline.label_groups).
        ``at_gt_size``: a truth map of any size is accepted; its shape becomes that image's ``ori_shape`` and the labels are produced at
        that size and counted (the configs that resize the image before inference and score at the original size).  The route follows
        ``resize_head``: sg_label_head_resized_multi with "fused", stitch + resize + post-process with "canvas".
        With ``area_thd`` set the labels that are counted are the filtered ones (SegPipeline.label_groups); with ``min_region`` set,
        the sieved ones.
        ``boundary_ratio`` / ``boundary_px``: Boundary IoU next to the plain metric.  With both None and ``metric`` None or a plain
        ``IoUMetric``, nothing above changes.  With one of them set, or with a ``BoundaryIoUMetric`` passed in, the metric is a
        ``BoundaryIoUMetric``: built here with the band width ``boundary_ratio`` of each image's diagonal or the fixed ``boundary_px``,
        or the one passed in, whose own ratio / width hold.  Every flush group's flat labels then go to ``metric.add_flat`` with the
        sizes of its images, which adds one sg_boundary_accumulate call per group, and the result carries ``BIoU`` and
        ``summary['mBIoU']``.  It reads final labels only, so it composes with ``at_gt_size``, ``area_thd``, ``min_region``, PAMR,
        ``blend`` and TTA.
        ``relaxed_px`` / ``relaxed_ratio`` / ``relaxed_mode``: relaxed precision / recall / F (``relaxed_mode`` "region", the road
        score) or the boundary F-score ("contour") next to the plain metric (the definition: sg_tolerant_accumulate in
        include/segearth_hip.h).  With both None and no ``RelaxedMetric`` passed in, nothing above changes.  With one of them set a
        ``RelaxedMetric`` is built here with the fixed tolerance ``relaxed_px`` or ``relaxed_ratio`` of each image's diagonal; one that
        is passed in keeps its own settings.  It is fed by ``add_flat`` per flush group exactly where the boundary metric is fed, which
        adds one sg_tolerant_accumulate call per group, and composes in the same way.  ``relaxed_*`` together with ``boundary_*``,
        or a passed metric of the other kind, is refused: one metric object with both tables is not built.
        ``object_iou`` / ``object_min_area`` / ``object_include_bg``: object-level precision / recall / F1 and panoptic quality next to
        the plain metric (the definition: sg_object_match in include/segearth_hip.h).  With ``object_iou`` None and no ``ObjectMetric``
        passed in, nothing above changes.  With it set (a float or a ``(num, den)`` pair in [1/2, 1)) an ``ObjectMetric`` is built here:
        regions connected under ``region_connectivity``, of at least ``object_min_area`` pixels and, unless ``object_include_bg``, not
        of the class ``bg_idx``; one that is passed in keeps its own settings.  It is fed by ``add_flat`` per flush group where the other
        two are, which adds one sg_object_match call per group; it reads final labels only and composes in the same way.  ``object_*``
        together with ``boundary_*`` or ``relaxed_*``, or a passed metric of another kind, is refused."""
        from .metrics import BoundaryIoUMetric, IoUMetric, ObjectMetric, RelaxedMetric, _ImageShapeMetric
        # the kinds of metric with a second table: the class, whether its keyword arguments were given, their words in the refusals,
        # and what the class is built with next to IoUMetric's arguments.  A kind is wanted by its arguments or by a metric of its class.
        kinds = ((ObjectMetric, object_iou is not None, "object_*", "object_iou needs an",
                  dict(object_iou=object_iou, min_area=object_min_area, connectivity=getattr(self, "region_connectivity", 4),
                       skip_label=None if object_include_bg else int(self.bg_idx))),
                 (RelaxedMetric, relaxed_px is not None or relaxed_ratio is not None, "relaxed_*", "relaxed_px / relaxed_ratio need a",
                  dict(mode=relaxed_mode, tolerance_px=relaxed_px, **({} if relaxed_ratio is None else {"tolerance_ratio": relaxed_ratio}))),
                 (BoundaryIoUMetric, boundary_ratio is not None or boundary_px is not None, "boundary_*", "boundary_ratio / boundary_px need a",
                  dict(boundary_px=boundary_px, **({} if boundary_ratio is None else {"boundary_ratio": boundary_ratio}))))
        wanted = [k for k in kinds if k[1] or isinstance(metric, k[0])]
        if getattr(self, "tile_group", None) is not None:
            raise ValueError("evaluate: tile_group sharding is not supported (each rank would have to count its own band against the "
                             "matching rows of the truth); evaluate whole images per rank and call metric.reduce(group)")
        if len(wanted) > 1:
            raise ValueError(f"evaluate: {' together with '.join(k[2] for k in wanted)} (or a metric of another kind) in one call is not "
                             "supported: one metric object with several tables is not built; evaluate twice")
        cls, _, _, needs, own = wanted[0] if wanted else (IoUMetric, False, "", "", {})
        if wanted and metric is not None and not isinstance(metric, cls):
            raise TypeError(f"evaluate: {needs} {cls.__name__} (or metric=None to have one built), got {type(metric).__name__}")
        if metric is None:
            metric = cls(ignore_index=ignore_index, iou_metrics=list(iou_metrics), num_classes=self.num_classes,
                         reduce_zero_label=reduce_zero_label, **own)
        elif metric.num_classes is None:
            metric.num_classes = self.num_classes
        elif metric.num_classes != self.num_classes:
            raise ValueError(f"evaluate: the metric counts {metric.num_classes} classes, the class file has {self.num_classes}")
        batch = torch.is_tensor(inputs)
        imgs = inputs.float() if batch else [x[0].float() if x.dim() == 4 else x.float() for x in inputs]
        n = imgs.shape[0] if batch else len(imgs)
        if len(gt_maps) != n:
            raise ValueError(f"evaluate: {n} images but {len(gt_maps)} ground-truth maps")
        dev = self.query_features.device
        gts = [torch.as_tensor(g) for g in gt_maps]
        ori = None
        if at_gt_size:
            if any(g.dim() not in (2, 3) or (g.dim() == 3 and g.shape[0] != 1) or g.numel() == 0 for g in gts):
                raise ValueError("evaluate: a ground-truth map must be a non-empty [H,W] or [1,H,W]")
            ori = [tuple(int(v) for v in g.shape[-2:]) for g in gts]
            if all(o == tuple(imgs[i].shape[-2:]) for i, o in enumerate(ori)):
                ori = None                                                   # nothing to resize: today's routes
        for i, g in enumerate(gts):
            hw = tuple(imgs[i].shape[-2:])
            if not at_gt_size and tuple(g.shape) not in (hw, (1,) + hw):
                raise ValueError(f"evaluate: ground truth {i} has shape {tuple(g.shape)}, image {i} is {hw}")
        dtype = torch.uint8 if all(g.dtype == torch.uint8 for g in gts) else torch.int64
        off = [0]
        for g in gts:
            off.append(off[-1] + g.numel())
        if all(not g.is_cuda for g in gts):                                  # one host buffer, one copy to the device per call
            gt_flat = torch.cat([g.reshape(-1).to(dtype) for g in gts]).to(dev)
        else:
            gt_flat = torch.cat([g.reshape(-1).to(device=dev, dtype=dtype) for g in gts])

        def feed(flat, gt, maps):                                            # a metric with a second table needs the sizes of the images
            if isinstance(metric, _ImageShapeMetric):
                metric.add_flat(flat, gt, [tuple(x.shape[-2:]) for x in maps])
            else:
                metric.add(flat, gt)

        if self.slide_crop <= 0:                                            # whole-image inference has no windows to pack
            labs = self.predict_many(imgs, None, ori_shapes=ori) if at_gt_size else [self.predict(imgs[i][None], None) for i in range(n)]
            for i in range(n):
                feed(labs[i].reshape(-1), gt_flat[off[i]:off[i + 1]], [labs[i]])
            return metric.compute(), metric
        for idx, _, labs, flat in self._pipeline().label_groups(imgs, self.slide_stride, self.slide_crop, want_probs=False, ori_shapes=ori):
            if idx == list(range(idx[0], idx[0] + len(idx))):                # the group's images are neighbours in the call: a slice
                gt = gt_flat[off[idx[0]]:off[idx[-1] + 1]]
            else:                                                            # tile-size groups interleave images: gather on the device
                gt = torch.cat([gt_flat[off[k]:off[k + 1]] for k in idx])
            feed(flat, gt, labs)
        return metric.compute(), metric

    def postprocess_result(self, seg_logits, data_samples):
        """Reference segmentor.py:475-499: class probabilities [K,H,W] + labels [1,H,W] per image."""
        pipe = self._pipeline()
        batch_size = seg_logits.shape[0]
        for i in range(batch_size):
            probs, seg_pred = pipe.postprocess(seg_logits[i].float())
            seg_pred = pipe.sieve(seg_pred)                                  # min_region: the last step on the labels; seg_logits stay
            if data_samples is None:
                return seg_pred
            self._fill_sample(data_samples[i], probs, seg_pred, i)
        return data_samples

    def _generate_palette(self, n):
        """Reference segmentor.py:568-578: deterministic HSV palette, the background class dimmed."""
        import colorsys
        palette = []
        for idx in range(n):
            r, g, b = colorsys.hsv_to_rgb((idx / max(1, n)) % 1.0, 0.75, 1.0 if idx != self.bg_idx else 0.2)
            palette.append([int(r * 255), int(g * 255), int(b * 255)])
        return np.array(palette, dtype=np.uint8)

    def _write_maps(self, probs, seg_pred, sample, i):
        """Colour mask -> result_dir/<stem>.png, confidence map -> heatmap_dir/<stem>.png.  The images are rendered on the device
        (sg_render_maps); only the PNG encoding is host work.  Without OpenCV the reference's own fall-back colour ramp is used."""
        from . import ops
        from PIL import Image
        meta = sample.metainfo if hasattr(sample, "metainfo") else {}
        stem = None
        for key in ("img_path", "ori_path", "filename", "ori_filename"):
            if key in meta and meta[key]:
                stem = os.path.splitext(os.path.basename(meta[key]))[0]
                break
        if stem is None:
            stem = f"sample_{i}"
        palette = getattr(self, "_palette_cache", None)
        if palette is None or len(palette) < self.num_classes:
            palette = self._palette_cache = self._generate_palette(self.num_classes)
        mask, heat = ops.render_maps(seg_pred, probs, torch.from_numpy(palette), want_mask=bool(self.result_dir), want_heat=bool(self.heatmap_dir))
        if self.result_dir:
            os.makedirs(self.result_dir, exist_ok=True)
            Image.fromarray(mask.cpu().numpy()).save(os.path.join(self.result_dir, f"{stem}.png"))
        if self.heatmap_dir:
            os.makedirs(self.heatmap_dir, exist_ok=True)
            Image.fromarray(heat.cpu().numpy()).save(os.path.join(self.heatmap_dir, f"{stem}.png"))

    def compute_padsize(self, H: int, W: int, patch_size: int):
        return compute_padsize(H, W, patch_size)

    # mmseg abstract hooks the reference leaves empty (segmentor.py:548-566)
    def _forward(self, data_samples=None):
        """ """

    def inference(self, img, batch_img_metas):
        """ """

    def encode_decode(self, inputs, batch_img_metas):
        """ """

    def extract_feat(self, inputs):
        """ """

    def loss(self, inputs, data_samples):
        """ """


class SegmentorEx(_HipSegmentorBase):
    """Drop-in of reference ``segmentor.SegmentorEx`` (constructor kwargs of segmentor.py:33-63)."""

    def __init__(self, clip_type, vit_type, model_type, name_path, device=torch.device("cuda"), ignore_residual=True, prob_thd=0.0,
                 logit_scale=50, slide_stride=112, slide_crop=224, cls_token_lambda=0.0, global_debias_factor=0.0, bg_idx=0,
                 apply_sim_feat_up=False, sim_feat_up_cfg=dict(model_name="jbu_one", model_path="your/model/path"),
                 apply_ctd=False, apply_outlier_suppression=False, outlier_suppression_cfg=None,
                 apply_self_attn_enhancement=False, self_attn_enhancement_cfg=None, apply_layer_fusion=False,
                 layer_fusion_lambda=0.5, layer_fusion_threshold=0.7, apply_similarity_enhancement=False,
                 similarity_enhancement_cfg=None, result_dir=None, heatmap_dir=None,
                 # -- drop-in extras (see module docstring) --
                 checkpoint=None, text_features=None, text_encoder=None, precision="f16x2", synthetic_ok=False, tiles_per_launch=None,
                 tokenizer=None, cross_tile_fusion_cfg=None, tile_group=None, pack_images=False, label_head="auto", prob_head="auto",
                 pamr_steps=0, pamr_stride=(8, 16), resize_head="canvas", area_thd=None, min_region=None, region_connectivity=4,
                 region_fill="neighbour", blend="uniform", blend_ramp=None, tta_scales=None, tta_flip=False, tta_head="auto"):
        data_preprocessor = SegDataPreProcessor(mean=list(Wt.PIXEL_MEAN), std=list(Wt.PIXEL_STD), bgr_to_rgb=True)
        super().__init__(data_preprocessor=data_preprocessor)
        if model_type == "GEM":
            raise ValueError("model_type='GEM' crashes in the reference SegmentorEx (it unpacks (cls, feats), SURVEY.md R5); "
                             "use segearth_segmentor.Segmentor with cls_token_lambda=0")
        visual = self._setup(clip_type, vit_type, model_type, name_path, device, ignore_residual, prob_thd, logit_scale, slide_stride,
                             slide_crop, cls_token_lambda, bg_idx, _to_bool(apply_sim_feat_up), sim_feat_up_cfg, global_debias_factor,
                             checkpoint, text_features, text_encoder, precision, synthetic_ok, tiles_per_launch, tokenizer=tokenizer,
                             tile_group=tile_group, label_head=label_head, prob_head=prob_head, pamr_steps=pamr_steps, pamr_stride=pamr_stride,
                             resize_head=resize_head, area_thd=area_thd, min_region=min_region, region_connectivity=region_connectivity,
                             region_fill=region_fill, blend=blend, blend_ramp=blend_ramp, tta_scales=tta_scales, tta_flip=tta_flip,
                             tta_head=tta_head)
        # opt-in extra: kwargs of the reference's CrossTileFusion (cross_tile_fusion.py:24-60), which the reference never calls (R2)
        self.cross_tile_fusion_cfg = cross_tile_fusion_cfg
        self.apply_ctd = _to_bool(apply_ctd)                                # segmentor.py:184-194, 339-365: DBSCAN + cluster debias, on the device here
        # attention-map layer fusion (segmentor.py:189-193, 302-304): the reference's own code only runs it with one head;
        # built here with the semantics that case pins (oracle/vit.py).  layer_fusion_threshold is unused by the reference.
        self.apply_layer_fusion, self.layer_fusion_lambda, self.layer_fusion_threshold = _to_bool(apply_layer_fusion), layer_fusion_lambda, layer_fusion_threshold
        self.apply_similarity_enhancement = _to_bool(apply_similarity_enhancement)
        if self.apply_similarity_enhancement:                               # segmentor.py:196-220
            c = dict(similarity_weight=1.0, temperature=1.0, add_self_similarity=True)
            c.update(similarity_enhancement_cfg or {})
            visual.similarity_enhancer = SimilarityEnhancementModule(**c)
        self.apply_self_attn_enhancement = _to_bool(apply_self_attn_enhancement)
        if self.apply_self_attn_enhancement:                                # segmentor.py:222-249
            c = dict(enhancement_strength=0.1, min_self_attn_threshold=0.15, mode="feature")
            c.update(self_attn_enhancement_cfg or {})
            visual.self_attn_enhancer = SelfAttentionEnhancementModule(**c)
        self.apply_outlier_suppression = _to_bool(apply_outlier_suppression)
        if self.apply_outlier_suppression:                                  # segmentor.py:251-274
            c = dict(top_k=10)
            c.update(outlier_suppression_cfg or {})
            visual.outlier_suppressor = OutlierSuppressionModule(top_k=c["top_k"])
        self.result_dir, self.heatmap_dir = result_dir, heatmap_dir
        self.pack_images = _to_bool(pack_images)                          # predict / forward_slide with B > 1 on the packed path


class Segmentor(_HipSegmentorBase):
    """Drop-in of reference ``segearth_segmentor.Segmentor`` (segearth_segmentor.py:23-41): no refiners, no global
    debias; the CLS token is only requested when ``cls_token_lambda != 0``; GEM runs here."""

    def __init__(self, clip_type, vit_type, model_type, name_path, device=torch.device("cuda"), ignore_residual=True, prob_thd=0.0,
                 logit_scale=50, slide_stride=112, slide_crop=224, cls_token_lambda=0, bg_idx=0, apply_sim_feat_up=True,
                 sim_feat_up_cfg=dict(model_name="jbu_one", model_path="your/model/path"),
                 checkpoint=None, text_features=None, text_encoder=None, precision="f16x2", synthetic_ok=False, tiles_per_launch=None,
                 tokenizer=None, cross_tile_fusion_cfg=None, tile_group=None, apply_outlier_suppression=False, outlier_suppression_cfg=None,
                 pack_images=False, label_head="auto", prob_head="auto", pamr_steps=0, pamr_stride=(8, 16), resize_head="canvas",
                 area_thd=None, min_region=None, region_connectivity=4, region_fill="neighbour", blend="uniform", blend_ramp=None,
                 tta_scales=None, tta_flip=False, tta_head="auto"):
        data_preprocessor = SegDataPreProcessor(mean=list(Wt.PIXEL_MEAN), std=list(Wt.PIXEL_STD), bgr_to_rgb=True)
        super().__init__(data_preprocessor=data_preprocessor)
        if model_type == "GEM" and cls_token_lambda != 0:
            raise ValueError("GEM returns no CLS token (gem_utils.py:198-199): cls_token_lambda must be 0 (SURVEY.md R5)")
        self._setup(clip_type, vit_type, model_type, name_path, device, ignore_residual, prob_thd, logit_scale, slide_stride,
                    slide_crop, cls_token_lambda, bg_idx, apply_sim_feat_up, sim_feat_up_cfg, 0.0,
                    checkpoint, text_features, text_encoder, precision, synthetic_ok, tiles_per_launch, tokenizer=tokenizer,
                    tile_group=tile_group, label_head=label_head, prob_head=prob_head, pamr_steps=pamr_steps, pamr_stride=pamr_stride,
                             resize_head=resize_head, area_thd=area_thd, min_region=min_region, region_connectivity=region_connectivity,
                             region_fill=region_fill, blend=blend, blend_ramp=blend_ramp, tta_scales=tta_scales, tta_flip=tta_flip,
                             tta_head=tta_head)
        # opt-in extra: kwargs of the reference's CrossTileFusion (cross_tile_fusion.py:24-60), which the reference never calls (R2)
        self.cross_tile_fusion_cfg = cross_tile_fusion_cfg
        self.output_cls_token = cls_token_lambda != 0
        self.pack_images = _to_bool(pack_images)                          # predict / forward_slide with B > 1 on the packed path
        self.apply_similarity_enhancement = False
        # opt-in extra (BASELINE configs[2]: "GEM self-self attn + outlier_suppression" in ONE forward).  The reference cannot run that
        # composition (SegmentorEx crashes on GEM and this class has no refiners); the definition built here -- detection on the
        # ordinary stream's attention of block L-2, suppression on the GEM stream before ln_post -- is written down in DESIGN.md section 7 and
        # restated in oracle/vit.py::gem_forward.  Same kwargs as SegmentorEx (segmentor.py:251-274).
        self.apply_outlier_suppression = _to_bool(apply_outlier_suppression)
        if self.apply_outlier_suppression:
            c = dict(top_k=10)
            c.update(outlier_suppression_cfg or {})
            self.net.visual.outlier_suppressor = OutlierSuppressionModule(top_k=c["top_k"])
