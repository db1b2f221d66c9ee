"""Host side of the SimFeatUp upsamplers: owns an ``sg_jbu`` context (reference
simfeatup_dev/upsamplers.py: ``get_upsampler('jbu_one' | 'jbu_stack' | 'bilinear', dim)`` + ``load_state_dict``) and produces
per-pixel class logits for a batch of tiles.  Arithmetic happens in libsegearth_hip.so."""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, ops, weights as Wt
from ._lib import TileBatch, check
from .ops import precision_id, ptr, stream_ptr

KINDS = {"jbu_one": 0, "jbu_stack": 1, "bilinear": 2, "resize_conv": 3}

# why the reference's other upsamplers (upsamplers.py:353-369) are refused
REFUSED = {
    "ifa": "its output is 2x the patch grid per side, so the reference's own view(1, C, image_w * image_h) at segmentor.py:372 fails for it",
    "carafe": "it needs mmcv's native CARAFE op, which the reference does not ship",
    "sapa": "it needs the sapa package's native ops, which the reference does not ship",
}


def get_upsampler(upsampler: str, dim: int, device="cuda:0", precision="f32") -> "HipJBU":
    """Same factory name as the reference (upsamplers.py:353-369): 'jbu_one', 'jbu_stack', 'bilinear' and 'resize_conv' ride the HIP path."""
    if upsampler in REFUSED:
        raise ValueError(f"upsampler {upsampler!r} is not supported: {REFUSED[upsampler]}")
    if upsampler not in KINDS:
        raise ValueError(f"Unknown upsampler {upsampler}")
    return HipJBU(upsampler, dim, device, precision)


class HipJBU:
    def __init__(self, model_name: str, feat_dim: int, device="cuda:0", precision="f32"):
        if model_name not in KINDS:
            get_upsampler(model_name, feat_dim)                              # raises with the reason
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("HipJBU needs a GPU: the hot path has no CPU implementation")
        self.model_name, self.feat_dim = model_name, feat_dim
        self.device = torch.device(device)
        # the upsampler has a parity (f32) and a throughput (bf16) path: fp8 / f16 towers feed the bf16 one; the exact two-plane f16 tower gets the
        # f32 kernels with their three linears on the two-plane f16 GEMM (f32-grade results, SG_PREC_F16X2)
        pid = precision_id(precision)
        self.precision = pid if pid in (_lib.PREC_F32, _lib.PREC_F16X2) else _lib.PREC_BF16
        self._ctx = C.c_void_p()
        self._ws = {}
        self.tiles_per_launch = 8            # tiles per JBU launch (workspace ~2.2 GB per 512-pixel tile)
        self.fused_tail = True               # bf16 mode: sg_jbu_logits[_wide] (no [S^2, C] feature map); False = upsample + cosine_logits
        # more than 32 queries: True = the fused wide tail (sg_jbu_logits_wide, C <= 1216), False = upsample + cosine_logits there
        self.wide_tail = False
        with torch.cuda.device(self.device):
            check(self.lib.sg_jbu_create(C.byref(self._ctx), self.device.index or 0, KINDS[model_name], feat_dim), "sg_jbu_create")

    def __del__(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is not None and ctx.value:
            self.lib.sg_jbu_destroy(ctx)
            self._ctx = C.c_void_p()

    @property
    def is_bilinear(self) -> bool:
        return self.model_name == "bilinear"

    @property
    def is_resize_conv(self) -> bool:
        return self.model_name == "resize_conv"

    def output_hw(self, grid, padded_hw):
        """Per-pixel logit map size of one tile: JBU upsamples the patch grid 16x whatever the patch size; Bilinear resizes
        to the padded tile itself (upsamplers.py:349)."""
        return tuple(padded_hw) if self.is_bilinear else (16 * grid[0], 16 * grid[1])

    @classmethod
    def from_config(cls, model_name, feat_dim, model_path, device, synthetic_ok=False, precision="f32"):
        up = cls(model_name, feat_dim, device, precision)
        if up.is_bilinear:
            # no parameters: no checkpoint needed; a given one must hold an empty state_dict (the reference's strict load, segmentor.py:283)
            if model_path and os.path.exists(model_path):
                ckpt = torch.load(model_path, map_location="cpu", weights_only=True)["state_dict"]
                if len(ckpt):
                    raise RuntimeError(f"Error(s) in loading state_dict for Bilinear: unexpected key(s) {sorted(ckpt)[:8]} in {model_path!r}")
            return up
        if model_path and os.path.exists(model_path):
            ckpt = torch.load(model_path, map_location="cpu", weights_only=True)["state_dict"]
            up.load_state_dict({k[10:]: v for k, v in ckpt.items()})       # strips 'upsampler.' (segmentor.py:282)
        elif synthetic_ok:
            warnings.warn(f"SimFeatUp: checkpoint {model_path!r} not found, using SYNTHETIC upsampler weights")
            up.load_state_dict(Wt.make_resize_conv_weights(feat_dim, seed=3) if up.is_resize_conv else Wt.make_jbu_weights(model_name, feat_dim, seed=3))
        else:
            raise FileNotFoundError(f"SimFeatUp checkpoint {model_path!r} not found (the configured jbu_one blob is not in the tree)")
        return up

    def load_state_dict(self, state_dict: Dict[str, "np.ndarray | torch.Tensor"], strict: bool = True):
        if self.is_bilinear and len(state_dict):
            raise RuntimeError(f"Error(s) in loading state_dict for Bilinear: unexpected key(s) {sorted(state_dict)[:8]}")
        if self.is_resize_conv and strict:                                  # the reference's strict load (segmentor.py:283)
            want = set(Wt.resize_conv_keys())
            missing, extra = sorted(want - set(state_dict)), sorted(set(state_dict) - want)
            if missing or extra:
                raise RuntimeError(f"Error(s) in loading state_dict for LayeredResizeConv: missing key(s) {missing}, unexpected key(s) {extra}")
        with torch.cuda.device(self.device):
            s = stream_ptr(self.device)
            for name, value in state_dict.items():
                t = torch.as_tensor(value).detach().to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
                check(self.lib.sg_jbu_set_tensor(self._ctx, name.encode(), ptr(t), t.numel(), s), f"sg_jbu_set_tensor({name})")
            torch.cuda.current_stream(self.device).synchronize()

    def _workspace(self, nbytes):
        """One arena per stream (as HipVisionTower._workspace): launches on different streams may overlap and must not share scratch."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes + 256:
            self._ws[key] = None
            ws = self._ws[key] = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        p = ws.data_ptr()
        off = (-p) % 256
        return C.c_void_p(p + off), ws.numel() - off

    def __call__(self, source: torch.Tensor, guidance: torch.Tensor) -> torch.Tensor:
        """Reference call shape: source [B,C,h,w], guidance [B,3,H,W] -> [B,C,16h,16w] (upsamplers.py:278-325; Bilinear: [B,C,H,W])."""
        B, Cc, h, w = source.shape
        tok = source.permute(0, 2, 3, 1).reshape(B, h * w, Cc)
        out = self.upsample_tokens(tok, guidance, h, w)
        oh, ow = self.output_hw((h, w), guidance.shape[-2:])
        return out.reshape(B, oh, ow, Cc).permute(0, 3, 1, 2)

    def upsample_tokens(self, tokens: torch.Tensor, guidance: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
        """tokens [B, gh*gw, C] pixel-major, guidance [B,3,GH,GW] -> [B, 16gh*16gw, C] (Bilinear: [B, GH*GW, C])."""
        tokens = tokens.contiguous().float()
        guidance = guidance.contiguous().float()
        B, n, Cc = tokens.shape
        assert n == gh * gw and Cc == self.feat_dim
        oh, ow = self.output_hw((gh, gw), guidance.shape[-2:])
        with torch.cuda.device(self.device):
            out = torch.empty(B, oh * ow, Cc, dtype=torch.float32, device=self.device)
            need = self.lib.sg_jbu_workspace_bytes(self._ctx, B, gh, gw)
            wp, wn = self._workspace(need)
            check(self.lib.sg_jbu_upsample(self._ctx, ptr(tokens), ptr(guidance), B, gh, gw, guidance.shape[-2], guidance.shape[-1],
                                           self.precision, ptr(out), wp, wn, stream_ptr(self.device)), "sg_jbu_upsample")
        return out

    def logits(self, tokens, cls, scene, windows, tile_hw, pad_lt, grid, text, global_debias_factor, cls_token_lambda, scene_index=None,
               padded_hw=None):
        """Per-pixel logits [T, Q, 16gh, 16gw] (Bilinear: [T, Q, ph, pw]) for the tiles of one launch: global debias -> JBU -> cosine logits
        (reference order, segmentor.py:317-379; the reference runs B=1, :369-372).  ``tiles_per_launch`` tiles go through the
        upsampler per launch -- no per-tile host loop; the chunk bounds the workspace (C x S^2 f32 = 0.5 GB per 512-pixel tile)."""
        T = tokens.shape[0]
        gh, gw = grid
        th, tw = tile_hw
        l, t = pad_lt
        # the guidance is the normalised, zero-padded tile; JBU upsamples 16x regardless of the ViT's patch size
        ph, pw = padded_hw if padded_hw is not None else (th + 2 * t, tw + 2 * l)
        fmt = _lib.IMG_U8_NHWC if scene.dtype == torch.uint8 else _lib.IMG_F32_NCHW
        scene = scene.contiguous()
        H, W = (scene.shape[-3], scene.shape[-2]) if fmt == _lib.IMG_U8_NHWC else (scene.shape[-2], scene.shape[-1])
        text = text.contiguous()
        Q = text.shape[0]
        with torch.cuda.device(self.device):
            if cls is not None and global_debias_factor != 0:
                tokens = ops.global_debias(tokens, cls, float(global_debias_factor))
            outs = []
            windows = windows.to(device=self.device, dtype=torch.int32).contiguous()
            if scene_index is not None:
                scene_index = scene_index.to(device=self.device, dtype=torch.int32).contiguous()
            step = max(1, int(self.tiles_per_launch))
            for i in range(0, T, step):
                c = min(step, T - i)
                tb = TileBatch()
                tb.scene, tb.format, tb.scene_h, tb.scene_w = scene.data_ptr(), fmt, H, W
                wi = windows[i:i + c].contiguous()
                tb.windows = wi.data_ptr()
                if scene_index is not None:
                    si = scene_index[i:i + c].contiguous()
                    tb.scene_index = si.data_ptr()
                    tb.scene_stride = 3 * H * W
                tb.n_tiles, tb.tile_h, tb.tile_w, tb.pad_l, tb.pad_t, tb.grid_h, tb.grid_w = c, th, tw, l, t, gh, gw
                guid = torch.empty(c, 3, ph, pw, dtype=torch.float32, device=self.device)
                check(self.lib.sg_extract_tiles(C.byref(tb), ph, pw, ptr(guid), stream_ptr(self.device)), "sg_extract_tiles")
                lam = float(cls_token_lambda) if cls is not None else 0.0
                if self.is_bilinear:
                    # every precision: the per-pixel logits come from per-token products and Gram terms, no [GH*GW, C] map (f32 arithmetic)
                    # (any Q in one call: the library walks the queries in chunks of 32, the kernels' bound, and writes them in place)
                    lg = torch.empty(c, Q, ph * pw, dtype=torch.float32, device=self.device)
                    tk = tokens[i:i + c].contiguous().float()
                    ci = None if (cls is None or lam == 0.0) else cls[i:i + c].contiguous().float()
                    need = self.lib.sg_jbu_workspace_bytes_wide(self._ctx, c, gh, gw, Q)
                    wp, wn = self._workspace(need)
                    check(self.lib.sg_jbu_logits_wide(self._ctx, ptr(tk), ptr(guid), c, gh, gw, ph, pw, self.precision, ptr(text), Q,
                                                      ptr(ci), lam, ptr(lg), wp, wn, stream_ptr(self.device)), "sg_jbu_logits_wide")
                elif self.fused_tail and not self.is_resize_conv and self.precision == _lib.PREC_BF16 and self.feat_dim % 64 == 0 and self.feat_dim >= 512 and (Q <= 32 or (self.wide_tail and self.feat_dim <= 1216)):
                    # throughput mode: JBU + L2-norm + x T^T in one call; the [S^2, C] feature map never reaches HBM (more than 32 queries:
                    # the wide matrix-pipe tail, whose two resident query groups need C <= 1216; up to 32 the wide entry is sg_jbu_logits itself)
                    lg = torch.empty(c, Q, 256 * gh * gw, dtype=torch.float32, device=self.device)
                    tk = tokens[i:i + c].contiguous().float()
                    ci = None if (cls is None or lam == 0.0) else cls[i:i + c].contiguous().float()
                    need = self.lib.sg_jbu_workspace_bytes_wide(self._ctx, c, gh, gw, Q)
                    wp, wn = self._workspace(need)
                    check(self.lib.sg_jbu_logits_wide(self._ctx, ptr(tk), ptr(guid), c, gh, gw, ph, pw, self.precision, ptr(text), Q, ptr(ci), lam,
                                                      ptr(lg), wp, wn, stream_ptr(self.device)), "sg_jbu_logits_wide")
                else:
                    feats = self.upsample_tokens(tokens[i:i + c], guid, gh, gw)                      # [c, 256 n, C]
                    lg = ops.cosine_logits(feats, None if cls is None else cls[i:i + c], text, 0.0, lam, two_plane=self.precision == _lib.PREC_F16X2)
                outs.append(lg.reshape(c, Q, *self.output_hw((gh, gw), (ph, pw))))
        return torch.cat(outs, 0) if len(outs) > 1 else outs[0]
