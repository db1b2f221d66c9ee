"""Thin torch-tensor wrappers over the C ABI (one Python function per exported op).

PyTorch is plumbing here: it owns device memory and the stream; every computation happens in
libsegearth_hip.so.  Nothing in this module falls back to torch arithmetic.  (``topk_from_probs`` is a torch
sort by design: it turns the [K,H,W] probabilities of the canvas route into the top-k head's outputs on the routes
where the fused head cannot run; it replaces no kernel.)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import PREC_BF16, PREC_F16, PREC_F16X2, PREC_F32, PREC_FP8, MODEL_TYPES, check


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libsegearth_hip ops need device tensors (no CPU fallback exists)")


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """The caller's current stream ON ``device`` (default: the current device)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_tensor_device(fn):
    """Run an op on the device its first GPU tensor argument lives on: the context-free entry points launch on the CURRENT
    device, so a tensor on cuda:1 in a process whose current device is cuda:0 must switch first (stream_ptr() then picks that
    device's current stream)."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if torch.is_tensor(a) and a.is_cuda:
                with torch.cuda.device(a.device):
                    return fn(*args, **kwargs)
        return fn(*args, **kwargs)
    return wrapper


def precision_id(precision) -> int:
    if precision in (PREC_F32, "f32", "fp32", torch.float32):
        return PREC_F32
    if precision in (PREC_BF16, "bf16", torch.bfloat16):
        return PREC_BF16
    if precision in (PREC_FP8, "fp8"):
        return PREC_FP8
    if precision in (PREC_F16, "f16", "fp16", "half", torch.float16):
        return PREC_F16
    if precision in (PREC_F16X2, "f16x2", "exact"):       # two-plane f16: f32-grade results on the f16 matrix pipe (include/segearth_hip.h)
        return PREC_F16X2
    raise ValueError(f"unknown precision {precision!r}")


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().float()


def scratch(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256) + 256, dtype=torch.uint8, device=device)


def _aligned(buf: torch.Tensor) -> Tuple[C.c_void_p, int]:
    p = buf.data_ptr()
    off = (-p) % 256
    return C.c_void_p(p + off), buf.numel() - off


@on_tensor_device
def linear(A, W, bias=None, residual=None, act: int = 0, precision="bf16"):
    """act(A @ W^T + bias) (+ residual); act 0 none / 1 QuickGELU / 2 erf-GELU."""
    lib = _lib.load()
    A, W = _f32(A), _f32(W)
    _require_gpu(A, W, bias, residual)
    M, K = A.shape
    N = W.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    Kp = (K + 63) // 64 * 64
    buf = scratch((M + N) * Kp * 4 + 1024, A.device)      # 4 bytes per element covers every operand form (two-plane f16 included)
    sp, sn = _aligned(buf)
    bias = None if bias is None else _f32(bias)
    residual = None if residual is None else _f32(residual)
    check(lib.sg_op_linear(ptr(A), ptr(W), ptr(bias), ptr(residual), ptr(out), M, N, K, act, precision_id(precision), sp, sn,
                           stream_ptr()), "sg_op_linear")
    return out


@on_tensor_device
def quantize_rows_fp8(x):
    """f32 [rows, D] -> (uint8 e4m3 [rows, D], f32 scales [rows]); scale = max|row| / 448."""
    lib = _lib.load()
    x = _f32(x)
    _require_gpu(x)
    rows, D = x.shape
    q = torch.empty(rows, D, dtype=torch.uint8, device=x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib.sg_quantize_rows_fp8(ptr(x), rows, D, ptr(q), ptr(sc), stream_ptr()), "sg_quantize_rows_fp8")
    return q, sc


@on_tensor_device
def ln_chain(A, W1, b1, x, gamma, beta, W2, b2, act: int = 0, precision="bf16", fold: bool = True):
    """x_new = x + A @ W1^T + b1;  y = act(LayerNorm(x_new) @ W2^T + b2): the residual GEMM -> LayerNorm -> GEMM chain of a block, with the
    LayerNorm folded into the two GEMMs (fold) or as its own pass.  Returns (x_new, y), both f32."""
    lib = _lib.load()
    A, W1, b1, gamma, beta, W2, b2 = (_f32(t) for t in (A, W1, b1, gamma, beta, W2, b2))
    x = _f32(x).clone()
    M, K1 = A.shape
    D, N2 = W1.shape[0], W2.shape[0]
    y = torch.empty(M, N2, dtype=torch.float32, device=A.device)
    nbytes = lib.sg_op_ln_chain_scratch_bytes(M, K1, D, N2)
    buf = scratch(nbytes, A.device)
    sp, sn = _aligned(buf)
    check(lib.sg_op_ln_chain(ptr(A), ptr(W1), ptr(b1), ptr(x), ptr(gamma), ptr(beta), ptr(W2), ptr(b2), ptr(y), M, K1, D, N2, act,
                             precision_id(precision), int(fold), sp, sn, stream_ptr()), "sg_op_ln_chain")
    return x, y


@on_tensor_device
def gemm_fp8_mx(a8, w8, sw, sa=None, a_mx=None, bias=None, residual=None, act: int = 0, out_bf16: bool = False, mx_out: bool = False):
    """The MXFP8 forms of the fp8 GEMM (include/segearth_hip.h: sg_gemm_fp8_mx_raw) on caller-quantised operands.  a8 [M,K] u8 with
    either per-row scales `sa` [M] or E8M0 block scales `a_mx` [K/128, M, 4] u8; w8 [N,K] u8 with per-row scales sw [N].
    Returns C, or (c8 [M,N] u8, c_scale [N/128, M, 4] u8) with mx_out."""
    lib = _lib.load()
    M, K = a8.shape
    N = w8.shape[0]
    bias = None if bias is None else _f32(bias)
    residual = None if residual is None else _f32(residual)
    if mx_out:
        c8 = torch.empty(M, N, dtype=torch.uint8, device=a8.device)
        cs = torch.zeros(N // 128, M, 4, dtype=torch.uint8, device=a8.device)
        out = None
    else:
        out = torch.empty(M, N, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=a8.device)
        c8 = cs = None
    check(lib.sg_gemm_fp8_mx_raw(ptr(a8), ptr(sa), ptr(a_mx), ptr(w8), ptr(sw), ptr(bias), ptr(residual), ptr(out), ptr(c8), ptr(cs),
                                 M, N, K, act, int(out_bf16), stream_ptr()), "sg_gemm_fp8_mx_raw")
    return (c8, cs) if mx_out else out


@on_tensor_device
def linear_fp8(A, W, bias=None, residual=None, act: int = 0, out_bf16: bool = False):
    """act(dequant(fp8(A) @ fp8(W)^T) + bias) (+ residual) on the fp8 MFMA path; A [M,K], W [N,K] f32, K % 128 == 0."""
    lib = _lib.load()
    a8, sa = quantize_rows_fp8(A)
    w8, sw = quantize_rows_fp8(W)
    M, K = A.shape
    N = W.shape[0]
    out = torch.empty(M, N, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=A.device)
    bias = None if bias is None else _f32(bias)
    residual = None if residual is None else _f32(residual)
    check(lib.sg_gemm_fp8_raw(ptr(a8), ptr(sa), ptr(w8), ptr(sw), ptr(bias), ptr(residual), ptr(out), M, N, K, act, int(out_bf16),
                              stream_ptr()), "sg_gemm_fp8_raw")
    return out, (a8, sa, w8, sw)


@on_tensor_device
def layernorm(x, gamma, beta, eps: float = 1e-5):
    lib = _lib.load()
    x, gamma, beta = _f32(x), _f32(gamma), _f32(beta)
    _require_gpu(x, gamma, beta)
    D = x.shape[-1]
    y = torch.empty_like(x)
    check(lib.sg_op_layernorm(ptr(x), ptr(gamma), ptr(beta), ptr(y), x.numel() // D, D, eps, stream_ptr()), "sg_op_layernorm")
    return y


@on_tensor_device
def attention(qkv, heads: int, variant: str = "vanilla", sim=None, sim_weight: float = 1.0, precision="bf16",
              want_stats: bool = False):
    """Multi-term attention over packed qkv [B,N,3D] -> ctx [B,N,D] (+ head-averaged A[0,:], diag(A))."""
    lib = _lib.load()
    qkv = _f32(qkv)
    _require_gpu(qkv, sim)
    B, N, D3 = qkv.shape
    D = D3 // 3
    ctx = torch.empty(B, N, D, dtype=torch.float32, device=qkv.device)
    a_cls = torch.empty(B, N, dtype=torch.float32, device=qkv.device) if want_stats else None
    a_diag = torch.empty(B, N, dtype=torch.float32, device=qkv.device) if want_stats else None
    pid = precision_id(precision)
    buf = scratch(lib.sg_op_attention_scratch_bytes(B, N, D, heads, pid), qkv.device)
    sp, sn = _aligned(buf)
    sim = None if sim is None else _f32(sim)
    check(lib.sg_op_attention(ptr(qkv), B, N, D, heads, MODEL_TYPES[variant], ptr(sim), float(sim_weight), ptr(ctx), ptr(a_cls),
                              ptr(a_diag), pid, sp, sn, stream_ptr()), "sg_op_attention")
    return (ctx, a_cls, a_diag) if want_stats else ctx


@on_tensor_device
def similarity_map(patches, temperature: float = 1.0, add_self_similarity: bool = True, precision="f32"):
    """patches [B,n,D] -> cosine self-similarity [B,n,n] (similarity_enhancement.py:37-66)."""
    lib = _lib.load()
    patches = _f32(patches)
    _require_gpu(patches)
    B, n, D = patches.shape
    sim = torch.empty(B, n, n, dtype=torch.float32, device=patches.device)
    buf = scratch(B * n * D * 4 + 1024, patches.device)
    sp, sn = _aligned(buf)
    check(lib.sg_similarity_map(ptr(patches), n * D, D, B, n, D, float(temperature), int(add_self_similarity),
                                precision_id(precision), ptr(sim), sp, sn, stream_ptr()), "sg_similarity_map")
    return sim


@on_tensor_device
def outlier_suppress(feats, attn_cls, attn_diag, gh: int, gw: int, top_k: int = 10, contamination_temp: float = 0.1):
    """feats [B,gh*gw,D] (returns a refined copy) + the selected indices [B,k]."""
    lib = _lib.load()
    feats = _f32(feats).clone()
    attn_cls, attn_diag = _f32(attn_cls), _f32(attn_diag)
    _require_gpu(feats, attn_cls, attn_diag)
    B, n, D = feats.shape
    k = min(top_k, n)
    idx = torch.empty(B, k, dtype=torch.int32, device=feats.device)
    buf = scratch(lib.sg_outlier_scratch_bytes(B, D, k), feats.device)
    sp, _ = _aligned(buf)
    check(lib.sg_outlier_suppress(ptr(feats), ptr(attn_cls), ptr(attn_diag), B, gh, gw, D, top_k, float(contamination_temp),
                                  ptr(idx), sp, stream_ptr()), "sg_outlier_suppress")
    return feats, idx


@on_tensor_device
def weak_token_replace(feats, attn_diag, gh: int, gw: int, top_k: int = 10):
    lib = _lib.load()
    feats = _f32(feats).clone()
    attn_diag = _f32(attn_diag)
    _require_gpu(feats, attn_diag)
    B, n, D = feats.shape
    k = min(top_k, n)
    idx = torch.empty(B, k, dtype=torch.int32, device=feats.device)
    buf = scratch(lib.sg_outlier_scratch_bytes(B, D, k), feats.device)
    sp, _ = _aligned(buf)
    check(lib.sg_weak_token_replace(ptr(feats), ptr(attn_diag), B, gh, gw, D, top_k, ptr(idx), sp, stream_ptr()),
          "sg_weak_token_replace")
    return feats, idx


COSINE_LDS_BYTES = 160 * 1024      # what sg_cosine_logits stages in LDS at most: (Q*E + E + Q) floats (head.hip)
POSTPROCESS_MAX_Q = 64             # PP_MAX_Q of sg_postprocess / sg_postprocess_multi (head.hip); beyond it: sg_postprocess_wide


@on_tensor_device
def cosine_logits(tokens, cls, text, global_debias_factor: float = 0.0, cls_token_lambda: float = 0.0, two_plane: bool = False):
    """tokens [B,n,E], cls [B,E] or None, text [Q,E] -> logits [B,Q,n] (segmentor.py:309-336,374-386).
    ``two_plane`` (no global debias): the per-pixel form of the exact tower mode -- the product on the f16 matrix pipe, operands as two f16 planes.
    Each feature / text element then carries a representation error of max(2^-22 |x|, 2^-25): an absolute floor of 2^-25 per element, so
    the result is f32-grade for per-element magnitudes of 1e-2 and above and its error grows as 1 / scale below that (CPU emulation, E = 768,
    Q = 16, max |err| by token scale: 1 7e-8, 1e-2 2.6e-7, 1e-3 2.5e-6, 1e-4 2.5e-5, 1e-5 2.3e-4; measured on an MI355X with every row at
    2^-13, E = 96: 7.1e-5)."""
    lib = _lib.load()
    tokens, text = _f32(tokens), _f32(text)
    cls = None if cls is None else _f32(cls)
    _require_gpu(tokens, text, cls)
    B, n, E = tokens.shape
    Q = text.shape[0]
    out = torch.empty(B, Q, n, dtype=torch.float32, device=tokens.device)
    if two_plane and float(global_debias_factor) == 0.0:
        check(lib.sg_cosine_logits_two_plane(ptr(tokens), ptr(cls), ptr(text), B, n, E, Q, float(cls_token_lambda), ptr(out), stream_ptr()),
              "sg_cosine_logits_two_plane")
        return out
    if (Q * E + E + Q) * 4 > COSINE_LDS_BYTES:            # sg_cosine_logits would refuse ("exceeds LDS"): the text rows go through LDS in chunks
        check(lib.sg_cosine_logits_wide(ptr(tokens), ptr(cls), ptr(text), B, n, E, Q, float(global_debias_factor), float(cls_token_lambda),
                                        ptr(out), stream_ptr()), "sg_cosine_logits_wide")
        return out
    check(lib.sg_cosine_logits(ptr(tokens), ptr(cls), ptr(text), B, n, E, Q, float(global_debias_factor), float(cls_token_lambda),
                               ptr(out), stream_ptr()), "sg_cosine_logits")
    return out


def _stitch(entry, tile_logits, windows, up_hw, pad_tl, canvas_hw, ramp=None):
    """sg_stitch and sg_stitch_blend.  No window-count check here: the entries have none either."""
    lib = _lib.load()
    tile_logits = _f32(tile_logits)
    windows = windows.to(device=tile_logits.device, dtype=torch.int32).contiguous()
    _require_gpu(tile_logits)
    T, Q, gh, gw = tile_logits.shape
    H, W = canvas_hw
    tail, ramp = _ramp_args(entry, ramp, tile_logits.device)
    canvas = torch.empty(Q, H, W, dtype=torch.float32, device=tile_logits.device)
    check(getattr(lib, entry)(ptr(tile_logits), ptr(windows), T, Q, gh, gw, up_hw[0], up_hw[1], pad_tl[0], pad_tl[1], H, W, ptr(canvas), *tail,
                              stream_ptr()), entry)
    return canvas


@on_tensor_device
def stitch(tile_logits, windows, up_hw, pad_tl, canvas_hw):
    """tile_logits [T,Q,gh,gw]; windows int32 [T,4] (y1,y2,x1,x2) -> canvas [Q,H,W]."""
    return _stitch("sg_stitch", tile_logits, windows, up_hw, pad_tl, canvas_hw)


@on_tensor_device
def resize_bilinear(src, size):
    """[C,h,w] -> [C,H,W], align_corners=False."""
    lib = _lib.load()
    src = _f32(src)
    _require_gpu(src)
    Cc, h, w = src.shape
    H, W = size
    dst = torch.empty(Cc, H, W, dtype=torch.float32, device=src.device)
    check(lib.sg_resize_bilinear(ptr(src), Cc, h, w, ptr(dst), H, W, stream_ptr()), "sg_resize_bilinear")
    return dst


@on_tensor_device
def postprocess(logits, query_idx, num_classes: int, logit_scale: float, prob_thd: float, bg_idx: int, want_probs: bool = True):
    """logits [Q,H,W] -> (probs [K,H,W] or None, labels int64 [1,H,W]) (segmentor.py:475-489)."""
    lib = _lib.load()
    logits = _f32(logits)
    _require_gpu(logits)
    Q, H, W = logits.shape
    qi = query_idx.to(device=logits.device, dtype=torch.int32).contiguous()
    probs = torch.empty(num_classes, H, W, dtype=torch.float32, device=logits.device) if want_probs else None
    labels = torch.empty(1, H, W, dtype=torch.int64, device=logits.device)
    entry, name = (lib.sg_postprocess, "sg_postprocess") if Q <= POSTPROCESS_MAX_Q else (lib.sg_postprocess_wide, "sg_postprocess_wide")
    check(entry(ptr(logits), ptr(qi), Q, num_classes, H, W, float(logit_scale), float(prob_thd), int(bg_idx),
                ptr(probs), ptr(labels), stream_ptr()), name)
    return probs, labels


def _prefix(counts):
    out = [0]
    for c in counts:
        out.append(out[-1] + int(c))
    return out


def flat_views(flat, planes: int, image_hw):
    """The views [planes,H,W] of one flat buffer that holds N images back to back with ``planes`` values per pixel."""
    pix = _prefix(h * w for h, w in image_hw)
    return [flat[planes * pix[n]:planes * pix[n + 1]].view(planes, h, w) for n, (h, w) in enumerate(image_hw)]


def _tile_args(what, tile_logits, windows, up_hw, pad_tl, query_idx):
    """What every single-image head takes: tile_logits [T,Q,gh,gw], windows int32 [T,4] (y1,y2,x1,x2) and the query indices, checked
    against each other -> (device, the entry's leading arguments through pad_tl, query indices int32, the tensors those arguments point
    into: hold them until the launch)."""
    tile_logits = _f32(tile_logits)
    windows = windows.to(device=tile_logits.device, dtype=torch.int32).contiguous()
    _require_gpu(tile_logits)
    T, Q, gh, gw = tile_logits.shape
    qi = query_idx.to(device=tile_logits.device, dtype=torch.int32).contiguous()
    if int(qi.numel()) != Q or int(windows.numel()) != 4 * T:
        raise ValueError(f"{what}: {T} tiles of {Q} queries, but {windows.numel() // 4} windows and {qi.numel()} query indices")
    return tile_logits.device, (ptr(tile_logits), ptr(windows), T, Q, gh, gw, up_hw[0], up_hw[1], pad_tl[0], pad_tl[1]), qi, (tile_logits, windows)


def _multi_args(what, tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx=None, out_hw=None, planes: int = 1):
    """What every multi-image launch takes.  tile_logits [T,Q,gh,gw]; windows [T,4] in each image's own coordinates; tile_image [T] =
    image of each tile (0..N-1); image_hw [(H, W)] * N; image_tiles [(first, count)] * N; out_hw [(H, W)] * N for the resized heads, whose
    outputs, offsets and blocks are counted in OUTPUT pixels.  Checks the sizes against each other and builds the two descriptor tensors:
    i32 [image hw | image tiles | out hw] and i64 [planes * first output pixel | prefix of the 64 x 4 blocks].
    -> (device, the entry's leading arguments through the block count, query indices int32 or None, the prefix of the output pixels, the
    tensors those arguments point into: hold them until the launch)."""
    tile_logits = _f32(tile_logits)
    _require_gpu(tile_logits)
    dev = tile_logits.device
    T, Q, gh, gw = tile_logits.shape
    N = len(image_hw)
    qi = None if query_idx is None else query_idx.to(device=dev, dtype=torch.int32).contiguous()
    windows = torch.as_tensor(windows, dtype=torch.int32).to(dev).contiguous()
    tile_image = torch.as_tensor(tile_image, dtype=torch.int32).to(dev).contiguous()
    if (qi is not None and int(qi.numel()) != Q) or int(windows.numel()) != 4 * T or int(tile_image.numel()) != T or len(image_tiles) != N or \
            (out_hw is not None and len(out_hw) != N):
        raise ValueError(f"{what}: tile logits, windows, tile_image, image descriptors and query indices disagree in size")
    if any(f < 0 or c <= 0 or f + c > T for f, c in image_tiles):
        raise ValueError(f"{what}: image_tiles {list(image_tiles)} leave the {T} tiles")
    sizes = image_hw if out_hw is None else out_hw
    pix = _prefix(h * w for h, w in sizes)
    blocks = _prefix(-(-w // 64) * -(-h // 4) for h, w in sizes)
    i32 = torch.tensor([list(hw) for hw in image_hw] + [list(ft) for ft in image_tiles] + [list(hw) for hw in out_hw or ()],
                       dtype=torch.int32).to(dev)
    i64 = torch.tensor([planes * p for p in pix[:-1]] + blocks, dtype=torch.int64).to(dev)
    desc = (ptr(i32), ptr(i32[N:])) + ((ptr(i32[2 * N:]),) if out_hw is not None else ()) + (ptr(i64), ptr(i64[N:]), N, blocks[-1])
    lead = (ptr(tile_logits), ptr(windows), ptr(tile_image), T, Q, gh, gw, up_hw[0], up_hw[1], pad_tl[0], pad_tl[1]) + desc
    return dev, lead, qi, pix, (tile_logits, windows, tile_image, i32, i64)


def _label_outputs(dev, want_conf: bool, H: int, W: int):
    """-> (labels int64 [1,H,W], conf f32 [H,W] or None)"""
    return torch.empty(1, H, W, dtype=torch.int64, device=dev), torch.empty(H, W, dtype=torch.float32, device=dev) if want_conf else None


def _label_outputs_multi(dev, want_conf: bool, pixels: int):
    """-> (labels int64 [pixels], conf f32 [pixels] or None): the images back to back."""
    return torch.empty(pixels, dtype=torch.int64, device=dev), torch.empty(pixels, dtype=torch.float32, device=dev) if want_conf else None


def _label_results_multi(labels, conf, sizes, flat_conf: bool = False):
    """What the multi-image label heads return: (label maps [1,H,W], the flat buffer they are views of), and with a ``conf`` its maps
    [H,W] (``flat_conf``: the flat buffer itself) as a third result."""
    lab = flat_views(labels, 1, sizes)
    if conf is None:
        return lab, labels
    return lab, labels, (conf if flat_conf else [c[0] for c in flat_views(conf, 1, sizes)])


def _topk_outputs(dev, k, H: int, W: int):
    """-> (classes int32, probs f32), both [k,H,W]; a ``k`` below 1 is left for the entry to refuse."""
    kk = max(int(k), 0)
    return torch.empty(kk, H, W, dtype=torch.int32, device=dev), torch.empty(kk, H, W, dtype=torch.float32, device=dev)


def _topk_outputs_multi(dev, k, pixels: int):
    """-> (max(k, 0), classes int32, probs f32), both flat with k planes per image, the images back to back."""
    kk = max(int(k), 0)
    return kk, torch.empty(kk * pixels, dtype=torch.int32, device=dev), torch.empty(kk * pixels, dtype=torch.float32, device=dev)


def _label_head(entry, tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes, logit_scale, prob_thd, bg_idx, want_conf,
                ramp=None):
    """sg_label_head and sg_label_head_blend."""
    lib = _lib.load()
    dev, lead, qi, hold = _tile_args(entry[3:], tile_logits, windows, up_hw, pad_tl, query_idx)
    H, W = canvas_hw
    tail, ramp = _ramp_args(entry, ramp, dev)
    labels, conf = _label_outputs(dev, want_conf, H, W)
    check(getattr(lib, entry)(*lead, H, W, ptr(qi), int(num_classes), float(logit_scale), float(prob_thd), int(bg_idx), ptr(labels), ptr(conf),
                              *tail, stream_ptr()), entry)
    return (labels, conf) if want_conf else labels


def _stitch_multi(entry, tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, ramp=None):
    """sg_stitch_multi and sg_stitch_blend_multi."""
    lib = _lib.load()
    Q = tile_logits.shape[1]
    dev, lead, _, pix, hold = _multi_args(entry[3:], tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, planes=Q)
    tail, ramp = _ramp_args(entry, ramp, dev)
    canvases = torch.empty(Q * pix[-1], dtype=torch.float32, device=dev)
    check(getattr(lib, entry)(*lead, canvases.numel(), ptr(canvases), *tail, stream_ptr()), entry)
    return canvases, flat_views(canvases, Q, image_hw)


def _label_head_multi(entry, tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes, logit_scale,
                      prob_thd, bg_idx, want_conf, flat_conf, ramp=None):
    """sg_label_head_multi and sg_label_head_blend_multi."""
    lib = _lib.load()
    dev, lead, qi, pix, hold = _multi_args(entry[3:], tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx)
    tail, ramp = _ramp_args(entry, ramp, dev)
    labels, conf = _label_outputs_multi(dev, want_conf, pix[-1])
    check(getattr(lib, entry)(*lead, pix[-1], ptr(qi), int(num_classes), float(logit_scale), float(prob_thd), int(bg_idx), ptr(labels),
                              ptr(conf), *tail, stream_ptr()), entry)
    return _label_results_multi(labels, conf, image_hw, flat_conf)


@on_tensor_device
def label_head(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes: int, logit_scale: float, prob_thd: float,
               bg_idx: int, want_conf: bool = False):
    """sg_label_head: ``stitch`` + ``postprocess`` without the canvas, for any Q.  tile_logits [T,Q,gh,gw]; windows int32 [T,4]
    -> labels int64 [1,H,W], or (labels, conf f32 [H,W] = the winning class's probability) with ``want_conf``."""
    return _label_head("sg_label_head", tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes, logit_scale, prob_thd, bg_idx,
                       want_conf)


@on_tensor_device
def stitch_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles):
    """The canvases of N images in one launch (sg_stitch_multi); the arguments: ``_multi_args``.
    -> (canvases: one flat f32 buffer, list of N views [Q,H,W] into it)."""
    return _stitch_multi("sg_stitch_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles)


@on_tensor_device
def label_head_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes: int,
                     logit_scale: float, prob_thd: float, bg_idx: int, want_conf: bool = False, flat_conf: bool = False):
    """sg_label_head_multi: the labels of N images in one launch, from their tile logits (arguments as ``stitch_multi`` plus the
    post-process parameters).  -> (list of labels int64 [1,H,W], the flat int64 buffer they are views of, images back to back), plus
    the list of conf f32 [H,W] maps as a third result with ``want_conf`` (``flat_conf``: the one flat f32 buffer those maps are views
    of instead of the list).  Equals ``label_head`` per image byte for byte."""
    return _label_head_multi("sg_label_head_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes,
                             logit_scale, prob_thd, bg_idx, want_conf, flat_conf)


BLEND_KINDS = ("uniform", "linear", "hann")
BLEND_MAX_RAMP = 2048                                                    # SG_BLEND_MAX_RAMP (include/segearth_hip.h)
_BLEND_TABLES: dict = {}                                                 # (kind, R, device) -> the device table


def blend_args(blend, blend_ramp=None):
    """The ``blend`` / ``blend_ramp`` options checked -> (blend, blend_ramp): ``blend`` one of BLEND_KINDS, ``blend_ramp`` None (the
    full window: half the tile's smaller side, resolved where the tile size is known) or an integer in [1, BLEND_MAX_RAMP - 1]."""
    if blend not in BLEND_KINDS:
        raise ValueError(f"blend must be one of {BLEND_KINDS}, got {blend!r}")
    if blend_ramp is None:
        return blend, None
    import numbers
    if isinstance(blend_ramp, bool) or not isinstance(blend_ramp, numbers.Integral) or not 1 <= blend_ramp <= BLEND_MAX_RAMP - 1:
        raise ValueError(f"blend_ramp must be None or an integer in [1, {BLEND_MAX_RAMP - 1}], got {blend_ramp!r}")
    return blend, int(blend_ramp)


def blend_ramp(kind: str, R: int) -> torch.Tensor:
    """The ramp table of sg_stitch_blend on the host, f32 [R + 1]: r[d] = (d + 0.5) / R ("linear") or sin^2(pi/2 (d + 0.5) / R) ("hann")
    for d < R and r[R] = 1 exactly, computed in float64 and rounded once.  "uniform": the one entry 1.0, the plain mean."""
    import math
    kind, R = blend_args(kind, R)
    if kind == "uniform":
        return torch.ones(1, dtype=torch.float32)
    ramp = [(d + 0.5) / R for d in range(R)]
    if kind == "hann":
        ramp = [math.sin(0.5 * math.pi * v) ** 2 for v in ramp]
    return torch.tensor(ramp + [1.0], dtype=torch.float64).to(torch.float32)


def blend_table(kind: str, R: int, device) -> torch.Tensor:
    """``blend_ramp(kind, R)`` on ``device``, built once per (kind, R, device)."""
    key = (kind, int(R), str(torch.device(device)))
    if key not in _BLEND_TABLES:
        _BLEND_TABLES[key] = blend_ramp(kind, R).to(device)
    return _BLEND_TABLES[key]


def _ramp_args(entry: str, ramp, device):
    """What a ``_blend`` entry takes behind its counterpart's arguments, from a caller's ramp tensor -> ((pointer of the f32 table on
    ``device``, its length), the table: hold it until the launch); ((), None) for every other entry."""
    if "_blend" not in entry:
        return (), None
    ramp = _f32(ramp).to(device).reshape(-1)
    if not 1 <= int(ramp.numel()) <= BLEND_MAX_RAMP:
        raise ValueError(f"{entry[3:]}: a ramp of {ramp.numel()} entries, must be 1 .. {BLEND_MAX_RAMP}")
    return (ptr(ramp), int(ramp.numel())), ramp


@on_tensor_device
def stitch_blend(tile_logits, windows, up_hw, pad_tl, canvas_hw, ramp):
    """sg_stitch_blend: ``stitch`` with every tile weighted by ``ramp`` (f32 [L], ``blend_ramp``) of the pixel's distance to the tile's
    own window edges and divided by the sum of the weights -> canvas [Q,H,W]."""
    return _stitch("sg_stitch_blend", tile_logits, windows, up_hw, pad_tl, canvas_hw, ramp)


@on_tensor_device
def stitch_blend_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, ramp):
    """sg_stitch_blend_multi: ``stitch_multi`` with the weights of ``stitch_blend``; the same results."""
    return _stitch_multi("sg_stitch_blend_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, ramp)


@on_tensor_device
def label_head_blend(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes: int, logit_scale: float, prob_thd: float,
                     bg_idx: int, ramp, want_conf: bool = False):
    """sg_label_head_blend: ``label_head`` on the blended stitch (``stitch_blend``'s value per pixel and query); the same results."""
    return _label_head("sg_label_head_blend", tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes, logit_scale, prob_thd,
                       bg_idx, want_conf, ramp)


@on_tensor_device
def label_head_blend_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes: int,
                           logit_scale: float, prob_thd: float, bg_idx: int, ramp, want_conf: bool = False, flat_conf: bool = False):
    """sg_label_head_blend_multi: ``label_head_multi`` on the blended stitch; the same results, ``label_head_blend`` per image byte for
    byte."""
    return _label_head_multi("sg_label_head_blend_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx,
                             num_classes, logit_scale, prob_thd, bg_idx, want_conf, flat_conf, ramp)


@on_tensor_device
def prob_head(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes: int, logit_scale: float, prob_thd: float, bg_idx: int):
    """sg_prob_head: ``stitch`` + ``postprocess`` without the canvas, for any Q.  Arguments as ``label_head``
    -> (probs f32 [K,H,W], labels int64 [1,H,W]), byte for byte what ``postprocess(stitch(...))`` returns."""
    lib = _lib.load()
    dev, lead, qi, hold = _tile_args("prob_head", tile_logits, windows, up_hw, pad_tl, query_idx)
    H, W = canvas_hw
    probs = torch.empty(int(num_classes), H, W, dtype=torch.float32, device=dev)
    labels = torch.empty(1, H, W, dtype=torch.int64, device=dev)
    check(lib.sg_prob_head(*lead, H, W, ptr(qi), int(num_classes), float(logit_scale), float(prob_thd), int(bg_idx), ptr(probs), ptr(labels),
                           stream_ptr()), "sg_prob_head")
    return probs, labels


@on_tensor_device
def prob_head_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes: int,
                    logit_scale: float, prob_thd: float, bg_idx: int, flat_probs: bool = False):
    """sg_prob_head_multi: the class probabilities and labels of N images in one launch, from their tile logits (arguments as
    ``label_head_multi``).  -> (list of probs f32 [K,H,W], list of labels int64 [1,H,W], the flat int64 buffer the label maps are views
    of, images back to back): what ``postprocess_multi(..., want_probs=True, flat_labels=True)`` returns, and ``prob_head`` per image
    byte for byte.  The probs of image n are a view at K * (its first pixel) of one flat f32 buffer (a fourth result with ``flat_probs``)."""
    lib = _lib.load()
    dev, lead, qi, pix, hold = _multi_args("prob_head_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx)
    K = int(num_classes)
    labels = torch.empty(pix[-1], dtype=torch.int64, device=dev)
    probs = torch.empty(max(K, 0) * pix[-1], dtype=torch.float32, device=dev)
    check(lib.sg_prob_head_multi(*lead, pix[-1], ptr(qi), K, float(logit_scale), float(prob_thd), int(bg_idx), ptr(probs), ptr(labels),
                                 stream_ptr()), "sg_prob_head_multi")
    prb, lab = flat_views(probs, K, image_hw), flat_views(labels, 1, image_hw)
    return (prb, lab, labels, probs) if flat_probs else (prb, lab, labels)


TOPK_MAX = 8                                                             # SG_TOPK_MAX (include/segearth_hip.h)


@on_tensor_device
def topk_head(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes: int, logit_scale: float, k: int):
    """sg_topk_head: the k best classes per pixel with their probabilities, from the tile logits, without a canvas or [K,H,W] planes,
    for any Q.  Arguments as ``label_head`` with ``k`` (1 .. min(8, K)) for the threshold -> (classes int32 [k,H,W], probs f32
    [k,H,W]), slots in descending probability, equal values by ascending class; -1 / 0 in a slot no class filled (classes that own no
    query never appear).  Plane 0 is ``label_head``'s label before the threshold and its conf, byte for byte."""
    lib = _lib.load()
    dev, lead, qi, hold = _tile_args("topk_head", tile_logits, windows, up_hw, pad_tl, query_idx)
    H, W = canvas_hw
    classes, probs = _topk_outputs(dev, k, H, W)
    check(lib.sg_topk_head(*lead, H, W, ptr(qi), int(num_classes), float(logit_scale), int(k), ptr(classes), ptr(probs), stream_ptr()),
          "sg_topk_head")
    return classes, probs


@on_tensor_device
def topk_head_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes: int,
                    logit_scale: float, k: int):
    """sg_topk_head_multi: ``topk_head`` for N images in one launch (arguments as ``label_head_multi`` with ``k`` for the threshold).
    -> (list of classes int32 [k,H,W], list of probs f32 [k,H,W]): views at k * (the image's first pixel) of two flat buffers.  Equals
    ``topk_head`` per image byte for byte."""
    lib = _lib.load()
    dev, lead, qi, pix, hold = _multi_args("topk_head_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx)
    kk, classes, probs = _topk_outputs_multi(dev, k, pix[-1])
    check(lib.sg_topk_head_multi(*lead, pix[-1], ptr(qi), int(num_classes), float(logit_scale), int(k), ptr(classes), ptr(probs), stream_ptr()),
          "sg_topk_head_multi")
    return flat_views(classes, kk, image_hw), flat_views(probs, kk, image_hw)


RESIZED_FORMS = {"auto": 0, "direct": 1, "staged": 2}                    # SG_RESIZED_* (include/segearth_hip.h)
RESIZED_STAGE_PIX = 512                                                  # RS_STAGE_PIX (csrc/head.hip): 16 KiB per chunk of 8 queries


def resized_footprint(canvas_hw, out_hw):
    """(rows, columns) of the canvas that a block of 64 x 4 output pixels can touch: csrc/head.hip's rs_span."""
    (h, w), (H, W) = canvas_hw, out_hw
    return -(-4 * h // H) + 2, -(-64 * w // W) + 2


def _resized_form(form: str, what: str, pairs) -> int:
    if form not in RESIZED_FORMS:
        raise ValueError(f"{what}: form={form!r} is none of {sorted(RESIZED_FORMS)}")
    if form == "staged":
        for chw, ohw in pairs:
            r, c = resized_footprint(chw, ohw)
            if r * c > RESIZED_STAGE_PIX:
                raise ValueError(f"{what}: the staged form does not fit {tuple(chw)} -> {tuple(ohw)}: a block's footprint of {r} x {c} "
                                 f"canvas pixels exceeds the stage of {RESIZED_STAGE_PIX}")
    return RESIZED_FORMS[form]


@on_tensor_device
def label_head_resized(tile_logits, windows, up_hw, pad_tl, canvas_hw, out_hw, query_idx, num_classes: int, logit_scale: float,
                       prob_thd: float, bg_idx: int, want_conf: bool = False, form: str = "auto"):
    """sg_label_head_resized: ``label_head`` at another ``ori_shape`` -- stitch, count division, bilinear resize of the [h,w] canvas to
    ``out_hw``, post-process -- with neither canvas.  -> labels int64 [1,H,W] (and conf f32 [H,W] with ``want_conf``), (H, W) = out_hw.
    ``form``: "direct", "staged" (refused where a block's footprint does not fit the stage) or "auto"; the bytes do not depend on it."""
    flags = _resized_form(form, "label_head_resized", [(canvas_hw, out_hw)])
    lib = _lib.load()
    dev, lead, qi, hold = _tile_args("label_head_resized", tile_logits, windows, up_hw, pad_tl, query_idx)
    (h, w), (H, W) = canvas_hw, out_hw
    labels, conf = _label_outputs(dev, want_conf, H, W)
    check(lib.sg_label_head_resized(*lead, h, w, H, W, ptr(qi), int(num_classes), float(logit_scale), float(prob_thd), int(bg_idx),
                                    ptr(labels), ptr(conf), flags, stream_ptr()), "sg_label_head_resized")
    return (labels, conf) if want_conf else labels


@on_tensor_device
def label_head_resized_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, out_hw, query_idx, num_classes: int,
                             logit_scale: float, prob_thd: float, bg_idx: int, want_conf: bool = False, form: str = "auto"):
    """sg_label_head_resized_multi: ``label_head_resized`` for N images in one launch (arguments as ``label_head_multi`` plus
    ``out_hw`` [(H, W)] * N, each image's ori_shape; an image whose out_hw is its canvas size runs with identity taps).  -> (list of
    labels int64 [1,H,W], the flat int64 buffer they are views of), plus the list of conf maps with ``want_conf``.  Equals
    ``label_head_resized`` per image byte for byte."""
    out_hw = [tuple(int(v) for v in s) for s in out_hw]
    flags = _resized_form(form, "label_head_resized_multi", zip(image_hw, out_hw))
    lib = _lib.load()
    dev, lead, qi, pix, hold = _multi_args("label_head_resized_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles,
                                           query_idx, out_hw)
    labels, conf = _label_outputs_multi(dev, want_conf, pix[-1])
    check(lib.sg_label_head_resized_multi(*lead, pix[-1], ptr(qi), int(num_classes), float(logit_scale), float(prob_thd), int(bg_idx),
                                          ptr(labels), ptr(conf), flags, stream_ptr()), "sg_label_head_resized_multi")
    return _label_results_multi(labels, conf, out_hw)


@on_tensor_device
def topk_head_resized(tile_logits, windows, up_hw, pad_tl, canvas_hw, out_hw, query_idx, num_classes: int, logit_scale: float, k: int,
                      form: str = "auto"):
    """sg_topk_head_resized: ``topk_head`` at another ``ori_shape`` (see ``label_head_resized``) -> (classes int32 [k,H,W], probs f32
    [k,H,W]), (H, W) = out_hw.  Plane 0 is ``label_head_resized``'s label before the threshold and its conf, byte for byte."""
    flags = _resized_form(form, "topk_head_resized", [(canvas_hw, out_hw)])
    lib = _lib.load()
    dev, lead, qi, hold = _tile_args("topk_head_resized", tile_logits, windows, up_hw, pad_tl, query_idx)
    (h, w), (H, W) = canvas_hw, out_hw
    classes, probs = _topk_outputs(dev, k, H, W)
    check(lib.sg_topk_head_resized(*lead, h, w, H, W, ptr(qi), int(num_classes), float(logit_scale), int(k), ptr(classes), ptr(probs), flags,
                                   stream_ptr()), "sg_topk_head_resized")
    return classes, probs


@on_tensor_device
def topk_head_resized_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, out_hw, query_idx, num_classes: int,
                            logit_scale: float, k: int, form: str = "auto"):
    """sg_topk_head_resized_multi: ``topk_head_resized`` for N images in one launch (arguments as ``label_head_resized_multi`` with
    ``k`` for the threshold) -> (list of classes int32 [k,H,W], list of probs f32 [k,H,W]): views at k * (the image's first output
    pixel) of two flat buffers.  Equals ``topk_head_resized`` per image byte for byte."""
    out_hw = [tuple(int(v) for v in s) for s in out_hw]
    flags = _resized_form(form, "topk_head_resized_multi", zip(image_hw, out_hw))
    lib = _lib.load()
    dev, lead, qi, pix, hold = _multi_args("topk_head_resized_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles,
                                           query_idx, out_hw)
    kk, classes, probs = _topk_outputs_multi(dev, k, pix[-1])
    check(lib.sg_topk_head_resized_multi(*lead, pix[-1], ptr(qi), int(num_classes), float(logit_scale), int(k), ptr(classes), ptr(probs), flags,
                                         stream_ptr()), "sg_topk_head_resized_multi")
    return flat_views(classes, kk, out_hw), flat_views(probs, kk, out_hw)


TTA_MAX_VIEWS = 8                                                        # SG_TTA_MAX_VIEWS (include/segearth_hip.h)
TTA_VIEW_FIELDS = 11                                                     # SG_TTA_VIEW_FIELDS
TTA_MAX_Q = POSTPROCESS_MAX_Q                                            # sg_tta_head's bound on Q; beyond: tta_accumulate / tta_finish


def tta_views(hw, scales, flip: bool = False):
    """The views of test-time augmentation for an image of ``hw``: ``scales`` x ({False, True} if ``flip`` else {False}), scale outer
    -> [(scale, flipped, (h, w))] with (h, w) = (max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5))).  ``scales=None`` means (1.0,).
    A pure function (no device); more than TTA_MAX_VIEWS views, no view or a scale that is no positive finite number is refused."""
    H, W = int(hw[0]), int(hw[1])
    if H <= 0 or W <= 0:
        raise ValueError(f"tta_views: bad image size {tuple(hw)}")
    scales = (1.0,) if scales is None else tuple(float(s) for s in ([scales] if isinstance(scales, (int, float)) else scales))
    if not scales or any(not (s > 0.0 and s != float("inf")) for s in scales):
        raise ValueError(f"tta_scales must be a non-empty sequence of positive finite numbers, got {scales!r}")
    views = [(s, f, (max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5)))) for s in scales for f in ((False, True) if flip else (False,))]
    if len(views) > TTA_MAX_VIEWS:
        raise ValueError(f"test-time augmentation takes at most {TTA_MAX_VIEWS} views, got {len(views)} ({len(scales)} scales"
                         f"{' x 2 for the flip' if flip else ''})")
    return views


@on_tensor_device
def tta_head(views, out_hw, query_idx, num_classes: int, logit_scale: float, prob_thd: float, bg_idx: int, want_conf: bool = False,
             want_probs: bool = False, form: str = "auto"):
    """sg_tta_head: the class probabilities of V views of one image merged at ``out_hw`` in one launch, no canvas and no per-view planes
    (the definition: include/segearth_hip.h).  ``views``: [(tile_logits [T_v,Q,gh_v,gw_v], windows int32 [T_v,4], up_hw, pad_tl,
    canvas_hw, flipped)] in merge order.  -> labels int64 [1,H,W], then conf f32 [H,W] with ``want_conf`` and the mean planes f32
    [K,H,W] with ``want_probs`` (a tuple when either is asked).  The views' tile logits are copied into one buffer (one view: used as
    it is).  ``form``: as ``label_head_resized``, per view; a view that does not fit the stage runs direct."""
    if form not in RESIZED_FORMS:
        raise ValueError(f"tta_head: form={form!r} is none of {sorted(RESIZED_FORMS)}")
    if not 1 <= len(views) <= TTA_MAX_VIEWS:
        raise ValueError(f"tta_head: {len(views)} views, must lie in [1, {TTA_MAX_VIEWS}]")
    lib = _lib.load()
    tls, wins, table, first = [], [], [], 0
    dev, Q = None, None
    for v, (tl, win, up_hw, pad_tl, canvas_hw, flipped) in enumerate(views):
        tl = _f32(tl)
        _require_gpu(tl)
        T, q, gh, gw = tl.shape
        dev, Q = (tl.device, q) if dev is None else (dev, Q)
        win = torch.as_tensor(win, dtype=torch.int32).to(dev).contiguous()
        if q != Q or int(win.numel()) != 4 * T or tl.device != dev:
            raise ValueError(f"tta_head: view {v} has {T} tiles of {q} queries and {win.numel() // 4} windows; the first view has {Q} queries")
        tls.append(tl.reshape(-1)); wins.append(win.reshape(-1, 4))
        table.append([T, first, gh, gw, up_hw[0], up_hw[1], pad_tl[0], pad_tl[1], canvas_hw[0], canvas_hw[1], int(bool(flipped))])
        first += T
    qi = query_idx.to(device=dev, dtype=torch.int32).contiguous()
    if int(qi.numel()) != Q:
        raise ValueError(f"tta_head: {Q} queries but {qi.numel()} query indices")
    logits = tls[0] if len(tls) == 1 else torch.cat(tls)
    windows = wins[0] if len(wins) == 1 else torch.cat(wins)
    desc = (C.c_int32 * (len(table) * TTA_VIEW_FIELDS))(*[int(x) for row in table for x in row])
    H, W = (int(v) for v in out_hw)
    K = int(num_classes)
    labels = torch.empty(1, H, W, dtype=torch.int64, device=dev)
    conf = torch.empty(H, W, dtype=torch.float32, device=dev) if want_conf else None
    probs = torch.empty(K, H, W, dtype=torch.float32, device=dev) if want_probs else None
    check(lib.sg_tta_head(ptr(logits), int(logits.numel()), ptr(windows), first, desc, len(table), Q, H, W, ptr(qi), K, float(logit_scale),
                          float(prob_thd), int(bg_idx), ptr(labels), ptr(conf), ptr(probs), RESIZED_FORMS[form], stream_ptr()), "sg_tta_head")
    out = (labels,) + ((conf,) if want_conf else ()) + ((probs,) if want_probs else ())
    return out if len(out) > 1 else labels


@on_tensor_device
def tta_accumulate(probs_view, flipped: bool, acc=None):
    """sg_tta_accumulate: ``acc`` += one view's probability planes f32 [K,H,W] (mirrored along the width when ``flipped``), IN PLACE;
    ``acc=None`` starts a new accumulator with this view.  -> acc."""
    lib = _lib.load()
    p = _f32(probs_view)
    _require_gpu(p)
    K, H, W = p.shape
    first = acc is None
    if first:
        acc = torch.empty_like(p)
    elif tuple(acc.shape) != (K, H, W) or acc.dtype != torch.float32 or not acc.is_contiguous() or acc.device != p.device:
        raise ValueError(f"tta_accumulate: the accumulator must be a contiguous f32 {(K, H, W)} tensor on the view's device")
    check(lib.sg_tta_accumulate(ptr(p), K, H, W, int(bool(flipped)), ptr(acc), int(first), stream_ptr()), "sg_tta_accumulate")
    return acc


@on_tensor_device
def tta_finish(acc, n_views: int, prob_thd: float, bg_idx: int, want_conf: bool = False, want_probs: bool = False):
    """sg_tta_finish: the accumulator of ``n_views`` views -> labels int64 [1,H,W], then conf f32 [H,W] with ``want_conf`` and the mean
    planes with ``want_probs`` -- written IN PLACE over ``acc``, which is what is returned (a tuple when either is asked)."""
    lib = _lib.load()
    _require_gpu(acc)
    if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.dim() != 3:
        raise ValueError("tta_finish: the accumulator must be a contiguous f32 [K,H,W] tensor")
    K, H, W = acc.shape
    labels = torch.empty(1, H, W, dtype=torch.int64, device=acc.device)
    conf = torch.empty(H, W, dtype=torch.float32, device=acc.device) if want_conf else None
    check(lib.sg_tta_finish(ptr(acc), int(n_views), K, H, W, float(prob_thd), int(bg_idx), ptr(labels), ptr(conf),
                            ptr(acc) if want_probs else None, stream_ptr()), "sg_tta_finish")
    out = (labels,) + ((conf,) if want_conf else ()) + ((acc,) if want_probs else ())
    return out if len(out) > 1 else labels


def topk_from_probs(probs, query_idx, k: int):
    """The canvas-route equivalent of ``topk_head`` in torch (host or device tensors): class probabilities [K,H,W] (what ``postprocess``
    returns) -> (classes int32 [k,H,W], probs f32 [k,H,W]) by a stable descending sort over the classes, so equal values keep ascending
    class order; a class that owns no query is left out, and the slots it leaves are -1 / 0.  Not a hot path: it serves the routes on
    which the fused head cannot run (PAMR, a resize, whole-image inference), which have the [K,H,W] planes anyway."""
    K = int(probs.shape[0])
    k = int(k)
    if not 1 <= k <= min(TOPK_MAX, K):
        raise ValueError(f"topk_from_probs: k={k} must lie in [1, min({TOPK_MAX}, K={K})]")
    qi = torch.as_tensor(query_idx).reshape(-1).to(device=probs.device, dtype=torch.int64)
    owned = torch.zeros(K, dtype=torch.bool, device=probs.device)
    owned[qi[(qi >= 0) & (qi < K)]] = True
    p = probs.float().masked_fill(~owned.view(K, 1, 1), -1.0)         # below every probability: the unowned classes sort last
    vals, idx = torch.sort(p, dim=0, descending=True, stable=True)
    vals, idx = vals[:k], idx[:k]
    empty = ~owned[idx]
    return idx.to(torch.int32).masked_fill(empty, -1), vals.masked_fill(empty, 0.0).contiguous()


@on_tensor_device
def postprocess_multi(canvases, canvas_hw, query_idx, num_classes: int, logit_scale: float, prob_thd: float, bg_idx: int,
                      out_hw=None, want_probs: bool = True, canvas_offsets=None, flat_labels: bool = False, flat_probs: bool = False):
    """sg_postprocess_multi: N canvases [Q,h,w] in one flat buffer (packed back to back, or at ``canvas_offsets`` elements) ->
    (list of probs [K,H,W] or None, list of labels int64 [1,H,W]); (H, W) = out_hw[n] (default: the canvas size) -- a different size
    is the bilinear resize of sg_resize_bilinear, fused.  ``flat_labels`` adds a third result: the one int64 buffer the label maps
    are views of, images back to back (what sg_confusion_accumulate takes for a whole flush group); ``flat_probs`` (with it and
    ``want_probs``) a fourth: the one f32 buffer the probs are views of, image n at K * (its first pixel)."""
    lib = _lib.load()
    _require_gpu(canvases)
    if canvases.dtype != torch.float32 or not canvases.is_contiguous():
        raise ValueError("postprocess_multi: canvases must be one contiguous f32 buffer")
    dev = canvases.device
    N = len(canvas_hw)
    out_hw = list(canvas_hw) if out_hw is None else [tuple(s) for s in out_hw]
    qi = query_idx.to(device=dev, dtype=torch.int32).contiguous()
    Q, K = int(qi.numel()), int(num_classes)
    if canvas_offsets is None:
        canvas_offsets = [Q * p for p in _prefix(h * w for h, w in canvas_hw)[:-1]]
    pix = _prefix(h * w for h, w in out_hw)
    blocks = _prefix(-(-(h * w) // 256) for h, w in out_hw)
    i32 = torch.tensor([list(hw) for hw in canvas_hw] + [list(hw) for hw in out_hw], dtype=torch.int32).to(dev)
    i64 = torch.tensor(list(canvas_offsets) + pix[:-1] + blocks, dtype=torch.int64).to(dev)
    labels = torch.empty(pix[-1], dtype=torch.int64, device=dev)
    probs = torch.empty(K * pix[-1], dtype=torch.float32, device=dev) if want_probs else None
    check(lib.sg_postprocess_multi(ptr(canvases), ptr(i32), ptr(i64), ptr(i32[N:]), ptr(i64[N:]), ptr(i64[2 * N:]), N, blocks[-1],
                                   canvases.numel(), pix[-1], ptr(qi), Q, K, float(logit_scale), float(prob_thd), int(bg_idx), ptr(probs),
                                   ptr(labels), stream_ptr()), "sg_postprocess_multi")
    lab = flat_views(labels, 1, out_hw)
    prb = flat_views(probs, K, out_hw) if want_probs else [None] * N
    if flat_labels and flat_probs:
        return prb, lab, labels, probs
    return (prb, lab, labels) if flat_labels else (prb, lab)


PAMR_MAX_DILATIONS, PAMR_MAX_DILATION, PAMR_MAX_STEPS = 8, 64, 64        # limits of sg_pamr (csrc/pamr.hip)


def pamr_dilations(dilations):
    """The dilations as (tuple of ints, host int array for the C ABI), checked against the limits the entries state."""
    d = (int(dilations),) if isinstance(dilations, int) else tuple(int(x) for x in dilations)
    if not 1 <= len(d) <= PAMR_MAX_DILATIONS or any(not 1 <= x <= PAMR_MAX_DILATION for x in d):
        raise ValueError(f"pamr: dilations {d!r}: need 1 to {PAMR_MAX_DILATIONS} values, each in [1, {PAMR_MAX_DILATION}]")
    return d, (C.c_int * len(d))(*d)


@on_tensor_device
def scene_planes(scene):
    """u8 [H,W,3] scene -> its normalised f32 planes [3,H,W] (sg_extract_tiles with one whole-scene window): the PAMR guidance of a u8
    scene.  Each value is the plain f32 quotient (float(u) - mean) / std, one rounding in the subtraction and one in the division, which is
    what torch computes from the same bytes.  The tower's ingest (patchify_kernel) holds the same bits wherever the subtraction is exact; in
    channel 2 from u = 233 and channel 0 from u = 251 it corrects the quotient to the nearest f32 and the two may differ in the last bit
    (tests/test_gpu_tiles_reference.py pins both).  A float [3,H,W] scene is its own guidance and is returned as it is."""
    if scene.dtype != torch.uint8:
        return _f32(scene)
    lib = _lib.load()
    scene = scene.contiguous()
    _require_gpu(scene)
    if scene.dim() != 3 or scene.shape[-1] != 3:
        raise ValueError(f"scene_planes: a u8 scene is [H,W,3], got {tuple(scene.shape)}")
    H, W = int(scene.shape[0]), int(scene.shape[1])
    win = torch.tensor([[0, H, 0, W]], dtype=torch.int32, device=scene.device)
    tb = _lib.TileBatch()
    tb.scene, tb.format, tb.scene_h, tb.scene_w, tb.windows = scene.data_ptr(), _lib.IMG_U8_NHWC, H, W, win.data_ptr()
    tb.n_tiles, tb.tile_h, tb.tile_w = 1, H, W
    out = torch.empty(3, H, W, dtype=torch.float32, device=scene.device)
    check(lib.sg_extract_tiles(C.byref(tb), H, W, ptr(out), stream_ptr()), "sg_extract_tiles")
    return out


def _pamr_args(logits, guide):
    _require_gpu(logits, guide)
    if logits.dim() != 3 or guide.dim() != 3 or guide.shape[0] != 3 or tuple(guide.shape[1:]) != tuple(logits.shape[1:]):
        raise ValueError(f"pamr: logits [Q,H,W] and guide [3,H,W] of one size, got {tuple(logits.shape)} and {tuple(guide.shape)}")


@on_tensor_device
def pamr_weights(guide, dilations):
    """sg_pamr_affinity: guide f32 [3,H,W] (the normalised image) -> the PAMR weights [8D,H,W], a softmax over the 8 offsets of each of
    the D dilations (include/segearth_hip.h states the definition)."""
    lib = _lib.load()
    guide = _f32(guide)
    _require_gpu(guide)
    if guide.dim() != 3 or guide.shape[0] != 3:
        raise ValueError(f"pamr_weights: guide is [3,H,W], got {tuple(guide.shape)}")
    d, arr = pamr_dilations(dilations)
    H, W = int(guide.shape[1]), int(guide.shape[2])
    w = torch.empty(8 * len(d), H, W, dtype=torch.float32, device=guide.device)
    check(lib.sg_pamr_affinity(ptr(guide), H, W, arr, len(d), ptr(w), stream_ptr()), "sg_pamr_affinity")
    return w


@on_tensor_device
def pamr_step(weights, logits, dilations):
    """sg_pamr_step: one refinement step, weights [8D,H,W] + logits [Q,H,W] -> new logits [Q,H,W]."""
    lib = _lib.load()
    weights, logits = _f32(weights), _f32(logits)
    _require_gpu(weights, logits)
    d, arr = pamr_dilations(dilations)
    Q, H, W = (int(x) for x in logits.shape)
    if tuple(weights.shape) != (8 * len(d), H, W):
        raise ValueError(f"pamr_step: weights {tuple(weights.shape)} do not fit {len(d)} dilations on logits {tuple(logits.shape)}")
    out = torch.empty_like(logits)
    check(lib.sg_pamr_step(ptr(weights), ptr(logits), ptr(out), Q, H, W, arr, len(d), stream_ptr()), "sg_pamr_step")
    return out


@on_tensor_device
def pamr(logits, guide, steps: int, dilations=(8, 16), inplace: bool = False):
    """sg_pamr: logits [Q,H,W] refined by ``steps`` PAMR steps under guide f32 [3,H,W] (the normalised image at the logits' size).
    Returns a refined copy, or ``logits`` itself, refined where it lies, with ``inplace`` (a contiguous f32 device tensor then).
    ``steps = 0`` returns the input values."""
    lib = _lib.load()
    steps = int(steps)
    if not 0 <= steps <= PAMR_MAX_STEPS:
        raise ValueError(f"pamr: steps={steps} outside [0, {PAMR_MAX_STEPS}]")
    _pamr_args(logits, guide)
    if inplace:
        if logits.dtype != torch.float32 or not logits.is_contiguous():
            raise ValueError("pamr: inplace needs a contiguous f32 tensor")
        out = logits
    else:
        out = _f32(logits).clone()
    guide = _f32(guide)
    d, arr = pamr_dilations(dilations)
    Q, H, W = (int(x) for x in out.shape)
    if steps == 0:
        return out
    buf = scratch(lib.sg_pamr_workspace_bytes(Q, H, W, len(d)), out.device)
    sp, sn = _aligned(buf)
    check(lib.sg_pamr(ptr(guide), ptr(out), Q, H, W, arr, len(d), steps, sp, sn, stream_ptr()), "sg_pamr")
    return out


def _same_pixels(a, b) -> bool:
    """Equal shapes up to leading singleton dimensions ([1,H,W] labels against [H,W] truth; flat buffers against flat buffers)."""
    sa, sb = list(a.shape), list(b.shape)
    while len(sa) > 1 and sa[0] == 1:
        sa.pop(0)
    while len(sb) > 1 and sb[0] == 1:
        sb.pop(0)
    return sa == sb


@on_tensor_device
def confusion_accumulate(labels, gt, table, K: int, ignore_index: int = 255, reduce_zero_label: bool = False):
    """sg_confusion_accumulate on the current stream: adds the confusion counts of (labels, gt) to ``table`` int64 [(K+1),(K+1)] (row =
    prediction, column = ground truth, index K = outside [0,K)) in place and returns it.  labels int64, gt uint8 or int64, of one shape
    up to leading 1s: an image, or the flat label buffer of a flush group.  mmseg's intersect_and_union, counted on the device."""
    lib = _lib.load()
    _require_gpu(labels, gt, table)
    K = int(K)
    if labels.dtype != torch.int64:
        raise TypeError(f"confusion_accumulate: labels must be int64, got {labels.dtype}")
    if gt.dtype not in (torch.uint8, torch.int64):
        raise TypeError(f"confusion_accumulate: gt must be uint8 or int64, got {gt.dtype}")
    if not _same_pixels(labels, gt):
        raise ValueError(f"confusion_accumulate: labels {tuple(labels.shape)} and gt {tuple(gt.shape)} differ in shape")
    if table.dtype != torch.int64 or not table.is_contiguous() or table.numel() != (K + 1) * (K + 1):
        raise ValueError(f"confusion_accumulate: table must be contiguous int64 with {(K + 1) * (K + 1)} elements for K={K}")
    if gt.device != labels.device or table.device != labels.device:
        raise ValueError("confusion_accumulate: labels, gt and table must live on one device")
    if labels.numel() == 0:                # nothing to count; an empty tensor has no storage (a null data pointer, which the entry refuses)
        return table
    labels, gt = labels.contiguous(), gt.contiguous()
    fmt = _lib.GT_U8 if gt.dtype == torch.uint8 else _lib.GT_I64
    check(lib.sg_confusion_accumulate(ptr(labels), ptr(gt), fmt, labels.numel(), K, int(ignore_index), int(bool(reduce_zero_label)),
                                      ptr(table), stream_ptr()), "sg_confusion_accumulate")
    return table


AREA_MAX_K = 4096                                                        # SG_AREA_MAX_K (include/segearth_hip.h)
AREA_SPAN = 4096                                                         # pixels per block of sg_class_area_multi


def area_args(what: str, K: int, bg_idx: int, area_thd=None):
    """The checks every area_thd entry point shares: 0 <= bg_idx < K and, when given, a threshold that is a number >= 0."""
    K, bg_idx = int(K), int(bg_idx)
    if not 0 <= bg_idx < K:
        raise ValueError(f"{what}: area_thd needs 0 <= bg_idx < K (the background class is always kept), got bg_idx={bg_idx}, K={K}")
    if area_thd is not None and not float(area_thd) >= 0.0:
        raise ValueError(f"{what}: area_thd must be a number >= 0 (a share of the non-background pixels), got {area_thd!r}")
    return K, bg_idx


def _i64_labels(what, labels):
    _require_gpu(labels)
    if labels.dtype != torch.int64 or not labels.is_contiguous():
        raise TypeError(f"{what}: labels must be a contiguous int64 tensor, got {labels.dtype}")
    return labels


@on_tensor_device
def class_area(labels, K: int, counts=None):
    """sg_class_area: adds the number of pixels of every class in ``labels`` (int64, any shape; values outside [0,K) are not counted) to
    ``counts`` int64 [K] (default: a zeroed one) and returns it.  Integer counts: byte-identical across repeats."""
    lib = _lib.load()
    labels = _i64_labels("class_area", labels)
    K = int(K)
    if counts is None:
        counts = torch.zeros(max(K, 1), dtype=torch.int64, device=labels.device)
    elif counts.dtype != torch.int64 or not counts.is_contiguous() or counts.numel() != K or counts.device != labels.device:
        raise ValueError(f"class_area: counts must be contiguous int64 [{K}] on the labels' device")
    if labels.numel() == 0 and 1 <= K <= AREA_MAX_K:                     # an empty tensor has no storage (a null pointer, which the entry refuses)
        return counts
    check(lib.sg_class_area(ptr(labels), labels.numel(), K, ptr(counts), stream_ptr()), "sg_class_area")
    return counts


@on_tensor_device
def class_area_multi(labels, image_pixels, K: int):
    """sg_class_area_multi: ``labels`` = the flat int64 label buffer of N images back to back (what ``label_head_multi`` /
    ``postprocess_multi(flat_labels=True)`` return), ``image_pixels`` = their pixel counts -> counts int64 [N,K], one launch."""
    lib = _lib.load()
    labels = _i64_labels("class_area_multi", labels)
    K, N = int(K), len(image_pixels)
    pix = _prefix(image_pixels)
    if N == 0 or any(int(p) <= 0 for p in image_pixels) or pix[-1] != labels.numel():
        raise ValueError(f"class_area_multi: {N} images of {list(image_pixels)} pixels against {labels.numel()} labels")
    blocks = _prefix(-(-int(p) // AREA_SPAN) for p in image_pixels)
    counts = torch.zeros(N, max(K, 1), dtype=torch.int64, device=labels.device)
    i64 = torch.tensor([int(p) for p in image_pixels] + pix[:-1] + blocks, dtype=torch.int64).to(labels.device)
    check(lib.sg_class_area_multi(ptr(labels), ptr(i64), ptr(i64[N:]), ptr(i64[2 * N:]), N, blocks[-1], pix[-1], K, ptr(counts), stream_ptr()),
          "sg_class_area_multi")
    return counts


@on_tensor_device
def area_keep(counts, bg_idx: int, area_thd: float):
    """sg_area_keep: counts int64 [K] or [N,K] -> keep int32 of the same shape: keep[c] = c == bg_idx or area[c] > area_thd * (the sum
    of the non-background areas), compared in double on the device.  Nothing comes to the host."""
    lib = _lib.load()
    _require_gpu(counts)
    if counts.dtype != torch.int64 or not counts.is_contiguous() or counts.dim() not in (1, 2):
        raise ValueError("area_keep: counts must be contiguous int64 [K] or [N,K]")
    K, bg_idx = area_args("area_keep", counts.shape[-1], bg_idx, area_thd)
    keep = torch.empty(counts.shape, dtype=torch.int32, device=counts.device)
    check(lib.sg_area_keep(ptr(counts), counts.numel() // K, K, bg_idx, float(area_thd), ptr(keep), stream_ptr()), "sg_area_keep")
    return keep


def _keep_arg(what, keep, shape, device):
    if keep.dtype != torch.int32 or not keep.is_contiguous() or tuple(keep.shape) != tuple(shape) or keep.device != device:
        raise ValueError(f"{what}: keep must be contiguous int32 {list(shape)} on the device of the other arguments")
    return keep


@on_tensor_device
def area_filter_probs(probs, labels, keep, prob_thd: float, bg_idx: int):
    """sg_area_filter_probs, IN PLACE: probs f32 [K,H,W] get the planes of dropped classes zeroed; labels int64 [1,H,W] or [H,W] hold
    the first-pass labels (the arg-max before prob_thd) on entry and the final labels on return: the kept class of the largest
    probability, ``bg_idx`` below ``prob_thd``.  keep int32 [K] (``area_keep``).  Returns ``labels``."""
    lib = _lib.load()
    _require_gpu(probs)
    if probs.dtype != torch.float32 or not probs.is_contiguous() or probs.dim() != 3:
        raise ValueError("area_filter_probs: probs must be a contiguous f32 [K,H,W] tensor")
    K, H, W = probs.shape
    K, bg_idx = area_args("area_filter_probs", K, bg_idx)
    labels = _i64_labels("area_filter_probs", labels)
    if labels.numel() != H * W or labels.device != probs.device:
        raise ValueError(f"area_filter_probs: labels {tuple(labels.shape)} against probs {tuple(probs.shape)}")
    _keep_arg("area_filter_probs", keep, (K,), probs.device)
    check(lib.sg_area_filter_probs(ptr(probs), ptr(labels), ptr(keep), K, H, W, float(prob_thd), bg_idx, ptr(labels), stream_ptr()),
          "sg_area_filter_probs")
    return labels


@on_tensor_device
def area_filter_probs_multi(probs, labels, keep, out_hw, prob_thd: float, bg_idx: int):
    """sg_area_filter_probs_multi, IN PLACE, on the flat outputs of ``postprocess_multi`` / ``prob_head_multi``: ``labels`` the flat int64
    buffer of N images back to back, ``probs`` the flat f32 buffer with image n's [K,H,W] at K * (its first pixel), keep int32 [N,K],
    out_hw [(H, W)] * N.  One launch.  Returns ``labels``."""
    lib = _lib.load()
    _require_gpu(probs)
    N = len(out_hw)
    labels = _i64_labels("area_filter_probs_multi", labels)
    if N == 0 or keep.dim() != 2:
        raise ValueError("area_filter_probs_multi: keep must be [N,K] for N >= 1 images")
    K, bg_idx = area_args("area_filter_probs_multi", keep.shape[1], bg_idx)
    pix = _prefix(h * w for h, w in out_hw)
    if probs.dtype != torch.float32 or not probs.is_contiguous() or probs.numel() != K * pix[-1] or labels.numel() != pix[-1] or \
            labels.device != probs.device or any(h <= 0 or w <= 0 for h, w in out_hw):
        raise ValueError(f"area_filter_probs_multi: {pix[-1]} pixels of K={K} against {probs.numel()} probabilities and {labels.numel()} labels")
    _keep_arg("area_filter_probs_multi", keep, (N, K), probs.device)
    blocks = _prefix(-(-(h * w) // 256) for h, w in out_hw)
    i32 = torch.tensor([list(hw) for hw in out_hw], dtype=torch.int32).to(probs.device)
    i64 = torch.tensor(pix[:-1] + blocks, dtype=torch.int64).to(probs.device)
    check(lib.sg_area_filter_probs_multi(ptr(probs), ptr(labels), ptr(keep), ptr(i32), ptr(i64), ptr(i64[N:]), N, blocks[-1], pix[-1], K,
                                         float(prob_thd), bg_idx, ptr(labels), stream_ptr()), "sg_area_filter_probs_multi")
    return labels


@on_tensor_device
def area_filter(probs, area_thd: float, prob_thd: float, bg_idx: int):
    """area_thd for a caller who holds class probabilities f32 [K,H,W] of one image: a class that wins less than (or exactly) the share
    ``area_thd`` of the non-background pixels is removed from the image and its pixels go to the best remaining class (the definition:
    include/segearth_hip.h).  -> (probs' [K,H,W] with the dropped planes zeroed, labels int64 [1,H,W], keep int32 [K]); ``probs`` is left
    as it was.  The arg-max of the first pass is taken by the filter kernel itself (every class kept, every pixel undecided), then
    ``class_area`` -> ``area_keep`` -> ``area_filter_probs``; nothing synchronises with the host."""
    _require_gpu(probs)
    if probs.dim() != 3:
        raise ValueError("area_filter: probs must be [K,H,W]")
    K, bg_idx = area_args("area_filter", probs.shape[0], bg_idx, area_thd)
    out = probs.float().contiguous().clone()
    labels = torch.full((1,) + tuple(out.shape[1:]), -1, dtype=torch.int64, device=out.device)
    area_filter_probs(out, labels, torch.ones(K, dtype=torch.int32, device=out.device), float("-inf"), bg_idx)
    keep = area_keep(class_area(labels, K), bg_idx, area_thd)
    area_filter_probs(out, labels, keep, prob_thd, bg_idx)
    return out, labels, keep


@on_tensor_device
def area_relabel(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes: int, logit_scale: float, prob_thd: float,
                 bg_idx: int, keep, conf, labels):
    """sg_area_relabel: the second decision of area_thd on the labels-only route, no canvas and no probability planes.  Arguments as
    ``label_head`` plus keep int32 [K] and the first pass's outputs (``label_head(..., prob_thd=0, want_conf=True)``): conf f32 [H,W] and
    labels int64 [1,H,W], which are rewritten IN PLACE and returned.  Equals ``label_head`` on a ``query_idx`` whose dropped queries are -1."""
    lib = _lib.load()
    dev, lead, qi, hold = _tile_args("area_relabel", tile_logits, windows, up_hw, pad_tl, query_idx)
    H, W = canvas_hw
    K, bg_idx = area_args("area_relabel", num_classes, bg_idx)
    labels = _i64_labels("area_relabel", labels)
    if labels.numel() != H * W or conf.dtype != torch.float32 or not conf.is_contiguous() or conf.numel() != H * W or \
            conf.device != dev or labels.device != dev:
        raise ValueError(f"area_relabel: labels {tuple(labels.shape)} / conf {tuple(conf.shape)} are not the first pass of a {H} x {W} image")
    _keep_arg("area_relabel", keep, (K,), dev)
    check(lib.sg_area_relabel(*lead, H, W, ptr(qi), K, float(logit_scale), float(prob_thd), bg_idx, ptr(keep), ptr(conf), ptr(labels),
                              stream_ptr()), "sg_area_relabel")
    return labels


@on_tensor_device
def area_relabel_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes: int,
                       logit_scale: float, prob_thd: float, bg_idx: int, keep, conf, labels):
    """sg_area_relabel_multi: ``area_relabel`` for the tiles of N images in one launch (arguments as ``label_head_multi``): keep int32
    [N,K]; conf f32 and labels int64 are the flat first-pass buffers of ``label_head_multi(..., prob_thd=0, want_conf=True)``, images
    back to back; labels are rewritten IN PLACE and returned.  Equals ``area_relabel`` per image byte for byte."""
    lib = _lib.load()
    dev, lead, qi, pix, hold = _multi_args("area_relabel_multi", tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx)
    K, bg_idx = area_args("area_relabel_multi", num_classes, bg_idx)
    labels = _i64_labels("area_relabel_multi", labels)
    if labels.numel() != pix[-1] or conf.dtype != torch.float32 or not conf.is_contiguous() or conf.numel() != pix[-1] or \
            conf.device != dev or labels.device != dev:
        raise ValueError(f"area_relabel_multi: labels / conf are not the flat first pass of {pix[-1]} pixels")
    _keep_arg("area_relabel_multi", keep, (len(image_hw), K), dev)
    check(lib.sg_area_relabel_multi(*lead, pix[-1], ptr(qi), K, float(logit_scale), float(prob_thd), bg_idx, ptr(keep), ptr(conf), ptr(labels),
                                    stream_ptr()), "sg_area_relabel_multi")
    return labels


@on_tensor_device
def render_maps(labels, probs, palette, want_mask: bool = True, want_heat: bool = True):
    """labels int64 [1,H,W] or [H,W], probs [K,H,W], palette uint8 [K,3] -> (mask uint8 [H,W,3] | None, heat uint8 [H,W,3] | None)."""
    lib = _lib.load()
    labels = labels.reshape(labels.shape[-2], labels.shape[-1]).contiguous()
    _require_gpu(labels, probs)
    H, W = labels.shape
    K = int(palette.shape[0])
    pal = palette.to(device=labels.device, dtype=torch.uint8).contiguous()
    probs = None if probs is None else _f32(probs)
    mask = torch.empty(H, W, 3, dtype=torch.uint8, device=labels.device) if want_mask else None
    heat = torch.empty(H, W, 3, dtype=torch.uint8, device=labels.device) if want_heat else None
    check(lib.sg_render_maps(ptr(labels), ptr(probs), ptr(pal), K, H, W, ptr(mask), ptr(heat), stream_ptr()), "sg_render_maps")
    return mask, heat


@on_tensor_device
def adaptive_conv(inp, filters):
    """FeatUp AdaptiveConv.apply: inp [B,C,h+d-1,w+d-1], filters [B,h,w,d,d] -> [B,C,h,w]."""
    lib = _lib.load()
    inp, filters = _f32(inp), _f32(filters)
    _require_gpu(inp, filters)
    B, Cc = inp.shape[:2]
    _, h, w, d, _ = filters.shape
    out = torch.empty(B, Cc, h, w, dtype=torch.float32, device=inp.device)
    check(lib.sg_adaptive_conv(ptr(inp), ptr(filters), B, Cc, h, w, d, ptr(out), stream_ptr()), "sg_adaptive_conv")
    return out


@on_tensor_device
def cross_tile_fusion(tokens, hg: int, wg: int, gh: int, gw: int, boundary_width: int = 2, fusion_mode: str = "weighted",
                      fusion_strength: float = 0.3):
    """tokens [hg*wg, gh*gw, C] (tiles in raster order) -> fused copy (reference cross_tile_fusion.py, B=1 tile-by-tile semantics)."""
    lib = _lib.load()
    tokens = _f32(tokens).clone()
    _require_gpu(tokens)
    T, n, Cc = tokens.shape
    assert T == hg * wg and n == gh * gw
    buf = scratch(lib.sg_cross_tile_scratch_bytes(T, gh, gw, Cc, boundary_width), tokens.device)
    sp, _ = _aligned(buf)
    check(lib.sg_cross_tile_fusion(ptr(tokens), hg, wg, gh, gw, Cc, boundary_width, 0 if fusion_mode == "weighted" else 1,
                                   float(fusion_strength), sp, stream_ptr()), "sg_cross_tile_fusion")
    return tokens


@on_tensor_device
def global_debias(tokens, cls, factor: float):
    """tokens - cls_hat * (cos(tokens, cls_hat) * factor)  (segmentor.py:322-336); cls is normalised inside."""
    lib = _lib.load()
    tokens, cls = _f32(tokens), _f32(cls)
    _require_gpu(tokens, cls)
    B, n, E = tokens.shape
    out = torch.empty_like(tokens)
    check(lib.sg_global_debias(ptr(tokens), ptr(cls), B, n, E, float(factor), ptr(out), stream_ptr()), "sg_global_debias")
    return out


@on_tensor_device
def ctd_debias(tokens, cls, eps: float = 1.1, min_samples: int = 11, factor: float = -1.5, want_labels: bool = True, normalize_cls: bool = False):
    """Cluster-Then-Debias (segmentor.py:339-365): tokens [B,n,C], CLS features [B,C] (unit unless ``normalize_cls``) ->
    (debiased copy, labels int32 [B,n])."""
    lib = _lib.load()
    tokens = _f32(tokens).clone()
    cls = _f32(cls)
    _require_gpu(tokens, cls)
    B, n, Cc = tokens.shape
    labels = torch.empty(B, n, dtype=torch.int32, device=tokens.device) if want_labels else None
    need = lib.sg_ctd_scratch_bytes(B, n, Cc)
    buf = scratch(need, tokens.device)
    sp, sn = _aligned(buf)
    check(lib.sg_ctd_debias(ptr(tokens), ptr(cls), B, n, Cc, float(eps), int(min_samples), float(factor), int(normalize_cls), ptr(labels), sp, sn,
                            stream_ptr()), "sg_ctd_debias")
    return tokens, labels


class CrossTileSteps:
    """The three device steps of the sharded cross-tile fusion (sg_cross_tile_pack / _fuse / _apply) for a rank holding tiles
    [tile0, tile0+n_local) of a scene whose tile grid is ``wg`` wide.  ``pipeline.sharded_cross_tile_fusion`` drives them and
    does the two strip all-gathers in between; the CPU tests replace this class with a torch stand-in."""

    def __init__(self, gh: int, gw: int, C_: int, boundary_width: int, fusion_mode: str, fusion_strength: float, wg: int):
        self.lib = _lib.load()
        self.gh, self.gw, self.C, self.bw, self.wg = gh, gw, C_, boundary_width, wg
        self.mode = 0 if fusion_mode == "weighted" else 1
        self.strength = float(fusion_strength)

    def strip_len(self, which: int) -> int:
        return self.gh * self.bw if which == 0 else self.bw * self.gw

    @on_tensor_device
    def pack(self, tokens, tile0: int, which: int, left_result=None):
        _require_gpu(tokens, left_result)
        out = torch.empty(tokens.shape[0], self.strip_len(which), self.C, dtype=torch.float32, device=tokens.device)
        check(self.lib.sg_cross_tile_pack(ptr(tokens), ptr(left_result), tokens.shape[0], tile0, self.wg, self.gh, self.gw, self.C, self.bw,
                                          which, ptr(out), stream_ptr()), "sg_cross_tile_pack")
        return out

    @on_tensor_device
    def fuse(self, tokens, tile0: int, nbr_strips, which: int):
        _require_gpu(tokens, nbr_strips)
        res = torch.zeros(tokens.shape[0], self.strip_len(which), self.C, dtype=torch.float32, device=tokens.device)
        check(self.lib.sg_cross_tile_fuse(ptr(tokens), ptr(nbr_strips), tokens.shape[0], tile0, self.wg, self.gh, self.gw, self.C, self.bw,
                                          self.mode, self.strength, which, ptr(res), stream_ptr()), "sg_cross_tile_fuse")
        return res

    @on_tensor_device
    def apply(self, tokens, tile0: int, left_result, top_result):
        _require_gpu(tokens, left_result, top_result)
        check(self.lib.sg_cross_tile_apply(ptr(tokens), ptr(left_result), ptr(top_result), tokens.shape[0], tile0, self.wg, self.gh, self.gw,
                                           self.C, self.bw, stream_ptr()), "sg_cross_tile_apply")
        return tokens


SIEVE_FILLS = {"bg": 0, "neighbour": 1}                                  # SG_SIEVE_FILL_* (include/segearth_hip.h)
SIEVE_MAX_PIXELS = (1 << 31) - 1                                         # per image: region roots are 32-bit raster indices


def sieve_args(min_region, connectivity=4, fill="neighbour"):
    """The checks of the min_region options, shared by ``sieve`` and the constructors: min_region an integer >= 1, connectivity 4 or
    8, fill "bg" or "neighbour" -> (min_region, connectivity, fill)."""
    if isinstance(min_region, bool) or not isinstance(min_region, int) or min_region < 1:
        raise ValueError(f"min_region must be an integer >= 1 (a region is small when its area is below it), got {min_region!r}")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"region connectivity must be 4 or 8, got {connectivity!r}")
    if fill not in SIEVE_FILLS:
        raise ValueError(f"region fill must be one of {tuple(SIEVE_FILLS)}, got {fill!r}")
    return int(min_region), int(connectivity), fill


@on_tensor_device
def sieve_flat(labels, image_hw, min_region, connectivity=4, fill="neighbour", bg_idx=0, out=None):
    """sg_sieve on a flat int64 buffer that holds N label maps back to back (what the multi-image heads return), sizes ``image_hw``:
    one call, one launch sequence per 64 images.  In place unless ``out`` (a flat int64 buffer of the same size) is given; returns the
    buffer that was written.  Nothing synchronises with the host."""
    lib = _lib.load()
    min_region, connectivity, fill = sieve_args(min_region, connectivity, fill)
    labels = _i64_labels("sieve", labels)
    image_hw = [(int(h), int(w)) for h, w in image_hw]
    pix = _prefix(h * w for h, w in image_hw)
    if not image_hw or any(h <= 0 or w <= 0 for h, w in image_hw) or pix[-1] != labels.numel():
        raise ValueError(f"sieve: {len(image_hw)} images of sizes {image_hw} against {labels.numel()} labels")
    if any(h * w > SIEVE_MAX_PIXELS for h, w in image_hw):
        raise ValueError(f"sieve: an image of 2^31 or more pixels is not supported (region roots are 32-bit raster indices), got {image_hw}")
    if out is None:
        out = labels
    elif out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != labels.numel() or out.device != labels.device:
        raise ValueError("sieve: out must be a contiguous int64 tensor of the labels' size on the labels' device")
    N = len(image_hw)
    hw = (C.c_int32 * (2 * N))(*[v for s in image_hw for v in s])
    off = (C.c_int64 * N)(*pix[:-1])
    nbytes = int(lib.sg_sieve_workspace_bytes(pix[-1], SIEVE_FILLS[fill]))
    buf = scratch(nbytes, labels.device)
    wp, wn = _aligned(buf)
    check(lib.sg_sieve(ptr(labels), ptr(out), hw, off, N, min_region, connectivity, SIEVE_FILLS[fill], int(bg_idx), wp, wn, stream_ptr()),
          "sg_sieve")
    return out


def sieve(labels, min_region, connectivity=4, fill="neighbour", bg_idx=0, out=None):
    """Sieve the connected regions of fewer than ``min_region`` pixels out of a label map (the definition: sg_sieve in
    include/segearth_hip.h).  ``labels``: int64 [H,W] or [1,H,W] on the device, or a list of such maps of any sizes -- a list is packed
    into one flat buffer and served by one sg_sieve call.  ``fill="bg"``: a small region that is not background becomes ``bg_idx``
    (remove_small_objects); ``fill="neighbour"``: every small region takes the label of its largest adjacent kept region, ties to the
    smaller root, ``bg_idx`` when there is none (one pass, not iterated to a fixed point).  Returns new tensors of the same shapes, or
    writes ``out`` (same shapes; ``out=labels`` sieves in place) and returns it."""
    many = isinstance(labels, (list, tuple))
    maps = list(labels) if many else [labels]
    outs = None if out is None else (list(out) if many else [out])
    if not maps or (outs is not None and len(outs) != len(maps)):
        raise ValueError("sieve: needs at least one label map, and one out per map")
    for m in maps:
        if not torch.is_tensor(m) or m.dim() not in (2, 3) or (m.dim() == 3 and m.shape[0] != 1) or m.numel() == 0:
            raise ValueError("sieve: a label map must be a non-empty int64 [H,W] or [1,H,W] tensor")
        _i64_labels("sieve", m)
    hw = [tuple(m.shape[-2:]) for m in maps]
    if len(maps) == 1:
        dst = outs[0] if outs is not None else torch.empty_like(maps[0])
        if tuple(dst.shape) != tuple(maps[0].shape):
            raise ValueError(f"sieve: out {tuple(dst.shape)} against labels {tuple(maps[0].shape)}")
        sieve_flat(maps[0].reshape(-1), hw, min_region, connectivity, fill, bg_idx, out=dst.reshape(-1) if dst.is_contiguous() else dst)
        return [dst] if many else dst
    flat = sieve_flat(torch.cat([m.reshape(-1) for m in maps]), hw, min_region, connectivity, fill, bg_idx)
    res = [v.view(m.shape) for v, m in zip(flat_views(flat, 1, hw), maps)]
    if outs is None:
        return res
    for o, r in zip(outs, res):
        o.copy_(r)
    return outs


# ---- the region table (sg_regions; the definition: include/segearth_hip.h) ------------------------------------------------------------------
REGION_COLUMNS = {"image": 0, "root": 1, "label": 2, "area": 3, "y0": 4, "x0": 5, "y1": 6, "x1": 7, "sum_y": 8, "sum_x": 9, "score_q": 10}    # SG_REGION_*
REGION_FIELDS = 12                                                       # SG_REGION_FIELDS
REGION_SCORE_ONE = 1 << 24                                               # q(1.0)
REGIONS_BLOCK_PIXELS = 2048                                              # SG_REGIONS_BLOCK_PIXELS
REGIONS_SCAN_BLOCKS = 1024                                               # SG_REGIONS_SCAN_BLOCKS
REGIONS_FIRST_ROWS = 1 << 18                                             # max_regions=None: the rows of the first call
REGIONS_MAX_PIXELS = (1 << 31) - 1                                       # per call: row indices are 32-bit


def regions_args(connectivity=4, min_area=1, skip_label=None, max_regions=None):
    """The checks of the region-table options: connectivity 4 or 8, min_area an integer >= 1, skip_label None or an integer, max_regions
    None or an integer >= 1 -> the four as given."""
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"regions: connectivity must be 4 or 8, got {connectivity!r}")
    if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 1:
        raise ValueError(f"regions: min_area must be an integer >= 1 (a region is listed when its area is at least it), got {min_area!r}")
    if skip_label is not None and (isinstance(skip_label, bool) or not isinstance(skip_label, int)):
        raise ValueError(f"regions: skip_label must be None or an integer label, got {skip_label!r}")
    if max_regions is not None and (isinstance(max_regions, bool) or not isinstance(max_regions, int) or max_regions < 1):
        raise ValueError(f"regions: max_regions must be None or an integer >= 1, got {max_regions!r}")
    return int(connectivity), int(min_area), skip_label, max_regions


@on_tensor_device
def regions_table(labels, image_hw, conf, connectivity, min_area, skip_label, max_regions, table, region_of=None):
    """One sg_regions call, raw: ``labels`` flat int64, ``conf`` flat f32 or None, ``table`` int64 [>= max_regions, 12] written in place
    (rows beyond the listed regions keep their bytes), ``region_of`` flat int32 or None -> counts int64 [N+1] on the device.  Nothing
    synchronises with the host."""
    lib = _lib.load()
    N = len(image_hw)
    pix = _prefix(h * w for h, w in image_hw)
    hw = (C.c_int32 * (2 * N))(*[v for s in image_hw for v in s])
    off = (C.c_int64 * N)(*pix[:-1])
    counts = torch.empty(N + 1, dtype=torch.int64, device=labels.device)
    buf = scratch(int(lib.sg_regions_workspace_bytes(pix[-1], max_regions)), labels.device)
    wp, wn = _aligned(buf)
    check(lib.sg_regions(ptr(labels), ptr(conf), hw, off, N, connectivity, min_area, 0 if skip_label is None else int(skip_label),
                         int(skip_label is not None), max_regions, ptr(table), ptr(region_of), ptr(counts), wp, wn, stream_ptr()), "sg_regions")
    return counts


def regions_flat(labels, image_hw, conf=None, connectivity=4, min_area=1, skip_label=None, max_regions=None, want_map=False):
    """The region table of N label maps that lie back to back in one flat int64 buffer (what the multi-image heads return), sizes
    ``image_hw``; ``conf``: None or an f32 buffer of the same layout.  See ``regions`` for the options and the result; ``region_of`` is
    one int32 [H,W] view per image."""
    connectivity, min_area, skip_label, max_regions = regions_args(connectivity, min_area, skip_label, max_regions)
    labels = _i64_labels("regions", labels)
    image_hw = [(int(h), int(w)) for h, w in image_hw]
    total_pix = sum(h * w for h, w in image_hw)
    if not image_hw or any(h <= 0 or w <= 0 for h, w in image_hw) or total_pix != labels.numel():
        raise ValueError(f"regions: {len(image_hw)} images of sizes {image_hw} against {labels.numel()} labels")
    if total_pix > REGIONS_MAX_PIXELS:
        raise ValueError(f"regions: 2^31 or more pixels in one call are not supported (row indices are 32-bit), got {total_pix}")
    if conf is not None:
        _require_gpu(conf)
        if conf.dtype != torch.float32 or not conf.is_contiguous() or conf.numel() != labels.numel() or conf.device != labels.device:
            raise ValueError("regions: conf must be a contiguous f32 tensor of the labels' size on the labels' device")
    N = len(image_hw)
    rows = min(total_pix, REGIONS_FIRST_ROWS) if max_regions is None else max_regions
    region_of = torch.empty(total_pix, dtype=torch.int32, device=labels.device) if want_map else None
    table = torch.empty(rows, REGION_FIELDS, dtype=torch.int64, device=labels.device)
    counts = regions_table(labels.view(-1), image_hw, conf, connectivity, min_area, skip_label, rows, table, region_of).cpu()   # THE host read
    total = int(counts[N])
    if total > rows and max_regions is None:                                 # too few rows on the first call: once more with the exact number
        rows = total
        table = torch.empty(rows, REGION_FIELDS, dtype=torch.int64, device=labels.device)
        regions_table(labels.view(-1), image_hw, conf, connectivity, min_area, skip_label, rows, table, region_of)
    t = table[:min(total, rows)]
    col = REGION_COLUMNS
    area = t[:, col["area"]]
    out = {k: t[:, col[k]] for k in ("image", "root", "label", "area")}
    out["bbox"] = t[:, col["y0"]:col["x1"] + 1]
    out["centroid"] = t[:, col["sum_y"]:col["sum_x"] + 1].double() / area.double()[:, None]
    out["score"] = None if conf is None else t[:, col["score_q"]].double() / float(REGION_SCORE_ONE) / area.double()
    out["score_q"] = None if conf is None else t[:, col["score_q"]]
    out["counts"] = counts[:N].to(labels.device)
    out["counts_host"] = counts[:N]                                          # what was read: a caller that splits the rows needs no second read
    if total > rows:
        out["truncated"] = True
    if want_map:
        out["region_of"] = [v[0] for v in flat_views(region_of, 1, image_hw)]
    return out


def label_confidence(probs, labels):
    """probs f32 [K,H,W], labels int64 [1,H,W] -> f32 [1,H,W]: the probability of each pixel's label; 0 where the label is no class plane
    (outside [0, K)).  Plain torch: what ``predict_regions(with_score=True)`` hands to sg_regions as ``conf``."""
    K = probs.shape[0]
    inside = (labels >= 0) & (labels < K)
    return torch.where(inside, probs.gather(0, labels.clamp(0, K - 1)), torch.zeros((), device=probs.device, dtype=probs.dtype)).float()


def regions(labels, conf=None, connectivity=4, min_area=1, skip_label=None, max_regions=None, want_map=False):
    """List the connected regions of a label map (the definition: sg_regions in include/segearth_hip.h; regions, roots and connectivity
    are those of ``sieve``).  ``labels``: int64 [H,W] or [1,H,W] on the device, or a list of such maps of any sizes -- a list is packed
    into one flat buffer and served by one sg_regions call; ``conf``: None, or f32 of the labels' shape(s), a per-pixel confidence.
    A region is listed when it has at least ``min_area`` pixels and its label is not ``skip_label``; the rows are ordered by (image,
    root).  Returns a dict of device tensors over the R listed regions: ``image``, ``root``, ``label``, ``area`` int64 [R]; ``bbox``
    int64 [R,4] (y0, x0, y1, x1), half-open; ``centroid`` float64 [R,2] (y, x); ``score`` float64 [R], the region's mean clamp(conf, 0,
    1) from the exact integer sum ``score_q`` of conf in steps of 2^-24 (both None without ``conf``); ``counts`` int64 [N], the regions
    per image (``counts_host``: the same on the host, as it was read); with ``want_map`` ``region_of``, per map an int32 [H,W] of each pixel's row (-1: not listed).
    ``max_regions=None`` starts with min(pixels, 2^18) rows and calls once more with the exact total if those were too few; an explicit
    ``max_regions`` truncates the table to its first rows (``counts`` and ``region_of`` stay uncapped) and adds ``truncated=True``.
    The one host read is ``counts`` after the call, to slice the table."""
    many = isinstance(labels, (list, tuple))
    maps = list(labels) if many else [labels]
    confs = None if conf is None else (list(conf) if many else [conf])
    if not maps or (confs is not None and len(confs) != len(maps)):
        raise ValueError("regions: needs at least one label map, and one conf per map")
    for m in maps:
        if not torch.is_tensor(m) or m.dim() not in (2, 3) or (m.dim() == 3 and m.shape[0] != 1) or m.numel() == 0:
            raise ValueError("regions: a label map must be a non-empty int64 [H,W] or [1,H,W] tensor")
        _i64_labels("regions", m)
    if confs is not None and any(not torch.is_tensor(c) or c.numel() != m.numel() or c.dtype != torch.float32 for c, m in zip(confs, maps)):
        raise ValueError("regions: conf must be f32 of the labels' shape")
    hw = [tuple(m.shape[-2:]) for m in maps]
    flat = maps[0].reshape(-1) if len(maps) == 1 else torch.cat([m.reshape(-1) for m in maps])
    cflat = None if confs is None else (confs[0].contiguous().reshape(-1) if len(maps) == 1 else torch.cat([c.reshape(-1) for c in confs]))
    out = regions_flat(flat, hw, cflat, connectivity, min_area, skip_label, max_regions, want_map)
    if want_map and not many:
        out["region_of"] = out["region_of"][0]
    return out


# ---- What the entries that count flat buffers image by image share (boundary, tolerant, object matching) ------------------------------------
CONFUSION_MAX_K = 127                                                    # the cap of sg_confusion_accumulate: one metric object holds its table too
_MAX_PIXELS = (1 << 31) - 1                                              # pixel indices are 32-bit on the device


def _image_sizes(who: str, image_hw, per_call: bool):
    """Sizes of the images of a call as int pairs: at least one, all positive, below 2^31 pixels each or (``per_call``) together."""
    image_hw = [(int(h), int(w)) for h, w in image_hw]
    if not image_hw or any(h <= 0 or w <= 0 for h, w in image_hw):
        raise ValueError(f"{who}: needs at least one image of positive size, got {image_hw}")
    if per_call and sum(h * w for h, w in image_hw) > _MAX_PIXELS:
        raise ValueError(f"{who}: 2^31 or more pixels in one call are not supported (region roots are 32-bit)")
    if not per_call and any(h * w > _MAX_PIXELS for h, w in image_hw):
        raise ValueError(f"{who}: an image of 2^31 or more pixels is not supported, got {image_hw}")
    return image_hw


def _per_image_ints(who: str, values, n_images: int, lo: int, hi: int, plural: str, name: str):
    """One value for every image or one per image, integers in [lo, hi] -> the list of ``n_images`` values."""
    vs = list(values) if isinstance(values, (list, tuple)) else [values] * n_images
    if len(vs) != n_images:
        raise ValueError(f"{who}: {len(vs)} {plural} for {n_images} images")
    for v in vs:
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{who}: {name} must be an integer in [{lo}, {hi}], got {v!r}")
    return vs


def _image_arrays(image_hw):
    """The C arrays of N images that lie back to back -> (N, prefix sums of their pixels, int32 [2N] sizes, int64 [N] pixel offsets)."""
    N = len(image_hw)
    pix = _prefix(h * w for h, w in image_hw)
    return N, pix, (C.c_int32 * (2 * N))(*[v for s in image_hw for v in s]), (C.c_int64 * N)(*pix[:-1])


def _flat_call(who: str, labels, gt, image_hw, K: int, table, table_name: str, rows: int, extra=None, extra_name: Optional[str] = None):
    """The checks of a call on the flat int64 labels and uint8 / int64 truth of the images ``image_hw`` (already checked) that adds to
    the int64 ``table`` [rows, K], in the order the callers refuse: K, the dtypes, the pixels against the sizes, the table, ``extra``
    (None, or a uint8 buffer of one byte per pixel: object_match's match_map), the device.  Nothing here touches the library
    -> (contiguous flat labels, contiguous flat truth, N, pixels of the call, sizes array, offsets array, ground-truth format code)."""
    if not 1 <= K <= CONFUSION_MAX_K:
        raise ValueError(f"{who}: K={K} outside [1, {CONFUSION_MAX_K}] (the cap of sg_confusion_accumulate)")
    if not torch.is_tensor(labels) or labels.dtype != torch.int64:
        raise TypeError(f"{who}: labels must be an int64 tensor")
    if not torch.is_tensor(gt) or gt.dtype not in (torch.uint8, torch.int64):
        raise TypeError(f"{who}: gt must be a uint8 or int64 tensor")
    N, pix, hw, off = _image_arrays(image_hw)
    if labels.numel() != pix[-1] or gt.numel() != pix[-1]:
        raise ValueError(f"{who}: {N} images of sizes {image_hw} against {labels.numel()} labels and {gt.numel()} truth pixels")
    if not torch.is_tensor(table) or table.dtype != torch.int64 or not table.is_contiguous() or table.numel() != rows * K:
        raise ValueError(f"{who}: {table_name} must be contiguous int64 with {rows * K} elements for K={K}")
    if extra is not None and (not torch.is_tensor(extra) or extra.dtype != torch.uint8 or not extra.is_contiguous() or extra.numel() != pix[-1]):
        raise ValueError(f"{who}: {extra_name} must be a contiguous uint8 tensor of {pix[-1]} elements")
    _require_gpu(labels, gt, table)
    if gt.device != labels.device or table.device != labels.device or (extra is not None and extra.device != labels.device):
        names = f"labels, gt and {table_name}" if extra_name is None else f"labels, gt, {table_name} and {extra_name}"
        raise ValueError(f"{who}: {names} must live on one device")
    fmt = _lib.GT_U8 if gt.dtype == torch.uint8 else _lib.GT_I64
    return labels.contiguous().view(-1), gt.contiguous().view(-1), N, pix[-1], hw, off, fmt


# ---- Boundary IoU (sg_boundary_band / sg_boundary_accumulate; the definition: include/segearth_hip.h) --------------------------------------
BOUNDARY_MAX_D = 4095                                                    # the widest band the entries take
BOUNDARY_MAX_K = CONFUSION_MAX_K
BOUNDARY_MAX_PIXELS = _MAX_PIXELS                                        # per image


def boundary_width(hw, ratio=0.02):
    """The band width of an image of size ``hw`` = (H, W): d = max(1, int(round(ratio * sqrt(H*H + W*W)))), host arithmetic in double
    with Python's round, as in the official Boundary IoU code (ratio 0.02 of the diagonal: 14 px on a 512 tile, 101 px on 2048 x 4608)."""
    import math
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not (ratio > 0) or not math.isfinite(ratio):
        raise ValueError(f"boundary_ratio must be a finite number > 0 (a share of the image diagonal), got {ratio!r}")
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1:
        raise ValueError(f"boundary_width: an image of size {h} x {w}")
    d = max(1, int(round(float(ratio) * math.sqrt(h * h + w * w))))
    if d > BOUNDARY_MAX_D:
        raise ValueError(f"boundary_width: ratio {ratio} of the diagonal of {h} x {w} is {d} px, above the limit of {BOUNDARY_MAX_D}")
    return d


def boundary_args(image_hw, d):
    """The checks of the boundary entries, before any library call: sizes positive and below 2^31 pixels per image, every width an
    integer in [1, 4095]; one width serves every image -> (image_hw, widths)."""
    image_hw = _image_sizes("boundary", image_hw, per_call=False)
    return image_hw, _per_image_ints("boundary", d, len(image_hw), 1, BOUNDARY_MAX_D, "widths", "the band width d")


@on_tensor_device
def boundary_band_flat(labels, image_hw, d):
    """sg_boundary_band on a flat int64 or uint8 buffer that holds N label maps back to back, sizes ``image_hw``, widths ``d`` (one
    integer, or one per image) -> the flat uint8 band buffer, 0 / 1.  One call; nothing synchronises with the host."""
    image_hw, ds = boundary_args(image_hw, d)
    if not torch.is_tensor(labels) or labels.dtype not in (torch.int64, torch.uint8) or not labels.is_contiguous():
        raise TypeError("boundary_band: labels must be a contiguous int64 or uint8 tensor")
    N, pix, hw, off = _image_arrays(image_hw)
    if pix[-1] != labels.numel():
        raise ValueError(f"boundary_band: {N} images of sizes {image_hw} against {labels.numel()} labels")
    _require_gpu(labels)
    lib = _lib.load()
    band = torch.empty(labels.numel(), dtype=torch.uint8, device=labels.device)
    buf = scratch(int(lib.sg_boundary_workspace_bytes(pix[-1])) // 4, labels.device)
    wp, wn = _aligned(buf)
    fmt = _lib.GT_U8 if labels.dtype == torch.uint8 else _lib.GT_I64
    check(lib.sg_boundary_band(ptr(labels), fmt, hw, off, (C.c_int32 * N)(*ds), N, ptr(band), wp, wn, stream_ptr()), "sg_boundary_band")
    return band


def boundary_band(labels, d):
    """The boundary band of a label map (the definition: sg_boundary_band in include/segearth_hip.h): 1 where the (2d+1) x (2d+1) window
    around a pixel leaves the image or holds another label -- for every class at once the pixels of its mask within ``d`` of its contour.
    ``labels``: int64 or uint8 [H,W] or [1,H,W] on the device, or a list of such maps of any sizes (one dtype) -- a list is packed into
    one flat buffer and served by one call; ``d`` one integer or one per map.  Returns uint8 maps of the same shapes."""
    many = isinstance(labels, (list, tuple))
    maps = list(labels) if many else [labels]
    if not maps:
        raise ValueError("boundary_band: needs at least one label map")
    for m in maps:
        if not torch.is_tensor(m) or m.dim() not in (2, 3) or (m.dim() == 3 and m.shape[0] != 1) or m.numel() == 0:
            raise ValueError("boundary_band: a label map must be a non-empty int64 or uint8 [H,W] or [1,H,W] tensor")
        if m.dtype != maps[0].dtype or m.dtype not in (torch.int64, torch.uint8):
            raise TypeError(f"boundary_band: label maps must all be int64 or all uint8, got {m.dtype}")
    hw = [tuple(m.shape[-2:]) for m in maps]
    boundary_args(hw, d)
    flat = maps[0].reshape(-1).contiguous() if len(maps) == 1 else torch.cat([m.reshape(-1) for m in maps])
    band = boundary_band_flat(flat, hw, d)
    res = [v.view(m.shape) for v, m in zip(flat_views(band, 1, hw), maps)]
    return res if many else res[0]


@on_tensor_device
def boundary_accumulate(labels_flat, gt_flat, image_hw, d, areas, K: int, ignore_index: int = 255, reduce_zero_label: bool = False):
    """sg_boundary_accumulate on the current stream: the bands of the predictions and of the (transformed) truth of N images that lie
    back to back in ``labels_flat`` (int64) and ``gt_flat`` (uint8 or int64), sizes ``image_hw``, widths ``d`` (one integer or one per
    image); the band-restricted counts are ADDED to ``areas`` int64 [3,K] (intersection, prediction band, truth band), which is
    returned.  Nothing comes back to the host."""
    image_hw, ds = boundary_args(image_hw, d)
    K = int(K)
    labels_flat, gt_flat, N, total, hw, off, fmt = _flat_call("boundary_accumulate", labels_flat, gt_flat, image_hw, K, areas, "areas", 3)
    lib = _lib.load()
    buf = scratch(int(lib.sg_boundary_workspace_bytes(total)), labels_flat.device)
    wp, wn = _aligned(buf)
    check(lib.sg_boundary_accumulate(ptr(labels_flat), ptr(gt_flat), fmt, hw, off, (C.c_int32 * N)(*ds), N, K, int(ignore_index),
                                     int(bool(reduce_zero_label)), ptr(areas), wp, wn, stream_ptr()), "sg_boundary_accumulate")
    return areas


# ---- Tolerant matching: relaxed precision / recall and the boundary F-score (sg_tolerant_accumulate; the definition: include/segearth_hip.h) --
TOLERANT_MAX_SQ = 254 * 254                                              # the largest squared tolerance: a radius of 254 px
TOLERANT_MAX_K = CONFUSION_MAX_K
TOLERANT_MODES = {"region": _lib.TOL_REGION, "contour": _lib.TOL_CONTOUR}


def tolerance_sq(hw, ratio=0.0075):
    """The squared tolerance of an image of size ``hw`` = (H, W): r = max(1, ceil(ratio * sqrt(H*H + W*W))), tol_sq = r*r, host
    arithmetic in double (ratio 0.0075 of the diagonal, the boundary F-measure's: 6 px on a 512 tile, 38 px on 2048 x 4608)."""
    import math
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not (ratio > 0) or not math.isfinite(ratio):
        raise ValueError(f"tolerance_ratio must be a finite number > 0 (a share of the image diagonal), got {ratio!r}")
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1:
        raise ValueError(f"tolerance_sq: an image of size {h} x {w}")
    r = max(1, int(math.ceil(float(ratio) * math.sqrt(h * h + w * w))))
    if r * r > TOLERANT_MAX_SQ:
        raise ValueError(f"tolerance_sq: ratio {ratio} of the diagonal of {h} x {w} is {r} px, above the limit of 254 (distances are "
                         "kept in one byte)")
    return r * r


def tolerant_args(image_hw, tol_sq, mode):
    """The checks of sg_tolerant_accumulate, before any library call: sizes positive and below 2^31 pixels per image, every squared
    tolerance an integer in [0, 254^2] (one serves every image), a known mode -> (image_hw, tolerances, mode code)."""
    if mode not in TOLERANT_MODES:
        raise ValueError(f"tolerant: mode must be one of {sorted(TOLERANT_MODES)}, got {mode!r}")
    image_hw = _image_sizes("tolerant", image_hw, per_call=False)
    ts = _per_image_ints("tolerant", tol_sq, len(image_hw), 0, TOLERANT_MAX_SQ, "tolerances", "the squared tolerance tol_sq")
    return image_hw, ts, TOLERANT_MODES[mode]


@on_tensor_device
def tolerant_accumulate(labels_flat, gt_flat, image_hw, tol_sq, counts, K: int, ignore_index: int = 255, reduce_zero_label: bool = False,
                        mode: str = "region"):
    """sg_tolerant_accumulate on the current stream: per class, the marked pixels (``mode`` "region": all; "contour": the class
    outlines) of the predictions that have a marked pixel of the same class of the (transformed) truth within sqrt(``tol_sq``) pixels,
    and the other way round, over N images that lie back to back in ``labels_flat`` (int64) and ``gt_flat`` (uint8 or int64), sizes
    ``image_hw``, squared tolerances ``tol_sq`` (one integer or one per image).  The counts are ADDED to ``counts`` int64 [4,K]
    (predicted, predicted and right, true, true and found), which is returned.  Nothing comes back to the host."""
    image_hw, ts, mode_code = tolerant_args(image_hw, tol_sq, mode)
    K = int(K)
    labels_flat, gt_flat, N, total, hw, off, fmt = _flat_call("tolerant_accumulate", labels_flat, gt_flat, image_hw, K, counts, "counts", 4)
    lib = _lib.load()
    buf = scratch(int(lib.sg_tolerant_workspace_bytes(total, K)), labels_flat.device)
    wp, wn = _aligned(buf)
    check(lib.sg_tolerant_accumulate(ptr(labels_flat), ptr(gt_flat), fmt, hw, off, (C.c_int32 * N)(*ts), N, K, mode_code, int(ignore_index),
                                     int(bool(reduce_zero_label)), ptr(counts), wp, wn, stream_ptr()), "sg_tolerant_accumulate")
    return counts


# ---- Object matching: object-level precision / recall / F1 and panoptic quality (sg_object_match; the definition: include/segearth_hip.h) --
OBJECT_MAX_K = CONFUSION_MAX_K
OBJECT_MAX_DEN = 1 << 20                                                 # the largest denominator of the IoU threshold
OBJECT_SQ_ONE = 1 << 24                                                  # row 3 of the counts: IoU in steps of 2^-24
OBJECT_MAX_PIXELS = _MAX_PIXELS                                          # per call
OBJECT_MATCHED_PRED, OBJECT_UNMATCHED_PRED, OBJECT_MATCHED_TRUE, OBJECT_UNMATCHED_TRUE = 1, 2, 4, 8      # the bits of match_map


def object_iou_fraction(t):
    """The IoU threshold of the object match as an exact fraction: ``t`` is a ``(num, den)`` pair of integers or a float, which is
    converted by ``fractions.Fraction(str(float(t)))`` (0.5 -> (1, 2), 0.6 -> (3, 5): the decimal that was written, not the binary
    double behind it).  The threshold must lie in [1/2, 1) -- below 1/2 the match is not unique -- with a denominator of at most 2^20
    -> (num, den) in lowest terms."""
    import math
    from fractions import Fraction
    if isinstance(t, (tuple, list)):
        if len(t) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in t) or t[1] < 1:
            raise ValueError(f"object_iou: a threshold pair must be (num, den) of integers with den >= 1, got {t!r}")
        f = Fraction(int(t[0]), int(t[1]))
    elif isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t):
        raise ValueError(f"object_iou must be a finite number or a (num, den) pair, got {t!r}")
    else:
        f = Fraction(str(float(t)))
    if not Fraction(1, 2) <= f < 1:
        raise ValueError(f"object_iou={t!r} outside [1/2, 1): below 1/2 an object could have two partners, at 1 nothing matches")
    if f.denominator > OBJECT_MAX_DEN:
        raise ValueError(f"object_iou={t!r} has the denominator {f.denominator}, above the limit of 2^20")
    return f.numerator, f.denominator


def object_args(image_hw, K, iou=(1, 2), connectivity=4, min_area=1, skip_label=None):
    """The checks of sg_object_match, before any library call: sizes positive and below 2^31 pixels per call, K in [1, 127], a threshold
    in [1/2, 1), connectivity 4 or 8, min_area an integer >= 1, skip_label None or an integer -> (image_hw, K, (num, den))."""
    image_hw = _image_sizes("object_match", image_hw, per_call=True)
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= OBJECT_MAX_K:
        raise ValueError(f"object_match: K={K!r} outside [1, {OBJECT_MAX_K}] (the cap of sg_confusion_accumulate)")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"object_match: connectivity must be 4 or 8, got {connectivity!r}")
    if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 1:
        raise ValueError(f"object_match: min_area must be an integer >= 1 (a region is an object when its area is at least it), got {min_area!r}")
    if skip_label is not None and (isinstance(skip_label, bool) or not isinstance(skip_label, int)):
        raise ValueError(f"object_match: skip_label must be None or an integer label, got {skip_label!r}")
    return image_hw, int(K), object_iou_fraction(iou)


@on_tensor_device
def object_match(labels, gt, image_hw, counts, K, iou=(1, 2), connectivity=4, min_area=1, skip_label=None, ignore_index=255,
                 reduce_zero_label=False, match_map=None):
    """sg_object_match on the current stream: per class, the connected regions of the predictions matched against those of the
    (transformed) truth at an IoU strictly above ``iou`` (a float or a ``(num, den)`` pair in [1/2, 1)), over N images that lie back to
    back in ``labels`` (int64) and ``gt`` (uint8 or int64), sizes ``image_hw``.  A region is an object when its value is a class in
    [0, K) other than ``skip_label``, it has at least ``min_area`` pixels and, for the truth, it is not ``ignore_index``.  The counts
    are ADDED to ``counts`` int64 [4,K] (matched pairs, predicted objects, true objects, the matched pairs' IoU in steps of 2^-24), which
    is returned; ``match_map``: None or a uint8 tensor of the labels' size that receives 1 / 2 (matched / unmatched predicted object)
    plus 4 / 8 (matched / unmatched true object) per pixel.  Nothing comes back to the host."""
    image_hw, K, (num, den) = object_args(image_hw, K, iou, connectivity, min_area, skip_label)
    labels, gt, N, total, hw, off, fmt = _flat_call("object_match", labels, gt, image_hw, K, counts, "counts", 4, match_map, "match_map")
    lib = _lib.load()
    buf = scratch(int(lib.sg_object_workspace_bytes(total)), labels.device)
    wp, wn = _aligned(buf)
    check(lib.sg_object_match(ptr(labels), ptr(gt), fmt, hw, off, N, K, int(connectivity), int(min_area), 0 if skip_label is None else int(skip_label),
                              int(skip_label is not None), num, den, int(ignore_index), int(bool(reduce_zero_label)), ptr(counts), ptr(match_map),
                              wp, wn, stream_ptr()), "sg_object_match")
    return counts
