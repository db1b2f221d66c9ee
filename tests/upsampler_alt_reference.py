"""f64 restatement of the SimFeatUp ``bilinear`` upsampler (reference simfeatup_dev/upsamplers.py:343-350, ``Bilinear``), of the
per-pixel logits built on it (segmentor.py:368-379) and of ``resize_conv`` (LayeredResizeConv, :178-200), with per-element error bounds for the HIP kernels in the style of
tests/jbu_reference.py and tests/gemm_reference.py.

Two coordinate rules:
  * ``taps(..., f32=False)``: PyTorch's F.interpolate(mode='bilinear', align_corners=False) in exact arithmetic (ATen
    area_pixel_compute_source_index), used against the fixture minted from the reference;
  * ``taps(..., f32=True)``: the same rule evaluated in f32 exactly as the kernels do (bilinear_tap in rowops.h), with a clamped second
    index folded into the first, so that the f64 results are taken on the kernels' own operands.
The Gram form (``gram_logits``) is the kernels' formula in f64: by linearity the normalised interpolated feature's product with the text is
(sum_k w_k y_k) / sqrt(sum_kl w_k w_l <f_k, f_l>) over the four corners of the pixel's cell.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def taps(in_size: int, out_size: int, f32: bool = True):
    """-> (i0, i1, l0, l1) arrays of length out_size: out[d] = l0 * in[i0] + l1 * in[i1]."""
    d = np.arange(out_size)
    if in_size == out_size:
        return d.copy(), d.copy(), np.ones(out_size), np.zeros(out_size)
    if f32:
        scale = np.float32(in_size) / np.float32(out_size)
        src = (scale * (d.astype(np.float32) + np.float32(0.5)) - np.float32(0.5)).astype(np.float32)
    else:
        src = (in_size / out_size) * (d + 0.5) - 0.5
    src = np.maximum(src, 0)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0).astype(np.float32 if f32 else np.float64)
    l0 = (np.float32(1) - l1) if f32 else 1.0 - l1
    if f32:                                              # bilinear_cell: a clamped second index folds into the first
        same = i1 == i0
        l0 = np.where(same, (l0 + l1).astype(np.float32), l0)
        l1 = np.where(same, np.float32(0), l1)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def interp_matrix(in_size: int, out_size: int, f32: bool = True) -> np.ndarray:
    """[out, in] f64 matrix of the 1-D interpolation."""
    i0, i1, l0, l1 = taps(in_size, out_size, f32)
    m = np.zeros((out_size, in_size))
    np.add.at(m, (np.arange(out_size), i0), l0)
    np.add.at(m, (np.arange(out_size), i1), l1)
    return m


def bilinear_upsample(tokens, gh, gw, GH, GW, f32: bool = True) -> np.ndarray:
    """Bilinear.forward on pixel-major tokens [B, gh*gw, C] -> [B, GH*GW, C] f64 (separable: rows, then columns)."""
    t = np.asarray(tokens, np.float64).reshape(-1, gh, gw, tokens.shape[-1])
    my, mx = interp_matrix(gh, GH, f32), interp_matrix(gw, GW, f32)
    out = np.einsum("Yi,bijc,Xj->bYXc", my, t, mx)
    return out.reshape(t.shape[0], GH * GW, -1)


def cls_logits(cls, text):
    c = np.asarray(cls, np.float64)
    return (c / np.linalg.norm(c, axis=-1, keepdims=True)) @ np.asarray(text, np.float64).T


def logits(tokens, text, gh, gw, GH, GW, cls=None, lam=0.0, f32: bool = True) -> np.ndarray:
    """Interpolate, then normalise, then x T^T (+ lam * cls logits): [B, Q, GH*GW] f64."""
    f = bilinear_upsample(tokens, gh, gw, GH, GW, f32)
    f = f / np.linalg.norm(f, axis=-1, keepdims=True)
    out = np.einsum("bpc,qc->bqp", f, np.asarray(text, np.float64))
    if cls is not None and lam != 0.0:
        out = out + lam * cls_logits(cls, text)[:, :, None]
    return out


def _corners(gh, gw, GH, GW):
    r0, r1, v0, v1 = taps(gh, GH, True)
    c0, c1, u0, u1 = taps(gw, GW, True)
    r1 = np.minimum(r0 + 1, gh - 1)
    c1 = np.minimum(c0 + 1, gw - 1)
    idx = [(r0[:, None] * gw + c0[None, :]), (r0[:, None] * gw + c1[None, :]), (r1[:, None] * gw + c0[None, :]),
           (r1[:, None] * gw + c1[None, :])]
    w = [v0[:, None] * u0[None, :], v0[:, None] * u1[None, :], v1[:, None] * u0[None, :], v1[:, None] * u1[None, :]]
    return [i.reshape(-1) for i in idx], [x.reshape(-1) for x in w]


def gram_terms(tokens, gh, gw):
    """The prologue's five Gram terms per token [B, n, 5] (absent neighbours count as zero)."""
    t = np.asarray(tokens, np.float64).reshape(-1, gh, gw, tokens.shape[-1])
    z = np.zeros_like(t)
    r = z.copy(); r[:, :, :-1] = t[:, :, 1:]
    d = z.copy(); d[:, :-1] = t[:, 1:]
    dr = z.copy(); dr[:, :-1, :-1] = t[:, 1:, 1:]
    g = np.stack([(t * t).sum(-1), (t * r).sum(-1), (t * d).sum(-1), (t * dr).sum(-1), (r * d).sum(-1)], -1)
    return g.reshape(t.shape[0], gh * gw, 5)


def gram_logits(tokens, text, gh, gw, GH, GW, cls=None, lam=0.0) -> np.ndarray:
    """The kernels' formula in f64: [B, Q, GH*GW]."""
    t = np.asarray(tokens, np.float64)
    y = t @ np.asarray(text, np.float64).T                               # [B, n, Q]
    g = gram_terms(t, gh, gw)
    (k00, k01, k10, k11), (w00, w01, w10, w11) = _corners(gh, gw, GH, GW)
    num = w00[:, None] * y[:, k00] + w01[:, None] * y[:, k01] + w10[:, None] * y[:, k10] + w11[:, None] * y[:, k11]
    d2 = (w00 ** 2 * g[:, k00, 0] + w01 ** 2 * g[:, k01, 0] + w10 ** 2 * g[:, k10, 0] + w11 ** 2 * g[:, k11, 0]
          + 2 * (w00 * (w01 * g[:, k00, 1] + w10 * g[:, k00, 2] + w11 * g[:, k00, 3]) + w01 * (w10 * g[:, k00, 4] + w11 * g[:, k01, 2])
                 + w10 * w11 * g[:, k10, 1]))
    out = (num / np.sqrt(d2)[:, :, None]).transpose(0, 2, 1)
    if cls is not None and lam != 0.0:
        out = out + lam * cls_logits(cls, text)[:, :, None]
    return out


def logits_bound(tokens, text, gh, gw, GH, GW, cls=None, lam=0.0):
    """(reference [B, Q, GH*GW] f64, per-element bound on |kernel - reference|) for sg_jbu_logits of kind 2 on these operands
    (include/segearth_hip.h): the prologue's dots (gamma_C), the cell's 4-term numerator and 10-term Gram sum, the division and the
    CLS term, and the rounding of the tap coordinates.  The M^2 / D2 factor carries the Gram form's loss where neighbours nearly cancel."""
    t = np.asarray(tokens, np.float64)
    T = np.asarray(text, np.float64)
    C = t.shape[-1]
    ref = logits(t, T, gh, gw, GH, GW, cls, lam, f32=True)
    y = t @ T.T
    A = np.abs(t) @ np.abs(T).T                                          # sum_c |f_kc T_qc|  [B, n, Q]
    nrm = np.linalg.norm(t, axis=-1)                                     # [B, n]
    (k00, k01, k10, k11), ws = _corners(gh, gw, GH, GW)
    ks = (k00, k01, k10, k11)
    num = sum(w[:, None] * y[:, k] for w, k in zip(ws, ks))             # [B, P, Q]
    Aw = sum(w[:, None] * A[:, k] for w, k in zip(ws, ks))
    Yw = sum(w[:, None] * np.abs(y[:, k]) for w, k in zip(ws, ks))
    M = sum(w * nrm[:, k] for w, k in zip(ws, ks))                       # [B, P]
    f = bilinear_upsample(t, gh, gw, GH, GW, True)
    D2 = (f * f).sum(-1)                                                 # [B, P]
    sd = np.sqrt(D2)[:, :, None]
    b = (gamma(C) * Aw + gamma(5) * Yw) / sd
    b = b + np.abs(num) / sd * (gamma(C) + gamma(16)) * (M ** 2 / D2)[:, :, None] / 2
    b = b + 6 * U * np.abs(num) / sd
    # the source coordinate scale * (d + 0.5) - 0.5 may be contracted to one fma in the kernel: each axis weight moves by at most 2u * in,
    # so |df| <= 4 * 2u (gh + gw) max_k |f_k| and the normalised product moves by at most 2 |df| |T_q| / |f(p)|
    nmax = np.maximum.reduce([nrm[:, k] for k in ks])                   # [B, P]
    b = b + (2 * 8 * U * (gh + gw) * nmax[:, :, None] / sd) * np.linalg.norm(T, axis=-1)[None, None, :]
    b = b.transpose(0, 2, 1)
    if cls is not None and lam != 0.0:
        c = np.asarray(cls, np.float64)
        cn = np.linalg.norm(c, axis=-1, keepdims=True)
        cb = (gamma(C) * (np.abs(c) @ np.abs(T).T) + np.abs(c @ T.T) * (gamma(C) + 4 * U)) / cn    # [B, Q]
        b = b + abs(lam) * (cb + 2 * U * np.abs(c @ T.T) / cn)[:, :, None]
    b = b + 2 * U * np.abs(ref)
    return ref, b


# ---- resize_conv: LayeredResizeConv(dim, 1) (upsamplers.py:178-200) ---------------------------------------------------------------------
EPS_OPERAND = {"f32": 0.0, "f16x2": 2.0 ** -21, "bf16": 2.0 ** -8}     # relative rounding of a GEMM operand as the precision stores it


def resize2d(x, H, W, f32: bool = True):
    """[B, c, h, w] -> [B, c, H, W] f64 bilinear (align_corners=False), separable."""
    x = np.asarray(x, np.float64)
    return np.einsum("Yi,bcij,Xj->bcYX", interp_matrix(x.shape[-2], H, f32), x, interp_matrix(x.shape[-1], W, f32))


def resize_conv_stages(src, guid, w, f32: bool = True):
    """The four stages in f64: src [B, C, h, w], guid [B, 3, GH, GW], w the state dict -> list of (A [B, C+3, 2h, 2w], stage output)."""
    x = np.asarray(src, np.float64)
    out = []
    for k in range(1, 5):
        big = resize2d(x, 2 * x.shape[-2], 2 * x.shape[-1], f32)
        g = resize2d(guid, big.shape[-2], big.shape[-1], f32)
        a = np.concatenate([big, g], 1)
        W = np.asarray(w[f"conv{k}.weight"], np.float64)[:, :, 0, 0]
        y = np.einsum("oc,bchw->bohw", W, a) + np.asarray(w[f"conv{k}.bias"], np.float64)[None, :, None, None]
        x = big + (np.maximum(y, 0) if k < 4 else y)
        out.append((a, x))
    return out


def resize_conv_bound(src, guid, w, precision: str):
    """(f64 reference output [B, C, 16h, 16w], per-element bound) for sg_jbu_upsample of kind 3.  Per stage: the producer's bilinear blends
    (4u of the blend of |x|), the GEMM over K = C + 3 with operands rounded as the precision stores them (2 eps_op + gamma_K of
    |W| |a| + |b|) and the epilogue's two roundings; an error e carried into a stage grows to at most up(e) + |W_src| up(e) (bilinear
    resizes are convex blends and ReLU is 1-Lipschitz).  The guidance's own coordinate rounding adds 8u GH max|g| |W_guid|."""
    stages = resize_conv_stages(src, guid, w, True)
    C = np.asarray(src).shape[1]
    eps = EPS_OPERAND[precision]
    gk = gamma(C + 3)
    GH = max(np.asarray(guid).shape[-2:])
    gmax = np.abs(np.asarray(guid, np.float64)).max()
    x_abs = np.abs(np.asarray(src, np.float64))
    e = np.zeros_like(x_abs)
    for k, (a, x) in enumerate(stages, 1):
        H2, W2 = a.shape[-2:]
        W = np.abs(np.asarray(w[f"conv{k}.weight"], np.float64)[:, :, 0, 0])
        b = np.abs(np.asarray(w[f"conv{k}.bias"], np.float64))[None, :, None, None]
        up_abs = resize2d(x_abs, H2, W2)
        up_e = resize2d(e, H2, W2)
        a_abs = np.abs(a)
        a_abs[:, :C] = up_abs                                              # the blend of |x| bounds the blended source
        prod = np.einsum("oc,bchw->bohw", W, a_abs) + b
        loc = (2 * eps + gk) * prod + 4 * U * np.einsum("oc,bchw->bohw", W[:, :C], up_abs) + 4 * U * up_abs
        loc = loc + 8 * U * GH * gmax * W[:, C:].sum(1)[None, :, None, None]
        loc = loc + 2 * U * (np.abs(x) + prod)
        e = up_e + np.einsum("oc,bchw->bohw", W[:, :C], up_e) + loc
        x_abs = up_abs + prod
    return stages[-1][1], e
