"""float64 numpy reference of the segmentation tail: bilinear upsample of each tile's logits (torch's align_corners=False taps),
un-pad, overlap-add in raster order, count division, x logit_scale, softmax over queries, per-class maximum over synonyms, argmax
(lowest class index), prob_thd -> bg_idx.  Test infrastructure only; shared by the CPU and the GPU tests of the label head.

Also the acceptance rule those tests share.  A pixel COUNTS unless its float64 top-two class-probability gap, or |conf - prob_thd|, is
below G = 1e-3: the stitched logits carry a few f32 roundings of values below 1 (absolute error about 1e-6 at most), the scale of 50
turns that into about 5e-5 on the exponent, so probabilities are off by less than about 2e-4; G is that with a 5x margin.  On every
counted pixel the label must equal the reference's and conf must lie within G; at most CAP = 1 % of the pixels of a case may be left
uncounted (a Monte-Carlo run on independent pixels with the post-interpolation spread of the test inputs gave 0.04-0.12 % for the
label gap and up to 0.08 % for the threshold, Q = 7...257; tests/test_head_reference_cpu.py confirms it on the real reference).
"""
import numpy as np

G = 1e-3
CAP = 0.01


def taps(n_in: int, n_out: int) -> np.ndarray:
    """[n_out, n_in] interpolation matrix of F.interpolate(mode='bilinear', align_corners=False) along one axis, in float64
    (ATen area_pixel_compute_source_index: src = max(scale * (dst + 0.5) - 0.5, 0), taps floor(src) and the next, clamped)."""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    if n_in == n_out:
        m[np.arange(n_out), np.arange(n_out)] = 1.0
        return m
    scale = n_in / n_out
    src = np.maximum(scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0
    np.add.at(m, (np.arange(n_out), i0), 1.0 - l1)
    np.add.at(m, (np.arange(n_out), i1), l1)
    return m


def upsample(tile: np.ndarray, up_hw) -> np.ndarray:
    """[Q, gh, gw] -> [Q, up_h, up_w], float64."""
    wy, wx = taps(tile.shape[1], up_hw[0]), taps(tile.shape[2], up_hw[1])
    return np.einsum("yg,qgh,xh->qyx", wy, tile.astype(np.float64), wx, optimize=True)


def stitch(tile_logits: np.ndarray, windows, up_hw, pad_tl, canvas_hw) -> np.ndarray:
    """tile_logits [T,Q,gh,gw], windows [(y1,y2,x1,x2)] in raster order -> the count-normalised canvas [Q,H,W] in float64 (a window
    may reach outside the canvas rows, as the windows of a canvas band do)."""
    T, Q = tile_logits.shape[:2]
    H, W = canvas_hw
    acc = np.zeros((Q, H, W), dtype=np.float64)
    cnt = np.zeros((H, W), dtype=np.float64)
    for t, (y1, y2, x1, x2) in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
        up = upsample(tile_logits[t], up_hw)[:, pad_tl[0]:pad_tl[0] + (y2 - y1), pad_tl[1]:pad_tl[1] + (x2 - x1)]
        ya, yb, xa, xb = max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)
        if yb <= ya or xb <= xa:
            continue
        acc[:, ya:yb, xa:xb] += up[:, ya - y1:yb - y1, xa - x1:xb - x1]
        cnt[ya:yb, xa:xb] += 1.0
    return np.where(cnt > 0, acc / np.maximum(cnt, 1.0), 0.0)


def tail(canvas: np.ndarray, query_idx, K: int, logit_scale: float, prob_thd: float, bg_idx: int):
    """canvas [Q,H,W] -> dict(probs [K,H,W], labels int64 [H,W], conf [H,W], gap [H,W] = top-two class-probability gap), float64.
    K == Q means class(q) = q (the reference skips the synonym merge then)."""
    canvas = np.asarray(canvas, dtype=np.float64)
    Q = canvas.shape[0]
    v = canvas * float(logit_scale)
    e = np.exp(v - v.max(0, keepdims=True))
    p = e / e.sum(0, keepdims=True)
    qi = np.arange(Q) if K == Q else np.asarray(query_idx).reshape(-1)
    if K == Q:
        probs = p
    else:
        # (probabilities * one_hot).max over queries: the zeros of the other queries take part in the max
        probs = np.zeros((K,) + canvas.shape[1:])
        if len(set(qi.tolist())) == 1 and 0 <= qi[0] < K:
            probs[qi[0]] = -np.inf                                 # no other query contributes a zero to this class's max
        for q in range(Q):
            if 0 <= qi[q] < K:
                probs[qi[q]] = np.maximum(probs[qi[q]], p[q])
    labels = probs.argmax(0).astype(np.int64)                      # the first maximum: the lowest class index
    conf = probs.max(0)
    if K > 1:
        top2 = np.partition(probs, K - 2, axis=0)[K - 2:]
        gap = top2[1] - top2[0]
    else:
        gap = np.full(conf.shape, np.inf)
    labels = np.where(conf < prob_thd, bg_idx, labels)
    return dict(probs=probs, labels=labels, conf=conf, gap=gap)


def label_head(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, K, logit_scale, prob_thd, bg_idx):
    return tail(stitch(tile_logits, windows, up_hw, pad_tl, canvas_hw), query_idx, K, logit_scale, prob_thd, bg_idx)


def counted(ref: dict, prob_thd: float) -> np.ndarray:
    """Pixels on which a label is decided beyond f32 rounding (module docstring)."""
    return (ref["gap"] >= G) & (np.abs(ref["conf"] - prob_thd) >= G)


def check_labels(ref: dict, labels, conf, prob_thd: float, what: str = ""):
    """The acceptance rule: returns the uncounted fraction after asserting the cap, the labels and (when given) conf."""
    ok = counted(ref, prob_thd)
    frac = 1.0 - ok.mean()
    labels = np.asarray(labels).reshape(ref["labels"].shape)
    bad = int((labels[ok] != ref["labels"][ok]).sum())
    print(f"{what}: uncounted {100 * frac:.3f} %, label mismatches on counted pixels {bad}", end="")
    if conf is not None:
        dc = float(np.abs(np.asarray(conf, dtype=np.float64).reshape(ref["conf"].shape) - ref["conf"])[ok].max()) if ok.any() else 0.0
        print(f", max |conf - ref| {dc:.3e}", end="")
    print()
    assert frac <= CAP, f"{what}: {100 * frac:.2f} % of the pixels are within {G} of a tie or of the threshold"
    assert bad == 0, f"{what}: {bad} counted pixels differ from the float64 reference"
    if conf is not None:
        assert dc <= G, f"{what}: conf is off by {dc}"
    return frac


# ---- the shapes the GPU test runs (the CPU test confirms the cap on the same inputs) ------------------------------------------------
def slide_windows(H, W, stride, crop):
    hg = max(H - crop + stride - 1, 0) // stride + 1
    wg = max(W - crop + stride - 1, 0) // stride + 1
    out = []
    for hi in range(hg):
        for wi in range(wg):
            y2, x2 = min(hi * stride + crop, H), min(wi * stride + crop, W)
            out.append((max(y2 - crop, 0), y2, max(x2 - crop, 0), x2))
    return out


# name -> (H, W, stride, crop, (gh, gw), up_hw, pad_tl): canvases of about 70 x 90 whose last window is shifted back (counts 1, 2, 4);
# "dense" has more than 64 tiles over one block (the candidate list's fall-back)
GEOMETRIES = {
    "a": (70, 90, 28, 40, (3, 3), (42, 44), (1, 2)),
    "b": (66, 93, 30, 44, (5, 4), (48, 46), (2, 1)),
    "dense": (40, 70, 2, 32, (3, 4), (40, 40), (4, 4)),
}
QS = (1, 7, 8, 9, 64, 65, 130, 257)


def make_case(geom: str, Q: int, merge: bool, seed: int = 0):
    """-> dict(tile_logits f32 [T,Q,gh,gw] i.i.d. N(0, 0.3^2), windows, up_hw, pad_tl, hw, query_idx int32 [Q], K).  ``merge``: K about
    Q / 2 with shuffled (unsorted) query_idx, every class owning at least one query; otherwise K = Q."""
    H, W, stride, crop, grid, up_hw, pad_tl = GEOMETRIES[geom]
    rng = np.random.default_rng(1000 * seed + 7 * Q + len(geom))
    wins = slide_windows(H, W, stride, crop)
    tl = (0.3 * rng.standard_normal((len(wins), Q) + grid)).astype(np.float32)
    if merge and Q > 1:
        K = max(1, Q // 2)
        qi = np.concatenate([np.arange(K), rng.integers(0, K, Q - K)])
        rng.shuffle(qi)
    else:
        K, qi = Q, np.arange(Q)
    return dict(tile_logits=tl, windows=np.asarray(wins, dtype=np.int32), up_hw=up_hw, pad_tl=pad_tl, hw=(H, W),
                query_idx=qi.astype(np.int32), K=K)


# =====================================================================================================================================
# Per-element references and bounds of every kernel of csrc/head.hip (tests/test_gpu_head_reference.py, tests/test_head_bound_cpu.py).
#
# Everything below is numpy float64 on the CPU.  A bound is built from the magnitudes of the operands and from the shape of the kernel's
# summation, never from observed outputs.  u = 2^-24.  ASSUMPTIONS about the device's libm, the ones rowops_reference.py states: expf
# within 2 ulp (EXPF = 2^-22 relative); sqrtf and the f32 division are budgeted a full ulp each (SQRT = 2 u).  F32_TINY = 2^-149 is the
# absolute floor of one f32 rounding.  Every bound carries a factor (1 + 1e-3) for the second-order terms and + F32_TINY so that an exact
# zero has a non-zero bound.
# =====================================================================================================================================
import torch  # noqa: E402

from gemm_reference import U, check_within  # noqa: E402,F401
from rowops_reference import EXPF, F32_TINY, SQRT, depth  # noqa: E402

SLACK = 1.0 + 1e-3
H2_REL, H2_ABS, H2_LO = 2.0 ** -22, 2.0 ** -25, 2.0 ** -11


def within(got, ref, bound, what=""):
    """check_within on numpy arrays: every element of got within bound of ref; returns the largest err / bound."""
    return check_within(torch.as_tensor(np.ascontiguousarray(got)), torch.as_tensor(np.ascontiguousarray(ref, dtype=np.float64)),
                        torch.as_tensor(np.ascontiguousarray(bound, dtype=np.float64)), what)


def f32v(x: float) -> float:
    """The value a C `float` argument carries."""
    return float(np.float32(x))


# ---- cosine logits ---------------------------------------------------------------------------------------------------------------------
def lane16_depth(E: int) -> int:
    """Roundings on the longest path of a 16-lane sum of E products as cosine_logits_kernel / cosine_logits_wide_kernel form it: the
    product (1), (a + b) + (c + d) inside a float4 (2), one accumulating add per float4 of the lane (ceil(E / 64)), the 4-step butterfly."""
    return -(-E // 64) + 7


def cosine_reference(tok, cls, text, debias, lam):
    """(logits [B,Q,n], bound) in f64 of sg_cosine_logits / sg_cosine_logits_wide (segmentor.py:309-336, 374-379):
    c = cls / |cls|, cl = c . T^T, w = cos(f, c) debias, f' = f - c w, xh = f' / |f'|, logit = xh . t + lam cl.  tok [B,n,E], cls [B,E] or
    None, text [Q,E].  A zero token row gives NaN (x / |x|), value and bound.

    Bound, with D = lane16_depth(E) u for the 16-lane sums and d64 = depth(E) + 1 for the two 64-lane sums of the CLS prologue:
      * an element of the unit CLS is off relatively by rc = d64 u / 2 (the norm: half the sum's error) + 2 SQRT (sqrtf, division);
        cl by (d64 u + rc) sum |c t|;
      * |f|^2 by D ff, f . c by (D + rc) sum |f c|, c . c (= 1) by D + 2 rc; w = f.c / (sqrt ff sqrt cc) debias by
        dw = |debias| (d(f.c) / |f| + |cos| (D / 2 + (D + 2 rc) / 2 + 3 SQRT + 2 u)): two sqrtf and the division at SQRT each, the product of the
        roots and the x debias at u each;
      * the debiased feature by df = |c| dw + rc |c w| + u (|f| + 2 |c w|): the cancellation term, the product's and the subtraction's
        rounding (u |f'| <= u (|f| + |c w|));
      * |f'|^2 by D nn + sum (2 |f'| df + df^2); 1 / sqrt by half of that relatively + 2 SQRT; xh = f' inv by df / |f'| + |xh| (that + u);
      * the dot with a text row by D sum |xh t| + sum |t| dxh;
      * + lam cl by |lam| dcl + u |lam cl| + u |logit|."""
    x, t = np.asarray(tok, dtype=np.float64), np.asarray(text, dtype=np.float64)
    E = x.shape[-1]
    D = lane16_depth(E) * U
    debias, lam = f32v(debias), f32v(lam)
    use_cls = cls is not None
    with np.errstate(invalid="ignore", divide="ignore"):
        if use_cls:
            c = np.asarray(cls, dtype=np.float64)
            ch = c / np.sqrt((c * c).sum(-1, keepdims=True))
            d64 = depth(E) + 1
            rc = 0.5 * d64 * U + 2 * SQRT
            cl = ch @ t.T                                                 # [B,Q]
            dcl = (d64 * U + rc) * (np.abs(ch) @ np.abs(t).T)
        f, df = x, np.zeros_like(x)
        if use_cls and debias != 0.0:
            nf = np.sqrt((x * x).sum(-1))
            fc = np.einsum("bne,be->bn", x, ch)
            dfc = (D + rc) * np.einsum("bne,be->bn", np.abs(x), np.abs(ch))
            cosv = fc / nf
            w = cosv * debias
            dw = abs(debias) * (dfc / nf + np.abs(cosv) * (0.5 * D + 0.5 * (D + 2 * rc) + 3 * SQRT + 2 * U))
            cw = ch[:, None, :] * w[..., None]
            f = x - cw
            df = np.abs(ch)[:, None, :] * dw[..., None] + rc * np.abs(cw) + U * (np.abs(x) + 2 * np.abs(cw))
        nn = (f * f).sum(-1, keepdims=True)
        nrm = np.sqrt(nn)
        dnn = D * nn + (2 * np.abs(f) * df + df * df).sum(-1, keepdims=True)
        xh = f / nrm
        dxh = df / nrm + np.abs(xh) * (0.5 * dnn / nn + 2 * SQRT + U)
        out = xh @ t.T                                                    # [B,n,Q]
        b = D * (np.abs(xh) @ np.abs(t).T) + dxh @ np.abs(t).T
        if use_cls and lam != 0.0:
            out = out + lam * cl[:, None, :]
            b = b + abs(lam) * dcl[:, None, :] + U * np.abs(lam * cl)[:, None, :]
        b = (b + U * np.abs(out)) * SLACK + F32_TINY
    return out.transpose(0, 2, 1), b.transpose(0, 2, 1)


def _h2_err(a):
    """Representation error of hi + lo = f16(a) + f16(a - hi): max(2^-22 |a|, 2^-25) (common.h); zero is exact."""
    return np.where(a == 0, 0.0, np.maximum(H2_REL * np.abs(a), H2_ABS))


def _h2_lo(a):
    """Largest |lo|: half an f16 ulp of a, 2^-11 |a|, or half the f16 subnormal spacing."""
    return np.where(a == 0, 0.0, np.maximum(H2_LO * np.abs(a), H2_ABS))


def cosine_two_plane_reference(tok, cls, text, lam):
    """(logits [B,Q,n], bound) of cosine_logits_mfma_kernel: x . t / max(|x|, 1e-12) + lam (cls / |cls|) . t.

    Bound: tokens and text are each hi + lo with a representation error of max(2^-22 |a|, 2^-25) per element (an ABSOLUTE floor: the
    kernel is not scale-invariant although the quantity is); the three-product scheme drops lo . lo (|lo| <= max(2^-11 |a|, 2^-25)); so the
    exact sum of the issued products misses x . t by rep = sum (ex |t| + |x| et + ex et + lo_x lo_t).  The f32 accumulation on the matrix
    unit is charged E u sum |terms|.  |x|^2 is an fma chain of E / 4 per lane and 2 shuffle adds: relatively (E / 4 + 2) u, halved by the
    root, + SQRT (sqrtf) + SQRT (the reciprocal); acc * inv + cl one rounding each.  The CLS term: both 64-lane sums at depth(E) + 1, the
    reciprocal root as above, lam * d * inv two roundings."""
    x, t = np.asarray(tok, dtype=np.float64), np.asarray(text, dtype=np.float64)
    E = x.shape[-1]
    lam = f32v(lam)
    ex, et = _h2_err(x), _h2_err(t)
    S = np.abs(x) @ np.abs(t).T
    rep = ex @ np.abs(t).T + np.abs(x) @ et.T + ex @ et.T + _h2_lo(x) @ _h2_lo(t).T
    ddot = rep + E * U * (S + rep)
    den = np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
    out = (x @ t.T) / den
    b = ddot / den + np.abs(out) * (0.5 * (E // 4 + 2) * U + 2 * SQRT + U)
    if cls is not None and lam != 0.0:
        c = np.asarray(cls, dtype=np.float64)
        cn = np.sqrt((c * c).sum(-1, keepdims=True))
        d64 = (depth(E) + 1) * U
        cl = (c @ t.T) / cn
        dcl = d64 * (np.abs(c) @ np.abs(t).T) / cn + np.abs(cl) * (0.5 * d64 + 2 * SQRT + 2 * U)
        out = out + lam * cl[:, None, :]
        b = b + abs(lam) * dcl[:, None, :]
    b = (b + U * np.abs(out)) * SLACK + F32_TINY
    return out.transpose(0, 2, 1), b.transpose(0, 2, 1)


def _sum16(terms):
    """terms [..., nv, 16] f32 (one value per float4 and lane) -> the 16-lane sum: a lane accumulates its float4s in order, then the xor
    butterfly 8, 4, 2, 1."""
    acc = np.zeros(terms.shape[:-2] + (16,), dtype=np.float32)
    for k in range(terms.shape[-2]):
        acc = acc + terms[..., k, :]
    w = 16
    while w > 1:
        w //= 2
        acc = acc[..., :w] + acc[..., w:2 * w]
    return acc[..., 0]


def _dot4(a, b):
    """a, b [..., nv, 16, 4] f32 -> (a0 b0 + a1 b1) + (a2 b2 + a3 b3) per float4."""
    p = a * b
    return (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])


def _lanes(a, E):
    """[..., E] f32 -> [..., nv, 16, 4], zero padded to a multiple of 64."""
    pad = (-E) % 64
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (pad,), dtype=np.float32)], -1)
    return a.reshape(a.shape[:-1] + (-1, 16, 4))


def _wave_sum(v):
    """The 64-lane strided sum of rowops_reference.lane_sum on an f32 numpy array (last axis)."""
    pad = (-v.shape[-1]) % 64
    v = np.concatenate([v, np.zeros(v.shape[:-1] + (pad,), dtype=np.float32)], -1).reshape(v.shape[:-1] + (-1, 64))
    acc = v[..., 0, :]
    for r in range(1, v.shape[-2]):
        acc = acc + v[..., r, :]
    w = 64
    while w > 1:
        w //= 2
        acc = acc[..., :w] + acc[..., w:2 * w]
    return acc[..., 0]


def cosine_emulate(tok, cls, text, debias, lam, mut=None):
    """cosine_logits_kernel in f32 with its summation shape -> [B,Q,n]; `mut` names one of the listed slips."""
    f = np.float32
    x, t = np.asarray(tok, dtype=f).copy(), np.asarray(text, dtype=f)
    B, n, E = x.shape
    Q = t.shape[0]
    debias, lam = f(debias), f(lam)
    use_cls = cls is not None
    tl = _lanes(t, E)
    if mut == "drop_last_float4" and E % 64:                              # `i + 4 < E` for `i < E`: the row's last float4 never loaded
        x[..., E - 4:] = 0
        tl = _lanes(np.concatenate([t[:, :E - 4], np.zeros((Q, 4), dtype=f)], -1), E)
    with np.errstate(invalid="ignore", divide="ignore"):
        if use_cls:
            c = np.asarray(cls, dtype=f)
            if mut == "cls_image0":
                c = np.broadcast_to(c[:1], c.shape)
            sC = c / np.sqrt(_wave_sum(c * c))[:, None]
            sCL = np.stack([_wave_sum(sC * t[q][None]) for q in range(Q)], -1)        # [B,Q]
        xl = _lanes(x, E)
        ff = _sum16(_dot4(xl, xl))
        if use_cls and debias != 0:
            cl_ = _lanes(sC, E)[:, None]
            fc, cc = _sum16(_dot4(xl, cl_)), _sum16(_dot4(cl_, cl_))
            w = (fc / (np.sqrt(ff) * np.sqrt(cc))) * debias
            sub = _lanes(c, E)[:, None] if mut == "debias_raw_cls" else cl_
            xl = xl - sub * w[..., None, None, None]
        nn = _sum16(_dot4(xl, xl))
        inv = f(1.0) / np.sqrt(ff if mut == "no_renorm" else nn)
        xs = xl * inv[..., None, None, None]
        out = np.stack([_sum16(_dot4(xs, tl[q])) for q in range(Q)], 1)               # [B,Q,n]
        if use_cls and lam != 0:
            if mut == "lambda_sign":
                lam = -lam
            out = out + (sCL if mut == "cls_logit_unscaled" else sCL * lam)[:, :, None]
    return out


def split_h2_np(a):
    """(hi, lo) f16 planes of f32 values as split_h2 forms them (values inside the f16 range)."""
    a = np.asarray(a, dtype=np.float32)
    hi = a.astype(np.float16)
    return hi, (a - hi.astype(np.float32)).astype(np.float16)


def cosine_two_plane_emulate(tok, cls, text, lam):
    """cosine_logits_mfma_kernel on the CPU: the planes exactly as split_h2 makes them, the three products summed (in f64, rounded to f32:
    the matrix unit's accumulation order is not reproduced), the norm and the CLS term in f32."""
    f = np.float32
    x, t = np.asarray(tok, dtype=f), np.asarray(text, dtype=f)
    xh, xl = (p.astype(np.float64) for p in split_h2_np(x))
    th, tl = (p.astype(np.float64) for p in split_h2_np(t))
    acc = (xh @ th.T + xl @ th.T + xh @ tl.T).astype(f)
    nx = (x.astype(np.float64) ** 2).sum(-1).astype(f)
    inv = f(1.0) / np.maximum(np.sqrt(nx), f(1e-12))
    out = acc * inv[..., None]
    if cls is not None and lam != 0:
        c = np.asarray(cls, dtype=f)
        cinv = f(1.0) / np.sqrt(_wave_sum(c * c))
        d = np.stack([_wave_sum(c * t[q][None]) for q in range(t.shape[0])], -1)
        out = out + (f(lam) * d * cinv[:, None])[:, None, :]
    return out.transpose(0, 2, 1)


def make_cosine_case(B, n, E, Q, kind, seed):
    """(tok [B,n,E], cls [B,E], text [Q,E]) f32.  Text rows of norms 0.3 .. 3 (not unit), a different CLS row per image.  kind:
    'scales'  per-token scales 2^-30 .. 2^30 (geometric over the tokens);
    'offset'  features at 10 +- 1;
    'cancel'  tokens = cls / |cls| + 1e-3 noise (with debias 1.0 the debiased feature is what a cancellation leaves);
    'zero'    as 'scales' at 2^-3 .. 2^3 with token row 0 of image 0 all zero."""
    rng = np.random.default_rng(10007 * seed + 131 * E + 17 * n + Q)
    tok = rng.standard_normal((B, n, E))
    cls = rng.standard_normal((B, E)) * (1.0 + np.arange(B))[:, None]
    text = rng.standard_normal((Q, E)) / np.sqrt(E) * np.exp2(np.linspace(-1.7, 1.6, Q))[:, None]
    if kind == "scales":
        tok = tok * np.exp2(np.linspace(-30, 30, n) if n > 1 else np.array([30.0]))[None, :, None]
    elif kind == "offset":
        tok, cls = tok + 10.0, cls + 3.0
    elif kind == "cancel":
        tok = (cls / np.linalg.norm(cls, axis=-1, keepdims=True))[:, None, :] + 1e-3 * tok
    elif kind == "zero":
        tok = tok * np.exp2(np.linspace(-3, 3, n))[None, :, None]
        tok[0, 0] = 0.0
    return tok.astype(np.float32), cls.astype(np.float32), text.astype(np.float32)


# the parameter sets of the issue: no cls, then (debias, lambda)
COSINE_PARAMS = (None, (0.2, 0.0), (0.0, -0.3), (1.0, 0.5))
COSINE_E = (4, 60, 64, 68, 512, 516, 768, 772, 1024, 1028, 2048)
COSINE_N = (1, 3, 5, 31, 32, 33)


def cosine_cases():
    """A covering subset of E x n x B x Q x parameters x data: every E with every parameter set, every n, both B and both Q several times."""
    kinds = ("scales", "offset", "cancel")
    out = []
    for i, E in enumerate(COSINE_E):
        for j, par in enumerate(COSINE_PARAMS):
            k = i + j
            kind = "cancel" if par == (1.0, 0.5) else kinds[k % 2]
            out.append((E, COSINE_N[k % 6], (1, 3)[k % 2], (5, 1)[(k // 2) % 2], par, kind))
    return out


# ---- stitch / resize ---------------------------------------------------------------------------------------------------------------------
def tap_err(n_in: int, n_out: int) -> np.ndarray:
    """[n_out] bound on the error of the f32 tap weights of rowops.h: bilinear_tap: scale = f32(in) / f32(out) (u), its product with
    dst + 0.5 (u), the - 0.5 (u), all on src + 1 at most; src - i0 is exact, 1 - l1 rounds once: 4 u (src + 1).  The same size is an exact
    identity."""
    if n_in == n_out:
        return np.zeros(n_out)
    src = np.maximum(n_in / n_out * (np.arange(n_out) + 0.5) - 0.5, 0.0)
    return 4 * U * (src + 1.0)


def _max_diff(a, axis):
    """max |a[i + 1] - a[i]| along `axis` over the two trailing (grid) axes of a [..., gh, gw]; 0 for a single cell."""
    if a.shape[axis] < 2:
        return np.zeros(a.shape[:-2])
    return np.abs(np.diff(a, axis=axis)).max((-2, -1))


def _upsample_bound_parts(tile, up_hw):
    """tile [Q,gh,gw] f64 -> (e [Q,up_h,up_w], m [Q,up_h,up_w]): the tap-weight term e_y Dy + e_x Dx (the interpolant is piecewise linear
    and continuous with slope at most the largest neighbour difference D along an axis, so a source coordinate off by e moves it by e D at
    most, also across a cell border) and the magnitude m = the interpolation of |tile|."""
    a = np.abs(tile)
    m = np.einsum("yg,qgh,xh->qyx", taps(tile.shape[1], up_hw[0]), a, taps(tile.shape[2], up_hw[1]), optimize=True)
    ey, ex = tap_err(tile.shape[1], up_hw[0]), tap_err(tile.shape[2], up_hw[1])
    e = ey[None, :, None] * _max_diff(tile, -2)[:, None, None] + ex[None, None, :] * _max_diff(tile, -1)[:, None, None]
    return e, m


def stitch_bound(tile_logits, windows, up_hw, pad_tl, canvas_hw) -> np.ndarray:
    """bound [Q,H,W] on |sg_stitch - stitch(...)|: ((sum_tiles e_y Dy + e_x Dx) + (cnt + 5) u sum_tiles m) / cnt over the cnt tiles that
    cover a pixel (_upsample_bound_parts).  The u term: 4 roundings on the longest path of one tile's 4 products and 3 adds, cnt - 1
    accumulating adds (the first add to 0 is exact), the division, one spare."""
    tl = np.asarray(tile_logits, dtype=np.float64)
    T, Q = tl.shape[:2]
    H, W = canvas_hw
    es, ms, cnt = np.zeros((Q, H, W)), np.zeros((Q, H, W)), np.zeros((H, W))
    for t, (y1, y2, x1, x2) in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
        ya, yb, xa, xb = max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)
        if yb <= ya or xb <= xa:
            continue
        e, m = _upsample_bound_parts(tl[t], up_hw)
        sl = (slice(None), slice(pad_tl[0] + ya - y1, pad_tl[0] + yb - y1), slice(pad_tl[1] + xa - x1, pad_tl[1] + xb - x1))
        es[:, ya:yb, xa:xb] += e[sl]
        ms[:, ya:yb, xa:xb] += m[sl]
        cnt[ya:yb, xa:xb] += 1.0
    return (es + (cnt + 5) * U * ms) / np.maximum(cnt, 1.0) * SLACK + F32_TINY


def resize_reference(src, size):
    """(dst [C,H,W], bound) of sg_resize_bilinear: F.interpolate(bilinear, align_corners=False) from `taps`; the bound is one tile of
    stitch_bound: e_y Dy + e_x Dx + 6 u m (4 roundings on the longest path, two spare)."""
    s = np.asarray(src, dtype=np.float64)
    dst = upsample(s, size)
    e, m = _upsample_bound_parts(s, size)
    return dst, (e + 6 * U * m) * SLACK + F32_TINY


def tap_f32(dst, n_in, n_out, align_corners=False):
    """rowops.h: bilinear_tap in f32 for an integer array dst -> (i0, i1, l0, l1)."""
    f = np.float32
    dst = np.asarray(dst)
    if n_in == n_out and not align_corners:
        return dst, dst, np.ones(dst.shape, dtype=f), np.zeros(dst.shape, dtype=f)
    if align_corners:
        src = dst.astype(f) * (f(n_in - 1) / f(max(n_out - 1, 1)))
    else:
        src = np.maximum((f(n_in) / f(n_out)) * (dst.astype(f) + f(0.5)) - f(0.5), f(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(f)
    return i0, i1, f(1) - l1, l1


def _blend_f32(p, ty, tx):
    """p [Q,gh,gw] f32, taps of the rows / columns -> [Q,len(y),len(x)] as the kernels blend: top and bottom rows first, then the two."""
    ya, yb, wy0, wy1 = ty
    xa, xb, wx0, wx1 = tx
    top = p[:, ya][:, :, xa] * wx0 + p[:, ya][:, :, xb] * wx1
    bot = p[:, yb][:, :, xa] * wx0 + p[:, yb][:, :, xb] * wx1
    return top * wy0[None, :, None] + bot * wy1[None, :, None]


def stitch_emulate(tile_logits, windows, up_hw, pad_tl, canvas_hw, mut=None):
    """stitch_kernel in f32: f32 taps, the covering tiles added in raster order, divided by the count."""
    f = np.float32
    tl = np.asarray(tile_logits, dtype=f)
    T, Q, gh, gw = tl.shape
    H, W = canvas_hw
    pt, pl = (pad_tl[1], pad_tl[0]) if mut == "swap_pad" else pad_tl
    ac = mut == "align_corners"
    acc, cnt = np.zeros((Q, H, W), dtype=f), np.zeros((H, W), dtype=f)
    for t, (y1, y2, x1, x2) in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
        ya, yb, xa, xb = max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)
        if yb <= ya or xb <= xa:
            continue
        ry, rx = np.arange(ya, yb) - y1 + pt, np.arange(xa, xb) - x1 + pl
        if mut == "swap_taps":                                            # the rows' taps from (gw, up_w), the columns' from (gh, up_h)
            ty, tx = tap_f32(ry, gw, up_hw[1]), tap_f32(rx, gh, up_hw[0])
            ty = (np.minimum(ty[0], gh - 1), np.minimum(ty[1], gh - 1)) + ty[2:]
            tx = (np.minimum(tx[0], gw - 1), np.minimum(tx[1], gw - 1)) + tx[2:]
        else:
            ty, tx = tap_f32(ry, gh, up_hw[0], ac), tap_f32(rx, gw, up_hw[1], ac)
        acc[:, ya:yb, xa:xb] += _blend_f32(tl[t], ty, tx)
        cnt[ya:yb, xa:xb] += f(1)
    if mut == "no_count_div":
        return acc
    den = np.full_like(cnt, f(T)) if mut == "div_by_T" else np.maximum(cnt, f(1))
    return np.where(cnt > 0, acc / den, f(0))


def resize_emulate(src, size):
    s = np.asarray(src, dtype=np.float32)
    return _blend_f32(s, tap_f32(np.arange(size[0]), s.shape[1], size[0]), tap_f32(np.arange(size[1]), s.shape[2], size[1]))


# ---- the tail ------------------------------------------------------------------------------------------------------------------------------
def tail_bound(canvas, dcanvas, query_idx, K: int, scale: float) -> dict:
    """dict(probs [K,H,W], conf [H,W]): bounds on the class probabilities and on conf = max_k of a device tail fed a canvas that is within
    dcanvas of `canvas` (0 for sg_postprocess* on the given canvas; stitch_bound / the resize bound for the fused heads).

    The exponent a = scale v - max is off by da = scale dcanvas + u (|scale v| + |a|) (the product and the subtraction; a shift common to all
    queries cancels in the quotient).  exp(a) then carries da + EXPF relatively, the sum of Q such terms sum_j p_j (da_j + EXPF) + Q u, the
    division u: a probability p_q is off by p_q (da_q + sum_j p_j da_j + 2 EXPF + (Q + 2) u) + F32_TINY (an underflowing term is a
    subnormal rounding).  A class probability is the maximum over its queries (and an exact 0 where another class owns a query):
    |max a - max b| <= max |a - b|, so its bound is the largest of its queries'; conf likewise over the classes."""
    v = np.asarray(canvas, dtype=np.float64) * f32v(scale)
    Q = v.shape[0]
    a = v - v.max(0, keepdims=True)
    e = np.exp(a)
    p = e / e.sum(0, keepdims=True)
    da = f32v(scale) * np.broadcast_to(np.asarray(dcanvas, dtype=np.float64), v.shape) + U * (np.abs(v) + np.abs(a))
    bq = p * (da + (p * da).sum(0, keepdims=True) + 2 * EXPF + (Q + 2) * U) * SLACK + F32_TINY
    if K == Q:
        bp = bq
    else:
        qi = np.asarray(query_idx).reshape(-1)
        bp = np.full((K,) + v.shape[1:], F32_TINY)
        for q in range(Q):
            if 0 <= qi[q] < K:
                bp[qi[q]] = np.maximum(bp[qi[q]], bq[q])
    return dict(probs=bp, conf=bp.max(0))


def counted_tight(ref: dict, bound: dict, thd: float) -> np.ndarray:
    """Pixels on which the label is decided beyond the bounds: the f64 top-two class-probability gap exceeds the sum of those two classes'
    bounds and |conf - thd| exceeds conf's bound."""
    probs = ref["probs"]
    ok = np.abs(ref["conf"] - thd) > bound["conf"]
    if probs.shape[0] > 1:
        top2 = np.argsort(probs, axis=0, kind="stable")[-2:]
        ok &= ref["gap"] > np.take_along_axis(bound["probs"], top2, 0).sum(0)
    return ok


def check_tight(ref, bound, thd, got_labels, got_probs, got_conf, what):
    """Probabilities (and conf) per element within the bound, labels equal on every counted_tight pixel, at most CAP uncounted.  Returns
    (largest err / bound, uncounted share, largest err / bound over the probabilities of at least 2^-120: below that a value is a multiple
    of the subnormal spacing 2^-149 and one spacing against the F32_TINY floor reads as a ratio near 1)."""
    ratio = normal = 0.0
    if got_probs is not None:
        fin = np.isfinite(ref["probs"])
        got_probs = np.asarray(got_probs)
        assert np.array_equal(got_probs[~fin], ref["probs"][~fin]), f"{what}: -inf classes differ"
        ratio = within(got_probs[fin], ref["probs"][fin], bound["probs"][fin], what + " probs")
        big = fin & (ref["probs"] >= 2.0 ** -120)
        if big.any():
            normal = within(got_probs[big], ref["probs"][big], bound["probs"][big], what + " probs")
    if got_conf is not None:
        r = within(got_conf, ref["conf"], bound["conf"], what + " conf")
        ratio, normal = max(ratio, r), max(normal, r)
    ok = counted_tight(ref, bound, thd)
    frac = 1.0 - ok.mean()
    assert frac <= CAP, f"{what}: {100 * frac:.2f} % of the pixels are inside the bounds of a tie or of the threshold"
    labels = np.asarray(got_labels).reshape(ref["labels"].shape)
    bad = int((labels[ok] != ref["labels"][ok]).sum())
    assert bad == 0, f"{what}: {bad} counted pixels differ from the float64 reference"
    return ratio, frac, normal


def tail_emulate(canvas, query_idx, K, scale, thd, bg, form="two_pass", mut=None):
    """The three device tails in f32 on a canvas [Q,...] -> dict(probs [K,...] | None, labels, conf).
    'two_pass': class_tail (maximum, exponentials summed in query order, per-class maximum, classes ascending, strict >);
    'wide':     postprocess_wide_kernel (the same sums, queries ascending, ties to the lower class);
    'online':   label_head_block (chunks of 8 queries, running maximum with a rescaled sum, best scaled logit, conf = exp(best - max) / sum)."""
    f = np.float32
    c = np.asarray(canvas, dtype=f)
    Q = c.shape[0]
    shp = c.shape[1:]
    qi = np.arange(Q) if K == Q else np.asarray(query_idx).reshape(-1)
    v = c * f(scale)
    thd = f(thd)
    below = (lambda b: b <= thd) if mut == "le_threshold" else (lambda b: b < thd)
    with np.errstate(invalid="ignore", over="ignore"):
        if form == "online":
            vmax, s = np.full(shp, -np.inf, dtype=f), np.zeros(shp, dtype=f)
            best, best_c = np.full(shp, -np.inf, dtype=f), np.zeros(shp, dtype=np.int64)
            for q0 in range(0, Q, 8):
                ch = v[q0:q0 + 8]
                cm = ch.max(0)
                mv = cm > vmax
                if mut != "online_no_rescale":
                    s = np.where(mv, s * np.exp(np.where(mv, vmax - cm, f(0))), s)
                vmax = np.where(mv, cm, vmax)
                for k in range(ch.shape[0]):
                    s = s + np.exp(ch[k] - vmax)
                    cq = int(qi[q0 + k])
                    if 0 <= cq < K:
                        tie = (ch[k] == best) & ((cq > best_c) if mut == "tie_highest_class" else (cq < best_c))
                        up = (ch[k] > best) | (tie if mut != "tie_lowest_query" else False)
                        best, best_c = np.where(up, ch[k], best), np.where(up, cq, best_c)
            conf = np.exp(best - vmax) / s
            return dict(probs=None, labels=np.where(below(conf), bg, best_c), conf=conf)
        mx = v.max(0)
        e = np.exp(v - mx)
        s = np.zeros(shp, dtype=f)
        for q in range(Q):
            s = s + e[q]
        p = e / s
        if form == "wide":
            same = len(set(qi.tolist())) == 1
            probs = np.zeros((K,) + shp, dtype=f)
            if same and 0 <= qi[0] < K and mut != "no_zeros_in_max":
                probs[qi[0]] = -np.inf
            if mut == "no_zeros_in_max":
                probs[:] = -np.inf
            best, arg = np.full(shp, -np.inf, dtype=f), np.zeros(shp, dtype=np.int64)
            for q in range(Q):
                cq = int(qi[q])
                if not 0 <= cq < K:
                    continue
                probs[cq] = np.maximum(probs[cq], p[q])
                tie = (p[q] == best) & ((cq > arg) if mut == "tie_highest_class" else (cq < arg))
                up = (p[q] > best) | (tie if mut != "tie_lowest_query" else False)
                best, arg = np.where(up, p[q], best), np.where(up, cq, arg)
        else:
            probs = np.zeros((K,) + shp, dtype=f)
            best, arg = np.full(shp, -np.inf, dtype=f), np.zeros(shp, dtype=np.int64)
            for cq in range(K):
                own = [q for q in range(Q) if qi[q] == cq]
                m = np.full(shp, -np.inf, dtype=f)
                for q in own:
                    m = np.maximum(m, p[q])
                pc = np.maximum(m, f(0)) if (len(own) < Q and mut != "no_zeros_in_max" and K != Q) else m
                probs[cq] = pc
                up = (pc >= best) if mut == "tie_highest_class" else (pc > best)
                best, arg = np.where(up, pc, best), np.where(up, cq, arg)
    return dict(probs=probs, labels=np.where(below(best), bg, arg), conf=best)


def make_tail_case(Q, HW, classes, data, seed=0):
    """(canvas f32 [Q,1,HW], query_idx int32 [Q], K).  classes: 'ident' K = Q; 'merge' K about Q / 2, shuffled; 'unnamed' classes {0, 2} of
    K = 3 (class 1 owns no query); 'outside' as 'merge' with query 0 in class -1 and the last in class K; 'one' every query in class 0 of
    K = 1.  data: 'plain' 0.25 N(0,1); 'spread' every second pixel with queries down to -120 / scale below the maximum (terms that
    underflow); 'offset' plain + 100."""
    rng = np.random.default_rng(977 * seed + 31 * Q + HW)
    c = 0.25 * rng.standard_normal((Q, 1, HW))
    if data == "spread" and Q > 1:
        c[:, :, ::2] -= (rng.uniform(80.0, 120.0, (Q, 1, (HW + 1) // 2)) / 50.0) * (np.arange(Q) % 2)[:, None, None]
    elif data == "offset":
        c += 100.0
    if classes == "ident" or Q == 1:
        K, qi = Q, np.arange(Q)
    elif classes in ("merge", "outside"):
        K = max(1, Q // 2)
        qi = np.concatenate([np.arange(K), rng.integers(0, K, Q - K)])
        rng.shuffle(qi)
        if classes == "outside" and Q >= 4:
            qi[0], qi[-1] = -1, K
    elif classes == "unnamed":
        K, qi = min(3, Q), np.array([2, 0] * Q)[:Q] if Q >= 3 else np.zeros(Q, dtype=np.int64)
    else:
        K, qi = 1, np.zeros(Q, dtype=np.int64)
    return c.astype(np.float32), qi.astype(np.int32), int(K)


def tie_case(Q, merged, shape=(1, 70), seed=0):
    """Two bit-identical query planes (queries qa < qb) that dominate every element -> (planes f32 [Q, *shape], query_idx, K, the class
    that must win).  K = Q: class(q) = q, the lower class is query qa's.  `merged` (Q >= 3): K < Q and the HIGHER class owns the LOWER
    query index, so a tail that lets the first query win, or the last class, gives the wrong label."""
    rng = np.random.default_rng(4242 + 13 * Q + seed)
    c = (0.1 * rng.standard_normal((Q,) + tuple(shape))).astype(np.float32)
    qa, qb = min(1, Q - 2), Q - 1
    c[qa] = c[qb] = (0.1 * rng.standard_normal(tuple(shape)) + 1.0).astype(np.float32)
    if not merged:
        return c, np.arange(Q, dtype=np.int32), Q, qa
    K = max(2, Q // 2)
    assert K < Q
    qi = np.arange(Q) % K
    qi[qa], qi[qb] = K - 1, 0
    return c, qi.astype(np.int32), int(K), 0


# ---- render_maps ---------------------------------------------------------------------------------------------------------------------------
def render_reference(labels, probs, palette, mut=None):
    """(mask uint8 [...,3], heat uint8 [...,3]) exactly as render_maps_kernel writes them: mask = palette[clip(label, 0, K - 1)];
    g = uint8(trunc(f32(clip(nan_to_num(max_k probs, nan = 0), 0, 1)) * f32(255))), heat = (g, 0, 255 - g).  An f32 reproduction: equality
    is exact."""
    pal = np.asarray(palette, dtype=np.uint8)
    K = pal.shape[0]
    lab = np.asarray(labels).astype(np.int64)
    mask = pal[np.mod(lab, K)] if mut == "label_unclipped" else pal[np.clip(lab, 0, K - 1)]
    p = np.asarray(probs, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(p).any(0), np.float32(0), np.nan_to_num(p, nan=-np.inf, posinf=np.inf, neginf=-np.inf).max(0))
        c = np.clip(c, np.float32(0), np.float32(1)).astype(np.float32)
        prod = c * np.float32(255.0)
        g = (np.rint(prod) if mut == "heat_rounded" else np.trunc(prod)).astype(np.uint8)
    heat = np.stack([g, np.zeros_like(g), (255 - g.astype(np.int64)).astype(np.uint8)], -1)
    return mask, heat


def make_render_case(HW, K, seed=0):
    """labels int64 [HW] with -1, K and 255 among them; probs f32 [K,HW] with NaN, +-inf, values outside [0,1], uniform
    values in (0,1) and k / 255."""
    rng = np.random.default_rng(31 * HW + K + seed)
    labels = rng.integers(0, K, HW).astype(np.int64)
    probs = rng.uniform(0.0, 1.0, (K, HW)).astype(np.float32)
    m = min(HW, 256)
    probs[0, :m:2] = (np.arange(0, m, 2, dtype=np.float64) / 255.0).astype(np.float32)      # even pixels: k / 255 exactly (as f32), k = pixel
    probs[1:, :m] = 0.5 * probs[0, :m]                                     # class 0 is the maximum there
    special = [(-1, np.nan), (K, np.inf), (255, -np.inf), (0, 1.5), (K - 1, -0.25)]
    for j, (lab, val) in enumerate(special):
        if HW > 1:
            i = HW - 1 - (j % HW)
            labels[i] = lab
            probs[(j + 1) % K, i] = val
    if HW == 1:
        labels[0], probs[K - 1, 0] = -1, np.nan
    return labels, probs


def make_palette(K):
    return ((np.arange(K * 3).reshape(K, 3) * 37 + 11) % 256).astype(np.uint8)


# ---- the cases the GPU module runs (the CPU module runs the same ones through the emulations) --------------------------------------------
def _wide_windows(k):
    """k windows that all cover the 4 x 64 canvas and reach past each of its sides: more than 64 of them is the every-window branch."""
    return [(-(i % 2), 5 - (i % 2), -(i % 5), 68 - (i % 5)) for i in range(k)]


# name -> (windows, (gh, gw), up_hw, pad_tl, (H, W)): hand-built window lists; gh != gw, up_h != up_w, pad_t != pad_l everywhere
HAND_STITCH = {
    "w64": (_wide_windows(64), (2, 3), (6, 70), (1, 2), (4, 64)),         # exactly ST_MAXC candidates over the one block: the list
    "w65": (_wide_windows(65), (2, 3), (6, 70), (1, 2), (4, 64)),         # one more: every window is tested
    "hole": ([(0, 3, 0, 30), (2, 5, 40, 65)], (2, 3), (4, 32), (1, 2), (5, 65)),          # columns 30 .. 39 and two corners uncovered
    "1x1": ([(-1, 2, -2, 3), (0, 1, 0, 1)], (3, 2), (4, 7), (1, 2), (1, 1)),
    "3x63": ([(-1, 3, -2, 40), (0, 3, 30, 65), (-1, 2, 0, 63)], (2, 5), (6, 70), (1, 2), (3, 63)),
}
STITCH_CASES = [("a", 1, "plain"), ("a", 8, "offset"), ("b", 7, "plain"), ("b", 9, "offset"), ("dense", 17, "plain"), ("dense", 7, "offset"),
                ("w64", 9, "plain"), ("w65", 8, "offset"), ("w65", 17, "plain"), ("hole", 7, "plain"), ("1x1", 1, "offset"), ("1x1", 9, "plain"),
                ("3x63", 17, "offset"), ("3x63", 8, "plain")]


def stitch_geometry(name):
    """-> (windows int32 [T,4], (gh, gw), up_hw, pad_tl, (H, W))"""
    if name in HAND_STITCH:
        w, grid, up, pad, hw = HAND_STITCH[name]
        return np.asarray(w, dtype=np.int32), grid, up, pad, hw
    H, W, stride, crop, grid, up, pad = GEOMETRIES[name]
    return np.asarray(slide_windows(H, W, stride, crop), dtype=np.int32), grid, up, pad, (H, W)


def make_stitch_case(name, Q, data, seed=0):
    """dict(tile_logits f32 [T,Q,gh,gw], windows, up_hw, pad_tl, hw).  data: 'plain' N(0, 0.3^2), 'offset' the same + 100."""
    wins, grid, up, pad, hw = stitch_geometry(name)
    rng = np.random.default_rng(100 * seed + 7 * Q + len(name))
    tl = 0.3 * rng.standard_normal((len(wins), Q) + tuple(grid)) + (100.0 if data == "offset" else 0.0)
    return dict(tile_logits=tl.astype(np.float32), windows=wins, up_hw=up, pad_tl=pad, hw=hw)


def one_hot_cases(name, tile):
    """A single 1.0 moved over every grid cell of tile `tile`, one query plane per cell, in batches of at most 17 planes: any wrong tap or
    swapped axis is an O(1) error."""
    wins, grid, up, pad, hw = stitch_geometry(name)
    cells = grid[0] * grid[1]
    out = []
    for c0 in range(0, cells, 17):
        Q = min(17, cells - c0)
        tl = np.zeros((len(wins), Q) + tuple(grid), dtype=np.float32)
        for k in range(Q):
            tl[tile, k].reshape(-1)[c0 + k] = 1.0
        out.append(dict(tile_logits=tl, windows=wins, up_hw=up, pad_tl=pad, hw=hw))
    return out


MULTI_HW = [(40, 70), (32, 32), (50, 33)]


def make_multi_case(Q, seed=0):
    """Three images of different sizes in one call: dict(tile_logits [T,Q,3,4], windows [T,4] in each image's coordinates, tile_image [T],
    image_hw, image_tiles [(first, count)], up_hw, pad_tl, per_image [(windows, slice)])."""
    rng = np.random.default_rng(555 + Q + seed)
    wins = [slide_windows(h, w, 20, 32) for h, w in MULTI_HW]
    counts = [len(w) for w in wins]
    first = [0] + list(np.cumsum(counts)[:-1])
    tl = (0.3 * rng.standard_normal((sum(counts), Q, 3, 4))).astype(np.float32)
    return dict(tile_logits=tl, windows=np.asarray([w for ws in wins for w in ws], dtype=np.int32),
                tile_image=np.asarray([n for n, k in enumerate(counts) for _ in range(k)], dtype=np.int32), image_hw=MULTI_HW,
                image_tiles=[(int(a), int(k)) for a, k in zip(first, counts)], up_hw=(40, 44), pad_tl=(1, 2))


RESIZE_SHAPES = (((1, 1), (5, 7)), ((2, 3), (5, 4)), ((7, 9), (21, 30)), ((16, 16), (9, 11)), ((3, 4), (200, 70)), ((10, 12), (10, 12)),
                 ((5, 6), (1, 1)))
RESIZE_C = (1, 2, 5)

PP_Q, PPW_Q, PP_HW = (1, 2, 15, 16, 17, 63, 64), (1, 7, 64, 65, 130), (1, 255, 256, 257)
TAIL_CLASSES, TAIL_DATA = ("ident", "merge", "unnamed", "outside", "one"), ("plain", "spread", "offset")


def tail_cases(qs):
    """A covering subset of Q x HW x class map x data: every Q with every class map, HW and data rotating."""
    return [(Q, PP_HW[(i + j) % 4], cl, TAIL_DATA[(i + 2 * j) % 3]) for i, Q in enumerate(qs) for j, cl in enumerate(TAIL_CLASSES)]


HEAD_Q = (7, 9, 64, 65, 130)
# (geometry, Q, sign of the 0.05 q plane offset, merged class map)
HEAD_CASES = [("a", Q, s, (i + (s > 0)) % 2 == 1) for i, Q in enumerate(HEAD_Q) for s in (+1, -1)] + \
             [("dense", Q, (+1, -1)[i % 2], i % 2 == 0) for i, Q in enumerate(HEAD_Q)]


def make_head_case(geom, Q, sign, merge):
    """make_case with plane q offset by sign * 0.05 q: the online maximum moves in every chunk (+) or never (-)."""
    c = make_case(geom, Q, merge, seed=3)
    c["tile_logits"] = (c["tile_logits"] + np.float32(sign * 0.05) * np.arange(Q, dtype=np.float32)[None, :, None, None]).astype(np.float32)
    return c
