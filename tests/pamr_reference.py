"""float64 reference of PAMR (the definition in include/segearth_hip.h, sg_pamr) with a per-element bound for an f32 evaluation.  Test
infrastructure only; shared by tests/test_pamr_bound_cpu.py and tests/test_gpu_pamr.py.

``weights`` and ``step`` are ONE restatement of the definition in numpy, run in float64 (``reference``) or in float32 (``emulate``: the
kernels' arithmetic, same order of the sums, no fused multiply-add), optionally with one of the MUTATIONS.

The bound.  u = 2^-24; ASSUMPTIONS (those of rowops_reference.py): expf within 2 ulp (EXPF), sqrtf and the division budgeted one ulp
(SQRT = 2 u) each.  n = 9D window samples, K = 8D neighbours.  Per pixel and channel, with c the centre value, e_i = v_i - c the samples'
differences to it, R = max |e_i| and sigma the reference's standard deviation:
  mean of e      : the e_i carry u R, their sequential sum (n - 1) u sum|e_i|, the division 2 u       -> (n + 2) u R
  deviations     : e_i - mean, one more rounding of a value below 2 R                                  -> (n + 5) u R =: dd
  ss = sum dev^2 : 2 sum|dev| dd + n u ss, and sum|dev| <= sqrt(n ss) = sqrt(n (n - 1)) sigma
  sigma          : sqrt(ss / (n - 1)) with 2 u for the division and 2 u for the root:
                     dsigma = (n + 5) sqrt(n / (n - 1)) u R + (n / 2 + 3) u sigma                      <- THE SIGMA TERM
  den            : 1e-8 + 0.1 sigma with the two constants and two operations rounded                  -> 0.1 dsigma + 3 u den
  t = |d| / den  : d rounded (u), the division (2 u)                                                   -> t (6 u + 0.1 dsigma / den)
  a_k = -sum_c t / 3 : two additions and a division                                                    -> da_k = sum_c dt / 3 + 4 u |a_k|
  x_k = a_k - max : a shift common to all k cancels in the softmax                                     -> eps_k = da_k + u |x_k|
  w_k            : exp (EXPF each for numerator and sum), the sum of K terms, the division:
                     dw_k = w_k (expm1(eps_k + sum_j w_j eps_j) + 2 EXPF + (K + 1) u)
The sigma term is carried by 0.1 dsigma / den: where sigma is far above 1e-7 it is a relative (n + 5) sqrt(n / (n - 1)) R / sigma u on
every t, and R <= 2 sqrt(n - 1) sigma; the differences to the centre are what keeps it relative (a mean of the raw values would carry
u |v| instead of u R, which is the conditioning note of the header).
A step: E_{t+1}(p) = sum_k w_k E_t(n_k) + sum_k dw_k |m_t(n_k)| + K u sum_k w_k |m_t(n_k)| (the error already there, averaged; the
weights' error; K products and additions): linear in the number of steps.  Every bound carries SLACK = 1 + 1e-3 for the second-order
terms and + F32_TINY so that an exact zero has a non-zero bound.
"""
import numpy as np

from gemm_reference import U
from rowops_reference import EXPF, F32_TINY

SLACK = 1.0 + 1e-3
OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
PIXEL_MEAN = (122.771, 116.746, 104.094)
PIXEL_STD = (68.501, 66.632, 70.323)
MUTATIONS = ("biased_std", "centre_once", "zero_pad", "no_tenth", "channel_sum", "softmax_per_dilation", "in_place", "mirrored_offset")
KINDS = ("noise", "smooth", "blocks", "flat")


def shift(a, dy, dx, zero_pad=False):
    """a[..., clamp(y + dy), clamp(x + dx)] (replicate padding), or zeros outside with ``zero_pad``."""
    H, W = a.shape[-2:]
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    out = a[..., np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]]
    if zero_pad:
        ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        out = np.where(ok, out, np.zeros((), dtype=a.dtype))
    return out


def weights(g, dilations, dt=np.float64, mut=None, want_bound=False):
    """g [3,H,W] -> w [8D,H,W] in dtype ``dt`` (and its f32-evaluation bound, float64, with ``want_bound``)."""
    g = np.asarray(g).astype(dt)
    D = len(dilations)
    n, K = 9 * D, 8 * D
    zp = mut == "zero_pad"
    offs = list(OFFSETS)
    if mut == "mirrored_offset":
        offs[2] = (1, 1)                                                    # (-1, 1) mirrored in y
    win = [(d * dy, d * dx) for d in dilations for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    if mut == "centre_once":
        win = [o for i, o in enumerate(win) if o != (0, 0) or i == 4]
    nw = len(win)
    one = dt(1)
    asum = [np.zeros(g.shape[1:], dtype=dt) for _ in range(K)]
    dasum = [np.zeros(g.shape[1:]) for _ in range(K)]
    for c in range(3):
        ctr = g[c]
        e = [shift(g[c], dy, dx, zp) - ctr for dy, dx in win]
        tot = np.zeros_like(ctr)
        for v in e:
            tot = tot + v
        mean = tot / dt(nw)
        ss = np.zeros_like(ctr)
        for v in e:
            dv = v - mean
            ss = ss + dv * dv
        sigma = np.sqrt(ss / dt(nw if mut == "biased_std" else nw - 1))
        den = dt(1e-8) + (one if mut == "no_tenth" else dt(0.1)) * sigma
        if want_bound:
            R = np.max(np.abs(np.stack(e)), 0).astype(np.float64)
            dsig = (n + 5) * np.sqrt(n / (n - 1)) * U * R + (n / 2 + 3) * U * sigma
        k = 0
        for d in dilations:
            for dy, dx in offs:
                t = np.abs(ctr - shift(g[c], d * dy, d * dx, zp)) / den
                asum[k] = asum[k] + t
                if want_bound:
                    dasum[k] = dasum[k] + t * (6 * U + 0.1 * dsig / den)
                k += 1
    a = np.stack([-s if mut == "channel_sum" else -s / dt(3) for s in asum])
    if mut == "softmax_per_dilation":
        a5 = a.reshape(D, 8, *a.shape[1:])
        ex = np.exp(a5 - a5.max(1, keepdims=True))
        w = (ex / ex.sum(1, keepdims=True) / dt(D)).reshape(a.shape)
    else:
        ex = np.exp(a - a.max(0, keepdims=True))
        tot = np.zeros_like(ex[0])
        for k in range(K):
            tot = tot + ex[k]
        w = ex / tot
    w = w.astype(dt)
    if not want_bound:
        return w
    da = np.stack(dasum) / 3 + 4 * U * np.abs(a)
    eps = da + U * np.abs(a - a.max(0, keepdims=True))
    bw = w * (np.expm1(eps + (w * eps).sum(0, keepdims=True)) + 2 * EXPF + (K + 1) * U)
    return w, bw


def step(w, m, dilations, mut=None):
    """One step in the dtype of ``w`` and ``m``: out[q,p] = sum_k w_k(p) m[q, n_k(p)], k ascending."""
    offs = list(OFFSETS)
    if mut == "mirrored_offset":
        offs[2] = (1, 1)
    if mut == "in_place":                                                   # raster order, reading what this step has already written
        out = m.copy()
        H, W = m.shape[-2:]
        for y in range(H):
            for x in range(W):
                acc = np.zeros(m.shape[0], dtype=m.dtype)
                k = 0
                for d in dilations:
                    for dy, dx in offs:
                        acc = acc + w[k, y, x] * out[:, min(max(y + d * dy, 0), H - 1), min(max(x + d * dx, 0), W - 1)]
                        k += 1
                out[:, y, x] = acc
        return out
    out = np.zeros_like(m)
    k = 0
    for d in dilations:
        for dy, dx in offs:
            out = out + w[k][None] * shift(m, d * dy, d * dx, mut == "zero_pad")
            k += 1
    return out


def step_bound(w, bw, m, E, dilations):
    """The error bound after one more step (module docstring): w, bw, m = the reference's weights, their bound and m_t; E = the bound on m_t."""
    K = w.shape[0]
    out = np.zeros_like(m)
    k = 0
    for d in dilations:
        for dy, dx in OFFSETS:
            mk = np.abs(shift(m, d * dy, d * dx))
            out = out + w[k][None] * shift(E, d * dy, d * dx) + (bw[k] + K * U * w[k])[None] * mk
            k += 1
    return out


def reference(g, m0, dilations, steps):
    """-> dict(w, bw, out={t: m_t}, bound={t: bound_t}) for every t in ``steps`` (an iterable of step counts), all float64."""
    steps = sorted(set(int(t) for t in steps))
    w, bw = weights(g, dilations, want_bound=True)
    res = dict(w=w, bw=bw * SLACK + F32_TINY, out={}, bound={})
    m = np.asarray(m0).astype(np.float64)
    E = np.zeros_like(m)
    for t in range(0, (steps[-1] if steps else 0) + 1):
        if t in steps:
            res["out"][t], res["bound"][t] = m, E * SLACK + F32_TINY
        if t < steps[-1]:
            E = step_bound(w, bw, m, E, dilations)
            m = step(w, m, dilations)
    return res


def emulate(g, m0, dilations, steps, mut=None):
    """The same in float32 (inputs rounded to f32 first), optionally mutated -> (w, m_steps)."""
    w = weights(np.asarray(g, dtype=np.float32), dilations, dt=np.float32, mut=mut)
    m = np.asarray(m0, dtype=np.float32)
    for _ in range(int(steps)):
        m = step(w, m, dilations, mut=mut)
    return w, m


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def normalise(u8):
    """u8 [H,W,3] -> f32 [3,H,W], (u - mean) / std in f32 as the ingest computes it."""
    x = u8.astype(np.float32).transpose(2, 0, 1)
    mean = np.asarray(PIXEL_MEAN, dtype=np.float32)[:, None, None]
    std = np.asarray(PIXEL_STD, dtype=np.float32)[:, None, None]
    return np.ascontiguousarray(((x - mean) / std).astype(np.float32))


def image_u8(kind, H, W, seed=0):
    """The guidance images of the tests, u8 [H,W,3]: uniform noise, bicubically smoothed noise, 16-pixel constant blocks, flat."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "smooth":
        import torch
        lo = torch.from_numpy(rng.uniform(0, 255, (1, 3, -(-H // 8) + 2, -(-W // 8) + 2)))
        up = torch.nn.functional.interpolate(lo, size=(H, W), mode="bicubic", align_corners=False)[0]
        return up.clamp(0, 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    if kind == "blocks":
        b = rng.integers(0, 256, (-(-H // 16), -(-W // 16), 3), dtype=np.uint8)
        return np.kron(b, np.ones((16, 16, 1), dtype=np.uint8))[:H, :W].copy()
    if kind == "flat":
        return np.full((H, W, 3), 93, dtype=np.uint8)
    raise ValueError(kind)


def logits(Q, H, W, seed=0):
    return (0.2 + 0.1 * np.random.default_rng(1000 + seed).standard_normal((Q, H, W))).astype(np.float32)
