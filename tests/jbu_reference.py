"""f64 references and per-element error bounds for the pieces of the HIP JBU upsampler (csrc/jbu.hip; used by
tests/test_gpu_jbu_reference.py and tests/test_jbu_bound_cpu.py).

Every piece is checked on the operands its kernel actually consumed -- captured from the real kernel sequence with sg_jbu_set_capture
and decoded from their storage -- so errors do not compound across stages.  Every bound is built term by term from the magnitudes of those
operands, never from the observed outputs; each term is documented where it is added.  Layouts are pixel-major: a stage's features are
[B, h, w, C], its kernel rows [B, H, W, d*d] (H = 2h, W = 2w).  Plain torch; everything runs on whatever device its inputs live on.
"""
from __future__ import annotations

import math

import torch

from gemm_reference import U, H2_REL, half_ulp, h2_delta, pack_h2, unpack_h2, gemm_reference, gemm_bound, check_within  # noqa: F401

KEY_DIM = 32
A_CUBIC = -0.75
F32_TENTH = float(torch.tensor(0.1, dtype=torch.float32))       # the f32 constant 0.1f of the GEMM epilogues and the load-time bias scale
EXPF = 2.0 ** -22                                                # ASSUMPTION (as attention_reference): expf, exp2, rcp within 2 ulp
LOWRES = {5: dict(LW=12, OFF=4, KP=160), 3: dict(LW=10, OFF=3, KP=128)}   # LowCfg<R>: low-res window side, origin offset, K slots


# ---- storage -----------------------------------------------------------------------------------------------------------------------
def decode(raw: torch.Tensor, fmt: str, cols: int, rows=None) -> torch.Tensor:
    """Captured bytes (uint8) of rows of `cols` elements in `fmt` ('f32', 'bf16', 'f16', 'h2') -> float64 [rows, cols] (`rows`: only
    those row indices, selected before the conversion)."""
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "h2": torch.float16}[fmt]
    v = raw.view(dt).view(-1, 2 * cols if fmt == "h2" else cols)
    if rows is not None:
        v = v[rows]
    return unpack_h2(v) if fmt == "h2" else v.double()


def encode(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """The bytes a kernel stores for the f32 values x [rows, cols] in `fmt` (round to nearest even; f16 saturating; two-plane split)."""
    x = x.float().contiguous()
    if fmt == "f32":
        q = x
    elif fmt == "bf16":
        q = x.to(torch.bfloat16)
    elif fmt == "f16":
        q = x.clamp(-65504.0, 65504.0).half()
    elif fmt == "h2":
        q = pack_h2(x)
    else:
        raise ValueError(fmt)
    return q.contiguous().view(torch.uint8).reshape(-1)


def rounded(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """f32 values rounded to `fmt` as f64 (two-plane: hi + lo)."""
    cols = x.shape[-1]
    return decode(encode(x, fmt), fmt, cols).view(x.shape)


def store_bound(mag: torch.Tensor, fmt: str) -> torch.Tensor:
    """The error of storing a value of magnitude <= mag in `fmt`."""
    return h2_delta(mag) if fmt == "h2" else half_ulp(mag, fmt)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def reflect(u: torch.Tensor, n: int, mode: str = "reflect") -> torch.Tensor:
    """F.pad(mode='reflect') index map (pad < n); 'replicate' for the mutation tests."""
    if mode == "replicate":
        return u.clamp(0, n - 1)
    u = torch.where(u < 0, -u, u)
    return torch.where(u >= n, 2 * (n - 1) - u, u)


def cubic_taps(n_in: int, n_out: int, *, A: float = A_CUBIC, align_corners: bool = False, device="cpu"):
    """torch's bicubic upsampling along one axis: (idx [n_out, 4] long, w [n_out, 4] f64) with the 4 taps clamped into [0, n_in)."""
    dst = torch.arange(n_out, dtype=torch.float64, device=device)
    if align_corners:
        src = dst * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        src = (n_in / n_out) * (dst + 0.5) - 0.5
    fl = torch.floor(src)
    t = src - fl

    def c1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def c2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A

    w = torch.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], 1)
    idx = (fl.long()[:, None] - 1 + torch.arange(4, device=device)[None]).clamp(0, n_in - 1)
    return idx, w


def bicubic_rows(src: torch.Tensor, b, y, x, H: int, W: int, **kw):
    """(value, magnitude) of bicubic2x(src) at hi-res pixels (b, y, x): src [B, h, w, C] f64 -> [n, C] each; the magnitude is
    sum_s |w_s| |src_s| over the 16 taps (clamped taps counted separately, as the kernels add them)."""
    _, h, w, _ = src.shape
    iy, wy = cubic_taps(h, H, device=src.device, **kw)
    ix, wx = cubic_taps(w, W, device=src.device, **kw)
    iy, wy, ix, wx = iy[y], wy[y], ix[x], wx[x]
    val = torch.zeros(b.shape[0], src.shape[-1], dtype=torch.float64, device=src.device)
    mag = torch.zeros_like(val)
    for a in range(4):
        for k in range(4):
            v = src[b, iy[:, a], ix[:, k]]
            c = (wy[:, a] * wx[:, k])[:, None]
            val += c * v
            mag += c.abs() * v.abs()
    return val, mag


def window_abs_sum(src: torch.Tensor, b, y, x, r: int) -> torch.Tensor:
    """Sum of |src| over the in-image part of the low-res window a pixel's 8 x 8 block stages in jbu_conv_lowres*_kernel<r>
    (origin (ty0 / 2 - OFF, tx0 / 2 - OFF), side LW): the floor terms of the f16 / two-plane Keff elements live there."""
    L = LOWRES[r]
    B, h, w, C = src.shape
    P = torch.zeros(B, h + 1, w + 1, C, dtype=torch.float64, device=src.device)
    P[:, 1:, 1:] = src.abs().cumsum(1).cumsum(2)
    y0 = ((y // 8) * 8) // 2 - L["OFF"]
    x0 = ((x // 8) * 8) // 2 - L["OFF"]
    ya, yb = y0.clamp(0, h), (y0 + L["LW"]).clamp(0, h)
    xa, xb = x0.clamp(0, w), (x0 + L["LW"]).clamp(0, w)
    return P[b, yb, xb] - P[b, ya, xb] - P[b, yb, xa] + P[b, ya, xa]


def sample_all(B, H, W, device):
    g = torch.stack(torch.meshgrid(torch.arange(B, device=device), torch.arange(H, device=device), torch.arange(W, device=device),
                                   indexing="ij"), -1).reshape(-1, 3)
    return g[:, 0], g[:, 1], g[:, 2]


def sample_border_blocks(B, H, W, n_random, seed, device):
    """All border rows and columns; in every 8 x 8 block its corner (7, 7), one random pixel of its last row and one of its last column
    (ragged blocks: their last row / column inside the image); a random sample; the last pixel of the last image."""
    gen = torch.Generator().manual_seed(seed)
    pts = []
    for b in range(B):
        for yy in (0, H - 1):
            xs = torch.arange(W)
            pts.append(torch.stack([torch.full_like(xs, b), torch.full_like(xs, yy), xs], -1))
        for xx in (0, W - 1):
            ys = torch.arange(H)
            pts.append(torch.stack([torch.full_like(ys, b), ys, torch.full_like(ys, xx)], -1))
        by, bx = torch.meshgrid(torch.arange(0, H, 8), torch.arange(0, W, 8), indexing="ij")
        by, bx = by.reshape(-1), bx.reshape(-1)
        ly, lx = (by + 7).clamp(max=H - 1), (bx + 7).clamp(max=W - 1)
        ry = torch.minimum(by + torch.randint(0, 8, by.shape, generator=gen), ly)
        rx = torch.minimum(bx + torch.randint(0, 8, bx.shape, generator=gen), lx)
        bb = torch.full_like(by, b)
        pts += [torch.stack([bb, ly, lx], -1), torch.stack([bb, ly, rx], -1), torch.stack([bb, ry, lx], -1)]
    pts.append(torch.stack([torch.randint(0, n, (n_random,), generator=gen) for n in (B, H, W)], -1))
    pts.append(torch.tensor([[B - 1, H - 1, W - 1]]))
    p = torch.unique(torch.cat(pts), dim=0).to(device)
    return p[:, 0], p[:, 1], p[:, 2]


# ---- range kernel ------------------------------------------------------------------------------------------------------------------
def range_reference(proj, r: int, range_temp: float, sigma: float, keys: str, b, y, x, *, pad="reflect", spatial=True, clamp=1e-7):
    """X rows (the normalised range x spatial kernel) of pixels (b, y, x) in f64 from the captured f32 keys proj [B, H, W, 32], with the
    per-element bound of jbu_kernel_tiled_kernel<0,false> (keys 'f32'), jbu_kernel_mfma_kernel<R,false> ('f16': keys staged as f16,
    hardware exp2 / rcp) or jbu_kernel_mfma_kernel<R,true> ('h2': two-plane keys, expf and true division).
    Returns (X [n, d2], bound [n, d2], clamp_fired [n]).

    Terms.  Per tap t the score s_t = temp <k_t, k_c> carries an absolute error Delta_t:
      * key storage: f32 none; f16 sum_k hu(|a|)|b| + |a|hu(|b|) + hu hu (hu = half an f16 ulp, subnormal floor included); two-plane
        sum_k delta(a)|b| + |a|delta(b) + the dropped lo.lo product 2^-22 S (S = sum_k |a||b|);
      * the 32-term f32 accumulation (f32: products rounded too, 33 roundings; f16: 32 exact products; two-plane: 96 products of <= 1.01 S):
        2u n S;
      * temp = clamp(exp(range_temp), 1e-4, 1e4) from expf (EXPF relative) and the product temp * dot (u): |s_t| (EXPF + 2u).
    With Delta = max_t Delta_t the softmax weights of the kernel lie within exp(+-2 Delta) of the exact ones (the shift by the maximum
    cancels).  On top, relative: exp / exp2 of (s_t - max) (EXPF, plus the rounding of the difference and of the log2(e) product:
    3u |s_t - max|), the spatial factor exp(-(fi^2 + fj^2) / (2 sigma^2)) (EXPF plus 8u of its argument for the f32 geometry fi = -1 + i step),
    the 64-lane sum of e (16u), the reciprocal (EXPF) and the products by it and by the spatial factor (4u): rho_k.  The sum of the k_t
    (16u) then has relative error <= max_t rho_k + 16u, clamp(1e-7) does not increase a relative error, and the division (EXPF) and the f32
    store (half an ulp) close the bound.  Where the weights underflow, the subnormal spacing of f32 adds an absolute floor."""
    d = 2 * r + 1
    B, H, W, _ = proj.shape
    p = proj.double()
    kc = p[b, y, x]                                                    # [n, 32]
    temp = min(max(math.exp(range_temp), 1e-4), 1e4)
    s, key_err, S = [], [], []
    for t in range(d * d):
        i, j = divmod(t, d)
        kt = p[b, reflect(y + i - r, H, pad), reflect(x + j - r, W, pad)]
        s.append(temp * (kt * kc).sum(-1))
        Sa = (kt.abs() * kc.abs()).sum(-1)
        S.append(Sa)
        if keys == "f32":
            key_err.append(2 * U * 33 * Sa)
        elif keys == "f16":
            ha, hb = half_ulp(kt.abs(), "f16"), half_ulp(kc.abs(), "f16")
            rep = (ha * kc.abs() + kt.abs() * hb + ha * hb).sum(-1)
            key_err.append(rep + 2 * U * 32 * (Sa + rep))
        elif keys == "h2":
            rep = (h2_delta(kt) * kc.abs() + kt.abs() * h2_delta(kc)).sum(-1) + H2_REL * Sa
            key_err.append(rep + 2 * U * 96 * (1.01 * Sa + rep))
        else:
            raise ValueError(keys)
    s = torch.stack(s, 1)
    delta = temp * torch.stack(key_err, 1) + s.abs() * (EXPF + 2 * U)
    Dm = delta.max(1, keepdim=True).values
    e = torch.softmax(s, 1)
    ii = torch.arange(d * d, device=proj.device) // d
    jj = torch.arange(d * d, device=proj.device) % d
    fi, fj = -1 + ii * (2.0 / (d - 1)), -1 + jj * (2.0 / (d - 1))
    arg = (fi * fi + fj * fj) / (2 * sigma * sigma)
    sp = torch.exp(-arg).double() if spatial else torch.ones_like(arg, dtype=torch.float64)
    k = e * sp[None]
    s2 = k.sum(1, keepdim=True)
    fired = (s2 < clamp).squeeze(1)
    X = k / s2.clamp(min=clamp)
    smax = s.max(1, keepdim=True).values
    rho_k = torch.expm1(2 * Dm) + EXPF + 3 * U * (s - smax).abs() + EXPF + 8 * U * arg[None] + 16 * U + EXPF + 4 * U
    rho_n = rho_k.max(1, keepdim=True).values + 16 * U
    rho = (1 + rho_k) * (1 + rho_n) * (1 + EXPF) - 1
    # f32 underflow: e, e * inv and k may be subnormal, absolute error 2^-150 each (inv <= 1, sp <= 1), amplified by the division by the sum
    bnd = rho * X + 3 * 2.0 ** -150 / s2.clamp(min=clamp) * (1 + rho)
    return X, bnd + half_ulp(X + bnd, "f32"), fired


# ---- adaptive convolution ----------------------------------------------------------------------------------------------------------
def conv_reference(K, r: int, b, y, x, *, src=None, hr=None, pad="reflect", taps=None, transpose=False, **bicubic_kw):
    """out[p, c] = sum_t K[p, t] hr[p (+) t, c] in f64 at pixels (b, y, x), hr = bicubic2x(src) (A = -0.75, align_corners = False,
    torch's border clamp of the 4 taps) or the captured hi-res tensor `hr`, (+) = reflect padding r.  K [B, H, W, >= d2] f64.
    Returns a dict with out and the magnitudes the bounds use: M = sum_t |K_t| A_t (A_t = sum_s |w_s||src_s|, or |hr_t|),
    MK16 = sum_t hu_f16(|K_t|) A_t, MKbf = sum_t hu_bf16(|K_t|) A_t.  `taps` / `transpose` / `pad` / bicubic_kw: mutation hooks."""
    d = 2 * r + 1
    B, H, W = K.shape[:3]
    C = (src if src is not None else hr).shape[-1]
    z = lambda: torch.zeros(b.shape[0], C, dtype=torch.float64, device=K.device)  # noqa: E731
    out, M, MK16, MKbf = z(), z(), z(), z()
    for t in (range(d * d) if taps is None else taps):
        i, j = divmod(t, d)
        if transpose:
            i, j = j, i
        yy, xx = reflect(y + i - r, H, pad), reflect(x + j - r, W, pad)
        if hr is not None:
            v = hr[b, yy, xx].double()
            a = v.abs()
        else:
            v, a = bicubic_rows(src, b, yy, xx, H, W, **bicubic_kw)
        kt = K[b, y, x, t][:, None]
        out += kt * v
        M += kt.abs() * a
        MK16 += half_ulp(kt.abs(), "f16") * a
        MKbf += half_ulp(kt.abs(), "bf16") * a
    return dict(out=out, M=M, MK16=MK16, MKbf=MKbf)


def conv_bound(ref, kind: str, r: int, out_fmt: str, *, src=None, b=None, y=None, x=None) -> torch.Tensor:
    """Per-element bound on |stored kernel output - f64 reference| of one adaptive-convolution kernel (ref: conv_reference's dict).

    * 'valu' (jbu_adaptive_conv_kernel on the captured f32 hr): d2 f32 products and sums, 2u d2 M.
    * 'mfma' (jbu_adaptive_conv_mfma_kernel on the captured bf16 hr): K rounded to bf16 in the kernel, sum_t hu_bf16(|K_t|)|hr_t|; f32
      accumulation over KP = align32((8 + 2r)^2) slots of products <= (1 + 2^-8) M: 2u KP.
    * 'lowres' (jbu_conv_lowres_kernel<r> on the captured bf16 source): out = sum_s Keff_s src_s with Keff = Wy^T K Wx:
      K rows to f16 (sum_t hu_f16(|K_t|) A_t); the two cubic tables to f16 (2 x 2^-11 M, the weights are normal f16 numbers);
      T = K . Wx with f32 dot2 accumulation (2u D M); T to f16 (2^-11 M relative, plus the subnormal floor 2^-25 on every T element, which
      reaches the output through at most 8 table weights <= 1 per low-res row: 8 2^-25 D sum_window |src|); Keff = Wy^T . T with f32 dot2
      accumulation (2u D M); F = Keff to bf16 (2^-8 (1 + 2^-8) M); the bf16 MFMA over KP slots (2u KP (1 + 2^-7) M).
    * 'lowres_x2' (jbu_conv_lowres_x2_kernel<r> on the captured two-plane source): the f32 cubic tables (8u M), T and Keff in f32 (2u D M
      each); Keff split into two f16 planes (2^-22 M + 2^-25 sum_window |src|); the dropped F_lo . src_lo product
      (<= (2^-11 |Keff| + 2^-25)(2^-11 |src| + 2^-25): 2^-22 (1.01) M + 2^-36 sum_window |src|); three MFMAs per product over KP slots
      (2u 3 KP 1.01 M).
    Then the store of the output in out_fmt at the largest magnitude it can have."""
    M = ref["M"]
    D = 2 * r + 1
    if kind == "valu":
        e = 2 * U * D * D * M
    elif kind == "mfma":
        KPm = ((8 + 2 * r) ** 2 + 31) // 32 * 32
        e = ref["MKbf"] + 2 * U * KPm * (1 + 2.0 ** -8) * M
    elif kind in ("lowres", "lowres_x2"):
        L = LOWRES[r]
        S_win = window_abs_sum(src, b, y, x, r)
        if kind == "lowres":
            e = (ref["MK16"] + 2 * 2.0 ** -11 * M + 2 * U * D * M + 2.0 ** -11 * M + 8 * 2.0 ** -25 * D * S_win + 2 * U * D * M
                 + 2.0 ** -8 * (1 + 2.0 ** -8) * M + 2 * U * L["KP"] * (1 + 2.0 ** -7) * M)
        else:
            e = (8 * U * M + 4 * U * D * M + H2_REL * M + 2.0 ** -25 * S_win + H2_REL * 1.01 * M + 2.0 ** -36 * S_win
                 + 2 * U * 3 * L["KP"] * 1.01 * M)
    else:
        raise ValueError(kind)
    return e + store_bound(ref["out"].abs() + e, out_fmt)


def bicubic_bound(mag: torch.Tensor, val: torch.Tensor, out_fmt: str) -> torch.Tensor:
    """jbu_bicubic_kernel: 4-tap rows then the 4-tap column in f32 (2u 4 + 2u 4 relative to sum |wy||wx||src|), the f32 cubic weights
    (4u relative each, two factors), then the store in out_fmt."""
    e = (16 * U + 8 * U) * mag
    return e + store_bound(val.abs() + e, out_fmt)


# ---- small GEMMs -------------------------------------------------------------------------------------------------------------------
def scaled_gemm(A, W, bias01, residual, *, out_fmt: str, two_plane: bool = False):
    """out = residual + 0.1f (A . W^T) + bias01 (the fixup / final 1x1 epilogue: alpha = 0.1f, bias scaled by 0.1f at load), as
    gemm_reference / gemm_bound with W scaled by 0.1f in f64: the alpha product and the bias add are two of gemm_bound's three extra
    roundings, the residual add is covered by the f32 store."""
    Ws = W.double() * F32_TENTH
    pre, ref = gemm_reference(A, Ws, bias01, residual, 0)
    return ref, gemm_bound(A, Ws, bias01, pre, ref, act=0, out_fmt=out_fmt, two_plane=two_plane)


def range_proj_reference(gs, w0, b0, w3, b3):
    """jbu_range_proj_kernel: proj = W3 GELU(W0 g + b0) + b3 per pixel in f32 (erff GELU).  The first layer is a K = 3 GEMM
    (gemm_bound with the exact GELU's Lipschitz constant and erf_gelu's approximation), the second a K = 32 GEMM on the exact hidden
    values whose bound adds the hidden error carried through |W3|."""
    pre0, h = gemm_reference(gs, w0, b0, None, 2)
    bh = gemm_bound(gs, w0, b0, pre0, h, act=2, out_fmt="f32", fast_act=False)
    pre1, proj = gemm_reference(h, w3, b3, None, 0)
    bp = gemm_bound(h, w3, b3, pre1, proj, act=0, out_fmt="f32") + bh @ w3.double().abs().T
    return proj, bp


def pool_reference(g, H: int, W: int):
    """F.adaptive_avg_pool2d(g [B, 3, GH, GW] -> (H, W)) pixel-major [B, H, W, 3] in f64, with the bound of the f32 sum of n terms and
    its division: 2u (n + 1) mean |g|, plus the store.  The windows are separable: out = Py g Px^T with row weights 1 / n_y, 1 / n_x."""
    B, _, GH, GW = g.shape

    def pm(n_in, n_out):
        P = torch.zeros(n_out, n_in, dtype=torch.float64, device=g.device)
        n = torch.zeros(n_out, dtype=torch.float64, device=g.device)
        for o in range(n_out):
            a, b = (o * n_in) // n_out, ((o + 1) * n_in + n_out - 1) // n_out
            P[o, a:b] = 1.0 / (b - a)
            n[o] = b - a
        return P, n

    Py, ny = pm(GH, H)
    Px, nx = pm(GW, W)
    gd = g.double()
    out = torch.einsum("yY,bcYX,xX->byxc", Py, gd, Px)
    mag = torch.einsum("yY,bcYX,xX->byxc", Py, gd.abs(), Px) * (2 * U * (ny[:, None] * nx[None, :] + 1))[None, :, :, None]
    return out, mag + half_ulp(out.abs() + mag, "f32")


def rowdot_reference(x, Wr, bias01, slot_cols: int = 64):
    """The fused tail's row-dot slots: sum over each run of 64 columns of z (2x + z) = |out|^2 - |x|^2 with out = x + z,
    z = 0.1f x . Wr^T + bias01 (x the bf16 rows, Wr the bf16 weight), in f64.  Bound: the GEMM bound bz on z carried through
    z (2x + z) (bz |2x + 2z| + bz^2); the epilogue's f32 arithmetic per element (o = x + z and a difference of squares, or z (2x + z):
    at most four roundings of magnitudes <= o^2 + x^2); the 64-term f32 sum (2u 64 sum |term|); the store."""
    z, bz = scaled_gemm(x, Wr, bias01, None, out_fmt="f32")
    o = x + z
    term = z * (2 * x + z)
    n = x.shape[-1] // slot_cols
    ref = term.view(-1, n, slot_cols).sum(-1)
    e = bz * (2 * x + 2 * z).abs() + bz * bz + 4 * U * (o * o + x * x) + 2 * U * slot_cols * term.abs()
    bnd = e.view(-1, n, slot_cols).sum(-1)
    return ref, bnd + half_ulp(ref.abs() + bnd, "f32")


def median_tightness(bound: torch.Tensor, ref: torch.Tensor) -> float:
    """Median of bound / |ref| over the elements with |ref| above 1e-3 of the largest: how far from vacuous the bound is."""
    a = ref.abs()
    m = a > 1e-3 * float(a.max())
    return float((bound[m] / a[m]).median()) if bool(m.any()) else 0.0
