"""f64 references, per-element error bounds, f32 emulations and case generators for the row kernels of csrc/rowops.hip (used by
tests/test_gpu_rowops_reference.py and tests/test_rowops_bound_cpu.py).

Everything is plain torch / numpy in float64 on the CPU.  A bound is built from the magnitudes of the operands and from the shape of the
kernel's summation -- one wavefront per row: lane l adds the terms l, l + 64, ... (at most T = ceil(terms / 64) of them), then a 6-step
butterfly, so a sum of non-negative or signed terms misses the exact one by at most (T + 6) u sum|term| to first order -- never from
observed outputs.  The output format's half ulp (two-plane: max(2^-22 |x|, 2^-25)) is added per element.

ASSUMPTIONS about the device's libm (nobody has measured them on this part; attention_reference.py makes the first one too):
  * expf within 2 ulp (EXPF = 2^-22 relative), logf within 2 ulp plus 2 u absolute,
  * sqrtf and the f32 division correctly rounded (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt); the bounds budget a full
    ulp (2 u) for each.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from gemm_reference import FORMATS, U, check_within, h2_delta, half_ulp, pack_h2, unpack_h2  # noqa: F401

EXPF = 2.0 ** -22                                  # ASSUMPTION: device expf within 2 ulp
LOGF = 2.0 ** -22                                  # ASSUMPTION: device logf within 2 ulp (relative), + 2 u absolute near log = 0
SQRT = 2 * U                                       # budget for sqrtf / division (correctly rounded by default: 1 u)
KINDS = ("f32", "bf16", "f16", "h2")
PREC = {"f32": 0, "bf16": 1, "f16": 3, "h2": 4}    # sg_precision codes naming a storage
F16_MAX = 65504.0
FP8_MAX = 448.0
FLT_MIN = float(np.finfo(np.float32).tiny)
F32_TINY = 2.0 ** -149                             # spacing of the f32 subnormals: the absolute floor of one rounding


# ---- shared helpers --------------------------------------------------------------------------------------------------------------------
def lane_sum(v):
    """Sum over the last axis as the kernels do: lane l adds elements l, l + 64, ... in order, then the xor butterfly 32, 16, .., 1."""
    pad = (-v.shape[-1]) % 64
    v = torch.nn.functional.pad(v, (0, pad)).view(*v.shape[:-1], -1, 64)
    acc = v[..., 0, :]
    for r in range(1, v.shape[-2]):
        acc = acc + v[..., r, :]
    w = 64
    while w > 1:
        w //= 2
        acc = acc[..., :w] + acc[..., w:2 * w]
    return acc[..., 0]


def group_sum(v, lanes):
    """Sum of `lanes` per-lane partial sums held in the last axis (the 8- / 16-lane DPP butterflies of the short-row kernels)."""
    w = lanes
    while w > 1:
        w //= 2
        v = v[..., :w] + v[..., w:2 * w]
    return v[..., 0]


def vec4_lane_sum(v):
    """LayerNorm's row sum: each float4 as (x + y) + (z + w), lane l adds float4 l, l + 64, ..., then the butterfly."""
    q = v.view(*v.shape[:-1], -1, 4)
    return lane_sum((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))


def depth(terms: int) -> int:
    """Additions on the longest path of a 64-lane strided sum of `terms` terms."""
    return max(1, -(-terms // 64)) + 6


def store(x: torch.Tensor, kind: str) -> torch.Tensor:
    """f32 / f64 values -> the storage `kind` as the kernels write it (round to nearest even, f16 saturating, two-plane groups)."""
    x = x.float()
    if kind == "f32":
        return x
    if kind == "bf16":
        return x.bfloat16()
    if kind == "f16":
        return x.clamp(-F16_MAX, F16_MAX).half()
    return pack_h2(x)


def load(s: torch.Tensor, kind: str) -> torch.Tensor:
    """Storage -> the float64 values it holds."""
    return unpack_h2(s) if kind == "h2" else s.double()


def storage_dtype(kind: str):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "h2": torch.float16}[kind]


def storage_cols(cols: int, kind: str) -> int:
    """Storage elements (of storage_dtype) per `cols` logical elements."""
    return 2 * cols if kind == "h2" else cols


def out_bound(mag: torch.Tensor, kind: str) -> torch.Tensor:
    """Largest error of one round-to-nearest store of a value of magnitude `mag` into `kind`."""
    return h2_delta(mag) if kind == "h2" else half_ulp(mag, kind)


def rounded_once(x: torch.Tensor, kind: str) -> torch.Tensor:
    """The f64 value of x (f32-representable) after ONE rounding to the storage format -- what pack / transpose / patchify must equal."""
    return load(store(x, kind), kind)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
def layernorm_reference(x, gamma, beta, eps, out_kind="f32"):
    """(y, bound) in f64: y = (x - mean) / sqrt(var + eps) * gamma + beta, biased variance, eps inside the square root.

    Bound, with d = depth(D / 4) + 2 (two additions inside a float4): the mean misses by dm = (d + 1) u sum|x| / D; a centred value by
    dc = dm + u |c|; the variance by [sum (2 |c| dc + dc^2) + (d + 2) u sum (|c| + dc)^2] / D; rstd = 1 / sqrt(var + eps) relatively by
    dvar / (2 (var + eps)) + u / 2 (the add) + SQRT (sqrtf) + SQRT (division); the normalised value n = c rstd by rstd dc + |n| (rel +
    u); y = n gamma + beta by |gamma| dn + u |n gamma| + u |y| (+ 2^-148: the two roundings' subnormal floor).  The store adds the output format's half ulp."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    D = x.shape[-1]
    d = depth(D // 4) + 2
    mean = x.mean(-1, keepdim=True)
    c = x - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    n = c * rstd
    y = n * gamma + beta
    dm = (d + 1) * U * x.abs().sum(-1, keepdim=True) / D
    dc = dm + U * c.abs()
    dvar = ((2 * c.abs() * dc + dc * dc).sum(-1, keepdim=True) + (d + 2) * U * ((c.abs() + dc) ** 2).sum(-1, keepdim=True)) / D
    rel = dvar / (2 * (var + eps)) + 0.5 * U + 2 * SQRT
    dn = rstd * dc * (1 + rel) + n.abs() * (rel + U)
    dy = gamma.abs() * dn + U * (n * gamma).abs() + U * (y.abs() + gamma.abs() * dn) + 2 * F32_TINY
    return y, dy + out_bound(y.abs() + dy, out_kind), dy


def layernorm_emulate(x, gamma, beta, eps, mut=None):
    """ln_row in f32 with the kernel's summation shape; `mut` names one of the listed slips."""
    x = x.float()
    D = x.shape[-1]
    eps = torch.tensor(eps, dtype=torch.float32)
    xs = x
    if mut == "drop_last_vec" and (D // 4) % 64 != 0:                    # the statistics and the stores miss the last float4
        xs = x[..., :D - 4]
    Ds = torch.tensor(float(D), dtype=torch.float32)
    if mut == "one_pass":
        mean = vec4_lane_sum(xs)[..., None] / Ds
        var = vec4_lane_sum(xs * xs)[..., None] / Ds - mean * mean
    else:
        mean = vec4_lane_sum(xs)[..., None] / Ds
        c = xs - mean
        var = vec4_lane_sum(c * c)[..., None] / (Ds - 1 if mut == "div_d_minus_1" else Ds)
    rstd = 1.0 / (torch.sqrt(var) + eps) if mut == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    g, b = gamma.float(), beta.float()
    if mut == "gamma_stride":                                            # float4 index used as an element index: gamma[idx .. idx+3]
        idx = (torch.arange(D) // 4)[:, None].squeeze(-1) + torch.arange(D) % 4
        g, b = g[idx], b[idx]
    y = (x - mean) * rstd * g + b
    if mut == "drop_last_vec" and (D // 4) % 64 != 0:
        y[..., D - 4:] = 0.0
    return y


LN_D = (4, 64, 252, 256, 260, 768, 2048)
LN_ROWS = (1, 5, 9)


def make_ln_case(rows, D, seed, offset=1e3, const_row=True):
    """Rows two decades apart; row 1 (if any) with its mean at `offset` times its spread; the last row (rows >= 3) constant.  gamma ~ 1 +-
    0.5, beta ~ +-0.5.  Returns x [rows, D], gamma, beta (f32)."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(rows, D, generator=g)
    x = x * (10.0 ** torch.linspace(-1, 1, rows))[:, None]
    if rows >= 2:
        x[1] = x[1] + offset * x[1].std()
    if rows >= 3 and const_row:
        x[rows - 1] = 0.75
    gamma = 1.0 + 0.5 * torch.randn(D, generator=g).clamp(-1.8, 1.8)
    beta = 0.5 * torch.randn(D, generator=g)
    return x.float(), gamma.float(), beta.float()


def make_ln_fp8_case(rows, D, seed, tiny=False):
    """LayerNorm inputs for the fp8 output: the offset-mean row at 30 times its spread (its larger LayerNorm bound would put more than the
    allowed share of elements on e4m3 rounding boundaries), row 0's largest output in its last element.  `tiny`: gamma scaled to 1e-37 and
    beta = 0, so every row's amax is about 1e-37 and the constant row's output is exactly zero (scale 1, zero bytes)."""
    x, gamma, beta = make_ln_case(rows, D, seed, offset=30.0, const_row=tiny)
    x[0, D - 1] = 8.0 * x[0].abs().max() + 1.0
    gamma[D - 1] = 1.5
    if tiny:
        gamma, beta = gamma * 1e-37, torch.zeros_like(beta)
    return x, gamma, beta


# ---- fp8 (OCP e4m3) row quantisation ------------------------------------------------------------------------------------------------------
def e4m3_rne(v: torch.Tensor):
    """(byte, value) of the e4m3fn code nearest to v (ties to even), |v| clamped to 448: spacing 2^(e-3) for 2^e <= |v| < 2^(e+1), e >= -6;
    2^-9 below 2^-6.  v: float64 tensor."""
    a = v.abs().clamp(max=FP8_MAX)
    _, e = torch.frexp(a)
    e = torch.where(a > 0, e - 1, torch.full_like(e, -6)).clamp(min=-6)
    step = torch.ldexp(torch.ones_like(a), e - 3)
    k = torch.from_numpy(np.rint((a / step).numpy()))                    # round half to even; k in [0, 16]
    q = (k * step).clamp(max=FP8_MAX)
    _, e2 = torch.frexp(q)
    e2 = e2 - 1
    normal = q >= 2.0 ** -6
    expf_ = torch.where(normal, e2 + 7, torch.zeros_like(e2))
    mant = torch.where(normal, (q / torch.ldexp(torch.ones_like(q), e2) - 1.0) * 8.0, q * 2.0 ** 9)
    byte = (expf_.long() * 8 + mant.long()) | torch.where(torch.signbit(v), 128, 0)
    return byte.to(torch.uint8), torch.where(torch.signbit(v), -q, q)


def e4m3_value(byte: torch.Tensor) -> torch.Tensor:
    """The float64 value of e4m3fn bytes (0x7f / 0xff are NaN)."""
    b = byte.long()
    ef, m = (b >> 3) & 15, (b & 7).double()
    mag = torch.where(ef > 0, torch.ldexp(1.0 + m / 8.0, ef - 7), m * 2.0 ** -9)
    mag = torch.where((b & 127) == 127, torch.full_like(mag, float("nan")), mag)
    return torch.where((b & 128) > 0, -mag, mag)


def fp8_scale_f32(amax: np.ndarray, mut=None) -> tuple[np.ndarray, np.ndarray]:
    """(scale, inv) in f32 exactly as the kernels compute them: scale = max(amax / 448, FLT_MIN) for amax > 0, 1 for an all-zero row."""
    amax = amax.astype(np.float32)
    with np.errstate(divide="ignore", over="ignore"):
        sc = np.where(amax > 0, np.maximum(amax / np.float32(240.0 if mut == "amax_240" else FP8_MAX), np.float32(FLT_MIN)), np.float32(1.0))
        sc = sc.astype(np.float32)
        inv = (np.float32(1.0) / sc).astype(np.float32)
    return sc, inv


def quantize_rows_expected(v: torch.Tensor, mut=None):
    """Exact (bytes, scale) of quantize_rows_fp8 on the f32-representable values v [rows, D]: every step reproduced in f32."""
    vn = v.float().numpy()
    amax = np.abs(vn).max(-1)
    if mut == "scale_per_4_rows":
        amax = np.repeat(np.maximum.reduceat(amax, np.arange(0, len(amax), 4)), 4)[:len(amax)]
    sc, inv = fp8_scale_f32(amax, mut)
    with np.errstate(over="ignore", invalid="ignore"):
        p = (vn * inv[:, None]).astype(np.float32)
    p64 = torch.from_numpy(p.astype(np.float64))
    if mut == "truncate":
        byte, val = e4m3_rne(p64)
        over = val.abs() > p64.abs()                                     # step the magnitude code down where rounding went up
        byte = torch.where(over, byte - 1, byte)
        return byte, torch.from_numpy(sc)
    return e4m3_rne(p64)[0], torch.from_numpy(sc)


def fp8_within_half_step(byte, scale, v) -> bool:
    """Bytes finite and q * scale within half an e4m3 step (in q units: 2^(e-4), 2^-10 in the subnormal range) of v."""
    q = e4m3_value(byte)
    if bool(torch.isnan(q).any()):
        return False
    sc = scale.double()[:, None]
    p = v.double() / sc
    _, e = torch.frexp(p.abs())
    half = torch.ldexp(torch.ones_like(p), (e - 1).clamp(min=-6) - 4)
    return bool(((q - p).abs() <= half * (1 + 2.0 ** -20)).all())


def layernorm_fp8_check(byte, scale, x, gamma, beta, eps, what=""):
    """layernorm_fp8 against the f64 LayerNorm: the scale within (the LayerNorm bound at the row maximum) / 448 + u scale of amax / 448; a byte
    equal to e4m3_rne(v inv) for the kernel's own inv = f32(1 / scale), where the f64 pre-image p = v inv -- moved by at most
    delta = dy inv + u |p| (dy: the LayerNorm bound before any store) -- does not reach a rounding boundary; either neighbouring code where it
    does.  Returns (share of such elements, largest scale error / bound)."""
    y, _, dy = layernorm_reference(x, gamma, beta, eps)
    amax, arg = y.abs().max(-1)
    damax = dy.gather(-1, arg[:, None])[:, 0]
    for r in range(y.shape[0]):                                         # another element may overtake the f64 maximum inside its bound
        damax[r] = torch.maximum(damax[r], ((y[r].abs() + dy[r]).max() - amax[r]))
    sc = scale.double()
    zero = amax == 0
    want = torch.where(zero, torch.ones_like(amax), (amax / FP8_MAX).clamp(min=FLT_MIN))
    sb = damax / FP8_MAX + 2 * U * want
    ratio = float(((sc - want).abs() / sb).max())
    assert bool(((sc - want).abs() <= sb).all()), f"{what}: scale {sc.tolist()} vs {want.tolist()} (bound {sb.tolist()})"
    inv = torch.from_numpy((np.float32(1.0) / scale.numpy().astype(np.float32)).astype(np.float64))[:, None]
    p = y * inv
    delta = dy * inv + U * p.abs()
    lo, hi = e4m3_rne(p - delta)[1], e4m3_rne(p + delta)[1]
    q = e4m3_value(byte)
    assert not bool(torch.isnan(q).any()), f"{what}: NaN bytes"
    ok = (q >= lo) & (q <= hi)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} bytes outside the admissible codes; first {(~ok).nonzero()[0].tolist()}"
    share = float((lo != hi).double().mean())
    assert share <= 0.02, f"{what}: {share:.3%} of the elements sit on an e4m3 rounding boundary"
    return share, ratio


def layernorm_fp8_emulate(x, gamma, beta, eps, mut=None):
    """layernorm_fp8_kernel in f32: (bytes, scale)."""
    v = layernorm_emulate(x, gamma, beta, eps)
    return quantize_rows_expected(v, mut)


def make_quant_case(rows, D, seed, kind="f32"):
    """Values in the storage `kind` (returned as storage and as f32): rows decades apart, row 0 all zero (rows >= 3), row 1 tiny
    (amax 1e-37; the f16 storage's smallest subnormals instead), the last row's maximum in its last element."""
    g = torch.Generator().manual_seed(2000 + seed)
    v = torch.randn(rows, D, generator=g) * (10.0 ** torch.linspace(-2, 2, rows))[:, None]
    if rows >= 3:
        v[0] = 0.0
        v[1] = torch.randn(D, generator=g).clamp(-1, 1) * (1e-37 if kind != "f16" else 3e-7)
        v[1, D // 2] = 1e-37 if kind != "f16" else 3e-7
        v[1, 0] = 0.0
    v[rows - 1, D - 1] = 4.0 * v[rows - 1].abs().max() + 1.0
    s = store(v, kind)
    return s, s.float()


# ---- row L2 normalisation ----------------------------------------------------------------------------------------------------------------
def l2norm_reference(x, eps, out_kind, lanes=64):
    """(y, bound): y = x / max(||x||, eps) (F.normalize).  x: the values the kernel read (f64).  The sum of squares over D terms misses by
    (dsum + 1) u ss, dsum the additions on the longest path (general kernel: depth(D); short kernels: 8 per lane + log2(lanes)); its root
    halves that and adds SQRT; the division and the product one rounding each.  Rows whose norm lies within that error of eps may take
    either branch of the max: the bound covers both."""
    x = x.double()
    D = x.shape[-1]
    dsum = depth(D) if lanes == 64 else 8 + int(math.log2(lanes))
    ss = (x * x).sum(-1, keepdim=True)
    nrm = torch.sqrt(ss)
    den = nrm.clamp(min=eps)
    y = x / den
    rel = 0.5 * (dsum + 1) * U + SQRT + SQRT + U
    dy = y.abs() * rel * (1 + 1e-3)
    near = (nrm - eps).abs() <= nrm * rel
    dy = torch.where(near, dy + y.abs() * rel, dy)
    return y, dy + out_bound(y.abs() + dy, out_kind)


def l2norm_emulate(x, eps, lanes=64, mut=None):
    """f32 emulation; x f32 [rows, D] (the values read).  lanes 64: general kernel; 8 / 16: short kernels (8 elements per lane)."""
    x = x.float()
    rows, D = x.shape
    if lanes == 64:
        ss = lane_sum(x * x)
    else:
        pad = lanes * 8 - D
        sq = torch.nn.functional.pad(x * x, (0, pad)).view(rows, lanes, 8)
        part = sq[..., 0]
        for e in range(1, 8):
            part = part + sq[..., e]
        if mut == "wrong_lane_group" and lanes == 8:                    # a 16-lane sum where 8 lanes own a row: pairs of rows share a sum
            if rows % 2:
                part = torch.cat([part, part[-1:]], 0)
            ss = group_sum(part.view(-1, 16), 16).repeat_interleave(2)[:rows]
        else:
            ss = group_sum(part, lanes)
    e = torch.tensor(eps, dtype=torch.float32)
    nrm = torch.sqrt(ss)
    inv = 1.0 / (nrm + e) if mut == "norm_plus_eps" else 1.0 / torch.maximum(nrm, e)
    return x * inv[:, None]


def make_l2_case(rows, D, seed, kind="f32", special=True):
    """Every row a different norm (geometric, 2^-4 .. 2^4); with `special`, row 0 zero and row 1 of norm 1e-15 (f32 input only; rows >= 3)."""
    g = torch.Generator().manual_seed(3000 + seed)
    v = torch.randn(rows, D, generator=g)
    v = v * torch.exp2(torch.linspace(-4, 4, rows))[:, None] if rows > 1 else v
    if special and rows >= 3:
        v[0] = 0.0
        if kind == "f32":
            v[1] = v[1] / v[1].norm() * 1e-15
    s = store(v, kind)
    return s, load(s, kind)


# ---- materialised softmax -----------------------------------------------------------------------------------------------------------------
def softmax_args(scores, B, H, N, sc, bias, bias_w, bias_bstride, rn, cn):
    """(a, da): the first-stage additive bias term w bias[b, i-1, j-1] (x rn[b,h,i]) (x cn[b,h,j]) as [B,H,N,N] f64 (zero at i == 0 or
    j == 0) and the bound on its f32 evaluation (three roundings)."""
    t = torch.zeros(B, H, N, N, dtype=torch.float64)
    if bias is None:
        return t, t.clone()
    n = N - 1
    for b in range(B):
        bb = bias.double().reshape(-1)[b * bias_bstride: b * bias_bstride + n * n].view(n, n)
        t[b, :, 1:, 1:] = bb
    w = torch.full((B, H, N, 1), float(bias_w), dtype=torch.float64)
    if rn is not None:
        w = w * rn.double().view(B, H, N, 1)
    t = t * w
    if cn is not None:
        t = t * cn.double().view(B, H, 1, N)
    return t, 3 * U * t.abs()


def _softmax_stage(a, da, N):
    """softmax over the last axis of a (+-da), -inf = masked: (p, dp) with the kernel's error model: a - mx one rounding, expf EXPF, the sum
    (depth(N) + the weighted relative error of its terms), the reciprocal and the product one rounding each."""
    mx = a.max(-1, keepdim=True)[0]
    arg = a - mx
    e = torch.exp(arg)
    s = e.sum(-1, keepdim=True)
    p = e / s
    live = torch.isfinite(a)
    rel_e = torch.where(live, EXPF + da + U * arg.abs().nan_to_num(posinf=0.0, neginf=0.0), torch.zeros_like(a))
    rel_s = (e * rel_e).sum(-1, keepdim=True) / s + depth(N) * U
    return p, s, mx, p * (rel_e + rel_s + 3 * U) * (1 + 1e-3), rel_s


def softmax_reference(scores, B, H, N, *, scale=1.0, scale_per_image=None, bias=None, bias_w=0.0, bias_bstride=0, rn=None, cn=None,
                      mode=0, causal=False, prefill=None):
    """f64 reference of softmax_rows: dict(out, bound, lse, lse_bound).  scores [B*H*N, N] raw dot products (f32)."""
    s = scores.double().view(B, H, N, N)
    sc = torch.full((B, 1, 1, 1), float(scale), dtype=torch.float64) if scale_per_image is None else scale_per_image.double().view(B, 1, 1, 1)
    t, dt = softmax_args(scores, B, H, N, sc, bias, bias_w, bias_bstride, rn, cn)
    a1 = s * sc
    da1 = U * a1.abs()
    mask = torch.ones(N, N).tril().bool() if causal else torch.ones(N, N).bool()
    ninf = torch.tensor(float("-inf"), dtype=torch.float64)
    if mode == 0:
        a = a1 + t
        da = da1 + dt + U * a.abs()
        p, ssum, mx, dp, rel_s = _softmax_stage(torch.where(mask, a, ninf), da, N)
    else:
        p1, ssum, mx, dp1, rel_s = _softmax_stage(torch.where(mask, a1, ninf), da1, N)
        a2 = p1 + t
        da2 = dp1 + dt + U * a2.abs()
        p, _, _, dp, _ = _softmax_stage(torch.where(mask, a2, ninf), da2, N)
    lse = (mx + torch.log(ssum))[..., 0]
    da_row = torch.where(mask, da if mode == 0 else da1, torch.zeros_like(a1)).max(-1)[0]
    lse_bound = da_row + rel_s[..., 0] * (1 + 1e-3) + LOGF * torch.log(ssum)[..., 0].abs() + 2 * U + U * (mx[..., 0].abs() + lse.abs())
    p = torch.where(mask, p, torch.zeros_like(p))
    dp = torch.where(mask, dp, torch.zeros_like(dp))
    out = p
    if prefill is not None:
        out = prefill.double().view(B, H, N, N) + p
        dp = dp + U * out.abs()
    bound = dp + torch.where(mask, half_ulp(out.abs() + dp, "f32"), torch.zeros_like(dp))
    return dict(out=out.reshape(B * H * N, N), bound=bound.reshape(B * H * N, N), lse=lse.reshape(-1), lse_bound=lse_bound.reshape(-1),
                exact_zero=(~mask)[None, None].expand(B, H, N, N).reshape(B * H * N, N))


def softmax_emulate(scores, B, H, N, *, scale=1.0, scale_per_image=None, bias=None, bias_w=0.0, bias_bstride=0, rn=None, cn=None,
                    mode=0, causal=False, prefill=None, mut=None):
    """softmax_rows_kernel in f32, row by row with the lane-strided sums; `mut` names one of the listed slips.  Returns (out, lse)."""
    f = torch.float32
    s = scores.float().view(B, H, N, N)
    out = torch.zeros(B, H, N, N, dtype=f) if prefill is None else prefill.float().view(B, H, N, N).clone()
    lse = torch.zeros(B, H, N, dtype=f)
    n = N - 1
    for b in range(B):
        for h in range(H):
            sidx = (b * H + h) if mut == "scale_bh" else b
            sc = torch.tensor(float(scale), dtype=f) if scale_per_image is None else scale_per_image.float()[sidx % scale_per_image.numel()]
            bb = None
            if bias is not None:
                bb = bias.float().reshape(-1)[b * bias_bstride: b * bias_bstride + n * n].view(n, n)
                if mut == "bias_transposed":
                    bb = bb.t()
            for i in range(N):
                Nk = (i if mut == "causal_nk_i" else i + 1) if causal else N
                Nk = max(Nk, 1)
                w = torch.tensor(float(bias_w), dtype=f)
                if rn is not None:
                    w = w * rn.float().view(B, H, N)[b, h, i]
                add = torch.zeros(Nk, dtype=f)
                if bb is not None and i > 0:
                    if mut == "bias_at_cls":
                        row = torch.cat([bb[i - 1], bb[i - 1, -1:]])[:Nk]
                        add = w * row * (cn.float().view(B, H, N)[b, h, :Nk] if cn is not None else 1.0)
                    else:
                        add[1:] = w * bb[i - 1, :Nk - 1] * (cn.float().view(B, H, N)[b, h, 1:Nk] if cn is not None else 1.0)
                v = s[b, h, i, :Nk] * sc
                first = v + add if (mode == 0 or mut == "bias_before_first") else v
                mx = first.max()
                e = torch.exp(first - mx)
                sm = lane_sum(e)
                lse[b, h, i] = mx + torch.log(sm)
                p = e * (1.0 / sm)
                if mode == 1:
                    p2 = p if mut == "bias_before_first" else p + add
                    mx2 = p2.max()
                    e2 = torch.exp(p2 - mx2)
                    p = e2 * (1.0 / lane_sum(e2))
                if prefill is not None and mut != "accumulate_overwrites":
                    out[b, h, i, :Nk] = out[b, h, i, :Nk] + p
                else:
                    out[b, h, i, :Nk] = p
                    if prefill is None:
                        out[b, h, i, Nk:] = 0.0
    return out.view(B * H * N, N), lse.view(-1)


SOFTMAX_N = (2, 64, 65, 130)
SOFTMAX_VARIANTS = ("plain", "bias_shared", "bias_per_image", "factors", "scale_per_image", "accumulate", "causal", "mode1_bias",
                    "mode1_causal")


def make_softmax_case(N, variant, seed, B=2, H=3):
    """kwargs of softmax_reference / softmax_emulate + scores for one variant: scores reach +-80, the bias is asymmetric."""
    g = torch.Generator().manual_seed(4000 + seed)
    scores = 20.0 * torch.randn(B * H * N, N, generator=g)
    scores[:, 0] = 80.0 * torch.sign(torch.randn(B * H * N, generator=g))
    scores[:, N - 1] = -80.0 if N > 2 else scores[:, N - 1]
    scores = scores.clamp(-80, 80)
    n = N - 1
    kw = dict(scale=0.125, mode=0)
    bias = torch.rand(B, n, n, generator=g) * 2.0 - 0.5                   # asymmetric on purpose
    if variant == "bias_shared":
        kw.update(bias=bias[0].contiguous(), bias_w=3.0, bias_bstride=0)
    elif variant == "bias_per_image":
        kw.update(bias=bias, bias_w=3.0, bias_bstride=n * n)
    elif variant == "factors":
        kw.update(bias=bias, bias_w=1.5, bias_bstride=n * n, rn=0.5 + torch.rand(B, H, N, generator=g), cn=0.5 + torch.rand(B, H, N, generator=g))
    elif variant == "scale_per_image":
        kw.update(scale_per_image=torch.tensor([0.05, 0.3])[:B])
    elif variant == "accumulate":
        kw.update(prefill=torch.rand(B * H * N, N, generator=g))
    elif variant == "causal":
        kw.update(causal=True)
    elif variant == "mode1_bias":
        kw.update(mode=1, bias=bias, bias_w=3.0, bias_bstride=n * n)
    elif variant == "mode1_causal":
        kw.update(mode=1, causal=True, bias=bias, bias_w=3.0, bias_bstride=n * n)
    return scores, kw


# ---- pack_rows / transpose_pack ---------------------------------------------------------------------------------------------------------------
def pack_rows_reference(src, cols, cols_pad, kind):
    """src [rows, ld] f32 -> the exact f64 content of dst [rows, cols_pad]: one rounding, zero padding."""
    out = torch.zeros(src.shape[0], cols_pad, dtype=torch.float64)
    out[:, :cols] = rounded_once(src[:, :cols], kind) if kind != "h2" else rounded_once(
        torch.nn.functional.pad(src[:, :cols], (0, cols_pad - cols)), kind)[:, :cols]
    return out


def transpose_pack_reference(src, kind):
    return rounded_once(src.t().contiguous(), kind)


# ---- embed_assemble ----------------------------------------------------------------------------------------------------------------------------
def embed_assemble_reference(patches, cls_emb, pos, gamma, beta, eps, B, N):
    """(x, bound) [B, N, D]: LayerNorm of the f32-rounded sum (t == 0 ? cls : patch) + pos[t] -- the kernel adds in f32 (one rounding,
    reproduced exactly here) before the row statistics."""
    D = pos.shape[-1]
    tok = torch.cat([cls_emb.float().view(1, 1, D).expand(B, 1, D), patches.float().view(B, N - 1, D)], 1) + pos.float()[None, :N]
    y, bound, _ = layernorm_reference(tok.view(B * N, D), gamma, beta, eps)
    return y.view(B, N, D), bound.view(B, N, D)


# ---- positional-embedding resize -------------------------------------------------------------------------------------------------------------
def _cubic(x, A):
    """Keys' cubic convolution kernel with parameter A at distance |x|."""
    x = x.abs()
    near = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    far = ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return torch.where(x < 1.0, near, torch.where(x < 2.0, far, torch.zeros_like(x)))


def resize_scale(g0, g, mode, f32=True, mut=None):
    """The source step per output cell: mode 0 1 / ((g + 0.1) / g0) evaluated in double (Python's scale_factor), mode 1 g0 / g; `f32`
    rounds it to the f32 the kernel (and ATen, for f32 tensors) carries."""
    s = (g0 / g) if (mode == 1 or mut == "scale_g0_over_g") else 1.0 / ((g + 0.1) / g0)
    if mut == "align_corners":
        s = (g0 - 1) / max(g - 1, 1)
    return float(np.float32(s)) if f32 else s


def resize_weights(g0, g, mode, f32=True, mut=None):
    """(W, dW) [g, g0] f64: the separable interpolation matrix along one axis and the bound on its f32 evaluation.
    mode 0: bicubic A = -0.75, src = scale (dst + 0.5) - 0.5 NOT clamped, the four taps floor(src) - 1 .. + 2 clamped into the grid (their
    weights add up where they coincide).  mode 1: A = -0.5, support 2 max(scale, 1), every in-range sample of the stretched kernel,
    renormalised to sum 1.  The f32 source coordinate misses by 2 u (|scale (dst + 0.5)| + 1); both kernels' slopes are below 1.5, their
    Horner evaluation (intermediates up to 12) adds 64 u; mode 1's normalisation propagates the relative error of its total."""
    scale = resize_scale(g0, g, mode, f32, mut)
    dst = torch.arange(g, dtype=torch.float64)
    W = torch.zeros(g, g0, dtype=torch.float64)
    dW = torch.zeros(g, g0, dtype=torch.float64)
    if mode == 0:
        A = -0.5 if mut == "A_minus_half" else -0.75
        src = scale * dst if mut == "align_corners" else scale * (dst + 0.5) - 0.5
        if mut == "clamp_src":
            src = src.clamp(min=0.0)
        dsrc = 2 * U * ((scale * (dst + 0.5)).abs() + 1.0)
        fl = torch.floor(src)
        t = src - fl
        for k in range(4):
            j = (fl.long() - 1 + k).clamp(0, g0 - 1)
            w = _cubic(t + 1.0 - k, A)
            W.scatter_add_(1, j[:, None], w[:, None])
            dW.scatter_add_(1, j[:, None], (1.5 * dsrc + 64 * U)[:, None])
        return W, dW
    A = -0.5
    support = 2.0 * max(scale, 1.0)
    inv = 1.0 / max(scale, 1.0)
    center = scale * (dst + 0.5)
    j = torch.arange(g0, dtype=torch.float64)
    arg = (j[None, :] - center[:, None] + 0.5) * inv
    raw = _cubic(arg, A)
    inside = arg.abs() < 2.0
    draw = torch.where(inside | ((arg.abs() - 2.0).abs() < 1e-5), 1.5 * inv * 2 * U * (center[:, None].abs() + j[None, :] + 1.0) + 64 * U, torch.zeros_like(raw))
    if mut == "no_renorm":
        return raw * inv, draw
    tot = raw.sum(1, keepdim=True)
    n = inside.sum(1, keepdim=True).double()
    W = raw / tot
    dW = (draw + W.abs() * (draw.sum(1, keepdim=True) + n * U * raw.abs().sum(1, keepdim=True))) / tot.abs() + U * W.abs()
    return W, dW


def posembed_resize_reference(pos, g0, gh, gw, mode, f32=True, mut=None):
    """(out, bound) [1 + gh gw, D] f64: row 0 = pos[0] (bound 0), the grid rows = Wy (x) Wx applied to pos[1:] viewed [g0, g0, D]."""
    D = pos.shape[-1]
    grid = pos[1:].double().view(g0, g0, D)
    Wy, dWy = resize_weights(g0, gh, mode, f32, mut)
    Wx, dWx = resize_weights(g0, gw, mode, f32, mut)
    out = torch.einsum("ya,xb,abd->yxd", Wy, Wx, grid)
    ag = grid.abs()
    S = torch.einsum("ya,xb,abd->yxd", Wy.abs(), Wx.abs(), ag)
    err = (torch.einsum("ya,xb,abd->yxd", dWy, Wx.abs(), ag) + torch.einsum("ya,xb,abd->yxd", Wy.abs() + dWy, dWx, ag))
    taps = float(((Wy != 0).sum(1).max() + (Wx != 0).sum(1).max() + 2))
    b = err + taps * U * S
    b = b + half_ulp(out.abs() + b, "f32")
    full = torch.cat([pos[:1].double(), out.reshape(gh * gw, D)], 0)
    return full, torch.cat([torch.zeros(1, D, dtype=torch.float64), b.reshape(gh * gw, D)], 0)


def posembed_resize_emulate(pos, g0, gh, gw, mode, mut=None):
    """The kernel's arithmetic in f32: weights from the f32 scale, evaluated in f32, rows then columns accumulated tap by tap."""
    D = pos.shape[-1]
    if mut == "swap_hw":                                                 # the (gw, gh) result laid out as if it were (gh, gw)
        return posembed_resize_emulate(pos, g0, gw, gh, mode)
    Wy, Wx = resize_weights(g0, gh, mode, True, mut)[0].float(), resize_weights(g0, gw, mode, True, mut)[0].float()
    grid = pos[1:].float().view(g0, g0, D)
    acc = torch.zeros(gh, gw, D)
    for a in range(g0):
        row = torch.zeros(gw, D)
        for b in range(g0):
            row = row + Wx[:, b, None] * grid[a, b][None]
        acc = acc + Wy[:, a, None, None] * row[None]
    return torch.cat([pos[:1].float(), acc.view(gh * gw, D)], 0)


RESIZE_CASES = ((7, 9, 5), (7, 7, 9), (7, 3, 4), (7, 14, 14), (16, 3, 37))
RESIZE_D = (8, 33)


def make_pos(g0, D, seed):
    g = torch.Generator().manual_seed(5000 + seed)
    return (torch.randn(1 + g0 * g0, D, generator=g) * 0.5 + 0.25).float()


# ---- LayerNorm folded into the GEMMs --------------------------------------------------------------------------------------------------------
def ln_stats_reference(st, eps, mut=None):
    """st [S, rows, 2] f32 slices (sum, centred sum of squares) of 64 elements each -> (mean, rstd, dmean, drstd) by Chan's combination:
    m2 = sum_i css_i + 64 (sum_i / 64 - mean)^2.  The kernel adds serially over the S slices (S roundings of a partial sum)."""
    st = st.double()
    S = st.shape[0]
    sm, css = st[..., 0], st[..., 1]
    mean = sm.sum(0) / (64 * S)
    d = sm / 64.0 - mean
    terms = css + (0.0 if mut == "no_between" else 64.0 * d * d)
    m2 = terms.sum(0)
    var = m2 / (64 * S)
    rstd = 1.0 / torch.sqrt(var + eps)
    dmean = (S * U * sm.abs().sum(0)) / (64 * S) + U * mean.abs()
    dd = dmean + U * d.abs()
    dterm = 64.0 * (2 * d.abs() * dd + dd * dd) + 3 * U * 64.0 * d * d + U * terms.abs()
    dvar = (dterm.sum(0) + (S + 1) * U * terms.abs().sum(0)) / (64 * S)
    rel = dvar / (2 * (var + eps)) + 0.5 * U + 2 * SQRT
    return mean, rstd, dmean + half_ulp(mean.abs() + dmean, "f32"), rstd * rel * (1 + 1e-3) + half_ulp(rstd, "f32")


def ln_stats_emulate(st, eps, mut=None):
    st = st.float()
    S = st.shape[0]
    tot = torch.zeros(st.shape[1])
    for i in range(S):
        tot = tot + st[i, :, 0]
    mean = tot / float(S * 64)
    m2 = torch.zeros_like(mean)
    for i in range(S):
        d = st[i, :, 0] * (1.0 / 64.0) - mean
        m2 = m2 + (st[i, :, 1] if mut == "no_between" else st[i, :, 1] + 64.0 * d * d)
    return mean, 1.0 / torch.sqrt(m2 / float(S * 64) + torch.tensor(eps, dtype=torch.float32))


def make_ln_stats_case(S, rows, seed):
    """Slice statistics [S, rows, 2] f32 of rows whose 64-wide slices have means 1e3 apart."""
    g = torch.Generator().manual_seed(6000 + seed)
    x = torch.randn(rows, S, 64, generator=g, dtype=torch.float64) + 1e3 * torch.arange(S, dtype=torch.float64)[None, :, None]
    sm = x.sum(-1)
    css = ((x - x.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([sm, css], -1).permute(1, 0, 2).contiguous().float()


def fold_ln_weight_reference(W, gamma, beta, bias, kind, Wp_written=None, mut=None):
    """dict(Wp exact storage, Wp_alt, c, c_bound, bias_f, bias_bound).  Wp = store(f32(W gamma)) exactly; c is held to the sum of the Wp the
    kernel WROTE (Wp_written, storage) when given; both sums are 64-lane strided over K.  Two-plane: hi = f16(f32(W gamma)) either way, but
    lo = f16(p - hi) may take p = f32(W gamma) (Wp) or, where the compiler contracts the product into the subtraction (one fma: the
    language allows it), the exact product (Wp_alt) -- both are W' rounded once to the two planes."""
    K = W.shape[1]
    prod = W.float() * gamma.float()[None]
    Wp = store(prod, kind)
    Wp_alt = Wp
    if kind == "h2":
        hi = prod.half()
        lo = (W.double() * gamma.double()[None] - hi.double()).float().half()
        Wp_alt = torch.stack([hi.view(-1, K // 8, 8), lo.view(-1, K // 8, 8)], dim=-2).reshape(-1, 2 * K)
    vals = load(Wp_written if Wp_written is not None else Wp, kind)
    if mut == "c_unrounded":
        vals = prod.double()
    c = vals.sum(1)
    cb = (depth(K) + (1 if kind == "h2" else 0)) * U * vals.abs().sum(1)
    cb = cb + half_ulp(c.abs() + cb, "f32")
    t = beta.double()[None] * W.double()
    bf = t.sum(1) + (bias.double() if bias is not None else 0.0)
    bb = (depth(K) + 1) * U * t.abs().sum(1) + U * bf.abs()
    bb = bb + half_ulp(bf.abs() + bb, "f32")
    return dict(Wp=Wp, Wp_alt=Wp_alt, c=c, c_bound=cb, bias_f=bf, bias_bound=bb)


def fold_ln_weight_emulate(W, gamma, beta, bias, kind, mut=None):
    prod = W.float() * gamma.float()[None]
    Wp = store(prod, kind)
    vals = prod if mut == "c_unrounded" else load(Wp, kind).float()
    c = lane_sum(vals)
    bf = lane_sum(beta.float()[None] * W.float()) + (bias.float() if bias is not None else 0.0)
    return Wp, c, bf


def make_fold_case(N, K, seed, with_bias=True):
    g = torch.Generator().manual_seed(7000 + seed)
    W = (torch.randn(N, K, generator=g) * 0.05).float()
    gamma = (1.0 + 0.3 * torch.randn(K, generator=g)).float()
    beta = (0.2 * torch.randn(K, generator=g)).float()
    bias = torch.randn(N, generator=g).float() if with_bias else None
    return W, gamma, beta, bias


# ---- small ops -----------------------------------------------------------------------------------------------------------------------------------
def gaussian_bias_reference(gh, gw, std):
    """(omega, bound) [gh gw, gh gw]: exp(-(dy^2 + dx^2) / (2 std^2)); the host's f32 1 / (2 std^2) misses by 3 u, the product by u, expf by
    EXPF, so the relative error is EXPF + 5 u |argument|."""
    std = float(np.float32(std))
    cell = torch.arange(gh * gw)
    y, x = (cell // gw).double(), (cell % gw).double()
    arg = ((y[:, None] - y[None]) ** 2 + (x[:, None] - x[None]) ** 2) / (2.0 * std * std)
    om = torch.exp(-arg)
    b = om * (EXPF + 5 * U * arg)
    return om, b + half_ulp(om + b, "f32")


def norm_reference(x, terms):
    """(||x|| over the last axis, bound): sum of squares (depth(terms) + 1) u relative, halved by the root, + SQRT, + the f32 store."""
    x = x.double()
    nrm = torch.sqrt((x * x).sum(-1))
    b = nrm * (0.5 * (depth(terms) + 1) * U + SQRT) * (1 + 1e-3)
    return nrm, b, b + half_ulp(nrm + b, "f32")


def head_norms_reference(x, B, N, H, dh):
    """x [B, N, H, dh] (values read) -> out [B, H, N], bound."""
    nrm, _, b = norm_reference(x.view(B, N, H, dh), dh)
    return nrm.permute(0, 2, 1).contiguous(), b.permute(0, 2, 1).contiguous()


def axpby_reference(y, x, a, b):
    a, b = float(np.float32(a)), float(np.float32(b))
    ax, by = a * x.double(), b * y.double()
    r = ax + by
    bound = U * (ax.abs() + by.abs())
    return r, bound + half_ulp(r.abs() + bound, "f32")


def gem_inv_temp_reference(x, scale):
    """x [B, N, D] -> out [B] = scale mean_t ||x[b, t]||: wave w adds the norms of tokens w, w + 4, ... (ceil(N / 4) terms), three more
    additions, the division and the product."""
    B, N, D = x.shape
    nrm, b, _ = norm_reference(x, D)
    scale = float(np.float32(scale))
    out = nrm.mean(1) * scale
    bound = (b.sum(1) / N * abs(scale)) + (-(-N // 4) + 3 + 2) * U * nrm.sum(1) / N * abs(scale)
    return out, bound + half_ulp(out.abs() + bound, "f32")


# ---- patchify ----------------------------------------------------------------------------------------------------------------------------------
PATCH_MEAN = (122.771, 116.746, 104.094)          # SegDataPreProcessor mean / std as quoted in csrc/patchify.hip (held in f32 there)
PATCH_STD = (68.501, 66.632, 70.323)


def patchify_reference(scene, windows, scene_index, tile_h, tile_w, pad_l, pad_t, gh, gw, P, Kpad, mut=None):
    """The exact f64 patch matrix [T gh gw, Kpad] and a mask of the cells that carry pixels.  scene: uint8 [B, H, W, 3] (normalised with the
    f32 constants: (u - mean) / std) or f32 [B, 3, H, W]; windows [T, 4] = y1, y2, x1, x2; column k = c P P + py P + px; the window sits
    pad_t rows down and pad_l columns right of the patch grid's origin; everything else is zero."""
    u8 = scene.dtype == torch.uint8
    if mut == "layout_swapped":                                          # the same memory read in the other layout
        if u8:
            Bn, Hs, Ws, _ = scene.shape
            scene = scene.contiguous().view(Bn, 3, Hs, Ws).permute(0, 2, 3, 1)
        else:
            Bn, _, Hs, Ws = scene.shape
            scene = scene.contiguous().view(Bn, Hs, Ws, 3).permute(0, 3, 1, 2)
    if u8:
        mean = torch.tensor(np.array(PATCH_MEAN, dtype=np.float32).astype(np.float64))
        std = torch.tensor(np.array(PATCH_STD, dtype=np.float32).astype(np.float64))
        img = ((scene.double() - mean) / std).permute(0, 3, 1, 2)
    else:
        img = scene.double()
    if mut == "pad_swapped":
        pad_l, pad_t = pad_t, pad_l
    T = windows.shape[0]
    canvas = torch.zeros(T, 3, gh * P, gw * P, dtype=torch.float64)
    live = torch.zeros(T, 3, gh * P, gw * P, dtype=torch.bool)
    for t in range(T):
        y1, x1 = int(windows[t, 0]), int(windows[t, 2])
        b = int(scene_index[t]) if scene_index is not None else 0
        h, w = min(tile_h, gh * P - pad_t), min(tile_w, gw * P - pad_l)
        canvas[t, :, pad_t:pad_t + h, pad_l:pad_l + w] = img[b, :, y1:y1 + h, x1:x1 + w]
        live[t, :, pad_t:pad_t + h, pad_l:pad_l + w] = True

    def cols(c):
        c = c.view(T, 3, gh, P, gw, P)
        c = c.permute(0, 2, 4, 1, 5, 3) if mut == "pxpy_swapped" else c.permute(0, 2, 4, 1, 3, 5)
        return c.reshape(T * gh * gw, 3 * P * P)
    out = torch.zeros(T * gh * gw, Kpad, dtype=torch.float64)
    mask = torch.zeros(T * gh * gw, Kpad, dtype=torch.bool)
    out[:, :3 * P * P] = cols(canvas)
    mask[:, :3 * P * P] = cols(live)
    return out, mask


def patchify_interval(exact, u8, kind):
    """(lo, hi) admissible stored values: from f32 the value rounded once; from u8 the rounding of exact -+ 1 ulp of f32 (the subtraction
    and the division one rounding each)."""
    if not u8:
        r = rounded_once(exact, kind)
        return r, r
    ulp = 2 * half_ulp(exact.abs(), "f32")
    if kind == "f32":                                                    # no output rounding: the f32 value itself
        return exact - ulp, exact + ulp
    if kind == "h2":                                                     # an f32 value within 1 ulp, held as hi + lo
        return exact - ulp - h2_delta(exact.abs() + ulp), exact + ulp + h2_delta(exact.abs() + ulp)
    return rounded_once(exact - ulp, kind), rounded_once(exact + ulp, kind)


def gather_rows(flat, so, si, inner, rows, D):
    """Rows of D contiguous elements at (r // inner) so + (r % inner) si of a flat tensor -> [rows, D] (l2norm_rows' addressing)."""
    r = torch.arange(rows)
    start = (r // inner) * so + (r % inner) * si
    return flat[start[:, None] + torch.arange(D)[None]]


def make_patch_case(P, gh, gw, u8, seed, B=2, T=2, pad_t=3, pad_l=5):
    """A 2-image scene and 2 tiles (the second from image 1 through scene_index) whose window is smaller than the patch grid minus the
    padding; u8 scenes hold every value 0 .. 255 in every channel."""
    g = torch.Generator().manual_seed(8000 + seed)
    tile_h, tile_w = gh * P - pad_t - 1, gw * P - pad_l - 2
    Hs, Ws = tile_h + 7, tile_w + 9
    if u8:
        scene = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8)
        ramp = torch.arange(256, dtype=torch.uint8)
        scene[0, 2, 4:4 + min(256, Ws - 4)] = ramp[:min(256, Ws - 4), None]
        scene[1, 3, 1:1 + min(256, Ws - 1)] = ramp.flip(0)[:min(256, Ws - 1), None]
    else:
        scene = torch.randn(B, 3, Hs, Ws, generator=g).float()
    windows = torch.tensor([[2, 2 + tile_h, 4, 4 + tile_w], [3, 3 + tile_h, 1, 1 + tile_w]], dtype=torch.int32)
    return dict(scene=scene, windows=windows, scene_index=torch.tensor([0, 1], dtype=torch.int32), tile_h=tile_h, tile_w=tile_w,
                pad_l=pad_l, pad_t=pad_t, gh=gh, gw=gw, P=P, scene_h=Hs, scene_w=Ws)


def std_kpad(P):
    return (3 * P * P + 63) // 64 * 64


PATCH_SHAPES = ((14, None), (16, None), (32, None), (4, 64), (14, "std+64"))     # (P, Kpad): None = the standard padding
