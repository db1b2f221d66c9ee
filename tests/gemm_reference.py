"""f64 references and per-element error bounds for the HIP GEMMs (used by tests/test_gpu_gemm_reference.py and tests/test_gemm_bound_cpu.py).

Everything here is plain torch in float64 and runs on whatever device its inputs live on.  The bound of an output element is built from
the magnitudes of the operands the kernel actually consumed -- never from the observed outputs -- term by term as documented in
`gemm_bound`.  Operand conventions: A [.., M, K], W [.., N, K] (K-contiguous, the library's layout), C = act(A.W^T + bias) (+ residual).
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24                                     # unit roundoff of f32 (round to nearest)
H2_REL, H2_ABS = 2.0 ** -22, 2.0 ** -25            # two-plane representation error max(2^-22 |x|, 2^-25) (common.h)
# output formats: significand bits p (with the implicit one) and the smallest binary exponent e (|x| = m 2^e, m in [0.5, 1)) whose
# spacing 2^(e - p) is still that of the normal numbers -- below it the subnormal spacing holds
FORMATS = {"f32": (24, -125), "bf16": (8, -125), "f16": (11, -13)}
# Lipschitz constants of the exact activations on the real line: GELU' peaks at 1.1289 (x = sqrt 2), QuickGELU' = x sigmoid(1.702 x)'
# peaks at 1.0998 (both checked on a fine grid by tests/test_gemm_bound_cpu.py)
LIPSCHITZ = {0: 1.0, 1: 1.13, 2: 1.13}


def act_f64(x: torch.Tensor, act: int) -> torch.Tensor:
    """The exact activations: 0 none, 1 QuickGELU x sigmoid(1.702 x), 2 erf-GELU 0.5 x (1 + erf(x / sqrt 2))."""
    if act == 0:
        return x
    if act == 1:
        return x * torch.sigmoid(1.702 * x)
    if act == 2:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    raise ValueError(act)


def half_ulp(mag: torch.Tensor, fmt: str) -> torch.Tensor:
    """Half the spacing of `fmt` at magnitude `mag` (>= 0), subnormal floor included: the largest error of a round-to-nearest store."""
    p, emin = FORMATS[fmt]
    _, e = torch.frexp(mag)
    e = torch.where(mag > 0, torch.clamp(e, min=emin), torch.full_like(e, emin))
    return torch.ldexp(torch.ones_like(mag), e - p - 1)


def h2_delta(x: torch.Tensor) -> torch.Tensor:
    """Representation error of a two-plane element x = hi + lo: max(2^-22 |x|, 2^-25) (lo is an f16 with spacing 2^-24 at the bottom)."""
    return torch.clamp(x.abs() * H2_REL, min=H2_ABS)


def act_approx_bound(xm: torch.Tensor, ym: torch.Tensor, act: int, fast: bool) -> torch.Tensor:
    """Bound on |device activation(x) - exact activation(x)| for an f32 argument, given |x| <= xm and |act(x)| <= ym (common.h):

    * QuickGELU, `quick_gelu` (2-byte / fp8 epilogues) and `quick_gelu_split` (two-plane): the exponent argument carries the rounding of
      the f32 constant and of its product with x (relative 2^-23 of |t| = 2.456 |x|, 1.5x that in the split form's -1.702f x then
      log2(e) steps), the hardware exp2 and rcp 1 ulp each (2^-23), 1 + e and x * r one rounding each; the relative error of
      e propagates into 1 / (1 + e) damped by e / (1 + e) <= 1.  Together |y| (4 |x| + 3) 2^-23.
    * GELU, `erf_gelu_fast` (2-byte / fp8): Abramowitz-Stegun 7.1.26, |erf error| <= 1.5e-7; its f32 evaluation (t on the hardware rcp,
      a degree-5 Horner polynomial with sum |a_i| < 4.5, the hardware exp2 of -log2(e) z^2) adds < 112 2^-24 absolute to erf; halved by
      0.5 |x|, plus the last two roundings: < 4e-6 |x|.
    * GELU, `erf_gelu` (two-plane: erff, 2 ulp; argument and the three products one rounding each): < 2^-20 |x|.
    """
    if act == 0:
        return torch.zeros_like(xm)
    if act == 1:
        return ym * (4.0 * xm + 3.0) * 2.0 ** -23
    if act == 2:
        return xm * (4e-6 if fast else 2.0 ** -20)
    raise ValueError(act)


def matmul_f64(A: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """A [.., M, K] . W [.., N, K]^T in float64."""
    return torch.matmul(A.double(), W.double().transpose(-1, -2))


def gemm_reference(A: torch.Tensor, W: torch.Tensor, bias=None, residual=None, act: int = 0):
    """(pre-activation, output) in float64 from the operands the kernel consumed (already rounded to its storage)."""
    pre = matmul_f64(A, W)
    if bias is not None:
        pre = pre + bias.double()
    out = act_f64(pre, act)
    if residual is not None:
        out = out + residual.double()
    return pre, out


def gemm_bound(A: torch.Tensor, W: torch.Tensor, bias, pre: torch.Tensor, out: torch.Tensor, *, act: int, out_fmt: str,
               two_plane: bool = False, fast_act: bool = True) -> torch.Tensor:
    """Per-element bound on |kernel output - f64 reference| for a GEMM with f32 accumulation.

    A, W: the values the reference used (the rounded 2-byte operands, the de-quantised e4m3 bytes times their scales, or -- two_plane --
    the original f32 values); pre / out: `gemm_reference`'s results.  With S = |A| . |W|^T in f64 the terms are:

    * accumulation: every product of two bf16 / f16 / e4m3 values is exact in f32, every addition of the K-long sum (whatever its order
      or the matrix unit's internal grouping) is a faithful f32 rounding, i.e. at most 2u of a partial sum bounded by S: 2u K S.  Three
      more roundings (the scale products of the fp8 path, the bias add) add 2u 3 (S + |bias|).  Two-plane operands issue 3K products
      (hi.hi + hi.lo + lo.hi) whose magnitudes sum to at most 1.01 S (|hi| <= |x| (1 + 2^-11), |lo| <= 2^-11 |x|).
    * two-plane representation: hi + lo misses x by delta(x) = max(2^-22 |x|, 2^-25), so the exact product of the planes misses that of
      the originals by sum_k delta(a)|w| + |a| delta(w) (= delta(A).|W|^T + |A|.delta(W)^T), and the omitted lo.lo term by 2^-22 S.
    * activation: the pre-activation bound times the exact activation's Lipschitz constant (<= 1.13), plus the device approximation's
      own error (`act_approx_bound`, evaluated at the largest |x| the kernel can have seen).
    * output: half an ulp of the output format at the largest magnitude the stored value can have, per element (f32 -- which also covers
      the residual add --, bf16, or f16 with its subnormal floor); for a two-plane C the store's own representation error
      max(2^-22 |r|, 2^-25).
    """
    A64, W64 = A.double(), W.double()
    S = matmul_f64(A64.abs(), W64.abs())
    K = A.shape[-1]
    b = bias.double().abs() if bias is not None else torch.zeros((), dtype=torch.float64, device=S.device)
    if two_plane:
        rep = matmul_f64(h2_delta(A64), W64.abs()) + matmul_f64(A64.abs(), h2_delta(W64)) + H2_REL * S
        bpre = 2 * U * (3 * K) * (1.01 * S + rep) + 2 * U * 3 * (1.01 * S + rep + b) + rep
    else:
        bpre = 2 * U * K * S + 2 * U * 3 * (S + b)
    L = LIPSCHITZ[act]
    xm = pre.abs() + bpre
    ym = act_f64(pre, act).abs() + L * bpre
    bval = L * bpre + act_approx_bound(xm, ym, act, fast_act)
    mag = out.abs() + bval
    if out_fmt == "h2":
        bout = h2_delta(mag)
    else:
        bout = half_ulp(mag, out_fmt)
    return bval + bout


def check_within(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """Every element of `got` within `bound` of `ref` (NaN / inf fail); returns the largest err / bound ratio."""
    err = (got.double() - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements outside the bound; first at {i}: got {float(got[i])}, "
                             f"ref {float(ref[i])}, bound {float(bound[i])}")
    return float((err / bound).max())


# ---- operand storage ---------------------------------------------------------------------------------------------------------------
def pack_h2(x: torch.Tensor) -> torch.Tensor:
    """f32 [.., K] (K % 8 == 0) -> two-plane storage as f16 [.., 2K]: groups of 8 elements as [8 hi][8 lo], hi = f16(x), lo = f16(x - hi)."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    lead, k = x.shape[:-1], x.shape[-1]
    return torch.stack([hi.view(*lead, k // 8, 8), lo.view(*lead, k // 8, 8)], dim=-2).reshape(*lead, 2 * k)


def unpack_h2(p: torch.Tensor) -> torch.Tensor:
    """Two-plane storage f16 [.., 2K] -> the float64 values hi + lo [.., K]."""
    lead, k2 = p.shape[:-1], p.shape[-1]
    g = p.view(*lead, k2 // 16, 2, 8).double()
    return (g[..., 0, :] + g[..., 1, :]).reshape(*lead, k2 // 2)
