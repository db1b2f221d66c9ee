"""f64 references and per-element error bounds for the HIP GEMMs (used by tests/test_gpu_gemm_reference.py and tests/test_gemm_bound_cpu.py;
the MXFP8 helpers at the end by tests/test_gpu_gemm_mx_reference.py and tests/test_gemm_mx_bound_cpu.py).

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
FORMATS = {"f32": (24, -125), "bf16": (8, -125), "f16": (11, -13), "e4m3": (4, -5)}
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
               two_plane: bool = False, fast_act: bool = True, extra_pre=None) -> torch.Tensor:
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
    * extra_pre: a further per-element bound on the pre-activation error, in the output's units, derived from a stated model by the caller
      (`f8_align_bound` for the block-scaled fp8 forms).
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
    if extra_pre is not None:
        bpre = bpre + extra_pre
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


# ---- MXFP8: e4m3 bytes with one E8M0 scale per 32 elements (include/segearth_hip.h: sg_gemm_fp8_mx_raw) ---------------------------------------
# Hardware model the bounds on the block-scaled forms rest on (stated, not fitted):
#   * every product of two e4m3 values and a power-of-two block scale is exact: 4 + 4 significand bits, and the scale only moves the exponent
#     (operands and scales are kept where every such product and every partial sum is a normal f32);
#   * v_mfma_scale_f32_16x16x128_f8f6f4 sums a 128-wide K step in groups of 16 consecutive K.  Inside a group the products are aligned to the
#     group's largest exponent (the sum of the two operands' exponents, an e4m3 subnormal counting as 2^-6, plus the block scale) and only the bits
#     down to 2^-13 of it are kept: a product 2^-13 of the largest still counts, one of 2^-14 is dropped.  Across groups the window is far
#     wider (a product 2^-27 of the largest term of its 64-wide half, accumulator included, still counts); what is kept is summed exactly and
#     rounded to f32 once per half.  This is MEASURED on the
#     instruction itself with chosen operands (tools/mx_accum_probe.hip, recorded in DESIGN.md), not taken from a GEMM's error.  Hence a group
#     with n non-zero products loses less than (n - 1) 2^(Emax - 13): the largest product (8 significant bits) is exact, every other loses less
#     than one unit -- `f8_align_bound`;
#   * the rest -- per half 64 products each cut below 2^-27 of the largest term, and one rounding: (2^-21 + 2^-24) of the partial sum of |terms|
#     -- is well inside 2u 64 of it, so it stays within `gemm_bound`'s 2u K S term, with the reference operand A = mx_decode(a8, a_mx).
# The MX epilogue holds act(..) in f32 (bounded by gemm_bound(.., out_fmt="f32")), takes the block maximum of |value| over 32 columns exactly,
# picks the scale by `mx_scale_rule`, multiplies by the exact power of two 2^(127 - E) and rounds to e4m3 to nearest (ties to even).
F8_ALIGN_BITS = 13                                        # tools/mx_accum_probe.hip: bits kept below a 16-group's largest product exponent


def e4m3_exponent(b8: torch.Tensor):
    """(binary exponent the matrix unit aligns an e4m3 byte by: its exponent field - 7, a subnormal counting as -6; the byte is non-zero)."""
    field = ((b8 >> 3) & 0xF).to(torch.float32)
    return torch.clamp(field, min=1.0) - 7.0, (b8 & 0x7F) != 0


def f8_align_bound(a8: torch.Tensor, w8: torch.Tensor, a_blk=None) -> torch.Tensor:
    """Bound [M, N], in accumulator units, on what the fp8 matrix unit loses inside its groups of 16 consecutive K (the model above): per group
    (n - 1) 2^(Emax - 13) with n the non-zero products and Emax the largest exponent sum.  a8 [M, K], w8 [N, K] e4m3 bytes; a_blk [M, K/32] the
    E8M0 bytes of A's blocks (None: no block scales)."""
    ea, na = e4m3_exponent(a8)
    ew, nw = e4m3_exponent(w8)
    if a_blk is not None:
        ea = ea + (a_blk.to(torch.float32) - 127.0).repeat_interleave(32, dim=1)
    ninf = float("-inf")
    ea, ew = torch.where(na, ea, torch.full_like(ea, ninf)), torch.where(nw, ew, torch.full_like(ew, ninf))
    out = torch.zeros(a8.shape[0], w8.shape[0], dtype=torch.float64, device=a8.device)
    for k in range(0, a8.shape[1], 16):
        emax = (ea[:, None, k:k + 16] + ew[None, :, k:k + 16]).amax(dim=2).double()
        n = na[:, k:k + 16].double() @ nw[:, k:k + 16].double().T
        out += (n - 1).clamp(min=0) * torch.exp2(emax - F8_ALIGN_BITS)
    return out


def mx_decode(bytes_u8: torch.Tensor, scales_u8: torch.Tensor):
    """e4m3 bytes [R, C] with E8M0 block scales laid out [C/128][R][4] (the four 32-element blocks of one 128-wide step of a row form one dword)
    -> (float64 [R, C] = e4m3 value x 2^(byte - 127), the scale bytes per block [R, C/32] as int64)."""
    R, Cc = bytes_u8.shape
    assert bytes_u8.dtype == torch.uint8 and scales_u8.dtype == torch.uint8 and tuple(scales_u8.shape) == (Cc // 128, R, 4) and Cc % 128 == 0
    blk = scales_u8.permute(1, 0, 2).reshape(R, Cc // 32).to(torch.int64)
    val = bytes_u8.view(torch.float8_e4m3fn).to(torch.float32).double()
    return torch.ldexp(val, (blk - 127).repeat_interleave(32, dim=1)), blk


def mx_scale_rule(amax: torch.Tensor) -> torch.Tensor:
    """The E8M0 byte of a block with maximum magnitude `amax` (real, >= 0): the smallest integer E >= 0 with amax <= 448 2^(E - 127), E = 0 for
    amax = 0.  Through frexp, amax = m 2^e with m in [0.5, 1): 448 = 0.875 2^9, so E = 127 + e - 9 + (m > 0.875), clamped at 0 -- no
    floating-point logarithm.  For a normal f32 this is the kernel's bit rule "exponent field - 8, + 1 if the mantissa exceeds 1.75's"."""
    a = amax.double()
    m, e = torch.frexp(a)
    E = 127 + e.to(torch.int64) - 9 + (m > 0.875).to(torch.int64)
    return torch.where(a > 0, E.clamp(min=0), torch.zeros_like(E))


def mx_output_check(c8: torch.Tensor, cs: torch.Tensor, ref: torch.Tensor, B: torch.Tensor, what: str = ""):
    """An MX output (e4m3 bytes c8 [M, N], scale bytes cs [N/128][M][4]) against the f64 post-activation reference `ref`, with B the bound on
    the f32 value the epilogue holds before it quantises (gemm_bound(.., out_fmt="f32")):
      1. no byte is an e4m3 NaN (byte & 0x7f == 0x7f) and no scale byte is 255 -- outputs start as 0xFF, so a cell never written fails here;
      2. each block's scale byte lies in [mx_scale_rule(max_blk max(|ref| - B, 0)), mx_scale_rule(max_blk (|ref| + B))]; a block where the two
         ends differ is ambiguous (either byte is accepted);
      3. each element, with s = 2^(byte - 127) of the output's OWN scale: |decode - ref| <= B + s half_ulp((|ref| + B) / s, "e4m3").
    Returns (largest err / bound, share of ambiguous blocks)."""
    M, N = c8.shape
    nan8 = (c8 & 0x7F) == 0x7F
    assert not bool(nan8.any()), f"{what}: {int(nan8.sum())} output bytes are e4m3 NaN (or were never written)"
    assert not bool((cs == 255).any()), f"{what}: {int((cs == 255).sum())} scale bytes are 255 (NaN, or never written)"
    got, blk = mx_decode(c8, cs)
    ref = ref.double()
    hi_mag = ref.abs() + B
    lo = mx_scale_rule((ref.abs() - B).clamp(min=0).view(M, N // 32, 32).amax(dim=2))
    hi = mx_scale_rule(hi_mag.view(M, N // 32, 32).amax(dim=2))
    bad = (blk < lo) | (blk > hi)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} block scales outside the rule; first at (row, block) {i}: byte "
                             f"{int(blk[i])}, allowed {int(lo[i])}..{int(hi[i])}")
    ambiguous = float((lo != hi).double().mean())
    s = torch.ldexp(torch.ones_like(ref), (blk - 127).repeat_interleave(32, dim=1))
    bound = B + s * half_ulp(hi_mag / s, "e4m3")
    return check_within(got, ref, bound, what), ambiguous


def mx_coherent_operands(M_, N_, K_, g, device="cpu", row_gain=None):
    """f32 A [M_, K_] >= 0 and W [N_, K_] with one sign per output column: every product of an output element has the same sign, so
    S = |A|.|W|^T equals |A.W^T| and the worst-case bound B = 2u (K + 3) S + .. is ~1e-4 of the VALUE.  With zero-mean operands S is
    ~0.31 sqrt(K) times a block's maximum, B spans ~2e-4 of it, and about 0.07 % of all blocks have their maximum within B of a scale
    threshold 448 2^k whatever the kernel does -- which would let the "either byte" allowance of `mx_output_check` be met by the inputs
    alone.  Rows carry gains 2^[-4, 2] (or `row_gain`), columns 2^[-3, 1]: neighbouring rows and blocks differ in their scale bytes, and
    the pre-activations (0.1 .. 100 in magnitude, both signs) cover the activations' curved range."""
    rand = lambda *s: torch.rand(*s, generator=g, device=device)
    randn = lambda *s: torch.randn(*s, generator=g, device=device)
    rg = torch.exp2(rand(M_) * 6 - 4) if row_gain is None else row_gain
    A = randn(M_, K_).abs() * rg[:, None]
    sign = torch.where(rand(N_) < 0.5, -1.0, 1.0)
    W = randn(N_, K_).abs() * K_ ** -0.5 * (sign * torch.exp2(rand(N_) * 4 - 3))[:, None]
    return A, W


# The exact table: operands on which every block maximum of the MX epilogue is exactly 448 2^k, 464 2^k (= 448 + 16) or 480 2^k, every sum is
# exact in f32, and the expected scale and data bytes are written down here -- not derived through a bound.  Row m of A holds (448, 0), (448, 16),
# (448, 32) or nothing in its first two K positions (m % 4 = 0, 1, 2, 3; per-row scale 1); W's first two K positions both hold w(n), with the six
# values of MX_TABLE_W in consecutive columns of every 32-column block (starting at column 5 b % 26 of block b, so the block maximum sits in a
# different lane of the quad each time) and per-row scale 2^k, k = -20, 0, 20 by block.  So C[m, n] = T(m) w(n) 2^k with T = 448, 464, 480, 0.
MX_TABLE_W = (1.0, 0.5, -0.5, 0.25, -1.0, 0.0)
MX_TABLE = {                                               # T -> (scale byte - 127 - k, the e4m3 bytes of T w / 2^(that) for w in MX_TABLE_W)
    448: (0, (0x7E, 0x76, 0xF6, 0x6E, 0xFE, 0x00)),        # 448 224 -224 112 -448: the largest e4m3 value itself, E = 127 + k kept
    464: (1, (0x76, 0x6E, 0xEE, 0x66, 0xF6, 0x00)),        # 232 116 -116 58 -232: all ties, to even: 224 112 -112 56 -224
    480: (1, (0x77, 0x6F, 0xEF, 0x67, 0xF7, 0x00)),        # 240 120 -120 60 -240: representable
}
MX_TABLE_K = (-20, 0, 20)


def mx_exact_table(M: int, N: int, K: int, device="cpu"):
    """(A8 [M, K] u8, sa [M], W8 [N, K] u8, sw [N], expected c8 [M, N] u8, expected cs [N/128][M][4] u8) of the exact-table case (act 0, no bias)."""
    assert N % 128 == 0 and K >= 2
    A = torch.zeros(M, K)
    m = torch.arange(M)
    A[m % 4 != 3, 0] = 448.0
    A[m % 4 == 1, 1] = 16.0
    A[m % 4 == 2, 1] = 32.0
    W = torch.zeros(N, K)
    sw = torch.ones(N)
    c8 = torch.zeros(M, N, dtype=torch.uint8)
    E = torch.zeros(M, N // 32, dtype=torch.uint8)
    for b in range(N // 32):
        k, c0 = MX_TABLE_K[b % 3], 32 * b + (5 * b) % 26
        sw[32 * b:32 * b + 32] = 2.0 ** k
        W[c0:c0 + 6, 0] = W[c0:c0 + 6, 1] = torch.tensor(MX_TABLE_W)
        for r, T in enumerate((448, 464, 480)):
            dE, data = MX_TABLE[T]
            E[r::4, b] = 127 + k + dE
            c8[r::4, c0:c0 + 6] = torch.tensor(data, dtype=torch.uint8)
    cs = E.view(M, N // 128, 4).permute(1, 0, 2).contiguous()
    to8 = lambda x: x.to(torch.float8_e4m3fn).view(torch.uint8)
    return tuple(t.to(device) for t in (to8(A), torch.ones(M), to8(W), sw, c8, cs))
