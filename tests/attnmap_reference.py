"""f64 references, per-element error bounds and case tables for the parity-mode f32 GEMM in its strided / batched forms
(csrc/gemm_f32.hip through sg_gemm_f32_raw) and for the attention-map stages built on it: the head-averaged attention
(sg_attn_average_raw), the mode='attention' enhancer (sg_attn_enhance_raw), the layer-fusion re-weighting (sg_layer_fusion_apply_raw) and
the similarity map (sg_similarity_map).  Used by tests/test_gpu_gemm_f32_reference.py, tests/test_gpu_attnmap_reference.py and
tests/test_attnmap_bound_cpu.py.

Conventions as in gemm_reference / refine_reference: u = 2^-24, every f32 operation is charged 2u of the magnitude it rounds, a sum of n
terms 2u n of the sum of the magnitudes, a 64-lane strided sum 2u lane_terms(n); ASSUMPTION: expf, erff and the reciprocal are within
2 ulp (EXPF).  TINY is the absolute floor wherever an f32 intermediate may underflow.  Every bound is a tensor built term by term from the
magnitudes of the operands the kernels consume, never from an observed output; each term is commented where it is added.  Elements the
reference makes exact (column 0 of the boosted map, masked columns, the CLS row the enhancer leaves alone, the zeroed diagonal) carry the
bound 0 and are compared for equality.  Plain torch / numpy on the CPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from gemm_reference import U, gemm_bound
from refine_reference import (EXPF, RANK_GAP, TINY, check_within, decade_rows, f32, lane_terms, rank_gap,  # noqa: F401
                              selection_reference, selection_scores)
import rowops_reference as RW
from oracle import refine as OR

KINDS = RW.KINDS                                    # "f32", "bf16", "f16", "h2"
PREC = RW.PREC
EPS_ROW = 1e-8                                      # the "+ 1e-8" of both row normalisations (the kernels hold it as an f32 constant)


# ---- the f32 GEMM, any strides ----------------------------------------------------------------------------------------------------
def strided_index(rows: int, cols: int, s_row: int, s_col: int, so: int, si: int, batch: int, inner: int) -> torch.Tensor:
    """Flat element index [batch, rows, cols] of element (r, c) of problem z: (z // inner) so + (z % inner) si + r s_row + c s_col."""
    z = torch.arange(batch)
    return ((z // inner) * so + (z % inner) * si)[:, None, None] + torch.arange(rows)[None, :, None] * s_row \
        + torch.arange(cols)[None, None, :] * s_col


def gemm_indices(g: dict):
    """(A [batch, M, K], B [batch, K, N], C [batch, M, N], residual [batch, M, N]) flat indices of the form g (GemmF32Args' fields by name);
    the residual is batched by C's strides with its own leading dimension, as the kernel reads it."""
    bt, inn = g["batch"], g["inner"]
    return (strided_index(g["M"], g["K"], g["lda"], 1, g["sAo"], g["sAi"], bt, inn),
            strided_index(g["K"], g["N"], g["sbk"], g["sbn"], g["sBo"], g["sBi"], bt, inn),
            strided_index(g["M"], g["N"], g["ldc"], 1, g["sCo"], g["sCi"], bt, inn),
            strided_index(g["M"], g["N"], g["ldr"], 1, g["sCo"], g["sCi"], bt, inn))


def gemm_products(bufA: torch.Tensor, bufB: torch.Tensor, g: dict):
    """(acc, S) [batch, M, N] f64: sum_k A(m, k) B(k, n) and sum_k |A(m, k)| |B(k, n)|, by plain indexing of the flat buffers, one k at a
    time (no layout is assumed beyond the strides of g)."""
    ia, ib, _, _ = gemm_indices(g)
    a, b = bufA.double().reshape(-1)[ia], bufB.double().reshape(-1)[ib]
    acc = torch.zeros(g["batch"], g["M"], g["N"], dtype=torch.float64)
    S = torch.zeros_like(acc)
    for k in range(g["K"]):
        col, row = a[:, :, k, None], b[:, k, None, :]
        acc += col * row
        S += col.abs() * row.abs()
    return acc, S


def act_f64(x: torch.Tensor, act: int) -> torch.Tensor:
    """0 none, 1 QuickGELU x sigmoid(1.702 x), 2 erf-GELU, 3 ReLU (csrc/common.h: enum Act)."""
    if act == 0:
        return x
    if act == 1:
        return x * torch.sigmoid(1.702 * x)
    if act == 2:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == 3:
        return x.clamp(min=0.0)
    raise ValueError(act)


ACT_LIPSCHITZ = {0: 1.0, 1: 1.13, 2: 1.13, 3: 1.0}   # gemm_reference.LIPSCHITZ, and ReLU


def act_f32_bound(xm: torch.Tensor, ym: torch.Tensor, act: int) -> torch.Tensor:
    """|device activation(x) - exact activation(x)| for an f32 x with |x| <= xm, |act(x)| <= ym, parity-mode forms (common.h):
      * quick_gelu_exact x (1 / (1 + expf(-1.702f x))): the constant's rounding and the product 4u |1.702 x| on the exponent's argument,
        i.e. relative on e; expf EXPF; both damped by e / (1 + e) <= 1; 1 + e 2u; the reciprocal EXPF; the product 2u -- relative to |y|.
      * erf_gelu 0.5f x (1 + erff(x 0.7071f)): the argument's two roundings 4u |a| pass through erf' = 1.1284 exp(-a^2), and
        1.1284 a exp(-a^2) <= 0.49, so < 2u; erff EXPF of |erf| <= 1; 1 + erf 2u of at most 2 = 4u: absolute on the bracket, times 0.5 |x|;
        the two products 4u |y|.
      * ReLU and none: exact."""
    if act in (0, 3):
        return torch.zeros_like(xm)
    if act == 1:
        return ym * (4 * U * 1.702 * xm + EXPF + 2 * U + EXPF + 2 * U) + TINY
    if act == 2:
        return 0.5 * xm * (2 * U + EXPF + 4 * U) + 4 * U * ym + TINY
    raise ValueError(act)


def gemm_epilogue_reference(acc, S, K: int, alpha: float, bias=None, residual=None, act: int = 0):
    """(out, bound) [batch, M, N] f64 of act(alpha acc + bias[n]) + residual from `gemm_products`; alpha is the f32 value the kernel gets,
    residual the gathered [batch, M, N] values.  Terms, in the kernel's order:
      * the K-long fmaf chain of the matrix unit, one rounding per step:            2u K S
      * x = acc alpha, one product (|acc| <= S):                                    2u |alpha| S, the chain's error scaled by |alpha|
      * x += bias[n]:                                                               2u (|alpha| S + |bias|)
      * the activation: the above times its Lipschitz constant, plus `act_f32_bound` at the largest |x| the kernel can have seen
      * x += residual:                                                              2u (|act| + its bound + |residual|)
      * TINY once (products of small operands)."""
    a = abs(alpha)
    pre = alpha * acc
    bpre = 2 * U * K * S * a + 2 * U * a * S
    if bias is not None:
        pre = pre + bias.double()
        bpre = bpre + 2 * U * (a * S + bias.double().abs())
    val = act_f64(pre, act)
    bval = ACT_LIPSCHITZ[act] * bpre + act_f32_bound(pre.abs() + bpre, val.abs() + ACT_LIPSCHITZ[act] * bpre, act)
    out = val
    if residual is not None:
        out = val + residual.double()
        bval = bval + 2 * U * (val.abs() + bval + residual.double().abs())
    return out, bval + TINY


def gemm_strided_reference(bufA, bufB, g: dict, bias=None, bufR=None):
    """The whole of one sg_gemm_f32_raw call: dict(out, bound [batch, M, N] f64, ic = the flat indices of C's elements)."""
    _, _, ic, ir = gemm_indices(g)
    acc, S = gemm_products(bufA, bufB, g)
    res = None if bufR is None else bufR.reshape(-1)[ir]
    out, bound = gemm_epilogue_reference(acc, S, g["K"], f32(g["alpha"]), bias, res, g["act"])
    return dict(out=out, bound=bound, ic=ic)


# case table of the GEMM forms ---------------------------------------------------------------------------------------------------------
GEMM_MN = ((1, 1), (127, 129), (130, 260))          # one element; one ragged tile; more than one tile both ways, both ragged
GEMM_K = (1, 15, 17, 197)                           # below, just below and just above one FK = 16 step; 12 steps and a ragged 5
GEMM_LAYOUTS = ("nk", "kn")                         # B stored [N, ldb] (sbk = 1, sbn = ldb > K) / [K, ldb] (sbn = 1, sbk = ldb > N: b_n_fast)
GEMM_ALPHAS = (1.0, 0.37, -2.0)
GEMM_EPILOGUES = (("none", False, 0, False), ("bias", True, 0, False), ("bias+quickgelu", True, 1, False), ("bias+gelu", True, 2, False),
                  ("bias+relu", True, 3, False), ("bias+residual", True, 0, True))          # (name, bias, act, residual)
GEMM_BATCH, GEMM_INNER = 6, 3


def _no_multiples(vals) -> bool:
    return all(a != b and a % b != 0 and b % a != 0 for i, a in enumerate(vals) for b in vals[i + 1:])


def pick_batch_strides(eA: int, eB: int, eC: int):
    """(sAo, sAi, sBo, sBi, sCo, sCi): the three inner strides clear their operand's extent, the outer ones three inner steps; six
    distinct values, none a multiple of another (so that exchanging any two addresses other elements).  The smallest paddings that do."""
    chosen = []

    def take(at_least: int) -> int:
        v = at_least
        while not _no_multiples(chosen + [v]):
            v += 1
        chosen.append(v)
        return v

    sAi, sBi, sCi = take(eA + 2), take(eB + 3), take(eC + 5)
    sAo, sBo, sCo = take(3 * sAi + 1), take(3 * sBi + 1), take(3 * sCi + 1)
    return sAo, sAi, sBo, sBi, sCo, sCi


def gemm_form(M: int, N: int, K: int, layout: str, batch: int = GEMM_BATCH, inner: int = GEMM_INNER) -> dict:
    """The strides of one table case: lda > K, ldc > N, ldr != ldc, ldb past the fast dimension, two-level batching."""
    lda, ldc, ldr = K + 3, N + 5, N + 2
    ldb = (K + 2) if layout == "nk" else (N + 7)
    sbk, sbn = (1, ldb) if layout == "nk" else (ldb, 1)
    eA, eC = (M - 1) * lda + K, (M - 1) * ldc + N
    eB = (N - 1) * sbn + (K - 1) * sbk + 1
    sAo, sAi, sBo, sBi, sCo, sCi = pick_batch_strides(eA, eB, eC)
    return dict(M=M, N=N, K=K, batch=batch, inner=inner, lda=lda, sAo=sAo, sAi=sAi, sbk=sbk, sbn=sbn, sBo=sBo, sBi=sBi,
                ldc=ldc, ldr=ldr, sCo=sCo, sCi=sCi, act=0, alpha=1.0)


def buffer_len(idx: torch.Tensor) -> int:
    return int(idx.max()) + 1


GEMM_SENTINEL = -12345.5


def make_gemm_buffers(g: dict, seed: int):
    """Flat f32 buffers (A, B, bias [N], residual, C) that cover the form's indices, with a few elements of slack; C and every element
    of A / B / residual outside the operands hold values a wrong stride would pick up (A, B: N(0, 1) everywhere; C: the sentinel)."""
    ia, ib, ic, ir = gemm_indices(g)
    gen = torch.Generator().manual_seed(7000 + seed)
    A = torch.randn(buffer_len(ia) + 8, generator=gen)
    B = torch.randn(buffer_len(ib) + 8, generator=gen) * g["K"] ** -0.5
    bias = torch.randn(g["N"], generator=gen) * 0.5
    R = torch.randn(max(buffer_len(ir), buffer_len(ic)) + 8, generator=gen)
    Cbuf = torch.full((buffer_len(ic) + 8,), GEMM_SENTINEL)
    return A, B, bias, R, Cbuf


def gemm_cases():
    """[(tag, M, N, K, layout)] of the table, in a fixed order (the index seeds the operands and rotates alpha over the epilogues)."""
    return [(f"{M}x{N}x{K} {lay}", M, N, K, lay) for (M, N) in GEMM_MN for K in GEMM_K for lay in GEMM_LAYOUTS]


def alpha_of(case_index: int, epilogue_index: int) -> float:
    """alpha rotates so that over the table every epilogue and every shape meets each of the three values."""
    return GEMM_ALPHAS[(case_index // 2 + case_index % 2 + epilogue_index) % 3]


def aliased_form(n: int = 130, D: int = 17, batch: int = 2) -> dict:
    """similarity_from_xhat's form: A and B are the same [batch, n, D] buffer (sbk = 1, sbn = D, strideA = strideB), C [batch, n, n]."""
    return dict(M=n, N=n, K=D, batch=batch, inner=1, lda=D, sAo=n * D, sAi=0, sbk=1, sbn=D, sBo=n * D, sBi=0, ldc=n, ldr=n, sCo=n * n,
                sCi=0, act=0, alpha=2.0)


def reweight_form(N: int = 197, D: int = 64, batch: int = 2) -> dict:
    """The enhancer's and the layer fusion's form: A [batch, N, N] . tokens [batch, N, D] (sbk = D, sbn = 1: the b_n_fast loader, K = N)."""
    return dict(M=N, N=D, K=N, batch=batch, inner=1, lda=N, sAo=N * N, sAi=0, sbk=D, sbn=1, sBo=N * D, sBi=0, ldc=D, ldr=D, sCo=N * D,
                sCi=0, act=0, alpha=1.0)


# ---- shared pieces of the attention-map stages -------------------------------------------------------------------------------------------
def softmax_with_bound(v: torch.Tensor, d: torch.Tensor):
    """softmax over the last axis of the f64 arguments v known to +-d, as softmax_rows_kernel evaluates it: (w, dw).
      * the common shift cancels; with per-entry errors d_j, log(w'_j / w_j) lies within d_j + M, M = log sum_l w_l exp(d_l)
        (refine_reference.attention_fuse_bound): w_j expm1(d_j + M);
      * relative on top: v_j - max one rounding 2u |v_j - max| (beyond 110 the term underflows to the TINY floor), expf EXPF;
        the N-term 64-lane sum 2u lane_terms(N) plus the weighted mean of its terms' relative errors; the reciprocal EXPF; the product 2u;
      * TINY: a term below the smallest normal f32 may be flushed."""
    N = v.shape[-1]
    w = torch.softmax(v, -1)
    M = torch.log((w * torch.exp(d.clamp(max=50.0))).sum(-1, keepdim=True))
    we = w * torch.expm1((d + M).clamp(max=50.0))
    rel = EXPF + 2 * U * (v.max(-1, keepdim=True).values - v).clamp(max=110.0)
    rho = rel + (w * rel).sum(-1, keepdim=True) + 2 * U * lane_terms(N) + EXPF + 2 * U
    return w, we * (1 + rho) + w * rho + TINY


def row_normalise_bound(t: torch.Tensor, dt: torch.Tensor):
    """t / (sum_j t_j + 1e-8) over the last axis for the f64 terms t known to +-dt, as attn_boost_kernel / fusion_mask_normalize_kernel do:
    (value, bound).  The 64-lane sum misses by 2u lane_terms(N) sum|t| + sum dt; + 1e-8f one addition 2u, and the f32 constant differs
    from 1e-8 by at most u 1e-8; the reciprocal EXPF; the product 2u; each term's own error dt_j over the denominator."""
    N = t.shape[-1]
    den = t.sum(-1, keepdim=True) + EPS_ROW
    dsum = 2 * U * lane_terms(N) * t.abs().sum(-1, keepdim=True) + dt.sum(-1, keepdim=True) + U * EPS_ROW
    rel = dsum / den.abs() + 2 * U + EXPF + 2 * U
    val = t / den
    return val, val.abs() * rel + dt / den.abs()


def reweight_with_bound(a: torch.Tensor, da: torch.Tensor, x: torch.Tensor):
    """a [B, N, N] (known to +-da) . x [B, N, D] through the f32 GEMM (K = N, alpha = 1): (value, bound) with the operand error carried
    through |x|, the chain 2u N, the alpha product 2u, and TINY."""
    N = a.shape[-1]
    mag = (a.abs() + da) @ x.abs()
    return a @ x, da @ x.abs() + 2 * U * (N + 1) * mag + TINY


# ---- head-averaged attention -----------------------------------------------------------------------------------------------------------
def scale_f32(dh: int) -> float:
    """1.0f / sqrtf((float)dh) as the host computes it (both operations correctly rounded)."""
    return float(np.float32(1.0) / np.sqrt(np.float32(dh)))


def average_probs_reference(probs: torch.Tensor):
    """Parity mode: probs [B, H, N, N] f32 given; head_mean_kernel adds the H values in order and divides: 2u H mean|p| for the sum, 2u
    for the division."""
    p = probs.double()
    H = p.shape[1]
    return p.mean(1), 2 * U * (H + 1) * p.abs().mean(1) + TINY


def average_qkv_reference(vals: torch.Tensor, H: int):
    """2-byte modes: vals [B, N, 3D] f64 = the stored bf16 / f16 / two-plane values, which unpack_qk_kernel turns into f32 exactly, so the
    whole stage is f32 arithmetic on them:
      * scores q_i . k_j per head through the f32 GEMM (K = dh, alpha = 1): 2u (dh + 1) S;
      * softmax_rows: the product with the f32 scale 2u |v| on top of the scaled score error, then `softmax_with_bound`;
      * head_mean: 2u (H + 1) of the mean magnitude, the per-head errors averaged."""
    B, N, D3 = vals.shape
    D = D3 // 3
    dh = D // H
    q = vals[..., :D].view(B, N, H, dh).permute(0, 2, 1, 3)
    k = vals[..., D:2 * D].view(B, N, H, dh).permute(0, 2, 1, 3)
    dot, S = q @ k.transpose(-1, -2), q.abs() @ k.abs().transpose(-1, -2)
    sc = scale_f32(dh)
    v = dot * sc
    d = sc * (2 * U * (dh + 1) * S + TINY) + 2 * U * v.abs()
    w, dw = softmax_with_bound(v, d)
    return w.mean(1), dw.mean(1) + 2 * U * (H + 1) * (w + dw).mean(1) + TINY


# ---- mode='attention' enhancer ---------------------------------------------------------------------------------------------------------
def enhance_reference(tokens: torch.Tensor, A: torch.Tensor, strength: float, threshold: float):
    """oracle.refine.self_attention_enhance(mode="attention") in f64 on tokens [B, N, D] and the map A [B, N, N] (f32; strength, threshold
    the f32 values the kernel receives).  Returns dict(out, bound [B, N, D]; amap, amap_bound [B, N, N] = what the kernel leaves in A).
      * boost_i = max(threshold - A_ii, 0) strength for i >= 1: the subtraction and the product, 4u boost; a difference that is not
        positive gives exactly 0 (an f32 subtraction has the exact sign);
      * the diagonal term A_ii + boost_i: 2u of it, plus the boost's error;
      * `row_normalise_bound` on the terms; column 0 is then written as 0 (bound 0);
      * `reweight_with_bound`; row 0 of tokens is not written (bound 0)."""
    B, N, D = tokens.shape
    gh = int(round(math.sqrt(N - 1)))
    assert gh * gh == N - 1
    a, x = A.double(), tokens.double()
    diag = torch.diagonal(a, dim1=1, dim2=2)
    boost = (threshold - diag).clamp(min=0.0) * strength
    boost[:, 0] = 0.0
    t = a + torch.diag_embed(boost)
    dt = torch.diag_embed(torch.where(boost > 0, 4 * U * boost + 2 * U * (diag.abs() + boost), torch.zeros_like(boost)))
    amap, damap = row_normalise_bound(t, dt)
    amap[:, :, 0], damap[:, :, 0] = 0.0, 0.0
    prod, dprod = reweight_with_bound(amap, damap, x)
    out, bound = x.clone(), torch.zeros_like(x)
    out[:, 1:], bound[:, 1:] = prod[:, 1:], dprod[:, 1:]
    grid = x[:, 1:].permute(0, 2, 1).reshape(B, D, gh, gh)
    orc = OR.self_attention_enhance(grid, a, enhancement_strength=strength, min_self_attn_threshold=threshold, mode="attention")
    orc = orc.reshape(B, D, N - 1).permute(0, 2, 1)
    if not bool(((orc - out[:, 1:]).abs() <= 1e-6 * bound[:, 1:] + 1e-300).all()):      # f64 summation orders differ by ~1e-16
        raise AssertionError("enhance_reference disagrees with the oracle")
    return dict(out=out, bound=bound, amap=amap, amap_bound=damap, boosted=boost > 0)


# ---- layer fusion --------------------------------------------------------------------------------------------------------------------------
def fusion_reference(acc: torch.Tensor, tokens: torch.Tensor, top_k: int):
    """The fusion branch of oracle.vit.vit_forward (reference transformer.py:647-690) on a given fused map acc [B, N, N] and last-block
    output tokens [B, N, D] (f32), in f64: dict(a_cls, a_diag [B, N] f32 exact copies; idx [B, k]; gap; amap, amap_bound [B, N, N];
    out, bound [B, N, D]; masked [B, N] bool).
      * row 0 and the diagonal are copied (exact); the selection is refine_reference's (determinate where gap > 2.4e-7);
      * masked columns are written as 0 (bound 0); the rest `row_normalise_bound` (terms read exactly) and `reweight_with_bound`."""
    B, N, D = tokens.shape
    n = N - 1
    k = min(top_k, n)
    a, x = acc.double(), tokens.double()
    a_cls, a_diag = acc[:, 0, :].clone(), torch.diagonal(acc, dim1=1, dim2=2).clone()
    scores = selection_scores(a_cls, a_diag, False)
    idx = selection_reference(scores, k)
    assert torch.equal(torch.sort(idx, 1).values, torch.sort(OR.detect_outliers(a, n, top_k), 1).values)
    masked = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        masked[b, idx[b] + 1] = True
    am = torch.where(masked[:, None, :], torch.zeros_like(a), a)
    amap, damap = row_normalise_bound(am, torch.zeros_like(am))
    damap = torch.where(masked[:, None, :], torch.zeros_like(damap), damap)
    out, bound = reweight_with_bound(amap, damap, x)
    mask = (~masked).double()
    orc = a * mask[:, None, :]
    orc = torch.bmm(orc / (orc.sum(-1, keepdim=True) + 1e-8), x)                      # oracle/vit.py, the fusion branch, verbatim
    if not bool(((orc - out).abs() <= 1e-6 * bound).all()):
        raise AssertionError("fusion_reference disagrees with the oracle's statement")
    return dict(a_cls=a_cls, a_diag=a_diag, idx=idx, gap=rank_gap(scores, k), amap=amap, amap_bound=damap, out=out, bound=bound,
                masked=masked)


# ---- similarity map --------------------------------------------------------------------------------------------------------------------------
def similarity_reference(xhat: torch.Tensor, temperature: float, add_self: bool, kind: str):
    """sim [B, n, n] = (1 / temperature) xhat . xhat^T of the STORED normalised rows xhat [B, n, D] f64 (read back from the caller's
    scratch), diagonal zeroed without add_self: (value, bound).  alpha = 1.0f / temperature as the host computes it.
      * f32: the f32 GEMM's terms (chain 2u D S, alpha product 2u S) scaled by |alpha|;
      * 2-byte / two-plane: gemm_reference.gemm_bound of the unscaled product (f32 output) scaled by |alpha|, plus the alpha product 2u;
      * the zeroed diagonal is exact (bound 0)."""
    alpha = float(np.float32(1.0) / np.float32(temperature))
    acc = xhat @ xhat.transpose(1, 2)
    if kind == "f32":
        S = xhat.abs() @ xhat.abs().transpose(1, 2)
        bound = abs(alpha) * (2 * U * xhat.shape[-1] * S + 2 * U * S) + TINY
    else:
        b0 = gemm_bound(xhat, xhat, None, acc, acc, act=0, out_fmt="f32", two_plane=(kind == "h2"))
        bound = abs(alpha) * b0 + 2 * U * abs(alpha) * (acc.abs() + b0) + TINY
    sim = alpha * acc
    if not add_self:
        eye = torch.eye(xhat.shape[1], dtype=torch.bool)[None]
        sim, bound = sim.masked_fill(eye, 0.0), bound.masked_fill(eye, 0.0)
    return sim, bound


# ---- case table of the stages ----------------------------------------------------------------------------------------------------------------
GRIDS = (1, 6, 8, 14, 18)                           # N = gh^2 + 1 = 2, 37, 65, 197, 325
BATCHES = (1, 3)
HEADS = ((3, 32), (2, 64))                          # (H, dh): D = 96, 128
TOP_KS = (1, 30, 300)
THRESHOLDS = (0.15, 0.0)                            # 0: no row is boosted
STRENGTH = 0.5
SIM_N = (36, 196, 324)
SIM_D = (64, 192)
SIM_TEMPS = (1.0, 0.5)
SIM_B = 2
TOKEN_PAD = 24                                      # elements between the images of the enhancer's tokens (sb = N D + TOKEN_PAD)
FAINT = 3e-8                                        # row sum of the enhancer's faint row: the + 1e-8 is a quarter of its denominator


def tokens_of(gh: int) -> int:
    return gh * gh + 1


def lane_tail(N: int) -> int:
    return N % 64


def stage_cases():
    """[(gh, B, H, dh)]: the full cross of the table."""
    return [(gh, B, H, dh) for gh in GRIDS for B in BATCHES for (H, dh) in HEADS]


def case_seed(gh: int, B: int, H: int) -> int:
    return 100 * gh + 10 * B + H


def softmax_map(gen, B: int, N: int, sharp: float = 3.0) -> torch.Tensor:
    return torch.softmax(sharp * torch.randn(B, N, N, generator=gen, dtype=torch.float64), -1)


def make_average_case(gh: int, B: int, H: int, dh: int):
    """qkv [B, N, 3D] f32 with q, k ~ 2 N(0, 1): logits of standard deviation 4, a softmax far from uniform; probs [B, H, N, N] f32 = the
    f64 softmax of the same logits rounded once (the parity-mode input)."""
    N, D = tokens_of(gh), H * dh
    gen = torch.Generator().manual_seed(11000 + case_seed(gh, B, H))
    qkv = 2.0 * torch.randn(B, N, 3 * D, generator=gen)
    q = qkv[..., :D].double().view(B, N, H, dh).permute(0, 2, 1, 3)
    k = qkv[..., D:2 * D].double().view(B, N, H, dh).permute(0, 2, 1, 3)
    probs = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), -1).float()
    return dict(qkv=qkv, probs=probs)


def make_enhance_case(gh: int, B: int, D: int, seed: int):
    """A [B, N, N]: rows (1 - p_i) softmax(off-diagonal logits) with p_i on the diagonal, p_i uniform in (0.02, 0.35) so that diagonals fall
    on both sides of the 0.15 threshold, p_0 = 0.05 (a boost of the CLS row would show), the last row scaled to a sum of FAINT (N > 2);
    tokens: decade rows."""
    N = tokens_of(gh)
    gen = torch.Generator().manual_seed(12000 + seed)
    logits = 3.0 * torch.randn(B, N, N, generator=gen, dtype=torch.float64)
    eye = torch.eye(N, dtype=torch.bool)[None]
    off = torch.softmax(logits.masked_fill(eye, float("-inf")), -1)
    p = 0.02 + 0.33 * torch.rand(B, N, generator=gen, dtype=torch.float64)
    p[:, 0] = 0.05
    A = off * (1 - p)[..., None] + torch.diag_embed(p)
    if N > 2:
        A[:, N - 1] *= FAINT
    return dict(A=A.float(), tokens=decade_rows(gen, B, N, D))


def make_fusion_case(gh: int, B: int, D: int, top_k: int, seed: int):
    """acc [B, N, N] f32: 0.5 A1 + 0.5 A2 of two softmax maps (the EMA of two blocks), reseeded deterministically until the first k + 1
    selection scores are RANK_GAP apart; the row of the first selected token of image 0 then keeps only its masked columns, so that it
    normalises to exactly 0 through the + 1e-8 (N > 2).  tokens: decade rows."""
    N = tokens_of(gh)
    n = N - 1
    k = min(top_k, n)
    for attempt in range(64):
        gen = torch.Generator().manual_seed(13000 + seed + 1000 * attempt)
        acc = (0.5 * softmax_map(gen, B, N) + 0.5 * softmax_map(gen, B, N, 1.0)).float()
        scores = selection_scores(acc[:, 0, :], torch.diagonal(acc, dim1=1, dim2=2), False)
        if rank_gap(scores, k) >= RANK_GAP:
            break
    else:
        raise AssertionError("no seed gives the rank gap")
    idx = selection_reference(scores, k)
    if N > 2:
        r = 1 + int(idx[0, 0])
        keep = torch.zeros(N, dtype=torch.bool)
        keep[idx[0] + 1] = True
        acc[0, r] = torch.where(keep, acc[0, r], torch.zeros(N))
    return dict(acc=acc, tokens=decade_rows(gen, B, N, D), emptied_row=(1 + int(idx[0, 0])) if N > 2 else None)


def make_similarity_case(n: int, D: int, seed: int, B: int = SIM_B):
    """x [B, n + 1, D + 8] f32 decade rows: the patch rows start one row in, rows D + 8 apart, images (n + 1)(D + 8) apart -- the tower's
    p.x + D with a padded row on top."""
    gen = torch.Generator().manual_seed(14000 + seed)
    return decade_rows(gen, B, n + 1, D + 8)
