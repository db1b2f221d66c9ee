"""f64 references and per-element error bounds for the token refiners (csrc/refine.hip: top-k selection, outlier suppression, weak-token
replacement, cross-tile fusion) and for Cluster-Then-Debias (csrc/ctd.hip); used by tests/test_gpu_refine_reference.py,
tests/test_gpu_ctd_reference.py and tests/test_refine_bound_cpu.py.

The values come from the oracle (oracle/refine.py, oracle/ctd.py) run on float64 copies of the f32 operands the kernels consume.  Every
bound is a tensor built term by term from the magnitudes of those operands, never from an observed output; each term is documented where
it is added.  Conventions as in gemm_reference: u = 2^-24, every f32 operation is charged 2u of the magnitude it rounds, a sum of n terms
2u n of the sum of the magnitudes.  ASSUMPTION (as attention_reference): expf and the reciprocal are within 2 ulp (EXPF).
Plain torch / numpy on the CPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from gemm_reference import U
from gemm_reference import check_within as _check_within
from attention_reference import EXPF
from oracle import refine as OR, ctd as OC

NEIGHBOURS = torch.tensor(OR.NEIGHBOUR_OFFSETS, dtype=torch.long)
UNTOUCHED, REPLACEMENT, CLEANED = 0, 1, 2
TINY = 2.0 ** -126                                  # absolute floor wherever an f32 intermediate may underflow


def f32(v: float) -> float:
    """The f32 value a float argument of the C ABI becomes."""
    return float(torch.tensor(v, dtype=torch.float32))


def check_within(got, ref, bound, what: str = "") -> float:
    """gemm_reference.check_within; the returned worst err / bound leaves out the elements whose bound is 0 (exact results, which the
    check itself holds to err = 0)."""
    _check_within(got, ref, bound, what)
    err = (got.double() - ref).abs()
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def lane_terms(D: int) -> int:
    """Roundings on the longest path of a 64-lane strided f32 dot product of length D: ceil(D/64) multiply-adds in the lane, six butterfly
    additions, one spare."""
    return (D + 63) // 64 + 7


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def selection_scores(a_cls, a_diag, weak: bool) -> torch.Tensor:
    """f64 scores of the n patch tokens from the f32 rows a_cls / a_diag [B, n + 1] (column 0 = CLS): A[cls,i] / (A[i,i] + 1e-8), or
    -A[i,i] for weak tokens; larger = selected first."""
    d = a_diag.double()[:, 1:]
    return -d if weak else a_cls.double()[:, 1:] / (d + 1e-8)


def selection_reference(scores: torch.Tensor, k: int) -> torch.Tensor:
    """First k indices of a STABLE descending sort: exact ties resolve to the lowest index (select_topk_kernel's rule)."""
    return torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :k]


def rank_gap(scores: torch.Tensor, k: int) -> float:
    """Smallest relative gap between consecutive scores among the first k + 1 of the descending order, exact ties ignored.  The f32
    score takes two roundings (1.2e-7 relative), so the kernel's order is the reference's wherever the gap is above 2.4e-7."""
    s = torch.sort(scores, dim=1, descending=True, stable=True).values[:, :k + 1]
    gap = (s[:, :-1] - s[:, 1:]) / torch.maximum(s[:, :-1].abs(), s[:, 1:].abs()).clamp_min(1e-300)
    gap = gap[gap > 0]
    return float(gap.min()) if gap.numel() else math.inf


# ---- outlier suppression / weak-token replacement ---------------------------------------------------------------------------------
def neighbour_cells(idx_b: torch.Tensor, gh: int, gw: int):
    """(rows, cols, target cells [k, 8]) of the clamped 8-neighbourhoods of the cells idx_b [k]."""
    rows, cols = torch.div(idx_b, gw, rounding_mode="trunc"), idx_b % gw
    ny = (rows[:, None] + NEIGHBOURS[None, :, 0]).clamp(0, gh - 1)
    nx = (cols[:, None] + NEIGHBOURS[None, :, 1]).clamp(0, gw - 1)
    return rows, cols, ny * gw + nx


def write_map(idx_b: torch.Tensor, tgt: torch.Tensor, n: int, decontaminate: bool):
    """Which write produced every cell: kind [n] (UNTOUCHED / REPLACEMENT / CLEANED) and the (outlier i, neighbour j) of it.  The
    reference's order: neighbour cells take the LAST (i, j) pair that targets them, pairs clamped onto their own outlier are skipped,
    outlier cells are written last."""
    kind = torch.zeros(n, dtype=torch.int8)
    wi = torch.full((n,), -1, dtype=torch.long)
    wj = torch.full((n,), -1, dtype=torch.long)
    cells = idx_b.tolist()
    if decontaminate:
        t = tgt.tolist()
        for i, cell in enumerate(cells):
            for j in range(8):
                if t[i][j] != cell:
                    kind[t[i][j]], wi[t[i][j]], wj[t[i][j]] = CLEANED, i, j
    for i, cell in enumerate(cells):
        kind[cell], wi[cell], wj[cell] = REPLACEMENT, i, -1
    return kind, wi, wj


def neighbour_refine_reference(feats, idx, gh: int, gw: int, temp: float, decontaminate: bool):
    """oracle.refine.suppress_outliers (decontaminate) / replace_weak_tokens on f64 copies of feats [B, n, D] (f32) with the selected
    cells idx [B, k]; temp is the f32 value the kernel receives.  Returns dict(out, bound [B, n, D] f64, kind, wi, wj [B, n]).

    Bound terms (refine_compute_kernel; c = the outlier's row, x_j its j-th neighbour, both read from the ORIGINAL map):
      * cosine: dot, |x|^2 and |c|^2 are 64-lane strided f32 sums, relative g = 2u lane_terms(D) of sum |x c| (of the squares: of
        themselves); two square roots (g/2 + 2u each), their product and the division (2u each):
        dcos = g sum|x c| / (|x||c|) + |cos| (g + 8u).  An all-zero row gives dot = 0 exactly and the 1e-12 clamp: dcos = 0.
      * softmax over the 8 values a_j = clamp(1 - cos_j, 0) (1-Lipschitz; the subtraction 2u, a_j - max <= 2 in magnitude 4u):
        d_j = dcos_j + 6u.  The common shift cancels, so log(w'_j / w_j) lies within d_j + M, M = log sum_l w_l exp(d_l) (Jensen below,
        the weighted exponential above).  On top, relative: expf (EXPF), the 8-term sum (16u), the division (2u).
      * replacement = sum_j x_j w_j, 8 multiply-adds: sum_j |x_j| (dw_j + 16u w'_j).
      * cleaned_j = x_j - c sigma_j, sigma = clamp(cos temp, 0, 1) (1-Lipschitz, the product 2u):
        |c| dsigma + 2u (|x| + 2 |c| (sigma + dsigma)), dsigma = |temp| dcos + 2u |cos temp|.
    """
    B, n, D = feats.shape
    x64 = feats.double()
    grid = x64.permute(0, 2, 1).reshape(B, D, gh, gw)
    idx = idx.long()
    out = (OR.suppress_outliers(grid, idx, temp) if decontaminate else OR.replace_weak_tokens(grid, idx)).reshape(B, D, n).permute(0, 2, 1)
    out = out.contiguous()
    bound = torch.zeros_like(out)
    mine = x64.clone()
    kinds, wis, wjs = [], [], []
    g = 2 * U * lane_terms(D)
    for b in range(B):
        _, _, tgt = neighbour_cells(idx[b], gh, gw)
        c = x64[b, idx[b]]                                            # [k, D]
        nb = x64[b, tgt]                                              # [k, 8, D]
        nn, cc = nb.norm(dim=2), c.norm(dim=1)[:, None]
        den = nn.clamp_min(1e-12) * cc.clamp_min(1e-12)
        cos = (nb * c[:, None]).sum(2) / den
        dcos = g * (nb.abs() * c.abs()[:, None]).sum(2) / den + cos.abs() * (g + 8 * U)
        a = (1.0 - cos).clamp(min=0.0)
        w = torch.softmax(a, 1)
        dj = dcos + 6 * U
        M = torch.log((w * torch.exp(dj)).sum(1, keepdim=True))
        rho = EXPF + 18 * U
        dw = w * (torch.expm1(dj + M) * (1 + rho) + rho)
        rep = (nb * w[:, :, None]).sum(1)
        brep = (nb.abs() * (dw + 16 * U * (w + dw))[:, :, None]).sum(1)
        sigma = (cos * temp).clamp(0, 1)
        dsig = abs(temp) * dcos + 2 * U * (cos * temp).abs()
        cleaned = nb - c[:, None] * sigma[:, :, None]
        bcl = c.abs()[:, None] * dsig[:, :, None] + 2 * U * (nb.abs() + 2 * c.abs()[:, None] * (sigma + dsig)[:, :, None])
        kind, wi, wj = write_map(idx[b], tgt, n, decontaminate)
        r = kind == REPLACEMENT
        mine[b, r], bound[b, r] = rep[wi[r]], brep[wi[r]]
        q = kind == CLEANED
        mine[b, q], bound[b, q] = cleaned[wi[q], wj[q]], bcl[wi[q], wj[q]]
        kinds.append(kind); wis.append(wi); wjs.append(wj)
    if not bool(((mine - out).abs() <= 1e-6 * bound).all()):          # f64 summation orders differ by ~1e-16 of the magnitudes
        raise AssertionError("the write map of refine_reference disagrees with the oracle")
    return dict(out=out, bound=bound, kind=torch.stack(kinds), wi=torch.stack(wis), wj=torch.stack(wjs))


# ---- cross-tile fusion -------------------------------------------------------------------------------------------------------------
def attention_fuse_bound(cur, nbr, s: float) -> torch.Tensor:
    """Bound of ctf_fuse_kernel, attention mode, on out = cur (1 - s) + softmax(cur . [cur; nbr]^T / sqrt C) [cur; nbr] s for the f64
    strips cur, nbr [S, C].
      * scores: a 64-lane strided dot (g = 2u lane_terms(C) of sum |x y|), sqrtf(C) and the division (4u of |dot|), all over sqrt C.
      * softmax over L2 = 2S: the shift cancels; with per-entry score errors d_j, log(w'_j / w_j) lies within d_j + M,
        M = log sum_l w_l exp(d_l), and 1 - w_j = sum_{l != j} w_l moves by at most sum_{l != j} w_l expm1(d_l + M): the smaller of the
        two.  Relative on top: expf (EXPF), the rounding of r_j - max (2u |r_j - max|, terms beyond 110 underflow to the TINY floor),
        the L2-term sum (2u L2 plus the weighted mean of the per-term errors), the division (2u).
      * aggregate over the 2S rows: sum_j dw_j |v_j| + 2u 2S sum_j w'_j |v_j|.
      * blend: 1 - s, two products and the sum, 6u (|x| (1 - s) + |agg| s)."""
    S, C = cur.shape
    both = torch.cat([cur, nbr], 0)
    L2 = 2 * S
    g = 2 * U * lane_terms(C)
    dot = cur @ both.T
    sc = dot / math.sqrt(C)
    d = (g * (cur.abs() @ both.abs().T) + 4 * U * dot.abs()) / math.sqrt(C)
    w = torch.softmax(sc, 1)
    M = torch.log((w * torch.exp(d.clamp(max=50.0))).sum(1, keepdim=True))
    e = torch.expm1((d + M).clamp(max=50.0))
    we = w * e
    other = we.sum(1, keepdim=True) - we
    rel = EXPF + 2 * U * (sc.max(1, keepdim=True).values - sc).clamp(max=110.0)
    rho = rel + (w * rel).sum(1, keepdim=True) + 2 * U * L2 + 2 * U
    dw = torch.minimum(we, other) * (1 + rho) + w * rho + TINY
    agg = w @ both
    dagg = dw @ both.abs() + 2 * U * L2 * ((w + dw) @ both.abs())
    return s * dagg + 6 * U * (cur.abs() * (1 - s) + (agg.abs() + dagg) * s)


def weighted_fuse_bound(cur, nbr, strength: float, eps: float) -> torch.Tensor:
    """Bound of ctf_fuse_kernel, weighted mode (oracle.refine.fuse_weighted), by first-order interval arithmetic through
      sim_ij = <x_i, y_j> / ((|x_i| + eps)(|y_j| + eps)): 64-lane strided dots, g = 2u lane_terms(C): g sum|x y| / den + |sim| (g + 8u);
      mean over L2 = S entries: mean(dsim) + 2u L2 mean|sim|;
      V = sum (sim - mean)^2: sum (2 |d| dd + dd^2) + 2u (L2 + 1) V with dd = dsim + dmean + 2u |d|;  var = V / (L2 - 1): + 2u var;
      std: |sqrt a - sqrt b| <= |a - b| / (sqrt a + sqrt b) and <= sqrt |a - b|, whichever is smaller (finite as std -> 0), + 2u std;
      thr = mean + std: dmean + dstd + 2u |thr|;  margin m_j = relu(sim_j - thr) (1-Lipschitz): dsim_j + dthr + 2u |sim_j - thr|;
      local = clamp(mean m, 0, 1): mean(dm) + 2u (L2 + 1) mean(m);  blend factor sf = strength local: strength dlocal + 2u sf;
      raw_j = m_j^2: 2 m dm + dm^2 + 2u raw;  wsum = sum raw + eps: sum draw + 2u L2 wsum;  w_j = raw_j / wsum:
        draw_j / lo + raw_j dwsum / (wsum lo) + 2u w_j with lo = max(wsum - dwsum, eps / 2);
      agg = sum_j w_j y_j: sum dw_j |y_j| + 2u S sum (w_j + dw_j) |y_j|;
      out = x (1 - sf) + agg sf: (|x| + |agg|) dsf + (sf + dsf) dagg + 6u (|x| + (|agg| + dagg)(sf + dsf))."""
    S, C = cur.shape
    L2 = S
    g = 2 * U * lane_terms(C)
    rc, rn = cur.norm(dim=1, keepdim=True) + eps, nbr.norm(dim=1, keepdim=True) + eps
    den = rc * rn.T
    sim = (cur @ nbr.T) / den
    dsim = g * (cur.abs() @ nbr.abs().T) / den + sim.abs() * (g + 8 * U)
    mean = sim.mean(1, keepdim=True)
    dmean = dsim.mean(1, keepdim=True) + 2 * U * L2 * sim.abs().mean(1, keepdim=True)
    dev = sim - mean
    ddev = dsim + dmean + 2 * U * dev.abs()
    V = (dev * dev).sum(1, keepdim=True)
    dV = (2 * dev.abs() * ddev + ddev * ddev).sum(1, keepdim=True) + 2 * U * (L2 + 1) * V
    var = V / (L2 - 1)
    dvar = dV / (L2 - 1) + 2 * U * var
    std = var.sqrt()
    dstd = torch.minimum(dvar / (std + (var - dvar).clamp(min=0).sqrt()).clamp_min(1e-300), dvar.sqrt()) + 2 * U * std
    thr = mean + std
    dthr = dmean + dstd + 2 * U * thr.abs()
    m = (sim - thr).clamp(min=0)
    dm = dsim + dthr + 2 * U * (sim - thr).abs()
    dm = torch.where((sim - thr) < -dm, torch.zeros_like(dm), dm)      # a margin that stays clamped at 0 whatever the error is exact
    local = m.mean(1, keepdim=True).clamp(0, 1)
    dlocal = dm.mean(1, keepdim=True) + 2 * U * (L2 + 1) * m.mean(1, keepdim=True)
    sf = strength * local
    dsf = strength * dlocal + 2 * U * sf
    raw = m * m
    draw = 2 * m * dm + dm * dm + 2 * U * raw
    wsum = raw.sum(1, keepdim=True) + eps
    dwsum = draw.sum(1, keepdim=True) + 2 * U * L2 * wsum
    lo = (wsum - dwsum).clamp(min=eps / 2)
    w = raw / wsum
    dw = draw / lo + raw * dwsum / (wsum * lo) + 2 * U * w
    agg = w @ nbr
    dagg = dw @ nbr.abs() + 2 * U * S * ((w + dw) @ nbr.abs())
    return (cur.abs() + agg.abs()) * dsf + (sf + dsf) * dagg + 6 * U * (cur.abs() + (agg.abs() + dagg) * (sf + dsf))


def cross_tile_reference(tokens, hg: int, wg: int, gh: int, gw: int, bw: int, mode: str, strength: float, final_left=None):
    """CrossTileFusionOracle's data flow in f64 for the scene tokens [hg*wg, gh*gw, C] (f32, tiles in raster order; strength = the f32
    value the kernel receives):  left = fuse(ORIGINAL left columns, ORIGINAL right columns of the left neighbour) -> columns [0, bw);
    top = fuse(ORIGINAL top rows, FINAL bottom rows of the upper neighbour) -> rows [0, bw); the left result wins the corner.
    Returns dict(out, bound [T, n, C] f64, strip [T, n] bool).

    The top pass consumes a RESULT of the left pass (columns [0, bw) of the neighbour's bottom rows).  `final_left` [T, n, C], the
    output under test, supplies those values as the operands the top pass actually consumed (they are themselves held to the left
    pass's bound), so that the top bound needs no propagation through the fusion; without it the f64 left results are used and the
    returned values are exactly the oracle's."""
    T, n, C = tokens.shape
    x = tokens.double().view(T, gh, gw, C)
    eps = f32(1e-6)
    if mode == "attention":
        fuse = lambda c, nb: (OR.fuse_attention(c[None], nb[None], strength)[0], attention_fuse_bound(c, nb, strength))   # noqa: E731
    else:
        fuse = lambda c, nb: (OR.fuse_weighted(c[None], nb[None], strength, eps)[0], weighted_fuse_bound(c, nb, strength, eps))  # noqa: E731
    out, bound = x.clone(), torch.zeros_like(x)
    strip = torch.zeros(T, gh, gw, dtype=torch.bool)
    left = {}
    for t in range(T):
        if t % wg > 0:
            left[t] = fuse(x[t][:, :bw].reshape(-1, C), x[t - 1][:, gw - bw:].reshape(-1, C))
    fl = None if final_left is None else final_left.double().view(T, gh, gw, C)
    for t in range(T):
        if t // wg > 0:
            up = t - wg
            bottom = x[up][gh - bw:].clone()                                                  # [bw, gw, C]
            if up % wg > 0:
                bottom[:, :bw] = fl[up][gh - bw:, :bw] if fl is not None else left[up][0].view(gh, bw, C)[gh - bw:]
            v, bd = fuse(x[t][:bw].reshape(-1, C), bottom.reshape(-1, C))
            out[t][:bw], bound[t][:bw], strip[t][:bw] = v.view(bw, gw, C), bd.view(bw, gw, C), True
        if t in left:
            out[t][:, :bw], bound[t][:, :bw], strip[t][:, :bw] = left[t][0].view(gh, bw, C), left[t][1].view(gh, bw, C), True
    return dict(out=out.view(T, n, C), bound=bound.view(T, n, C), strip=strip.view(T, n))


# ---- Cluster-Then-Debias -----------------------------------------------------------------------------------------------------------
def debias_reference(x, cls, labels, factor: float):
    """oracle.ctd.adaptive_debiasing in f64 for tokens x [B, n, C], CLS rows cls [B, C] (f32) and labels [B, n], with the bound of
    ctd_proto_sim_kernel / ctd_apply_kernel per element:
      * prototype = (index-order f32 sum over the cnt members) / cnt: 2u cnt mean|x| + 2u |proto|;
      * |proto| + 1.1 and |cls| + 1.1: a 256-thread block sum of squares (g = 2u (ceil(C/256) + 10) of itself, halved by the root),
        the root and the addition: ||dproto||_2 + |proto| (g/2 + 2u) + 2u np;  |cls| (g/2 + 2u) + 2u nc;
      * sim = clamp(sum_c (proto_c / np)(cls_c / nc), -1, 1) (1-Lipschitz): sum_c dproto_c |cls_c| / (np nc)
        + sum_c |proto_c cls_c| / (np nc) (dnp / np + dnc / nc + 6u + g);
      * x + sim (factor cls): |factor cls| dsim + 4u |sim factor cls| + 2u (|x| + |sim factor cls|).
    Rows labelled -1 are untouched (bound 0)."""
    B, n, C = x.shape
    x64, c64 = x.double(), cls.double()
    out, bound = x64.clone(), torch.zeros_like(x64)
    g = 2 * U * ((C + 255) // 256 + 10)
    for b in range(B):
        lab = labels[b].long()
        K = int(lab.max()) + 1
        if K <= 0:
            continue
        valid = lab >= 0
        ids = lab[valid]
        cnt = torch.zeros(K, dtype=torch.float64).index_add_(0, ids, torch.ones(ids.shape[0], dtype=torch.float64)).clamp_min(1.0)[:, None]
        proto = torch.zeros(K, C, dtype=torch.float64).index_add_(0, ids, x64[b, valid]) / cnt
        amean = torch.zeros(K, C, dtype=torch.float64).index_add_(0, ids, x64[b, valid].abs()) / cnt
        dproto = 2 * U * cnt * amean + 2 * U * proto.abs()
        pn, cn = proto.norm(dim=1, keepdim=True), c64[b].norm()
        np_, nc_ = pn + 1.1, cn + 1.1
        dnp = dproto.norm(dim=1, keepdim=True) + pn * (g / 2 + 2 * U) + 2 * U * np_
        dnc = cn * (g / 2 + 2 * U) + 2 * U * nc_
        sim = ((proto / np_) * (c64[b] / nc_)[None]).sum(1, keepdim=True).clamp(-1.0, 1.0)
        dsim = (dproto * c64[b].abs()[None]).sum(1, keepdim=True) / (np_ * nc_) \
            + (proto.abs() * c64[b].abs()[None]).sum(1, keepdim=True) / (np_ * nc_) * (dnp / np_ + dnc / nc_ + 6 * U + g)
        fc = (factor * c64[b])[None]                                                          # [1, C]
        add = sim[ids] * fc
        out[b, valid] = x64[b, valid] + add
        bound[b, valid] = fc.abs() * dsim[ids] + 4 * U * add.abs() + 2 * U * (x64[b, valid].abs() + add.abs())
    return out, bound


def ctd_reference(x, cls, eps: float, min_samples: int, factor: float):
    """Cluster-Then-Debias of tokens x [B, n, C] (f32) in f64: labels from oracle.ctd.dbscan_labels on the oracle's f32 points, the
    debiased tokens and their bound (`debias_reference`), and radius_margin = min |d^2 - eps^2| over all pairs of a tile
    (oracle.ctd.neighbour_matrix on the f32 points): how far the f32 rounding of the points may move a pair before a label can change."""
    pts = OC.ctd_points(x)
    labels, margin = [], math.inf
    for b in range(x.shape[0]):
        p = pts[b].numpy()
        labels.append(torch.from_numpy(OC.dbscan_labels(p, eps, min_samples)))
        margin = min(margin, float(np.abs(OC.neighbour_matrix(p, eps)[1] - float(eps) ** 2).min()))
    labels = torch.stack(labels)
    out, bound = debias_reference(x, cls, labels, factor)
    return dict(labels=labels, out=out, bound=bound, radius_margin=margin)


# ---- case generators (shared by the GPU modules and tests/test_refine_bound_cpu.py) ------------------------------------------------
RANK_GAP = 2.0 ** -20                               # 4x the 2.4e-7 by which two f32 scores can close up
RADIUS_MARGIN = 2e-6
REFINE_CASES = [(3, 5, 9, 20, 12), (2, 9, 5, 72, 40), (1, 20, 20, 328, 300), (2, 1, 7, 8, 3), (2, 7, 1, 8, 3), (1, 37, 37, 64, 30)]
CONTESTED_GRID = (20, 20)                           # the one refiner case in which no cell need stay untouched
FUSION_CASES = [(2, 3, 6, 10, 1, 8), (3, 2, 10, 6, 3, 40), (1, 4, 9, 7, 2, 200), (4, 1, 7, 9, 2, 72), (2, 2, 64, 64, 2, 8), (1, 1, 8, 8, 2, 16)]


def decade_rows(gen, *shape) -> torch.Tensor:
    """N(0, 1) rows scaled by exp(2 N(0, 1)): magnitudes from about 1e-2 to 1e2, as real last-block tokens."""
    return (torch.randn(*shape, generator=gen) * torch.exp(2 * torch.randn(*shape[:-1], 1, generator=gen))).float()


def make_refine_case(B: int, gh: int, gw: int, D: int, k: int, weak: bool, seed: int = 0):
    """Attention rows whose first k + 1 scores are at least RANK_GAP apart (reseeded deterministically until they are), decade rows,
    one all-zero token beside the first selected cell, and -- except on the contested grid -- a corner block that is never selected,
    so that its corner cell stays untouched.  Returns dict(feats, a_cls, a_diag [B, n + 1], idx [B, k])."""
    n = gh * gw
    cells = torch.arange(n)
    block = ((cells // gw >= gh - 2) & (cells % gw >= gw - 2)) if (gh, gw) != CONTESTED_GRID else torch.zeros(n, dtype=torch.bool)
    assert n - int(block.sum()) >= k
    for attempt in range(64):
        gen = torch.Generator().manual_seed(seed + 1000 * attempt)
        a_cls = (torch.rand(B, n + 1, generator=gen) * 0.9 + 0.1).float()
        a_diag = (torch.rand(B, n + 1, generator=gen) * 0.9 + 0.1).float()
        if weak:
            a_diag[:, 1:][:, block] += 2.0
        else:
            a_cls[:, 1:][:, block] *= 1e-3
        scores = selection_scores(a_cls, a_diag, weak)
        if rank_gap(scores, k) >= RANK_GAP:
            break
    else:
        raise AssertionError("no seed gives the rank gap")
    idx = selection_reference(scores, k)
    feats = decade_rows(gen, B, n, D)
    _, _, tgt = neighbour_cells(idx[0, :1], gh, gw)
    zero = [t for t in tgt[0].tolist() if t != int(idx[0, 0])]
    if zero:
        feats[0, zero[0]] = 0.0                      # reaches the 1e-12 clamp of the normalisation
    return dict(feats=feats, a_cls=a_cls, a_diag=a_diag, idx=idx)


def make_tie_case(weak: bool, seed: int = 0):
    """(1, 5, 9, 20, 12) with four exactly equal scores on ranks 10..13, straddling k = 12: the two lowest indices of the four are
    selected, lowest first."""
    B, gh, gw, D, k = 1, 5, 9, 20, 12
    case = make_refine_case(B, gh, gw, D, k, weak, seed)
    scores = selection_scores(case["a_cls"], case["a_diag"], weak)
    order = torch.sort(scores[0], descending=True, stable=True).indices.tolist()
    holder, spare = order[k - 2], sorted(order[k + 4:k + 7])
    for t in spare:
        case["a_cls"][0, 1 + t], case["a_diag"][0, 1 + t] = case["a_cls"][0, 1 + holder], case["a_diag"][0, 1 + holder]
    scores = selection_scores(case["a_cls"], case["a_diag"], weak)
    assert rank_gap(scores, k + 2) >= RANK_GAP and int((scores[0] == scores[0, holder]).sum()) == 4
    case["idx"] = selection_reference(scores, k)
    case["tied"] = sorted(spare + [holder])
    case["shape"] = (B, gh, gw, D, k)
    return case


def make_fusion_case(hg: int, wg: int, gh: int, gw: int, C: int, seed: int = 0) -> torch.Tensor:
    return decade_rows(torch.Generator().manual_seed(seed), hg * wg, gh * gw, C)


def arc_tokens(theta, C: int, g, plane=None) -> np.ndarray:
    """Rows (cos t, sin t) in the channel pair `plane` (default 0), scaled by factors in [0.5, 3] that the normalisation removes."""
    theta = np.asarray(theta, np.float64)
    x = np.zeros((theta.shape[0], C), np.float64)
    pl = np.zeros(theta.shape[0], np.int64) if plane is None else np.asarray(plane)
    x[np.arange(theta.shape[0]), 2 * pl] = np.cos(theta)
    x[np.arange(theta.shape[0]), 2 * pl + 1] = np.sin(theta)
    return (x.astype(np.float32) * g.uniform(0.5, 3.0, (theta.shape[0], 1)).astype(np.float32))


def make_chain(n: int, seed: int = 0, C: int = 8):
    """n points 6/n rad apart, shuffled; eps = 1.6 spacings, min_samples 3: one cluster, the two ends border points."""
    g = np.random.default_rng(seed)
    perm = g.permutation(n)
    x = arc_tokens(perm * (6.0 / n), C, g)
    return dict(x=torch.from_numpy(x)[None], eps=1.6 * 6.0 / n, min_samples=3, ends=[int(np.argmin(perm)), int(np.argmax(perm))])


CONTESTED_EPS, CONTESTED_MS = 0.05, 11


def make_contested(seed: int = 0, C: int = 8):
    """Three tiles of 25 points at eps 0.05 / min_samples 11.
    Tile 0, the contested border: blobX (10 points within 1e-3 of angle 0), tX = 0.9 eps, z = 1.8 eps, tY = 2.7 eps, blobY (10 points at
    3.6 eps); order: one blobY point, tX, blobX, z, the rest of blobY, two noise points, tY.  Y holds index 0, so Y = cluster 0, X = 1;
    z is not core (neighbours tX, tY, itself) and takes 0, although its lowest-index core neighbour tX belongs to cluster 1.
    Tile 1: all noise (25 points 2 eps apart).
    Tile 2, numbering: e = 1.8 eps (border of P through the hub tP = 0.9 eps only) at index 0, the 11 points of blob Q (angle 1), then
    blobP (10 points at angle 0), two noise points, tP.  Q has the smallest core index: Q = 0, P = 1 and e takes 1; numbering clusters by
    their first member of any kind would give P = 0."""
    g = np.random.default_rng(seed)
    e = CONTESTED_EPS
    blob = lambda c, m: c + g.uniform(-1e-3, 1e-3, m)   # noqa: E731
    bx, by = blob(0.0, 10), blob(3.6 * e, 10)
    t0 = np.concatenate([by[:1], [0.9 * e], bx, [1.8 * e], by[1:], [2.0, 2.5], [2.7 * e]])
    t1 = 2 * e * np.arange(25)
    t2 = np.concatenate([[1.8 * e], blob(1.0, 11), blob(0.0, 10), [2.0, 2.5], [0.9 * e]])
    x = np.stack([arc_tokens(t, C, g) for t in (t0, t1, t2)])
    return dict(x=torch.from_numpy(x), eps=e, min_samples=CONTESTED_MS, z=12, tX=1, e=0)


def make_near_radius(seed: int = 0, C: int = 32, eps: float = 1.1, pairs: int = 16):
    """One plane per pair (points of different planes are sqrt 2 apart): a_k at angle 0 with nine blob points 2e-4..1e-3 rad on the far
    side (10 neighbours with itself), b_k at d^2 = eps^2 + s_k delta_k, delta geometric over [4e-6, 5e-5], s alternating.  a_k is core
    (min_samples 11), and its plane a cluster, exactly when b_k is inside the radius; otherwise the whole plane is noise.  Shuffled.
    Reseeded until the oracle's radius_margin on the f32 points is at least RADIUS_MARGIN."""
    assert 2 * pairs <= C
    delta = np.geomspace(4e-6, 5e-5, pairs)
    sign = np.where(np.arange(pairs) % 2 == 0, -1.0, 1.0)
    for attempt in range(64):
        g = np.random.default_rng(seed + 1000 * attempt)
        th, pl = [], []
        for k in range(pairs):
            th += [0.0, math.acos(1.0 - (eps * eps + sign[k] * delta[k]) / 2.0)] + list(-g.uniform(2e-4, 1e-3, 9))
            pl += [k] * 11
        perm = g.permutation(len(th))
        x = torch.from_numpy(arc_tokens(np.asarray(th)[perm], C, g, np.asarray(pl)[perm]))[None]
        _, d2 = OC.neighbour_matrix(OC.ctd_points(x)[0].numpy(), eps)
        if float(np.abs(d2 - eps * eps).min()) >= RADIUS_MARGIN:
            inside = [int(np.nonzero(perm == 11 * k)[0][0]) for k in range(pairs) if sign[k] < 0]
            outside = [int(np.nonzero(perm == 11 * k)[0][0]) for k in range(pairs) if sign[k] > 0]
            return dict(x=x, eps=eps, min_samples=11, inside=inside, outside=outside)
    raise AssertionError("no seed gives the radius margin")


def make_blobs(n: int, C: int, eps: float, seed: int = 0):
    """oracle.ctd.make_clustered_tokens, reseeded until radius_margin >= RADIUS_MARGIN."""
    for attempt in range(256):
        x = torch.from_numpy(OC.make_clustered_tokens(1, n, C, seed=seed + 1000 * attempt))
        _, d2 = OC.neighbour_matrix(OC.ctd_points(x)[0].numpy(), eps)
        if float(np.abs(d2 - eps * eps).min()) >= RADIUS_MARGIN:
            return x
    raise AssertionError("no seed gives the radius margin")
