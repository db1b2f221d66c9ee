"""f64 references and per-element error bounds for the fused attention kernels (used by tests/test_gpu_attention_reference.py and
tests/test_attention_bound_cpu.py), plus the case generators both modules share.

Everything is plain torch in float64 on whatever device the inputs live on.  The reference runs on the operands exactly as the kernel
consumes them (decoded bf16 / f16 storage, hi + lo of two-plane storage) and on the f32 scale, bias, bias_rn / bias_cn, scale_per_image and
lse_in the kernel was given.  Every bound is built from operand magnitudes, never from observed outputs; `attention_bound` derives each term.

Operand layout of this module: Q[t], K[t], V as [B, N, H, dh]; bias [Bb, N-1, N-1] (Bb = 1 when shared) read as bias[key-1][query-1], as the
kernel does (the map is symmetric in the library); bias_rn / bias_cn / lse_in [B, H, N]; scale [B] (the f32 per-image scale, or `scale`
broadcast).
"""
from __future__ import annotations

import math

import torch

from gemm_reference import H2_REL, U, h2_delta, half_ulp

LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))    # the kernel's constants, as f32
LN2_F32 = float(torch.tensor(0.6931471805599453, dtype=torch.float32))
LOG2E = 1.0 / math.log(2.0)
KT = 64                                            # keys per tile
TAU = 8.0                                          # lazy rescale threshold, log2 units
HW1 = 2.0 ** -23                                   # hardware exp2 / rcp: 1 ulp (the constant gemm_reference uses)
LOG_ABS = 2.0 ** -22                               # ASSUMPTION: hardware log2 within 2^-22 absolute + 1 ulp relative of its result
EXPF = 2.0 ** -22                                  # ASSUMPTION: device expf within 2 ulp
# operand / probability formats: relative half-ulp rho and absolute (subnormal) floor a of a round-to-nearest conversion
RHO = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "h2": H2_REL}
FLOOR = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25, "h2": 2.0 ** -25}
F16_MAX = 65504.0


def c2_of(scale: torch.Tensor) -> torch.Tensor:
    """The kernel's c2 = f32(scale) * f32(LOG2E) in f32 (one round-to-nearest multiply), as f64."""
    return (scale.float() * torch.tensor(LOG2E_F32, dtype=torch.float32, device=scale.device)).double()


def exact_c2_scale(k: int) -> float:
    """An f32 scale near 2^k ln 2 whose kernel c2 = f32(scale) * f32(LOG2E) is exactly 2^k (searched over f32 neighbours)."""
    s = torch.tensor(2.0 ** k * math.log(2.0), dtype=torch.float32)
    cand = [s]
    up, dn = s.clone(), s.clone()
    for _ in range(16):
        up = torch.nextafter(up, torch.tensor(float("inf")))
        dn = torch.nextafter(dn, torch.tensor(0.0))
        cand += [up, dn]
    for c in cand:
        if float(c2_of(c.view(1))[0]) == 2.0 ** k:
            return float(c)
    raise AssertionError(f"no f32 scale gives c2 = 2^{k}")


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _bias_full(bias, bias_w, bias_rn, bias_cn, B, H, N):
    """[B, H, N(query), N(key)] f64 additive term: bias_w bias[key-1][query-1] (rn[query] cn[key]); 0 in row / column 0."""
    if bias is None:
        return None
    n = N - 1
    bt = bias.double().reshape(-1, n, n).transpose(-1, -2)                   # [Bb, query-1, key-1]
    full = torch.zeros(bt.shape[0], N, N, dtype=torch.float64, device=bias.device)
    full[:, 1:, 1:] = bt
    full = full.expand(B, N, N)[:, None] * float(bias_w)
    if bias_cn is not None:
        full = full * bias_rn.double()[..., :, None] * bias_cn.double()[..., None, :]
    return full.expand(B, H, N, N)


def attention_reference(Q, K, V, *, scale, sum_scores, causal=False, bias=None, bias_w=0.0, bias_rn=None, bias_cn=None,
                        resoftmax=False, lse_in=None, out_scale=1.0):
    """The operation in float64.  Returns a dict: ctx [B,N,H,dh], lse [B,H,N] (of the last stream), and per stream the f64 scores z
    (ln units, masked = -inf), weights w, the raw product magnitude S = sum_t |q_t|.|k_t| and the resoftmax inner term r (for the bound)."""
    B, N, H, dh = V.shape
    sc = scale.double().view(B, 1, 1, 1)
    terms = list(range(len(Q)))
    groups = [terms] if sum_scores else [[t] for t in terms]
    bf = _bias_full(bias, bias_w, bias_rn, bias_cn, B, H, N)
    mask = None
    if causal:
        mask = torch.ones(N, N, dtype=torch.bool, device=V.device).triu(1)   # key > query
    Vd = V.double().permute(0, 2, 1, 3)                                    # [B,H,N,dh]
    streams, ctx = [], 0.0
    for g in groups:
        raw = sum(torch.matmul(Q[t].double().permute(0, 2, 1, 3), K[t].double().permute(0, 2, 3, 1)) for t in g) * sc
        S = sum(torch.matmul(Q[t].double().abs().permute(0, 2, 1, 3), K[t].double().abs().permute(0, 2, 3, 1)) for t in g)
        r = None
        z = raw
        if resoftmax:
            r = torch.exp(raw - lse_in.double()[..., None])
            z = r
        if bf is not None:
            z = z + bf
        if mask is not None:
            z = z.masked_fill(mask, float("-inf"))
        lse = torch.logsumexp(z, dim=-1)
        w = torch.exp(z - lse[..., None])
        ctx = ctx + torch.matmul(w, Vd)
        streams.append(dict(z=z, w=w, S=S, r=r, lse=lse, terms=g))
    ctx = (ctx * float(out_scale)).permute(0, 2, 1, 3)
    return dict(ctx=ctx, lse=streams[-1]["lse"], streams=streams, B=B, N=N, H=H, dh=dh, scale=scale, bf=bf, Q=Q, K=K, V=V,
                sum_scores=sum_scores, out_scale=float(out_scale), lse_in=lse_in, mask=mask)


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
def attention_bound(ref, *, fmt: str, lean: bool, c2_exact: bool = False, lse_in_err=None):
    """Per-element bounds (ctx [B,N,H,dh], lse [B,H,N]) on |kernel - reference| for the fused attention (attention.hip).

    fmt: operand storage 'bf16' / 'f16' / 'h2'; lean: the lean path (nothing added to the scores: Q pre-multiplied by c2 and re-rounded,
    score accumulator started at -m_run) or the generic one.  c2_exact: c2 = f32(scale) f32(LOG2E) is a power of two, so the lean path's
    re-rounding of c2 q to bf16 / f16 is exact (f16 keeps its subnormal floor).  lse_in_err: a bound on |lse_in - true log-sum-exp| when the
    kernel is fed another kernel's LSE (the composed 'Experimental'), added to the re-softmax argument.

    Notation, per (image, head, query i, stream): x_ij = log2(e) z_ij the score in log2 units; S_ij = sum |q||k| over the stream's terms and
    dh; Xr_ij = c2 S_ij; n = TS dh products per score (3 TS dh in two-plane: hi.hi + lo.hi + hi.lo; their magnitudes sum to <= 1.01 S since
    |hi| <= |x| (1 + 2^-11), |lo| <= 2^-11 |x|); u = 2^-24.

    Score error E_ij (log2 units, absolute, of the exponent argument the kernel feeds exp2 relative to the running maximum):
    * c2: the kernel's c2 misses scale log2(e) by a relative theta computed exactly from the f32 values: theta Xr.
    * accumulation: every MFMA product of two operand values is exact in f32 and every addition a faithful rounding (as gemm_bound), so
      2u (n + 1) times the largest partial sum.  Lean: the accumulator starts at -m_run, so partial sums are <= Mrow + S'_ij with
      S' = sum |q'||k| <= (1 + rho_q + 2u) Xr + a_q sum|k|.  Generic: <= S (times c2 after the f32 product, one more rounding u |v|).
      Two-plane omits lo.lo: <= 2^-22 1.01 S (times c2).
    * lean Q rounding: q' = fmt(f32(c2 q)) misses c2 q by rho_q (1 + u) |c2 q| + u |c2 q| + a_q (bf16 2^-8, f16 2^-11 + the subnormal
      floor 2^-25; two-plane: (hi + lo) c2 is two f32 roundings, then the split, h2_delta); summed against |k|: qerr . |K|^T.  With an
      exact power-of-two c2 the bf16 / f16 re-rounding is exact apart from the f16 subnormal floor.
    * generic bias: bias * (cn * rn) two roundings, * bias_w one, * LOG2E (rounded constant + product) two, the add one: 6u |b| log2e +
      u |v|.  Re-softmax: lse_in * LOG2E two roundings, the subtraction one, exp2 1 ulp: the inner term r carries a relative error
      e^{ln2 e_a} (1 + 2^-23) - 1 for an argument error e_a; then (r + b) * LOG2E adds 3u of |v|.
    * the exponent argument: generic sc - m_run one rounding u (|x| + |m|) <= 2u Mrow; lean sacc -= delta at a rescale, the same.
    Mrow bounds |x~_ij| over the row and |m_run| (m_run only ever takes a seen row maximum): 1.01 (magnitude of x incl. bias / r) + the
    absolute floors; 1.01 covers every relative perturbation above (all < 2^-8 + 2^-10).

    Score error in ln units Delta_i = max_j [ ln2 E_ij ] + 2^-23 (exp2, relative) + R eta, with R = ceil(N/64) rescales at most (a rescale
    per key tile), each scaling o_acc and l_run by the SAME rounded alpha -- alpha's own error (exp2 1 ulp, argument rounding ln2 u 2 Mrow,
    the lean path's m_run + delta rounding) shifts the earlier keys against the later ones, and the two products round once each:
    eta = 2^-23 + ln2 u 2 Mrow + 2u.  Per-key errors of at most Delta change every normalised weight by a factor within e^{+-2 Delta}.

    Context of one stream, with W = sum_j w_ij |v_jd| (f64 weights) and G = e^{2 Delta} W:
        err <= (e^{2 Delta} - 1) W + gamma G + 1.01 a_P sum_j |v_jd|,
    gamma = (1 + rho_P)(1 + 2u n_pv [1.01])(1 + eps_l)/(1 - eps_l)(1 + 2^-23)(1 + u)(1 + [2^-22 1.01]) - 1:
    * P conversion: relative rho_P (bf16 2^-8, f16 2^-11, two-plane 2^-22) and absolute a_P (f16 / two-plane 2^-25).  INVARIANT: m_run is
      always a seen row maximum, so the key that set it has P = exp2(0) = 1 and every later rescale keeps l_run >= 1; and P <= 2^8
      (TAU).  The numerator uses rounded P, the denominator unrounded p: an absolute floor on P is then at most a_P |v| per key after the
      division by l >= 1.
    * PV: f32 accumulation over n_pv = 64 ceil(N/64) keys (masked keys carry P = 0; three times that, magnitudes 1.01, two-plane), and the
      omitted V_lo.P_lo (2^-22 1.01).
    * l_run: f32 sum of non-negative terms, each through <= 32 + ceil(N/64) roundings: eps_l = 1.01 u (32 + ceil(N/64)).
    * 1 / l_run: rcp 1 ulp (2^-23), o * inv one rounding.
    Streams and output: the o_tot sum adds 2u per stream of the magnitude A = sum_s G_s (1 + gamma_s) + a_P sum |v| (multi-stream only);
    out_scale one rounding u A; then the store: half an ulp of bf16 / f16 at |ref| + bound (subnormal floor), h2_delta for two-plane, and
    f16 saturation at 65504 (what lies beyond is the clamp's error).

    LSE (of the last stream; lse = ln2 (m + log2 l)): Delta (a shift of every score by <= Delta moves the log-sum-exp by <= Delta), l's
    relative eps_l (ln(1 + e) <= e / (1 - e)), the hardware log2 (ASSUMPTION, LOG_ABS absolute + 2^-23 relative of log2 l <= 9 + log2 N:
    l <= N 2^8), the add u (Mrow + 9 + log2 N) and the f32 LN2 (constant + product: 2u) of the result, all times ln2 where in log2 units.
    """
    B, N, H, dh = ref["B"], ref["N"], ref["H"], ref["dh"]
    dev = ref["V"].device
    two = fmt == "h2"
    scale = ref["scale"].double().view(B, 1, 1, 1).abs()
    c2 = c2_of(ref["scale"]).view(B, 1, 1, 1)
    c2t = scale * LOG2E
    theta = ((c2 - c2t).abs() / c2t)
    ntiles = (N + KT - 1) // KT
    R = ntiles
    eps_l = 1.01 * U * (32 + ntiles)
    rho_p, a_p = RHO[fmt], FLOOR[fmt]
    Vd = ref["V"].double().permute(0, 2, 1, 3).abs()                        # [B,H,N,dh]
    mask = ref["mask"]
    Vsum = Vd.sum(dim=2, keepdim=True)                                        # [B,H,1,dh] over all keys (an upper bound for masked rows)
    if mask is not None:
        Vsum = torch.matmul((~mask).double(), Vd)                             # [B,H,N,dh] unmasked keys only
    per_stream, A_tot, lse_b = [], 0.0, None
    for st in ref["streams"]:
        g = st["terms"]
        TS = len(g)
        S = st["S"]
        n_add = (3 if two else 1) * TS * dh + 1
        kabs = sum(ref["K"][t].double().abs().permute(0, 2, 3, 1) for t in g)   # [B,H,dh,N]
        Xr = c2t * S
        if lean:
            rho_q = RHO[fmt]
            if two:
                qerr = [h2_delta(c2t * 1.0001 * ref["Q"][t].double().abs()) + 3 * U * c2t * ref["Q"][t].double().abs() for t in g]
            elif c2_exact:
                qerr = [torch.full_like(ref["Q"][t].double(), FLOOR[fmt]) for t in g]
            else:
                qerr = [(rho_q * (1 + U) + U) * c2t * ref["Q"][t].double().abs() + FLOOR[fmt] for t in g]
            Eq = sum(torch.matmul(qerr[i].permute(0, 2, 1, 3), ref["K"][t].double().abs().permute(0, 2, 3, 1)) for i, t in enumerate(g))
            Sp = (1 + 2.0 ** -8 + 2 * U) * Xr + Eq
            mag = Xr + Eq
        else:
            mag = Xr.clone()
            if st["r"] is not None:
                mag = st["r"] * LOG2E
            if ref["bf"] is not None:
                mag = mag + ref["bf"].abs() * LOG2E
        if mask is not None:
            mag = mag.masked_fill(mask, 0.0)
        Mrow = 1.01 * mag.amax(dim=-1, keepdim=True) + 2.0 ** -30
        lo_lo = 1.01 * H2_REL * Xr if two else 0.0
        if lean:
            E = theta * Xr + 2 * U * n_add * (Mrow + Sp) * (1.01 if two else 1.0) + lo_lo + Eq + 2 * U * Mrow
        else:
            E_raw = theta * Xr + 2 * U * n_add * Xr * (1.01 if two else 1.0) + lo_lo + 1.02 * U * Xr
            if st["r"] is not None:
                lse2 = ref["lse_in"].double().abs()[..., None] * LOG2E
                e_a = E_raw + 2 * U * lse2 * 1.01 + U * (1.01 * Xr + 1.01 * lse2)
                if lse_in_err is not None:
                    e_a = e_a + lse_in_err.double()[..., None] * LOG2E
                rerr = st["r"] * (torch.expm1(math.log(2.0) * e_a) * (1 + HW1) + HW1)
                E = LOG2E * rerr
                if ref["bf"] is not None:
                    E = E + 4 * U * ref["bf"].abs() * LOG2E * 1.01
                E = E + 3 * U * 1.01 * mag
            else:
                E = E_raw
                if ref["bf"] is not None:
                    E = E + 6 * U * ref["bf"].abs() * LOG2E * 1.01 + U * 1.01 * mag
            E = E + 2 * U * Mrow
        if mask is not None:
            E = E.masked_fill(mask, 0.0)
        eta = HW1 + math.log(2.0) * U * 2 * Mrow + 2 * U
        Delta = math.log(2.0) * E.amax(dim=-1, keepdim=True) + HW1 + R * eta         # [B,H,N,1]
        W = torch.matmul(st["w"], Vd)                                               # [B,H,N,dh]
        grow = torch.exp(2 * Delta)
        n_pv = KT * ntiles * (3 if two else 1)
        gamma = ((1 + rho_p) * (1 + 2 * U * n_pv * (1.01 if two else 1.0)) * (1 + eps_l) / (1 - eps_l) * (1 + HW1) * (1 + U)
                 * (1 + (1.01 * H2_REL if two else 0.0)) - 1)
        G = grow * W
        err = (grow - 1) * W + gamma * G + 1.01 * a_p * Vsum
        per_stream.append(err)
        A_tot = A_tot + G * (1 + gamma) + a_p * Vsum
        # LSE of this stream (the kernel writes the last one's)
        lmax = 9 + math.log2(N)
        lse_b = (Delta[..., 0] + eps_l / (1 - eps_l) * 1.01
                 + math.log(2.0) * (LOG_ABS + HW1 * lmax + U * (Mrow[..., 0] + lmax)) + 2 * U * math.log(2.0) * 1.01 * (Mrow[..., 0] + lmax))
    multi = not ref["sum_scores"] and len(ref["streams"]) > 1
    os_ = abs(ref["out_scale"])
    total = sum(per_stream)
    if multi:
        total = total + 2 * U * len(per_stream) * A_tot
    bval = os_ * total + U * os_ * A_tot * 1.01
    bval = bval.permute(0, 2, 1, 3)
    mag = ref["ctx"].abs() + bval
    if two:
        bout = h2_delta(mag)
    else:
        bout = half_ulp(mag, fmt)
    if fmt != "bf16":
        bout = bout + (mag - F16_MAX).clamp(min=0)
    return dict(ctx=bval + bout, lse=lse_b)


# ---- head-averaged statistics ------------------------------------------------------------------------------------------------------
def stats_reference(Q, K, lse, scale):
    """a_cls [B,N] = mean_h exp(scale q_0.k_j - lse[b,h,0]), a_diag [B,N] = mean_h exp(scale q_j.k_j - lse[b,h,j]) in f64, with the
    per-head arguments' magnitudes for the bound.  Q, K [B,N,H,dh]; lse [B,H,N] f32 as given to the kernel."""
    Qd, Kd, l = Q.double(), K.double(), lse.double()
    s = float(scale)
    dc = (Qd[:, :1] * Kd).sum(-1)                                           # [B,N,H]
    dd = (Qd * Kd).sum(-1)
    Sc = (Qd[:, :1].abs() * Kd.abs()).sum(-1)
    Sd = (Qd.abs() * Kd.abs()).sum(-1)
    lt = l.permute(0, 2, 1)                                                 # [B,N,H]
    ac = torch.exp(dc * s - lt[:, :1])
    ad = torch.exp(dd * s - lt)
    return dict(cls=ac.mean(-1), diag=ad.mean(-1), ac=ac, ad=ad, Sc=Sc * s, Sd=Sd * s, argc=(dc * s - lt[:, :1]).abs(),
                argd=(dd * s - lt).abs(), dh=Q.shape[-1], H=Q.shape[2])


def stats_bound(ref, fmt):
    """Bound on |kernel - reference| of a_cls / a_diag: per head the f32 dot product (<= dh - 1 additions of partial sums <= S, 2u dh S;
    two-plane elements are hi + lo summed in f32 first, one more u per product), * scale and - lse one rounding each (u |.|), expf
    (ASSUMPTION: 2 ulp) -- a relative error e^{ea} (1 + EXPF) - 1 of the head's term; the head sum (H additions, then the fast kernel's
    6-step wave sum: depth <= H + 6) and / H one rounding: (2u (H + 7)) of the mean of |terms| times (1 + their relative error)."""
    dh, H = ref["dh"], ref["H"]
    k = 2 * U * dh + (3 * U if fmt == "h2" else 0.0) + U
    out = {}
    for name, a, S, arg in (("cls", ref["ac"], ref["Sc"], ref["argc"]), ("diag", ref["ad"], ref["Sd"], ref["argd"])):
        ea = k * 1.01 * S + U * 1.01 * (S + arg)
        rel = torch.expm1(ea) * (1 + EXPF) + EXPF
        per = a * rel
        out[name] = per.mean(-1) + 2 * U * (H + 7) * (a * (1 + rel)).mean(-1)
    return out


def check_within(got, ref, bound, what=""):
    """Every element of `got` within `bound` of `ref` (NaN / inf fail); returns the largest err / bound ratio."""
    err = (got.double() - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements outside the bound; first at {i}: got {float(got[i])}, "
                             f"ref {float(ref[i])}, bound {float(bound[i])}")
    return float((err / bound).max())


# ---- case generators ---------------------------------------------------------------------------------------------------------------
OUTLIER_KEYS = (0, 63, 64, 127)


def to_fmt(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """f32 values -> what the kernel will consume, as f32 (bf16 / f16: rounded; two-plane: the f32 value itself, stored by pack_h2)."""
    if fmt == "bf16":
        return x.bfloat16().float()
    if fmt == "f16":
        return x.clamp(-F16_MAX, F16_MAX).half().float()
    return x.float()


def make_case(design, *, fmt, B, N, H, dh, n_terms=1, seed=0, device="cpu", scale=None):
    """Operands (f32, already in `fmt`'s value set for bf16 / f16) of one data design, as Q[t], K[t], V [B,N,H,dh] and the f32 scale.

    normal     N(0,1) q, k, v; scale dh^-1/2 unless given.
    outlier    keys 0, 63, 64, 127 and N-1 score 32 nats above the rest for every query (q_0 = 4, k_j = 64 e_0, scale 1/8 or the exact-c2
               2^-3 ln2 scale gives 2^5 log2 units): their V rows are small integers, exact in every format.
    stair9     exact c2 = 2^-3, q_0 = 8: key tile t scores 10 t log2 units (+ noise < 0.1): every tile raises the row maximum by >= 9, a rescale
               on every tile.
    stair8     tile 0 at 0, every later tile exactly 8 log2 units higher: no rescale after the first tile, P = 2^8.
    underflow  tile 0 at 0, later tiles 136 log2 units above: alpha = 2^-136, i.e. 0 after the first tile.
    equal      every key the same vector: all scores equal.
    fraction   tile 0 at 0, later tiles at log2(1 + 2^-7 - 2^-12) (bf16 k): P ~ 1.0076, rounded up by nearest-even, down by truncation; V 0
               on tile 0 and 1 elsewhere.
    """
    g = torch.Generator(device=device).manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=g, device=device, dtype=torch.float32)

    Q = [rn(B, N, H, dh) for _ in range(n_terms)]
    K = [rn(B, N, H, dh) for _ in range(n_terms)]
    V = rn(B, N, H, dh)
    tile = (torch.arange(N, device=device) // KT).float()
    sc = scale
    if design == "normal":
        sc = dh ** -0.5 if sc is None else sc
    elif design == "outlier":
        sc = 0.125 if sc is None else sc
        keys = sorted({k for k in OUTLIER_KEYS + (N - 1,) if k < N})
        for t in range(n_terms):
            Q[t][..., 0] = 4.0
            K[t][..., 0] = 0.0
            for j in keys:
                K[t][:, j] = 0.0
                K[t][:, j, :, 0] = 64.0
        for j in keys:
            V[:, j] = ((j + 3 * torch.arange(dh, device=device)) % 7 - 3).float()
    elif design in ("stair9", "stair8", "underflow", "equal", "fraction"):
        sc = exact_c2_scale(-3) if sc is None else sc
        noise = 2.0 ** -6 if design == "stair9" else 0.0
        for t in range(n_terms):
            Q[t] = Q[t] * noise
            K[t] = K[t] * noise
            Q[t][..., 0] = 8.0 / n_terms
            if design == "stair9":
                K[t][..., 0] = (10.0 * tile)[None, :, None]
            elif design == "stair8":
                K[t][..., 0] = (8.0 * (tile > 0).float())[None, :, None]
            elif design == "underflow":
                K[t][..., 0] = (136.0 * (tile > 0).float())[None, :, None]
            elif design == "equal":
                K[t][...] = K[t][:, :1]
                K[t][..., 0] = 1.0
            else:
                K[t][..., 0] = (math.log2(1 + 2.0 ** -7 - 2.0 ** -12) * (tile > 0).float())[None, :, None]
        if design == "fraction":
            V = (tile > 0).float()[None, :, None, None].expand(B, N, H, dh).clone()
    else:
        raise ValueError(design)
    Q = [to_fmt(q, fmt) for q in Q]
    K = [to_fmt(k, fmt) for k in K]
    V = to_fmt(V, fmt)
    return Q, K, V, float(torch.tensor(sc, dtype=torch.float32))
