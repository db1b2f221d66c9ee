"""The per-element attention bound of tests/attention_reference.py has teeth (CPU only).  An f32 emulation of the kernels' arithmetic passes
it: tile-wise online softmax with the lazy 2^8 threshold, P rounded to the operand format, l summed in another order.  Each of the small,
localised mistakes a fused attention kernel can make fails it, on the same case generators the GPU module uses.  The staircase designs
also show that the rescale branch is reached: a rescale that skips o_acc or l_run fails on `stair9` and changes nothing on `stair8`."""
import math

import pytest
import torch

from attention_reference import (KT, LN2_F32, LOG2E_F32, TAU, attention_bound, attention_reference, c2_of, check_within, exact_c2_scale,
                                 make_case)


def rnd_fmt(p, fmt, trunc=False, lose_lo=False):
    """Probabilities / values -> the format's value set, in f32 (two-plane: hi + lo)."""
    if fmt == "bf16":
        if trunc:
            return (p.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)
        return p.bfloat16().float()
    if fmt == "f16":
        return p.half().float()
    hi = p.half()
    if lose_lo:
        return hi.float()
    return hi.float() + (p - hi.float()).half().float()


def emulate(Q, K, V, *, fmt, lean, scale, sum_scores, causal=False, bias=None, bias_w=0.0, bias_rn=None, bias_cn=None, resoftmax=False,
            lse_in=None, out_scale=1.0, mut=()):
    """The kernels' arithmetic in f32 on [B,N,H,dh] operands; `mut` names the mistakes to make.  Returns (ctx [B,N,H,dh], lse [B,H,N])."""
    mut = dict.fromkeys(mut, True) if not isinstance(mut, dict) else mut
    B, N, H, dh = V.shape
    c2 = c2_of(scale).float().view(B, 1, 1, 1)
    log2e = torch.tensor(LOG2E_F32)
    terms = list(range(len(Q)))
    groups = [terms] if sum_scores else [[t] for t in terms]
    Vh = V.permute(0, 2, 1, 3).float()
    if fmt == "h2" and mut.get("lose_lo_v"):
        Vh = Vh.half().float()
    keys = torch.arange(N)
    mask = torch.zeros(N, N, dtype=torch.bool)
    if causal:
        mask = keys[None, :] > keys[:, None] + mut.get("causal_shift", 0)
    for j in mut.get("drop", ()):
        mask[:, j] = True
    bfull = None
    if bias is not None:
        n = N - 1
        bt = bias.float().reshape(-1, n, n)                                  # [Bb, key-1, query-1]
        kidx = torch.arange(1, N) + (1 if mut.get("bias_shift") else 0)
        kidx = kidx.clamp(max=N - 1)
        full = torch.zeros(bt.shape[0], N, N)
        full[:, 1:, 1:] = bt[:, kidx - 1, :].transpose(-1, -2)
        bfull = full[:, None].expand(B, H, N, N)
        if bias_cn is not None:
            rn, cn = (bias_cn, bias_rn) if mut.get("swap_rn_cn") else (bias_rn, bias_cn)
            bfull = bfull * (cn.float()[..., None, :] * rn.float()[..., :, None])
        bfull = bfull * torch.tensor(bias_w, dtype=torch.float32)
    scores = []
    for g in groups:
        if lean:
            sacc = sum(torch.matmul(rnd_fmt(Q[t].float() * c2, fmt).permute(0, 2, 1, 3), K[t].float().permute(0, 2, 3, 1)) for t in g)
            x = sacc
        else:
            sacc = sum(torch.matmul(Q[t].float().permute(0, 2, 1, 3), K[t].float().permute(0, 2, 3, 1)) for t in g)
            x = sacc * c2
            if resoftmax:
                l12 = lse_in.float()[..., None] * (1.0 if mut.get("lse_log2") else log2e)
                x = torch.exp2(x - l12)
                if bfull is not None:
                    x = x + bfull
                x = x * log2e
            elif bfull is not None:
                x = x + bfull * log2e
        scores.append(x)
    if mut.get("score_space"):
        scores = [sum(scores)]
    n_keys = N
    Vk = Vh
    if mut.get("unmask_tail"):                                                # the clamped row N-1 counted once more
        scores = [torch.cat([x, x[..., -1:]], dim=-1) for x in scores]
        Vk = torch.cat([Vh, Vh[:, :, -1:]], dim=2)
        mask = torch.cat([mask, mask[:, -1:]], dim=1)
        n_keys = N + 1
    ctx, lse = 0.0, None
    for x in scores:
        x = x.masked_fill(mask, float("-inf"))
        m = torch.full((B, H, N, 1), float("-inf"))
        l = torch.zeros(B, H, N, 1)
        o = torch.zeros(B, H, N, dh)
        for k0 in range(0, n_keys, KT):
            xt = x[..., k0:k0 + KT]
            mloc = xt.amax(dim=-1, keepdim=True)
            need = (mloc > m + TAU) | torch.isinf(m)
            m_new = torch.where(need, torch.maximum(m, mloc), m)
            alpha = torch.where(need & ~torch.isinf(m), torch.exp2(m - m_new), torch.ones_like(m))
            if not mut.get("skip_o"):
                o = o * alpha
            if not mut.get("skip_l"):
                l = l * alpha
            m = m_new
            msub = torch.where(torch.isinf(m), torch.zeros_like(m), m)
            p = torch.exp2(xt - msub)
            l = l + p.flip(-1).sum(-1, keepdim=True)                          # another order than the reference's
            P = rnd_fmt(p, fmt, trunc=mut.get("trunc_p", False), lose_lo=mut.get("lose_lo_p", False))
            o = o + torch.matmul(P, Vk[:, :, k0:k0 + KT])
        ctx = ctx + o * (1.0 / l)
        lse = (m + torch.log2(l))[..., 0] * LN2_F32
    if not mut.get("no_out_scale"):
        ctx = ctx * out_scale
    ctx = ctx.permute(0, 2, 1, 3)
    return rnd_fmt(ctx, fmt), lse


def build_case(design, fmt, *, N=257, B=1, H=2, dh=64, n_terms=1, sum_scores=0, causal=False, bias=False, gauss=False, resoftmax=False,
               spi=None, out_scale=1.0, seed=0):
    Q, K, V, sc = make_case(design, fmt=fmt, B=B, N=N, H=H, dh=dh, n_terms=n_terms, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    kw = dict(sum_scores=sum_scores, causal=causal, out_scale=out_scale)
    scale = torch.full((B,), sc) if spi is None else torch.tensor(spi, dtype=torch.float32)
    if bias:
        b = torch.randn(B, N - 1, N - 1, generator=g)
        kw.update(bias=(b + b.transpose(-1, -2)) * 0.5, bias_w=0.75)
        if gauss:
            kw.update(bias_rn=torch.rand(B, H, N, generator=g) + 0.5, bias_cn=torch.rand(B, H, N, generator=g) + 0.5)
    if resoftmax:
        first = attention_reference(Q, K, V, scale=scale, sum_scores=sum_scores)
        kw.update(resoftmax=True, lse_in=first["lse"].float())
    return Q, K, V, scale, kw


def bound_for(Q, K, V, scale, kw, fmt, lean):
    ref = attention_reference(Q, K, V, scale=scale, **kw)
    exact = bool((c2_of(scale) == torch.exp2(torch.round(torch.log2(c2_of(scale))))).all())
    return ref, attention_bound(ref, fmt=fmt, lean=lean, c2_exact=exact)


def passes(design, fmt, lean, mut=(), **kw):
    Q, K, V, scale, akw = build_case(design, fmt, **kw)
    ref, b = bound_for(Q, K, V, scale, akw, fmt, lean)
    got, lse = emulate(Q, K, V, fmt=fmt, lean=lean, scale=scale, mut=mut, **akw)
    ratio = check_within(got, ref["ctx"], b["ctx"], f"{design} {fmt} lean={lean} {mut}")
    lratio = check_within(lse, ref["lse"], b["lse"], "lse")
    return ratio, lratio


def fails(design, fmt, lean, mut, **kw):
    with pytest.raises(AssertionError, match="outside the bound"):
        passes(design, fmt, lean, mut, **kw)


CONTROL = [
    ("normal", dict()), ("normal", dict(N=129, dh=32)), ("normal", dict(N=63, dh=80)), ("normal", dict(N=65, dh=128)),
    ("outlier", dict()), ("stair9", dict(N=300)), ("stair8", dict(N=200)), ("underflow", dict(N=130)), ("equal", dict(N=197)),
    ("fraction", dict(N=129)), ("normal", dict(n_terms=3)), ("normal", dict(n_terms=2, sum_scores=1)),
]


@pytest.mark.parametrize("fmt", ["bf16", "f16", "h2"])
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("design,kw", CONTROL)
def test_emulation_passes(design, kw, fmt, lean):
    ratio, lratio = passes(design, fmt, lean, **kw)
    print(f"{design} {kw} {fmt} lean={lean}: ctx err/bound {ratio:.3g}, lse {lratio:.3g}")
    assert ratio < 1 and lratio < 1


@pytest.mark.parametrize("fmt", ["bf16", "f16", "h2"])
@pytest.mark.parametrize("kw", [dict(bias=True), dict(bias=True, gauss=True), dict(causal=True, N=77, H=8), dict(resoftmax=True, bias=True),
                                dict(resoftmax=True, n_terms=2, sum_scores=1, bias=True), dict(n_terms=3, bias=True),
                                dict(n_terms=3, spi=[3.0, 7.5], B=2, out_scale=1 / 3)])
def test_emulation_passes_generic(kw, fmt):
    ratio, lratio = passes("normal", fmt, False, **kw)
    print(f"generic {kw} {fmt}: ctx err/bound {ratio:.3g}, lse {lratio:.3g}")
    assert ratio < 1 and lratio < 1


# ---- mutations -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16", "h2"])
@pytest.mark.parametrize("key", [0, 63, 64, "last"])
def test_dropped_key_fails(fmt, key):
    N = 197
    fails("outlier", fmt, True, dict(drop=(N - 1 if key == "last" else key,)), N=N)


@pytest.mark.parametrize("fmt", ["bf16", "h2"])
def test_unmasked_tail_fails(fmt):
    fails("outlier", fmt, True, ("unmask_tail",), N=197)


@pytest.mark.parametrize("shift", [-1, 1])
def test_causal_off_by_one_fails(shift):
    fails("normal", "bf16", False, dict(causal_shift=shift), causal=True, N=77, H=8)


@pytest.mark.parametrize("fmt", ["bf16", "f16", "h2"])
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("skip", ["skip_o", "skip_l"])
def test_rescale_skips_fail_on_stair9_only(fmt, lean, skip):
    """stair9 raises the row maximum by >= 9 log2 units per tile, so each tile rescales; stair8 never rescales after the first tile."""
    fails("stair9", fmt, lean, (skip,), N=300)
    ratio, _ = passes("stair8", fmt, lean, (skip,), N=300)
    assert ratio < 1


def test_bias_from_neighbouring_key_fails():
    fails("normal", "bf16", False, ("bias_shift",), bias=True)


def test_rn_cn_swapped_fails():
    fails("normal", "f16", False, ("swap_rn_cn",), bias=True, gauss=True)


def test_lost_lo_plane_of_p_fails():
    fails("fraction", "h2", False, ("lose_lo_p",), N=129)


def test_lost_lo_plane_of_v_fails():
    """All-equal scores and V = 1/3 everywhere: the context is exactly 1/3, and f16(1/3) misses it by 2.4e-4 relative."""
    Q, K, V, sc = make_case("equal", fmt="h2", B=1, N=129, H=2, dh=64)
    V = torch.full_like(V, 1 / 3)
    scale = torch.full((1,), sc)
    ref, b = bound_for(Q, K, V, scale, dict(sum_scores=0), "h2", False)
    got, _ = emulate(Q, K, V, fmt="h2", lean=False, scale=scale, sum_scores=0)
    check_within(got, ref["ctx"], b["ctx"], "both planes")
    got, _ = emulate(Q, K, V, fmt="h2", lean=False, scale=scale, sum_scores=0, mut=("lose_lo_v",))
    with pytest.raises(AssertionError, match="outside the bound"):
        check_within(got, ref["ctx"], b["ctx"], "hi plane only")


@pytest.mark.parametrize("fmt", ["bf16", "h2"])
def test_out_scale_not_applied_fails(fmt):
    fails("normal", fmt, False, ("no_out_scale",), n_terms=3, spi=[3.0, 7.5], B=2, out_scale=1 / 3)


def test_streams_summed_in_score_space_fails():
    fails("normal", "bf16", True, ("score_space",), n_terms=2)


def test_lse_in_log2_units_fails():
    fails("normal", "bf16", False, ("lse_log2",), resoftmax=True, bias=True)


def test_truncated_p_fails():
    fails("fraction", "bf16", False, ("trunc_p",), N=1370)
    ratio, _ = passes("fraction", "bf16", False, (), N=1370)              # rounded to nearest even, the same P pass
    assert ratio < 1


def test_exact_c2_scales():
    for k in range(-6, 3):
        s = exact_c2_scale(k)
        assert float(c2_of(torch.tensor([s]))[0]) == 2.0 ** k
        assert abs(s / (2.0 ** k * math.log(2.0)) - 1) < 2e-6
