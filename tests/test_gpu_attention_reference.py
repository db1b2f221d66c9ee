"""Every fused attention instantiation against a float64 reference of the same operation, element by element, with the per-element bound of
tests/attention_reference.py (score error, P conversion, accumulation, rescales, stream sum and store; no constant fitted to outputs).
Each case
  * runs sg_attention_raw on operands in the kernel's own storage (bf16 / f16 / two-plane) and compares with the reference on the decoded
    storage, using the f32 scale, bias, lse_in and per-image scales the kernel was given,
  * asserts from sg_attention_last_kernel() which instantiation ran (dh, TS, lean / generic / Experimental, single / multi-stream,
    context / LSE-only, operand kind), in which workgroup order, with how many LDS buffers and on which grid,
  * starts ctx and lse_out as NaN inside guard bands, and checks the bands and the gap columns of a strided ctx (ctx_st > H dh) untouched.
All 144 instantiations (4 head dims x 3 operand kinds x 12 kernels) run at least once, over N in {1 .. 4097} and the data designs of
attention_reference.make_case (N(0,1), outlier keys, rescale staircases, underflow, all-equal).  Then the GEM and text-tower shapes, the
three workgroup orders, images past 2^31 elements, the statistics kernels and the composed sg_op_attention."""
import ctypes as C
import math

import pytest
import torch

from attention_reference import (KT, attention_bound, attention_reference, c2_of, check_within, exact_c2_scale, make_case,
                                 stats_bound, stats_reference, to_fmt)
from gemm_reference import U, pack_h2, unpack_h2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PREC = {"bf16": 1, "f16": 3, "h2": 4}
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "h2": torch.float16}
GUARD = 4096
GUARD_BYTE = 0xA5
RESULTS = {}                                                      # family -> (cases, largest err / bound)
SEEN = set()                                                      # (kind, dh, ts, gk, multi, pv) instantiations run
ORDERS = set()


def _lib():
    from clip_decontamination_amd import _lib as L
    return L.load()


def cdiv(a, b):
    return (a + b - 1) // b


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def record(family, ratio):
    n, worst = RESULTS.get(family, (0, 0.0))
    RESULTS[family] = (n + 1, max(worst, ratio))


class Guarded:
    """A buffer inside GUARD bytes of GUARD_BYTE either side, itself all-ones bytes (NaN in every format)."""

    def __init__(self, numel, dtype):
        esz = torch.empty((), dtype=dtype).element_size()
        self.n = numel * esz
        self.buf = torch.full((self.n + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + self.n] = 0xFF
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype)

    def check_guards(self, what):
        assert bool((self.buf[:GUARD] == GUARD_BYTE).all()), f"{what}: a store landed in the guard band before the buffer"
        assert bool((self.buf[GUARD + self.n:] == GUARD_BYTE).all()), f"{what}: a store landed in the guard band after the buffer"


def place(x, sb, st, fmt):
    """x [B,N,D] f32 (in fmt's value set) -> (storage buffer, decoded f64 [B,N,D]) with element strides sb / st (two-plane: 2x in f16)."""
    B, N, D = x.shape
    f = 2 if fmt == "h2" else 1
    n = ((B - 1) * sb + (N - 1) * st + D) * f
    buf = torch.zeros(n + 64, dtype=DT[fmt], device=DEV)
    stored = pack_h2(x) if fmt == "h2" else x.to(DT[fmt])
    buf.as_strided((B, N, D * f), (sb * f, st * f, 1)).copy_(stored)
    dec = unpack_h2(stored) if fmt == "h2" else stored.double()
    return buf, dec


def expect_attn(fmt, dh, ts, gk, multi, pv, B, N, H, bias):
    order = (2 if (B >= 16 and H % 4 == 0) else 1) if bias else 0
    nqb = cdiv(N, 128)
    grid = (cdiv(B, 8) * 8 * H * nqb if order == 2 else cdiv(B * nqb, 8) * 8 * H if order == 1 else cdiv(H * B, 8) * 8 * nqb)
    nb = 1 if (fmt == "h2" and dh == 128 and ts == 2) else 2
    return (f"attn dh={dh} ts={ts} gk={gk} multi={multi} pv={pv} kind={fmt} order={('head', 'qblock', 'images')[order]} nb={nb} "
            f"grid={grid}")


def run_attn(fmt, design, *, B=1, N=129, H=2, dh=64, n_terms=1, sum_scores=0, causal=False, bias=None, resoftmax=False, pv=True,
             lse=True, spi=None, out_scale=1.0, scale=None, ctx_gap=8, qk_pad=16, same_qkv=False, v_st3=False, sb_pad=0, seed=0,
             family=None):
    """One sg_attention_raw case; bias None / 'sim' (per image) / 'shared' (bias_bstride 0) / 'gauss' (shared, with rn / cn)."""
    lib = _lib()
    D = H * dh
    Q, K, V, sc = make_case(design, fmt=fmt, B=B, N=N, H=H, dh=dh, n_terms=n_terms, seed=seed, device=DEV, scale=scale)
    if same_qkv:                                                  # GEM: q = k = v, l2-normalised per head
        X = Q[0]
        X = to_fmt(X / X.norm(dim=-1, keepdim=True).clamp(min=1e-6), fmt)
        Q, K, V = [X] * n_terms, [X] * n_terms, X
    st = D + qk_pad
    sb = N * st + sb_pad
    bufs, Qd, Kd = [], [], []
    for t in range(n_terms):
        bq, dq = place(Q[t].reshape(B, N, D), sb, st, fmt)
        if same_qkv:
            bk, dk = bq, dq
        else:
            bk, dk = place(K[t].reshape(B, N, D), sb, st, fmt)
        bufs += [bq, bk]
        Qd.append(dq.view(B, N, H, dh))
        Kd.append(dk.view(B, N, H, dh))
    if same_qkv and not v_st3:
        bv, dv, v_sb, v_st = bufs[0], Qd[0].reshape(B, N, D), sb, st
    else:
        v_st = 3 * D if v_st3 else D
        v_sb = N * v_st
        full = torch.zeros(B, N, v_st, device=DEV)
        off = 2 * D if v_st3 else 0
        full[..., off:off + D] = V.reshape(B, N, D)
        bv_full, dv_full = place(full, v_sb, v_st, fmt)
        f = 2 if fmt == "h2" else 1
        bv = bv_full[off * f:]
        dv = dv_full[..., off:off + D]
    Vd = dv.reshape(B, N, H, dh)
    scale_t = torch.full((B,), sc, device=DEV) if spi is None else torch.tensor(spi, dtype=torch.float32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed + 7)
    kw = dict(sum_scores=sum_scores, causal=causal, out_scale=out_scale)
    b_t = rn_t = cn_t = None
    bias_w, bstride = 0.0, 0
    if bias:
        Bb = B if bias == "sim" else 1
        b = torch.randn(Bb, N - 1, N - 1, generator=g, device=DEV)
        b_t = ((b + b.transpose(-1, -2)) * 0.5).contiguous()
        bias_w, bstride = 0.8, ((N - 1) ** 2 if bias == "sim" else 0)
        kw.update(bias=b_t, bias_w=bias_w)
        if bias == "gauss":
            rn_t = torch.rand(B, H, N, generator=g, device=DEV) + 0.5
            cn_t = torch.rand(B, H, N, generator=g, device=DEV) + 0.5
            kw.update(bias_rn=rn_t, bias_cn=cn_t)
    lse_in = None
    if resoftmax:
        first = attention_reference(Qd, Kd, Vd, scale=scale_t, sum_scores=sum_scores)
        lse_in = first["lse"].float().contiguous()
        kw.update(resoftmax=True, lse_in=lse_in)
    ts = n_terms if sum_scores else 1
    gk = 0 if not (bias or resoftmax or causal) else (2 if (bias and resoftmax and not causal and bias != "gauss" and (sum_scores or n_terms == 1) and pv) else 1)
    multi = int(pv and not sum_scores and n_terms > 1)
    ctx_st = D + ctx_gap
    f = 2 if fmt == "h2" else 1
    ctx = Guarded(B * N * ctx_st * f, DT[fmt]) if pv else None
    lse_out = Guarded(B * H * N, torch.float32) if lse else None
    q_ptrs = [ptr(bufs[2 * t]) for t in range(n_terms)] + [None] * (3 - n_terms)
    k_ptrs = [ptr(bufs[2 * t + 1]) for t in range(n_terms)] + [None] * (3 - n_terms)
    rc = lib.sg_attention_raw(PREC[fmt], *q_ptrs, *k_ptrs, sb, st, ptr(bv), v_sb, v_st, B, N, H, dh, n_terms, sum_scores, int(causal),
                              sc, ptr(scale_t) if spi is not None else None, ptr(b_t), bias_w, bstride, ptr(rn_t), ptr(cn_t), int(resoftmax),
                              ptr(lse_in), ptr(lse_out.t) if lse else None, ptr(ctx.t) if pv else None, N * ctx_st, ctx_st, out_scale,
                              stream())
    assert rc == 0, lib.sg_last_error()
    rec = lib.sg_attention_last_kernel().decode()
    assert rec == expect_attn(fmt, dh, ts, gk, multi, int(pv), B, N, H, bias), rec
    torch.cuda.synchronize()
    SEEN.add((fmt, dh, ts, gk, multi, int(pv)))
    ORDERS.add(rec.split("order=")[1].split()[0])
    ref = attention_reference(Qd, Kd, Vd, scale=scale_t, **kw)
    exact = bool((c2_of(scale_t) == torch.exp2(torch.round(torch.log2(c2_of(scale_t))))).all())
    bd = attention_bound(ref, fmt=fmt, lean=gk == 0, c2_exact=exact)
    what = f"{fmt} {design} B={B} N={N} H={H} dh={dh} terms={n_terms} sum={sum_scores} causal={causal} bias={bias} rs={resoftmax} [{rec}]"
    fam = family or f"{fmt} {('lean', 'generic', 'exper')[gk]}{' multi' if multi else ''}{'' if pv else ' lse-only'}"
    worst = 0.0
    if pv:
        ctx.check_guards(what)
        v = ctx.t.view(B, N, ctx_st * f)
        gap = v[..., D * f:]
        assert bool((gap.contiguous().view(torch.uint8) == 0xFF).all()), f"{what}: a store landed in the gap columns of ctx"
        got = unpack_h2(v[..., :D * f]) if fmt == "h2" else v[..., :D]
        worst = check_within(got.reshape(B, N, H, dh), ref["ctx"], bd["ctx"], what)
    if lse:
        lse_out.check_guards(what + " lse")
        worst = max(worst, check_within(lse_out.t.view(B, H, N), ref["lse"], bd["lse"], what + " lse"))
    record(fam, worst)
    print(f"{what}: max err/bound {worst:.3g}")
    return worst


# ---- all 144 instantiations ------------------------------------------------------------------------------------------------------------
# (name, kwargs) per kernel of one (head dim, operand kind): lean / generic / Experimental x single / multi x context / LSE-only x TS 1 / 2
KERNELS = [
    ("lean1", dict()),
    ("lean_multi", dict(n_terms=3)),
    ("lean_lse", dict(pv=False)),
    ("gen1", dict(causal=True)),
    ("gen_multi", dict(n_terms=2, bias="sim")),
    ("gen_lse", dict(pv=False, bias="gauss")),
    ("exper1", dict(bias="sim", resoftmax=True)),
    ("lean2", dict(n_terms=2, sum_scores=1)),
    ("lean2_lse", dict(n_terms=2, sum_scores=1, pv=False)),
    ("gen2", dict(n_terms=2, sum_scores=1, bias="gauss")),
    ("gen2_lse", dict(n_terms=2, sum_scores=1, pv=False, causal=True)),
    ("exper2", dict(n_terms=2, sum_scores=1, bias="sim", resoftmax=True)),
]
NS = [1, 2, 31, 63, 64, 65, 127, 128, 129, 197, 257]
DESIGNS = ["normal", "outlier", "stair9", "stair8", "underflow", "equal"]
SWEEP = [(fmt, dh, i) for fmt in ("bf16", "f16", "h2") for dh in (32, 64, 80, 128) for i in range(len(KERNELS))]


@pytest.mark.parametrize("fmt,dh,i", SWEEP, ids=[f"{f}-{d}-{KERNELS[i][0]}" for f, d, i in SWEEP])
def test_instantiation(fmt, dh, i):
    name, kw = KERNELS[i]
    j = i + dh + 5 * ("bf16", "f16", "h2").index(fmt)
    N = NS[j % len(NS)]
    if kw.get("bias") or kw.get("causal"):
        N = max(N, 31)                                            # a bias needs N - 1 >= 1 keys of its own
    design = DESIGNS[(j // 2) % len(DESIGNS)]
    if design in ("stair9", "stair8", "underflow") and N <= KT:
        N += KT + 1
    run_attn(fmt, design, N=N, dh=dh, B=1 + (j % 2), seed=j, **kw)


def test_every_instantiation_ran():
    assert len(SEEN) == 144, sorted(SEEN)


# ---- shapes, designs and orders -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16", "h2"])
@pytest.mark.parametrize("design,N,kw", [
    ("normal", 1370, dict()), ("outlier", 1370, dict()), ("stair9", 1370, dict()), ("stair8", 257, dict()), ("underflow", 4097, dict(H=1)),
    ("equal", 1370, dict()), ("outlier", 4097, dict(H=1, causal=True)), ("stair9", 4097, dict(H=1, bias="sim")),
    ("normal", 1370, dict(n_terms=3)), ("normal", 197, dict(scale=exact_c2_scale(-3))),
])
def test_designs(fmt, design, N, kw):
    run_attn(fmt, design, N=N, seed=N + len(kw), **kw)


@pytest.mark.parametrize("fmt", ["bf16", "h2"])
@pytest.mark.parametrize("B,H,bias", [(16, 4, "gauss"), (16, 4, "sim"), (17, 4, "shared"), (16, 6, "sim"), (3, 2, "sim"), (16, 4, None)])
def test_workgroup_orders(fmt, B, H, bias):
    run_attn(fmt, "normal", B=B, H=H, N=65, dh=32, bias=bias, seed=B * H)


def test_all_orders_ran():
    assert ORDERS == {"head", "qblock", "images"}, ORDERS


@pytest.mark.parametrize("fmt", ["bf16", "f16", "h2"])
def test_gem_shape(fmt):
    """GEM: per-image scale, q = k = v, then three streams with V strides 3D and out_scale 1/3."""
    run_attn(fmt, "normal", B=2, N=197, H=2, dh=64, spi=[3.0, 7.5], same_qkv=True, family=f"{fmt} gem")
    run_attn(fmt, "normal", B=2, N=197, H=2, dh=64, n_terms=3, spi=[3.0, 7.5], out_scale=1 / 3, same_qkv=True, v_st3=True, qk_pad=0,
             family=f"{fmt} gem")


@pytest.mark.parametrize("fmt", ["bf16", "f16", "h2"])
def test_text_tower_shape(fmt):
    run_attn(fmt, "normal", B=2, N=77, H=8, dh=64, causal=True, family=f"{fmt} text")


@pytest.mark.parametrize("fmt", ["bf16", "h2"])
def test_image_past_2_31(fmt):
    """B = 2 with a batch stride past 2^31 elements: image 1's operands start beyond 32-bit element offsets (q = k = v, as GEM)."""
    N, H, dh = 129, 2, 64
    st = H * dh + 16
    run_attn(fmt, "normal", B=2, N=N, H=H, dh=dh, same_qkv=True, sb_pad=(1 << 31) - N * st + 4096, family=f"{fmt} past 2^31")
    torch.cuda.empty_cache()


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dh,lph", [("bf16", 32, 4), ("bf16", 64, 8), ("bf16", 128, 16), ("f16", 32, 4), ("f16", 64, 8), ("f16", 128, 16),
                                        ("bf16", 80, 0), ("f16", 80, 0), ("h2", 64, 0), ("h2", 80, 0)])
def test_stats(fmt, dh, lph):
    lib = _lib()
    B, N, H = 2, 197, 3
    D = H * dh
    Q, K, V, sc = make_case("outlier", fmt=fmt, B=B, N=N, H=H, dh=dh, seed=dh + lph, device=DEV)
    st = 2 * D + 8
    x = torch.cat([Q[0].reshape(B, N, D), K[0].reshape(B, N, D)], dim=-1)
    buf, dec = place(x, N * st, st, fmt)
    Qd, Kd = dec[..., :D].reshape(B, N, H, dh), dec[..., D:].reshape(B, N, H, dh)
    scale_t = torch.full((B,), sc, device=DEV)
    lse = attention_reference([Qd], [Kd], Vd_dummy(B, N, H, dh), scale=scale_t, sum_scores=0)["lse"].float().contiguous()
    a_cls, a_diag = Guarded(B * N, torch.float32), Guarded(B * N, torch.float32)
    rc = lib.sg_attention_stats_raw(PREC[fmt], ptr(buf), N * st, st, ptr(lse), B, N, H, dh, sc, ptr(a_cls.t), ptr(a_diag.t), stream())
    assert rc == 0, lib.sg_last_error()
    rec = lib.sg_attention_last_kernel().decode()
    kind = {"bf16": "bf16", "f16": "f16", "h2": "h2"}[fmt]
    assert rec == f"{'stats_fast' if lph else 'stats_generic'} lph={lph} kind={kind} grid={cdiv(N, 4) * B}", rec
    torch.cuda.synchronize()
    a_cls.check_guards("a_cls"); a_diag.check_guards("a_diag")
    ref = stats_reference(Qd, Kd, lse, sc)
    bd = stats_bound(ref, fmt)
    r1 = check_within(a_cls.t.view(B, N), ref["cls"], bd["cls"], f"stats {rec} cls")
    r2 = check_within(a_diag.t.view(B, N), ref["diag"], bd["diag"], f"stats {rec} diag")
    record(f"{fmt} stats {'fast' if lph else 'generic'}", max(r1, r2))


def Vd_dummy(B, N, H, dh):
    return torch.zeros(B, N, H, dh, dtype=torch.float64, device=DEV)


# ---- the composed entry ---------------------------------------------------------------------------------------------------------------
VARIANTS = {  # name -> (term (q, k) selections, sum_scores, scale multiplier, resoftmax); 0 q, 1 k, 2 v
    "vanilla": ([(0, 1)], 0, 1.0, False), "ClearCLIP": ([(0, 0)], 0, 1.0, False), "SCLIP": ([(0, 0), (1, 1)], 0, 1.0, False),
    "SegEarth": ([(0, 0), (1, 1), (2, 2)], 0, 1.0, False), "SFP": ([(0, 0), (1, 1)], 1, 0.5, False),
    "Experimental": ([(1, 1), (0, 0)], 1, 1.0, True),
}


@pytest.mark.parametrize("prec", ["bf16", "f16", "f16x2"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_composed_op_attention(variant, prec):
    from clip_decontamination_amd import ops
    fmt = {"bf16": "bf16", "f16": "f16", "f16x2": "h2"}[prec]
    B, N, H, dh = 1, 197, 2, 64
    D = H * dh
    g = torch.Generator(device=DEV).manual_seed(len(variant))
    qkv = torch.randn(B, N, 3 * D, generator=g, device=DEV)
    qkv = qkv.bfloat16().float() if fmt == "bf16" else qkv.half().float()          # pre-rounded: the library's packing is exact
    assert torch.equal(qkv.half().float() if fmt != "bf16" else qkv.bfloat16().float(), qkv)
    sel, sum_scores, smul, rs = VARIANTS[variant]
    sim = None
    if rs:
        s = torch.randn(B, N - 1, N - 1, generator=g, device=DEV)
        sim = ((s + s.transpose(-1, -2)) * 0.5).contiguous()
    out = ops.attention(qkv, H, variant, sim, 0.8, precision=prec)
    torch.cuda.synchronize()
    rec = _lib().sg_attention_last_kernel().decode()
    parts = qkv.double().view(B, N, 3, H, dh)
    Qd = [parts[:, :, a] for a, _ in sel]
    Kd = [parts[:, :, b] for _, b in sel]
    Vd = parts[:, :, 2]
    scale = float(torch.tensor(smul / math.sqrt(dh), dtype=torch.float32))
    scale_t = torch.full((B,), scale, device=DEV)
    kw = dict(sum_scores=sum_scores)
    lse_err = None
    if rs:
        first = attention_reference(Qd, Kd, Vd, scale=scale_t, sum_scores=sum_scores)
        # the library's first pass is the LEAN LSE pass (c2 q re-rounded), the second the generic one: carry the first pass's LSE bound
        lse_err = attention_bound(first, fmt=fmt, lean=True)["lse"] + U * first["lse"].abs() * 1.01
        kw.update(resoftmax=True, lse_in=first["lse"], bias=sim, bias_w=0.8)
    ref = attention_reference(Qd, Kd, Vd, scale=scale_t, **kw)
    bd = attention_bound(ref, fmt=fmt, lean=not rs, lse_in_err=lse_err)
    bctx = bd["ctx"] + (U * (ref["ctx"].abs() + bd["ctx"]) if fmt == "h2" else 0.0)   # two-plane -> f32 unpack: hi + lo in f32
    ratio = check_within(out.view(B, N, H, dh), ref["ctx"], bctx, f"sg_op_attention {variant} {prec} [{rec}]")
    assert rec.startswith("attn ") and f"kind={fmt}" in rec, rec
    record(f"{fmt} composed", ratio)


def test_record_says_none_after_a_refused_call():
    lib = _lib()
    run_attn("bf16", "normal", N=65, dh=32)
    x = torch.zeros(4096, dtype=torch.bfloat16, device=DEV)
    rc = lib.sg_attention_raw(1, ptr(x), None, None, ptr(x), None, None, 8 * 96, 96, ptr(x), 8 * 96, 96, 1, 8, 1, 96, 1, 0, 0, 0.1,
                              None, None, 0.0, 0, None, None, 0, None, None, ptr(x), 8 * 96, 96, 1.0, stream())
    assert rc != 0 and b"not built" in lib.sg_last_error()
    assert lib.sg_attention_last_kernel() == b"none"


def test_summary():
    """Prints the number of cases and the largest err / bound per family (run last in this module)."""
    print(f"SUMMARY instantiations {len(SEEN)}, orders {sorted(ORDERS)}")
    for fam in sorted(RESULTS):
        n, worst = RESULTS[fam]
        print(f"SUMMARY {fam}: {n} cases, largest err/bound {worst:.3g}")
