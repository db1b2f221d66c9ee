"""The bounds of tests/attnmap_reference.py on the CPU (no GPU needed): on every case the GPU modules run, an f32 restatement of each
stage in the kernel's operation order -- 64-lane strided sums where the kernels have them -- stays inside its bound, and each listed
single-fault mutant -- the kind of slip a kernel makes -- fails the same check on a named case:
  tail_dropped      a 64-stride row loop that stops at N rounded down to a multiple of 64
  col0_kept         column 0 of the boosted map not zeroed
  boost_row0        the diagonal boost applied to the CLS row too
  no_eps            the + 1e-8 of a row normalisation omitted
  mask_off_by_one   masked column idx instead of idx + 1
  mean_h_minus_1    head mean divided by H - 1
  alpha_dropped     the GEMM's alpha not applied
  batch_swapped     inner-batch stride exchanged with the outer one
  ragged_k          the last, ragged K step of the b_n_fast loader truncated
  pitch             the write-back copying N D instead of (N - 1) D elements per image
Also: the strided f64 GEMM reference equals torch.einsum on gathered operands, the rank-gap condition holds for every fusion seed, the
case table has the lane tails and thresholds the GPU module's docstring claims, the raw entries refuse before any launch."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attnmap_reference as AR                                          # noqa: E402
from attnmap_reference import RW, check_within                          # noqa: E402
from rowops_reference import lane_sum                                   # noqa: E402
from oracle import refine as OR                                         # noqa: E402

F32 = torch.float32
SENTINEL = -12345.5
GEMM_CASES = AR.gemm_cases()
CASES = AR.stage_cases()
IDS = ["N%d B%d H%d dh%d" % (AR.tokens_of(gh), B, H, dh) for gh, B, H, dh in CASES]
SIM_CASES = [(n, D, kind) for n in AR.SIM_N for D in AR.SIM_D for kind in AR.KINDS]
EPS32 = torch.tensor(1e-8, dtype=F32)


def within(got, ref, bound) -> bool:
    try:
        check_within(got, ref, bound)
    except AssertionError:
        return False
    return True


def trunc64(N: int, mut) -> int:
    return N // 64 * 64 if mut == "tail_dropped" else N


# ---- f32 GEMM ---------------------------------------------------------------------------------------------------------------------------
def act_f32(x, act):
    if act == 1:
        return x * (1.0 / (1.0 + torch.exp(torch.tensor(-1.702, dtype=F32) * x)))
    if act == 2:
        return 0.5 * x * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752440, dtype=F32)))
    if act == 3:
        return x.clamp(min=0.0)
    return x


def emulate_gemm(A, B, g, bias, R, Cbuf, mut=None):
    """gemm_f32_kernel in f32 on the flat buffers: returns C's buffer after the call."""
    gi = dict(g, sAo=g["sAi"], sAi=g["sAo"]) if mut == "batch_swapped" else g
    ia, ib, ic, ir = AR.gemm_indices(gi)
    a, b = A.float()[ia % A.numel()], B.float()[ib]
    if mut == "ragged_k" and g["sbn"] == 1 and g["sbk"] != 1:
        kt = g["K"] // 16 * 16
        a, b = a[:, :, :kt], b[:, :kt, :]
    x = torch.matmul(a, b)
    if mut != "alpha_dropped":
        x = x * torch.tensor(g["alpha"], dtype=F32)
    if bias is not None:
        x = x + bias.float()
    x = act_f32(x, g["act"])
    if R is not None:
        x = x + R.float()[ir]
    out = Cbuf.clone()
    out[ic] = x
    return out


_GEMM = {}


def gemm_case(ci):
    if ci not in _GEMM:
        tag, M, N, K, layout = GEMM_CASES[ci]
        g = AR.gemm_form(M, N, K, layout)
        bufs = AR.make_gemm_buffers(g, ci)
        _GEMM[ci] = (g, bufs, AR.gemm_products(bufs[0], bufs[1], g))
    return _GEMM[ci]


def gemm_ok(ci, ei, mut=None) -> bool:
    g, (A, B, bias, R, Cbuf), (acc, S) = gemm_case(ci)
    name, has_bias, act, has_res = AR.GEMM_EPILOGUES[ei]
    gg = dict(g, act=act, alpha=AR.alpha_of(ci, ei))
    _, _, ic, ir = AR.gemm_indices(gg)
    got = emulate_gemm(A, B, gg, bias if has_bias else None, R if has_res else None, Cbuf, mut)
    ref, bound = AR.gemm_epilogue_reference(acc, S, gg["K"], AR.f32(gg["alpha"]), bias if has_bias else None, R[ir] if has_res else None, act)
    rest = torch.ones(Cbuf.numel(), dtype=torch.bool)
    rest[ic.reshape(-1)] = False
    return within(got[ic], ref, bound) and bool((got[rest] == AR.GEMM_SENTINEL).all())


@pytest.mark.parametrize("ci", range(len(GEMM_CASES)), ids=[c[0] for c in GEMM_CASES])
def test_gemm_f32_restatement_inside_the_bound(ci):
    for ei in range(len(AR.GEMM_EPILOGUES)):
        assert gemm_ok(ci, ei), AR.GEMM_EPILOGUES[ei][0]


def case_index(M, N, K, layout):
    return [c[1:] for c in GEMM_CASES].index((M, N, K, layout))


# (mutant, case it must fail on, epilogue index, why there)
GEMM_MUTATIONS = [
    ("alpha_dropped", (127, 129, 15, "nk"), 0),           # whichever epilogue has alpha != 1 there (picked below)
    ("batch_swapped", (130, 260, 17, "kn"), 0),           # six unrelated strides: problem (zo, zi) = (0, 1) reads another block
    ("ragged_k", (127, 129, 17, "kn"), 0),                # K = 17: the 17th product is dropped
    ("ragged_k", (1, 1, 15, "kn"), 1),                    # K = 15: nothing is summed at all
    ("ragged_k", (130, 260, 197, "kn"), 5),               # 12 full steps and a ragged 5
]


@pytest.mark.parametrize("mut,shape,ei", GEMM_MUTATIONS)
def test_gemm_mutants_fail(mut, shape, ei):
    ci = case_index(*shape)
    if mut == "alpha_dropped":
        ei = next(e for e in range(6) if AR.alpha_of(ci, e) != 1.0)
    assert gemm_ok(ci, ei) and not gemm_ok(ci, ei, mut)


def test_strided_reference_equals_einsum_on_gathered_operands():
    for ci in (0, 9, 14, 23):
        g, (A, B, *_), (acc, S) = gemm_case(ci)
        a = torch.stack([torch.as_strided(A, (g["M"], g["K"]), (g["lda"], 1), (z // g["inner"]) * g["sAo"] + (z % g["inner"]) * g["sAi"])
                         for z in range(g["batch"])]).double()
        b = torch.stack([torch.as_strided(B, (g["K"], g["N"]), (g["sbk"], g["sbn"]), (z // g["inner"]) * g["sBo"] + (z % g["inner"]) * g["sBi"])
                         for z in range(g["batch"])]).double()
        want = torch.einsum("zmk,zkn->zmn", a, b)
        assert bool(((acc - want).abs() <= 1e-13 * S + 1e-300).all())
        assert bool(((S - torch.einsum("zmk,zkn->zmn", a.abs(), b.abs())).abs() <= 1e-13 * S).all())
    for g in (AR.aliased_form(), AR.reweight_form()):
        gen = torch.Generator().manual_seed(1)
        A = torch.randn(g["batch"] * g["M"] * g["K"], generator=gen)
        B = A if g["sbk"] == 1 else torch.randn(g["batch"] * g["K"] * g["N"], generator=gen)
        acc, S = AR.gemm_products(A, B, g)
        a = A.double().view(g["batch"], g["M"], g["K"])
        b = a.transpose(1, 2) if g["sbk"] == 1 else B.double().view(g["batch"], g["K"], g["N"])
        assert bool(((acc - a @ b).abs() <= 1e-13 * S).all())


def test_gemm_table_reaches_what_it_claims():
    pairs = set()
    for ci, (tag, M, N, K, layout) in enumerate(GEMM_CASES):
        g = AR.gemm_form(M, N, K, layout)
        st = [g[k] for k in ("sAo", "sAi", "sBo", "sBi", "sCo", "sCi")]
        assert AR._no_multiples(st), (tag, st)
        assert g["lda"] > K and g["ldc"] > N and g["ldr"] != g["ldc"] and g["ldr"] >= N
        assert (g["sbk"] == 1 and g["sbn"] > K) if layout == "nk" else (g["sbn"] == 1 and g["sbk"] > N)
        assert g["batch"] == 6 and g["inner"] == 3
        _, _, ic, _ = AR.gemm_indices(g)
        assert ic.unique().numel() == ic.numel()                        # no two problems share an element of C
        pairs |= {(AR.alpha_of(ci, ei), ei, layout) for ei in range(len(AR.GEMM_EPILOGUES))}
    assert len(pairs) == 3 * len(AR.GEMM_EPILOGUES) * 2                # every alpha meets every epilogue on both loaders
    assert [K % 16 for K in AR.GEMM_K] == [1, 15, 1, 5] and max(AR.GEMM_K) > 16 * 12
    assert any(M > 128 and N > 256 for M, N in AR.GEMM_MN) and (1, 1) in AR.GEMM_MN


def test_raw_entries_refuse_before_any_launch():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)                                        # never dereferenced
    g = AR.gemm_form(5, 7, 9, "kn", batch=2, inner=1)

    def gemm(**kw):
        h = dict(g, **kw)
        return lib.sg_gemm_f32_raw(h.get("A", p), h["lda"], h["sAo"], h["sAi"], p, h["sbk"], h["sbn"], h["sBo"], h["sBi"], None, None, h["ldr"],
                                   p, h["ldc"], h["sCo"], h["sCi"], h["M"], h["N"], h["K"], h["batch"], h["inner"], 0, 1.0, None)

    for field in ("M", "N", "K", "batch", "inner"):
        for bad in (0, -1):
            assert gemm(**{field: bad}) != 0 and b"gemm_f32: empty problem" in lib.sg_last_error(), (field, bad)
    assert gemm(A=None) != 0 and b"null pointer" in lib.sg_last_error()
    assert lib.sg_attn_average_raw(2, p, 1, 5, 8, 2, p, 1 << 20, p, None) != 0 and b"bad kind" in lib.sg_last_error()
    assert lib.sg_attn_average_raw(1, p, 1, 5, 9, 2, p, 1 << 20, p, None) != 0 and b"bad shape" in lib.sg_last_error()
    assert lib.sg_attn_average_raw(1, p, 1, 5, 8, 2, ctypes.c_void_p(1 << 20), 16, p, None) != 0 and b"scratch" in lib.sg_last_error()
    assert lib.sg_attn_enhance_raw(p, 80, 12, p, 2, 5, 8, 0.5, 0.15, p, None) != 0 and b"dense token rows" in lib.sg_last_error()
    assert lib.sg_attn_enhance_raw(p, 40, 8, p, 2, 1, 8, 0.5, 0.15, p, None) != 0 and b"bad shape" in lib.sg_last_error()
    assert lib.sg_layer_fusion_apply_raw(p, p, 1, 5, 8, 0, p, p, p, p, None) != 0 and b"bad shape" in lib.sg_last_error()
    assert lib.sg_layer_fusion_apply_raw(p, p, 1, 5, 8, 3, p, None, p, p, None) != 0 and b"null pointer" in lib.sg_last_error()


# ---- head-averaged attention -----------------------------------------------------------------------------------------------------------
def emulate_average_probs(probs, mut=None):
    H = probs.shape[1]
    acc = torch.zeros_like(probs[:, 0])
    for h in range(H):
        acc = acc + probs[:, h]
    return acc / torch.tensor(float(H - 1 if mut == "mean_h_minus_1" else H), dtype=F32)


def emulate_average_qkv(vals, H, mut=None):
    """unpack (exact), per-head f32 scores, softmax_rows_kernel's three passes with 64-lane sums, head_mean_kernel."""
    B, N, D3 = vals.shape
    D = D3 // 3
    dh = D // H
    x = vals.float()
    q = x[..., :D].view(B, N, H, dh).permute(0, 2, 1, 3)
    k = x[..., D:2 * D].view(B, N, H, dh).permute(0, 2, 1, 3)
    v = torch.matmul(q, k.transpose(-1, -2)) * torch.tensor(AR.scale_f32(dh), dtype=F32)
    Nk = trunc64(N, mut)
    p = torch.zeros_like(v)
    if Nk > 0:
        vv = v[..., :Nk]
        e = torch.exp(vv - vv.max(-1, keepdim=True).values)
        p[..., :Nk] = e * (1.0 / lane_sum(e))[..., None]
    return emulate_average_probs(p, mut)


_AVG = {}


def average_case(ci, kind):
    if (ci, kind) not in _AVG:
        gh, B, H, dh = CASES[ci]
        case = AR.make_average_case(gh, B, H, dh)
        if kind == "f32":
            _AVG[(ci, kind)] = (case["probs"], *AR.average_probs_reference(case["probs"]))
        else:
            vals = RW.load(RW.store(case["qkv"], kind), kind)
            _AVG[(ci, kind)] = (vals, *AR.average_qkv_reference(vals, H))
    return _AVG[(ci, kind)]


def average_ok(ci, kind, mut=None) -> bool:
    src, ref, bound = average_case(ci, kind)
    got = emulate_average_probs(src, mut) if kind == "f32" else emulate_average_qkv(src, CASES[ci][2], mut)
    rows_ok = bool(((got.double().sum(-1) - 1.0).abs() <= bound.sum(-1) + (ref.sum(-1) - 1.0).abs()).all())
    return within(got, ref, bound) and rows_ok


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_average_f32_restatement_inside_the_bound(ci):
    gh, B, H, dh = CASES[ci]
    N = AR.tokens_of(gh)
    for kind in AR.KINDS:
        assert average_ok(ci, kind), kind
    vals, ref, _ = average_case(ci, "bf16")
    assert vals.dtype == torch.float64 and torch.equal(vals.float().double(), vals)      # the stored values are exact in f32
    assert torch.equal(RW.load(RW.store(vals, "h2"), "h2").float().double(), RW.load(RW.store(vals, "h2"), "h2"))
    if N > 2:
        assert float(ref.max(-1).values.median()) > 4.0 / N                             # far from uniform


# ---- mode='attention' enhancer ---------------------------------------------------------------------------------------------------------
def emulate_enhance(flat, A, N, D, strength, thr, mut=None):
    """attn_boost_kernel, the f32 GEMM and the pitched write-back on the flat token buffer [B, sb]: (tokens buffer, what is left in A)."""
    B, sb = flat.shape
    a = A.float().clone()
    s32, t32 = torch.tensor(strength, dtype=F32), torch.tensor(thr, dtype=F32)
    diag = torch.diagonal(a, dim1=1, dim2=2)
    boost = (t32 - diag).clamp(min=0.0) * s32
    if mut != "boost_row0":
        boost[:, 0] = 0.0
    t = a + torch.diag_embed(boost)
    Nk = trunc64(N, mut)
    ssum = lane_sum(t[..., :Nk]) if Nk > 0 else torch.zeros(B, N)
    inv = 1.0 / (ssum if mut == "no_eps" else ssum + EPS32)
    amap = a.clone()
    amap[..., :Nk] = t[..., :Nk] * inv[..., None]
    if mut != "col0_kept":
        amap[..., 0] = 0.0
    x = flat[:, :N * D].reshape(B, N, D)
    tmp = torch.matmul(amap, x).reshape(-1)
    out = flat.clone().reshape(-1)
    width = N * D if mut == "pitch" else (N - 1) * D
    tmp = torch.cat([tmp, torch.zeros(N * D)])
    for b in range(B):
        dst = b * sb + D
        n_el = min(width, out.numel() - dst)
        out[dst:dst + n_el] = tmp[b * N * D + D: b * N * D + D + n_el]
    return out.view(B, sb), amap


_ENH = {}


def enhance_case(ci, thr):
    if (ci, thr) not in _ENH:
        gh, B, H, dh = CASES[ci]
        N, D = AR.tokens_of(gh), H * dh
        case = AR.make_enhance_case(gh, B, D, AR.case_seed(gh, B, H))
        flat = torch.full((B, N * D + AR.TOKEN_PAD), SENTINEL)
        flat[:, :N * D] = case["tokens"].reshape(B, N * D)
        _ENH[(ci, thr)] = (case, flat, AR.enhance_reference(case["tokens"], case["A"], AR.f32(AR.STRENGTH), AR.f32(thr)))
    return _ENH[(ci, thr)]


def enhance_ok(ci, thr, mut=None) -> bool:
    gh, B, H, dh = CASES[ci]
    N, D = AR.tokens_of(gh), H * dh
    case, flat, ref = enhance_case(ci, thr)
    got, amap = emulate_enhance(flat, case["A"], N, D, AR.f32(AR.STRENGTH), AR.f32(thr), mut)
    tok = got[:, :N * D].reshape(B, N, D)
    return (bool((got[:, N * D:] == SENTINEL).all()) and torch.equal(tok[:, 0], case["tokens"][:, 0])
            and within(tok, ref["out"], ref["bound"]) and bool((amap[:, :, 0] == 0).all()) and within(amap, ref["amap"], ref["amap_bound"]))


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_enhance_f32_restatement_inside_the_bound(ci):
    N = AR.tokens_of(CASES[ci][0])
    for thr in AR.THRESHOLDS:
        assert enhance_ok(ci, thr), thr
        boosted = enhance_case(ci, thr)[2]["boosted"]
        if thr == 0.0:
            assert not bool(boosted.any())
        elif N > 2:
            assert bool(boosted[:, 1:].any()) and not bool(boosted[:, 1:].all()) and not bool(boosted[:, 0].any())


# ---- layer fusion --------------------------------------------------------------------------------------------------------------------------
def emulate_fusion(acc, tokens, top_k, mut=None):
    """fusion_row_diag, select_topk (f32 scores, stable order), fusion_mask_normalize_kernel with its 64-lane sum, the f32 GEMM."""
    B, N, D = tokens.shape
    k = min(top_k, N - 1)
    a = acc.float().clone()
    a_cls, a_diag = a[:, 0, :].clone(), torch.diagonal(a, dim1=1, dim2=2).clone()
    scores = a_cls[:, 1:] / (a_diag[:, 1:] + EPS32)
    idx = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :k]
    masked = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        masked[b, idx[b] + (0 if mut == "mask_off_by_one" else 1)] = True
    Nk = trunc64(N, mut)
    v = torch.where(masked[:, None, :], torch.zeros_like(a), a)
    amap = a.clone()
    ssum = lane_sum(v[..., :Nk]) if Nk > 0 else torch.zeros(B, N)
    inv = 1.0 / (ssum if mut == "no_eps" else ssum + EPS32)
    amap[..., :Nk] = v[..., :Nk] * inv[..., None]
    return a_cls, a_diag, idx, amap, torch.matmul(amap, tokens.float())


_FUS = {}


def fusion_case(ci, top_k):
    if (ci, top_k) not in _FUS:
        gh, B, H, dh = CASES[ci]
        case = AR.make_fusion_case(gh, B, H * dh, top_k, AR.case_seed(gh, B, H))
        _FUS[(ci, top_k)] = (case, AR.fusion_reference(case["acc"], case["tokens"], top_k))
    return _FUS[(ci, top_k)]


def fusion_ok(ci, top_k, mut=None) -> bool:
    case, ref = fusion_case(ci, top_k)
    a_cls, a_diag, idx, amap, out = emulate_fusion(case["acc"], case["tokens"], top_k, mut)
    cols = ref["masked"][:, None, :].expand_as(amap)
    return (torch.equal(a_cls, ref["a_cls"]) and torch.equal(a_diag, ref["a_diag"]) and torch.equal(idx, ref["idx"])
            and bool((amap[cols] == 0).all()) and within(amap, ref["amap"], ref["amap_bound"]) and within(out, ref["out"], ref["bound"]))


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_fusion_f32_restatement_inside_the_bound_and_rank_gap(ci):
    N = AR.tokens_of(CASES[ci][0])
    for top_k in AR.TOP_KS:
        case, ref = fusion_case(ci, top_k)
        assert ref["gap"] > 2.4e-7 and ref["gap"] >= AR.RANK_GAP        # the selection is determinate for every committed seed
        assert ref["idx"].shape[1] == min(top_k, N - 1)
        if N > 2:
            r = case["emptied_row"]
            assert float(ref["amap"][0, r].abs().max()) == 0.0 and float(case["acc"][0, r].sum()) > 0    # all its mass was masked
        assert fusion_ok(ci, top_k), top_k


# ---- similarity map --------------------------------------------------------------------------------------------------------------------------
def emulate_similarity(x, n, D, kind, temp, add_self, mut=None):
    """l2norm_rows (64-lane sum) into the storage `kind`, the product of the stored rows in f32, alpha, zero_diag_kernel."""
    B = x.shape[0]
    rows = x[:, 1:, :D].reshape(B * n, D)
    stored = RW.store(RW.l2norm_emulate(rows, 1e-12).view(B, n, D), kind)
    xhat = RW.load(stored, kind)
    sim = torch.matmul(xhat.float(), xhat.float().transpose(1, 2))
    if mut != "alpha_dropped":
        sim = sim * (torch.tensor(1.0, dtype=F32) / torch.tensor(temp, dtype=F32))
    if not add_self:
        sim = sim.masked_fill(torch.eye(n, dtype=torch.bool)[None], 0.0)
    return xhat, sim


def similarity_ok(n, D, kind, temp, add_self, mut=None) -> bool:
    x = AR.make_similarity_case(n, D, seed=n + D)
    xhat, sim = emulate_similarity(x, n, D, kind, temp, add_self, mut)
    y, ybound = RW.l2norm_reference(x[:, 1:, :D].double(), 1e-12, kind, 64)
    ref, bound = AR.similarity_reference(xhat, AR.f32(temp), bool(add_self), kind)
    if not add_self and not bool((torch.diagonal(bound, dim1=1, dim2=2) == 0).all()):
        return False
    return within(xhat, y, ybound) and within(sim, ref, bound)


@pytest.mark.parametrize("n,D,kind", SIM_CASES, ids=["n%d D%d %s" % c for c in SIM_CASES])
def test_similarity_f32_restatement_inside_the_bound(n, D, kind):
    for temp in AR.SIM_TEMPS:
        for add_self in (0, 1):
            assert similarity_ok(n, D, kind, temp, add_self), (temp, add_self)
    assert not similarity_ok(n, D, kind, 0.5, 1, "alpha_dropped")


def test_similarity_reference_is_the_oracle():
    x = AR.make_similarity_case(36, 64, seed=100)
    rows = x[:, 1:, :64]
    xhat = torch.nn.functional.normalize(rows.double(), dim=-1)
    for temp in AR.SIM_TEMPS:
        for add_self in (False, True):
            ref, _ = AR.similarity_reference(xhat, AR.f32(temp), add_self, "f32")
            assert float((OR.similarity_map(rows, temp, add_self).double() - ref).abs().max()) < 2e-6 / temp


# ---- the stage mutants ---------------------------------------------------------------------------------------------------------------------
def stage_index(N, B, H):
    return [(AR.tokens_of(gh), b, h) for gh, b, h, _ in CASES].index((N, B, H))


# (mutant, stage, case (N, B, H), extra = kind / threshold / top_k, why there)
STAGE_MUTATIONS = [
    ("tail_dropped", "average", (65, 1, 3), "bf16"),          # N = 65: the one tail column is never summed nor written
    ("tail_dropped", "average", (197, 3, 2), "h2"),
    ("tail_dropped", "enhance", (65, 3, 2), 0.15),
    ("tail_dropped", "enhance", (37, 1, 3), 0.15),            # N < 64: nothing is summed
    ("tail_dropped", "fusion", (325, 1, 3), 300),
    ("tail_dropped", "fusion", (197, 3, 2), 30),
    ("col0_kept", "enhance", (197, 1, 3), 0.15),
    ("col0_kept", "enhance", (2, 1, 3), 0.0),
    ("boost_row0", "enhance", (197, 3, 2), 0.15),             # A[0, 0] = 0.05 < threshold: visible in the map left in A
    ("no_eps", "enhance", (325, 1, 2), 0.0),                  # the faint row: 1e-8 is a quarter of its denominator
    ("no_eps", "fusion", (37, 1, 3), 1),                      # the emptied row: 0 / 0
    ("no_eps", "fusion", (325, 3, 2), 300),
    ("mask_off_by_one", "fusion", (65, 1, 2), 1),
    ("mask_off_by_one", "fusion", (325, 3, 3), 300),
    ("mean_h_minus_1", "average", (2, 1, 3), "f32"),
    ("mean_h_minus_1", "average", (325, 3, 2), "f16"),
    ("pitch", "enhance", (197, 3, 3), 0.15),                  # spills into the next image's CLS row and the padding
    ("pitch", "enhance", (2, 1, 2), 0.0),                     # B = 1: into the padding after the image
]


@pytest.mark.parametrize("mut,stage,shape,extra", STAGE_MUTATIONS)
def test_stage_mutants_fail(mut, stage, shape, extra):
    ci = stage_index(*shape)
    ok = {"average": lambda m: average_ok(ci, extra, m), "enhance": lambda m: enhance_ok(ci, extra, m),
          "fusion": lambda m: fusion_ok(ci, extra, m)}[stage]
    assert ok(None) and not ok(mut)


def test_case_table_has_the_tails_and_thresholds_claimed():
    Ns = [AR.tokens_of(gh) for gh in AR.GRIDS]
    assert Ns == [2, 37, 65, 197, 325]
    assert [AR.lane_tail(N) for N in Ns] == [2, 37, 1, 5, 5]            # N = 65 and 197 leave ragged 64-lane tails of 1 and 5
    assert 325 % 4 == 1 and (325 + 3) // 4 == 82                        # cdiv(N, 4) blocks, the last one with a single row
    assert min(300, 324) > 256                                          # the index-staging loop of fusion_mask_normalize iterates
    assert all(min(300, N - 1) == N - 1 for N in Ns[:4])                # top_k >= n clamps
    assert sorted({H * dh for H, dh in AR.HEADS}) == [96, 128] and AR.BATCHES == (1, 3) and AR.TOP_KS == (1, 30, 300)
    assert len(CASES) == 20 and AR.SIM_N == (36, 196, 324) and AR.SIM_D == (64, 192) and AR.SIM_TEMPS == (1.0, 0.5)
    assert all(n % 128 != 0 for n in AR.SIM_N)                          # zero_diag and the map's tiles off the tile size
