"""The attention-map stages of the vision tower, each through its raw entry, against the f64 references of tests/attnmap_reference.py,
element by element: the head-averaged attention (sg_attn_average_raw: head_mean_kernel; 2-byte modes: unpack_qk_kernel, the per-head f32
GEMM, softmax_rows, head_mean), the mode='attention' enhancer (sg_attn_enhance_raw: attn_boost_kernel, the [N, N] . [N, D] GEMM, the
pitched write-back), the layer-fusion re-weighting (sg_layer_fusion_apply_raw: fusion_row_diag, select_topk, fusion_mask_normalize, the
GEMM, the copy back) and the similarity map (sg_similarity_map: l2norm_rows, the batched aliased GEMM with alpha = 1 / temperature,
zero_diag_kernel).  The towers reach these only at N <= 37; here N = 2, 37, 65, 197, 325 (64-lane tails of 2, 37, 1, 5, 5; cdiv(N, 4)
blocks with a partial last one), B = 1 / 3, D = 96 / 128, top_k = 1 / 30 / 300 (k > 256: the index-staging loop; top_k >= n clamps).
Exact elements (column 0 of the boosted map, masked columns, the CLS row, the zeroed diagonal, padding, guard bands) are compared for
equality.  tests/test_attnmap_bound_cpu.py shows on the same cases that the bounds hold for f32 arithmetic and fail the listed slips."""
import ctypes as C
import os
import sys
from collections import defaultdict

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attnmap_reference as AR                                          # noqa: E402
from attnmap_reference import RW, check_within                          # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 1 << 16
F_SENTINEL, I_SENTINEL = -12345.5, -77
WORST = defaultdict(float)                     # (stage, case) -> largest err / bound
CASES = AR.stage_cases()
IDS = ["N%d B%d H%d dh%d" % (AR.tokens_of(gh), B, H, dh) for gh, B, H, dh in CASES]
SIM_CASES = [(n, D, kind) for n in AR.SIM_N for D in AR.SIM_D for kind in AR.KINDS]


@pytest.fixture(scope="module")
def lib():
    from clip_decontamination_amd import _lib
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(t, sentinel):
    """A device copy of the CPU tensor t with GUARD bytes of `sentinel` on each side: (whole buffer, view of the payload)."""
    g = GUARD // t.element_size()
    big = torch.full((2 * g + t.numel(),), sentinel, dtype=t.dtype, device=DEV)
    view = big[g:g + t.numel()].view(t.shape)
    view.copy_(t)
    return big, view


def guard_intact(big, numel, sentinel) -> bool:
    g = GUARD // big.element_size()
    return bool((big[:g] == sentinel).all()) and bool((big[g + numel:] == sentinel).all())


def aligned_scratch(nbytes):
    buf = torch.zeros(nbytes + 512, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 256
    return buf, C.c_void_p(buf.data_ptr() + off), off


def note(stage, case, ratio):
    WORST[(stage, case)] = max(WORST[(stage, case)], ratio)
    print(f"{stage} {case}: err/bound {ratio:.3g}")


# ---- head-averaged attention -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_average_vs_f64(lib, ci):
    gh, B, H, dh = CASES[ci]
    N, D = AR.tokens_of(gh), H * dh
    case = AR.make_average_case(gh, B, H, dh)
    for kind in AR.KINDS:
        if kind == "f32":
            src = case["probs"].to(DEV)
            ref, bound = AR.average_probs_reference(case["probs"])
            sp, nbytes = None, 0
        else:
            stored = RW.store(case["qkv"], kind)
            src = stored.to(DEV)
            ref, bound = AR.average_qkv_reference(RW.load(stored, kind), H)
            nbytes = 4 * (N * 2 * D + 2 * H * N * N) + 3 * 256
            keep, sp, _ = aligned_scratch(nbytes)
        big, out = guarded(torch.full((B, N, N), F_SENTINEL), F_SENTINEL)
        rc = lib.sg_attn_average_raw(AR.PREC[kind], P(src), B, N, D, H, sp, nbytes, P(out), stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.sg_last_error()
        assert guard_intact(big, out.numel(), F_SENTINEL)
        got = out.cpu()
        note("average " + kind, IDS[ci], check_within(got, ref, bound, f"average {kind} {IDS[ci]}"))
        rows = got.double().sum(-1)
        assert bool(((rows - 1.0).abs() <= bound.sum(-1) + (ref.sum(-1) - 1.0).abs()).all()), f"average {kind} {IDS[ci]}: a row does not sum to 1"


# ---- mode='attention' enhancer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_enhance_vs_f64(lib, ci):
    gh, B, H, dh = CASES[ci]
    N, D = AR.tokens_of(gh), H * dh
    sb = N * D + AR.TOKEN_PAD
    case = AR.make_enhance_case(gh, B, D, AR.case_seed(gh, B, H))
    flat = torch.full((B, sb), F_SENTINEL)
    flat[:, :N * D] = case["tokens"].reshape(B, N * D)
    for thr in AR.THRESHOLDS:
        ref = AR.enhance_reference(case["tokens"], case["A"], AR.f32(AR.STRENGTH), AR.f32(thr))
        if thr == 0.0:
            assert not bool(ref["boosted"].any())
        elif N > 2:
            assert bool(ref["boosted"][:, 1:].any()) and not bool(ref["boosted"][:, 1:].all())      # both fmaxf branches
        tbig, tok = guarded(flat, F_SENTINEL)
        abig, A = guarded(case["A"], F_SENTINEL)
        mbig, tmp = guarded(torch.full((B, N, D), F_SENTINEL), F_SENTINEL)
        rc = lib.sg_attn_enhance_raw(P(tok), sb, D, P(A), B, N, D, float(AR.STRENGTH), float(thr), P(tmp), stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.sg_last_error()
        assert guard_intact(tbig, tok.numel(), F_SENTINEL) and guard_intact(abig, A.numel(), F_SENTINEL) and guard_intact(mbig, tmp.numel(), F_SENTINEL)
        got = tok.cpu()
        assert bool((got[:, N * D:] == F_SENTINEL).all()), "the write-back touched the padding between images"
        got = got[:, :N * D].reshape(B, N, D)
        assert torch.equal(got[:, 0], case["tokens"][:, 0]), "the CLS row changed"
        tag = f"{IDS[ci]} thr {thr}"
        note("enhance tokens", tag, check_within(got, ref["out"], ref["bound"], f"enhance tokens {tag}"))
        amap = A.cpu()                                                   # documented as destroyed: it holds the boosted, normalised map
        assert bool((amap[:, :, 0] == 0).all()), "column 0 of the boosted map is not exactly 0"
        note("enhance map", tag, check_within(amap, ref["amap"], ref["amap_bound"], f"enhance map {tag}"))


def test_enhance_refuses_strided_rows_and_launches_nothing(lib):
    tok = torch.full((2 * 5 * 16,), F_SENTINEL, device=DEV)
    A = torch.full((2, 5, 5), F_SENTINEL, device=DEV)
    assert lib.sg_attn_enhance_raw(P(tok), 80, 12, P(A), 2, 5, 8, 0.5, 0.15, P(tok), stream()) != 0
    assert b"dense token rows" in lib.sg_last_error()
    assert lib.sg_attn_enhance_raw(P(tok), 80, 8, P(A), 0, 5, 8, 0.5, 0.15, P(tok), stream()) != 0
    torch.cuda.synchronize()
    assert bool((tok == F_SENTINEL).all()) and bool((A == F_SENTINEL).all())


# ---- layer fusion --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_fusion_apply_vs_f64(lib, ci):
    gh, B, H, dh = CASES[ci]
    N, D = AR.tokens_of(gh), H * dh
    for top_k in AR.TOP_KS:
        case = AR.make_fusion_case(gh, B, D, top_k, AR.case_seed(gh, B, H))
        ref = AR.fusion_reference(case["acc"], case["tokens"], top_k)
        assert ref["gap"] > 2.4e-7                                       # the selection is determinate (checked before any launch)
        k = ref["idx"].shape[1]
        assert k == min(top_k, N - 1)
        abig, acc = guarded(case["acc"], F_SENTINEL)
        tbig, tok = guarded(case["tokens"], F_SENTINEL)
        cbig, a_cls = guarded(torch.full((B, N), F_SENTINEL), F_SENTINEL)
        dbig, a_diag = guarded(torch.full((B, N), F_SENTINEL), F_SENTINEL)
        ibig, idx = guarded(torch.full((B, k), I_SENTINEL, dtype=torch.int32), I_SENTINEL)
        mbig, tmp = guarded(torch.full((B, N, D), F_SENTINEL), F_SENTINEL)
        rc = lib.sg_layer_fusion_apply_raw(P(acc), P(tok), B, N, D, top_k, P(a_cls), P(a_diag), P(idx), P(tmp), stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.sg_last_error()
        for big, view, s in ((abig, acc, F_SENTINEL), (tbig, tok, F_SENTINEL), (cbig, a_cls, F_SENTINEL), (dbig, a_diag, F_SENTINEL),
                             (ibig, idx, I_SENTINEL), (mbig, tmp, F_SENTINEL)):
            assert guard_intact(big, view.numel(), s)
        tag = f"{IDS[ci]} top_k {top_k}"
        assert torch.equal(a_cls.cpu(), ref["a_cls"]) and torch.equal(a_diag.cpu(), ref["a_diag"]), f"{tag}: row 0 / diagonal"
        assert torch.equal(idx.cpu().long(), ref["idx"]), f"{tag}: selected indices"
        amap = acc.cpu()
        cols = ref["masked"][:, None, :].expand(B, N, N)
        assert bool((amap[cols] == 0).all()), f"{tag}: a masked column is not exactly 0"
        note("fusion map", tag, check_within(amap, ref["amap"], ref["amap_bound"], f"fusion map {tag}"))
        note("fusion tokens", tag, check_within(tok.cpu(), ref["out"], ref["bound"], f"fusion tokens {tag}"))


# ---- similarity map --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,kind", SIM_CASES, ids=["n%d D%d %s" % c for c in SIM_CASES])
def test_similarity_map_vs_f64(lib, n, D, kind):
    B, ld = AR.SIM_B, D + 8
    x = AR.make_similarity_case(n, D, seed=n + D)
    dx = x.to(DEV)
    rows = x[:, 1:, :D].double()
    y, ybound = RW.l2norm_reference(rows, 1e-12, kind, 64)
    esz = 2 if kind in ("bf16", "f16") else 4
    nbytes = B * n * D * esz
    for temp in AR.SIM_TEMPS:
        for add_self in (0, 1):
            keep, sp, off = aligned_scratch(nbytes)
            big, sim = guarded(torch.full((B, n, n), F_SENTINEL), F_SENTINEL)
            rc = lib.sg_similarity_map(C.c_void_p(dx.data_ptr() + 4 * ld), (n + 1) * ld, ld, B, n, D, float(temp), add_self, AR.PREC[kind],
                                       P(sim), sp, nbytes, stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.sg_last_error()
            assert guard_intact(big, sim.numel(), F_SENTINEL)
            raw = keep[off:off + nbytes].cpu()
            assert bool((keep[off + nbytes:] == 0).all()), "a store landed past xhat in the scratch"
            stored = raw.view(RW.storage_dtype(kind)).view(B, n, RW.storage_cols(D, kind))
            xhat = RW.load(stored, kind)
            tag = f"n{n} D{D} T{temp} self{add_self}"
            note("similarity xhat " + kind, tag, check_within(xhat, y, ybound, f"xhat {kind} {tag}"))
            ref, bound = AR.similarity_reference(xhat, AR.f32(temp), bool(add_self), kind)
            got = sim.cpu()
            if not add_self:
                assert bool((torch.diagonal(got, dim1=1, dim2=2) == 0).all()), f"{tag}: the diagonal is not exactly 0"
            note("similarity map " + kind, tag, check_within(got, ref, bound, f"sim {kind} {tag}"))


def test_zz_worst_ratios():
    """Runs last (module order): the err / bound table of the module, the largest ratio per stage and the worst case of each."""
    stages = defaultdict(lambda: (0.0, ""))
    for (stage, case), v in WORST.items():
        if v >= stages[stage][0]:
            stages[stage] = (v, case)
    print("attention-map stages, largest err / bound per stage (worst case):")
    for stage in sorted(stages):
        print(f"  {stage:>22} | {stages[stage][1]:<32} {stages[stage][0]:.3g}")
    print("per (stage, case):")
    for key in sorted(WORST):
        print(f"  {key[0]:>22} | {key[1]:<32} {WORST[key]:.3g}")
    assert WORST and all(v <= 1.0 for v in WORST.values())
