"""The token refiners of csrc/refine.hip (top-k selection, outlier suppression, weak-token replacement, cross-tile fusion) against the
f64 references of tests/refine_reference.py, element by element: selected indices exact, untouched cells bit-identical, written cells
within a bound built from the operand magnitudes, a 64 KiB guard band on each side of the buffers the kernels write.  The cases take
the branches the fixture tests leave out: non-square and degenerate grids, the 256-strides of select / compute / scatter, nearly every
cell contested, rows two decades apart, sigma clamped at 0 and at 1, the fusion's strip-length cap with its opted-in LDS.
tests/test_refine_bound_cpu.py shows on the same generators that the bounds hold for f32 arithmetic and fail the listed mutations."""
import ctypes as C
import os
import sys
from collections import defaultdict

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_reference as R                                            # noqa: E402
from refine_reference import check_within                               # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 1 << 16
F_SENTINEL, I_SENTINEL = -12345.5, -77
TEMPS = (0.1, 5.0)
STRENGTHS = (0.3, 1.0)
WORST = defaultdict(float)                    # (op, case) -> largest err / bound


@pytest.fixture(scope="module")
def ops():
    from clip_decontamination_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from clip_decontamination_amd import _lib
    return _lib.load()


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


def P(t):
    return C.c_void_p(t.data_ptr())


def run_refiner(ops, lib, weak, case, gh, gw, k, temp):
    """The op through ops.*, then once more through the C ABI on guarded buffers: same bits, guard bands unchanged."""
    feats, a_cls, a_diag = case["feats"].to(DEV), case["a_cls"].to(DEV), case["a_diag"].to(DEV)
    if weak:
        out, idx = ops.weak_token_replace(feats, a_diag, gh, gw, k)
    else:
        out, idx = ops.outlier_suppress(feats, a_cls, a_diag, gh, gw, k, temp)
    B, n, D = feats.shape
    fbig, fview = guarded(case["feats"], F_SENTINEL)
    ibig, iview = guarded(torch.zeros(B, k, dtype=torch.int32), I_SENTINEL)
    sp, _ = ops._aligned(ops.scratch(lib.sg_outlier_scratch_bytes(B, D, k), DEV))
    if weak:
        rc = lib.sg_weak_token_replace(P(fview), P(a_diag), B, gh, gw, D, k, P(iview), sp, ops.stream_ptr())
    else:
        rc = lib.sg_outlier_suppress(P(fview), P(a_cls), P(a_diag), B, gh, gw, D, k, float(temp), P(iview), sp, ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.sg_last_error()
    assert torch.equal(fview, out) and torch.equal(iview, idx)
    assert guard_intact(fbig, fview.numel(), F_SENTINEL) and guard_intact(ibig, iview.numel(), I_SENTINEL)
    return out.cpu(), idx.cpu()


def check_refiner(ops, lib, weak, case, shape, tag):
    B, gh, gw, D, k = shape
    name = "weak_token_replace" if weak else "outlier_suppress"
    scores = R.selection_scores(case["a_cls"], case["a_diag"], weak)
    assert R.rank_gap(scores, k) >= R.RANK_GAP                           # checked on the CPU before any launch
    for temp in (TEMPS[:1] if weak else TEMPS):
        ref = R.neighbour_refine_reference(case["feats"], case["idx"], gh, gw, R.f32(temp), not weak)
        written = ref["kind"] > 0
        untouched = int((~written).sum())
        assert untouched >= 1 or (gh, gw) == R.CONTESTED_GRID
        out, idx = run_refiner(ops, lib, weak, case, gh, gw, k, temp)
        assert torch.equal(idx.long(), case["idx"]), f"{name} {tag}: selected indices"
        assert torch.equal(out[~written], case["feats"][~written]), f"{name} {tag}: an untouched cell changed"
        ratio = check_within(out[written], ref["out"][written], ref["bound"][written], f"{name} {tag} temp {temp}")
        key = (name, f"{tag} temp {temp}" if not weak else tag)
        WORST[key] = max(WORST[key], ratio)
        print(f"{name} {tag} temp {temp}: {untouched} untouched cells, err/bound {ratio:.3g}")


@pytest.mark.parametrize("weak", [False, True], ids=["outlier", "weak"])
@pytest.mark.parametrize("ci", range(len(R.REFINE_CASES)))
def test_refiners_vs_f64(ops, lib, ci, weak):
    shape = R.REFINE_CASES[ci]
    check_refiner(ops, lib, weak, R.make_refine_case(*shape, weak, seed=ci), shape, "B%d %dx%d D%d k%d" % shape)


@pytest.mark.parametrize("weak", [False, True], ids=["outlier", "weak"])
def test_refiners_exact_ties_straddling_rank_k(ops, lib, weak):
    """Four exactly equal scores on ranks k - 2 .. k + 1: the two lowest indices are selected, lowest first."""
    case = R.make_tie_case(weak, seed=7)
    k = case["shape"][4]
    assert case["idx"][0, k - 2:].tolist() == case["tied"][:2]
    check_refiner(ops, lib, weak, case, case["shape"], "ties")


# ---- cross-tile fusion -------------------------------------------------------------------------------------------------------------
def run_fusion(ops, lib, tok, hg, wg, gh, gw, bw, mode, strength):
    out = ops.cross_tile_fusion(tok.to(DEV), hg, wg, gh, gw, bw, mode, strength)
    T, n, Cc = tok.shape
    big, view = guarded(tok, F_SENTINEL)
    sp, _ = ops._aligned(ops.scratch(lib.sg_cross_tile_scratch_bytes(T, gh, gw, Cc, bw), DEV))
    rc = lib.sg_cross_tile_fusion(P(view), hg, wg, gh, gw, Cc, bw, 0 if mode == "weighted" else 1, float(strength), sp, ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.sg_last_error()
    assert torch.equal(view, out) and guard_intact(big, view.numel(), F_SENTINEL)
    return out.cpu()


@pytest.mark.parametrize("mode", ["weighted", "attention"])
@pytest.mark.parametrize("ci", range(len(R.FUSION_CASES)))
def test_cross_tile_fusion_vs_f64(ops, lib, ci, mode):
    hg, wg, gh, gw, bw, Cc = R.FUSION_CASES[ci]
    tok = R.make_fusion_case(hg, wg, gh, gw, Cc, seed=ci)
    tag = f"{hg}x{wg} tiles {gh}x{gw} bw{bw} C{Cc}"
    for strength in STRENGTHS:
        out = run_fusion(ops, lib, tok, hg, wg, gh, gw, bw, mode, strength)
        # the top pass is held on the operands it consumed: the left results are columns [0, bw) of the output (refine_reference)
        ref = R.cross_tile_reference(tok, hg, wg, gh, gw, bw, mode, R.f32(strength), final_left=out)
        st = ref["strip"]
        assert torch.equal(out[~st], tok[~st]), f"{mode} {tag}: a row outside the strips changed"
        if hg * wg == 1:
            assert not bool(st.any()) and torch.equal(out, tok)
            continue
        assert bool(st.any())
        ratio = check_within(out[st], ref["out"][st], ref["bound"][st], f"{mode} {tag} strength {strength}")
        WORST[(f"cross_tile_fusion {mode}", f"{tag} s{strength}")] = ratio
        print(f"cross_tile_fusion {mode} {tag} strength {strength}: err/bound {ratio:.3g}")


@pytest.mark.parametrize("mode", ["weighted", "attention"])
@pytest.mark.parametrize("ci", [0, 1])
def test_cross_tile_steps_split_over_ranks_equal_the_single_call(ops, ci, mode):
    """pack / fuse / apply driven as ranks holding uneven runs of tiles (strips concatenated instead of all-gathered) on the two
    non-square 2-D scenes: bit-identical to sg_cross_tile_fusion."""
    hg, wg, gh, gw, bw, Cc = R.FUSION_CASES[ci]
    tok = R.make_fusion_case(hg, wg, gh, gw, Cc, seed=ci).to(DEV)
    T = hg * wg
    whole = ops.cross_tile_fusion(tok, hg, wg, gh, gw, bw, mode, 0.3)
    for parts in ([(0, 1), (1, 4), (4, T)], [(0, 4), (4, T)], [(t, t + 1) for t in range(T)]):
        steps = ops.CrossTileSteps(gh, gw, Cc, bw, mode, 0.3, wg)
        local = [tok[a:b].clone() for a, b in parts]
        right = torch.cat([steps.pack(x, a, 0) for x, (a, _) in zip(local, parts)], 0)
        left = [steps.fuse(x, a, right, 0) for x, (a, _) in zip(local, parts)]
        bottom = torch.cat([steps.pack(x, a, 1, lf) for x, (a, _), lf in zip(local, parts, left)], 0)
        top = [steps.fuse(x, a, bottom, 1) for x, (a, _) in zip(local, parts)]
        out = torch.cat([steps.apply(x, a, lf, tp) for x, (a, _), lf, tp in zip(local, parts, left, top)], 0)
        assert torch.equal(out, whole), parts


def test_cross_tile_fusion_rejects_long_strips_and_small_grids(ops):
    tok = torch.zeros(2, 43 * 6, 4, device=DEV)
    with pytest.raises(RuntimeError, match="strips longer than 128"):
        ops.cross_tile_fusion(tok, 1, 2, 43, 6, 3, "weighted", 0.3)          # gh bw = 129
    tok = torch.zeros(2, 3 * 8, 4, device=DEV)
    with pytest.raises(RuntimeError, match="too small for boundary width"):
        ops.cross_tile_fusion(tok, 1, 2, 3, 8, 2, "weighted", 0.3)           # gh < 2 bw


def test_zz_worst_ratios():
    """Runs last (module order): the err / bound table of the module."""
    print("refiners and fusion, largest err / bound per (op, case):")
    for key in sorted(WORST):
        print(f"  {key[0]:>28} | {key[1]:<40} {WORST[key]:.3g}")
    assert all(v <= 1.0 for v in WORST.values())
