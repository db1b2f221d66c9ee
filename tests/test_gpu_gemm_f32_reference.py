"""The parity-mode f32 GEMM (csrc/gemm_f32.hip) in every form it has, through sg_gemm_f32_raw, against the f64 reference of
tests/attnmap_reference.py, element by element: both B layouts (the [N, K] loader and the b_n_fast [K, N] one), lda > K, ldc > N,
two-level batching with six unrelated strides, alpha 1 / 0.37 / -2, every epilogue, K below / beside / across the 16-wide K step, tiles
ragged both ways; the aliased A == B form of the similarity map and the [N, N] . [N, D] form of the enhancer and the layer fusion at
N = 197.  C is pre-filled with a sentinel inside guard bands: every element the form does not address must keep it.
tests/test_attnmap_bound_cpu.py shows on the same table that the bounds hold for f32 arithmetic and fail the listed slips."""
import ctypes as C
import os
import sys
from collections import defaultdict

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attnmap_reference as AR                                          # noqa: E402
from attnmap_reference import check_within                              # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 1 << 14                                # elements of sentinel on each side of C
WORST = defaultdict(float)                     # (form, epilogue) -> largest err / bound
CASES = AR.gemm_cases()


@pytest.fixture(scope="module")
def lib():
    from clip_decontamination_amd import _lib
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, A, B, bias, R, Cv, g):
    return lib.sg_gemm_f32_raw(P(A), g["lda"], g["sAo"], g["sAi"], P(B), g["sbk"], g["sbn"], g["sBo"], g["sBi"], P(bias), P(R), g["ldr"],
                               P(Cv), g["ldc"], g["sCo"], g["sCi"], g["M"], g["N"], g["K"], g["batch"], g["inner"], g["act"],
                               float(g["alpha"]), stream())


def guarded_c(numel):
    big = torch.full((numel + 2 * GUARD,), AR.GEMM_SENTINEL, dtype=torch.float32, device=DEV)
    return big, big[GUARD:GUARD + numel]


def run_form(lib, g, A, B, bias, R, Cbuf, acc, S, what):
    """One launch of the form g on device copies of the flat buffers; every addressed element within its bound, the rest of C and the
    guard bands still the sentinel.  Returns the largest err / bound."""
    _, _, ic, ir = AR.gemm_indices(g)
    big, view = guarded_c(Cbuf.numel())
    rc = call(lib, A, B, bias, R, view, g)
    torch.cuda.synchronize()
    assert rc == 0, lib.sg_last_error()
    whole = big.cpu()
    got = whole[GUARD:GUARD + Cbuf.numel()]
    ref, bound = AR.gemm_epilogue_reference(acc, S, g["K"], AR.f32(g["alpha"]), None if bias is None else bias.cpu(),
                                            None if R is None else R.cpu().reshape(-1)[ir], g["act"])
    ratio = check_within(got[ic], ref, bound, what)
    rest = torch.ones(whole.numel(), dtype=torch.bool)
    rest[GUARD + ic.reshape(-1)] = False
    assert bool((whole[rest] == AR.GEMM_SENTINEL).all()), f"{what}: a store landed outside C's elements (padding columns, gaps or guard bands)"
    return ratio


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c[0] for c in CASES])
def test_strided_batched_forms_vs_f64(lib, ci):
    tag, M, N, K, layout = CASES[ci]
    g = AR.gemm_form(M, N, K, layout)
    A, B, bias, R, Cbuf = AR.make_gemm_buffers(g, ci)
    acc, S = AR.gemm_products(A, B, g)                                  # shared by the six epilogues
    dA, dB, dbias, dR = A.to(DEV), B.to(DEV), bias.to(DEV), R.to(DEV)
    for ei, (name, has_bias, act, has_res) in enumerate(AR.GEMM_EPILOGUES):
        gg = dict(g, act=act, alpha=AR.alpha_of(ci, ei))
        ratio = run_form(lib, gg, dA, dB, dbias if has_bias else None, dR if has_res else None, Cbuf, acc, S, f"{tag} {name} alpha {gg['alpha']}")
        WORST[(layout, name)] = max(WORST[(layout, name)], ratio)
        print(f"gemm_f32 {tag} {name} alpha {gg['alpha']}: err/bound {ratio:.3g}")


@pytest.mark.parametrize("alpha", AR.GEMM_ALPHAS)
def test_aliased_operands_vs_f64(lib, alpha):
    """similarity_from_xhat's form: A and B are one buffer."""
    g = dict(AR.aliased_form(), alpha=alpha)
    X = torch.randn(g["batch"] * g["M"] * g["K"], generator=torch.Generator().manual_seed(7100))
    acc, S = AR.gemm_products(X, X, g)
    dX = X.to(DEV)
    Cbuf = torch.empty(g["batch"] * g["M"] * g["N"])
    ratio = run_form(lib, g, dX, dX, None, None, Cbuf, acc, S, f"aliased alpha {alpha}")
    WORST[("aliased", f"alpha {alpha}")] = ratio
    print(f"gemm_f32 aliased A == B alpha {alpha}: err/bound {ratio:.3g}")


def test_map_times_tokens_form_vs_f64(lib):
    """[N, N] . [N, D] at N = 197, D = 64, batch 2: K crosses 12 full steps and a ragged one on the b_n_fast loader."""
    g = AR.reweight_form()
    gen = torch.Generator().manual_seed(7200)
    A = torch.softmax(3.0 * torch.randn(g["batch"], g["M"], g["K"], generator=gen), -1).reshape(-1)
    X = AR.decade_rows(gen, g["batch"], g["K"], g["N"]).reshape(-1)
    acc, S = AR.gemm_products(A, X, g)
    Cbuf = torch.empty(g["batch"] * g["M"] * g["N"])
    ratio = run_form(lib, g, A.to(DEV), X.to(DEV), None, None, Cbuf, acc, S, "map . tokens")
    WORST[("map . tokens", "N 197 D 64")] = ratio
    print(f"gemm_f32 [N,N].[N,D] N 197 D 64: err/bound {ratio:.3g}")


def test_refusals_launch_nothing(lib):
    g = AR.gemm_form(5, 7, 9, "kn", batch=2, inner=1)
    A, B, bias, R, Cbuf = AR.make_gemm_buffers(g, 99)
    dA, dB = A.to(DEV), B.to(DEV)
    big, view = guarded_c(Cbuf.numel())
    for field in ("M", "N", "K", "batch", "inner"):
        for bad in (0, -1):
            assert call(lib, dA, dB, None, None, view, dict(g, **{field: bad})) != 0, (field, bad)
            assert b"gemm_f32" in lib.sg_last_error()
    assert call(lib, None, dB, None, None, view, g) != 0 and call(lib, dA, None, None, None, view, g) != 0
    assert call(lib, dA, dB, None, None, None, g) != 0
    torch.cuda.synchronize()
    assert bool((big == AR.GEMM_SENTINEL).all())


def test_zz_worst_ratios():
    """Runs last (module order): the err / bound table of the module."""
    print("f32 GEMM, largest err / bound per (form, epilogue):")
    for key in sorted(WORST):
        print(f"  {key[0]:>14} | {key[1]:<16} {WORST[key]:.3g}")
    assert WORST and all(v <= 1.0 for v in WORST.values())
