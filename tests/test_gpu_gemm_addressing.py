"""Address generation of the persistent GEMM on 128-byte K steps (gemm_bf16_persist_k64): ring positions kept as rotating state, piece
offsets formed once per output tile, fragment reads from per-lane bases.  Every case runs the default dispatch and tuning code 38 (the
32-element-K-step kernel, which issues the same MFMA sequence per accumulator) on the same seeded operands and asks for equal bits.  The
shapes sit where such state can go wrong: workgroups that run a second tile from a ring position other than 0, tiles without a steady K
step, K-step counts that are no multiple of 2 or 3, clamped edge rows with a 64-column last N tile, blockIdx.y batching, the N-group tile
order, and the folded-LayerNorm chain (producer and consumer epilogues, 2-byte copy, statistics).
The two-plane f16 and fp8 kernels run the same body and share this addressing; they have no bit-identical sibling kernel and stay bounded
element by element by the f64 references of test_gpu_gemm_reference.py / test_gpu_gemm_fp8_reference.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OLD = 38                                                        # tuning code: the 32-element-K-step persistent kernel
PREC = {"bf16": 1, "f16": 3}                                    # SG_PREC_BF16 / SG_PREC_F16
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _lib():
    from clip_decontamination_amd import _lib as L
    return L.load()


def both(fn):
    """fn() under the default dispatch and under tuning code 38; each run must have launched the kernel it is meant to test."""
    lib = _lib()
    new = fn()
    assert lib.sg_gemm_persist_last_kstep() == 64
    lib.sg_set_gemm_config(OLD)
    try:
        old = fn()
        assert lib.sg_gemm_persist_last_kstep() == 32
    finally:
        lib.sg_set_gemm_config(-1)
    torch.cuda.synchronize()
    return new, old


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * scale


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def raw(prec, A, W, bias, R, M, N, K, batch, act, packed):
    """One GEMM on caller-packed operands: sg_gemm_bf16_raw for single bf16 problems, sg_gemm_raw otherwise."""
    lib = _lib()
    lead = (batch,) if batch > 1 else ()
    out = torch.empty(*lead, M, N, device=DEV, dtype=DT[prec] if packed else torch.float32)
    if prec == "bf16" and batch == 1:
        rc = lib.sg_gemm_bf16_raw(ptr(A), ptr(W), ptr(bias), ptr(R), ptr(out), M, N, K, act, int(packed), stream())
    else:
        rc = lib.sg_gemm_raw(PREC[prec], ptr(A), ptr(W), ptr(bias), ptr(R), ptr(out), M, N, K, batch, act, int(packed), stream())
    assert rc == 0, lib.sg_last_error()
    return out


# 17 x 16 = 272 output tiles: more than the workgroups of the grid (one per CU, 256), so some workgroups run two tiles and enter the second
# one at ring position s = K / 64.  K / 64 = 4 (no steady step), 5, 7, 13 (steps not a multiple of 2 or 3).
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("K,form", [(256, "act1"), (320, "f32_residual"), (448, "act0"), (832, "act2")])
def test_ring_state_across_tiles(prec, K, form):
    from clip_decontamination_amd import ops
    M, N = 4315, 4096
    assert (M + 255) // 256 * (N // 256) > n_cu()
    A, W, b = rnd(M, K, seed=K), rnd(N, K, seed=K + 1, scale=K ** -0.5), rnd(N, seed=K + 2, scale=0.1)
    if form == "f32_residual":
        R = rnd(M, N, seed=K + 3)
        new, old = both(lambda: ops.linear(A, W, b, R, 0, prec))
    else:
        new, old = both(lambda: ops.linear(A, W, b, None, int(form[-1]), prec))
    assert torch.isfinite(new).all()
    assert torch.equal(new, old)


# Rows past M re-read row M - 1 (one row / all but one row of the last M tile are real); N = 576: three N tiles, the last 64 columns wide.
# A single problem reaches the persistent kernel from 2 x tiles >= CUs on, so M is the smallest value with that many 256-row tiles.
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("rem", [1, 255])
@pytest.mark.parametrize("packed", [True, False])
def test_clamped_rows(prec, rem, packed):
    N, K = 576, 448
    tiles_m = max(5, (n_cu() + 5) // 6)                            # 2 x (tiles_m x 3) >= CUs; 1025 / 1279 rows where that already suffices
    M = (tiles_m - 1) * 256 + rem
    A, W = rnd(M, K, seed=71 + rem).to(DT[prec]), rnd(N, K, seed=72 + rem, scale=K ** -0.5).to(DT[prec])
    bias, R = rnd(N, seed=73, scale=0.1), (None if packed else rnd(M, N, seed=74))
    new, old = both(lambda: raw(prec, A, W, bias, R, M, N, K, 1, 1 if packed else 0, packed))
    assert torch.isfinite(new.float()).all()
    assert torch.equal(new, old)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("packed", [True, False])
def test_batched(prec, packed):
    """blockIdx.y batching: three problems per launch, per-problem operand and output strides."""
    B, M, N, K = 3, 4315, 1024, 320
    A, W = rnd(B, M, K, seed=81).to(DT[prec]), rnd(B, N, K, seed=82, scale=K ** -0.5).to(DT[prec])
    bias, R = rnd(N, seed=83, scale=0.1), (None if packed else rnd(B, M, N, seed=84))
    new, old = both(lambda: raw(prec, A, W, bias, R, M, N, K, B, 0, packed))
    assert torch.isfinite(new.float()).all()
    assert torch.equal(new, old)
    assert not torch.equal(new[0], new[1])


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_ngroup_order(prec):
    """M = N = 4096, K = 1024: 256 tiles on 256 workgroups under the N-group tile order."""
    from clip_decontamination_amd import ops
    M, N, K = 4096, 4096, 1024
    A, W, b = rnd(M, K, seed=91), rnd(N, K, seed=92, scale=K ** -0.5), rnd(N, seed=93, scale=0.1)
    new, old = both(lambda: ops.linear(A, W, b, None, 1, prec))
    if n_cu() == 256:
        assert _lib().sg_gemm_last_kernel().decode().endswith("ngroup=6")
    assert torch.equal(new, old)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_folded_chain(prec):
    """sg_op_ln_chain with fold = 1: the residual stream x (producer epilogue: f32 + residual, 2-byte copy, slice statistics) and the
    consumer's output y."""
    from clip_decontamination_amd import ops
    M, K1, D, N2, act = 4315, 1024, 1024, 4096, 1
    A, W1, b1 = rnd(M, K1, seed=101), rnd(D, K1, seed=102, scale=K1 ** -0.5), rnd(D, seed=103, scale=0.1)
    x = rnd(M, D, seed=104) * torch.logspace(-1, 1, M, device=DEV).view(M, 1)
    gamma, beta = 1.0 + 0.3 * rnd(D, seed=105), 0.2 * rnd(D, seed=106)
    W2, b2 = rnd(N2, D, seed=107, scale=D ** -0.5), rnd(N2, seed=108, scale=0.1)
    (xn, yn), (xo, yo) = both(lambda: ops.ln_chain(A, W1, b1, x, gamma, beta, W2, b2, act, prec, fold=True))
    assert torch.isfinite(yn).all()
    assert torch.equal(xn, xo)
    assert torch.equal(yn, yo)
