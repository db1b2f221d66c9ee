"""The persistent bf16 GEMM on 128-byte K steps (gemm_bf16_persist_k64, the default for K % 64 == 0, K / 64 >= 4) against the 32-element
kernel it replaced (tuning code 38) on the same seeded operands: both issue the same MFMA sequence per accumulator, so every output must
be bit-identical -- every epilogue form, both 2-byte operand types, the N-group tile order, the folded-LayerNorm chain and a whole tower."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OLD = 38                                                        # tuning code: the 32-element-K-step persistent kernel


def _lib():
    from clip_decontamination_amd import _lib as L
    return L.load()


def both(fn, kstep=64):
    """fn() under the default dispatch and under tuning code 38, in this order; the tuning code is reset whatever happens.  After each run the
    library's record of the last persistent launch must name the kernel that ran: `kstep` (64 = gemm_bf16_persist_k64) for the default, 32 under
    code 38 -- so a dispatch that quietly fell back would not compare the old kernel with itself."""
    lib = _lib()
    new = fn()
    assert lib.sg_gemm_persist_last_kstep() == kstep
    lib.sg_set_gemm_config(OLD)
    try:
        old = fn()
        assert lib.sg_gemm_persist_last_kstep() == 32
    finally:
        lib.sg_set_gemm_config(-1)
    torch.cuda.synchronize()
    return new, old


def rnd(*shape, seed, scale=1.0):
    return (torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)) * scale).to(DEV)


# M = 12 x 1370 rows: not a multiple of 256, and >= 128 output tiles at N = 1024 (fewer go to the 128 x 128 ring kernel)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("N,K", [(1024, 768), (3072, 1024), (4096, 1024), (1024, 4096), (576, 1024)])
@pytest.mark.parametrize("form", ["act0", "act1", "act2", "f32_residual"])
def test_linear_bit_identical(prec, N, K, form):
    from clip_decontamination_amd import ops
    M = 12 * 1370 if N >= 1024 else 24 * 1370                  # N = 576: three N tiles, so twice the rows for >= 128 tiles
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3, scale=0.1)
    if form == "f32_residual":
        R = rnd(M, N, seed=4)
        new, old = both(lambda: ops.linear(A, W, b, R, 0, prec))
    else:
        new, old = both(lambda: ops.linear(A, W, b, None, int(form[-1]), prec))
    assert torch.isfinite(new).all()
    assert torch.equal(new, old)


@pytest.mark.parametrize("act,cbf", [(0, 1), (1, 1), (0, 0)])
def test_raw_gemm_bit_identical(act, cbf):
    """sg_gemm_bf16_raw on caller-packed bf16 operands: 2-byte and f32 (+ residual) outputs of the QKV-like and proj-like shapes."""
    lib = _lib()
    M, N, K = 12 * 1370, 3072 if cbf else 1024, 1024 if cbf else 4096
    A, W = rnd(M, K, seed=11).bfloat16(), rnd(N, K, seed=12, scale=K ** -0.5).bfloat16()
    bias, R = rnd(N, seed=13), (None if cbf else rnd(M, N, seed=14))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def run():
        out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16 if cbf else torch.float32)
        assert lib.sg_gemm_bf16_raw(P(A), P(W), P(bias), P(R), P(out), M, N, K, act, cbf, stream) == 0, lib.sg_last_error()
        return out
    new, old = both(run)
    assert torch.equal(new, old)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_ngroup_order_bit_identical(prec):
    """M = 32 x 1370, N = 4096, K = 1024: enough M tiles per XCD for the W-panel-resident (N-group) tile order."""
    from clip_decontamination_amd import ops
    M, N, K = 32 * 1370, 4096, 1024
    A, W, b = rnd(M, K, seed=21), rnd(N, K, seed=22, scale=K ** -0.5), rnd(N, seed=23, scale=0.1)
    new, old = both(lambda: ops.linear(A, W, b, None, 1, prec))
    assert torch.equal(new, old)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("K", [192, 544])
def test_short_or_padded_k_bit_identical(prec, K):
    """K = 192 (three 64-element steps): the dispatch rule keeps the 32-element kernel under both codes (old against old, checked to be so);
    K = 544 is padded to 576 by the operand packing and runs the 128-byte kernel on the zero-padded operands."""
    from clip_decontamination_amd import ops
    M, N = 12 * 1370, 1024
    A, W, b = rnd(M, K, seed=31), rnd(N, K, seed=32, scale=K ** -0.5), rnd(N, seed=33, scale=0.1)
    new, old = both(lambda: ops.linear(A, W, b, None, 0, prec), kstep=32 if K == 192 else 64)
    assert torch.equal(new, old)


def test_raw_gemm_refuses_k_not_multiple_of_64():
    """A K with K % 64 == 32 never reaches a persistent kernel: the bf16 GEMM entry (here sg_gemm_bf16_raw, which passes K unpadded) refuses
    it before any launch, under both codes."""
    lib = _lib()
    M, N, K = 12 * 1370, 1024, 544
    A, W = rnd(M, K, seed=41).bfloat16(), rnd(N, K, seed=42).bfloat16()
    out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    for code in (-1, OLD):
        lib.sg_set_gemm_config(code)
        try:
            assert lib.sg_gemm_bf16_raw(P(A), P(W), None, None, P(out), M, N, K, 0, 1, stream) != 0
            assert b"multiple of 64" in lib.sg_last_error()
        finally:
            lib.sg_set_gemm_config(-1)


def test_refused_code_keeps_the_setting():
    """A refused tuning code (the retired tile code 5) leaves the thread's setting as it was: under code 38 the next persistent launch still
    runs the 32-element kernel."""
    lib = _lib()
    M, N, K = 12 * 1370, 1024, 1024
    A, W = rnd(M, K, seed=61).bfloat16(), rnd(N, K, seed=62, scale=K ** -0.5).bfloat16()
    out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    lib.sg_set_gemm_config(OLD)
    try:
        assert lib.sg_set_gemm_config(5) != 0
        assert b"unknown tuning code 5" in lib.sg_last_error()
        assert lib.sg_gemm_bf16_raw(P(A), P(W), None, None, P(out), M, N, K, 0, 1, stream) == 0, lib.sg_last_error()
        assert lib.sg_gemm_persist_last_kstep() == 32
    finally:
        lib.sg_set_gemm_config(-1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_batched_similarity_bit_identical(prec):
    """The blockIdx.y-batched form: the similarity map of 4 tiles (one GEMM launch, batch 4; n = 1288 rows: a multiple of 8 for the vector
    epilogue, not of 256)."""
    from clip_decontamination_amd import ops
    x = rnd(4, 1288, 1024, seed=51)
    new, old = both(lambda: ops.similarity_map(x, 0.5, True, prec))
    assert torch.isfinite(new).all()
    assert torch.equal(new, old)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("M,K1,D,N2,act", [(1370, 1024, 1024, 3072, 0), (2055, 4096, 1024, 4096, 1), (1200, 768, 768, 3072, 2),
                                          (1024, 512, 512, 512, 0), (1100, 512, 576, 640, 1)])
def test_ln_chain_folded_bit_identical(prec, M, K1, D, N2, act):
    """The folded-LayerNorm chain (producer GEMM with the 2-byte copy and slice statistics -> consumer GEMM with the per-row statistics):
    the residual stream x and the consumer's output y."""
    from clip_decontamination_amd import ops
    A, W1, b1 = rnd(M, K1, seed=1), rnd(D, K1, seed=2, scale=K1 ** -0.5), rnd(D, seed=3, scale=0.1)
    x = rnd(M, D, seed=4) * torch.logspace(-1, 1, M, device=DEV).view(M, 1)
    gamma, beta = 1.0 + 0.3 * rnd(D, seed=5), 0.2 * rnd(D, seed=6)
    W2, b2 = rnd(N2, D, seed=7, scale=D ** -0.5), rnd(N2, seed=8, scale=0.1)
    (xn, yn), (xo, yo) = both(lambda: ops.ln_chain(A, W1, b1, x, gamma, beta, W2, b2, act, prec, fold=True))
    assert torch.equal(xn, xo)
    assert torch.equal(yn, yo)


def test_tower_tile_logits_bit_identical():
    """One machine-filling ViT-L/14 bf16 launch, 119 tiles of 512 x 512 (the default bench line's tower): the patch-grid logits."""
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.engine import HipVisionTower, HipCLIP
    from clip_decontamination_amd.pipeline import SegPipeline
    cfg = Wt.vit_config("ViT-L-14")
    tower = HipVisionTower(cfg, Wt.make_vit_weights(cfg, seed=0), precision="bf16", device=DEV)
    text = torch.from_numpy(Wt.make_text_features(8, cfg.embed_dim))
    pipe = SegPipeline(HipCLIP(tower), text, torch.arange(8), model_type="SegEarth", global_debias_factor=0.0, prob_thd=0.0, bg_idx=0,
                       tiles_per_launch=119)
    scene = torch.from_numpy(Wt.make_tiles_u8(1, 1024, seed=1234, smooth=True)[0]).to(DEV)
    H, Wd = 7 * 256 + 256, 17 * 256 + 256
    scene = scene[torch.arange(H, device=DEV) % 1024][:, torch.arange(Wd, device=DEV) % 1024].contiguous()
    wins = [(y * 256, y * 256 + 512, x * 256, x * 256 + 512) for y in range(7) for x in range(17)]
    new, old = both(lambda: pipe.tile_logits(scene, wins, (512, 512)).clone())
    assert new.shape[0] == 119
    assert torch.isfinite(new).all()
    assert torch.equal(new, old)
