"""The lean dh-64 attention kernels stage K / V by LDS-DMA (attention.hip, attn_kernel<..., DMA = true>).  Tuning code 39 keeps the
register-staged body reachable in the same process; the two must agree BIT FOR BIT (torch.equal on ctx and lse) on every shape and data
design that reaches the new body: ragged key tails, the rescale branch on every tile, underflowing tiles, outlier keys, ragged last XCD
groups, both 2-byte operand kinds, two summed terms, several streams and the log-sum-exp-only pass.  The other head dims (and the generic,
'Experimental' and two-plane bodies) keep the staged body under both settings.  Then a 119-tile ViT-L/14 tower, the bench's launch."""
import ctypes as C

import pytest
import torch

from attention_reference import make_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PREC = {"bf16": 1, "f16": 3}
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
STAGED = 39


def _lib():
    from clip_decontamination_amd import _lib as L
    return L.load()


def run(lib, fmt, design, B, N, H, dh, n_terms=1, sum_scores=0, pv=True, seed=0):
    """One sg_attention_raw call on a packed [B, N, (Q | K) * terms | V] buffer; returns (ctx, lse, body)."""
    D = H * dh
    Q, K, V, sc = make_case(design, fmt=fmt, B=B, N=N, H=H, dh=dh, n_terms=n_terms, seed=seed, device=DEV)
    st = (2 * n_terms + 1) * D + 8                                # a QKV-like token stride with a gap
    buf = torch.zeros(B, N, st, dtype=DT[fmt], device=DEV)
    for t in range(n_terms):
        buf[..., 2 * t * D:(2 * t + 1) * D] = Q[t].reshape(B, N, D).to(DT[fmt])
        buf[..., (2 * t + 1) * D:(2 * t + 2) * D] = K[t].reshape(B, N, D).to(DT[fmt])
    buf[..., 2 * n_terms * D:(2 * n_terms + 1) * D] = V.reshape(B, N, D).to(DT[fmt])
    esz = buf.element_size()
    base = buf.data_ptr()
    q = [C.c_void_p(base + 2 * t * D * esz) for t in range(n_terms)] + [None] * (3 - n_terms)
    k = [C.c_void_p(base + (2 * t + 1) * D * esz) for t in range(n_terms)] + [None] * (3 - n_terms)
    v = C.c_void_p(base + 2 * n_terms * D * esz)
    ctx = torch.full((B, N, D), float("nan"), dtype=DT[fmt], device=DEV) if pv else None
    lse = torch.full((B, H, N), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.sg_attention_raw(PREC[fmt], *q, *k, N * st, st, v, N * st, st, B, N, H, dh, n_terms, sum_scores, 0, sc, None, None, 0.0, 0,
                              None, None, 0, None, C.c_void_p(lse.data_ptr()), C.c_void_p(ctx.data_ptr()) if pv else None, N * D, D, 1.0,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.sg_last_error()
    body = lib.sg_attention_last_body().decode()
    torch.cuda.synchronize()
    return ctx, lse, body


def both(fmt, design, **kw):
    lib = _lib()
    new = run(lib, fmt, design, **kw)
    lib.sg_set_gemm_config(STAGED)
    try:
        old = run(lib, fmt, design, **kw)
    finally:
        lib.sg_set_gemm_config(-1)
    return new, old


CASES = [(design, N, B, H) for design, N, B, H in [
    ("normal", 1, 1, 2), ("normal", 63, 3, 3), ("normal", 64, 1, 2), ("normal", 65, 5, 2), ("normal", 129, 2, 7), ("normal", 1370, 3, 16),
    ("stair9", 1370, 1, 5), ("stair9", 4097, 1, 1), ("underflow", 4097, 1, 1), ("underflow", 129, 3, 3), ("outlier", 1370, 2, 3),
    ("outlier", 65, 9, 1), ("stair8", 257, 1, 2), ("equal", 129, 1, 2)]]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("design,N,B,H", CASES, ids=[f"{d}-N{n}-B{b}-H{h}" for d, n, b, h in CASES])
def test_dma_body_bit_identical(fmt, design, N, B, H):
    (c1, l1, b1), (c0, l0, b0) = both(fmt, design, B=B, N=N, H=H, dh=64)
    assert (b1, b0) == ("dma", "staged")
    assert torch.equal(c1, c0), f"ctx differs: max {(c1.float() - c0.float()).abs().max().item()}"
    assert torch.equal(l1, l0), f"lse differs: max {(l1 - l0).abs().max().item()}"


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["multi", "sum2", "lse", "sum2_lse"])
def test_dma_body_other_lean_forms(fmt, kind):
    kw = dict(multi=dict(n_terms=3), sum2=dict(n_terms=2, sum_scores=1), lse=dict(pv=False), sum2_lse=dict(n_terms=2, sum_scores=1, pv=False))[kind]
    for design, N in (("stair9", 1370), ("normal", 65)):
        (c1, l1, b1), (c0, l0, b0) = both(fmt, design, B=3, N=N, H=3, dh=64, **kw)
        assert (b1, b0) == ("dma", "staged")
        assert torch.equal(l1, l0)
        if c1 is not None:
            assert torch.equal(c1, c0)


@pytest.mark.parametrize("dh", [32, 80, 128])
def test_other_head_dims_keep_the_staged_body(dh):
    (c1, l1, b1), (c0, l0, b0) = both("bf16", "stair9", B=2, N=129, H=3, dh=dh)
    assert (b1, b0) == ("staged", "staged")
    assert torch.equal(c1, c0) and torch.equal(l1, l0)


def test_vit_l14_tower_bit_identical():
    """The bench's launch: ViT-L/14, 119 tiles of 512 pixels in one tower call, bf16 -- the tower output with the LDS-DMA body equals the
    register-staged one bit for bit."""
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.engine import HipVisionTower, HipCLIP
    lib = _lib()
    cfg = Wt.vit_config("ViT-L-14")
    net = HipCLIP(HipVisionTower(cfg, Wt.make_vit_weights(cfg, seed=0), precision="bf16", device=DEV))
    img = torch.from_numpy(Wt.normalize_tiles(Wt.make_tiles_u8(119, 512, seed=5, smooth=True))).to(DEV)
    with torch.no_grad():
        _, tok_new = net.encode_image(img, "SegEarth", True, output_cls_token=True)
        lib.sg_set_gemm_config(STAGED)
        try:
            _, tok_old = net.encode_image(img, "SegEarth", True, output_cls_token=True)
        finally:
            lib.sg_set_gemm_config(-1)
    torch.cuda.synchronize()
    assert torch.isfinite(tok_new).all()
    assert torch.equal(tok_new, tok_old)
