"""The dh-64 'Experimental' last-block attention (similarity-map bias + re-softmax, attn_kernel<64, TS, 2, ..., DMA = true>) stages K / V by
LDS-DMA, fetches the map of a steady key tile with unpredicated loads and masks the key tail in the last tile only.  Tuning code 40 keeps
the register-staged body reachable in the same process; no floating-point operation differs, so the two must agree BIT FOR BIT
(torch.equal on ctx) wherever a branch of the new body can go wrong: a single tile that is first and last at once (N = 2, 63), exactly one
full tile (64), a one-key tail (65, 129, 193), a query-block boundary (128 / 129), three tiles = the steady form exactly once (193), the
real shape (1370); both workgroup orders (whole images per XCD with a ragged last group, and query-block order with H not a multiple of
4); a positive, a zero and a negative map weight (token 0's bias is +-0); data designs whose rescale branch fires on late tiles; both
2-byte operand kinds; one and two summed score terms.  ctx starts as NaN and is one row longer than N: every row < N must be written,
the extra row must not.  Accuracy against f64 stays with tests/test_gpu_attention_reference.py (exper1 / exper2)."""
import ctypes as C

import pytest
import torch

from attention_reference import make_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PREC = {"bf16": 1, "f16": 3}
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
STAGED = 40
DH = 64
ORDERS = {"images": (17, 4), "qblock": (3, 3)}               # (B, H): whole images per XCD (ragged last group) / the other order
TERMS = {"exper1": 1, "exper2": 2}


def _lib():
    from clip_decontamination_amd import _lib as L
    return L.load()


class Case:
    """Packed [B, N, (Q | K) * terms | V] operands, a symmetric f32 map [B, n, n] (the kernel reads it as bias[key][query]) and the
    log-sum-exp of a first pass (resoftmax = 0, ctx = None), as attn_generic composes the 'Experimental' block."""

    def __init__(self, lib, fmt, design, B, N, H, n_terms, seed=0):
        self.lib, self.fmt, self.B, self.N, self.H, self.n_terms = lib, fmt, B, N, H, n_terms
        D = self.D = H * DH
        Q, K, V, self.sc = make_case(design, fmt=fmt, B=B, N=N, H=H, dh=DH, n_terms=n_terms, seed=seed, device=DEV)
        self.st = st = (2 * n_terms + 1) * D + 8                  # a QKV-like token stride with a gap
        self.buf = buf = torch.zeros(B, N, st, dtype=DT[fmt], device=DEV)
        for t in range(n_terms):
            buf[..., 2 * t * D:(2 * t + 1) * D] = Q[t].reshape(B, N, D).to(DT[fmt])
            buf[..., (2 * t + 1) * D:(2 * t + 2) * D] = K[t].reshape(B, N, D).to(DT[fmt])
        buf[..., 2 * n_terms * D:(2 * n_terms + 1) * D] = V.reshape(B, N, D).to(DT[fmt])
        g = torch.Generator(device=DEV).manual_seed(seed + 7)
        m = torch.randn(B, N - 1, N - 1, generator=g, device=DEV)
        self.sim = ((m + m.transpose(-1, -2)) * 0.5).contiguous()
        if N == 1:
            self.sim = torch.zeros(B, 1, 1, device=DEV)           # an empty map, but not a null pointer
        self.lse = torch.full((B, H, N), float("nan"), dtype=torch.float32, device=DEV)
        self._launch(None, 0.0, 0, None, self.lse, None)          # first pass: the lean log-sum-exp-only kernel
        torch.cuda.synchronize()
        assert torch.isfinite(self.lse).all()

    def _launch(self, bias, bias_w, resoftmax, lse_in, lse_out, ctx):
        esz, base, D, n, N, st = self.buf.element_size(), self.buf.data_ptr(), self.D, self.n_terms, self.N, self.st
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        q = [C.c_void_p(base + 2 * t * D * esz) for t in range(n)] + [None] * (3 - n)
        k = [C.c_void_p(base + (2 * t + 1) * D * esz) for t in range(n)] + [None] * (3 - n)
        v = C.c_void_p(base + 2 * n * D * esz)
        rc = self.lib.sg_attention_raw(PREC[self.fmt], *q, *k, N * st, st, v, N * st, st, self.B, N, self.H, DH, n, int(n > 1), 0, self.sc, None,
                                       p(bias), bias_w, (N - 1) ** 2, None, None, resoftmax, p(lse_in), p(lse_out), p(ctx), (N + 1) * D, D, 1.0,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.lib.sg_last_error()

    def run(self, bias_w):
        """The 'Experimental' launch into a NaN-filled ctx of N + 1 rows; returns (ctx, body, kernel text)."""
        ctx = torch.full((self.B, self.N + 1, self.D), float("nan"), dtype=DT[self.fmt], device=DEV)
        self._launch(self.sim, bias_w, 1, self.lse, None, ctx)
        body, kern = self.lib.sg_attention_last_body().decode(), self.lib.sg_attention_last_kernel().decode()
        torch.cuda.synchronize()
        return ctx, body, kern


def check(case, bias_w, what):
    lib, N = case.lib, case.N
    new, b1, k1 = case.run(bias_w)
    again, _, _ = case.run(bias_w)
    lib.sg_set_gemm_config(STAGED)
    try:
        old, b0, k0 = case.run(bias_w)
    finally:
        lib.sg_set_gemm_config(-1)
    assert (b1, b0) == ("dma", "staged"), (what, b1, b0)
    assert k1 == k0 and f" ts={case.n_terms} gk=2 " in k1, (what, k1, k0)
    for name, c in (("dma", new), ("staged", old)):
        assert torch.isfinite(c[:, :N]).all(), f"{what}: {name} left a row < N unwritten or not finite"
        assert torch.isnan(c[:, N]).all(), f"{what}: {name} wrote row N of ctx"
    assert torch.equal(new[:, :N], again[:, :N]), f"{what}: the same launch twice differs"
    assert torch.equal(new[:, :N], old[:, :N]), f"{what}: ctx differs, max {(new[:, :N].float() - old[:, :N].float()).abs().max().item()}"


NS = [2, 63, 64, 65, 128, 129, 193, 1370]


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", list(TERMS))
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_exper_dma_body_bit_identical(fmt, kind, N, order):
    B, H = ORDERS[order]
    case = Case(_lib(), fmt, "normal", B, N, H, TERMS[kind])
    check(case, 0.8, f"{fmt} {kind} N={N} {order}")


@pytest.mark.parametrize("design", ["normal", "outlier", "stair9"])
@pytest.mark.parametrize("N", [65, 193, 1370])
@pytest.mark.parametrize("kind", list(TERMS))
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_exper_dma_body_designs_and_map_weights(fmt, kind, N, design):
    """Late-tile rescales (outlier / stair9) and the three map weights: with weight 0 or a negative one, token 0's and the masked keys'
    zero bias is -0 or +0 -- the sums it enters must not care."""
    B, H = ORDERS["qblock"] if N == 1370 else ORDERS["images"]
    case = Case(_lib(), fmt, design, B, N, H, TERMS[kind], seed=3)
    for bias_w in (0.8, 0.0, -0.5):
        check(case, bias_w, f"{fmt} {kind} {design} N={N} w={bias_w}")


def test_single_token_keeps_the_staged_body():
    """N = 1 has no similarity map to clamp the new body's edge loads into: the launch stays on the register-staged body."""
    lib = _lib()
    case = Case(lib, "bf16", "normal", 3, 1, 3, 1)
    ctx, body, _ = case.run(0.8)
    assert body == "staged" and torch.isfinite(ctx[:, :1]).all()


def test_vit_l14_experimental_tower_bit_identical():
    """ViT-L/14, model_type 'Experimental' with the similarity enhancement on, 17 tiles of 518 pixels (1370 tokens, whole images per XCD): the
    output tokens with the LDS-DMA last-block body equal those with the register-staged one bit for bit."""
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.engine import HipVisionTower, HipCLIP, SimilarityEnhancementModule
    lib = _lib()
    cfg = Wt.vit_config("ViT-L-14")
    net = HipCLIP(HipVisionTower(cfg, Wt.make_vit_weights(cfg, seed=0), precision="bf16", device=DEV))
    net.visual.similarity_enhancer = SimilarityEnhancementModule(similarity_weight=1.0, temperature=1.0, add_self_similarity=True)
    img = torch.from_numpy(Wt.normalize_tiles(Wt.make_tiles_u8(17, 518, seed=5, smooth=True))).to(DEV)
    with torch.no_grad():
        _, tok_new = net.encode_image(img, "Experimental", True, output_cls_token=True, apply_similarity_enhancement=True)
        b1, k1 = lib.sg_attention_last_body().decode(), lib.sg_attention_last_kernel().decode()
        lib.sg_set_gemm_config(STAGED)
        try:
            _, tok_old = net.encode_image(img, "Experimental", True, output_cls_token=True, apply_similarity_enhancement=True)
            b0 = lib.sg_attention_last_body().decode()
        finally:
            lib.sg_set_gemm_config(-1)
    torch.cuda.synchronize()
    assert " gk=2 " in k1 and "order=images" in k1, k1
    assert (b1, b0) == ("dma", "staged")
    assert torch.isfinite(tok_new).all()
    assert torch.equal(tok_new, tok_old)
