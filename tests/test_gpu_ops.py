"""GPU parity of the building-block HIP ops, each called through the C ABI, against a plain
torch fp32 reference of the same op (or the oracle restatement where the op is path-specific).

Tolerances: SG_PREC_F32 runs on the f32 MFMA (exact fmaf chains) -> 2e-4 absolute on O(1) data;
SG_PREC_BF16 rounds operands to bf16 (8 significant bits, f32 accumulate) -> 3e-2 of the output
scale for GEMM-shaped ops."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import refine as OR, jbu as OJ, segment as OS   # noqa: E402  (checker only)


@pytest.fixture(scope="module")
def ops():
    from clip_decontamination_amd import ops as o
    return o


DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


@pytest.mark.parametrize("M,N,K", [(197, 192, 192), (64, 64, 64), (130, 260, 588), (2740, 3072, 1024), (1370, 1024, 4096), (33, 7, 50)])
@pytest.mark.parametrize("prec,tol", [("f32", 2e-5), ("f16x2", 2e-5), ("bf16", 2e-2), ("f16", 3e-3)])
def test_linear(ops, M, N, K, prec, tol):
    A, W, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3, scale=0.1), rnd(M, N, seed=4)
    for act in (0, 1, 2):
        ref = A @ W.T + b
        if act == 1:
            ref = ref * torch.sigmoid(1.702 * ref)
        elif act == 2:
            ref = torch.nn.functional.gelu(ref)
        ref = ref + r
        out = ops.linear(A.to(DEV), W.to(DEV), b.to(DEV), r.to(DEV), act=act, precision=prec)
        assert rel_err(out, ref) < tol, (M, N, K, act, rel_err(out, ref))
    out = ops.linear(A.to(DEV), W.to(DEV), None, None, act=0, precision=prec)
    assert rel_err(out, A @ W.T) < tol


def test_linear_identity_asymmetric(ops):
    """A = I against an asymmetric W catches a transposed fragment / C layout (guide §3)."""
    n = 128
    W = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 251) / 251.0
    out = ops.linear(torch.eye(n).to(DEV), W.to(DEV), precision="bf16")
    assert rel_err(out, W.T.bfloat16().float()) < 1e-6
    out = ops.linear(torch.eye(n).to(DEV), W.to(DEV), precision="f16")
    assert rel_err(out, W.T.half().float()) < 1e-6
    out = ops.linear(torch.eye(n).to(DEV), W.to(DEV), precision="f32")
    assert rel_err(out, W.T) < 1e-6
    out = ops.linear(torch.eye(n).to(DEV), W.to(DEV), precision="f16x2")          # two planes: 22 significant bits of W survive
    assert rel_err(out, W.T) < 1e-6


@pytest.mark.parametrize("rows,D", [(5, 64), (197, 768), (1370, 1024), (3, 1280)])
def test_layernorm(ops, rows, D):
    x, g, b = rnd(rows, D, seed=5, scale=3.0) + 0.5, rnd(D, seed=6) * 0.1 + 1, rnd(D, seed=7) * 0.1
    ref = torch.nn.functional.layer_norm(x, (D,), g, b, 1e-5)
    out = ops.layernorm(x.to(DEV), g.to(DEV), b.to(DEV))
    assert (out.cpu() - ref).abs().max().item() < 1e-5


def attention_reference(qkv, H, variant, sim=None, w=1.0):
    B, N, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = [t.view(B, N, H, dh).permute(0, 2, 1, 3) for t in qkv.chunk(3, -1)]
    scale = dh ** -0.5

    def bias(s):
        if sim is None:
            return s
        pad = torch.zeros(B, 1, N, N)
        pad[:, 0, 1:, 1:] = sim
        return s + w * pad

    ss = lambda t: (t @ t.transpose(-1, -2)) * scale
    if variant == "vanilla":
        a = torch.softmax(bias((q @ k.transpose(-1, -2)) * scale), -1)
    elif variant == "ClearCLIP":
        a = torch.softmax(bias(ss(q)), -1)
    elif variant == "SCLIP":
        a = torch.softmax(bias(ss(q)), -1) + torch.softmax(bias(ss(k)), -1)
    elif variant == "SegEarth":
        a = torch.softmax(bias(ss(q)), -1) + torch.softmax(bias(ss(k)), -1) + torch.softmax(bias(ss(v)), -1)
    elif variant == "SFP":
        a = torch.softmax(bias(0.5 * (ss(q) + ss(k))), -1)
    elif variant == "Experimental":
        a = torch.softmax(bias(torch.softmax(ss(k) + ss(q), -1)), -1)
    elif variant in ("NACLIP", "NOnly", "GAV"):
        from oracle.vit import gaussian_bias
        g = int(round((N - 1) ** 0.5))
        omega = gaussian_bias(g, g)[None, None]
        if variant == "NACLIP":
            sco = ss(k)
        else:
            omega = omega * scale * (q.norm(dim=-1).unsqueeze(-1) * k.norm(dim=-1).unsqueeze(-2))
            sco = torch.zeros(B, H, N, N) if variant == "NOnly" else (q @ k.transpose(-1, -2)) * scale
        a = torch.softmax(sco + omega, -1)
    ctx = (a @ v).permute(0, 2, 1, 3).reshape(B, N, D)
    return ctx, a


SHAPES = [(2, 37, 64, 2), (1, 197, 128, 2), (1, 300, 160, 2), (1, 1370, 128, 2), (2, 65, 256, 2)]


@pytest.mark.parametrize("B,N,D,H", SHAPES)
@pytest.mark.parametrize("variant", ["vanilla", "ClearCLIP", "SCLIP", "SegEarth", "SFP", "Experimental"])
@pytest.mark.parametrize("prec,tol", [("f32", 2e-5), ("f16x2", 2e-5), ("bf16", 2.5e-2), ("f16", 4e-3)])
def test_attention(ops, B, N, D, H, variant, prec, tol):
    qkv = rnd(B, N, 3 * D, seed=N + D, scale=1.0)
    sim = None
    if variant in ("SegEarth", "Experimental", "ClearCLIP"):
        f = torch.nn.functional.normalize(rnd(B, N - 1, 24, seed=9), dim=-1)
        sim = f @ f.transpose(1, 2)
    ref, _ = attention_reference(qkv, H, variant, sim, 0.8)
    out = ops.attention(qkv.to(DEV), H, variant, None if sim is None else sim.to(DEV), 0.8, precision=prec)
    assert rel_err(out, ref) < tol, rel_err(out, ref)


@pytest.mark.parametrize("B,H", [(19, 4), (17, 8), (16, 6)])
@pytest.mark.parametrize("variant", ["Experimental", "SegEarth"])
@pytest.mark.parametrize("prec,tol", [("f16x2", 2e-5), ("bf16", 2.5e-2), ("f16", 4e-3)])
def test_attention_with_bias_many_images(ops, B, H, variant, prec, tol):
    """>= 16 images per launch and heads % 4 == 0: the biased kernels map workgroups as whole images per XCD, head groups of 4, all query
    blocks of a group (attention.hip); (16, 6) keeps the older (query block, head) order.  N = 300: three query blocks, ragged last key tile."""
    N, D = 300, 32 * H
    qkv = rnd(B, N, 3 * D, seed=B + H, scale=1.0)
    f = torch.nn.functional.normalize(rnd(B, N - 1, 24, seed=9), dim=-1)
    sim = f @ f.transpose(1, 2)
    ref, _ = attention_reference(qkv, H, variant, sim, 0.8)
    out = ops.attention(qkv.to(DEV), H, variant, sim.to(DEV), 0.8, precision=prec)
    assert rel_err(out, ref) < tol, rel_err(out, ref)


@pytest.mark.parametrize("variant", ["NACLIP", "NOnly", "GAV"])
@pytest.mark.parametrize("prec,tol", [("f32", 2e-5), ("f16x2", 2e-5), ("bf16", 2.5e-2), ("f16", 4e-3)])
def test_attention_gaussian_window(ops, variant, prec, tol):
    """NACLIP / NOnly / GAV (reference open_clip/transformer.py:909-932): Gaussian neighbourhood bias, square grids."""
    for (B, g, D, H) in ((2, 6, 64, 2), (1, 14, 128, 2), (1, 37, 128, 2)):
        N = g * g + 1
        qkv = rnd(B, N, 3 * D, seed=g)
        ref, _ = attention_reference(qkv, H, variant)
        out = ops.attention(qkv.to(DEV), H, variant, precision=prec)
        assert rel_err(out, ref) < tol, (variant, g, rel_err(out, ref))


@pytest.mark.parametrize("prec,tol", [("f32", 1e-5), ("f16x2", 1e-5), ("bf16", 3e-2), ("f16", 4e-3)])
def test_attention_stats(ops, prec, tol):
    B, N, D, H = 2, 101, 128, 2
    qkv = rnd(B, N, 3 * D, seed=3)
    ref, a = attention_reference(qkv, H, "vanilla")
    am = a.mean(1)
    ctx, a_cls, a_diag = ops.attention(qkv.to(DEV), H, "vanilla", precision=prec, want_stats=True)
    assert rel_err(ctx, ref) < max(tol, 2e-5)
    assert rel_err(a_cls, am[:, 0]) < tol
    assert rel_err(a_diag, torch.diagonal(am, dim1=-2, dim2=-1)) < tol


@pytest.mark.parametrize("prec,tol", [("f32", 2e-6), ("f16x2", 2e-6), ("bf16", 1e-2), ("f16", 1.5e-3)])
def test_similarity_map(ops, golden, prec, tol):
    g = golden("refine")
    f = torch.from_numpy(g["sim_feats"])
    if prec != "f32":                        # the half-precision GEMM needs D % 64 == 0
        f = torch.cat([f, torch.zeros(*f.shape[:2], 24)], -1)
    a = ops.similarity_map(f.to(DEV), 1.0, True, prec)
    b = ops.similarity_map(f.to(DEV), 0.5, False, prec)
    assert (a.cpu() - torch.from_numpy(g["sim_a"])).abs().max().item() < tol
    assert (b.cpu() - torch.from_numpy(g["sim_b"])).abs().max().item() < 2 * tol


def test_outlier_suppression_matches_reference_fixture(ops, golden):
    g = golden("refine")
    grid, attn = torch.from_numpy(g["grid"]), torch.from_numpy(g["attn"])
    B, D, gh, gw = grid.shape
    feats = grid.reshape(B, D, gh * gw).permute(0, 2, 1).contiguous()
    a_cls, a_diag = attn[:, 0].contiguous(), torch.diagonal(attn, dim1=-2, dim2=-1).contiguous()
    out, idx = ops.outlier_suppress(feats.to(DEV), a_cls.to(DEV), a_diag.to(DEV), gh, gw, 8, 0.1)
    assert torch.equal(idx.cpu().long(), torch.from_numpy(g["outlier_idx"]))
    ref = torch.from_numpy(g["suppressed"]).reshape(B, D, gh * gw).permute(0, 2, 1)
    assert (out.cpu() - ref).abs().max().item() < 1e-5


def test_weak_token_replace(ops, golden):
    g = golden("refine")
    grid, attn = torch.from_numpy(g["grid"]), torch.from_numpy(g["attn"])
    B, D, gh, gw = grid.shape
    feats = grid.reshape(B, D, gh * gw).permute(0, 2, 1).contiguous()
    a_diag = torch.diagonal(attn, dim1=-2, dim2=-1).contiguous()
    out, _ = ops.weak_token_replace(feats.to(DEV), a_diag.to(DEV), gh, gw, 6)
    ref = torch.from_numpy(g["selfattn_feature"]).reshape(B, D, gh * gw).permute(0, 2, 1)
    assert (out.cpu() - ref).abs().max().item() < 1e-5


def test_outlier_edge_cases(ops):
    """k >= n (every token an outlier), 1x1 and 2x2 grids, adjacent outliers: compare with the oracle."""
    for gh, k in ((1, 3), (2, 4), (3, 9), (5, 7)):
        n, D = gh * gh, 16
        grid = rnd(1, D, gh, gh, seed=gh)
        attn = torch.softmax(rnd(1, n + 1, n + 1, seed=gh + 10) * 2, -1)
        idx = OR.detect_outliers(attn, n, k)
        ref = OR.suppress_outliers(grid, idx, 0.1).reshape(1, D, n).permute(0, 2, 1)
        feats = grid.reshape(1, D, n).permute(0, 2, 1).contiguous()
        out, gi = ops.outlier_suppress(feats.to(DEV), attn[:, 0].contiguous().to(DEV),
                                       torch.diagonal(attn, dim1=-2, dim2=-1).contiguous().to(DEV), gh, gh, k, 0.1)
        assert torch.equal(gi.cpu().long(), idx)
        assert (out.cpu() - ref).abs().max().item() < 1e-5


def test_cosine_logits(ops):
    B, n, E, Q = 2, 50, 96, 8
    tok, cls = rnd(B, n, E, seed=1), rnd(B, E, seed=2)
    text = torch.nn.functional.normalize(rnd(Q, E, seed=3), dim=-1)
    for debias, lam in ((0.0, 0.0), (0.2, 0.0), (0.2, -0.3), (0.0, 0.5)):
        c = cls / cls.norm(dim=-1, keepdim=True)
        cl = c @ text.T
        f = tok
        if debias:
            sim = ((f / f.norm(dim=-1, keepdim=True)) * (c / c.norm(dim=-1, keepdim=True)).unsqueeze(1)).sum(-1)
            f = f - c.unsqueeze(1) * (sim.unsqueeze(-1) * debias)
        f = f / f.norm(dim=-1, keepdim=True)
        ref = f @ text.T
        if lam:
            ref = ref + cl.unsqueeze(1) * lam
        out = ops.cosine_logits(tok.to(DEV), cls.to(DEV), text.to(DEV), debias, lam)
        assert (out.cpu() - ref.permute(0, 2, 1)).abs().max().item() < 2e-6
    out = ops.cosine_logits(tok.to(DEV), None, text.to(DEV))
    f = tok / tok.norm(dim=-1, keepdim=True)
    assert (out.cpu() - (f @ text.T).permute(0, 2, 1)).abs().max().item() < 2e-6


@pytest.mark.parametrize("B,n,E,Q,lam", [(2, 16384 + 37, 96, 7, -0.3), (1, 20000, 768, 16, 0.0), (3, 16384, 64, 1, 0.5), (1, 65536 + 2, 128, 13, 0.2)])
def test_cosine_logits_per_pixel_form(ops, B, n, E, Q, lam):
    """sg_cosine_logits_two_plane (the per-pixel logits of the exact tower mode) runs as a GEMM on the matrix pipe: f32 rows split into two f16 planes,
    three MFMAs per product (head.hip: cosine_logits_mfma_kernel).  f32-grade against f64, ragged n (not a multiple of 4 / 64), Q below 16, cls term."""
    tok, cls = rnd(B, n, E, seed=11) * torch.logspace(-2, 2, n).view(1, n, 1), rnd(B, E, seed=12)
    text = torch.nn.functional.normalize(rnd(Q, E, seed=13), dim=-1)
    f = tok.double()
    ref = (f / f.norm(dim=-1, keepdim=True)) @ text.double().T
    if lam:
        c = cls.double()
        ref = ref + ((c / c.norm(dim=-1, keepdim=True)) @ text.double().T).unsqueeze(1) * lam
    out = ops.cosine_logits(tok.to(DEV), cls.to(DEV) if lam else None, text.to(DEV), 0.0, lam, two_plane=True)
    err = (out.cpu().double() - ref.permute(0, 2, 1)).abs().max().item()
    print(f"per-pixel cosine logits B={B} n={n} E={E} Q={Q}: max err {err:.2e}")
    assert out.shape == (B, Q, n) and err < 2e-6


@pytest.mark.parametrize("src,dst", [((7, 9), (21, 30)), ((14, 14), (224, 224)), ((37, 37), (518, 518)), ((10, 12), (10, 12)), ((16, 16), (9, 11))])
def test_resize_bilinear(ops, src, dst):
    x = rnd(5, *src, seed=4)
    ref = torch.nn.functional.interpolate(x[None], size=dst, mode="bilinear")[0]
    out = ops.resize_bilinear(x.to(DEV), dst)
    assert (out.cpu() - ref).abs().max().item() < 2e-6


@pytest.mark.parametrize("Q,H,W,crop,stride,P", [(6, 75, 60, 36, 20, 8), (11, 130, 200, 36, 20, 8),
                                                 (3, 52, 56, 32, 2, 8)])       # last: 143 windows, > 64 overlap one block
def test_stitch_equals_reference_loop(ops, Q, H, W, crop, stride, P):
    """Write-once stitch vs the reference's per-tile upsample / un-pad / add / count loop (segmentor.py:416-447)."""
    o = OS.SegOracle.__new__(OS.SegOracle)
    o.slide_stride, o.slide_crop = stride, crop
    wins = o.tile_windows(H, W)
    l, r, t, b = OS.compute_padsize(crop, crop, P)
    g = (crop + t + b) // P
    tl = rnd(len(wins), Q, g, g, seed=8)
    preds, count = torch.zeros(Q, H, W), torch.zeros(1, H, W)
    for i, (y1, y2, x1, x2) in enumerate(wins):
        up = torch.nn.functional.interpolate(tl[i][None], size=(crop + t + b, crop + l + r), mode="bilinear")[0]
        preds[:, y1:y2, x1:x2] += up[:, t:t + (y2 - y1), l:l + (x2 - x1)]
        count[:, y1:y2, x1:x2] += 1
    ref = preds / count
    out = ops.stitch(tl.to(DEV), torch.tensor([[y1, y2, x1, x2] for (y1, y2, x1, x2) in wins]), (crop + t + b, crop + l + r), (t, l), (H, W))
    assert (out.cpu() - ref).abs().max().item() < 3e-6


def test_postprocess(ops, golden):
    g = golden("segment")
    qidx = torch.tensor([0, 0, 1, 2, 3, 4, 5, 5])
    for name, thd, bg in (("ex_base", 0.1, 5), ("ex_pad", 0.0, 0), ("se_plain", 0.0, 0)):
        logits = torch.from_numpy(g[f"{name}.logits"])[0]
        o = OS.SegOracle.__new__(OS.SegOracle)
        o.logit_scale, o.query_idx, o.prob_thd, o.bg_idx = 50.0, qidx, thd, bg
        p_ref, pred_ref = o.postprocess(logits)
        probs, labels = ops.postprocess(logits.to(DEV), qidx, 6, 50.0, thd, bg)
        assert (probs.cpu() - p_ref).abs().max().item() < 1e-5
        assert torch.equal(labels.cpu(), torch.from_numpy(g[f"{name}.pred"]))
    # identity class map (K == Q): no synonym merge
    logits = rnd(5, 9, 11, seed=2) * 0.1
    probs, labels = ops.postprocess(logits.to(DEV), torch.arange(5), 5, 50.0, 0.3, 2)
    p = torch.softmax(logits * 50, 0)
    pred = p.argmax(0, keepdim=True)
    pred[p.max(0, keepdim=True)[0] < 0.3] = 2
    assert torch.equal(labels.cpu(), pred) and (probs.cpu() - p).abs().max().item() < 1e-5


def test_adaptive_conv(ops, golden):
    g = golden("jbu")
    out = ops.adaptive_conv(torch.from_numpy(g["ac_in"]).to(DEV), torch.from_numpy(g["ac_filt"]).to(DEV))
    assert (out.cpu() - torch.from_numpy(g["ac_out"])).abs().max().item() < 1e-5


# ---- SimFeatUp JBU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f16x2"])
@pytest.mark.parametrize("name", ["jbu_one", "jbu_stack"])
def test_jbu_matches_reference_fixture(golden, name, prec):
    """End-to-end upsampler against the fixture minted from the reference modules (adaptive conv = the reference's
    in-tree torch form of FeatUp's CUDA op; third party, unpinned -- see oracle/jbu.py)."""
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.upsampler import get_upsampler
    g = golden("jbu")
    src, guid = torch.from_numpy(g[f"{name}.src"]), torch.from_numpy(g[f"{name}.guidance"])
    C = src.shape[1]
    up = get_upsampler(name, C, DEV, prec)                 # f16x2: the f32 kernels with the three linears on the two-plane f16 GEMM -- same bound
    up.load_state_dict(Wt.make_jbu_weights(name, C, seed=3))
    out = up(src.to(DEV), guid.to(DEV))
    ref = torch.from_numpy(g[f"{name}.out"])
    err = (out.cpu() - ref).abs().max().item()
    assert err < 2e-4 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_jbu_on_the_trained_checkpoint(golden, precision):
    """The HIP upsampler on the reference's own trained JBUStack(512) checkpoint (weights + reference output in the fixture):
    f32 <= 2e-4 relative; bf16 (matrix-core adaptive conv, bf16 fixup linears) reported and bounded at 2x its measured error."""
    from clip_decontamination_amd.upsampler import get_upsampler
    g = golden("jbu_real")
    w = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w.")}
    up = get_upsampler("jbu_stack", 512, DEV, precision)
    up.load_state_dict(w)
    out = up(torch.from_numpy(g["src"]).to(DEV), torch.from_numpy(g["guidance"]).to(DEV))[0].cpu()
    scale = float(np.abs(g["out_c64"]).max())
    err = (out[:64] - torch.from_numpy(g["out_c64"])).abs().max().item() / scale
    err_sq = ((out * out).sum(0) - torch.from_numpy(g["out_sq"])).abs().max().item() / float(np.abs(g["out_sq"]).max())
    print(f"jbu_stack trained weights [{precision}]: max rel err {err:.3e}, energy rel err {err_sq:.3e}")
    tol = 2e-4 if precision == "f32" else 1.2e-2            # measured (r2): f32 6e-7; bf16 5.0e-3 / 5.6e-3
    assert err < tol and err_sq < tol, (err, err_sq)


@pytest.mark.parametrize("prec,tol", [("bf16", 1.5e-2), ("f16x2", 2e-4)])
@pytest.mark.parametrize("name,C,gh,gw", [("jbu_one", 64, 4, 4), ("jbu_one", 128, 3, 5), ("jbu_stack", 64, 5, 3), ("jbu_one", 64, 9, 10)])
def test_jbu_throughput_mode_lowres_conv_vs_oracle(name, C, gh, gw, prec, tol):
    """bf16 throughput mode (C % 64 == 0): the adaptive convolution runs on the LOW-RES source with the bicubic 2x folded into the
    per-pixel kernel (Keff = Wy^T K Wx, jbu_conv_lowres_kernel, radius 5 and 3); borders, ragged last blocks (sizes that are not
    multiples of 8) and batches against the fp32 oracle.  bf16 rounds features and kernel weights: ~5e-3 relative measured.
    f16x2: the same formulation on two-plane f16 operands (jbu_conv_lowres_x2_kernel, the exact range kernel, two-plane linears) at the f32 path's bound."""
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.upsampler import get_upsampler
    from oracle import vit as OV
    wnp = Wt.make_jbu_weights(name, C, seed=3)
    src = rnd(2, C, gh, gw, seed=1)
    guid = torch.nn.functional.interpolate(rnd(2, 3, 5, 7, seed=2), size=(16 * gh, 16 * gw), mode="bicubic") + 0.2 * rnd(2, 3, 16 * gh, 16 * gw, seed=3)
    ref = torch.cat([OJ.jbu_forward(OV.to_torch(wnp), src[i:i + 1], guid[i:i + 1]) for i in range(2)], 0)
    up = get_upsampler(name, C, DEV, prec)
    up.load_state_dict(wnp)
    out = up(src.to(DEV), guid.to(DEV)).cpu()
    rel = (out - ref).abs().max().item() / ref.abs().max().item()
    print(f"low-res conv [{name} C={C} {gh}x{gw} {prec}]: max rel err {rel:.3e}")
    assert rel < tol, rel


@pytest.mark.parametrize("name,prec,tol", [("jbu_one", "f32", 2e-4), ("jbu_one", "f16x2", 2e-4), ("jbu_stack", "f16x2", 2e-4), ("jbu_one", "bf16", 1.5e-2), ("jbu_stack", "bf16", 1.5e-2)])
def test_jbu_512_launch_shape_vs_oracle(name, prec, tol):
    """The launch shape of `bench.py --upsampler` / BASELINE configs[3]: a 32 x 32 token grid taken 16x to 512 x 512 pixels (stages 64, 128, 256, 512),
    on a 64-channel slice so that the oracle (tap loop, no unfold) finishes in seconds.  Every stage's grid, the reflect borders of the 512 stage and the
    8-tiles-per-launch batching of the product are exercised at the sizes the bench runs; f32 parity path and bf16 throughput path (low-res adaptive conv)."""
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.upsampler import get_upsampler
    from oracle import vit as OV
    C, g, B = 64, 32, 2
    wnp = Wt.make_jbu_weights(name, C, seed=3)
    src = rnd(B, C, g, g, seed=21)
    guid = torch.from_numpy(Wt.normalize_tiles(Wt.make_tiles_u8(B, 16 * g, seed=77, smooth=True)))            # [B,3,512,512], normalised as the tiles are
    with torch.no_grad():
        ref = torch.cat([OJ.jbu_forward(OV.to_torch(wnp), src[i:i + 1], guid[i:i + 1]) for i in range(B)], 0)
    up = get_upsampler(name, C, DEV, prec)
    up.load_state_dict(wnp)
    out = up(src.to(DEV), guid.to(DEV)).cpu()
    rel = (out - ref).abs().max().item() / ref.abs().max().item()
    print(f"JBU 32x32 -> 512x512 [{name} {prec}]: max rel err {rel:.3e}")
    assert out.shape == (B, C, 512, 512) and rel < tol, rel


@pytest.mark.parametrize("use_cls", [False, True])
def test_jbu_fused_logits_tail_equals_unfused_and_oracle(golden, ops, use_cls):
    """sg_jbu_logits (bf16 throughput mode: row-dot GEMM epilogue + Q-wide f32 product, the [S^2, C] map never written) against
    (a) the unfused bf16 path (sg_jbu_upsample -> sg_cosine_logits) and (b) the fp32 oracle, on the reference's trained JBUStack(512)."""
    import ctypes as C
    from clip_decontamination_amd import _lib
    from clip_decontamination_amd.upsampler import get_upsampler
    from clip_decontamination_amd.ops import ptr, stream_ptr
    g = golden("jbu_real")
    w = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w.")}
    up = get_upsampler("jbu_stack", 512, DEV, "bf16")
    up.load_state_dict(w)
    B, Q, gs = 2, 15, 4
    src = torch.cat([torch.from_numpy(g["src"]), rnd(1, 512, gs, gs, seed=5)], 0)
    guid = torch.cat([torch.from_numpy(g["guidance"]), torch.from_numpy(g["guidance"]).flip(-1) * 0.7], 0)
    text = torch.nn.functional.normalize(rnd(Q, 512, seed=8), dim=-1)
    cls = rnd(B, 512, seed=9) if use_cls else None
    lam = -0.3 if use_cls else 0.0
    tok = src.permute(0, 2, 3, 1).reshape(B, gs * gs, 512).contiguous().to(DEV)
    feats = up.upsample_tokens(tok, guid.to(DEV), gs, gs)
    unfused = ops.cosine_logits(feats, None if cls is None else cls.to(DEV), text.to(DEV), 0.0, lam)            # [B,Q,P]
    lib = _lib.load()
    P = 256 * gs * gs
    fused = torch.empty(B, Q, P, dtype=torch.float32, device=DEV)
    need = lib.sg_jbu_workspace_bytes(up._ctx, B, gs, gs)
    wp, wn = up._workspace(need)
    gd, td = guid.to(DEV).contiguous(), text.to(DEV).contiguous()
    cd = None if cls is None else cls.to(DEV).contiguous()
    _lib.check(lib.sg_jbu_logits(up._ctx, ptr(tok), ptr(gd), B, gs, gs, 16 * gs, 16 * gs, _lib.PREC_BF16, ptr(td), Q, ptr(cd), lam, ptr(fused), wp, wn,
                                 stream_ptr()), "sg_jbu_logits")
    d_fu = (fused - unfused).abs().max().item()
    with torch.no_grad():
        o = torch.cat([OJ.jbu_forward(w, src[i:i + 1], guid[i:i + 1]) for i in range(B)], 0)                  # [B,C,S,S]
        f = o.reshape(B, 512, P).permute(0, 2, 1)
        ref = (f / f.norm(dim=-1, keepdim=True)) @ text.T
        if use_cls:
            cn = cls / cls.norm(dim=-1, keepdim=True)
            ref = ref + lam * (cn @ text.T).unsqueeze(1)
        ref = ref.permute(0, 2, 1)
    d_or = (fused.cpu() - ref).abs().max().item()
    d_un = (unfused.cpu() - ref).abs().max().item()
    print(f"fused JBU tail (cls={use_cls}): |fused - unfused| = {d_fu:.3e}; vs fp32 oracle: fused {d_or:.3e}, unfused {d_un:.3e}")
    assert d_fu < 2e-3 and d_or < 3e-3


def test_jbu_fused_tail_feature_dim_not_a_multiple_of_256(ops):
    """C = 640 (64 | C, 256 does not divide C): the row-dot epilogue of the persistent GEMM must not write slice sums for the columns past C
    (the waves of the last 256-wide tile that own no 64-column slice), and a C = 512 upsampler run first must not pin the pixel-logits
    kernel's dynamic-LDS limit at the smaller size.  Fused tail against the unfused bf16 path."""
    import ctypes as C
    from clip_decontamination_amd import _lib, weights as Wt
    from clip_decontamination_amd.upsampler import get_upsampler
    from clip_decontamination_amd.ops import ptr, stream_ptr
    lib = _lib.load()
    for Cdim in (512, 640):
        up = get_upsampler("jbu_stack", Cdim, DEV, "bf16")
        up.load_state_dict(Wt.make_jbu_weights("jbu_stack", Cdim, seed=3))
        B, Q, gs = 1, 9, 4
        tok = rnd(B, gs * gs, Cdim, seed=11).to(DEV)
        guid = (torch.nn.functional.interpolate(rnd(B, 3, 6, 6, seed=12), size=(16 * gs, 16 * gs), mode="bicubic") + 0.1 * rnd(B, 3, 16 * gs, 16 * gs, seed=13)).to(DEV)
        text = torch.nn.functional.normalize(rnd(Q, Cdim, seed=14), dim=-1).to(DEV)
        feats = up.upsample_tokens(tok, guid, gs, gs)
        unfused = ops.cosine_logits(feats, None, text, 0.0, 0.0)
        P = 256 * gs * gs
        fused = torch.empty(B, Q, P, dtype=torch.float32, device=DEV)
        need = lib.sg_jbu_workspace_bytes(up._ctx, B, gs, gs)
        wp, wn = up._workspace(need)
        _lib.check(lib.sg_jbu_logits(up._ctx, ptr(tok), ptr(guid.contiguous()), B, gs, gs, 16 * gs, 16 * gs, _lib.PREC_BF16, ptr(text.contiguous()), Q, None, 0.0,
                                     ptr(fused), wp, wn, stream_ptr()), "sg_jbu_logits")
        d = (fused - unfused).abs().max().item()
        print(f"fused JBU tail C={Cdim}: |fused - unfused| = {d:.3e}")
        assert d < 2e-3, (Cdim, d)


def test_jbu_against_oracle_nonsquare_and_batched():
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.upsampler import get_upsampler
    from oracle import vit as OV
    C, gh, gw = 32, 4, 6
    wnp = Wt.make_jbu_weights("jbu_stack", C, seed=3)
    src = rnd(2, C, gh, gw, seed=1)
    guid = torch.nn.functional.interpolate(rnd(2, 3, 5, 7, seed=2), size=(16 * gh, 16 * gw), mode="bicubic") + 0.2 * rnd(2, 3, 16 * gh, 16 * gw, seed=3)
    ref = torch.cat([OJ.jbu_forward(OV.to_torch(wnp), src[i:i + 1], guid[i:i + 1]) for i in range(2)], 0)
    up = get_upsampler("jbu_stack", C, DEV, "f32")
    up.load_state_dict(wnp)
    out = up(src.to(DEV), guid.to(DEV))
    assert (out.cpu() - ref).abs().max().item() < 2e-4 * max(1.0, ref.abs().max().item())


def test_global_debias_one_shape_vs_torch(ops):
    import ctypes as C
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    tok, cls = rnd(2, 20, 48, seed=1).to(DEV), rnd(2, 48, seed=2).to(DEV)
    out = torch.empty_like(tok)
    _lib.check(lib.sg_global_debias(ops.ptr(tok), ops.ptr(cls), 2, 20, 48, 0.2, ops.ptr(out), ops.stream_ptr()))
    c = (cls / cls.norm(dim=-1, keepdim=True)).cpu()
    t = tok.cpu()
    sim = ((t / t.norm(dim=-1, keepdim=True)) * (c / c.norm(dim=-1, keepdim=True)).unsqueeze(1)).sum(-1)
    ref = t - c.unsqueeze(1) * (sim.unsqueeze(-1) * 0.2)
    assert (out.cpu() - ref).abs().max().item() < 2e-6


@pytest.mark.parametrize("mode", ["weighted", "attention"])
def test_cross_tile_fusion_matches_reference_fixture(ops, golden, mode):
    """Fixture: the reference CrossTileFusion module run tile by tile (raster order) on a 2x3 scene."""
    g = golden("refine")
    tiles = torch.from_numpy(g["ctf_tiles"])                   # [2,3,1,36,16]
    hg, wg = tiles.shape[:2]
    tok = tiles.reshape(hg * wg, 36, 16)
    out = ops.cross_tile_fusion(tok.to(DEV), hg, wg, 6, 6, 2, mode, 0.3)
    ref = torch.from_numpy(g[f"ctf_{mode}"]).reshape(hg * wg, 36, 16)
    assert (out.cpu() - ref).abs().max().item() < 2e-5


def test_cross_tile_fusion_larger_grid_vs_oracle(ops):
    hg, wg, gp, C = 3, 4, 9, 40
    tok = rnd(hg * wg, gp * gp, C, seed=3)
    for mode in ("weighted", "attention"):
        o = OR.CrossTileFusionOracle(mode, 2, 0.5)
        ref = torch.stack([o(tok[t:t + 1].clone(), t // wg, t % wg, gp, gp)[0] for t in range(hg * wg)], 0)
        out = ops.cross_tile_fusion(tok.to(DEV), hg, wg, gp, gp, 2, mode, 0.5)
        assert (out.cpu() - ref).abs().max().item() < 3e-5


# ---- Cluster-Then-Debias (CTD.py via segmentor.py:339-365) ---------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_ctd_matches_reference_fixture(ops, golden, tag):
    """Fixture = the reference's cluster_patch_tokens_dbscan (scikit-learn DBSCAN) + adaptive_debiasing.  Labels are integer
    work: exact.  The fixture holds no pair within 1e-4 of eps^2 (checked when it was minted)."""
    g = golden("ctd")
    out, labels = ops.ctd_debias(torch.from_numpy(g[f"{tag}.tokens"]).to(DEV), torch.from_numpy(g[f"{tag}.cls"]).to(DEV))
    assert np.array_equal(labels.cpu().numpy(), g[f"{tag}.labels"])
    assert (out.cpu() - torch.from_numpy(g[f"{tag}.out"])).abs().max().item() < 1e-5


def test_ctd_real_grid_vs_oracle(ops):
    """The L/14 tile shape (37 x 37 tokens, 768 channels), 3 tiles, raw (un-normalised) CLS features."""
    from oracle import ctd as OC
    x = torch.from_numpy(OC.make_clustered_tokens(3, 1369, 768, seed=2, spread=0.5, n_centers=9))
    cls = torch.from_numpy(np.random.default_rng(9).standard_normal((3, 768)).astype(np.float32))
    out, labels = ops.ctd_debias(x.to(DEV), cls.to(DEV), normalize_cls=True)
    ref, rlab = OC.ctd_debias(x, cls / cls.norm(dim=-1, keepdim=True))
    pts = OC.ctd_points(x)
    margin = min(np.abs(OC.neighbour_matrix(pts[b].numpy(), 1.1)[1] - 1.21).min() for b in range(3))
    same = (labels.cpu().long() == rlab).float().mean().item()
    print(f"[ctd 37x37x768] clusters {[int(l.max()) + 1 for l in rlab]}, noise {[int((l < 0).sum()) for l in rlab]}, "
          f"closest pair to the radius {margin:.2e}, label agreement {same:.6f}")
    if margin > 1e-6:                                        # no pair sits on the radius to within the f32 rounding of the points
        assert same == 1.0
        assert (out.cpu() - ref).abs().max().item() < 1e-4
    else:
        assert same > 0.99


def test_ctd_edge_cases(ops):
    g = torch.Generator().manual_seed(0)
    # all noise (isotropic points in 64-D never have 11 neighbours within cos > 0.395): tokens unchanged, labels -1
    x = torch.randn(2, 50, 64, generator=g)
    cls = torch.nn.functional.normalize(torch.randn(2, 64, generator=g), dim=-1)
    out, labels = ops.ctd_debias(x.to(DEV), cls.to(DEV))
    assert (labels == -1).all() and torch.equal(out.cpu(), x)
    # one cluster holding every token (identical directions)
    y = torch.randn(1, 1, 64, generator=g).expand(1, 40, 64) * torch.linspace(0.5, 2.0, 40).view(1, 40, 1)
    out, labels = ops.ctd_debias(y.contiguous().to(DEV), cls[:1].to(DEV))
    assert (labels == 0).all()
    from oracle import ctd as OC
    ref, _ = OC.ctd_debias(y.contiguous(), cls[:1])
    assert (out.cpu() - ref).abs().max().item() < 1e-5
    # fewer points than min_samples
    out, labels = ops.ctd_debias(x[:, :5].contiguous().to(DEV), cls.to(DEV))
    assert (labels == -1).all()


def test_known_answer_centre_of_a_3x3_grid(ops):
    """Reference test_som.py:130-182 (the repo's only known-answer vector): centre of a 3 x 3 grid of 1..9 -> neighbour mean 5.0."""
    feats = torch.arange(1, 10, dtype=torch.float32).reshape(1, 9, 1).repeat(1, 1, 4)
    feats[0, 4] = 100.0
    a_cls = torch.zeros(1, 10); a_cls[0, 5] = 1.0              # token 4 (+1 for CLS) has all the CLS attention
    a_diag = torch.full((1, 10), 0.5)
    out, idx = ops.outlier_suppress(feats.to(DEV), a_cls.to(DEV), a_diag.to(DEV), 3, 3, 1, 0.0)
    assert idx.cpu().tolist() == [[4]]
    assert torch.allclose(out[0, 4].cpu(), torch.full((4,), 5.0), atol=1e-5)
    out2, idx2 = ops.weak_token_replace(feats.to(DEV), torch.tensor([[0.5, 0.9, 0.9, 0.9, 0.9, 0.1, 0.9, 0.9, 0.9, 0.9]]).to(DEV), 3, 3, 1)
    assert idx2.cpu().tolist() == [[4]]
    assert torch.allclose(out2[0, 4].cpu(), torch.full((4,), 5.0), atol=1e-5)


def test_new_entry_points_reject_bad_arguments(ops):
    import ctypes as C
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1, 16, 8, device=DEV)
    cls = torch.zeros(1, 8, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    assert lib.sg_ctd_debias(P(x), P(cls), 1, 16, 6, C.c_double(1.1), 11, C.c_float(-1.5), 0, None, P(buf), buf.numel(), None) != 0   # C % 4
    assert b"multiple of 4" in lib.sg_last_error()
    assert lib.sg_ctd_debias(P(x), P(cls), 1, 16, 8, C.c_double(1.1), 11, C.c_float(-1.5), 0, None, P(buf), 16, None) != 0            # scratch too small
    assert b"scratch" in lib.sg_last_error()
    assert lib.sg_render_maps(None, None, None, 3, 4, 4, P(buf), None, None) != 0                                                   # mask without labels
    assert lib.sg_gemm_fp8_raw(P(buf), P(cls), P(buf), P(cls), None, None, P(x), 4, 8, 64, 0, 0, None) != 0                          # K % 128
    assert b"128" in lib.sg_last_error()


# ---- LayerNorm folded into its neighbouring GEMMs (sg_op_ln_chain; the towers' 2-byte modes) -----------------------------------------
def _ln_chain_ref(A, W1, b1, x, g, be, W2, b2, act):
    xn = x.double() + A.double() @ W1.double().T + b1.double()
    y = torch.nn.functional.layer_norm(xn, (xn.shape[1],), g.double(), be.double(), 1e-5) @ W2.double().T + b2.double()
    if act == 1:
        y = y * torch.sigmoid(1.702 * y)
    elif act == 2:
        y = torch.nn.functional.gelu(y)
    return xn.float(), y.float()


@pytest.mark.parametrize("M,K1,D,N2,act,mean_shift,outlier", [(1370, 1024, 1024, 3072, 0, 0.0, 20.0), (2055, 4096, 1024, 4096, 1, 0.0, 20.0),
                                                              (1200, 768, 768, 3072, 2, 3.0, 20.0), (1100, 512, 576, 640, 1, 0.5, 20.0),
                                                              (1370, 1024, 1024, 3072, 1, 10.0, 300.0)])
def test_ln_chain_folded_two_plane_is_f32_grade(M, K1, D, N2, act, mean_shift, outlier):
    """The folded LayerNorm in the exact mode (SG_PREC_F16X2, round 3): the two-plane copy of the raw residual rows out of the producing epilogue,
    rstd (x.W'^T - mean c) + b' in the consuming one.  Against f64: the folded chain must stay at the error level of the unfolded two-plane chain
    (explicit LayerNorm pass) -- f32 grade -- including rows whose mean sits many sigma from zero and a massive-activation channel, where the
    mean * c cancellation is largest; the f32 residual stream is the same GEMM either way."""
    from clip_decontamination_amd import ops
    g = lambda *sh, seed, sc=1.0: (torch.from_numpy(np.random.default_rng(seed).standard_normal(sh).astype(np.float32)) * sc).to(DEV)
    A, W1, b1 = g(M, K1, seed=1), g(D, K1, seed=2, sc=K1 ** -0.5), g(D, seed=3, sc=0.1)
    x = g(M, D, seed=4) * torch.logspace(-1, 1, M, device=DEV).view(M, 1) + mean_shift
    x[:, 7] += outlier
    gamma, beta = 1.0 + 0.3 * g(D, seed=5), 0.2 * g(D, seed=6)
    W2, b2 = g(N2, D, seed=7, sc=D ** -0.5), g(N2, seed=8, sc=0.1)
    xf, yf = ops.ln_chain(A, W1, b1, x, gamma, beta, W2, b2, act, "f16x2", fold=True)
    xu, yu = ops.ln_chain(A, W1, b1, x, gamma, beta, W2, b2, act, "f16x2", fold=False)
    xr, yr = _ln_chain_ref(A, W1, b1, x, gamma, beta, W2, b2, act)
    assert torch.equal(xf, xu)
    ef, eu = (yf - yr).abs(), (yu - yr).abs()
    scale = yr.abs().max().item()
    print(f"f16x2 M={M} D={D} N2={N2} shift={mean_shift} outlier={outlier}: folded max {ef.max().item():.3e} mean {ef.mean().item():.3e} | "
          f"unfolded max {eu.max().item():.3e} mean {eu.mean().item():.3e} (|y| max {scale:.2f})")
    assert ef.max().item() < 2e-5 * scale                       # the two-plane linear's own bound (test_linear)
    assert ef.mean().item() < 3.0 * eu.mean().item() + 1e-7 * scale


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("M,K1,D,N2,act,mean_shift,outlier", [(1370, 1024, 1024, 3072, 0, 0.0, 20.0), (2055, 4096, 1024, 4096, 1, 0.0, 20.0),
                                                              (1200, 768, 768, 3072, 2, 3.0, 20.0), (1024, 512, 512, 512, 0, -1.0, 20.0),
                                                              (1100, 512, 576, 640, 1, 0.5, 20.0),     # D, N2 multiples of 64 but not of the 256-wide tile
                                                              (1370, 1024, 1024, 3072, 0, 10.0, 300.0)])  # massive-activation channel (>= 100 sigma for most rows) + row means of 1..100 sigma
def test_ln_chain_folded_matches_unfolded_and_f64(prec, M, K1, D, N2, act, mean_shift, outlier):
    """Residual GEMM -> LayerNorm -> GEMM with the LayerNorm folded into the two epilogues: the f32 residual stream must equal the unfolded
    path's bit for bit (same GEMM), y must be as close to the f64 result as the unfolded path's (2-byte operands either way) -- also when
    the rows have a mean several standard deviations away from 0 (the case the centred statistics and the exact mean * c cancellation are for)."""
    from clip_decontamination_amd import ops
    g = lambda *sh, seed, sc=1.0: (torch.from_numpy(np.random.default_rng(seed).standard_normal(sh).astype(np.float32)) * sc).to(DEV)
    A, W1, b1 = g(M, K1, seed=1), g(D, K1, seed=2, sc=K1 ** -0.5), g(D, seed=3, sc=0.1)
    x = g(M, D, seed=4) * torch.logspace(-1, 1, M, device=DEV).view(M, 1) + mean_shift
    x[:, 7] += outlier                                         # one outlier channel, as real residual streams have
    gamma, beta = 1.0 + 0.3 * g(D, seed=5), 0.2 * g(D, seed=6)
    W2, b2 = g(N2, D, seed=7, sc=D ** -0.5), g(N2, seed=8, sc=0.1)
    xf, yf = ops.ln_chain(A, W1, b1, x, gamma, beta, W2, b2, act, prec, fold=True)
    xu, yu = ops.ln_chain(A, W1, b1, x, gamma, beta, W2, b2, act, prec, fold=False)
    xr, yr = _ln_chain_ref(A, W1, b1, x, gamma, beta, W2, b2, act)
    assert torch.equal(xf, xu)                                  # the residual stream itself is untouched by the folding
    assert (xf - xr).abs().max().item() < 2e-2 * xr.abs().max().item()
    ef = (yf - yr).abs()
    eu = (yu - yr).abs()
    scale = yr.abs().max().item()
    print(f"{prec} M={M} D={D} N2={N2}: folded max {ef.max().item():.3e} mean {ef.mean().item():.3e} | unfolded max {eu.max().item():.3e} mean {eu.mean().item():.3e} (|y| max {scale:.2f})")
    assert ef.mean().item() < 1.5 * eu.mean().item() + 1e-6
    assert ef.max().item() < 2.5 * eu.max().item() + 1e-3 * scale
