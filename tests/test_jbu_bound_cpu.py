"""The JBU bounds of tests/jbu_reference.py on the CPU (no GPU needed): an f32 emulation of each piece with the kernels' operand roundings
passes its bound, and each listed mutation of the arithmetic -- the kind of slip a kernel makes -- fails it on at least one design."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jbu_reference import (F32_TENTH, check_within, conv_bound, conv_reference, cubic_taps, range_reference, reflect,  # noqa: E402
                           rounded, rowdot_reference, sample_all, unpack_h2, pack_h2)


def dense_taps(n_in, n_out):
    """The bicubic rows as a dense [n_out, n_in] matrix (clamped taps added), f64."""
    idx, w = cubic_taps(n_in, n_out)
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    M.scatter_add_(1, idx, w)
    return M


def make_conv(B, h, w, C, r, seed, design="randn"):
    g = torch.Generator().manual_seed(seed)
    H, W = 2 * h, 2 * w
    d2 = (2 * r + 1) ** 2
    K = torch.softmax(torch.randn(B, H, W, d2, generator=g) * 2, -1) + 0.01 * torch.randn(B, H, W, d2, generator=g)
    src = torch.randn(B, h, w, C, generator=g)
    if design == "decades":
        src = src * 10.0 ** torch.randint(-2, 2, (B, h, w, 1), generator=g).float()
    if design == "near_half_ulp":               # f16 hi plane 1, lo plane ~ +2^-11: the lo plane carries a coherent share
        src = torch.full((B, h, w, C), 1.0 + 0.999 * 2.0 ** -11)
    if design == "onehot_third":                # K = 1/3 at the centre tap, source 1: every Keff element is a cubic-weight product times 1/3,
        K = torch.zeros(B, H, W, d2)             # whose f16 hi plane misses it by a share of the same sign pixel after pixel
        K[..., d2 // 2] = 1.0 / 3.0
        src = torch.ones(B, h, w, C)
        return K, src
    return K.float(), src.float()


def emulate_conv(K, src, r, kind, drop=None):
    """The kernels' arithmetic in f32 with their operand roundings (summation orders differ, within the accumulation terms);
    drop = 'src_lo' / 'keff_lo': the two-plane product without that lo plane (a mutation)."""
    B, H, W, d2 = K.shape
    _, h, w, C = src.shape
    D = 2 * r + 1
    My, Mx = dense_taps(h, H), dense_taps(w, W)
    out = torch.zeros(B, H, W, C, dtype=torch.float32)
    for b in range(B):
        for y in range(H):
            wy = My[reflect(y + torch.arange(D) - r, H)]                       # [D, h]
            for x in range(W):
                wx = Mx[reflect(x + torch.arange(D) - r, W)]                   # [D, w]
                k = K[b, y, x].view(D, D)
                if kind == "lowres":
                    T = (k.half().float() @ wx.float().half().float())          # f16 K and tables, f32 accumulation
                    Keff = wy.float().half().float().T @ T.half().float()       # T to f16, f32 accumulation
                    F = Keff.to(torch.bfloat16).float()
                    out[b, y, x] = (F.reshape(-1) @ src[b].reshape(h * w, C).to(torch.bfloat16).float())
                else:                                                           # lowres_x2: f32 tables and Keff, two planes
                    Keff = wy.float().T @ (k @ wx.float())
                    Fh = Keff.half().float()
                    Fl = (Keff - Fh).half().float()
                    s2 = pack_h2(src[b].reshape(h * w, C))
                    sv = s2.view(h * w, C // 8, 2, 8)
                    sh, sl = sv[:, :, 0].reshape(h * w, C).float(), sv[:, :, 1].reshape(h * w, C).float()
                    acc = Fh.reshape(-1) @ sh
                    if drop != "src_lo":
                        acc = acc + Fh.reshape(-1) @ sl
                    if drop != "keff_lo":
                        acc = acc + Fl.reshape(-1) @ sh
                    out[b, y, x] = acc
    return out


def src_as_consumed(src, kind):
    C = src.shape[-1]
    if kind == "lowres":
        return src.to(torch.bfloat16).double()
    return unpack_h2(pack_h2(src.reshape(-1, C))).view(src.shape)


@pytest.mark.parametrize("kind,r,grid", [("lowres", 3, (3, 5)), ("lowres", 5, (3, 3)), ("lowres_x2", 3, (5, 3)), ("lowres_x2", 5, (3, 3))])
@pytest.mark.parametrize("design", ["randn", "decades"])
def test_lowres_emulation_within_bound(kind, r, grid, design):
    h, w = grid
    K, src = make_conv(1, h, w, 16, r, seed=r + h, design=design)
    got = emulate_conv(K, src, r, kind)
    B, H, W = K.shape[:3]
    b, y, x = sample_all(B, H, W, "cpu")
    sc = src_as_consumed(src, kind)
    Kc = K.half().double() if kind == "lowres" else K.double()
    ref = conv_reference(Kc, r, b, y, x, src=sc)
    bnd = conv_bound(ref, kind, r, "f32", src=sc, b=b, y=y, x=x)
    check_within(got.view(-1, 16), ref["out"], bnd, f"{kind} emulation")


def _fails(got, ref, bnd):
    with pytest.raises(AssertionError):
        check_within(got, ref, bnd, "mutant")


MUTANTS = {
    "replicate_pad": dict(pad="replicate"),
    "bicubic_A_-0.5": dict(A=-0.5),
    "align_corners": dict(align_corners=True),
    "dropped_last_tap": dict(taps="drop_last"),
    "transposed_window": dict(transpose=True),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_conv_mutants_fail(mutant):
    """Each mutation of the convolution's geometry, evaluated exactly, leaves the bound of the true operation (the two-plane low-res
    kernel's, that of the f16x2 drop-in precision) on the 3 x 5 grid whose every pixel is within r of a border."""
    r, h, w = 3, 3, 5
    K, src = make_conv(1, h, w, 8, r, seed=11)
    B, H, W = K.shape[:3]
    b, y, x = sample_all(B, H, W, "cpu")
    Kd, sd = K.double(), src.double()
    ref = conv_reference(Kd, r, b, y, x, src=sd)
    bnd = conv_bound(ref, "lowres_x2", r, "f32", src=sd, b=b, y=y, x=x)
    kw = dict(MUTANTS[mutant])
    if kw.get("taps") == "drop_last":
        kw["taps"] = range((2 * r + 1) ** 2 - 1)
    mut = conv_reference(Kd, r, b, y, x, src=sd, **kw)
    _fails(mut["out"], ref["out"], bnd)


def test_swapped_tables_on_non_square_grid_fail():
    """Wx and Wy swapped: the row table built for the column count and the column table for the row count (3 x 5 grid)."""
    r, h, w = 3, 3, 5
    K, src = make_conv(1, h, w, 8, r, seed=12)
    B, H, W = K.shape[:3]
    b, y, x = sample_all(B, H, W, "cpu")
    Kd, sd = K.double(), src.double()
    ref = conv_reference(Kd, r, b, y, x, src=sd)
    bnd = conv_bound(ref, "lowres_x2", r, "f32", src=sd, b=b, y=y, x=x)
    # the slip: each axis built from the other axis' table (taps clamped into the real extent; the missing columns repeat the last row)
    iyx, wyx = cubic_taps(w, W)
    My_wrong = torch.zeros(H, h, dtype=torch.float64)
    My_wrong.scatter_add_(1, iyx[:H].clamp(max=h - 1), wyx[:H])
    ihx, whx = cubic_taps(h, H)
    idx = torch.cat([ihx, ihx[-1:].expand(W - H, 4)])
    wv = torch.cat([whx, whx[-1:].expand(W - H, 4)])
    Mx_wrong = torch.zeros(W, w, dtype=torch.float64)
    Mx_wrong.scatter_add_(1, idx, wv)
    hr = torch.einsum("Yy,byxc,Xx->bYXc", My_wrong, sd, Mx_wrong)
    mut = conv_reference(Kd, r, b, y, x, hr=hr)
    _fails(mut["out"], ref["out"], bnd)


def test_ragged_block_row_from_neighbour_fails():
    """The last row of a ragged 8 x 8 block (H = 6) computed with the kernel row of its neighbour."""
    r, h, w = 3, 3, 5
    K, src = make_conv(1, h, w, 8, r, seed=13)
    B, H, W = K.shape[:3]
    b, y, x = sample_all(B, H, W, "cpu")
    Kd, sd = K.double(), src.double()
    ref = conv_reference(Kd, r, b, y, x, src=sd)
    bnd = conv_bound(ref, "lowres_x2", r, "f32", src=sd, b=b, y=y, x=x)
    Km = Kd.clone()
    Km[:, H - 1] = Kd[:, H - 2]
    _fails(conv_reference(Km, r, b, y, x, src=sd)["out"], ref["out"], bnd)


@pytest.mark.parametrize("drop,design", [("src_lo", "near_half_ulp"), ("keff_lo", "onehot_third")])
def test_x2_lost_lo_plane_fails(drop, design):
    """The two-plane convolution without the source's lo plane (every source element just below 1 + half an f16 ulp) or without Keff's lo
    plane (K = 1/3 at the centre tap on a constant source): on these designs the lost planes are coherent, so the lost share (~2^-11 of
    the output) is several times the bound, while the correct emulation stays far inside it."""
    r, h, w = 3, 3, 3
    K, src = make_conv(1, h, w, 16, r, seed=14, design=design)
    B, H, W = K.shape[:3]
    b, y, x = sample_all(B, H, W, "cpu")
    sc = src_as_consumed(src, "lowres_x2")
    ref = conv_reference(K.double(), r, b, y, x, src=sc)
    bnd = conv_bound(ref, "lowres_x2", r, "f32", src=sc, b=b, y=y, x=x)
    check_within(emulate_conv(K, src, r, "lowres_x2").view(-1, 16), ref["out"], bnd, "two-plane emulation")
    got = emulate_conv(K, src, r, "lowres_x2", drop=drop)
    _fails(got.view(-1, 16), ref["out"], bnd)


# ---- range kernel ------------------------------------------------------------------------------------------------------------------
def emulate_range(proj, r, rt, sigma, keys):
    """jbu_kernel_*: scores from keys as stored (f32 / f16), f32 softmax, spatial factor, normalisation -- in f32."""
    B, H, W, _ = proj.shape
    d = 2 * r + 1
    p = proj.half().float() if keys == "f16" else proj
    temp = min(max(float(torch.tensor(rt).exp()), 1e-4), 1e4)
    b, y, x = sample_all(B, H, W, "cpu")
    kc = p[b, y, x]
    s = torch.stack([(p[b, reflect(y + t // d - r, H), reflect(x + t % d - r, W)] * kc).sum(-1) for t in range(d * d)], 1) * temp
    e = torch.exp(s - s.max(1, keepdim=True).values)
    step = torch.tensor(2.0 / (d - 1), dtype=torch.float32)
    t = torch.arange(d * d)
    fi, fj = -1 + (t // d).float() * step, -1 + (t % d).float() * step
    sp = torch.exp(-(fi * fi + fj * fj) / (2 * torch.tensor(sigma) ** 2))
    k = e / e.sum(1, keepdim=True) * sp
    return k / k.sum(1, keepdim=True).clamp(min=1e-7)


def range_case(design):
    g = torch.Generator().manual_seed(21)
    proj = torch.randn(1, 6, 10, 32, generator=g)
    if design == "small_sigma":                 # keys along one direction with per-pixel lengths: a longer neighbour out-scores the centre,
        v = torch.randn(32, generator=g)         # whose softmax weight then falls below 1e-7 while the spatial factor kills the winner
        m = 1 + torch.rand(1, 6, 10, 1, generator=g)
        return (v * 2 / v.norm()) * m, float(torch.tensor(20.0).log()), 0.05
    return proj * 0.3, 0.3, 0.8


@pytest.mark.parametrize("keys", ["f32", "f16"])
@pytest.mark.parametrize("design", ["plain", "small_sigma"])
def test_range_emulation_within_bound(keys, design):
    proj, rt, sig = range_case(design)
    B, H, W, _ = proj.shape
    b, y, x = sample_all(B, H, W, "cpu")
    X, bnd, fired = range_reference(proj, 3, rt, sig, keys, b, y, x)
    if design == "small_sigma":
        assert bool(fired.any()), "the clamp(1e-7) branch never fires in this design"
    check_within(emulate_range(proj, 3, rt, sig, keys), X, bnd, "range emulation")


@pytest.mark.parametrize("mutant,design", [("no_spatial", "plain"), ("clamp_1e-6", "small_sigma"), ("replicate", "plain"),
                                           ("transposed", "plain")])
def test_range_mutants_fail(mutant, design):
    proj, rt, sig = range_case(design)
    B, H, W, _ = proj.shape
    b, y, x = sample_all(B, H, W, "cpu")
    X, bnd, _ = range_reference(proj, 3, rt, sig, "f32", b, y, x)
    kw = {"no_spatial": dict(spatial=False), "clamp_1e-6": dict(clamp=1e-6), "replicate": dict(pad="replicate"), "transposed": {}}[mutant]
    Xm, _, _ = range_reference(proj, 3, rt, sig, "f32", b, y, x, **kw)
    if mutant == "transposed":                  # tap (i, j) stored at (j, i)
        Xm = Xm.view(-1, 7, 7).transpose(1, 2).reshape(-1, 49)
    _fails(Xm, X, bnd)


# ---- fused tail --------------------------------------------------------------------------------------------------------------------
def test_rowdot_emulation_and_missing_square():
    g = torch.Generator().manual_seed(31)
    C = 128
    x = torch.randn(40, C, generator=g).to(torch.bfloat16).double()
    Wf = torch.randn(C, C, generator=g) * C ** -0.5
    bf = torch.randn(C, generator=g) * 0.1
    Wr = rounded(Wf, "bf16")
    b01 = (bf * torch.tensor(F32_TENTH, dtype=torch.float32)).double()
    ref, bnd = rowdot_reference(x, Wr, b01)
    z = (x.float() @ Wr.float().T) * torch.tensor(F32_TENTH, dtype=torch.float32) + b01.float()
    emu = (z * (2 * x.float() + z)).view(40, 2, 64).sum(-1)
    check_within(emu, ref, bnd, "row-dot emulation")
    _fails((z * 2 * x.float()).view(40, 2, 64).sum(-1), ref, bnd)
