"""The row-kernel references and bounds of tests/rowops_reference.py on the CPU (no GPU needed), on the case generators the GPU module
uses: (1) each reference equals torch's own f64 operation, (2) an f32 emulation of each kernel -- 64-lane strided accumulation plus a
butterfly -- stays inside its bound on every case, (3) each listed mutation of the arithmetic or of the addressing -- the kind of slip a
kernel makes -- fails on a named case.  The refusals that the host functions make before any launch are checked here too."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_reference as R                                            # noqa: E402
from rowops_reference import check_within                               # noqa: E402
from oracle import vit as OV                                            # noqa: E402

EPS = 1e-5


def inside(got, ref, bound) -> bool:
    try:
        check_within(got, ref, bound)
    except AssertionError:
        return False
    return True


# ---- (1) the references are torch's operations in f64 ----------------------------------------------------------------------------------------
def test_layernorm_and_normalize_references_equal_torch():
    for rows, D in ((5, 260), (9, 2048), (1, 4)):
        x, g, b = R.make_ln_case(rows, D, seed=D)
        y, _, _ = R.layernorm_reference(x, g, b, EPS)
        assert torch.allclose(y, F.layer_norm(x.double(), (D,), g.double(), b.double(), EPS), rtol=1e-12, atol=1e-12)
    for rows, D in ((7, 65), (7, 1), (4101, 40)):
        _, v = R.make_l2_case(rows, D, seed=D)
        y, _ = R.l2norm_reference(v, 1e-12, "f32")
        assert torch.allclose(y, F.normalize(v.double(), dim=-1, eps=1e-12), rtol=1e-13, atol=0)


@pytest.mark.parametrize("g0,gh,gw", R.RESIZE_CASES + ((16, 7, 9),))
def test_resize_references_equal_torch_interpolate(g0, gh, gw):
    """Non-square targets, up- and downscaling, both modes, with the scale carried in double as F.interpolate does for f64 tensors."""
    pos = R.make_pos(g0, 5, seed=gh).double()
    grid = pos[1:].reshape(1, g0, g0, 5).permute(0, 3, 1, 2)
    plain = F.interpolate(grid, scale_factor=((gh + 0.1) / g0, (gw + 0.1) / g0), mode="bicubic")
    aa = F.interpolate(grid, size=(gh, gw), mode="bicubic", antialias=True)
    assert plain.shape[-2:] == (gh, gw)
    for mode, want in ((0, plain), (1, aa)):
        ref, _ = R.posembed_resize_reference(pos, g0, gh, gw, mode, f32=False)
        assert torch.equal(ref[0], pos[0])
        assert torch.allclose(ref[1:], want.permute(0, 2, 3, 1).reshape(gh * gw, 5), rtol=0, atol=1e-13)


@pytest.mark.parametrize("variant", R.SOFTMAX_VARIANTS)
def test_softmax_references_equal_torch_softmax(variant):
    B, H, N = 2, 3, 65
    scores, kw = R.make_softmax_case(N, variant, seed=1)
    ref = R.softmax_reference(scores, B, H, N, **kw)
    s = scores.double().view(B, H, N, N)
    sc = kw["scale_per_image"].double().view(B, 1, 1, 1) if kw.get("scale_per_image") is not None else kw["scale"]
    t = torch.zeros(B, H, N, N, dtype=torch.float64)
    if kw.get("bias") is not None:
        bias = kw["bias"].double()
        bias = bias[None].expand(B, -1, -1) if kw["bias_bstride"] == 0 else bias
        t[:, :, 1:, 1:] = bias[:, None] * kw["bias_w"]
        if kw.get("rn") is not None:
            t = t * kw["rn"].double()[..., None] * kw["cn"].double()[:, :, None, :]
    mask = torch.zeros(N, N, dtype=torch.float64)
    if kw.get("causal"):
        mask = torch.full((N, N), float("-inf"), dtype=torch.float64).triu(1)
    if kw["mode"] == 0:
        want = torch.softmax(s * sc + t + mask, -1)
        lse = torch.logsumexp(s * sc + t + mask, -1)
    else:
        want = torch.softmax(torch.softmax(s * sc + mask, -1) + t + mask, -1)
        lse = torch.logsumexp(s * sc + mask, -1)
    if kw.get("prefill") is not None:
        want = want + kw["prefill"].double().view(B, H, N, N)
    assert torch.allclose(ref["out"], want.reshape(B * H * N, N), rtol=1e-12, atol=1e-300)
    assert torch.allclose(ref["lse"], lse.reshape(-1), rtol=1e-13, atol=1e-13)
    if kw.get("causal"):
        assert bool((ref["out"][ref["exact_zero"]] == 0).all()) and bool((ref["bound"][ref["exact_zero"]] == 0).all())


def test_gaussian_bias_reference_equals_the_oracle():
    for gh, gw, std in ((3, 5, 1.0), (4, 4, 2.5)):
        om, _ = R.gaussian_bias_reference(gh, gw, std)
        want = OV.gaussian_bias(gh, gw, std)
        assert bool((want[0] == 0).all()) and bool((want[:, 0] == 0).all())
        assert torch.allclose(om, want[1:, 1:].double(), rtol=1e-6, atol=1e-7)           # the oracle evaluates in f32


def test_e4m3_encoding_equals_torch_float8():
    g = torch.Generator().manual_seed(0)                                 # f32 values: torch converts from f32, a single rounding
    v = torch.cat([torch.linspace(-460, 460, 100001), torch.randn(50000, generator=g) * 0.02,
                   torch.tensor([0.0, -0.0, 2.0 ** -10, 3 * 2.0 ** -10, 1.5 * 2.0 ** -9, 448.0, 464.0, 2.0 ** -6])]).double()
    byte, val = R.e4m3_rne(v)
    want = v.float().clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(byte, want.view(torch.uint8))
    assert torch.equal(val, want.double()) and torch.equal(R.e4m3_value(byte), val)
    allb = torch.arange(256, dtype=torch.uint8)
    t = allb.view(torch.float8_e4m3fn).double()
    assert torch.equal(torch.isnan(t), torch.isnan(R.e4m3_value(allb)))
    assert torch.equal(t.nan_to_num(0.0), R.e4m3_value(allb).nan_to_num(0.0))


# ---- (2) + (3): LayerNorm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.LN_D)
@pytest.mark.parametrize("rows", R.LN_ROWS)
def test_layernorm_f32_emulation_inside_the_bound(rows, D):
    x, g, b = R.make_ln_case(rows, D, seed=D + rows)
    emu = R.layernorm_emulate(x, g, b, EPS)
    for kind in R.KINDS:
        if kind == "h2" and D % 8:
            continue
        y, bound, _ = R.layernorm_reference(x, g, b, EPS, kind)
        r = check_within(R.load(R.store(emu, kind), kind), y, bound, f"layernorm {kind} rows {rows} D {D}")
        assert r <= 1.0
    if rows >= 3:                                                        # the constant row: rstd = 1 / sqrt(eps), output = beta
        y, _, _ = R.layernorm_reference(x, g, b, EPS)
        assert torch.allclose(y[rows - 1], b.double(), atol=1e-12)


@pytest.mark.parametrize("mut,rows,D", [("div_d_minus_1", 5, 2048), ("div_d_minus_1", 1, 4), ("eps_outside", 5, 64), ("one_pass", 5, 768),
                                        ("drop_last_vec", 5, 260), ("drop_last_vec", 9, 252), ("gamma_stride", 1, 64)])
def test_layernorm_mutations_fail(mut, rows, D):
    x, g, b = R.make_ln_case(rows, D, seed=D + rows)
    y, bound, _ = R.layernorm_reference(x, g, b, EPS)
    assert inside(R.layernorm_emulate(x, g, b, EPS), y, bound)
    got = R.layernorm_emulate(x, g, b, EPS, mut)
    assert not inside(got, y, bound)
    if mut == "one_pass":                                                # it is the offset-mean row that gives it away
        assert not inside(got[1], y[1], bound[1]) and inside(got[0], y[0], bound[0])


def test_embed_assemble_reference_is_layernorm_of_the_f32_sum():
    B, N, D = 2, 6, 260
    g = torch.Generator().manual_seed(5)
    patches, cls, pos = torch.randn(B * (N - 1), D, generator=g), torch.randn(D, generator=g), torch.randn(N, D, generator=g)
    _, gamma, beta = R.make_ln_case(1, D, 3)
    y, bound = R.embed_assemble_reference(patches, cls, pos, gamma, beta, EPS, B, N)
    tok = torch.cat([cls.view(1, 1, D).expand(B, 1, D), patches.view(B, N - 1, D)], 1) + pos[None]
    assert inside(R.layernorm_emulate(tok.view(B * N, D), gamma, beta, EPS).view(B, N, D), y, bound)
    assert torch.equal(y[0, 0], y[1, 0])                                 # the CLS row is ln(cls + pos[0]) for both images
    want, _, _ = R.layernorm_reference((cls + pos[0])[None], gamma, beta, EPS)
    assert torch.equal(y[0, 0], want[0])


# ---- fp8 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("D", R.LN_D)
def test_quantize_rows_expected_bytes_dequantise_within_half_a_step(D, kind):
    _, v = R.make_quant_case(5, D, seed=D, kind=kind)
    byte, scale = R.quantize_rows_expected(v)
    assert float(scale[0]) == 1.0 and bool((byte[0] == 0).all())         # the all-zero row
    assert R.fp8_within_half_step(byte, scale, v)                        # the tiny row (amax 1e-37) included
    assert bool(torch.isfinite(R.e4m3_value(byte)).all())
    assert int(byte[4, D - 1]) == 0x7e                                   # the row maximum in the last element encodes as 448
    big = v.abs().max(-1)[0] >= 2.0 ** -100                              # rows the scale floor leaves alone
    assert torch.equal(scale[big], (v.abs().max(-1)[0] / 448.0)[big])


def test_fp8_tiny_row_without_the_scale_floor_is_all_nan():
    """Suspect 1 on paper: amax = 1e-37 gives scale 2.2e-40, whose f32 reciprocal is +inf."""
    with np.errstate(over="ignore", divide="ignore"):
        sc = np.float32(1e-37) / np.float32(448.0)
        assert np.isinf(np.float32(1.0) / sc)
    sc, inv = R.fp8_scale_f32(np.array([1e-37], dtype=np.float32))
    assert float(sc[0]) == R.FLT_MIN and np.isfinite(inv[0])


@pytest.mark.parametrize("mut", ["amax_240", "truncate", "scale_per_4_rows"])
def test_fp8_mutations_fail(mut):
    _, v = R.make_quant_case(5, 260, seed=260)
    byte, scale = R.quantize_rows_expected(v)
    mb, ms = R.quantize_rows_expected(v, mut)
    assert not (torch.equal(mb, byte) and torch.equal(ms, scale))
    x, g, b = R.make_ln_fp8_case(5, 260, seed=1)
    mb, ms = R.layernorm_fp8_emulate(x, g, b, EPS, mut)
    with pytest.raises(AssertionError):
        R.layernorm_fp8_check(mb, ms, x, g, b, EPS, mut)


@pytest.mark.parametrize("tiny", [False, True])
@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_fp8_emulation_is_admissible_and_rarely_ambiguous(D, tiny):
    """The f32 emulation alone: every byte among the admissible codes, the share of elements on a rounding boundary under the 2 % cap."""
    x, g, b = R.make_ln_fp8_case(5, D, seed=D + 5, tiny=tiny)
    byte, scale = R.layernorm_fp8_emulate(x, g, b, EPS)
    share, ratio = R.layernorm_fp8_check(byte, scale, x, g, b, EPS, f"D {D}")
    print(f"layernorm_fp8 D {D}: {share:.3%} of the elements on a rounding boundary, scale err/bound {ratio:.3g}")
    assert share <= 0.02 and ratio <= 1.0
    y, _, _ = R.layernorm_reference(x, g, b, EPS)
    assert int(y[0].abs().argmax()) == D - 1 and (tiny or int(byte[0, D - 1]) & 0x7f == 0x7e)   # the row maximum in the last lane's last element
    if tiny:
        assert float(scale[4]) == 1.0 and bool((byte[4] == 0).all()) and float(y.abs().max()) < 1e-35
        assert bool((scale[:4] == R.FLT_MIN).all())


# ---- l2norm ----------------------------------------------------------------------------------------------------------------------------------------
L2_GENERAL = [(rows, D) for rows in (1, 7) for D in (1, 63, 64, 65, 768)]
L2_SHORT = [(4101, 8, 8), (4101, 40, 8), (4101, 64, 8), (4099, 72, 16), (4099, 128, 16)]


@pytest.mark.parametrize("rows,D", L2_GENERAL)
def test_l2norm_emulation_inside_the_bound(rows, D):
    for kin in ("f32", "bf16", "f16"):
        _, v = R.make_l2_case(rows, D, seed=D, kind=kin)
        emu = R.l2norm_emulate(v, 1e-12)
        for kout in R.KINDS:
            if kout == "h2" and D % 8:
                continue
            y, bound = R.l2norm_reference(v, 1e-12, kout)
            assert check_within(R.load(R.store(emu, kout), kout), y, bound, f"l2norm {kin}->{kout} {rows}x{D}") <= 1.0
        if rows >= 3 and kin == "f32":
            assert bool((emu[0] == 0).all()) and abs(float(emu[1].double().norm()) - 1e-3) < 1e-8      # norm 1e-15 / eps 1e-12


@pytest.mark.parametrize("rows,D,lanes", L2_SHORT)
def test_l2norm_short_emulation_inside_the_bound(rows, D, lanes):
    _, v = R.make_l2_case(rows, D, seed=D, special=False)
    y, bound = R.l2norm_reference(v, 1e-12, "f32", lanes)
    assert check_within(R.l2norm_emulate(v, 1e-12, lanes), y, bound) <= 1.0


def test_l2norm_mutations_fail():
    _, v = R.make_l2_case(7, 65, seed=65)
    y, bound = R.l2norm_reference(v, 1e-12, "f32")
    assert not inside(R.l2norm_emulate(v, 1e-12, mut="norm_plus_eps"), y, bound)         # the norm-1e-15 row
    _, v = R.make_l2_case(4101, 40, seed=40, special=False)
    y, bound = R.l2norm_reference(v, 1e-12, "f32", 8)
    assert not inside(R.l2norm_emulate(v, 1e-12, 8, mut="wrong_lane_group"), y, bound)
    flat = torch.arange(400, dtype=torch.float32)                        # so and si swapped: other rows are read
    assert not torch.equal(R.gather_rows(flat, 96, 24, 3, 7, 8), R.gather_rows(flat, 24, 96, 3, 7, 8))


# ---- softmax ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", R.SOFTMAX_VARIANTS)
@pytest.mark.parametrize("N", R.SOFTMAX_N)
def test_softmax_emulation_inside_the_bound(N, variant):
    scores, kw = R.make_softmax_case(N, variant, seed=N)
    ref = R.softmax_reference(scores, 2, 3, N, **kw)
    out, lse = R.softmax_emulate(scores, 2, 3, N, **kw)
    z = ref["exact_zero"]
    assert bool((out[z] == 0).all()) or kw.get("prefill") is not None
    assert check_within(out[~z], ref["out"][~z], ref["bound"][~z], f"softmax {variant} N {N}") <= 1.0
    assert check_within(lse, ref["lse"], ref["lse_bound"], f"lse {variant} N {N}") <= 1.0


@pytest.mark.parametrize("mut,variant", [("bias_transposed", "bias_per_image"), ("bias_at_cls", "bias_shared"), ("scale_bh", "scale_per_image"),
                                         ("causal_nk_i", "causal"), ("bias_before_first", "mode1_bias"), ("accumulate_overwrites", "accumulate")])
def test_softmax_mutations_fail(mut, variant):
    N = 65
    scores, kw = R.make_softmax_case(N, variant, seed=N)
    ref = R.softmax_reference(scores, 2, 3, N, **kw)
    out, _ = R.softmax_emulate(scores, 2, 3, N, **kw)
    assert inside(out, ref["out"], ref["bound"] + 0.0)
    out, _ = R.softmax_emulate(scores, 2, 3, N, mut=mut, **kw)
    assert not inside(out, ref["out"], ref["bound"])


def test_softmax_mode1_causal_tail_left_unwritten_fails():
    """Suspect 2 on paper: mode 1 that does not zero the keys after the query leaves whatever the buffer held."""
    N = 65
    scores, kw = R.make_softmax_case(N, "mode1_causal", seed=N)
    ref = R.softmax_reference(scores, 2, 3, N, **kw)
    out, _ = R.softmax_emulate(scores, 2, 3, N, **kw)
    z = ref["exact_zero"]
    assert bool((out[z] == 0).all())
    stale = torch.where(z, torch.full_like(out, -12345.5), out)
    assert not bool((stale[z] == 0).all())


# ---- resize ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.RESIZE_D)
@pytest.mark.parametrize("g0,gh,gw", R.RESIZE_CASES)
def test_resize_emulation_inside_the_bound(g0, gh, gw, D):
    pos = R.make_pos(g0, D, seed=gh * 40 + gw)
    for mode in (0, 1):
        ref, bound = R.posembed_resize_reference(pos, g0, gh, gw, mode)
        emu = R.posembed_resize_emulate(pos, g0, gh, gw, mode)
        assert torch.equal(emu[0], pos[0])
        assert check_within(emu[1:], ref[1:], bound[1:], f"resize mode {mode} {g0}->{gh}x{gw}") <= 1.0


@pytest.mark.parametrize("mut,mode,case", [("A_minus_half", 0, (7, 9, 5)), ("scale_g0_over_g", 0, (7, 9, 5)), ("clamp_src", 0, (7, 14, 14)),
                                           ("align_corners", 0, (7, 7, 9)), ("no_renorm", 1, (16, 3, 37)), ("no_renorm", 1, (7, 3, 4)),
                                           ("swap_hw", 0, (7, 9, 5)), ("swap_hw", 1, (16, 3, 37))])
def test_resize_mutations_fail(mut, mode, case):
    g0, gh, gw = case
    pos = R.make_pos(g0, 8, seed=gh * 40 + gw)
    ref, bound = R.posembed_resize_reference(pos, g0, gh, gw, mode)
    assert not inside(R.posembed_resize_emulate(pos, g0, gh, gw, mode, mut)[1:], ref[1:], bound[1:])


# ---- folded LayerNorm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("S", [1, 8, 16])
def test_ln_stats_emulation_inside_the_bound_and_between_term_needed(S, rows):
    st = R.make_ln_stats_case(S, rows, seed=S)
    mean, rstd, dmean, drstd = R.ln_stats_reference(st, EPS)
    em, er = R.ln_stats_emulate(st, EPS)
    assert check_within(em, mean, dmean) <= 1.0 and check_within(er, rstd, drstd) <= 1.0
    x = torch.randn(3, S * 64, dtype=torch.float64)                      # Chan's combination is the row's own mean / variance
    sl = x.view(3, S, 64)
    st2 = torch.stack([sl.sum(-1), ((sl - sl.mean(-1, keepdim=True)) ** 2).sum(-1)], -1).permute(1, 0, 2)
    m2, r2, _, _ = R.ln_stats_reference(st2, EPS)
    assert torch.allclose(m2, x.mean(-1)) and torch.allclose(r2, 1.0 / torch.sqrt(x.var(-1, unbiased=False) + EPS))
    if S > 1:
        _, er = R.ln_stats_emulate(st, EPS, mut="no_between")
        assert not inside(er, rstd, drstd)


@pytest.mark.parametrize("kind", ["bf16", "f16", "h2"])
@pytest.mark.parametrize("N,K", [(1, 64), (5, 200), (8, 768)])
def test_fold_ln_weight_emulation_inside_the_bound(N, K, kind):
    if kind == "h2" and K % 8:
        K = 64
    W, gamma, beta, bias = R.make_fold_case(N, K, seed=K + N, with_bias=N != 5)
    ref = R.fold_ln_weight_reference(W, gamma, beta, bias, kind)
    Wp, c, bf = R.fold_ln_weight_emulate(W, gamma, beta, bias, kind)
    assert torch.equal(Wp, ref["Wp"])
    assert check_within(c, ref["c"], ref["c_bound"]) <= 1.0 and check_within(bf, ref["bias_f"], ref["bias_bound"]) <= 1.0


@pytest.mark.parametrize("K", [64, 768])
def test_fold_ln_weight_c_from_unrounded_products_fails_at_bf16(K):
    W, gamma, beta, bias = R.make_fold_case(8, K, seed=K + 8)
    ref = R.fold_ln_weight_reference(W, gamma, beta, bias, "bf16")
    _, c, _ = R.fold_ln_weight_emulate(W, gamma, beta, bias, "bf16", mut="c_unrounded")
    assert not inside(c, ref["c"], ref["c_bound"])


# ---- small ops -------------------------------------------------------------------------------------------------------------------------------------
def test_small_op_emulations_inside_their_bounds():
    om, bound = R.gaussian_bias_reference(3, 5, 1.0)
    cell = torch.arange(15)
    y, x = (cell // 5).float(), (cell % 5).float()
    d2 = (y[:, None] - y[None]) ** 2 + (x[:, None] - x[None]) ** 2
    assert check_within(torch.exp(-d2 * torch.tensor(0.5)), om, bound) <= 1.0
    assert not inside(torch.exp(-d2 * torch.tensor(0.5)).view(3, 5, 3, 5).permute(1, 0, 3, 2).reshape(15, 15), om, bound)  # gh / gw swapped
    g = torch.Generator().manual_seed(9)
    for dh in (32, 80):
        v = torch.randn(2, 7, 3, dh, generator=g)
        nrm, bound = R.head_norms_reference(v, 2, 7, 3, dh)
        assert check_within(torch.sqrt(R.lane_sum(v * v)).permute(0, 2, 1), nrm, bound) <= 1.0
    yv, xv = torch.randn(257, generator=g), torch.randn(257, generator=g)
    r, bound = R.axpby_reference(yv, xv, 0.3, -1.7)
    assert check_within(torch.tensor(0.3) * xv + torch.tensor(-1.7) * yv, r, bound) <= 1.0
    for N in (1, 3, 5, 197):
        v = torch.randn(2, N, 100, generator=g)
        out, bound = R.gem_inv_temp_reference(v, 0.07)
        nr = torch.sqrt(R.lane_sum(v * v))
        acc = torch.zeros(2, 4)
        for t in range(N):
            acc[:, t % 4] = acc[:, t % 4] + nr[:, t]
        emu = ((acc[:, 0] + acc[:, 1]) + acc[:, 2] + acc[:, 3]) / float(N) * torch.tensor(0.07)
        assert check_within(emu, out, bound) <= 1.0


# ---- pack / transpose / patchify: exact --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_pack_references_round_once_and_pad_with_zeros(kind):
    g = torch.Generator().manual_seed(11)
    src = torch.randn(5, 24, generator=g) * 300.0
    ref = R.pack_rows_reference(src, 19, 24, kind)
    assert bool((ref[:, 19:] == 0).all())
    assert torch.equal(ref[:, :19], R.rounded_once(src[:, :19].contiguous(), kind) if kind != "h2" else ref[:, :19])
    if kind in ("bf16", "f16"):
        assert torch.equal(ref[:, :19], src[:, :19].to(R.storage_dtype(kind)).double())
    else:
        assert float((ref[:, :19] - src[:, :19].double()).abs().max()) <= float(R.out_bound(src.double().abs(), kind).max())
    t = R.transpose_pack_reference(src[:, :8].contiguous().t().contiguous(), kind)       # [8, 5] -> [5, 8]
    assert t.shape == (5, 8) and torch.equal(t, R.rounded_once(src[:, :8].contiguous(), kind))


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("mut", ["layout_swapped", "pad_swapped", "pxpy_swapped"])
def test_patchify_mutations_fail(mut, u8):
    c = R.make_patch_case(4, 2, 3, u8, seed=4)
    args = (c["scene"], c["windows"], c["scene_index"], c["tile_h"], c["tile_w"], c["pad_l"], c["pad_t"], 2, 3, 4, 64)
    ref, mask = R.patchify_reference(*args)
    assert bool((ref[:, 48:] == 0).all()) and bool((ref[~mask] == 0).all()) and int(mask.sum()) == 2 * 3 * c["tile_h"] * c["tile_w"]
    lo, hi = R.patchify_interval(ref, u8, "f32")
    got, _ = R.patchify_reference(*args, mut=mut)
    assert not bool(((got >= lo) & (got <= hi)).all())


def test_patchify_u8_normalisation_in_f32():
    """(u - mean) / std over every u and channel against the f64 value.  Plain IEEE f32 -- subtract, divide -- is within half an ulp where
    the subtraction is exact (|u - mean| < 128) but up to 1.37 ulp beyond it (channel 2, mean 104.094, from u = 233: the subtraction rounds
    too), which misses the 1 ulp the GPU module holds the kernel to.  The kernel's form -- the subtraction's exact residual e and the
    division's remainder folded back where e != 0 -- is within 1 ulp everywhere (0.5 observed) and bit-identical to the plain form wherever
    e == 0."""
    f = np.float32
    u = np.arange(256, dtype=np.float32)
    worst_plain, worst_kernel = [], []
    for ch in range(3):
        m, s = f(R.PATCH_MEAN[ch]), f(R.PATCH_STD[ch])
        d = (u - m).astype(np.float32)
        e = ((u - d).astype(np.float32) - m).astype(np.float32)
        assert np.array_equal(d.astype(np.float64) + e.astype(np.float64), u.astype(np.float64) - np.float64(m))     # the residual is exact
        q = (d / s).astype(np.float32)
        r = (d.astype(np.float64) - q.astype(np.float64) * np.float64(s)).astype(np.float32)                          # fmaf(-q, std, d)
        v = np.where(e != 0, (q + ((r + e).astype(np.float32) / s).astype(np.float32)).astype(np.float32), q)
        exact = (u.astype(np.float64) - np.float64(m)) / np.float64(s)
        ulp = 2 * R.half_ulp(torch.from_numpy(np.abs(exact)), "f32").numpy()
        worst_plain.append(float((np.abs(q - exact) / ulp).max()))
        worst_kernel.append(float((np.abs(v - exact) / ulp).max()))
        assert np.array_equal(e != 0, np.abs(u.astype(np.float64) - np.float64(m)) >= 128) or ch != 2
        assert np.array_equal(v[e == 0], q[e == 0])
    print("patchify u8 -> f32, worst error in ulp per channel: plain", worst_plain, "kernel", worst_kernel)
    assert max(worst_plain) > 1.0                                        # the plain form would fail the 1-ulp check ...
    assert max(worst_kernel) <= 1.0                                      # ... the kernel's form passes it


# ---- refusals made before any launch (visible without a GPU) ---------------------------------------------------------------------------------------
def test_row_entry_refusals_without_gpu():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(1 << 20)                                           # never dereferenced: every call below is refused before any launch
    tiles = _lib.TileBatch(scene=1 << 20, format=0, scene_h=64, scene_w=64, windows=1 << 20, scene_index=None, scene_stride=0, n_tiles=1,
                           tile_h=20, tile_w=20, pad_l=5, pad_t=3, grid_h=2, grid_w=2)

    def patch(P=14, Kpad=640, kind=0, **kw):
        t = _lib.TileBatch.from_buffer_copy(tiles)
        for k, v in kw.items():
            setattr(t, k, v)
        return lib.sg_patchify_raw(C.byref(t), P, Kpad, p, kind, None)

    cases = [
        (lambda: lib.sg_layernorm_raw(p, 2052, p, p, p, 2052, 0, 1, 2052, 1e-5, None), b"layernorm: D=2052"),
        (lambda: lib.sg_layernorm_raw(p, 8, p, p, p, 8, 0, 1, 6, 1e-5, None), b"layernorm: D=6"),
        (lambda: lib.sg_layernorm_raw(p, 66, p, p, p, 64, 0, 1, 64, 1e-5, None), b"row strides must be multiples of 4"),
        (lambda: lib.sg_layernorm_raw(p, 12, p, p, p, 16, 4, 1, 12, 1e-5, None), b"two-plane f16 output needs D"),
        (lambda: lib.sg_layernorm_raw(p, 64, p, p, p, 64, 2, 1, 64, 1e-5, None), b"bad kind 2"),
        (lambda: lib.sg_layernorm_raw(None, 64, p, p, p, 64, 0, 1, 64, 1e-5, None), b"null pointer"),
        (lambda: lib.sg_layernorm_fp8_raw(p, 64, p, p, p, 66, p, 1, 64, 1e-5, None), b"layernorm_fp8: row strides"),
        (lambda: lib.sg_quantize_rows_raw(p, 0, 6, p, 8, p, 1, 6, None), b"quantize_rows_fp8: D=6"),
        (lambda: lib.sg_quantize_rows_raw(p, 4, 8, p, 8, p, 1, 8, None), b"bad kind 4"),
        (lambda: lib.sg_embed_assemble_raw(p, 66, p, p, p, p, p, 1, 2, 64, 1e-5, None), b"embed_assemble: unsupported"),
        (lambda: lib.sg_posembed_resize_raw(p, 16, 8, 2, 16, 1, p, None), b"posembed_resize: downscale"),
        (lambda: lib.sg_pack_rows_raw(p, 2, 10, 10, p, 12, 4, None), b"pack_rows: two-plane"),
        (lambda: lib.sg_transpose_pack_raw(p, 12, 3, p, 4, None), b"transpose_pack: two-plane"),
        (lambda: lib.sg_ln_stats_finalize_raw(p, 4, 100, 1e-5, p, None), b"ln_stats_finalize: D=100"),
        (lambda: lib.sg_fold_ln_weight_raw(p, 4, 64, p, p, None, 0, p, p, p, None), b"fold_ln_weight: 2-byte"),
        (lambda: lib.sg_fold_ln_weight_raw(p, 4, 60, p, p, None, 4, p, p, p, None), b"fold_ln_weight: two-plane"),
        (lambda: lib.sg_l2norm_rows_raw(p, 4, 12, 0, 1, p, 0, 12, 0, 2, 8, 1e-12, None), b"l2norm_rows: two-plane"),
        (lambda: lib.sg_softmax_rows_raw(p, 8, 8, 8, 1, None, 1.0, None, 0.0, 0, None, None, 2, 0, 0, p, None, None), b"mode=2"),
        (lambda: patch(Kpad=576), b"patchify: Kpad too small"),
        (lambda: patch(tile_h=26), b"patchify: grid does not cover"),
        (lambda: patch(n_tiles=0), b"patchify: empty batch"),
        (lambda: patch(n_tiles=65536), b"patchify: too many tiles"),
        (lambda: patch(P=4, Kpad=52, kind=4, tile_h=4, tile_w=2), b"patchify: two-plane"),
    ]
    for call, msg in cases:
        assert call() != 0, msg
        assert msg in lib.sg_last_error(), (msg, lib.sg_last_error())
