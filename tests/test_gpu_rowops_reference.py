"""The row kernels of csrc/rowops.hip and csrc/patchify.hip against the f64 references of tests/rowops_reference.py, element by element,
each through its raw C entry (sg_*_raw: one host function, arguments one to one).  Every output and scale buffer sits between two 64 KiB
guard bands of a sentinel; the gaps inside a buffer (row strides larger than the row, the yo / yi strides) must keep the sentinel too.
Written cells are held to a bound built from the operand magnitudes; packing, transposing and patchifying from f32 and the fp8 bytes are
exact.  The shapes take the branches the tower tests never reach: D % 256 != 0, rows % 4 != 0, strides larger than the row, non-square
grids, the short-row kernels behind rows >= 4096.  tests/test_rowops_bound_cpu.py shows on the same generators that the bounds hold for
f32 arithmetic and fail the listed mutations."""
import ctypes as C
import os
import sys
from collections import defaultdict

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_reference as R                                            # noqa: E402
from rowops_reference import check_within                               # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 1 << 16
SENT = {torch.float32: -12345.5, torch.bfloat16: -12345.5, torch.float16: -1234.5, torch.uint8: 0xA5}
EPS = 1e-5
WORST = defaultdict(float)                    # (op, case) -> largest err / bound


@pytest.fixture(scope="module")
def lib():
    from clip_decontamination_amd import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


KEEP = []                                     # device copies of a call's inputs, alive until ok() has synchronised


def PD(t):
    """Device pointer of a copy of the CPU tensor t; the copy lives until the call it feeds has finished (ok())."""
    KEEP.append(t.to(DEV))
    return P(KEEP[-1])


class Guarded:
    """`numel` elements of `dtype` on the device, sentinel-filled, between two guard bands; `.view` is the payload (1-D)."""

    def __init__(self, numel, dtype, init=None):
        self.sent = torch.tensor(SENT[dtype], dtype=dtype)
        self.g = GUARD // self.sent.element_size()
        self.big = torch.full((2 * self.g + numel,), SENT[dtype], dtype=dtype, device=DEV)
        self.view = self.big[self.g:self.g + numel]
        if init is not None:
            self.view.copy_(init.reshape(-1))

    def finish(self):
        """Guard bands intact -> the payload on the CPU."""
        torch.cuda.synchronize()
        s = self.sent.to(DEV)
        assert bool((self.big[:self.g] == s).all()) and bool((self.big[self.g + self.view.numel():] == s).all()), "guard band overwritten"
        return self.view.cpu()

    def is_sentinel(self, cpu_vals):
        return cpu_vals == self.sent


def rows_out(payload, rows, ld, D, kind):
    """Split a strided output payload (storage elements) into (written [rows, storage D], gaps): row stride `ld` logical elements."""
    m = 2 if kind == "h2" else 1
    buf = payload.view(rows, ld * m)
    return buf[:, :D * m], buf[:, D * m:]


def record(op, case, ratio):
    WORST[(op, case)] = max(WORST[(op, case)], ratio)


def ok(lib, rc):
    torch.cuda.synchronize()
    KEEP.clear()
    assert rc == 0, lib.sg_last_error()


# ---- layernorm ---------------------------------------------------------------------------------------------------------------------------------
# two-plane rows are multiples of 8 elements: those cases use the multiples of 8 among the sizes (the refusal is checked on the CPU)
@pytest.mark.parametrize("D,kind", [(D, k) for D in R.LN_D for k in R.KINDS if k != "h2" or D % 8 == 0])
@pytest.mark.parametrize("rows", R.LN_ROWS)
def test_layernorm_vs_f64(lib, rows, D, kind):
    x, g, b = R.make_ln_case(rows, D, seed=D + rows)
    ldx, ldy = D + 4, D + 8
    xb = torch.full((rows, ldx), 3e30)                                   # the stride padding must never be read into the statistics
    xb[:, :D] = x
    m = 2 if kind == "h2" else 1
    out = Guarded(rows * ldy * m, R.storage_dtype(kind))
    ok(lib, lib.sg_layernorm_raw(PD(xb), ldx, PD(g), PD(b), P(out.view), ldy, R.PREC[kind], rows, D, EPS, stream()))
    got, gap = rows_out(out.finish(), rows, ldy, D, kind)
    assert bool(out.is_sentinel(gap).all()), "the gap between rows was written"
    y, bound, _ = R.layernorm_reference(x, g, b, EPS, kind)
    record("layernorm " + kind, f"rows {rows} D {D}", check_within(R.load(got, kind), y, bound, f"layernorm {kind} rows {rows} D {D}"))


# ---- fp8 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiny", [False, True], ids=["plain", "tiny"])
@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_fp8_vs_f64(lib, D, tiny):
    """`tiny`: every row's amax near 1e-37 (suspect 1: finite bytes, the floored scale), the constant row all zero (scale 1, zero bytes)."""
    rows, ldx, ldy = 5, D + 4, D + 8
    x, g, b = R.make_ln_fp8_case(rows, D, seed=D + 5, tiny=tiny)
    xb = torch.full((rows, ldx), 3e30)
    xb[:, :D] = x
    out, sc = Guarded(rows * ldy, torch.uint8), Guarded(rows, torch.float32)
    ok(lib, lib.sg_layernorm_fp8_raw(PD(xb), ldx, PD(g), PD(b), P(out.view), ldy, P(sc.view), rows, D, EPS, stream()))
    byte, gap = rows_out(out.finish(), rows, ldy, D, "u8")
    scale = sc.finish()
    assert bool((gap == 0xA5).all())
    print(f"layernorm_fp8 D {D} tiny {tiny}: scale {scale.tolist()}, row 0 bytes {byte[0, :8].tolist()}")
    assert bool(torch.isfinite(scale).all()) and not bool(torch.isnan(R.e4m3_value(byte)).any()), "inf scale / NaN bytes"
    share, ratio = R.layernorm_fp8_check(byte, scale, x, g, b, EPS, f"layernorm_fp8 D {D} tiny {tiny}")
    print(f"layernorm_fp8 D {D} tiny {tiny}: {share:.3%} of the elements on an e4m3 rounding boundary")
    record("layernorm_fp8 scale", f"D {D} {'tiny' if tiny else 'plain'}", ratio)
    if tiny:
        assert float(scale[4]) == 1.0 and bool((byte[4] == 0).all())


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("D", R.LN_D)
def test_quantize_rows_exact(lib, D, kind):
    """Bytes and scales bit-identical to the f32 reproduction; the all-zero row (scale 1, zero bytes), the amax = 1e-37 row (suspect 1: finite
    bytes that dequantise within half an e4m3 step), the row maximum in the last lane's last element."""
    rows, ldx, ldy = 5, D + 4, D + 8
    s, v = R.make_quant_case(rows, D, seed=D, kind=kind)
    xb = torch.full((rows, ldx), 7.0, dtype=s.dtype)
    xb[:, :D] = s
    out, sc = Guarded(rows * ldy, torch.uint8), Guarded(rows, torch.float32)
    ok(lib, lib.sg_quantize_rows_raw(PD(xb), R.PREC[kind], ldx, P(out.view), ldy, P(sc.view), rows, D, stream()))
    byte, gap = rows_out(out.finish(), rows, ldy, D, "u8")
    scale = sc.finish()
    assert bool((gap == 0xA5).all())
    print(f"quantize_rows {kind} D {D}: tiny row scale {float(scale[1]):.6g}, bytes {byte[1, :8].tolist()} ... {byte[1, D // 2]}")
    assert float(scale[0]) == 1.0 and bool((byte[0] == 0).all())
    assert bool(torch.isfinite(scale).all()) and bool(torch.isfinite(R.e4m3_value(byte[1])).all()), "the tiny row: inf scale / NaN bytes"
    assert R.fp8_within_half_step(byte, scale, v)
    want_b, want_s = R.quantize_rows_expected(v)
    assert torch.equal(scale, want_s), (scale.tolist(), want_s.tolist())
    assert torch.equal(byte, want_b), f"{int((byte != want_b).sum())} bytes differ"
    assert int(byte[rows - 1, D - 1]) == 0x7e


# ---- embed_assemble ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 260, 768])
@pytest.mark.parametrize("N", [2, 6, 197])
def test_embed_assemble_vs_f64(lib, N, D):
    B, ldp = 2, D + 4
    g = torch.Generator().manual_seed(N * 1000 + D)
    patches = torch.randn(B * (N - 1), D, generator=g)
    cls, pos = torch.randn(D, generator=g), torch.randn(N, D, generator=g) * 0.5
    _, gamma, beta = R.make_ln_case(1, D, seed=D)
    pb = torch.full((B * (N - 1), ldp), 3e30)
    pb[:, :D] = patches
    out = Guarded(B * N * D, torch.float32)
    ok(lib, lib.sg_embed_assemble_raw(PD(pb), ldp, PD(cls), PD(pos), PD(gamma), PD(beta), P(out.view),
                                      B, N, D, EPS, stream()))
    got = out.finish().view(B, N, D)
    y, bound = R.embed_assemble_reference(patches, cls, pos, gamma, beta, EPS, B, N)
    record("embed_assemble", f"N {N} D {D}", check_within(got, y, bound, f"embed_assemble N {N} D {D}"))
    want, wb, _ = R.layernorm_reference((cls + pos[0])[None], gamma, beta, EPS)          # the CLS row is ln(cls + pos[0]) for both images
    for bi in range(B):
        check_within(got[bi, 0], want[0], wb[0], f"CLS row of image {bi}")
    assert torch.equal(got[0, 0], got[1, 0])


# ---- posembed_resize ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["bicubic", "antialias"])
@pytest.mark.parametrize("D", R.RESIZE_D)
@pytest.mark.parametrize("g0,gh,gw", R.RESIZE_CASES)
def test_posembed_resize_vs_f64(lib, g0, gh, gw, D, mode):
    pos = R.make_pos(g0, D, seed=gh * 40 + gw)
    out = Guarded((1 + gh * gw) * D, torch.float32)
    ok(lib, lib.sg_posembed_resize_raw(PD(pos), g0, D, gh, gw, mode, P(out.view), stream()))
    got = out.finish().view(1 + gh * gw, D)
    assert torch.equal(got[0], pos[0]), "position 0 must pass through bit-exact"
    ref, bound = R.posembed_resize_reference(pos, g0, gh, gw, mode)
    record(f"posembed_resize mode {mode}", f"{g0} -> {gh}x{gw} D {D}", check_within(got[1:], ref[1:], bound[1:], f"resize {g0}->{gh}x{gw}"))


def test_posembed_resize_refuses_a_window_over_24_taps(lib):
    pos = R.make_pos(16, 8, seed=0).to(DEV)
    out = Guarded(33 * 8, torch.float32)
    assert lib.sg_posembed_resize_raw(P(pos), 16, 8, 2, 16, 1, P(out.view), stream()) != 0
    assert b"downscale" in lib.sg_last_error()
    assert bool(out.is_sentinel(out.finish()).all())


# ---- pack_rows / transpose_pack ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("rows,cols,cols_pad,ld", [(5, 19, 24, 23), (37, 50, 56, 51), (3, 8, 8, 8)])
def test_pack_rows_exact(lib, rows, cols, cols_pad, ld, kind):
    g = torch.Generator().manual_seed(rows)
    src = torch.randn(rows, ld, generator=g) * 300.0
    m = 2 if kind == "h2" else 1
    out = Guarded(rows * cols_pad * m, R.storage_dtype(kind))
    ok(lib, lib.sg_pack_rows_raw(PD(src), rows, cols, ld, P(out.view), cols_pad, R.PREC[kind], stream()))
    got = R.load(out.finish().view(rows, cols_pad * m), kind)
    assert torch.equal(got, R.pack_rows_reference(src, cols, cols_pad, kind))
    assert bool((got[:, cols:] == 0).all())


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("rows,cols", [(16, 37), (8, 3)])
def test_transpose_pack_exact(lib, rows, cols, kind):
    g = torch.Generator().manual_seed(cols)
    src = torch.randn(rows, cols, generator=g) * 300.0
    m = 2 if kind == "h2" else 1
    out = Guarded(rows * cols * m, R.storage_dtype(kind))
    ok(lib, lib.sg_transpose_pack_raw(PD(src), rows, cols, P(out.view), R.PREC[kind], stream()))
    assert torch.equal(R.load(out.finish().view(cols, rows * m), kind), R.transpose_pack_reference(src, kind))


# ---- folded LayerNorm --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("S", [1, 8, 16])
def test_ln_stats_finalize_vs_f64(lib, S, rows):
    st = R.make_ln_stats_case(S, rows, seed=S)
    out = Guarded(rows * 2, torch.float32)
    ok(lib, lib.sg_ln_stats_finalize_raw(PD(st), rows, 64 * S, EPS, P(out.view), stream()))
    got = out.finish().view(rows, 2)
    mean, rstd, dmean, drstd = R.ln_stats_reference(st, EPS)
    record("ln_stats_finalize mean", f"S {S} rows {rows}", check_within(got[:, 0], mean, dmean, "mean"))
    record("ln_stats_finalize rstd", f"S {S} rows {rows}", check_within(got[:, 1], rstd, drstd, "rstd"))


@pytest.mark.parametrize("K,kind", [(K, k) for K in (64, 200, 768) for k in ("bf16", "f16", "h2") if k != "h2" or K % 8 == 0])
@pytest.mark.parametrize("N", [1, 5, 8])
def test_fold_ln_weight_vs_f64(lib, N, K, kind):
    W, gamma, beta, bias = R.make_fold_case(N, K, seed=K + N, with_bias=N != 5)
    m = 2 if kind == "h2" else 1
    wp, c, bf = Guarded(N * K * m, R.storage_dtype(kind)), Guarded(N, torch.float32), Guarded(N, torch.float32)
    ok(lib, lib.sg_fold_ln_weight_raw(PD(W), N, K, PD(gamma), PD(beta), PD(bias) if bias is not None else None,
                                      R.PREC[kind], P(wp.view), P(c.view), P(bf.view), stream()))
    Wp = wp.finish().view(N, K * m)
    ref = R.fold_ln_weight_reference(W, gamma, beta, bias, kind, Wp_written=Wp)
    bits, want, alt = Wp.view(torch.int16), ref["Wp"].view(torch.int16), ref["Wp_alt"].view(torch.int16)
    assert bool(((bits == want) | (bits == alt)).all()), "W' is the product rounded once"
    if kind == "h2":                                                     # the hi plane has one admissible value; lo: see the reference
        assert torch.equal(bits.view(N, K // 8, 2, 8)[:, :, 0], want.view(N, K // 8, 2, 8)[:, :, 0])
        print(f"fold_ln_weight h2 N {N} K {K}: {int((bits != want).sum())} of {N * K} lo elements come from the contracted product")
    record("fold_ln_weight c " + kind, f"N {N} K {K}", check_within(c.finish(), ref["c"], ref["c_bound"], "c"))
    record("fold_ln_weight bias " + kind, f"N {N} K {K}", check_within(bf.finish(), ref["bias_f"], ref["bias_bound"], "bias_f"))


# ---- l2norm ----------------------------------------------------------------------------------------------------------------------------------------------------
L2_PAIRS = [("f32", "f32"), ("f32", "bf16"), ("f32", "f16"), ("f32", "h2"), ("bf16", "bf16"), ("f16", "f16"), ("h2", "h2"), ("bf16", "f32"),
            ("f16", "f32"), ("h2", "f32")]


def run_l2norm(lib, rows, D, kin, kout, inner, so, si, yo, yi, in_place, lanes, tag, seed, special=True):
    s, v = R.make_l2_case(rows, D, seed=seed, kind=kin, special=special)
    mi, mo = (2 if kin == "h2" else 1), (2 if kout == "h2" else 1)
    outer = -(-rows // inner)
    r = torch.arange(rows)
    xoff, yoff = (r // inner) * so + (r % inner) * si, (r // inner) * yo + (r % inner) * yi
    assert int(xoff.max()) + D <= outer * so and int(yoff.max()) + D <= outer * yo        # every row inside its buffer
    xin = torch.full((outer * so * mi,), SENT[s.dtype], dtype=s.dtype)   # whatever lies between the rows is never read or written
    xin[(xoff * mi)[:, None] + torch.arange(D * mi)[None]] = s
    if in_place:
        out = Guarded(outer * so * mi, s.dtype, init=xin)
        xp = P(out.view)
    else:
        out = Guarded(outer * yo * mo, R.storage_dtype(kout))
        xp = PD(xin)
    ok(lib, lib.sg_l2norm_rows_raw(xp, R.PREC[kin], so, si, inner, P(out.view), R.PREC[kout], yo, yi, rows, D, 1e-12, stream()))
    pay = out.finish()
    idx = (yoff * mo)[:, None] + torch.arange(D * mo)[None]
    got = R.load(pay[idx], kout)
    rest = torch.ones(pay.numel(), dtype=torch.bool)
    rest[idx.reshape(-1)] = False
    assert bool(out.is_sentinel(pay[rest]).all()), "a cell outside the rows was written"
    y, bound = R.l2norm_reference(v, 1e-12, kout, lanes)
    record(f"l2norm_rows {kin}->{kout}" + (" short" if lanes != 64 else ""), tag, check_within(got, y, bound, f"l2norm {kin}->{kout} {tag}"))
    if special and rows >= 3:
        assert bool((got[0] == 0).all()), "a zero row gives a zero row"


@pytest.mark.parametrize("D,kin,kout", [(D, a, b) for D in (1, 63, 64, 65, 768) for a, b in L2_PAIRS if "h2" not in (a, b) or D % 8 == 0])
@pytest.mark.parametrize("rows", [1, 7])
def test_l2norm_rows_general_vs_f64(lib, D, rows, kin, kout):
    """inner = 3 with so, si, yo, yi all different, then in place (same kind) with the input's own strides."""
    Dp = (D + 7) // 8 * 8
    so, si, yo, yi = 3 * Dp + 24, Dp + 8, 3 * Dp + 48, Dp + 16
    run_l2norm(lib, rows, D, kin, kout, 3, so, si, yo, yi, False, 64, f"rows {rows} D {D}", seed=D)
    if kin == kout:
        run_l2norm(lib, rows, D, kin, kout, 3, so, si, so, si, True, 64, f"rows {rows} D {D} in place", seed=D + 1)


@pytest.mark.parametrize("kin,kout", L2_PAIRS)
@pytest.mark.parametrize("rows,D,lanes", [(4101, 8, 8), (4101, 40, 8), (4101, 64, 8), (4099, 72, 16), (4099, 128, 16)])
def test_l2norm_rows_short_kernels_vs_f64(lib, rows, D, lanes, kin, kout):
    """rows >= 4096 with D <= 128, D % 8 == 0: 8 (D <= 64) or 16 lanes own a row; every row has a different norm."""
    run_l2norm(lib, rows, D, kin, kout, 1, D + 8, 0, D + 16, 0, False, lanes, f"rows {rows} D {D}", seed=D, special=False)
    if kin == kout:
        run_l2norm(lib, rows, D, kin, kout, 1, D, 0, D, 0, True, lanes, f"rows {rows} D {D} in place", seed=D + 1, special=False)


# ---- softmax_rows ------------------------------------------------------------------------------------------------------------------------------------------------
def run_softmax(lib, N, variant):
    B, H = 2, 3
    rows, ld = B * H * N, N + 1
    scores, kw = R.make_softmax_case(N, variant, seed=N)
    sb = torch.full((rows, ld), 3e30)
    sb[:, :N] = scores
    pre = kw.get("prefill")
    init = torch.full((rows, ld), SENT[torch.float32])
    if pre is not None:
        init[:, :N] = pre
    out, lse = Guarded(rows * ld, torch.float32, init=init), Guarded(rows, torch.float32)
    ptr = lambda t: PD(t) if t is not None else None                     # noqa: E731
    ok(lib, lib.sg_softmax_rows_raw(PD(sb), ld, rows, N, H, ptr(kw.get("scale_per_image")), kw["scale"], ptr(kw.get("bias")),
                                    kw.get("bias_w", 0.0), kw.get("bias_bstride", 0), ptr(kw.get("rn")), ptr(kw.get("cn")), kw["mode"],
                                    1 if pre is not None else 0,
                                    1 if kw.get("causal") else 0, P(out.view), P(lse.view), stream()))
    got, gap = rows_out(out.finish(), rows, ld, N, "f32")
    assert bool(out.is_sentinel(gap).all())
    ref = R.softmax_reference(scores, B, H, N, **kw)
    return got, lse.finish(), ref


@pytest.mark.parametrize("variant", [v for v in R.SOFTMAX_VARIANTS if v != "mode1_causal"])
@pytest.mark.parametrize("N", R.SOFTMAX_N)
def test_softmax_rows_vs_f64(lib, N, variant):
    got, lse, ref = run_softmax(lib, N, variant)
    z = ref["exact_zero"]
    assert bool((got[z] == 0).all()), "keys after the query must get exactly 0"
    record("softmax_rows " + variant, f"N {N}", check_within(got[~z], ref["out"][~z], ref["bound"][~z], f"softmax {variant} N {N}"))
    record("softmax_rows lse " + variant, f"N {N}", check_within(lse, ref["lse"], ref["lse_bound"], f"lse {variant} N {N}"))


@pytest.mark.parametrize("N", R.SOFTMAX_N)
def test_softmax_rows_mode1_causal_vs_f64(lib, N):
    """Suspect 2: the double softmax with causal masking must write 0 for the keys after the query, as mode 0 does."""
    got, lse, ref = run_softmax(lib, N, "mode1_causal")
    z = ref["exact_zero"]
    record("softmax_rows mode1_causal", f"N {N}", check_within(got[~z], ref["out"][~z], ref["bound"][~z], f"softmax mode1_causal N {N}"))
    record("softmax_rows lse mode1_causal", f"N {N}", check_within(lse, ref["lse"], ref["lse_bound"], f"lse mode1_causal N {N}"))
    assert bool((got[z] == 0).all()), f"keys after the query hold {got[z][:4].tolist()} instead of 0"


# ---- gaussian_bias, head_norms, axpby, gem_inv_temp ----------------------------------------------------------------------------------------------------------------
def test_gaussian_bias_vs_f64(lib):
    gh, gw, std = 3, 5, 1.0
    out = Guarded((gh * gw) ** 2, torch.float32)
    ok(lib, lib.sg_gaussian_bias_raw(gh, gw, std, P(out.view), stream()))
    om, bound = R.gaussian_bias_reference(gh, gw, std)
    record("gaussian_bias", "3x5", check_within(out.finish().view(gh * gw, gh * gw), om, bound, "gaussian_bias"))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dh", [32, 80])
def test_head_norms_vs_f64(lib, dh, kind):
    B, N, H = 2, 7, 3                                                    # N H = 21: the last workgroup is partly idle
    st, sb = H * dh + 8, N * (H * dh + 8) + 16
    g = torch.Generator().manual_seed(dh)
    v = torch.randn(B, N, H * dh, generator=g) * torch.exp2(torch.linspace(-3, 3, N))[None, :, None]
    s = R.store(v, kind)
    m = 2 if kind == "h2" else 1
    xb = torch.full((B * sb * m,), 9.0, dtype=s.dtype)
    off = (torch.arange(B)[:, None] * sb + torch.arange(N)[None] * st).reshape(-1) * m
    xb[off[:, None] + torch.arange(H * dh * m)[None]] = s.view(B * N, H * dh * m)
    out = Guarded(B * H * N, torch.float32)
    ok(lib, lib.sg_head_norms_raw(PD(xb), R.PREC[kind], sb, st, B, N, H, dh, P(out.view), stream()))
    nrm, bound = R.head_norms_reference(R.load(s, kind), B, N, H, dh)
    record("head_norms " + kind, f"dh {dh}", check_within(out.finish().view(B, H, N), nrm, bound, f"head_norms {kind} dh {dh}"))


def test_axpby_vs_f64(lib):
    g = torch.Generator().manual_seed(257)
    y, x = torch.randn(257, generator=g), torch.randn(257, generator=g)
    out = Guarded(257, torch.float32, init=y)
    ok(lib, lib.sg_axpby_raw(P(out.view), PD(x), 0.3, -1.7, 257, stream()))
    r, bound = R.axpby_reference(y, x, 0.3, -1.7)
    record("axpby", "n 257", check_within(out.finish(), r, bound, "axpby"))


@pytest.mark.parametrize("N", [1, 3, 5, 197])
def test_gem_inv_temp_vs_f64(lib, N):
    g = torch.Generator().manual_seed(N)
    v = torch.randn(2, N, 100, generator=g)
    out = Guarded(2, torch.float32)
    ok(lib, lib.sg_gem_inv_temp_raw(PD(v), 2, N, 100, 0.07, P(out.view), stream()))
    ref, bound = R.gem_inv_temp_reference(v, 0.07)
    record("gem_inv_temp", f"N {N}", check_within(out.finish(), ref, bound, f"gem_inv_temp N {N}"))


# ---- patchify ----------------------------------------------------------------------------------------------------------------------------------------------------------
def run_patchify(lib, P_, kpad, u8, kind, seed):
    from clip_decontamination_amd import _lib
    gh, gw = 2, 3
    Kpad = R.std_kpad(P_) + 64 if kpad == "std+64" else (kpad or R.std_kpad(P_))
    c = R.make_patch_case(P_, gh, gw, u8, seed=seed)
    scene, win, sidx = c["scene"].to(DEV), c["windows"].to(DEV), c["scene_index"].to(DEV)           # alive to the end of this function
    assert int(c["windows"][:, 1].max()) <= c["scene_h"] and int(c["windows"][:, 3].max()) <= c["scene_w"]      # windows inside the scene
    tb = _lib.TileBatch(scene=scene.data_ptr(), format=_lib.IMG_U8_NHWC if u8 else _lib.IMG_F32_NCHW, scene_h=c["scene_h"], scene_w=c["scene_w"],
                        windows=win.data_ptr(), scene_index=sidx.data_ptr(), scene_stride=3 * c["scene_h"] * c["scene_w"], n_tiles=2,
                        tile_h=c["tile_h"], tile_w=c["tile_w"], pad_l=c["pad_l"], pad_t=c["pad_t"], grid_h=gh, grid_w=gw)
    m = 2 if kind == "h2" else 1
    rows = 2 * gh * gw
    out = Guarded(rows * Kpad * m, R.storage_dtype(kind))
    ok(lib, lib.sg_patchify_raw(C.byref(tb), P_, Kpad, P(out.view), R.PREC[kind], stream()))
    got = R.load(out.finish().view(rows, Kpad * m), kind)
    ref, mask = R.patchify_reference(c["scene"], c["windows"], c["scene_index"], c["tile_h"], c["tile_w"], c["pad_l"], c["pad_t"], gh, gw, P_, Kpad)
    assert bool((got[~mask] == 0).all()), "padding and the columns >= 3 P P must be exactly zero"
    return got, ref, mask


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("P_,kpad", R.PATCH_SHAPES)
def test_patchify_from_f32_is_the_rounded_copy(lib, P_, kpad, kind):
    got, ref, _ = run_patchify(lib, P_, kpad, False, kind, seed=P_)
    assert torch.equal(got, R.rounded_once(ref, kind))


def test_patchify_from_u8_within_one_ulp(lib):
    """Every shape and output kind from a u8 scene holding all of 0 .. 255 in every channel: the stored value is the rounding of a value
    within 1 ulp (f32) of (u - mean) / std.  The layout, the padding and the zero columns are exact in every case.  The plain f32
    subtract-then-divide misses this by up to 1.37 ulp in channel 2 from u = 233 (|u - 104.094| >= 128: the subtraction rounds too); the
    kernel folds the subtraction's residual back there (tests/test_rowops_bound_cpu.py::test_patchify_u8_normalisation_in_f32)."""
    worst, bad = 0.0, []
    for P_, kpad in R.PATCH_SHAPES:
        for kind in R.KINDS:
            got, ref, mask = run_patchify(lib, P_, kpad, True, kind, seed=P_)
            lo, hi = R.patchify_interval(ref, True, kind)
            inside = (got >= lo) & (got <= hi)
            if kind == "f32":
                ulps = ((got - ref).abs() / (2 * R.half_ulp(ref.abs(), "f32")))[mask]
                worst = max(worst, float(ulps.max()))
                print(f"patchify u8 P {P_} Kpad {kpad}: worst {float(ulps.max()):.3f} ulp, {int((ulps > 1).sum())} of {ulps.numel()} beyond 1 ulp")
            # whatever the last ulp does, the pixel must be the right one: the neighbouring u values are 1 / std ~ 0.014 away
            assert bool(((got - ref).abs() <= 1e-2 * ref.abs().clamp(min=1.0))[mask].all()), f"P {P_} {kind}: wrong pixel"
            if not bool(inside.all()):
                bad.append((P_, kpad, kind, int((~inside).sum())))
    print(f"patchify u8 -> f32: worst error {worst:.3f} ulp; cases with elements beyond 1 ulp: {bad}")
    assert not bad, f"beyond 1 ulp of (u - mean) / std: {bad} (worst {worst:.3f} ulp)"


def test_zz_worst_ratios():
    """Runs last (module order): the err / bound table of the module."""
    print("row kernels, largest err / bound per (op, case):")
    per_op = defaultdict(float)
    for key in sorted(WORST):
        print(f"  {key[0]:>34} | {key[1]:<28} {WORST[key]:.3g}")
        per_op[key[0]] = max(per_op[key[0]], WORST[key])
    print("per operation:", {k: float(f"{v:.3g}") for k, v in sorted(per_op.items())})
    assert WORST and all(v <= 1.0 for v in WORST.values())
