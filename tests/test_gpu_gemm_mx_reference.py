"""The MXFP8 forms of the fp8 GEMM (sg_gemm_fp8_mx_raw: the 256 x 256 ring kernel with a block-scaled operand through the scale operand of
v_mfma_scale_f32_16x16x128_f8f6f4 and / or a block-scaled output out of the epilogue) against float64 references, element by element
(tests/gemm_reference.py: `mx_decode`, `mx_scale_rule`, `mx_output_check`, and `gemm_bound` with, for a block-scaled operand, the matrix
unit's measured 13-bit alignment inside its groups of 16 K as the one added term `f8_align_bound` -- the hardware model is stated there; tests/test_gemm_mx_bound_cpu.py shows what the checks catch).  Every case
  * pre-fills C, c_mx and c_mx_scale with 0xFF between guard bands and checks the bands (0xFF is NaN in e4m3, bf16 and f32 and the E8M0 NaN:
    a cell never written fails),
  * asserts from sg_gemm_last_kernel() which of the five instantiations ran (_fc1 / _fc2 / _proj / _mxa / _out) on ceil(M/256) ceil(N/256) tiles,
  * compares every element.
Shapes are the smallest the dispatch accepts (M >= 1024, N >= 256) that reach the edges: M = 1030 (five row tiles, the last 6 rows deep),
N = 264 (a last column tile 8 wide) or, with an MX output, 384 (a half-filled one); K = 128 / 256 / 640 (one step, exactly the two stages,
five steps: the ring wraps); 4 tiles (fewer than the 8 XCDs of the tile order) and 10 (two XCDs carry one tile more).
No scale byte 255 and no NaN data is ever fed, and every operand, product and sum stays a normal f32."""
import pytest
import torch

from gemm_reference import (check_within, f8_align_bound, gemm_bound, gemm_reference, mx_coherent_operands, mx_decode, mx_exact_table, mx_output_check)
from test_gpu_gemm_reference import DEV, GUARD, Guarded, _lib, cdiv, expect_record, ptr, quantize_fp8, reset, rnd, stream

pytestmark = pytest.mark.gpu

FAM = "fp8_mx_ring256x256_"
AMBIGUOUS_CAP = 1e-3                                              # share of blocks whose reference maximum lies within B of a scale threshold
RESULTS = {}                                                      # form -> [cases, largest err / bound, largest ambiguous share]
F8 = torch.float8_e4m3fn


def record(form, ratio, ambiguous=0.0):
    n, worst, amb = RESULTS.get(form, (0, 0.0, 0.0))
    RESULTS[form] = (n + 1, max(worst, ratio), max(amb, ambiguous))


def e4m3_bytes(x):
    """f32 -> e4m3 bytes (torch's conversion on the host: round to nearest even; values here are far inside +-448)."""
    return x.cpu().to(F8).view(torch.uint8).to(DEV)


def dec8(b8, scale):
    return b8.view(F8).to(torch.float32).double() * scale.double()[:, None]


def block_scales(K, M, lo, hi, seed):
    """E8M0 bytes [K/128][M][4], independent per (step, row, block), uniform in [lo, hi]."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(lo, hi + 1, (K // 128, M, 4), generator=g, device=DEV, dtype=torch.uint8)


def launch(M, N, K, *, a8, sa=None, a_mx=None, W8, sw, bias=None, R=None, act=0, out="f32", family, alias=False):
    """One sg_gemm_fp8_mx_raw call with every output buffer guarded and pre-filled; `out` is "f32", "bf16" or "mx" (then C must stay untouched);
    alias: the residual IS C (the tower's in-place proj).  Returns (C, c8, cs, record)."""
    lib = _lib()
    c = Guarded((M, N), torch.bfloat16 if out == "bf16" else torch.float32)
    c8 = Guarded((M, N), torch.uint8) if out == "mx" else None
    cs = Guarded((N // 128, M, 4), torch.uint8) if out == "mx" else None
    res = R
    if alias:
        c.c.copy_(R)
        res = c.c
    try:
        rc = lib.sg_gemm_fp8_mx_raw(ptr(a8), ptr(sa), ptr(a_mx), ptr(W8), ptr(sw), ptr(bias), ptr(res), ptr(c.c), ptr(c8.c if c8 is not None else None),
                                    ptr(cs.c if cs is not None else None), M, N, K, act, int(out == "bf16"), stream())
        assert rc == 0, lib.sg_last_error()
        rec = expect_record(FAM + family, cdiv(M, 256) * cdiv(N, 256))
    finally:
        reset()
    torch.cuda.synchronize()
    for gbuf in (c, c8, cs):
        if gbuf is not None:
            gbuf.check_guards()
    if out == "mx":
        assert bool((c.buf[GUARD:GUARD + c.n] == 0xFF).all()), "an MX-output call wrote to C"
        return None, c8.c, cs.c, rec
    return c.c, None, None, rec


# ---- MX output: row-scaled A, the epilogue writes e4m3 + one scale byte per 32 columns ---------------------------------------------------------
def fc_operands(M, N, K, seed, row_gain=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    A, W = mx_coherent_operands(M, N, K, g, device=DEV, row_gain=row_gain)
    return A, W, rnd(N, seed=seed + 1, scale=0.1)


def run_mx_out(M, N, K, act, family, *, A, W, bias, form):
    A8, sa = quantize_fp8(A)
    W8, sw = quantize_fp8(W)
    _, c8, cs, rec = launch(M, N, K, a8=A8, sa=sa, W8=W8, sw=sw, bias=bias, act=act, out="mx", family=family)
    Aref, Wref = dec8(A8, sa), dec8(W8, sw)
    pre, ref = gemm_reference(Aref, Wref, bias, None, act)
    B = gemm_bound(Aref, Wref, bias, pre, ref, act=act, out_fmt="f32")
    what = f"{form} M={M} N={N} K={K} act={act} [{rec}]"
    ratio, ambiguous = mx_output_check(c8, cs, ref, B, what)
    print(f"{what}: max err/bound {ratio:.3g}, ambiguous blocks {100 * ambiguous:.4f} %")
    record(form, ratio, ambiguous)
    assert ambiguous <= AMBIGUOUS_CAP, f"{what}: {ambiguous} of the blocks accept either scale byte"
    return c8, cs


_FC1 = {}


def fc1_output():
    """Case 1's first run, (1030, 384, 256) QuickGELU: computed and checked once, shared with the hand-off case."""
    if not _FC1:
        A, W, bias = fc_operands(1030, 384, 256, seed=400)
        _FC1["out"] = run_mx_out(1030, 384, 256, 1, "fc1", A=A, W=W, bias=bias, form="fc_form")
    return _FC1["out"]


def test_fc_form_quickgelu():
    """SPEC 2: per-row sa, MX output after QuickGELU; 5 x 2 tiles, the second column tile half filled, exactly STAGES K steps."""
    fc1_output()


def test_fc_form_gelu():
    """SPEC 3: MX output after GELU; 4 tiles, one K step."""
    A, W, bias = fc_operands(1024, 256, 128, seed=410)
    run_mx_out(1024, 256, 128, 2, "fc2", A=A, W=W, bias=bias, form="fc_form")


def test_generic_mx_output_wide_rows_and_zero_blocks():
    """The run-time mx_out body without activation, five K steps.  A's rows span 1e-6 .. 1e6; rows 7 and 1029 of A are zero and the bias is zero
    on columns 128-255: those blocks must come back as scale byte 0 with data bytes 0x00."""
    M, N, K = 1030, 384, 640
    A, W, bias = fc_operands(M, N, K, seed=420, row_gain=torch.logspace(-6, 6, M, device=DEV))
    A[7] = 0
    A[1029] = 0
    bias[128:256] = 0
    c8, cs = run_mx_out(M, N, K, 0, "out", A=A, W=W, bias=bias, form="generic c_mx")
    for r in (7, 1029):
        assert bool((cs[1, r] == 0).all()) and bool((c8[r, 128:256] == 0).all()), f"row {r}: an all-zero block is scale 0, bytes 0x00"
        assert bool((cs[0, r] != 0).all()) and bool((cs[2, r] != 0).all())              # the bias alone elsewhere in these rows


def test_exact_table():
    """Block maxima of exactly 448 2^k (E = 127 + k kept, byte 0x7e), 464 2^k (E + 1, 232 -> 224: the tie to even) and 480 2^k (E + 1, 240), k = -20,
    0, 20, all-zero rows (scale 0, bytes 0x00); every sum is exact in f32, so scale and data bytes must EQUAL the written table of
    tests/gemm_reference.py -- no bound, no ambiguous block."""
    M, N, K = 1024, 256, 128
    A8, sa, W8, sw, want8, wants = mx_exact_table(M, N, K, DEV)
    _, c8, cs, _ = launch(M, N, K, a8=A8, sa=sa, W8=W8, sw=sw, act=0, out="mx", family="out")
    bad_s, bad_d = cs != wants, c8 != want8
    assert not bool(bad_s.any()), f"{int(bad_s.sum())} scale bytes differ from the table; first at {tuple(bad_s.nonzero()[0].tolist())}"
    assert not bool(bad_d.any()), f"{int(bad_d.sum())} data bytes differ from the table; first at {tuple(bad_d.nonzero()[0].tolist())}"
    record("exact table", 0.0)


# ---- MX operand: A with one E8M0 scale per (row, 32 K elements) ----------------------------------------------------------------------------------
def run_mxa(M, N, K, *, act=0, out="f32", bias=True, residual=False, alias=False, family, form, seed, scale_range=(111, 143), zero_block=False):
    a8 = e4m3_bytes(rnd(M, K, seed=seed))
    a_mx = block_scales(K, M, *scale_range, seed=seed + 1)
    if zero_block:                                                 # K block 2 of every fourth row: data bytes 0, scale byte 0 (2^-127)
        a8[::4, 64:96] = 0
        a_mx[0, ::4, 2] = 0
    W8, sw = quantize_fp8(rnd(N, K, seed=seed + 2, scale=K ** -0.5))
    b = rnd(N, seed=seed + 3, scale=0.1) if bias else None
    R = rnd(M, N, seed=seed + 4) if residual else None
    R0 = R.clone() if alias else R                                 # the reference's residual: a copy made before the launch
    got, _, _, rec = launch(M, N, K, a8=a8, a_mx=a_mx, W8=W8, sw=sw, bias=b, R=R, act=act, out=out, family=family, alias=alias)
    Aref, blk = mx_decode(a8, a_mx)
    assert int(blk.max()) < 255
    Wref = dec8(W8, sw)
    pre, ref = gemm_reference(Aref, Wref, b, R0, act)
    bound = gemm_bound(Aref, Wref, b, pre, ref, act=act, out_fmt=out, extra_pre=f8_align_bound(a8, W8, blk) * sw.double()[None, :])
    what = f"{form} M={M} N={N} K={K} act={act} out={out} res={residual} alias={alias} scales={scale_range} [{rec}]"
    ratio = check_within(got, ref, bound, what)
    print(f"{what}: max err/bound {ratio:.3g}")
    record(form, ratio)


@pytest.mark.parametrize("M,N,K,alias", [(1030, 264, 640, False), (1024, 256, 128, False), (1030, 264, 640, True)])
def test_proj_form(M, N, K, alias):
    """SPEC 4 with MXA: f32 C + residual, no activation; once with the residual aliased to C, as the tower calls it."""
    run_mxa(M, N, K, residual=True, alias=alias, family="proj", form="proj_form", seed=500 + K + int(alias))


@pytest.mark.parametrize("act", [0, 1, 2])
def test_mx_operand_generic_bf16(act):
    run_mxa(1030, 264, 256, act=act, out="bf16", family="mxa", form="generic MXA", seed=520 + act)


def test_mx_operand_generic_f32_no_residual():
    run_mxa(1030, 264, 384, act=2, bias=False, family="mxa", form="generic MXA", seed=530)


def test_proj_form_wide_spread():
    """Scale bytes in [87, 167]: blocks of one K step up to 2^80 apart; every product and sum still a normal f32."""
    run_mxa(1030, 264, 640, residual=True, family="proj", form="proj_form wide spread", seed=540, scale_range=(87, 167))


def test_proj_form_zero_block():
    """K block 2 of every fourth row: bytes 0 under scale byte 0 -- contributes exactly 0, and the result is finite."""
    run_mxa(1030, 264, 640, residual=True, family="proj", form="proj_form zero block", seed=550, zero_block=True)


def test_mx_operand_with_mx_output():
    """Block-scaled A and MX output in one call (the generic MXA body with the run-time mx_out), QuickGELU, three K steps."""
    M, N, K = 1030, 384, 384
    g = torch.Generator(device=DEV).manual_seed(560)
    A, W = mx_coherent_operands(M, N, K, g, device=DEV, row_gain=torch.ones(M, device=DEV))
    a8 = e4m3_bytes(A)
    a_mx = block_scales(K, M, 111, 143, seed=561)
    W8, sw = quantize_fp8(W * 2.0 ** -12)                          # the largest blocks of A are ~2^16: keeps |pre-activation| <~ 100, where
                                                                   # QuickGELU's own error term (4 |x| + 3) 2^-23 |y| stays ~1e-5 of the value
    bias = rnd(N, seed=562, scale=0.1)
    _, c8, cs, rec = launch(M, N, K, a8=a8, a_mx=a_mx, W8=W8, sw=sw, bias=bias, act=1, out="mx", family="mxa")
    Aref, Wref = mx_decode(a8, a_mx)[0], dec8(W8, sw)
    pre, ref = gemm_reference(Aref, Wref, bias, None, 1)
    B = gemm_bound(Aref, Wref, bias, pre, ref, act=1, out_fmt="f32")
    what = f"MXA + c_mx M={M} N={N} K={K} act=1 [{rec}]"
    ratio, ambiguous = mx_output_check(c8, cs, ref, B, what)
    print(f"{what}: max err/bound {ratio:.3g}, ambiguous blocks {100 * ambiguous:.4f} %")
    record("MXA + c_mx", ratio, ambiguous)
    assert ambiguous <= AMBIGUOUS_CAP


def test_hand_off():
    """Producer and consumer agree on the layout: the fc form's own (c8, cs) as the proj form's operand (K = 384, N = 264), against the f64
    product of the decoded bytes."""
    c8, cs = fc1_output()
    M, K, N = 1030, 384, 264
    assert not bool(((c8 & 0x7F) == 0x7F).any()) and not bool((cs == 255).any())           # never feed NaN data or a NaN scale
    W8, sw = quantize_fp8(rnd(N, K, seed=570, scale=K ** -0.5))
    b, R = rnd(N, seed=571, scale=0.1), rnd(M, N, seed=572)
    got, _, _, rec = launch(M, N, K, a8=c8, a_mx=cs, W8=W8, sw=sw, bias=b, R=R, act=0, out="f32", family="proj")
    (Aref, blk), Wref = mx_decode(c8, cs), dec8(W8, sw)
    pre, ref = gemm_reference(Aref, Wref, b, R, 0)
    bound = gemm_bound(Aref, Wref, b, pre, ref, act=0, out_fmt="f32", extra_pre=f8_align_bound(c8, W8, blk) * sw.double()[None, :])
    ratio = check_within(got, ref, bound, f"hand-off [{rec}]")
    print(f"hand-off fc_form -> proj_form [{rec}]: max err/bound {ratio:.3g}")
    record("hand-off", ratio)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
REFUSALS = {"M = 1023": dict(M=1023, mxa=True), "N = 248": dict(N=248, mxa=True), "c_mx with N = 264": dict(N=264, mx_out=True),
            "c_mx with a residual": dict(mx_out=True, residual=True), "both sa and a_mx": dict(mxa=True, both=True),
            "neither sa nor a_mx": dict(neither=True), "c_mx without c_mx_scale": dict(mx_out=True, no_scale=True)}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals(case):
    """A refused call returns non-zero with a message, launches nothing (the record reads "none" although a valid call went before) and leaves C,
    c_mx, c_mx_scale and their guard bands untouched."""
    lib = _lib()
    kw = REFUSALS[case]
    M, N, K = kw.get("M", 1024), kw.get("N", 256), 128
    def operands(M_, N_):
        return (torch.zeros(M_, K, dtype=torch.uint8, device=DEV), torch.zeros(N_, K, dtype=torch.uint8, device=DEV), torch.ones(N_, device=DEV),
                torch.ones(M_, device=DEV), torch.full((K // 128, M_, 4), 127, dtype=torch.uint8, device=DEV))
    a8, W8, sw, sa, a_mx = operands(1024, 256)                     # a valid call first: the record is not "none"
    launch(1024, 256, K, a8=a8, a_mx=a_mx, W8=W8, sw=sw, R=torch.zeros(1024, 256, device=DEV), family="proj")
    assert lib.sg_gemm_last_kernel() != b"none"
    a8, W8, sw, sa, a_mx = operands(M, N)
    R = torch.zeros(M, N, device=DEV) if kw.get("residual") else None
    c = Guarded((M, N), torch.float32)
    c8 = Guarded((M, N), torch.uint8)
    cs = Guarded((cdiv(N, 128), M, 4), torch.uint8)
    use_sa = kw.get("both") or not (kw.get("mxa") or kw.get("neither"))
    use_mx = kw.get("mxa") and not kw.get("neither")
    mx_out = kw.get("mx_out")
    rc = lib.sg_gemm_fp8_mx_raw(ptr(a8), ptr(sa if use_sa else None), ptr(a_mx if use_mx else None), ptr(W8), ptr(sw), None, ptr(R), ptr(c.c),
                                ptr(c8.c if mx_out else None), ptr(cs.c if mx_out and not kw.get("no_scale") else None), M, N, K, 0, 0, stream())
    assert rc != 0, f"{case}: accepted"
    assert len(lib.sg_last_error()) > 0
    assert lib.sg_gemm_last_kernel() == b"none"
    torch.cuda.synchronize()
    for gbuf in (c, c8, cs):
        gbuf.check_guards()
        assert bool((gbuf.buf[GUARD:GUARD + gbuf.n] == 0xFF).all()), f"{case}: a refused call wrote to an output"


def test_summary():
    """Prints the number of cases, the largest err / bound and the largest ambiguous-block share per form (run last in this module)."""
    for form in sorted(RESULTS):
        n, worst, amb = RESULTS[form]
        print(f"SUMMARY MX {form}: {n} cases, largest err/bound {worst:.3g}, ambiguous blocks {100 * amb:.4f} %")
