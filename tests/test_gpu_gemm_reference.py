"""Every GEMM kernel the dispatch behind gemm_bf16() reaches, against a float64 reference of the same operation, element by element, with
a per-element bound built from |A|.|W|^T (tests/gemm_reference.py: accumulation, two-plane representation, activation, output rounding --
no constant fitted to observed outputs).  Each case
  * runs on the operands the kernel consumes (bf16 / f16 storage, two-plane storage of f32 values, e4m3 bytes + scales),
  * asserts from sg_gemm_last_kernel() that the intended kernel ran, with the intended grid and N-group size,
  * compares every output element (C is pre-filled with NaN, so an element never written fails),
  * checks that guard bands right before and after C are untouched,
  * and resets the tuning code (-1), the tile order (1000) and the grid cap (2000) whatever happens.
Ragged shapes (M = 4100, N = 2056: 153 tiles of 256 x 256, the last one 4 rows x 8 columns) and grid caps of 1 / 3 / 7 / 61 workgroups make
one persistent workgroup run 1 to 153 tiles: the K-step stream across tile boundaries, the tile switch and the last steps of a tile all
meet the reference."""
import ctypes as C

import pytest
import torch

from gemm_reference import check_within, gemm_bound, gemm_reference, pack_h2, unpack_h2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PREC = {"bf16": 1, "f16": 3, "h2": 4}
GUARD = 4096                                                      # bytes of guard band on either side of C
GUARD_BYTE = 0xA5
RESULTS = {}                                                      # kernel family -> [cases, largest err / bound]


def _lib():
    from clip_decontamination_amd import _lib as L
    return L.load()


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cdiv(a, b):
    return (a + b - 1) // b


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * scale


class Guarded:
    """C inside a byte buffer with GUARD bytes of GUARD_BYTE either side; C itself starts as all-ones bytes (NaN in every format)."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype
        n = torch.Size(shape).numel() * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((n + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + n] = 0xFF
        self.c = self.buf[GUARD:GUARD + n].view(dtype).view(shape)
        self.n = n

    def check_guards(self):
        head, tail = self.buf[:GUARD], self.buf[GUARD + self.n:]
        assert bool((head == GUARD_BYTE).all()), "a store landed in the guard band before C"
        assert bool((tail == GUARD_BYTE).all()), "a store landed in the guard band after C"


def configure(codes):
    lib = _lib()
    for c in codes:
        lib.sg_set_gemm_config(c)


def reset():
    configure((-1, 1000, 2000))


def expect_record(family, grid, ngroup=0):
    rec = _lib().sg_gemm_last_kernel().decode()
    assert rec == f"{family} grid={grid} ngroup={ngroup}", rec
    return rec


def record(family, ratio):
    n, worst = RESULTS.get(family, (0, 0.0))
    RESULTS[family] = (n + 1, max(worst, ratio))


def persist_grid(M, N, cap=0):
    g = min(cdiv(M, 256) * cdiv(N, 256), n_cu())
    return min(g, cap) if cap else g


def run_raw(prec, M, N, K, *, act=0, packed=True, bias=True, residual=False, batch=1, codes=(), family, grid, ngroup=0, seed=0,
            wscale=None):
    """One sg_gemm_raw case against the f64 reference; returns the largest err / bound."""
    lib = _lib()
    lead = (batch,) if batch > 1 else ()
    A32 = rnd(*lead, M, K, seed=seed)
    W32 = rnd(*lead, N, K, seed=seed + 1, scale=K ** -0.5 if wscale is None else wscale)
    b = rnd(N, seed=seed + 2, scale=0.1) if bias else None
    R = rnd(*lead, M, N, seed=seed + 3) if residual else None
    if prec == "h2":
        A, W = pack_h2(A32), pack_h2(W32)
        Aref, Wref = A32, W32
        cdt, out_fmt, ncols = torch.float16, "h2", 2 * N
    else:
        dt = torch.bfloat16 if prec == "bf16" else torch.float16
        A, W = A32.to(dt), W32.to(dt)
        Aref, Wref = A, W
        cdt, out_fmt, ncols = dt, prec, N
    if not packed:
        cdt, out_fmt, ncols = torch.float32, "f32", N
    out = Guarded((*lead, M, ncols), cdt)
    configure(codes)
    try:
        rc = lib.sg_gemm_raw(PREC[prec], ptr(A), ptr(W), ptr(b), ptr(R), ptr(out.c), M, N, K, batch, act, int(packed), stream())
        assert rc == 0, lib.sg_last_error()
        rec = expect_record(family, grid, ngroup)
    finally:
        reset()
    torch.cuda.synchronize()
    out.check_guards()
    got = unpack_h2(out.c) if (prec == "h2" and packed) else out.c
    pre, ref = gemm_reference(Aref, Wref, b, R, act)
    bound = gemm_bound(Aref, Wref, b, pre, ref, act=act, out_fmt=out_fmt, two_plane=prec == "h2", fast_act=prec != "h2")
    what = f"{prec} M={M} N={N} K={K} batch={batch} act={act} packed={packed} res={residual} codes={codes} [{rec}]"
    ratio = check_within(got, ref, bound, what)
    print(f"{what}: max err/bound {ratio:.3g}")
    record(family, ratio)
    return ratio


# ---- persistent bf16 / f16: gemm_bf16_persist_k64 (default) and gemm_bf16_persist (code 38) ----------------------------------------------
RM, RN = 4100, 2056                                               # 17 x 9 = 153 tiles; last tile 4 rows x 8 columns
CAPS = [0, 1, 3, 7, 61]
VARIANTS = {"k64": ((), "persist_k64"), "k32": ((38,), "persist_k32")}


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("variant", ["k64", "k32"])
@pytest.mark.parametrize("K", [256, 320, 448, 1024])
@pytest.mark.parametrize("cap", CAPS)
def test_persist_ragged_caps(prec, variant, K, cap):
    codes, fam = VARIANTS[variant]
    # the epilogue form rotates with the cap, so every K meets 2-byte and f32 outputs
    act, packed, residual = [(1, True, False), (0, True, False), (2, True, False), (0, False, True), (1, False, True)][CAPS.index(cap)]
    run_raw(prec, RM, RN, K, act=act, packed=packed, residual=residual, codes=codes + ((2000 + cap,) if cap else ()), family=fam,
            grid=persist_grid(RM, RN, cap), seed=K + cap)


FORMS = {"c2_act0": dict(act=0), "c2_act1": dict(act=1), "c2_act2": dict(act=2), "f32_res_act0": dict(act=0, packed=False, residual=True),
         "f32_res_act1": dict(act=1, packed=False, residual=True), "f32_nores": dict(act=2, packed=False),
         "c2_nobias": dict(act=1, bias=False), "f32_res_nobias": dict(act=0, packed=False, residual=True, bias=False)}


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("variant", ["k64", "k32"])
@pytest.mark.parametrize("form", list(FORMS))
def test_persist_epilogue_forms(prec, variant, form):
    codes, fam = VARIANTS[variant]
    run_raw(prec, RM, RN, 320, codes=codes + (2007,), family=fam, grid=7, seed=50, **FORMS[form])


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("variant", ["k64", "k32"])
def test_persist_uncapped_uneven(prec, variant):
    """M = 16440, N = 1096: 65 x 5 = 325 tiles, so most workgroups run two tiles and the rest one."""
    codes, fam = VARIANTS[variant]
    M, N = 16440, 1096
    run_raw(prec, M, N, 1024, act=1, codes=codes, family=fam, grid=persist_grid(M, N), seed=60)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("order", ["auto", "forced5", "raster"])
def test_persist_ngroup_order(prec, order):
    """M = 4252, N = 4088, K = 1024 (17 x 16 tiles): the automatic N-group order is 6 tiles wide (its last group 4), 1006 forces 5, 1001 is
    the raster order."""
    if n_cu() != 256:
        pytest.skip(f"the N-group shapes are sized for 256 CUs (this device has {n_cu()})")
    M, N = 4252, 4088
    codes, ng = {"auto": ((), 6), "forced5": ((1006,), 5), "raster": ((1001,), 0)}[order]
    run_raw(prec, M, N, 1024, act=2, codes=codes, family="persist_k64", grid=256, ngroup=ng, seed=70)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("packed", [True, False])
def test_persist_batched(prec, packed):
    """batch = 4 contiguous problems on blockIdx.y (15 tiles each)."""
    run_raw(prec, 1100, 520, 256, act=0 if packed else 1, packed=packed, residual=not packed, batch=4, family="persist_k64",
            grid=15, seed=80)


# ---- persistent two-plane f16 (gemm_h2_persist) ------------------------------------------------------------------------------------------
H2_FORMS = {"h2c_act0": dict(act=0), "h2c_act1": dict(act=1), "h2c_act2": dict(act=2), "f32_res": dict(act=0, packed=False, residual=True)}


@pytest.mark.parametrize("form", list(H2_FORMS))
@pytest.mark.parametrize("K", [128, 224, 1024])
def test_h2_persist_forms(form, K):
    run_raw("h2", RM, RN, K, codes=(2007,) if K == 224 else (), family="h2_persist", grid=7 if K == 224 else persist_grid(RM, RN),
            seed=90 + K, **H2_FORMS[form])


@pytest.mark.parametrize("cap", [1, 3, 61])
def test_h2_persist_caps(cap):
    run_raw("h2", RM, RN, 256, act=2, codes=(2000 + cap,), family="h2_persist", grid=cap, seed=95 + cap)


def test_h2_persist_uncapped_uneven():
    run_raw("h2", 16440, 1096, 512, act=1, family="h2_persist", grid=persist_grid(16440, 1096), seed=99)


@pytest.mark.parametrize("packed", [True, False])
def test_h2_small_magnitude(packed):
    """W ~ 1e-3 N(0, 1): the planes of W sit in the f16 subnormal range, where the 2^-25 floor of the representation error (not 22
    significant bits) is what holds -- bounded by the delta term."""
    run_raw("h2", RM, RN, 1024, act=0, packed=packed, residual=not packed, wscale=1e-3, family="h2_persist",
            grid=persist_grid(RM, RN), seed=100)


def planes(*shape, seed):
    """Chosen planes (f16): hi in {-3..3}, lo in {-3..3} 2^-8 -- not a rounding remainder of hi: the kernel only multiplies planes."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    hi = torch.randint(-3, 4, shape, generator=g, device=DEV).to(torch.float16)
    lo = (torch.randint(-3, 4, shape, generator=g, device=DEV) * 2.0 ** -8).to(torch.float16)
    return hi, lo


def store_planes(hi, lo):
    lead, k = hi.shape[:-1], hi.shape[-1]
    return torch.stack([hi.view(*lead, k // 8, 8), lo.view(*lead, k // 8, 8)], dim=-2).reshape(*lead, 2 * k)


@pytest.mark.parametrize("kernel", ["h2_persist", "h2_persist_cap3", "h2_pingpong", "h2_ring128"])
def test_h2_planes_exact(kernel):
    """The two-plane GEMM is hi.hi + hi.lo + lo.hi, and on planes whose products and partial sums are all multiples of 2^-8 below 2^14 every
    f32 operation is exact: the output must EQUAL that sum, in any summation order.  The f64 bound above is a worst case (2u 3K S) that a
    lost lo plane (an error of ~2^-12 of the result) would pass; this cannot.  A's lo plane is zero on odd K, W's on even K, so the
    omitted lo.lo term is exactly zero."""
    lib = _lib()
    M, N, K, codes, fam, grid = {"h2_persist": (RM, RN, 1024, (), "h2_persist", 153), "h2_persist_cap3": (RM, RN, 224, (2003,), "h2_persist", 3),
                                 "h2_pingpong": (RM, RN, 128, (), "h2_pingpong", 153),
                                 "h2_ring128": (SM, SN, 256, (), "h2_ring128", cdiv(SM, 128) * cdiv(SN, 128))}[kernel]
    ah, al = planes(M, K, seed=300)
    wh, wl = planes(N, K, seed=301)
    al[:, 1::2] = 0
    wl[:, 0::2] = 0
    g = torch.Generator(device=DEV).manual_seed(302)
    b = (torch.randint(-64, 65, (N,), generator=g, device=DEV) * 2.0 ** -8).float()
    R = (torch.randint(-64, 65, (M, N), generator=g, device=DEV) * 2.0 ** -8).float() if kernel != "h2_pingpong" else None
    A, W = store_planes(ah, al), store_planes(wh, wl)                 # named: a temporary would go back to the allocator before the launch
    out = Guarded((M, N), torch.float32)
    configure(codes)
    try:
        rc = lib.sg_gemm_raw(PREC["h2"], ptr(A), ptr(W), ptr(b), ptr(R), ptr(out.c), M, N, K, 1, 0, 0, stream())
        assert rc == 0, lib.sg_last_error()
        expect_record(fam, grid)
    finally:
        reset()
    torch.cuda.synchronize()
    out.check_guards()
    ahd, ald, whd, wld = ah.double(), al.double(), wh.double(), wl.double()
    ref = ahd @ whd.T + ahd @ wld.T + ald @ whd.T + b.double()
    if R is not None:
        ref = ref + R.double()
    assert ref.abs().max() < 2 ** 14
    bad = (out.c.double() != ref)
    assert not bool(bad.any()), f"{kernel}: {int(bad.sum())} elements differ from the exact plane products"
    record(fam + " (exact planes)", 0.0)


# ---- persistent fp8 (gemm_fp8_persist) ---------------------------------------------------------------------------------------------
def quantize_fp8(x):
    lib = _lib()
    rows, D = x.shape
    q = torch.empty(rows, D, dtype=torch.uint8, device=DEV)
    s = torch.empty(rows, dtype=torch.float32, device=DEV)
    assert lib.sg_quantize_rows_fp8(ptr(x), rows, D, ptr(q), ptr(s), stream()) == 0, lib.sg_last_error()
    return q, s


def run_fp8(M, N, K, *, act, packed, residual, codes=(), family, grid, seed):
    lib = _lib()
    A8, sa = quantize_fp8(rnd(M, K, seed=seed))
    W8, sw = quantize_fp8(rnd(N, K, seed=seed + 1, scale=K ** -0.5))
    b = rnd(N, seed=seed + 2, scale=0.1)
    R = rnd(M, N, seed=seed + 3) if residual else None
    out = Guarded((M, N), torch.bfloat16 if packed else torch.float32)
    configure(codes)
    try:
        rc = lib.sg_gemm_fp8_raw(ptr(A8), ptr(sa), ptr(W8), ptr(sw), ptr(b), ptr(R), ptr(out.c), M, N, K, act, int(packed), stream())
        assert rc == 0, lib.sg_last_error()
        rec = expect_record(family, grid)
    finally:
        reset()
    torch.cuda.synchronize()
    out.check_guards()
    Aref = A8.view(torch.float8_e4m3fn).double() * sa.double()[:, None]        # the de-quantised bytes the kernel multiplies
    Wref = W8.view(torch.float8_e4m3fn).double() * sw.double()[:, None]
    pre, ref = gemm_reference(Aref, Wref, b, R, act)
    bound = gemm_bound(Aref, Wref, b, pre, ref, act=act, out_fmt="bf16" if packed else "f32")
    what = f"fp8 M={M} N={N} K={K} act={act} packed={packed} res={residual} codes={codes} [{rec}]"
    ratio = check_within(out.c, ref, bound, what)
    print(f"{what}: max err/bound {ratio:.3g}")
    record(family, ratio)


FP8_FORMS = {"c2_act1": dict(act=1, packed=True, residual=False), "c2_act2": dict(act=2, packed=True, residual=False),
             "f32_res": dict(act=0, packed=False, residual=True)}


@pytest.mark.parametrize("form", list(FP8_FORMS))
@pytest.mark.parametrize("K,code", [(2048, None), (4096, None), (512, 32), (1024, 32)])
@pytest.mark.parametrize("cap", [0, 7])
def test_fp8_persist(form, K, code, cap):
    codes = ((code,) if code else ()) + ((2000 + cap,) if cap else ())
    run_fp8(RM, RN, K, codes=codes, family="fp8_persist", grid=persist_grid(RM, RN, cap), seed=110 + K + cap, **FP8_FORMS[form])


def test_fp8_persist_single_workgroup():
    run_fp8(RM, RN, 2048, act=0, packed=True, residual=False, codes=(2001,), family="fp8_persist", grid=1, seed=120)


@pytest.mark.parametrize("M,family,grid", [(4100, "fp8_ring256x256", 17 * 9), (1000, "fp8_ring128", 8 * 17)])
@pytest.mark.parametrize("form", ["c2_act0", "f32_res"])
def test_fp8_ring(M, family, grid, form):
    """Code 31 keeps the ring kernels (M >= 1024: 256 x 256 tiles, the 2-byte no-activation form specialised); M < 1024 always runs them."""
    kw = dict(act=0, packed=True, residual=False) if form == "c2_act0" else dict(act=0, packed=False, residual=True)
    run_fp8(M, RN, 512, codes=(31,) if M >= 1024 else (), family=family, grid=grid, seed=130 + M, **kw)


# ---- large offsets: A beyond 2^31 bytes, C beyond 2^32 bytes --------------------------------------------------------------------------
def sampled_rows(M, row_bytes_list, seed):
    """The first and last rows, the rows around every 2^31-byte boundary of each operand, and 2048 random rows."""
    rows = [torch.arange(0, 256), torch.arange(M - 256, M)]
    for rb in row_bytes_list:
        for j in range(1, M * rb // 2 ** 31 + 1):
            r = (j * 2 ** 31) // rb
            rows.append(torch.arange(max(r - 128, 0), min(r + 128, M)))
    g = torch.Generator().manual_seed(seed)
    rows.append(torch.randint(0, M, (2048,), generator=g))
    return torch.unique(torch.cat(rows)).to(DEV)


def _large_case(prec):
    lib = _lib()
    M, N, K = 1_100_000, 1024, 1024
    A32 = torch.randn(M, K, device=DEV, dtype=torch.float32, generator=torch.Generator(device=DEV).manual_seed(140))   # built on the device
    W32 = rnd(N, K, seed=141, scale=K ** -0.5)
    b = rnd(N, seed=142, scale=0.1)
    if prec == "bf16":
        A, W = A32.bfloat16(), W32.bfloat16()
        del A32
        out = Guarded((M, N), torch.float32)
        packed, out_fmt, a_row, c_row, fam = False, "f32", 2 * K, 4 * N, "persist_k64"
    else:
        A, W = pack_h2(A32), pack_h2(W32)
        out = Guarded((M, 2 * N), torch.float16)
        packed, out_fmt, a_row, c_row, fam = True, "h2", 4 * K, 4 * N, "h2_persist"
    assert A.numel() * A.element_size() > 2 ** 31 and out.n > 2 ** 32
    try:
        rc = lib.sg_gemm_raw(PREC[prec], ptr(A), ptr(W), ptr(b), None, ptr(out.c), M, N, K, 1, 0, int(packed), stream())
        assert rc == 0, lib.sg_last_error()
        expect_record(fam, persist_grid(M, N))
    finally:
        reset()
    torch.cuda.synchronize()
    out.check_guards()
    rows = sampled_rows(M, [a_row, c_row], 143)
    Aref, Wref = (A[rows], W) if prec == "bf16" else (A32[rows], W32)
    got = out.c[rows]
    got = unpack_h2(got) if packed else got
    pre, ref = gemm_reference(Aref, Wref, b, None, 0)
    bound = gemm_bound(Aref, Wref, b, pre, ref, act=0, out_fmt=out_fmt, two_plane=prec == "h2", fast_act=prec != "h2")
    ratio = check_within(got, ref, bound, f"large {prec}")
    print(f"large offsets {prec}: {rows.numel()} rows checked, max err/bound {ratio:.3g}")
    record(fam, ratio)


@pytest.mark.parametrize("prec", ["bf16", "h2"])
def test_large_offsets(prec):
    """M = 1.1 M rows, K = N = 1024: A spans 2.25 GB (bf16) / 4.5 GB (two-plane), C 4.5 GB (f32 / two-plane).  Sampled row blocks in f64;
    the buffers (up to ~20 GB while the two-plane operand is packed) are released afterwards."""
    torch.cuda.empty_cache()
    try:
        _large_case(prec)
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- the non-persistent kernels: the 128 x 128 ring (few-tile launches) and the 256 x 256 ping-pong (large launches the persistent kernel
# does not take: K / 32 < 4 or the scalar epilogue) ------------------------------------------------------------------------------------
SM, SN, SK = 1100, 520, 256                                      # 5 x 3 tiles of 256 x 256: a few-tile launch


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("form", ["c2_act2", "f32_res"])
def test_ring128_few_tiles(prec, form):
    kw = dict(act=2) if form == "c2_act2" else dict(act=0, packed=False, residual=True)
    run_raw(prec, SM, SN, SK, family="ring128", grid=cdiv(SM, 128) * cdiv(SN, 128), seed=170, **kw)


PP_FORMS = {"c2_act2": dict(act=2), "c2_act1": dict(act=1), "f32_res": dict(act=0, packed=False, residual=True)}


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("form", list(PP_FORMS))
def test_pingpong_short_k(prec, form):
    """K = 64 at >= 128 tiles: K / 32 < 4 sends the persistent dispatch to the ping-pong kernel (its vector epilogue, 2-byte and f32 +
    residual outputs)."""
    run_raw(prec, RM, RN, 64, family="pingpong", grid=153, seed=190, **PP_FORMS[form])


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("large", [False, True])
def test_n_not_multiple_of_8(prec, large):
    """The scalar (non-vector) epilogues: N % 8 != 0 on the few-tile ring kernel and, at >= 128 tiles, on the ping-pong kernel."""
    M, N = (RM, 2055) if large else (SM, 517)
    fam, grid = ("pingpong", 153) if large else ("ring128", cdiv(M, 128) * cdiv(N, 128))
    run_raw(prec, M, N, 256, act=1, family=fam, grid=grid, seed=210)
    run_raw(prec, M, N, 256, act=0, packed=False, residual=True, family=fam, grid=grid, seed=211)


def test_h2_pingpong_and_ring128():
    """Two-plane forms outside the persistent kernel: an f32 C without residual (no compile-time epilogue) at >= 128 tiles runs the
    ping-pong kernel; a few-tile launch runs the 128 x 128 ring kernel."""
    run_raw("h2", RM, RN, 128, act=1, packed=False, family="h2_pingpong", grid=153, seed=220)
    run_raw("h2", SM, SN, 128, act=2, family="h2_ring128", grid=cdiv(SM, 128) * cdiv(SN, 128), seed=221)
    run_raw("h2", SM, SN, 128, act=0, packed=False, residual=True, family="h2_ring128", grid=cdiv(SM, 128) * cdiv(SN, 128), seed=222)


def test_f32_gemm_control():
    """SG_PREC_F32 through sg_op_linear: the f32 GEMM, held to the same bound (its products round once each, inside the 2u K S term).
    It does not go through gemm_bf16(), so it leaves the kernel record alone."""
    from clip_decontamination_amd import ops
    M, N, K = 1100, 520, 300
    A, W = rnd(M, K, seed=230), rnd(N, K, seed=231, scale=K ** -0.5)
    b, R = rnd(N, seed=232, scale=0.1), rnd(M, N, seed=233)
    run_raw("bf16", SM, SN, SK, family="ring128", grid=cdiv(SM, 128) * cdiv(SN, 128), seed=234)
    before = _lib().sg_gemm_last_kernel()
    got = ops.linear(A, W, b, R, 0, "f32")
    torch.cuda.synchronize()
    assert _lib().sg_gemm_last_kernel() == before
    pre, ref = gemm_reference(A, W, b, R, 0)
    ratio = check_within(got, ref, gemm_bound(A, W, b, pre, ref, act=0, out_fmt="f32"), "f32 GEMM")
    print(f"f32 GEMM: max err/bound {ratio:.3g}")
    record("f32", ratio)


def test_record_says_none_after_a_refused_call():
    """A call refused before any launch leaves no stale record behind."""
    lib = _lib()
    run_raw("bf16", SM, SN, SK, family="ring128", grid=cdiv(SM, 128) * cdiv(SN, 128), seed=240)
    A = torch.zeros(SM, 96, dtype=torch.bfloat16, device=DEV)
    W = torch.zeros(SN, 96, dtype=torch.bfloat16, device=DEV)
    out = torch.empty(SM, SN, dtype=torch.bfloat16, device=DEV)
    assert lib.sg_gemm_raw(1, ptr(A), ptr(W), None, None, ptr(out), SM, SN, 96, 1, 0, 1, stream()) != 0   # K % 64 != 0
    assert lib.sg_gemm_last_kernel() == b"none"
    assert lib.sg_gemm_raw(0, ptr(A), ptr(W), None, None, ptr(out), SM, SN, 96, 1, 0, 1, stream()) != 0   # f32: not a raw storage
    assert b"bad precision" in lib.sg_last_error()


def test_summary():
    """Prints the number of cases and the largest err / bound per kernel family (run last in this module)."""
    for fam in sorted(RESULTS):
        n, worst = RESULTS[fam]
        print(f"SUMMARY {fam}: {n} cases, largest err/bound {worst:.3g}")
