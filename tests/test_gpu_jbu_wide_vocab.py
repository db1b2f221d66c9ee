"""The JBU upsampler's fused logits tail for more than 32 queries (sg_jbu_logits_wide, jbu_pixel_logits_wide_kernel) and the bilinear kind's
one-call form.  The tail is held per element to the f64 scheme of test_jbu_logits_tail_vs_f64 (tests/test_gpu_jbu_reference.py) on the
operands it actually consumed -- the captures at query stride Qp = 16 ceil(Q / 16) -- with that test's formulas and its matrix-pipe term
2^-16 (|x| . |G|); further: column independence, the untouched range up to 32 queries, the fused against the unfused host path, the
bilinear chunks, repeats and the refusals.  run_wide() is tests/test_gpu_jbu_reference.py's run() with the wide entry and capture sizes.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jbu_reference import U, F32_TENTH, decode, rounded, check_within, half_ulp, rowdot_reference  # noqa: E402
from test_gpu_jbu_reference import DEV, GUARD, lib_, ptr, stream, make_weights, make_inputs, upsampler, same_bytes  # noqa: E402
import upsampler_alt_reference as UR  # noqa: E402

pytestmark = pytest.mark.gpu
WIDE = "jbu_pixel_logits_wide_kernel"
TAIL_SLOTS = ("FIN_A", "GEFF", "G0", "CLSL", "ROWDOT")
_UPS = {}


def qp_of(Q):
    return 32 if Q <= 32 else (Q + 15) // 16 * 16


def shared_upsampler(Cf):
    """One jbu_stack upsampler (and its weights) per feature width for the whole module."""
    if Cf not in _UPS:
        w = make_weights("jbu_stack", Cf, "smooth")
        _UPS[Cf] = (upsampler("jbu_stack", Cf, "bf16", w), w)
    return _UPS[Cf]


def text_rows(Q, Cf, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(Q, Cf, generator=g), dim=-1).to(DEV).contiguous()


def run_wide(up, src, guid, gh, gw, text, Q, cls, lam, *, entry="wide", capture=True, precision=None, short=0, expect_ok=True):
    """sg_jbu_logits_wide (entry='wide') or sg_jbu_logits on these operands between NaN guard bands, the tail slots captured at query
    stride qp_of(Q).  Returns (logits [B * Q * P] f32, captured {name: uint8 tensor}, record dict) or, with expect_ok=False,
    (return code, error string, whether the output is still all NaN)."""
    _lib, lib = lib_()
    B, Cf = src.shape[0], up.feat_dim
    need = lib.sg_jbu_workspace_bytes_wide(up._ctx, B, gh, gw, Q) if entry == "wide" else lib.sg_jbu_workspace_bytes(up._ctx, B, gh, gw)
    ws = torch.full(((need + 2 * GUARD) // 4 + 1,), float("nan"), device=DEV)
    P = 256 * gh * gw if up.model_name != "bilinear" else guid.shape[-2] * guid.shape[-1]
    n_out = B * Q * P
    out = torch.full((n_out + 2 * GUARD // 4,), float("nan"), device=DEV)
    cap = _lib.JbuCapture()
    bufs = {}
    px, Qp = B * P, qp_of(Q)
    if capture:
        for i, name in enumerate(_lib.JBU_CAP_TAIL):
            if name not in TAIL_SLOTS:
                continue
            nb = {"GEFF": Cf * Qp * 4, "G0": Qp * 4, "CLSL": B * Qp * 4, "ROWDOT": px * (Cf // 64 + 1) * 4, "FIN_A": px * Cf * 2}[name]
            t = torch.empty(nb, dtype=torch.uint8, device=DEV)
            bufs[name] = t
            cap.tail[i].dst, cap.tail[i].cap = t.data_ptr(), nb
        if up.model_name != "bilinear":                         # the last stage's bf16 output: what the tail's A operand must be, bit for bit
            i, nb = _lib.JBU_CAP_STAGE.index("OUT16"), px * Cf * 2
            t = torch.empty(nb, dtype=torch.uint8, device=DEV)
            bufs["OUT16"] = t
            cap.stage[3][i].dst, cap.stage[3][i].cap = t.data_ptr(), nb
    torch.cuda.synchronize()
    _lib.check(lib.sg_jbu_set_capture(up._ctx, C.addressof(cap) if capture else None), "sg_jbu_set_capture")
    try:
        fn = lib.sg_jbu_logits_wide if entry == "wide" else lib.sg_jbu_logits
        rc = fn(up._ctx, ptr(src), ptr(guid), B, gh, gw, guid.shape[-2], guid.shape[-1], up.precision if precision is None else precision,
                ptr(text), Q, ptr(cls) if cls is not None else None, lam, ptr(out, GUARD), ptr(ws, GUARD), need - short, stream())
        err = lib.sg_last_error()
        torch.cuda.synchronize()
    finally:
        lib.sg_jbu_set_capture(up._ctx, None)
    if not expect_ok:
        return rc, err, bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())
    _lib.check(rc, f"sg_jbu_logits ({entry})")
    rec = dict(tok.split("=", 1) for tok in lib.sg_jbu_last_kernels().decode().split())
    wb = ws.view(torch.uint8)
    nanb = torch.full((1,), float("nan"), device=DEV).view(torch.uint8)
    for what, band in (("workspace head", wb[:GUARD]), ("workspace tail", wb[GUARD + need:GUARD + need + GUARD - 4]),
                       ("output head", out.view(torch.uint8)[:GUARD]), ("output tail", out.view(torch.uint8)[GUARD + 4 * n_out:])):
        assert bool((band.view(-1, 4) == nanb).all()), f"{what} guard band overwritten"
    got = out[GUARD // 4:GUARD // 4 + n_out]
    assert bool(torch.isfinite(got).all()), "non-finite output"
    capd = {}
    for name, t in bufs.items():
        nb = cap.stage[3][_lib.JBU_CAP_STAGE.index("OUT16")].bytes if name == "OUT16" else cap.tail[_lib.JBU_CAP_TAIL.index(name)].bytes
        if nb:
            capd[name] = t[:nb]
    return got, capd, rec


def check_tail(w, Cf, B, P, text, Q, cls, lam, out, capd, what):
    """Geff, g0, the CLS logits, the row-dot slots and the logits against f64 on the captured operands: the formulas of
    test_jbu_logits_tail_vs_f64 at query stride Qp, with the matrix-pipe representation term 2^-16 (|x| . |G|).  Returns the largest
    err / bound over the pieces."""
    Qp, with_cls = qp_of(Q), cls is not None and lam != 0.0
    assert capd["GEFF"].numel() == Cf * Qp * 4 and capd["G0"].numel() == Qp * 4, "capture sizes at query stride Qp"
    assert capd["FIN_A"].numel() == B * P * Cf * 2
    same_bytes(capd["FIN_A"], capd["OUT16"], f"{what}: tail A = stage-3 bf16 output")
    x = decode(capd["FIN_A"], "bf16", Cf)                                   # [px, C]
    T = text.double()
    Wf = torch.from_numpy(w["fixup_proj.1.weight"]).to(DEV).view(Cf, Cf).double()
    bf01 = (torch.from_numpy(w["fixup_proj.1.bias"]).to(DEV).float() * torch.tensor(F32_TENTH, dtype=torch.float32)).double()
    worst = 0.0
    G = decode(capd["GEFF"], "f32", Qp)[:, :Q]
    S = Wf.abs().T @ T.abs().T
    ref = T.T + F32_TENTH * (Wf.T @ T.T)
    bnd = F32_TENTH * 2 * U * (Cf + 2) * S + 2 * U * (T.T.abs() + F32_TENTH * S)
    bnd = bnd + half_ulp(ref.abs() + bnd, "f32")
    worst = max(worst, check_within(G, ref, bnd, f"{what}: Geff"))
    g0 = decode(capd["G0"], "f32", Qp)[0, :Q]
    ref = T @ bf01
    bnd = 2 * U * (Cf + 2) * (T.abs() @ bf01.abs())
    bnd = bnd + half_ulp(ref.abs() + bnd, "f32")
    worst = max(worst, check_within(g0, ref, bnd, f"{what}: g0"))
    if with_cls:
        assert capd["CLSL"].numel() == B * Qp * 4
        clsl = decode(capd["CLSL"], "f32", Qp)[:, :Q]
        c = cls.double()
        nrm = c.norm(dim=-1, keepdim=True)
        ref = (c @ T.T) / nrm
        bnd = 2 * U * (Cf + 1) * (c.abs() @ T.abs().T) / nrm + ref.abs() * (U * Cf + 2 * 2.0 ** -22 + U)
        bnd = bnd + half_ulp(ref.abs() + bnd, "f32")
        worst = max(worst, check_within(clsl, ref, bnd, f"{what}: cls logits"))
    else:
        assert "CLSL" not in capd
    slots_n = Cf // 64
    rd = decode(capd["ROWDOT"], "f32", slots_n)
    ref, bnd = rowdot_reference(x, rounded(Wf.float(), "bf16"), bf01)
    worst = max(worst, check_within(rd, ref, bnd, f"{what}: row-dot slots"))
    num = x @ G + g0[None]
    SxG = x.abs() @ G.abs()
    n2 = (x * x).sum(-1) + rd.sum(-1)
    inv = n2.rsqrt()
    clv = (lam * decode(capd["CLSL"], "f32", Qp)[:, :Q]) if with_cls else torch.zeros(B, Q, dtype=torch.float64, device=DEV)
    bidx = torch.arange(B * P, device=DEV) // P
    ref = num * inv[:, None] + clv[bidx]
    rep = 2.0 ** -16 * SxG                                                    # Geff as two bf16 planes on the matrix pipe
    dN = rep + 2 * U * (2 * Cf + 1) * SxG + U * (SxG + g0.abs()[None])
    rho = (2 * U * Cf * (x * x).sum(-1) + 2 * U * (slots_n + 1) * ((x * x).sum(-1) + rd.abs().sum(-1))) / n2 / 2 + 2 * 2.0 ** -22
    bnd = dN * inv[:, None] * (1 + rho[:, None]) + num.abs() * inv[:, None] * rho[:, None] + 2 * U * num.abs() * inv[:, None] + 2 * U * clv.abs()[bidx]
    bnd = bnd + half_ulp(ref.abs() + bnd, "f32")
    got = out.view(B, Q, P).permute(0, 2, 1).reshape(B * P, Q)
    worst = max(worst, check_within(got, ref, bnd, f"{what}: logits"))
    return worst


def check_record(rec, with_cls):
    tail = rec["tail"].split(",")
    assert WIDE in tail and "jbu_geff_kernel" in tail and (("jbu_cls_logits_kernel" in tail) == with_cls), rec
    assert rec["final.a"] == "bf16", rec


def tail_case(B, gh, gw, Cf, Q, with_cls, seed=None):
    up, w = shared_upsampler(Cf)
    seed = Q + Cf + gh if seed is None else seed
    src, guid = make_inputs(B, Cf, gh, gw, "smooth", seed=seed)
    src, guid = src.to(DEV), guid.to(DEV)
    text = text_rows(Q, Cf, seed)
    cls = torch.randn(B, Cf, generator=torch.Generator().manual_seed(seed + 1)).to(DEV).contiguous() if with_cls else None
    lam = 0.3 if with_cls else 0.0
    out, capd, rec = run_wide(up, src, guid, gh, gw, text, Q, cls, lam)
    check_record(rec, with_cls)
    worst = check_tail(w, Cf, B, 256 * gh * gw, text, Q, cls, lam, out, capd, f"C={Cf} Q={Q} {B}x{gh}x{gw} cls={with_cls}")
    print(f"wide tail C={Cf} Q={Q} B={B} {gh}x{gw} cls={with_cls}: worst err/bound {worst:.3g}")


# ---- 1. per-element f64 bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cls", [False, True])
@pytest.mark.parametrize("Q", [33, 48, 49, 130])
@pytest.mark.parametrize("Cf", [512, 640])
@pytest.mark.parametrize("shape", [(2, 2, 3), (1, 3, 3)], ids=["2x2x3", "1x3x3"])
def test_wide_tail_vs_f64(shape, Cf, Q, with_cls):
    """33: one live column in the last group; 48: whole groups; 49 at C = 640: two passes of two groups; 130: the head tests' vocabulary.
    (1, 3, 3) gives 2304 pixels: the last workgroup's waves run out of pixels mid-round."""
    tail_case(*shape, Cf, Q, with_cls)


@pytest.mark.parametrize("Cf,Q,shape", [(512, 70, (2, 2, 3)), (640, 70, (1, 3, 3)), (1024, 40, (1, 2, 2))],
                         ids=["C512-Q70", "C640-Q70", "C1024-Q40"])
def test_wide_tail_partial_last_pass_vs_f64(Cf, Q, shape):
    """The group counts the cases above do not reach: five groups as 3 + 2 (a last pass with a dead resident group) and, at C = 1024
    where only two groups fit, three groups as 2 + 1 on the two-group instantiation."""
    tail_case(*shape, Cf, Q, True)


# ---- 2. column independence ----------------------------------------------------------------------------------------------------------
def test_wide_tail_columns_are_independent():
    Cf, Q, B, gh, gw = 512, 40, 2, 2, 3
    up, w = shared_upsampler(Cf)
    src, guid = make_inputs(B, Cf, gh, gw, "smooth", seed=40)
    src, guid = src.to(DEV), guid.to(DEV)
    text = text_rows(Q, Cf, 40)
    cls = torch.randn(B, Cf, generator=torch.Generator().manual_seed(41)).to(DEV).contiguous()
    P = 256 * gh * gw
    a, _, _ = run_wide(up, src, guid, gh, gw, text, Q, cls, 0.3, capture=False)
    b, _, _ = run_wide(up, src, guid, gh, gw, text.flip(0).contiguous(), Q, cls, 0.3, capture=False)
    same_bytes(a.view(B, Q, P).contiguous().view(torch.uint8).reshape(-1), b.view(B, Q, P).flip(1).contiguous().view(torch.uint8).reshape(-1),
               "query q of the ordered run = query 39 - q of the reversed run")
    # row 17 among 39 other rows: still within the f64 bound of the operands that run consumed
    other = text_rows(Q, Cf, 99)
    other[17] = text[17]
    out, capd, rec = run_wide(up, src, guid, gh, gw, other, Q, cls, 0.3)
    check_record(rec, True)
    check_tail(w, Cf, B, P, other, Q, cls, 0.3, out, capd, "row 17 among other rows")


# ---- 3. existing range untouched ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [16, 32])
def test_wide_entry_is_the_narrow_entry_up_to_32_queries(Q):
    Cf, B, gh, gw = 512, 2, 2, 3
    up, _ = shared_upsampler(Cf)
    _, lib = lib_()
    src, guid = make_inputs(B, Cf, gh, gw, "smooth", seed=Q)
    src, guid = src.to(DEV), guid.to(DEV)
    text = text_rows(Q, Cf, Q)
    cls = torch.randn(B, Cf, generator=torch.Generator().manual_seed(Q)).to(DEV).contiguous()
    assert lib.sg_jbu_workspace_bytes_wide(up._ctx, B, gh, gw, Q) == lib.sg_jbu_workspace_bytes(up._ctx, B, gh, gw)
    a, ca, ra = run_wide(up, src, guid, gh, gw, text, Q, cls, 0.3, entry="wide")
    b, cb, rb = run_wide(up, src, guid, gh, gw, text, Q, cls, 0.3, entry="narrow")
    same_bytes(a.view(torch.uint8), b.view(torch.uint8), f"Q={Q}: wide entry = narrow entry")
    assert ra == rb and WIDE not in ra["tail"], (ra, rb)
    assert ca["GEFF"].numel() == Cf * 32 * 4 and ca["G0"].numel() == 128 and ca["CLSL"].numel() == B * 128
    for name in ca:
        if name in ("GEFF", "G0", "CLSL"):                      # their live columns (the padding columns are scratch no kernel writes)
            la, lb = (c.view(torch.float32).view(-1, 32)[:, :Q].contiguous().view(torch.uint8).reshape(-1) for c in (ca[name], cb[name]))
            same_bytes(la, lb, f"Q={Q}: capture {name}[:, :Q]")
        else:
            same_bytes(ca[name], cb[name], f"Q={Q}: capture {name}")


# ---- 4. fused against unfused through the host class -------------------------------------------------------------------------------------
def _host_logits(up, tok, cls, scene, windows, tile_hw, grid, text, lam, padded_hw):
    out = up.logits(tok, cls, scene, windows, tile_hw, (0, 0), grid, text, 0.0, lam, padded_hw=padded_hw)
    torch.cuda.synchronize()
    return out, up.lib.sg_jbu_last_kernels().decode()


def test_host_fused_wide_tail_against_unfused():
    from clip_decontamination_amd import weights as Wt
    Cf, Q, g = 512, 40, 2
    up, _ = shared_upsampler(Cf)
    scene = torch.from_numpy(Wt.make_tiles_u8(1, 48, seed=5, smooth=True)[0][:32]).contiguous().to(DEV)       # [32, 48, 3] u8
    windows = torch.tensor([[0, 32, 0, 32], [0, 32, 16, 48]], dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(44)
    tok = torch.randn(2, g * g, Cf, generator=gen).to(DEV)
    cls = torch.randn(2, Cf, generator=gen).to(DEV)
    text = text_rows(Q, Cf, 45)
    assert up.fused_tail
    wide_default = up.wide_tail
    try:
        up.wide_tail = True
        fused, rec_f = _host_logits(up, tok, cls, scene, windows, (32, 32), (g, g), text, -0.3, (32, 32))
        up.fused_tail = False
        unfused, rec_u = _host_logits(up, tok, cls, scene, windows, (32, 32), (g, g), text, -0.3, (32, 32))
    finally:
        up.fused_tail, up.wide_tail = True, wide_default
    assert fused.shape == unfused.shape == (2, Q, 32, 32)
    d = (fused - unfused).abs().max().item()
    print(f"host logits Q={Q}: |fused - unfused| = {d:.3e}")
    assert WIDE in rec_f and "tail=" in rec_f, rec_f
    assert WIDE not in rec_u and "tail=" not in rec_u, rec_u
    assert d < 2e-3, d                                           # the tolerance of test_jbu_fused_logits_tail_equals_unfused_and_oracle


# ---- 5. bilinear: one call ------------------------------------------------------------------------------------------------------------------
def test_bilinear_one_call_equals_the_chunks_and_f64():
    from clip_decontamination_amd.upsampler import get_upsampler
    B, gh, gw, Pp, Cf, Q, lam = 2, 3, 4, 14, 64, 70, -0.3
    GH, GW = Pp * gh, Pp * gw
    rng = np.random.default_rng(70)
    tok = rng.standard_normal((B, gh * gw, Cf)).astype(np.float32)
    text = rng.standard_normal((Q, Cf)).astype(np.float32)
    text /= np.linalg.norm(text, axis=-1, keepdims=True)
    cls = rng.standard_normal((B, Cf)).astype(np.float32)
    up = get_upsampler("bilinear", Cf, str(DEV), "f32")
    tk, tx, cl = torch.from_numpy(tok).to(DEV), torch.from_numpy(text).to(DEV), torch.from_numpy(cls).to(DEV)
    guid = torch.zeros(B, 3, GH, GW, device=DEV)
    one, _, rec = run_wide(up, tk, guid, gh, gw, tx, Q, cl, lam, capture=False)
    assert rec["tail"] == "bilinear_prologue_kernel,jbu_cls_logits_kernel,bilinear_pixel_logits_kernel", rec
    parts = []
    for q0 in (0, 32, 64):
        qn = min(32, Q - q0)
        part, _, _ = run_wide(up, tk, guid, gh, gw, tx[q0:q0 + qn].contiguous(), qn, cl, lam, entry="narrow", capture=False)
        parts.append(part.view(B, qn, GH * GW))
    same_bytes(one.view(torch.uint8), torch.cat(parts, 1).contiguous().view(torch.uint8).reshape(-1), "one wide call = the 32 / 32 / 6 chunks")
    # through the host class, against f64 within the reference file's bound
    scene = torch.zeros(GH, GW, 3, dtype=torch.uint8, device=DEV)
    windows = torch.tensor([[0, GH, 0, GW]] * B, dtype=torch.int32, device=DEV)
    got = up.logits(tk, cl, scene, windows, (GH, GW), (0, 0), (gh, gw), tx, 0.0, lam, padded_hw=(GH, GW))
    torch.cuda.synchronize()
    same_bytes(got.contiguous().view(torch.uint8).reshape(-1), one.view(torch.uint8), "HipJBU.logits = the wide call")
    ref, bnd = UR.logits_bound(tok.astype(np.float64), text.astype(np.float64), gh, gw, GH, GW, cls.astype(np.float64), lam)
    err = np.abs(got.reshape(B, Q, GH * GW).cpu().numpy().astype(np.float64) - ref)
    assert (err <= bnd).all(), f"max err/bound {(err / bnd).max():.3g}"


# ---- 6. reproducibility -----------------------------------------------------------------------------------------------------------------------
def test_wide_tail_repeats_bit_for_bit():
    Cf, Q, B, gh, gw = 640, 49, 2, 2, 3
    up, _ = shared_upsampler(Cf)
    src, guid = make_inputs(B, Cf, gh, gw, "smooth", seed=6)
    src, guid = src.to(DEV), guid.to(DEV)
    text = text_rows(Q, Cf, 6)
    cls = torch.randn(B, Cf, generator=torch.Generator().manual_seed(7)).to(DEV).contiguous()
    first = None
    for k in range(5):
        out, _, rec = run_wide(up, src, guid, gh, gw, text, Q, cls, 0.3, capture=False)
        assert WIDE in rec["tail"]
        if first is None:
            first = out.clone()
        else:
            same_bytes(out.view(torch.uint8), first.view(torch.uint8), f"repeat {k}")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_wide_refusals_launch_nothing():
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.upsampler import get_upsampler
    _lib, lib = lib_()
    Cf, B, gh, gw = 512, 2, 2, 3
    up, _ = shared_upsampler(Cf)
    src, guid = make_inputs(B, Cf, gh, gw, "smooth", seed=3)
    src, guid = src.to(DEV), guid.to(DEV)
    text = text_rows(33, Cf, 3)
    rc_up = get_upsampler("resize_conv", 64, str(DEV), "bf16")
    rc_up.load_state_dict(Wt.make_resize_conv_weights(64, seed=3))
    rc_src, rc_guid = make_inputs(1, 64, 2, 2, "smooth", seed=3)
    cases = [
        ("narrow entry at Q = 33", dict(up=up, src=src, guid=guid, text=text, entry="narrow"), b"1 <= Q <= 32"),
        ("wide entry, SG_PREC_F32", dict(up=up, src=src, guid=guid, text=text, precision=_lib.PREC_F32), b"bf16 throughput path"),
        ("wide entry, resize_conv", dict(up=rc_up, src=rc_src.to(DEV), guid=rc_guid.to(DEV), text=text_rows(33, 64, 3)), b"resize_conv has no fused logits tail"),
        ("wide entry, workspace one byte short", dict(up=up, src=src, guid=guid, text=text, short=1), b"workspace"),
    ]
    for what, kw, msg in cases:
        u = kw.pop("up")
        s_, g_, t_ = kw.pop("src"), kw.pop("guid"), kw.pop("text")
        before = lib.sg_jbu_last_kernels()
        gh_, gw_ = (2, 2) if u is rc_up else (gh, gw)
        rc, err, untouched = run_wide(u, s_, g_, gh_, gw_, t_, 33, None, 0.0, capture=False, expect_ok=False, **kw)
        assert rc != 0 and err and msg in err, (what, rc, err)
        assert untouched, f"{what}: the refused call wrote to the output or the workspace"
        assert lib.sg_jbu_last_kernels() == before, f"{what}: the refused call changed the launch record"
