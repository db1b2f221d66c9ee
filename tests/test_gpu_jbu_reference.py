"""Every kernel of the HIP JBU upsampler (csrc/jbu.hip) against an f64 reference with a per-element bound (tests/jbu_reference.py).

The real kernel sequence of sg_jbu_upsample / sg_jbu_logits runs with capture on (sg_jbu_set_capture): after each kernel the library copies
what it read and wrote, in its stored format.  Each piece is then checked on the operands it actually consumed -- pool, range_proj, the
range x spatial kernel, the exact rounding of its operand rows, the two fixup GEMMs, the bicubic, the adaptive convolution of whichever
kernel dispatch chose, the stage-to-stage hand-over (bit for bit), the final 1x1 and the fused logits tail.  sg_jbu_last_kernels() says what
ran; the workspace and the output sit between NaN guard bands and are NaN-filled before the call, so a kernel that reads scratch no earlier
kernel wrote, or writes outside its region, shows up.  A final test asserts that every instantiation dispatch can reach ran at least once.
"""
import ctypes as C
import math
import os
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jbu_reference import (U, F32_TENTH, decode, encode, rounded, check_within, gemm_reference, gemm_bound, pool_reference,  # noqa: E402
                           range_proj_reference, range_reference, conv_reference, conv_bound, bicubic_rows, bicubic_bound, scaled_gemm,
                           median_tightness, sample_all, sample_border_blocks, half_ulp, rowdot_reference)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 1 << 16
RAN = set()                                   # instantiations seen in sg_jbu_last_kernels over the module
WORST = defaultdict(float)                    # (piece, fmt) -> largest err / bound
TIGHT = defaultdict(float)                    # (piece, fmt) -> largest median bound / |ref|
CHECKS = defaultdict(int)                     # (piece, fmt) -> checks run
# the median of bound / |ref| a piece's bound may reach per storage format (every bound must be able to fail)
TIGHT_LIMIT = {"f32": 2e-3, "h2": 2e-3, "bf16": 0.1, "f16": 0.1}
# ... except the range kernel's: a score error Delta moves the softmax weights by up to exp(2 Delta), Delta ~ temp 2u 33 |k|^2 with f32 keys
# and ~ temp 2^-10 |k|^2 with f16 keys (|k|^2 ~ 10 here)
RANGE_TIGHT_LIMIT = {"f32": 2e-2, "h2": 2e-2, "f16": 0.5}
# ... and the tail's sums of mixed-sign terms (g0 = bf . T, the row-dot slots sum z (2x + z)), whose |ref| sits well below the magnitude
# sum that bounds their rounding
SUM_TIGHT_LIMIT = {"tail_g0": 2e-2, "tail_rowdot": 5e-2, "tail_logits": 2e-2}
# designs whose softmax is ill-conditioned by construction (temperature 20 .. 1e4): the score rounding alone moves the weights by about
# their size, so the range kernel's bound is honest but cannot be tight there; its tightness is asserted on the other designs
ILL_CONDITIONED = {"temp_hi", "steps", "small_sigma"}


def lib_():
    from clip_decontamination_amd import _lib
    return _lib, _lib.load()


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- designs -----------------------------------------------------------------------------------------------------------------------
def make_weights(kind, Cf, design, seed=3):
    from clip_decontamination_amd import weights as Wt
    w = {k: np.array(v, dtype=np.float32) for k, v in Wt.make_jbu_weights(kind, Cf, seed=seed).items()}
    for k in list(w):
        if k.endswith("range_temp"):
            w[k] = np.asarray({"temp_lo": -12.0, "temp_hi": 12.0, "steps": math.log(60.0), "small_sigma": 12.0}.get(design, float(w[k])),
                              np.float32)
        if k.endswith("sigma_spatial") and design == "small_sigma":
            w[k] = np.asarray(0.05, np.float32)
    return w


def make_inputs(B, Cf, gh, gw, design, seed):
    g = torch.Generator().manual_seed(seed)
    GH, GW = 16 * gh, 16 * gw
    if design in ("smooth", "temp_lo", "temp_hi", "decades"):
        from clip_decontamination_amd import weights as Wt
        t = torch.from_numpy(Wt.make_tiles_u8(B, max(GH, GW), seed=seed, smooth=True)).float()[:, :GH, :GW]
        guid = ((t - torch.tensor([122.771, 116.746, 104.094])) / torch.tensor([68.501, 66.632, 70.323])).permute(0, 3, 1, 2)
    elif design == "const_guid":
        guid = torch.full((B, 3, GH, GW), 0.25)
    elif design == "small_sigma":               # a ramp: |key|^2 grows along it, so at temperature 1e4 an off-centre tap wins the softmax
        yy, xx = torch.meshgrid(torch.arange(GH), torch.arange(GW), indexing="ij")
        ramp = -2 + 4 * (yy + xx).float() / (GH + GW)
        guid = torch.stack([ramp, 0.5 * ramp, -ramp]).expand(B, 3, GH, GW).contiguous()
    elif design == "steps":                    # high-contrast vertical / horizontal steps: near one-hot range weights
        yy, xx = torch.meshgrid(torch.arange(GH), torch.arange(GW), indexing="ij")
        pat = (((yy // 12) + (xx // 20)) % 2).float() * 4 - 2
        guid = torch.stack([pat, -pat, pat * 0.5]).expand(B, 3, GH, GW) + 0.1 * torch.arange(B).view(B, 1, 1, 1)
    else:
        raise ValueError(design)
    src = torch.randn(B, gh * gw, Cf, generator=g)
    if design == "decades":                    # per-pixel magnitudes across four decades
        src = src * (10.0 ** torch.randint(-2, 2, (B, gh * gw, 1), generator=g).float())
    return src.contiguous(), guid.contiguous()


# ---- running with capture ----------------------------------------------------------------------------------------------------------
def expected_dispatch(kind, prec, Cf, gh, gw, B):
    """What jbu_stages / the final GEMM / the tail dispatch for a configuration (the product's rules, restated), with each stage's
    convolution grid: 8 x 8 pixel blocks x images (the VALU kernel: x 32-channel chunks in between)."""
    r = 5 if kind == "jbu_one" else 3
    fast = prec == "bf16" and Cf % 8 == 0
    x2 = prec == "f16x2"
    low = prec == "bf16" and Cf % 64 == 0 and gh >= 2 and gw >= 2
    x2low = x2 and Cf % 64 == 0 and gh >= 2 and gw >= 2
    e = {}
    for k in range(4):
        e[f"s{k}.range"] = f"jbu_kernel_mfma_kernel<{r},{'true' if x2 else 'false'}>" if (x2 or fast) else "jbu_kernel_tiled_kernel<0,false>"
        e[f"s{k}.x16"] = "h2" if x2 else ("f16" if low else "bf16") if fast else "none"
        e[f"s{k}.kf"] = "f16" if low else "f32"
        e[f"s{k}.src"] = "h2" if x2low else "bf16" if low else "f32"
        e[f"s{k}.conv"] = (f"jbu_conv_lowres_x2_kernel<{r}>" if x2low else f"jbu_conv_lowres_kernel<{r}>" if low else
                           "jbu_adaptive_conv_mfma_kernel" if fast else "jbu_adaptive_conv_kernel")
        e[f"s{k}.bicubic"] = "none" if (x2low or low) else "jbu_bicubic_kernel<bf16_t>" if fast else "jbu_bicubic_kernel<float>"
        e[f"s{k}.out16"] = "h2" if x2low else "bf16" if low else "none"
        blocks = -(-(gh << (k + 1)) // 8) * -(-(gw << (k + 1)) // 8)
        e[f"s{k}.grid"] = f"{blocks}x{-(-Cf // 32)}x{B}" if e[f"s{k}.conv"] == "jbu_adaptive_conv_kernel" else f"{blocks}x{B}x1"
    e["final.a"] = "bf16" if (prec == "bf16" and Cf % 64 == 0) else "h2" if (x2 and Cf % 32 == 0) else "f32"
    if e["final.a"] == "f32":
        e["final"] = "gemm_f32"
    return e


def run(up, src, guid, gh, gw, *, slots="all", logits=None):
    """Run sg_jbu_upsample (or sg_jbu_logits with logits = (text, Q, cls, lambda)) with capture of `slots` ('all' or a set of
    (stage, name) / ('tail', name)) between NaN guard bands.  Returns (out, captured {key: uint8 tensor}, record dict, need)."""
    _lib, lib = lib_()
    B = src.shape[0]
    Cf = up.feat_dim
    need = lib.sg_jbu_workspace_bytes(up._ctx, B, gh, gw)
    ws = torch.full(((need + 2 * GUARD) // 4 + 1,), float("nan"), device=DEV)
    P = 256 * gh * gw
    if logits is None:
        n_out = B * P * Cf
    else:
        n_out = B * logits[1] * P
    out = torch.full((n_out + 2 * GUARD // 4,), float("nan"), device=DEV)
    cap = _lib.JbuCapture()
    bufs = {}
    Hs = [(gh << (k + 1), gw << (k + 1)) for k in range(4)]
    rows = 128 * 4                              # the widest row any per-pixel slot holds (KP1 two-plane: 128 x 4 bytes)
    for k in range(4):
        px = B * Hs[k][0] * Hs[k][1]
        for i, name in enumerate(_lib.JBU_CAP_STAGE):
            if slots != "all" and (k, name) not in slots:
                continue
            nb = px * (rows if name in ("GS", "PROJ", "X", "X16", "H1", "KF") else Cf * 4)
            t = torch.empty(nb, dtype=torch.uint8, device=DEV)
            bufs[(k, name)] = t
            cap.stage[k][i].dst, cap.stage[k][i].cap = t.data_ptr(), nb
    px = B * P
    for i, name in enumerate(_lib.JBU_CAP_TAIL):
        if slots != "all" and ("tail", name) not in slots:
            continue
        nb = {"GEFF": Cf * 32 * 4, "G0": 128, "CLSL": B * 128, "ROWDOT": px * (Cf // 64 + 1) * 4}.get(name, px * Cf * 4)
        t = torch.empty(nb, dtype=torch.uint8, device=DEV)
        bufs[("tail", name)] = t
        cap.tail[i].dst, cap.tail[i].cap = t.data_ptr(), nb
    torch.cuda.synchronize()
    _lib.check(lib.sg_jbu_set_capture(up._ctx, C.addressof(cap)), "sg_jbu_set_capture")
    try:
        wsp = ptr(ws, GUARD)
        if logits is None:
            rc = lib.sg_jbu_upsample(up._ctx, ptr(src), ptr(guid), B, gh, gw, guid.shape[-2], guid.shape[-1], up.precision,
                                     ptr(out, GUARD), wsp, need, stream())
        else:
            text, Q, cls, lam = logits
            rc = lib.sg_jbu_logits(up._ctx, ptr(src), ptr(guid), B, gh, gw, guid.shape[-2], guid.shape[-1], up.precision, ptr(text), Q,
                                   ptr(cls) if cls is not None else None, lam, ptr(out, GUARD), wsp, need, stream())
        _lib.check(rc, "sg_jbu_upsample" if logits is None else "sg_jbu_logits")
        torch.cuda.synchronize()
    finally:
        lib.sg_jbu_set_capture(up._ctx, None)
    rec = dict(tok.split("=", 1) for tok in lib.sg_jbu_last_kernels().decode().split())
    for key, val in rec.items():
        if key.endswith((".range", ".conv", ".bicubic")) or key == "final":
            RAN.add(val)
        if key == "tail":
            RAN.update(val.split(","))
    RAN.add(f"final:{rec.get('final.a')}")
    # guard bands: nothing written outside the workspace and the output
    wb = ws.view(torch.uint8)
    nanb = torch.full((1,), float("nan"), device=DEV).view(torch.uint8)
    for what, band in (("workspace head", wb[:GUARD]), ("workspace tail", wb[GUARD + need:GUARD + need + GUARD - 4]),
                       ("output head", out.view(torch.uint8)[:GUARD]), ("output tail", out.view(torch.uint8)[GUARD + 4 * n_out:])):
        assert bool((band.view(-1, 4) == nanb).all()), f"{what} guard band overwritten"
    got = out[GUARD // 4:GUARD // 4 + n_out]
    assert bool(torch.isfinite(got).all()), "non-finite output"
    capd = {}
    for key, t in bufs.items():
        i = (_lib.JBU_CAP_STAGE.index(key[1]) if key[0] != "tail" else _lib.JBU_CAP_TAIL.index(key[1]))
        nb = cap.stage[key[0]][i].bytes if key[0] != "tail" else cap.tail[i].bytes
        if nb:
            capd[key] = t[:nb]
    return got, capd, rec, need


def note(piece, fmt, ratio, tight, check_tight=True, operands=None):
    """Record a piece's largest err / bound and assert its median bound / |ref| below the limit of its operand format (default: fmt)."""
    WORST[(piece, fmt)] = max(WORST[(piece, fmt)], ratio)
    CHECKS[(piece, fmt)] += 1
    if not check_tight:
        return
    TIGHT[(piece, fmt)] = max(TIGHT[(piece, fmt)], tight)
    lim = SUM_TIGHT_LIMIT[piece] if piece in SUM_TIGHT_LIMIT else (RANGE_TIGHT_LIMIT if piece == "range" else TIGHT_LIMIT)[operands or fmt]
    assert tight < lim, f"{piece} [{fmt}]: median bound / |ref| = {tight:.3g} (limit {lim}): bound too loose"


def same_bytes(a, b, what):
    """Bit-for-bit equality, in chunks of 2^28 bytes (index tensors past 2^31 elements are not to be trusted)."""
    assert a.numel() == b.numel(), f"{what}: {a.numel()} vs {b.numel()} bytes"
    step = 1 << 28
    for o in range(0, a.numel(), step):
        bad = (a[o:o + step] != b[o:o + step]).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} bytes differ in chunk {o >> 28}, first at byte {o + int(bad[0])}"


# ---- the per-stage checks ----------------------------------------------------------------------------------------------------------
def check_chain(up, w, src, guid, gh, gw, prec, capd, rec, out, *, full=True, n_random=2000, seed=0, design="smooth"):
    """All pieces of all stages (full) or the last stage's convolution and the final 1x1 on sampled pixels."""
    kind = up.model_name
    B, Cf = src.shape[0], up.feat_dim
    r = 5 if kind == "jbu_one" else 3
    d = 2 * r + 1
    d2 = d * d
    NP, KP1 = (d2 + 63) // 64 * 64, (d2 + 3 + 63) // 64 * 64
    exp = expected_dispatch(kind, prec, Cf, gh, gw, B)
    for key, val in exp.items():
        assert rec.get(key) == val, f"dispatch {key}: ran {rec.get(key)}, expected {val} ({rec})"
    prev_out = None
    h, wd = gh, gw
    for k in range(4):
        up_name = "up" if kind == "jbu_one" else f"up{k + 1}"
        W_ = {n: torch.from_numpy(w[f"{up_name}.{n}"]).to(DEV) for n in ("range_proj.0.weight", "range_proj.0.bias", "range_proj.3.weight",
                                                                       "range_proj.3.bias", "fixup_proj.0.weight", "fixup_proj.0.bias",
                                                                       "fixup_proj.3.weight", "fixup_proj.3.bias")}
        rt, sig = float(w[f"{up_name}.range_temp"]), float(w[f"{up_name}.sigma_spatial"])
        H, Wd = 2 * h, 2 * wd
        px = B * H * Wd
        x16f, kff, srcf, o16f = rec[f"s{k}.x16"], rec[f"s{k}.kf"], rec[f"s{k}.src"], rec[f"s{k}.out16"]
        conv = rec[f"s{k}.conv"]
        if full or k == 3:
            bb, yy, xx = sample_all(B, H, Wd, DEV) if full else sample_border_blocks(B, H, Wd, n_random, seed + k, DEV)
            pix = (bb * H + yy) * Wd + xx
        if full:
            # pool and range_proj
            gs = decode(capd[(k, "GS")], "f32", 3)
            ref, bnd = pool_reference(guid.to(DEV), H, Wd)
            note("pool", "f32", check_within(gs, ref.reshape(-1, 3), bnd.reshape(-1, 3), f"s{k} pool"), median_tightness(bnd, ref))
            proj = decode(capd[(k, "PROJ")], "f32", 32)
            ref, bnd = range_proj_reference(gs, W_["range_proj.0.weight"].view(32, 3), W_["range_proj.0.bias"],
                                            W_["range_proj.3.weight"].view(32, 32), W_["range_proj.3.bias"])
            note("range_proj", "f32", check_within(proj, ref, bnd, f"s{k} range_proj"), median_tightness(bnd, ref))
            # range x spatial kernel
            keys = {"h2": "h2", "bf16": "f16", "f16": "f16", "none": "f32"}[x16f]
            Xr, Xb, fired = range_reference(proj.float().view(B, H, Wd, 32), r, rt, sig, keys, bb, yy, xx)
            if (k, "X") in capd:
                X = decode(capd[(k, "X")], "f32", d2 + 3)
                note("range", "f32" if keys == "f32" else keys, check_within(X[pix, :d2], Xr, Xb, f"s{k} range kernel X"), median_tightness(Xb, Xr),
                     design not in ILL_CONDITIONED)
                same_bytes(capd[(k, "X")].view(torch.float32).view(-1, d2 + 3)[:, d2:].contiguous().view(torch.uint8).reshape(-1),
                           capd[(k, "GS")], f"s{k} X guidance columns")
            if x16f != "none":
                X16 = decode(capd[(k, "X16")], x16f, KP1)
                if (k, "X") in capd:                  # operand rows = the rounding of the f32 rows, bit for bit; zero padding
                    Xrow = torch.zeros(px, KP1, dtype=torch.float32, device=DEV)
                    Xrow[:, :d2 + 3] = capd[(k, "X")].view(torch.float32).view(-1, d2 + 3)
                    same_bytes(capd[(k, "X16")], encode(Xrow, x16f), f"s{k} X16 = {x16f}(X)")
                else:                                 # f16 rows of the all-f16 chain: against the reference, guidance and padding exact
                    bx = Xb + half_ulp(Xr.abs() + Xb, "f16")
                    note("range", "f16", check_within(X16[pix, :d2], Xr, bx, f"s{k} range kernel X16"), median_tightness(bx, Xr),
                         design not in ILL_CONDITIONED)
                    assert torch.equal(X16[:, d2:d2 + 3], rounded(gs.float(), "f16")), f"s{k} X16 guidance columns"
                    assert bool((X16[:, d2 + 3:] == 0).all()), f"s{k} X16 padding columns"
            # fixup GEMMs
            W0 = W_["fixup_proj.0.weight"].view(d2, d2 + 3)
            W3 = W_["fixup_proj.3.weight"].view(d2, d2)
            if x16f == "none":
                A, W0r, hf, ld1 = decode(capd[(k, "X")], "f32", d2 + 3), W0, "f32", d2
            else:
                A = X16
                W0p = torch.zeros(NP, KP1, device=DEV)
                W0p[:d2, :d2 + 3] = W0
                W0r = W0p if x16f == "h2" else rounded(W0p, x16f)
                hf, ld1 = x16f, NP
            b0 = torch.zeros(W0r.shape[0], dtype=torch.float64, device=DEV)
            b0[:d2] = W_["fixup_proj.0.bias"].double()
            pre, ref = gemm_reference(A, W0r, b0, None, 2)
            bnd = gemm_bound(A, W0r, b0, pre, ref, act=2, out_fmt=hf, two_plane=hf == "h2", fast_act=hf in ("bf16", "f16"))
            H1 = decode(capd[(k, "H1")], hf, ld1)
            note("fixup0", hf, check_within(H1[:, :d2], ref[:, :d2], bnd[:, :d2], f"s{k} fixup GELU GEMM"), median_tightness(bnd[:, :d2], ref[:, :d2]))
            if ld1 > d2:
                assert bool((H1[:, d2:] == 0).all()), f"s{k} H1 padding columns"
            b01 = (W_["fixup_proj.3.bias"].float() * torch.tensor(F32_TENTH, dtype=torch.float32)).double()
            res = decode(capd[(k, "X16")], "f16", KP1)[:, :d2] if kff == "f16" else decode(capd[(k, "X")], "f32", d2 + 3)[:, :d2]
            W3r = W3 if hf in ("f32", "h2") else rounded(W3, hf)
            ref, bnd = scaled_gemm(H1[:, :d2], W3r, b01, res, out_fmt=kff, two_plane=hf == "h2")
            ldk = d2 if x16f == "none" else NP
            Kf = decode(capd[(k, "KF")], kff, ldk)
            note("fixup1", kff, check_within(Kf[:, :d2], ref, bnd, f"s{k} fixup residual GEMM"), median_tightness(bnd, ref))
        if (k, "SRC") not in capd:                  # sampled mode: only the last stage was captured
            h, wd = H, Wd
            continue
        # the convolution's source: stage 0 = the tokens as stored, later stages = the previous stage's stored output, bit for bit
        S = capd[(k, "SRC")]
        if k == 0:
            same_bytes(S, encode(src.to(DEV).view(-1, Cf), srcf), "s0 source")
        elif prev_out is not None:
            same_bytes(S, prev_out, f"s{k} source = stage {k - 1} output")
        srcv = decode(S, srcf, Cf).view(B, h, wd, Cf)
        if (k, "OUT16") in capd:
            prev_out = capd[(k, "OUT16")]
        elif (k, "OUT") in capd:
            prev_out = capd[(k, "OUT")]
        if not (full or k == 3):
            h, wd = H, Wd
            continue
        Kf = decode(capd[(k, "KF")], kff, d2 if x16f == "none" else NP)[:, :d2].reshape(B, H, Wd, d2)
        if conv.startswith("jbu_adaptive_conv"):
            hrf = "bf16" if "mfma" in conv else "f32"
            hr = decode(capd[(k, "HR")], hrf, Cf).view(B, H, Wd, Cf)
            val, mag = bicubic_rows(srcv, bb, yy, xx, H, Wd)
            bnd = bicubic_bound(mag, val, hrf)
            note("bicubic", hrf, check_within(hr[bb, yy, xx], val, bnd, f"s{k} bicubic"), median_tightness(bnd, val))
            cref = conv_reference(Kf, r, bb, yy, xx, hr=hr)
            ckind = "mfma" if "mfma" in conv else "valu"
        else:
            cref = conv_reference(Kf, r, bb, yy, xx, src=srcv)
            ckind = "lowres_x2" if "x2" in conv else "lowres"
        for slot, fmt in (("OUT", "f32"), ("OUT16", o16f)):
            if (k, slot) not in capd:
                continue
            o = decode(capd[(k, slot)], fmt, Cf, rows=(bb * H + yy) * Wd + xx)
            bnd = conv_bound(cref, ckind, r, fmt, src=srcv, b=bb, y=yy, x=xx)
            note(f"conv_{ckind}", fmt, check_within(o, cref["out"], bnd, f"s{k} {conv} -> {slot}"), median_tightness(bnd, cref["out"]),
                 operands={"valu": "f32", "mfma": "bf16", "lowres": "bf16", "lowres_x2": "h2"}[ckind])
        if (k, "OUT") in capd and (k, "OUT16") in capd:
            same_bytes(capd[(k, "OUT16")], encode(capd[(k, "OUT")].view(torch.float32).view(-1, Cf), o16f), f"s{k} OUT16 = {o16f}(OUT)")
        h, wd = H, Wd
    return bb, yy, xx


def check_final(up, w, capd, rec, out, bb, yy, xx, gh, gw):
    """out = x + 0.1 (x . Wf^T + bf) on the captured A operand and f32 residual, plus the bit-for-bit hand-over from the last stage."""
    Cf = up.feat_dim
    fa = rec["final.a"]
    if (3, "OUT") in capd:
        same_bytes(capd[("tail", "FIN_RES")], capd[(3, "OUT")], "final residual = stage-3 output")
    if fa == "bf16" and (3, "OUT16") in capd:
        same_bytes(capd[("tail", "FIN_A")], capd[(3, "OUT16")], "final A = stage-3 bf16 copy")
    same_bytes(capd[("tail", "FIN_A")], encode(capd[("tail", "FIN_RES")].view(torch.float32).view(-1, Cf), fa), f"final A = {fa}(x)")
    H, Wd = 16 * gh, 16 * gw
    pix = (bb * H + yy) * Wd + xx
    A = decode(capd[("tail", "FIN_A")], fa, Cf, rows=pix)
    R = decode(capd[("tail", "FIN_RES")], "f32", Cf, rows=pix)
    Wf = torch.from_numpy(w["fixup_proj.1.weight"]).to(DEV).view(Cf, Cf)
    Wr = Wf if fa in ("f32", "h2") else rounded(Wf, fa)
    b01 = (torch.from_numpy(w["fixup_proj.1.bias"]).to(DEV).float() * torch.tensor(F32_TENTH, dtype=torch.float32)).double()
    ref, bnd = scaled_gemm(A, Wr, b01, R, out_fmt="f32", two_plane=fa == "h2")
    got = out.view(-1, Cf)[pix]
    note("final", "f32", operands=fa, ratio=check_within(got, ref, bnd, f"final 1x1 ({rec.get('final')})"), tight=median_tightness(bnd, ref))


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def upsampler(kind, Cf, prec, w):
    from clip_decontamination_amd.upsampler import get_upsampler
    up = get_upsampler(kind, Cf, str(DEV), prec)
    up.load_state_dict(w)
    return up


CASES = [
    # kind, C, prec, (gh, gw), B, design
    ("jbu_stack", 36, "bf16", (2, 2), 1, "smooth"),        # C % 8 != 0: the whole f32 chain under bf16; smallest jbu_stack grid
    ("jbu_one", 36, "f16x2", (3, 3), 1, "smooth"),         # ragged 32-channel chunk; smallest jbu_one grid (r = oh - 1)
    ("jbu_one", 36, "f32", (3, 5), 2, "steps"),
    ("jbu_one", 40, "bf16", (3, 3), 1, "smooth"),          # bf16 MFMA convolution without the low-res path, f32 final GEMM
    ("jbu_stack", 40, "bf16", (5, 3), 3, "decades"),
    ("jbu_stack", 40, "f16x2", (3, 5), 1, "smooth"),        # f16x2, C % 64 != 0: two-plane fixups, f32 bicubic + VALU conv, f32 final
    ("jbu_stack", 64, "bf16", (2, 2), 1, "const_guid"),
    ("jbu_one", 64, "f16x2", (3, 3), 2, "temp_hi"),
    ("jbu_stack", 64, "f32", (5, 3), 1, "temp_lo"),
    ("jbu_stack", 64, "bf16", (3, 5), 3, "smooth"),
    ("jbu_stack", 64, "f32", (3, 5), 1, "small_sigma"),     # clamp(1e-7) fires: off-centre argmax at temperature 1e4, sigma 0.05
    ("jbu_one", 96, "f16x2", (3, 3), 1, "smooth"),          # f16x2, C % 32 == 0, C % 64 != 0: VALU conv + two-plane final GEMM
    ("jbu_stack", 192, "bf16", (3, 3), 1, "steps"),         # 1.5 chunks of 128 channels
    ("jbu_stack", 192, "f16x2", (5, 5), 1, "decades"),
    ("jbu_one", 192, "f32", (3, 3), 1, "smooth"),
    ("jbu_stack", 512, "f16x2", (2, 2), 3, "smooth"),
    ("jbu_one", 640, "bf16", (3, 3), 1, "smooth"),
]


@pytest.mark.parametrize("kind,Cf,prec,grid,B,design", CASES, ids=[f"{c[0]}-C{c[1]}-{c[2]}-{c[3][0]}x{c[3][1]}-B{c[4]}-{c[5]}" for c in CASES])
def test_jbu_pieces_vs_f64(kind, Cf, prec, grid, B, design):
    gh, gw = grid
    w = make_weights(kind, Cf, design)
    src, guid = make_inputs(B, Cf, gh, gw, design, seed=Cf + gh + 7 * gw)
    up = upsampler(kind, Cf, prec, w)
    src, guid = src.to(DEV), guid.to(DEV)
    out, capd, rec, _ = run(up, src, guid, gh, gw)
    bb, yy, xx = check_chain(up, w, src, guid, gh, gw, prec, capd, rec, out, design=design)
    check_final(up, w, capd, rec, out, bb, yy, xx, gh, gw)
    if design == "small_sigma":                 # the clamp(1e-7) branch fires somewhere, as the reference says
        r = 5 if kind == "jbu_one" else 3
        proj = decode(capd[(0, "PROJ")], "f32", 32).float().view(B, 2 * gh, 2 * gw, 32)
        b_, y_, x_ = sample_all(B, 2 * gh, 2 * gw, DEV)
        _, _, fired = range_reference(proj, r, float(w["up1.range_temp"]), 0.05, "f32", b_, y_, x_)
        assert bool(fired.any()), "small sigma: the normalisation clamp never fired"
    print(f"{kind} C={Cf} {prec} {gh}x{gw} B={B} {design}: worst err/bound so far {max(WORST.values()):.3g}")


def test_jbu_trained_weights_vs_f64(golden):
    """The reference's trained JBUStack(512) checkpoint in the exact and the throughput mode."""
    g = golden("jbu_real")
    w = {k[2:]: np.asarray(v, np.float32) for k, v in g.items() if k.startswith("w.")}
    assert w, "jbu_real.npz lost its w.* weight keys"
    src = torch.from_numpy(g["src"]).float()
    guid = torch.from_numpy(g["guidance"]).float()
    B, Cf, gh, gw = src.shape
    tok = src.permute(0, 2, 3, 1).reshape(B, gh * gw, Cf).contiguous().to(DEV)
    guid = guid.contiguous().to(DEV)
    for prec in ("bf16", "f16x2"):
        up = upsampler("jbu_stack", Cf, prec, w)
        out, capd, rec, _ = run(up, tok, guid, gh, gw)
        bb, yy, xx = check_chain(up, w, tok, guid, gh, gw, prec, capd, rec, out)
        check_final(up, w, capd, rec, out, bb, yy, xx, gh, gw)


def test_f16_is_routed_to_bf16():
    w = make_weights("jbu_stack", 64, "smooth")
    up = upsampler("jbu_stack", 64, "f16", w)
    _lib, _ = lib_()
    assert up.precision == _lib.PREC_BF16
    src, guid = make_inputs(1, 64, 2, 2, "smooth", 1)
    _, _, rec, _ = run(up, src.to(DEV), guid.to(DEV), 2, 2, slots=set())
    assert rec["s0.conv"] == "jbu_conv_lowres_kernel<3>" and rec["final.a"] == "bf16", rec


@pytest.mark.parametrize("kind,prec,B,Cf", [("jbu_stack", "bf16", 8, 512), ("jbu_one", "f16x2", 8, 512), ("jbu_stack", "bf16", 9, 1024),
                                            ("jbu_stack", "f16x2", 9, 1024)],
                         ids=["bench-bf16", "bench-one-f16x2", "2^31-bf16", "2^31-f16x2"])
def test_jbu_launch_shapes_sampled(kind, prec, B, Cf):
    """32 x 32 -> 512 x 512 at B = 8 (the bench shape) and a feature map past 2^31 elements (B = 9, C = 1024): the last stage's
    convolution and the final 1x1 on sampled pixels (borders, every block's last row and column, a random sample, the last pixel)."""
    gh = gw = 32
    w = make_weights(kind, Cf, "smooth")
    src, guid = make_inputs(B, Cf, gh, gw, "smooth", seed=B)
    up = upsampler(kind, Cf, prec, w)
    slots = {(3, "SRC"), (3, "KF"), (3, "OUT"), (3, "OUT16"), ("tail", "FIN_A"), ("tail", "FIN_RES")}
    if B * 256 * gh * gw * Cf > 2 ** 31:
        slots -= {(3, "OUT")}
    out, capd, rec, _ = run(up, src.to(DEV), guid.to(DEV), gh, gw, slots=slots)
    bb, yy, xx = check_chain(up, w, src.to(DEV), guid.to(DEV), gh, gw, prec, capd, rec, out, full=False, n_random=4000, seed=B)
    check_final(up, w, capd, rec, out, bb, yy, xx, gh, gw)
    del out, capd
    torch.cuda.empty_cache()


# ---- fused logits tail ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 9, 16, 17, 32])
@pytest.mark.parametrize("with_cls", [False, True])
def test_jbu_logits_tail_vs_f64(Q, with_cls):
    kind, Cf, gh, gw, B = "jbu_stack", 640 if Q in (9, 32) else 512, 2, 3, 2
    w = make_weights(kind, Cf, "smooth")
    src, guid = make_inputs(B, Cf, gh, gw, "smooth", seed=Q)
    src, guid = src.to(DEV), guid.to(DEV)
    g = torch.Generator().manual_seed(Q)
    text = torch.nn.functional.normalize(torch.randn(Q, Cf, generator=g), dim=-1).to(DEV).contiguous()
    cls = torch.randn(B, Cf, generator=g).to(DEV).contiguous() if with_cls else None
    lam = 0.3 if with_cls else 0.0
    up = upsampler(kind, Cf, "bf16", w)
    slots = {(3, "OUT16"), ("tail", "FIN_A"), ("tail", "GEFF"), ("tail", "G0"), ("tail", "CLSL"), ("tail", "ROWDOT")}
    out, capd, rec, _ = run(up, src, guid, gh, gw, slots=slots, logits=(text, Q, cls, lam))
    tail = rec["tail"].split(",")
    want = "jbu_pixel_logits_mfma_kernel" if Q <= 16 else "jbu_pixel_logits_kernel<32>"
    assert want in tail and "jbu_geff_kernel" in tail and (("jbu_cls_logits_kernel" in tail) == with_cls), rec
    same_bytes(capd[("tail", "FIN_A")], capd[(3, "OUT16")], "tail A = stage-3 bf16 output")
    P = 256 * gh * gw
    x = decode(capd[("tail", "FIN_A")], "bf16", Cf)                        # [px, C]
    T = text.double()
    Wf = torch.from_numpy(w["fixup_proj.1.weight"]).to(DEV).view(Cf, Cf).double()
    bf01 = (torch.from_numpy(w["fixup_proj.1.bias"]).to(DEV).float() * torch.tensor(F32_TENTH, dtype=torch.float32)).double()
    # Geff[c, q] = T[q, c] + 0.1f sum_k Wf[k, c] T[q, k]: f32 sums of C products (2u (C + 2)), the 0.1f product and the add, the store
    geff = decode(capd[("tail", "GEFF")], "f32", 32)[:, :Q]
    S = Wf.abs().T @ T.abs().T
    ref = T.T + F32_TENTH * (Wf.T @ T.T)
    bnd = F32_TENTH * 2 * U * (Cf + 2) * S + 2 * U * (T.T.abs() + F32_TENTH * S)
    bnd = bnd + half_ulp(ref.abs() + bnd, "f32")
    note("tail_geff", "f32", check_within(geff, ref, bnd, "Geff"), median_tightness(bnd, ref))
    g0 = decode(capd[("tail", "G0")], "f32", 32)[0, :Q]
    ref = T @ bf01
    bnd = 2 * U * (Cf + 2) * (T.abs() @ bf01.abs())
    bnd = bnd + half_ulp(ref.abs() + bnd, "f32")
    note("tail_g0", "f32", check_within(g0, ref, bnd, "g0"), median_tightness(bnd, ref))
    if with_cls:
        clsl = decode(capd[("tail", "CLSL")], "f32", 32)[:, :Q]
        c = cls.double()
        nrm = c.norm(dim=-1, keepdim=True)
        ref = (c @ T.T) / nrm
        # dot: 2u (C + 1) |cls| . |T|; 1 / sqrt(sum cls^2): the sum (2u C relative) halved by the root, the root and the division (EXPF each),
        # the product (u)
        bnd = 2 * U * (Cf + 1) * (c.abs() @ T.abs().T) / nrm + ref.abs() * (U * Cf + 2 * 2.0 ** -22 + U)
        bnd = bnd + half_ulp(ref.abs() + bnd, "f32")
        note("tail_cls", "f32", check_within(clsl, ref, bnd, "cls logits"), median_tightness(bnd, ref))
    # row-dot slots: sum over 64 columns of z (2x + z), z = 0.1f x . Wf16^T + bf01 with the GEMM bound bz on z
    slots_n = Cf // 64
    rd = decode(capd[("tail", "ROWDOT")], "f32", slots_n)
    ref, bnd = rowdot_reference(x, rounded(Wf.float(), "bf16"), bf01)
    note("tail_rowdot", "f32", check_within(rd, ref, bnd, "row-dot slots"), median_tightness(bnd, ref))
    # logits on the captured operands: (x . Geff + g0) / sqrt(|x|^2 + sum slots) + lambda clsl
    G = decode(capd[("tail", "GEFF")], "f32", 32)[:, :Q]
    num = x @ G + g0[None]
    SxG = x.abs() @ G.abs()
    n2 = (x * x).sum(-1) + rd.sum(-1)
    inv = n2.rsqrt()
    clv = (lam * decode(capd[("tail", "CLSL")], "f32", 32)[:, :Q]) if with_cls else torch.zeros(B, Q, dtype=torch.float64, device=DEV)
    bidx = torch.arange(B * P, device=DEV) // P
    ref = num * inv[:, None] + clv[bidx]
    # numerator: Geff as two bf16 planes (matrix-pipe form: 2^-16 |G|) or f32 (VALU form); f32 accumulation 2u (2C + 1) S; g0 add.
    # |x|^2 (2u C) and the fixed-order slot sum (2u slots) relative to |x|^2 + sum |slots|; 1 / sqrt: two roundings of EXPF, halved sum error
    rep = 2.0 ** -16 * SxG if Q <= 16 else 0.0
    dN = rep + 2 * U * (2 * Cf + 1) * SxG + U * (SxG + g0.abs()[None])
    rho = (2 * U * Cf * (x * x).sum(-1) + 2 * U * (slots_n + 1) * ((x * x).sum(-1) + rd.abs().sum(-1))) / n2 / 2 + 2 * 2.0 ** -22
    bnd = dN * inv[:, None] * (1 + rho[:, None]) + num.abs() * inv[:, None] * rho[:, None] + 2 * U * num.abs() * inv[:, None] + 2 * U * clv.abs()[bidx]
    bnd = bnd + half_ulp(ref.abs() + bnd, "f32")
    got = out.view(B, Q, P).permute(0, 2, 1).reshape(B * P, Q)
    note("tail_logits", "f32", check_within(got, ref, bnd, f"logits Q={Q}"), median_tightness(bnd, ref))
    print(f"tail Q={Q} cls={with_cls}: worst err/bound {max(WORST.values()):.3g}")


def test_zz_every_reachable_instantiation_ran():
    """Runs last (module order): every instantiation dispatch can reach was launched by some case above.  Unreachable ones (radius is
    always 3 or 5, the matrix-pipe tail takes Q <= 16) are listed in DESIGN.md section 4."""
    want = {"jbu_kernel_tiled_kernel<0,false>", "jbu_kernel_mfma_kernel<5,false>", "jbu_kernel_mfma_kernel<3,false>",
            "jbu_kernel_mfma_kernel<5,true>", "jbu_kernel_mfma_kernel<3,true>", "jbu_bicubic_kernel<float>", "jbu_bicubic_kernel<bf16_t>",
            "jbu_adaptive_conv_kernel", "jbu_adaptive_conv_mfma_kernel", "jbu_conv_lowres_kernel<5>", "jbu_conv_lowres_kernel<3>",
            "jbu_conv_lowres_x2_kernel<5>", "jbu_conv_lowres_x2_kernel<3>", "jbu_pixel_logits_mfma_kernel", "jbu_pixel_logits_kernel<32>",
            "jbu_geff_kernel", "jbu_cls_logits_kernel", "gemm_f32", "final:f32", "final:bf16", "final:h2"}
    missing = want - RAN
    for key in sorted(WORST):
        print(f"  {key[0]:>16} [{key[1]:>4}]: {CHECKS[key]:3d} checks, max err/bound {WORST[key]:.3g}, median bound/|ref| up to {TIGHT[key]:.3g}")
    assert not missing, f"never ran: {sorted(missing)}"
