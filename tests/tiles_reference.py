"""References, per-element bounds, f32 restatements and case generators for the three small kernels at the end of csrc/jbu.hip:
extract_tiles_kernel (sg_extract_tiles), global_debias_kernel (sg_global_debias) and adaptive_conv_nchw_kernel (sg_adaptive_conv).  Used
by tests/test_gpu_tiles_reference.py and tests/test_tiles_bound_cpu.py.  Plain numpy / torch on the CPU.

sg_extract_tiles is exact.  From an f32 [B,3,H,W] scene the output holds the scene's bytes inside the window and +0.0 in the left / top
pad and in the band right of / below tile + pad.  From a u8 [B,H,W,3] scene it holds (float(u) - mean[c]) / std[c] evaluated in IEEE
float32 -- one rounding in the subtraction, one in the division, which is what numpy float32 and torch compute and what HIP's default
correctly rounded f32 division gives.  That plain quotient is NOT always the nearest f32 of the real quotient: quotient_table() compares
it with the float64 quotient of the same f32 constants.  Where the subtraction is exact (|u - mean| < 128, and all of channel 1, whose
mean has a zero last bit) the plain quotient is the nearest f32 (<= 0.5 ulp).  Where it rounds as well -- channel 2 from u = 233 and
channel 0 from u = 251 -- the error reaches 1.374 ulp (channel 2, u = 234) and 1.202 ulp (channel 0, u = 255).  patchify_kernel corrects
exactly those cells to the nearest f32 (csrc/patchify.hip, whose comment names channel 2 only; its test e != 0 covers both);
extract_tiles_kernel keeps the plain quotient, because the guidance image must stay the value torch computes from the same bytes.
A window that leaves the scene is outside the kernel's domain: the windows live on the device, the host entry cannot validate them, and
keeping them inside the scene is the caller's contract.  Every generated window is inside its scene (asserted by the CPU module); no test
passes one that is not.

sg_global_debias is held to the float64 value of  out = x - c (<x, c> / (|x| |c|) factor),  c = cls / |cls|,  on the f32 inputs, with a
per-element bound that follows the kernel's order (u = 2^-24; 2u per f32 operation; a 64-lane strided sum of n terms g = 2u (ceil(n / 64)
+ 7) relative to the sum of the terms' magnitudes; sqrtf and the reciprocal within 2 ulp = 4u, ASSUMED):
  1. s_inv = 1 / sqrtf(sum cls^2):   r_s = (1 - g)^-1/2 - 1, then 4u, 4u                          (relative)
  2. c_i = cls_i s_inv:              r_c = r_s, 2u                                                  (relative to cls_i / |cls|)
  3. ff = sum x^2:  g.   cc = sum c_i^2:  r_cc = r_c, r_c, g.   fc = sum x_i c_i is a sum of mixed sign, so its error is absolute:
     e_fc = (r_c + g (1 + r_c)) sum |x_i c_i|
  4. w = fc / (sqrtf(ff) sqrtf(cc)) factor:  the denominator r_den = sqrt of g, 4u, sqrt of r_cc, 4u, 2u; the quotient misses the exact
     cosine q by e_q = |q| r_inv + e_fc / (|x| |c|) (1 + r_inv), r_inv = 1 / (1 - r_den) - 1; the division and the product with factor
     2u each:  e_w = |factor| (e_q + (|q| + e_q) ((1 + 2u)^2 - 1))
  5. out_i = x_i - (cls_i s_inv) w:  e_p = |c_i| (|w| ((1 + r_c)(1 + 2u) - 1) + e_w (1 + r_c)(1 + 2u)), and the subtraction (fused or
     not) 2u (|out_i| + e_p).
No term of it is large: the median of bound / |out| stays below 2e-5 on every generated case, so all cases meet the 2e-3 tightness limit
and none needs an exception.  Domain: no zero-norm token row and no cls whose squared norm under- or overflows f32 (the generated norms
are 1e-3, 1 and 30); a zero row is 0 / 0 in the float64 reference as well, so there is nothing to compare there.  Negative zeros are not
generated either: at factor 0 the kernel computes x - (+-0), which returns every x bit for bit except -0.0 - (-0.0) = +0.0.

sg_adaptive_conv is held to  out[b,c,y,x] = sum_{i,j<d} in[b,c,y+i,x+j] filt[b,y,x,i,j]  in float64 with jbu_reference.conv_bound's 'valu'
form, 2u d^2 sum |in filt| plus the f32 store.
"""
from __future__ import annotations

import numpy as np
import torch

from jbu_reference import U, check_within, conv_bound, half_ulp, median_tightness  # noqa: F401
from rowops_reference import PATCH_MEAN, PATCH_STD, lane_sum

TIGHT_LIMIT = 2e-3                                 # the JBU module's f32 limit on median(bound / |ref|)
JBU_MEAN = (122.771, 116.746, 104.094)             # j_mean / j_std of csrc/jbu.hip (held in f32 there)
JBU_STD = (68.501, 66.632, 70.323)
MEAN32 = np.array(JBU_MEAN, dtype=np.float32)
STD32 = np.array(JBU_STD, dtype=np.float32)
assert JBU_MEAN == PATCH_MEAN and JBU_STD == PATCH_STD


# ---- extract: the quotient ---------------------------------------------------------------------------------------------------------------
def quotient_table():
    """Over every channel c and byte u: (plain [3, 256] float32 = (f32(u) - mean) / std in IEEE float32, exact [3, 256] float64 = the
    quotient of the same f32 constants in float64, err [3, 256] = |plain - exact| in ulps of f32 at exact)."""
    u = np.arange(256, dtype=np.float32)[None, :]
    plain = (u - MEAN32[:, None]) / STD32[:, None]
    assert plain.dtype == np.float32
    exact = (u.astype(np.float64) - MEAN32.astype(np.float64)[:, None]) / STD32.astype(np.float64)[:, None]
    ulp = 2 * half_ulp(torch.from_numpy(np.abs(exact)), "f32").numpy()
    return plain, exact, np.abs(plain.astype(np.float64) - exact) / ulp


def patchify_form_table():
    """patchify_kernel's u8 normalisation over every (c, u) in float32: the plain quotient, corrected by the subtraction's residual and the
    division's remainder where the subtraction rounded (csrc/patchify.hip)."""
    f = np.float32
    u = np.broadcast_to(np.arange(256, dtype=f)[None, :], (3, 256))
    m, s = MEAN32[:, None], STD32[:, None]
    d = (u - m).astype(f)
    e = ((u - d).astype(f) - m).astype(f)
    q = (d / s).astype(f)
    r = (d.astype(np.float64) - q.astype(np.float64) * s.astype(np.float64)).astype(f)              # fmaf(-q, std, d)
    return np.where(e != 0, (q + ((r + e).astype(f) / s).astype(f)).astype(f), q)


def exact_subtraction():
    """[3, 256] bool: the f32 subtraction f32(u) - mean is exact.  It is wherever |u - mean| < 128 (the difference then has the spacing of
    mean or a finer one), and beyond that where mean's last bit happens to be zero."""
    u = np.arange(256, dtype=np.float32)[None, :]
    d = u - MEAN32[:, None]
    return d.astype(np.float64) == u.astype(np.float64) - MEAN32.astype(np.float64)[:, None]


# ---- extract: cases ----------------------------------------------------------------------------------------------------------------------
SCENE_B, SCENE_H, SCENE_W = 3, 41, 67
TILES = {1: (17, 23), 3: (20, 31), 5: (19, 26)}    # n_tiles -> (tile_h, tile_w)
PADS = ((0, 0), (3, 5), (5, 0))                    # (pad_l, pad_t)
UPS = ("exact", "prod", "rows")
OUT_OF_ORDER = (2, 0, 2, 1, 0)


def make_scene(fmt, B=SCENE_B, H=SCENE_H, W=SCENE_W, seed=0):
    """f32 [B,3,H,W] normal deviates, or u8 [B,H,W,3]: a 16 x 16 ramp of every byte value tiled in, shifted per channel and per image, so
    that any window of 16 x 16 or more holds all of 0 .. 255 in every channel (the ramp repeats every 16 pixels; the f32 scenes, which go
    through the same window arithmetic, do not repeat)."""
    if fmt == "f32":
        return np.random.default_rng(9100 + seed).standard_normal((B, 3, H, W)).astype(np.float32)
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    return (((y % 16) * 16 + (x % 16) + 85 * c + 37 * b + seed) % 256).astype(np.uint8)


def _case(name, fmt, scene, windows, index, tile, pad, up):
    B, H, W = (scene.shape[0], scene.shape[2], scene.shape[3]) if fmt == "f32" else scene.shape[:3]
    return dict(name=name, fmt=fmt, scene=scene, scene_h=H, scene_w=W, scene_stride=3 * H * W,
                windows=np.asarray(windows, dtype=np.int32).reshape(-1, 4), scene_index=None if index is None else np.asarray(index, dtype=np.int32),
                n_tiles=len(windows), tile_h=tile[0], tile_w=tile[1], pad_l=pad[0], pad_t=pad[1], up_h=up[0], up_w=up[1])


def make_extract_case(fmt, T, pad, up, k=0):
    """T windows of TILES[T] rotating through: top-left corner, bottom-right corner, right border, bottom border, interior (k shifts the
    rotation, so that the single-tile cases do not all sit in the top-left corner).  up: 'exact' = tile + pad; 'prod' = the production
    shape tile + 2 pad (tile + (3, 2) where the pad is zero: larger in both directions either way); 'rows' = more rows only.
    Five tiles come from three scenes out of order with repeats (scene_index), fewer from scene 0 with scene_index NULL."""
    th, tw = TILES[T]
    pl, pt = pad
    H, W = SCENE_H, SCENE_W
    pos = [(0, 0), (H - th, W - tw), (3, W - tw), (H - th, 2), (5, 7)]
    win = [(y, y + th, x, x + tw) for y, x in (pos[(t + k) % 5] for t in range(T))]
    uh, uw = {"exact": (th + pt, tw + pl), "prod": (th + 2 * pt if pt else th + 3, tw + 2 * pl if pl else tw + 2), "rows": (th + pt + 4, tw + pl)}[up]
    return _case(f"{fmt}-T{T}-pad{pl}x{pt}-{up}", fmt, make_scene(fmt, seed=k), win, OUT_OF_ORDER if T == 5 else None, (th, tw), pad, (uh, uw))


def extract_cases():
    out, k = [], 0
    for fmt in ("f32", "u8"):
        for T in (1, 3, 5):
            for pad in PADS:
                for up in UPS:
                    out.append(make_extract_case(fmt, T, pad, up, k))
                    k += 1
        H, W = SCENE_H, SCENE_W
        # the ops.scene_planes form: one window equal to the whole scene
        out.append(_case(f"{fmt}-whole-scene", fmt, make_scene(fmt, B=1, seed=91), [(0, H, 0, W)], None, (H, W), (0, 0), (H, W)))
        # one output column: tile_w = up_w = 1, windows on the left border, the right border and inside
        out.append(_case(f"{fmt}-up_w-1", fmt, make_scene(fmt, seed=92), [(0, 9, 0, 1), (H - 9, H, W - 1, W), (7, 16, 30, 31)], [1, 2, 0], (9, 1), (0, 2),
                         (13, 1)))
    return out


EXTRACT_CASES = extract_cases()
EXTRACT_BY_NAME = {c["name"]: c for c in EXTRACT_CASES}


def normalised(scene_u8):
    """u8 [.., H, W, 3] -> (f32(u) - mean[c]) / std[c] in float32, same layout."""
    v = (scene_u8.astype(np.float32) - MEAN32) / STD32
    assert v.dtype == np.float32
    return v


def extract_reference(c):
    """float32 [T, 3, up_h, up_w] by plain indexing."""
    img = c["scene"] if c["fmt"] == "f32" else np.moveaxis(normalised(c["scene"]), -1, 1)
    out = np.zeros((c["n_tiles"], 3, c["up_h"], c["up_w"]), dtype=np.float32)
    th, tw, pl, pt = c["tile_h"], c["tile_w"], c["pad_l"], c["pad_t"]
    for t in range(c["n_tiles"]):
        y1, x1 = int(c["windows"][t, 0]), int(c["windows"][t, 2])
        b = 0 if c["scene_index"] is None else int(c["scene_index"][t])
        out[t, :, pt:pt + th, pl:pl + tw] = img[b, :, y1:y1 + th, x1:x1 + tw]
    return out


def extract_bytes(c):
    """int16 [T, 3, up_h, up_w]: the byte each cell of a u8 case was made from, -1 in the pads and the band."""
    assert c["fmt"] == "u8"
    out = np.full((c["n_tiles"], 3, c["up_h"], c["up_w"]), -1, dtype=np.int16)
    th, tw, pl, pt = c["tile_h"], c["tile_w"], c["pad_l"], c["pad_t"]
    for t in range(c["n_tiles"]):
        y1, x1 = int(c["windows"][t, 0]), int(c["windows"][t, 2])
        b = 0 if c["scene_index"] is None else int(c["scene_index"][t])
        out[t, :, pt:pt + th, pl:pl + tw] = np.moveaxis(c["scene"][b, y1:y1 + th, x1:x1 + tw], -1, 0)
    return out


EXTRACT_MUTANTS = ("pads_exchanged", "scene_index_ignored", "u8_as_nchw", "next_channel_constants", "band_not_zeroed", "x0_from_next_slot")


def extract_restated(c, mut=None):
    """extract_tiles_kernel's own index arithmetic over the flat scene, cell by cell (mut: one of EXTRACT_MUTANTS; a mutant's address is
    clipped into the scene buffer)."""
    T, uh, uw = c["n_tiles"], c["up_h"], c["up_w"]
    th, tw, pl, pt, H, W = c["tile_h"], c["tile_w"], c["pad_l"], c["pad_t"], c["scene_h"], c["scene_w"]
    if mut == "pads_exchanged":
        pl, pt = pt, pl
    per = 3 * uh * uw
    i = np.arange(per * T, dtype=np.int64)
    tile, rem = i // per, i % per
    ch, y, x = rem // (uh * uw), (rem // uw) % uh, rem % uw
    ty, tx = y - pt, x - pl
    inside = (ty >= 0) & (tx >= 0) if mut == "band_not_zeroed" else (ty >= 0) & (ty < th) & (tx >= 0) & (tx < tw)
    sy = c["windows"][tile, 0].astype(np.int64) + ty
    sx = c["windows"][tile, 3 if mut == "x0_from_next_slot" else 2].astype(np.int64) + tx
    off = 0 if (c["scene_index"] is None or mut == "scene_index_ignored") else c["scene_index"][tile].astype(np.int64) * c["scene_stride"]
    flat = c["scene"].reshape(-1)
    nchw = c["fmt"] == "f32" or mut == "u8_as_nchw"
    addr = off + ((ch * H + sy) * W + sx if nchw else (sy * W + sx) * 3 + ch)
    if mut is None:
        assert bool(((addr >= 0) & (addr < flat.size))[inside].all()), "a window leaves the scene"
    v = flat[np.clip(addr, 0, flat.size - 1)]
    if c["fmt"] == "u8":
        cm = (ch + 1) % 3 if mut == "next_channel_constants" else ch
        v = (v.astype(np.float32) - MEAN32[cm]) / STD32[cm]
    return np.where(inside, v, np.float32(0)).astype(np.float32).reshape(T, 3, uh, uw)


def same_bytes(a, b):
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def patches_to_planes(mat, T, gh, gw, P):
    """The inverse of the patch layout of rowops_reference.patchify_reference: [T gh gw, >= 3 P P] (column k = c P P + py P + px) ->
    planes [T, 3, gh P, gw P]."""
    m = mat[:, :3 * P * P].reshape(T, gh, gw, 3, P, P)
    return m.permute(0, 3, 1, 4, 2, 5).reshape(T, 3, gh * P, gw * P)


def patch_case_as_extract(pc):
    """A rowops_reference.make_patch_case (u8) as an extract case whose output is the whole patch grid."""
    s = pc["scene"].numpy()
    return _case("patch-case", "u8", s, pc["windows"].numpy(), pc["scene_index"].numpy(), (pc["tile_h"], pc["tile_w"]), (pc["pad_l"], pc["pad_t"]),
                 (pc["gh"] * pc["P"], pc["gw"] * pc["P"]))


# ---- global debias -----------------------------------------------------------------------------------------------------------------------
DEBIAS_E = (1, 2, 48, 63, 64, 65, 512, 640)
DEBIAS_N = (1, 3, 4, 5, 197)
DEBIAS_B = (1, 3)
DEBIAS_FACTORS = (0.2, -1.5, 0.0)
CLS_NORMS = (1e-3, 1.0, 30.0)


def make_debias_case(B, n, E, seed=0):
    """tokens [B, n, E], cls [B, E] float32.  Image b's cls has norm CLS_NORMS[(b + seed) % 3]; token rows are normal deviates scaled by
    10^[-2, 2].  Where n >= 4 the last three rows of every image are: parallel to cls (cos = 1), anti-parallel (cos = -1), and orthogonal by
    construction (x[2k] = cls[2k + 1], x[2k + 1] = -cls[2k]: the products cancel in pairs; an odd width ends in a triple that cancels to
    f32 rounding; E >= 2, otherwise a plain row).  No element is zero."""
    g = torch.Generator().manual_seed(7300 + 1000 * seed + 31 * E + n)
    cls = torch.randn(B, E, generator=g, dtype=torch.float64)
    cls = cls.sign() * cls.abs().clamp(min=0.05)                        # no element so small that a one-element cls loses its norm
    norms = torch.tensor([CLS_NORMS[(b + seed) % 3] for b in range(B)], dtype=torch.float64)
    cls = (cls / cls.norm(dim=-1, keepdim=True) * norms[:, None]).float()
    tok = torch.randn(B, n, E, generator=g, dtype=torch.float64)
    tok = tok.sign() * tok.abs().clamp(min=1e-3)
    tok = tok * 10.0 ** (torch.rand(B, n, 1, generator=g, dtype=torch.float64) * 4 - 2)
    if n >= 2:                                                           # the two ends of the range in every image
        tok[:, 0] *= 1e-2 / tok[:, 0].abs().max(-1, keepdim=True).values
        tok[:, 1] *= 1e2 / tok[:, 1].abs().max(-1, keepdim=True).values
    tok = tok.float()
    if n >= 4:
        chat = cls.double() / cls.double().norm(dim=-1, keepdim=True)
        tok[:, n - 3] = (3.7 * chat).float()
        tok[:, n - 2] = (-0.41 * chat).float()
        if E >= 2:
            o = torch.zeros(B, E)
            k = E // 2 * 2 if E % 2 == 0 else E - 3
            o[:, 0:k:2] = cls[:, 1:k:2]
            o[:, 1:k:2] = -cls[:, 0:k:2]
            if E % 2:                                                    # the odd width's last three: (c, c, -(a + b)) against (a, b, c)
                a, b_, c_ = cls[:, E - 3].double(), cls[:, E - 2].double(), cls[:, E - 1].double()
                o[:, E - 3], o[:, E - 2], o[:, E - 1] = c_.float(), c_.float(), (-(a + b_)).float()
            tok[:, n - 1] = o
    return tok.contiguous(), cls.contiguous()


def _comp(*r):
    p = 1.0
    for a in r:
        p = p * (1.0 + a)
    return p - 1.0


def _isqrt_rel(r):
    """|(1 +- r)^(-+1/2) - 1| for a relative error r under a square root (or its reciprocal)."""
    return (1.0 - r) ** -0.5 - 1.0


def debias_reference(tok, cls, factor, mut=None):
    """(out [B, n, E] float64, bound) of sg_global_debias on the f32 inputs; the docstring of this module derives the bound.
    mut ('cls_not_normalised', 'factor_dropped', 'token_norm_omitted'): the exact value of that fault, for the CPU module."""
    x, c0 = tok.double(), cls.double()
    f = float(np.float32(factor))
    E = x.shape[-1]
    g = 2 * U * (-(-E // 64) + 7)
    cn = c0.norm(dim=-1, keepdim=True)
    c = (c0 if mut == "cls_not_normalised" else c0 / cn)[:, None, :]     # [B, 1, E]
    xn = x.norm(dim=-1, keepdim=True)
    den = xn * c.norm(dim=-1, keepdim=True)
    if mut == "token_norm_omitted":
        den = c.norm(dim=-1, keepdim=True).expand_as(xn)
    q = (x * c).sum(-1, keepdim=True) / den
    w = q * (1.0 if mut == "factor_dropped" else f)
    out = x - c * w
    # the bound, in the kernel's order
    r_s = _comp(_isqrt_rel(g), 4 * U, 4 * U)
    r_c = _comp(r_s, 2 * U)
    r_cc = _comp(r_c, r_c, g)
    e_fc = (r_c + g * (1 + r_c)) * (x * c).abs().sum(-1, keepdim=True)
    r_den = _comp(_isqrt_rel(g), 4 * U, _isqrt_rel(r_cc), 4 * U, 2 * U)
    r_inv = 1.0 / (1.0 - r_den) - 1.0
    e_q = q.abs() * r_inv + e_fc / den * (1 + r_inv)
    e_w = abs(f) * (e_q + (q.abs() + e_q) * _comp(2 * U, 2 * U))
    r_p = _comp(r_c, 2 * U)
    e_p = c.abs() * (w.abs() * r_p + e_w * (1 + r_p))
    return out, e_p + 2 * U * (out.abs() + e_p)


DEBIAS_MUTANTS = ("cls_not_normalised", "factor_dropped", "tail_lanes_dropped", "token_norm_omitted", "last_rows_unwritten")


def debias_restated(tok, cls, factor, mut=None):
    """global_debias_kernel in float32 in its own order: lane l adds elements l, l + 64, ..., the xor butterfly, one wave per row, four
    rows per block.  Rows nobody writes stay NaN."""
    f32 = torch.float32
    B, n, E = tok.shape
    fac = torch.tensor(1.0 if mut == "factor_dropped" else float(np.float32(factor)), dtype=f32)

    def wsum(v):
        if mut == "tail_lanes_dropped" and E > 64 and E % 64:           # the lanes idle in the last trip leave before the butterfly:
            v = v.clone()                                                # their partial sums of the earlier trips are lost
            v[..., torch.arange(E) % 64 >= E % 64] = 0
        return lane_sum(v)
    one = torch.tensor(1.0, dtype=f32)
    ci = one / torch.sqrt(wsum(cls * cls))                               # [B]
    if mut == "cls_not_normalised":
        ci = torch.ones_like(ci)
    c = (cls * ci[:, None])[:, None, :]                                  # [B, 1, E]
    ff, fc, cc = wsum(tok * tok), wsum(tok * c), wsum((c * c).expand_as(tok))
    den = torch.sqrt(cc) if mut == "token_norm_omitted" else torch.sqrt(ff) * torch.sqrt(cc)
    w = (fc / den) * fac
    out = tok - c * w[..., None]
    if mut == "last_rows_unwritten" and n % 4:
        out[:, n - n % 4:] = float("nan")
    return out


# ---- adaptive convolution ----------------------------------------------------------------------------------------------------------------
CONV_W = (1, 63, 64, 65, 130)
CONV_H = (1, 3, 4, 5, 9)
CONV_D = (1, 3, 7)
CONV_BC = ((1, 1), (2, 3), (1, 33))


def make_conv_case(B, C, h, w, d, seed=0, onehot=False):
    """input [B, C, h + d - 1, w + d - 1], filters [B, h, w, d, d] float32: normal deviates plus a ramp along x and a steeper one along y
    (neither symmetric in (y, x) nor in (i, j)).  onehot: every pixel's filter is 1 at a tap (i, j) of its own and 0 elsewhere."""
    g = torch.Generator().manual_seed(5100 + 977 * seed + 131 * h + 17 * w + d)
    hp, wp = h + d - 1, w + d - 1
    inp = torch.randn(B, C, hp, wp, generator=g) + 0.05 * torch.arange(wp) - 0.3 * torch.arange(hp)[:, None]
    if onehot:
        t = torch.randint(0, d * d, (B, h, w), generator=g)
        filt = torch.nn.functional.one_hot(t, d * d).float().view(B, h, w, d, d)
        return inp.float().contiguous(), filt.contiguous(), t
    filt = torch.softmax(torch.randn(B, h, w, d * d, generator=g) * 2, -1) + 0.02 * torch.randn(B, h, w, d * d, generator=g)
    filt = filt.view(B, h, w, d, d) * (1 + 0.1 * torch.arange(d) - 0.25 * torch.arange(d)[:, None])
    return inp.float().contiguous(), filt.float().contiguous()


CONV_MUTANTS = ("filter_transposed", "row_pitch_w", "filter_shared_across_y")


def adaptive_conv_reference(inp, filt, mut=None):
    """conv_bound's dict (out, M = sum |in filt|) in float64, [B, C, h, w] each; mut: the exact value of one of CONV_MUTANTS."""
    B, C = inp.shape[:2]
    _, h, w, d, _ = filt.shape
    x, k = inp.double(), filt.double()
    if mut == "filter_transposed":
        k = k.transpose(3, 4)
    if mut == "filter_shared_across_y":
        k = k[:, :1].expand_as(k)
    if mut == "row_pitch_w":                                             # the kernel's address with wp = w: ((bc hp + row) w + col)
        hp, wp = h + d - 1, w + d - 1
        addr = (torch.arange(B * C * hp)[:, None] * w + torch.arange(wp)[None]).reshape(-1)
        x = x.reshape(-1)[addr].view(B, C, hp, wp)
    out = torch.zeros(B, C, h, w, dtype=torch.float64)
    M = torch.zeros_like(out)
    for i in range(d):
        for j in range(d):
            p = x[:, :, i:i + h, j:j + w] * k[:, None, :, :, i, j]
            out += p
            M += p.abs()
    return dict(out=out, M=M)


def adaptive_conv_bound(ref, d):
    assert d % 2 == 1
    return conv_bound(ref, "valu", (d - 1) // 2, "f32")


def adaptive_conv_restated(inp, filt):
    """adaptive_conv_nchw_kernel in float32: taps in (i, j) order into one accumulator."""
    _, h, w, d, _ = filt.shape
    acc = torch.zeros(inp.shape[0], inp.shape[1], h, w, dtype=torch.float32)
    for i in range(d):
        for j in range(d):
            acc = acc + inp[:, :, i:i + h, j:j + w] * filt[:, None, :, :, i, j]
    return acc
