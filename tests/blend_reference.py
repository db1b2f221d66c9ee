"""float64 numpy reference of the weighted window blend (sg_stitch_blend, include/segearth_hip.h), its per-element bound, an f32
emulation of the kernel's order and the slips the bound has to catch.  Test infrastructure only; shared by the CPU and the GPU tests.

The ramp is an f32 table r[0 .. L-1].  A tile t = (y1, y2, x1, x2) that covers pixel (y, x) enters with the weight
    w_t = fl32(r[min(dy, L-1)] * r[min(dx, L-1)]),  dy = min(y - y1, y2 - 1 - y),  dx = min(x - x1, x2 - 1 - x)
(distances in the window's own coordinates) and canvas = sum_t w_t u_t / sum_t w_t over the covering tiles in raster order, 0 where no
tile covers; u_t is head_reference.stitch's bilinear value.  The reference takes the f32-rounded product for w_t, so the reference and the
kernel use the same weights and the bound has nothing to budget for them.
"""
import numpy as np

import head_reference as HR
from head_reference import F32_TINY, SLACK, U

KINDS = ("linear", "hann")


def ramp(kind: str, R: int) -> np.ndarray:
    """f32 [R + 1]: r[d] = (d + 0.5) / R ("linear") or sin^2(pi/2 (d + 0.5) / R) ("hann") for d < R, r[R] = 1; float64 rounded once."""
    assert kind in KINDS and R >= 1
    v = (np.arange(R, dtype=np.float64) + 0.5) / R
    if kind == "hann":
        v = np.sin(0.5 * np.pi * v) ** 2
    return np.concatenate([v, [1.0]]).astype(np.float32)


UNIFORM = np.ones(1, dtype=np.float32)


def _dist(lo, hi, n, mut):
    """For canvas coordinates 0 .. n-1 of an axis and a window [lo, hi): (a, b, d) = the covered range [a, b) and the distance of each of
    its coordinates to the window's nearer edge."""
    a, b = max(lo, 0), min(hi, n)
    c = np.arange(a, b)
    if mut == "start_only":
        return a, b, c - lo
    if mut == "canvas_coords":                                            # the window clipped to the canvas first: wrong on a band
        return a, b, np.minimum(c - a, b - 1 - c)
    return a, b, np.minimum(c - lo, hi - 1 - c)


def _weights(win, hw, r, mut=None):
    """-> (ya, yb, xa, xb, w f32 [yb - ya, xb - xa]) of one window over a canvas of ``hw``; None when it covers nothing."""
    y1, y2, x1, x2 = win
    ya, yb, dy = _dist(y1, y2, hw[0], mut)
    xa, xb, dx = _dist(x1, x2, hw[1], mut)
    if yb <= ya or xb <= xa:
        return None
    L = len(r)
    if mut == "no_clamp":                                                 # a read past the table: whatever lies there, zeros here
        r = np.concatenate([r, np.zeros(max(int(dy.max()), int(dx.max())) + 1, dtype=np.float32)])
    else:
        dy, dx = np.minimum(dy, L - 1), np.minimum(dx, L - 1)
    return ya, yb, xa, xb, r[dy][:, None] * r[dx][None, :]               # the f32 product


def upsampled(tile_logits, up_hw):
    """Per tile (u, e, m): the float64 upsample [Q,up_h,up_w], its tap-weight term and its magnitude (head_reference).  They do not depend
    on the ramp: a test that runs one case under several ramps computes them once and hands them to the two functions below."""
    tl = np.asarray(tile_logits, dtype=np.float64)
    return [(HR.upsample(t, up_hw),) + HR._upsample_bound_parts(t, up_hw) for t in tl]


def stitch_blend(tile_logits, windows, up_hw, pad_tl, canvas_hw, r, ups=None) -> np.ndarray:
    """tile_logits [T,Q,gh,gw], windows [(y1,y2,x1,x2)] in raster order, r the f32 ramp -> the blended canvas [Q,H,W] in float64 (a
    window may reach outside the canvas rows, as the windows of a canvas band do).  ``ups``: ``upsampled`` of these tiles."""
    r = np.asarray(r, dtype=np.float32)
    Q = tile_logits.shape[1]
    H, W = canvas_hw
    acc, wsum = np.zeros((Q, H, W)), np.zeros((H, W))
    for t, win in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
        cov = _weights(win, canvas_hw, r)
        if cov is None:
            continue
        ya, yb, xa, xb, w = cov
        y1, _, x1, _ = win
        up = ups[t][0] if ups is not None else HR.upsample(tile_logits[t], up_hw)
        acc[:, ya:yb, xa:xb] += w.astype(np.float64) * up[:, pad_tl[0] + ya - y1:pad_tl[0] + yb - y1, pad_tl[1] + xa - x1:pad_tl[1] + xb - x1]
        wsum[ya:yb, xa:xb] += w
    return np.where(wsum > 0, acc / np.where(wsum > 0, wsum, 1.0), 0.0)


def weight_sum(windows, canvas_hw, r) -> np.ndarray:
    """sum_t w_t [H,W] in float64 (the partition-of-unity check)."""
    wsum = np.zeros(canvas_hw)
    for win in np.asarray(windows).reshape(-1, 4).tolist():
        cov = _weights(win, canvas_hw, np.asarray(r, dtype=np.float32))
        if cov is not None:
            ya, yb, xa, xb, w = cov
            wsum[ya:yb, xa:xb] += w
    return wsum


def stitch_blend_bound(tile_logits, windows, up_hw, pad_tl, canvas_hw, r, ups=None) -> np.ndarray:
    """bound [Q,H,W] on |sg_stitch_blend - stitch_blend(...)|, from operand magnitudes the way head_reference.stitch_bound is built.
    With e_t, m_t the tap-weight term and the magnitude of tile t's upsample (head_reference._upsample_bound_parts), n the number of
    covering tiles and wsum = sum w_t:
      * a tile's value is off by e_t + 4 u m_t (4 roundings on the longest path of its 4 products and 3 adds) and enters through
        w_t / wsum;
      * w u: one rounding, u w_t m_t (the kernel fuses it into the add; an unfused product has it);
      * the accumulation of n terms: n u on sum w_t m_t; the same n additions on wsum: n u relatively, on a quotient of at most
        sum w_t m_t / wsum;
      * the division: u on that quotient; one spare.
    Together (sum w_t e_t + (2 n + 7) u sum w_t m_t) / wsum, x SLACK + F32_TINY."""
    tl = np.asarray(tile_logits, dtype=np.float64)
    r = np.asarray(r, dtype=np.float32)
    Q = tl.shape[1]
    H, W = canvas_hw
    es, ms, wsum, n = np.zeros((Q, H, W)), np.zeros((Q, H, W)), np.zeros((H, W)), np.zeros((H, W))
    for t, win in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
        cov = _weights(win, canvas_hw, r)
        if cov is None:
            continue
        ya, yb, xa, xb, w = cov
        y1, _, x1, _ = win
        e, m = ups[t][1:] if ups is not None else HR._upsample_bound_parts(tl[t], up_hw)
        sl = (slice(None), slice(pad_tl[0] + ya - y1, pad_tl[0] + yb - y1), slice(pad_tl[1] + xa - x1, pad_tl[1] + xb - x1))
        w = w.astype(np.float64)
        es[:, ya:yb, xa:xb] += w * e[sl]
        ms[:, ya:yb, xa:xb] += w * m[sl]
        wsum[ya:yb, xa:xb] += w
        n[ya:yb, xa:xb] += 1.0
    return (es + (2 * n + 7) * U * ms) / np.where(wsum > 0, wsum, 1.0) * SLACK + F32_TINY


MUTANTS = ("start_only", "canvas_coords", "div_count", "no_clamp")


def stitch_blend_emulate(tile_logits, windows, up_hw, pad_tl, canvas_hw, r, mut=None) -> np.ndarray:
    """stitch_blend_kernel in f32: f32 taps and blend (head_reference.stitch_emulate's), acc = fma(w, u, acc) and wsum += w over the
    covering tiles in raster order, acc / wsum.  ``mut`` names one of MUTANTS:
      start_only     the distance from the window's start only (no min with the distance to its end);
      canvas_coords  distances in canvas rather than window coordinates: the window clipped to the canvas first (wrong on a band);
      div_count      division by the number of covering tiles instead of the sum of the weights;
      no_clamp       the table read at d instead of min(d, L - 1)."""
    f = np.float32
    tl = np.asarray(tile_logits, dtype=f)
    r = np.asarray(r, dtype=f)
    Q, gh, gw = tl.shape[1:]
    H, W = canvas_hw
    acc, wsum, cnt = np.zeros((Q, H, W), dtype=f), np.zeros((H, W), dtype=f), np.zeros((H, W), dtype=f)
    for t, win in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
        cov = _weights(win, canvas_hw, r, mut)
        if cov is None:
            continue
        ya, yb, xa, xb, w = cov
        y1, _, x1, _ = win
        ty = HR.tap_f32(np.arange(ya, yb) - y1 + pad_tl[0], gh, up_hw[0])
        tx = HR.tap_f32(np.arange(xa, xb) - x1 + pad_tl[1], gw, up_hw[1])
        u = HR._blend_f32(tl[t], ty, tx)
        # the fused multiply-add: the product of two f32 is exact in f64, the sum is rounded to f64 and then to f32
        acc[:, ya:yb, xa:xb] = (w.astype(np.float64) * u.astype(np.float64) + acc[:, ya:yb, xa:xb].astype(np.float64)).astype(f)
        wsum[ya:yb, xa:xb] += w
        cnt[ya:yb, xa:xb] += f(1)
    den = cnt if mut == "div_count" else wsum
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, acc / np.where(den > 0, den, f(1)), f(0))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def crop_of(name: str) -> int:
    """The smaller side of a geometry's windows (head_reference.stitch_geometry)."""
    w = HR.stitch_geometry(name)[0]
    return int(min((w[:, 1] - w[:, 0]).min(), (w[:, 3] - w[:, 2]).min()))


def stitch_ramps(name: str):
    """The ramps every stitch case runs with: "hann" over the full window, "linear" at R = 1 and R = 5 and "hann" at R = 3 (the clamp at
    L - 1 is exercised only by R < crop / 2)."""
    return [("hann", max(1, crop_of(name) // 2)), ("linear", 1), ("linear", 5), ("hann", 3)]


STITCH_Q = (1, 8, 9, 17)                                                  # a partial chunk, a full chunk, a chunk boundary, two chunks and one
STITCH_GEOMETRIES = ("a", "b", "dense", "w64", "w65", "hole", "1x1", "3x63")        # head_reference.STITCH_CASES' and HAND_STITCH's


def stitch_case(name: str, Q: int):
    """head_reference.make_stitch_case, 'plain' and 'offset' data alternating over the cases."""
    return HR.make_stitch_case(name, Q, ("plain", "offset")[(STITCH_GEOMETRIES.index(name) + STITCH_Q.index(Q)) % 2])


# label-head cases.  "dense" only at Q = 7 and 9: at Q = 64 and 130 the reference alone leaves 1.2 to 2.3 % of its pixels within G of a
# tie, above head_reference.CAP.
HEAD_GEOM_Q = [(g, Q) for g in ("a", "b") for Q in (7, 9, 64, 65, 130)] + [("dense", 7), ("dense", 9)]
HEAD_RAMPS = (("hann", None), ("linear", 5))                              # None: crop / 2


def head_cases(geom: str, Q: int):
    """(case of head_reference.make_head_case, merged, prob_thd, ramp spec) over merged x prob_thd x ramp; the sign of the plane offset
    (the online maximum moves in every chunk, or never) alternates."""
    out = []
    for i, (merged, thd, spec) in enumerate((m, t, s) for m in (False, True) for t in (0.0, 0.3) for s in HEAD_RAMPS):
        out.append((HR.make_head_case(geom, Q, (+1, -1)[(i + Q) % 2], merged), merged, thd, spec))
    return out


def head_ramp(geom: str, spec):
    kind, R = spec
    return ramp(kind, R if R is not None else max(1, HR.GEOMETRIES[geom][3] // 2))


def band_of(case, a: int, b: int):
    """Rows [a, b) of a stitch case as a canvas of its own: the windows that overlap it, shifted by -a -> (tile_logits, windows, (b - a, W))."""
    w = np.asarray(case["windows"]).reshape(-1, 4)
    keep = (w[:, 0] < b) & (w[:, 1] > a)
    wb = w[keep].copy()
    wb[:, 0:2] -= a
    return case["tile_logits"][keep], wb.astype(np.int32), (b - a, case["hw"][1])
