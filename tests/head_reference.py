"""float64 numpy reference of the segmentation tail: bilinear upsample of each tile's logits (torch's align_corners=False taps),
un-pad, overlap-add in raster order, count division, x logit_scale, softmax over queries, per-class maximum over synonyms, argmax
(lowest class index), prob_thd -> bg_idx.  Test infrastructure only; shared by the CPU and the GPU tests of the label head.

Also the acceptance rule those tests share.  A pixel COUNTS unless its float64 top-two class-probability gap, or |conf - prob_thd|, is
below G = 1e-3: the stitched logits carry a few f32 roundings of values below 1 (absolute error about 1e-6 at most), the scale of 50
turns that into about 5e-5 on the exponent, so probabilities are off by less than about 2e-4; G is that with a 5x margin.  On every
counted pixel the label must equal the reference's and conf must lie within G; at most CAP = 1 % of the pixels of a case may be left
uncounted (a Monte-Carlo run on independent pixels with the post-interpolation spread of the test inputs gave 0.04-0.12 % for the
label gap and up to 0.08 % for the threshold, Q = 7...257; tests/test_head_reference_cpu.py confirms it on the real reference).
"""
import numpy as np

G = 1e-3
CAP = 0.01


def taps(n_in: int, n_out: int) -> np.ndarray:
    """[n_out, n_in] interpolation matrix of F.interpolate(mode='bilinear', align_corners=False) along one axis, in float64
    (ATen area_pixel_compute_source_index: src = max(scale * (dst + 0.5) - 0.5, 0), taps floor(src) and the next, clamped)."""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    if n_in == n_out:
        m[np.arange(n_out), np.arange(n_out)] = 1.0
        return m
    scale = n_in / n_out
    src = np.maximum(scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0
    np.add.at(m, (np.arange(n_out), i0), 1.0 - l1)
    np.add.at(m, (np.arange(n_out), i1), l1)
    return m


def upsample(tile: np.ndarray, up_hw) -> np.ndarray:
    """[Q, gh, gw] -> [Q, up_h, up_w], float64."""
    wy, wx = taps(tile.shape[1], up_hw[0]), taps(tile.shape[2], up_hw[1])
    return np.einsum("yg,qgh,xh->qyx", wy, tile.astype(np.float64), wx, optimize=True)


def stitch(tile_logits: np.ndarray, windows, up_hw, pad_tl, canvas_hw) -> np.ndarray:
    """tile_logits [T,Q,gh,gw], windows [(y1,y2,x1,x2)] in raster order -> the count-normalised canvas [Q,H,W] in float64 (a window
    may reach outside the canvas rows, as the windows of a canvas band do)."""
    T, Q = tile_logits.shape[:2]
    H, W = canvas_hw
    acc = np.zeros((Q, H, W), dtype=np.float64)
    cnt = np.zeros((H, W), dtype=np.float64)
    for t, (y1, y2, x1, x2) in enumerate(np.asarray(windows).reshape(-1, 4).tolist()):
        up = upsample(tile_logits[t], up_hw)[:, pad_tl[0]:pad_tl[0] + (y2 - y1), pad_tl[1]:pad_tl[1] + (x2 - x1)]
        ya, yb, xa, xb = max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)
        if yb <= ya or xb <= xa:
            continue
        acc[:, ya:yb, xa:xb] += up[:, ya - y1:yb - y1, xa - x1:xb - x1]
        cnt[ya:yb, xa:xb] += 1.0
    return np.where(cnt > 0, acc / np.maximum(cnt, 1.0), 0.0)


def tail(canvas: np.ndarray, query_idx, K: int, logit_scale: float, prob_thd: float, bg_idx: int):
    """canvas [Q,H,W] -> dict(probs [K,H,W], labels int64 [H,W], conf [H,W], gap [H,W] = top-two class-probability gap), float64.
    K == Q means class(q) = q (the reference skips the synonym merge then)."""
    canvas = np.asarray(canvas, dtype=np.float64)
    Q = canvas.shape[0]
    v = canvas * float(logit_scale)
    e = np.exp(v - v.max(0, keepdims=True))
    p = e / e.sum(0, keepdims=True)
    qi = np.arange(Q) if K == Q else np.asarray(query_idx).reshape(-1)
    if K == Q:
        probs = p
    else:
        # (probabilities * one_hot).max over queries: the zeros of the other queries take part in the max
        probs = np.zeros((K,) + canvas.shape[1:])
        if len(set(qi.tolist())) == 1 and 0 <= qi[0] < K:
            probs[qi[0]] = -np.inf                                 # no other query contributes a zero to this class's max
        for q in range(Q):
            if 0 <= qi[q] < K:
                probs[qi[q]] = np.maximum(probs[qi[q]], p[q])
    labels = probs.argmax(0).astype(np.int64)                      # the first maximum: the lowest class index
    conf = probs.max(0)
    if K > 1:
        top2 = np.partition(probs, K - 2, axis=0)[K - 2:]
        gap = top2[1] - top2[0]
    else:
        gap = np.full(conf.shape, np.inf)
    labels = np.where(conf < prob_thd, bg_idx, labels)
    return dict(probs=probs, labels=labels, conf=conf, gap=gap)


def label_head(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, K, logit_scale, prob_thd, bg_idx):
    return tail(stitch(tile_logits, windows, up_hw, pad_tl, canvas_hw), query_idx, K, logit_scale, prob_thd, bg_idx)


def counted(ref: dict, prob_thd: float) -> np.ndarray:
    """Pixels on which a label is decided beyond f32 rounding (module docstring)."""
    return (ref["gap"] >= G) & (np.abs(ref["conf"] - prob_thd) >= G)


def check_labels(ref: dict, labels, conf, prob_thd: float, what: str = ""):
    """The acceptance rule: returns the uncounted fraction after asserting the cap, the labels and (when given) conf."""
    ok = counted(ref, prob_thd)
    frac = 1.0 - ok.mean()
    labels = np.asarray(labels).reshape(ref["labels"].shape)
    bad = int((labels[ok] != ref["labels"][ok]).sum())
    print(f"{what}: uncounted {100 * frac:.3f} %, label mismatches on counted pixels {bad}", end="")
    if conf is not None:
        dc = float(np.abs(np.asarray(conf, dtype=np.float64).reshape(ref["conf"].shape) - ref["conf"])[ok].max()) if ok.any() else 0.0
        print(f", max |conf - ref| {dc:.3e}", end="")
    print()
    assert frac <= CAP, f"{what}: {100 * frac:.2f} % of the pixels are within {G} of a tie or of the threshold"
    assert bad == 0, f"{what}: {bad} counted pixels differ from the float64 reference"
    if conf is not None:
        assert dc <= G, f"{what}: conf is off by {dc}"
    return frac


# ---- the shapes the GPU test runs (the CPU test confirms the cap on the same inputs) ------------------------------------------------
def slide_windows(H, W, stride, crop):
    hg = max(H - crop + stride - 1, 0) // stride + 1
    wg = max(W - crop + stride - 1, 0) // stride + 1
    out = []
    for hi in range(hg):
        for wi in range(wg):
            y2, x2 = min(hi * stride + crop, H), min(wi * stride + crop, W)
            out.append((max(y2 - crop, 0), y2, max(x2 - crop, 0), x2))
    return out


# name -> (H, W, stride, crop, (gh, gw), up_hw, pad_tl): canvases of about 70 x 90 whose last window is shifted back (counts 1, 2, 4);
# "dense" has more than 64 tiles over one block (the candidate list's fall-back)
GEOMETRIES = {
    "a": (70, 90, 28, 40, (3, 3), (42, 44), (1, 2)),
    "b": (66, 93, 30, 44, (5, 4), (48, 46), (2, 1)),
    "dense": (40, 70, 2, 32, (3, 4), (40, 40), (4, 4)),
}
QS = (1, 7, 8, 9, 64, 65, 130, 257)


def make_case(geom: str, Q: int, merge: bool, seed: int = 0):
    """-> dict(tile_logits f32 [T,Q,gh,gw] i.i.d. N(0, 0.3^2), windows, up_hw, pad_tl, hw, query_idx int32 [Q], K).  ``merge``: K about
    Q / 2 with shuffled (unsorted) query_idx, every class owning at least one query; otherwise K = Q."""
    H, W, stride, crop, grid, up_hw, pad_tl = GEOMETRIES[geom]
    rng = np.random.default_rng(1000 * seed + 7 * Q + len(geom))
    wins = slide_windows(H, W, stride, crop)
    tl = (0.3 * rng.standard_normal((len(wins), Q) + grid)).astype(np.float32)
    if merge and Q > 1:
        K = max(1, Q // 2)
        qi = np.concatenate([np.arange(K), rng.integers(0, K, Q - K)])
        rng.shuffle(qi)
    else:
        K, qi = Q, np.arange(Q)
    return dict(tile_logits=tl, windows=np.asarray(wins, dtype=np.int32), up_hw=up_hw, pad_tl=pad_tl, hw=(H, W),
                query_idx=qi.astype(np.int32), K=K)
