"""float64 reference, f32 emulation and mutants of the test-time-augmentation merge (sg_tta_head, sg_tta_accumulate + sg_tta_finish).
Test infrastructure only; shared by tests/test_tta_reference_cpu.py and tests/test_gpu_tta.py.

The reference is mmseg's SegTTAModel over the reference's postprocess_result, built from head_reference and head_resized_reference:
per view head_reference.stitch -> head_reference.upsample to the output size -> mirrored along the width if the view is flipped ->
softmax and per-class maximum in float64 (head_reference.tail); then the mean of the views' class probabilities, the arg-max (lowest
class on a tie) and the threshold.

Views are topk_reference.case geometries "a" and "b" at the same (Q, merge): different canvases, windows and tile grids.  All views of
a case share ONE class map, geometry "a"'s (make_case draws it after the tile logits, so "b"'s differs).

Bound: P is the mean of the views' class probabilities, a convex combination, so its error is at most the mean of the per-view
head_reference.tail_bound fed head_resized_reference.canvas_bound (mirrored with its view).

Acceptance.  (1) P and conf per element within the bound above.  (2) On EVERY pixel the label is the first arg-max of the returned mean
planes with the threshold applied to their maximum, and conf is that maximum, exactly: together with (1) this pins every label up to
the bound, ties included.  (3) head_reference.check_labels (G = 1e-3, CAP = 1 %), verbatim wherever the float64 reference itself meets
its cap: every single-view case does (at most 0.14 % of the pixels within G of a tie).  A merge of several views does not, and no
rounding is involved: at the logit scale of 50 each view's softmax is close to one-hot, so wherever two views name different classes
the mean is two values near 1 / 2 whose order is decided by residuals of about 1e-3.  In the reference alone 4 to 11 % of the pixels
of the multi-view cases lie within G of such a tie (0.8 to 1.3 % at [a, a-flipped] with Q = 64; the one multi-view case below 1 % is
[a, b-flipped, a-flipped], Q = 5, merged); a smaller scale trades them for the flat ties of Q = 64 (5 to 20 % at scales 4 to 8), and
the per-element bounds (about 5e-4) give a band as wide as G.  The cap was derived for one softmax and no implementation can meet it
for a mean of them, so there check_labels' own assertions are kept on the pixels it counts (equal labels, conf within G), its cap is
printed instead of asserted, and (2) is what covers the remaining pixels.
"""
import functools

import numpy as np

import head_reference as HR
import head_resized_reference as RR
import topk_reference as TR

SCALE = TR.SCALE
THDS = RR.THDS
BG = RR.BG
QS = (5, 16, 17, 64)                                                      # below, at and above one chunk pair; both QMAX instantiations full
OUTS = RR.OUT_SIZES["a"]                                                  # upscale, downscale, mixed, identity of view "a"; no width is a multiple of 64
A, AF, B, BF = ("a", False), ("a", True), ("b", False), ("b", True)
VIEW_SETS = {"a": (A,), "a+af": (A, AF), "a+bf+af": (A, BF, AF), "eight": (A, AF, B, BF, AF, B, A, BF)}
# every view set with every Q and both class maps; the output size rotates so that each set and each Q meets all four sizes
CASES = [(s, Q, m, OUTS[(i + j + int(m)) % 4]) for i, s in enumerate(VIEW_SETS) for j, Q in enumerate(QS) for m in (False, True)]
MUTANTS = ("no_unflip", "mean_of_logits", "flip_rows", "divide_by_scales")


def case_id(vs, Q, merge, out):
    return f"{vs}-Q{Q}-{'merge' if merge else 'ident'}-{out[0]}x{out[1]}"


def class_map(Q: int, merge: bool):
    c = TR.case("a", Q, merge)
    return c["query_idx"], c["K"]


@functools.lru_cache(maxsize=8)
def view(geom: str, flip: bool, Q: int, merge: bool, out) -> dict:
    """One view at the output size: dict(probs [K,OH,OW] float64, bound [K,OH,OW]), mirrored when flipped; computed once, never modified."""
    qi, K = class_map(Q, merge)
    c = dict(TR.case(geom, Q, merge))
    c["out"] = tuple(out)
    c["resized"] = HR.upsample(c["canvas"], out)
    probs = HR.tail(c["resized"], qi, K, SCALE, 0.0, BG)["probs"]
    bound = HR.tail_bound(c["resized"], RR.canvas_bound(c), qi, K, SCALE)["probs"]
    if flip:
        probs, bound = probs[:, :, ::-1], bound[:, :, ::-1]
    return dict(probs=np.ascontiguousarray(probs), bound=np.ascontiguousarray(bound))


def finish(P, thd: float) -> dict:
    """The mean planes -> dict(probs, labels, conf, gap) in head_reference.tail's layout."""
    K = P.shape[0]
    labels = P.argmax(0).astype(np.int64)                                 # the first maximum: the lowest class
    conf = P.max(0)
    if K > 1:
        top2 = np.partition(P, K - 2, axis=0)[K - 2:]
        gap = top2[1] - top2[0]
    else:
        gap = np.full(conf.shape, np.inf)
    return dict(probs=P, labels=np.where(conf < thd, BG, labels), conf=conf, gap=gap)


@functools.lru_cache(maxsize=2)
def merged(vs: str, Q: int, merge: bool, out):
    """(P float64 [K,OH,OW], bound [K,OH,OW]) of a view set, summed in ascending view order."""
    views = VIEW_SETS[vs] if isinstance(vs, str) else vs                  # a name, or a tuple of (geometry, flipped)
    P = bound = 0.0
    for g, f in views:
        v = view(g, f, Q, merge, tuple(out))
        P, bound = P + v["probs"], bound + v["bound"]
    return P / len(views), bound / len(views)


def reference(vs, Q, merge, out, thd):
    """-> (ref dict of `finish`, dict(probs, conf) of bounds)."""
    P, bound = merged(vs, Q, merge, tuple(out))
    return finish(P, thd), dict(probs=bound, conf=bound.max(0))


def device_views(vs, Q, merge):
    """What ops.tta_head takes, as numpy: [(tile_logits, windows, up_hw, pad_tl, canvas_hw, flipped)]."""
    out = []
    for g, f in (VIEW_SETS[vs] if isinstance(vs, str) else vs):
        c = TR.case(g, Q, merge)
        out.append((c["tile_logits"], np.asarray(c["windows"], dtype=np.int32), c["up_hw"], c["pad_tl"], c["hw"], f))
    return out


def check(ref, bound, labels, conf, probs, thd, what):
    """The acceptance rule (module docstring, 'Acceptance').  Returns (share uncounted by G, worst probs err / bound, worst conf err /
    bound)."""
    labels = np.asarray(labels).reshape(ref["labels"].shape)
    conf32 = np.asarray(conf, dtype=np.float32).reshape(ref["conf"].shape)
    probs = np.asarray(probs, dtype=np.float32).reshape(ref["probs"].shape)
    rp = HR.within(probs, ref["probs"], bound["probs"], what + " probs")
    rc = HR.within(conf32, ref["conf"], bound["conf"], what + " conf")
    best = probs.max(0)
    assert best.tobytes() == conf32.tobytes(), f"{what}: conf is not the maximum of the mean planes"
    own = np.where(best < np.float32(thd), BG, probs.argmax(0))
    assert np.array_equal(labels, own), f"{what}: {int((labels != own).sum())} labels are not the first arg-max of the mean planes"
    ok = HR.counted(ref, thd)
    g_frac = float(1.0 - ok.mean())
    if g_frac <= HR.CAP:
        HR.check_labels(ref, labels, conf32, thd, what)                            # the existing rule, verbatim
    else:                                                                          # its label and conf assertions; its cap cannot hold
        bad = int((labels[ok] != ref["labels"][ok]).sum())
        dc = float(np.abs(conf32.astype(np.float64) - ref["conf"])[ok].max()) if ok.any() else 0.0
        print(f"{what}: {100 * g_frac:.2f} % within G of a tie in the float64 reference itself, label mismatches beyond G {bad}, "
              f"max |conf - ref| {dc:.3e}")
        assert bad == 0 and dc <= HR.G, f"{what}: {bad} pixels beyond G differ, conf off by {dc}"
    print(f"{what}: probs err / bound {rp:.3f}, conf err / bound {rc:.3f}")
    return g_frac, rp, rc


# ---- the kernel's arithmetic in f32 ---------------------------------------------------------------------------------------------------------
def _view_probs_f32(canvas, qi, K):
    """sg_tta_head's per-view statements on an f32 resized canvas [Q,OH,OW]: the online softmax in chunks of 8 queries, the largest
    scaled logit of every class, P_v[c] = exp(cmax - vmax) / sum, 0 for a class without a query."""
    f = np.float32
    v = np.asarray(canvas, dtype=f) * f(SCALE)
    Q, shp = v.shape[0], v.shape[1:]
    qi = np.arange(Q) if K == Q else np.asarray(qi).reshape(-1)
    vmax, s = np.full(shp, -np.inf, dtype=f), np.zeros(shp, dtype=f)
    cmax = np.full((K,) + shp, -np.inf, dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        for q0 in range(0, Q, 8):
            ch = v[q0:q0 + 8]
            cm = ch.max(0)
            mv = cm > vmax
            s = np.where(mv, s * np.exp(np.where(mv, vmax - cm, f(0))), s)
            vmax = np.where(mv, cm, vmax)
            for k in range(ch.shape[0]):
                s = s + np.exp(ch[k] - vmax)
                c = int(qi[q0 + k])
                if 0 <= c < K:
                    cmax[c] = np.maximum(cmax[c], ch[k])
        return np.where(np.isfinite(cmax), np.exp(np.where(np.isfinite(cmax), cmax, f(0)) - vmax) / s, f(0)).astype(f)


def emulate(vs, Q, merge, out, thd, mut=None):
    """-> (labels, conf f32, probs f32 [K,OH,OW]) as the kernel computes them.  mut: 'no_unflip' (a flipped view is read unmirrored),
    'mean_of_logits' (the views' resized logits are averaged before ONE softmax), 'flip_rows' (a flipped view is mirrored along the
    height), 'divide_by_scales' (the sum is divided by the number of scales -- half the views of a set with flips -- instead of V)."""
    f = np.float32
    qi, K = class_map(Q, merge)
    views = VIEW_SETS[vs]
    acc = None
    for g, flip in views:
        r = RR.emulate(g, Q, merge, tuple(out))
        x = r if mut == "mean_of_logits" else _view_probs_f32(r, qi, K)
        if flip and mut != "no_unflip":
            x = x[:, ::-1, :] if mut == "flip_rows" else x[:, :, ::-1]
        acc = x.astype(f) if acc is None else (acc + x).astype(f)
    n = len(views)
    if mut == "divide_by_scales" and any(fl for _, fl in views):          # scales x {unflipped, flipped}: half as many scales as views
        n = max(1, n // 2)
    P = (acc / f(n)).astype(f)
    if mut == "mean_of_logits":
        P = _view_probs_f32(P, qi, K)
    best = P.max(0)
    labels = np.where(best < f(thd), BG, P.argmax(0)).astype(np.int64)
    return labels, best, P
