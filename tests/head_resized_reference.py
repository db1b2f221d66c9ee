"""float64 reference, f32 emulation and mutants of the label / top-k heads at another ori_shape (sg_label_head_resized,
sg_topk_head_resized and their multi-image forms).  Test infrastructure only; shared by tests/test_head_resized_reference_cpu.py and
tests/test_gpu_head_resized.py.

The reference is the reference project's order of operations (segmentor.py:447-449, 475-489): head_reference.stitch (preds / count),
head_reference.upsample of that canvas to the output size (F.interpolate, bilinear, align_corners=False), then head_reference.tail or
topk_reference.rank.  The acceptance rules are the existing ones, unchanged: head_reference.check_labels (G, CAP) for the labels and
conf, topk_reference.check (GL, REL, CAP) for the slots.  Nothing in the resize changes their derivation: a bilinear blend is a convex
combination, so the resized canvas carries no more absolute error than the stitched one plus the blend's own few roundings.

Per element, conf and the slot probabilities are also held to head_reference.tail_bound, fed the canvas error
upsample(stitch_bound) + the bound of resize_reference: the stitch error of the four taps passes through the same convex combination
(so its bound is the interpolation of the bounds), and the blend adds what sg_resize_bilinear's bound budgets.
"""
import functools

import numpy as np

import head_reference as HR
import topk_reference as TR

SCALE = TR.SCALE
THDS = (0.0, 0.3)
BG = 0
# geometry -> output sizes: an upscale of about 2.3x (the 448 -> 1024 ratio), a downscale, one axis up and the other down, identity
OUT_SIZES = {"a": ((161, 207), (33, 41), (45, 170), (70, 90)), "b": ((151, 213), (29, 50), (100, 61), (66, 93))}
CASES = [(g, Q, m, o) for g in ("a", "b") for Q in HR.QS for m in (False, True) for o in OUT_SIZES[g]]
MUTANTS = ("align_corners", "swap_out_hw", "blend_before_div")


def case_id(geom, Q, merge, out):
    return f"{geom}-Q{Q}-{'merge' if merge else 'ident'}-{out[0]}x{out[1]}"


def is_upscale(hw, out):
    return out[0] >= hw[0] and out[1] >= hw[1]


@functools.lru_cache(maxsize=4)                                           # a Q = 257 case at 161 x 207 is 70 MB of float64
def resized(geom: str, Q: int, merge: bool, out) -> dict:
    """topk_reference.case plus the float64 canvas at `out`, its ranking and the canvas error bound; computed once, never modified."""
    c = dict(TR.case(geom, Q, merge))
    c["out"] = tuple(out)
    c["resized"] = HR.upsample(c["canvas"], out)
    c["ranked"] = TR.rank(c["resized"], c["query_idx"], c["K"], SCALE)
    return c


def canvas_bound(c: dict) -> np.ndarray:
    """bound [Q,OH,OW] on |device resized canvas - c['resized']| (module docstring)."""
    sb = HR.stitch_bound(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
    return HR.upsample(sb, c["out"]) + HR.resize_reference(c["canvas"], c["out"])[1]


def tail(c: dict, thd: float) -> dict:
    return HR.tail(c["resized"], c["query_idx"], c["K"], SCALE, thd, BG)


def reference_of(tile_logits, windows, up_hw, pad_tl, hw, out) -> np.ndarray:
    """The float64 resized canvas of inputs that are no `resized` case."""
    return HR.upsample(HR.stitch(tile_logits, windows, up_hw, pad_tl, hw), out)


def _counts(windows, hw):
    cnt = np.zeros(hw, dtype=np.float32)
    for y1, y2, x1, x2 in np.asarray(windows).reshape(-1, 4).tolist():
        cnt[max(y1, 0):min(y2, hw[0]), max(x1, 0):min(x2, hw[1])] += np.float32(1)
    return cnt


def _resize_f32(src, out, mut=None):
    """head_reference.resize_emulate with the resize mutants."""
    s = np.asarray(src, dtype=np.float32)
    h, w = s.shape[1:]
    if mut == "align_corners":
        ty, tx = HR.tap_f32(np.arange(out[0]), h, out[0], True), HR.tap_f32(np.arange(out[1]), w, out[1], True)
    elif mut == "swap_out_hw":                                             # the rows' scale from the output width and the other way round
        ty, tx = HR.tap_f32(np.arange(out[0]), h, out[1]), HR.tap_f32(np.arange(out[1]), w, out[0])
        ty = (np.minimum(ty[0], h - 1), np.minimum(ty[1], h - 1)) + ty[2:]
        tx = (np.minimum(tx[0], w - 1), np.minimum(tx[1], w - 1)) + tx[2:]
    else:
        return HR.resize_emulate(s, out)
    return HR._blend_f32(s, ty, tx)


@functools.lru_cache(maxsize=None)
def _stitched_f32(geom, Q, merge, div: bool):
    c = TR.case(geom, Q, merge)
    return HR.stitch_emulate(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"], None if div else "no_count_div")


def emulate(geom, Q, merge, out, mut=None) -> np.ndarray:
    """The kernels' arithmetic in f32 (every product rounded, as they are compiled): stitch_emulate, then resize_emulate.
    mut: 'align_corners' (the resize's taps), 'swap_out_hw' (its two scales exchanged), 'blend_before_div' (the sums and the counts are
    blended and then divided: wrong wherever neighbouring taps have different counts)."""
    if mut == "blend_before_div":
        c = TR.case(geom, Q, merge)
        sums = _resize_f32(_stitched_f32(geom, Q, merge, False), out)
        cnt = _resize_f32(_counts(c["windows"], c["hw"])[None], out)[0]
        return np.where(cnt > 0, sums / np.maximum(cnt, np.float32(1e-30)), np.float32(0))
    return _resize_f32(_stitched_f32(geom, Q, merge, True), out, mut)


def heads_of(canvas_f32, c: dict, thd: float, k: int):
    """What the two heads return for a device canvas: the tail and the ranking in float64 on the given f32 values."""
    t = HR.tail(canvas_f32, c["query_idx"], c["K"], SCALE, thd, BG)
    top = TR.topk(TR.rank(canvas_f32, c["query_idx"], c["K"], SCALE), k)
    return t["labels"], t["conf"], top["classes"], top["probs"]
