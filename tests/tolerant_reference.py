"""A plain numpy restatement of the tolerant-matching definition (include/segearth_hip.h, the comment block of sg_tolerant_accumulate),
written straight from it.  Two forms that share no step with the kernels' row-segment decomposition:

    contour(lab)                                             -> bool [H,W]: a 4-neighbour inside the image holds another value
    counts_literal(pred, gt, tol_sq, K, ...)                 -> int64 [4,K]: per class the OR of all shifts (dy,dx) with dy^2 + dx^2 <=
                                                                tol_sq of the zero-padded target set; for radii up to 12
    counts(pred, gt, tol_sq, K, ...)                         -> the same table for any radius: the exact squared distance to the nearest
                                                                target (nearest target of each COLUMN first, then the minimum over the
                                                                columns of dx^2 + that distance^2), compared with tol_sq
    counts_multi(pred, gt, tol_sqs, K, ...)                  -> {tol_sq: table}; the distances are computed once
    counts_batch(pairs, tol_sqs, K, ...)                     -> the sum over the images, one tolerance per image
    tolerance_sq(hw, ratio)                                  -> tol_sq from the image diagonal
    scores(counts)                                           -> (precision, recall, F) float64 [K], NaN where a denominator is 0
"""
import math

import numpy as np

from boundary_reference import K, SHAPES, WIDE_CASES, blocky, patterns, reduce_zero, truth_for, wide_patterns   # noqa: F401  (the input builders)

REGION, CONTOUR = "region", "contour"
FAR = 1 << 40                                                                  # "no target": above every squared distance of an image
TOL_SQS = [0, 1, 2, 9, 10, 25, 1600, 254 * 254]


def tolerance_sq(hw, ratio=0.0075):
    h, w = int(hw[0]), int(hw[1])
    r = max(1, int(math.ceil(float(ratio) * math.sqrt(h * h + w * w))))
    return r * r


def contour(lab):
    lab = np.asarray(lab).astype(np.int64)
    assert lab.ndim == 2
    out = np.zeros(lab.shape, dtype=bool)
    out[1:, :] |= lab[1:, :] != lab[:-1, :]
    out[:-1, :] |= lab[:-1, :] != lab[1:, :]
    out[:, 1:] |= lab[:, 1:] != lab[:, :-1]
    out[:, :-1] |= lab[:, :-1] != lab[:, 1:]
    return out


def _maps(pred, gt, reduce_zero_label, mode):
    pred = np.asarray(pred).astype(np.int64)
    gt = np.asarray(gt).astype(np.int64)
    assert pred.shape == gt.shape and pred.ndim == 2 and mode in (REGION, CONTOUR)
    if reduce_zero_label:
        gt = reduce_zero(gt)
    if mode == CONTOUR:
        mp, mg = contour(pred), contour(gt)                                    # an ignored truth value is a value like any other
    else:
        mp = mg = np.ones(pred.shape, dtype=bool)
    return pred, gt, mp, mg


def dilate_literal(target, tol_sq):
    """near(p) for every p: the OR of the zero-padded ``target`` shifted by every (dy,dx) with dy^2 + dx^2 <= tol_sq."""
    H, W = target.shape
    r = math.isqrt(tol_sq)
    pad = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    pad[r:r + H, r:r + W] = target
    out = np.zeros((H, W), dtype=bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy * dy + dx * dx <= tol_sq:
                out |= pad[r + dy:r + dy + H, r + dx:r + dx + W]
    return out


def counts_literal(pred, gt, tol_sq, K, ignore_index=255, reduce_zero_label=False, mode=REGION):
    assert 0 <= tol_sq <= 12 * 12 + 12, "the literal form loops over the whole disk: small radii only"
    pred, gt, mp, mg = _maps(pred, gt, reduce_zero_label, mode)
    counted = gt != ignore_index
    out = np.zeros((4, K), dtype=np.int64)
    for k in range(K):
        sp, sg = mp & (pred == k), mg & (gt == k)
        out[0, k] = np.count_nonzero(sp & counted)
        out[1, k] = np.count_nonzero(sp & counted & dilate_literal(sg, tol_sq))
        out[2, k] = np.count_nonzero(sg & counted)
        out[3, k] = np.count_nonzero(sg & counted & dilate_literal(sp, tol_sq))
    return out


def nearest_sq(target, rmax):
    """int64 [H,W]: the squared Euclidean distance to the nearest True pixel of ``target`` among those at most ``rmax`` columns away,
    FAR where there is none.  Column first: the vertical distance to the nearest target of each column, then the minimum over dx."""
    H, W = target.shape
    if not target.any():
        return np.full((H, W), FAR, dtype=np.int64)
    rows = np.arange(H, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(target, rows, -FAR), axis=0)
    dn = np.minimum.accumulate(np.where(target, rows, FAR)[::-1], axis=0)[::-1]
    vd = np.minimum(np.minimum(rows - up, dn - rows), 1 << 20)
    vd2 = vd * vd                                                              # 2^40 = FAR where the column holds no target
    best = vd2.copy()
    for dx in range(1, min(W - 1, rmax) + 1):
        if dx * dx >= best.max():
            break
        np.minimum(best[:, dx:], vd2[:, :-dx] + dx * dx, out=best[:, dx:])
        np.minimum(best[:, :-dx], vd2[:, dx:] + dx * dx, out=best[:, :-dx])
    return np.minimum(best, FAR)


def counts_multi(pred, gt, tol_sqs, K, ignore_index=255, reduce_zero_label=False, mode=REGION):
    tol_sqs = [int(t) for t in tol_sqs]
    assert all(t >= 0 for t in tol_sqs)
    pred, gt, mp, mg = _maps(pred, gt, reduce_zero_label, mode)
    counted = gt != ignore_index
    rmax = math.isqrt(max(tol_sqs))
    out = {t: np.zeros((4, K), dtype=np.int64) for t in tol_sqs}
    for k in range(K):
        sp, sg = mp & (pred == k), mg & (gt == k)
        src_p, src_g = sp & counted, sg & counted
        to_g = nearest_sq(sg, rmax) if src_p.any() else None
        to_p = nearest_sq(sp, rmax) if src_g.any() else None
        for t in tol_sqs:
            out[t][0, k] = np.count_nonzero(src_p)
            out[t][2, k] = np.count_nonzero(src_g)
            if to_g is not None:
                out[t][1, k] = np.count_nonzero(src_p & (to_g <= t))
            if to_p is not None:
                out[t][3, k] = np.count_nonzero(src_g & (to_p <= t))
    return out


def counts(pred, gt, tol_sq, K, ignore_index=255, reduce_zero_label=False, mode=REGION):
    return counts_multi(pred, gt, [tol_sq], K, ignore_index, reduce_zero_label, mode)[int(tol_sq)]


def counts_batch(pairs, tol_sqs, K, ignore_index=255, reduce_zero_label=False, mode=REGION):
    total = np.zeros((4, K), dtype=np.int64)
    for (p, g), t in zip(pairs, tol_sqs):
        total += counts(p, g, t, K, ignore_index, reduce_zero_label, mode)
    return total


def scores(table):
    a = np.asarray(table).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p, r = a[1] / a[0], a[3] / a[2]
        return p, r, 2 * p * r / (p + r)


# ---- inputs of the GPU tests beyond boundary_reference's ---------------------------------------------------------------------------------
CPU_MAPS = ("blocky", "blocky_fine", "checker", "corner", "vstripe_d+1")
PATTERN_D = 3                                                                 # the width boundary_reference.patterns builds its stripes from
WIDE_TOL = [(3, 600, 1), (11, 600, 25), (81, 2100, 1600), (3, 4100, 1), (7, 4100, 25)]     # (H, W, tol_sq): WIDE_CASES heights


def sparse_pair(H, W, pred_cols, gt_cols, rows=None):
    """Class 1 on single pixels over a background of class 0: the prediction holds it at ``pred_cols``, the truth at ``gt_cols``, in
    every row of ``rows`` (default: the middle row).  What matches is decided by single column distances."""
    rows = [H // 2] if rows is None else rows
    p, g = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    for y in rows:
        for c in pred_cols:
            if 0 <= c < W:
                p[y, c] = 1
        for c in gt_cols:
            if 0 <= c < W:
                g[y, c] = 1
    return p, g


def carry_pairs(H, W, tol_sq):
    """name -> (pred, truth): the nearest target of a source sits across an edge of the row pass (lanes of 8 columns, waves of 512,
    chunks of 2048), exactly r columns away (matched) and r + 1 away (not matched), to the left (through the carry of the previous chunk)
    and to the right (in the next chunk)."""
    r = math.isqrt(tol_sq)
    out = {}
    for e in (8, 64, 512, 1024, 2048, 4096):
        if e + r + 2 >= W or e - r - 2 < 0:
            continue
        # target left of the edge, source right of it (the source's nearest target comes through the carry) -- and the mirror image
        out[f"left_{e}_hit"] = sparse_pair(H, W, [e + r - 1], [e - 1])
        out[f"left_{e}_miss"] = sparse_pair(H, W, [e + r], [e - 1])
        out[f"right_{e}_hit"] = sparse_pair(H, W, [e - r], [e])
        out[f"right_{e}_miss"] = sparse_pair(H, W, [e - r - 1], [e])
    # one target in the first column, one in the last, sources everywhere between (class 1 sources at every 97th column)
    out["ends"] = sparse_pair(H, W, list(range(5, W, 97)), [0, W - 1])
    return out
