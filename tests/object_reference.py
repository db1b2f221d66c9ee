"""A brute-force restatement of the object match's definition (include/segearth_hip.h, the comment block of sg_object_match), in numpy and
``scipy.ndimage.label``: no union-find, no majority summary, no atomics.

    transform(g, rzl)                                              -> the truth after reduce_zero_label, int64
    objects(L, K, connectivity, min_area, skip_label, ignore)      -> (object index map int32 [H,W], -1: no object; classes, roots, areas)
    match(p, g, K, iou, ...)                                       -> (counts int64 [4,K], match_map uint8 [H,W], [(proot, groot), ...])
    match_batch(pairs, K, iou, ...)                                -> (counts, [match_map per image], [(image, proot, groot), ...])
    scores(counts)                                                 -> (precision, recall, F1, SQ, PQ), float64 [K] each

Every class of every map is labelled by itself, the FULL table of the intersections of predicted and true objects is built (np.unique over
the pairs of object indices), and the rule I * den > num * U is applied to every pair of one class with Python integers.

``mutant=`` one of MUTANTS restates the definition with one deliberate mistake; tests/test_object_reference_cpu.py shows that the inputs
of the GPU test tell every mutant from the reference, so a kernel that makes one of these mistakes cannot pass there.
"""
import numpy as np
from scipy import ndimage

MUTANTS = {
    "ge": ">= in place of >: a pair at exactly the threshold matches",
    "iou_over_p": "the IoU taken over |p| only (U = |p|)",
    "any_class": "the classes of the two objects not compared",
    "min_area_pred_only": "min_area applied to the prediction only",
    "ignore_is_object": "a region of ignored truth counted as an object",
    "greedy": "every predicted object, in root order, takes the first true object of its class it overlaps that is still free",
}
SQ_ONE = 1 << 24
_STRUCT = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}


def transform(g, rzl):
    g = np.asarray(g).astype(np.int64)
    return np.where((g == 0) | (g == 255), 255, g - 1) if rzl else g


def objects(L, K, connectivity=4, min_area=1, skip_label=None, ignore=None):
    """The objects of one map, ordered by (class, root)."""
    L = np.asarray(L, dtype=np.int64)
    assert L.ndim == 2 and connectivity in (4, 8) and min_area >= 1
    index = np.full(L.shape, -1, dtype=np.int32)
    classes, roots, areas = [], [], []
    for k in np.unique(L):
        k = int(k)
        if not 0 <= k < K or (skip_label is not None and k == skip_label) or (ignore is not None and k == ignore):
            continue
        comp, n = ndimage.label(L == k, structure=_STRUCT[connectivity])
        flat = comp.reshape(-1)
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        area = np.bincount(flat, minlength=n + 1)
        keep = np.flatnonzero(area[1:] >= min_area) + 1                              # ascending component number = ascending root
        order = keep[np.argsort(first[keep], kind="stable")]
        number = np.full(n + 1, -1, dtype=np.int32)
        number[order] = len(roots) + np.arange(order.size)
        index = np.where(comp > 0, number[comp], index)
        classes += [k] * order.size
        roots += [int(v) for v in first[order]]
        areas += [int(v) for v in area[order]]
    return index, classes, roots, areas


def match(p, g, K, iou=(1, 2), connectivity=4, min_area=1, skip_label=None, ignore_index=255, rzl=False, mutant=None):
    assert mutant is None or mutant in MUTANTS
    num, den = iou
    assert 1 <= num < den <= 1 << 20 and 2 * num >= den
    p = np.asarray(p, dtype=np.int64)
    g = transform(g, rzl)
    assert p.shape == g.shape and p.ndim == 2
    ip, cp, rp, ap = objects(p, K, connectivity, min_area, skip_label)
    ig, cg, rg, ag = objects(g, K, connectivity, 1 if mutant == "min_area_pred_only" else min_area, skip_label,
                             None if mutant == "ignore_is_object" else ignore_index)
    counts = [[0] * K for _ in range(4)]
    for k in cp:
        counts[1][k] += 1
    for k in cg:
        counts[2][k] += 1
    both = (ip >= 0) & (ig >= 0)
    code, inter = np.unique(ip[both].astype(np.int64) * max(len(rg), 1) + ig[both], return_counts=True)
    table = [(int(c) // max(len(rg), 1), int(c) % max(len(rg), 1), int(i)) for c, i in zip(code, inter)]     # every overlapping pair
    mp, mg, pairs = set(), set(), []
    if mutant == "greedy":
        table.sort(key=lambda t: (rp[t[0]], rg[t[1]]))
    for a, b, I in table:
        if cp[a] != cg[b] and mutant != "any_class":
            continue
        U = ap[a] if mutant == "iou_over_p" else ap[a] + ag[b] - I
        if mutant == "greedy":
            ok = a not in mp and b not in mg
        elif mutant == "ge":
            ok = I * den >= num * U
        else:
            ok = I * den > num * U
        if ok:
            counts[0][cp[a]] += 1
            counts[3][cp[a]] += (I * SQ_ONE) // U
            mp.add(a); mg.add(b); pairs.append((rp[a], rg[b]))
    mark_p = np.array([1 if a in mp else 2 for a in range(len(rp))] + [0], dtype=np.uint8)
    mark_g = np.array([4 if b in mg else 8 for b in range(len(rg))] + [0], dtype=np.uint8)
    mm = mark_p[ip] + mark_g[ig]                                                     # index -1: the trailing 0
    return np.array(counts, dtype=np.int64), mm.astype(np.uint8), sorted(pairs)


def match_batch(pairs, K, iou=(1, 2), **kw):
    counts, maps, matched = np.zeros((4, K), dtype=np.int64), [], []
    for n, (p, g) in enumerate(pairs):
        c, m, pr = match(p, g, K, iou, **kw)
        counts += c
        maps.append(m)
        matched += [(n, a, b) for a, b in pr]
    return counts, maps, matched


def scores(counts):
    tp, pred, true, q = (np.asarray(counts)[i].astype(np.float64) for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        rq, sq = 2 * tp / (pred + true), q / float(SQ_ONE) / tp
        return tp / pred, tp / true, rq, sq, sq * rq


# ---- the pattern makers and the inputs of the GPU test (tests/test_gpu_object.py) and of the power check -----------------------------
SHAPES = [(1, 1), (1, 7), (7, 1), (17, 64), (64, 65), (67, 131), (130, 257)]      # the labelling tile is 64 x 16
IOUS = ((1, 2), (3, 4), ((1 << 20) - 1, 1 << 20))
K = 5
BG = 0


def blocky(H, W, K, cell, seed):
    """Random blocks of cell x cell pixels with classes 0 .. K + 1: K and K + 1 lie outside [0, K)."""
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, K + 2, (H // cell + 1, W // cell + 1)), np.ones((cell, cell), dtype=np.int64))[:H, :W].astype(np.int64)


def speckled(H, W, K, seed):
    """Per-pixel noise on three classes: many regions of 1 to a few pixels, some of them equal in both maps."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, min(K, 3), (H, W)).astype(np.int64)


def truth_for(p, fmt, move=(1, 2), rzl=False):
    """A truth for the prediction ``p``: the map moved by ``move``, an ignored rectangle (255), a patch left exactly as the prediction;
    with ``rzl`` one class up, so that reduce_zero_label brings it back, and raw zeros in a corner."""
    H, W = p.shape
    g = np.roll(p, move, axis=(0, 1)).astype(np.int64)
    g[H // 2:H // 2 + H // 3 + 1, W // 3:W // 3 + W // 4 + 1] = p[H // 2:H // 2 + H // 3 + 1, W // 3:W // 3 + W // 4 + 1]
    if rzl:
        g = g + 1
        g[:max(H // 8, 0), :max(W // 8, 0)] = 0
    if H >= 7 and W >= 7:
        g[H // 5:H // 5 + 3, W // 2:W // 2 + 5] = 255
    return p, g.astype(fmt)


# hand-worked pairs on a background of class 0: name -> (prediction, truth, {iou: TP of class 1 (and 2)})
def hand_maps():
    out = {}

    def canvas(h=12, w=14):
        return np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    p, g = canvas()
    p[2:6, 2:6] = 1; g[2:6, 3:7] = 1                                                   # I = 12, U = 20: 0.6
    out["moved_by_a_column"] = (p, g, {(1, 2): 1, (3, 4): 0})
    p, g = canvas()
    p[2:4, 2:4] = 1; g[2:4, 2:6] = 1                                                   # I = 4, U = 8: exactly 1/2
    out["exactly_half"] = (p, g, {(1, 2): 0, (3, 4): 0})
    p, g = canvas()
    p[5, 1:12] = 1; g[2:9, 1:4] = 1; g[2:9, 5:8] = 1; g[2:9, 9:12] = 1                 # 3 + 3 + 3 of 11 pixels: no majority
    out["three_ways"] = (p, g, {(1, 2): 0, (3, 4): 0})
    p, g = canvas()
    p[4:7, 4:7] = 1; g[1:10, 1:10] = 1                                                 # I = 9 = |p|, U = 81
    out["majority_too_large"] = (p, g, {(1, 2): 0, (3, 4): 0})
    p, g = canvas()
    p[2:6, 2:4] = 1; p[2:6, 5:7] = 1; g[2:6, 2:7] = 1                                  # 8 of 20 each
    out["two_halves"] = (p, g, {(1, 2): 0, (3, 4): 0})
    p, g = canvas()
    p[2:6, 2:5] = 1; p[2:6, 6:7] = 1; g[2:6, 2:7] = 1                                  # 12 of 20 and 4 of 20
    out["large_and_small_part"] = (p, g, {(1, 2): 1, (3, 4): 0})
    p, g = canvas()
    p[2:6, 2:6] = 1; g[2:6, 2:6] = 2                                                   # the same square, another class
    out["other_class"] = (p, g, {(1, 2): 0, (3, 4): 0})
    p, g = canvas()
    p[2:6, 2:6] = 1; g[2:6, 2:6] = 1; p[8:10, 8:12] = 2; g[8:10, 8:11] = 2             # IoU 1 and 3/4 exactly
    out["equal_and_three_quarters"] = (p, g, {(1, 2): 2, (3, 4): 1})
    return out


def hand_embedded(H=67, W=131):
    """All hand-worked pairs on one canvas, each at a corner of the 64 x 16 labelling tiles so that its objects cross tile borders."""
    p, g = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    spots = [(12, 60), (28, 60), (44, 60), (12, 2), (28, 100), (44, 110), (12, 100), (28, 20)]      # (y + 4, x + 4) = (16 k, 64) for the first three
    want = {iou: 0 for iou in IOUS[:2]}
    for (y, x), (name, (hp, hg, tp)) in zip(spots, hand_maps().items()):
        h, w = hp.shape
        assert y + h <= H and x + w <= W and not p[y:y + h, x:x + w].any(), name
        p[y:y + h, x:x + w] = hp; g[y:y + h, x:x + w] = hg
        for iou in want:
            want[iou] += tp[iou]
    return p, g, want


def spanning():
    """300 x 300: ONE predicted object of class 1 that spans every tile (the whole map but its first row) against a truth with a hole in
    it: the counters pass 2^16 and one entry is hit from every workgroup."""
    p = np.ones((300, 300), dtype=np.int64)
    p[0, :] = 0
    g = np.ones((300, 300), dtype=np.int64)
    g[100:160, 120:200] = 0
    g[120:140, 150:170] = 1                                                         # an island in the hole: a second true object
    return p, g


def tiny65():
    rng = np.random.default_rng(65)
    out = []
    for _ in range(65):
        p = rng.integers(0, 3, (3, 5)).astype(np.int64)
        g = p.copy()
        g[rng.integers(0, 3), rng.integers(0, 5)] = rng.integers(0, 3)
        out.append((p, g.astype(np.uint8)))
    return out


def three_images():
    shapes, out = [(5, 7), (33, 70), (20, 13)], []
    for i, (H, W) in enumerate(shapes):
        p, g = truth_for(blocky(H, W, K, 4, 40 + i), np.uint8)
        p[-1, -1] = p[0, 0] = 2
        out.append((p, g))
    return out


def gpu_cases():
    """Every input of the GPU test: (what, [(p, g) per image], K, rzl, ignore_index, [(iou, connectivity, min_area, skip_label), ...])."""
    every = [(iou, c, a, s) for iou in IOUS for c in (4, 8) for a in (1, 5) for s in (None, BG)]
    few = [((1, 2), 4, 1, None), ((3, 4), 8, 5, BG), (IOUS[2], 8, 1, BG), ((1, 2), 8, 5, None)]
    for H, W in SHAPES:
        big = H * W > 64 * 65
        for name, m in (("blocky", blocky(H, W, K, 6, 31 * H + W)), ("speckled", speckled(H, W, K, H + W))):
            for fmt, rzl in ((np.uint8, False), (np.int64, True), (np.uint8, True), (np.int64, False)):
                if big and (fmt, rzl) in ((np.uint8, True), (np.int64, False)):
                    continue
                p, g = truth_for(m, fmt, rzl=rzl)
                yield (H, W, name, fmt.__name__, rzl), [(p, g)], K, rzl, 255, (few if big else every)
    p, g, _ = hand_embedded()
    yield "hand", [(p, g.astype(np.uint8))], 3, False, 255, [(iou, c, 1, s) for iou in IOUS for c in (4, 8) for s in (None, BG)]
    p, g = truth_for(blocky(40, 77, K, 6, 8), np.int64)
    g[20:30, 40:60] = (1 << 32) + 2                                                 # differs from class 2 only above bit 32
    g[22:28, 45:55] = 2
    yield "ignore_index_1", [(p, g)], K, False, 1, [((1, 2), 4, 1, None), ((3, 4), 8, 1, None), ((1, 2), 4, 5, BG)]
    for Kc in (1, 127):
        rng = np.random.default_rng(Kc)
        p = np.kron(rng.integers(0, Kc + 2, (17, 17)), np.ones((4, 4), dtype=np.int64))[:64, :65].astype(np.int64)
        g = np.roll(p, (0, 1), axis=(0, 1)).astype(np.uint8)
        g[5:15, 40:60] = 255
        yield ("K", Kc), [(p, g)], Kc, False, 255, [((1, 2), 4, 1, None), ((3, 4), 4, 1, None), ((1, 2), 8, 5, 0)]
    yield "spanning", [spanning()], 2, False, 255, [((1, 2), 4, 1, None), ((3, 4), 8, 1, BG), (IOUS[2], 4, 1, None)]
    flat = np.full((512, 512), 1, dtype=np.int64)
    yield "flat", [(flat, flat.astype(np.uint8))], 2, False, 255, [((1, 2), 4, 1, None), (IOUS[2], 8, 5, BG)]
    yield "three_images", three_images(), K, False, 255, few
    yield "tiny65", tiny65(), 3, False, 255, [((1, 2), 4, 1, None), ((3, 4), 8, 1, None), ((1, 2), 4, 2, BG)]
