"""A plain numpy restatement of the Boundary IoU definition (include/segearth_hip.h, the comment block of sg_boundary_band), written
straight from it: a pixel is in the band iff one of the (2d+1)^2 shifted copies of the map, padded with a value no map holds, differs
from the map there.  Nothing is decomposed into rows and columns, so this reference and the kernels cannot share a mistake.

    band_padded(lab, d)                                      -> uint8 [H,W], 0 / 1: the literal form, all shifts of the padded map
    band(lab, d)                                             -> the same map; shifts only where the window stays inside the image
    boundary_areas(pred, gt, d, K, ignore_index, reduce_zero) -> int64 [3,K]: band intersection, prediction band, truth band
    boundary_areas_batch(pairs, ds, K, ...)                  -> the sum over the images
    width(hw, ratio)                                         -> d from the image diagonal
    biou(areas)                                              -> float64 [K], NaN where the denominator is 0
"""
import math

import numpy as np


def reduce_zero(label):
    """mmseg LoadAnnotations(reduce_zero_label=True): raw 0 -> 255, raw 255 stays 255, every other value -> value - 1."""
    label = np.asarray(label).astype(np.int64)
    return np.where((label == 0) | (label == 255), 255, label - 1)


def width(hw, ratio=0.02):
    h, w = int(hw[0]), int(hw[1])
    return max(1, int(round(float(ratio) * math.sqrt(h * h + w * w))))


def band_padded(lab, d):
    """The definition, literally: band(y,x) = 1 iff one of the (2d+1)^2 shifted copies of the map, padded with a value no map holds,
    differs from lab[y,x].  The padding is kept apart as an `inside` plane, so it equals no label whatever values the map holds.
    Cost H * W * (2d+1)^2: for small maps and widths (tests/test_boundary_reference_cpu.py holds ``band`` to it)."""
    lab = np.asarray(lab).astype(np.int64)
    assert lab.ndim == 2 and d >= 1
    H, W = lab.shape
    val = np.zeros((H + 2 * d, W + 2 * d), dtype=np.int64)
    inside = np.zeros((H + 2 * d, W + 2 * d), dtype=bool)
    val[d:d + H, d:d + W] = lab
    inside[d:d + H, d:d + W] = True
    out = np.zeros((H, W), dtype=bool)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            out |= ~inside[dy:dy + H, dx:dx + W] | (val[dy:dy + H, dx:dx + W] != lab)
    return out.astype(np.uint8)


def band(lab, d):
    """The same map with the two clauses of the definition taken apart, so that a width above the image costs nothing: a pixel whose
    window leaves the image (y < d, y >= H - d, x < d, x >= W - d) is in the band by the first clause; every other pixel is compared
    with all (2d+1)^2 shifted copies of the map, every one of which lies inside the image there.  Still no row / column decomposition."""
    lab = np.asarray(lab).astype(np.int64)
    assert lab.ndim == 2 and d >= 1
    H, W = lab.shape
    out = np.ones((H, W), dtype=bool)
    h, w = H - 2 * d, W - 2 * d
    if h > 0 and w > 0:
        centre = lab[d:d + h, d:d + w]
        differs = np.zeros((h, w), dtype=bool)
        for dy in range(2 * d + 1):
            for dx in range(2 * d + 1):
                differs |= lab[dy:dy + h, dx:dx + w] != centre
        out[d:d + h, d:d + w] = differs
    return out.astype(np.uint8)


def boundary_areas(pred, gt, d, K, ignore_index=255, reduce_zero_label=False):
    pred = np.asarray(pred).astype(np.int64)
    gt = np.asarray(gt).astype(np.int64)
    assert pred.shape == gt.shape and pred.ndim == 2
    if reduce_zero_label:
        gt = reduce_zero(gt)
    band_p, band_g = band(pred, d).astype(bool), band(gt, d).astype(bool)      # ignored truth stays in the map as a value of its own
    counted = gt != ignore_index
    areas = np.zeros((3, K), dtype=np.int64)
    for k in range(K):
        areas[0, k] = np.count_nonzero(counted & (pred == k) & (gt == k) & band_p & band_g)
        areas[1, k] = np.count_nonzero(counted & (pred == k) & band_p)
        areas[2, k] = np.count_nonzero(counted & (gt == k) & band_g)
    return areas


def boundary_areas_batch(pairs, ds, K, ignore_index=255, reduce_zero_label=False):
    total = np.zeros((3, K), dtype=np.int64)
    for (p, g), d in zip(pairs, ds):
        total += boundary_areas(p, g, d, K, ignore_index, reduce_zero_label)
    return total


def biou(areas):
    a = np.asarray(areas).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return a[0] / (a[1] + a[2] - a[0])


# ---- the inputs of tests/test_gpu_boundary.py ---------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (7, 1), (17, 64), (64, 65), (67, 131), (130, 257)]
WIDTHS = [1, 2, 5, 40, 300]
K = 5


def blocky(H, W, classes, cell, seed):
    """A random map of cell x cell blocks, shifted by a random phase so that block edges fall anywhere."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, classes, (H // cell + 2, W // cell + 2))
    oy, ox = (int(v) for v in rng.integers(0, cell, 2))
    return np.kron(coarse, np.ones((cell, cell), dtype=np.int64))[oy:oy + H, ox:ox + W].astype(np.int64)


def patterns(H, W, d):
    """name -> int64 [H,W]: a flat map; a checkerboard of 1-pixel cells; vertical and horizontal stripes of width exactly d, d + 1 and
    2d + 1 (the widths at which an off-by-one in either pass changes the answer; a 2d + 1 stripe keeps exactly one centre line out of
    the band); blocky random maps with K = 5; a map whose only foreign pixel sits in a corner."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = {"flat": np.full((H, W), 2, dtype=np.int64), "checker": ((yy + xx) & 1).astype(np.int64)}
    for name, w in (("d", d), ("d+1", d + 1), ("2d+1", 2 * d + 1)):
        out[f"vstripe_{name}"] = ((xx // w) % 3).astype(np.int64)
        out[f"hstripe_{name}"] = ((yy // w) % 3).astype(np.int64)
    out["blocky"] = blocky(H, W, K, max(2, min(2 * d + 2, 24)), 11 * H + W + d)
    out["blocky_fine"] = blocky(H, W, K, 3, 5 * H + W)
    corner = np.zeros((H, W), dtype=np.int64)
    corner[H - 1, W - 1] = 1
    out["corner"] = corner
    return out


def truth_for(pred, fmt, seed):
    """A truth for ``pred``: the same map moved by (2, -3) pixels (wrapped), with an ignored rectangle (255) that touches classes, a
    patch of raw zeros (ignored under reduce_zero_label) and, like the prediction's copy returned with it, values outside [0, K): u8 200
    and 254; int64 also -3 and 2^40.  -> (pred with out-of-range values, truth) as int64 / ``fmt`` arrays."""
    rng = np.random.default_rng(seed)
    H, W = pred.shape
    gt = np.roll(pred, (2, -3), axis=(0, 1)).astype(np.int64)
    p = pred.copy()
    if H * W > 1:
        gt[H // 3:H // 3 + max(1, H // 4), W // 4:W // 4 + max(1, W // 3)] = 255
        gt[(2 * H) // 3:, : max(1, W // 5)] = 0
        far = (-3, 1 << 40) if fmt == np.int64 else (200, 254)
        for m, vals in ((gt, far), (p, (-3, 1 << 40, K, 99))):
            for v in vals:
                y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
                m[y:y + 2, x:x + 3] = v
    return p, gt.astype(fmt)


# ---- wide rows: the row pass works in lanes of 8 columns, waves of 512 and chunks of 2048 columns with a carry from chunk to chunk -------
WIDE_CASES = [(3, 600, 1), (11, 600, 5), (3, 4100, 1), (5, 2100, 2), (81, 2100, 40), (7, 4100, 3)]        # (H, W, d), H >= 2d + 1
ROW_EDGES = (8, 64, 511, 512, 513, 1024, 1536, 2047, 2048, 2049, 2560, 4095, 4096, 4097)


def runs_map(H, W, breaks, classes=3):
    """Rows of runs: the label changes at every column of ``breaks`` (cyclic in ``classes``), the same in every row."""
    row = np.zeros(W, dtype=np.int64)
    for b in sorted(set(int(b) for b in breaks if 0 < b < W)):
        row[b:] += 1
    return np.repeat((row % classes)[None], H, axis=0)


def wide_patterns(H, W, d):
    """name -> int64 [H,W], H >= 2d + 1 so that the centre rows show what the row pass wrote.  Runs that begin or end exactly at, one
    before and one after every lane, wave and chunk edge; runs of exactly 2d and 2d + 1 columns that straddle an edge; a run that starts
    d columns before a chunk edge, so that the lane at x + d that settles its first columns sits in the next chunk and takes the run's
    start from the carry; one run across every chunk; random runs; and rows that differ from the others across a chunk edge."""
    assert H >= 2 * d + 1
    rng = np.random.default_rng(H * 7 + W + d)
    edges = [e for e in ROW_EDGES if e < W]
    out = {"one_run": np.full((H, W), 1, dtype=np.int64), "edges": runs_map(H, W, edges)}
    for k, width in (("2d", 2 * d), ("2d+1", 2 * d + 1), ("2d+2", 2 * d + 2)):
        br = []
        for e in edges:
            if e in (511, 512, 2047, 2048, 4095, 4096):                                       # the run [e - d, e - d + width) straddles e
                br += [e - d, e - d + width]
        out[f"straddle_{k}"] = runs_map(H, W, br)
    out["start_before_chunk"] = runs_map(H, W, [e - d for e in edges if e % 2048 == 0] + [e - 2 * d - 1 for e in edges if e % 2048 == 0])
    out["far_start"] = runs_map(H, W, [3] + [W - 2])                                          # one run from column 3 across every chunk
    out["random_runs"] = runs_map(H, W, np.cumsum(rng.integers(1, 3 * (2 * d + 1), W // (2 * d + 1) + 8)), classes=K)
    rows = runs_map(H, W, [e + 1 for e in edges])
    y = H // 2 + (1 if H > 2 * d + 1 else 0)
    for e in edges:
        if e % 512 == 0:
            rows[min(y, H - 1), max(0, e - 3):e + 4] = 4                                      # a row that differs across the edge
    out["rows_differ"] = rows
    return out
