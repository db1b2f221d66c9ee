"""A plain numpy restatement of the min_region definition (include/segearth_hip.h, the comment block of sg_sieve), independent of the
kernels' algorithm: regions by a sequential raster scan over row runs with a union-find on the runs (no tiles, no atomics), areas by
bincount, the neighbour choice by sorting every adjacent (small pixel, kept pixel) pair.

    regions(lab, connectivity)                      -> root int64 [H,W]: the smallest raster index y*W + x of each pixel's region
    sieve(lab, min_region, connectivity, fill, bg)  -> the sieved map (a new array)
    sieve_batch(maps, ...)                          -> the same per image: images never connect

``mutant=`` one of MUTANTS restates the definition with one deliberate mistake; tests/test_sieve_reference_cpu.py shows that the
inputs of the GPU test tell every mutant from the reference, so a kernel that makes one of these mistakes cannot pass there.
"""
import functools

import numpy as np

FILLS = ("bg", "neighbour")
MUTANTS = {
    "conn8_as_4": "connectivity 8 treated as 4",
    "area_le": "a region of exactly min_region pixels counted as small (<= for <)",
    "tie_larger_root": "a tie on the neighbour's area resolved to the larger root",
    "bg_regions_sieved_in_bg_mode": "fill 'bg' also sieves small background regions (into their best kept neighbour)",
    "small_neighbour_wins": "a small adjacent region allowed to win the neighbour choice",
    "batch_connects": "the last pixel of an image and the first pixel of the next one in the flat buffer treated as neighbours",
}


def regions(lab, connectivity):
    """root int64 [H,W].  Row by row: the runs of equal labels, each united with the runs of the row above that it touches (sharing a
    column; with connectivity 8 also a corner) and that hold the same label.  Run ids grow in raster order of the runs' first pixels
    and a union keeps the smaller id, so a region's final id is its first run and its root that run's first pixel."""
    lab = np.asarray(lab)
    assert lab.ndim == 2 and connectivity in (4, 8)
    H, W = lab.shape
    d = 1 if connectivity == 8 else 0
    parent, first, length = [], [], []

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    prev = []
    for y in range(H):
        row = lab[y]
        cuts = (np.flatnonzero(row[1:] != row[:-1]) + 1).tolist()
        cur = []
        for s, e in zip([0] + cuts, cuts + [W]):
            i = len(parent)
            parent.append(i); first.append(y * W + s); length.append(e - s)
            cur.append((s, e, i, row[s]))
        j = 0
        for s, e, i, v in cur:
            while j < len(prev) and prev[j][1] + d <= s:                      # the run above ends before this one starts
                j += 1
            k = j
            while k < len(prev) and prev[k][0] < e + d:
                if prev[k][3] == v:
                    a, b = find(i), find(prev[k][2])
                    if a != b:
                        parent[max(a, b)] = min(a, b)
                k += 1
        prev = cur
    roots = np.array([first[find(i)] for i in range(len(parent))], dtype=np.int64)
    return np.repeat(roots, np.array(length, dtype=np.int64)).reshape(H, W)


@functools.lru_cache(maxsize=4)
def _pairs(H, W, connectivity):
    """Every ordered pair (pixel, neighbour) of raster indices under the connectivity."""
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    a, b = [], []
    for dy, dx in steps:
        p = idx[:H - dy, max(0, -dx):W - max(0, dx)].reshape(-1)
        q = idx[dy:, max(0, dx):W + min(0, dx)].reshape(-1)
        a += [p, q]; b += [q, p]
    return np.concatenate(a), np.concatenate(b)


def _sieve_roots(lab, root, area, min_region, connectivity, fill, bg_idx, mutant):
    """The fills, given every pixel's root and every root's area (area indexed by root)."""
    H, W = lab.shape
    flat, r = lab.reshape(-1), root.reshape(-1)
    small_root = area <= min_region if mutant == "area_le" else area < min_region          # meaningful at roots
    small = small_root[r]
    out = flat.copy()
    if fill == "bg" and mutant != "bg_regions_sieved_in_bg_mode":
        out[small & (flat != bg_idx)] = bg_idx
        return out.reshape(H, W)
    a, b = _pairs(H, W, connectivity)
    ok = small[a] & (r[a] != r[b])
    if mutant != "small_neighbour_wins":
        ok &= ~small[b]
    ra, rb = r[a[ok]], r[b[ok]]
    new_of_root = np.full(flat.size, bg_idx, dtype=np.int64)                 # a small region without a kept neighbour falls to bg_idx
    if ra.size:
        tie = -rb if mutant == "tie_larger_root" else rb
        order = np.lexsort((tie, -area[rb], ra))                             # by region; the largest area first; then the smaller root
        ra, rb = ra[order], rb[order]
        head = np.concatenate(([True], ra[1:] != ra[:-1]))
        new_of_root[ra[head]] = flat[rb[head]]
    if fill == "bg":                                                         # the mutant: only background regions take the neighbour fill
        roots = np.unique(r[small])
        new_of_root[roots[flat[roots] != bg_idx]] = bg_idx
    out[small] = new_of_root[r[small]]
    return out.reshape(H, W)


def sieve(lab, min_region, connectivity=4, fill="neighbour", bg_idx=0, mutant=None, root=None):
    """``root``: ``regions(lab, connectivity)`` where the caller already holds it (the same map under several settings)."""
    assert mutant is None or mutant in MUTANTS
    lab = np.asarray(lab, dtype=np.int64)
    assert lab.ndim == 2 and min_region >= 1 and connectivity in (4, 8) and fill in FILLS
    conn = 4 if mutant == "conn8_as_4" else connectivity
    if root is None or conn != connectivity:
        root = regions(lab, conn)
    area = np.bincount(root.reshape(-1), minlength=lab.size)
    return _sieve_roots(lab, root, area, min_region, conn, fill, bg_idx, mutant)


def sieve_batch(maps, min_region, connectivity=4, fill="neighbour", bg_idx=0, mutant=None):
    """Image by image.  The ``batch_connects`` mutant unites the region of an image's last pixel with the region of the next image's
    first pixel when their labels agree (what indexing the flat buffer across an image boundary would do): the two regions share one
    area, and adjacent pixels of either see the united region."""
    maps = [np.asarray(m, dtype=np.int64) for m in maps]
    if mutant != "batch_connects":
        return [sieve(m, min_region, connectivity, fill, bg_idx, mutant) for m in maps]
    roots = [regions(m, connectivity) for m in maps]
    areas = [np.bincount(r.reshape(-1), minlength=m.size) for r, m in zip(roots, maps)]
    for n in range(len(maps) - 1):
        if maps[n].reshape(-1)[-1] == maps[n + 1].reshape(-1)[0]:
            ra, rb = roots[n].reshape(-1)[-1], roots[n + 1].reshape(-1)[0]
            total = areas[n][ra] + areas[n + 1][rb]
            areas[n][ra] = areas[n + 1][rb] = total
    return [_sieve_roots(m, r, a, min_region, connectivity, fill, bg_idx, None) for m, r, a in zip(maps, roots, areas)]


# ---- the label maps of the GPU test (tests/test_gpu_sieve.py) and of the power check (tests/test_sieve_reference_cpu.py) ------------
SHAPES = [(1, 1), (1, 200), (200, 1), (5, 64), (4, 65), (33, 70), (67, 131), (130, 257)]       # the kernels' LDS tile is 64 x 16
MIN_REGIONS = (1, 2, 5, 64, None)                                                               # None: more than the pixel count
BG = 1


def _fit(a, H, W):
    return np.ascontiguousarray(a[:H, :W].astype(np.int64))


def patterns(H, W, seed=0):
    """name -> int64 [H,W].  Labels are small non-negative numbers except in 'iid7', which also holds negative and > 2^32 values."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    out = {}
    out["iid2"] = rng.integers(0, 2, (H, W))
    out["iid3"] = rng.integers(0, 3, (H, W))
    out["iid7"] = np.array([0, 1, 2, 3, -5, (1 << 40) + 3, 6], dtype=np.int64)[rng.integers(0, 7, (H, W))]
    out["blocky"] = rng.integers(0, 4, (H // 7 + 2, W // 9 + 2))[y // 7, x // 9]
    # a one-pixel-wide serpentine through the whole image: rows 0, 2, 4 ... full, joined at alternating ends
    s = np.zeros((H, W), dtype=np.int64)
    s[0::2] = 2
    s[1::4, W - 1:] = 2
    s[3::4, :1] = 2
    out["serpentine"] = s
    # a square spiral of width 1 with gaps of width 1
    sp = np.zeros((H, W), dtype=np.int64)
    ring = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    sp[ring % 2 == 0] = 3
    for k in range(0, min(H, W) // 2, 2):                                 # open each ring and bridge it to the next one
        if k + 1 < H and k < W:
            sp[k + 1, k] = 0
        if k + 1 < H and k + 1 < W:
            sp[k + 1, k + 1] = 3
    out["spiral"] = sp
    out["checkerboard"] = (y + x) % 2
    out["rings"] = (np.maximum(np.abs(y - H // 2), np.abs(x - W // 2)) // 3) % 3
    out["stripes"] = np.where((x + y) % 5 == 0, 2, np.where(x % 6 == 0, 3, np.where(y % 4 == 0, 4, 0)))
    # blobs of area exactly 4 and 5 (min_region 5: the first goes, the second stays) and 63 / 64, on a background of BG
    e = np.full((H, W), BG, dtype=np.int64)
    for y0, x0, n, v in ((1, 1, 4, 2), (1, 8, 5, 2), (3, 1, 63, 3), (3, 66, 64, 3), (20, 60, 63, 4), (40, 3, 64, 4)):
        if y0 < H:
            e[y0, x0:x0 + n] = v
    out["exact"] = e
    # a tie: one pixel whose only neighbours are two kept regions of equal area (the one with the smaller root must win), and one
    # between a smaller region on the left and a larger one on the right (the larger area must win, though its root is larger)
    t = np.full((H, W), BG, dtype=np.int64)
    if H >= 7 and W >= 21:
        for y0, left in ((0, 10), (4, 9)):
            t[y0:y0 + 3, 10 - left:10], t[y0:y0 + 3, 11:21] = 2, 3
            t[y0, 10], t[y0 + 1, 10], t[y0 + 2, 10] = 2, 5, 3
        # the second band: 28 pixels of 2 against 31 of 3
        t[3, :21] = 6
    elif W >= 5:
        t[0, 0:2], t[0, 2], t[0, 3:5] = 2, 5, 3
    elif H >= 5:
        t[0:2, 0], t[2, 0], t[3:5, 0] = 2, 5, 3
    out["tie"] = t
    # small regions that touch only other small regions: a mosaic of 1 x 2 dominoes of four labels, nothing kept for min_region > 2
    out["all_small"] = ((x // 2 + 2 * (y % 2)) % 4) + 2
    out["flat"] = np.full((H, W), 4, dtype=np.int64)
    return {k: _fit(np.asarray(v), H, W) for k, v in out.items()}


def min_region_of(m, H, W):
    return H * W + 3 if m is None else m


def batch_maps():
    """Three images of different sizes for one flat buffer: image n ends and image n + 1 begins with the same non-background label, in
    regions that are small alone and kept together (so a kernel that connects them shows)."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 3, (19, 70)).astype(np.int64) + 2
    b = rng.integers(0, 3, (33, 17)).astype(np.int64) + 2
    c = rng.integers(0, 3, (5, 130)).astype(np.int64) + 2
    a[-1, -3:], a[-2, -3:] = 9, BG
    b[0, :3], b[1, :3] = 9, BG
    b[-1, -3:], b[-2, -3:] = 8, BG
    c[0, :3], c[1, :3] = 8, BG
    return [a, b, c]
