"""A plain numpy restatement of the region table's definition (include/segearth_hip.h, the comment block of sg_regions), built on
``sieve_reference.regions`` (the root of every pixel, by a sequential scan over row runs: no tiles, no atomics):

    q(conf)                                                        -> int64: round-half-even of clamp(conf, 0, 1) * 2^24, NaN -> 0
    all_rows(lab, connectivity, conf)                              -> (rows int64 [R,12] of EVERY region of one image, root map)
    listed(rows, min_area, skip_label)                             -> the listed rows among them
    assemble([(listed rows, root map) per image], max_regions)     -> the call's table, counts and region_of
    table(maps, connectivity, min_area, skip_label, confs, max_regions)
                                                                   -> (rows int64 [min(total, max_regions),12], counts int64 [N+1],
                                                                       region_of: one int32 [H,W] per image)

The rows of an image come from np.unique over the root map (ascending roots), its areas from the unique counts, the box from
np.minimum.at / np.maximum.at, the sums from np.bincount (exact: every sum stays far below 2^53).

``mutant=`` one of MUTANTS restates the definition with one deliberate mistake; tests/test_regions_reference_cpu.py shows that the
inputs of the GPU test tell every mutant from the reference, so a kernel that makes one of these mistakes cannot pass there.
"""
import numpy as np

import sieve_reference as S

FIELDS = 12
IMAGE, ROOT, LABEL, AREA, Y0, X0, Y1, X1, SUM_Y, SUM_X, SCORE_Q = range(11)
MUTANTS = {
    "box_inclusive": "Y1 / X1 hold the last row / column instead of one past it",
    "order_by_label": "the rows of an image ordered by (label, root) instead of root",
    "min_area_gt": "a region of exactly min_area pixels not listed (> for >=)",
    "skip_listed": "regions labelled skip_label listed all the same",
    "conn8_as_4": "connectivity 8 treated as 4",
    "batch_connects": "the last pixel of an image and the first pixel of the next one in the flat buffer treated as neighbours",
    "q_truncates": "q truncates instead of rounding to nearest even",
    "sums_swapped": "SUM_Y and SUM_X swapped",
    "counts_capped": "counts capped at max_regions",
    "region_of_capped": "region_of shows -1 for rows at or beyond max_regions",
}


def q(conf, mutant=None):
    """f32 in, int64 out.  The product with 2^24 is exact (in f32 as in the f64 used here), so rounding it is the whole definition."""
    c = np.asarray(conf, dtype=np.float32).astype(np.float64)
    c = np.where(np.isnan(c), 0.0, np.clip(c, 0.0, 1.0)) * float(1 << 24)
    return (np.floor(c) if mutant == "q_truncates" else np.rint(c)).astype(np.int64)         # np.rint rounds half to even


def all_rows(lab, connectivity=4, conf=None, mutant=None, extra_area=None, root=None):
    """Every region of one image, listed or not, ascending root, IMAGE = 0 -> (rows [R,12], root map [H,W]).  ``extra_area``: {root:
    pixels} added to a region's area (the batch_connects mutant); ``root``: ``sieve_reference.regions(lab, connectivity)`` where the
    caller already holds it."""
    assert mutant is None or mutant in MUTANTS
    lab = np.asarray(lab, dtype=np.int64)
    assert lab.ndim == 2 and connectivity in (4, 8)
    H, W = lab.shape
    conn = 4 if mutant == "conn8_as_4" else connectivity
    if root is None or conn != connectivity:
        root = S.regions(lab, conn)
    roots, inv, area = np.unique(root.reshape(-1), return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    area = area.astype(np.int64)
    for r, a in (extra_area or {}).items():
        area[np.searchsorted(roots, r)] += a
    y, x = (v.reshape(-1) for v in np.mgrid[0:H, 0:W])
    n = roots.size
    rows = np.zeros((n, FIELDS), dtype=np.int64)
    rows[:, ROOT], rows[:, LABEL], rows[:, AREA] = roots, lab.reshape(-1)[roots], area
    y0, x0 = np.full(n, H, dtype=np.int64), np.full(n, W, dtype=np.int64)
    y1, x1 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    np.minimum.at(y0, inv, y); np.minimum.at(x0, inv, x)
    np.maximum.at(y1, inv, y); np.maximum.at(x1, inv, x)
    last = 0 if mutant == "box_inclusive" else 1
    rows[:, Y0], rows[:, X0], rows[:, Y1], rows[:, X1] = y0, x0, y1 + last, x1 + last
    sy = np.bincount(inv, weights=y, minlength=n).astype(np.int64)
    sx = np.bincount(inv, weights=x, minlength=n).astype(np.int64)
    rows[:, SUM_Y], rows[:, SUM_X] = (sx, sy) if mutant == "sums_swapped" else (sy, sx)
    if conf is not None:
        rows[:, SCORE_Q] = np.bincount(inv, weights=q(np.asarray(conf).reshape(-1), mutant), minlength=n).astype(np.int64)
    return rows, root


def listed(rows, min_area=1, skip_label=None, mutant=None):
    """The listed ones among ``all_rows``, in the table's order."""
    assert min_area >= 1
    keep = rows[:, AREA] > min_area if mutant == "min_area_gt" else rows[:, AREA] >= min_area
    if skip_label is not None and mutant != "skip_listed":
        keep = keep & (rows[:, LABEL] != skip_label)
    rows = rows[keep]
    if mutant == "order_by_label":
        rows = rows[np.lexsort((rows[:, ROOT], rows[:, LABEL]))]
    return rows


def assemble(images, max_regions=None, mutant=None):
    """``images``: per image (its listed rows, its root map) -> (rows [min(total, max_regions),12], counts [N+1], region_of per image);
    ``counts`` and ``region_of`` are uncapped."""
    out, counts, region_of, r0 = [], [], [], 0
    for n, (rows, root) in enumerate(images):
        rows = rows.copy()
        rows[:, IMAGE] = n
        row_of_root = np.full(root.size, -1, dtype=np.int64)
        row_of_root[rows[:, ROOT]] = r0 + np.arange(len(rows))
        region_of.append(row_of_root[root].astype(np.int32))
        out.append(rows)
        counts.append(len(rows))
        r0 += len(rows)
    rows = np.concatenate(out)
    counts = np.array(counts + [r0], dtype=np.int64)
    if max_regions is not None:
        rows = rows[:max_regions]
        if mutant == "counts_capped":
            ends = np.minimum(np.cumsum(counts[:-1]), max_regions)
            counts = np.concatenate((np.diff(np.concatenate(([0], ends))), [min(r0, max_regions)])).astype(np.int64)
        if mutant == "region_of_capped":
            region_of = [np.where(v >= max_regions, -1, v).astype(np.int32) for v in region_of]
    return rows, counts, region_of


def table(maps, connectivity=4, min_area=1, skip_label=None, confs=None, max_regions=None, mutant=None, roots=None):
    """The call's table over the images ``maps`` in order -> (rows, counts, region_of) as ``assemble`` returns them.  ``roots``: the
    root maps where the caller holds them."""
    maps = [np.asarray(m, dtype=np.int64) for m in maps]
    roots = [S.regions(m, connectivity) for m in maps] if roots is None else roots
    extra = [dict() for _ in maps]
    if mutant == "batch_connects":                       # the two regions share one area, as indexing across the image boundary would give
        for n in range(len(maps) - 1):
            if maps[n].reshape(-1)[-1] == maps[n + 1].reshape(-1)[0]:
                ra, rb = int(roots[n].reshape(-1)[-1]), int(roots[n + 1].reshape(-1)[0])
                extra[n][ra] = int((roots[n + 1] == rb).sum())
                extra[n + 1][rb] = int((roots[n] == ra).sum())
    images = []
    for n, m in enumerate(maps):
        rows, root = all_rows(m, connectivity, None if confs is None else confs[n], mutant, extra[n], roots[n])
        images.append((listed(rows, min_area, skip_label, mutant), root))
    return assemble(images, max_regions, mutant)


# ---- the inputs of the GPU test (tests/test_gpu_regions.py) and of the power check (tests/test_regions_reference_cpu.py) ----------------
MIN_AREAS = (1, 5, 64)
SKIPS = (None, S.BG)
CAP_SHAPE = (130, 257)                                   # checkerboard: 33 410 regions, capped at 1, 1000 and total - 1


def tie_conf(H, W, seed=0):
    """f32 [H,W]: random values in [0, 1), with hand-placed values in the first pixels: (k + 0.5) * 2^-24 for even and odd k (ties: to
    even), the largest f32 below a tie and the smallest above it, above 1, below 0, -0.0, NaN, inf, and exactly 0 and 1."""
    rng = np.random.default_rng(seed + 7 * H + W)
    c = rng.random((H, W), dtype=np.float32)
    u = np.float32(2.0 ** -24)
    special = [np.float32(0.5) * u, np.float32(1.5) * u, np.float32(2.5) * u, np.float32(1001.5) * u, np.float32(1002.5) * u,
               np.nextafter(np.float32(6.5) * u, np.float32(0)), np.nextafter(np.float32(6.5) * u, np.float32(1)),
               np.float32(1.25), np.float32(-0.75), np.float32(-0.0), np.float32("nan"), np.float32("inf"), np.float32(0), np.float32(1),
               np.float32(4097.5) * u, np.float32(4098.5) * u]
    flat = c.reshape(-1)
    k = min(len(special), flat.size)
    flat[:k] = special[:k]
    return c


def seventy_tiny():
    """70 tiny images (more than SG_SIEVE_GROUP = 64): the row offset crosses launch sequences."""
    rng = np.random.default_rng(11)
    return [rng.integers(0, 3, (int(rng.integers(1, 6)), int(rng.integers(1, 9)))).astype(np.int64) + 1 for _ in range(70)]


def coarse_blocks(H, W, bh=32, bw=64, seed=3):
    """Blocks of bh x bw pixels of four labels: few runs per row, so the reference stays fast on a large map."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(rng.integers(0, 4, (H // bh + 1, W // bw + 1))[y // bh, x // bw].astype(np.int64))


def gpu_cases():
    """Every input of the GPU test: (what, maps, connectivity, confs or None, [(min_area, skip_label, max_regions or None), ...])."""
    every = [(a, s, None) for a in MIN_AREAS for s in SKIPS]
    cb = S.patterns(*CAP_SHAPE)["checkerboard"]
    total = cb.size                                                           # connectivity 4: every pixel is a region
    yield "capped", [cb], 4, [tie_conf(*CAP_SHAPE)], [(1, None, 1), (1, None, 1000), (1, None, total - 1)]
    for conn in (4, 8):
        maps = S.batch_maps()
        yield "batch", maps, conn, [tie_conf(*m.shape, seed=n) for n, m in enumerate(maps)], every + [(2, None, 40), (1, S.BG, 7)]
    yield "seventy", seventy_tiny(), 4, None, [(1, None, None), (2, 1, None), (1, None, 100)]
    for H, W in S.SHAPES:
        for conn in (4, 8):
            for name, m in S.patterns(H, W).items():
                yield (H, W, name), [m], conn, [tie_conf(H, W)], every
