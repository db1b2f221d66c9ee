"""tests/regions_reference.py against hand-worked label maps whose answers are written out here, against an independent method
(scipy.ndimage.label per class, find_objects, ndimage.sum) on the maps of the GPU test, and against its own mutants: the inputs of
tests/test_gpu_regions.py tell every mutant from the reference."""
import numpy as np
import pytest

import regions_reference as G
import sieve_reference as S

_ROOTS = {}


def roots_of(what, maps, conn):
    key = (what, conn)
    if key not in _ROOTS:
        _ROOTS[key] = [S.regions(m, conn) for m in maps]
    return _ROOTS[key]


def test_q_rounds_half_to_even_and_clamps():
    u = 2.0 ** -24
    c = np.array([0.5 * u, 1.5 * u, 2.5 * u, 3.5 * u, 0.25 * u, 0.75 * u, 1.0, 1.5, -1.0, -0.0, np.nan, np.inf, -np.inf, 0.5], dtype=np.float32)
    assert G.q(c).tolist() == [0, 2, 2, 4, 0, 1, 1 << 24, 1 << 24, 0, 0, 0, 1 << 24, 0, 1 << 23]
    assert G.q(c, "q_truncates").tolist()[:6] == [0, 1, 2, 3, 0, 0]


def test_a_hand_worked_table():
    m = np.array([[2, 2, 0, 3],
                  [0, 2, 0, 3],
                  [3, 0, 2, 2]], dtype=np.int64)
    conf = np.full((3, 4), 0.5, dtype=np.float32)
    rows, counts, region_of = G.table([m], 4, 1, None, [conf])
    half = 1 << 23
    #            image root label area y0 x0 y1 x1 sum_y sum_x score_q 0
    assert rows.tolist() == [[0, 0, 2, 3, 0, 0, 2, 2, 1, 2, 3 * half, 0],
                             [0, 2, 0, 2, 0, 2, 2, 3, 1, 4, 2 * half, 0],
                             [0, 3, 3, 2, 0, 3, 2, 4, 1, 6, 2 * half, 0],
                             [0, 4, 0, 1, 1, 0, 2, 1, 1, 0, half, 0],
                             [0, 8, 3, 1, 2, 0, 3, 1, 2, 0, half, 0],
                             [0, 9, 0, 1, 2, 1, 3, 2, 2, 1, half, 0],
                             [0, 10, 2, 2, 2, 2, 3, 4, 4, 5, 2 * half, 0]]
    assert counts.tolist() == [7, 7]
    assert region_of[0].tolist() == [[0, 0, 1, 2], [3, 0, 1, 2], [4, 5, 6, 6]]
    # connectivity 8: the 2s join through (1,1)-(2,2), the 0s through (1,0)-(2,1) and (1,2)-(2,1)
    rows8, counts8, of8 = G.table([m], 8, 1, None, None)
    assert rows8[:, G.ROOT].tolist() == [0, 2, 3, 8] and rows8[:, G.AREA].tolist() == [5, 4, 2, 1] and rows8[:, G.SCORE_Q].tolist() == [0] * 4
    assert rows8[0].tolist() == [0, 0, 2, 5, 0, 0, 3, 4, 5, 7, 0, 0]
    assert of8[0].tolist() == [[0, 0, 1, 2], [1, 0, 1, 2], [3, 1, 0, 0]]
    # min_area and skip_label: listed rows renumber, the others show -1
    rows, counts, region_of = G.table([m], 4, 2, 0, None)
    assert rows[:, G.ROOT].tolist() == [0, 3, 10] and counts.tolist() == [3, 3]
    assert region_of[0].tolist() == [[0, 0, -1, 1], [-1, 0, -1, 1], [-1, -1, 2, 2]]
    # max_regions: the first rows only; counts and region_of stay
    rows, counts, region_of = G.table([m], 4, 1, None, None, max_regions=2)
    assert rows[:, G.ROOT].tolist() == [0, 2] and counts.tolist() == [7, 7] and region_of[0].max() == 6
    # two images never connect, and the rows run on
    rows, counts, region_of = G.table([m[:1], m[:1]], 4, 1, None, None)
    assert rows[:, G.IMAGE].tolist() == [0, 0, 0, 1, 1, 1] and counts.tolist() == [3, 3, 6] and region_of[1].tolist() == [[3, 3, 4, 5]]


def test_the_reference_agrees_with_scipy():
    """Independent method: ndimage.label per class (its labels grow in raster order of the regions' first pixels), find_objects for the
    boxes, ndimage.sum for the areas, the coordinate sums and the score.  Counts on every shape of the GPU test; roots, order and
    every column on the shapes small enough to compare row by row."""
    from scipy import ndimage
    for H, W in S.SHAPES:
        conf = G.tie_conf(H, W)
        qv = G.q(conf).astype(np.float64)
        y, x = np.mgrid[0:H, 0:W]
        for name, m in S.patterns(H, W).items():
            for conn, st in ((4, None), (8, np.ones((3, 3), dtype=int))):
                rows, _ = G.all_rows(m, conn, conf, root=roots_of((H, W, name), [m], conn)[0])
                found = []
                for v in np.unique(m):
                    lab, n = ndimage.label(m == v, structure=st)
                    if H * W > 70 * 33:
                        found += [None] * n
                        continue
                    idx = np.arange(1, n + 1)
                    area, sy, sx, sq = (ndimage.sum(w, lab, idx) for w in (np.ones_like(lab), y, x, qv))
                    first = ndimage.minimum(y * W + x, lab, idx)
                    for k, sl in enumerate(ndimage.find_objects(lab)):
                        found.append([0, int(first[k]), int(v), int(area[k]), sl[0].start, sl[1].start, sl[0].stop, sl[1].stop, int(sy[k]), int(sx[k]),
                                      int(sq[k]), 0])
                assert len(found) == len(rows), (H, W, name, conn)
                if found and found[0] is not None:
                    assert sorted(found, key=lambda r: r[1]) == rows.tolist(), (H, W, name, conn)
    m = S.patterns(130, 257)
    assert len(G.all_rows(m["flat"], 4)[0]) == 1 and len(G.all_rows(m["checkerboard"], 4)[0]) == 130 * 257


def _told_apart(want, got):
    return any(not np.array_equal(a, b) for a, b in zip([want[0], want[1]] + want[2], [got[0], got[1]] + got[2])) or want[0].shape != got[0].shape


@pytest.mark.parametrize("mutant", sorted(G.MUTANTS))
def test_gpu_inputs_tell_every_mutant_from_the_reference(mutant):
    for what, maps, conn, confs, options in G.gpu_cases():
        if (mutant == "conn8_as_4" and conn == 4) or (mutant == "batch_connects") != (what == "batch") or (mutant == "q_truncates" and confs is None):
            continue                                                           # the mutant restates the reference there
        if mutant in ("counts_capped", "region_of_capped") and all(mx is None for _, _, mx in options):
            continue
        roots = roots_of(what, maps, conn)
        for min_area, skip, mx in options:
            want = G.table(maps, conn, min_area, skip, confs, mx, roots=roots)
            got = G.table(maps, conn, min_area, skip, confs, mx, mutant=mutant, roots=roots)
            if _told_apart(want, got):
                print(f"{mutant}: first told apart by {what}, connectivity={conn}, min_area={min_area}, skip_label={skip}, max_regions={mx}")
                return
    pytest.fail(f"no input of the GPU test distinguishes the mutant '{mutant}' ({G.MUTANTS[mutant]})")


def test_the_exact_pattern_holds_regions_at_the_thresholds():
    rows, _ = G.all_rows(S.patterns(67, 131)["exact"], 4)
    areas = sorted(rows[:, G.AREA].tolist())
    assert {4, 5, 63, 64} <= set(areas)
    assert len(G.listed(rows, 5)) == len(rows) - 1 and len(G.listed(rows, 64, S.BG)) == areas.count(64)
