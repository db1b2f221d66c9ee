"""tests/sieve_reference.py against hand-worked label maps whose answers are written out here, against scipy.ndimage.label where scipy
imports, and the power of the GPU test's inputs: every mutant of the reference differs from it on at least one of them."""
import numpy as np
import pytest

import sieve_reference as R


def A(rows):
    return np.array(rows, dtype=np.int64)


def test_regions_of_a_diagonal_under_both_connectivities():
    m = A([[1, 0, 0],
           [0, 1, 0],
           [0, 0, 1]])
    # 4: three single 1s; the zeros above and below the diagonal are two regions of three
    assert R.regions(m, 4).tolist() == [[0, 1, 1], [3, 4, 1], [3, 3, 8]]
    # 8: the diagonal is one region, and the zeros meet across it at (0,1)-(1,0)
    assert R.regions(m, 8).tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
    assert R.sieve(m, 2, 4, "bg", 0).tolist() == [[0, 0, 0]] * 3
    assert R.sieve(m, 2, 8, "bg", 0).tolist() == m.tolist()
    assert R.sieve(m, 4, 8, "bg", 0).tolist() == [[0, 0, 0]] * 3               # the diagonal has three pixels


def test_min_region_one_changes_nothing():
    m = R.patterns(9, 13)["iid7"]
    for conn in (4, 8):
        for fill in R.FILLS:
            assert np.array_equal(R.sieve(m, 1, conn, fill, 0), m)


def test_strict_comparison_on_the_area():
    m = A([[1, 1, 0, 2, 2, 2]])
    assert R.sieve(m, 3, 4, "bg", 0).tolist() == [[0, 0, 0, 2, 2, 2]]          # area 2 < 3 goes, area 3 stays
    assert R.sieve(m, 2, 4, "bg", 0).tolist() == [[1, 1, 0, 2, 2, 2]]          # area 2 is not below 2
    # neighbour: the 1s touch only the small 0 and fall to bg_idx; the 0 touches the kept 2s
    assert R.sieve(m, 3, 4, "neighbour", 0).tolist() == [[0, 0, 2, 2, 2, 2]]
    assert R.sieve(m, 3, 4, "neighbour", 9).tolist() == [[9, 9, 2, 2, 2, 2]]


def test_bg_fill_never_touches_background_regions():
    m = A([[0, 2, 2, 0, 3]])
    assert R.sieve(m, 2, 4, "bg", 0).tolist() == [[0, 2, 2, 0, 0]]
    assert R.sieve(m, 2, 4, "neighbour", 0).tolist() == [[2, 2, 2, 2, 0]]      # sieve: the single 0s go too; the 3 touches no kept region


def test_tie_goes_to_the_smaller_root_and_area_beats_root():
    assert R.sieve(A([[2, 2, 5, 3, 3]]), 2, 4, "neighbour", 0).tolist() == [[2, 2, 2, 3, 3]]
    assert R.sieve(A([[2, 2, 5, 3, 3, 3]]), 2, 4, "neighbour", 0).tolist() == [[2, 2, 3, 3, 3, 3]]
    assert R.sieve(A([[2, 2, 2, 5, 3, 3]]), 2, 4, "neighbour", 0).tolist() == [[2, 2, 2, 2, 3, 3]]
    # corner adjacency counts with connectivity 8 only: the 5 touches the 3s by an edge and the 2s (the larger region) by a corner
    m = A([[2, 2, 2, 2],
           [3, 3, 3, 5]])
    m2 = A([[2, 2, 2, 7],
            [2, 3, 3, 5],
            [2, 3, 3, 3]])
    assert R.sieve(m, 2, 4, "neighbour", 0).tolist() == [[2, 2, 2, 2], [3, 3, 3, 2]]        # 4 pixels of 2 above it, 3 of 3 beside it
    assert R.sieve(m2, 2, 4, "neighbour", 0)[1, 3] == 3 and R.sieve(m2, 2, 4, "neighbour", 0)[0, 3] == 2
    assert R.sieve(m2, 2, 8, "neighbour", 0)[1, 3] == 2                       # by the corner (0,2): five 2s against five 3s, root 0 < root 5


def test_one_pass_is_not_a_fixed_point():
    m = A([[2, 5, 3, 3]])
    once = R.sieve(m, 2, 4, "neighbour", 0)
    assert once.tolist() == [[0, 3, 3, 3]]                                     # the 2 sees only the small 5; the 5 sees the kept 3s
    assert R.sieve(once, 2, 4, "neighbour", 0).tolist() == [[3, 3, 3, 3]]


def test_nested_regions_and_any_int64_label():
    big, neg = (1 << 40) + 3, -5
    m = A([[big] * 5,
           [big, neg, neg, neg, big],
           [big, neg, 7, neg, big],
           [big, neg, neg, neg, big],
           [big] * 5])
    assert R.sieve(m, 2, 4, "neighbour", 0)[2, 2] == neg
    want = np.full((5, 5), big, dtype=np.int64)
    want[2, 2] = 0                                                            # the ring of 8 goes to the frame of 16; the centre touched only the small ring
    assert np.array_equal(R.sieve(m, 9, 4, "neighbour", 0), want)
    assert R.sieve(m, 9, 4, "bg", neg)[2, 2] == neg and R.sieve(m, 9, 4, "bg", neg)[1, 1] == neg


def test_images_of_a_batch_never_connect():
    a, b = A([[2, 2, 9]]), A([[9, 3, 3]])
    assert [x.tolist() for x in R.sieve_batch([a, b], 2, 4, "bg", 0)] == [[[2, 2, 0]], [[0, 3, 3]]]
    assert [x.tolist() for x in R.sieve_batch([a, b], 2, 4, "bg", 0, mutant="batch_connects")] == [[[2, 2, 9]], [[9, 3, 3]]]


def test_regions_equal_scipy_label():
    ndimage = pytest.importorskip("scipy.ndimage")
    for H, W in ((1, 1), (1, 40), (33, 70), (67, 131)):
        for name, m in R.patterns(H, W).items():
            for conn, st in ((4, None), (8, np.ones((3, 3), dtype=int))):
                root = R.regions(m, conn)
                assert np.array_equal(root.reshape(-1)[root.reshape(-1)], root.reshape(-1)), "a root is its own root"
                for v in np.unique(m):
                    sel = m == v
                    lab, n = ndimage.label(sel, structure=st)
                    pairs = set(zip(lab[sel].tolist(), root[sel].tolist()))
                    assert len(pairs) == n == len(set(root[sel].tolist())), (H, W, name, conn, int(v))
                    first = {}
                    for i in np.flatnonzero(sel.reshape(-1)).tolist():          # the root is the region's smallest raster index
                        first.setdefault(lab.reshape(-1)[i], i)
                    assert set(first.values()) == set(root[sel].tolist())


def _gpu_inputs():
    """Every (maps, min_region, connectivity, fill) the GPU test runs: the single maps, smallest shapes first, then the batch."""
    for H, W in R.SHAPES:
        for name, m in R.patterns(H, W).items():
            for conn in (4, 8):
                for fill in R.FILLS:
                    for mr in R.MIN_REGIONS:
                        yield (H, W, name), [m], R.min_region_of(mr, H, W), conn, fill
    for conn in (4, 8):
        for fill in R.FILLS:
            for mr in (2, 5, 64):
                yield "batch", R.batch_maps(), mr, conn, fill


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_gpu_inputs_tell_every_mutant_from_the_reference(mutant):
    for what, maps, mr, conn, fill in _gpu_inputs():
        if (mutant == "conn8_as_4" and conn == 4) or (mutant == "bg_regions_sieved_in_bg_mode" and fill != "bg") or \
                (mutant in ("tie_larger_root", "small_neighbour_wins") and fill != "neighbour") or (mutant == "batch_connects") != (what == "batch"):
            continue                                                           # the mutant restates the reference there
        want = R.sieve_batch(maps, mr, conn, fill, R.BG)
        got = R.sieve_batch(maps, mr, conn, fill, R.BG, mutant=mutant)
        if any(not np.array_equal(w, g) for w, g in zip(want, got)):
            print(f"{mutant}: first told apart by {what}, min_region={mr}, connectivity={conn}, fill={fill}")
            return
    pytest.fail(f"no input of the GPU test distinguishes the mutant '{mutant}' ({R.MUTANTS[mutant]})")


def test_the_tie_pattern_holds_a_tie():
    """The hand-made tie of the GPU inputs: the pixel 5 at (1,10) lies between regions of 31 pixels each and goes to the left one (root
    0); the one at (5,10) between 28 and 31 pixels and goes to the right one, whose root is larger."""
    t = R.patterns(33, 70)["tie"]
    root = R.regions(t, 4)
    area = np.bincount(root.reshape(-1), minlength=t.size)
    assert area[root[1, 9]] == area[root[1, 11]] == 31 and root[1, 9] < root[1, 11]
    assert area[root[5, 9]] == 28 and area[root[5, 11]] == 31 and root[5, 9] < root[5, 11]
    out = R.sieve(t, 5, 4, "neighbour", R.BG)
    assert out[1, 10] == 2 and out[5, 10] == 3
    assert R.sieve(t, 5, 4, "neighbour", R.BG, mutant="tie_larger_root")[1, 10] == 3
