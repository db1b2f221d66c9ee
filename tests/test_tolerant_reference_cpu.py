"""tests/tolerant_reference.py against itself and against scipy, without a GPU: the any-radius form against the literal OR of all shifts of
the disk; both against scipy.ndimage.distance_transform_edt where scipy is importable; the two identities of the definition (tol_sq = 0
in region mode is the confusion table; a tolerance above the image's diagonal matches a source iff its class is marked anywhere in the
other map); hand-worked cases; tolerance_sq."""
import numpy as np
import pytest

import boundary_reference as B
import iou_reference as IOU
import tolerant_reference as R

SMALL_TOL = [0, 1, 2, 9, 10, 25]
MODES = (R.REGION, R.CONTOUR)


def _inputs(H, W):
    pats = B.patterns(H, W, R.PATTERN_D)
    for n in R.CPU_MAPS:
        for fmt in (np.uint8, np.int64):
            yield n, fmt, B.truth_for(pats[n], fmt, 7 * H + W)


@pytest.mark.parametrize("shape", B.SHAPES[:5], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", MODES)
def test_any_radius_form_equals_the_literal_form(shape, mode):
    H, W = shape
    told = 0
    for n, fmt, (p, g) in _inputs(H, W):
        for rzl in (False, True):
            got = R.counts_multi(p, g, SMALL_TOL, B.K, 255, rzl, mode)
            for t in SMALL_TOL:
                want = R.counts_literal(p, g, t, B.K, 255, rzl, mode)
                assert np.array_equal(got[t], want), (n, fmt.__name__, rzl, t)
                assert np.array_equal(R.counts(p, g, t, B.K, 255, rzl, mode), want)
            told += int(any(not np.array_equal(got[a], got[b]) for a, b in zip(SMALL_TOL, SMALL_TOL[1:])))
    assert told > 0 or H * W < 8


def test_the_inputs_tell_the_radii_apart():
    """On the 67 x 131 blocky map every step 0 -> 1 -> 2 -> 9 -> 10 -> 25 changes the counts in both modes; at 1600 all sources match."""
    p, g = B.truth_for(B.patterns(67, 131, R.PATTERN_D)["blocky"], np.uint8, 3)
    for mode in MODES:
        got = R.counts_multi(p, g, SMALL_TOL + [1600], B.K, 255, False, mode)
        for a, b in zip(SMALL_TOL, SMALL_TOL[1:]):
            assert not np.array_equal(got[a], got[b]), (mode, a, b)
            assert (got[a][[1, 3]] <= got[b][[1, 3]]).all()
        assert np.array_equal(got[1600][1], got[1600][0]) and np.array_equal(got[1600][3], got[1600][2])
        assert (got[0][1] < got[0][0]).all()


@pytest.mark.parametrize("mode", MODES)
def test_both_forms_equal_scipy_edt(mode):
    nd = pytest.importorskip("scipy.ndimage")
    K = B.K
    for H, W in ((17, 64), (33, 70)):
        p, g = B.truth_for(B.patterns(H, W, R.PATTERN_D)["blocky"], np.int64, H)
        mp, mg = (R.contour(p), R.contour(g)) if mode == R.CONTOUR else (np.ones((H, W), bool), np.ones((H, W), bool))
        counted = g != 255
        for t in SMALL_TOL + [144, 400]:
            want = np.zeros((4, K), dtype=np.int64)
            for k in range(K):
                sp, sg = mp & (p == k), mg & (g == k)
                dg = nd.distance_transform_edt(~sg) if sg.any() else np.full((H, W), 1e9)
                dp = nd.distance_transform_edt(~sp) if sp.any() else np.full((H, W), 1e9)
                want[0, k], want[2, k] = np.count_nonzero(sp & counted), np.count_nonzero(sg & counted)
                want[1, k] = np.count_nonzero(sp & counted & (np.rint(dg * dg) <= t))
                want[3, k] = np.count_nonzero(sg & counted & (np.rint(dp * dp) <= t))
            assert np.array_equal(R.counts(p, g, t, K, 255, False, mode), want), t
            if t <= 144:
                assert np.array_equal(R.counts_literal(p, g, t, K, 255, False, mode), want), t


def test_zero_tolerance_in_region_mode_is_the_confusion_table():
    K = B.K
    for H, W in B.SHAPES:
        for fmt in (np.uint8, np.int64):
            p, g = B.truth_for(B.patterns(H, W, R.PATTERN_D)["blocky"], fmt, H + W)
            for rzl in (False, True):
                inter, _, pred, label = IOU.intersect_and_union(p, g, K, 255, rzl)
                got = R.counts(p, g, 0, K, 255, rzl, R.REGION)
                assert np.array_equal(got, np.stack([pred, inter, label, inter])), (H, W, fmt.__name__, rzl)


@pytest.mark.parametrize("mode", MODES)
def test_a_tolerance_above_the_diagonal_matches_whatever_is_marked_anywhere(mode):
    K = B.K
    for H, W in B.SHAPES[:6]:
        p, g = B.truth_for(B.patterns(H, W, R.PATTERN_D)["blocky"], np.int64, H)
        p = np.where(p == 3, 4, p)                                             # class 3 is absent from the prediction
        t = (H - 1) ** 2 + (W - 1) ** 2
        got = R.counts(p, g, t, K, 255, False, mode)
        mp, mg = (R.contour(p), R.contour(g)) if mode == R.CONTOUR else (np.ones((H, W), bool), np.ones((H, W), bool))
        for k in range(K):
            in_g, in_p = (mg & (g == k)).any(), (mp & (p == k)).any()
            assert got[1, k] == (got[0, k] if in_g else 0) and got[3, k] == (got[2, k] if in_p else 0), (H, W, k)
        assert got[3, 3] == 0


def test_nine_is_not_ten():
    """A single target at the offset (1, 3): 1 + 9 = 10."""
    p, g = np.zeros((9, 9), dtype=np.int64), np.zeros((9, 9), dtype=np.int64)
    p[4, 4], g[5, 7] = 1, 1
    for fn in (R.counts, R.counts_literal):
        assert fn(p, g, 9, 2)[:, 1].tolist() == [1, 0, 1, 0]
        assert fn(p, g, 10, 2)[:, 1].tolist() == [1, 1, 1, 1]
        assert fn(p, g, 9, 2, mode=R.CONTOUR)[:, 1].tolist() == [1, 0, 1, 0]
        assert fn(p, g, 10, 2, mode=R.CONTOUR)[:, 1].tolist() == [1, 1, 1, 1]


def test_a_line_moved_by_two_pixels():
    """A one-pixel-wide line moved by 2 px: relaxed precision = recall = 1 at tol_sq = 4 and 0 at tol_sq = 3."""
    p, g = np.zeros((12, 20), dtype=np.int64), np.zeros((12, 20), dtype=np.int64)
    p[5, :], g[7, :] = 1, 1
    for fn in (R.counts, R.counts_literal):
        pr, rc, f = R.scores(fn(p, g, 4, 2))
        assert pr[1] == rc[1] == f[1] == 1.0
        pr, rc, f = R.scores(fn(p, g, 3, 2))
        assert pr[1] == rc[1] == 0.0 and np.isnan(f[1])
        assert fn(p, g, 3, 2)[:, 1].tolist() == [20, 0, 20, 0]


def test_one_pixel_has_no_contour():
    one = np.array([[1]])
    assert not R.contour(one).any()
    assert R.counts(one, one, 0, 2, mode=R.CONTOUR).tolist() == [[0, 0]] * 4
    assert R.counts(one, one, 0, 2, mode=R.REGION).tolist() == [[0, 1]] * 4
    lab = np.array([[0, 0, 1], [0, 0, 1]])                                     # the image border is not a contour
    assert R.contour(lab).tolist() == [[False, True, True], [False, True, True]]


def test_ignored_truth_is_a_value_for_the_contour_and_no_source():
    g = np.array([[1, 1, 255, 255]] * 3)
    p = np.ones((3, 4), dtype=np.int64)
    got = R.counts(p, g, 0, 2, 255, False, R.CONTOUR)
    assert got[:, 1].tolist() == [0, 0, 3, 0]                                  # the truth's class 1 has a contour at the ignored area
    got = R.counts(p, g, 1, 2, 255, False, R.REGION)
    assert got[:, 1].tolist() == [6, 6, 6, 6]                                  # sources under ignored truth are not counted


def test_tolerance_from_the_ratio():
    assert R.tolerance_sq((2048, 4608)) == 38 * 38
    assert R.tolerance_sq((512, 512)) == 6 * 6
    assert R.tolerance_sq((1, 1)) == 1
    assert R.tolerance_sq((300, 400), 0.0099) == 25 and R.tolerance_sq((300, 400), 0.0101) == 36      # the ceiling of 4.95 and of 5.05
