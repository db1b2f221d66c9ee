"""tests/boundary_reference.py against the paper's own construction, without a GPU: per class mask - erode^d(pad0(mask)) with the
erosion written as d iterated 3 x 3 minima in numpy (and scipy.ndimage.binary_erosion where scipy is importable); the literal padded
form against the form that takes the two clauses apart; the identity d >= max(H, W) -> areas = the areas of the confusion table;
boundary_width and metrics_from_boundary on hand-made inputs."""
import numpy as np
import pytest

import boundary_reference as R
import iou_reference as IOU


def erode3(mask):
    """One 3 x 3 erosion of a 0 / 1 map with zeros outside (cv2.erode on the zero-padded mask, as the official code pads)."""
    H, W = mask.shape
    p = np.zeros((H + 2, W + 2), dtype=mask.dtype)
    p[1:-1, 1:-1] = mask
    out = np.ones_like(mask)
    for dy in range(3):
        for dx in range(3):
            out = np.minimum(out, p[dy:dy + H, dx:dx + W])
    return out


def paper_band(lab, d, classes):
    """The union over the classes of mask_c - erode^d(pad0(mask_c)): every pixel has one label, so the union is one bit per pixel."""
    out = np.zeros(lab.shape, dtype=np.uint8)
    for c in classes:
        mask = (lab == c).astype(np.uint8)
        er = mask
        for _ in range(d):
            er = erode3(er)
        out |= mask - er
    return out


CASES = [(H, W, d) for H, W in ((1, 1), (1, 7), (7, 1), (9, 14), (17, 30), (33, 21)) for d in (1, 2, 5, 12)]


@pytest.mark.parametrize("H,W,d", CASES)
def test_reference_is_the_papers_mask_minus_erosion(H, W, d):
    for name, m in R.patterns(H, W, d).items():
        got = R.band(m, d)
        assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got, R.band_padded(m, d)), name
        assert np.array_equal(got, paper_band(m, d, np.unique(m))), name
    m = R.patterns(H, W, d)["vstripe_2d+1"]
    if W >= 3 * (2 * d + 1) and H > 2 * d:                       # a whole stripe away from the left and right edges: one centre line is out of the band
        assert not R.band(m, d)[d:H - d, (2 * d + 1) + d].any() and R.band(m, d)[d:H - d, (2 * d + 1) + d - 1].all()
    assert R.band(R.patterns(H, W, 1)["checker"], 1).all()


def test_reference_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for H, W, d in ((17, 30, 2), (33, 21, 5), (40, 41, 1)):
        for name, m in R.patterns(H, W, d).items():
            want = np.zeros((H, W), dtype=np.uint8)
            for c in np.unique(m):
                mask = m == c
                want |= (mask & ~ndi.binary_erosion(mask, structure=np.ones((3, 3), dtype=bool), iterations=d, border_value=0)).astype(np.uint8)
            assert np.array_equal(R.band(m, d), want), (name, H, W, d)


@pytest.mark.parametrize("fmt", [np.uint8, np.int64])
@pytest.mark.parametrize("rzl", [False, True])
def test_every_pixel_in_the_band_gives_the_confusion_areas(fmt, rzl):
    from clip_decontamination_amd.metrics import areas_from_confusion
    H, W = 17, 30
    p, g = R.truth_for(R.patterns(H, W, 2)["blocky_fine"], fmt, 3)
    for d in (30, 31, 300):
        areas = R.boundary_areas(p, g, d, R.K, 255, rzl)
        inter, _, pred, label = areas_from_confusion(IOU.confusion_table(p, g, R.K, 255, rzl))
        assert np.array_equal(areas, np.stack([inter, pred, label]))
        i2, _, p2, l2 = IOU.intersect_and_union(p, g, R.K, 255, rzl)
        assert np.array_equal(areas, np.stack([i2, p2, l2]))
    small = R.boundary_areas(p, g, 1, R.K, 255, rzl)              # 3 x 3 blocks: their centres are out of the band
    assert (small <= areas).all() and (small < areas).any() and small[0].sum() > 0


def test_ignored_truth_keeps_its_place_in_the_map():
    """A class next to an ignored area has a boundary there; the ignored pixels themselves are not counted."""
    g = np.zeros((9, 20), dtype=np.uint8)
    g[:, 10:] = 255
    p = np.zeros((9, 20), dtype=np.int64)
    a = R.boundary_areas(p, g, 1, 1)
    inner = 7 * 8                                                 # class 0 is columns 0..9; out of the band: rows 1..7, columns 1..8
    assert a[2, 0] == 90 - inner                                  # column 9 borders the ignored area and is in the truth's band
    assert a[1, 0] == 90 - 7 * 9                                  # the flat prediction's band is the image rim, counted where the truth is not ignored
    assert a[0, 0] == 90 - 7 * 9                                  # the rim is in both bands


def test_boundary_width():
    from clip_decontamination_amd import ops
    # 0.02 * sqrt(2) * 512 = 14.48: 14 px on a 512 tile
    for hw, want in (((512, 512), 14), ((448, 448), 13), ((2048, 4608), 101), ((1, 1), 1)):
        assert ops.boundary_width(hw) == want == R.width(hw)
    assert ops.boundary_width((100, 100), 0.5) == 71 and ops.boundary_width((3, 4), 0.5) == 2      # round(2.5) = 2: Python's round
    for bad in (0, -0.1, float("nan"), float("inf"), "0.02", True):
        with pytest.raises(ValueError, match="boundary_ratio"):
            ops.boundary_width((10, 10), bad)
    with pytest.raises(ValueError, match="4095"):
        ops.boundary_width((4000, 4000), 0.9)


def test_metrics_from_boundary():
    from clip_decontamination_amd.metrics import metrics_from_boundary
    areas = np.array([[3, 0, 0, 5], [4, 2, 0, 5], [6, 0, 0, 5]], dtype=np.int64)
    out = metrics_from_boundary(areas)
    assert out["BIoU"].dtype == np.float64
    assert out["BIoU"][0] == 3 / 7 and out["BIoU"][1] == 0.0 and np.isnan(out["BIoU"][2]) and out["BIoU"][3] == 1.0
    assert out["summary"] == {"mBIoU": float(np.round((3 / 7 + 0 + 1) / 3 * 100, 2))}          # the absent class is left out of the mean
    assert np.array_equal(out["BIoU"], R.biou(areas), equal_nan=True)
    filled = metrics_from_boundary(areas, nan_to_num=0)
    assert filled["BIoU"][2] == 0.0 and filled["summary"]["mBIoU"] == float(np.round((3 / 7 + 1) / 4 * 100, 2))
    import torch
    assert np.array_equal(metrics_from_boundary(torch.from_numpy(areas))["BIoU"], out["BIoU"], equal_nan=True)
    assert np.isnan(metrics_from_boundary(np.zeros((3, 2), dtype=np.int64))["summary"]["mBIoU"])
    with pytest.raises(ValueError):
        metrics_from_boundary(np.zeros((2, 4), dtype=np.int64))
    with pytest.raises(TypeError):
        metrics_from_boundary(np.zeros((3, 4)))
