"""The object scores behind evaluate (f32 tiny-8 tower, synthetic weights, the scenes and class file of tests/test_gpu_boundary_route.py:
40 x 150 and 47 x 61, crop 32, stride 16, Q = 8 -> K = 5), on SegmentorEx and Segmentor.

evaluate(images, gts, object_iou=0.5) must count what an ObjectMetric fed with the labels of predict_many counts, and what
tests/object_reference.py counts on those labels -- at the truth's size and with min_region set as well -- while the plain part of the
result stays what evaluate returns without the option; a metric passed back in accumulates with its own settings; without the option
nothing of the object path is called and the labels' bytes are the same; object_* with boundary_* or relaxed_*, a metric of another kind
and tile_group are refused."""
import numpy as np
import pytest
import torch

import object_reference as R
from test_gpu_boundary_route import BG, DEV, K, SHAPES, images
from test_gpu_tolerant_route import seg_of

pytestmark = pytest.mark.gpu

KEYS = {"ObjPrecision", "ObjRecall", "ObjF1", "SQ", "PQ"}
MEANS = {"m" + k for k in KEYS}


def truths(shapes, labels=None):
    """uint8 truth per image with an ignored rectangle: the labels moved by one column where labels are given, so that large regions still
    match and narrow ones do not; blocks otherwise."""
    out = []
    for i, hw in enumerate(shapes):
        g = R.blocky(hw[0], hw[1], K - 2, 7, 70 + i) if labels is None else np.roll(labels[i][0].cpu().numpy(), (0, 1), axis=(0, 1))
        g = g.astype(np.uint8)
        g[3:9, 10:30] = 255
        out.append(torch.from_numpy(g))
    return out


def same_plain(a, b):
    assert set(a) - KEYS == set(b) and KEYS <= set(a)
    for k in b:
        if k == "summary":
            assert set(a[k]) - MEANS == set(b[k]) and MEANS <= set(a[k])
            assert all(a[k][x] == v or (np.isnan(a[k][x]) and np.isnan(v)) for x, v in b[k].items())
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def check_scores(res, want):
    for name, v in zip(("ObjPrecision", "ObjRecall", "ObjF1", "SQ", "PQ"), R.scores(want)):
        assert np.array_equal(res[name], v, equal_nan=True), name
        mean = float(np.round(np.nanmean(v) * 100, 2)) if not np.isnan(v).all() else float("nan")
        assert res["summary"]["m" + name] == mean or (np.isnan(mean) and np.isnan(res["summary"]["m" + name])), name


CASES = [("SegmentorEx", {}, False), ("SegmentorEx", {}, True), ("SegmentorEx", {"min_region": 6, "region_connectivity": 8}, False),
         ("Segmentor", {"min_region": 6}, True)]


@pytest.mark.parametrize("cls,kw,at_gt_size", CASES, ids=["ex-plain", "ex-at_gt_size", "ex-min_region-conn8", "seg-min_region-at_gt_size"])
def test_evaluate_counts_what_the_reference_counts(tmp_path_factory, cls, kw, at_gt_size):
    from clip_decontamination_amd.metrics import ObjectMetric
    seg = seg_of(tmp_path_factory, cls, **kw)
    conn = kw.get("region_connectivity", 4)
    imgs = images()
    oris = [(33, 170), SHAPES[1]] if at_gt_size else SHAPES
    labels = seg.predict_many(imgs, None, ori_shapes=oris) if at_gt_size else seg.predict_many(imgs)
    assert [tuple(x.shape[-2:]) for x in labels] == [tuple(o) for o in oris]
    gts = truths(oris, labels)
    pairs = [(lab[0].cpu().numpy(), g.numpy()) for lab, g in zip(labels, gts)]
    res0, metric0 = seg.evaluate(imgs, gts, at_gt_size=at_gt_size)
    assert type(metric0).__name__ == "IoUMetric" and not (set(res0) | set(res0["summary"])) & (KEYS | MEANS)
    res, metric = seg.evaluate(imgs, gts, object_iou=0.5, at_gt_size=at_gt_size)
    assert isinstance(metric, ObjectMetric)
    assert (metric.object_iou, metric.min_area, metric.connectivity, metric.skip_label) == ((1, 2), 1, conn, BG)
    want = R.match_batch(pairs, K, (1, 2), connectivity=conn, skip_label=BG)[0]
    assert want[0].sum() > 0 and (want[0] < want[1]).any() and (want[0] < want[2]).any(), "the case would show nothing"
    assert np.array_equal(metric.object_counts.cpu().numpy(), want)
    check_scores(res, want)
    assert torch.equal(metric.confusion, metric0.confusion)
    same_plain(res, res0)
    # the same as an ObjectMetric fed by hand with the labels of predict_many
    hand = ObjectMetric(num_classes=K, object_iou=0.5, connectivity=conn, skip_label=BG)
    for lab, g in zip(labels, gts):
        hand.add(lab, g.to(DEV))
    assert torch.equal(hand.object_counts, metric.object_counts) and torch.equal(hand.confusion, metric.confusion)
    # a higher threshold, a minimum area and the background as a class
    res3, metric3 = seg.evaluate(imgs, gts, object_iou=(3, 4), object_min_area=4, object_include_bg=True, at_gt_size=at_gt_size)
    want3 = R.match_batch(pairs, K, (3, 4), connectivity=conn, min_area=4)[0]
    assert (metric3.object_iou, metric3.min_area, metric3.skip_label) == ((3, 4), 4, None)
    assert np.array_equal(metric3.object_counts.cpu().numpy(), want3) and not np.array_equal(want3, want)
    check_scores(res3, want3)
    same_plain(res3, res0)
    # the returned metric accumulates with its own settings, with or without the option named again
    res2, again = seg.evaluate(imgs, gts, metric=metric, object_iou=0.75, at_gt_size=at_gt_size)
    assert again is metric and np.array_equal(metric.object_counts.cpu().numpy(), 2 * want)
    assert torch.equal(metric.confusion, 2 * metric0.confusion)
    assert np.array_equal(res2["PQ"], res["PQ"], equal_nan=True)
    seg.evaluate(imgs, gts, metric=metric, at_gt_size=at_gt_size)
    assert np.array_equal(metric.object_counts.cpu().numpy(), 3 * want)


def test_whole_image_inference(tmp_path_factory):
    """slide_crop = 0 goes image by image."""
    imgs = [x[:, :40, :48].contiguous() for x in images()]
    seg = seg_of(tmp_path_factory, slide_crop=0)
    labels = [seg.predict(x[None], None) for x in imgs]
    gts = truths([(40, 48)] * 2, labels)
    res, metric = seg.evaluate(imgs, gts, object_iou=0.5)
    want = R.match_batch([(lab[0].cpu().numpy(), g.numpy()) for lab, g in zip(labels, gts)], K, (1, 2), skip_label=BG)[0]
    assert np.array_equal(metric.object_counts.cpu().numpy(), want) and want[1].sum() > 0


def test_without_the_option_nothing_of_the_object_path_runs(tmp_path_factory, monkeypatch):
    from clip_decontamination_amd import _lib, ops
    seg = seg_of(tmp_path_factory)
    imgs = images()
    gts = truths(SHAPES)
    before = [x.clone() for x in seg.predict_many(imgs)]
    calls = []
    lib = _lib.load()

    class Spy:
        """The loaded library with the object entries counted."""
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("sg_object"):
                calls.append(name)
            return fn

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    monkeypatch.setattr(ops, "object_match", lambda *a, **k: calls.append("object_match"))
    res, metric = seg.evaluate(imgs, gts)
    assert calls == [] and type(metric).__name__ == "IoUMetric" and "PQ" not in res
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    res1, metric1 = seg.evaluate(imgs, gts, object_iou=0.5)                              # the spy does see the option's calls
    assert "sg_object_match" in calls and "sg_object_workspace_bytes" in calls
    assert torch.equal(metric1.confusion, metric.confusion) and res1["summary"]["mIoU"] == res["summary"]["mIoU"]
    monkeypatch.undo()
    after = seg.predict_many(imgs)
    assert all(torch.equal(a, b) for a, b in zip(before, after))                         # the labels' bytes, with the option used in between


def test_refusals(tmp_path_factory):
    from clip_decontamination_amd.metrics import BoundaryIoUMetric, IoUMetric, ObjectMetric, RelaxedMetric
    seg = seg_of(tmp_path_factory)
    imgs = images()
    gts = truths(SHAPES)
    for other in (IoUMetric(num_classes=K), RelaxedMetric(num_classes=K), BoundaryIoUMetric(num_classes=K)):
        with pytest.raises((TypeError, ValueError), match="ObjectMetric|one call"):
            seg.evaluate(imgs, gts, metric=other, object_iou=0.5)
    with pytest.raises(TypeError, match="ObjectMetric"):
        seg.evaluate(imgs, gts, metric=IoUMetric(num_classes=K), object_iou=0.5)
    for kw in (dict(object_iou=0.5, boundary_px=2), dict(object_iou=0.5, relaxed_px=2), dict(object_iou=0.5, relaxed_ratio=0.01),
               dict(object_iou=0.5, boundary_ratio=0.02), dict(boundary_px=2, metric=ObjectMetric(num_classes=K)),
               dict(relaxed_px=2, metric=ObjectMetric(num_classes=K)), dict(object_iou=0.5, metric=RelaxedMetric(num_classes=K))):
        with pytest.raises(ValueError, match="one call"):
            seg.evaluate(imgs, gts, **kw)
    for kw, word in ((dict(object_iou=0.49), "object_iou"), (dict(object_iou=1.0), "object_iou"), (dict(object_iou=(1, 3)), "object_iou"),
                     (dict(object_iou=0.5, object_min_area=0), "min_area"), (dict(object_iou=0.5, object_min_area=2.5), "min_area")):
        with pytest.raises(ValueError, match=word):
            seg.evaluate(imgs, gts, **kw)
    seg.tile_group = "world"
    try:
        with pytest.raises(ValueError, match="tile_group sharding is not supported"):
            seg.evaluate(imgs, gts, object_iou=0.5)
    finally:
        seg.tile_group = None
