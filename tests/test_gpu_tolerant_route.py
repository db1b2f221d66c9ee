"""The tolerant scores behind evaluate (f32 tiny-8 tower, synthetic weights, the scenes and class file of
tests/test_gpu_boundary_route.py: 40 x 150 and 47 x 61, crop 32, stride 16, Q = 8 -> K = 5), on SegmentorEx and Segmentor.

evaluate(images, gts, relaxed_px=3) and evaluate(..., relaxed_ratio=0.0075, relaxed_mode="contour") must count what
tests/tolerant_reference.py counts on the labels predict_many returns for the same inputs -- at the truth's size and with min_region set
as well -- while the plain part of the result stays what evaluate returns without the option; a metric passed back in accumulates with its
own settings; without the option nothing of the tolerant path is called and the labels' bytes are the same; relaxed_* with boundary_*, a
metric of the other kind and tile_group are refused."""
import numpy as np
import pytest
import torch

import tolerant_reference as R
from test_gpu_boundary_route import BG, DEV, K, SHAPES, class_file, images

pytestmark = pytest.mark.gpu

PX = 3
_SEG = {}
NEW_KEYS = {R.REGION: ({"RelPrecision", "RelRecall", "RelFscore"}, {"mRelPrecision", "mRelRecall", "mRelFscore"}),
            R.CONTOUR: ({"BPrecision", "BRecall", "BFscore"}, {"mBPrecision", "mBRecall", "mBF"})}


def seg_of(tmp_path_factory, cls="SegmentorEx", **kw):
    key = (cls,) + tuple(sorted(kw.items()))
    if key not in _SEG:
        import segearth_segmentor
        import segmentor
        args = dict(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path=class_file(tmp_path_factory),
                    device=torch.device(DEV), precision="f32", synthetic_ok=True, prob_thd=0.05, bg_idx=BG, apply_sim_feat_up=False,
                    slide_crop=32, slide_stride=16)
        args.update(kw)
        _SEG[key] = (segmentor.SegmentorEx if cls == "SegmentorEx" else segearth_segmentor.Segmentor)(**args)
    return _SEG[key]


def truths(shapes, labels=None):
    """uint8 truth per image with an ignored rectangle: the labels moved by (3, 2) pixels where labels are given -- 13 > 3^2, so a
    structure narrower than the move is not found at 3 px while the inside of a wide one is -- blocks otherwise."""
    out = []
    for i, hw in enumerate(shapes):
        g = R.blocky(hw[0], hw[1], K, 7, 70 + i) if labels is None else np.roll(labels[i][0].cpu().numpy(), (3, 2), axis=(0, 1))
        g = g.astype(np.uint8)
        g[3:9, 10:30] = 255
        out.append(torch.from_numpy(g))
    return out


def same_plain(a, b, mode):
    keys, means = NEW_KEYS[mode]
    assert set(a) - keys == set(b) and keys <= set(a)
    for k in b:
        if k == "summary":
            assert set(a[k]) - means == set(b[k]) and means <= set(a[k])
            assert all(a[k][x] == v or (np.isnan(a[k][x]) and np.isnan(v)) for x, v in b[k].items())
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def check_scores(res, want, mode):
    names = ("RelPrecision", "RelRecall", "RelFscore") if mode == R.REGION else ("BPrecision", "BRecall", "BFscore")
    means = ("mRelPrecision", "mRelRecall", "mRelFscore") if mode == R.REGION else ("mBPrecision", "mBRecall", "mBF")
    for name, mean, v in zip(names, means, R.scores(want)):
        assert np.array_equal(res[name], v, equal_nan=True), name
        assert res["summary"][mean] == float(np.round(np.nanmean(v) * 100, 2)), mean


CASES = [("SegmentorEx", {}, False), ("SegmentorEx", {}, True), ("SegmentorEx", {"min_region": 6}, False),
         ("Segmentor", {}, False), ("Segmentor", {"min_region": 6}, True)]


@pytest.mark.parametrize("cls,kw,at_gt_size", CASES, ids=["ex-plain", "ex-at_gt_size", "ex-min_region", "seg-plain", "seg-min_region-at_gt_size"])
def test_evaluate_counts_what_the_reference_counts(tmp_path_factory, cls, kw, at_gt_size):
    from clip_decontamination_amd.metrics import RelaxedMetric
    seg = seg_of(tmp_path_factory, cls, **kw)
    imgs = images()
    oris = [(33, 170), SHAPES[1]] if at_gt_size else SHAPES
    labels = seg.predict_many(imgs, None, ori_shapes=oris) if at_gt_size else seg.predict_many(imgs)
    assert [tuple(x.shape[-2:]) for x in labels] == [tuple(o) for o in oris]
    gts = truths(oris, labels)
    pairs = [(lab[0].cpu().numpy(), g.numpy()) for lab, g in zip(labels, gts)]
    res0, metric0 = seg.evaluate(imgs, gts, at_gt_size=at_gt_size)
    assert type(metric0).__name__ == "IoUMetric" and not (set(res0) | set(res0["summary"])) & set().union(*NEW_KEYS[R.REGION], *NEW_KEYS[R.CONTOUR])
    # a fixed tolerance in region mode: relaxed precision / recall
    res, metric = seg.evaluate(imgs, gts, relaxed_px=PX, at_gt_size=at_gt_size)
    assert isinstance(metric, RelaxedMetric) and metric.tolerance_px == PX and metric.mode == "region"
    want = R.counts_batch(pairs, [PX * PX] * len(pairs), K)
    assert (want[1] < want[0]).any() and (want[1] > R.counts_batch(pairs, [0, 0], K)[1]).any(), "the tolerance changes nothing: the case would show nothing"
    assert np.array_equal(metric.tolerant_counts.cpu().numpy(), want)
    check_scores(res, want, R.REGION)
    assert torch.equal(metric.confusion, metric0.confusion)
    same_plain(res, res0, R.REGION)
    # the ratio in contour mode: the boundary F-score, each image with its own tolerance
    resc, metricc = seg.evaluate(imgs, gts, relaxed_ratio=0.0075, relaxed_mode="contour", at_gt_size=at_gt_size)
    ts = [R.tolerance_sq(o) for o in oris]
    assert ts == [4, 1]
    wantc = R.counts_batch(pairs, ts, K, mode=R.CONTOUR)
    assert wantc[1].sum() > 0 and (wantc[1] < wantc[0]).any()
    assert metricc.mode == "contour" and np.array_equal(metricc.tolerant_counts.cpu().numpy(), wantc)
    check_scores(resc, wantc, R.CONTOUR)
    same_plain(resc, res0, R.CONTOUR)
    # the returned metric accumulates with its own settings, with or without the option named again
    res2, again = seg.evaluate(imgs, gts, metric=metric, relaxed_px=7, at_gt_size=at_gt_size)
    assert again is metric and np.array_equal(metric.tolerant_counts.cpu().numpy(), 2 * want)
    assert torch.equal(metric.confusion, 2 * metric0.confusion)
    assert np.array_equal(res2["RelFscore"], res["RelFscore"], equal_nan=True)
    seg.evaluate(imgs, gts, metric=metric, at_gt_size=at_gt_size)
    assert np.array_equal(metric.tolerant_counts.cpu().numpy(), 3 * want)


def test_whole_image_inference(tmp_path_factory):
    """slide_crop = 0 goes image by image."""
    imgs = [x[:, :40, :48].contiguous() for x in images()]
    seg = seg_of(tmp_path_factory, slide_crop=0)
    labels = [seg.predict(x[None], None) for x in imgs]
    gts = truths([(40, 48)] * 2, labels)
    res, metric = seg.evaluate(imgs, gts, relaxed_px=2)
    want = R.counts_batch([(lab[0].cpu().numpy(), g.numpy()) for lab, g in zip(labels, gts)], [4, 4], K)
    assert np.array_equal(metric.tolerant_counts.cpu().numpy(), want) and want[1].sum() > 0


def test_without_the_option_nothing_of_the_tolerant_path_runs(tmp_path_factory, monkeypatch):
    from clip_decontamination_amd import _lib, ops
    seg = seg_of(tmp_path_factory)
    imgs = images()
    gts = truths(SHAPES)
    before = [x.clone() for x in seg.predict_many(imgs)]
    calls = []
    lib = _lib.load()

    class Spy:
        """The loaded library with the tolerant entries counted."""
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("sg_tolerant"):
                calls.append(name)
            return fn

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    monkeypatch.setattr(ops, "tolerant_accumulate", lambda *a, **k: calls.append("tolerant_accumulate"))
    res, metric = seg.evaluate(imgs, gts)
    assert calls == [] and type(metric).__name__ == "IoUMetric" and "RelFscore" not in res
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    res1, metric1 = seg.evaluate(imgs, gts, relaxed_px=PX)                               # the spy does see the option's calls
    assert "sg_tolerant_accumulate" in calls
    assert torch.equal(metric1.confusion, metric.confusion)
    monkeypatch.undo()
    after = seg.predict_many(imgs)
    assert all(torch.equal(a, b) for a, b in zip(before, after))                         # the labels' bytes, with the option used in between


def test_refusals(tmp_path_factory):
    from clip_decontamination_amd.metrics import BoundaryIoUMetric, IoUMetric, RelaxedMetric
    seg = seg_of(tmp_path_factory)
    imgs = images()
    gts = truths(SHAPES)
    with pytest.raises(TypeError, match="RelaxedMetric"):
        seg.evaluate(imgs, gts, metric=IoUMetric(num_classes=K), relaxed_px=PX)
    for kw in (dict(relaxed_px=PX, boundary_px=2), dict(relaxed_ratio=0.01, boundary_ratio=0.02),
               dict(relaxed_px=PX, metric=BoundaryIoUMetric(num_classes=K)), dict(boundary_px=2, metric=RelaxedMetric(num_classes=K))):
        with pytest.raises(ValueError, match="one call"):
            seg.evaluate(imgs, gts, **kw)
    for kw, word in ((dict(relaxed_px=-1), "tolerance_px"), (dict(relaxed_px=255), "tolerance_px"), (dict(relaxed_px=2.5), "tolerance_px"),
                     (dict(relaxed_ratio=-1), "tolerance_ratio"), (dict(relaxed_px=2, relaxed_mode="band"), "mode")):
        with pytest.raises(ValueError, match=word):
            seg.evaluate(imgs, gts, **kw)
    seg.tile_group = "world"
    try:
        with pytest.raises(ValueError, match="tile_group sharding is not supported"):
            seg.evaluate(imgs, gts, relaxed_px=PX)
    finally:
        seg.tile_group = None
