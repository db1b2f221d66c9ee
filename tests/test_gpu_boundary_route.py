"""Boundary IoU behind evaluate (f32 tiny-8 tower, synthetic weights, the scenes and class file of tests/test_gpu_sieve_route.py: 40 x 150
and 47 x 61, crop 32, stride 16, Q = 8 -> K = 5).

evaluate(images, gts, boundary_px=3) must count what tests/boundary_reference.py counts on the labels predict returns -- at the truth's
size and with min_region set as well -- while the plain part of its result stays what evaluate returns without the option; a metric
passed back in accumulates; without the option nothing of the boundary path is called; tile_group is refused."""
import numpy as np
import pytest
import torch

import boundary_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(40, 150), (47, 61)]
Q, K, BG = 8, 5, 3
PX = 3
_SEG = {}


def class_file(tmp_path_factory):
    lines, q = [], 0
    for c in range(K):
        k = 2 if c < Q - K else 1
        lines.append(",".join(f"thing{q + i}" for i in range(k)))
        q += k
    path = tmp_path_factory.getbasetemp() / "boundary_cls.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def seg_of(tmp_path_factory, **kw):
    key = tuple(sorted(kw.items()))
    if key not in _SEG:
        import segmentor
        args = dict(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path=class_file(tmp_path_factory),
                    device=torch.device(DEV), precision="f32", synthetic_ok=True, prob_thd=0.05, bg_idx=BG, apply_sim_feat_up=False,
                    slide_crop=32, slide_stride=16)
        args.update(kw)
        _SEG[key] = segmentor.SegmentorEx(**args)
    return _SEG[key]


def images():
    from clip_decontamination_amd import weights as Wt
    mean = torch.tensor(Wt.PIXEL_MEAN, device=DEV).view(3, 1, 1)
    std = torch.tensor(Wt.PIXEL_STD, device=DEV).view(3, 1, 1)
    out = []
    for i, hw in enumerate(SHAPES):
        u8 = torch.from_numpy(np.random.default_rng(20 + i).integers(0, 233, hw + (3,), dtype=np.uint8)).to(DEV)
        out.append(((u8.permute(2, 0, 1).float() - mean) / std).contiguous())
    return out


def truths(shapes, labels=None):
    """uint8 truth per image with an ignored rectangle: the labels moved by two pixels where labels are given (so that the bands
    meet), blocks otherwise."""
    out = []
    for i, hw in enumerate(shapes):
        g = R.blocky(hw[0], hw[1], K, 7, 70 + i) if labels is None else np.roll(labels[i][0].cpu().numpy(), (2, 1), axis=(0, 1))
        g = g.astype(np.uint8)
        g[3:9, 10:30] = 255
        out.append(torch.from_numpy(g))
    return out


def same_plain(a, b):
    assert set(a) - {"BIoU"} == set(b)
    for k in b:
        if k == "summary":
            assert {x: v for x, v in a[k].items() if x != "mBIoU"} == b[k] or \
                all(a[k][x] == v or (np.isnan(a[k][x]) and np.isnan(v)) for x, v in b[k].items())
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.mark.parametrize("kw,at_gt_size", [({}, False), ({}, True), ({"min_region": 6}, False)], ids=["plain", "at_gt_size", "min_region"])
def test_evaluate_counts_what_the_reference_counts(tmp_path_factory, kw, at_gt_size):
    from clip_decontamination_amd.metrics import BoundaryIoUMetric
    seg = seg_of(tmp_path_factory, **kw)
    imgs = images()
    oris = [(33, 170), SHAPES[1]] if at_gt_size else SHAPES
    labels = seg.predict_many(imgs, None, ori_shapes=oris) if at_gt_size else seg.predict_many(imgs)
    assert [tuple(x.shape[-2:]) for x in labels] == [tuple(o) for o in oris]
    gts = truths(oris, labels)
    res, metric = seg.evaluate(imgs, gts, boundary_px=PX, at_gt_size=at_gt_size)
    assert isinstance(metric, BoundaryIoUMetric) and metric.boundary_px == PX
    pairs = [(lab[0].cpu().numpy(), g.numpy()) for lab, g in zip(labels, gts)]
    want = R.boundary_areas_batch(pairs, [PX] * len(pairs), K)
    assert want[0].sum() > 0 and (want[0] < want[1]).any(), "the bands never meet or never differ: the case would show nothing"
    assert np.array_equal(metric.boundary_areas.cpu().numpy(), want)
    assert np.array_equal(res["BIoU"], R.biou(want), equal_nan=True)
    assert res["summary"]["mBIoU"] == float(np.round(np.nanmean(R.biou(want)) * 100, 2))
    # the plain part is evaluate's without the option, exactly
    res0, metric0 = seg.evaluate(imgs, gts, at_gt_size=at_gt_size)
    assert type(metric0).__name__ == "IoUMetric" and "BIoU" not in res0 and "mBIoU" not in res0["summary"]
    assert torch.equal(metric.confusion, metric0.confusion)
    same_plain(res, res0)
    # the returned metric accumulates, with or without the option named again
    res2, again = seg.evaluate(imgs, gts, metric=metric, boundary_px=PX, at_gt_size=at_gt_size)
    assert again is metric and np.array_equal(metric.boundary_areas.cpu().numpy(), 2 * want)
    assert torch.equal(metric.confusion, 2 * metric0.confusion)
    assert np.array_equal(res2["BIoU"], res["BIoU"], equal_nan=True)
    seg.evaluate(imgs, gts, metric=metric, at_gt_size=at_gt_size)
    assert np.array_equal(metric.boundary_areas.cpu().numpy(), 3 * want)


def test_ratio_and_whole_image_inference(tmp_path_factory):
    """boundary_ratio sets each image's own width; slide_crop = 0 goes image by image."""
    imgs = images()
    for kw in ({}, {"slide_crop": 0}):
        seg = seg_of(tmp_path_factory, **kw)
        xs = imgs if not kw else [x[:, :40, :48].contiguous() for x in imgs]
        labels = [seg.predict(x[None], None) for x in xs]
        shapes = [tuple(x.shape[-2:]) for x in xs]
        gts = truths(shapes, labels)
        res, metric = seg.evaluate(xs, gts, boundary_ratio=0.03)
        ds = [R.width(s, 0.03) for s in shapes]
        assert ds == ([5, 2] if not kw else [2, 2])
        want = R.boundary_areas_batch([(lab[0].cpu().numpy(), g.numpy()) for lab, g in zip(labels, gts)], ds, K)
        assert np.array_equal(metric.boundary_areas.cpu().numpy(), want) and want[0].sum() > 0


def test_without_the_option_nothing_of_the_boundary_path_runs(tmp_path_factory, monkeypatch):
    from clip_decontamination_amd import _lib, ops
    seg = seg_of(tmp_path_factory)
    imgs = images()
    gts = truths(SHAPES)
    calls = []
    lib = _lib.load()

    class Spy:
        """The loaded library with the boundary entries counted."""
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("sg_boundary"):
                calls.append(name)
            return fn

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    for name in ("boundary_accumulate", "boundary_band_flat", "boundary_band"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    res, metric = seg.evaluate(imgs, gts)
    assert calls == [] and type(metric).__name__ == "IoUMetric" and "BIoU" not in res
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    seg.evaluate(imgs, gts, boundary_px=PX)                                              # the spy does see the option's calls
    assert "sg_boundary_accumulate" in calls and "sg_boundary_band" not in calls


def test_refusals(tmp_path_factory):
    from clip_decontamination_amd.metrics import IoUMetric
    seg = seg_of(tmp_path_factory)
    imgs = images()
    gts = truths(SHAPES)
    with pytest.raises(TypeError, match="BoundaryIoUMetric"):
        seg.evaluate(imgs, gts, metric=IoUMetric(num_classes=K), boundary_px=PX)
    for kw, word in ((dict(boundary_px=0), "boundary_px"), (dict(boundary_px=2.5), "boundary_px"), (dict(boundary_ratio=-1), "boundary_ratio")):
        with pytest.raises(ValueError, match=word):
            seg.evaluate(imgs, gts, **kw)
    seg.tile_group = "world"
    try:
        with pytest.raises(ValueError, match="tile_group sharding is not supported"):
            seg.evaluate(imgs, gts, boundary_px=PX)
    finally:
        seg.tile_group = None
