"""``resize_head="fused"`` behind the drop-in classes and SegPipeline (f32 tiny-8 tower, synthetic weights, crop 32, stride 16, images of
about 72 x 88, Q = 8 -> K = 5 and Q = 65 -> K = 40): ``predict_many(..., ori_shapes=)``, ``predict_topk``, ``segment_scene(ori_shape=)``
and ``evaluate(at_gt_size=True)`` call the resized heads once per flush group, stitch no canvas and equal the ops on
SegPipeline.tile_logits byte for byte; with the default ``resize_head`` every call is today's route byte for byte; PAMR, ``tile_group``
and ``at_gt_size=False`` behave as before."""
import numpy as np
import pytest
import torch

import iou_reference as IR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(72, 88), (48, 64), (70, 91)]
ORIS = [(165, 201), (48, 64), (31, 40)]                                   # an upscale (448 -> 1024's ratio), an image that keeps its size, a downscale
QK = {8: 5, 65: 40}
CANVAS_OPS = ("stitch", "stitch_multi", "resize_bilinear", "postprocess", "postprocess_multi")
HEAD_OPS = ("label_head", "label_head_multi", "topk_head", "topk_head_multi", "label_head_resized", "label_head_resized_multi",
            "topk_head_resized", "topk_head_resized_multi")
_SEG = {}


class Sample:
    def __init__(self, meta):
        self.metainfo, self.data = meta, {}

    def set_data(self, d):
        self.data.update(d)


def class_file(tmp_path_factory, Q):
    K = QK[Q]
    lines, q = [], 0
    for c in range(K):
        k = 2 if c < Q - K else 1
        lines.append(",".join(f"thing{q + i}" for i in range(k)))
        q += k
    path = tmp_path_factory.getbasetemp() / f"resized_cls_{Q}.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def seg_of(tmp_path_factory, Q, cls_name="SegmentorEx", **kw):
    key = (Q, cls_name, tuple(sorted(kw.items())))
    if key not in _SEG:
        import segearth_segmentor
        import segmentor
        cls = segmentor.SegmentorEx if cls_name == "SegmentorEx" else segearth_segmentor.Segmentor
        args = dict(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path=class_file(tmp_path_factory, Q),
                    device=torch.device(DEV), precision="f32", synthetic_ok=True, prob_thd=0.05, bg_idx=3, apply_sim_feat_up=False,
                    slide_crop=32, slide_stride=16)
        args.update(kw)
        _SEG[key] = cls(**args)
    return _SEG[key]


def images():
    return [torch.from_numpy(np.random.default_rng(40 + i).standard_normal((3,) + hw).astype(np.float32)).to(DEV)
            for i, hw in enumerate(SHAPES)]


def count_calls(monkeypatch, calls):
    """Counts every head / canvas op and every flush group."""
    from clip_decontamination_amd import ops
    from clip_decontamination_amd.pipeline import SegPipeline

    def counted(fn, name):
        def wrap(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)
        return wrap

    for name in CANVAS_OPS + HEAD_OPS:
        monkeypatch.setattr(ops, name, counted(getattr(ops, name), name))
    monkeypatch.setattr(SegPipeline, "_packed_tile_logits", counted(SegPipeline._packed_tile_logits, "flush_groups"))


def tiles_of(seg, x):
    pipe = seg._pipeline()
    H, W, stride, crop, wins, tile_hw, pad_tl, up_hw, grid = pipe._geometry(x, 16, 32)
    tl = pipe.tile_logits(x, wins, tile_hw, grid_of_tiles=grid)
    return tl, torch.tensor(wins, dtype=torch.int32), up_hw, pad_tl, (H, W)


def labels_on_tile_logits(seg, x, ori):
    from clip_decontamination_amd import ops
    return ops.label_head_resized(*tiles_of(seg, x), ori, seg.query_idx, seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx,
                                  form="direct")


def topk_on_tile_logits(seg, x, ori, k):
    from clip_decontamination_amd import ops
    return ops.topk_head_resized(*tiles_of(seg, x), ori, seg.query_idx, seg.num_classes, seg.logit_scale, k, form="direct")


def same(a, b):
    return torch.equal(a[0], b[0]) and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def canvas_labels(seg, x, ori):
    """Today's route from public pieces: forward_slide at ori_shape -> post-process."""
    from clip_decontamination_amd import ops
    logits = seg.forward_slide(x[None], [dict(ori_shape=ori)], 16, 32)[0]
    return ops.postprocess(logits, seg.query_idx, seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx)


@pytest.mark.parametrize("one_image_per_group", [False, True], ids=["one-group", "group-per-image"])
@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_fused_is_one_launch_per_flush_group_without_a_canvas(tmp_path_factory, monkeypatch, Q, cls_name, one_image_per_group):
    from clip_decontamination_amd.pipeline import SegPipeline
    seg = seg_of(tmp_path_factory, Q, cls_name, resize_head="fused")
    imgs, k = images(), 3
    want_l = [labels_on_tile_logits(seg, x, o) for x, o in zip(imgs, ORIS)]
    want_k = [topk_on_tile_logits(seg, x, o, k) for x, o in zip(imgs, ORIS)]
    if one_image_per_group:                                                 # the unresized image's group keeps today's kernels and bytes
        from clip_decontamination_amd import ops
        monkeypatch.setattr(SegPipeline, "flush_bytes", 1)
        want_l[1] = seg.predict_many(imgs[1:2], None)[0]
        want_k[1] = ops.topk_head(*tiles_of(seg, imgs[1]), seg.query_idx, seg.num_classes, seg.logit_scale, k)
    calls = {}
    count_calls(monkeypatch, calls)
    labels = seg.predict_many(imgs, None, ori_shapes=ORIS)
    n = calls.pop("flush_groups")
    assert n == (3 if one_image_per_group else 1)
    if not one_image_per_group:
        assert calls == {"label_head_resized_multi": 1}
    elif Q > 64:                                                            # the group of the unresized image keeps today's kernel
        assert calls == {"label_head_resized_multi": 2, "label_head_multi": 1}
    else:
        assert calls == {"label_head_resized_multi": 2, "stitch_multi": 1, "postprocess_multi": 1}
    for got, want, o in zip(labels, want_l, ORIS):
        assert got.shape == (1,) + o and got.dtype == torch.int64 and torch.equal(got, want)
    calls.clear()
    out = seg.predict_topk(imgs, k, [Sample(dict(ori_shape=o)) for o in ORIS])
    n = calls.pop("flush_groups")
    assert calls == ({"topk_head_resized_multi": 2, "topk_head_multi": 1} if one_image_per_group else {"topk_head_resized_multi": 1})
    for ds, want, o in zip(out, want_k, ORIS):
        got = (ds.data["seg_topk_classes"].data, ds.data["seg_topk_probs"].data)
        assert got[0].shape == (k,) + o and same(got, want)
        pred = torch.where(got[1][0] < seg.prob_thd, torch.full_like(got[0][0], seg.bg_idx), got[0][0]).long()[None]
        assert torch.equal(ds.data["pred_sem_seg"].data, pred)


@pytest.mark.parametrize("Q", [8, 65])
def test_segment_scene_at_another_ori_shape(tmp_path_factory, monkeypatch, Q):
    seg, base = seg_of(tmp_path_factory, Q, resize_head="fused"), seg_of(tmp_path_factory, Q)
    x, ori = images()[0], ORIS[0]
    want_l, want_k = labels_on_tile_logits(seg, x, ori), topk_on_tile_logits(seg, x, ori, 2)
    today = canvas_labels(base, x, ori)
    calls = {}
    count_calls(monkeypatch, calls)
    assert torch.equal(seg._pipeline().segment_scene(x, 16, 32, ori_shape=ori), want_l)
    assert same(seg._pipeline().segment_scene(x, 16, 32, topk=2, ori_shape=ori), want_k)
    assert calls == {"label_head_resized": 1, "topk_head_resized": 1}
    calls.clear()
    got = base._pipeline().segment_scene(x, 16, 32, ori_shape=ori)           # the default: stitch, resize, post-process
    assert calls == {"stitch": 1, "resize_bilinear": 1, "postprocess": 1} and torch.equal(got, today[1])
    from clip_decontamination_amd import ops
    assert same(base._pipeline().segment_scene(x, 16, 32, topk=2, ori_shape=ori), ops.topk_from_probs(today[0], base.query_idx, 2))
    own = tuple(x.shape[-2:])                                                # the image's own size: nothing changes
    assert torch.equal(seg._pipeline().segment_scene(x, 16, 32, ori_shape=own), base._pipeline().segment_scene(x, 16, 32))


def host_confusion(labels, gts, K):
    """The table of tests/iou_reference.py over the images of a call."""
    return sum(IR.confusion_table(lab.cpu().numpy(), gt.numpy(), K) for lab, gt in zip(labels, gts))


@pytest.mark.parametrize("Q", [8, 65])
def test_evaluate_at_the_truth_maps_size(tmp_path_factory, monkeypatch, Q):
    """Both routes count their own labels at the truth's size; the two tables are equal when the labels agree and otherwise differ by
    exactly the pixels where the labels differ (each table is checked against a host count of its route's labels)."""
    fused, base = seg_of(tmp_path_factory, Q, resize_head="fused"), seg_of(tmp_path_factory, Q)
    K = QK[Q]
    imgs = images()
    rng = np.random.default_rng(5)
    gts = [torch.from_numpy(rng.integers(0, K, o).astype(np.uint8)) for o in ORIS]
    gts[0][:7] = 255
    with pytest.raises(ValueError, match="has shape"):
        fused.evaluate(imgs, gts)
    with pytest.raises(ValueError, match="has shape"):
        base.evaluate(imgs, gts, at_gt_size=False)
    lab_f = fused.predict_many(imgs, None, ori_shapes=ORIS)
    lab_c = base.predict_many(imgs, None, ori_shapes=ORIS)
    for lc, x, o in zip(lab_c, imgs, ORIS):
        assert torch.equal(lc, canvas_labels(base, x, o)[1])                 # the default route is today's, byte for byte
    calls = {}
    count_calls(monkeypatch, calls)
    res_f, m_f = fused.evaluate(imgs, gts, at_gt_size=True)
    assert calls == {"flush_groups": 1, "label_head_resized_multi": 1}
    calls.clear()
    res_c, m_c = base.evaluate(imgs, gts, at_gt_size=True)
    assert calls.get("label_head_resized_multi", 0) == 0 and calls.get("stitch_multi", 0) == 1
    t_f, t_c = m_f.confusion.cpu().numpy(), m_c.confusion.cpu().numpy()
    assert np.array_equal(t_f, host_confusion(lab_f, gts, K)) and np.array_equal(t_c, host_confusion(lab_c, gts, K))
    assert t_f.sum() == t_c.sum() == sum(int((g != 255).sum()) for g in gts)
    differ = sum(int((a != b).sum()) for a, b in zip(lab_f, lab_c))
    print(f"Q={Q}: {differ} of {sum(a.numel() for a in lab_f)} labels differ between the routes")
    if differ == 0:
        assert np.array_equal(t_f, t_c)
    assert np.abs(t_f - t_c).sum() <= 2 * differ
    same_size = [torch.from_numpy(rng.integers(0, K, hw).astype(np.uint8)) for hw in SHAPES]
    a, b = fused.evaluate(imgs, same_size, at_gt_size=True)[1], base.evaluate(imgs, same_size)[1]
    assert torch.equal(a.confusion, b.confusion)                             # nothing to resize: today's route and bytes


@pytest.mark.parametrize("Q", [8, 65])
def test_the_default_is_todays_route(tmp_path_factory, monkeypatch, Q):
    """``resize_head`` left alone: no resized head is called, and the results are the canvas route's bytes."""
    from clip_decontamination_amd import ops
    seg = seg_of(tmp_path_factory, Q)
    assert seg.resize_head == "canvas" and seg._pipeline().resize_head == "canvas" and not seg._pipeline().fused_resize_head()
    imgs, k = images(), 3
    want = [canvas_labels(seg, x, o) for x, o in zip(imgs, ORIS)]
    calls = {}
    count_calls(monkeypatch, calls)
    labels = seg.predict_many(imgs, None, ori_shapes=ORIS)
    out = seg.predict_topk(imgs, k, [Sample(dict(ori_shape=o)) for o in ORIS])
    assert not any("resized" in name for name in calls), calls
    for got, ds, (p, l) in zip(labels, out, want):
        assert torch.equal(got, l)
        assert same((ds.data["seg_topk_classes"].data, ds.data["seg_topk_probs"].data), ops.topk_from_probs(p, seg.query_idx, k))
    plain = seg.predict_many(imgs, None)
    assert all(torch.equal(a, b) for a, b in zip(plain, seg.predict_many(imgs, None, ori_shapes=[None] * 3)))


def test_pamr_tile_group_and_bad_options(tmp_path_factory, monkeypatch):
    """PAMR keeps the canvas route whatever resize_head says; tile_group stays refused; an unknown resize_head is refused."""
    kw = dict(pamr_steps=4, pamr_stride=(8, 16))
    fused, base = seg_of(tmp_path_factory, 8, resize_head="fused", **kw), seg_of(tmp_path_factory, 8, **kw)
    imgs = images()
    want = base.predict_many(imgs, None, ori_shapes=ORIS)
    want_k = base.predict_topk(imgs[:1], 2, [Sample(dict(ori_shape=ORIS[0]))])[0]
    calls = {}
    count_calls(monkeypatch, calls)
    got = fused.predict_many(imgs, None, ori_shapes=ORIS)
    got_k = fused.predict_topk(imgs[:1], 2, [Sample(dict(ori_shape=ORIS[0]))])[0]
    assert not any("resized" in name for name in calls) and calls.get("stitch_multi", 0) >= 2
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(got_k.data["seg_topk_classes"].data, want_k.data["seg_topk_classes"].data)
    assert torch.equal(fused._pipeline().segment_scene(imgs[0], 16, 32, ori_shape=ORIS[0]), want[0])
    assert not torch.equal(want[0], seg_of(tmp_path_factory, 8).predict_many(imgs[:1], None, ori_shapes=ORIS[:1])[0]), "PAMR changed nothing"
    plain = seg_of(tmp_path_factory, 8, resize_head="fused")
    with pytest.raises(ValueError, match="under tile_group sharding is not built"):
        plain._pipeline().segment_scene(imgs[0], 16, 32, group="world", ori_shape=ORIS[0])
    with pytest.raises(ValueError, match="top-k under tile_group sharding is not built"):
        plain._pipeline().segment_scene(imgs[0], 16, 32, group="world", topk=2, ori_shape=ORIS[0])
    sharded = seg_of(tmp_path_factory, 8, resize_head="fused", tile_group="world")
    with pytest.raises(ValueError, match="top-k under tile_group sharding is not built"):
        sharded.predict_topk(imgs[:1], 2, [Sample(dict(ori_shape=ORIS[0]))])
    with pytest.raises(ValueError, match="tile_group"):
        sharded.evaluate(imgs[:1], [torch.zeros(ORIS[0], dtype=torch.uint8)], at_gt_size=True)
    with pytest.raises(ValueError, match="resize_head must be one of"):
        seg_of(tmp_path_factory, 8, resize_head="auto")
    with pytest.raises(ValueError, match="ori_shapes goes with data_samples=None"):
        plain.predict_many(imgs[:1], [Sample(dict(ori_shape=ORIS[0]))], ori_shapes=ORIS[:1])
