"""min_region behind the drop-in classes and SegPipeline (f32 tiny-8 tower, synthetic weights, the scenes and class file of
tests/test_gpu_area_route.py: 40 x 150 and 47 x 61, crop 32, stride 16, Q = 8 -> K = 5).

An instance without the option supplies the labels; the same call on an instance with min_region must return
tests/sieve_reference.py applied to those labels, byte for byte, on every route (canvas, fused label head, fused probability head,
with area_thd, at another ori_shape through both resize heads, whole-image inference), and leave seg_logits as they are.  min_region
is chosen from the unsieved labels so that on every image some region is small and some region is kept."""
import numpy as np
import pytest
import torch

import sieve_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(40, 150), (47, 61)]
Q, K, BG = 8, 5, 3
_SEG = {}


class Sample:
    def __init__(self, meta):
        self.metainfo, self.data = meta, {}

    def set_data(self, d):
        self.data.update(d)


def class_file(tmp_path_factory):
    """One class per line, synonyms separated by commas: the first Q - K classes get two names."""
    lines, q = [], 0
    for c in range(K):
        k = 2 if c < Q - K else 1
        lines.append(",".join(f"thing{q + i}" for i in range(k)))
        q += k
    path = tmp_path_factory.getbasetemp() / "sieve_cls.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def seg_of(tmp_path_factory, cls_name="SegmentorEx", **kw):
    key = (cls_name, tuple(sorted(kw.items())))
    if key not in _SEG:
        import segearth_segmentor
        import segmentor
        cls = segmentor.SegmentorEx if cls_name == "SegmentorEx" else segearth_segmentor.Segmentor
        args = dict(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path=class_file(tmp_path_factory),
                    device=torch.device(DEV), precision="f32", synthetic_ok=True, prob_thd=0.05, bg_idx=BG, apply_sim_feat_up=False,
                    slide_crop=32, slide_stride=16)
        args.update(kw)
        _SEG[key] = cls(**args)
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


def choose_min_region(labels, connectivity):
    """The smallest min_region that makes the smallest regions of every image small while every image keeps a region: one more than the
    largest of the images' smallest region areas.  Asserted, so a case that would show nothing fails instead of passing."""
    areas = []
    for lab in labels:
        root = R.regions(lab[0].cpu().numpy(), connectivity)
        a = np.bincount(root.reshape(-1))
        areas.append(a[a > 0])
    m = int(max(a.min() for a in areas)) + 1
    for a in areas:
        assert (a < m).any() and (a >= m).any(), f"min_region {m} splits nothing: region areas {sorted(a.tolist())}"
    return m


def reference(labels, m, connectivity, fill):
    """tests/sieve_reference.py on device label maps [1,H,W] -> the same, on the device."""
    out = [torch.from_numpy(R.sieve(lab[0].cpu().numpy(), m, connectivity, fill, BG))[None].to(DEV) for lab in labels]
    assert any(not torch.equal(a, b) for a, b in zip(out, labels)), "the sieve moved no label: the case would show nothing"
    return out


def same_samples(got, base, want_labels):
    for g, b, w in zip(got, base, want_labels):
        assert set(g.data) == {"seg_logits", "pred_sem_seg"}
        assert g.data["seg_logits"].data.cpu().numpy().tobytes() == b.data["seg_logits"].data.cpu().numpy().tobytes()   # untouched
        lab = g.data["pred_sem_seg"].data
        assert lab.dtype == torch.int64 and lab.shape == w.shape and torch.equal(lab, w)


@pytest.mark.parametrize("connectivity,fill", [(4, "neighbour"), (8, "bg")])
@pytest.mark.parametrize("head", ["canvas", "fused"])
@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
def test_every_call_returns_the_sieved_labels(tmp_path_factory, cls_name, head, connectivity, fill):
    from clip_decontamination_amd import ops
    kw = dict(label_head=head, prob_head=head)
    base = seg_of(tmp_path_factory, cls_name, **kw)
    imgs = images()
    plain = base.predict_many(imgs)
    m = choose_min_region(plain, connectivity)
    seg = seg_of(tmp_path_factory, cls_name, min_region=m, region_connectivity=connectivity, region_fill=fill, **kw)
    pipe = seg._pipeline()
    assert pipe.fused_label_head() == (head == "fused") and pipe.fused_prob_head() == (head == "fused")
    assert pipe.tail_route("labels") == base._pipeline().tail_route("labels")          # the route is what it is without the option
    want = reference(plain, m, connectivity, fill)
    # labels only: predict, predict_many, segment_scene
    for x, p, w in zip(imgs, plain, want):
        assert torch.equal(base.predict(x[None], None), p)
        assert torch.equal(seg.predict(x[None], None), w)
        assert torch.equal(pipe.segment_scene(x, 16, 32), w)
    got = seg.predict_many(imgs)
    assert all(torch.equal(g, w) and g.dtype == torch.int64 for g, w in zip(got, want))
    # data samples: pred_sem_seg sieved, seg_logits as without the option
    metas = [dict(ori_shape=tuple(x.shape[-2:])) for x in imgs]
    base_ds = base.predict_many(imgs, [Sample(mt) for mt in metas])
    assert all(torch.equal(d.data["pred_sem_seg"].data, p) for d, p in zip(base_ds, plain))
    same_samples(seg.predict_many(imgs, [Sample(mt) for mt in metas]), base_ds, want)
    same_samples([seg.predict(x[None], [Sample(mt)])[0] for x, mt in zip(imgs, metas)], base_ds, want)
    p_, l_ = pipe.segment_scene(imgs[1], 16, 32, want_probs=True)
    assert torch.equal(l_, want[1]) and torch.equal(p_, base_ds[1].data["seg_logits"].data)
    # evaluate counts the sieved labels
    gts = [torch.from_numpy(np.random.default_rng(7 + i).integers(0, K, hw).astype(np.uint8)) for i, hw in enumerate(SHAPES)]
    _, metric = seg.evaluate(imgs, gts)
    table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=DEV)
    for lab, g in zip(want, gts):
        ops.confusion_accumulate(lab, g.to(DEV), table, K)
    assert torch.equal(metric.confusion.to(DEV), table)
    _, metric0 = base.evaluate(imgs, gts)
    assert not torch.equal(metric0.confusion.to(DEV), table)


@pytest.mark.parametrize("head", ["canvas", "fused"])
def test_after_area_thd(tmp_path_factory, head):
    """area_thd first (its own two decisions), then the sieve on its labels."""
    kw = dict(label_head=head, prob_head=head, area_thd=0.12)
    base = seg_of(tmp_path_factory, **kw)
    imgs = images()
    plain = base.predict_many(imgs)
    m = choose_min_region(plain, 4)
    seg = seg_of(tmp_path_factory, min_region=m, **kw)
    want = reference(plain, m, 4, "neighbour")
    assert all(torch.equal(g, w) for g, w in zip(seg.predict_many(imgs), want))
    assert all(torch.equal(seg.predict(x[None], None), w) for x, w in zip(imgs, want))
    metas = [dict(ori_shape=tuple(x.shape[-2:])) for x in imgs]
    same_samples(seg.predict_many(imgs, [Sample(mt) for mt in metas]), base.predict_many(imgs, [Sample(mt) for mt in metas]), want)


@pytest.mark.parametrize("resize_head", ["canvas", "fused"])
def test_at_another_ori_shape(tmp_path_factory, resize_head):
    """The sieve runs at ori_shape, after the resize, whichever head resizes."""
    from clip_decontamination_amd import ops
    oris = [(33, 170), SHAPES[1]]
    base = seg_of(tmp_path_factory, resize_head=resize_head)
    imgs = images()
    plain = base.predict_many(imgs, None, ori_shapes=oris)
    assert [tuple(p.shape[-2:]) for p in plain] == oris
    m = choose_min_region(plain, 8)
    seg = seg_of(tmp_path_factory, resize_head=resize_head, min_region=m, region_connectivity=8)
    want = reference(plain, m, 8, "neighbour")
    assert all(torch.equal(g, w) for g, w in zip(seg.predict_many(imgs, None, ori_shapes=oris), want))
    assert torch.equal(seg._pipeline().segment_scene(imgs[0], 16, 32, ori_shape=oris[0]), want[0])
    base_ds = base.predict_many(imgs, [Sample(dict(ori_shape=o)) for o in oris])
    same_samples(seg.predict_many(imgs, [Sample(dict(ori_shape=o)) for o in oris]), base_ds, want)
    same_samples([seg.predict(imgs[0][None], [Sample(dict(ori_shape=oris[0]))])[0]], base_ds[:1], want[:1])
    gts = [torch.from_numpy(np.random.default_rng(3 + i).integers(0, K, hw).astype(np.uint8)) for i, hw in enumerate(oris)]
    _, metric = seg.evaluate(imgs, gts, at_gt_size=True)
    table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=DEV)
    for lab, g in zip(want, gts):
        ops.confusion_accumulate(lab, g.to(DEV), table, K)
    assert torch.equal(metric.confusion.to(DEV), table)


def test_whole_image_inference_and_pamr(tmp_path_factory):
    imgs = images()
    x = imgs[1][:, :40, :48].contiguous()
    for kw, xs in ((dict(slide_crop=0), [x]), (dict(pamr_steps=2, pamr_stride=(8, 16)), imgs)):
        base = seg_of(tmp_path_factory, "Segmentor", **kw)
        plain = [base.predict(v[None], None) for v in xs]
        m = choose_min_region(plain, 4)
        seg = seg_of(tmp_path_factory, "Segmentor", min_region=m, region_fill="bg", **kw)
        want = reference(plain, m, 4, "bg")
        assert all(torch.equal(seg.predict(v[None], None), w) for v, w in zip(xs, want))
        assert all(torch.equal(g, w) for g, w in zip(seg.predict_many(xs), want))
        metas = [dict(ori_shape=tuple(v.shape[-2:])) for v in xs]
        base_ds = [base.predict(v[None], [Sample(mt)])[0] for v, mt in zip(xs, metas)]
        same_samples([seg.predict(v[None], [Sample(mt)])[0] for v, mt in zip(xs, metas)], base_ds, want)


def test_refusals(tmp_path_factory):
    from clip_decontamination_amd import pipeline as P
    seg = seg_of(tmp_path_factory, min_region=4)
    x = images()[1]
    for fn in (lambda: seg_of(tmp_path_factory, tile_group="world", min_region=4),
               lambda: seg._pipeline().segment_scene(x, 16, 32, group="world")):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == P.SIEVE_TILE_GROUP
    for fn in (lambda: seg.predict_topk([x], 2), lambda: seg._pipeline().segment_scene(x, 16, 32, topk=2),
               lambda: seg._pipeline().segment_scenes([x], 16, 32, topk=2)):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == P.SIEVE_TOPK
    for kw, word in ((dict(min_region=0), "min_region"), (dict(min_region=1.5), "min_region"), (dict(min_region=4, region_connectivity=6), "connectivity"),
                     (dict(min_region=4, region_fill="nearest"), "fill")):
        with pytest.raises(ValueError, match=word):
            seg_of(tmp_path_factory, **kw)
    seg.min_region = 0                                                          # the pipeline is rebuilt per call: attribute edits are checked too
    with pytest.raises(ValueError, match="min_region"):
        seg.predict(x[None], None)
    seg.min_region = 4


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
def test_min_region_none_is_the_instance_without_the_keyword(tmp_path_factory, cls_name):
    base = seg_of(tmp_path_factory, cls_name)
    off = seg_of(tmp_path_factory, cls_name, min_region=None, region_connectivity=8, region_fill="bg")
    one = seg_of(tmp_path_factory, cls_name, min_region=1)                      # min_region = 1 changes nothing either
    imgs = images()
    assert off.min_region is None and off._pipeline().min_region is None
    for o in ([tuple(x.shape[-2:]) for x in imgs], [(33, 170), SHAPES[1]]):
        a = base.predict_many(imgs, [Sample(dict(ori_shape=s)) for s in o])
        for other in (off, one):
            b = other.predict_many(imgs, [Sample(dict(ori_shape=s)) for s in o])
            for da, db in zip(a, b):
                assert torch.equal(da.data["seg_logits"].data, db.data["seg_logits"].data)
                assert torch.equal(da.data["pred_sem_seg"].data, db.data["pred_sem_seg"].data)
    for x in imgs:
        assert torch.equal(base.predict(x[None], None), off.predict(x[None], None))
        assert torch.equal(base.predict(x[None], None), one.predict(x[None], None))
    assert all(torch.equal(a, b) for a, b in zip(base.predict_many(imgs), off.predict_many(imgs)))
    assert all(torch.equal(a, b) for a, b in zip(base.predict_many(imgs), one.predict_many(imgs)))
