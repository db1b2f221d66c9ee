"""PAMR behind the drop-in classes and SegPipeline (f32 tiny-8 tower, synthetic weights, scenes of 40 x 150 and 47 x 61).  With
``pamr_steps=10`` every tail that returns labels or probabilities must equal, byte for byte, the composition made from public pieces:
forward_slide (the unrefined logits, resized to ori_shape) -> ops.pamr under the image (resized likewise) -> ops.postprocess, whatever
label_head / prob_head say.  With ``pamr_steps=0`` every result equals an instance built without the kwargs.

The u8 scenes hold values up to 232 only: from 233 on the tower's u8 ingest corrects channel 2's (u - mean) / std to the nearest f32
(csrc/patchify.hip) while sg_extract_tiles, which makes the guidance, keeps the plain f32 quotient; below that both are the plain quotient,
which is also what torch computes, so a float image with the same bytes exists."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS, DIL = 10, (8, 16)
SHAPES = [(40, 150), (47, 61)]
QK = {8: 5, 65: 40}
HEADS = ("auto", "fused", "canvas")
_SEG = {}


class Sample:
    def __init__(self, meta):
        self.metainfo, self.data = meta, {}

    def set_data(self, d):
        self.data.update(d)


def class_file(tmp_path_factory, Q):
    """One class per line, synonyms separated by commas: the first Q - K classes get two names."""
    K = QK[Q]
    lines, q = [], 0
    for c in range(K):
        k = 2 if c < Q - K else 1
        lines.append(",".join(f"thing{q + i}" for i in range(k)))
        q += k
    assert q == Q
    path = tmp_path_factory.getbasetemp() / f"pamr_cls_{Q}.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def seg_of(tmp_path_factory, Q, head=None, steps=None, cls_name="SegmentorEx", **kw):
    """A drop-in instance, cached per setting; head=None / steps=None: built without those kwargs."""
    key = (Q, head, steps, cls_name, tuple(sorted(kw.items())))
    if key not in _SEG:
        import segearth_segmentor
        import segmentor
        cls = segmentor.SegmentorEx if cls_name == "SegmentorEx" else segearth_segmentor.Segmentor
        if head is not None:
            kw.update(label_head=head, prob_head=head)
        if steps is not None:
            kw.update(pamr_steps=steps, pamr_stride=DIL)
        args = dict(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path=class_file(tmp_path_factory, Q),
                    device=torch.device(DEV), precision="f32", synthetic_ok=True, prob_thd=0.05, bg_idx=3, apply_sim_feat_up=False,
                    slide_crop=32, slide_stride=16)
        args.update(kw)
        _SEG[key] = cls(**args)
    return _SEG[key]


def scene_u8(hw, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 233, hw + (3,), dtype=np.uint8)).to(DEV)


def as_float(u8):
    from clip_decontamination_amd import weights as Wt
    mean = torch.tensor(Wt.PIXEL_MEAN, device=DEV).view(3, 1, 1)
    std = torch.tensor(Wt.PIXEL_STD, device=DEV).view(3, 1, 1)
    return ((u8.permute(2, 0, 1).float() - mean) / std).contiguous()


def images():
    return [as_float(scene_u8(hw, 20 + i)) for i, hw in enumerate(SHAPES)]


def compose(base, x, ori=None, steps=STEPS):
    """The public pieces: unrefined logits at ori_shape -> PAMR under the image at that size -> post-process.  x f32 [3,H,W]."""
    from clip_decontamination_amd import ops
    ori = tuple(x.shape[-2:]) if ori is None else tuple(ori)
    logits = base.forward_slide(x[None], [dict(ori_shape=ori)], 16, 32)[0]
    guide = x if ori == tuple(x.shape[-2:]) else ops.resize_bilinear(x, ori)
    refined = ops.pamr(logits, guide, steps, DIL)
    return ops.postprocess(refined, base.query_idx, base.num_classes, base.logit_scale, base.prob_thd, base.bg_idx)


def sample_out(ds):
    return ds.data["seg_logits"].data, ds.data["pred_sem_seg"].data


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("Q", [8, 65])
def test_predict(tmp_path_factory, Q, head):
    base, seg = seg_of(tmp_path_factory, Q), seg_of(tmp_path_factory, Q, head, STEPS)
    for x in images():
        want_p, want_l = compose(base, x)
        got_l = seg.predict(x[None], None)
        assert got_l.dtype == torch.int64 and torch.equal(got_l, want_l)
        got_p, got_l = sample_out(seg.predict(x[None], [Sample(dict(ori_shape=tuple(x.shape[-2:])))])[0])
        assert torch.equal(got_p, want_p) and torch.equal(got_l, want_l)
        plain = base.predict(x[None], None)
        assert not torch.equal(plain, want_l), "PAMR changed no label: the case would show nothing"
    x = images()[0]
    ori = (33, 170)                                                     # another ori_shape: resize, then PAMR under the resized image
    want_p, want_l = compose(base, x, ori)
    got_p, got_l = sample_out(seg.predict(x[None], [Sample(dict(ori_shape=ori))])[0])
    assert got_p.shape[1:] == ori and torch.equal(got_p, want_p) and torch.equal(got_l, want_l)


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("Q", [8, 65])
def test_predict_many_and_evaluate(tmp_path_factory, Q, head):
    from clip_decontamination_amd import ops
    base, seg = seg_of(tmp_path_factory, Q), seg_of(tmp_path_factory, Q, head, STEPS)
    imgs = images() + [images()[0]]
    oris = [tuple(imgs[0].shape[-2:]), tuple(imgs[1].shape[-2:]), (33, 170)]      # the third sample has another ori_shape
    want = [compose(base, x, o) for x, o in zip(imgs, oris)]
    out = seg.predict_many(imgs, [Sample(dict(ori_shape=o)) for o in oris])
    for ds, (p, l) in zip(out, want):
        got_p, got_l = sample_out(ds)
        assert torch.equal(got_p, p) and torch.equal(got_l, l)
    labels = seg.predict_many(imgs[:2])
    assert all(torch.equal(a, w[1]) for a, w in zip(labels, want))
    K = seg.num_classes
    rng = np.random.default_rng(5)
    gts = [rng.integers(0, K, tuple(x.shape[-2:])).astype(np.uint8) for x in imgs[:2]]
    _, metric = seg.evaluate(imgs[:2], gts)
    table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=DEV)
    for (_, l), g in zip(want, gts):
        ops.confusion_accumulate(l, torch.from_numpy(g).to(DEV), table, K)
    assert torch.equal(metric.confusion.to(DEV), table) and int(table.sum()) == sum(g.size for g in gts)


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("Q", [8, 65])
def test_segment_scene_u8_and_float(tmp_path_factory, Q, head):
    base, seg = seg_of(tmp_path_factory, Q), seg_of(tmp_path_factory, Q, head, STEPS)
    pipe = seg._pipeline()
    for i, hw in enumerate(SHAPES):
        u8 = scene_u8(hw, 20 + i)
        x = as_float(u8)
        want_p, want_l = compose(base, x)
        assert torch.equal(pipe.segment_scene(x, 16, 32), want_l)
        assert torch.equal(pipe.segment_scene(u8, 16, 32), want_l)               # u8 and float input of one image: equal bytes
        got_p, got_l = pipe.segment_scene(u8, 16, 32, want_probs=True)
        assert torch.equal(got_p, want_p) and torch.equal(got_l, want_l)
    many = pipe.segment_scenes([scene_u8(hw, 20 + i) for i, hw in enumerate(SHAPES)], 16, 32)
    assert all(torch.equal(a, compose(base, x)[1]) for a, x in zip(many, images()))


def test_whole_image_inference(tmp_path_factory):
    """slide_crop <= 0: forward_feature's logits, refined under the image, then post-processed."""
    from clip_decontamination_amd import ops
    base = seg_of(tmp_path_factory, 8, cls_name="Segmentor", slide_crop=0)
    seg = seg_of(tmp_path_factory, 8, "auto", STEPS, cls_name="Segmentor", slide_crop=0)
    x = as_float(scene_u8((40, 48), 31))
    logits = base.forward_feature(x[None], (40, 48))[0]
    want_p, want_l = ops.postprocess(ops.pamr(logits, x, STEPS, DIL), base.query_idx, base.num_classes, base.logit_scale, base.prob_thd, base.bg_idx)
    assert torch.equal(seg.predict(x[None], None), want_l)
    got_p, got_l = sample_out(seg.predict(x[None], [Sample(dict(ori_shape=(40, 48)))])[0])
    assert torch.equal(got_p, want_p) and torch.equal(got_l, want_l)


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_zero_steps_changes_nothing(tmp_path_factory, Q, cls_name):
    base, off = seg_of(tmp_path_factory, Q, cls_name=cls_name), seg_of(tmp_path_factory, Q, None, 0, cls_name=cls_name)
    imgs = images()
    oris = [tuple(imgs[0].shape[-2:]), (50, 70)]
    for x in imgs:
        assert torch.equal(off.predict(x[None], None), base.predict(x[None], None))
    a = off.predict_many(imgs, [Sample(dict(ori_shape=o)) for o in oris])
    b = base.predict_many(imgs, [Sample(dict(ori_shape=o)) for o in oris])
    for da, db in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(sample_out(da), sample_out(db)))
    gts = [np.random.default_rng(6).integers(0, base.num_classes, tuple(x.shape[-2:])).astype(np.uint8) for x in imgs]
    assert torch.equal(off.evaluate(imgs, gts)[1].confusion.cpu(), base.evaluate(imgs, gts)[1].confusion.cpu())
    u8 = scene_u8(SHAPES[1], 21)
    pa, pb = off._pipeline(), base._pipeline()
    assert torch.equal(pa.segment_scene(u8, 16, 32), pb.segment_scene(u8, 16, 32))
    ra, rb = pa.segment_scene(u8, 16, 32, want_probs=True), pb.segment_scene(u8, 16, 32, want_probs=True)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])


def test_tile_group_is_refused_with_the_reason(tmp_path_factory):
    from clip_decontamination_amd.pipeline import SegPipeline
    with pytest.raises(ValueError, match="halo of pamr_steps"):
        seg_of(tmp_path_factory, 8, None, STEPS, tile_group="world")
    seg = seg_of(tmp_path_factory, 8, "auto", STEPS)
    pipe = seg._pipeline()
    with pytest.raises(ValueError, match="halo of pamr_steps"):
        pipe.segment_scene(images()[0], 16, 32, group="world")
    with pytest.raises(ValueError, match="halo of pamr_steps"):
        SegPipeline(seg.net, seg.query_features, seg.query_idx, pamr_steps=STEPS, tile_group="world")
