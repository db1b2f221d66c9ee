"""The top-k head behind the drop-in classes and SegPipeline (f32 tiny-8 tower, synthetic weights, the scenes of
tests/test_gpu_pamr_route.py: 40 x 150 and 47 x 61, crop 32, stride 16, Q = 8 -> K = 5 and Q = 65 -> K = 40).  ``predict_topk`` must equal,
byte for byte, ops.topk_head on SegPipeline.tile_logits of the same image; with PAMR on or another ``ori_shape`` it must equal the
composition from public pieces (forward_slide -> ops.pamr -> ops.postprocess -> ops.topk_from_probs); ``tile_group`` is refused with the
reason; and calls without ``topk`` return what they returned before."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS, DIL = 10, (8, 16)
SHAPES = [(40, 150), (47, 61)]
QK = {8: 5, 65: 40}
KS = {8: (1, 3, 5), 65: (2, 8)}
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
    path = tmp_path_factory.getbasetemp() / f"topk_cls_{Q}.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def seg_of(tmp_path_factory, Q, cls_name="SegmentorEx", **kw):
    """A drop-in instance, cached per setting."""
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


def scene_u8(hw, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 233, hw + (3,), dtype=np.uint8)).to(DEV)


def as_float(u8):
    from clip_decontamination_amd import weights as Wt
    mean = torch.tensor(Wt.PIXEL_MEAN, device=DEV).view(3, 1, 1)
    std = torch.tensor(Wt.PIXEL_STD, device=DEV).view(3, 1, 1)
    return ((u8.permute(2, 0, 1).float() - mean) / std).contiguous()


def images():
    return [as_float(scene_u8(hw, 20 + i)) for i, hw in enumerate(SHAPES)]


def same(a, b):
    """Two (classes, probs) pairs, byte for byte."""
    return a[0].dtype == b[0].dtype == torch.int32 and a[1].dtype == b[1].dtype == torch.float32 and torch.equal(a[0], b[0]) and \
        a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def head_on_tile_logits(seg, x, k):
    """ops.topk_head on SegPipeline.tile_logits of the image."""
    from clip_decontamination_amd import ops
    pipe = seg._pipeline()
    H, W, stride, crop, wins, tile_hw, pad_tl, up_hw, grid = pipe._geometry(x, 16, 32)
    tl = pipe.tile_logits(x, wins, tile_hw, grid_of_tiles=grid)
    return ops.topk_head(tl, torch.tensor(wins, dtype=torch.int32), up_hw, pad_tl, (H, W), seg.query_idx, seg.num_classes, seg.logit_scale, k)


def compose(seg, x, k, ori=None, steps=0):
    """The canvas route from public pieces: logits at ori_shape -> PAMR under the image at that size -> post-process -> sort."""
    from clip_decontamination_amd import ops
    ori = tuple(x.shape[-2:]) if ori is None else tuple(ori)
    logits = seg.forward_slide(x[None], [dict(ori_shape=ori)], 16, 32)[0]
    if steps > 0:
        guide = x if ori == tuple(x.shape[-2:]) else ops.resize_bilinear(x, ori)
        logits = ops.pamr(logits, guide, steps, DIL)
    probs, _ = ops.postprocess(logits, seg.query_idx, seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx)
    return ops.topk_from_probs(probs, seg.query_idx, k)


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_predict_topk_is_the_head_on_the_tile_logits(tmp_path_factory, Q, cls_name):
    seg = seg_of(tmp_path_factory, Q, cls_name)
    imgs = images()
    pipe = seg._pipeline()
    for k in KS[Q]:
        want = [head_on_tile_logits(seg, x, k) for x in imgs]
        got = seg.predict_topk(imgs, k)
        assert len(got) == len(imgs)
        for g, w, x in zip(got, want, imgs):
            assert g[0].shape == g[1].shape == (k,) + tuple(x.shape[-2:]) and same(g, w)
        many = pipe.segment_scenes(imgs, 16, 32, topk=k)
        assert all(same(g, w) for g, w in zip(many, want))
        for x, w in zip(imgs, want):
            assert same(pipe.segment_scene(x, 16, 32, topk=k), w)
        batch = seg.predict_topk(imgs[0][None], k)                            # a [B,3,H,W] batch, as predict_many takes
        assert len(batch) == 1 and same(batch[0], want[0])
    u8 = scene_u8(SHAPES[1], 21)
    assert same(pipe.segment_scene(u8, 16, 32, topk=KS[Q][0]), head_on_tile_logits(seg, as_float(u8), KS[Q][0]))


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
def test_data_samples(tmp_path_factory, cls_name):
    """seg_topk_classes / seg_topk_probs are the planes, pred_sem_seg is plane 0 with prob_thd -> bg_idx applied (int64 [1,H,W]) and equals
    what predict's labels-only tail gives on the fused label head; no seg_logits is set."""
    Q, k = 65, 5
    seg = seg_of(tmp_path_factory, Q, cls_name)
    imgs = images()
    was = seg.prob_thd
    try:
        for x in imgs:
            want = head_on_tile_logits(seg, x, k)
            seg.prob_thd = thd = float(want[1][0].median())                  # both branches of the threshold are taken
            ds = seg.predict_topk([x], k, [Sample(dict(ori_shape=tuple(x.shape[-2:])))])[0]
            assert set(ds.data) == {"seg_topk_classes", "seg_topk_probs", "pred_sem_seg"}
            assert same((ds.data["seg_topk_classes"].data, ds.data["seg_topk_probs"].data), want)
            pred = ds.data["pred_sem_seg"].data
            assert pred.dtype == torch.int64 and pred.shape == (1,) + tuple(x.shape[-2:])
            below = want[1][0] < torch.tensor(thd, dtype=torch.float32, device=DEV)
            assert bool(below.any()) and bool((~below).any())
            assert torch.equal(pred, torch.where(below, torch.full_like(want[0][0], 3), want[0][0]).long()[None])
            assert torch.equal(pred, seg.predict(x[None], None))             # Q = 65: the fused label head (label_head="auto")
    finally:
        seg.prob_thd = was


@pytest.mark.parametrize("Q", [8, 65])
def test_fallback_to_the_canvas_route(tmp_path_factory, Q):
    """PAMR on, or an ori_shape of another size: the canvas, the resize, PAMR, post-process, then ops.topk_from_probs."""
    k = KS[Q][-1]
    base, seg = seg_of(tmp_path_factory, Q), seg_of(tmp_path_factory, Q, pamr_steps=STEPS, pamr_stride=DIL)
    imgs = images()
    got = seg.predict_topk(imgs, k)
    for g, x in zip(got, imgs):
        assert same(g, compose(base, x, k, steps=STEPS))
        assert same(seg._pipeline().segment_scene(x, 16, 32, topk=k), g)
    assert not same(got[0], base.predict_topk(imgs[:1], k)[0]), "PAMR changed nothing: the case would show nothing"
    oris = [(33, 170), tuple(imgs[1].shape[-2:])]                          # the first sample has another ori_shape
    for s, steps in ((base, 0), (seg, STEPS)):
        out = s.predict_topk(imgs, k, [Sample(dict(ori_shape=o)) for o in oris])
        for ds, x, o in zip(out, imgs, oris):
            g = (ds.data["seg_topk_classes"].data, ds.data["seg_topk_probs"].data)
            assert g[0].shape == (k,) + o and same(g, compose(base, x, k, o, steps))
            pred = torch.where(g[1][0] < s.prob_thd, torch.full_like(g[0][0], s.bg_idx), g[0][0]).long()[None]
            assert torch.equal(ds.data["pred_sem_seg"].data, pred)


def test_whole_image_inference(tmp_path_factory):
    """slide_crop <= 0: forward_feature's logits, post-processed and sorted."""
    from clip_decontamination_amd import ops
    seg = seg_of(tmp_path_factory, 8, "Segmentor", slide_crop=0)
    x = as_float(scene_u8((40, 48), 31))
    logits = seg.forward_feature(x[None], (40, 48))[0]
    probs, _ = ops.postprocess(logits, seg.query_idx, seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx)
    assert same(seg.predict_topk([x], 3)[0], ops.topk_from_probs(probs, seg.query_idx, 3))


def test_refusals(tmp_path_factory):
    seg = seg_of(tmp_path_factory, 8)
    pipe = seg._pipeline()
    x = images()[1]
    with pytest.raises(ValueError, match="top-k under tile_group sharding is not built"):
        pipe.segment_scene(x, 16, 32, group="world", topk=2)
    sharded = seg_of(tmp_path_factory, 8, tile_group="world")
    with pytest.raises(ValueError, match="top-k under tile_group sharding is not built"):
        sharded.predict_topk([x], 2)
    with pytest.raises(ValueError, match="top-k under tile_group sharding is not built"):
        sharded._pipeline().segment_scenes([x], 16, 32, topk=2)
    with pytest.raises(ValueError, match="exclude each other"):
        pipe.segment_scene(x, 16, 32, want_probs=True, topk=2)
    with pytest.raises(ValueError, match="exclude each other"):
        pipe.segment_scenes([x], 16, 32, want_probs=True, topk=2)
    for k in (-1, 6, 9):                                                    # K = 5
        with pytest.raises(ValueError, match="topk must lie in"):
            seg.predict_topk([x], k)
    with pytest.raises(ValueError, match="topk must lie in"):
        seg.predict_topk([x], 0)


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_calls_without_topk_are_what_they_were(tmp_path_factory, Q, cls_name):
    """predict, predict_many and segment_scene without a topk argument: the composition from the pieces they were made of before
    (forward_slide -> ops.postprocess), and ``topk=0`` spelled out changes nothing."""
    from clip_decontamination_amd import ops
    seg = seg_of(tmp_path_factory, Q, cls_name)
    pipe = seg._pipeline()
    imgs = images()
    oris = [tuple(imgs[0].shape[-2:]), (50, 70)]
    want = []
    for x, o in zip(imgs, oris):
        logits = seg.forward_slide(x[None], [dict(ori_shape=o)], 16, 32)[0]
        want.append(ops.postprocess(logits, seg.query_idx, seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx))
    out = seg.predict_many(imgs, [Sample(dict(ori_shape=o)) for o in oris])
    for ds, (p, l) in zip(out, want):
        assert set(ds.data) == {"seg_logits", "pred_sem_seg"}
        assert torch.equal(ds.data["seg_logits"].data, p) and torch.equal(ds.data["pred_sem_seg"].data, l)
    ds = seg.predict(imgs[0][None], [Sample(dict(ori_shape=oris[0]))])[0]
    assert torch.equal(ds.data["seg_logits"].data, want[0][0]) and torch.equal(ds.data["pred_sem_seg"].data, want[0][1])
    u8 = scene_u8(SHAPES[1], 21)
    assert torch.equal(pipe.segment_scene(u8, 16, 32), pipe.segment_scene(u8, 16, 32, topk=0))
    pa, pb = pipe.segment_scene(u8, 16, 32, want_probs=True), pipe.segment_scene(u8, 16, 32, want_probs=True, topk=0)
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
    la, lb = pipe.segment_scenes(imgs, 16, 32), pipe.segment_scenes(imgs, 16, 32, topk=0)
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    if Q <= 64:                                                             # the labels-only tail on the canvas route (label_head="auto")
        assert torch.equal(seg.predict(imgs[0][None], None), want[0][1])
