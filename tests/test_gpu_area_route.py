"""area_thd behind the drop-in classes and SegPipeline (f32 tiny-8 tower, synthetic weights, the scenes and class files of
tests/test_gpu_topk_route.py: 40 x 150 and 47 x 61, crop 32, stride 16, Q = 8 -> K = 5 and Q = 65 -> K = 40).

An instance without the option supplies the first-pass probabilities; area_thd is chosen from them by the widest-gap rule of
tests/area_reference.py (over both images: the midpoint of a gap between adjacent non-background areas that leaves the widest margin on
either), with that file's two preconditions asserted.  Wherever probabilities exist the routes must equal ``ops.area_filter`` on those
probabilities byte for byte; the labels-only routes equal its labels byte for byte on the canvas route and on every counted pixel on the
fused label head (counted: area_reference's rule, evaluated on those probabilities)."""
import numpy as np
import pytest
import torch

import area_reference as AR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS, DIL = 10, (8, 16)
SHAPES = [(40, 150), (47, 61)]
QK = {8: 5, 65: 40}
BG = 3
_SEG, _THD = {}, {}


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
    path = tmp_path_factory.getbasetemp() / f"area_cls_{Q}.txt"
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
                    device=torch.device(DEV), precision="f32", synthetic_ok=True, prob_thd=0.05, bg_idx=BG, apply_sim_feat_up=False,
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


def unfiltered(seg, imgs, oris=None):
    """The probabilities [K,H,W] of an instance without the option, per image, through predict with data samples."""
    oris = [tuple(x.shape[-2:]) for x in imgs] if oris is None else oris
    return [seg.predict(x[None], [Sample(dict(ori_shape=o))])[0].data["seg_logits"].data for x, o in zip(imgs, oris)]


def choose_thd(probs, prob_thd):
    """The widest-gap rule over several images: among the midpoints of the gaps between adjacent non-background areas of any image that
    drop a class of positive area and keep a non-background class on every image, the one whose nearest area (over all images) is
    farthest, in pixels.  Both preconditions are asserted for every image."""
    ps = [p.cpu().numpy().astype(np.float64) for p in probs]
    K = ps[0].shape[0]
    areas = [np.bincount(p.argmax(0).reshape(-1), minlength=K) for p in ps]
    nb = [np.delete(a, BG) for a in areas]

    def margin(t):
        return min(float(np.abs(a - t * a.sum()).min()) for a in nb)

    cands = []
    for a in nb:
        s = np.sort(a)
        cands += [float(s[i] + s[i + 1]) / 2.0 / float(a.sum()) for i in range(len(s) - 1) if s[i + 1] > s[i]]

    def splits(t):                                                            # on every image: a class of positive area goes, one stays
        return all(bool(((a <= t * a.sum()) & (a > 0)).any()) and bool((a > t * a.sum()).any()) for a in nb)

    cands = [t for t in cands if splits(t)]
    assert cands, "no gap between adjacent areas splits the classes of every image"
    thd = max(cands, key=margin)
    for p, a in zip(ps, nb):
        top2 = np.partition(p, K - 2, axis=0)[K - 2:]
        undecided = int((top2[1] - top2[0] < AR.G).sum())
        m = float(np.abs(a - thd * a.sum()).min())
        keep = a > thd * a.sum()
        print(f"area_thd {thd:.4f}: areas {a.tolist()}, margin {m:.1f} px against {undecided} undecided first labels")
        assert m > undecided, "an area lies closer to the bound than the first pass is decided"
        assert bool((~keep & (a > 0)).any()) and bool(keep.any()), "the threshold drops nothing or keeps nothing"
    return thd


def setup(tmp_path_factory, Q, cls_name="SegmentorEx", **kw):
    """(the instance without the option, the same instance with it, area_thd, the images)."""
    base = seg_of(tmp_path_factory, Q, cls_name, **kw)
    imgs = images()
    key = (Q, cls_name, tuple(sorted(kw.items())))
    if key not in _THD:
        _THD[key] = choose_thd(unfiltered(base, imgs), base.prob_thd)
    return base, seg_of(tmp_path_factory, Q, cls_name, area_thd=_THD[key], **kw), _THD[key], imgs


def filtered(base, probs, thd):
    from clip_decontamination_amd import ops
    return [ops.area_filter(p, thd, base.prob_thd, BG) for p in probs]


def counted(p32, keep, prob_thd):
    """area_reference's acceptance rule on the unfiltered f32 probabilities of one image."""
    p = p32.cpu().numpy().astype(np.float64)
    K = p.shape[0]
    top2 = np.partition(p, K - 2, axis=0)[K - 2:]
    kp = np.where(keep.cpu().numpy().astype(bool)[:, None, None], p, -np.inf)
    p1 = kp.max(0)
    p2 = np.maximum(np.partition(kp, K - 2, axis=0)[K - 2], 0.0)
    rel = np.where(p1 > 0, (p1 - p2) / np.where(p1 > 0, p1, 1.0), 0.0)
    ok = (top2[1] - top2[0] >= AR.G) & (rel >= AR.G) & (np.abs(p1 - prob_thd) >= AR.G)
    assert 1.0 - ok.mean() <= AR.CAP, f"{100 * (1 - ok.mean()):.2f} % of the pixels are uncounted"
    return torch.from_numpy(ok).to(DEV)


def same_sample(ds, want):
    p, l, _ = want
    assert set(ds.data) == {"seg_logits", "pred_sem_seg"}
    got_p, got_l = ds.data["seg_logits"].data, ds.data["pred_sem_seg"].data
    assert got_p.dtype == torch.float32 and got_l.dtype == torch.int64 and got_l.shape == l.shape
    assert got_p.cpu().numpy().tobytes() == p.cpu().numpy().tobytes() and torch.equal(got_l, l)


@pytest.mark.parametrize("prob_head", ["canvas", "fused"])
@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_data_samples_hold_the_filtered_probabilities(tmp_path_factory, Q, cls_name, prob_head):
    base, seg, thd, imgs = setup(tmp_path_factory, Q, cls_name, prob_head=prob_head)
    want = filtered(base, unfiltered(base, imgs), thd)
    assert any(bool((w[1] != torch.where(p.max(0).values < base.prob_thd, BG, p.argmax(0))[None]).any())
               for w, p in zip(want, unfiltered(base, imgs))), "the filter moved no label: the case would show nothing"
    for x, w in zip(imgs, want):
        same_sample(seg.predict(x[None], [Sample(dict(ori_shape=tuple(x.shape[-2:])))])[0], w)
    out = seg.predict_many(imgs, [Sample(dict(ori_shape=tuple(x.shape[-2:]))) for x in imgs])
    for ds, w in zip(out, want):
        same_sample(ds, w)
    pipe = seg._pipeline()
    p, l = pipe.segment_scene(imgs[1], 16, 32, want_probs=True)
    assert torch.equal(p, want[1][0]) and torch.equal(l, want[1][1])


@pytest.mark.parametrize("Q", [8, 65])
def test_with_pamr_at_another_ori_shape_and_whole_image(tmp_path_factory, Q):
    imgs = images()
    # PAMR on: the refined canvas, then the two decisions
    base, seg, thd, _ = setup(tmp_path_factory, Q, pamr_steps=STEPS, pamr_stride=DIL)
    want = filtered(base, unfiltered(base, imgs), thd)
    for ds, w in zip(seg.predict_many(imgs, [Sample(dict(ori_shape=tuple(x.shape[-2:]))) for x in imgs]), want):
        same_sample(ds, w)
    same_sample(seg.predict(imgs[0][None], [Sample(dict(ori_shape=SHAPES[0]))])[0], want[0])
    assert torch.equal(seg.predict(imgs[0][None], None), want[0][1])              # labels only: the canvas route under PAMR
    # another ori_shape (the first image), with and without PAMR, and through resize_head="fused", which takes the canvas route here
    oris = [(33, 170), SHAPES[1]]
    for kw in (dict(), dict(pamr_steps=STEPS, pamr_stride=DIL), dict(resize_head="fused")):
        base = seg_of(tmp_path_factory, Q, **kw)
        probs = unfiltered(base, imgs, oris)
        thd = choose_thd(probs, base.prob_thd)
        seg = seg_of(tmp_path_factory, Q, area_thd=0.5, **kw)
        seg.area_thd = thd                                                        # the pipeline is rebuilt per call: attribute edits are honoured
        want = filtered(base, probs, thd)
        for ds, w in zip(seg.predict_many(imgs, [Sample(dict(ori_shape=o)) for o in oris]), want):
            same_sample(ds, w)
        same_sample(seg.predict(imgs[0][None], [Sample(dict(ori_shape=oris[0]))])[0], want[0])
        labs = seg.predict_many(imgs, None, ori_shapes=oris)                      # labels only at another size
        assert all(torch.equal(a, w[1]) for a, w in zip(labs, want))
        assert torch.equal(seg._pipeline().segment_scene(imgs[0], 16, 32, ori_shape=oris[0]), want[0][1])
    # whole-image inference
    x = as_float(scene_u8((40, 48), 31))
    base = seg_of(tmp_path_factory, Q, "Segmentor", slide_crop=0)
    probs = unfiltered(base, [x])
    thd = choose_thd(probs, base.prob_thd)
    seg = seg_of(tmp_path_factory, Q, "Segmentor", slide_crop=0, area_thd=thd)
    want = filtered(base, probs, thd)[0]
    same_sample(seg.predict(x[None], [Sample(dict(ori_shape=(40, 48)))])[0], want)
    same_sample(seg.predict_many([x], [Sample(dict(ori_shape=(40, 48)))])[0], want)
    assert torch.equal(seg.predict_many([x])[0], want[1])


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_labels_only_routes(tmp_path_factory, Q, cls_name):
    from clip_decontamination_amd import ops
    base, _, thd, imgs = setup(tmp_path_factory, Q, cls_name)
    probs = unfiltered(base, imgs)
    want = filtered(base, probs, thd)
    gts = [torch.from_numpy(np.random.default_rng(7 + i).integers(0, QK[Q], hw).astype(np.uint8)) for i, hw in enumerate(SHAPES)]
    for head in ("canvas", "fused"):
        seg = seg_of(tmp_path_factory, Q, cls_name, label_head=head, area_thd=thd)
        pipe = seg._pipeline()
        assert pipe.fused_label_head() == (head == "fused")
        got = {"predict_many": seg.predict_many(imgs), "segment_scene": [pipe.segment_scene(x, 16, 32) for x in imgs],
               "predict": [seg.predict(x[None], None) for x in imgs]}
        for route, labs in got.items():
            for n, (lab, w, p) in enumerate(zip(labs, want, probs)):
                assert lab.dtype == torch.int64 and lab.shape == w[1].shape
                if head == "canvas":
                    assert torch.equal(lab, w[1]), (route, n)
                else:
                    ok = counted(p, w[2], base.prob_thd)
                    bad = int((lab[0][ok] != w[1][0][ok]).sum())
                    print(f"Q={Q} {route} image {n}: uncounted {100 * (1 - ok.float().mean()):.3f} %, mismatches on counted pixels {bad}")
                    assert bad == 0, (route, n)
        # evaluate counts the filtered labels of its own route
        _, metric = seg.evaluate(imgs, gts)
        table = torch.zeros(QK[Q] + 1, QK[Q] + 1, dtype=torch.int64, device=DEV)
        for lab, g in zip(got["predict_many"], gts):
            ops.confusion_accumulate(lab, g.to(DEV), table, QK[Q])
        assert torch.equal(metric.confusion.to(DEV), table)
    if Q > 64:                                                                     # label_head="auto" beyond 64 queries is the fused head
        auto = seg_of(tmp_path_factory, Q, cls_name, area_thd=thd)
        assert auto._pipeline().fused_label_head()
        assert all(torch.equal(a, b) for a, b in zip(auto.predict_many(imgs), got["predict_many"]))


def test_refusals(tmp_path_factory):
    seg = seg_of(tmp_path_factory, 8, area_thd=0.1)
    x = images()[1]
    with pytest.raises(ValueError, match="area_thd under tile_group sharding is not built"):
        seg_of(tmp_path_factory, 8, tile_group="world", area_thd=0.1)
    with pytest.raises(ValueError, match="area_thd under tile_group sharding is not built"):
        seg._pipeline().segment_scene(x, 16, 32, group="world")
    with pytest.raises(ValueError, match="area_thd"):
        seg.predict_topk([x], 2)
    with pytest.raises(ValueError, match="area_thd"):
        seg._pipeline().segment_scene(x, 16, 32, topk=2)
    with pytest.raises(ValueError, match="area_thd"):
        seg._pipeline().segment_scenes([x], 16, 32, topk=2)
    with pytest.raises(ValueError, match="bg_idx"):
        seg_of(tmp_path_factory, 8, bg_idx=5, area_thd=0.1)                       # K = 5
    with pytest.raises(ValueError, match="area_thd"):
        seg_of(tmp_path_factory, 8, area_thd=-0.5)
    assert seg_of(tmp_path_factory, 8, bg_idx=5).bg_idx == 5                       # without the option a bg_idx outside the classes stays legal


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_area_thd_none_is_the_instance_without_the_keyword(tmp_path_factory, Q, cls_name):
    base = seg_of(tmp_path_factory, Q, cls_name)
    off = seg_of(tmp_path_factory, Q, cls_name, area_thd=None)
    imgs = images()
    assert off.area_thd is None and off._pipeline().area_thd is None
    oris = [(33, 170), SHAPES[1]]
    for o in ([tuple(x.shape[-2:]) for x in imgs], oris):
        a = base.predict_many(imgs, [Sample(dict(ori_shape=s)) for s in o])
        b = off.predict_many(imgs, [Sample(dict(ori_shape=s)) for s in o])
        for da, db in zip(a, b):
            assert torch.equal(da.data["seg_logits"].data, db.data["seg_logits"].data)
            assert torch.equal(da.data["pred_sem_seg"].data, db.data["pred_sem_seg"].data)
    for x in imgs:
        da = base.predict(x[None], [Sample(dict(ori_shape=tuple(x.shape[-2:])))])[0]
        db = off.predict(x[None], [Sample(dict(ori_shape=tuple(x.shape[-2:])))])[0]
        assert torch.equal(da.data["seg_logits"].data, db.data["seg_logits"].data)
        assert torch.equal(da.data["pred_sem_seg"].data, db.data["pred_sem_seg"].data)
        assert torch.equal(base.predict(x[None], None), off.predict(x[None], None))
    assert all(torch.equal(a, b) for a, b in zip(base.predict_many(imgs), off.predict_many(imgs)))
