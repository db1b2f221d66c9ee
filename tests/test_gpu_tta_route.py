"""Test-time augmentation behind SegPipeline and the drop-in classes (f32 tiny-8 tower, synthetic weights, crop 32, stride 16, an image
of 72 x 88, Q = 8 -> K = 5): ``segment_scene`` with ``tta_scales=(0.5, 1.0), tta_flip=True`` against the merge computed on the host
from the four resized / flipped scenes (built here with F.interpolate and torch.flip, slid by ``forward_slide`` and by
``tile_logits``), within the bound of tests/tta_reference.py; the fused head and the canvas route against the same reference;
``predict``, ``predict_many`` and ``evaluate`` with ``min_region``; and with the options off every call returns the bytes of an instance
built without them."""
import numpy as np
import pytest
import torch

import head_reference as HR
import head_resized_reference as RR
import tta_reference as TT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HW = (72, 88)
SCALES = (0.5, 1.0)
Q, K = 8, 5
_SEG = {}


class Sample:
    def __init__(self, meta):
        self.metainfo, self.data = meta, {}

    def set_data(self, d):
        self.data.update(d)


def seg_of(tmp_path_factory, **kw):
    key = tuple(sorted(kw.items()))
    if key not in _SEG:
        import segmentor
        path = tmp_path_factory.getbasetemp() / "tta_cls.txt"
        path.write_text("a0,a1\nb0,b1\nc0,c1\nd0\ne0\n")
        args = dict(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path=str(path), device=torch.device(DEV), precision="f32",
                    synthetic_ok=True, prob_thd=0.25, bg_idx=TT.BG, apply_sim_feat_up=False, slide_crop=32, slide_stride=16)
        args.update(kw)
        _SEG[key] = segmentor.SegmentorEx(**args)
    return _SEG[key]


def image(seed=0, hw=HW):
    return torch.from_numpy(np.random.default_rng(70 + seed).standard_normal((3,) + hw).astype(np.float32)).to(DEV)


def host_views(x):
    """The four views, built independently of the pipeline: (scene, flipped), scale outer."""
    out = []
    for s in SCALES:
        hw = (max(1, int(HW[0] * s + 0.5)), max(1, int(HW[1] * s + 0.5)))
        v = x if hw == HW else torch.nn.functional.interpolate(x[None], size=hw, mode="bilinear", align_corners=False, antialias=False)[0]
        out += [(v, False), (torch.flip(v, dims=[2]).contiguous(), True)]
    return out


def host_reference(seg, x, out_hw, thd):
    """-> (ref, bound, P32): the float64 merge and its bound from each view's tile logits (head_reference.stitch -> upsample -> tail),
    and the merge of the four ``forward_slide`` canvases in float64 (what a user would compute with four calls today)."""
    pipe = seg._pipeline()
    qi = seg.query_idx.cpu().numpy()
    P = bound = P_slide = 0.0
    for v, flipped in host_views(x):
        h, w, _, _, wins, tile_hw, pad_tl, up_hw, grid = pipe._geometry(v, 16, 32)
        tl = pipe.tile_logits(v, wins, tile_hw, grid_of_tiles=grid).cpu().numpy()
        c = dict(tile_logits=tl, windows=np.asarray(wins, dtype=np.int32), up_hw=up_hw, pad_tl=pad_tl, hw=(h, w), out=tuple(out_hw))
        c["canvas"] = HR.stitch(tl, c["windows"], up_hw, pad_tl, (h, w))
        c["resized"] = HR.upsample(c["canvas"], out_hw)
        p = HR.tail(c["resized"], qi, K, seg.logit_scale, 0.0, TT.BG)["probs"]
        b = HR.tail_bound(c["resized"], RR.canvas_bound(c), qi, K, seg.logit_scale)["probs"]
        slide = pipe.forward_slide(v, 16, 32, ori_shape=out_hw)[0].cpu().numpy()
        ps = HR.tail(slide, qi, K, seg.logit_scale, 0.0, TT.BG)["probs"]
        if flipped:
            p, b, ps = p[:, :, ::-1], b[:, :, ::-1], ps[:, :, ::-1]
        P, bound, P_slide = P + p, bound + b, P_slide + ps
    return TT.finish(P / 4, thd), dict(probs=bound / 4, conf=(bound / 4).max(0)), P_slide / 4


@pytest.mark.parametrize("out_hw", [HW, (100, 61)], ids=["own-size", "ori-100x61"])
def test_segment_scene_is_the_host_merge_of_the_four_views(tmp_path_factory, out_hw):
    x = image()
    results = {}
    for head in ("fused", "canvas"):
        seg = seg_of(tmp_path_factory, tta_scales=SCALES, tta_flip=True, tta_head=head)
        pipe = seg._pipeline()
        assert pipe.tail_route("probs").route == ("tta_head" if head == "fused" else "tta_canvas")
        ref, bound, P_slide = host_reference(seg, x, out_hw, seg.prob_thd)
        probs, labels = pipe.segment_scene(x, 16, 32, want_probs=True, ori_shape=out_hw)
        assert probs.shape == (K,) + tuple(out_hw) and labels.shape == (1,) + tuple(out_hw) and labels.dtype == torch.int64
        p, l = probs.cpu().numpy(), labels.cpu().numpy()[0]
        TT.check(ref, bound, l, p.max(0), p, seg.prob_thd, f"segment_scene {head} {out_hw}")
        # four forward_slide calls merged on the host: each view's canvas is within the same canvas bound of the float64 one
        r = HR.within(p, P_slide, 2 * bound["probs"], f"{head} against the merged forward_slide calls")
        print(f"{head} {out_hw}: against four forward_slide calls, err / (2 bound) {r:.3f}")
        only = pipe.segment_scene(x, 16, 32, ori_shape=out_hw)
        assert torch.equal(only, labels)                                   # labels alone: the same labels, no planes
        results[head] = (l, p)
    ok = HR.counted(ref, seg.prob_thd)
    assert np.array_equal(results["fused"][0][ok], results["canvas"][0][ok])
    assert np.abs(results["fused"][1] - results["canvas"][1]).max() <= 2 * bound["probs"].max()


def test_predict_predict_many_and_evaluate_with_min_region(tmp_path_factory):
    seg = seg_of(tmp_path_factory, tta_scales=SCALES, tta_flip=True, min_region=6)
    plain = seg_of(tmp_path_factory, tta_scales=SCALES, tta_flip=True)
    imgs = [image(0), image(1, (48, 64))]
    labs = seg.predict_many(imgs)
    unsieved = plain.predict_many(imgs)
    pipe = seg._pipeline()
    for x, l, u in zip(imgs, labs, unsieved):
        assert l.shape == (1,) + tuple(x.shape[-2:]) and torch.equal(l, pipe.segment_scene(x, 16, 32))
        assert torch.equal(l, pipe.sieve(u.clone()))                       # min_region follows on the final labels
    assert any(not torch.equal(l, u) for l, u in zip(labs, unsieved))
    assert torch.equal(seg.predict(imgs[0][None], None), labs[0])
    ds = [Sample(dict(ori_shape=(60, 75))), Sample(dict(ori_shape=(48, 64)))]
    seg.predict_many(imgs, ds)
    for d, x in zip(ds, imgs):
        prb, lab = d.data["seg_logits"].data, d.data["pred_sem_seg"].data
        assert prb.shape == (K,) + d.metainfo["ori_shape"] and lab.shape == (1,) + d.metainfo["ori_shape"]
        assert float(prb.sum(0).max()) <= 1.0 + 1e-5                       # the mean planes: class probabilities
        p2, l2 = pipe.tta_image(x, 16, 32, d.metainfo["ori_shape"], True)
        assert torch.equal(prb, p2) and torch.equal(lab, l2)
    gts = [torch.randint(0, K, x.shape[-2:], generator=torch.Generator().manual_seed(i), dtype=torch.uint8) for i, x in enumerate(imgs)]
    res, metric = seg.evaluate(imgs, gts)
    table = metric.confusion.cpu()                                         # row = prediction, column = ground truth
    assert int(table.sum()) == sum(g.numel() for g in gts) and isinstance(res, dict) and res
    want = torch.zeros_like(table)
    for l, g in zip(labs, gts):
        want[:K, :K] += torch.bincount(l.reshape(-1).cpu() * K + g.reshape(-1).long(), minlength=K * K).view(K, K)
    assert torch.equal(table, want)
    big = [torch.randint(0, K, (90, 110), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)]
    _, m2 = seg.evaluate(imgs[:1], big, at_gt_size=True)
    assert int(m2.confusion.sum()) == 90 * 110
    with pytest.raises(ValueError, match="top-k together with test-time augmentation is not built"):
        seg.predict_topk(imgs, 2)


def test_with_the_options_off_every_call_returns_todays_bytes(tmp_path_factory):
    base = seg_of(tmp_path_factory)
    off = seg_of(tmp_path_factory, tta_scales=None, tta_flip=False, tta_head="canvas")
    imgs = [image(0), image(1, (48, 64))]
    for a, b in zip(base.predict_many(imgs), off.predict_many(imgs)):
        assert torch.equal(a, b)
    da, db = [Sample(dict(ori_shape=HW))], [Sample(dict(ori_shape=HW))]
    base.predict(imgs[0][None], da), off.predict(imgs[0][None], db)
    assert torch.equal(da[0].data["seg_logits"].data, db[0].data["seg_logits"].data)
    assert torch.equal(da[0].data["pred_sem_seg"].data, db[0].data["pred_sem_seg"].data)


def test_whole_image_inference_merges_view_by_view(tmp_path_factory):
    """``slide_crop <= 0``: every view goes through ``forward_feature`` at the output size and the canvas-route merge.  The reference is
    the float64 tail on the device's own f32 logits of each view (built here), so the bound is tail_bound with no canvas error."""
    seg = seg_of(tmp_path_factory, slide_crop=0, tta_scales=(0.5, 1.0), tta_flip=True)
    x = image(2, (64, 80))
    pipe = seg._pipeline()
    qi = seg.query_idx.cpu().numpy()
    P = bound = 0.0
    for s in (0.5, 1.0):
        hw = (int(64 * s + 0.5), int(80 * s + 0.5))
        v = x if s == 1.0 else torch.nn.functional.interpolate(x[None], size=hw, mode="bilinear", align_corners=False, antialias=False)[0]
        for flipped in (False, True):
            vv = torch.flip(v, dims=[2]).contiguous() if flipped else v
            lg = pipe.forward_feature(vv[None], (64, 80))[0].cpu().numpy()
            p = HR.tail(lg, qi, K, seg.logit_scale, 0.0, TT.BG)["probs"]
            b = HR.tail_bound(lg, 0.0, qi, K, seg.logit_scale)["probs"]
            P, bound = P + (p[:, :, ::-1] if flipped else p), bound + (b[:, :, ::-1] if flipped else b)
    ref, bound = TT.finish(P / 4, seg.prob_thd), dict(probs=bound / 4, conf=(bound / 4).max(0))
    ds = [Sample(dict(ori_shape=(64, 80)))]
    seg.predict(x[None], ds)
    p, l = ds[0].data["seg_logits"].data.cpu().numpy(), ds[0].data["pred_sem_seg"].data.cpu().numpy()[0]
    TT.check(ref, bound, l, p.max(0), p, seg.prob_thd, "whole image")
    assert torch.equal(seg.predict(x[None], None), ds[0].data["pred_sem_seg"].data)
    assert torch.equal(seg.predict_many([x])[0], ds[0].data["pred_sem_seg"].data)
