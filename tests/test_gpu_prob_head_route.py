"""The fused probability head behind the drop-in classes: ``prob_head="fused"`` must leave in the data samples, and in the result_dir /
heatmap_dir images, exactly what ``prob_head="canvas"`` leaves (f32 tower, tiny synthetic weights)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class Sample:
    def __init__(self, meta):
        self.metainfo, self.data = meta, {}

    def set_data(self, d):
        self.data.update(d)


def class_file(tmp_path, n_queries, n_classes):
    """One class per line, synonyms separated by commas: the first n_queries - n_classes classes get two names."""
    lines, q = [], 0
    for c in range(n_classes):
        k = 2 if c < n_queries - n_classes else 1
        lines.append(",".join(f"thing{q + i}" for i in range(k)))
        q += k
    assert q == n_queries
    path = tmp_path / f"cls_{n_queries}.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


QK = {9: 6, 70: 40}


def build(cls_name, name_path, **kw):
    import segearth_segmentor
    import segmentor
    cls = segmentor.SegmentorEx if cls_name == "SegmentorEx" else segearth_segmentor.Segmentor
    kw.setdefault("apply_sim_feat_up", False)
    kw.setdefault("vit_type", "tiny-8")
    kw.setdefault("slide_crop", 32)
    kw.setdefault("slide_stride", 16)
    return cls(clip_type="CLIP", model_type="SegEarth", name_path=name_path, device=torch.device("cuda:0"), precision="f32", synthetic_ok=True,
               prob_thd=0.05, bg_idx=5, **kw)


def image(h, w, seed=11):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((1, 3, h, w)).astype(np.float32)).cuda()


def predict(seg, x, ori=None, **meta):
    ds = seg.predict(x, [Sample(dict(ori_shape=tuple(x.shape[-2:]) if ori is None else ori, **meta))])[0]
    return ds.data["seg_logits"].data, ds.data["pred_sem_seg"].data


def counted(monkeypatch, calls, name):
    from clip_decontamination_amd import ops
    fn = getattr(ops, name)

    def wrap(*a, **k):
        calls[name] = calls.get(name, 0) + 1
        return fn(*a, **k)

    monkeypatch.setattr(ops, name, wrap)


@pytest.mark.parametrize("Q", [9, 70])
@pytest.mark.parametrize("cls_name", ["Segmentor", "SegmentorEx"])
def test_predict_fused_equals_canvas(tmp_path, monkeypatch, cls_name, Q):
    path = class_file(tmp_path, Q, QK[Q])
    x = image(72, 88)
    want_p, want_l = predict(build(cls_name, path, prob_head="canvas"), x)
    calls = {}
    counted(monkeypatch, calls, "prob_head")
    counted(monkeypatch, calls, "stitch")
    got_p, got_l = predict(build(cls_name, path, prob_head="fused"), x)
    assert calls == {"prob_head": 1}                                          # the fused head ran, no canvas was stitched
    assert got_p.shape == (QK[Q], 72, 88) and got_l.shape == (1, 72, 88) and got_l.dtype == torch.int64
    assert torch.equal(got_p, want_p) and torch.equal(got_l, want_l)


def test_predict_fused_equals_canvas_on_per_pixel_logits(tmp_path):
    """The ``bilinear`` upsampler (no checkpoint): tile logits per pixel, not per patch."""
    path = class_file(tmp_path, 9, 6)
    kw = dict(vit_type="tiny-14", apply_sim_feat_up=True, sim_feat_up_cfg=dict(model_name="bilinear", model_path=None),
              slide_crop=40, slide_stride=24)
    x = image(72, 88, seed=3)
    want_p, want_l = predict(build("SegmentorEx", path, prob_head="canvas", **kw), x)
    got_p, got_l = predict(build("SegmentorEx", path, prob_head="fused", **kw), x)
    assert torch.equal(got_p, want_p) and torch.equal(got_l, want_l)


def test_another_ori_shape_keeps_the_canvas(tmp_path, monkeypatch):
    path = class_file(tmp_path, 9, 6)
    x = image(72, 88)
    want_p, want_l = predict(build("SegmentorEx", path, prob_head="canvas"), x, ori=(60, 99))
    calls = {}
    counted(monkeypatch, calls, "prob_head")
    got_p, got_l = predict(build("SegmentorEx", path, prob_head="fused"), x, ori=(60, 99))
    assert calls == {}                                                        # the resize is not fused: the canvas route ran
    assert got_p.shape == (6, 60, 99) and torch.equal(got_p, want_p) and torch.equal(got_l, want_l)


@pytest.mark.parametrize("Q", [9, 70])
def test_predict_many_is_one_launch_per_flush_group(tmp_path, monkeypatch, Q):
    from clip_decontamination_amd.pipeline import SegPipeline
    seg = build("SegmentorEx", class_file(tmp_path, Q, QK[Q]), prob_head="fused")
    imgs = [image(72, 88, 1), image(48, 64, 2), image(40, 150, 3)]
    single = [predict(seg, x) for x in imgs]
    calls = {}
    for name in ("prob_head_multi", "stitch_multi", "stitch", "postprocess", "postprocess_multi"):
        counted(monkeypatch, calls, name)
    groups = SegPipeline._packed_tile_logits

    def flush_group(*a, **k):
        calls["flush_groups"] = calls.get("flush_groups", 0) + 1
        return groups(*a, **k)

    monkeypatch.setattr(SegPipeline, "_packed_tile_logits", flush_group)
    out = seg.predict_many(imgs, [Sample(dict(ori_shape=tuple(x.shape[-2:]))) for x in imgs])
    assert calls["flush_groups"] >= 1 and calls == {"flush_groups": calls["flush_groups"], "prob_head_multi": calls["flush_groups"]}
    for ds, (p, l) in zip(out, single):
        assert torch.equal(ds.data["seg_logits"].data, p) and torch.equal(ds.data["pred_sem_seg"].data, l)


def test_written_images_are_identical_files(tmp_path):
    path = class_file(tmp_path, 9, 6)
    x = image(72, 88)
    files = {}
    for mode in ("canvas", "fused"):
        seg = build("SegmentorEx", path, prob_head=mode, result_dir=str(tmp_path / mode / "res"), heatmap_dir=str(tmp_path / mode / "heat"))
        predict(seg, x, img_path="/data/scene_7.tif")
        files[mode] = [(tmp_path / mode / d / "scene_7.png").read_bytes() for d in ("res", "heat")]
    assert all(len(b) > 0 for b in files["canvas"]) and files["canvas"] == files["fused"]


def test_unknown_value_is_refused(tmp_path):
    path = class_file(tmp_path, 9, 6)
    for cls_name in ("Segmentor", "SegmentorEx"):
        with pytest.raises(ValueError, match="prob_head"):
            build(cls_name, path, prob_head="both")
