"""Weighted window blending on the device: sg_stitch_blend[_multi] and sg_label_head_blend[_multi] against the float64 reference of
tests/blend_reference.py (element by element within its bound; labels under head_reference.check_labels), byte for byte against the
unweighted entries under a one-entry ramp, against each other (multi against single, a canvas band against the whole canvas, repeats),
and behind SegPipeline and the drop-in classes on the f32 tiny-8 tower, where ``blend="hann"`` must return exactly what the blended ops
give on the same tile logits and ``blend="uniform"`` exactly what an instance built without the option returns.  Shapes are
head_reference's canvases of about 70 x 90."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_reference as BR  # noqa: E402
import head_reference as HR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALE, BG = 50.0, 0


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def stitch_args(c):
    return dev(c["tile_logits"]), dev(c["windows"]), c["up_hw"], c["pad_tl"], c["hw"]


def same(a, b):
    """Two device tensors, byte for byte."""
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def head_post(c, thd):
    return dev(c["query_idx"]), c["K"], SCALE, thd, BG


# ---- 1. the canvas against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BR.STITCH_GEOMETRIES)
def test_stitch_blend_vs_f64(name):
    from clip_decontamination_amd import ops
    worst = 0.0
    for Q in BR.STITCH_Q:
        c = BR.stitch_case(name, Q)
        host = (c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
        ups = BR.upsampled(c["tile_logits"], c["up_hw"])
        covered = BR.weight_sum(c["windows"], c["hw"], BR.UNIFORM) > 0
        for kind, R in BR.stitch_ramps(name):
            r = BR.ramp(kind, R)
            got = ops.stitch_blend(*stitch_args(c), dev(r)).cpu().numpy()
            what = f"stitch_blend {name} Q={Q} {kind} R={R}"
            worst = max(worst, HR.within(got, BR.stitch_blend(*host, r, ups), BR.stitch_blend_bound(*host, r, ups), what))
            assert not got[:, ~covered].any(), f"{what}: a pixel no tile covers is not exactly 0"
    if name == "hole":
        assert (~covered).sum() > 0
    print(f"stitch_blend {name}: largest err / bound {worst:.3f}")


# ---- 2. a one-entry ramp of 1.0 is the unweighted entry, byte for byte --------------------------------------------------------------------
@pytest.mark.parametrize("name", BR.STITCH_GEOMETRIES)
def test_uniform_ramp_is_sg_stitch(name):
    from clip_decontamination_amd import ops
    one = dev(BR.UNIFORM)
    for Q in BR.STITCH_Q:
        args = stitch_args(BR.stitch_case(name, Q))
        assert same(ops.stitch_blend(*args, one), ops.stitch(*args)), f"{name} Q={Q}"


@pytest.mark.parametrize("geom,Q", BR.HEAD_GEOM_Q)
def test_uniform_ramp_is_sg_label_head(geom, Q):
    from clip_decontamination_amd import ops
    one = dev(BR.UNIFORM)
    for c, merged, thd, _ in BR.head_cases(geom, Q)[::2]:
        args, post = stitch_args(c), head_post(c, thd)
        lab, conf = ops.label_head(*args, *post, want_conf=True)
        lab_b, conf_b = ops.label_head_blend(*args, *post, one, want_conf=True)
        assert same(lab_b, lab) and same(conf_b, conf), f"{geom} Q={Q} merged={merged} thd={thd}"


# ---- 3. the multi-image entries are the single-image entries per image ----------------------------------------------------------------------
@pytest.mark.parametrize("Q", [7, 17])
def test_multi_is_single_per_image(Q):
    from clip_decontamination_amd import ops
    c = HR.make_multi_case(Q)
    r = dev(BR.ramp("hann", 16))
    K = max(1, Q // 2)
    qi = dev(np.random.default_rng(Q).permutation(np.arange(Q) % K).astype(np.int32))
    multi = (dev(c["tile_logits"]), c["windows"], c["tile_image"], c["up_hw"], c["pad_tl"], c["image_hw"], c["image_tiles"])
    _, canvases = ops.stitch_blend_multi(*multi, r)
    labs, _, confs = ops.label_head_blend_multi(*multi, qi, K, SCALE, 0.3, BG, r, want_conf=True)
    for n, (a, k) in enumerate(c["image_tiles"]):
        one = (dev(c["tile_logits"][a:a + k]), dev(c["windows"][a:a + k]), c["up_hw"], c["pad_tl"], c["image_hw"][n])
        assert same(canvases[n], ops.stitch_blend(*one, r)), f"canvas of image {n}"
        lab, conf = ops.label_head_blend(*one, qi, K, SCALE, 0.3, BG, r, want_conf=True)
        assert same(labs[n], lab) and same(confs[n], conf), f"labels of image {n}"


# ---- 4. the label head against tail(stitch_blend) in float64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,Q", BR.HEAD_GEOM_Q)
def test_label_head_blend_vs_f64(geom, Q):
    from clip_decontamination_amd import ops
    for c, merged, thd, spec in BR.head_cases(geom, Q):
        r = BR.head_ramp(geom, spec)
        ref = HR.tail(BR.stitch_blend(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"], r), c["query_idx"], c["K"], SCALE, thd, BG)
        args, post = stitch_args(c), head_post(c, thd)
        lab, conf = ops.label_head_blend(*args, *post, dev(r), want_conf=True)
        what = f"label_head_blend {geom} Q={Q} merged={merged} thd={thd} {spec}"
        HR.check_labels(ref, lab.cpu().numpy(), conf.cpu().numpy(), thd, what)
        T = c["tile_logits"].shape[0]
        labs, _, confs = ops.label_head_blend_multi(args[0], c["windows"], np.zeros(T, dtype=np.int32), c["up_hw"], c["pad_tl"], [c["hw"]],
                                                    [(0, T)], *post, dev(r), want_conf=True)
        assert same(labs[0], lab) and same(confs[0], conf), what + ": the multi entry on this one image"


# ---- 5. a canvas band with shifted windows is the rows of the whole canvas ---------------------------------------------------------------------
@pytest.mark.parametrize("name,Q", [("a", 9), ("b", 17), ("dense", 8)])
def test_a_band_is_the_rows_of_the_whole_canvas(name, Q):
    from clip_decontamination_amd import ops
    c = BR.stitch_case(name, Q)
    H = c["hw"][0]
    r = dev(BR.ramp("hann", max(1, BR.crop_of(name) // 2)))
    K = max(1, Q // 2)
    post = (dev((np.arange(Q) % K).astype(np.int32)), K, SCALE, 0.3, BG)
    whole = ops.stitch_blend(*stitch_args(c), r)
    lab, conf = ops.label_head_blend(*stitch_args(c), *post, r, want_conf=True)
    for a, b in ((0, 13), (H // 3, 2 * H // 3 + 1), (H - 9, H)):
        tl, wb, hw = BR.band_of(c, a, b)
        band = (dev(tl), dev(wb), c["up_hw"], c["pad_tl"], hw)
        assert same(ops.stitch_blend(*band, r), whole[:, a:b].contiguous()), f"rows {a}..{b}"
        lab_b, conf_b = ops.label_head_blend(*band, *post, r, want_conf=True)
        assert same(lab_b, lab[:, a:b].contiguous()) and same(conf_b, conf[a:b].contiguous()), f"labels of rows {a}..{b}"


# ---- 6. repeats ---------------------------------------------------------------------------------------------------------------------------
def test_repeats_are_byte_identical():
    from clip_decontamination_amd import ops
    c = BR.stitch_case("dense", 17)
    r = dev(BR.ramp("linear", 5))
    post = (dev(np.arange(17, dtype=np.int32)), 17, SCALE, 0.3, BG)
    first = (ops.stitch_blend(*stitch_args(c), r),) + ops.label_head_blend(*stitch_args(c), *post, r, want_conf=True)
    for _ in range(3):
        again = (ops.stitch_blend(*stitch_args(c), r),) + ops.label_head_blend(*stitch_args(c), *post, r, want_conf=True)
        assert all(same(x, y) for x, y in zip(first, again))


# ---- 7. behind the pipeline: the f32 tiny-8 tower, synthetic weights -------------------------------------------------------------------------
SHAPES = [(40, 150), (47, 61)]
QK = {8: 5, 65: 40}
CROP, STRIDE = 32, 16
_SEG = {}


def class_file(tmp_path_factory, Q):
    """One class per line, synonyms separated by commas: the first Q - K classes get two names."""
    K = QK[Q]
    lines, q = [], 0
    for c in range(K):
        k = 2 if c < Q - K else 1
        lines.append(",".join(f"thing{q + i}" for i in range(k)))
        q += k
    path = tmp_path_factory.getbasetemp() / f"blend_cls_{Q}.txt"
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
                    slide_crop=CROP, slide_stride=STRIDE)
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


def tiles_of(pipe, x):
    """What the blended ops take for image x: SegPipeline.tile_logits and the geometry of its windows."""
    H, W, stride, crop, wins, tile_hw, pad_tl, up_hw, grid = pipe._geometry(x, STRIDE, CROP)
    tl = pipe.tile_logits(x, wins, tile_hw, grid_of_tiles=grid)
    return tl, torch.tensor(wins, dtype=torch.int32), up_hw, pad_tl, (H, W)


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_the_pipeline_returns_what_the_blended_ops_give(tmp_path_factory, Q, cls_name):
    from clip_decontamination_amd import ops
    seg = seg_of(tmp_path_factory, Q, cls_name, blend="hann")
    plain = seg_of(tmp_path_factory, Q, cls_name)
    pipe = seg._pipeline()
    assert (pipe.blend, pipe.blend_ramp) == ("hann", None)
    ramp = ops.blend_ramp("hann", CROP // 2).to(DEV)                          # blend_ramp=None: half the 32 x 32 window
    imgs = images()
    post = (seg.query_idx, seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx)
    want_lab, want_probs, want_topk, want_canvas = [], [], [], []
    for x in imgs:
        args = tiles_of(pipe, x)
        canvas = ops.stitch_blend(*args, ramp)
        probs, lab = ops.postprocess(canvas, *post)
        want_canvas.append(canvas)
        want_probs.append((probs, lab))
        want_topk.append(ops.topk_from_probs(probs, seg.query_idx, 3))
        # labels only: the fused head beyond 64 queries (label_head="auto"), the canvas route up to there
        want_lab.append(ops.label_head_blend(*args, *post, ramp) if Q > 64 else lab)
    for x, lab, (probs, plab), (tc, tp), canvas in zip(imgs, want_lab, want_probs, want_topk, want_canvas):
        assert same(pipe.segment_scene(x, STRIDE, CROP), lab)
        p, l = pipe.segment_scene(x, STRIDE, CROP, want_probs=True)
        assert same(p, probs) and same(l, plab)
        c, p = pipe.segment_scene(x, STRIDE, CROP, topk=3)
        assert same(c, tc) and same(p, tp)
        assert same(pipe.forward_slide(x, STRIDE, CROP)[0], canvas)
        assert same(seg.predict(x[None], None), lab)
        assert not same(canvas, plain._pipeline().forward_slide(x, STRIDE, CROP)[0]), "blending changed nothing: the case would show nothing"
    assert all(same(g, w) for g, w in zip(pipe.segment_scenes(imgs, STRIDE, CROP), want_lab))
    prb, lab = pipe.segment_scenes(imgs, STRIDE, CROP, want_probs=True)
    assert all(same(p, w[0]) and same(l, w[1]) for p, l, w in zip(prb, lab, want_probs))
    assert all(same(g[0], w[0]) and same(g[1], w[1]) for g, w in zip(pipe.segment_scenes(imgs, STRIDE, CROP, topk=3), want_topk))
    assert all(same(g[0], w) for g, w in zip(pipe.forward_slide_many(imgs, STRIDE, CROP), want_canvas))
    fused = seg_of(tmp_path_factory, Q, cls_name, blend="hann", label_head="fused")._pipeline()      # the fused head at Q = 8 too
    for x, g in zip(imgs, fused.segment_scenes(imgs, STRIDE, CROP)):
        w = ops.label_head_blend(*tiles_of(fused, x), *post, ramp)
        assert same(g, w) and same(fused.segment_scene(x, STRIDE, CROP), w)


@pytest.mark.parametrize("Q", [8, 65])
def test_area_thd_behind_a_blended_stitch(tmp_path_factory, Q):
    """area_thd with blend on takes the canvas route whatever label_head says (sg_area_relabel gathers unweighted): stitch_blend, the
    first pass with prob_thd = 0, the areas, the filter."""
    from clip_decontamination_amd import ops
    thd = 0.1
    seg = seg_of(tmp_path_factory, Q, blend="hann", area_thd=thd, label_head="fused")
    pipe = seg._pipeline()
    ramp = ops.blend_ramp("hann", CROP // 2).to(DEV)
    imgs = images()
    want = []
    for x in imgs:
        canvas = ops.stitch_blend(*tiles_of(pipe, x), ramp)
        probs, lab = ops.postprocess(canvas, seg.query_idx, seg.num_classes, seg.logit_scale, 0.0, seg.bg_idx)
        keep = ops.area_keep(ops.class_area(lab, seg.num_classes), seg.bg_idx, thd)
        ops.area_filter_probs(probs, lab, keep, seg.prob_thd, seg.bg_idx)
        want.append((probs, lab))
    for x, (probs, lab) in zip(imgs, want):
        assert same(pipe.segment_scene(x, STRIDE, CROP), lab)
        p, l = pipe.segment_scene(x, STRIDE, CROP, want_probs=True)
        assert same(p, probs) and same(l, lab)
    assert all(same(g, w[1]) for g, w in zip(pipe.segment_scenes(imgs, STRIDE, CROP), want))


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
@pytest.mark.parametrize("Q", [8, 65])
def test_uniform_is_an_instance_without_the_option(tmp_path_factory, Q, cls_name):
    off, plain = seg_of(tmp_path_factory, Q, cls_name, blend="uniform", blend_ramp=7), seg_of(tmp_path_factory, Q, cls_name)
    a, b = off._pipeline(), plain._pipeline()
    assert a.blend == b.blend == "uniform"
    imgs = images()
    for x in imgs:
        assert same(a.segment_scene(x, STRIDE, CROP), b.segment_scene(x, STRIDE, CROP))
        pa, pb = a.segment_scene(x, STRIDE, CROP, want_probs=True), b.segment_scene(x, STRIDE, CROP, want_probs=True)
        assert same(pa[0], pb[0]) and same(pa[1], pb[1])
        assert same(a.forward_slide(x, STRIDE, CROP), b.forward_slide(x, STRIDE, CROP))
        assert same(off.predict(x[None], None), plain.predict(x[None], None))
    assert all(same(g, w) for g, w in zip(a.segment_scenes(imgs, STRIDE, CROP), b.segment_scenes(imgs, STRIDE, CROP)))
    ta, tb = a.segment_scenes(imgs, STRIDE, CROP, topk=3), b.segment_scenes(imgs, STRIDE, CROP, topk=3)
    assert all(same(g[0], w[0]) and same(g[1], w[1]) for g, w in zip(ta, tb))


def test_an_explicit_ramp_length(tmp_path_factory):
    """blend_ramp=5 with "linear": the table of R = 5 whatever the window size."""
    from clip_decontamination_amd import ops
    seg = seg_of(tmp_path_factory, 65, blend="linear", blend_ramp=5)
    pipe = seg._pipeline()
    ramp = ops.blend_ramp("linear", 5).to(DEV)
    for x in images():
        want = ops.label_head_blend(*tiles_of(pipe, x), seg.query_idx, seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx, ramp)
        assert same(pipe.segment_scene(x, STRIDE, CROP), want)
