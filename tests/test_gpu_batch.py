"""Packed multi-image inference on the GPU: the multi-canvas head (sg_stitch_multi / sg_postprocess_multi) against the per-image
entry points bit for bit, the packed pipeline (SegPipeline.forward_slide_many / segment_scenes) against forward_slide per image,
the drop-in predict_many against predict, and the 2-byte modes against the CPU oracle."""
import os

import numpy as np
import pytest
import torch

from clip_decontamination_amd import ops, weights as Wt
from clip_decontamination_amd.engine import (HipCLIP, HipVisionTower, OutlierSuppressionModule, SimilarityEnhancementModule,
                                             compute_padsize)
from clip_decontamination_amd.pipeline import SegPipeline, tile_windows
from oracle import segment as OS, vit as OV          # checker only

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SIM = dict(similarity_weight=1.0, temperature=1.0, add_self_similarity=True)
QIDX = [0, 0, 1, 2, 3, 4, 5, 5]
# five ragged scenes: two larger than the crop in both axes, one exactly the crop, one smaller than the crop, one mixed
SHAPES = [(60, 76), (36, 36), (50, 90), (30, 28), (80, 52)]


def setup_module(_m):
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def rand(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * scale)


def scenes(kind, shapes=SHAPES, seed=0):
    if kind == "u8":
        return [torch.from_numpy(np.random.default_rng(seed + i).integers(0, 256, (h, w, 3), dtype=np.uint8)).to(DEV)
                for i, (h, w) in enumerate(shapes)]
    return [rand((3, h, w), seed + i).to(DEV) for i, (h, w) in enumerate(shapes)]


# ---- 1. sg_stitch_multi == sg_stitch per image ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 11, 16])                 # 11: a ragged last chunk of queries
@pytest.mark.parametrize("per_pixel", [False, True])
def test_stitch_multi_equals_stitch_per_image(Q, per_pixel):
    shapes = [(100, 90), (36, 36), (77, 120), (50, 41), (36, 200)]
    P, crop, stride = 8, (36, 36), (20, 20)
    l, r, t, b = compute_padsize(36, 36, P)
    up = (36 + t + b, 36 + l + r)
    g = up if per_pixel else (up[0] // P, up[1] // P)
    wins, tile_image, image_tiles = [], [], []
    for n, (H, W) in enumerate(shapes):
        w = tile_windows(H, W, stride, crop)
        image_tiles.append((len(wins), len(w)))
        wins += w
        tile_image += [n] * len(w)
    tl = rand((len(wins), Q) + g, 7 + Q).to(DEV)
    _, views = ops.stitch_multi(tl, wins, tile_image, up, (t, l), shapes, image_tiles)
    for n, (H, W) in enumerate(shapes):
        a, c = image_tiles[n]
        ref = ops.stitch(tl[a:a + c], torch.tensor(wins[a:a + c], dtype=torch.int32), up, (t, l), (H, W))
        assert torch.equal(views[n], ref), f"image {n}"


def test_multi_heads_equal_single_when_every_window_is_tested():
    """Stride 2 under crop 32 puts more than 64 windows over one 64 x 4 block: the candidate list overflows and the per-pixel loop
    tests every window of the image, the one path that reads tile_image per pixel.  Canvases, labels and conf against the per-image
    entry points."""
    shapes, P, crop, stride, Q = [(52, 56), (40, 70)], 8, (32, 32), (2, 2), 3
    l, r, t, b = compute_padsize(32, 32, P)
    up = (32 + t + b, 32 + l + r)
    wins, tile_image, image_tiles = [], [], []
    for n, (H, W) in enumerate(shapes):
        w = tile_windows(H, W, stride, crop)
        assert max(sum(y1 < by + 4 and y2 > by and x1 < bx + 64 and x2 > bx for (y1, y2, x1, x2) in w)
                   for by in range(0, H, 4) for bx in range(0, W, 64)) > 64
        image_tiles.append((len(wins), len(w)))
        wins += w
        tile_image += [n] * len(w)
    tl = rand((len(wins), Q, up[0] // P, up[1] // P), 19).to(DEV)
    qi, K = torch.tensor([0, 1, 1]), 2
    _, views = ops.stitch_multi(tl, wins, tile_image, up, (t, l), shapes, image_tiles)
    lab, _, conf = ops.label_head_multi(tl, wins, tile_image, up, (t, l), shapes, image_tiles, qi, K, 50.0, 0.3, 0, want_conf=True)
    for n, (H, W) in enumerate(shapes):
        a, c = image_tiles[n]
        win = torch.tensor(wins[a:a + c], dtype=torch.int32)
        assert torch.equal(views[n], ops.stitch(tl[a:a + c], win, up, (t, l), (H, W))), f"canvas of image {n}"
        rl, rc = ops.label_head(tl[a:a + c], win, up, (t, l), (H, W), qi, K, 50.0, 0.3, 0, want_conf=True)
        assert torch.equal(lab[n], rl), f"labels of image {n}"
        assert torch.equal(conf[n], rc), f"conf of image {n}"


# ---- 2. sg_postprocess_multi == sg_resize_bilinear + sg_postprocess per image --------------------------------------------------
# Q = 17 and 40 run the kernels' 64-query instantiation (odd and even Q, one class per query and about Q / 2 classes)
@pytest.mark.parametrize("qidx", [QIDX, [0, 1, 2, 3, 4], list(range(17)), [q // 2 for q in range(17)], list(range(40)),
                                  [q // 2 for q in range(40)]],
                         ids=["synonyms", "one_per_class", "q17_one_per_class", "q17_synonyms", "q40_one_per_class", "q40_synonyms"])
@pytest.mark.parametrize("prob_thd", [0.0, 0.3])
@pytest.mark.parametrize("want_probs", [True, False])
def test_postprocess_multi_equals_resize_and_postprocess(qidx, prob_thd, want_probs):
    canvas_hw = [(60, 76), (36, 36), (50, 90), (30, 28), (80, 52)]
    out_hw = [(60, 76), (45, 31), (50, 90), (67, 70), (33, 52)]        # same size (no resize) for two, resized for three
    Q, K = len(qidx), max(qidx) + 1
    if Q > 16:                                                          # small canvases: one image resized, one not
        canvas_hw, out_hw = [(40, 50), (23, 31)], [(40, 50), (37, 29)]
    qi = torch.tensor(qidx)
    canv = [rand((Q, h, w), 50 + n, 0.05).to(DEV) for n, (h, w) in enumerate(canvas_hw)]
    flat = torch.cat([c.reshape(-1) for c in canv])
    prb, lab = ops.postprocess_multi(flat, canvas_hw, qi, K, 50.0, prob_thd, 5 if K > 5 else 0, out_hw, want_probs)
    n_bg = 0
    for n, (c, o) in enumerate(zip(canv, out_hw)):
        src = ops.resize_bilinear(c, o) if tuple(o) != tuple(c.shape[1:]) else c
        rp, rl = ops.postprocess(src, qi, K, 50.0, prob_thd, 5 if K > 5 else 0, want_probs)
        assert torch.equal(lab[n], rl), f"labels of image {n}"
        if want_probs:
            assert torch.equal(prb[n], rp), f"probs of image {n}"
        else:
            assert prb[n] is None
        n_bg += int((rl == (5 if K > 5 else 0)).sum())
    assert 0 < n_bg < sum(h * w for h, w in out_hw)


# ---- 3 / 4. the packed pipeline == forward_slide per image (f32) ----------------------------------------------------------------
def tiny_pipe(kind, precision="f32", tiles_per_launch=7):
    if kind == "jbu":
        from clip_decontamination_amd.upsampler import HipJBU
        cfg = Wt.vit_config("tiny-16")
        up = HipJBU("jbu_stack", cfg.embed_dim, "cuda:0", precision)
        up.load_state_dict(Wt.make_jbu_weights("jbu_stack", cfg.embed_dim, seed=3))
        tower = HipVisionTower(cfg, Wt.make_vit_weights(cfg, seed=0), precision=precision, device=DEV)
        text = torch.from_numpy(Wt.make_text_features(len(QIDX), cfg.embed_dim))
        return SegPipeline(HipCLIP(tower), text, torch.tensor(QIDX), model_type="SegEarth", global_debias_factor=0.2, prob_thd=0.1,
                           bg_idx=5, upsampler=up, tiles_per_launch=tiles_per_launch), (32, 48)
    cfg = Wt.vit_config("tiny-8")
    tower = HipVisionTower(cfg, Wt.make_vit_weights(cfg, seed=0), precision=precision, device=DEV)
    text = torch.from_numpy(Wt.make_text_features(len(QIDX), cfg.embed_dim))
    kw = dict(model_type="Experimental", global_debias_factor=0.2, prob_thd=0.1, bg_idx=5, tiles_per_launch=tiles_per_launch)
    if kind in ("refine_ctd", "refine", "sim"):
        tower.similarity_enhancer = SimilarityEnhancementModule(**SIM)
        if kind != "sim":
            tower.outlier_suppressor = OutlierSuppressionModule(top_k=6)
        kw.update(apply_similarity_enhancement=True, apply_ctd=kind == "refine_ctd")
    elif kind == "fusion":
        kw.update(model_type="SegEarth", cross_tile_fusion=dict(fusion_mode="weighted", cache_boundary_width=2, fusion_strength=0.3))
    return SegPipeline(HipCLIP(tower), text, torch.tensor(QIDX), **kw), (20, 36)


def per_image(pipe, imgs, stride, crop):
    return [pipe.forward_slide(s, stride, crop) for s in imgs]


@pytest.mark.parametrize("kind", ["refine_ctd", "jbu", "fusion"])
@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_forward_slide_many_equals_forward_slide(kind, fmt):
    pipe, (stride, crop) = tiny_pipe(kind)
    shapes = SHAPES if kind != "jbu" else [(64, 96), (48, 48), (80, 56), (40, 44), (100, 60)]
    imgs = scenes(fmt, shapes, seed=11)
    ref = per_image(pipe, imgs, stride, crop)
    ori = [None, (41, 40), None, (30, 28), (90, 50)]
    got = pipe.forward_slide_many(imgs, stride, crop)
    got_ori = pipe.forward_slide_many(imgs, stride, crop, ori_shapes=ori)
    for n, r in enumerate(ref):
        assert torch.equal(got[n], r), f"{kind} {fmt}: image {n}"
        want = r if ori[n] is None or tuple(ori[n]) == tuple(r.shape[-2:]) else ops.resize_bilinear(r[0], ori[n]).unsqueeze(0)
        assert torch.equal(got_ori[n], want), f"{kind} {fmt}: image {n} resized"
    labels = pipe.segment_scenes(imgs, stride, crop)
    for n, r in enumerate(ref):
        assert torch.equal(labels[n], pipe.postprocess(r[0], want_probs=False)[1])


@pytest.mark.parametrize("kind", ["refine", "jbu"])
@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_pack_buffer_padding_is_never_read(kind, fmt):
    pipe, (stride, crop) = tiny_pipe(kind)
    shapes = SHAPES if kind != "jbu" else [(64, 96), (48, 48), (80, 56), (40, 44), (100, 60)]
    imgs = scenes(fmt, shapes, seed=17)
    ref = per_image(pipe, imgs, stride, crop)
    pipe.pack_fill = 255 if fmt == "u8" else float("nan")
    got = pipe.forward_slide_many(imgs, stride, crop)
    for n, r in enumerate(ref):
        assert torch.equal(got[n], r), f"{kind} {fmt}: image {n}"
        assert not torch.isnan(got[n]).any()


def test_batch_tensor_is_used_in_place():
    pipe, (stride, crop) = tiny_pipe("refine")
    batch = rand((3, 3, 50, 70), 23).to(DEV)
    got = pipe.forward_slide_many(batch, stride, crop)
    for n in range(3):
        assert torch.equal(got[n], pipe.forward_slide(batch[n], stride, crop))


# ---- 5. 2-byte modes against the oracle ----------------------------------------------------------------------------------------
# the bounds smoke() holds the tiny tower to in each mode (f16x2 carries the exact-mode bar: 1e-3, labels equal up to oracle ties).  The
# outlier suppressor is left out here: its top-k selection flips on 2-byte rounding of near-equal scores, which moves whole tokens.
TOL = {"f16x2": (1e-3, 1.0), "bf16": (1.2e-2, 0.992), "f16": (7.5e-4, 0.9986)}


def labels_match_up_to_ties(pred, ref_logits, oracle):
    probs, ref_pred = oracle.postprocess(ref_logits)
    bad = (pred != ref_pred)[0]
    if not bool(bad.any()):
        return True
    pmax = probs.max(0)[0][bad]
    ours = probs[:, bad].gather(0, pred[0][bad][None])[0]
    return bool((((pmax - ours).abs() < 1e-4) | ((pmax - oracle.prob_thd).abs() < 1e-4)).all())


@pytest.mark.parametrize("prec", ["f16x2", "bf16", "f16"])
def test_two_byte_modes_packed_vs_oracle(prec):
    pipe, (stride, crop) = tiny_pipe("sim", precision=prec, tiles_per_launch=64)
    imgs = scenes("f32", SHAPES, seed=29)
    got = pipe.forward_slide_many(imgs, stride, crop)
    cfg = pipe.visual.cfg
    o = OS.SegOracle(cfg, OV.to_torch(Wt.make_vit_weights(cfg, seed=0)), pipe.text.cpu(), torch.tensor(QIDX), model_type="Experimental",
                     global_debias_factor=0.2, similarity_cfg=SIM, prob_thd=0.1, bg_idx=5, slide_crop=crop, slide_stride=stride)
    tol, floor = TOL[prec]
    agree, total, err, err_one = 0, 0, 0.0, 0.0
    for n, s in enumerate(imgs):
        with torch.no_grad():
            ref = o.forward_slide(s.cpu()[None])
        err = max(err, (got[n].cpu() - ref).abs().max().item())
        err_one = max(err_one, (pipe.forward_slide(s, stride, crop).cpu() - ref).abs().max().item())
        pred = pipe.postprocess(got[n][0], want_probs=False)[1].cpu()
        agree += int((pred == o.postprocess(ref[0])[1]).sum())
        total += pred.numel()
        if prec == "f16x2":
            assert labels_match_up_to_ties(pred, ref[0], o), f"image {n}: label mismatch away from a tie"
    print(f"[packed {prec}] max|dlogit| = {err:.2e} (per-image path {err_one:.2e}), label agreement = {agree / total:.4f}")
    assert err < tol and agree / total >= floor


# ---- 6. launch count ------------------------------------------------------------------------------------------------------------
def test_one_launch_of_each_for_a_packed_batch(monkeypatch):
    pipe, (stride, crop) = tiny_pipe("refine", tiles_per_launch=64)
    imgs = scenes("u8", [(56, 56)] * 12, seed=3)                       # 4 windows each at crop 36 / stride 20: 48 tiles
    assert len(tile_windows(56, 56, (stride, stride), (crop, crop))) == 4
    calls = {"tower": 0, "stitch_multi": 0, "postprocess_multi": 0}

    def counted(name, fn):
        def wrap(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrap

    monkeypatch.setattr(HipVisionTower, "forward_tiles", counted("tower", HipVisionTower.forward_tiles))
    monkeypatch.setattr(ops, "stitch_multi", counted("stitch_multi", ops.stitch_multi))
    monkeypatch.setattr(ops, "postprocess_multi", counted("postprocess_multi", ops.postprocess_multi))
    labels = pipe.segment_scenes(imgs, stride, crop)
    assert calls == {"tower": 1, "stitch_multi": 1, "postprocess_multi": 1}
    assert len(labels) == 12 and all(tuple(x.shape) == (1, 56, 56) for x in labels)


def test_tile_group_is_refused_by_the_packed_path():
    pipe, (stride, crop) = tiny_pipe("refine")
    pipe.tile_group = "world"
    with pytest.raises(ValueError, match="per image"):
        pipe.forward_slide_many(scenes("f32", SHAPES[:2]), stride, crop)


# ---- 7. drop-in predict_many == predict per sample -----------------------------------------------------------------------------
class Sample:
    def __init__(self, meta):
        self.metainfo = meta
        self.data = {}

    def set_data(self, d):
        self.data.update(d)


def build_seg(tmp_path=None, **kw):
    import segmentor
    cfg = Wt.vit_config("tiny-8")
    maps = dict(result_dir=str(tmp_path / "res"), heatmap_dir=str(tmp_path / "heat")) if tmp_path is not None else {}
    return segmentor.SegmentorEx(clip_type="CLIP", vit_type="tiny-8", model_type="Experimental",
                                 name_path=os.path.join(ROOT, "configs", "cls_potsdam.txt"), device=DEV, precision="f32", synthetic_ok=True,
                                 text_features=torch.from_numpy(Wt.make_text_features(len(QIDX), cfg.embed_dim)), global_debias_factor=0.2,
                                 apply_outlier_suppression=True, outlier_suppression_cfg=dict(top_k=6), prob_thd=0.1, bg_idx=5,
                                 slide_crop=36, slide_stride=20, tiles_per_launch=9, **maps, **kw)


def test_predict_many_equals_predict(tmp_path):
    imgs = [rand((3, h, w), 40 + n).to(DEV) for n, (h, w) in enumerate(SHAPES)]
    oris = [(60, 76), (40, 33), (50, 90), (30, 28), (64, 64)]
    a = build_seg(tmp_path / "one")
    b = build_seg(tmp_path / "many")
    one = [a.predict(x[None], [Sample(dict(ori_shape=o, img_path=f"/d/tile_{n}.tif"))])[0] for n, (x, o) in enumerate(zip(imgs, oris))]
    many = b.predict_many(imgs, [Sample(dict(ori_shape=o, img_path=f"/d/tile_{n}.tif")) for n, o in enumerate(oris)])
    for n, (s1, s2) in enumerate(zip(one, many)):
        for key in ("seg_logits", "pred_sem_seg"):
            assert torch.equal(s1.data[key].data, s2.data[key].data), f"{key} of sample {n}"
        for d in ("res", "heat"):
            f1, f2 = tmp_path / "one" / d / f"tile_{n}.png", tmp_path / "many" / d / f"tile_{n}.png"
            assert f1.read_bytes() == f2.read_bytes()
    labels = b.predict_many(imgs)                                      # no data samples: one label map per image
    for n, x in enumerate(imgs):
        assert torch.equal(labels[n], a.predict(x[None], None))


def test_pack_images_routes_predict(monkeypatch):
    batch = rand((3, 3, 50, 70), 61).to(DEV)
    calls = []
    orig = SegPipeline.forward_slide_many
    monkeypatch.setattr(SegPipeline, "forward_slide_many", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    off = build_seg()
    per = off.predict(batch, [Sample(dict(ori_shape=(50, 70))) for _ in range(3)])
    assert calls == []                                                  # default: the per-image loop
    on = build_seg(pack_images=True)
    packed = on.predict(batch, [Sample(dict(ori_shape=(50, 70))) for _ in range(3)])
    assert calls == [1]
    for s1, s2 in zip(per, packed):
        assert torch.equal(s1.data["pred_sem_seg"].data, s2.data["pred_sem_seg"].data)
        assert torch.equal(s1.data["seg_logits"].data, s2.data["seg_logits"].data)


# ---- 8. the launch shape at real size ---------------------------------------------------------------------------------------------
def test_l14_512_sixteen_images_one_launch_f16x2(monkeypatch):
    """16 single-window 512^2 images in ONE tower launch (8,208 tokens per GEMM: the persistent folded-LayerNorm kernels a one-tile
    launch never reaches), f16x2, against the oracle on images 0 and 15."""
    cfg = Wt.vit_config("ViT-L/14")
    wnp = Wt.make_vit_weights(cfg, seed=0)
    qidx = [0, 0, 1, 2, 3, 4, 5, 5]
    text = torch.from_numpy(Wt.make_text_features(len(qidx), cfg.embed_dim))
    pipe = SegPipeline(HipCLIP(HipVisionTower(cfg, wnp, precision="f16x2", device=DEV)), text, torch.tensor(qidx), model_type="SegEarth",
                       global_debias_factor=0.2, prob_thd=0.1, bg_idx=5, tiles_per_launch=119)
    u8 = Wt.make_tiles_u8(16, 512, seed=5, smooth=True)                # [16,3,512,512]
    batch = torch.from_numpy(Wt.normalize_tiles(u8)).to(DEV)
    calls = []
    orig = HipVisionTower.forward_tiles
    monkeypatch.setattr(HipVisionTower, "forward_tiles", lambda self, *a, **k: calls.append(a[1].shape[0]) or orig(self, *a, **k))
    got = pipe.forward_slide_many(batch, 512, 512)
    assert calls == [16]
    o = OS.SegOracle(cfg, OV.to_torch(wnp), text, torch.tensor(qidx), model_type="SegEarth", global_debias_factor=0.2, prob_thd=0.1,
                     bg_idx=5, slide_crop=512, slide_stride=512)
    for n in (0, 15):
        with torch.no_grad():
            ref = o.forward_slide(batch[n:n + 1].cpu())
        err = (got[n].cpu() - ref).abs().max().item()
        pred = pipe.postprocess(got[n][0], want_probs=False)[1].cpu()
        print(f"[L/14 512 x16 f16x2] image {n}: max|dlogit| = {err:.2e}")
        assert err < 1e-3
        assert labels_match_up_to_ties(pred, ref[0], o), f"image {n}: label mismatch away from a tie"
