"""sg_confusion_accumulate, IoUMetric and the segmentors' evaluate() on the GPU.  The bar is EXACT integer equality of the whole
(K+1) x (K+1) table with the CPU reference (tests/iou_reference.py: mmseg's formula on integer histograms) -- counts are integers
end to end, so there is no tolerance anywhere in this file."""
import os

import numpy as np
import pytest
import torch

import iou_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POTSDAM = os.path.join(ROOT, "configs", "cls_potsdam.txt")
SHAPES = [(1, 1), (37, 53), (1024, 1024), (2999, 3001)]
KS = [1, 2, 6, 16, 64]


def np_gt(gt, fmt):
    return gt.astype(np.uint8) if fmt == "u8" else gt.astype(np.int64)


def count(pred, gt, K, fmt, ignore_index=255, rzl=False, table=None):
    """One sg_confusion_accumulate call on device copies of (pred, gt) -> the table as numpy."""
    from clip_decontamination_amd import ops
    lab = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.int64)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(np_gt(gt, fmt))).cuda()
    t = torch.zeros(K + 1, K + 1, dtype=torch.int64, device="cuda") if table is None else table
    out = ops.confusion_accumulate(lab, g, t, K, ignore_index, rzl)
    assert out is t
    return t.cpu().numpy()


def random_maps(seed, shape, K, ignore_index=255):
    """Uniformly random labels in [0,K) and truth over [0,K), the ignore index, 0 and 255 (the reduce_zero_label boundary values)."""
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, K, size=shape)
    vals = np.concatenate([np.arange(K), [ignore_index, 0, 1, 254, 255]])
    gt = rng.choice(vals, size=shape)
    return pred.astype(np.int64), gt.astype(np.int64)


def blocky_maps(seed, shape, K, block=64):
    """Constant block x block squares, as real masks are; prediction and truth disagree on about a quarter of the squares."""
    rng = np.random.default_rng(seed)
    gh, gw = -(-shape[0] // block), -(-shape[1] // block)
    gt_b = rng.integers(0, K, size=(gh, gw))
    pred_b = np.where(rng.random((gh, gw)) < 0.25, rng.integers(0, K, size=(gh, gw)), gt_b)
    gt_b = np.where(rng.random((gh, gw)) < 0.1, 255, gt_b)
    up = lambda a: np.kron(a, np.ones((block, block), dtype=np.int64))[:shape[0], :shape[1]]
    return up(pred_b).astype(np.int64), up(gt_b).astype(np.int64)


# ---- 1. the kernel against the reference: shapes x K x truth format x reduce_zero_label x ignore_index ---------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("K", KS)
def test_random_maps_equal_the_reference(shape, K):
    for ignore_index in (255, 3):
        pred, gt = random_maps(shape[0] * 7 + K, shape, K, ignore_index)
        for rzl in (False, True):
            want = R.confusion_table(pred, gt, K, ignore_index, rzl)
            for fmt in ("u8", "i64"):
                got = count(pred, gt, K, fmt, ignore_index, rzl)
                assert got.dtype == np.int64 and np.array_equal(got, want), (shape, K, fmt, rzl, ignore_index)
            # the three mmseg areas are the table's diagonal and margins
            from clip_decontamination_amd.metrics import areas_from_confusion
            for a, b in zip(areas_from_confusion(want), R.intersect_and_union(pred, gt, K, ignore_index, rzl)):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("fmt", ["u8", "i64"])
def test_blocky_maps_equal_the_reference(shape, K, fmt):
    pred, gt = blocky_maps(K, shape, K)
    for rzl in (False, True):
        assert np.array_equal(count(pred, gt, K, fmt, 255, rzl), R.confusion_table(pred, gt, K, 255, rzl)), rzl


@pytest.mark.parametrize("fmt", ["u8", "i64"])
def test_uniform_map_one_bin(fmt):
    """16.7 M pixels in one bin: the contention case (every lane of every wave on one LDS address without the aggregation) and the
    32-bit-partial case (2^24 counts folded into the int64 table)."""
    K, n = 6, 4096
    pred = np.full((n, n), 2, dtype=np.int64)
    gt = np.full((n, n), 2, dtype=np.int64)
    got = count(pred, gt, K, fmt)
    want = np.zeros((K + 1, K + 1), dtype=np.int64)
    want[2, 2] = n * n
    assert np.array_equal(got, want)
    gt[:] = 4                                                        # all wrong, still one bin
    want[:] = 0
    want[2, 4] = n * n
    assert np.array_equal(count(pred, gt, K, fmt), want)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("fmt", ["u8", "i64"])
def test_out_of_range_predictions_and_truths(K, fmt):
    rng = np.random.default_rng(K)
    shape = (257, 129)
    pred = rng.choice(np.concatenate([np.arange(K), [K, K + 1, 1000, -1, -7, 1 << 40]]), size=shape).astype(np.int64)
    hi = [K, K + 2, 200, 254] if fmt == "u8" else [K, K + 2, 200, 254, 256, 70000, -1, -255, 1 << 33]
    gt = rng.choice(np.concatenate([np.arange(K), hi, [255]]), size=shape).astype(np.int64)
    for ignore_index in (255, 200):
        for rzl in (False, True):
            want = R.confusion_table(pred, gt, K, ignore_index, rzl)
            assert want[K, :].sum() > 0 and want[:, K].sum() > 0
            assert np.array_equal(count(pred, gt, K, fmt, ignore_index, rzl), want), (ignore_index, rzl)


def test_reduce_zero_label_boundary_values_on_the_device():
    K = 254
    gt = np.array([0, 1, 254, 255] * 5, dtype=np.int64)
    pred = np.array([0, 0, 253, 253] * 5, dtype=np.int64)
    for fmt in ("u8", "i64"):
        for ignore_index in (255, 253):
            assert K > 127                                           # beyond the LDS table: refused with the reason, not miscounted
            with pytest.raises(RuntimeError, match="exceeds 127"):
                count(pred, gt, K, fmt, ignore_index, True)
    K = 127                                                          # the largest K the entry takes
    pred = np.array([0, 0, 126, 126, 5] * 4, dtype=np.int64)
    gt = np.array([0, 1, 127, 255, 254] * 4, dtype=np.int64)
    for fmt in ("u8", "i64"):
        for ignore_index in (255, 126, 253):
            want = R.confusion_table(pred, gt, K, ignore_index, True)
            assert np.array_equal(count(pred, gt, K, fmt, ignore_index, True), want), (fmt, ignore_index)


# ---- 2. buffer alignment, accumulation, empty input, streams, repeats ---------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "i64"])
def test_buffers_offset_from_their_allocation(fmt):
    """The flush-group case: label and truth slices that start an odd number of elements into their allocations, at lengths around
    the 16-pixel run (shorter than the unaligned head included)."""
    from clip_decontamination_amd import ops
    K = 6
    for n in (1, 5, 15, 16, 17, 31, 33, 1000, 100003):
        for lo, go in ((1, 1), (3, 7), (5, 13), (7, 15), (0, 9), (1, 0)):
            pred, gt = random_maps(n + lo + 16 * go, (n,), K)
            lab_buf = torch.full((n + lo + 2,), K + 5, dtype=torch.int64, device="cuda")
            gt_buf = torch.full((n + go + 2,), 1, dtype=torch.uint8 if fmt == "u8" else torch.int64, device="cuda")
            lab, g = lab_buf[lo:lo + n], gt_buf[go:go + n]
            lab.copy_(torch.from_numpy(pred))
            g.copy_(torch.from_numpy(np_gt(gt, fmt)))
            t = torch.zeros(K + 1, K + 1, dtype=torch.int64, device="cuda")
            ops.confusion_accumulate(lab, g, t, K)
            assert np.array_equal(t.cpu().numpy(), R.confusion_table(pred, gt, K)), (n, lo, go)


def test_two_calls_accumulate_and_empty_input_is_a_no_op():
    from clip_decontamination_amd import ops
    K = 16
    a, b = random_maps(1, (301, 211), K), blocky_maps(2, (512, 300), K)
    t = torch.zeros(K + 1, K + 1, dtype=torch.int64, device="cuda")
    count(*a, K, "u8", table=t)
    got = count(*b, K, "i64", table=t)
    want = R.confusion_table(*a, K) + R.confusion_table(*b, K)
    assert np.array_equal(got, want)
    ops.confusion_accumulate(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.uint8, device="cuda"), t, K)
    ops.confusion_accumulate(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), t, K)
    assert np.array_equal(t.cpu().numpy(), want)


def test_binding_refuses_mismatched_shapes_and_wrong_types():
    from clip_decontamination_amd import ops
    t = torch.zeros(7, 7, dtype=torch.int64, device="cuda")
    lab = torch.zeros(4, 5, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="differ in shape"):
        ops.confusion_accumulate(lab, torch.zeros(5, 4, dtype=torch.uint8, device="cuda"), t, 6)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.confusion_accumulate(lab, torch.zeros(21, dtype=torch.uint8, device="cuda"), t, 6)
    with pytest.raises(TypeError):
        ops.confusion_accumulate(lab.int(), torch.zeros(4, 5, dtype=torch.uint8, device="cuda"), t, 6)
    with pytest.raises(TypeError):
        ops.confusion_accumulate(lab, torch.zeros(4, 5, dtype=torch.int32, device="cuda"), t, 6)
    with pytest.raises(ValueError, match="table"):
        ops.confusion_accumulate(lab, torch.zeros(4, 5, dtype=torch.uint8, device="cuda"), t, 5)
    ops.confusion_accumulate(lab[None], torch.zeros(4, 5, dtype=torch.uint8, device="cuda"), t, 6)        # [1,H,W] labels, [H,W] truth
    assert int(t[0, 0]) == 20 and int(t.sum()) == 20


def test_non_default_stream_and_repeats_are_byte_identical():
    from clip_decontamination_amd import ops
    K = 6
    pred, gt = random_maps(9, (1024, 1024), K)
    bp, bg = blocky_maps(9, (1024, 1024), K)
    for p, g in ((pred, gt), (bp, bg)):
        first = count(p, g, K, "u8")
        for _ in range(3):
            assert count(p, g, K, "u8").tobytes() == first.tobytes()
        lab, gd = torch.from_numpy(p).cuda(), torch.from_numpy(np_gt(g, "u8")).cuda()
        t = torch.zeros(K + 1, K + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ops.confusion_accumulate(lab, gd, t, K)
        s.synchronize()
        assert t.cpu().numpy().tobytes() == first.tobytes()
        assert np.array_equal(first, R.confusion_table(p, g, K))


# ---- 3. the metric object ---------------------------------------------------------------------------------------------------------
def test_metric_add_process_reset_compute():
    from clip_decontamination_amd.metrics import IoUMetric
    K = 6
    pairs = [random_maps(20 + i, s, K) for i, s in enumerate([(40, 56), (33, 71), (64, 64)])]
    kw = dict(num_classes=K, iou_metrics=["mIoU", "mDice", "mFscore"], beta=2)
    m = IoUMetric(**kw)
    for p, g in pairs:
        m.add(torch.from_numpy(p).cuda()[None], torch.from_numpy(g.astype(np.uint8)).cuda())
    assert m.confusion.is_cuda                                       # the table stays on the device until compute()
    want = sum(R.confusion_table(p, g, K) for p, g in pairs)
    assert np.array_equal(m.confusion.cpu().numpy(), want)
    ref = R.iou_metrics(pairs, K, metrics=("mIoU", "mDice", "mFscore"), beta=2)
    got = m.compute()
    assert got["summary"] == ref["summary"]
    for k in ("IoU", "Acc", "Dice", "Fscore", "Precision", "Recall"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k

    class Data:
        def __init__(self, data):
            self.data = data

    class Sample:
        def __init__(self, pred, gt):
            self.pred_sem_seg, self.gt_sem_seg = Data(pred), Data(gt)

    dict_style, obj_style = IoUMetric(**kw), IoUMetric(**kw)
    dict_style.process(None, [{"pred_sem_seg": {"data": torch.from_numpy(p).cuda()[None]}, "gt_sem_seg": {"data": torch.from_numpy(g)[None]}}
                              for p, g in pairs])
    obj_style.process(None, [Sample(torch.from_numpy(p).cuda()[None], torch.from_numpy(g.astype(np.uint8)).cuda()[None]) for p, g in pairs])
    assert torch.equal(dict_style.confusion, m.confusion) and torch.equal(obj_style.confusion, m.confusion)
    m.reset()
    assert int(m.confusion.sum()) == 0


def test_metric_with_reduce_zero_label_and_other_ignore_index():
    from clip_decontamination_amd.metrics import IoUMetric
    K = 5
    pred, gt = random_maps(31, (97, 103), K, ignore_index=7)
    m = IoUMetric(ignore_index=7, num_classes=K, reduce_zero_label=True)
    m.add(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())
    assert np.array_equal(m.confusion.cpu().numpy(), R.confusion_table(pred, gt, K, 7, True))
    assert m.compute()["summary"] == R.iou_metrics([(pred, gt)], K, 7, True)["summary"]


# ---- 4. evaluate() end to end on the tiny synthetic tower ---------------------------------------------------------------------------
def build(cls_name, **kw):
    import segearth_segmentor
    import segmentor
    from clip_decontamination_amd import weights as Wt
    cls = segmentor.SegmentorEx if cls_name == "SegmentorEx" else segearth_segmentor.Segmentor
    text = torch.from_numpy(Wt.make_text_features(8, Wt.vit_config("tiny-8").embed_dim))
    return cls(clip_type="CLIP", vit_type="tiny-8", name_path=POTSDAM, device=torch.device("cuda:0"), precision="f32",
               synthetic_ok=True, text_features=text, **kw)


def images_and_truth(seed, sizes, K, as_numpy=False):
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(rng.standard_normal((3, h, w), dtype=np.float32)).cuda() for h, w in sizes]
    gts = [rng.choice(np.concatenate([np.arange(K), [255, K]]), size=(h, w)).astype(np.uint8) for h, w in sizes]
    return imgs, (gts if as_numpy else [torch.from_numpy(g) for g in gts])


SEG_CASES = {
    "SegmentorEx": dict(model_type="SegEarth", global_debias_factor=0.2, prob_thd=0.3, bg_idx=5, slide_crop=32, slide_stride=16),
    "Segmentor": dict(model_type="SegEarth", cls_token_lambda=-0.3, prob_thd=0.3, bg_idx=4, slide_crop=32, slide_stride=16,
                      apply_sim_feat_up=False),
}


@pytest.mark.parametrize("cls_name", list(SEG_CASES))
def test_evaluate_equals_the_reference_on_predicts_labels(cls_name):
    """In f32 the packed path equals the per-image path bit for bit, so evaluate()'s table must equal, exactly, the reference
    applied to the labels predict() returns.  The sizes put an image smaller than the crop (a tile-size group of its own) between
    the others, so one flush group's images are not neighbours in the call."""
    seg = build(cls_name, **SEG_CASES[cls_name])
    K = seg.num_classes
    sizes = [(56, 56), (30, 34), (40, 72), (64, 48)]
    imgs, gts = images_and_truth(5, sizes, K)
    # prob_thd is read at call time: set it to the median winning probability of these images, so that about half of the pixels are
    # thresholded to bg_idx whatever the synthetic tower's confidence is
    seg.prob_thd = 0.0
    free = [seg._pipeline().postprocess(seg.forward_slide(im[None], None, 16, 32)[0]) for im in imgs]
    seg.prob_thd = float(torch.cat([p.max(0).values.reshape(-1) for p, _ in free]).median())
    preds = [seg.predict(im[None], None).cpu().numpy() for im in imgs]
    bg = SEG_CASES[cls_name]["bg_idx"]
    moved = [p[0] != l[0].cpu().numpy() for p, (_, l) in zip(preds, free)]
    assert sum(int(m.sum()) for m in moved) > 0, "prob_thd moved no pixel to bg_idx: the case would test nothing"
    assert all((p[0][m] == bg).all() for p, m in zip(preds, moved))
    want = sum(R.confusion_table(p, g.numpy(), K) for p, g in zip(preds, gts))
    res, metric = seg.evaluate(imgs, gts)
    assert np.array_equal(metric.confusion.cpu().numpy(), want)
    assert res["summary"] == R.iou_metrics([(p, g.numpy()) for p, g in zip(preds, gts)], K)["summary"]
    assert set(res) == {"aAcc", "IoU", "Acc", "summary"} and len(res["IoU"]) == K
    # a dataset loop: the metric passed back in accumulates; numpy [1,H,W] int64 truth this time
    imgs2, gts2 = images_and_truth(6, [(48, 48), (36, 60)], K, as_numpy=True)
    preds2 = [seg.predict(im[None], None).cpu().numpy() for im in imgs2]
    res2, metric2 = seg.evaluate(imgs2, [g.astype(np.int64)[None] for g in gts2], metric=metric)
    assert metric2 is metric
    want2 = want + sum(R.confusion_table(p, g, K) for p, g in zip(preds2, gts2))
    assert np.array_equal(metric.confusion.cpu().numpy(), want2)
    pairs = [(p, g.numpy()) for p, g in zip(preds, gts)] + list(zip(preds2, gts2))
    assert res2["summary"] == R.iou_metrics(pairs, K)["summary"]


def test_evaluate_options_batch_input_and_refusals():
    seg = build("SegmentorEx", **SEG_CASES["SegmentorEx"])
    K = seg.num_classes
    rng = np.random.default_rng(8)
    batch = torch.from_numpy(rng.standard_normal((3, 3, 48, 64), dtype=np.float32)).cuda()
    gts = [rng.integers(0, K + 1, size=(48, 64)).astype(np.uint8) for _ in range(3)]
    preds = [seg.predict(batch[i][None], None).cpu().numpy() for i in range(3)]
    res, metric = seg.evaluate(batch, gts, reduce_zero_label=True, ignore_index=2, iou_metrics=("mDice", "mFscore"))
    want = sum(R.confusion_table(p, g, K, 2, True) for p, g in zip(preds, gts))
    assert np.array_equal(metric.confusion.cpu().numpy(), want)
    assert res["summary"] == R.iou_metrics(list(zip(preds, gts)), K, 2, True, metrics=("mDice", "mFscore"))["summary"]
    with pytest.raises(ValueError, match="ground-truth maps"):
        seg.evaluate(batch, gts[:2])
    with pytest.raises(ValueError, match="has shape"):
        seg.evaluate(batch, [g.T for g in gts])
    from clip_decontamination_amd.metrics import IoUMetric
    with pytest.raises(ValueError, match="classes"):
        seg.evaluate(batch, gts, metric=IoUMetric(num_classes=K + 1))
    seg.tile_group = "world"
    with pytest.raises(ValueError, match="tile_group"):
        seg.evaluate(batch, gts)


def test_evaluate_whole_image_inference():
    """slide_crop <= 0: no windows to pack, image by image through predict()."""
    kw = dict(SEG_CASES["SegmentorEx"], slide_crop=0)
    seg = build("SegmentorEx", **kw)
    K = seg.num_classes
    imgs, gts = images_and_truth(11, [(32, 48), (40, 40)], K)
    preds = [seg.predict(im[None], None).cpu().numpy() for im in imgs]
    _, metric = seg.evaluate(imgs, gts)
    assert np.array_equal(metric.confusion.cpu().numpy(), sum(R.confusion_table(p, g.numpy(), K) for p, g in zip(preds, gts)))


def test_against_mmseg_when_installed():
    mmseg_metrics = pytest.importorskip("mmseg.evaluation.metrics")
    K = 6
    pred, gt = random_maps(77, (300, 200), K)
    a = mmseg_metrics.IoUMetric.intersect_and_union(torch.from_numpy(pred), torch.from_numpy(gt), K, 255)
    for x, y in zip(a, R.intersect_and_union(pred, gt, K)):
        assert np.array_equal(x.numpy().astype(np.int64), y)
    assert np.array_equal(count(pred, gt, K, "u8"), R.confusion_table(pred, gt, K))
