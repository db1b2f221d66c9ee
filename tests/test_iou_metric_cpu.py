"""The IoU metric's host side without a GPU: metrics_from_confusion against mmseg's formula restated with integer histograms
(tests/iou_reference.py), the reduce_zero_label mapping, construction from the shipped config line, reduce() over a gloo group, and
the refusals of sg_confusion_accumulate (argument checks run before any device work)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import iou_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_case(seed, K, shape=(61, 47), ignore_index=255, p_ignore=0.1, p_gt_out=0.05, p_pred_out=0.05, absent=None):
    """Label maps with ignored pixels, truth values >= K that are not the ignore index, predictions >= K, and (``absent``) a class
    that occurs in neither."""
    rng = np.random.default_rng(seed)
    classes = np.array([k for k in range(K) if k != absent])
    pred = rng.choice(classes, size=shape)
    gt = rng.choice(classes, size=shape)
    out_gt = np.array([v for v in (K, K + 3, 200, 254) if v != ignore_index])
    gt = np.where(rng.random(shape) < p_gt_out, rng.choice(out_gt, size=shape), gt)
    gt = np.where(rng.random(shape) < p_ignore, ignore_index, gt)
    pred = np.where(rng.random(shape) < p_pred_out, rng.choice([K, K + 1, 1000], size=shape), pred)
    return pred.astype(np.int64), gt.astype(np.int64)


def assert_same_metrics(got, want):
    assert set(got) == set(want)
    for k in want:
        if k == "summary":
            assert set(got[k]) == set(want[k])
            for m in want[k]:
                assert np.array_equal(np.float64(got[k][m]), np.float64(want[k][m]), equal_nan=True), (m, got[k][m], want[k][m])
        else:
            assert np.array_equal(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64), equal_nan=True), k


ALL = ("mIoU", "mDice", "mFscore")


@pytest.mark.parametrize("K", [1, 2, 6, 16])
@pytest.mark.parametrize("ignore_index", [255, 3])
@pytest.mark.parametrize("metrics,beta,nan_to_num", [(("mIoU",), 1, None), (("mDice",), 1, None), (("mFscore",), 1, None),
                                                     (("mFscore",), 2, None), (ALL, 1, None), (ALL, 3, 0), (("mIoU",), 1, -1)])
def test_metrics_from_confusion_equal_the_reference(K, ignore_index, metrics, beta, nan_to_num):
    from clip_decontamination_amd.metrics import metrics_from_confusion
    absent = 1 if K > 2 else None
    pairs = [random_case(100 * K + s, K, ignore_index=ignore_index, absent=absent) for s in range(3)]
    table = sum(R.confusion_table(p, g, K, ignore_index) for p, g in pairs)
    got = metrics_from_confusion(table, metrics, nan_to_num, beta)
    want = R.iou_metrics(pairs, K, ignore_index, metrics=metrics, nan_to_num=nan_to_num, beta=beta)
    assert_same_metrics(got, want)
    if absent is not None and nan_to_num is None and "mIoU" in metrics:
        assert np.isnan(got["IoU"][absent]) and np.isnan(got["Acc"][absent])
        seen = np.delete(got["IoU"], absent)
        assert not np.isnan(seen).any()
        assert got["summary"]["mIoU"] == float(np.round(seen.mean() * 100, 2))        # the absent class is left out of the mean
    if absent is not None and nan_to_num is not None:
        assert all(not np.isnan(np.asarray(v)).any() for k, v in got.items() if k != "summary")
        assert got["IoU"][absent] == nan_to_num


def test_areas_are_the_tables_margins():
    from clip_decontamination_amd.metrics import areas_from_confusion
    K = 6
    pred, gt = random_case(7, K)
    got = areas_from_confusion(torch.from_numpy(R.confusion_table(pred, gt, K)))
    for a, b in zip(got, R.intersect_and_union(pred, gt, K)):
        assert a.dtype == np.int64 and np.array_equal(a, b)


def test_summary_is_rounded_to_two_decimals():
    from clip_decontamination_amd.metrics import metrics_from_confusion
    # IoU = 1/3 and 1/3 -> 33.33; Acc = 1/3 and 1 -> 66.67; aAcc = 2/4 -> 50.0
    table = np.array([[1, 0, 0], [2, 1, 0], [0, 0, 0]], dtype=np.int64)
    got = metrics_from_confusion(table)
    assert got["IoU"].tolist() == [1 / 3, 1 / 3] and got["Acc"].tolist() == [1 / 3, 1.0]
    assert got["summary"] == {"aAcc": 50.0, "mIoU": 33.33, "mAcc": 66.67}
    assert got["aAcc"] == 0.5


def test_unknown_metric_is_refused():
    from clip_decontamination_amd.metrics import IoUMetric, metrics_from_confusion
    with pytest.raises(KeyError):
        metrics_from_confusion(np.zeros((3, 3), dtype=np.int64), ("mAP",))
    with pytest.raises(KeyError):
        IoUMetric(iou_metrics=["mAP"])
    with pytest.raises(TypeError):                                 # a misspelt keyword must not be swallowed
        IoUMetric(ignore_idx=3)
    with pytest.raises(TypeError):
        IoUMetric(reduce_zero_labels=True)
    with pytest.raises(NotImplementedError):
        IoUMetric(format_only=True)
    assert IoUMetric(collect_device="gpu", prefix="x", output_dir=None, format_only=False).ignore_index == 255


def test_reduce_zero_label_boundary_values():
    """raw 0 -> 255 (ignored under the default ignore_index), 1 -> class 0, 254 -> 253, 255 stays 255: mmseg's LoadAnnotations rule.  The
    mapping itself lives in the kernel (held to it in tests/test_gpu_iou_metric.py); here the reference helper's statement of it is
    pinned on the boundary values, and the package's margins of the resulting tables must give mmseg's areas under the same rule."""
    from clip_decontamination_amd.metrics import areas_from_confusion, metrics_from_confusion
    assert R.reduce_zero(np.array([0, 1, 2, 254, 255])).tolist() == [255, 0, 1, 253, 255]
    K = 254
    gt = np.array([0, 1, 254, 255], dtype=np.uint8)
    pred = np.array([0, 0, 253, 253], dtype=np.int64)
    t = R.confusion_table(pred, gt, K, 255, reduce_zero_label=True)
    assert t.sum() == 2 and t[0, 0] == 1 and t[253, 253] == 1
    t3 = R.confusion_table(pred, gt, K, 253, reduce_zero_label=True)         # another ignore index: the 255s now count, as out of range
    assert t3.sum() == 3 and t3[0, K] == 1 and t3[253, K] == 1 and t3[0, 0] == 1
    for table, ignore_index in ((t, 255), (t3, 253)):
        want = R.intersect_and_union(pred, gt, K, ignore_index, reduce_zero_label=True)
        for a, b in zip(areas_from_confusion(table), want):
            assert np.array_equal(a, b)
        assert_same_metrics(metrics_from_confusion(table), R.total_area_to_metrics(*want))
    inter, union, ap, al = R.intersect_and_union(pred, gt, K, 255, reduce_zero_label=True)
    assert inter[0] == 1 and inter[253] == 1 and al.sum() == 2 and ap.sum() == 2


def test_metric_constructs_from_the_shipped_config_line():
    from clip_decontamination_amd.metrics import IoUMetric
    spec = importlib.util.spec_from_file_location("base_config", os.path.join(ROOT, "configs", "base_config.py"))
    cfg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cfg)
    assert cfg.test_evaluator["type"] == "IoUMetric"
    m = IoUMetric(**{k: v for k, v in cfg.test_evaluator.items() if k != "type"})
    assert m.metrics == ["mIoU"] and m.ignore_index == 255 and m.reduce_zero_label is False and m.num_classes is None
    with pytest.raises(RuntimeError, match="num_classes"):
        m.compute()
    m.num_classes = 6
    assert tuple(m.confusion.shape) == (7, 7) and m.confusion.dtype == torch.int64 and int(m.confusion.sum()) == 0
    pred, gt = random_case(3, 6)
    m.add_confusion(torch.from_numpy(R.confusion_table(pred, gt, 6)))
    assert_same_metrics(m.compute(), R.iou_metrics([(pred, gt)], 6))
    m.reset()
    assert int(m.confusion.sum()) == 0


def test_add_needs_device_tensors():
    from clip_decontamination_amd.metrics import IoUMetric
    m = IoUMetric(num_classes=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(torch.zeros(4, 4, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.uint8))


def _reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    from clip_decontamination_amd.metrics import IoUMetric
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        K = 6
        m = IoUMetric(num_classes=K, iou_metrics=["mIoU", "mFscore"])
        pred, gt = random_case(40 + rank, K)
        m.add_confusion(torch.from_numpy(R.confusion_table(pred, gt, K)))
        m.reduce(dist.group.WORLD)
        q.put((rank, m.confusion.clone().numpy(), m.compute()["summary"]))
    finally:
        dist.destroy_process_group()


def test_reduce_sums_the_tables_of_a_gloo_group():
    from test_distributed_cpu import _run_ranks
    K, world = 6, 2
    res = _run_ranks(_reduce_worker, world, ())
    pairs = [random_case(40 + r, K) for r in range(world)]
    want = sum(R.confusion_table(p, g, K) for p, g in pairs)
    summary = R.iou_metrics(pairs, K, metrics=("mIoU", "mFscore"))["summary"]
    assert sorted(r[0] for r in res) == list(range(world))
    for rank, table, got in res:
        assert table.dtype == np.int64 and np.array_equal(table, want), rank
        assert got == summary, rank


def test_confusion_accumulate_refusals_without_gpu():
    """sg_confusion_accumulate runs every argument check before its first HIP call, so each refusal is visible on CPU."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)                                   # never dereferenced: every call below is refused before any launch

    def call(labels=p, gt=p, fmt=_lib.GT_U8, n=100, K=6, table=p):
        return lib.sg_confusion_accumulate(labels, gt, fmt, n, K, 255, 0, table, None)

    cases = [
        (dict(K=0), b"K=0"),
        (dict(K=-3), b"K=-3"),
        (dict(K=4096), b"K=4096 exceeds"),
        (dict(labels=None), b"null pointer"),
        (dict(gt=None), b"null pointer"),
        (dict(table=None), b"null pointer"),
        (dict(fmt=2), b"unknown ground-truth format 2"),
        (dict(fmt=-1), b"unknown ground-truth format -1"),
        (dict(n=-1), b"n_pixels=-1"),
        (dict(labels=ctypes.c_void_p((1 << 20) + 4)), b"8-byte aligned"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in lib.sg_last_error(), (kw, lib.sg_last_error())
    assert call(n=0) == 0                                          # nothing to count: a valid no-op, no launch
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.check(call(gt=None), "sg_confusion_accumulate")


def test_ops_binding_refuses_host_tensors_and_mismatched_shapes():
    from clip_decontamination_amd import ops
    lab = torch.zeros(4, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.confusion_accumulate(lab, torch.zeros(4, 5, dtype=torch.uint8), torch.zeros(7, 7, dtype=torch.int64), 6)
    assert ops._same_pixels(torch.zeros(1, 4, 5), torch.zeros(4, 5)) and ops._same_pixels(torch.zeros(20), torch.zeros(20))
    assert not ops._same_pixels(torch.zeros(4, 5), torch.zeros(5, 4)) and not ops._same_pixels(torch.zeros(20), torch.zeros(4, 5))
