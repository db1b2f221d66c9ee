"""CPU reference for the IoU metric: mmseg's own formula (IoUMetric.intersect_and_union, total_area_to_metrics, the summary of
compute_metrics) restated with INTEGER histograms -- numpy ``bincount`` in int64 where mmseg runs ``torch.histc`` in float32.

It equals mmseg wherever histc's float32 counts are exact, i.e. below 2^24 pixels per class per image; above that mmseg's own
counts round and this reference (like the device kernel) keeps counting exactly.  Everything here is numpy on the host; nothing is
shared with the code under test.
"""
import numpy as np


def reduce_zero(label):
    """mmseg LoadAnnotations(reduce_zero_label=True): raw 0 -> 255, raw 255 stays 255, every other value -> value - 1 (the 255 is
    literal, whatever ignore_index is)."""
    label = np.asarray(label).astype(np.int64)
    return np.where((label == 0) | (label == 255), 255, label - 1)


def _hist(values, K):
    values = values[(values >= 0) & (values < K)]          # torch.histc(min=0, max=K-1) drops what lies outside
    return np.bincount(values, minlength=K).astype(np.int64)[:K]


def intersect_and_union(pred, label, K, ignore_index=255, reduce_zero_label=False):
    """-> (area_intersect, area_union, area_pred_label, area_label), int64 [K] each."""
    pred = np.asarray(pred).astype(np.int64).reshape(-1)
    label = np.asarray(label).astype(np.int64).reshape(-1)
    assert pred.shape == label.shape
    if reduce_zero_label:
        label = reduce_zero(label)
    mask = label != ignore_index
    pred, label = pred[mask], label[mask]
    inter = _hist(pred[pred == label], K)
    area_pred, area_label = _hist(pred, K), _hist(label, K)
    return inter, area_pred + area_label - inter, area_pred, area_label


def confusion_table(pred, label, K, ignore_index=255, reduce_zero_label=False):
    """The (K+1) x (K+1) int64 table the device accumulates: row = prediction, column = truth, index K = outside [0,K)."""
    pred = np.asarray(pred).astype(np.int64).reshape(-1)
    label = np.asarray(label).astype(np.int64).reshape(-1)
    assert pred.shape == label.shape
    if reduce_zero_label:
        label = reduce_zero(label)
    mask = label != ignore_index
    pred, label = pred[mask], label[mask]
    p = np.where((pred >= 0) & (pred < K), pred, K)
    g = np.where((label >= 0) & (label < K), label, K)
    return np.bincount(p * (K + 1) + g, minlength=(K + 1) ** 2).astype(np.int64).reshape(K + 1, K + 1)


def total_area_to_metrics(inter, union, area_pred, area_label, metrics=("mIoU",), nan_to_num=None, beta=1):
    """mmseg's ratios in float64, and its printed summary (nanmean * 100 rounded to 2 decimals) under 'summary'."""
    inter, union, area_pred, area_label = (np.asarray(a, dtype=np.float64) for a in (inter, union, area_pred, area_label))
    ret = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        ret["aAcc"] = np.float64(inter.sum() / area_label.sum())
        for m in metrics:
            if m == "mIoU":
                ret["IoU"], ret["Acc"] = inter / union, inter / area_label
            elif m == "mDice":
                ret["Dice"], ret["Acc"] = 2 * inter / (area_pred + area_label), inter / area_label
            elif m == "mFscore":
                precision, recall = inter / area_pred, inter / area_label
                ret["Fscore"] = (1 + beta ** 2) * (precision * recall) / ((beta ** 2 * precision) + recall)
                ret["Precision"], ret["Recall"] = precision, recall
            else:
                raise KeyError(m)
        if nan_to_num is not None:
            ret = {k: np.nan_to_num(v, nan=nan_to_num) for k, v in ret.items()}
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            summary = {(k if k == "aAcc" else "m" + k): float(np.round(np.nanmean(v) * 100, 2)) for k, v in ret.items()}
    ret["summary"] = summary
    return ret


def iou_metrics(pairs, K, ignore_index=255, reduce_zero_label=False, metrics=("mIoU",), nan_to_num=None, beta=1):
    """mmseg's whole route over a list of (pred, label) images: per-image areas, summed, then the ratios."""
    tot = [np.zeros(K, dtype=np.int64) for _ in range(4)]
    for pred, label in pairs:
        for t, a in zip(tot, intersect_and_union(pred, label, K, ignore_index, reduce_zero_label)):
            t += a
    return total_area_to_metrics(*tot, metrics=metrics, nan_to_num=nan_to_num, beta=beta)
