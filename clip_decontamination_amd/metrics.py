"""mmseg's ``IoUMetric`` on the HIP path (reference configs/base_config.py: ``test_evaluator = dict(type='IoUMetric', ...)``).

The counting -- mmseg's ``intersect_and_union`` -- runs on the device (``sg_confusion_accumulate``): labels and ground truth stay
there and only the ``(K+1) x (K+1)`` int64 confusion table comes back.  Row = prediction, column = ground truth, index K = "outside
[0,K)", which reproduces ``torch.histc(min=0, max=K-1)`` dropping an out-of-range value from one histogram while the pixel still
counts in the others:

    area_intersect[k] = table[k][k]     area_pred_label[k] = sum_g table[k][g]     area_label[k] = sum_p table[p][k]

The ratios are host arithmetic in float64 (``metrics_from_confusion``), a restatement of mmseg's ``total_area_to_metrics`` and of
the summary step of ``compute_metrics``.  Counts are integers, so they equal mmseg's wherever its float32 ``histc`` counts are exact.
"""
from __future__ import annotations

import warnings
from typing import Optional, Sequence

import numpy as np
import torch

ALLOWED_METRICS = ("mIoU", "mDice", "mFscore")


def _as_table(table) -> np.ndarray:
    t = table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] < 2:
        raise ValueError(f"confusion table must be [(K+1),(K+1)] with K >= 1, got shape {t.shape}")
    if not np.issubdtype(t.dtype, np.integer):
        raise TypeError(f"confusion table must hold integers, got {t.dtype}")
    return t.astype(np.int64)


def areas_from_confusion(table):
    """(area_intersect, area_union, area_pred_label, area_label), int64 [K] each, from a [(K+1),(K+1)] table."""
    t = _as_table(table)
    K = t.shape[0] - 1
    inter = np.diagonal(t)[:K].copy()
    pred = t[:K, :].sum(axis=1)
    label = t[:, :K].sum(axis=0)
    return inter, pred + label - inter, pred, label


def metrics_from_confusion(table, metrics: Sequence[str] = ("mIoU",), nan_to_num: Optional[int] = None, beta: int = 1) -> dict:
    """mmseg ``IoUMetric.total_area_to_metrics`` + the summary of ``compute_metrics`` from the confusion table, in float64.

    Returns ``aAcc`` (a ratio), the per-class vectors (float64 [K] ratios) -- ``IoU`` and ``Acc`` for mIoU, ``Dice`` and ``Acc`` for
    mDice, ``Fscore`` / ``Precision`` / ``Recall`` for mFscore -- and ``summary``: ``aAcc`` plus one ``m<name>`` per vector, each
    ``nanmean * 100`` rounded to 2 decimals as mmseg prints them.  A class absent from prediction and truth is NaN and left out of
    the mean (``nan_to_num`` replaces NaN first, as in mmseg)."""
    if isinstance(metrics, str):
        metrics = [metrics]
    for m in metrics:
        if m not in ALLOWED_METRICS:
            raise KeyError(f"metrics {metrics} is not supported (allowed: {ALLOWED_METRICS})")
    inter, union, pred, label = (a.astype(np.float64) for a in areas_from_confusion(table))
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["aAcc"] = inter.sum() / label.sum()
        for m in metrics:
            if m == "mIoU":
                out["IoU"] = inter / union
                out["Acc"] = inter / label
            elif m == "mDice":
                out["Dice"] = 2 * inter / (pred + label)
                out["Acc"] = inter / label
            else:
                precision, recall = inter / pred, inter / label
                out["Fscore"] = (1 + beta ** 2) * (precision * recall) / ((beta ** 2 * precision) + recall)
                out["Precision"], out["Recall"] = precision, recall
    out = {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}
    if nan_to_num is not None:
        out = {k: np.nan_to_num(v, nan=nan_to_num) for k, v in out.items()}
    with warnings.catch_warnings():                      # nanmean of an all-NaN vector (no class seen) is NaN by design, not a warning
        warnings.simplefilter("ignore", category=RuntimeWarning)
        summary = {(k if k == "aAcc" else "m" + k): float(np.round(np.nanmean(v) * 100, 2)) for k, v in out.items()}
    out["aAcc"] = float(out["aAcc"])
    out["summary"] = summary
    return out


def _field(obj, name):
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


class IoUMetric:
    """mmseg ``IoUMetric`` semantics over a device-side confusion table.  The constructor takes mmseg's kwargs, so
    ``IoUMetric(**{k: v for k, v in cfg.test_evaluator.items() if k != 'type'})`` works; ``num_classes`` may also be set later (the
    segmentors' ``evaluate`` fills it from the class file, ``process`` from ``dataset_meta['classes']``).

    ``add(labels, gt)`` counts device tensors; ``process(data_batch, data_samples)`` is mmseg's call shape; ``reduce(group)`` sums the
    table over a torch.distributed group (one all_reduce); ``compute()`` returns ``metrics_from_confusion`` of the table, which lives
    on the device until then.  Only totals are kept (mmseg sums its per-image results too)."""

    def __init__(self, ignore_index: int = 255, iou_metrics: Sequence[str] = ("mIoU",), nan_to_num: Optional[int] = None, beta: int = 1,
                 num_classes: Optional[int] = None, reduce_zero_label: bool = False, collect_device: str = "cpu",
                 output_dir: Optional[str] = None, format_only: bool = False, prefix: Optional[str] = None):
        # collect_device / prefix belong to mmengine's BaseMetric and are accepted for config compatibility; the two mmseg options that
        # write prediction PNGs instead of scoring are refused, not ignored.  Any other keyword is a TypeError, as for any function.
        if format_only or output_dir is not None:
            raise NotImplementedError("IoUMetric: output_dir / format_only (writing prediction PNGs instead of scoring) are not built; "
                                      "result_dir on the segmentors writes the label images")
        metrics = [iou_metrics] if isinstance(iou_metrics, str) else list(iou_metrics)
        for m in metrics:
            if m not in ALLOWED_METRICS:
                raise KeyError(f"metrics {metrics} is not supported (allowed: {ALLOWED_METRICS})")
        self.ignore_index, self.metrics, self.nan_to_num, self.beta = int(ignore_index), metrics, nan_to_num, beta
        self.num_classes = None if num_classes is None else int(num_classes)
        self.reduce_zero_label = bool(reduce_zero_label)
        self.dataset_meta = None
        self._table: Optional[torch.Tensor] = None

    # -- the table ----------------------------------------------------------------------------------------------------------
    def _classes(self) -> int:
        if self.num_classes is None and self.dataset_meta and "classes" in self.dataset_meta:
            self.num_classes = len(self.dataset_meta["classes"])
        if self.num_classes is None or self.num_classes < 1:
            raise RuntimeError("IoUMetric: num_classes is not set (pass num_classes=, or dataset_meta with 'classes')")
        return self.num_classes

    def _ensure(self, device) -> torch.Tensor:
        K = self._classes()
        if self._table is None:
            self._table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=device)
        elif self._table.device != torch.device(device):          # the table follows the data (a table read before the first add is on the CPU)
            self._table = self._table.to(device)
        return self._table

    @property
    def confusion(self) -> torch.Tensor:
        """The (K+1) x (K+1) int64 table, row = prediction, column = ground truth, index K = outside [0,K)."""
        return self._ensure("cpu" if self._table is None else self._table.device)

    def reset(self) -> None:
        self._table = None

    def add_confusion(self, table) -> None:
        """Adds an already counted (K+1) x (K+1) table (another metric's, a saved partial result); any device."""
        t = torch.as_tensor(table)
        K = self._classes()
        if t.dtype != torch.int64 or tuple(t.shape) != (K + 1, K + 1):
            raise ValueError(f"add_confusion: need an int64 table of shape {(K + 1, K + 1)}, got {t.dtype} {tuple(t.shape)}")
        self._ensure(t.device).add_(t)

    # -- counting -----------------------------------------------------------------------------------------------------------
    def add(self, labels: torch.Tensor, gt: torch.Tensor) -> None:
        """Counts one image, or a flat run of images: labels int64 and gt uint8 / int64 device tensors of one shape (up to leading
        1s).  One sg_confusion_accumulate launch on the current stream; nothing returns to the host."""
        from . import ops
        if not (torch.is_tensor(labels) and labels.is_cuda):
            raise RuntimeError("IoUMetric.add counts on the GPU (sg_confusion_accumulate): labels must be a device tensor; "
                               "there is no CPU fallback")
        gt = torch.as_tensor(gt)
        if gt.dtype not in (torch.uint8, torch.int64):
            gt = gt.to(torch.int64)
        gt = gt.to(labels.device)
        ops.confusion_accumulate(labels, gt, self._ensure(labels.device), self._classes(), self.ignore_index, self.reduce_zero_label)

    def process(self, data_batch, data_samples) -> None:
        """mmseg's ``process``: every sample (object or dict) carries ``pred_sem_seg`` and ``gt_sem_seg``, each with ``.data`` /
        ``['data']``."""
        for sample in data_samples:
            pred = _field(_field(sample, "pred_sem_seg"), "data")
            gt = _field(_field(sample, "gt_sem_seg"), "data")
            self.add(pred, torch.as_tensor(gt))

    # -- results ------------------------------------------------------------------------------------------------------------
    def reduce(self, group=None) -> None:
        """Sums the table over the ranks of ``group`` (default: the world): one all_reduce on the int64 table, wherever it lives (a
        device table under NCCL, a CPU table under gloo)."""
        import torch.distributed as dist
        dist.all_reduce(self.confusion, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> dict:
        return metrics_from_confusion(self.confusion, self.metrics, self.nan_to_num, self.beta)


try:  # with mmseg installed the class is also buildable from a config, under a name that leaves mmseg's own IoUMetric alone
    from mmseg.registry import METRICS as _METRICS
    _METRICS.register_module(name="HipIoUMetric", module=IoUMetric)
except Exception:
    pass
