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


def _one_map(who: str, labels, gt):
    """The checks of ``add`` on the metrics that need an image's shape: one non-empty [H,W] / [1,H,W] map each, of one size
    -> (gt as a tensor, (H, W))."""
    gt = torch.as_tensor(gt)
    for name, t in (("labels", labels), ("gt", gt)):
        if not torch.is_tensor(t) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1) or t.numel() == 0:
            raise ValueError(f"{who}.add: {name} must be a non-empty [H,W] or [1,H,W] map (a flat buffer of images goes "
                             "through add_flat with their sizes)")
    if tuple(labels.shape[-2:]) != tuple(gt.shape[-2:]):
        raise ValueError(f"{who}.add: labels {tuple(labels.shape)} and gt {tuple(gt.shape)} differ in size")
    return gt, tuple(labels.shape[-2:])


def _flat_sizes(who: str, labels, image_hw):
    """The checks of ``add_flat`` on the sizes of a flush group, before anything is counted -> image_hw as int pairs."""
    image_hw = [(int(h), int(w)) for h, w in image_hw]
    if not image_hw or any(h < 1 or w < 1 for h, w in image_hw):
        raise ValueError(f"{who}.add_flat: needs at least one image of positive size, got {image_hw}")
    if not torch.is_tensor(labels) or labels.numel() != sum(h * w for h, w in image_hw):
        raise ValueError(f"{who}.add_flat: images of sizes {image_hw} against "
                         f"{labels.numel() if torch.is_tensor(labels) else type(labels).__name__} labels")
    return image_hw


def _flat_on_device(who: str, entry: str, labels, gt):
    """Flat labels and truth of one flush group on the labels' device; no CPU fallback."""
    if not labels.is_cuda:
        raise RuntimeError(f"{who} counts on the GPU ({entry}): labels must be a device tensor; there is no CPU fallback")
    gt = torch.as_tensor(gt)
    if gt.dtype not in (torch.uint8, torch.int64):
        gt = gt.to(torch.int64)
    return labels.reshape(-1), gt.to(labels.device).reshape(-1)


def metrics_from_boundary(areas, nan_to_num: Optional[int] = None) -> dict:
    """Boundary IoU (Cheng et al., CVPR 2021) from the band-restricted counts ``areas`` int64 [3,K] of ``sg_boundary_accumulate`` (rows:
    intersection of the two bands, prediction band, truth band): ``BIoU`` float64 [K] = areas[0] / (areas[1] + areas[2] - areas[0]),
    NaN where a class has no band pixel in prediction and truth, and ``summary['mBIoU']`` = ``nanmean * 100`` rounded to 2 decimals,
    with such a class left out of the mean (``nan_to_num`` replaces NaN first), as ``metrics_from_confusion`` treats ``IoU``."""
    a = areas.detach().cpu().numpy() if torch.is_tensor(areas) else np.asarray(areas)
    if a.ndim != 2 or a.shape[0] != 3 or a.shape[1] < 1:
        raise ValueError(f"boundary areas must be [3,K] with K >= 1, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"boundary areas must hold integers, got {a.dtype}")
    inter, pred, label = (a[i].astype(np.float64) for i in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        biou = np.asarray(inter / (pred + label - inter), dtype=np.float64)
    if nan_to_num is not None:
        biou = np.nan_to_num(biou, nan=nan_to_num)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        mean = float(np.round(np.nanmean(biou) * 100, 2))
    return {"BIoU": biou, "summary": {"mBIoU": mean}}


class BoundaryIoUMetric(IoUMetric):
    """``IoUMetric`` plus Boundary IoU: the confusion table as before and ``boundary_areas`` int64 [3,K], the counts restricted to the
    bands of prediction and truth (``sg_boundary_accumulate``).  The band width is ``boundary_ratio`` of each image's diagonal
    (``ops.boundary_width``; 0.02 as in the paper) or the fixed ``boundary_px``, which overrides the ratio.

    ``add(labels, gt)`` takes one 2-D map ([H,W] or [1,H,W]) and counts both tables; ``add_flat(labels, gt, image_hw)`` the flat buffers
    of a flush group with the sizes of its images; ``reduce(group)`` sums both tables; ``add_confusion`` is IoUMetric's and leaves the
    boundary counts alone; ``compute()`` returns IoUMetric's dict plus ``BIoU`` and ``summary['mBIoU']``."""

    def __init__(self, *args, boundary_ratio: float = 0.02, boundary_px: Optional[int] = None, **kwargs):
        from . import ops
        if boundary_px is not None:
            if isinstance(boundary_px, bool) or not isinstance(boundary_px, int) or not 1 <= boundary_px <= ops.BOUNDARY_MAX_D:
                raise ValueError(f"boundary_px must be an integer in [1, {ops.BOUNDARY_MAX_D}] or None, got {boundary_px!r}")
        else:
            ops.boundary_width((1, 1), boundary_ratio)                       # the ratio's own checks
        super().__init__(*args, **kwargs)
        if self.num_classes is not None and self.num_classes > ops.BOUNDARY_MAX_K:
            raise ValueError(f"BoundaryIoUMetric: num_classes={self.num_classes} exceeds {ops.BOUNDARY_MAX_K}")
        self.boundary_ratio, self.boundary_px = boundary_ratio, boundary_px
        self._areas: Optional[torch.Tensor] = None

    def width(self, hw) -> int:
        """The band width of an image of size ``hw``."""
        from . import ops
        return self.boundary_px if self.boundary_px is not None else ops.boundary_width(hw, self.boundary_ratio)

    def _ensure_areas(self, device) -> torch.Tensor:
        K = self._classes()
        if self._areas is None:
            self._areas = torch.zeros(3, K, dtype=torch.int64, device=device)
        elif self._areas.device != torch.device(device):
            self._areas = self._areas.to(device)
        return self._areas

    @property
    def boundary_areas(self) -> torch.Tensor:
        """The [3,K] int64 band counts: intersection, prediction band, truth band."""
        return self._ensure_areas("cpu" if self._areas is None else self._areas.device)

    def reset(self) -> None:
        super().reset()
        self._areas = None

    def add(self, labels: torch.Tensor, gt: torch.Tensor) -> None:
        """Counts one image in both tables: labels int64 and gt uint8 / int64, [H,W] or [1,H,W] of one size.  The band needs the
        image's shape, so a flat buffer goes through ``add_flat``."""
        gt, hw = _one_map("BoundaryIoUMetric", labels, gt)
        self.add_flat(labels.reshape(-1), gt.reshape(-1), [hw])

    def add_flat(self, labels: torch.Tensor, gt: torch.Tensor, image_hw) -> None:
        """Counts the images that lie back to back in the flat ``labels`` / ``gt`` buffers (a flush group's), sizes ``image_hw``: one
        sg_confusion_accumulate launch and one sg_boundary_accumulate call on the current stream."""
        from . import ops
        image_hw = _flat_sizes("BoundaryIoUMetric", labels, image_hw)
        ds = [self.width(hw) for hw in image_hw]
        labels, gt = _flat_on_device("BoundaryIoUMetric", "sg_boundary_accumulate", labels, gt)
        K = self._classes()
        ops.confusion_accumulate(labels, gt, self._ensure(labels.device), K, self.ignore_index, self.reduce_zero_label)
        ops.boundary_accumulate(labels, gt, image_hw, ds, self._ensure_areas(labels.device), K, self.ignore_index, self.reduce_zero_label)

    def reduce(self, group=None) -> None:
        """Sums both tables over the ranks of ``group``: two all_reduces."""
        import torch.distributed as dist
        super().reduce(group)
        dist.all_reduce(self.boundary_areas, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> dict:
        out = super().compute()
        b = metrics_from_boundary(self.boundary_areas, self.nan_to_num)
        out["BIoU"] = b["BIoU"]
        out["summary"] = dict(out["summary"], mBIoU=b["summary"]["mBIoU"])
        return out


TOLERANT_KEYS = {"region": ("RelPrecision", "RelRecall", "RelFscore", "mRelPrecision", "mRelRecall", "mRelFscore"),
                 "contour": ("BPrecision", "BRecall", "BFscore", "mBPrecision", "mBRecall", "mBF")}


def metrics_from_tolerant(counts, mode: str = "region", nan_to_num: Optional[int] = None) -> dict:
    """Relaxed precision / recall / F (``mode`` "region": Mnih & Hinton 2010) or the boundary precision / recall / F-score ("contour":
    Martin et al. 2004, Csurka et al. 2013) from the counts int64 [4,K] of ``sg_tolerant_accumulate`` (rows: predicted, predicted and
    right within the tolerance, true, true and found): precision = counts[1] / counts[0], recall = counts[3] / counts[2],
    F = 2PR / (P + R), float64 [K], NaN where a denominator is 0.  Keys ``RelPrecision`` / ``RelRecall`` / ``RelFscore`` or
    ``BPrecision`` / ``BRecall`` / ``BFscore``, and ``summary`` with ``mRelPrecision`` / ``mRelRecall`` / ``mRelFscore`` or
    ``mBPrecision`` / ``mBRecall`` / ``mBF``: ``nanmean * 100`` rounded to 2 decimals, NaN classes left out (``nan_to_num`` replaces NaN
    first), as ``metrics_from_boundary`` does."""
    if mode not in TOLERANT_KEYS:
        raise ValueError(f"metrics_from_tolerant: mode must be one of {sorted(TOLERANT_KEYS)}, got {mode!r}")
    a = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if a.ndim != 2 or a.shape[0] != 4 or a.shape[1] < 1:
        raise ValueError(f"tolerant counts must be [4,K] with K >= 1, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"tolerant counts must hold integers, got {a.dtype}")
    pred, right, true, found = (a[i].astype(np.float64) for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        p, r = right / pred, found / true
        vals = [np.asarray(v, dtype=np.float64) for v in (p, r, 2 * p * r / (p + r))]
    if nan_to_num is not None:
        vals = [np.nan_to_num(v, nan=nan_to_num) for v in vals]
    keys = TOLERANT_KEYS[mode]
    out = dict(zip(keys[:3], vals))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        out["summary"] = {k: float(np.round(np.nanmean(v) * 100, 2)) for k, v in zip(keys[3:], vals)}
    return out


class RelaxedMetric(IoUMetric):
    """``IoUMetric`` plus the tolerant scores: the confusion table as before and ``tolerant_counts`` int64 [4,K]
    (``sg_tolerant_accumulate``).  ``mode`` "region" gives relaxed precision / recall / F (roads), "contour" the boundary F-score.
    The tolerance is ``tolerance_ratio`` of each image's diagonal (``ops.tolerance_sq``; 0.0075) or the fixed ``tolerance_px``
    (an integer in [0, 254]), which overrides the ratio.

    ``add(labels, gt)`` takes one 2-D map ([H,W] or [1,H,W]) and counts both tables; ``add_flat(labels, gt, image_hw)`` the flat buffers
    of a flush group with the sizes of its images; ``reduce(group)`` sums both tables; ``add_confusion`` is IoUMetric's and leaves the
    tolerant counts alone; ``compute()`` returns IoUMetric's dict plus the keys of ``metrics_from_tolerant``, merged into ``summary``."""

    def __init__(self, *args, mode: str = "region", tolerance_px: Optional[int] = None, tolerance_ratio: float = 0.0075, **kwargs):
        from . import ops
        if mode not in ops.TOLERANT_MODES:
            raise ValueError(f"RelaxedMetric: mode must be one of {sorted(ops.TOLERANT_MODES)}, got {mode!r}")
        if tolerance_px is not None:
            if isinstance(tolerance_px, bool) or not isinstance(tolerance_px, int) or not 0 <= tolerance_px <= 254:
                raise ValueError(f"tolerance_px must be an integer in [0, 254] or None, got {tolerance_px!r}")
        else:
            ops.tolerance_sq((1, 1), tolerance_ratio)                        # the ratio's own checks
        super().__init__(*args, **kwargs)
        if self.num_classes is not None and self.num_classes > ops.TOLERANT_MAX_K:
            raise ValueError(f"RelaxedMetric: num_classes={self.num_classes} exceeds {ops.TOLERANT_MAX_K}")
        self.mode, self.tolerance_px, self.tolerance_ratio = mode, tolerance_px, tolerance_ratio
        self._counts: Optional[torch.Tensor] = None

    def tolerance_sq(self, hw) -> int:
        """The squared tolerance of an image of size ``hw``."""
        from . import ops
        return self.tolerance_px * self.tolerance_px if self.tolerance_px is not None else ops.tolerance_sq(hw, self.tolerance_ratio)

    def _ensure_counts(self, device) -> torch.Tensor:
        K = self._classes()
        if self._counts is None:
            self._counts = torch.zeros(4, K, dtype=torch.int64, device=device)
        elif self._counts.device != torch.device(device):
            self._counts = self._counts.to(device)
        return self._counts

    @property
    def tolerant_counts(self) -> torch.Tensor:
        """The [4,K] int64 counts: predicted, predicted and right, true, true and found."""
        return self._ensure_counts("cpu" if self._counts is None else self._counts.device)

    def reset(self) -> None:
        super().reset()
        self._counts = None

    def add(self, labels: torch.Tensor, gt: torch.Tensor) -> None:
        """Counts one image in both tables: labels int64 and gt uint8 / int64, [H,W] or [1,H,W] of one size.  The search needs the
        image's shape, so a flat buffer goes through ``add_flat``."""
        gt, hw = _one_map("RelaxedMetric", labels, gt)
        self.add_flat(labels.reshape(-1), gt.reshape(-1), [hw])

    def add_flat(self, labels: torch.Tensor, gt: torch.Tensor, image_hw) -> None:
        """Counts the images that lie back to back in the flat ``labels`` / ``gt`` buffers (a flush group's), sizes ``image_hw``: one
        sg_confusion_accumulate launch and one sg_tolerant_accumulate call on the current stream."""
        from . import ops
        image_hw = _flat_sizes("RelaxedMetric", labels, image_hw)
        ts = [self.tolerance_sq(hw) for hw in image_hw]
        labels, gt = _flat_on_device("RelaxedMetric", "sg_tolerant_accumulate", labels, gt)
        K = self._classes()
        ops.confusion_accumulate(labels, gt, self._ensure(labels.device), K, self.ignore_index, self.reduce_zero_label)
        ops.tolerant_accumulate(labels, gt, image_hw, ts, self._ensure_counts(labels.device), K, self.ignore_index, self.reduce_zero_label,
                                self.mode)

    def reduce(self, group=None) -> None:
        """Sums both tables over the ranks of ``group``: two all_reduces."""
        import torch.distributed as dist
        super().reduce(group)
        dist.all_reduce(self.tolerant_counts, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> dict:
        out = super().compute()
        t = metrics_from_tolerant(self.tolerant_counts, self.mode, self.nan_to_num)
        summary = dict(out["summary"], **t.pop("summary"))
        out.update(t)
        out["summary"] = summary
        return out


OBJECT_KEYS = ("ObjPrecision", "ObjRecall", "ObjF1", "SQ", "PQ")


def metrics_from_objects(counts, nan_to_num: Optional[int] = None) -> dict:
    """Object-level precision / recall / F1 and panoptic quality (Kirillov et al., CVPR 2019, with connected regions as the segments)
    from the counts int64 [4,K] of ``sg_object_match`` (rows: matched pairs TP, predicted objects, true objects, the matched pairs' IoU
    in steps of 2^-24): ``ObjPrecision`` = TP / counts[1], ``ObjRecall`` = TP / counts[2], ``ObjF1`` = RQ = 2 TP / (counts[1] +
    counts[2]), ``SQ`` = counts[3] / 2^24 / TP, ``PQ`` = SQ * RQ, float64 [K], NaN where a denominator is 0; and ``summary`` with
    ``mObjPrecision`` / ``mObjRecall`` / ``mObjF1`` / ``mSQ`` / ``mPQ``: ``nanmean * 100`` rounded to 2 decimals, NaN classes left out
    (``nan_to_num`` replaces NaN first), as ``metrics_from_tolerant`` does."""
    a = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if a.ndim != 2 or a.shape[0] != 4 or a.shape[1] < 1:
        raise ValueError(f"object counts must be [4,K] with K >= 1, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"object counts must hold integers, got {a.dtype}")
    tp, pred, true, iou_q = (a[i].astype(np.float64) for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        rq, sq = 2 * tp / (pred + true), iou_q / float(1 << 24) / tp
        vals = [np.asarray(v, dtype=np.float64) for v in (tp / pred, tp / true, rq, sq, sq * rq)]
    if nan_to_num is not None:
        vals = [np.nan_to_num(v, nan=nan_to_num) for v in vals]
    out = dict(zip(OBJECT_KEYS, vals))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        out["summary"] = {"m" + k: float(np.round(np.nanmean(v) * 100, 2)) for k, v in zip(OBJECT_KEYS, vals)}
    return out


class ObjectMetric(IoUMetric):
    """``IoUMetric`` plus the object-level scores: the confusion table as before and ``object_counts`` int64 [4,K]
    (``sg_object_match``): per class the connected regions of prediction and truth, matched where their IoU is strictly above
    ``object_iou`` (a float or a ``(num, den)`` pair in [1/2, 1), ``ops.object_iou_fraction``).  A region is an object when it has at
    least ``min_area`` pixels and its class is not ``skip_label`` (the background of a building or road set); ``connectivity`` 4 or 8.

    ``add(labels, gt)`` takes one 2-D map ([H,W] or [1,H,W]) and counts both tables; ``add_flat(labels, gt, image_hw)`` the flat buffers
    of a flush group with the sizes of its images; ``reduce(group)`` sums both tables; ``add_confusion`` is IoUMetric's and leaves the
    object counts alone; ``compute()`` returns IoUMetric's dict plus the keys of ``metrics_from_objects``, merged into ``summary``."""

    def __init__(self, *args, object_iou=0.5, min_area: int = 1, connectivity: int = 4, skip_label: Optional[int] = None, **kwargs):
        from . import ops
        self.object_iou = ops.object_args([(1, 1)], 1, object_iou, connectivity, min_area, skip_label)[2]
        super().__init__(*args, **kwargs)
        if self.num_classes is not None and self.num_classes > ops.OBJECT_MAX_K:
            raise ValueError(f"ObjectMetric: num_classes={self.num_classes} exceeds {ops.OBJECT_MAX_K}")
        self.min_area, self.connectivity, self.skip_label = int(min_area), int(connectivity), skip_label
        self._counts: Optional[torch.Tensor] = None

    def _ensure_counts(self, device) -> torch.Tensor:
        K = self._classes()
        if self._counts is None:
            self._counts = torch.zeros(4, K, dtype=torch.int64, device=device)
        elif self._counts.device != torch.device(device):
            self._counts = self._counts.to(device)
        return self._counts

    @property
    def object_counts(self) -> torch.Tensor:
        """The [4,K] int64 counts: matched pairs, predicted objects, true objects, the matched pairs' IoU in steps of 2^-24."""
        return self._ensure_counts("cpu" if self._counts is None else self._counts.device)

    def reset(self) -> None:
        super().reset()
        self._counts = None

    def add(self, labels: torch.Tensor, gt: torch.Tensor, match_map: Optional[torch.Tensor] = None) -> None:
        """Counts one image in both tables: labels int64 and gt uint8 / int64, [H,W] or [1,H,W] of one size.  The regions need the
        image's shape, so a flat buffer goes through ``add_flat``."""
        gt, hw = _one_map("ObjectMetric", labels, gt)
        self.add_flat(labels.reshape(-1), gt.reshape(-1), [hw], match_map)

    def add_flat(self, labels: torch.Tensor, gt: torch.Tensor, image_hw, match_map: Optional[torch.Tensor] = None) -> None:
        """Counts the images that lie back to back in the flat ``labels`` / ``gt`` buffers (a flush group's), sizes ``image_hw``: one
        sg_confusion_accumulate launch and one sg_object_match call on the current stream.  ``match_map``: None, or a uint8 tensor of
        the labels' size that receives the TP / FP / FN picture (``ops.object_match``)."""
        from . import ops
        image_hw = _flat_sizes("ObjectMetric", labels, image_hw)
        labels, gt = _flat_on_device("ObjectMetric", "sg_object_match", labels, gt)
        K = self._classes()
        ops.confusion_accumulate(labels, gt, self._ensure(labels.device), K, self.ignore_index, self.reduce_zero_label)
        ops.object_match(labels, gt, image_hw, self._ensure_counts(labels.device), K, self.object_iou, self.connectivity, self.min_area,
                         self.skip_label, self.ignore_index, self.reduce_zero_label, match_map)

    def reduce(self, group=None) -> None:
        """Sums both tables over the ranks of ``group``: two all_reduces."""
        import torch.distributed as dist
        super().reduce(group)
        dist.all_reduce(self.object_counts, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> dict:
        out = super().compute()
        t = metrics_from_objects(self.object_counts, self.nan_to_num)
        summary = dict(out["summary"], **t.pop("summary"))
        out.update(t)
        out["summary"] = summary
        return out


try:  # with mmseg installed the classes are also buildable from a config, under names that leave mmseg's own IoUMetric alone
    from mmseg.registry import METRICS as _METRICS
    _METRICS.register_module(name="HipIoUMetric", module=IoUMetric)
    _METRICS.register_module(name="HipBoundaryIoUMetric", module=BoundaryIoUMetric)
    _METRICS.register_module(name="HipRelaxedMetric", module=RelaxedMetric)
    _METRICS.register_module(name="HipObjectMetric", module=ObjectMetric)
except Exception:
    pass
