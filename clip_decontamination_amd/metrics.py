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
    out = _with_summary(out, [k if k == "aAcc" else "m" + k for k in out], nan_to_num)
    out["aAcc"] = float(out["aAcc"])
    return out


def _with_summary(vectors: dict, summary_keys, nan_to_num) -> dict:
    """The last step of every ``metrics_from_*``: the ratios as float64 (``nan_to_num`` replaces NaN first, as in mmseg) plus
    ``summary``, one ``nanmean * 100`` rounded to 2 decimals per ratio, under ``summary_keys`` in the ratios' order."""
    out = {k: np.asarray(v, dtype=np.float64) for k, v in vectors.items()}
    if nan_to_num is not None:
        out = {k: np.nan_to_num(v, nan=nan_to_num) for k, v in out.items()}
    with warnings.catch_warnings():                      # nanmean of an all-NaN vector (no class seen) is NaN by design, not a warning
        warnings.simplefilter("ignore", category=RuntimeWarning)
        summary = {s: float(np.round(np.nanmean(v) * 100, 2)) for s, v in zip(summary_keys, out.values())}
    out["summary"] = summary
    return out


def _count_rows(counts, rows: int, what: str):
    """The checks of the ``metrics_from_*`` of a second table: integer ``[rows, K]`` counts, K >= 1 -> its rows as float64 [K]."""
    a = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if a.ndim != 2 or a.shape[0] != rows or a.shape[1] < 1:
        raise ValueError(f"{what} must be [{rows},K] with K >= 1, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{what} must hold integers, got {a.dtype}")
    return (a[i].astype(np.float64) for i in range(rows))


def _field(obj, name):
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


def _lazy_table(table: Optional[torch.Tensor], shape, device=None) -> torch.Tensor:
    """A count table that follows the data: zeros of ``shape`` (int64) at its first use, moved when ``device`` is another than its own.
    ``device`` None: where it is; a table read before the first add is on the CPU."""
    if table is None:
        return torch.zeros(*shape, dtype=torch.int64, device="cpu" if device is None else device)
    return table if device is None or table.device == torch.device(device) else table.to(device)


def _gt_on(gt, device) -> torch.Tensor:
    """Ground truth as the entries take it: uint8 or int64 (anything else is widened), on the labels' device."""
    gt = torch.as_tensor(gt)
    if gt.dtype not in (torch.uint8, torch.int64):
        gt = gt.to(torch.int64)
    return gt.to(device)


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

    def _ensure(self, device=None) -> torch.Tensor:
        K = self._classes()
        self._table = _lazy_table(self._table, (K + 1, K + 1), device)
        return self._table

    @property
    def confusion(self) -> torch.Tensor:
        """The (K+1) x (K+1) int64 table, row = prediction, column = ground truth, index K = outside [0,K)."""
        return self._ensure()

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
        ops.confusion_accumulate(labels, _gt_on(gt, labels.device), self._ensure(labels.device), self._classes(), self.ignore_index,
                                 self.reduce_zero_label)

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


class _ImageShapeMetric(IoUMetric):
    """What the metrics that need an image's shape share: the confusion table as before and a second int64 table ``[_ROWS, K]``,
    counted by the subclass's entry ``_ENTRY``.  It is created at its first use and follows the data's device like the first; a
    subclass publishes it under its own property name.

    ``add(labels, gt)`` takes one 2-D map ([H,W] or [1,H,W]) and counts both tables; ``add_flat(labels, gt, image_hw)`` the flat buffers
    of a flush group with the sizes of its images; ``reduce(group)`` sums both tables; ``add_confusion`` is IoUMetric's and leaves the
    second table alone; ``compute()`` returns IoUMetric's dict plus the subclass's scores, merged into ``summary``.

    A subclass checks its own options before this constructor runs and supplies ``_count`` (its one ``ops`` call), ``_scores`` (its
    ``metrics_from_*``) and, where each image has a value of its own (a band width, a tolerance), ``_per_image``."""
    _ROWS, _ENTRY = 0, ""

    def __init__(self, *args, **kwargs):
        from . import ops
        super().__init__(*args, **kwargs)
        if self.num_classes is not None and self.num_classes > ops.CONFUSION_MAX_K:
            raise ValueError(f"{type(self).__name__}: num_classes={self.num_classes} exceeds {ops.CONFUSION_MAX_K}")
        self._second: Optional[torch.Tensor] = None

    def _ensure_second(self, device=None) -> torch.Tensor:
        self._second = _lazy_table(self._second, (self._ROWS, self._classes()), device)
        return self._second

    def reset(self) -> None:
        super().reset()
        self._second = None

    def _one_map(self, labels, gt):
        """The checks of ``add``: one non-empty [H,W] / [1,H,W] map each, of one size -> (gt as a tensor, (H, W))."""
        who = type(self).__name__
        gt = torch.as_tensor(gt)
        for name, t in (("labels", labels), ("gt", gt)):
            if not torch.is_tensor(t) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1) or t.numel() == 0:
                raise ValueError(f"{who}.add: {name} must be a non-empty [H,W] or [1,H,W] map (a flat buffer of images goes "
                                 "through add_flat with their sizes)")
        if tuple(labels.shape[-2:]) != tuple(gt.shape[-2:]):
            raise ValueError(f"{who}.add: labels {tuple(labels.shape)} and gt {tuple(gt.shape)} differ in size")
        return gt, tuple(labels.shape[-2:])

    def _flat_sizes(self, labels, image_hw):
        """The checks of ``add_flat`` on the sizes of a flush group, before anything is counted -> image_hw as int pairs."""
        who = type(self).__name__
        image_hw = [(int(h), int(w)) for h, w in image_hw]
        if not image_hw or any(h < 1 or w < 1 for h, w in image_hw):
            raise ValueError(f"{who}.add_flat: needs at least one image of positive size, got {image_hw}")
        if not torch.is_tensor(labels) or labels.numel() != sum(h * w for h, w in image_hw):
            raise ValueError(f"{who}.add_flat: images of sizes {image_hw} against "
                             f"{labels.numel() if torch.is_tensor(labels) else type(labels).__name__} labels")
        return image_hw

    def _flat_on_device(self, labels, gt):
        """Flat labels and truth of one flush group on the labels' device; no CPU fallback."""
        if not labels.is_cuda:
            raise RuntimeError(f"{type(self).__name__} counts on the GPU ({self._ENTRY}): labels must be a device tensor; there is no "
                               "CPU fallback")
        return labels.reshape(-1), _gt_on(gt, labels.device).reshape(-1)

    def _per_image(self, image_hw):
        """The subclass's value of every image, worked out (and refused) before anything is counted; handed to ``_count``."""
        return None

    def _count(self, labels, gt, image_hw, values, table, K, match_map) -> None:
        """The subclass's one ``ops`` call: adds the counts of the flat device buffers to ``table``.  ``match_map`` is ObjectMetric's."""
        raise NotImplementedError

    def _scores(self) -> dict:
        """The subclass's ``metrics_from_*`` of the second table."""
        raise NotImplementedError

    def add(self, labels: torch.Tensor, gt: torch.Tensor) -> None:
        """Counts one image in both tables: labels int64 and gt uint8 / int64, [H,W] or [1,H,W] of one size.  The second table needs
        the image's shape, so a flat buffer goes through ``add_flat``."""
        gt, hw = self._one_map(labels, gt)
        self.add_flat(labels.reshape(-1), gt.reshape(-1), [hw])

    def add_flat(self, labels: torch.Tensor, gt: torch.Tensor, image_hw) -> None:
        """Counts the images that lie back to back in the flat ``labels`` / ``gt`` buffers (a flush group's), sizes ``image_hw``: one
        sg_confusion_accumulate launch and one call of the subclass's entry on the current stream."""
        self._add_flat(labels, gt, image_hw)

    def _add_flat(self, labels, gt, image_hw, match_map=None) -> None:
        from . import ops
        image_hw = self._flat_sizes(labels, image_hw)
        values = self._per_image(image_hw)
        labels, gt = self._flat_on_device(labels, gt)
        K = self._classes()
        ops.confusion_accumulate(labels, gt, self._ensure(labels.device), K, self.ignore_index, self.reduce_zero_label)
        self._count(labels, gt, image_hw, values, self._ensure_second(labels.device), K, match_map)

    def reduce(self, group=None) -> None:
        """Sums both tables over the ranks of ``group``: two all_reduces."""
        import torch.distributed as dist
        super().reduce(group)
        dist.all_reduce(self._ensure_second(), op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> dict:
        out = super().compute()
        own = self._scores()
        summary = dict(out["summary"], **own.pop("summary"))
        out.update(own)
        out["summary"] = summary
        return out


def metrics_from_boundary(areas, nan_to_num: Optional[int] = None) -> dict:
    """Boundary IoU (Cheng et al., CVPR 2021) from the band-restricted counts ``areas`` int64 [3,K] of ``sg_boundary_accumulate`` (rows:
    intersection of the two bands, prediction band, truth band): ``BIoU`` float64 [K] = areas[0] / (areas[1] + areas[2] - areas[0]),
    NaN where a class has no band pixel in prediction and truth, and ``summary['mBIoU']`` = ``nanmean * 100`` rounded to 2 decimals,
    with such a class left out of the mean (``nan_to_num`` replaces NaN first), as ``metrics_from_confusion`` treats ``IoU``."""
    inter, pred, label = _count_rows(areas, 3, "boundary areas")
    with np.errstate(divide="ignore", invalid="ignore"):
        biou = inter / (pred + label - inter)
    return _with_summary({"BIoU": biou}, ["mBIoU"], nan_to_num)


class BoundaryIoUMetric(_ImageShapeMetric):
    """``IoUMetric`` plus Boundary IoU: the confusion table as before and ``boundary_areas`` int64 [3,K], the counts restricted to the
    bands of prediction and truth (``sg_boundary_accumulate``).  The band width is ``boundary_ratio`` of each image's diagonal
    (``ops.boundary_width``; 0.02 as in the paper) or the fixed ``boundary_px``, which overrides the ratio.

    ``add`` / ``add_flat`` / ``reduce`` / ``compute`` as the shared base describes them; ``compute()`` adds ``BIoU`` and
    ``summary['mBIoU']``."""
    _ROWS, _ENTRY = 3, "sg_boundary_accumulate"

    def __init__(self, *args, boundary_ratio: float = 0.02, boundary_px: Optional[int] = None, **kwargs):
        from . import ops
        if boundary_px is not None:
            if isinstance(boundary_px, bool) or not isinstance(boundary_px, int) or not 1 <= boundary_px <= ops.BOUNDARY_MAX_D:
                raise ValueError(f"boundary_px must be an integer in [1, {ops.BOUNDARY_MAX_D}] or None, got {boundary_px!r}")
        else:
            ops.boundary_width((1, 1), boundary_ratio)                       # the ratio's own checks
        super().__init__(*args, **kwargs)
        self.boundary_ratio, self.boundary_px = boundary_ratio, boundary_px

    def width(self, hw) -> int:
        """The band width of an image of size ``hw``."""
        from . import ops
        return self.boundary_px if self.boundary_px is not None else ops.boundary_width(hw, self.boundary_ratio)

    @property
    def boundary_areas(self) -> torch.Tensor:
        """The [3,K] int64 band counts: intersection, prediction band, truth band."""
        return self._ensure_second()

    def _per_image(self, image_hw):
        return [self.width(hw) for hw in image_hw]

    def _count(self, labels, gt, image_hw, values, table, K, match_map) -> None:
        from . import ops
        ops.boundary_accumulate(labels, gt, image_hw, values, table, K, self.ignore_index, self.reduce_zero_label)

    def _scores(self) -> dict:
        return metrics_from_boundary(self.boundary_areas, self.nan_to_num)


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
    pred, right, true, found = _count_rows(counts, 4, "tolerant counts")
    with np.errstate(divide="ignore", invalid="ignore"):
        p, r = right / pred, found / true
        f = 2 * p * r / (p + r)
    keys = TOLERANT_KEYS[mode]
    return _with_summary(dict(zip(keys[:3], (p, r, f))), keys[3:], nan_to_num)


class RelaxedMetric(_ImageShapeMetric):
    """``IoUMetric`` plus the tolerant scores: the confusion table as before and ``tolerant_counts`` int64 [4,K]
    (``sg_tolerant_accumulate``).  ``mode`` "region" gives relaxed precision / recall / F (roads), "contour" the boundary F-score.
    The tolerance is ``tolerance_ratio`` of each image's diagonal (``ops.tolerance_sq``; 0.0075) or the fixed ``tolerance_px``
    (an integer in [0, 254]), which overrides the ratio.

    ``add`` / ``add_flat`` / ``reduce`` / ``compute`` as the shared base describes them; ``compute()`` adds the keys of
    ``metrics_from_tolerant``."""
    _ROWS, _ENTRY = 4, "sg_tolerant_accumulate"

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
        self.mode, self.tolerance_px, self.tolerance_ratio = mode, tolerance_px, tolerance_ratio

    def tolerance_sq(self, hw) -> int:
        """The squared tolerance of an image of size ``hw``."""
        from . import ops
        return self.tolerance_px * self.tolerance_px if self.tolerance_px is not None else ops.tolerance_sq(hw, self.tolerance_ratio)

    @property
    def tolerant_counts(self) -> torch.Tensor:
        """The [4,K] int64 counts: predicted, predicted and right, true, true and found."""
        return self._ensure_second()

    def _per_image(self, image_hw):
        return [self.tolerance_sq(hw) for hw in image_hw]

    def _count(self, labels, gt, image_hw, values, table, K, match_map) -> None:
        from . import ops
        ops.tolerant_accumulate(labels, gt, image_hw, values, table, K, self.ignore_index, self.reduce_zero_label, self.mode)

    def _scores(self) -> dict:
        return metrics_from_tolerant(self.tolerant_counts, self.mode, self.nan_to_num)


OBJECT_KEYS = ("ObjPrecision", "ObjRecall", "ObjF1", "SQ", "PQ")


def metrics_from_objects(counts, nan_to_num: Optional[int] = None) -> dict:
    """Object-level precision / recall / F1 and panoptic quality (Kirillov et al., CVPR 2019, with connected regions as the segments)
    from the counts int64 [4,K] of ``sg_object_match`` (rows: matched pairs TP, predicted objects, true objects, the matched pairs' IoU
    in steps of 2^-24): ``ObjPrecision`` = TP / counts[1], ``ObjRecall`` = TP / counts[2], ``ObjF1`` = RQ = 2 TP / (counts[1] +
    counts[2]), ``SQ`` = counts[3] / 2^24 / TP, ``PQ`` = SQ * RQ, float64 [K], NaN where a denominator is 0; and ``summary`` with
    ``mObjPrecision`` / ``mObjRecall`` / ``mObjF1`` / ``mSQ`` / ``mPQ``: ``nanmean * 100`` rounded to 2 decimals, NaN classes left out
    (``nan_to_num`` replaces NaN first), as ``metrics_from_tolerant`` does."""
    tp, pred, true, iou_q = _count_rows(counts, 4, "object counts")
    with np.errstate(divide="ignore", invalid="ignore"):
        rq, sq = 2 * tp / (pred + true), iou_q / float(1 << 24) / tp
        vals = (tp / pred, tp / true, rq, sq, sq * rq)
    return _with_summary(dict(zip(OBJECT_KEYS, vals)), ["m" + k for k in OBJECT_KEYS], nan_to_num)


class ObjectMetric(_ImageShapeMetric):
    """``IoUMetric`` plus the object-level scores: the confusion table as before and ``object_counts`` int64 [4,K]
    (``sg_object_match``): per class the connected regions of prediction and truth, matched where their IoU is strictly above
    ``object_iou`` (a float or a ``(num, den)`` pair in [1/2, 1), ``ops.object_iou_fraction``).  A region is an object when it has at
    least ``min_area`` pixels and its class is not ``skip_label`` (the background of a building or road set); ``connectivity`` 4 or 8.

    ``add`` / ``add_flat`` / ``reduce`` / ``compute`` as the shared base describes them; ``add`` and ``add_flat`` also take
    ``match_map``: None, or a uint8 tensor of the labels' size that receives the TP / FP / FN picture (``ops.object_match``);
    ``compute()`` adds the keys of ``metrics_from_objects``."""
    _ROWS, _ENTRY = 4, "sg_object_match"

    def __init__(self, *args, object_iou=0.5, min_area: int = 1, connectivity: int = 4, skip_label: Optional[int] = None, **kwargs):
        from . import ops
        self.object_iou = ops.object_args([(1, 1)], 1, object_iou, connectivity, min_area, skip_label)[2]
        super().__init__(*args, **kwargs)
        self.min_area, self.connectivity, self.skip_label = int(min_area), int(connectivity), skip_label

    @property
    def object_counts(self) -> torch.Tensor:
        """The [4,K] int64 counts: matched pairs, predicted objects, true objects, the matched pairs' IoU in steps of 2^-24."""
        return self._ensure_second()

    def add(self, labels: torch.Tensor, gt: torch.Tensor, match_map: Optional[torch.Tensor] = None) -> None:
        """The base's ``add`` with ``match_map``, a uint8 tensor of the map's size."""
        gt, hw = self._one_map(labels, gt)
        self.add_flat(labels.reshape(-1), gt.reshape(-1), [hw], match_map)

    def add_flat(self, labels: torch.Tensor, gt: torch.Tensor, image_hw, match_map: Optional[torch.Tensor] = None) -> None:
        """The base's ``add_flat`` with ``match_map``, a uint8 tensor of the labels' size."""
        self._add_flat(labels, gt, image_hw, match_map)

    def _count(self, labels, gt, image_hw, values, table, K, match_map) -> None:
        from . import ops
        ops.object_match(labels, gt, image_hw, table, K, self.object_iou, self.connectivity, self.min_area, self.skip_label,
                         self.ignore_index, self.reduce_zero_label, match_map)

    def _scores(self) -> dict:
        return metrics_from_objects(self.object_counts, self.nan_to_num)


try:  # with mmseg installed the classes are also buildable from a config, under names that leave mmseg's own IoUMetric alone
    from mmseg.registry import METRICS as _METRICS
    _METRICS.register_module(name="HipIoUMetric", module=IoUMetric)
    _METRICS.register_module(name="HipBoundaryIoUMetric", module=BoundaryIoUMetric)
    _METRICS.register_module(name="HipRelaxedMetric", module=RelaxedMetric)
    _METRICS.register_module(name="HipObjectMetric", module=ObjectMetric)
except Exception:
    pass
