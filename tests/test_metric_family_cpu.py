"""The second table of BoundaryIoUMetric, RelaxedMetric and ObjectMetric over a gloo group, without a GPU: reduce() sums both tables on
every rank and compute() scores the sums."""
import os

import numpy as np
import pytest
import torch

K, WORLD = 3, 2
KINDS = {"BoundaryIoUMetric": ("boundary_areas", "metrics_from_boundary", 3),
         "RelaxedMetric": ("tolerant_counts", "metrics_from_tolerant", 4),
         "ObjectMetric": ("object_counts", "metrics_from_objects", 4)}


def _tables(rank, rows):
    """Rank-dependent counts, every entry positive (no score is NaN, so summaries compare with ==)."""
    confusion = torch.arange((K + 1) * (K + 1), dtype=torch.int64).reshape(K + 1, K + 1) * (rank + 1) + 1 + rank
    second = torch.arange(rows * K, dtype=torch.int64).reshape(rows, K) * (rank + 2) + 3 * rank + 1
    return confusion, second


def _reduce_worker(rank, world, port, kind, q):
    import torch.distributed as dist
    from clip_decontamination_amd import metrics
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        prop, _, rows = KINDS[kind]
        m = getattr(metrics, kind)(num_classes=K, iou_metrics=["mIoU", "mFscore"])
        confusion, second = _tables(rank, rows)
        m.add_confusion(confusion)
        getattr(m, prop).add_(second)                              # the live table, before the first add
        m.reduce(dist.group.WORLD)
        q.put((rank, m.confusion.clone().numpy(), getattr(m, prop).clone().numpy(), m.compute()["summary"]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_reduce_sums_both_tables_of_a_gloo_group(kind):
    from clip_decontamination_amd import metrics
    from test_distributed_cpu import _run_ranks
    _, scores, rows = KINDS[kind]
    res = _run_ranks(_reduce_worker, WORLD, (kind,))
    want_confusion = sum(_tables(r, rows)[0] for r in range(WORLD)).numpy()
    want_second = sum(_tables(r, rows)[1] for r in range(WORLD)).numpy()
    summary = dict(metrics.metrics_from_confusion(want_confusion, ["mIoU", "mFscore"])["summary"],
                   **getattr(metrics, scores)(want_second)["summary"])
    assert not any(np.isnan(v) for v in summary.values())
    assert sorted(r[0] for r in res) == list(range(WORLD))
    for rank, confusion, second, got in res:
        assert confusion.dtype == np.int64 and np.array_equal(confusion, want_confusion), rank
        assert second.dtype == np.int64 and second.shape == (rows, K) and np.array_equal(second, want_second), rank
        assert got == summary and list(got) == list(summary), rank
