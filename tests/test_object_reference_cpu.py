"""tests/object_reference.py against hand-worked maps and against itself: the pairs whose counts can be worked out on paper, the power of
the GPU case set against every mutant of the reference, and the identities of the definition."""
import numpy as np
import pytest

import object_reference as R

_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = list(R.gpu_cases())
    return _CASES


@pytest.mark.parametrize("name", sorted(R.hand_maps()))
def test_hand_worked_maps(name):
    p, g, want = R.hand_maps()[name]
    for iou, tp in want.items():
        for conn in (4, 8):
            counts, mm, pairs = R.match(p, g, 3, iou, connectivity=conn, skip_label=R.BG)
            assert counts[0].sum() == tp == len(pairs), (name, iou, counts.tolist())
            assert counts[0, 0] == counts[1, 0] == counts[2, 0] == 0                     # the background is skipped


def test_the_numbers_of_the_hand_worked_maps():
    H = R.hand_maps()
    p, g, _ = H["moved_by_a_column"]
    c, mm, pairs = R.match(p, g, 3, (1, 2), skip_label=0)
    assert c[:, 1].tolist() == [1, 1, 1, (12 << 24) // 20] and pairs == [(2 * 14 + 2, 2 * 14 + 3)]
    assert mm[2, 2] == 1 and mm[2, 3] == 5 and mm[2, 6] == 4 and mm[0, 0] == 0
    c, mm, pairs = R.match(p, g, 3, (3, 4), skip_label=0)
    assert c[:, 1].tolist() == [0, 1, 1, 0] and pairs == [] and mm[2, 2] == 2 and mm[2, 3] == 10 and mm[2, 6] == 8
    assert R.match(p, g, 3, (3, 5), skip_label=0)[0][0, 1] == 0                          # 12 / 20 is exactly 3/5: strict
    assert R.match(p, g, 3, (599, 1000), skip_label=0)[0][0, 1] == 1
    p, g, _ = H["exactly_half"]
    assert R.match(p, g, 3, (1, 2), skip_label=0)[0][:, 1].tolist() == [0, 1, 1, 0]
    assert R.match(p, g, 3, (1, 2), skip_label=0, mutant="ge")[0][:, 1].tolist() == [1, 1, 1, 1 << 23]
    p, g, _ = H["three_ways"]
    assert R.match(p, g, 3, (1, 2), skip_label=0)[0][:, 1].tolist() == [0, 1, 3, 0]
    p, g, _ = H["majority_too_large"]
    assert R.match(p, g, 3, (1, 2), skip_label=0)[0][:, 1].tolist() == [0, 1, 1, 0]
    assert R.match(p, g, 3, (1, 2), skip_label=0, mutant="iou_over_p")[0][0, 1] == 1
    p, g, _ = H["two_halves"]
    assert R.match(p, g, 3, (1, 2), skip_label=0)[0][:, 1].tolist() == [0, 2, 1, 0]
    p, g, _ = H["large_and_small_part"]
    c, mm, _ = R.match(p, g, 3, (1, 2), skip_label=0)
    assert c[:, 1].tolist() == [1, 2, 1, (12 << 24) // 20] and mm[2, 2] == 5 and mm[2, 6] == 6 and mm[2, 5] == 4
    p, g, _ = H["other_class"]
    c = R.match(p, g, 3, (1, 2), skip_label=0)[0]
    assert c[:, 1].tolist() == [0, 1, 0, 0] and c[:, 2].tolist() == [0, 0, 1, 0]
    p, g, _ = H["equal_and_three_quarters"]
    c = R.match(p, g, 3, (1, 2), skip_label=0)[0]
    assert c[:, 1].tolist() == [1, 1, 1, 1 << 24] and c[:, 2].tolist() == [1, 1, 1, 3 << 22]
    # without skip_label the background is an object too, with min_area it is the small ones that go
    c = R.match(p, g, 3, (1, 2))[0]
    assert c[:, 0].tolist()[:3] == [1, 1, 1]
    assert R.match(p, g, 3, (1, 2), skip_label=0, min_area=7)[0][:3, 2].tolist() == [0, 1, 0]      # 8 and 6 pixels


def test_the_embedded_hand_maps_keep_their_counts():
    p, g, want = R.hand_embedded()
    for iou, tp in want.items():
        for conn in (4, 8):
            assert R.match(p, g, 3, iou, connectivity=conn, skip_label=R.BG)[0][0].sum() == tp


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_gpu_cases_tell_every_mutant_from_the_reference(mutant):
    for what, pairs, K, rzl, ign, params in cases():
        for iou, conn, area, skip in params:
            kw = dict(connectivity=conn, min_area=area, skip_label=skip, ignore_index=ign, rzl=rzl)
            a = R.match_batch(pairs, K, iou, **kw)
            b = R.match_batch(pairs, K, iou, mutant=mutant, **kw)
            if not np.array_equal(a[0], b[0]) or any(not np.array_equal(x, y) for x, y in zip(a[1], b[1])):
                return
    pytest.fail(f"no GPU case tells the mutant '{mutant}' ({R.MUTANTS[mutant]}) from the reference")


def test_identities():
    for what, pairs, K, rzl, ign, params in cases():
        if isinstance(what, tuple) and what[0] == 130:
            continue
        for conn, area, skip in sorted({(c, a, s) for _, c, a, s in params}, key=str):
            kw = dict(connectivity=conn, min_area=area, skip_label=skip)
            tps = []
            for iou in R.IOUS:
                c = R.match_batch(pairs, K, iou, ignore_index=ign, rzl=rzl, **kw)[0]
                assert (c[0] <= np.minimum(c[1], c[2])).all() and (c[3] <= c[0] * R.SQ_ONE).all() and (2 * c[3] > c[0] * R.SQ_ONE - (c[0] == 0)).all()
                tps.append(c[0])
            assert (tps[0] >= tps[1]).all() and (tps[1] >= tps[2]).all(), what                  # TP never grows with the threshold
            # the prediction against itself: everything matches at IoU 1
            same = [(p, p) for p, _ in pairs]
            c = R.match_batch(same, K, R.IOUS[2], ignore_index=-1, **kw)[0]
            assert np.array_equal(c[0], c[1]) and np.array_equal(c[0], c[2]) and np.array_equal(c[3], c[0] * R.SQ_ONE), what
            # swapping the maps swaps rows 1 and 2 and keeps rows 0 and 3
            g2 = [(p, R.transform(g, rzl)) for p, g in pairs]
            a = R.match_batch(g2, K, (1, 2), ignore_index=-1, **kw)[0]
            b = R.match_batch([(g, p) for p, g in g2], K, (1, 2), ignore_index=-1, **kw)[0]
            assert np.array_equal(a[[0, 2, 1, 3]], b), what


def test_the_gpu_cases_are_not_degenerate():
    tp = {iou: 0 for iou in R.IOUS[:2]}
    fp, fn = dict(tp), dict(tp)
    for what, pairs, K, rzl, ign, params in cases():
        for conn, area, skip in sorted({(c, a, s) for _, c, a, s in params}, key=str):
            for iou in tp:
                c = R.match_batch(pairs, K, iou, connectivity=conn, min_area=area, skip_label=skip, ignore_index=ign, rzl=rzl)[0]
                tp[iou] += int(c[0].sum()); fp[iou] += int((c[1] - c[0]).sum()); fn[iou] += int((c[2] - c[0]).sum())
    assert all(v > 0 for d in (tp, fp, fn) for v in d.values()), (tp, fp, fn)
    assert tp[(1, 2)] > tp[(3, 4)]


def test_scores():
    counts = np.array([[2, 0, 0], [4, 3, 0], [2, 0, 0], [3 << 23, 0, 0]], dtype=np.int64)
    pr, rc, f1, sq, pq = R.scores(counts)
    assert pr[0] == 0.5 and rc[0] == 1.0 and f1[0] == 2 * 2 / 6 and sq[0] == 0.75 and pq[0] == 0.75 * 4 / 6
    assert pr[1] == 0.0 and np.isnan(rc[1]) and f1[1] == 0.0 and np.isnan(sq[1]) and np.isnan(pq[1])
    assert all(np.isnan(v[2]) for v in (pr, rc, f1, sq, pq))
