"""The numpy reference of area_thd (tests/area_reference.py) without a GPU: equal, byte for byte, to a torch transcription of the upstream
statement of the option (one_hot -> per-class sums -> compare -> multiply -> argmax -> threshold, written here from the definition in
include/segearth_hip.h, bg_idx = 0); the cap and the preconditions of every case the GPU tests run; and the corners of the definition:
the strict comparison at equality, total = 0, and area_thd = 0."""
import numpy as np
import pytest
import torch

import area_reference as AR


def upstream_torch(probs: torch.Tensor, area_thd: float, prob_thd: float):
    """The option as the segmenter family states it, bg_idx = 0: dropped classes are multiplied by zero and compared as zeros."""
    K = probs.shape[0]
    pred = probs.argmax(0)
    area = torch.nn.functional.one_hot(pred, K).sum((0, 1))                       # [K] int64
    keep = area.double() > area_thd * area[1:].sum().double()
    keep[0] = True
    probs = probs * keep[:, None, None].to(probs.dtype)
    labels = probs.argmax(0)
    labels[probs.max(0).values < prob_thd] = 0
    return probs, labels, keep


def test_reference_equals_the_upstream_statement():
    rng = np.random.default_rng(5)
    n = 0
    for case in range(200):
        K = 2 + case % 18                                                          # 2 .. 19
        H, W = int(rng.integers(3, 20)), int(rng.integers(3, 20))
        z = rng.standard_normal((K, H, W)) * 2.0 + rng.choice([0.0, -2.0, -4.0], size=(K, 1, 1))
        p = np.exp(z - z.max(0)) / np.exp(z - z.max(0)).sum(0)
        if case % 3 == 0:
            p = np.round(p, 1)                                                     # exact ties between classes, zeros included
        for thd in (0.0, 0.02, 0.1, 0.3, 1.0):
            ref = AR.area_filter(p, thd, 0.3, 0)
            tp, tl, tk = upstream_torch(torch.from_numpy(p), thd, 0.3)
            assert ref["keep"].tolist() == tk.tolist()
            assert ref["probs"].tobytes() == tp.numpy().tobytes()
            assert ref["labels"].tobytes() == tl.numpy().tobytes()
            n += int((~ref["keep"]).any())
    assert n > 300, "hardly any case dropped a class: the comparison would show nothing"


@pytest.mark.parametrize("case", AR.CASES, ids=AR.case_id)
def test_cap_and_preconditions_of_the_gpu_cases(case):
    AR.check_preconditions(AR.make_case(*case), AR.case_id(case))


def test_gpu_cases_cover_both_paths_of_the_relabel():
    """Some 64 x 4 block has no dropped first label (the skip) and some has one (the gather), over the cases of geometries a and b."""
    skip = gather = 0
    for case in AR.CASES:
        c = AR.make_case(*case)
        d = ~c["ref"]["keep"][c["first"]["labels"]]
        H, W = d.shape
        for y in range(0, H, 4):
            for x in range(0, W, 64):
                if d[y:y + 4, x:x + 64].any():
                    gather += 1
                else:
                    skip += 1
    assert skip > 0 and gather > 0, (skip, gather)


def test_strict_comparison_at_equality():
    # bg 10 pixels, class 1 one pixel, class 2 three: total = 4, area_thd * total = 1.0 exactly -> 1 > 1 is false, 3 > 1 is true
    assert AR.keep_of([10, 1, 3], 0, 0.25).tolist() == [True, False, True]
    l0 = np.array([0] * 10 + [1] + [2] * 3).reshape(2, 7)
    p = np.full((3, 2, 7), 0.2)
    np.put_along_axis(p, l0[None], 0.6, axis=0)
    ref = AR.area_filter(p, 0.25, 0.3, 0)
    assert ref["area"].tolist() == [10, 1, 3] and ref["keep"].tolist() == [True, False, True]
    assert (ref["probs"][1] == 0).all() and (ref["probs"][[0, 2]] == p[[0, 2]]).all()
    want = l0.copy()
    want[l0 == 1] = 0                                                              # best kept: 0.2 and 0.2, the lower index; below prob_thd -> bg anyway
    assert (ref["labels"] == want).all()


def test_total_zero_keeps_only_the_background():
    p = np.zeros((4, 3, 5))
    p[2] = 0.9
    p[[0, 1, 3]] = 0.1 / 3
    ref = AR.area_filter(p, 0.0, 0.3, 2)
    assert ref["total"] == 0 and ref["keep"].tolist() == [False, False, True, False]
    assert (ref["labels"] == 2).all() and (ref["probs"][[0, 1, 3]] == 0).all()


def test_area_thd_zero_changes_no_label_and_zeroes_the_planes_that_never_win():
    rng = np.random.default_rng(2)
    z = rng.standard_normal((6, 9, 11)) * 3.0
    z[4] -= 100.0                                                                  # class 4 never wins
    p = np.exp(z - z.max(0)) / np.exp(z - z.max(0)).sum(0)
    for bg in (0, 4):
        ref = AR.area_filter(p, 0.0, 0.3, bg)
        off = np.where(p.max(0) < 0.3, bg, p.argmax(0))
        assert (ref["labels"] == off).all()
        assert ref["area"][4] == 0 and ref["keep"][4] == (bg == 4)
        assert (ref["probs"][4] == (p[4] if bg == 4 else 0)).all() and (ref["probs"][[0, 1, 2, 3, 5]] == p[[0, 1, 2, 3, 5]]).all()
