"""The test-time-augmentation reference on the CPU (tests/tta_reference.py): the f32 emulation of sg_tta_head passes the acceptance rule of
tests/test_gpu_tta.py on every case that file runs -- so the float64 reference alone meets check_labels' cap and the bound leaves room for
the kernel's arithmetic -- each mutant is rejected on at least one case, and ``ops.tta_views`` lists the views the definition names."""
import numpy as np
import pytest

import tta_reference as TT

# the mutants are tried on a few cheap cases that have what each one needs: a flipped view (no_unflip, flip_rows, divide_by_scales),
# more than one view (mean_of_logits)
MUTANT_CASES = [c for c in TT.CASES if c[0] in ("a+af", "a+bf+af") and c[1] in (5, 17)]


@pytest.mark.parametrize("vs,Q,merge,out", TT.CASES, ids=[TT.case_id(*c) for c in TT.CASES])
def test_the_f32_emulation_passes_the_acceptance_rule(vs, Q, merge, out):
    for thd in TT.THDS:
        ref, bound = TT.reference(vs, Q, merge, out, thd)
        labels, conf, probs = TT.emulate(vs, Q, merge, out, thd)
        TT.check(ref, bound, labels, conf, probs, thd, f"{TT.case_id(vs, Q, merge, out)} thd={thd}")


def _passes(case, mut):
    vs, Q, merge, out = case
    try:
        for thd in TT.THDS:
            ref, bound = TT.reference(vs, Q, merge, out, thd)
            TT.check(ref, bound, *TT.emulate(vs, Q, merge, out, thd, mut), thd, f"{mut} {TT.case_id(*case)}")
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("mut", TT.MUTANTS)
def test_every_mutant_is_rejected(mut):
    assert MUTANT_CASES
    assert all(_passes(c, None) for c in MUTANT_CASES[:1])                 # the rule is not one that rejects everything
    rejected = [TT.case_id(*c) for c in MUTANT_CASES if not _passes(c, mut)]
    print(f"{mut}: rejected on {len(rejected)} of {len(MUTANT_CASES)} cases")
    assert rejected, f"{mut} passes every case"


def test_one_view_is_the_resized_label_head_reference():
    """[a] at any size: the merged reference is head_resized_reference's own tail."""
    import head_resized_reference as RR
    for Q, merge, out in ((5, False, TT.OUTS[0]), (17, True, TT.OUTS[1])):
        ref, _ = TT.reference("a", Q, merge, out, 0.3)
        c = RR.resized("a", Q, merge, out)
        t = RR.tail(c, 0.3)
        assert np.array_equal(ref["labels"], t["labels"]) and np.array_equal(ref["conf"], t["conf"])


def test_tta_views():
    from clip_decontamination_amd import ops
    assert ops.tta_views((100, 200), None) == [(1.0, False, (100, 200))]
    assert ops.tta_views((100, 200), None, True) == [(1.0, False, (100, 200)), (1.0, True, (100, 200))]
    v = ops.tta_views((101, 66), (0.75, 1.0, 1.25), True)
    assert [(s, f) for s, f, _ in v] == [(0.75, False), (0.75, True), (1.0, False), (1.0, True), (1.25, False), (1.25, True)]   # scale outer
    assert [hw for _, _, hw in v][::2] == [(76, 50), (101, 66), (126, 83)]          # 75.75 -> 76, 49.5 -> 50, 126.25 -> 126, 82.5 -> 83
    assert ops.tta_views((2, 2), (0.25,)) == [(0.25, False, (1, 1))]                # 0.5 rounds up
    assert ops.tta_views((1, 3), (0.1,)) == [(0.1, False, (1, 1))]                  # never below one pixel
    assert ops.tta_views((10, 10), 0.5) == [(0.5, False, (5, 5))]
    assert len(ops.tta_views((10, 10), (0.5, 0.75, 1.0, 1.25), True)) == 8 == ops.TTA_MAX_VIEWS
    with pytest.raises(ValueError, match="at most 8 views, got 10"):
        ops.tta_views((10, 10), (0.5, 0.75, 1.0, 1.25, 1.5), True)
    with pytest.raises(ValueError, match="at most 8 views, got 9"):
        ops.tta_views((10, 10), tuple(0.5 + 0.1 * i for i in range(9)))
    for bad in ((), (0.0,), (-1.0,), (float("inf"),), (float("nan"),)):
        with pytest.raises(ValueError, match="tta_scales must be"):
            ops.tta_views((10, 10), bad)
