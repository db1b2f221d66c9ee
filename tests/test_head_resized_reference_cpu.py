"""CPU-side checks of the heads at another ori_shape: the float64 reference of tests/head_resized_reference.py meets the caps of the
existing acceptance rules on every case the GPU test runs, an f32 emulation of the kernels' arithmetic passes those rules, three
mutants fail them; the C ABI of the four entries (declared, exported, refusals before any launch) and the ops-level refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import head_reference as HR
import head_resized_reference as RR
import topk_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
ENTRIES = ("sg_label_head_resized", "sg_label_head_resized_multi", "sg_topk_head_resized", "sg_topk_head_resized_multi")
_below_thd = {}                                                           # geometry -> some case has pixels under the 0.3 threshold


@pytest.mark.parametrize("geom,Q,merge,out", RR.CASES, ids=[RR.case_id(*c) for c in RR.CASES])
def test_the_reference_meets_the_caps_and_the_emulation_passes(geom, Q, merge, out):
    """Per case: the uncounted shares of both rules stay under 1 %, and stitch_emulate + resize_emulate (f32, every product rounded)
    passes check_labels and topk_reference.check against the float64 reference."""
    c = RR.resized(geom, Q, merge, out)
    emu = RR.emulate(geom, Q, merge, out)
    for thd in RR.THDS:
        ref = RR.tail(c, thd)
        got = HR.tail(emu, c["query_idx"], c["K"], RR.SCALE, thd, RR.BG)
        frac = HR.check_labels(ref, got["labels"], got["conf"], thd, f"{RR.case_id(geom, Q, merge, out)} thd={thd}")
        assert frac <= HR.CAP
        if thd > 0:
            _below_thd[geom] = _below_thd.get(geom, False) or bool((ref["conf"] < thd).any())
    ranked = TR.rank(emu, c["query_idx"], c["K"], RR.SCALE)
    for k in TR.ks_of(c["K"]):
        ref = TR.topk(c["ranked"], k)
        frac, worst = TR.shares(ref)
        assert frac <= TR.CAP and worst <= TR.CAP, (k, frac, worst)
        got = TR.topk(ranked, k)
        TR.check(ref, got["classes"], got["probs"], f"{RR.case_id(geom, Q, merge, out)} k={k}")


@pytest.mark.parametrize("geom", ["a", "b"])
def test_the_threshold_branch_is_taken_in_each_geometry(geom):
    """Per geometry, not per case: 'a' with Q = 8 / 9 at 33 x 41 has no pixel under 0.3."""
    if geom not in _below_thd:                                            # run alone: one case that does take it
        c = RR.resized(geom, 65, False, RR.OUT_SIZES[geom][0])
        _below_thd[geom] = bool((RR.tail(c, 0.3)["conf"] < 0.3).any())
    assert _below_thd[geom]


def _passes(geom, Q, merge, out, mut):
    c = RR.resized(geom, Q, merge, out)
    emu = RR.emulate(geom, Q, merge, out, mut)
    try:
        for thd in RR.THDS:
            got = HR.tail(emu, c["query_idx"], c["K"], RR.SCALE, thd, RR.BG)
            HR.check_labels(RR.tail(c, thd), got["labels"], got["conf"], thd, f"{mut} thd={thd}")
        k = min(3, c["K"])
        got = TR.topk(TR.rank(emu, c["query_idx"], c["K"], RR.SCALE), k)
        TR.check(TR.topk(c["ranked"], k), got["classes"], got["probs"], f"{mut} k={k}")
    except AssertionError:
        return False
    return True


MUTANT_CASES = [(g, 9, m, o) for g in ("a", "b") for m in (False, True) for o in RR.OUT_SIZES[g]]


@pytest.mark.parametrize("mut", RR.MUTANTS)
def test_a_mutant_fails_the_rule(mut):
    """align_corners taps in the resize, the two output extents exchanged, the blend before the count division: each fails the rule on
    at least one case (the unmutated emulation passes all of them, above)."""
    failed = [RR.case_id(*c) for c in MUTANT_CASES if not _passes(*c, mut)]
    print(f"{mut}: fails {len(failed)} of {len(MUTANT_CASES)} cases: {failed}")
    assert failed, f"the mutant {mut} passes every case"
    upscale = [RR.case_id(*c) for c in MUTANT_CASES if RR.is_upscale(HR.GEOMETRIES[c[0]][:2], c[3]) and c[3] != HR.GEOMETRIES[c[0]][:2]]
    assert set(failed) & set(upscale), f"{mut} passes every upscale case"


def test_the_footprint_bound_holds_and_the_upscales_fit_the_stage():
    """ops.resized_footprint (csrc/head.hip's rs_span) against the taps themselves, for every block of every case's output; the cases
    the GPU test compares the two forms on fit the stage of 512 canvas pixels."""
    from clip_decontamination_amd import ops
    for geom, sizes in RR.OUT_SIZES.items():
        h, w = HR.GEOMETRIES[geom][:2]
        for out in sizes + ((13, 23), (3, 5), (1, 1), (700, 900)):
            rows, cols = ops.resized_footprint((h, w), out)
            for n_in, n_out, blk, cap in ((h, out[0], 4, rows), (w, out[1], 64, cols)):
                i0, i1, _, _ = HR.tap_f32(np.arange(n_out), n_in, n_out)
                for b0 in range(0, n_out, blk):
                    last = min(b0 + blk, n_out) - 1
                    assert i1[last] - i0[b0] + 1 <= cap, (geom, out, b0)
            if RR.is_upscale((h, w), out):
                assert rows * cols <= ops.RESIZED_STAGE_PIX, (geom, out)
    assert ops.resized_footprint((448, 448), (1024, 1024)) == (4, 30)


# ---- the C ABI and the ops, on a machine without a GPU ------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entries():
    from clip_decontamination_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    for form, val in ops.RESIZED_FORMS.items():
        assert re.search(rf"#define\s+SG_RESIZED_{form.upper()}\s+{val}\b", src)


def test_refusals_happen_before_any_launch():
    """Every refusal returns non-zero with a message that names the values, from pointers that are never dereferenced."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)

    def label(*, tl=p, T=4, Q=8, K=8, hw=(70, 90), out=(161, 207), labels=p, flags=0):
        return lib.sg_label_head_resized(tl, p, T, Q, 3, 3, 42, 42, 1, 1, *hw, *out, p, K, 50.0, 0.0, 0, labels, None, flags, None)

    def topk(*, tl=p, T=4, Q=8, K=8, k=3, hw=(70, 90), out=(161, 207), probs=p, flags=0):
        return lib.sg_topk_head_resized(tl, p, T, Q, 3, 3, 42, 42, 1, 1, *hw, *out, p, K, 50.0, k, p, probs, flags, None)

    def label_multi(*, N=2, blocks=10, pixels=100, K=8, out_hw=p, flags=0):
        return lib.sg_label_head_resized_multi(p, p, p, 4, 8, 3, 3, 42, 42, 1, 1, p, p, out_hw, p, p, N, blocks, pixels, p, K, 50.0, 0.0, 0, p,
                                               None, flags, None)

    def topk_multi(*, N=2, blocks=10, pixels=100, K=8, k=3, out_hw=p, flags=0):
        return lib.sg_topk_head_resized_multi(p, p, p, 4, 8, 3, 3, 42, 42, 1, 1, p, p, out_hw, p, p, N, blocks, pixels, p, K, 50.0, k, p, p,
                                              flags, None)

    cases = [
        (label, dict(tl=None), b"null pointer"), (label, dict(labels=None), b"null pointer"), (label, dict(T=0), b"bad shape T=0"),
        (label, dict(out=(0, 5)), b"out=0x5"), (label, dict(K=9), b"K=9"), (label, dict(flags=3), b"flags=3"),
        (label, dict(out=(33, 41), flags=2), b"staged form does not fit"),
        (topk, dict(tl=None), b"null pointer"), (topk, dict(probs=None), b"null pointer"), (topk, dict(k=0), b"k=0"),
        (topk, dict(k=9), b"k=9"), (topk, dict(out=(7, 0)), b"out=7x0"), (topk, dict(flags=-1), b"flags=-1"),
        (topk, dict(out=(33, 41), flags=2), b"staged form does not fit"),
        (label_multi, dict(out_hw=None), b"null pointer"), (label_multi, dict(N=5), b"bad shape"),
        (label_multi, dict(blocks=0), b"total_blocks=0"), (label_multi, dict(pixels=0), b"out_pixels=0"),
        (label_multi, dict(flags=7), b"flags=7"),
        (topk_multi, dict(out_hw=None), b"null pointer"), (topk_multi, dict(k=9), b"k=9"), (topk_multi, dict(blocks=0), b"total_blocks=0"),
        (topk_multi, dict(pixels=0), b"out_pixels=0"), (topk_multi, dict(flags=7), b"flags=7"),
    ]
    for fn, kw, msg in cases:
        assert fn(**kw) != 0, kw
        err = lib.sg_last_error()
        assert msg in err and b"head_resized" in err, (kw, err)


def test_the_ops_refuse_a_staged_form_that_does_not_fit():
    """Before any device work: the reason names the footprint and the stage."""
    import torch
    from clip_decontamination_amd import ops
    c = HR.make_case("a", 8, False)
    tl, win, qi = torch.from_numpy(c["tile_logits"]), torch.from_numpy(c["windows"]), torch.from_numpy(c["query_idx"])
    with pytest.raises(ValueError, match=r"staged form does not fit \(70, 90\) -> \(33, 41\).*exceeds the stage of 512"):
        ops.label_head_resized(tl, win, c["up_hw"], c["pad_tl"], c["hw"], (33, 41), qi, 8, 50.0, 0.0, 0, form="staged")
    with pytest.raises(ValueError, match="staged form does not fit"):
        ops.topk_head_resized(tl, win, c["up_hw"], c["pad_tl"], c["hw"], (33, 41), qi, 8, 50.0, 3, form="staged")
    with pytest.raises(ValueError, match="form='tiled'"):
        ops.label_head_resized(tl, win, c["up_hw"], c["pad_tl"], c["hw"], (33, 41), qi, 8, 50.0, 0.0, 0, form="tiled")
