"""CPU-side checks of the top-k head: the float64 reference of tests/topk_reference.py meets its own cap on every case the GPU test
runs; hand-made cases through the reference and through ops.topk_from_probs; the C ABI of sg_topk_head / sg_topk_head_multi (declared,
exported, refusals before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import head_reference as HR
import topk_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")


@pytest.mark.parametrize("geom,Q,merge", TR.CASES + TR.DENSE + [("dense", 65, False)])
def test_the_reference_alone_meets_the_cap(geom, Q, merge):
    """The uncounted shares of the exact cases of tests/test_gpu_topk_head.py: at most CAP of all slots and of any single slot index."""
    c = TR.case(geom, Q, merge)
    for k in TR.ks_of(c["K"]):
        frac, worst = TR.shares(TR.topk(c["ranked"], k))
        print(f"{geom} Q={Q} K={c['K']} k={k}: uncounted {100 * frac:.3f} %, worst slot index {100 * worst:.3f} %")
        assert frac <= TR.CAP and worst <= TR.CAP, (geom, Q, merge, k, frac, worst)


def test_the_reference_passes_its_own_check_and_catches_a_swap():
    c = TR.case("a", 9, True)
    ref = TR.topk(c["ranked"], 3)
    TR.check(ref, ref["classes"], ref["probs"].astype(np.float32), "self")
    swapped = ref["classes"].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(AssertionError, match="another class"):
        TR.check(ref, swapped, ref["probs"], "swapped")
    with pytest.raises(AssertionError, match="of its bound"):
        TR.check(ref, ref["classes"], ref["probs"] * 1.002, "scaled")


def _canvas(values):
    """[Q] values -> canvas [Q,1,1] such that canvas * SCALE = values."""
    return (np.asarray(values, dtype=np.float64) / TR.SCALE).reshape(-1, 1, 1)


def _probs_f64(canvas, qi, K):
    return HR.tail(canvas, qi, K, TR.SCALE, 0.0, 0)["probs"]


def _both(values, qi, K, k):
    """The reference and ops.topk_from_probs (on the float64 class probabilities of head_reference.tail) on one pixel."""
    from clip_decontamination_amd import ops
    canvas = _canvas(values)
    ref = TR.topk(TR.rank(canvas, qi, K, TR.SCALE), k)
    cls, prb = ops.topk_from_probs(torch.from_numpy(_probs_f64(canvas, qi, K)), torch.as_tensor(qi), k)
    assert cls.dtype == torch.int32 and prb.dtype == torch.float32 and cls.shape == prb.shape == (k, 1, 1)
    return ref, cls.numpy().reshape(-1), prb.numpy().reshape(-1)


def test_synonyms_merge_into_one_slot():
    values, qi = [1.0, 3.0, 2.0, 0.5, 2.5], [0, 1, 0, 2, 1]                 # class 0: max(1, 2), class 1: max(3, 2.5), class 2: 0.5
    ref, cls, prb = _both(values, qi, 3, 3)
    assert ref["classes"].reshape(-1).tolist() == [1, 0, 2] == cls.tolist()
    e = np.exp(np.asarray(values))
    want = np.array([e[1], e[2], e[3]]) / e.sum()
    assert np.allclose(ref["probs"].reshape(-1), want, rtol=1e-12) and np.allclose(prb, want, rtol=1e-6)
    assert bool(ref["counted"].all())


def test_equal_values_are_ordered_by_class():
    values, qi = [2.0, 2.0, 2.0, 1.0], [2, 0, 1, 3]                          # three classes tie: ascending class, then class 3
    ref, cls, prb = _both(values, qi, 4, 4)
    assert ref["classes"].reshape(-1).tolist() == [0, 1, 2, 3] == cls.tolist()
    assert ref["counted"].reshape(-1).tolist() == [False, False, False, True]  # a tie is never a counted slot
    assert prb[0] == prb[1] == prb[2] > prb[3]


def test_a_class_without_a_query_gives_an_unfilled_slot():
    values, qi = [0.3, 1.0, 0.1], [0, 2, 3]                                   # class 1 of K = 4 owns no query
    ref, cls, prb = _both(values, qi, 4, 4)
    assert ref["classes"].reshape(-1).tolist() == [2, 0, 3, -1] == cls.tolist()
    assert ref["probs"].reshape(-1)[3] == 0.0 == prb[3] and bool(ref["counted"].all())
    ref2, cls2, _ = _both(values, qi, 4, 2)                                   # k = 2: rank 3 exists and is decided
    assert ref2["classes"].reshape(-1).tolist() == [2, 0] == cls2.tolist() and bool(ref2["counted"].all())


def test_an_uncovered_pixel_lists_the_classes_in_ascending_order():
    """No covering tile: every stitched value is 0 (head_reference.stitch), so the classes come in ascending index with equal
    probabilities 1 / Q and no slot is counted."""
    wins, grid, up, pad, hw = HR.stitch_geometry("hole")
    tl = np.random.default_rng(5).standard_normal((len(wins), 6) + tuple(grid)).astype(np.float32)
    canvas = HR.stitch(tl, wins, up, pad, hw)
    assert (canvas[:, :, 30:40] == 0).all()
    for qi, K in ((np.arange(6), 6), (np.array([2, 0, 1, 2, 0, 1]), 3)):
        ref = TR.topk(TR.rank(canvas, qi, K, TR.SCALE), 3)
        hole = ref["classes"][:, :, 30:40]
        assert (hole == np.arange(3)[:, None, None]).all()
        assert np.allclose(ref["probs"][:, :, 30:40], 1.0 / 6.0, rtol=1e-12)
        assert not ref["counted"][:, :, 30:40].any()


def test_k_equal_to_K():
    values, qi = [0.0, 4.0, 2.0], [0, 1, 2]
    ref, cls, prb = _both(values, qi, 3, 3)
    assert ref["classes"].reshape(-1).tolist() == [1, 2, 0] == cls.tolist()
    assert abs(ref["probs"].sum() - 1.0) < 1e-12 and abs(float(prb.sum()) - 1.0) < 1e-6
    assert bool(ref["counted"].all())                                         # there is no rank k + 1 to be close to


def test_topk_from_probs_refuses_a_bad_k():
    from clip_decontamination_amd import ops
    p = torch.rand(3, 2, 2)
    for k in (0, 4, 9):
        with pytest.raises(ValueError, match=f"k={k}"):
            ops.topk_from_probs(p, torch.arange(3), k)


# ---- the C ABI, on a machine without a GPU ------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_both_entries():
    from clip_decontamination_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sg_topk_head", "sg_topk_head_multi"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+SG_TOPK_MAX\s+8\b", src)
    from clip_decontamination_amd import ops
    assert ops.TOPK_MAX == TR.KMAX == 8


def test_refusals_happen_before_any_launch():
    """Every refusal returns non-zero with a message that names the values, from pointers that are never dereferenced."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)

    def single(*, tl=p, qi=p, T=4, Q=8, K=8, k=3, classes=p, probs=p):
        return lib.sg_topk_head(tl, p, T, Q, 3, 3, 42, 42, 1, 1, 70, 90, qi, K, 50.0, k, classes, probs, None)

    def multi(*, N=2, blocks=10, pixels=100, Q=8, K=8, k=3, classes=p, desc=p):
        return lib.sg_topk_head_multi(p, p, p, 4, Q, 3, 3, 42, 42, 1, 1, desc, p, p, p, N, blocks, pixels, p, K, 50.0, k, classes, p, None)

    cases = [
        (single, dict(k=0), b"k=0"),
        (single, dict(k=9), b"k=9"),
        (single, dict(k=5, K=4), b"k=5"),
        (single, dict(K=0), b"K=0"),
        (single, dict(K=9), b"K=9"),
        (single, dict(tl=None), b"null pointer"),
        (single, dict(qi=None), b"null pointer"),
        (single, dict(classes=None), b"null pointer"),
        (single, dict(probs=None), b"null pointer"),
        (single, dict(T=0), b"bad shape T=0"),
        (multi, dict(k=0), b"k=0"),
        (multi, dict(k=9), b"k=9"),
        (multi, dict(k=5, K=4), b"k=5"),
        (multi, dict(K=0), b"K=0"),
        (multi, dict(K=9), b"K=9"),
        (multi, dict(classes=None), b"null pointer"),
        (multi, dict(desc=None), b"null pointer"),
        (multi, dict(N=5), b"bad shape"),
        (multi, dict(blocks=0), b"total_blocks=0"),
        (multi, dict(pixels=0), b"out_pixels=0"),
    ]
    for fn, kw, msg in cases:
        assert fn(**kw) != 0, kw
        err = lib.sg_last_error()
        assert msg in err and (b"sg_topk_head_multi" if fn is multi else b"sg_topk_head:") in err, (kw, err)
