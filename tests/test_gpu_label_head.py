"""sg_label_head / sg_label_head_multi (stitch -> softmax -> synonym merge -> argmax -> threshold, labels only, any Q) against the float64
reference of tests/head_reference.py, whose module docstring holds the acceptance rule (G, CAP) and its derivation; against the canvas
path for Q <= 64; guard bands, repeatability, and multi == single byte for byte."""
import functools

import numpy as np
import pytest
import torch

import head_reference as HR

pytestmark = pytest.mark.gpu

SCALE, BG = 50.0, 3
GUARD = 64


@functools.lru_cache(maxsize=None)
def case(geom, Q, merge):
    c = HR.make_case(geom, Q, merge)
    c["canvas"] = HR.stitch(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])     # computed once, never modified
    return c


def run_head(c, thd, want_conf=True):
    from clip_decontamination_amd import ops
    tl = torch.from_numpy(c["tile_logits"]).cuda()
    return ops.label_head(tl, torch.from_numpy(c["windows"]), c["up_hw"], c["pad_tl"], c["hw"], torch.from_numpy(c["query_idx"]), c["K"],
                          SCALE, thd, BG, want_conf=want_conf)


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
@pytest.mark.parametrize("Q", HR.QS)
@pytest.mark.parametrize("geom", ["a", "b"])
def test_label_head_matches_the_f64_reference(geom, Q, merge):
    c = case(geom, Q, merge)
    for thd in (0.0, 0.3):
        ref = HR.tail(c["canvas"], c["query_idx"], c["K"], SCALE, thd, BG)
        labels, conf = run_head(c, thd)
        assert labels.shape == (1,) + c["hw"] and labels.dtype == torch.int64 and conf.shape == c["hw"]
        HR.check_labels(ref, labels.cpu().numpy(), conf.cpu().numpy(), thd, f"{geom} Q={Q} K={c['K']} thd={thd}")
        if thd > 0 and Q > 1:
            assert (ref["conf"] < thd).any(), "the case never takes the threshold branch"


@pytest.mark.parametrize("Q,merge", [(9, True)])
def test_more_than_64_tiles_over_one_block(Q, merge):
    """crop 32 at stride 2: 100 windows hit the first block, beyond the candidate list (ST_MAXC = 64) -> every window is tested.
    Up to 80 tiles cover a pixel here, so the stitched logits are means of many i.i.d. values and an order of magnitude flatter than in
    the other cases: in the float64 reference itself 0.46 % of the pixels are within G of a tie or of the threshold at Q = 9, 1.07 % at
    Q = 65 and 2.75 % at Q = 257 (tests/test_head_reference_cpu.py).  Q = 9 (two register chunks, the second ragged, shuffled synonyms)
    keeps the case under the cap; the fall-back itself does not depend on Q."""
    c = case("dense", Q, merge)
    assert len(c["windows"]) > 64
    ref = HR.tail(c["canvas"], c["query_idx"], c["K"], SCALE, 0.3, BG)
    labels, conf = run_head(c, 0.3)
    HR.check_labels(ref, labels.cpu().numpy(), conf.cpu().numpy(), 0.3, f"dense Q={Q}")


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
@pytest.mark.parametrize("Q", [q for q in HR.QS if q <= 64])
def test_label_head_against_the_canvas_path(Q, merge):
    """ops.stitch + ops.postprocess on the same inputs: the same criterion (pixels decided beyond f32 rounding) and the same cap."""
    from clip_decontamination_amd import ops
    c = case("b", Q, merge)
    for thd in (0.0, 0.3):
        ref = HR.tail(c["canvas"], c["query_idx"], c["K"], SCALE, thd, BG)
        canvas = ops.stitch(torch.from_numpy(c["tile_logits"]).cuda(), torch.from_numpy(c["windows"]), c["up_hw"], c["pad_tl"], c["hw"])
        probs, lab_c = ops.postprocess(canvas, torch.from_numpy(c["query_idx"]), c["K"], SCALE, thd, BG)
        labels, conf = run_head(c, thd)
        ok = HR.counted(ref, thd)
        assert 1.0 - ok.mean() <= HR.CAP
        assert np.array_equal(labels.cpu().numpy()[0][ok], lab_c.cpu().numpy()[0][ok])
        assert np.abs(conf.cpu().numpy() - probs.max(0)[0].cpu().numpy())[ok].max() <= HR.G


def test_outputs_stay_inside_their_guard_bands_and_repeat():
    """Raw entry on buffers with sentinel / NaN bands on both sides; two calls give the same bytes; conf may be NULL."""
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    c = case("a", 65, True)
    H, W = c["hw"]
    T, Q, gh, gw = c["tile_logits"].shape
    tl = torch.from_numpy(c["tile_logits"]).cuda()
    win = torch.from_numpy(c["windows"]).cuda()
    qi = torch.from_numpy(c["query_idx"]).cuda()
    outs = []
    for rep in range(2):
        lab = torch.full((H * W + 2 * GUARD,), -12345, dtype=torch.int64, device="cuda")
        conf = torch.full((H * W + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.sg_label_head(ops.ptr(tl), ops.ptr(win), T, Q, gh, gw, *c["up_hw"], *c["pad_tl"], H, W, ops.ptr(qi), c["K"], SCALE,
                                     0.3, BG, ops.ptr(lab[GUARD:]), ops.ptr(conf[GUARD:]), ops.stream_ptr()), "sg_label_head")
        torch.cuda.synchronize()
        for g in (lab[:GUARD], lab[-GUARD:]):
            assert bool((g == -12345).all())
        for g in (conf[:GUARD], conf[-GUARD:]):
            assert bool(torch.isnan(g).all())
        body = lab[GUARD:-GUARD]
        assert bool(((body >= 0) & (body < max(c["K"], BG + 1))).all()) and not bool(torch.isnan(conf[GUARD:-GUARD]).any())
        outs.append((lab.cpu(), conf.cpu()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert outs[0][1].numpy().tobytes() == outs[1][1].numpy().tobytes()
    only = torch.full((H * W,), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.sg_label_head(ops.ptr(tl), ops.ptr(win), T, Q, gh, gw, *c["up_hw"], *c["pad_tl"], H, W, ops.ptr(qi), c["K"], SCALE, 0.3, BG,
                                 ops.ptr(only), None, ops.stream_ptr()), "sg_label_head")
    assert torch.equal(only.cpu(), outs[0][0][GUARD:-GUARD])


def test_refusals_happen_before_the_launch():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    import ctypes
    p = ctypes.c_void_p(1 << 20)                                   # never dereferenced
    assert lib.sg_label_head(p, p, 4, 8, 3, 3, 42, 42, 1, 1, 70, 90, p, 9, 50.0, 0.0, 0, p, None, None) != 0
    assert b"K=9" in lib.sg_last_error()
    assert lib.sg_label_head(p, p, 4, 8, 3, 3, 42, 42, 1, 1, 70, 90, p, 0, 50.0, 0.0, 0, p, None, None) != 0
    assert lib.sg_label_head(p, p, 4, 8, 3, 3, 42, 42, 1, 1, 70, 90, None, 8, 50.0, 0.0, 0, p, None, None) != 0
    assert b"null pointer" in lib.sg_last_error()
    assert lib.sg_label_head(p, p, 0, 8, 3, 3, 42, 42, 1, 1, 70, 90, p, 8, 50.0, 0.0, 0, p, None, None) != 0
    assert b"bad shape" in lib.sg_last_error()
    assert lib.sg_label_head_multi(p, p, p, 4, 8, 3, 3, 42, 42, 1, 1, p, p, p, p, 5, 10, 100, p, 8, 50.0, 0.0, 0, p, None, None) != 0
    assert b"bad shape" in lib.sg_last_error()
    assert lib.sg_label_head_multi(p, p, p, 4, 8, 3, 3, 42, 42, 1, 1, p, p, p, p, 2, 0, 100, p, 8, 50.0, 0.0, 0, p, None, None) != 0
    assert b"total_blocks" in lib.sg_last_error()


@pytest.mark.parametrize("Q,merge", [(9, True), (130, False)])
def test_multi_equals_single_per_image(Q, merge):
    """Three images of different sizes (one window size) in one launch: byte-equal to sg_label_head per image, labels and conf."""
    from clip_decontamination_amd import ops
    H0, W0, stride, crop, grid, up_hw, pad_tl = HR.GEOMETRIES["a"]
    shapes = [(70, 90), (40, 57), (83, 40)]
    rng = np.random.default_rng(Q)
    wins = [HR.slide_windows(h, w, stride, crop) for h, w in shapes]
    n_t = [len(w) for w in wins]
    tl = torch.from_numpy((0.3 * rng.standard_normal((sum(n_t), Q) + grid)).astype(np.float32)).cuda()
    qi = torch.from_numpy(HR.make_case("a", Q, merge)["query_idx"])
    K = int(qi.max()) + 1 if merge else Q
    first = [0, n_t[0], n_t[0] + n_t[1]]
    tile_image = [n for n in range(3) for _ in range(n_t[n])]
    lab, flat, conf = ops.label_head_multi(tl, [w for ws in wins for w in ws], tile_image, up_hw, pad_tl, shapes, list(zip(first, n_t)), qi, K,
                                           SCALE, 0.3, BG, want_conf=True)
    assert flat.numel() == sum(h * w for h, w in shapes)
    for n, (h, w) in enumerate(shapes):
        l1, c1 = ops.label_head(tl[first[n]:first[n] + n_t[n]], torch.tensor(wins[n], dtype=torch.int32), up_hw, pad_tl, (h, w), qi, K, SCALE,
                                0.3, BG, want_conf=True)
        assert lab[n].shape == (1, h, w) and torch.equal(lab[n], l1), n
        assert conf[n].cpu().numpy().tobytes() == c1.cpu().numpy().tobytes(), n
        ref = HR.label_head(tl[first[n]:first[n] + n_t[n]].cpu().numpy(), wins[n], up_hw, pad_tl, (h, w), qi.numpy(), K, SCALE, 0.3, BG)
        HR.check_labels(ref, l1.cpu().numpy(), c1.cpu().numpy(), 0.3, f"multi image {n} Q={Q}")
