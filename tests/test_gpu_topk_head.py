"""sg_topk_head / sg_topk_head_multi (stitch -> softmax -> synonym merge -> the k best classes with their probabilities, any Q) against
the float64 reference of tests/topk_reference.py, whose module docstring holds the per-slot acceptance rule (GL, REL, CAP) and its
derivation; plane 0 against sg_label_head byte for byte; against the canvas route for Q <= 64; multi == single byte for byte; guard bands,
repeatability; classes without a query; pixels no tile covers.

Measured on the MI355X: no class mismatch on a counted slot in any case, worst err / bound of a counted probability 0.023 (geometry "b",
Q = 65, k = 8); DESIGN.md section 5 'Top-k head'."""
import numpy as np
import pytest
import torch

import head_reference as HR
import topk_reference as TR

pytestmark = pytest.mark.gpu

SCALE = TR.SCALE
GUARD = 64


def run_topk(c, k):
    from clip_decontamination_amd import ops
    tl = torch.from_numpy(c["tile_logits"]).cuda()
    cls, prb = ops.topk_head(tl, torch.from_numpy(c["windows"]), c["up_hw"], c["pad_tl"], c["hw"], torch.from_numpy(c["query_idx"]), c["K"],
                             SCALE, k)
    assert cls.shape == prb.shape == (k,) + tuple(c["hw"]) and cls.dtype == torch.int32 and prb.dtype == torch.float32
    return cls.cpu().numpy(), prb.cpu().numpy()


def check_range(cls, prb, K):
    assert ((cls >= -1) & (cls < K)).all()
    assert np.isfinite(prb).all() and (prb >= 0).all() and (prb <= 1).all()


@pytest.mark.parametrize("geom,Q,merge", TR.CASES, ids=[f"{g}-Q{Q}-{'merge' if m else 'ident'}" for g, Q, m in TR.CASES])
def test_topk_head_matches_the_f64_reference(geom, Q, merge):
    c = TR.case(geom, Q, merge)
    for k in TR.ks_of(c["K"]):
        cls, prb = run_topk(c, k)
        check_range(cls, prb, c["K"])
        TR.check(TR.topk(c["ranked"], k), cls, prb, f"{geom} Q={Q} K={c['K']} k={k}")


@pytest.mark.parametrize("geom,Q,merge", TR.DENSE + [("dense", 65, False)])
def test_more_than_64_tiles_over_one_block(geom, Q, merge):
    """crop 32 at stride 2: more windows hit the first block than the candidate list holds (ST_MAXC = 64), so every window is tested."""
    c = TR.case(geom, Q, merge)
    assert len(c["windows"]) > 64
    for k in TR.ks_of(c["K"]):
        cls, prb = run_topk(c, k)
        check_range(cls, prb, c["K"])
        TR.check(TR.topk(c["ranked"], k), cls, prb, f"dense Q={Q} K={c['K']} k={k}")


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
@pytest.mark.parametrize("Q", HR.QS)
def test_plane_0_is_the_label_head(Q, merge):
    """With prob_thd = 0 sg_label_head's labels are classes[0] on every pixel and its conf is probs[0] byte for byte: the two kernels run
    the same gather and the same statements, so a compiler that contracted them differently would show up here."""
    from clip_decontamination_amd import ops
    c = TR.case("a", Q, merge)
    tl = torch.from_numpy(c["tile_logits"]).cuda()
    labels, conf = ops.label_head(tl, torch.from_numpy(c["windows"]), c["up_hw"], c["pad_tl"], c["hw"], torch.from_numpy(c["query_idx"]),
                                  c["K"], SCALE, 0.0, 0, want_conf=True)
    for k in TR.ks_of(c["K"]):                                            # every KTOP instantiation
        cls, prb = run_topk(c, k)
        assert np.array_equal(cls[0], labels.cpu().numpy()[0]), k
        assert prb[0].tobytes() == conf.cpu().numpy().tobytes(), k


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
@pytest.mark.parametrize("Q", [q for q in HR.QS if q <= 64])
def test_topk_head_against_the_canvas_route(Q, merge):
    """ops.stitch + ops.postprocess + ops.topk_from_probs on the same inputs: held to the same reference by the same rule, and the two
    routes name the same class on every counted slot."""
    from clip_decontamination_amd import ops
    c = TR.case("b", Q, merge)
    qi = torch.from_numpy(c["query_idx"])
    canvas = ops.stitch(torch.from_numpy(c["tile_logits"]).cuda(), torch.from_numpy(c["windows"]), c["up_hw"], c["pad_tl"], c["hw"])
    probs, _ = ops.postprocess(canvas, qi, c["K"], SCALE, 0.0, 0)
    for k in TR.ks_of(c["K"]):
        ref = TR.topk(c["ranked"], k)
        cc, pc = ops.topk_from_probs(probs, qi, k)
        assert cc.dtype == torch.int32 and pc.dtype == torch.float32 and cc.shape == pc.shape == (k,) + tuple(c["hw"])
        cc, pc = cc.cpu().numpy(), pc.cpu().numpy()
        TR.check(ref, cc, pc, f"canvas route Q={Q} K={c['K']} k={k}")
        cls, prb = run_topk(c, k)
        ok = ref["counted"]
        assert np.array_equal(cls[ok], cc[ok])
        assert (np.abs(prb.astype(np.float64) - pc)[ok] <= 2 * (TR.REL * ref["probs"] + TR.ABS)[ok]).all()


@pytest.mark.parametrize("Q,merge", [(9, True), (9, False), (65, True), (65, False)])
def test_multi_equals_single_per_image(Q, merge):
    """Three images of 40 x 70, 32 x 32 and 50 x 33 in one launch: byte-equal to sg_topk_head per image, classes and probabilities."""
    from clip_decontamination_amd import ops
    m = HR.make_multi_case(Q)
    qi = torch.from_numpy(HR.make_case("a", Q, merge)["query_idx"])
    K = int(qi.max()) + 1 if merge else Q
    tl = torch.from_numpy(m["tile_logits"]).cuda()
    for k in sorted({min(3, K), min(8, K)}):
        cls, prb = ops.topk_head_multi(tl, m["windows"], m["tile_image"], m["up_hw"], m["pad_tl"], m["image_hw"], m["image_tiles"], qi, K,
                                       SCALE, k)
        for n, ((h, w), (first, count)) in enumerate(zip(m["image_hw"], m["image_tiles"])):
            wins = torch.from_numpy(m["windows"][first:first + count])
            c1, p1 = ops.topk_head(tl[first:first + count], wins, m["up_hw"], m["pad_tl"], (h, w), qi, K, SCALE, k)
            assert cls[n].shape == prb[n].shape == (k, h, w)
            assert torch.equal(cls[n], c1), (n, k)
            assert prb[n].cpu().numpy().tobytes() == p1.cpu().numpy().tobytes(), (n, k)
            canvas = HR.stitch(m["tile_logits"][first:first + count], m["windows"][first:first + count], m["up_hw"], m["pad_tl"], (h, w))
            TR.check(TR.topk(TR.rank(canvas, qi.numpy(), K, SCALE), k), c1.cpu().numpy(), p1.cpu().numpy(), f"multi image {n} Q={Q} k={k}",
                     cap=False)


@pytest.mark.parametrize("k", [3, 8])
def test_outputs_stay_inside_their_guard_bands_and_repeat(k):
    """Raw entry on buffers with sentinel / NaN bands on both sides of both outputs; two calls give the same bytes."""
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    c = TR.case("a", 65, True)
    H, W = c["hw"]
    T, Q, gh, gw = c["tile_logits"].shape
    tl = torch.from_numpy(c["tile_logits"]).cuda()
    win = torch.from_numpy(c["windows"]).cuda()
    qi = torch.from_numpy(c["query_idx"]).cuda()
    outs = []
    for rep in range(2):
        cls = torch.full((k * H * W + 2 * GUARD,), -12345, dtype=torch.int32, device="cuda")
        prb = torch.full((k * H * W + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.sg_topk_head(ops.ptr(tl), ops.ptr(win), T, Q, gh, gw, *c["up_hw"], *c["pad_tl"], H, W, ops.ptr(qi), c["K"], SCALE, k,
                                    ops.ptr(cls[GUARD:]), ops.ptr(prb[GUARD:]), ops.stream_ptr()), "sg_topk_head")
        torch.cuda.synchronize()
        for g in (cls[:GUARD], cls[-GUARD:]):
            assert bool((g == -12345).all())
        for g in (prb[:GUARD], prb[-GUARD:]):
            assert bool(torch.isnan(g).all())
        body = cls[GUARD:-GUARD]
        assert bool(((body >= -1) & (body < c["K"])).all()) and not bool(torch.isnan(prb[GUARD:-GUARD]).any())
        outs.append((cls.cpu(), prb.cpu()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert outs[0][1].numpy().tobytes() == outs[1][1].numpy().tobytes()
    TR.check(TR.topk(c["ranked"], k), outs[0][0][GUARD:-GUARD].numpy(), outs[0][1][GUARD:-GUARD].numpy(), f"raw entry k={k}")


def test_a_class_without_a_query_never_appears():
    """query_idx leaves class 1 of K = 4 without a query: with k = 4 the last slot is -1 / 0 on every pixel, and class 1 is in no slot."""
    c = dict(HR.make_case("a", 6, False))
    c["query_idx"], c["K"] = np.array([0, 2, 3, 0, 2, 3], dtype=np.int32), 4
    canvas = HR.stitch(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
    cls, prb = run_topk(c, 4)
    assert (cls[3] == -1).all() and (prb[3] == 0).all()
    assert (cls[:3] != 1).all() and (cls[:3] >= 0).all()
    TR.check(TR.topk(TR.rank(canvas, c["query_idx"], 4, SCALE), 4), cls, prb, "class 1 without a query")
    cls2, prb2 = run_topk(c, 2)
    assert np.array_equal(cls2, cls[:2]) and prb2.tobytes() == prb[:2].tobytes()


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
def test_a_pixel_no_tile_covers(merge):
    """Columns 30 .. 39 of the 'hole' canvas are covered by no tile: every stitched value is 0 there, so the classes come in ascending
    index with equal probabilities 1 / Q.  Elsewhere the reference holds (no cap: the uncovered pixels are ties by design)."""
    wins, grid, up, pad, hw = HR.stitch_geometry("hole")
    Q = 9
    tl = (0.3 * np.random.default_rng(11).standard_normal((len(wins), Q) + tuple(grid))).astype(np.float32)
    qi, K = (np.array([2, 0, 1, 3, 2, 0, 1, 3, 0], dtype=np.int32), 4) if merge else (np.arange(Q, dtype=np.int32), Q)
    c = dict(tile_logits=tl, windows=wins, up_hw=up, pad_tl=pad, hw=hw, query_idx=qi, K=K)
    canvas = HR.stitch(tl, wins, up, pad, hw)
    bare = np.ones(hw, dtype=bool)
    for y1, y2, x1, x2 in np.asarray(wins).tolist():
        bare[max(y1, 0):y2, max(x1, 0):x2] = False
    assert bare[:, 30:40].all() and not bare.all()
    for k in (3, 4):
        cls, prb = run_topk(c, k)
        ref = TR.topk(TR.rank(canvas, qi, K, SCALE), k)
        assert not ref["counted"][:, bare].any() and ref["counted"][:, ~bare].any()
        TR.check(ref, cls, prb, f"hole K={K} k={k}", cap=False)
        assert (cls[:, bare] == np.arange(k)[:, None]).all()
        assert (prb[:, bare] == prb[0, 0, 35]).all() and abs(float(prb[0, 0, 35]) * Q - 1.0) < 1e-6
