"""sg_label_head_resized / sg_topk_head_resized and their multi-image forms (stitch -> count division -> bilinear resize to another
ori_shape -> the label / top-k tails, no canvas) against the float64 reference of tests/head_resized_reference.py, by the existing
acceptance rules (head_reference.check_labels, topk_reference.check) and per element within head_reference.tail_bound; the staged form
against the direct one byte for byte; plane 0 against the label head; the canvas route; identity size against the unresized heads;
multi == single; guard bands and repeatability; tiny outputs, more than 64 candidates, uncovered pixels.

Measured on the MI355X: no label or class mismatch on a counted pixel or slot in any case; worst err / bound of a counted slot probability
0.282, worst conf err / tail_bound 0.099; at most 0.414 % of a case's pixels uncounted ("b", Q = 65, 29 x 50, threshold 0.3); staged ==
direct on every upscale and identity case; DESIGN.md section 5 'Heads at another ori_shape'."""
import numpy as np
import pytest
import torch

import head_reference as HR
import head_resized_reference as RR
import topk_reference as TR

pytestmark = pytest.mark.gpu

SCALE = RR.SCALE
GUARD = 64
_below_thd = {}


def _args(c):
    return (torch.from_numpy(c["tile_logits"]).cuda(), torch.from_numpy(np.asarray(c["windows"], dtype=np.int32)), c["up_hw"], c["pad_tl"],
            c["hw"])


def run_label(c, out, thd, form="auto"):
    from clip_decontamination_amd import ops
    labels, conf = ops.label_head_resized(*_args(c), out, torch.from_numpy(c["query_idx"]), c["K"], SCALE, thd, RR.BG, want_conf=True,
                                          form=form)
    assert labels.shape == (1,) + tuple(out) and conf.shape == tuple(out) and labels.dtype == torch.int64 and conf.dtype == torch.float32
    return labels.cpu().numpy()[0], conf.cpu().numpy()


def run_topk(c, out, k, form="auto"):
    from clip_decontamination_amd import ops
    cls, prb = ops.topk_head_resized(*_args(c), out, torch.from_numpy(c["query_idx"]), c["K"], SCALE, k, form=form)
    assert cls.shape == prb.shape == (k,) + tuple(out) and cls.dtype == torch.int32 and prb.dtype == torch.float32
    return cls.cpu().numpy(), prb.cpu().numpy()


def check_slots_within_the_bound(ref, bound, cls, prb, what):
    """Every slot probability within the largest class bound of its pixel (the j-th largest of K values moves by at most the largest
    move of any of them), and a counted slot within its own class's bound."""
    HR.within(prb, ref["probs"], np.broadcast_to(bound["conf"], prb.shape).copy(), what + " slots")
    ok = ref["counted"] & (ref["classes"] >= 0)
    own = np.take_along_axis(bound["probs"], np.maximum(ref["classes"], 0), 0)
    HR.within(prb[ok], ref["probs"][ok], own[ok], what + " counted slots")


@pytest.mark.parametrize("geom,Q,merge,out", RR.CASES, ids=[RR.case_id(*c) for c in RR.CASES])
def test_both_heads_match_the_f64_reference(geom, Q, merge, out):
    """Labels and conf by check_labels at both thresholds, the slots by topk_reference.check for every k; conf and the slot probabilities
    per element within tail_bound; plane 0 of the top-k head is the label head byte for byte; on an upscale the staged form is the
    direct form byte for byte."""
    c = RR.resized(geom, Q, merge, out)
    what = RR.case_id(geom, Q, merge, out)
    bound = HR.tail_bound(c["resized"], RR.canvas_bound(c), c["query_idx"], c["K"], SCALE)
    staged = RR.is_upscale(c["hw"], out)
    conf0 = None
    for thd in RR.THDS:
        ref = RR.tail(c, thd)
        labels, conf = run_label(c, out, thd, "direct")
        HR.check_labels(ref, labels, conf, thd, f"{what} thd={thd}")
        r = HR.within(conf, ref["conf"], bound["conf"], f"{what} conf")
        print(f"{what} thd={thd}: conf err / bound {r:.3f}")
        if thd > 0:
            _below_thd[geom] = _below_thd.get(geom, False) or bool((labels[conf < thd] == RR.BG).all() and (conf < thd).any())
        else:
            conf0, labels0 = conf, labels
        if staged:
            ls, cs = run_label(c, out, thd, "staged")
            assert np.array_equal(ls, labels) and cs.tobytes() == conf.tobytes(), f"{what}: staged != direct"
        la, ca = run_label(c, out, thd, "auto")
        assert np.array_equal(la, labels) and ca.tobytes() == conf.tobytes(), f"{what}: auto != direct"
    for k in TR.ks_of(c["K"]):
        ref = TR.topk(c["ranked"], k)
        cls, prb = run_topk(c, out, k, "direct")
        assert ((cls >= -1) & (cls < c["K"])).all() and np.isfinite(prb).all() and (prb >= 0).all() and (prb <= 1).all()
        TR.check(ref, cls, prb, f"{what} k={k}")
        check_slots_within_the_bound(ref, bound, cls, prb, f"{what} k={k}")
        assert np.array_equal(cls[0], labels0) and prb[0].tobytes() == conf0.tobytes(), f"{what} k={k}: plane 0 is not the label head"
        if staged:
            cs, ps = run_topk(c, out, k, "staged")
            assert np.array_equal(cs, cls) and ps.tobytes() == prb.tobytes(), f"{what} k={k}: staged != direct"


@pytest.mark.parametrize("geom", ["a", "b"])
def test_the_threshold_branch_is_taken_in_each_geometry(geom):
    """Per geometry, not per case ('a' with Q = 8 / 9 at 33 x 41 has no pixel under 0.3): some case wrote bg_idx under the threshold."""
    if geom not in _below_thd:                                            # run alone
        c = RR.resized(geom, 65, False, RR.OUT_SIZES[geom][0])
        labels, conf = run_label(c, c["out"], 0.3)
        _below_thd[geom] = bool((labels[conf < 0.3] == RR.BG).all() and (conf < 0.3).any())
    assert _below_thd[geom]


def test_a_staged_form_that_does_not_fit_is_refused_with_the_reason():
    c = RR.resized("a", 9, False, (33, 41))
    with pytest.raises(ValueError, match=r"staged form does not fit \(70, 90\) -> \(33, 41\): a block's footprint of 11 x 143"):
        run_label(c, (33, 41), 0.0, "staged")
    from clip_decontamination_amd import _lib, ops
    tl, win = _args(c)[:2]
    win, qi = win.cuda(), torch.from_numpy(c["query_idx"]).cuda()
    out = torch.full((33 * 41,), -7, dtype=torch.int64, device="cuda")
    T, Q, gh, gw = tl.shape
    rc = _lib.load().sg_label_head_resized(ops.ptr(tl), ops.ptr(win), T, Q, gh, gw, *c["up_hw"], *c["pad_tl"], 70, 90, 33, 41, ops.ptr(qi), Q,
                                           SCALE, 0.0, 0, ops.ptr(out), None, ops.RESIZED_FORMS["staged"], ops.stream_ptr())
    assert rc != 0 and b"staged form does not fit" in _lib.load().sg_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all())


@pytest.mark.parametrize("Q,merge", [(9, True), (9, False), (65, False)])
def test_more_than_64_candidates(Q, merge):
    """'dense' (crop 32 at stride 2) downscaled to 13 x 23: one block whose footprint is the whole canvas, more candidates than the list
    holds, so every window is tested.  Run with cap=False rules: 299 pixels are too few for a 1 % cap to mean anything."""
    c = dict(TR.case("dense", Q, merge))
    out = (13, 23)
    assert len(c["windows"]) > 64
    rs = RR.reference_of(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"], out)
    ref = HR.tail(rs, c["query_idx"], c["K"], SCALE, 0.0, RR.BG)
    labels, conf = run_label(c, out, 0.0)
    ok = HR.counted(ref, 0.0)
    assert ok.mean() > 0.9 and np.array_equal(labels[ok], ref["labels"][ok]) and np.abs(conf - ref["conf"])[ok].max() <= HR.G
    for k in TR.ks_of(c["K"]):
        cls, prb = run_topk(c, out, k)
        TR.check(TR.topk(TR.rank(rs, c["query_idx"], c["K"], SCALE), k), cls, prb, f"dense Q={Q} k={k}", cap=False)


@pytest.mark.parametrize("out", [(3, 5), (1, 1)])
@pytest.mark.parametrize("geom", ["a", "b"])
def test_tiny_outputs(geom, out):
    c = TR.case(geom, 9, True)
    rs = RR.reference_of(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"], out)
    ref = HR.tail(rs, c["query_idx"], c["K"], SCALE, 0.0, RR.BG)
    labels, conf = run_label(c, out, 0.0)
    ok = HR.counted(ref, 0.0)
    assert np.array_equal(labels[ok], ref["labels"][ok]) and (np.abs(conf - ref["conf"])[ok] <= HR.G).all()
    cls, prb = run_topk(c, out, 3)
    TR.check(TR.topk(TR.rank(rs, c["query_idx"], c["K"], SCALE), 3), cls, prb, f"{geom} {out}", cap=False)


@pytest.mark.parametrize("out,form", [((11, 150), "direct"), ((11, 150), "staged"), ((4, 20), "direct")])
def test_a_canvas_with_uncovered_pixels(out, form):
    """Columns 30 .. 39 of the 'hole' canvas are covered by no tile and count as 0 in the blend, divided by nothing: an output pixel whose
    four taps are all uncovered has equal probabilities 1 / Q and the classes in ascending order."""
    wins, grid, up, pad, hw = HR.stitch_geometry("hole")
    Q = 9
    tl = (0.3 * np.random.default_rng(11).standard_normal((len(wins), Q) + tuple(grid))).astype(np.float32)
    c = dict(tile_logits=tl, windows=wins, up_hw=up, pad_tl=pad, hw=hw, query_idx=np.arange(Q, dtype=np.int32), K=Q)
    rs = RR.reference_of(tl, wins, up, pad, hw, out)
    ref = TR.topk(TR.rank(rs, c["query_idx"], Q, SCALE), 3)
    cls, prb = run_topk(c, out, 3, form)
    assert np.isfinite(prb).all()
    TR.check(ref, cls, prb, f"hole {out} {form}", cap=False)
    bare = (rs == 0).all(0)
    assert bare.any() and not bare.all()
    assert (cls[:, bare] == np.arange(3)[:, None]).all() and np.allclose(prb[:, bare], 1.0 / Q, rtol=1e-6)
    labels, conf = run_label(c, out, 0.0, form)
    assert np.array_equal(labels, cls[0]) and conf.tobytes() == prb[0].tobytes()


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
@pytest.mark.parametrize("Q", [q for q in HR.QS if q <= 64])
@pytest.mark.parametrize("geom,out", [("a", (161, 207)), ("b", (29, 50))])
def test_against_the_canvas_route(geom, out, Q, merge):
    """ops.stitch -> ops.resize_bilinear -> ops.postprocess (-> ops.topk_from_probs): the same class on every counted pixel and slot."""
    from clip_decontamination_amd import ops
    c = RR.resized(geom, Q, merge, out)
    qi = torch.from_numpy(c["query_idx"])
    canvas = ops.resize_bilinear(ops.stitch(*_args(c)), out)
    probs, lab = ops.postprocess(canvas, qi, c["K"], SCALE, 0.0, RR.BG)
    ref = RR.tail(c, 0.0)
    labels, conf = run_label(c, out, 0.0)
    ok = HR.counted(ref, 0.0)
    assert np.array_equal(labels[ok], lab.cpu().numpy()[0][ok])
    assert (np.abs(conf - probs.max(0).values.cpu().numpy())[ok] <= HR.G).all()
    for k in TR.ks_of(c["K"]):
        r = TR.topk(c["ranked"], k)
        cc, pc = ops.topk_from_probs(probs, qi, k)
        cls, prb = run_topk(c, out, k)
        assert np.array_equal(cls[r["counted"]], cc.cpu().numpy()[r["counted"]])
        assert (np.abs(prb.astype(np.float64) - pc.cpu().numpy())[r["counted"]] <= 2 * (TR.REL * r["probs"] + TR.ABS)[r["counted"]]).all()


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
@pytest.mark.parametrize("Q", [9, 65, 257])
def test_identity_size_against_the_unresized_heads(Q, merge):
    """out = the canvas size: identity taps through the new kernel (every product rounded), against ops.label_head / ops.topk_head
    (contracted multiply-adds): the same class on every counted pixel and slot."""
    from clip_decontamination_amd import ops
    c = RR.resized("b", Q, merge, (66, 93))
    qi = torch.from_numpy(c["query_idx"])
    ref = RR.tail(c, 0.0)
    ok = HR.counted(ref, 0.0)
    l0, c0 = ops.label_head(*_args(c), qi, c["K"], SCALE, 0.0, RR.BG, want_conf=True)
    labels, conf = run_label(c, (66, 93), 0.0)
    assert np.array_equal(labels[ok], l0.cpu().numpy()[0][ok]) and (np.abs(conf - c0.cpu().numpy())[ok] <= HR.G).all()
    k = min(5, c["K"])
    r = TR.topk(c["ranked"], k)
    ck, _ = ops.topk_head(*_args(c), qi, c["K"], SCALE, k)
    cls, _ = run_topk(c, (66, 93), k)
    assert np.array_equal(cls[r["counted"]], ck.cpu().numpy()[r["counted"]])


MULTI_OUT = [(91, 160), (32, 32), (23, 40)]                               # an upscale, an unresized image, a downscale


@pytest.mark.parametrize("form", ["auto", "direct", "staged"])
@pytest.mark.parametrize("Q,merge", [(9, True), (65, False)])
def test_multi_equals_single_per_image(Q, merge, form):
    """Three images of 40 x 70, 32 x 32 and 50 x 33 to 91 x 160, 32 x 32 (unresized) and 23 x 40 in one launch: byte-equal to the single
    entries per image.  form='staged' is refused for the list (the downscale does not fit) and runs on the two images that fit."""
    from clip_decontamination_amd import ops
    m = HR.make_multi_case(Q)
    qi = torch.from_numpy(HR.make_case("a", Q, merge)["query_idx"])
    K = int(qi.max()) + 1 if merge else Q
    tl = torch.from_numpy(m["tile_logits"]).cuda()
    idx = [0, 1, 2]
    if form == "staged":
        with pytest.raises(ValueError, match=r"staged form does not fit \(50, 33\) -> \(23, 40\)"):
            ops.label_head_resized_multi(tl, m["windows"], m["tile_image"], m["up_hw"], m["pad_tl"], m["image_hw"], m["image_tiles"], MULTI_OUT,
                                         qi, K, SCALE, 0.3, 0, form=form)
        idx = [0, 1]
    n_t = sum(m["image_tiles"][n][1] for n in idx)
    hw, tiles, outs = [m["image_hw"][n] for n in idx], [m["image_tiles"][n] for n in idx], [MULTI_OUT[n] for n in idx]
    args = (tl[:n_t], m["windows"][:n_t], m["tile_image"][:n_t], m["up_hw"], m["pad_tl"], hw, tiles, outs, qi, K, SCALE)
    lab, flat, conf = ops.label_head_resized_multi(*args, 0.3, 0, want_conf=True, form=form)
    k = min(3, K)
    cls, prb = ops.topk_head_resized_multi(*args, k, form=form)
    assert flat.numel() == sum(h * w for h, w in outs)
    for n, ((h, w), (first, count), out) in enumerate(zip(hw, tiles, outs)):
        wins = torch.from_numpy(m["windows"][first:first + count])
        l1, c1 = ops.label_head_resized(tl[first:first + count], wins, m["up_hw"], m["pad_tl"], (h, w), out, qi, K, SCALE, 0.3, 0,
                                        want_conf=True, form="direct")
        assert lab[n].shape == (1,) + out and torch.equal(lab[n], l1) and conf[n].cpu().numpy().tobytes() == c1.cpu().numpy().tobytes(), n
        k1, p1 = ops.topk_head_resized(tl[first:first + count], wins, m["up_hw"], m["pad_tl"], (h, w), out, qi, K, SCALE, k, form="direct")
        assert cls[n].shape == (k,) + out and torch.equal(cls[n], k1) and prb[n].cpu().numpy().tobytes() == p1.cpu().numpy().tobytes(), n
        rs = RR.reference_of(m["tile_logits"][first:first + count], m["windows"][first:first + count], m["up_hw"], m["pad_tl"], (h, w), out)
        TR.check(TR.topk(TR.rank(rs, qi.numpy(), K, SCALE), k), k1.cpu().numpy(), p1.cpu().numpy(), f"multi image {n} Q={Q}", cap=False)


@pytest.mark.parametrize("form", ["direct", "staged"])
def test_outputs_stay_inside_their_guard_bands_and_repeat(form):
    """Raw entries on buffers with sentinel / NaN bands on both sides of every output; two calls give the same bytes."""
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    c = RR.resized("a", 65, True, (161, 207))
    OH, OW = c["out"]
    H, W = c["hw"]
    T, Q, gh, gw = c["tile_logits"].shape
    tl, win = _args(c)[:2]
    win, qi = win.cuda(), torch.from_numpy(c["query_idx"]).cuda()
    flags, k, n = ops.RESIZED_FORMS[form], 3, OH * OW
    runs = []
    for rep in range(2):
        lab = torch.full((n + 2 * GUARD,), -12345, dtype=torch.int64, device="cuda")
        conf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        cls = torch.full((k * n + 2 * GUARD,), -12345, dtype=torch.int32, device="cuda")
        prb = torch.full((k * n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.sg_label_head_resized(ops.ptr(tl), ops.ptr(win), T, Q, gh, gw, *c["up_hw"], *c["pad_tl"], H, W, OH, OW, ops.ptr(qi),
                                             c["K"], SCALE, 0.3, 0, ops.ptr(lab[GUARD:]), ops.ptr(conf[GUARD:]), flags, ops.stream_ptr()),
                   "sg_label_head_resized")
        _lib.check(lib.sg_topk_head_resized(ops.ptr(tl), ops.ptr(win), T, Q, gh, gw, *c["up_hw"], *c["pad_tl"], H, W, OH, OW, ops.ptr(qi),
                                            c["K"], SCALE, k, ops.ptr(cls[GUARD:]), ops.ptr(prb[GUARD:]), flags, ops.stream_ptr()),
                   "sg_topk_head_resized")
        torch.cuda.synchronize()
        for buf in (lab, cls):
            assert bool((buf[:GUARD] == -12345).all()) and bool((buf[-GUARD:] == -12345).all())
            assert bool(((buf[GUARD:-GUARD] >= -1) & (buf[GUARD:-GUARD] < c["K"])).all())
        for buf in (conf, prb):
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()) and not bool(torch.isnan(buf[GUARD:-GUARD]).any())
        runs.append([b.cpu().numpy().tobytes() for b in (lab, conf, cls, prb)])
    assert runs[0] == runs[1]
    HR.check_labels(RR.tail(c, 0.3), np.frombuffer(runs[0][0], dtype=np.int64)[GUARD:-GUARD], np.frombuffer(runs[0][1], dtype=np.float32)[GUARD:-GUARD],
                    0.3, f"raw entry {form}")
