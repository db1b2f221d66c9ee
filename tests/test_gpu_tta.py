"""sg_tta_head (the class probabilities of V views merged at the output size in one launch, no canvas) and the canvas-route pair
sg_tta_accumulate + sg_tta_finish against the float64 reference of tests/tta_reference.py: labels, conf and the mean planes element by
element by that module's acceptance rule; one unflipped view against sg_label_head_resized byte for byte in both forms; [a, a] against
[a]; repeats; the canvas route at Q = 64 and Q = 130; sg_tta_accumulate's mirror against torch.flip; refused descriptors; a flipped
view over an output whose width is no multiple of 64.

Measured on the MI355X: worst err / bound of a mean plane 0.318, of conf 0.077; no label mismatch on a pixel that check_labels counts,
in any case; every label the exact first arg-max of the returned planes.  The float64 reference itself has up to 10.3 % of a multi-view
case's pixels within G = 1e-3 of a tie (tests/tta_reference.py, 'Acceptance'), so check_labels' 1 % cap is asserted wherever the
reference meets it -- every single-view case (at most 0.14 %) and the few multi-view cases below 1 % -- and printed elsewhere."""
import ctypes

import numpy as np
import pytest
import torch

import head_resized_reference as RR
import topk_reference as TR
import tta_reference as TT

pytestmark = pytest.mark.gpu

SCALE = TT.SCALE


def _dev_views(vs, Q, merge):
    return [(torch.from_numpy(tl).cuda(), torch.from_numpy(win), up, pad, hw, f) for tl, win, up, pad, hw, f in TT.device_views(vs, Q, merge)]


def run_fused(vs, Q, merge, out, thd, form="auto", want_probs=True):
    from clip_decontamination_amd import ops
    qi, K = TT.class_map(Q, merge)
    res = ops.tta_head(_dev_views(vs, Q, merge), out, torch.from_numpy(qi), K, SCALE, thd, TT.BG, want_conf=True, want_probs=want_probs,
                       form=form)
    labels, conf = res[0], res[1]
    assert labels.shape == (1,) + tuple(out) and labels.dtype == torch.int64 and conf.shape == tuple(out) and conf.dtype == torch.float32
    if not want_probs:
        return labels.cpu().numpy()[0], conf.cpu().numpy(), None
    assert res[2].shape == (K,) + tuple(out) and res[2].dtype == torch.float32
    return labels.cpu().numpy()[0], conf.cpu().numpy(), res[2].cpu().numpy()


def run_canvas(vs, Q, merge, out, thd):
    """The canvas route per view: stitch -> resize -> the existing probability tail -> accumulate; then finish."""
    from clip_decontamination_amd import ops
    qi, K = TT.class_map(Q, merge)
    views = _dev_views(vs, Q, merge)
    acc = None
    for tl, win, up, pad, hw, f in views:
        canvas = ops.resize_bilinear(ops.stitch(tl, win, up, pad, hw), out)
        probs, _ = ops.postprocess(canvas, torch.from_numpy(qi), K, SCALE, 0.0, TT.BG, want_probs=True)
        acc = ops.tta_accumulate(probs, f, acc)
    labels, conf, probs = ops.tta_finish(acc, len(views), thd, TT.BG, want_conf=True, want_probs=True)
    assert probs.data_ptr() == acc.data_ptr()
    return labels.cpu().numpy()[0], conf.cpu().numpy(), probs.cpu().numpy()


@pytest.mark.parametrize("vs,Q,merge,out", TT.CASES, ids=[TT.case_id(*c) for c in TT.CASES])
def test_the_fused_head_matches_the_f64_reference(vs, Q, merge, out):
    """Every view set with every Q and both class maps, at both thresholds; labels and conf do not depend on whether the planes are asked."""
    what = TT.case_id(vs, Q, merge, out)
    for thd in TT.THDS:
        ref, bound = TT.reference(vs, Q, merge, out, thd)
        labels, conf, probs = run_fused(vs, Q, merge, out, thd)
        assert ((labels >= 0) & (labels < probs.shape[0])).all() and np.isfinite(probs).all()
        TT.check(ref, bound, labels, conf, probs, thd, f"{what} thd={thd}")
        l2, c2, _ = run_fused(vs, Q, merge, out, thd, want_probs=False)
        assert np.array_equal(l2, labels) and c2.tobytes() == conf.tobytes(), f"{what}: labels alone differ from labels with planes"
        if thd > 0:
            assert (labels[conf < thd] == TT.BG).all()


@pytest.mark.parametrize("Q,merge", [(5, False), (16, True), (17, False), (64, True)])
@pytest.mark.parametrize("out", TT.OUTS, ids=lambda o: f"{o[0]}x{o[1]}")
def test_one_unflipped_view_is_the_resized_label_head_byte_for_byte(Q, merge, out):
    from clip_decontamination_amd import ops
    c = TR.case("a", Q, merge)
    forms = ["direct", "auto"] + (["staged"] if RR.is_upscale(c["hw"], out) else [])
    for thd in TT.THDS:
        for form in forms:
            l0, c0 = ops.label_head_resized(torch.from_numpy(c["tile_logits"]).cuda(), torch.from_numpy(np.asarray(c["windows"], dtype=np.int32)),
                                            c["up_hw"], c["pad_tl"], c["hw"], out, torch.from_numpy(c["query_idx"]), c["K"], SCALE, thd, TT.BG,
                                            want_conf=True, form=form)
            labels, conf, _ = run_fused("a", Q, merge, out, thd, form)
            assert conf.tobytes() == c0.cpu().numpy().tobytes(), f"Q={Q} {out} {form}: conf differs"
            assert np.array_equal(labels, l0.cpu().numpy()[0]), f"Q={Q} {out} {form}: labels differ"


@pytest.mark.parametrize("Q,merge,out", [(5, True, TT.OUTS[0]), (17, False, TT.OUTS[1]), (64, False, TT.OUTS[2])])
def test_a_view_twice_is_the_view_and_repeats_are_identical(Q, merge, out):
    """(P + P) / 2 is exact, so [a, a] gives [a]'s bytes; two calls give the same bytes."""
    one = run_fused((TT.A,), Q, merge, out, 0.3)
    two = run_fused((TT.A, TT.A), Q, merge, out, 0.3)
    again = run_fused((TT.A, TT.A), Q, merge, out, 0.3)
    for a, b, c in zip(one, two, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    e1, e2 = run_fused("eight", Q, merge, out, 0.0), run_fused("eight", Q, merge, out, 0.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(e1, e2))


@pytest.mark.parametrize("vs", ["a+bf+af", "eight"])
@pytest.mark.parametrize("Q,merge", [(64, True), (130, False)])
def test_the_canvas_route_matches_the_f64_reference(vs, Q, merge):
    out = TT.OUTS[0] if Q == 64 else TT.OUTS[1]
    for thd in TT.THDS:
        ref, bound = TT.reference(vs, Q, merge, out, thd)
        TT.check(ref, bound, *run_canvas(vs, Q, merge, out, thd), thd, f"canvas {TT.case_id(vs, Q, merge, out)} thd={thd}")


def test_accumulate_mirrors_like_torch_flip():
    from clip_decontamination_amd import ops
    g = torch.Generator().manual_seed(3)
    for K, H, W in ((3, 5, 7), (2, 9, 130), (1, 1, 1)):
        a, b = torch.rand(K, H, W, generator=g).cuda(), torch.rand(K, H, W, generator=g).cuda()
        acc = ops.tta_accumulate(a, True)
        assert torch.equal(acc, torch.flip(a, dims=[2]))
        assert ops.tta_accumulate(b, True, acc) is acc and torch.equal(acc, torch.flip(a, dims=[2]) + torch.flip(b, dims=[2]))
        acc2 = ops.tta_accumulate(b, False, ops.tta_accumulate(a, False))
        assert torch.equal(acc2, a + b)
        labels, conf, probs = ops.tta_finish(acc2.clone(), 2, 0.0, 0, want_conf=True, want_probs=True)
        assert torch.equal(probs, (a + b) / 2) and torch.equal(conf, probs.max(0).values) and torch.equal(labels[0], probs.argmax(0))


@pytest.mark.parametrize("out", [(37, 130), (9, 64), (6, 65)], ids=lambda o: f"{o[0]}x{o[1]}")
def test_a_flipped_view_over_a_partial_last_block(out):
    """A width that is no multiple of 64 (and one that is, and one column more): the mirrored footprint of the partial block."""
    vs = (TT.AF, TT.B)
    for form in ("direct", "auto"):
        ref, bound = TT.reference(vs, 17, True, out, 0.0)
        TT.check(ref, bound, *run_fused(vs, 17, True, out, 0.0, form), 0.0, f"af+b {out} {form}")


def test_refused_descriptors_leave_the_outputs_untouched():
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    Q, out = 17, (33, 41)
    views = _dev_views("a+bf+af", Q, False)
    logits = torch.cat([v[0].reshape(-1) for v in views])
    windows = torch.cat([v[1].reshape(-1, 4) for v in views]).cuda()
    qi = torch.arange(Q, dtype=torch.int32, device="cuda")
    table, first = [], 0
    for tl, _, up, pad, hw, f in views:
        T, _, gh, gw = tl.shape
        table.append([T, first, gh, gw, up[0], up[1], pad[0], pad[1], hw[0], hw[1], int(f)])
        first += T
    n = out[0] * out[1]
    lab = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    conf = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    prb = torch.full((Q * n,), float("nan"), dtype=torch.float32, device="cuda")

    def call(table=table, V=3, q=Q, K=Q, bg=0, oh=out[0], ow=out[1], tiles=first, elems=int(logits.numel())):
        desc = (ctypes.c_int32 * (len(table) * ops.TTA_VIEW_FIELDS))(*[x for row in table for x in row])
        return lib.sg_tta_head(ops.ptr(logits), elems, ops.ptr(windows), tiles, desc, V, q, oh, ow, ops.ptr(qi), K, SCALE, 0.0, bg, ops.ptr(lab),
                               ops.ptr(conf), ops.ptr(prb), 0, ops.stream_ptr())

    def edited(v, field, value):
        t = [list(r) for r in table]
        t[v][field] = value
        return t

    bad = [(dict(V=0), "V=0 views"), (dict(V=9, table=table * 3), "V=9 views"), (dict(q=65, K=65), "Q=65 must lie in"), (dict(K=18), "K=18 must lie in"),
           (dict(K=0), "K=0 must lie in"), (dict(bg=-1), "bg_idx=-1 outside"), (dict(bg=Q), f"bg_idx={Q} outside"), (dict(oh=0), "bad output size"),
           (dict(ow=-3), "bad output size"), (dict(table=edited(1, 2, 0)), "view 1 has a bad shape"), (dict(table=edited(2, 9, -5)), "view 2 has a bad shape"),
           (dict(table=edited(0, 10, 2)), "flip=2"), (dict(table=edited(1, 1, 0)), "view 1 starts at tile 0"), (dict(tiles=first + 1), "the views hold"),
           (dict(elems=int(logits.numel()) - 1), "the views hold")]
    for kw, word in bad:
        rc = call(**kw)
        err = lib.sg_last_error().decode()
        assert rc != 0 and "sg_tta_head:" in err and word in err, (kw, rc, err)
    acc = torch.full((Q * n,), 0.5, dtype=torch.float32, device="cuda")
    assert lib.sg_tta_finish(ops.ptr(acc), 9, Q, out[0], out[1], 0.0, 0, ops.ptr(lab), ops.ptr(conf), ops.ptr(prb), ops.stream_ptr()) != 0
    assert "V=9 views" in lib.sg_last_error().decode()
    assert lib.sg_tta_finish(ops.ptr(acc), 2, Q, out[0], out[1], 0.0, Q, ops.ptr(lab), ops.ptr(conf), ops.ptr(prb), ops.stream_ptr()) != 0
    assert lib.sg_tta_accumulate(ops.ptr(acc), Q, out[0], out[1], 2, ops.ptr(prb), 0, ops.stream_ptr()) != 0
    assert lib.sg_tta_accumulate(ops.ptr(acc), Q, out[0], out[1], 0, ops.ptr(acc), 0, ops.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((lab == -7).all()) and bool(torch.isnan(conf).all()) and bool(torch.isnan(prb).all())
    assert call() == 0                                                    # and the good call runs
    torch.cuda.synchronize()
    assert bool(((lab >= 0) & (lab < Q)).all()) and not bool(torch.isnan(conf).any()) and not bool(torch.isnan(prb).any())
    with pytest.raises(ValueError, match=r"9 views, must lie in \[1, 8\]"):
        ops.tta_head(views * 3, out, qi, Q, SCALE, 0.0, 0)
