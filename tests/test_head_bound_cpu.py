"""tests/head_reference.py on the CPU: the references equal torch's own float64 operations, f32 emulations of each head kernel's arithmetic
order stay inside the bounds on the cases the GPU module runs (and counted_tight leaves at most CAP of a case uncounted), and every listed
mutation of an emulation falls outside a bound or fails a label / tie check on at least one case.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_reference as HR

SCALE = 50.0


# ---- the references are torch's float64 operations -------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,size", HR.RESIZE_SHAPES)
def test_resize_reference_is_interpolate(hw, size):
    x = torch.randn(3, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(hw[0] * 10 + size[1]))
    want = F.interpolate(x[None], size=size, mode="bilinear", align_corners=False)[0].numpy()
    got, bound = HR.resize_reference(x.numpy(), size)
    assert np.abs(got - want).max() < 1e-13 and bound.shape == got.shape and (bound > 0).all()
    if hw == size:
        assert np.array_equal(got, x.numpy())


@pytest.mark.parametrize("par", HR.COSINE_PARAMS)
@pytest.mark.parametrize("kind", ["scales", "offset", "cancel"])
def test_cosine_reference_is_the_segmentor_in_f64(par, kind):
    """A literal float64 transcription of segmentor.py:309-336, 374-379 with F.normalize for the last step."""
    tok, cls, text = (torch.from_numpy(a).double() for a in HR.make_cosine_case(3, 5, 68, 5, kind, seed=2))
    debias, lam = (HR.f32v(par[0]), HR.f32v(par[1])) if par else (0.0, 0.0)
    feats = tok
    cls_logits = None
    if par:
        c = cls / cls.norm(dim=-1, keepdim=True)
        cls_logits = c @ text.T
        if debias != 0:
            fn = feats / feats.norm(dim=-1, keepdim=True)
            cn = c / c.norm(dim=-1, keepdim=True)
            sim = (fn * cn.unsqueeze(1)).sum(-1)
            feats = feats - c.unsqueeze(1) * (sim.unsqueeze(-1) * debias)
    logits = F.normalize(feats, dim=-1, eps=0.0) @ text.T
    if par and lam != 0:
        logits = logits + cls_logits.unsqueeze(1) * lam
    got, bound = HR.cosine_reference(tok.numpy(), cls.numpy() if par else None, text.numpy(), debias, lam)
    want = logits.permute(0, 2, 1).numpy()
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    two, _ = HR.cosine_two_plane_reference(tok.numpy(), cls.numpy() if par else None, text.numpy(), lam)
    if not par or debias == 0:
        assert np.abs(two - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_tail_bound_probabilities_are_softmax():
    c, qi, K = HR.make_tail_case(17, 255, "ident", "plain")
    ref = HR.tail(c, qi, K, SCALE, 0.0, 0)
    want = torch.softmax(torch.from_numpy(c).double() * SCALE, 0).numpy()
    assert np.abs(ref["probs"] - want).max() < 1e-14
    b = HR.tail_bound(c, 0.0, qi, K, SCALE)
    assert b["probs"].shape == want.shape and (b["probs"] > 0).all() and (b["probs"] < 1e-4).all()


# ---- cosine logits ---------------------------------------------------------------------------------------------------------------------------
def _cos(case, mut=None):
    E, n, B, Q, par, kind = case
    tok, cls, text = HR.make_cosine_case(B, n, E, Q, kind, seed=1)
    cls = cls if par else None
    debias, lam = par or (0.0, 0.0)
    ref, bound = HR.cosine_reference(tok, cls, text, debias, lam)
    return HR.cosine_emulate(tok, cls, text, debias, lam, mut), ref, bound


def _outside(got, ref, bound):
    with np.errstate(invalid="ignore"):
        return not bool((np.abs(got.astype(np.float64) - ref) <= bound).all())


def test_cosine_emulation_inside_the_bound():
    worst = 0.0
    for case in HR.cosine_cases():
        got, ref, bound = _cos(case)
        worst = max(worst, HR.within(got, ref, bound, f"cosine {case}"))
    print(f"cosine emulation, largest err / bound {worst:.3f}")


def test_cosine_zero_row_is_nan_and_the_rest_is_inside():
    tok, cls, text = HR.make_cosine_case(2, 5, 68, 5, "zero", seed=1)
    for par in HR.COSINE_PARAMS:
        c, (debias, lam) = (cls if par else None), (par or (0.0, 0.0))
        ref, bound = HR.cosine_reference(tok, c, text, debias, lam)
        got = HR.cosine_emulate(tok, c, text, debias, lam)
        assert np.isnan(ref[0, :, 0]).all() and np.isnan(got[0, :, 0]).all()
        keep = np.ones(ref.shape, dtype=bool)
        keep[0, :, 0] = False
        HR.within(got[keep], ref[keep], bound[keep], f"zero row {par}")


@pytest.mark.parametrize("mut", ["drop_last_float4", "cls_image0", "debias_raw_cls", "no_renorm", "lambda_sign", "cls_logit_unscaled"])
def test_cosine_mutations_fall_outside(mut):
    hits = [case for case in HR.cosine_cases() if _outside(*_cos(case, mut))]
    print(f"{mut}: outside the bound on {len(hits)} of {len(HR.cosine_cases())} cases")
    assert hits


@pytest.mark.parametrize("E", [32, 96])
def test_two_plane_emulation_inside_the_bound(E):
    rng = np.random.default_rng(E)
    for lo, hi in ((-6, 6), (-13, -13)):
        tok = (rng.standard_normal((2, 37, E)) * np.exp2(np.linspace(lo, hi, 37))[None, :, None]).astype(np.float32)
        tok[1, 3] = 0.0
        cls = rng.standard_normal((2, E)).astype(np.float32)
        text = rng.standard_normal((13, E))
        text = (text / np.linalg.norm(text, axis=-1, keepdims=True)).astype(np.float32)
        for lam in (0.0, -0.3):
            ref, bound = HR.cosine_two_plane_reference(tok, cls, text, lam)
            r = HR.within(HR.cosine_two_plane_emulate(tok, cls, text, lam), ref, bound, f"two-plane E {E} scales 2^{lo}..2^{hi}")
            print(f"two-plane E {E} scales 2^{lo}..2^{hi} lam {lam}: err / bound {r:.3f}, largest bound {bound.max():.3e}")


# ---- stitch / resize ---------------------------------------------------------------------------------------------------------------------------
def _stitch_args(c):
    return c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"]


def _stitch_cases():
    out = [(f"{n} Q {Q} {d}", HR.make_stitch_case(n, Q, d)) for n, Q, d in HR.STITCH_CASES]
    for n in ("a", "b"):
        out += [(f"{n} one-hot {i}", c) for i, c in enumerate(HR.one_hot_cases(n, 4))]
    return out


STITCH = _stitch_cases()
STITCH_REF = {}


def _stitch_ref(name, c):
    if name not in STITCH_REF:
        STITCH_REF[name] = (HR.stitch(*_stitch_args(c)), HR.stitch_bound(*_stitch_args(c)))
    return STITCH_REF[name]


def test_stitch_emulation_inside_the_bound():
    worst = {}
    for name, c in STITCH:
        ref, bound = _stitch_ref(name, c)
        worst[name] = HR.within(HR.stitch_emulate(*_stitch_args(c)), ref, bound, f"stitch {name}")
    print("stitch emulation, err / bound:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    ref, _ = _stitch_ref(*[(n, c) for n, c in STITCH if n.startswith("hole")][0])
    assert (ref[:, :, 30:40] == 0).all() and (ref[:, 0, 40:] == 0).all() and (ref[:, 4, :30] == 0).all()


@pytest.mark.parametrize("mut", ["swap_taps", "swap_pad", "align_corners", "no_count_div", "div_by_T"])
def test_stitch_mutations_fall_outside(mut):
    hits = [name for name, c in STITCH if _outside(HR.stitch_emulate(*_stitch_args(c), mut=mut), *_stitch_ref(name, c))]
    print(f"{mut}: outside the bound on {hits}")
    assert hits


@pytest.mark.parametrize("hw,size", HR.RESIZE_SHAPES)
def test_resize_emulation_inside_the_bound(hw, size):
    for C in HR.RESIZE_C:
        for off in (0.0, 100.0):
            src = (np.random.default_rng(C + hw[0]).standard_normal((C,) + hw) + off).astype(np.float32)
            ref, bound = HR.resize_reference(src, size)
            HR.within(HR.resize_emulate(src, size), ref, bound, f"resize {hw}->{size} C {C}")


# ---- the tails -------------------------------------------------------------------------------------------------------------------------------------
def _tail_run(c, qi, K, thd, form, mut=None, dcanvas=0.0, canvas64=None):
    """Emulation against the reference through check_tight -> (ratio, uncounted share, ratio over normal values); AssertionError when
    outside."""
    ref = HR.tail(c if canvas64 is None else canvas64, qi, K, SCALE, thd, K - 1)
    bound = HR.tail_bound(c if canvas64 is None else canvas64, dcanvas, qi, K, SCALE)
    got = HR.tail_emulate(c, qi, K, SCALE, thd, K - 1, form, mut)
    return HR.check_tight(ref, bound, thd, got["labels"], got["probs"], got["conf"], f"{form} Q {c.shape[0]} K {K} thd {thd}")


def _tail_all(mut=None):
    """Every tail case through the forms that take it; returns the failures."""
    fails = []
    for qs, forms in ((HR.PP_Q, ("two_pass", "online")), (HR.PPW_Q, ("wide", "online"))):
        for Q, HW, cl, data in HR.tail_cases(qs):
            c, qi, K = HR.make_tail_case(Q, HW, cl, data)
            for thd in (0.0, 0.3):
                for form in forms:
                    try:
                        _tail_run(c, qi, K, thd, form, mut)
                    except AssertionError as e:
                        fails.append((form, Q, HW, cl, data, thd, str(e)[:80]))
    return fails


def test_tail_emulations_inside_the_bound_and_under_the_cap():
    fails = _tail_all()
    assert not fails, fails[:5]


def _ties(mut=None):
    """Exact ties through the three forms -> the list of (form, Q, merged) whose label is not the lower class everywhere."""
    wrong = []
    for Q in (2, 9, 64, 65, 130):
        for merged in (False, True):
            if merged and Q < 3:
                continue
            c, qi, K, want = HR.tie_case(Q, merged)
            for form in (("two_pass",) if Q <= 64 else ()) + ("wide", "online"):
                got = HR.tail_emulate(c, qi, K, SCALE, 0.0, 0, form, mut)
                if not (got["labels"] == want).all():
                    wrong.append((form, Q, merged))
    return wrong


def test_ties_go_to_the_lower_class_in_the_reference_and_the_emulations():
    for Q in (2, 9, 130):
        for merged in (False, True):
            if merged and Q < 3:
                continue
            c, qi, K, want = HR.tie_case(Q, merged)
            assert (HR.tail(c, qi, K, SCALE, 0.0, 0)["labels"] == want).all()
    assert not _ties()


def _threshold_exact(mut=None):
    """conf == prob_thd exactly (one query: the softmax is 1; two identical planes: 0.5) keeps the class: `<`, not `<=`."""
    wrong = []
    for Q, thd in ((1, 1.0), (2, 0.5)):
        c = np.full((Q, 1, 5), 0.25, dtype=np.float32)
        for form in ("two_pass", "wide", "online"):
            got = HR.tail_emulate(c, np.arange(Q), Q, SCALE, thd, 7, form, mut)
            if not (got["labels"] == 0).all():
                wrong.append((form, Q))
    return wrong


def test_threshold_is_strict():
    assert (HR.tail(np.full((1, 1, 5), 0.25), [0], 1, SCALE, 1.0, 7)["labels"] == 0).all()
    assert not _threshold_exact()


@pytest.mark.parametrize("mut", ["no_zeros_in_max", "le_threshold", "tie_highest_class", "tie_lowest_query", "online_no_rescale"])
def test_tail_mutations_are_caught(mut):
    if mut in ("tie_highest_class", "tie_lowest_query"):
        hits = _ties(mut)
    elif mut == "le_threshold":
        hits = _threshold_exact(mut)
    else:
        hits = _tail_all(mut)
    print(f"{mut}: caught on {len(hits)} cases, first {hits[:3]}")
    assert hits


# ---- the fused heads: the tail fed by the stitch, bound fed by stitch_bound ------------------------------------------------------------------
@pytest.mark.parametrize("geom,Q,sign,merge", HR.HEAD_CASES)
def test_head_emulations_inside_the_bound_and_under_the_cap(geom, Q, sign, merge):
    c = HR.make_head_case(geom, Q, sign, merge)
    canvas64, dcanvas = HR.stitch(*_stitch_args(c)), HR.stitch_bound(*_stitch_args(c))
    canvas32 = HR.stitch_emulate(*_stitch_args(c))
    HR.within(canvas32, canvas64, dcanvas, "stitch")
    for form in (("two_pass",) if Q <= 64 else ("wide",)) + ("online",):
        ratio, frac, _ = _tail_run(canvas32, c["query_idx"], c["K"], 0.3, form, dcanvas=dcanvas, canvas64=canvas64)
        print(f"{geom} Q {Q} sign {sign} K {c['K']} {form}: err / bound {ratio:.3f}, uncounted {100 * frac:.3f} %")
    if sign > 0 and Q > 8:                                                 # the maximum moves in every chunk: a missing rescale shows
        with pytest.raises(AssertionError):
            _tail_run(canvas32, c["query_idx"], c["K"], 0.3, "online", mut="online_no_rescale", dcanvas=dcanvas, canvas64=canvas64)


# ---- render_maps -------------------------------------------------------------------------------------------------------------------------------------
def test_render_reference_is_the_segmentor_colouring():
    labels, probs = HR.make_render_case(257, 6)
    pal = HR.make_palette(6)
    mask, heat = HR.render_reference(labels, probs, pal)
    t = torch.from_numpy(probs)
    conf = torch.nan_to_num(t.max(0)[0], nan=0.0).clamp(0, 1)
    g = (conf * 255).to(torch.uint8).numpy()
    assert np.array_equal(heat[..., 0], g) and (heat[..., 1] == 0).all() and np.array_equal(heat[..., 2], 255 - g)
    assert np.array_equal(mask, pal[np.clip(labels, 0, 5)])
    assert np.array_equal(heat[:250:2, 0], np.arange(0, 250, 2))            # k / 255 in f32 times 255 truncates to k for these k
    assert heat[-1, 0] == 0 and heat[-2, 0] == 255                          # NaN -> 0, +inf -> 1


@pytest.mark.parametrize("mut", ["heat_rounded", "label_unclipped"])
def test_render_mutations_change_bytes(mut):
    labels, probs = HR.make_render_case(257, 6)
    pal = HR.make_palette(6)
    a, b = HR.render_reference(labels, probs, pal), HR.render_reference(labels, probs, pal, mut)
    assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
