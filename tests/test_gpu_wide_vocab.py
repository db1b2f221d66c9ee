"""Large vocabularies: sg_cosine_logits_wide (any Q, the text rows chunked through LDS), sg_postprocess_wide (Q > 64), and the drop-in
classes end to end on a class file of 130 queries in 70 classes."""
import numpy as np
import pytest
import torch

import head_reference as HR

pytestmark = pytest.mark.gpu


# ---- cosine logits ------------------------------------------------------------------------------------------------------------------
def cosine_ref(tok, cls, text, debias, lam):
    """float64 restatement of segmentor.py:309-336, 374-386."""
    tok, text = tok.astype(np.float64), text.astype(np.float64)
    cl = None
    if cls is not None:
        c = cls.astype(np.float64)
        c = c / np.linalg.norm(c, axis=-1, keepdims=True)
        cl = c @ text.T                                                     # [B,Q]
        if debias != 0:
            fn = tok / np.linalg.norm(tok, axis=-1, keepdims=True)
            cn = c / np.linalg.norm(c, axis=-1, keepdims=True)
            sim = (fn * cn[:, None]).sum(-1)
            tok = tok - c[:, None] * (sim[..., None] * debias)
    tok = tok / np.linalg.norm(tok, axis=-1, keepdims=True)
    lg = tok @ text.T
    if cl is not None and lam != 0:
        lg = lg + cl[:, None] * lam
    return lg.transpose(0, 2, 1)                                            # [B,Q,n]


def cosine_inputs(E, Q, n=77, B=2, seed=0):
    rng = np.random.default_rng(seed + E + Q)
    tok = rng.standard_normal((B, n, E)).astype(np.float32)
    cls = rng.standard_normal((B, E)).astype(np.float32)
    text = rng.standard_normal((Q, E)).astype(np.float32)
    text /= np.linalg.norm(text, axis=-1, keepdims=True)                    # unit-scale inputs: unit-norm text rows, O(1) features
    return tok, cls, text


@pytest.mark.parametrize("use_cls,debias,lam", [(False, 0.0, 0.0), (True, 0.2, 0.0), (True, 0.0, -0.3), (True, 0.2, -0.3)])
@pytest.mark.parametrize("E,Q", [(768, 53), (768, 300), (64, 700)])
def test_cosine_logits_beyond_the_lds_limit(E, Q, use_cls, debias, lam):
    from clip_decontamination_amd import ops
    assert (Q * E + E + Q) * 4 > ops.COSINE_LDS_BYTES                       # sg_cosine_logits refuses these
    tok, cls, text = cosine_inputs(E, Q)
    got = ops.cosine_logits(torch.from_numpy(tok).cuda(), torch.from_numpy(cls).cuda() if use_cls else None, torch.from_numpy(text).cuda(),
                            debias, lam)
    want = cosine_ref(tok, cls if use_cls else None, text, debias, lam)
    assert got.shape == (2, Q, 77)
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"E={E} Q={Q} cls={use_cls} debias={debias} lambda={lam}: max |err| {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("use_cls,debias,lam", [(False, 0.0, 0.0), (True, 0.0, -0.3), (True, 0.2, -0.3)])
@pytest.mark.parametrize("E,n", [(768, 77), (64, 16), (1024, 33)])
def test_wide_entry_is_bit_equal_where_both_accept(E, n, use_cls, debias, lam):
    """Q = 16, both entries called directly: the outputs must be equal bit for bit.  They are by construction: the wide entry runs
    cosine_logits_kernel for every shape that kernel takes (one chunk).  The chunked kernel on its own was measured one unit in the last
    place apart on 11 of 2464 outputs at E = 768, n = 77 with debias 0.2 (equal without the debias): the compiler fuses the multiply-adds
    of the debias sums in another order in the two kernels."""
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    Q, B = 16, 2
    tok, cls, text = cosine_inputs(E, Q, n=n)
    t, c, x = torch.from_numpy(tok).cuda(), torch.from_numpy(cls).cuda() if use_cls else None, torch.from_numpy(text).cuda()
    a = torch.full((B, Q, n), float("nan"), device="cuda")
    b = torch.full((B, Q, n), float("nan"), device="cuda")
    _lib.check(lib.sg_cosine_logits(ops.ptr(t), ops.ptr(c), ops.ptr(x), B, n, E, Q, debias, lam, ops.ptr(a), ops.stream_ptr()), "sg_cosine_logits")
    _lib.check(lib.sg_cosine_logits_wide(ops.ptr(t), ops.ptr(c), ops.ptr(x), B, n, E, Q, debias, lam, ops.ptr(b), ops.stream_ptr()),
               "sg_cosine_logits_wide")
    assert not bool(torch.isnan(b).any())
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_routing_keeps_the_existing_entry_below_the_limit():
    """ops.cosine_logits calls the wide entry only when sg_cosine_logits would refuse: E = 768 takes Q = 52 as before."""
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    tok, cls, text = cosine_inputs(768, 52, n=20)
    t, x = torch.from_numpy(tok).cuda(), torch.from_numpy(text).cuda()
    assert (52 * 768 + 768 + 52) * 4 <= ops.COSINE_LDS_BYTES < (53 * 768 + 768 + 53) * 4
    a = torch.empty(2, 52, 20, device="cuda")
    _lib.check(lib.sg_cosine_logits(ops.ptr(t), None, ops.ptr(x), 2, 20, 768, 52, 0.0, 0.0, ops.ptr(a), ops.stream_ptr()), "sg_cosine_logits")
    assert torch.equal(ops.cosine_logits(t, None, x), a)
    assert lib.sg_cosine_logits(ops.ptr(t), None, ops.ptr(x), 2, 20, 768, 53, 0.0, 0.0, ops.ptr(a), ops.stream_ptr()) != 0
    assert b"exceeds LDS" in lib.sg_last_error()


# ---- postprocess --------------------------------------------------------------------------------------------------------------------
def canvas_case(Q, merge, H=37, W=45):
    c = HR.make_case("a", Q, merge)
    rng = np.random.default_rng(Q)
    return (0.25 * rng.standard_normal((Q, H, W))).astype(np.float32), c["query_idx"], c["K"]


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
@pytest.mark.parametrize("Q", [65, 257])
def test_postprocess_beyond_64_queries(Q, merge):
    from clip_decontamination_amd import ops
    lg, qi, K = canvas_case(Q, merge)
    for thd in (0.0, 0.3):
        ref = HR.tail(lg, qi, K, 50.0, thd, 3)
        probs, labels = ops.postprocess(torch.from_numpy(lg).cuda(), torch.from_numpy(qi), K, 50.0, thd, 3)
        assert probs.shape == (K, 37, 45) and labels.shape == (1, 37, 45)
        err = np.abs(probs.cpu().numpy() - ref["probs"]).max()
        print(f"Q={Q} K={K} thd={thd}: max |prob err| {err:.3e}")
        assert err <= 1e-5
        HR.check_labels(ref, labels.cpu().numpy(), probs.max(0)[0].cpu().numpy(), thd, f"postprocess Q={Q} K={K} thd={thd}")
        _, only = ops.postprocess(torch.from_numpy(lg).cuda(), torch.from_numpy(qi), K, 50.0, thd, 3, want_probs=False)
        assert torch.equal(only, labels)


@pytest.mark.parametrize("merge", [False, True], ids=["K=Q", "K=Q/2"])
def test_wide_postprocess_against_the_existing_kernel_at_64(merge):
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    Q, H, W = 64, 37, 45
    lg, qi, K = canvas_case(Q, merge)
    x, q = torch.from_numpy(lg).cuda(), torch.from_numpy(qi).cuda()
    ref = HR.tail(lg, qi, K, 50.0, 0.3, 3)
    out = []
    for entry in (lib.sg_postprocess, lib.sg_postprocess_wide):
        probs = torch.full((K, H, W), float("nan"), device="cuda")
        labels = torch.full((H, W), -1, dtype=torch.int64, device="cuda")
        _lib.check(entry(ops.ptr(x), ops.ptr(q), Q, K, H, W, 50.0, 0.3, 3, ops.ptr(probs), ops.ptr(labels), ops.stream_ptr()), "postprocess")
        out.append((probs.cpu().numpy(), labels.cpu().numpy()))
    err = np.abs(out[0][0] - out[1][0]).max()
    print(f"Q=64 K={K}: wide against the existing kernel, max |prob diff| {err:.3e}")
    assert err <= 1e-6
    ok = HR.counted(ref, 0.3)                                                # off ties
    assert 1.0 - ok.mean() <= HR.CAP and np.array_equal(out[0][1][ok], out[1][1][ok])


def test_one_class_for_every_query():
    """postprocess_kernel's any_other rule: a class that owns every query starts at -inf, any other class at 0."""
    from clip_decontamination_amd import ops
    lg, _, _ = canvas_case(70, False)
    qi = np.full(70, 1, dtype=np.int32)
    ref = HR.tail(lg, qi, 2, 50.0, 0.0, 0)
    probs, labels = ops.postprocess(torch.from_numpy(lg).cuda(), torch.from_numpy(qi), 2, 50.0, 0.0, 0)
    assert np.abs(probs.cpu().numpy() - ref["probs"]).max() <= 1e-5 and bool((probs[0] == 0).all())
    assert np.array_equal(labels.cpu().numpy()[0], ref["labels"])


# ---- end to end: 130 queries in 70 classes on the tiny tower ------------------------------------------------------------------------
def class_file(tmp_path, n_queries, n_classes):
    """One class per line, synonyms separated by commas: the first n_queries - n_classes classes get two names."""
    lines, q = [], 0
    for c in range(n_classes):
        k = 2 if c < n_queries - n_classes else 1
        lines.append(",".join(f"thing{q + i}" for i in range(k)))
        q += k
    assert q == n_queries
    path = tmp_path / f"cls_{n_queries}.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def build(name_path, **kw):
    import segmentor
    return segmentor.SegmentorEx(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path=name_path, device=torch.device("cuda:0"),
                                 precision="f32", synthetic_ok=True, slide_crop=32, slide_stride=16, prob_thd=0.02, bg_idx=5, **kw)


def images():
    rng = np.random.default_rng(11)
    return [torch.from_numpy(rng.standard_normal((1, 3, h, w)).astype(np.float32)).cuda() for h, w in ((72, 88), (48, 64))]


def off_ties(seg, x):
    """The labels of the canvas route (forward_slide + ops.postprocess) and the pixels they are decided on beyond f32 rounding.  With
    130 near-flat probabilities the absolute gap G of tests/head_reference.py would call every pixel a tie, so the rule is applied to
    the RELATIVE gap here: the two routes see the same f32 tile logits and differ by a few roundings of the scaled logit (about 5e-5 on
    the exponent, i.e. 5e-5 relative on a probability); a pixel counts when its top-two class probabilities, and its confidence and the
    threshold, differ by more than G = 1e-3 of the confidence -- twenty times that."""
    from clip_decontamination_amd import ops
    H, W = x.shape[-2:]
    canvas = seg.forward_slide(x, [dict(ori_shape=(H, W))], seg.slide_stride, seg.slide_crop)[0]
    _, lab = ops.postprocess(canvas, seg.query_idx, seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx, want_probs=False)
    ref = HR.tail(canvas.cpu().numpy(), seg.query_idx.cpu().numpy(), seg.num_classes, seg.logit_scale, seg.prob_thd, seg.bg_idx)
    ok = (ref["gap"] >= HR.G * ref["conf"]) & (np.abs(ref["conf"] - seg.prob_thd) >= HR.G * ref["conf"])
    print(f"{H}x{W} Q={seg.num_queries}: decided pixels {100 * ok.mean():.2f} %, background {100 * (ref['conf'] < seg.prob_thd).mean():.2f} %, "
          f"median conf {np.median(ref['conf']):.4f}")
    return lab.cpu().numpy()[0], ok


def test_drop_in_with_130_queries_in_70_classes(tmp_path):
    seg = build(class_file(tmp_path, 130, 70), label_head="fused")
    assert seg.num_queries == 130 and seg.num_classes == 70
    x, y = images()
    want = [off_ties(seg, im) for im in (x, y)]
    for lab, ok in want:
        assert ok.mean() >= 1.0 - HR.CAP
    one = seg.predict(x, None)
    assert one.shape == (1, 72, 88) and np.array_equal(one.cpu().numpy()[0][want[0][1]], want[0][0][want[0][1]])
    many = seg.predict_many([x, y])
    for got, (lab, ok) in zip(many, want):
        assert np.array_equal(got.cpu().numpy()[0][ok], lab[ok])
    assert torch.equal(many[0], one)
    auto = build(class_file(tmp_path, 130, 70))                               # "auto" takes the fused head beyond 64 queries
    assert torch.equal(auto.predict(x, None), one)
    gts = [torch.from_numpy(lab.astype(np.uint8)) for lab, _ in want]
    res, metric = seg.evaluate([x, y], gts)
    print("evaluate against the canvas route's labels: aAcc", res["aAcc"])
    assert res["aAcc"] >= 1.0 - HR.CAP                                         # the canvas route's labels as ground truth: equal off ties

    class Sample:
        def __init__(self, meta):
            self.metainfo, self.data = meta, {}

        def set_data(self, d):
            self.data.update(d)

    ds = seg.predict_many([x, y], [Sample(dict(ori_shape=(72, 88))), Sample(dict(ori_shape=(40, 50)))])   # probabilities: the canvas + wide post-process
    assert ds[0].data["seg_logits"].data.shape == (70, 72, 88) and ds[1].data["pred_sem_seg"].data.shape == (1, 40, 50)
    assert np.array_equal(ds[0].data["pred_sem_seg"].data.cpu().numpy()[0][want[0][1]], want[0][0][want[0][1]])


def test_label_head_modes_agree_byte_for_byte_at_9_queries(tmp_path):
    path = class_file(tmp_path, 9, 6)
    canvas, auto = build(path, label_head="canvas"), build(path, label_head="auto")
    x, y = images()
    a, b = canvas.predict(x, None), auto.predict(x, None)
    assert torch.equal(a, b)
    lab, ok = off_ties(canvas, x)
    assert torch.equal(a.cpu(), torch.from_numpy(lab)[None])                   # the canvas route itself, bit for bit
    for p, q in zip(canvas.predict_many([x, y]), auto.predict_many([x, y])):
        assert torch.equal(p, q)
    fused = build(path, label_head="fused").predict(x, None)
    assert np.array_equal(fused.cpu().numpy()[0][ok], lab[ok])
    with pytest.raises(ValueError, match="label_head"):
        build(path, label_head="both")
