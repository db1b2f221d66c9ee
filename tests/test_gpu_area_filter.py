"""The area_thd kernels on the MI355X (the definition: include/segearth_hip.h; the reference, the cases and the acceptance rule:
tests/area_reference.py).
  class_area[_multi]        against np.bincount: integers, so equal, and two repeats byte-identical
  area_keep                 against Python doubles, the equality row, total = 0 and counts beyond 2^24 included
  area_filter_probs[_multi] byte equality with the numpy statement of steps 4-5 on the device's own first-pass probabilities and labels
  area_relabel[_multi]      byte equality with ops.label_head on a query_idx whose dropped queries are -1 (the merge cases); the
                            acceptance rule against the float64 reference (all cases, K == Q included); multi == single; a case in
                            which nothing is dropped; repeats."""
import numpy as np
import pytest
import torch

import area_reference as AR
import head_reference as HR

pytestmark = pytest.mark.gpu

SCALE, THD = AR.LOGIT_SCALE, AR.PROB_THD
MULTI_HW = [(5, 7), (64, 4), (130, 67)]


def label_maps(n, K, rng):
    """A uniform, a blocky and a random map of n labels in [0,K), and the random one with -1 and K sprinkled in (never counted)."""
    blocky = np.repeat(rng.integers(0, K, n // 37 + 1), 37)[:n]
    noisy = rng.integers(0, K, n)
    out = rng.integers(-1, K + 1, n)
    return {"uniform": np.full(n, K - 1), "blocky": blocky, "random": noisy, "out-of-range": out}


def bincount(labels, K):
    labels = np.asarray(labels).reshape(-1)
    return np.bincount(labels[(labels >= 0) & (labels < K)], minlength=K).astype(np.int64)


@pytest.mark.parametrize("K", [1, 3, 19, 4096])
def test_class_area_against_bincount(K):
    from clip_decontamination_amd import ops
    assert ops.AREA_MAX_K == 4096
    rng = np.random.default_rng(K)
    for n in (1, 255, 257, 70001):
        for kind, lab in label_maps(n, K, rng).items():
            dev = torch.from_numpy(lab.astype(np.int64)).cuda()
            a, b = ops.class_area(dev, K), ops.class_area(dev, K)
            assert a.dtype == torch.int64 and a.shape == (K,)
            assert np.array_equal(a.cpu().numpy(), bincount(lab, K)), (K, n, kind)
            assert torch.equal(a, b), (K, n, kind)
    acc = ops.class_area(dev, K, counts=a)                                         # counts are ADDED: the caller zeroes them
    assert acc is a and np.array_equal(a.cpu().numpy(), 2 * bincount(lab, K))


def test_class_area_at_a_label_buffer_that_is_not_16_byte_aligned():
    from clip_decontamination_amd import ops
    lab = np.random.default_rng(1).integers(0, 7, 9001)
    dev = torch.from_numpy(lab.astype(np.int64)).cuda()
    for off in (1, 2, 3):
        assert np.array_equal(ops.class_area(dev[off:], 7).cpu().numpy(), bincount(lab[off:], 7))


@pytest.mark.parametrize("K", [1, 19, 4096])
def test_class_area_multi(K):
    from clip_decontamination_amd import ops
    rng = np.random.default_rng(100 + K)
    for kind in ("uniform", "blocky", "random", "out-of-range"):
        labs = [label_maps(h * w, K, rng)[kind] for h, w in MULTI_HW]
        flat = torch.from_numpy(np.concatenate(labs).astype(np.int64)).cuda()
        a = ops.class_area_multi(flat, [h * w for h, w in MULTI_HW], K)
        b = ops.class_area_multi(flat, [h * w for h, w in MULTI_HW], K)
        assert a.shape == (3, K) and torch.equal(a, b)
        for n, lab in enumerate(labs):
            assert np.array_equal(a[n].cpu().numpy(), bincount(lab, K)), (K, kind, n)
            assert torch.equal(a[n], ops.class_area(torch.from_numpy(lab.astype(np.int64)).cuda(), K))


def test_refusals():
    from clip_decontamination_amd import ops
    lab = torch.zeros(10, dtype=torch.int64, device="cuda")
    for K in (0, 4097):
        with pytest.raises(RuntimeError, match="SG_AREA_MAX_K"):
            ops.class_area(lab, K)
        with pytest.raises(RuntimeError, match="SG_AREA_MAX_K"):
            ops.class_area_multi(lab, [10], K)
    with pytest.raises(RuntimeError, match="SG_AREA_MAX_K"):
        ops.area_keep(torch.zeros(4097, dtype=torch.int64, device="cuda"), 0, 0.1)
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    for bg in (-1, 3):
        with pytest.raises(ValueError, match="bg_idx"):
            ops.area_keep(counts, bg, 0.1)
        with pytest.raises(ValueError, match="bg_idx"):
            ops.area_filter(torch.rand(3, 4, 4, device="cuda"), 0.1, 0.3, bg)
    with pytest.raises(ValueError, match="area_thd"):
        ops.area_keep(counts, 0, -0.1)
    with pytest.raises(TypeError, match="int64"):
        ops.class_area(lab.int(), 3)


def test_area_keep_against_python_doubles():
    from clip_decontamination_amd import ops
    rng = np.random.default_rng(3)
    rows = [([10, 1, 3], 0, 0.25),                                                 # equality: 1 > 0.25 * 4 is false, 3 > 1 is true
            ([0, 0, 7, 0], 2, 0.0), ([0, 0, 7, 0], 2, 0.5),                        # total = 0: the background alone
            ([5, 0, 5], 1, 0.0),                                                   # area_thd = 0 drops only what never wins
            ([3, 16777217, 16777217], 0, 0.5), ([3, 16777218, 16777216], 0, 0.5),  # beyond 2^24: exact in double, merged in f32
            ([7, 2 ** 40, 2 ** 40 + 1, 1], 3, 0.5), ([4, 9, 1], 0, 1.5)]
    for _ in range(40):
        K = int(rng.integers(1, 40))
        rows.append((rng.integers(0, 10 ** int(rng.integers(1, 12)), K).tolist(), int(rng.integers(0, K)), float(rng.choice([0.0, 0.01, 0.1, 0.5, 1.0]))))
    for area, bg, thd in rows:
        got = ops.area_keep(torch.tensor(area, dtype=torch.int64, device="cuda"), bg, thd)
        assert got.dtype == torch.int32 and got.cpu().numpy().astype(bool).tolist() == AR.keep_of(area, bg, thd).tolist(), (area, bg, thd)
    assert ops.area_keep(torch.tensor([10, 1, 3], device="cuda"), 0, 0.25).tolist() == [1, 0, 1]
    # [N,K]: one launch, every row on its own
    counts = rng.integers(0, 1000, (300, 19))
    got = ops.area_keep(torch.from_numpy(counts).cuda(), 3, 0.07).cpu().numpy().astype(bool)
    assert np.array_equal(got, np.stack([AR.keep_of(r, 3, 0.07) for r in counts]))


def dev_case(c):
    return dict(tl=torch.tensor(c["tile_logits"], device="cuda"), win=torch.tensor(c["windows"]), qi=torch.tensor(c["query_idx"]))       # copies: the case is read-only


def first_pass_probs(c, d, fused):
    """The device's first pass with probabilities: prob_thd = 0, so the labels are the plain arg-max."""
    from clip_decontamination_amd import ops
    if fused:
        return ops.prob_head(d["tl"], d["win"], c["up_hw"], c["pad_tl"], c["hw"], d["qi"], c["K"], SCALE, 0.0, c["bg_idx"])
    canvas = ops.stitch(d["tl"], d["win"], c["up_hw"], c["pad_tl"], c["hw"])
    return ops.postprocess(canvas, d["qi"], c["K"], SCALE, 0.0, c["bg_idx"])


@pytest.mark.parametrize("case", AR.CASES, ids=AR.case_id)
def test_area_filter_probs_is_the_numpy_statement_on_the_first_pass(case):
    from clip_decontamination_amd import ops
    c = AR.make_case(*case)
    AR.check_preconditions(c, AR.case_id(case))
    d = dev_case(c)
    K, bg, thd = c["K"], c["bg_idx"], c["area_thd"]
    for fused in (False, True):
        probs, labels = first_pass_probs(c, d, fused)
        p0, l0 = probs.cpu().numpy().copy(), labels.cpu().numpy().copy()
        assert np.array_equal(l0[0], p0.argmax(0)), "the first pass is not the plain arg-max"
        counts = ops.class_area(labels, K)
        keep = ops.area_keep(counts, bg, thd)
        assert np.array_equal(counts.cpu().numpy(), bincount(l0, K))
        assert keep.cpu().numpy().astype(bool).tolist() == c["ref"]["keep"].tolist(), "a keep bit differs from the float64 reference"
        want = AR.area_filter(p0, thd, THD, bg, l0=l0)
        out = ops.area_filter_probs(probs, labels, keep, THD, bg)
        assert out is labels and labels.shape == (1,) + tuple(c["hw"])
        assert probs.cpu().numpy().tobytes() == want["probs"].tobytes()
        assert labels.cpu().numpy().tobytes() == want["labels"].tobytes()
        AR.check_labels(c, labels.cpu().numpy(), f"{AR.case_id(case)} fused={fused}")
        # the stand-alone op for a caller who holds probabilities: its own arg-max, the same bytes
        fp, fl, fk = ops.area_filter(torch.from_numpy(p0).cuda(), thd, THD, bg)
        assert torch.equal(fp, probs) and torch.equal(fl, labels) and torch.equal(fk, keep)


def test_area_filter_probs_multi_is_the_single_form_per_image():
    from clip_decontamination_amd import ops
    rng = np.random.default_rng(11)
    K, bg = 19, 3
    ps = []
    for h, w in MULTI_HW:
        z = rng.standard_normal((K, h, w)) * 2.0 + np.where(np.arange(K) < 7, 0.0, -2.5)[:, None, None]
        ps.append((np.exp(z - z.max(0)) / np.exp(z - z.max(0)).sum(0)).astype(np.float32))
    ps[1][:, :8] = 0.0                                                             # pixels where every probability is exactly 0
    singles = [ops.area_filter(torch.from_numpy(p).cuda(), 0.08, THD, bg) for p in ps]
    probs = torch.cat([torch.from_numpy(p).cuda().reshape(-1) for p in ps])
    flat = torch.cat([torch.from_numpy(p.argmax(0)).cuda().reshape(-1) for p in ps])
    counts = ops.class_area_multi(flat, [h * w for h, w in MULTI_HW], K)
    keep = ops.area_keep(counts, bg, 0.08)
    assert 0 < int(keep.sum()) < keep.numel()
    ops.area_filter_probs_multi(probs, flat, keep, MULTI_HW, THD, bg)
    a = b = 0
    for n, ((h, w), p) in enumerate(zip(MULTI_HW, ps)):
        sp, sl, sk = singles[n]
        want = AR.area_filter(p, 0.08, THD, bg)
        assert torch.equal(keep[n], sk) and sk.cpu().numpy().astype(bool).tolist() == want["keep"].tolist()
        assert torch.equal(probs[K * a:K * (a + h * w)].view(K, h, w), sp) and sp.cpu().numpy().tobytes() == want["probs"].tobytes()
        assert torch.equal(flat[a:a + h * w].view(1, h, w), sl) and sl.cpu().numpy()[0].tobytes() == want["labels"].tobytes()
        a += h * w


def remapped(c):
    """query_idx with the queries of the reference's dropped classes set to -1."""
    qi = c["query_idx"].copy()
    qi[~c["ref"]["keep"][qi]] = -1
    return torch.from_numpy(qi)


def relabel(c, d, keep=None):
    from clip_decontamination_amd import ops
    K, bg = c["K"], c["bg_idx"]
    labels, conf = ops.label_head(d["tl"], d["win"], c["up_hw"], c["pad_tl"], c["hw"], d["qi"], K, SCALE, 0.0, bg, want_conf=True)
    first = labels.clone()
    if keep is None:
        keep = ops.area_keep(ops.class_area(labels, K), bg, c["area_thd"])
    out = ops.area_relabel(d["tl"], d["win"], c["up_hw"], c["pad_tl"], c["hw"], d["qi"], K, SCALE, THD, bg, keep, conf, labels)
    assert out is labels
    return labels, first, conf, keep


@pytest.mark.parametrize("case", AR.CASES, ids=AR.case_id)
def test_area_relabel(case):
    from clip_decontamination_amd import ops
    c = AR.make_case(*case)
    AR.check_preconditions(c, AR.case_id(case))
    d = dev_case(c)
    K, bg = c["K"], c["bg_idx"]
    labels, first, conf, keep = relabel(c, d)
    assert keep.cpu().numpy().astype(bool).tolist() == c["ref"]["keep"].tolist(), "a keep bit differs from the float64 reference"
    assert labels.dtype == torch.int64 and labels.shape == (1,) + tuple(c["hw"])
    AR.check_labels(c, labels.cpu().numpy(), AR.case_id(case))
    again = relabel(c, d)[0]
    assert torch.equal(labels, again), "repeats differ"
    dropped = ~keep.bool()[first[0]]
    assert bool(dropped.any()) and bool((~dropped).any())
    if K != len(c["query_idx"]):
        # the general K != Q path of sg_label_head on the remapped query_idx: byte for byte, on every pixel
        want = ops.label_head(d["tl"], d["win"], c["up_hw"], c["pad_tl"], c["hw"], remapped(c), K, SCALE, THD, bg)
        assert torch.equal(labels, want)


@pytest.mark.parametrize("case", [c for c in AR.CASES if c[0] == "a" and c[3] == 3], ids=AR.case_id)
def test_area_relabel_with_nothing_dropped(case):
    """Every class kept: no block gathers, and the output is conf0 < prob_thd ? bg_idx : l0 -- sg_label_head with the threshold."""
    from clip_decontamination_amd import ops
    c = AR.make_case(*case)
    d = dev_case(c)
    K, bg = c["K"], c["bg_idx"]
    labels, first, conf, _ = relabel(c, d, keep=torch.ones(K, dtype=torch.int32, device="cuda"))
    thd32 = torch.tensor(THD, dtype=torch.float32, device="cuda")
    assert torch.equal(labels[0], torch.where(conf < thd32, torch.full_like(first[0], bg), first[0]))
    assert torch.equal(labels, ops.label_head(d["tl"], d["win"], c["up_hw"], c["pad_tl"], c["hw"], d["qi"], K, SCALE, THD, bg))
    if K >= 8:
        assert bool((labels != first).any()), "the threshold moved no pixel: the case would show nothing"


@pytest.mark.parametrize("Q,merge", [(8, False), (9, True), (65, True)])
def test_area_relabel_multi_is_the_single_form_per_image(Q, merge):
    from clip_decontamination_amd import ops
    m = HR.make_multi_case(Q)
    base = HR.make_case("a", Q, merge)
    K, qi, bg = base["K"], base["query_idx"], min(3, base["K"] - 1)
    tl_np = (m["tile_logits"] + AR.class_bias(K, bg)[qi][None, :, None, None].astype(np.float32)).astype(np.float32)
    tl, qi_t = torch.from_numpy(tl_np).cuda(), torch.from_numpy(qi)
    args = (tl, m["windows"], m["tile_image"], m["up_hw"], m["pad_tl"], m["image_hw"], m["image_tiles"], qi_t, K, SCALE)
    lab, flat, conf = ops.label_head_multi(*args, 0.0, bg, want_conf=True, flat_conf=True)
    pixels = [h * w for h, w in m["image_hw"]]
    counts = ops.class_area_multi(flat, pixels, K)
    thds = [AR.widest_gap_thd(r, bg) for r in counts.cpu().numpy()]
    keep = torch.stack([ops.area_keep(counts[n], bg, thds[n]) for n in range(len(pixels))])       # its own threshold per image
    out = ops.area_relabel_multi(*args, THD, bg, keep, conf, flat)
    assert out is flat
    wins = torch.from_numpy(m["windows"])
    a = 0
    for n, ((f, cnt), hw) in enumerate(zip(m["image_tiles"], m["image_hw"])):
        l1, c1 = ops.label_head(tl[f:f + cnt], wins[f:f + cnt], m["up_hw"], m["pad_tl"], hw, qi_t, K, SCALE, 0.0, bg, want_conf=True)
        assert torch.equal(c1.reshape(-1), conf[a:a + pixels[n]])
        k1 = ops.area_keep(ops.class_area(l1, K), bg, thds[n])
        assert torch.equal(k1, keep[n]) and 1 <= int(k1.sum()) < K
        ops.area_relabel(tl[f:f + cnt], wins[f:f + cnt], m["up_hw"], m["pad_tl"], hw, qi_t, K, SCALE, THD, bg, k1, c1, l1)
        assert torch.equal(l1, lab[n]) and torch.equal(l1.reshape(-1), flat[a:a + pixels[n]]), n
        a += pixels[n]
