"""Every kernel of csrc/head.hip against the float64 references of tests/head_reference.py, element by element, each through its C entry
(one kernel per entry).  Every output sits between two 64 KiB guard bands of a sentinel, checked after each call.  Logits, canvases and
probabilities are held to bounds built from operand magnitudes and each kernel's summation shape; labels must equal the reference's on
every pixel whose decision lies beyond those bounds (counted_tight; at most CAP of a case may be uncounted); exact ties must go to the lower
class; render_maps is byte-exact.  tests/test_head_bound_cpu.py shows on the same generators that f32 emulations of the kernels stay inside
the bounds and that the listed mutations do not.

The two-plane cosine logits carry an absolute representation floor of 2^-25 per feature element, so their bound grows as 1 / (row scale).
At row scales 2^-6 .. 2^6 with unit-norm text the bound's largest element is 3.6e-6 (E = 32) / 6.6e-6 (E = 96): the worst-case charge for
the f32 accumulation alone, E u sum |terms|, is 3.7e-6 at E = 96, so the bound cannot itself stay under the 2e-6 the project claims there.
The test therefore holds every element to the bound AND the largest error to 2e-6 directly."""
import ctypes as C
import os
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_reference as HR                                             # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 1 << 16
SENT = {torch.float32: -12345.5, torch.int64: -7777, torch.uint8: 0xA5}
SCALE = 50.0
WORST = defaultdict(float)                    # (op, case) -> largest err / bound


@pytest.fixture(scope="module")
def lib():
    from clip_decontamination_amd import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


KEEP = []                                     # device copies of a call's inputs, alive until ok() has synchronised


def PD(a, dtype=None):
    """Device pointer of a copy of the numpy array / tensor a; the copy lives until the call it feeds has finished (ok())."""
    t = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a)
    KEEP.append((t.to(dtype) if dtype is not None else t).contiguous().to(DEV))
    return P(KEEP[-1])


class Guarded:
    """`numel` elements of `dtype` on the device, sentinel-filled, between two guard bands; `.view` is the payload (1-D)."""

    def __init__(self, numel, dtype=torch.float32):
        self.sent = torch.tensor(SENT[dtype], dtype=dtype)
        self.g = GUARD // self.sent.element_size()
        self.big = torch.full((2 * self.g + numel,), SENT[dtype], dtype=dtype, device=DEV)
        self.view = self.big[self.g:self.g + numel]

    def finish(self):
        """Guard bands intact -> the payload on the CPU (numpy)."""
        torch.cuda.synchronize()
        s = self.sent.to(DEV)
        assert bool((self.big[:self.g] == s).all()) and bool((self.big[self.g + self.view.numel():] == s).all()), "guard band overwritten"
        return self.view.cpu().numpy()

    def untouched(self):
        return bool((torch.as_tensor(self.finish()) == self.sent).all())


def record(op, case, ratio):
    WORST[(op, case)] = max(WORST[(op, case)], ratio)


def ok(lib, rc):
    torch.cuda.synchronize()
    KEEP.clear()
    assert rc == 0, lib.sg_last_error()


# ---- cosine logits ---------------------------------------------------------------------------------------------------------------------------
def run_cosine(lib, entry, tok, cls, text, debias, lam):
    B, n, E = tok.shape
    Q = text.shape[0]
    out = Guarded(B * Q * n)
    fn = getattr(lib, entry)
    ok(lib, fn(PD(tok), PD(cls) if cls is not None else None, PD(text), B, n, E, Q, debias, lam, P(out.view), stream()))
    return out.finish().reshape(B, Q, n)


@pytest.mark.parametrize("E,n,B,Q,par,kind", HR.cosine_cases())
def test_cosine_logits_vs_f64(lib, E, n, B, Q, par, kind):
    """All four NV instantiations (E / 64 <= 8, 12, 16, 32) on both sides of each switch, E % 64 != 0, n around the 32-token block."""
    tok, cls, text = HR.make_cosine_case(B, n, E, Q, kind, seed=1)
    cls = cls if par else None
    debias, lam = par or (0.0, 0.0)
    got = run_cosine(lib, "sg_cosine_logits", tok, cls, text, debias, lam)
    ref, bound = HR.cosine_reference(tok, cls, text, debias, lam)
    record("cosine_logits " + kind, f"E {E} n {n} B {B} Q {Q} {par}", HR.within(got, ref, bound, f"cosine E {E} n {n} {par} {kind}"))


@pytest.mark.parametrize("par", HR.COSINE_PARAMS)
def test_cosine_logits_zero_row_is_nan(lib, par):
    """x / |x| of an all-zero token row is NaN, as in the reference; every other token stays inside its bound."""
    tok, cls, text = HR.make_cosine_case(2, 5, 68, 5, "zero", seed=1)
    cls = cls if par else None
    debias, lam = par or (0.0, 0.0)
    got = run_cosine(lib, "sg_cosine_logits", tok, cls, text, debias, lam)
    ref, bound = HR.cosine_reference(tok, cls, text, debias, lam)
    assert np.isnan(got[0, :, 0]).all() and np.isnan(ref[0, :, 0]).all()
    keep = np.ones(ref.shape, dtype=bool)
    keep[0, :, 0] = False
    record("cosine_logits zero row", f"{par}", HR.within(got[keep], ref[keep], bound[keep], f"zero row {par}"))


WIDE = [(E, Q, (15, 16, 17)[(i + j) % 3], par) for i, (E, Q) in enumerate(((2048, 19), (2048, 37), (64, 630))) for j, par in enumerate(HR.COSINE_PARAMS)]
WIDE += [(768, 54, 17, (0.2, 0.0)), (768, 54, 15, (1.0, 0.5)), (1024, 41, 16, (0.0, -0.3)), (1024, 41, 17, None)]   # the NV = 12 / 16 instantiations


@pytest.mark.parametrize("E,Q,n,par", WIDE)
def test_cosine_logits_wide_vs_f64(lib, E, Q, n, par):
    """R < Q: the text rows pass through LDS in chunks (18 + 1, 18 + 18 + 1, 629 + 1; 52 + 2 and 38 + 3 for the two middle
    instantiations); n around the 16-token block."""
    assert (Q * E + E + Q) * 4 > 160 * 1024
    kind = "cancel" if par == (1.0, 0.5) else ("scales", "offset")[n % 2]
    tok, cls, text = HR.make_cosine_case(2, n, E, Q, kind, seed=2)
    cls = cls if par else None
    debias, lam = par or (0.0, 0.0)
    got = run_cosine(lib, "sg_cosine_logits_wide", tok, cls, text, debias, lam)
    ref, bound = HR.cosine_reference(tok, cls, text, debias, lam)
    record("cosine_logits_wide " + kind, f"E {E} Q {Q} n {n} {par}", HR.within(got, ref, bound, f"wide E {E} Q {Q} n {n} {par}"))


def run_two_plane(lib, tok, cls, text, lam):
    B, n, E = tok.shape
    Q = text.shape[0]
    out = Guarded(B * Q * n)
    ok(lib, lib.sg_cosine_logits_two_plane(PD(tok), PD(cls) if cls is not None else None, PD(text), B, n, E, Q, lam, P(out.view), stream()))
    return out.finish().reshape(B, Q, n)


def two_plane_case(n, E, Q, lo, hi, seed):
    rng = np.random.default_rng(seed)
    tok = (rng.standard_normal((2, n, E)) * np.exp2(np.linspace(lo, hi, n))[None, :, None]).astype(np.float32)
    cls = rng.standard_normal((2, E)).astype(np.float32)
    text = rng.standard_normal((Q, E))
    return tok, cls, (text / np.linalg.norm(text, axis=-1, keepdims=True)).astype(np.float32)


TWO_PLANE = [(4096, 32, 1, 0.0), (4097, 96, 13, -0.3), (4099, 32, 16, 0.5), (4096 + 37, 96, 16, 0.0), (4097, 32, 13, -0.3), (4096, 96, 1, 0.5)]


@pytest.mark.parametrize("n,E,Q,lam", TWO_PLANE)
def test_cosine_two_plane_vs_f64(lib, n, E, Q, lam):
    """Row scales 2^-6 .. 2^6, ragged n, one all-zero row (it must give lam * cls_logit): inside the bound, and within the 2e-6 the project
    claims for this range (module docstring: the bound itself is larger)."""
    tok, cls, text = two_plane_case(n, E, Q, -6, 6, seed=n + E + Q)
    tok[1, 5] = 0.0
    got = run_two_plane(lib, tok, cls if lam else None, text, lam)
    ref, bound = HR.cosine_two_plane_reference(tok, cls if lam else None, text, lam)
    err = float(np.abs(got - ref).max())
    print(f"two-plane n {n} E {E} Q {Q} lam {lam}: max |err| {err:.3e}, largest bound {bound.max():.3e}, zero-row bound {bound[1, :, 5].max():.3e}")
    record("cosine_two_plane 2^-6..2^6", f"n {n} E {E} Q {Q} lam {lam}", HR.within(got, ref, bound, f"two-plane n {n} E {E} Q {Q}"))
    assert err <= 2e-6
    assert bound[1, :, 5].max() < 1e-6                                      # the zero row is held to lam * cls_logit, not to a vacuous bound


def test_cosine_two_plane_small_rows_vs_f64(lib):
    """Every row at scale 2^-13: the representation floor dominates; held to the bound only (the device figure is printed)."""
    tok, cls, text = two_plane_case(4099, 96, 13, -13, -13, seed=13)
    got = run_two_plane(lib, tok, cls, text, -0.3)
    ref, bound = HR.cosine_two_plane_reference(tok, cls, text, -0.3)
    print(f"two-plane rows at 2^-13, E 96 Q 13: max |err| {float(np.abs(got - ref).max()):.3e}, largest bound {bound.max():.3e}")
    record("cosine_two_plane 2^-13", "n 4099 E 96 Q 13", HR.within(got, ref, bound, "two-plane 2^-13"))


def test_cosine_two_plane_reroutes_below_4096(lib):
    tok, cls, text = two_plane_case(4095, 32, 13, -2, 2, seed=5)
    assert np.array_equal(run_two_plane(lib, tok, cls, text, -0.3), run_cosine(lib, "sg_cosine_logits", tok, cls, text, 0.0, -0.3))


# ---- stitch / resize ---------------------------------------------------------------------------------------------------------------------------
def stitch_args(c):
    return c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"]


def run_stitch(lib, c):
    T, Q, gh, gw = c["tile_logits"].shape
    H, W = c["hw"]
    out = Guarded(Q * H * W)
    ok(lib, lib.sg_stitch(PD(c["tile_logits"]), PD(c["windows"]), T, Q, gh, gw, c["up_hw"][0], c["up_hw"][1], c["pad_tl"][0], c["pad_tl"][1],
                          H, W, P(out.view), stream()))
    return out.finish().reshape(Q, H, W)


@pytest.mark.parametrize("name,Q,data", HR.STITCH_CASES)
def test_stitch_vs_f64(lib, name, Q, data):
    c = HR.make_stitch_case(name, Q, data)
    got = run_stitch(lib, c)
    ref, bound = HR.stitch(*stitch_args(c)), HR.stitch_bound(*stitch_args(c))
    record("stitch " + data, f"{name} Q {Q}", HR.within(got, ref, bound, f"stitch {name} Q {Q} {data}"))
    if name == "hole":
        assert (got[:, :, 30:40] == 0).all() and (got[:, 0, 40:] == 0).all() and (got[:, 4, :30] == 0).all(), "an uncovered pixel must be 0"


@pytest.mark.parametrize("name", ["a", "b"])
def test_stitch_one_hot_vs_f64(lib, name):
    """A single 1.0 on every grid cell of one tile in turn: a wrong tap or a swapped axis is an O(1) error."""
    for i, c in enumerate(HR.one_hot_cases(name, 4)):
        ref, bound = HR.stitch(*stitch_args(c)), HR.stitch_bound(*stitch_args(c))
        record("stitch one-hot", f"{name} batch {i}", HR.within(run_stitch(lib, c), ref, bound, f"stitch one-hot {name} {i}"))


def multi_descriptors(c, per_pixel):
    """(i32 [2N,2] = image_hw then image_tiles, i64 = offsets (per_pixel elements per pixel) then the block prefix, pixel prefix, blocks)."""
    pix = np.concatenate([[0], np.cumsum([h * w for h, w in c["image_hw"]])])
    blocks = np.concatenate([[0], np.cumsum([-(-w // 64) * -(-h // 4) for h, w in c["image_hw"]])])
    i32 = np.asarray([list(hw) for hw in c["image_hw"]] + [list(ft) for ft in c["image_tiles"]], dtype=np.int32)
    i64 = np.concatenate([per_pixel * pix[:-1], blocks]).astype(np.int64)
    return i32, i64, pix, blocks


def per_image(c, n):
    a, k = c["image_tiles"][n]
    return c["tile_logits"][a:a + k], c["windows"][a:a + k], c["up_hw"], c["pad_tl"], c["image_hw"][n]


def test_stitch_multi_vs_f64(lib):
    """Three images of different sizes in one call, each canvas directly against the float64 stitch of its own tiles."""
    Q = 9
    c = HR.make_multi_case(Q)
    N, T = len(c["image_hw"]), c["tile_logits"].shape[0]
    i32, i64, pix, blocks = multi_descriptors(c, Q)
    out = Guarded(Q * int(pix[-1]))
    i32d, i64d = torch.as_tensor(i32).to(DEV), torch.as_tensor(i64).to(DEV)
    ok(lib, lib.sg_stitch_multi(PD(c["tile_logits"]), PD(c["windows"]), PD(c["tile_image"]), T, Q, 3, 4, c["up_hw"][0], c["up_hw"][1],
                                c["pad_tl"][0], c["pad_tl"][1], P(i32d), P(i32d[N:]), P(i64d), P(i64d[N:]), N, int(blocks[-1]),
                                Q * int(pix[-1]), P(out.view), stream()))
    got = out.finish()
    for n, (h, w) in enumerate(c["image_hw"]):
        ref, bound = HR.stitch(*per_image(c, n)), HR.stitch_bound(*per_image(c, n))
        record("stitch_multi", f"image {n} {h}x{w}", HR.within(got[Q * pix[n]:Q * pix[n + 1]].reshape(Q, h, w), ref, bound, f"stitch_multi image {n}"))


@pytest.mark.parametrize("C_", HR.RESIZE_C)
@pytest.mark.parametrize("hw,size", HR.RESIZE_SHAPES)
def test_resize_bilinear_vs_f64(lib, hw, size, C_):
    """The channel loop is vectorised in pairs with a scalar remainder: C = 1, 2, 5."""
    src = (np.random.default_rng(C_ + hw[0]).standard_normal((C_,) + hw) + (100.0 if C_ == 2 else 0.0)).astype(np.float32)
    out = Guarded(C_ * size[0] * size[1])
    ok(lib, lib.sg_resize_bilinear(PD(src), C_, hw[0], hw[1], P(out.view), size[0], size[1], stream()))
    got = out.finish().reshape((C_,) + size)
    ref, bound = HR.resize_reference(src, size)
    record("resize_bilinear", f"{hw} -> {size} C {C_}", HR.within(got, ref, bound, f"resize {hw}->{size} C {C_}"))
    if hw == size:
        assert np.array_equal(got, src), "the same size is an exact copy"


# ---- postprocess -------------------------------------------------------------------------------------------------------------------------------
def run_postprocess(lib, entry, canvas, qi, K, thd, bg, want_probs=True):
    Q, H, W = canvas.shape
    probs, labels = (Guarded(K * H * W) if want_probs else None), Guarded(H * W, torch.int64)
    ok(lib, getattr(lib, entry)(PD(canvas), PD(qi, torch.int32), Q, K, H, W, SCALE, thd, bg, P(probs.view) if want_probs else None,
                                P(labels.view), stream()))
    return (probs.finish().reshape(K, H, W) if want_probs else None), labels.finish().reshape(H, W)


def check_postprocess(lib, entry, Q, HW, classes, data):
    canvas, qi, K = HR.make_tail_case(Q, HW, classes, data)
    bound = HR.tail_bound(canvas, 0.0, qi, K, SCALE)
    for thd in (0.0, 0.3):
        bg = K - 1
        ref = HR.tail(canvas, qi, K, SCALE, thd, bg)
        probs, labels = run_postprocess(lib, entry, canvas, qi, K, thd, bg)
        what = f"{entry} Q {Q} HW {HW} {classes} {data} thd {thd}"
        ratio, frac, normal = HR.check_tight(ref, bound, thd, labels, probs, None, what)
        record(entry[3:] + " " + data, f"Q {Q} HW {HW} {classes}", ratio)
        record(entry[3:] + " " + data + " (p >= 2^-120)", f"Q {Q} HW {HW} {classes}", normal)
        _, only = run_postprocess(lib, entry, canvas, qi, K, thd, bg, want_probs=False)
        assert np.array_equal(only, labels), f"{what}: probs = NULL changes the labels"


@pytest.mark.parametrize("Q,HW,classes,data", HR.tail_cases(HR.PP_Q))
def test_postprocess_vs_f64(lib, Q, HW, classes, data):
    check_postprocess(lib, "sg_postprocess", Q, HW, classes, data)


@pytest.mark.parametrize("Q,HW,classes,data", HR.tail_cases(HR.PPW_Q))
def test_postprocess_wide_vs_f64(lib, Q, HW, classes, data):
    check_postprocess(lib, "sg_postprocess_wide", Q, HW, classes, data)


@pytest.mark.parametrize("Q", [5, 18])
def test_postprocess_multi_with_a_resize_vs_f64(lib, Q):
    """Two canvases, the first resized (7x9 -> 21x30), the second kept (6x5): the resize is evaluated per output pixel.  Q = 5 takes the
    odd last channel's path and the 16-query instantiation, Q = 18 the 64-query one."""
    K = Q
    chw, ohw = [(7, 9), (6, 5)], [(21, 30), (6, 5)]
    rng = np.random.default_rng(21)
    canv = [(0.25 * rng.standard_normal((Q,) + s)).astype(np.float32) for s in chw]
    flat = np.concatenate([c.reshape(-1) for c in canv])
    coff = [0, Q * 63]
    pix = [0, 630, 660]
    blocks = [0, -(-630 // 256), -(-630 // 256) + 1]
    i32 = torch.as_tensor(np.asarray(chw + ohw, dtype=np.int32)).to(DEV)
    i64 = torch.as_tensor(np.asarray(coff + pix[:-1] + blocks, dtype=np.int64)).to(DEV)
    probs, labels = Guarded(K * pix[-1]), Guarded(pix[-1], torch.int64)
    ok(lib, lib.sg_postprocess_multi(PD(flat), P(i32), P(i64), P(i32[2:]), P(i64[2:]), P(i64[4:]), 2, blocks[-1], flat.size, pix[-1],
                                     PD(np.arange(Q), torch.int32), Q, K, SCALE, 0.3, 0, P(probs.view), P(labels.view), stream()))
    gp, gl = probs.finish(), labels.finish()
    for n in range(2):
        c64, dc = HR.resize_reference(canv[n], ohw[n])
        if chw[n] == ohw[n]:
            dc = 0.0
        ref, bound = HR.tail(c64, np.arange(Q), K, SCALE, 0.3, 0), HR.tail_bound(c64, dc, np.arange(Q), K, SCALE)
        h, w = ohw[n]
        ratio, _, _ = HR.check_tight(ref, bound, 0.3, gl[pix[n]:pix[n + 1]], gp[K * pix[n]:K * pix[n + 1]].reshape(K, h, w), None,
                                     f"postprocess_multi Q {Q} image {n}")
        record("postprocess_multi", f"Q {Q} image {n}", ratio)


# ---- the fused heads ---------------------------------------------------------------------------------------------------------------------------
HEAD_REF = {}


def head_ref(geom, Q, sign, merge, thd=0.3):
    """The float64 reference and the bounds of one head case, computed once and shared by the label head and the probability head."""
    key = (geom, Q, sign, merge)
    if key not in HEAD_REF:
        c = HR.make_head_case(geom, Q, sign, merge)
        canvas, dcanvas = HR.stitch(*stitch_args(c)), HR.stitch_bound(*stitch_args(c))
        HEAD_REF[key] = (c, HR.tail(canvas, c["query_idx"], c["K"], SCALE, thd, c["K"] - 1), HR.tail_bound(canvas, dcanvas, c["query_idx"], c["K"], SCALE))
    return HEAD_REF[key]


def head_call(lib, entry, c, qi, K, thd, bg, second):
    """sg_label_head (second = conf) / sg_prob_head (second = probs) -> (second output, labels)."""
    T, Q, gh, gw = c["tile_logits"].shape
    H, W = c["hw"]
    labels, sec = Guarded(H * W, torch.int64), Guarded((K if entry == "sg_prob_head" else 1) * H * W)
    outs = (P(labels.view), P(sec.view)) if entry == "sg_label_head" else (P(sec.view), P(labels.view))
    ok(lib, getattr(lib, entry)(PD(c["tile_logits"]), PD(c["windows"]), T, Q, gh, gw, c["up_hw"][0], c["up_hw"][1], c["pad_tl"][0],
                                c["pad_tl"][1], H, W, PD(qi, torch.int32), K, SCALE, thd, bg, *outs, stream()))
    return sec.finish(), labels.finish().reshape(H, W)


@pytest.mark.parametrize("geom,Q,sign,merge", HR.HEAD_CASES)
def test_label_head_vs_f64(lib, geom, Q, sign, merge):
    c, ref, bound = head_ref(geom, Q, sign, merge)
    conf, labels = head_call(lib, "sg_label_head", c, c["query_idx"], c["K"], 0.3, c["K"] - 1, "conf")
    ratio, frac, _ = HR.check_tight(ref, bound, 0.3, labels, None, conf.reshape(c["hw"]), f"label_head {geom} Q {Q} sign {sign}")
    record("label_head conf", f"{geom} Q {Q} sign {sign} K {c['K']}", ratio)


@pytest.mark.parametrize("geom,Q,sign,merge", HR.HEAD_CASES)
def test_prob_head_vs_f64(lib, geom, Q, sign, merge):
    c, ref, bound = head_ref(geom, Q, sign, merge)
    probs, labels = head_call(lib, "sg_prob_head", c, c["query_idx"], c["K"], 0.3, c["K"] - 1, "probs")
    ratio, frac, normal = HR.check_tight(ref, bound, 0.3, labels, probs.reshape((c["K"],) + c["hw"]), None, f"prob_head {geom} Q {Q} sign {sign}")
    record("prob_head probs", f"{geom} Q {Q} sign {sign} K {c['K']}", ratio)
    record("prob_head probs (p >= 2^-120)", f"{geom} Q {Q} sign {sign} K {c['K']}", normal)


@pytest.mark.parametrize("entry,Q", [("sg_label_head_multi", 9), ("sg_prob_head_multi", 9), ("sg_prob_head_multi", 64), ("sg_prob_head_multi", 65)])
def test_head_multi_vs_f64(lib, entry, Q):
    """One call over three images of different sizes, every image directly against float64; a merged, shuffled class map.  The probability
    head at Q = 9, 64, 65: its three instantiations."""
    c = HR.make_multi_case(Q, seed=1)
    K = Q // 2
    qi = np.random.default_rng(Q).permutation(np.arange(Q) % K).astype(np.int32)
    N, T = len(c["image_hw"]), c["tile_logits"].shape[0]
    i32, i64, pix, blocks = multi_descriptors(c, 1)
    total = int(pix[-1])
    prob = entry == "sg_prob_head_multi"
    labels, sec = Guarded(total, torch.int64), Guarded((K if prob else 1) * total)
    outs = (P(sec.view), P(labels.view)) if prob else (P(labels.view), P(sec.view))
    i32d, i64d = torch.as_tensor(i32).to(DEV), torch.as_tensor(i64).to(DEV)
    ok(lib, getattr(lib, entry)(PD(c["tile_logits"]), PD(c["windows"]), PD(c["tile_image"]), T, Q, 3, 4, c["up_hw"][0], c["up_hw"][1],
                                c["pad_tl"][0], c["pad_tl"][1], P(i32d), P(i32d[N:]), P(i64d), P(i64d[N:]), N, int(blocks[-1]), total,
                                PD(qi), K, SCALE, 0.3, K - 1, *outs, stream()))
    gs, gl = sec.finish(), labels.finish()
    for n, (h, w) in enumerate(c["image_hw"]):
        canvas, dcanvas = HR.stitch(*per_image(c, n)), HR.stitch_bound(*per_image(c, n))
        ref, bound = HR.tail(canvas, qi, K, SCALE, 0.3, K - 1), HR.tail_bound(canvas, dcanvas, qi, K, SCALE)
        lab = gl[pix[n]:pix[n + 1]]
        if prob:
            ratio, _, _ = HR.check_tight(ref, bound, 0.3, lab, gs[K * pix[n]:K * pix[n + 1]].reshape(K, h, w), None, f"{entry} image {n}")
        else:
            ratio, _, _ = HR.check_tight(ref, bound, 0.3, lab, None, gs[pix[n]:pix[n + 1]].reshape(h, w), f"{entry} image {n}")
        record(entry[3:], f"image {n} {h}x{w} Q {Q}", ratio)


# ---- exact ties and the exact threshold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,merged", [(Q, m) for Q in (2, 9, 64, 65, 130) for m in (False, True) if Q >= 3 or not m])   # merged: K < Q
def test_exact_ties_go_to_the_lower_class(lib, Q, merged):
    """Two bit-identical dominating query planes; merged: the higher class owns the lower query index.  All four tails (class_tail through
    sg_postprocess and sg_prob_head for Q <= 64, the wide tail through sg_postprocess_wide and sg_prob_head beyond, the label head)."""
    canvas, qi, K, want = HR.tie_case(Q, merged, shape=(1, 257))
    for entry in (("sg_postprocess",) if Q <= 64 else ()) + ("sg_postprocess_wide",):
        probs, labels = run_postprocess(lib, entry, canvas, qi, K, 0.0, 0)
        assert (labels == want).all(), f"{entry}: {int((labels != want).sum())} tied pixels went to another class"
    wins, grid, up, pad, hw = HR.stitch_geometry("a")
    planes, _, _, _ = HR.tie_case(Q, merged, shape=(len(wins),) + tuple(grid))
    c = dict(tile_logits=np.ascontiguousarray(planes.transpose(1, 0, 2, 3)), windows=wins, up_hw=up, pad_tl=pad, hw=hw)
    for entry in ("sg_label_head", "sg_prob_head"):
        _, labels = head_call(lib, entry, c, qi, K, 0.0, 0, None)
        assert (labels == want).all(), f"{entry}: {int((labels != want).sum())} tied pixels went to another class"


def test_threshold_is_strict(lib):
    """conf == prob_thd exactly (one query: the softmax is exactly 1) keeps the class."""
    canvas = np.full((1, 1, 70), 0.25, dtype=np.float32)
    for entry in ("sg_postprocess", "sg_postprocess_wide"):
        assert (run_postprocess(lib, entry, canvas, np.zeros(1), 1, 1.0, 7)[1] == 0).all(), entry
    c = HR.make_case("a", 1, False)
    for entry in ("sg_label_head", "sg_prob_head"):
        assert (head_call(lib, entry, c, np.zeros(1), 1, 1.0, 7, None)[1] == 0).all(), entry


# ---- render_maps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("HW", [1, 255, 257])
def test_render_maps_bytes(lib, HW, K):
    labels, probs = HR.make_render_case(HW, K)
    pal = HR.make_palette(K)
    want_mask, want_heat = HR.render_reference(labels, probs, pal)
    for m, h in ((True, True), (True, False), (False, True)):
        mask, heat = Guarded(3 * HW, torch.uint8), Guarded(3 * HW, torch.uint8)
        ok(lib, lib.sg_render_maps(PD(labels), PD(probs), PD(pal), K, 1, HW, P(mask.view) if m else None, P(heat.view) if h else None, stream()))
        if m:
            assert np.array_equal(mask.finish().reshape(HW, 3), want_mask)
        else:
            assert mask.untouched()
        if h:
            assert np.array_equal(heat.finish().reshape(HW, 3), want_heat)
        else:
            assert heat.untouched()


def test_zz_worst_ratios():
    """Runs last (module order): the err / bound table of the module."""
    print("head kernels, largest err / bound per (op, case):")
    per_op = defaultdict(float)
    for key in sorted(WORST):
        print(f"  {key[0]:>34} | {key[1]:<40} {WORST[key]:.3g}")
        per_op[key[0]] = max(per_op[key[0]], WORST[key])
    print("per operation:", {k: float(f"{v:.3g}") for k, v in sorted(per_op.items())})
    assert WORST and all(v <= 1.0 for v in WORST.values())
