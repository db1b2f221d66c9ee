"""The PAMR kernels (csrc/pamr.hip) against the float64 reference of tests/pamr_reference.py, element by element, through their raw C
entries.  Every output buffer is filled with 0xFF bytes (NaN as f32) before the call and sits between two 64 KiB margins of 0xFF, which
are checked afterwards.  Guidance: normalised u8 images built on the CPU under fixed seeds (uniform noise, bicubically smoothed noise,
16-pixel constant blocks, flat); logits 0.2 + 0.1 randn.  tests/test_pamr_bound_cpu.py shows on the same generators that an f32
emulation stays inside the bounds and that the listed mutations of the definition do not.

Labels: ops.postprocess (scale 50, synonyms, prob_thd 0 and 0.5) of the refined logits must equal the float64 labels wherever the label
is decided beyond the bound: the reference's top-two gap of the scaled class logits is outside 2 * 50 * bound (plus the post-process's
own f32 roundings on that comparison), and |conf - prob_thd| is outside conf's bound (label_reference).  At most 0.5 % of a case may be
undecided; the share is a property of the reference alone (the cases and seeds were chosen on it) and is printed."""
import ctypes as C
import functools
import os
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_reference as HR                                             # noqa: E402
import pamr_reference as PR                                             # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 1 << 16
A, B, S = (1,), (8, 16), (1, 2, 4, 8, 12, 24)
STEPS = (1, 2, 10)
LABEL_CAP = 0.005
WORST = defaultdict(float)                    # (what, image kind) -> largest err / bound

# (image kind, (H, W), dilations, Q): every shape, dilation set, Q and kind, dilations larger than the image among them
CASES = [
    ("noise", (1, 1), A, 1), ("noise", (1, 1), B, 3), ("flat", (1, 1), S, 1),
    ("noise", (5, 7), A, 3), ("smooth", (5, 7), B, 17), ("blocks", (5, 7), S, 3), ("flat", (5, 7), B, 1), ("noise", (5, 7), S, 65),
    ("noise", (33, 64), A, 17), ("smooth", (33, 64), A, 3), ("blocks", (33, 64), B, 3), ("flat", (33, 64), S, 3),
    ("noise", (33, 64), B, 65), ("smooth", (33, 64), S, 17), ("blocks", (33, 64), A, 1), ("noise", (33, 64), S, 3),
    ("noise", (67, 131), A, 3), ("smooth", (67, 131), B, 17), ("blocks", (67, 131), S, 3), ("flat", (67, 131), A, 17),
    ("noise", (67, 131), B, 3), ("smooth", (67, 131), S, 1), ("blocks", (67, 131), B, 65), ("noise", (67, 131), S, 17),
    ("noise", (96, 257), A, 1), ("smooth", (96, 257), B, 3), ("blocks", (96, 257), S, 1), ("flat", (96, 257), B, 3),
    ("noise", (96, 257), B, 17), ("smooth", (96, 257), A, 65), ("noise", (96, 257), S, 3), ("blocks", (96, 257), A, 3),
]


@pytest.fixture(scope="module")
def lib():
    from clip_decontamination_amd import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def dil_arg(d):
    return (C.c_int * len(d))(*d)


class Guarded:
    """`numel` f32 elements on the device, every byte 0xFF (NaN), between two margins of 0xFF bytes; `.view` is the payload (1-D)."""

    def __init__(self, numel, init=None):
        self.big = torch.full((2 * GUARD + 4 * numel,), 0xFF, dtype=torch.uint8, device=DEV)
        self.view = self.big[GUARD:GUARD + 4 * numel].view(torch.float32)
        if init is not None:
            self.view.copy_(torch.as_tensor(init).reshape(-1))

    def finish(self):
        """Margins intact -> the payload on the CPU (numpy)."""
        torch.cuda.synchronize()
        n = self.view.numel() * 4
        assert bool((self.big[:GUARD] == 0xFF).all()) and bool((self.big[GUARD + n:] == 0xFF).all()), "margin overwritten"
        return self.view.cpu().numpy()


def ok(lib, rc):
    assert rc == 0, lib.sg_last_error()


@functools.lru_cache(maxsize=None)
def inputs(kind, hw, Q, seed=0, const=None):
    g = PR.normalise(PR.image_u8(kind, *hw, seed=seed))
    m0 = PR.logits(Q, *hw, seed=seed) if const is None else np.full((Q,) + hw, const, dtype=np.float32)
    return g, m0


@functools.lru_cache(maxsize=None)
def reference(kind, hw, dil, Q, seed=0, const=None):
    g, m0 = inputs(kind, hw, Q, seed, const)
    return PR.reference(g, m0, dil, (0,) + STEPS)


def device_weights(lib, g, hw, dil):
    w = Guarded(8 * len(dil) * hw[0] * hw[1])
    gd = torch.from_numpy(g).to(DEV)
    ok(lib, lib.sg_pamr_affinity(P(gd), hw[0], hw[1], dil_arg(dil), len(dil), P(w.view), stream()))
    return w, w.finish().reshape(8 * len(dil), *hw)


def device_steps(lib, w, m0, hw, dil, steps):
    """`steps` raw sg_pamr_step calls, each into a fresh guarded buffer -> {t: m_t} for every t."""
    Q = m0.shape[0]
    bufs, cur = [], torch.from_numpy(m0).to(DEV).reshape(-1)
    for _ in range(steps):
        bufs.append(Guarded(Q * hw[0] * hw[1]))
        ok(lib, lib.sg_pamr_step(P(w.view), P(cur), P(bufs[-1].view), Q, hw[0], hw[1], dil_arg(dil), len(dil), stream()))
        cur = bufs[-1].view
    return {t + 1: b.finish().reshape(Q, *hw) for t, b in enumerate(bufs)}


def device_pamr(lib, g, m0, hw, dil, steps):
    """sg_pamr in place on a guarded copy of m0, with a guarded workspace -> the refined logits."""
    Q = m0.shape[0]
    need = lib.sg_pamr_workspace_bytes(Q, hw[0], hw[1], len(dil))
    assert need >= (8 * len(dil) + Q) * hw[0] * hw[1] * 4
    ws = Guarded(-(-need // 4))
    io = Guarded(Q * hw[0] * hw[1], init=torch.from_numpy(m0))
    gd = torch.from_numpy(g).to(DEV)
    ok(lib, lib.sg_pamr(P(gd), P(io.view), Q, hw[0], hw[1], dil_arg(dil), len(dil), steps, P(ws.view), ws.view.numel() * 4, stream()))
    ws.finish()
    return io.finish().reshape(Q, *hw)


@pytest.mark.parametrize("kind,hw,dil,Q", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernels_vs_f64(lib, kind, hw, dil, Q):
    g, m0 = inputs(kind, hw, Q)
    ref = reference(kind, hw, dil, Q)
    K = 8 * len(dil)
    wbuf, w = device_weights(lib, g, hw, dil)
    rw = HR.within(w, ref["w"], ref["bw"], f"w {kind} {hw} {dil}")
    WORST[("w", kind)] = max(WORST[("w", kind)], rw)
    assert np.abs(w.astype(np.float64).sum(0) - 1.0).max() <= (K + 1) * PR.U
    if kind == "flat":
        assert np.all(w == np.float32(1.0) / np.float32(K))
    outs = device_steps(lib, wbuf, m0, hw, dil, max(STEPS))
    for t in STEPS:
        r = HR.within(outs[t], ref["out"][t], ref["bound"][t], f"out {kind} {hw} {dil} Q {Q} steps {t}")
        WORST[(f"steps {t}", kind)] = max(WORST[(f"steps {t}", kind)], r)
        print(f"{kind} {hw} {dil} Q {Q} steps {t}: err / bound {r:.3f} (w {rw:.3f})")
    for t in STEPS:                                                     # odd and even: the result is in logits_inout either way
        got = device_pamr(lib, g, m0, hw, dil, t)
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(outs[t])), f"sg_pamr({t}) differs from affinity + {t} steps"
    again = device_pamr(lib, g, m0, hw, dil, max(STEPS))
    assert again.tobytes() == outs[max(STEPS)].tobytes(), "two runs differ"
    _, w2 = device_weights(lib, g, hw, dil)
    assert w2.tobytes() == w.tobytes(), "two runs of the affinity differ"


@pytest.mark.parametrize("kind,hw,dil", [("noise", (33, 64), B), ("smooth", (67, 131), S), ("blocks", (5, 7), A)])
def test_constant_plane_stays_constant(lib, kind, hw, dil):
    g, m0 = inputs(kind, hw, 3, 0, 0.37)
    ref = reference(kind, hw, dil, 3, 0, 0.37)
    for t in STEPS:
        assert np.abs(ref["out"][t] - np.float64(np.float32(0.37))).max() < 1e-12
        got = device_pamr(lib, g, m0, hw, dil, t)
        r = HR.within(got, ref["out"][t], ref["bound"][t], f"constant plane {kind} steps {t}")
        WORST[("constant", kind)] = max(WORST[("constant", kind)], r)


@pytest.mark.parametrize("hw,dil,Q", [((5, 7), B, 3), ((67, 131), S, 17)])
def test_zero_steps_is_the_identity(lib, hw, dil, Q):
    from clip_decontamination_amd import ops
    g, m0 = inputs("noise", hw, Q)
    assert device_pamr(lib, g, m0, hw, dil, 0).tobytes() == m0.tobytes()
    md = torch.from_numpy(m0).to(DEV)
    out = ops.pamr(md, torch.from_numpy(g).to(DEV), 0, dil)
    assert out.cpu().numpy().tobytes() == m0.tobytes() and torch.equal(md.cpu(), torch.from_numpy(m0))


def test_ops_wrappers_equal_the_raw_entries(lib):
    from clip_decontamination_amd import ops
    kind, hw, dil, Q = "smooth", (33, 64), B, 17
    g, m0 = inputs(kind, hw, Q)
    gd, md = torch.from_numpy(g).to(DEV), torch.from_numpy(m0).to(DEV)
    w = ops.pamr_weights(gd, dil)
    assert w.cpu().numpy().tobytes() == device_weights(lib, g, hw, dil)[1].tobytes()
    raw = device_pamr(lib, g, m0, hw, dil, 3)
    m = md
    for _ in range(3):
        m = ops.pamr_step(w, m, dil)
    assert m.cpu().numpy().tobytes() == raw.tobytes()
    assert ops.pamr(md, gd, 3, dil).cpu().numpy().tobytes() == raw.tobytes() and torch.equal(md.cpu(), torch.from_numpy(m0))
    inpl = md.clone()
    assert ops.pamr(inpl, gd, 3, dil, inplace=True) is inpl and inpl.cpu().numpy().tobytes() == raw.tobytes()
    with pytest.raises(RuntimeError, match="in == out"):
        _lib_check_in_out(lib, w, md, hw, dil)


def _lib_check_in_out(lib, w, md, hw, dil):
    from clip_decontamination_amd._lib import check
    check(lib.sg_pamr_step(P(w), P(md), P(md), md.shape[0], hw[0], hw[1], dil_arg(dil), len(dil), stream()), "sg_pamr_step")


# ---- labels ----------------------------------------------------------------------------------------------------------------------------
LABEL_Q = 17
LABEL_QIDX = np.array([0, 0, 1, 2, 2, 2, 3, 4, 5, 5, 6, 7, 7, 8, 8, 8, 8], dtype=np.int32)     # synonyms: 17 queries, 9 classes
# (kind, (H, W), dilations, seed, prob_thd), chosen on the float64 reference alone (label_reference) so that at most 0.5 % of the pixels are
# undecided.  Every case holds for prob_thd = 0; at prob_thd = 0.5 the smooth and the noise images leave 0.6 to 1.7 % of their pixels
# inside conf's bound of the threshold under every seed tried (their median conf is about 0.5), so the threshold runs on the block images.
LABEL_CASES = [("blocks", (67, 131), B, 0, 0.0), ("blocks", (67, 131), B, 0, 0.5), ("blocks", (33, 64), S, 1, 0.0), ("blocks", (33, 64), S, 1, 0.5),
               ("blocks", (33, 64), B, 0, 0.5), ("smooth", (33, 64), B, 6, 0.0), ("noise", (33, 64), B, 2, 0.0), ("smooth", (67, 131), A, 1, 0.0)]


def label_reference(kind, hw, dil, seed, thd):
    """-> (reference tail dict, mask of the pixels whose label is decided beyond the bound), from the float64 reference alone.
    Ties: with L_c = the largest scaled logit 50 m_q among class c's queries (the softmax's normaliser is common to all classes, so the
    arg-max over class probabilities is the arg-max over L_c), a pixel is decided when the top-two gap L_1 - L_2 exceeds 50 (b_1 + b_2),
    b_i the logits' bound at the two deciding queries (at most 2 * 50 * bound), plus the post-process's own f32 roundings on that
    comparison: the two products (u |L_i|), two expf (EXPF each) and two divisions (2 u each).  Threshold: |conf - prob_thd| must
    exceed conf's bound (head_reference.tail_bound fed the logits' bound)."""
    ref = reference(kind, hw, dil, LABEL_Q, seed)
    m, b = ref["out"][10], ref["bound"][10]
    K = int(LABEL_QIDX.max()) + 1
    tail = HR.tail(m, LABEL_QIDX, K, 50.0, thd, 0)
    v = 50.0 * m
    L = np.full((K,) + hw, -np.inf)
    bL = np.zeros((K,) + hw)
    for q, c in enumerate(LABEL_QIDX):
        take = v[q] > L[c]
        L[c], bL[c] = np.where(take, v[q], L[c]), np.where(take, b[q], bL[c])
    top = np.argsort(L, axis=0, kind="stable")[-2:]
    L2, b2 = np.take_along_axis(L, top, 0), np.take_along_axis(bL, top, 0)
    own = PR.U * np.abs(L2).sum(0) + 2 * HR.EXPF + 4 * PR.U
    decided = (L2[1] - L2[0]) > 50.0 * b2.sum(0) + own
    if thd > 0:
        decided &= np.abs(tail["conf"] - thd) > HR.tail_bound(m, b, LABEL_QIDX, K, 50.0)["conf"]
    return tail, decided


@pytest.mark.parametrize("kind,hw,dil,seed,thd", LABEL_CASES)
def test_labels_after_postprocess(lib, kind, hw, dil, seed, thd):
    from clip_decontamination_amd import ops
    g, m0 = inputs(kind, hw, LABEL_Q, seed)
    tail, okmask = label_reference(kind, hw, dil, seed, thd)
    share = 1.0 - okmask.mean()
    got = torch.from_numpy(device_pamr(lib, g, m0, hw, dil, 10)).to(DEV)
    _, labels = ops.postprocess(got, torch.from_numpy(LABEL_QIDX), int(LABEL_QIDX.max()) + 1, 50.0, thd, 0, want_probs=False)
    labels = labels.cpu().numpy().reshape(hw)
    bad = int((labels[okmask] != tail["labels"][okmask]).sum())
    moved = float((tail["labels"] == 0).mean())
    print(f"labels {kind} {hw} {dil} thd {thd}: undecided {100 * share:.3f} %, mismatches on decided pixels {bad}, class 0 share {moved:.3f}")
    assert share <= LABEL_CAP, f"{100 * share:.2f} % of the pixels are inside the bound of a tie or of the threshold"
    assert bad == 0


def test_zz_worst_ratios_report():
    """Prints the largest err / bound per quantity and image kind (what DESIGN.md records); runs last in this file."""
    for key in sorted(WORST):
        print(f"worst err / bound {key[0]:>9s} {key[1]:>7s}: {WORST[key]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
