"""PAMR on the CPU: the float64 reference of tests/pamr_reference.py is pinned by an independent formulation (replicate padding plus
dilated 3 x 3 convolutions), an f32 emulation of the kernels stays inside the reference's bound on every image kind of the GPU test, each
listed mutation of the definition falls outside it, and the C entries refuse what the header says they refuse before any device work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pamr_reference as PR                                             # noqa: E402

H, W, Q = 33, 40, 3


def conv_formulation(g, m0, dilations, steps):
    """The definition again, from F.pad(mode='replicate') and dilated 3 x 3 conv2d kernels: nine-tap (the window sum), one-hot copies
    (the samples, the neighbours of a step) and centre minus neighbour (the differences), float64."""
    g = torch.from_numpy(np.asarray(g)).double()
    D = len(dilations)
    cmn, copy8, copy9 = torch.zeros(8, 1, 3, 3).double(), torch.zeros(8, 1, 3, 3).double(), torch.zeros(9, 1, 3, 3).double()
    for j, (dy, dx) in enumerate(PR.OFFSETS):
        cmn[j, 0, 1, 1] = 1.0
        cmn[j, 0, 1 + dy, 1 + dx] = -1.0
        copy8[j, 0, 1 + dy, 1 + dx] = 1.0
    for j in range(9):
        copy9[j, 0, j // 3, j % 3] = 1.0
    nine = torch.ones(1, 1, 3, 3).double()

    def conv(x, k, d):                                                  # x [C,H,W] -> [C, len(k), H, W]
        return F.conv2d(F.pad(x[:, None], (d, d, d, d), mode="replicate"), k, dilation=d)

    mean = sum(conv(g, nine, d)[:, 0] for d in dilations) / (9 * D)
    samples = torch.cat([conv(g, copy9, d) for d in dilations], 1)
    sigma = (((samples - mean[:, None]) ** 2).sum(1) / (9 * D - 1)).sqrt()
    diff = torch.cat([conv(g, cmn, d) for d in dilations], 1)
    w = torch.softmax((-diff.abs() / (1e-8 + 0.1 * sigma[:, None])).mean(0), 0)
    m = torch.from_numpy(np.asarray(m0)).double()
    for _ in range(steps):
        m = (torch.cat([conv(m, copy8, d) for d in dilations], 1) * w[None]).sum(1)
    return w.numpy(), m.numpy()


@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("dilations", [(1,), (2, 5), (8, 16), (1, 2, 4, 8, 12, 24)])
def test_reference_equals_the_conv_formulation(kind, dilations):
    """Pins the definition: replicate padding, the centre counted once per dilation, the divisor 9D - 1, one softmax over all 8D, the
    offsets' order (the conv kernels place each offset by its (dy, dx), not by its index)."""
    g = PR.normalise(PR.image_u8(kind, 19, 23, seed=3))
    m0 = PR.logits(2, 19, 23)
    ref = PR.reference(g, m0, dilations, [0, 1, 3])
    w, m = conv_formulation(g, m0, dilations, 3)
    assert np.abs(ref["w"] - w).max() <= 1e-12
    assert np.abs(ref["out"][3] - m).max() <= 1e-12
    assert np.array_equal(ref["out"][0], m0.astype(np.float64))
    if kind == "flat":
        assert np.all(ref["w"] == 1.0 / (8 * len(dilations)))


def ratios(ref, w, m, t):
    return float((np.abs(w - ref["w"]) / ref["bw"]).max()), float((np.abs(m - ref["out"][t]) / ref["bound"][t]).max())


@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("dilations,shape", [((1,), (5, 7)), ((2, 5), (H, W)), ((8, 16), (H, W)), ((1, 2, 4, 8, 12, 24), (20, 27))])
def test_f32_emulation_stays_inside_the_bound(kind, dilations, shape):
    g = PR.normalise(PR.image_u8(kind, *shape, seed=1))
    m0 = PR.logits(Q, *shape)
    ref = PR.reference(g, m0, dilations, [1, 10])
    for t in (1, 10):
        w, m = PR.emulate(g, m0, dilations, t)
        rw, rm = ratios(ref, w, m, t)
        print(f"{kind} {dilations} steps {t}: err / bound w {rw:.3f} out {rm:.3f}; max bound w {ref['bw'].max():.2e} out {ref['bound'][t].max():.2e}")
        assert rw <= 1.0 and rm <= 1.0
    if kind == "flat":
        assert np.all(w == np.float32(1.0) / np.float32(8 * len(dilations)))
    s = w.astype(np.float64).sum(0)
    assert np.abs(s - 1.0).max() <= (8 * len(dilations) + 1) * PR.U


@pytest.mark.parametrize("mut", PR.MUTATIONS)
def test_mutations_fall_outside_the_bound(mut):
    """Each mutation of the definition, evaluated in f32, leaves the bound on every non-flat image kind (weights or the output of two steps)."""
    dilations = (2, 5)
    for kind in ("noise", "smooth", "blocks"):
        g = PR.normalise(PR.image_u8(kind, H, W, seed=1))
        m0 = PR.logits(Q, H, W)
        ref = PR.reference(g, m0, dilations, [2])
        w, m = PR.emulate(g, m0, dilations, 2, mut=mut)
        rw, rm = ratios(ref, w, m, 2)
        print(f"{mut} on {kind}: err / bound w {rw:.3g} out {rm:.3g}")
        assert max(rw, rm) > 1.0, f"{mut} on {kind} is inside the bound"


def test_abi_refusals_without_gpu():
    """Null pointers, the limits, in == out and a workspace too small are refused before any device work, each with its message."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    p, p2 = C.c_void_p(1 << 20), C.c_void_p(1 << 21)                    # never dereferenced
    I = C.c_int

    def dil(*d):
        return (I * len(d))(*d)

    need = lib.sg_pamr_workspace_bytes(4, 10, 12, 2)
    assert need >= (16 + 4) * 10 * 12 * 4 and lib.sg_pamr_workspace_bytes(4, 10, 12, 0) == 0 and lib.sg_pamr_workspace_bytes(4, 10, 12, 9) == 0
    cases = [
        (lambda: lib.sg_pamr_affinity(None, 10, 12, dil(8, 16), 2, p, None), b"null pointer"),
        (lambda: lib.sg_pamr_affinity(p, 10, 12, dil(8, 16), 2, None, None), b"null pointer"),
        (lambda: lib.sg_pamr_affinity(p, 10, 12, None, 2, p2, None), b"null pointer"),
        (lambda: lib.sg_pamr_affinity(p, 0, 12, dil(8), 1, p2, None), b"at least 1"),
        (lambda: lib.sg_pamr_affinity(p, 10, 12, dil(8), 0, p2, None), b"n_dil=0"),
        (lambda: lib.sg_pamr_affinity(p, 10, 12, dil(*([1] * 9)), 9, p2, None), b"n_dil=9"),
        (lambda: lib.sg_pamr_affinity(p, 10, 12, dil(8, 0), 2, p2, None), b"dilation 1 is 0"),
        (lambda: lib.sg_pamr_affinity(p, 10, 12, dil(65), 1, p2, None), b"dilation 0 is 65"),
        (lambda: lib.sg_pamr_step(None, p, p2, 4, 10, 12, dil(8), 1, None), b"null pointer"),
        (lambda: lib.sg_pamr_step(p, p2, p2, 4, 10, 12, dil(8), 1, None), b"in == out"),
        (lambda: lib.sg_pamr_step(p, p, p2, 0, 10, 12, dil(8), 1, None), b"at least 1"),
        (lambda: lib.sg_pamr_step(p, p, p2, 4, 10, 12, dil(8), 9, None), b"n_dil=9"),
        (lambda: lib.sg_pamr(None, p, 4, 10, 12, dil(8, 16), 2, 10, p2, need, None), b"null pointer"),
        (lambda: lib.sg_pamr(p, None, 4, 10, 12, dil(8, 16), 2, 10, p2, need, None), b"null pointer"),
        (lambda: lib.sg_pamr(p, p, 4, 10, 12, dil(8, 16), 2, 10, None, need, None), b"null pointer"),
        (lambda: lib.sg_pamr(p, p, 4, 10, 12, dil(8, 16), 2, -1, p2, need, None), b"steps=-1"),
        (lambda: lib.sg_pamr(p, p, 4, 10, 12, dil(8, 16), 2, 65, p2, need, None), b"steps=65"),
        (lambda: lib.sg_pamr(p, p, 4, 10, 0, dil(8, 16), 2, 10, p2, need, None), b"at least 1"),
        (lambda: lib.sg_pamr(p, p, 4, 10, 12, dil(8, 99), 2, 10, p2, need, None), b"dilation 1 is 99"),
        (lambda: lib.sg_pamr(p, p, 4, 10, 12, dil(8, 16), 2, 10, p2, need - 1, None), b"workspace too small"),
    ]
    for call, msg in cases:
        assert call() != 0
        assert msg in lib.sg_last_error(), (msg, lib.sg_last_error())
    assert lib.sg_pamr(p, p, 4, 10, 12, dil(8, 16), 2, 0, None, 0, None) == 0        # steps = 0: the identity, nothing is launched


def test_python_refusals_without_gpu():
    from clip_decontamination_amd import ops
    from clip_decontamination_amd.pipeline import SegPipeline
    with pytest.raises(ValueError, match="dilations"):
        ops.pamr_dilations((8, 0))
    with pytest.raises(ValueError, match="dilations"):
        ops.pamr_dilations(tuple(range(1, 10)))
    with pytest.raises(ValueError, match="pamr_steps"):
        SegPipeline(None, None, None, pamr_steps=65)
    with pytest.raises(ValueError, match="halo"):
        SegPipeline(None, None, None, pamr_steps=10, tile_group="world")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pamr(torch.zeros(2, 4, 4), torch.zeros(3, 4, 4), 1, (1,))
