"""Cluster-Then-Debias (csrc/ctd.hip) through ops.ctd_debias with explicit eps / min_samples against tests/refine_reference.py: labels
exactly those of the oracle's DBSCAN (which tests/test_refine_bound_cpu.py pins to scikit-learn on the same inputs), noise rows
bit-identical, clustered rows within a per-element bound, want_labels=False the same tokens, a 64 KiB guard band around the token and
label buffers.  The inputs reach what blob clusters do not: a long label propagation (a shuffled chain), the n = 8192 cap with its
69 KiB of LDS and the skip beyond it, a contested border point, pairs within 5e-5 of the radius on both sides (the f64 re-evaluation),
and word-boundary sizes of the adjacency rows."""
import ctypes as C
import os
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_reference as R                                            # noqa: E402
from refine_reference import check_within                               # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 1 << 16
F_SENTINEL, I_SENTINEL = -12345.5, -77
FACTOR = -1.5
WORST = defaultdict(float)                    # case -> largest err / bound


@pytest.fixture(scope="module")
def ops():
    from clip_decontamination_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from clip_decontamination_amd import _lib
    return _lib.load()


def guarded(t, sentinel):
    g = GUARD // t.element_size()
    big = torch.full((2 * g + t.numel(),), sentinel, dtype=t.dtype, device=DEV)
    view = big[g:g + t.numel()].view(t.shape)
    view.copy_(t)
    return big, view


def guard_intact(big, numel, sentinel) -> bool:
    g = GUARD // big.element_size()
    return bool((big[:g] == sentinel).all()) and bool((big[g + numel:] == sentinel).all())


def P(t):
    return C.c_void_p(t.data_ptr())


def make_cls(B, Cc, seed=5):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((B, Cc)).astype(np.float32))


def run_ctd(ops, lib, x, cls, eps, ms):
    """ops.ctd_debias with and without labels, then the C ABI on guarded token and label buffers: same bits, guards unchanged."""
    xd, cd = x.to(DEV), cls.to(DEV)
    out, labels = ops.ctd_debias(xd, cd, eps=eps, min_samples=ms, factor=FACTOR)
    out2, none = ops.ctd_debias(xd, cd, eps=eps, min_samples=ms, factor=FACTOR, want_labels=False)
    assert none is None and torch.equal(out2, out), "want_labels=False changed the tokens"
    B, n, Cc = x.shape
    xbig, xview = guarded(x, F_SENTINEL)
    lbig, lview = guarded(torch.zeros(B, n, dtype=torch.int32), I_SENTINEL)
    sp, sn = ops._aligned(ops.scratch(lib.sg_ctd_scratch_bytes(B, n, Cc), DEV))
    rc = lib.sg_ctd_debias(P(xview), P(cd), B, n, Cc, float(eps), int(ms), FACTOR, 0, P(lview), sp, sn, ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.sg_last_error()
    assert torch.equal(xview, out) and torch.equal(lview, labels)
    assert guard_intact(xbig, xview.numel(), F_SENTINEL) and guard_intact(lbig, lview.numel(), I_SENTINEL)
    return out.cpu(), labels.cpu()


def check_ctd(ops, lib, name, x, eps, ms, margin=None):
    cls = make_cls(x.shape[0], x.shape[2])
    ref = R.ctd_reference(x, cls, eps, ms, FACTOR)
    if margin is not None:
        assert ref["radius_margin"] >= margin, ref["radius_margin"]      # on the CPU, before any launch
    out, labels = run_ctd(ops, lib, x, cls, eps, ms)
    assert torch.equal(labels.long(), ref["labels"]), \
        f"{name}: {int((labels.long() != ref['labels']).sum())} labels differ (radius margin {ref['radius_margin']:.2e})"
    noise = ref["labels"] < 0
    assert torch.equal(out[noise], x[noise]), f"{name}: a noise row changed"
    ratio = 0.0
    if bool((~noise).any()):
        ratio = check_within(out[~noise], ref["out"][~noise], ref["bound"][~noise], name)
        WORST[name] = max(WORST[name], ratio)
    print(f"ctd {name}: clusters {[int(l.max()) + 1 for l in ref['labels']]}, noise {[int((l < 0).sum()) for l in ref['labels']]}, "
          f"radius margin {ref['radius_margin']:.2e}, err/bound {ratio:.3g}")
    return ref


def test_ctd_chain_needs_a_long_propagation(ops, lib):
    ch = R.make_chain(2048)
    ref = check_ctd(ops, lib, "chain n=2048", ch["x"], ch["eps"], ch["min_samples"])
    assert bool((ref["labels"] == 0).all())                               # one cluster, no noise, the ends border points


def test_ctd_chain_at_the_point_cap_and_the_skip_beyond_it(ops, lib):
    ch = R.make_chain(8192)
    ref = check_ctd(ops, lib, "chain n=8192", ch["x"], ch["eps"], ch["min_samples"])
    assert bool((ref["labels"] == 0).all())
    x = torch.cat([ch["x"], ch["x"][:, :1]], 1).contiguous()              # n = 8193: the reference skips the clustering
    cls = make_cls(1, x.shape[2])
    out, labels = run_ctd(ops, lib, x, cls, ch["eps"], ch["min_samples"])
    assert bool((labels == -1).all()) and torch.equal(out, x)


def test_ctd_contested_border_point(ops, lib):
    co = R.make_contested()
    ref = check_ctd(ops, lib, "contested border", co["x"], co["eps"], co["min_samples"])
    lab = ref["labels"]
    assert lab[0, co["z"]] == 0 and lab[0, co["tX"]] == 1                 # z takes Y's label although tX is its lowest-index core neighbour
    assert bool((lab[1] == -1).all()) and lab[2, co["e"]] == 1 and lab[2, 1] == 0
    assert [int(l.max()) + 1 for l in lab] == [2, 0, 2]


def test_ctd_pairs_near_the_radius(ops, lib):
    nr = R.make_near_radius()
    ref = check_ctd(ops, lib, "near radius", nr["x"], nr["eps"], nr["min_samples"], margin=R.RADIUS_MARGIN)
    assert bool((ref["labels"][0, nr["inside"]] >= 0).all()) and bool((ref["labels"][0, nr["outside"]] == -1).all())


@pytest.mark.parametrize("Cc,eps,ms", [(4, 0.4, 5), (200, 1.1, 11)])
@pytest.mark.parametrize("n", [63, 64, 65, 1025])
def test_ctd_shapes(ops, lib, n, Cc, eps, ms):
    x = R.make_blobs(n, Cc, eps, seed=n + Cc)
    check_ctd(ops, lib, f"blobs n={n} C={Cc}", x, eps, ms, margin=R.RADIUS_MARGIN)


def test_zz_worst_ratios():
    """Runs last (module order): the err / bound table of the module."""
    print("Cluster-Then-Debias, largest err / bound per case:")
    for key in sorted(WORST):
        print(f"  {key:<24} {WORST[key]:.3g}")
    assert all(v <= 1.0 for v in WORST.values())
