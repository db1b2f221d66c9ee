"""sg_prob_head / sg_prob_head_multi: tile logits -> class probabilities + labels without the [Q,H,W] canvas.  The reference in every case
is the canvas route on the same tensors (ops.stitch -> ops.postprocess; ops.stitch_multi -> ops.postprocess_multi), and the comparison
is torch.equal on probabilities and labels: there is no tolerance.

Inputs: tile logits 0.1 * randn under a fixed seed, windows from pipeline.tile_windows, logit_scale = 50.  prob_thd in {0, 0.5}; at 0.5
every input is first checked on the CPU (float64, tests/head_reference.py) to have pixels on both sides of the threshold -- except Q = 1,
where the softmax over one query is 1 at every pixel and no pixel can lie below it (asserted as such)."""
import numpy as np
import pytest
import torch

import head_reference as HR

pytestmark = pytest.mark.gpu

SCALE = 50.0
# name -> (H, W, crop, stride, (gh, gw), up, pad)
GEOM = {
    "a": (40, 150, 32, 16, (4, 4), 32, 0),      # 18 tiles: clamped last row and column, a partial 64-pixel block, H a multiple of 4
    "b": (47, 61, 30, 15, (3, 3), 42, 6),       # a patch-14-like padded tile, H and W no multiples of 4 / 64
    "c": (48, 48, 32, 16, (32, 32), 32, 0),     # per-pixel tile logits as the upsamplers produce
    "d": (41, 41, 32, 1, (4, 4), 32, 0),        # 100 tiles, more than 64 candidates on most blocks: the every-window branch
}
REG_Q, WIDE_Q = (1, 7, 8, 9, 16, 33, 64), (65, 130)
_cases = {}


def case(geom, Q):
    """-> dict(tl [T,Q,gh,gw] cuda, tl_np, wins list, win [T,4] cuda, up, pad, hw): made once per (geometry, Q) and left unchanged."""
    if (geom, Q) not in _cases:
        from clip_decontamination_amd.pipeline import tile_windows
        H, W, crop, stride, grid, up, pad = GEOM[geom]
        wins = tile_windows(H, W, (stride, stride), (crop, crop))
        gen = torch.Generator().manual_seed(1000 * Q + ord(geom))
        tl = 0.1 * torch.randn(len(wins), Q, *grid, generator=gen)
        _cases[(geom, Q)] = dict(tl=tl.cuda(), tl_np=tl.numpy(), wins=wins, win=torch.tensor(wins, dtype=torch.int32, device="cuda"),
                                 up=(up, up), pad=(pad, pad), hw=(H, W))
    return _cases[(geom, Q)]


def canvas_route(c, qi, K, thd, bg):
    from clip_decontamination_amd import ops
    canvas = ops.stitch(c["tl"], c["win"], c["up"], c["pad"], c["hw"])
    return ops.postprocess(canvas, qi, K, SCALE, thd, bg, want_probs=True)


def raw_head(c, qi, K, thd, bg, probs=None, labels=None, null_probs=False):
    """The C entry on caller-owned buffers pre-filled with NaN / -1 -> (rc, probs [K,H,W], labels [1,H,W])."""
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    H, W = c["hw"]
    T, Q, gh, gw = c["tl"].shape
    probs = torch.full((max(K, 1), H, W), float("nan"), device="cuda") if probs is None else probs
    labels = torch.full((1, H, W), -1, dtype=torch.int64, device="cuda") if labels is None else labels
    q = qi.to(device="cuda", dtype=torch.int32).contiguous()
    rc = lib.sg_prob_head(ops.ptr(c["tl"]), ops.ptr(c["win"]), T, Q, gh, gw, c["up"][0], c["up"][1], c["pad"][0], c["pad"][1], H, W,
                          ops.ptr(q), K, SCALE, thd, bg, None if null_probs else ops.ptr(probs), ops.ptr(labels), ops.stream_ptr())
    torch.cuda.synchronize()
    return rc, probs, labels


def both_sides(c, qi, K, thd, what):
    """CPU, float64: the input has pixels decided above and below the threshold (beyond f32 rounding: HR.G)."""
    ref = HR.label_head(c["tl_np"], c["wins"], c["up"], c["pad"], c["hw"], np.asarray(qi), K, SCALE, thd, 0)
    above, below = int((ref["conf"] >= thd + HR.G).sum()), int((ref["conf"] < thd - HR.G).sum())
    print(f"{what}: conf >= {thd}: {above} pixels, below: {below}")
    return above, below


def check(c, qi, K, what):
    Q = c["tl"].shape[1]
    bg = 1 if K >= 2 else 0
    for thd in (0.0, 0.5):
        if thd > 0:
            above, below = both_sides(c, qi, K, thd, what)
            if Q == 1:
                assert below == 0 and above == c["hw"][0] * c["hw"][1]      # softmax over one query: 1 everywhere
            else:
                assert above > 0 and below > 0, f"{what}: the threshold {thd} does not split the input"
        want_p, want_l = canvas_route(c, qi, K, thd, bg)
        rc, probs, labels = raw_head(c, qi, K, thd, bg)
        assert rc == 0
        assert not bool(torch.isnan(probs).any()) and int(labels.min()) >= 0     # every element overwritten
        assert torch.equal(probs, want_p), f"{what} thd={thd}: probabilities differ from the canvas route"
        assert torch.equal(labels, want_l), f"{what} thd={thd}: labels differ from the canvas route"
        if thd > 0 and Q > 1:
            assert bool((labels == bg).any()) and bool((want_p.max(0)[0] < thd).any())
        rc2, probs2, labels2 = raw_head(c, qi, K, thd, bg)                       # a second call: the same bytes
        assert rc2 == 0 and torch.equal(probs2, probs) and torch.equal(labels2, labels)


@pytest.mark.parametrize("Q", REG_Q + WIDE_Q)
@pytest.mark.parametrize("geom", ["a", "b", "c"])
def test_equals_the_canvas_route(geom, Q):
    check(case(geom, Q), torch.arange(Q, dtype=torch.int32), Q, f"geometry {geom} Q=K={Q}")


def test_every_window_branch():
    c = case("d", 9)
    assert len(c["wins"]) == 100
    check(c, torch.arange(9, dtype=torch.int32), 9, "geometry d Q=K=9")


def class_maps(Q):
    rng = np.random.default_rng(Q)
    K = max(2, Q // 2)
    syn = np.concatenate([np.arange(K), rng.integers(0, K, Q - K)])
    rng.shuffle(syn)                                                          # synonyms, unsorted, every class named
    return {"synonyms": (syn, K), "unnamed_class": (np.array([2, 0] * Q)[:Q], 3), "one_class": (np.zeros(Q, dtype=np.int64), 1)}


@pytest.mark.parametrize("kind", ["synonyms", "unnamed_class", "one_class"])
@pytest.mark.parametrize("Q", [9, 64, 65])
def test_class_merge(Q, kind):
    qi, K = class_maps(Q)[kind]
    assert K < Q and (kind != "unnamed_class" or 1 not in qi)
    check(case("a", Q), torch.from_numpy(qi.astype(np.int32)), K, f"geometry a Q={Q} K={K} {kind}")


def test_op_returns_what_postprocess_returns():
    from clip_decontamination_amd import ops
    for Q in (9, 65):
        c = case("a", Q)
        qi = torch.arange(Q, dtype=torch.int32)
        probs, labels = ops.prob_head(c["tl"], c["win"], c["up"], c["pad"], c["hw"], qi, Q, SCALE, 0.5, 1)
        want_p, want_l = canvas_route(c, qi, Q, 0.5, 1)
        assert probs.shape == want_p.shape and labels.shape == want_l.shape == (1,) + c["hw"] and labels.dtype == torch.int64
        assert torch.equal(probs, want_p) and torch.equal(labels, want_l)


# ---- multi ---------------------------------------------------------------------------------------------------------------------------
MULTI_HW = [(40, 150), (32, 32), (50, 33)]


def multi_case(Q):
    from clip_decontamination_amd.pipeline import tile_windows
    wins = [tile_windows(h, w, (16, 16), (32, 32)) for h, w in MULTI_HW]
    counts = [len(w) for w in wins]
    assert counts == [18, 1, 6]
    gen = torch.Generator().manual_seed(77 + Q)
    tl = (0.1 * torch.randn(sum(counts), Q, 4, 4, generator=gen)).cuda()
    first = [0, counts[0], counts[0] + counts[1]]
    flat = [w for ws in wins for w in ws]
    local = [n for n, k in enumerate(counts) for _ in range(k)]
    return tl, wins, flat, local, list(zip(first, counts))


@pytest.mark.parametrize("Q", [9, 65])
def test_multi_equals_single_and_the_canvas_route(Q):
    from clip_decontamination_amd import ops
    tl, wins, flat, local, tiles = multi_case(Q)
    K = max(2, Q // 2)
    qi = torch.from_numpy(class_maps(Q)["synonyms"][0].astype(np.int32))
    args = (tl, torch.tensor(flat, dtype=torch.int32), local, (32, 32), (0, 0), MULTI_HW, tiles)
    prb, lab, flat_lab = ops.prob_head_multi(*args, qi, K, SCALE, 0.5, 1)
    prb2, lab2, _ = ops.prob_head_multi(*args, qi, K, SCALE, 0.5, 1)
    canvases, views = ops.stitch_multi(*args)
    if Q <= ops.POSTPROCESS_MAX_Q:
        want_p, want_l = ops.postprocess_multi(canvases, MULTI_HW, qi, K, SCALE, 0.5, 1)
    else:
        want = [ops.postprocess(v, qi, K, SCALE, 0.5, 1) for v in views]
        want_p, want_l = [p for p, _ in want], [l for _, l in want]
    pix = ops._prefix(h * w for h, w in MULTI_HW)
    assert flat_lab.shape == (pix[-1],) and flat_lab.dtype == torch.int64
    for n, (h, w) in enumerate(MULTI_HW):
        a, z = tiles[n][0], tiles[n][0] + tiles[n][1]
        one_p, one_l = ops.prob_head(tl[a:z], torch.tensor(wins[n], dtype=torch.int32), (32, 32), (0, 0), (h, w), qi, K, SCALE, 0.5, 1)
        assert prb[n].shape == (K, h, w) and lab[n].shape == (1, h, w)
        assert torch.equal(prb[n], one_p) and torch.equal(lab[n], one_l), f"image {n}: multi differs from the single-image head"
        assert torch.equal(prb[n], want_p[n]) and torch.equal(lab[n], want_l[n]), f"image {n}: multi differs from the canvas route"
        assert torch.equal(prb[n], prb2[n]) and torch.equal(lab[n], lab2[n])
        # the documented layout: labels at pix[n] of the flat buffer, probs at K * pix[n] elements of theirs
        assert torch.equal(flat_lab[pix[n]:pix[n + 1]].view(1, h, w), lab[n]) and lab[n].data_ptr() == flat_lab.data_ptr() + 8 * pix[n]
        assert prb[n].data_ptr() == prb[0].data_ptr() + 4 * K * pix[n]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["null_probs", "K>Q", "K<1"])
def test_refusals_write_nothing(what):
    from clip_decontamination_amd import _lib
    c = case("a", 9)
    K = {"null_probs": 9, "K>Q": 10, "K<1": 0}[what]
    H, W = c["hw"]
    probs = torch.full((10, H, W), float("nan"), device="cuda")
    labels = torch.full((1, H, W), -1, dtype=torch.int64, device="cuda")
    rc, _, _ = raw_head(c, torch.arange(9, dtype=torch.int32), K, 0.0, 0, probs=probs, labels=labels, null_probs=what == "null_probs")
    assert rc != 0 and b"sg_prob_head" in _lib.load().sg_last_error()
    assert bool(torch.isnan(probs).all()) and bool((labels == -1).all())


@pytest.mark.parametrize("what", ["null_probs", "K>Q", "K<1"])
def test_multi_refusals_write_nothing(what):
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    tl, wins, flat, local, tiles = multi_case(9)
    K = {"null_probs": 9, "K>Q": 10, "K<1": 0}[what]
    pix = ops._prefix(h * w for h, w in MULTI_HW)
    blocks = ops._prefix(-(-w // 64) * -(-h // 4) for h, w in MULTI_HW)
    i32 = torch.tensor([list(hw) for hw in MULTI_HW] + [list(t) for t in tiles], dtype=torch.int32).cuda()
    i64 = torch.tensor(pix[:-1] + blocks, dtype=torch.int64).cuda()
    win, ti = torch.tensor(flat, dtype=torch.int32).cuda(), torch.tensor(local, dtype=torch.int32).cuda()
    qi = torch.arange(9, dtype=torch.int32).cuda()
    probs = torch.full((10 * pix[-1],), float("nan"), device="cuda")
    labels = torch.full((pix[-1],), -1, dtype=torch.int64, device="cuda")
    rc = lib.sg_prob_head_multi(ops.ptr(tl), ops.ptr(win), ops.ptr(ti), tl.shape[0], 9, 4, 4, 32, 32, 0, 0, ops.ptr(i32), ops.ptr(i32[3:]),
                                ops.ptr(i64), ops.ptr(i64[3:]), 3, blocks[-1], pix[-1], ops.ptr(qi), K, SCALE, 0.0, 0,
                                None if what == "null_probs" else ops.ptr(probs), ops.ptr(labels), ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"sg_prob_head_multi" in lib.sg_last_error()
    assert bool(torch.isnan(probs).all()) and bool((labels == -1).all())


# ---- memory --------------------------------------------------------------------------------------------------------------------------
def test_no_buffer_of_canvas_size():
    from clip_decontamination_amd import ops
    Q = 130
    c = case("a", Q)
    H, W = c["hw"]
    qi = torch.arange(Q, dtype=torch.int32, device="cuda")

    def rise(fn):
        fn()                                                                  # warm: code objects loaded, nothing cached is counted below
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        del out
        return peak - base

    fused = rise(lambda: ops.prob_head(c["tl"], c["win"], c["up"], c["pad"], c["hw"], qi, Q, SCALE, 0.0, 1))
    canvas = rise(lambda: canvas_route(c, qi, Q, 0.0, 1))
    out_bytes = Q * H * W * 4 + H * W * 8
    print(f"peak rise: fused {fused} B, canvas route {canvas} B, outputs {out_bytes} B, canvas {Q * H * W * 4} B")
    assert fused <= out_bytes + (1 << 20)
    assert canvas >= fused + Q * H * W * 4
