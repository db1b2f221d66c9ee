"""sg_tolerant_accumulate against tests/tolerant_reference.py, exactly.

Small shapes: 1 x 1, 1 x 7, 7 x 1, 17 x 64, 64 x 65, 67 x 131 and 130 x 257 (one pixel, one row, one column, a tile of the count of 8 rows
x 256 columns just passed in either direction, several tiles); tol_sq 0, 1, 2, 9, 10, 25, 1600 and 254^2 (no search, the non-square disk,
above half the image, the cap); both modes; uint8 and int64 truth with an ignored rectangle and values outside [0, K) in both maps;
reduce_zero_label on and off; K = 1, 5, 9 and 127 (the class-group loop runs once, twice and sixteen times, with matches in a later group).
At 8 columns per lane those rows stay inside the first wave of the row pass, so its other edges have cases of their own: rows of 600,
2100 and 4100 columns with marked runs that begin, end and straddle the lane (8), wave (512) and chunk (2048) edges, and single targets
exactly r and r + 1 columns across every such edge, to the left (reached only through the carry of the previous chunk) and to the right
(in the next chunk).  The walk of the count loads 8 rows above and below per batch: r = 1, 3 (inside the first batch), 5 (25), 40 (1600:
five batches) and 254 (the last batch ends inside the table) are all run, against images both lower and higher than the radius.
Also: three images of different sizes and tolerances in one flat buffer; counts added to a non-zero table; byte-identical repeats; inputs
unchanged; every refusal with the counts untouched; the identity with sg_confusion_accumulate at tol_sq = 0; another ignore_index.
Every comparison is integer equality.
One image of 2^16 + 300 rows and 3 columns has more rows than the row pass has workgroups (2^16), which loops rows inside the kernel, and
more tiles (8 230 of 8 rows) than the count has workgroups (8 per CU), which loops tiles inside the kernel.
Not reached here: a count tile loop of more than a few iterations per workgroup (maps of many Mpix; tools/bench_tolerant.py compares one
with the host route)."""
import ctypes

import numpy as np
import pytest
import torch

import tolerant_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = (R.REGION, R.CONTOUR)
_WANT = {}


def dev(m):
    return torch.from_numpy(np.ascontiguousarray(m)).to(DEV)


def want_for(key, p, g, tols, K, ignore_index, rzl, mode):
    """The reference tables of one input for all its tolerances, computed once per key and left unchanged."""
    key = (key, tuple(tols), K, ignore_index, rzl, mode)
    if key not in _WANT:
        w = R.counts_multi(p, g, tols, K, ignore_index, rzl, mode)
        for t in w.values():
            t.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def run(p, g, hw, tol, K, ignore_index=255, rzl=False, mode=R.REGION, start=None):
    from clip_decontamination_amd import ops
    counts = torch.zeros(4, K, dtype=torch.int64, device=DEV) if start is None else start.clone()
    out = ops.tolerant_accumulate(dev(p).view(-1), dev(g).view(-1), hw, tol, counts, K, ignore_index, rzl, mode)
    assert out is counts
    return counts


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counts_equal_the_reference(shape, mode):
    H, W = shape
    K = R.K
    pats = R.patterns(H, W, R.PATTERN_D)
    names = R.CPU_MAPS if H * W <= 64 * 65 else ("blocky", "blocky_fine", "vstripe_d+1")
    moved = 0
    start = torch.arange(4 * K, dtype=torch.int64, device=DEV).view(4, K) * 1000 + 7        # counts are ADDED to what is there
    for n in names:
        for fmt, rzl in ((np.uint8, False), (np.int64, True), (np.uint8, True), (np.int64, False)):
            if H * W > 64 * 65 and n != "blocky" and (fmt, rzl) in ((np.uint8, True), (np.int64, False)):
                continue                                                     # the largest shapes: the full cross on one map
            p, g = R.truth_for(pats[n], fmt, 31 * H + W)
            want = want_for((H, W, n, fmt.__name__), p, g, R.TOL_SQS, K, 255, rzl, mode)
            px, gx = dev(p).view(-1), dev(g).view(-1)
            for t in R.TOL_SQS:
                got = run(p, g, [(H, W)], t, K, 255, rzl, mode, start)
                bad = np.argwhere((got - start).cpu().numpy() != want[t])
                assert bad.size == 0, (n, fmt.__name__, rzl, t, "first wrong (row, class):", bad[:4].tolist(),
                                       (got - start).cpu().numpy().tolist(), want[t].tolist())
                assert torch.equal(run(p, g, [(H, W)], t, K, 255, rzl, mode, start), got), ("repeat", n, t)
            assert torch.equal(px, dev(p).view(-1)) and torch.equal(gx, dev(g).view(-1))
            moved += int(any(not np.array_equal(want[a], want[b]) for a, b in zip(R.TOL_SQS, R.TOL_SQS[1:])))
    assert moved > 0 or H * W < 8


def test_inputs_are_not_written():
    from clip_decontamination_amd import ops
    H, W, K = 33, 70, R.K
    p, g = R.truth_for(R.blocky(H, W, K, 5, 3), np.int64, 4)
    px, gx = dev(p).view(-1), dev(g).view(-1)
    p0, g0 = px.clone(), gx.clone()
    for mode in MODES:
        counts = torch.zeros(4, K, dtype=torch.int64, device=DEV)
        ops.tolerant_accumulate(px, gx, [(H, W)], 25, counts, K, 255, True, mode)
        assert np.array_equal(counts.cpu().numpy(), R.counts(p, g, 25, K, 255, True, mode))
    assert torch.equal(px, p0) and torch.equal(gx, g0)


def test_another_ignore_index_and_raw_64_bit_values():
    """ignore_index = 1: 255 is then a value outside [0, K) and class 1 is never a counted source; values that differ only above bit 32
    are different values for the contour."""
    H, W, K = 40, 77, R.K
    p, g = R.truth_for(R.blocky(H, W, K, 6, 8), np.int64, 5)
    g[20:30, 40:60] = (1 << 32) + 2
    g[22:28, 45:55] = 2
    for mode in MODES:
        for t in (0, 2, 25):
            want = R.counts(p, g, t, K, 1, False, mode)
            assert np.array_equal(run(p, g, [(H, W)], t, K, 1, False, mode).cpu().numpy(), want), (mode, t)
            assert not want[2, 1] and want[2, 2] > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.WIDE_TOL, ids=lambda c: f"{c[0]}x{c[1]}_t{c[2]}")
def test_wide_rows_reach_every_edge_of_the_row_pass(case, mode):
    """Waves 1 to 3 of the row pass (columns from 512), its second and third chunk (from 2048 and 4096) and the carries between them, in
    both directions."""
    H, W, t = case
    K = R.K
    r = int(np.sqrt(t))
    pats = R.wide_patterns(H, W, min(r, (H - 1) // 2))                       # its d only sets the widths of the runs
    names = ("edges", "straddle_2d+1", "start_before_chunk", "random_runs", "rows_differ") if H < 50 else ("edges", "random_runs", "rows_differ")
    for n in names:
        for fmt, rzl in ((np.uint8, False), (np.int64, True)):
            p, g = R.truth_for(pats[n], fmt, W + r)
            if rzl:                                                          # the truth one class up, so that reduce_zero_label brings it back
                g = np.where(g.astype(np.int64) < K, g.astype(np.int64) + 1, g.astype(np.int64)).astype(fmt)
                g[:2, 506:520] = 0                                           # raw zeros across the wave edge: ignored under reduce_zero_label
            want = want_for(("wide", H, W, n, fmt.__name__), p, g, [t], K, 255, rzl, mode)[t]
            got = run(p, g, [(H, W)], t, K, 255, rzl, mode).cpu().numpy()
            assert np.array_equal(got, want), (n, fmt.__name__, rzl, got.tolist(), want.tolist())
    hits = misses = 0
    Hc = min(H, 5)                                                           # the edges are those of a row: a few rows tell as much
    pairs = R.carry_pairs(Hc, W, t)
    for n, (p, g) in pairs.items():
        want = want_for(("carry", Hc, W, n), p, g, [t], 2, 255, False, mode)[t]
        got = run(p, g.astype(np.uint8), [(Hc, W)], t, 2, 255, False, mode).cpu().numpy()
        assert np.array_equal(got, want), (n, got.tolist(), want.tolist())
        if n.endswith("_hit"):
            assert want[1, 1] == want[0, 1] == 1 and want[3, 1] == want[2, 1] == 1, n
            hits += 1
        if n.endswith("_miss"):
            assert want[1, 1] == 0 and want[3, 1] == 0 and want[0, 1] == want[2, 1] == 1, n
            misses += 1
    assert hits == misses and hits >= 6 and ("left_2048_hit" in pairs) == (W > 2048 + r + 2) and ("right_512_miss" in pairs)


def test_more_rows_than_row_workgroups_and_more_tiles_than_count_workgroups():
    """2^16 + 300 rows of 3 columns: horizontal stripes of 1 to 6 rows, the truth moved down by 2 rows, some rows that are not uniform."""
    H, W, K = (1 << 16) + 300, 3, 3
    rng = np.random.default_rng(9)
    p = np.repeat(np.repeat(np.arange(H // 2) % 3, rng.integers(1, 7, H // 2))[:H, None], W, axis=1).astype(np.int64)
    assert p.shape == (H, W)
    p[5::1000, 2] = 1
    g = np.roll(p, 2, axis=0).astype(np.uint8)
    g[(1 << 16) - 50:(1 << 16) + 50, 1] = 255
    for mode in MODES:
        want = R.counts_multi(p, g, [1, 5], K, 255, False, mode)
        assert not np.array_equal(want[1], want[5]) and (want[1][1] < want[1][0]).all()
        tail = R.counts(p[1 << 16:], g[1 << 16:], 5, K, 255, False, mode)
        assert tail[1].sum() > 0                                                        # the rows beyond the first 2^16 take part
        for t in (1, 5):
            got = run(p, g, [(H, W)], t, K, 255, False, mode).cpu().numpy()
            assert np.array_equal(got, want[t]), (mode, t, got.tolist(), want[t].tolist())


@pytest.mark.parametrize("K", [1, 9, 127])
def test_class_groups(K):
    """K = 1: one plane; 9: a second group of one class; 127: sixteen groups, the last of 7.  Classes K and K + 1 are outside."""
    H, W = 64, 65
    rng = np.random.default_rng(K)
    p = np.kron(rng.integers(0, K + 2, (H // 4 + 1, W // 4 + 1)), np.ones((4, 4), dtype=np.int64))[:H, :W]
    g = np.roll(p, (1, 2), axis=(0, 1)).astype(np.uint8)
    g[5:15, 40:60] = 255
    for mode in MODES:
        for t, rzl in ((0, False), (4, False), (9, True), (1600, False)):
            want = R.counts(p, g, t, K, 255, rzl, mode)
            got = run(p, g, [(H, W)], t, K, 255, rzl, mode).cpu().numpy()
            assert np.array_equal(got, want), (K, mode, t, rzl)
            if t == 4 and K > 8:
                assert want[1, 8:].sum() > 0 and want[3, 8:].sum() > 0 and (want[1, 8:] < want[0, 8:]).any()   # a later group matches, and not all of it


def test_three_images_in_one_flat_buffer():
    """Different sizes and tolerances at offsets that are no multiple of 8 or 16; the images never see each other: image n ends and image
    n + 1 begins with the same label, and a tolerance far above the first image's size."""
    from clip_decontamination_amd import ops
    shapes, tols, K = [(5, 7), (33, 70), (20, 13)], [1600, 10, 2], R.K
    pairs = []
    for i, (H, W) in enumerate(shapes):
        p, g = R.truth_for(R.blocky(H, W, K, 5, 40 + i), np.uint8, 50 + i)
        p[-1, -1] = p[0, 0] = 2
        pairs.append((p, g))
    flat_p = dev(np.concatenate([p.reshape(-1) for p, _ in pairs]))
    flat_g = dev(np.concatenate([g.reshape(-1) for _, g in pairs]))
    for mode in MODES:
        for fmt in (torch.uint8, torch.int64):
            for rzl in (False, True):
                counts = torch.full((4, K), 3, dtype=torch.int64, device=DEV)
                ops.tolerant_accumulate(flat_p, flat_g.to(fmt), shapes, tols, counts, K, 255, rzl, mode)
                want = R.counts_batch(pairs, tols, K, 255, rzl, mode)
                assert np.array_equal(counts.cpu().numpy() - 3, want), (mode, fmt, rzl)
                assert want.sum() > 0
    one = torch.zeros(4, K, dtype=torch.int64, device=DEV)
    ops.tolerant_accumulate(flat_p, flat_g, shapes, 9, one, K)                           # one tolerance serves every image
    assert np.array_equal(one.cpu().numpy(), R.counts_batch(pairs, [9, 9, 9], K))


def test_zero_tolerance_equals_the_confusion_table():
    """tol_sq = 0 in region mode: rows 1 and 3 are area_intersect, rows 0 and 2 area_pred_label and area_label of
    sg_confusion_accumulate on the same inputs."""
    from clip_decontamination_amd import ops
    from clip_decontamination_amd.metrics import areas_from_confusion
    K = R.K
    for H, W in ((67, 131), (130, 257), (1, 7)):
        for fmt in (np.uint8, np.int64):
            p, g = R.truth_for(R.patterns(H, W, 5)["blocky"], fmt, H)
            for rzl in (False, True):
                table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=DEV)
                ops.confusion_accumulate(dev(p).view(-1), dev(g).view(-1), table, K, 255, rzl)
                inter, _, pred, label = areas_from_confusion(table)
                got = run(p, g, [(H, W)], 0, K, 255, rzl, R.REGION).cpu().numpy()
                assert np.array_equal(got, np.stack([pred, inter, label, inter])), (H, W, fmt.__name__, rzl)


def test_a_tolerance_above_the_diagonal():
    """tol_sq >= (H-1)^2 + (W-1)^2: a source is matched iff its class is marked anywhere in the other map."""
    K = R.K
    for H, W in ((64, 65), (130, 120)):
        p, g = R.truth_for(R.patterns(H, W, 3)["blocky"], np.uint8, H)
        p = np.where(p == 3, 4, p)                                                       # class 3 is absent from the prediction
        t = (H - 1) ** 2 + (W - 1) ** 2
        for mode in MODES:
            got = run(p, g, [(H, W)], t, K, 255, False, mode).cpu().numpy()
            assert np.array_equal(got[1], got[0]) and got[3, 3] == 0 and got[2, 3] > 0
            assert np.array_equal(got[3, [0, 1, 2, 4]], got[2, [0, 1, 2, 4]])
            assert np.array_equal(got, R.counts(p, g, t, K, 255, False, mode))


def test_metric_object_counts_both_tables():
    from clip_decontamination_amd import ops
    from clip_decontamination_amd.metrics import RelaxedMetric, metrics_from_confusion
    K = R.K
    pairs = [R.truth_for(R.blocky(H, W, K, 6, 9 + H), np.uint8, H) for H, W in ((40, 50), (33, 70))]
    table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=DEV)
    for p, g in pairs:
        ops.confusion_accumulate(dev(p).view(-1), dev(g).view(-1), table, K)
    plain = metrics_from_confusion(table, ["mIoU", "mFscore"])
    for mode, keys in ((R.REGION, ("RelPrecision", "RelRecall", "RelFscore", "mRelPrecision", "mRelRecall", "mRelFscore")),
                       (R.CONTOUR, ("BPrecision", "BRecall", "BFscore", "mBPrecision", "mBRecall", "mBF"))):
        m = RelaxedMetric(num_classes=K, tolerance_px=2, mode=mode, iou_metrics=["mIoU", "mFscore"])
        m.add(dev(pairs[0][0]), dev(pairs[0][1])[None])
        m.add_flat(dev(pairs[1][0]).view(-1), pairs[1][1].reshape(-1), [(33, 70)])       # a host truth goes to the device
        assert torch.equal(m.confusion, table)
        want = R.counts_batch(pairs, [4, 4], K, mode=mode)
        assert np.array_equal(m.tolerant_counts.cpu().numpy(), want)
        out = m.compute()
        assert all(np.array_equal(out[k], plain[k], equal_nan=True) for k in plain if k != "summary")
        for k, v in zip(keys[:3], R.scores(want)):
            assert np.array_equal(out[k], v, equal_nan=True), k
        assert out["summary"] == dict(plain["summary"], **{k: float(np.round(np.nanmean(v) * 100, 2)) for k, v in zip(keys[3:], R.scores(want))})
    ratio = RelaxedMetric(num_classes=K, tolerance_ratio=0.05)                           # 0.05 of the diagonals: 4 and 4 px
    for p, g in pairs:
        ratio.add(dev(p), dev(g))
    ts = [R.tolerance_sq(p.shape, 0.05) for p, _ in pairs]
    assert ts == [16, 16]
    assert np.array_equal(ratio.tolerant_counts.cpu().numpy(), R.counts_batch(pairs, ts, K))


def test_refusals_leave_the_counts_untouched():
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    H, W, K = 17, 64, R.K
    p, g = R.truth_for(R.patterns(H, W, 2)["blocky"], np.uint8, 1)
    lab, gt = dev(p).view(-1), dev(g).view(-1)
    counts = torch.full((4, K), 5, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(lib.sg_tolerant_workspace_bytes(H * W, K)) + 256, dtype=torch.uint8, device=DEV)
    wp, wn = ops._aligned(ws)
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    P = ops.ptr

    def call(labels=P(lab), g_=P(gt), fmt=_lib.GT_U8, hw=(H, W), off=0, t=9, N=1, K_=K, mode=0, c_=P(counts), w=wp, n=wn, arrays=True):
        a = ((I32 * 2)(*hw), (I64 * 1)(off), (I32 * 1)(t)) if arrays else (None, None, None)
        return lib.sg_tolerant_accumulate(labels, g_, fmt, *a, N, K_, mode, 255, 0, c_, w, n, ops.stream_ptr())

    refused = [lambda: call(labels=None), lambda: call(g_=None), lambda: call(w=None), lambda: call(arrays=False), lambda: call(fmt=2),
               lambda: call(mode=2), lambda: call(N=0), lambda: call(hw=(H, 0)), lambda: call(hw=(1 << 15, 1 << 16)), lambda: call(t=-1),
               lambda: call(t=254 * 254 + 1), lambda: call(K_=0), lambda: call(K_=128), lambda: call(off=1), lambda: call(n=5 * 1280 - 1)]
    for i, fn in enumerate(refused):
        assert fn() == -1, i
        assert "sg_tolerant_accumulate" in lib.sg_last_error().decode()
    assert call(c_=None) == -1
    torch.cuda.synchronize()
    assert (counts == 5).all()
    assert call() == 0                                                                   # the same arguments, unrefused, do the work
    assert np.array_equal(counts.cpu().numpy() - 5, R.counts(p, g, 9, K))
