"""sg_boundary_band and sg_boundary_accumulate against tests/boundary_reference.py, exactly.

Small shapes: 1 x 1, 1 x 7, 7 x 1, 17 x 64, 64 x 65, 67 x 131 and 130 x 257 (one pixel, one row, one column, the 64-lane waves and
256-column groups of the column pass just passed, more than one row band), the widths 1, 2, 5, 40 and 300 (below a tile, above half the
image, above both sides), the maps of boundary_reference.patterns.  At 8 columns per lane these rows stay inside the first wave of the
row pass, so its other edges have cases of their own -- boundary_reference.WIDE_CASES, rows of 600, 2100 and 4100 columns with
H >= 2d + 1: runs that begin, end and straddle the lane (8), wave (512) and chunk (2048) edges, runs whose start reaches a later chunk
only through the carry, for bands and counts, uint8 and int64, reduce_zero_label on and off -- and one image of more rows than the row
pass has workgroups (2^20), which loops rows inside the kernel.
Also: uint8 and int64 truth with an ignored rectangle, values outside [0, K) in both maps, K = 1 and K = 127; three images of different
sizes and widths in one flat buffer; counts added to a non-zero table; byte-identical repeats; every refusal of the contract with the
outputs untouched; the identity with sg_confusion_accumulate at d = 300.  Every comparison is integer equality.
Not reached here: the second iteration of the count's grid-stride loop (above about 4 Mpix)."""
import ctypes

import numpy as np
import pytest
import torch

import boundary_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_BANDS = {}


def dev(m):
    return torch.from_numpy(np.ascontiguousarray(m)).to(DEV)


def ref_band(key, m, d):
    """The reference band of a map, computed once per (key, d) and left unchanged."""
    if (key, d) not in _BANDS:
        b = R.band(m, d)
        b.setflags(write=False)
        _BANDS[(key, d)] = b
    return _BANDS[(key, d)]


def areas_of(p, g, band_p, band_g, K, ignore_index):
    """The counts of the definition from reference bands (g already transformed)."""
    counted = g != ignore_index
    bp, bg = band_p.astype(bool), band_g.astype(bool)
    out = np.zeros((3, K), dtype=np.int64)
    for k in range(K):
        out[0, k] = np.count_nonzero(counted & (p == k) & (g == k) & bp & bg)
        out[1, k] = np.count_nonzero(counted & (p == k) & bp)
        out[2, k] = np.count_nonzero(counted & (g == k) & bg)
    return out


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_band_equals_the_reference(shape):
    from clip_decontamination_amd import ops
    H, W = shape
    inside = 0
    for d in R.WIDTHS:
        pats = R.patterns(H, W, d)
        want = {n: ref_band((H, W, n, d), m, d) for n, m in pats.items()}
        xs = [dev(m) for m in pats.values()]
        got = ops.boundary_band(xs, d)                                                  # every map of the width in one call
        for (n, m), x, g in zip(pats.items(), xs, got):
            assert g.dtype == torch.uint8 and g.shape == x.shape
            assert np.array_equal(g.cpu().numpy(), want[n]), (n, d)
            assert torch.equal(x, dev(m)), ("the input was written", n, d)
            inside += int((want[n] == 0).any())
        again = ops.boundary_band(xs, d)
        assert all(torch.equal(a, b) for a, b in zip(again, got)), ("repeat", d)
        for n in ("blocky", "vstripe_2d+1", "checker"):                                 # one map per call, int64 and uint8, [H,W] and [1,H,W]
            one = ops.boundary_band(dev(pats[n]), d)
            assert one.shape == (H, W) and np.array_equal(one.cpu().numpy(), want[n]), (n, d)
            u8 = ops.boundary_band(dev(pats[n].astype(np.uint8))[None], d)
            assert u8.shape == (1, H, W) and np.array_equal(u8[0].cpu().numpy(), want[n]), (n, d, "uint8")
        if d == 1:
            assert want["checker"].all()
    print(f"{H}x{W}: {inside} (map, width) pairs keep pixels out of the band")
    assert inside > 0 or min(H, W) < 3


def test_labels_are_raw_64_bit_values():
    """Values far outside [0, K), negative ones and ones that differ only above bit 32 are labels like any other."""
    from clip_decontamination_amd import ops
    m = R.patterns(33, 70, 2)["blocky"]
    for a, b in ((0, -1), (1, 1 << 40), (2, (1 << 32) + 2), (3, -(1 << 62))):
        m = np.where(m == a, b, m)
    m[10:20, 30:50] = 2                                                                  # next to (1 << 32) + 2: equal in the low 32 bits only
    assert np.array_equal(ops.boundary_band(dev(m), 2).cpu().numpy(), R.band(m, 2))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulate_equals_the_reference(shape):
    from clip_decontamination_amd import ops
    H, W = shape
    K = R.K
    moved = 0
    for d in R.WIDTHS:
        base = R.patterns(H, W, d)["blocky"]
        for fmt in (np.uint8, np.int64):
            p, g = R.truth_for(base, fmt, 31 * H + W)
            band_p = ref_band((H, W, "pred", fmt.__name__, d), p, d)
            for rzl in (False, True):
                gx = R.reduce_zero(g) if rzl else g.astype(np.int64)
                band_g = ref_band((H, W, "gt", fmt.__name__, rzl, d), gx, d)
                want = areas_of(p, gx, band_p, band_g, K, 255)
                start = torch.arange(3 * K, dtype=torch.int64, device=DEV).view(3, K) * 1000 + 7   # counts are ADDED to what is there
                areas = start.clone()
                out = ops.boundary_accumulate(dev(p).view(-1), dev(g).view(-1), [(H, W)], d, areas, K, 255, rzl)
                assert out is areas
                assert np.array_equal((areas - start).cpu().numpy(), want), (d, fmt.__name__, rzl)
                again = start.clone()
                ops.boundary_accumulate(dev(p).view(-1), dev(g).view(-1), [(H, W)], d, again, K, 255, rzl)
                assert torch.equal(again, areas), ("repeat", d, fmt.__name__, rzl)
                moved += int(want.any())
        # another ignore_index: 255 is then a label outside [0, K), and class 1 is ignored
        p, g = R.truth_for(base, np.int64, 5)
        want = areas_of(p, g, R.band(p, d), R.band(g, d), K, 1)
        areas = torch.zeros(3, K, dtype=torch.int64, device=DEV)
        ops.boundary_accumulate(dev(p).view(-1), dev(g).view(-1), [(H, W)], d, areas, K, 1, False)
        assert np.array_equal(areas.cpu().numpy(), want) and not want[2, 1], (d, "ignore_index=1")
    assert moved > 0


@pytest.mark.parametrize("case", R.WIDE_CASES, ids=lambda c: f"{c[0]}x{c[1]}_d{c[2]}")
def test_wide_rows_reach_every_edge_of_the_row_pass(case):
    """Waves 1 to 3 of the row pass (columns from 512), its second and third chunk (from 2048 and 4096) and the carry between them."""
    from clip_decontamination_amd import ops
    H, W, d = case
    pats = R.wide_patterns(H, W, d)
    want = {n: ref_band(("wide", H, W, n, d), m, d) for n, m in pats.items()}
    for n in pats:
        assert (want[n][d:H - d] == 0).any() and (want[n][d:H - d] == 1).any() or n in ("one_run",), n    # the centre rows tell
    got = ops.boundary_band([dev(m) for m in pats.values()], d)
    for n, g in zip(pats, got):
        bad = np.argwhere(g.cpu().numpy() != want[n])
        assert bad.size == 0, (n, "first wrong (y, x):", bad[:4].tolist())
    again = ops.boundary_band([dev(m) for m in pats.values()], d)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    got8 = ops.boundary_band([dev(m.astype(np.uint8)) for m in pats.values()], d)
    for n, g in zip(pats, got8):
        assert np.array_equal(g.cpu().numpy(), want[n]), (n, "uint8")
    # counts: prediction and truth both carry runs across the edges; the truth one class up so that reduce_zero_label brings it back
    K = R.K
    for fmt in (np.uint8, np.int64):
        for rzl in (False, True):
            p, g = R.truth_for(pats["random_runs"], fmt, W + d)
            if rzl:
                g = np.where(g.astype(np.int64) < K, g.astype(np.int64) + 1, g.astype(np.int64)).astype(fmt)
                g[:2, 506:520] = 0                                                       # raw zeros across the wave edge: ignored under reduce_zero_label
            gx = R.reduce_zero(g) if rzl else g.astype(np.int64)
            wanted = areas_of(p, gx, R.band(p, d), R.band(gx, d), K, 255)
            assert wanted[0].sum() > 0 and (wanted[0] < wanted[1]).any()
            areas = torch.zeros(3, K, dtype=torch.int64, device=DEV)
            ops.boundary_accumulate(dev(p).view(-1), dev(g).view(-1), [(H, W)], d, areas, K, 255, rzl)
            assert np.array_equal(areas.cpu().numpy(), wanted), (fmt.__name__, rzl)


def test_more_rows_than_row_workgroups():
    """An image of 2^20 + 1500 rows: the row pass loops rows inside a workgroup.  Three columns and d = 1, so the centre column shows
    what the row pass wrote; horizontal stripes of 1 to 6 rows."""
    from clip_decontamination_amd import ops
    H, W, d = (1 << 20) + 1500, 3, 1
    rng = np.random.default_rng(9)
    m = np.repeat(np.repeat(np.arange(H // 2) % 3, rng.integers(1, 7, H // 2))[:H, None], W, axis=1).astype(np.uint8)
    m[5::1000, 2] = 7                                                                    # rows that are not uniform
    assert m.shape == (H, W)
    want = R.band(m, d)
    assert (want[:, 1] == 0).sum() > H // 8 and want[(1 << 20) - 4:, 1].min() == 0       # rows out of the band beyond the first 2^20
    got = ops.boundary_band(dev(m), d).cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first wrong (y, x):", bad[:4].tolist())


@pytest.mark.parametrize("K", [1, 127])
def test_one_class_and_the_most_classes(K):
    from clip_decontamination_amd import ops
    H, W = 67, 131
    rng = np.random.default_rng(K)
    p = np.kron(rng.integers(0, K + 2, (H // 4 + 1, W // 4 + 1)), np.ones((4, 4), dtype=np.int64))[:H, :W]      # K and K + 1 are outside
    g = np.roll(p, (1, 2), axis=(0, 1)).astype(np.uint8)
    g[5:15, 40:90] = 255
    for d, rzl in ((1, False), (2, True), (300, False)):
        want = R.boundary_areas(p, g, d, K, 255, rzl)
        areas = torch.zeros(3, K, dtype=torch.int64, device=DEV)
        ops.boundary_accumulate(dev(p).view(-1), dev(g).view(-1), [(H, W)], d, areas, K, 255, rzl)
        assert np.array_equal(areas.cpu().numpy(), want), (K, d, rzl)
        assert want.sum() > 0


def test_three_images_in_one_flat_buffer():
    """Different sizes and widths at offsets that are no multiple of 8 or 16; the images never see each other: image n ends and image
    n + 1 begins with the same label."""
    from clip_decontamination_amd import ops
    shapes, ds, K = [(5, 7), (33, 70), (20, 13)], [1, 3, 40], R.K
    pairs = []
    for i, (H, W) in enumerate(shapes):
        p, g = R.truth_for(R.blocky(H, W, K, 5, 40 + i), np.uint8, 50 + i)
        p[-1, -1] = p[0, 0] = 2
        pairs.append((p, g))
    flat_p = dev(np.concatenate([p.reshape(-1) for p, _ in pairs]))
    flat_g = dev(np.concatenate([g.reshape(-1) for _, g in pairs]))
    bands = ops.boundary_band_flat(flat_p, shapes, ds)
    assert np.array_equal(bands.cpu().numpy(), np.concatenate([R.band(p, d).reshape(-1) for (p, _), d in zip(pairs, ds)]))
    bands_g = ops.boundary_band_flat(flat_g, shapes, ds)                                 # a uint8 buffer at odd byte offsets
    assert np.array_equal(bands_g.cpu().numpy(), np.concatenate([R.band(g, d).reshape(-1) for (_, g), d in zip(pairs, ds)]))
    per_map = ops.boundary_band([dev(p) for p, _ in pairs], ds)
    assert all(np.array_equal(b.cpu().numpy(), R.band(p, d)) for b, (p, _), d in zip(per_map, pairs, ds))
    for fmt in (torch.uint8, torch.int64):
        for rzl in (False, True):
            areas = torch.full((3, K), 3, dtype=torch.int64, device=DEV)
            ops.boundary_accumulate(flat_p, flat_g.to(fmt), shapes, ds, areas, K, 255, rzl)
            want = R.boundary_areas_batch(pairs, ds, K, 255, rzl)
            assert np.array_equal(areas.cpu().numpy() - 3, want), (fmt, rzl)
            assert want.all(axis=1).any() or want.sum() > 0


def test_wide_band_counts_equal_the_confusion_table():
    """d >= max(H, W): every pixel is in both bands and areas = (area_intersect, area_pred_label, area_label) of the confusion table."""
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
                areas = torch.zeros(3, K, dtype=torch.int64, device=DEV)
                ops.boundary_accumulate(dev(p).view(-1), dev(g).view(-1), [(H, W)], 300, areas, K, 255, rzl)
                assert np.array_equal(areas.cpu().numpy(), np.stack([inter, pred, label])), (H, W, fmt.__name__, rzl)


def test_metric_object_counts_both_tables():
    from clip_decontamination_amd import ops
    from clip_decontamination_amd.metrics import BoundaryIoUMetric, metrics_from_confusion
    K = R.K
    pairs = [R.truth_for(R.blocky(H, W, K, 6, 9 + H), np.uint8, H) for H, W in ((40, 50), (33, 70))]
    m = BoundaryIoUMetric(num_classes=K, boundary_px=2, iou_metrics=["mIoU", "mFscore"])
    m.add(dev(pairs[0][0]), dev(pairs[0][1])[None])
    m.add_flat(dev(pairs[1][0]).view(-1), pairs[1][1].reshape(-1), [(33, 70)])           # a host truth goes to the device
    table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=DEV)
    for p, g in pairs:
        ops.confusion_accumulate(dev(p).view(-1), dev(g).view(-1), table, K)
    assert torch.equal(m.confusion, table)
    want = R.boundary_areas_batch(pairs, [2, 2], K)
    assert np.array_equal(m.boundary_areas.cpu().numpy(), want)
    out = m.compute()
    plain = metrics_from_confusion(table, ["mIoU", "mFscore"])
    assert all(np.array_equal(out[k], plain[k], equal_nan=True) for k in plain if k != "summary")
    assert np.array_equal(out["BIoU"], R.biou(want), equal_nan=True)
    assert out["summary"] == dict(plain["summary"], mBIoU=float(np.round(np.nanmean(R.biou(want)) * 100, 2)))
    ratio = BoundaryIoUMetric(num_classes=K, boundary_ratio=0.05)                        # 0.05 of the diagonals: 3 and 4 px
    for p, g in pairs:
        ratio.add(dev(p), dev(g))
    assert np.array_equal(ratio.boundary_areas.cpu().numpy(), R.boundary_areas_batch(pairs, [R.width(p.shape, 0.05) for p, _ in pairs], K))
    assert [R.width(p.shape, 0.05) for p, _ in pairs] == [3, 4]


def test_refusals_leave_the_outputs_untouched():
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    H, W, K = 17, 64, R.K
    p, g = R.truth_for(R.patterns(H, W, 2)["blocky"], np.uint8, 1)
    lab, gt = dev(p).view(-1), dev(g).view(-1)
    band = torch.full((H * W,), 9, dtype=torch.uint8, device=DEV)
    areas = torch.full((3, K), 5, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(lib.sg_boundary_workspace_bytes(H * W)) + 256, dtype=torch.uint8, device=DEV)
    wp, wn = ops._aligned(ws)
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    P = ops.ptr

    def call_band(labels=P(lab), fmt=_lib.GT_I64, hw=(H, W), off=0, d=2, N=1, out=P(band), w=wp, n=wn, arrays=True):
        a = ((I32 * 2)(*hw), (I64 * 1)(off), (I32 * 1)(d)) if arrays else (None, None, None)
        return lib.sg_boundary_band(labels, fmt, *a, N, out, w, n, ops.stream_ptr())

    def call_acc(labels=P(lab), g_=P(gt), fmt=_lib.GT_U8, hw=(H, W), off=0, d=2, N=1, K_=K, a_=P(areas), w=wp, n=wn, arrays=True):
        a = ((I32 * 2)(*hw), (I64 * 1)(off), (I32 * 1)(d)) if arrays else (None, None, None)
        return lib.sg_boundary_accumulate(labels, g_, fmt, *a, N, K_, 255, 0, a_, w, n, ops.stream_ptr())

    refused = [lambda: call_band(labels=None), lambda: call_band(w=None), lambda: call_band(arrays=False), lambda: call_band(fmt=7),
               lambda: call_band(N=0), lambda: call_band(hw=(0, W)), lambda: call_band(hw=(H, -3)), lambda: call_band(hw=(1 << 16, 1 << 15)),
               lambda: call_band(d=0), lambda: call_band(d=4096), lambda: call_band(off=1), lambda: call_band(n=H * W - 1),
               lambda: call_acc(labels=None), lambda: call_acc(g_=None), lambda: call_acc(w=None), lambda: call_acc(arrays=False),
               lambda: call_acc(fmt=2), lambda: call_acc(N=0), lambda: call_acc(hw=(H, 0)), lambda: call_acc(hw=(1 << 15, 1 << 16)),
               lambda: call_acc(d=0), lambda: call_acc(d=4096), lambda: call_acc(K_=0), lambda: call_acc(K_=128),
               lambda: call_acc(n=4 * 1280 - 1)]
    for i, fn in enumerate(refused):
        assert fn() != 0, i
        err = lib.sg_last_error().decode()
        assert "sg_boundary_band" in err or "sg_boundary_accumulate" in err, err
    assert lib.sg_boundary_band(P(lab), _lib.GT_I64, (I32 * 2)(H, W), (I64 * 1)(0), (I32 * 1)(2), 1, None, wp, wn, ops.stream_ptr()) != 0
    assert lib.sg_boundary_accumulate(P(lab), P(gt), _lib.GT_U8, (I32 * 2)(H, W), (I64 * 1)(0), (I32 * 1)(2), 1, K, 255, 0, None, wp, wn,
                                      ops.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert (band == 9).all() and (areas == 5).all()
    assert call_band() == 0 and call_acc() == 0                                          # the same arguments, unrefused, do the work
    assert np.array_equal(band.cpu().numpy(), R.band(p, 2).reshape(-1))
    assert np.array_equal(areas.cpu().numpy() - 5, R.boundary_areas(p, g, 2, K))
