"""sg_object_match against tests/object_reference.py, exactly.

Shapes 1 x 1, 1 x 7, 7 x 1, 17 x 64, 64 x 65, 67 x 131 and 130 x 257 (one pixel, one row, one column, a labelling tile of 64 x 16 just
passed in either direction, several tiles); both connectivities; thresholds 1/2, 3/4 and (2^20 - 1) / 2^20; min_area 1 and 5; with and
without skip_label; uint8 and int64 truth with an ignored rectangle and values outside [0, K) in both maps; reduce_zero_label on and off;
ignore_index = 1; K = 1, 5 and 127.  Maps: blocks against themselves moved by (1, 2), per-pixel noise, the hand-worked pairs of
tests/test_object_reference_cpu.py at the corners of the labelling tiles, one 300 x 300 map whose single object spans every tile against a
truth with a hole (counters above 2^16, one word hit from every workgroup), a flat 512 x 512 map against itself.  match_map is compared
byte for byte, and leaving it out gives the same counts.  Also: three images of different sizes in one flat buffer, 65 images of 3 x 5 (a
second launch sequence), counts added to a non-zero table, byte-identical repeats, inputs unchanged, every refusal with counts and
match_map untouched.  Every comparison is integer equality.
The vote sweeps 32 768 pixels per workgroup through a cache of 64 pairs: 130 x 257, 300 x 300 and 512 x 512 take several such workgroups,
the noise maps overflow the list and evict from the cache in every chunk, the 65 tiny images take one workgroup each.
Not reached here: maps of many Mpix (tools/bench_object.py compares one with the host route)."""
import ctypes

import numpy as np
import pytest
import torch

import object_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = list(R.gpu_cases())


def dev(m):
    return torch.from_numpy(np.ascontiguousarray(m)).to(DEV)


def flat_of(pairs):
    p = dev(np.concatenate([a.reshape(-1) for a, _ in pairs]))
    g = dev(np.concatenate([b.reshape(-1) for _, b in pairs]))
    return p, g, [tuple(a.shape) for a, _ in pairs]


def run(p, g, hw, K, iou, conn, area, skip, ign=255, rzl=False, start=None, want_map=True):
    from clip_decontamination_amd import ops
    counts = torch.zeros(4, K, dtype=torch.int64, device=DEV) if start is None else start.clone()
    mm = torch.full((p.numel(),), 0xEE, dtype=torch.uint8, device=DEV) if want_map else None
    out = ops.object_match(p, g, hw, counts, K, iou, conn, area, skip, ign, rzl, mm)
    assert out is counts
    return counts, mm


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c[0]) if isinstance(c[0], tuple) else c[0])
def test_counts_and_map_equal_the_reference(case):
    what, pairs, K, rzl, ign, params = case
    p, g, hw = flat_of(pairs)
    p0, g0 = p.clone(), g.clone()
    start = torch.arange(4 * K, dtype=torch.int64, device=DEV).view(4, K) * 1000 + 7            # counts are ADDED to what is there
    for i, (iou, conn, area, skip) in enumerate(params):
        want, want_maps, _ = R.match_batch(pairs, K, iou, connectivity=conn, min_area=area, skip_label=skip, ignore_index=ign, rzl=rzl)
        got, mm = run(p, g, hw, K, iou, conn, area, skip, ign, rzl, start)
        delta = (got - start).cpu().numpy()
        bad = np.argwhere(delta != want)
        assert bad.size == 0, (what, iou, conn, area, skip, "first wrong (row, class):", bad[:4].tolist(), delta.tolist(), want.tolist())
        wm = np.concatenate([m.reshape(-1) for m in want_maps])
        diff = np.flatnonzero(mm.cpu().numpy() != wm)
        assert diff.size == 0, (what, iou, conn, area, skip, "first wrong pixels:", diff[:6].tolist(), mm.cpu().numpy()[diff[:6]].tolist(),
                                wm[diff[:6]].tolist())
        if i % 3 == 0:
            again, mm2 = run(p, g, hw, K, iou, conn, area, skip, ign, rzl, start)
            assert torch.equal(again, got) and torch.equal(mm2, mm), ("repeat", what, iou)
            nomap, none = run(p, g, hw, K, iou, conn, area, skip, ign, rzl, start, want_map=False)
            assert none is None and torch.equal(nomap, got), ("without match_map", what, iou)
    assert torch.equal(p, p0) and torch.equal(g, g0)


def test_the_hand_worked_pairs_one_by_one():
    for name, (p, g, want) in R.hand_maps().items():
        for iou, tp in want.items():
            got, mm = run(dev(p).view(-1), dev(g.astype(np.uint8)).view(-1), [p.shape], 3, iou, 4, 1, R.BG)
            ref, ref_map, _ = R.match(p, g, 3, iou, skip_label=R.BG)
            assert np.array_equal(got.cpu().numpy(), ref) and int(got[0].sum()) == tp, (name, iou, got.tolist())
            assert np.array_equal(mm.cpu().numpy().reshape(p.shape), ref_map), (name, iou)


def test_the_spanning_object_passes_two_to_the_sixteen():
    p, g = R.spanning()
    got, mm = run(dev(p).view(-1), dev(g).view(-1), [p.shape], 2, (1, 2), 4, 1, None)
    # |p| = 299 * 300; the truth's large object has 300 * 300 - 60 * 80 pixels, 300 of them in the row the prediction leaves out
    I, U = 300 * 300 - 60 * 80 - 300, 300 * 300
    ref = R.match(p, g, 2, (1, 2))[0]
    assert I > 1 << 16 and ref[:, 1].tolist() == [1, 1, 2, (I << 24) // U] and ref[:, 0].tolist() == [0, 1, 1, 0]
    assert np.array_equal(got.cpu().numpy(), ref)
    assert int(mm.view(300, 300)[130, 160]) == 1 + 8 and int(mm[0]) == 2 + 4 and int(mm.view(300, 300)[110, 130]) == 1 + 8


def test_the_matched_roots_join_the_region_table():
    """A root pixel's byte of match_map tells whether its region is matched: the join with sg_regions rows the header promises."""
    from clip_decontamination_amd import ops
    p, g, _ = R.hand_embedded()
    _, mm = run(dev(p).view(-1), dev(g.astype(np.uint8)).view(-1), [p.shape], 3, (1, 2), 4, 1, R.BG)
    rows = ops.regions(dev(p), connectivity=4, skip_label=R.BG)
    roots = rows["root"].cpu().numpy()
    matched = sorted(int(r) for r in roots if mm.cpu().numpy()[r] & 1)
    _, _, pairs = R.match(p, g, 3, (1, 2), skip_label=R.BG)
    assert matched == sorted(a for a, _ in pairs) and len(matched) > 0


def test_metric_object_counts_both_tables():
    from clip_decontamination_amd import ops
    from clip_decontamination_amd.metrics import ObjectMetric, metrics_from_confusion
    K = R.K
    pairs = R.three_images()[1:]
    table = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=DEV)
    for p, g in pairs:
        ops.confusion_accumulate(dev(p).view(-1), dev(g).view(-1), table, K)
    plain = metrics_from_confusion(table, ["mIoU", "mFscore"])
    m = ObjectMetric(num_classes=K, object_iou=0.5, min_area=2, connectivity=8, skip_label=R.BG, iou_metrics=["mIoU", "mFscore"])
    mm = torch.zeros(pairs[0][0].size, dtype=torch.uint8, device=DEV)
    m.add(dev(pairs[0][0]), dev(pairs[0][1])[None], match_map=mm)
    m.add_flat(dev(pairs[1][0]).view(-1), pairs[1][1].reshape(-1), [pairs[1][0].shape])       # a host truth goes to the device
    assert torch.equal(m.confusion, table)
    want, maps, _ = R.match_batch(pairs, K, (1, 2), connectivity=8, min_area=2, skip_label=R.BG)
    assert np.array_equal(m.object_counts.cpu().numpy(), want) and want[0].sum() > 0
    assert np.array_equal(mm.cpu().numpy(), maps[0].reshape(-1))
    out = m.compute()
    assert all(np.array_equal(out[k], plain[k], equal_nan=True) for k in plain if k != "summary")
    keys = ("ObjPrecision", "ObjRecall", "ObjF1", "SQ", "PQ")
    for k, v in zip(keys, R.scores(want)):
        assert np.array_equal(out[k], v, equal_nan=True), k
    assert out["summary"] == dict(plain["summary"], **{"m" + k: float(np.round(np.nanmean(v) * 100, 2)) for k, v in zip(keys, R.scores(want))})


def test_refusals_leave_counts_and_map_untouched():
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    H, W, K = 17, 64, R.K
    p, g = R.truth_for(R.blocky(H, W, K, 6, 1), np.uint8)
    lab, gt = dev(p).view(-1), dev(g).view(-1)
    counts = torch.full((4, K), 5, dtype=torch.int64, device=DEV)
    mm = torch.full((H * W,), 0x5A, dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(lib.sg_object_workspace_bytes(H * W)) + 256, dtype=torch.uint8, device=DEV)
    wp, wn = ops._aligned(ws)
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    P = ops.ptr

    def call(labels=P(lab), g_=P(gt), fmt=_lib.GT_U8, hw=(H, W), off=0, N=1, K_=K, conn=4, area=1, iou=(1, 2), c_=P(counts), m_=P(mm), w=wp, n=wn,
             arrays=True):
        a = ((I32 * 2)(*hw), (I64 * 1)(off)) if arrays else (None, None)
        return lib.sg_object_match(labels, g_, fmt, *a, N, K_, conn, area, 0, 0, iou[0], iou[1], 255, 0, c_, m_, w, n, ops.stream_ptr())

    refused = [lambda: call(labels=None), lambda: call(g_=None), lambda: call(w=None), lambda: call(arrays=False), lambda: call(fmt=2),
               lambda: call(N=0), lambda: call(hw=(H, 0)), lambda: call(hw=(1 << 15, 1 << 16)), lambda: call(K_=0), lambda: call(K_=128),
               lambda: call(conn=6), lambda: call(area=0), lambda: call(iou=(1, 3)), lambda: call(iou=(2, 2)), lambda: call(iou=(0, 1)),
               lambda: call(iou=(1 << 20, (1 << 20) + 1)), lambda: call(off=1), lambda: call(n=36 * H * W + 2 * 1280 - 1),
               lambda: call(labels=ctypes.c_void_p(lab.data_ptr() + 4))]
    for i, fn in enumerate(refused):
        assert fn() == -1, i
        assert "sg_object_match" in lib.sg_last_error().decode()
    assert call(c_=None) == -1
    torch.cuda.synchronize()
    assert (counts == 5).all() and (mm == 0x5A).all()
    assert call() == 0                                                                   # the same arguments, unrefused, do the work
    want, wm, _ = R.match(p, g, K, (1, 2))
    assert np.array_equal(counts.cpu().numpy() - 5, want) and np.array_equal(mm.cpu().numpy(), wm.reshape(-1))
