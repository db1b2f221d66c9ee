"""ops.regions (sg_regions) against tests/regions_reference.py, exactly: every column of every row, ``counts`` and ``region_of``, on every
input of ``regions_reference.gpu_cases()`` (tests/test_regions_reference_cpu.py shows that these inputs tell every mutant of the
reference apart): every shape, pattern and connectivity of the sieve's input tables with min_area 1 / 5 / 64, with and without
skip_label, with a conf that holds ties of q, values outside [0, 1] and NaN; a checkerboard capped at 1, 1000 and total - 1 rows over a
table pre-filled with a sentinel; three images in one flat buffer; 70 images, more than one launch sequence holds; and one map whose
per-pixel workgroups outnumber SG_REGIONS_SCAN_BLOCKS, so that the scan's workgroup takes a second pass.  Every call is made twice
and compared byte for byte."""
import numpy as np
import pytest
import torch

import regions_reference as G
import sieve_reference as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -0x0123456789ABCDEF


def dev(m):
    return torch.from_numpy(np.ascontiguousarray(m)).to(DEV)


SPARE = 3


def raw(maps, conn, min_area, skip, confs, max_regions):
    """One raw sg_regions call with ``max_regions`` over a sentinel-filled table of max_regions + SPARE rows: the spare rows lie beyond
    what the call may write whatever the number of regions -> (table, counts [N+1], region_of flat), on the host."""
    from clip_decontamination_amd import ops
    flat = torch.cat([dev(m).reshape(-1) for m in maps])
    conf = None if confs is None else torch.cat([dev(c).reshape(-1) for c in confs])
    table = torch.full((max_regions + SPARE, ops.REGION_FIELDS), SENTINEL, dtype=torch.int64, device=DEV)
    region_of = torch.full((flat.numel(),), -7, dtype=torch.int32, device=DEV)
    counts = ops.regions_table(flat, [m.shape for m in maps], conf, conn, min_area, skip, max_regions, table, region_of)
    return table.cpu().numpy(), counts.cpu().numpy(), region_of.cpu().numpy()


def check_case(what, maps, conn, confs, options):
    """The raw entry (twice: byte-identical) and ops.regions against the reference, for every option of the case."""
    from clip_decontamination_amd import ops
    roots = [S.regions(m, conn) for m in maps]
    every = [G.all_rows(m, conn, None if confs is None else confs[n], root=roots[n]) for n, m in enumerate(maps)]
    xs = [dev(m) for m in maps]
    cs = None if confs is None else [dev(c) for c in confs]
    for min_area, skip, mx in options:
        tag = (what, conn, min_area, skip, mx)
        want, counts, region_of = G.assemble([(G.listed(r, min_area, skip), root) for r, root in every], mx)
        total = int(counts[-1])
        rows = mx if mx is not None else max(total, 1) + 2                     # uncapped: two rows inside max_regions that no region takes
        t, c, ro = raw(maps, conn, min_area, skip, confs, rows)
        assert len(t) == rows + SPARE and len(want) == min(total, rows), tag
        assert np.array_equal(c, counts), tag
        assert np.array_equal(t[:len(want)], want), tag
        assert (t[len(want):] == SENTINEL).all(), ("rows beyond the listed ones were written", tag)
        assert (t[rows:] == SENTINEL).all() and len(t[rows:]) == SPARE, ("rows at or beyond max_regions were written", tag)
        assert np.array_equal(ro, np.concatenate([v.reshape(-1) for v in region_of])), tag
        t2, c2, ro2 = raw(maps, conn, min_area, skip, confs, rows)
        assert t.tobytes() == t2.tobytes() and c.tobytes() == c2.tobytes() and ro.tobytes() == ro2.tobytes(), ("repeat", tag)
        # the Python surface: sliced, split into columns, centroid and score in double
        out = ops.regions(xs if len(xs) > 1 else xs[0], cs if cs is None or len(xs) > 1 else cs[0], conn, min_area, skip, mx, want_map=True)
        got = torch.stack([out[k] for k in ("image", "root", "label", "area")], 1).cpu().numpy()
        assert np.array_equal(got, want[:, :4]) and np.array_equal(out["bbox"].cpu().numpy(), want[:, G.Y0:G.X1 + 1]), tag
        assert np.array_equal(out["counts"].cpu().numpy(), counts[:-1]) and out.get("truncated", False) == (mx is not None and total > mx), tag
        area = want[:, G.AREA].astype(np.float64)
        assert np.array_equal(out["centroid"].cpu().numpy(), want[:, G.SUM_Y:G.SUM_X + 1].astype(np.float64) / area[:, None]), tag
        if cs is None:
            assert out["score"] is None
        else:
            assert np.array_equal(out["score_q"].cpu().numpy(), want[:, G.SCORE_Q]), tag
            assert np.array_equal(out["score"].cpu().numpy(), want[:, G.SCORE_Q].astype(np.float64) / float(1 << 24) / area), tag
        maps_of = out["region_of"] if len(xs) > 1 else [out["region_of"]]
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(maps_of, region_of)), tag
        assert all(torch.equal(x, dev(m)) for x, m in zip(xs, maps)), ("the input was written", tag)
    return len(options)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_regions_equal_the_reference(shape, connectivity):
    n = 0
    for what, maps, conn, confs, options in G.gpu_cases():
        if isinstance(what, tuple) and what[:2] == shape and conn == connectivity:
            n += check_case(what, maps, conn, confs, options)
    assert n == len(S.patterns(*shape)) * len(G.MIN_AREAS) * len(G.SKIPS)


@pytest.mark.parametrize("what", ["capped", "batch", "seventy"])
def test_capped_tables_and_batches(what):
    n = 0
    for w, maps, conn, confs, options in G.gpu_cases():
        if w == what:
            n += check_case(w, maps, conn, confs, options)
    assert n > 0


def test_max_regions_none_grows_to_the_exact_total():
    """More regions than the first call's rows: ops.regions calls once more with the exact total."""
    from clip_decontamination_amd import ops
    m = S.patterns(*G.CAP_SHAPE)["checkerboard"]
    first = ops.REGIONS_FIRST_ROWS
    ops.REGIONS_FIRST_ROWS = 1000
    try:
        out = ops.regions(dev(m), connectivity=4)
    finally:
        ops.REGIONS_FIRST_ROWS = first
    assert "truncated" not in out and out["root"].cpu().tolist() == list(range(m.size)) and int(out["counts"][0]) == m.size


def test_the_scan_takes_a_second_pass():
    """A map of more than SG_REGIONS_SCAN_BLOCKS workgroups of SG_REGIONS_BLOCK_PIXELS pixels: the scan's single workgroup carries its
    running offset from the first pass of its loop into the second.  Coarse blocks keep the reference fast; a speckle of single pixels
    beyond the first pass's pixels puts listed roots into workgroups of the second pass."""
    from clip_decontamination_amd import ops
    W = 2048
    H = ops.REGIONS_SCAN_BLOCKS * ops.REGIONS_BLOCK_PIXELS // W + 37
    assert -(-H * W // ops.REGIONS_BLOCK_PIXELS) > ops.REGIONS_SCAN_BLOCKS
    m = G.coarse_blocks(H, W)
    rng = np.random.default_rng(9)
    ys, xs = rng.integers(H - 36, H, 300), rng.integers(0, W, 300)
    m[ys, xs] = 7
    conf = np.random.default_rng(10).random((H, W), dtype=np.float32)
    rows, root = G.all_rows(m, 8, conf)
    second = rows[:, G.ROOT] >= ops.REGIONS_SCAN_BLOCKS * ops.REGIONS_BLOCK_PIXELS
    assert second.sum() > 100 and (~second).sum() > 100
    for min_area, skip in ((1, None), (2, 0)):
        want, counts, region_of = G.assemble([(G.listed(rows, min_area, skip), root)])
        out = ops.regions(dev(m), dev(conf), 8, min_area, skip, want_map=True)
        got = torch.stack([out[k] for k in ("image", "root", "label", "area")], 1).cpu().numpy()
        assert np.array_equal(got, want[:, :4]) and np.array_equal(out["bbox"].cpu().numpy(), want[:, G.Y0:G.X1 + 1])
        assert np.array_equal(out["score_q"].cpu().numpy(), want[:, G.SCORE_Q])
        assert np.array_equal(out["centroid"].cpu().numpy(), want[:, G.SUM_Y:G.SUM_X + 1] / want[:, G.AREA].astype(np.float64)[:, None])
        assert int(out["counts"][0]) == counts[0] and np.array_equal(out["region_of"].cpu().numpy(), region_of[0])


def test_shapes_and_refusals():
    from clip_decontamination_amd import ops
    m = S.patterns(33, 70)["blocky"]
    x = dev(m)
    a, b = ops.regions(x), ops.regions(x[None])
    assert all(torch.equal(a[k], b[k]) for k in ("image", "root", "label", "area", "bbox", "centroid", "counts")) and a["score"] is None
    assert a["bbox"].shape == (a["root"].numel(), 4) and a["centroid"].dtype == torch.float64 and a["counts"].shape == (1,)
    f = ops.regions_flat(x.view(-1), [m.shape])
    assert torch.equal(f["root"], a["root"]) and torch.equal(f["bbox"], a["bbox"])
    with pytest.raises(TypeError, match="int64"):
        ops.regions(x.to(torch.int32))
    with pytest.raises(ValueError, match="min_area"):
        ops.regions(x, min_area=0)
    with pytest.raises(ValueError, match="connectivity"):
        ops.regions(x, connectivity=6)
    with pytest.raises(ValueError, match="conf"):
        ops.regions(x, conf=torch.zeros(3, 3, device=DEV))
    with pytest.raises(ValueError, match="images of sizes"):
        ops.regions_flat(x.view(-1), [(33, 69)])
