"""ops.sieve (sg_sieve) against tests/sieve_reference.py, exactly (torch.equal): every shape, pattern, connectivity, fill and min_region
of the reference's input tables, out of place, in place, and each of the two a second time (byte-identical repeats); a batch of three
images in one flat buffer whose neighbours in the buffer share a label; and more images than one launch sequence holds.

The kernels' LDS tile is 64 x 16: the shapes 5 x 64, 4 x 65, 33 x 70, 67 x 131 and 130 x 257 sit on, one above and one below its
multiples in both dimensions; tests/test_sieve_reference_cpu.py shows that these inputs tell every mutant of the reference apart."""
import numpy as np
import pytest
import torch

import sieve_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(m):
    return torch.from_numpy(np.ascontiguousarray(m)).to(DEV)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sieve_equals_the_reference(shape, connectivity):
    from clip_decontamination_amd import ops
    H, W = shape
    checked = changed = 0
    for name, m in R.patterns(H, W).items():
        root = R.regions(m, connectivity)
        x = dev(m)
        for fill in R.FILLS:
            for mr in R.MIN_REGIONS:
                mr = R.min_region_of(mr, H, W)
                want = dev(R.sieve(m, mr, connectivity, fill, R.BG, root=root))
                what = (name, fill, mr)
                out = ops.sieve(x, mr, connectivity, fill, R.BG)                               # out of place
                assert out.dtype == torch.int64 and out.shape == x.shape and out.data_ptr() != x.data_ptr()
                assert torch.equal(out, want), what
                assert torch.equal(x, dev(m)), ("the input was written", what)
                again = ops.sieve(x, mr, connectivity, fill, R.BG)
                assert torch.equal(again, out), ("repeat", what)
                for _ in range(2):                                                             # in place, twice on fresh copies
                    y = x.clone()
                    assert ops.sieve(y, mr, connectivity, fill, R.BG, out=y) is y
                    assert torch.equal(y, want), ("in place", what)
                if mr == 1:
                    assert torch.equal(out, x), ("min_region = 1 returns the input", what)
                checked += 1
                changed += int(not torch.equal(want, x))
    print(f"{H}x{W} connectivity {connectivity}: {checked} settings equal the reference, {changed} of them change the map")
    assert changed > 0 or H * W == 1


def test_one_h_w_maps_and_out_tensors():
    from clip_decontamination_amd import ops
    m = R.patterns(33, 70)["iid3"]
    want = dev(R.sieve(m, 5, 8, "neighbour", R.BG))
    x = dev(m)
    out3 = ops.sieve(x[None], 5, 8, "neighbour", R.BG)
    assert out3.shape == (1, 33, 70) and torch.equal(out3[0], want)
    dst = torch.full_like(x, -1)
    assert ops.sieve(x, 5, 8, "neighbour", R.BG, out=dst) is dst and torch.equal(dst, want)
    with pytest.raises(TypeError):
        ops.sieve(x.to(torch.int32), 5)
    with pytest.raises(ValueError, match="min_region"):
        ops.sieve(x, 0)
    with pytest.raises(ValueError, match="connectivity"):
        ops.sieve(x, 5, connectivity=6)
    with pytest.raises(ValueError, match="fill"):
        ops.sieve(x, 5, fill="nearest")


@pytest.mark.parametrize("connectivity", [4, 8])
def test_batch_in_one_flat_buffer(connectivity):
    """Image n ends and image n + 1 begins with the same label, in regions that are small alone and kept together."""
    from clip_decontamination_amd import ops
    maps = R.batch_maps()
    xs = [dev(m) for m in maps]
    for fill in R.FILLS:
        for mr in (1, 2, 5, 64):
            want = [dev(w) for w in R.sieve_batch(maps, mr, connectivity, fill, R.BG)]
            got = ops.sieve(xs, mr, connectivity, fill, R.BG)
            single = [ops.sieve(x, mr, connectivity, fill, R.BG) for x in xs]
            assert isinstance(got, list) and len(got) == 3
            for g, s, w, x in zip(got, single, want, xs):
                assert g.shape == x.shape and torch.equal(g, w) and torch.equal(s, w), (fill, mr)
            flat = torch.cat([x.reshape(-1) for x in xs])
            ops.sieve_flat(flat, [m.shape for m in maps], mr, connectivity, fill, R.BG)         # the pipeline's form: in place on the flat buffer
            assert torch.equal(flat, torch.cat([w.reshape(-1) for w in want])), (fill, mr)
    mixed = ops.sieve([xs[0], xs[1][None]], 5, connectivity, "bg", R.BG)                       # [H,W] and [1,H,W] in one list
    assert mixed[0].shape == xs[0].shape and mixed[1].shape == (1,) + tuple(xs[1].shape)


def test_more_images_than_one_launch_sequence():
    """70 small images in one call: the library serves 64 images per launch sequence, so the last six take a second one."""
    from clip_decontamination_amd import ops
    rng = np.random.default_rng(11)
    maps = [rng.integers(0, 3, (int(rng.integers(1, 20)), int(rng.integers(1, 80)))).astype(np.int64) for _ in range(70)]
    for connectivity, fill in ((4, "neighbour"), (8, "bg")):
        want = R.sieve_batch(maps, 4, connectivity, fill, R.BG)
        got = ops.sieve([dev(m) for m in maps], 4, connectivity, fill, R.BG)
        assert all(torch.equal(g, dev(w)) for g, w in zip(got, want))
