"""The packed-batch planner (pipeline.plan_images): pure host logic, no device."""
import pytest

from clip_decontamination_amd.pipeline import launch_chunks, plan_images, tile_windows

SHAPES = [(512, 512), (100, 37), (768, 512), (150, 200), (512, 512), (100, 37)]


def test_windows_per_image_match_tile_windows():
    groups = plan_images(SHAPES, 112, 224, 16, 32)
    seen = set()
    for g in groups:
        for k, i in enumerate(g.images):
            H, W = SHAPES[i]
            wins = tile_windows(H, W, (112, 112), (224, 224))
            a, n = g.first_tile[k], g.n_tiles[k]
            assert g.windows[a:a + n] == wins
            assert g.tile_image[a:a + n] == [i] * n
            assert all((y2 - y1, x2 - x1) == g.tile_hw for y1, y2, x1, x2 in wins)
            seen.add(i)
    assert seen == set(range(len(SHAPES)))
    # image-major order: the tiles of a group are its images' windows back to back
    for g in groups:
        assert g.first_tile == [sum(g.n_tiles[:k]) for k in range(len(g.images))]
        assert len(g.windows) == sum(g.n_tiles)


def test_tile_size_groups():
    groups = plan_images(SHAPES, 112, 224, 16, 32)
    by = {g.tile_hw: g.images for g in groups}
    assert by[(224, 224)] == [0, 2, 4]                 # 512^2 and 768x512 share the crop
    assert by[(100, 37)] == [1, 5]                     # smaller than the crop: the whole image, its own group
    assert by[(150, 200)] == [3]
    assert [g.tile_hw for g in groups] == [(224, 224), (100, 37), (150, 200)]   # order of first appearance
    assert by and groups[0].grids == [(4, 4), (6, 4), (4, 4)]


def test_chunks_equal_across_image_boundaries():
    shapes = [(512, 512)] * 12                          # 16 windows each: 192 tiles
    g, = plan_images(shapes, 112, 224, 16, 40)
    assert g.chunks == launch_chunks(192, 40)
    sizes = [b - a for a, b in g.chunks]
    assert max(sizes) - min(sizes) <= 1 and len(sizes) == 5
    assert any(a % 16 for a, _ in g.chunks)            # a chunk starts inside an image: launches cross image boundaries
    assert g.chunks[0][0] == 0 and g.chunks[-1][1] == 192
    assert all(g.chunks[k][1] == g.chunks[k + 1][0] for k in range(len(g.chunks) - 1))


def test_canvas_offsets_are_a_prefix_sum():
    groups = plan_images(SHAPES, 112, 224, 16, 32)
    for g in groups:
        acc = [0]
        for H, W in g.shapes:
            acc.append(acc[-1] + H * W)
        assert g.canvas_offsets == acc
        assert g.shapes == [SHAPES[i] for i in g.images]


def test_flush_groups_respect_the_bound_and_never_split_an_image():
    shapes = [(512, 512), (768, 512), (512, 512), (512, 512), (600, 700)]
    tb, pb = 1000, 4
    bound = 16 * tb + 512 * 512 * pb + 24 * tb + 768 * 512 * pb      # exactly the first two images
    g, = plan_images(shapes, 112, 224, 16, 20, tile_bytes=lambda thw: tb, pixel_bytes=pb, flush_bytes=bound)
    fl = g.flush
    assert fl[0].img_lo == 0 and fl[-1].img_hi == len(shapes)
    for f, nxt in zip(fl, fl[1:]):
        assert f.img_hi == nxt.img_lo and f.tile_hi == nxt.tile_lo
    assert (fl[0].img_lo, fl[0].img_hi) == (0, 2)
    for f in fl:
        need = sum(tb * g.n_tiles[k] + pb * g.shapes[k][0] * g.shapes[k][1] for k in range(f.img_lo, f.img_hi))
        assert need <= bound or f.img_hi - f.img_lo == 1
        assert f.tile_lo == g.first_tile[f.img_lo]
        assert f.tile_hi == g.first_tile[f.img_hi - 1] + g.n_tiles[f.img_hi - 1]      # whole images only
        assert f.chunks == [(f.tile_lo + a, f.tile_lo + b) for a, b in launch_chunks(f.tile_hi - f.tile_lo, 20)]
    # an image larger than the bound is a flush group of its own
    g2, = plan_images([(512, 512)] * 3, 112, 224, 16, 20, tile_bytes=tb, pixel_bytes=pb, flush_bytes=10)
    assert [(f.img_lo, f.img_hi) for f in g2.flush] == [(0, 1), (1, 2), (2, 3)]
    # no bound: one flush group holding the whole group, chunked as the group
    g3, = plan_images(shapes, 112, 224, 16, 20)
    assert len(g3.flush) == 1 and g3.flush[0].chunks == g3.chunks


def test_rejects_empty_images():
    with pytest.raises(ValueError):
        plan_images([(0, 10)], 112, 224, 16, 8)
