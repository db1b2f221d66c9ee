"""CPU checks of tests/blend_reference.py, the float64 reference that tests/test_gpu_blend.py holds sg_stitch_blend and
sg_label_head_blend to: the ramp tables, the uniform special case, the partition of unity, that the f32 emulation of the kernel lies
within the bound while every listed slip breaks it, what blending does to a seam, and that every label-head case of the GPU test leaves
at most head_reference.CAP of its pixels uncounted."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_reference as BR  # noqa: E402
import head_reference as HR  # noqa: E402


def test_ramp_values():
    f = np.float32
    assert BR.ramp("linear", 1).tolist() == [0.5, 1.0]
    assert BR.ramp("linear", 2).tolist() == [0.25, 0.75, 1.0]
    assert BR.ramp("linear", 5).tolist() == [f(0.1), f(0.3), f(0.5), f(0.7), f(0.9), 1.0]
    assert BR.ramp("hann", 1).tolist() == [f(math.sin(math.pi / 4) ** 2), 1.0]                  # 0.5 up to the rounding of sin
    assert abs(float(BR.ramp("hann", 1)[0]) - 0.5) < 1e-7
    h2 = BR.ramp("hann", 2)
    assert h2.dtype == np.float32 and h2.shape == (3,) and h2[2] == 1.0
    assert abs(float(h2[0]) - 0.14644660940672624) < 1e-8 and abs(float(h2[1]) - 0.8535533905932737) < 6e-8    # (2 -+ sqrt 2) / 4
    for kind in BR.KINDS:
        for R in (1, 3, 16, 256, 2047):
            r = BR.ramp(kind, R)
            assert r.shape == (R + 1,) and r[-1] == 1.0 and np.all(r > 0) and np.all(np.isfinite(r)) and np.all(np.diff(r) > 0)


def test_the_host_table_is_the_reference_table():
    from clip_decontamination_amd import ops
    for kind in BR.KINDS:
        for R in (1, 2, 5, 16, 20, 257):
            assert np.array_equal(ops.blend_ramp(kind, R).numpy(), BR.ramp(kind, R)), (kind, R)
    assert ops.blend_ramp("uniform", None).tolist() == [1.0]
    assert ops.BLEND_MAX_RAMP == 2048


@pytest.mark.parametrize("name", BR.STITCH_GEOMETRIES)
def test_a_one_entry_ramp_is_the_plain_mean(name):
    for Q in (1, 9):
        c = BR.stitch_case(name, Q)
        args = (c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
        assert np.abs(BR.stitch_blend(*args, BR.UNIFORM) - HR.stitch(*args)).max() == 0.0
        assert np.array_equal(BR.stitch_blend_emulate(*args, BR.UNIFORM), HR.stitch_emulate(*args))


def test_hann_over_half_the_crop_is_a_partition_of_unity():
    wins = HR.slide_windows(96, 96, 16, 32)
    ws = BR.weight_sum(wins, (96, 96), BR.ramp("hann", 16))
    assert np.abs(ws[16:80, 16:80] - 1.0).max() < 1e-7
    assert ws.min() == ws[0, 0] == ws[95, 95] and 5.7e-6 < ws.min() < 5.9e-6          # a corner: one tile, r[0]^2, cancels in the division


@pytest.mark.parametrize("name", BR.STITCH_GEOMETRIES)
def test_the_emulation_lies_within_the_bound(name):
    worst = 0.0
    for Q in BR.STITCH_Q:
        c = BR.stitch_case(name, Q)
        args = (c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
        ups = BR.upsampled(c["tile_logits"], c["up_hw"])
        for kind, R in BR.stitch_ramps(name):
            r = BR.ramp(kind, R)
            worst = max(worst, HR.within(BR.stitch_blend_emulate(*args, r), BR.stitch_blend(*args, r, ups),
                                         BR.stitch_blend_bound(*args, r, ups), f"{name} Q={Q} {kind} R={R}"))
    print(f"{name}: largest err / bound {worst:.3f}")


def _band(c, a, b):
    tl, wb, hw = BR.band_of(c, a, b)
    return (tl, wb, c["up_hw"], c["pad_tl"], hw)


# mutant -> (geometry, Q, ramp, band rows or None): the case on which it has to leave the bound
MUTANT_CASES = {"start_only": ("a", 8, ("hann", 20), None), "canvas_coords": ("a", 8, ("hann", 20), (25, 45)),
                "div_count": ("b", 9, ("hann", 22), None), "no_clamp": ("a", 8, ("linear", 5), None)}


@pytest.mark.parametrize("mut", BR.MUTANTS)
def test_every_mutant_breaks_the_bound(mut):
    name, Q, (kind, R), band = MUTANT_CASES[mut]
    c = BR.stitch_case(name, Q)
    args = _band(c, *band) if band else (c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
    r = BR.ramp(kind, R)
    ref, bound = BR.stitch_blend(*args, r), BR.stitch_blend_bound(*args, r)
    HR.within(BR.stitch_blend_emulate(*args, r), ref, bound, f"{mut}: the unmutated emulation")
    with pytest.raises(AssertionError):
        HR.within(BR.stitch_blend_emulate(*args, r, mut=mut), ref, bound, mut)


def test_a_band_is_the_rows_of_the_whole_canvas():
    """The weights depend on the position inside the tile's own window, so the shifted windows of a band give the same bytes."""
    c = BR.stitch_case("a", 9)
    r = BR.ramp("hann", 20)
    whole = BR.stitch_blend_emulate(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"], r)
    for a, b in ((0, 13), (25, 45), (41, 70)):
        assert np.array_equal(BR.stitch_blend_emulate(*_band(c, a, b), r), whole[:, a:b])


def test_blending_takes_the_step_out_of_a_seam():
    """Constant tiles c_t at 50 % overlap: along an axis the blended output moves only through a(i) = sin^2(pi/2 (i + 0.5) / R), whose
    step is at most pi / (2 R), so adjacent pixels differ by at most spread * pi / (2 R); the plain mean jumps at every window edge."""
    R = 16
    wins = np.asarray(HR.slide_windows(96, 96, 16, 32), dtype=np.int32)
    rng = np.random.default_rng(5)
    tl = np.broadcast_to(rng.standard_normal((len(wins), 1, 1, 1)), (len(wins), 1, 2, 2)).astype(np.float32)
    args = (tl, wins, (32, 32), (0, 0), (96, 96))
    spread = float(tl.max() - tl.min())
    limit = spread * math.pi / (2 * R) * (1 + 1e-3)

    def step(canvas):
        return max(np.abs(np.diff(canvas, axis=1)).max(), np.abs(np.diff(canvas, axis=2)).max())

    blended, plain = step(BR.stitch_blend(*args, BR.ramp("hann", R))), step(HR.stitch(*args))
    print(f"largest step / spread: blended {blended / spread:.3f}, limit {limit / spread:.3f}, plain mean {plain / spread:.3f}")
    assert blended <= limit < plain


@pytest.mark.parametrize("geom,Q", BR.HEAD_GEOM_Q)
def test_the_label_cases_stay_under_the_cap(geom, Q):
    worst = 0.0
    for c, merged, thd, spec in BR.head_cases(geom, Q):
        canvas = BR.stitch_blend(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"], BR.head_ramp(geom, spec))
        ref = HR.tail(canvas, c["query_idx"], c["K"], 50.0, thd, 0)
        worst = max(worst, 1.0 - HR.counted(ref, thd).mean())
    print(f"{geom} Q={Q}: at most {100 * worst:.3f} % uncounted")
    assert worst <= HR.CAP
