"""The references and bounds of tests/tiles_reference.py on the CPU (no GPU needed): an f32 restatement of each kernel in the kernel's own
order stays inside its bound on every committed case (tile extraction: is byte-equal), the committed seeds satisfy the domain conditions,
each listed single fault fails on a named case, and the plain f32 quotient of the u8 normalisation is compared with the float64 one."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_reference as R                                            # noqa: E402
import tiles_reference as T                                             # noqa: E402
from tiles_reference import check_within, median_tightness              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fails(got, ref, bnd):
    with pytest.raises(AssertionError):
        check_within(got, ref, bnd, "mutant")


# ---- (d) the quotient --------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "clip_decontamination_amd", "csrc", "jbu.hip")).read()
    for name, vals in (("j_mean", T.JBU_MEAN), ("j_std", T.JBU_STD)):
        m = re.search(name + r"\[3\] = \{([^}]*)\}", src)
        assert m and tuple(float(v.strip().rstrip("f")) for v in m.group(1).split(",")) == vals


def test_plain_f32_quotient_against_f64():
    """The plain quotient is the nearest f32 of the float64 quotient wherever the subtraction is exact.  The subtraction rounds where
    |u - mean| >= 128 and mean's last bit is set: channel 2 from u = 233 -- and channel 0 from u = 251, which csrc/patchify.hip's comment
    and tests/test_gpu_pamr_route.py do not mention (channel 1's mean has a zero last bit, so its subtraction stays exact to u = 255).
    Outside those two runs the plain quotient is within half an ulp; inside, it reaches 1.374 ulp (channel 2, u = 234; the 1.37 quoted
    in patchify.hip) and 1.202 ulp (channel 0, u = 255).  The patchify form is the nearest f32 at every (c, u) and has the plain
    quotient's bits wherever the subtraction is exact."""
    plain, exact, err = T.quotient_table()
    exact_sub = T.exact_subtraction()
    late = np.zeros((3, 256), dtype=bool)
    late[2, 233:] = True
    late[0, 251:] = True
    assert np.array_equal(~exact_sub, late)
    u = np.arange(256, dtype=np.float64)[None, :]
    assert not bool((exact_sub[(0, 2), :] & (np.abs(u - T.MEAN32.astype(np.float64)[:, None]) >= 128)[(0, 2), :]).any())
    nearest = exact.astype(np.float32)
    assert np.array_equal(plain[exact_sub], nearest[exact_sub]) and float(err[exact_sub].max()) <= 0.5
    differ = plain != nearest
    worst = {c: (float(err[c].max()), int(err[c].argmax())) for c in range(3)}
    print(f"plain f32 (u - mean) / std, worst ulp error per channel (at u): {worst}; beyond 1 ulp at "
          f"{[(int(c), int(v)) for c, v in zip(*np.nonzero(err > 1))]}; not the nearest f32 at {[(int(c), int(v)) for c, v in zip(*np.nonzero(differ))]}")
    assert worst[2][1] == 234 and 1.373 < worst[2][0] < 1.374 and worst[2][0] <= 1.37 + 5e-3
    assert worst[0][1] == 255 and 1.201 < worst[0][0] < 1.203
    assert worst[1][0] <= 0.5
    assert not bool((err > 1)[~late].any()) and [int(v) for v in np.nonzero(err[2] > 1)[0]] == [233, 234, 238, 239, 240, 244]
    assert bool(differ[2, 233:].any()) and bool(differ[0, 251:].any()) and not bool(differ[~late].any())
    pf = T.patchify_form_table()
    assert np.array_equal(pf.view(np.uint32), nearest.view(np.uint32))
    assert np.array_equal(pf[exact_sub], plain[exact_sub])


# ---- extract -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in T.EXTRACT_CASES])
def test_extract_restatement_is_byte_equal(name):
    c = T.EXTRACT_BY_NAME[name]
    ref = T.extract_reference(c)
    assert T.same_bytes(T.extract_restated(c), ref)
    pad = np.ones(ref.shape, dtype=bool)
    pad[:, :, c["pad_t"]:c["pad_t"] + c["tile_h"], c["pad_l"]:c["pad_l"] + c["tile_w"]] = False
    assert not ref.view(np.uint32)[pad].any()                            # +0.0, not -0.0
    assert ref.nbytes <= 1 << 20


def test_extract_cases_cover_what_they_claim():
    cases = T.EXTRACT_CASES
    for c in cases:
        w = c["windows"]
        assert bool((w[:, 0] >= 0).all() and (w[:, 2] >= 0).all() and (w[:, 1] <= c["scene_h"]).all() and (w[:, 3] <= c["scene_w"]).all()), c["name"]
        assert bool((w[:, 1] - w[:, 0] == c["tile_h"]).all() and (w[:, 3] - w[:, 2] == c["tile_w"]).all()), c["name"]
        assert c["up_h"] >= c["tile_h"] + c["pad_t"] and c["up_w"] >= c["tile_w"] + c["pad_l"]
        assert c["scene_h"] != c["scene_w"]
        if c["scene_index"] is not None:
            assert int(c["scene_index"].max()) < c["scene"].shape[0] and c["scene_stride"] == 3 * c["scene_h"] * c["scene_w"]
        if c["fmt"] == "u8" and min(c["tile_h"], c["tile_w"]) >= 16:        # every byte value in every channel is actually compared
            by = T.extract_bytes(c)
            for t in range(c["n_tiles"]):
                for ch in range(3):
                    assert np.array_equal(np.unique(by[t, ch][by[t, ch] >= 0]), np.arange(256)), c["name"]
    seen = np.concatenate([T.extract_bytes(c).transpose(1, 0, 2, 3).reshape(3, -1) for c in cases if c["fmt"] == "u8"], axis=1)
    assert all(set(range(256)) <= set(seen[ch].tolist()) for ch in range(3))
    for fmt in ("f32", "u8"):
        mine = [c for c in cases if c["fmt"] == fmt]
        assert {c["n_tiles"] for c in mine} >= {1, 3, 5}
        assert {(c["pad_l"], c["pad_t"]) for c in mine} >= set(T.PADS)
        assert any(c["tile_h"] != c["tile_w"] for c in mine)
        assert any((c["n_tiles"] * 3 * c["up_h"] * c["up_w"]) % 256 for c in mine)
        assert any(c["up_w"] == 1 for c in mine)
        assert any(c["up_h"] == c["tile_h"] + 2 * c["pad_t"] and c["up_w"] == c["tile_w"] + 2 * c["pad_l"] and c["pad_l"] and c["pad_t"] for c in mine)
        assert any(c["up_h"] > c["tile_h"] + c["pad_t"] and c["up_w"] == c["tile_w"] + c["pad_l"] for c in mine)
        assert any(c["tile_h"] == c["scene_h"] and c["tile_w"] == c["scene_w"] for c in mine)
        assert any(c["scene_index"] is not None and list(c["scene_index"]) == list(T.OUT_OF_ORDER) for c in mine)
        assert any(c["scene_index"] is None for c in mine)
        w = np.concatenate([c["windows"] for c in mine if c["tile_h"] != c["scene_h"]])
        assert (w[:, 0] == 0).any() and (w[:, 2] == 0).any() and (w[:, 1] == T.SCENE_H).any() and (w[:, 3] == T.SCENE_W).any()


# each fault on the case that shows it: both pads non-zero and different; five tiles through scene_index; a u8 scene; a band beyond tile + pad
EXTRACT_FAULT_CASE = {"pads_exchanged": "f32-T3-pad3x5-exact", "scene_index_ignored": "f32-T5-pad3x5-prod", "u8_as_nchw": "u8-T3-pad3x5-prod",
                      "next_channel_constants": "u8-T1-pad0x0-exact", "band_not_zeroed": "u8-T3-pad5x0-rows", "x0_from_next_slot": "f32-T1-pad5x0-prod"}


@pytest.mark.parametrize("mut", T.EXTRACT_MUTANTS)
def test_extract_faults_fail(mut):
    c = T.EXTRACT_BY_NAME[EXTRACT_FAULT_CASE[mut]]
    ref = T.extract_reference(c)
    assert T.same_bytes(T.extract_restated(c), ref) and not T.same_bytes(T.extract_restated(c, mut), ref)


def test_patches_to_planes_inverts_the_patch_layout():
    """patches_to_planes undoes rowops_reference.patchify_reference's column order, and the planes are extract_reference's up to the last ulp
    of the u8 normalisation (the patch reference is the float64 quotient)."""
    for P_ in (14, 16):
        pc = R.make_patch_case(P_, 2, 3, True, seed=P_)
        mat, mask = R.patchify_reference(pc["scene"], pc["windows"], pc["scene_index"], pc["tile_h"], pc["tile_w"], pc["pad_l"], pc["pad_t"], 2, 3, P_,
                                         R.std_kpad(P_))
        planes = T.patches_to_planes(mat, 2, 2, 3, P_).numpy()
        c = T.patch_case_as_extract(pc)
        ref = T.extract_reference(c)
        live = T.extract_bytes(c) >= 0
        assert np.array_equal(T.patches_to_planes(mask, 2, 2, 3, P_).numpy(), live)
        assert float(np.abs(planes - ref).max()) < 1e-6 and not planes[~live].any()
        b = T.extract_bytes(c)[:, 2]
        assert int((b >= 233).sum()) > 0                                 # the cells where the two kernels may differ are there


# ---- global debias -----------------------------------------------------------------------------------------------------------------------
DEBIAS_SHAPES = [(E, n) for E in T.DEBIAS_E for n in T.DEBIAS_N]


@pytest.mark.parametrize("E,n", DEBIAS_SHAPES)
def test_debias_restatement_within_bound(E, n):
    for B in T.DEBIAS_B:
        tok, cls = T.make_debias_case(B, n, E, seed=B)
        # (b) the domain: finite squared norms in f32, no zero rows, no negative zero
        ss = (cls * cls).sum(-1)
        assert bool(((ss > 1e-30) & (ss < 1e30)).all()) and bool(((tok * tok).sum(-1) > 1e-30).all())
        assert not bool(((tok == 0) & torch.signbit(tok)).any())
        for factor in T.DEBIAS_FACTORS:
            ref, bnd = T.debias_reference(tok, cls, factor)
            assert bool(torch.isfinite(ref).all())
            got = T.debias_restated(tok, cls, factor)
            r = check_within(got, ref, bnd, f"debias restated E {E} n {n} B {B} factor {factor}")
            assert r <= 0.6                                              # 2u is budgeted per operation that costs u
            if factor == 0:
                assert torch.equal(got.view(torch.int32), tok.view(torch.int32))
            else:
                assert median_tightness(bnd, ref) <= T.TIGHT_LIMIT


def test_grid_limit_and_wrapper_cases_within_bound():
    """The remaining committed cases of the GPU module: the grid-limit shapes and the wrapper inputs."""
    for (B, n, E, seed), factor, half in (((65535, 1, 2, 1), 0.2, False), ((3, 10, 65, 2), 0.2, False), ((3, 5, 64, 2), -1.5, True)):
        tok, cls = T.make_debias_case(B, n, E, seed=seed)
        if half:
            tok, cls = tok.half().float(), cls.half().float()
            assert bool(torch.isfinite(tok).all()) and bool(((tok * tok).sum(-1) > 1e-30).all()) and bool(((cls * cls).sum(-1) > 1e-30).all())
        ref, bnd = T.debias_reference(tok, cls, factor)
        check_within(T.debias_restated(tok, cls, factor), ref, bnd, f"debias B {B} n {n} E {E}")
        assert median_tightness(bnd, ref) <= T.TIGHT_LIMIT
    for B, C, h, w, d, seed in ((255, 257, 1, 1, 1, 3), (2, 3, 5, 65, 7, 4)):
        inp, filt = T.make_conv_case(B, C, h, w, d, seed=seed)
        ref = T.adaptive_conv_reference(inp, filt)
        check_within(T.adaptive_conv_restated(inp, filt), ref["out"], T.adaptive_conv_bound(ref, d), f"conv B {B} C {C}")


def test_debias_cases_hold_the_special_rows():
    tok, cls = T.make_debias_case(3, 197, 65, seed=3)
    x, c = tok.double(), cls.double()[:, None, :]
    cos = (x * c).sum(-1) / (x.norm(dim=-1) * c.norm(dim=-1))
    assert bool((cos[:, 194] > 1 - 1e-6).all()) and bool((cos[:, 195] < -1 + 1e-6).all()) and bool((cos[:, 196].abs() < 1e-7).all())
    assert sorted(float(f"{v:.3g}") for v in cls.norm(dim=-1)) == [1e-3, 1.0, 30.0]
    amax = tok.abs().amax(-1)
    assert float(amax.min()) <= 1.01e-2 and float(amax.max()) >= 99.0


# the fault -> (E, n, B, factor): two trips with one lane in the second; n % 4 != 0; a cls of norm 30 and 1e-3
DEBIAS_FAULT_CASE = {"cls_not_normalised": (48, 5, 3, 0.2), "factor_dropped": (48, 5, 3, 0.2), "tail_lanes_dropped": (65, 5, 1, 0.2),
                     "token_norm_omitted": (48, 5, 3, -1.5), "last_rows_unwritten": (64, 197, 1, 0.2)}


@pytest.mark.parametrize("mut", T.DEBIAS_MUTANTS)
def test_debias_faults_fail(mut):
    E, n, B, factor = DEBIAS_FAULT_CASE[mut]
    tok, cls = T.make_debias_case(B, n, E, seed=B)
    ref, bnd = T.debias_reference(tok, cls, factor)
    check_within(T.debias_restated(tok, cls, factor), ref, bnd, "restated")
    _fails(T.debias_restated(tok, cls, factor, mut), ref, bnd)
    if mut in ("cls_not_normalised", "factor_dropped", "token_norm_omitted"):   # the fault evaluated exactly leaves the bound as well
        _fails(T.debias_reference(tok, cls, factor, mut)[0], ref, bnd)


# ---- adaptive convolution ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", T.CONV_W)
@pytest.mark.parametrize("h", T.CONV_H)
def test_conv_restatement_within_bound(h, w):
    for d in T.CONV_D:
        for B, C in T.CONV_BC:
            inp, filt = T.make_conv_case(B, C, h, w, d, seed=B + C)
            ref = T.adaptive_conv_reference(inp, filt)
            bnd = T.adaptive_conv_bound(ref, d)
            r = check_within(T.adaptive_conv_restated(inp, filt), ref["out"], bnd, f"conv restated h {h} w {w} d {d} B {B} C {C}")
            assert r <= 0.6
            if h * w >= 9:
                assert median_tightness(bnd, ref["out"]) <= T.TIGHT_LIMIT
            if d > 1:                                                    # (b) neither operand is symmetric
                assert not torch.equal(filt, filt.transpose(3, 4))
            if h > 1 and w > 1:
                assert not torch.equal(inp[..., :min(h, w), :min(h, w)], inp[..., :min(h, w), :min(h, w)].transpose(2, 3))


def test_conv_onehot_selects_bit_for_bit():
    inp, filt, t = T.make_conv_case(2, 3, 5, 65, 7, seed=1, onehot=True)
    got = T.adaptive_conv_restated(inp, filt)
    y, x = torch.meshgrid(torch.arange(5), torch.arange(65), indexing="ij")
    sel = torch.stack([inp[b][:, y + t[b] // 7, x + t[b] % 7] for b in range(2)])
    assert torch.equal(got.view(torch.int32), sel.view(torch.int32))
    assert len(torch.unique(t)) == 49


CONV_FAULT_CASE = {"filter_transposed": (2, 3, 5, 65, 3), "row_pitch_w": (2, 3, 5, 65, 3), "filter_shared_across_y": (1, 1, 3, 63, 7)}


@pytest.mark.parametrize("mut", T.CONV_MUTANTS)
def test_conv_faults_fail(mut):
    B, C, h, w, d = CONV_FAULT_CASE[mut]
    inp, filt = T.make_conv_case(B, C, h, w, d, seed=B + C)
    ref = T.adaptive_conv_reference(inp, filt)
    bnd = T.adaptive_conv_bound(ref, d)
    check_within(T.adaptive_conv_restated(inp, filt), ref["out"], bnd, "restated")
    _fails(T.adaptive_conv_reference(inp, filt, mut)["out"], ref["out"], bnd)
