"""sg_extract_tiles, sg_global_debias and sg_adaptive_conv (the three small kernels at the end of csrc/jbu.hip) against the references of
tests/tiles_reference.py, each through its raw C entry with the arguments one to one.

Every output is NaN-filled and sits between two 64 KiB guard bands of NaN: after the call the bands must hold their bytes and no output
cell may still be NaN.  Tile extraction is compared byte for byte; global debias and the adaptive convolution element by element with the
derived bounds, whose tightness (median bound / |ref|) is asserted too.  A refused call returns non-zero, names itself in sg_last_error and
leaves the output's bytes alone.  No window leaves its scene: the kernel cannot validate device-side windows, in-scene windows are the
caller's contract (tiles_reference's docstring).  tests/test_tiles_bound_cpu.py shows on the same generators that an f32 restatement of
each kernel passes and that the listed single faults fail."""
import ctypes as C
import os
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_reference as R                                            # noqa: E402
import tiles_reference as T                                             # noqa: E402
from tiles_reference import check_within, median_tightness              # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 1 << 16
WORST = defaultdict(float)                    # (kernel, case) -> largest err / bound
TIGHT = defaultdict(float)                    # kernel -> largest median bound / |ref|
EXACT = defaultdict(int)                      # kernel -> cells compared byte for byte


@pytest.fixture(scope="module")
def lib():
    from clip_decontamination_amd import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Guarded:
    """`numel` f32 on the device, NaN-filled, between two NaN guard bands; `.view` is the payload."""

    def __init__(self, numel):
        self.g = GUARD // 4
        self.big = torch.full((2 * self.g + numel,), float("nan"), dtype=torch.float32, device=DEV)
        self.bits = int(torch.tensor(float("nan")).view(torch.int32))
        self.view = self.big[self.g:self.g + numel]

    def guards_intact(self):
        b = self.big.view(torch.int32)
        return bool((b[:self.g] == self.bits).all()) and bool((b[self.g + self.view.numel():] == self.bits).all())

    def finish(self):
        """Guard bands intact and every payload cell written -> the payload on the CPU."""
        torch.cuda.synchronize()
        assert self.guards_intact(), "guard band overwritten"
        out = self.view.cpu()
        assert not bool(torch.isnan(out).any()), f"{int(torch.isnan(out).sum())} output cells never written"
        return out

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.big.view(torch.int32) == self.bits).all())


def refused(lib, rc, out, name):
    assert rc != 0, f"{name}: accepted"
    assert name.encode() in lib.sg_last_error(), lib.sg_last_error()
    assert out.untouched(), f"{name}: a refused call wrote to the output"


def ok(lib, rc):
    torch.cuda.synchronize()
    assert rc == 0, lib.sg_last_error()


# ---- sg_extract_tiles --------------------------------------------------------------------------------------------------------------------
def tile_batch(c, scene_t, win_t, idx_t, **over):
    from clip_decontamination_amd import _lib
    kw = dict(scene=scene_t.data_ptr(), format=_lib.IMG_F32_NCHW if c["fmt"] == "f32" else _lib.IMG_U8_NHWC, scene_h=c["scene_h"], scene_w=c["scene_w"],
              windows=win_t.data_ptr(), scene_index=None if idx_t is None else idx_t.data_ptr(), scene_stride=c["scene_stride"], n_tiles=c["n_tiles"],
              tile_h=c["tile_h"], tile_w=c["tile_w"], pad_l=c["pad_l"], pad_t=c["pad_t"], grid_h=c.get("grid_h", 0), grid_w=c.get("grid_w", 0))
    kw.update(over)
    return _lib.TileBatch(**kw)


def on_device(c):
    """(scene, windows, scene_index) of a case on the device; the caller keeps them alive across the call."""
    w = c["windows"]
    assert int(w[:, 0].min()) >= 0 and int(w[:, 2].min()) >= 0 and int(w[:, 1].max()) <= c["scene_h"] and int(w[:, 3].max()) <= c["scene_w"]
    assert c["scene_index"] is None or int(c["scene_index"].max()) < c["scene"].shape[0]
    return (torch.from_numpy(c["scene"]).to(DEV), torch.from_numpy(w).to(DEV),
            None if c["scene_index"] is None else torch.from_numpy(c["scene_index"]).to(DEV))


def run_extract(lib, c):
    scene, win, idx = on_device(c)
    tb = tile_batch(c, scene, win, idx)
    out = Guarded(c["n_tiles"] * 3 * c["up_h"] * c["up_w"])
    ok(lib, lib.sg_extract_tiles(C.byref(tb), c["up_h"], c["up_w"], P(out.view), stream()))
    return out.finish().numpy().reshape(c["n_tiles"], 3, c["up_h"], c["up_w"])


@pytest.mark.parametrize("name", [c["name"] for c in T.EXTRACT_CASES])
def test_extract_tiles_is_exact(lib, name):
    c = T.EXTRACT_BY_NAME[name]
    got, ref = run_extract(lib, c), T.extract_reference(c)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} cells differ, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"
    EXACT["extract_tiles"] += bad.size


def test_extract_tiles_refusals(lib):
    c = T.EXTRACT_BY_NAME["f32-T3-pad3x5-exact"]
    scene, win, idx = on_device(c)
    out = Guarded(c["n_tiles"] * 3 * c["up_h"] * c["up_w"])
    uh, uw = c["up_h"], c["up_w"]
    refused(lib, lib.sg_extract_tiles(None, uh, uw, P(out.view), stream()), out, "sg_extract_tiles")
    refused(lib, lib.sg_extract_tiles(C.byref(tile_batch(c, scene, win, idx)), uh, uw, None, stream()), out, "sg_extract_tiles")
    for over in (dict(scene=None), dict(windows=None), dict(n_tiles=0)):
        refused(lib, lib.sg_extract_tiles(C.byref(tile_batch(c, scene, win, idx, **over)), uh, uw, P(out.view), stream()), out, "sg_extract_tiles")
    refused(lib, lib.sg_extract_tiles(C.byref(tile_batch(c, scene, win, idx)), uh - 1, uw, P(out.view), stream()), out, "sg_extract_tiles")
    refused(lib, lib.sg_extract_tiles(C.byref(tile_batch(c, scene, win, idx)), uh, uw - 1, P(out.view), stream()), out, "sg_extract_tiles")
    ok(lib, lib.sg_extract_tiles(C.byref(tile_batch(c, scene, win, idx)), uh, uw, P(out.view), stream()))      # the same arguments unbroken
    assert T.same_bytes(out.finish().numpy().reshape(-1), T.extract_reference(c).reshape(-1))


@pytest.mark.parametrize("P_", [14, 16])
def test_extract_against_patchify_on_one_u8_batch(lib, P_):
    """The same u8 tile batch through sg_patchify_raw (f32 patch matrix, gathered back to planes) and sg_extract_tiles.  The two are
    byte-equal wherever the subtraction u - mean is exact.  They differ exactly where the plain f32 quotient is not the nearest f32 of the
    float64 quotient -- cells of channel 2 from u = 233 and of channel 0 from u = 251, nowhere else -- and there patchify holds the nearest
    f32 and extract the plain quotient."""
    from clip_decontamination_amd import _lib
    gh, gw = 2, 3
    pc = R.make_patch_case(P_, gh, gw, True, seed=P_)
    c = dict(T.patch_case_as_extract(pc), grid_h=gh, grid_w=gw)
    scene, win, idx = on_device(c)
    tb = tile_batch(c, scene, win, idx)
    Kpad = R.std_kpad(P_)
    pm = Guarded(2 * gh * gw * Kpad)
    ok(lib, lib.sg_patchify_raw(C.byref(tb), P_, Kpad, P(pm.view), _lib.PREC_F32, stream()))
    planes_p = T.patches_to_planes(pm.finish().view(2 * gh * gw, Kpad), 2, gh, gw, P_).contiguous().numpy()
    out = Guarded(2 * 3 * c["up_h"] * c["up_w"])
    ok(lib, lib.sg_extract_tiles(C.byref(tb), c["up_h"], c["up_w"], P(out.view), stream()))
    planes_e = out.finish().numpy().reshape(planes_p.shape)
    assert T.same_bytes(planes_e, T.extract_reference(c))
    by = T.extract_bytes(c)
    ch = np.broadcast_to(np.arange(3)[None, :, None, None], by.shape)
    live = by >= 0
    plain, exact, _ = T.quotient_table()
    nearest = exact.astype(np.float32)
    exact_sub = np.ones(by.shape, dtype=bool)
    exact_sub[live] = T.exact_subtraction()[ch[live], by[live]]
    same = planes_p.view(np.uint32) == planes_e.view(np.uint32)
    assert bool(same[exact_sub].all()), "the two ingests differ where the subtraction is exact"
    late = live & (((ch == 2) & (by >= 233)) | ((ch == 0) & (by >= 251)))
    assert not bool((~same & ~late).any()), "the two ingests differ outside channel 2 from 233 / channel 0 from 251"
    assert int(late.sum()) > 0 and int((live & (ch == 2) & (by >= 233)).sum()) > 0
    assert np.array_equal(planes_p[late].view(np.uint32), nearest[ch[late], by[late]].view(np.uint32)), "patchify: not the nearest f32"
    assert np.array_equal(planes_e[late].view(np.uint32), plain[ch[late], by[late]].view(np.uint32)), "extract: not the plain quotient"
    assert np.array_equal(~same[late], (plain != nearest)[ch[late], by[late]]) and int((~same).sum()) > 0
    print(f"P {P_}: {int(live.sum())} live cells, {int(late.sum())} where the subtraction rounds, {int((~same).sum())} differ")


def test_scene_planes_wrapper(lib):
    from clip_decontamination_amd import ops
    big = T.make_scene("u8", B=1, H=45, W=70, seed=5)[0]
    for scene in (torch.from_numpy(big).to(DEV), torch.from_numpy(big).to(DEV)[2:43, 1:68]):
        got = ops.scene_planes(scene)
        torch.cuda.synchronize()
        ref = np.ascontiguousarray(np.moveaxis(T.normalised(scene.cpu().numpy()), -1, 0))
        assert tuple(got.shape) == ref.shape and T.same_bytes(got.cpu().numpy(), ref)
    assert not torch.from_numpy(big).to(DEV)[2:43, 1:68].is_contiguous()
    f = torch.from_numpy(T.make_scene("f32", B=1, seed=6)[0]).to(DEV)
    back = ops.scene_planes(f)
    assert back.dtype == torch.float32 and torch.equal(back.view(torch.int32), f.view(torch.int32))


# ---- sg_global_debias --------------------------------------------------------------------------------------------------------------------
def run_debias(lib, tok, cls, factor):
    B, n, E = tok.shape
    td, cd = tok.to(DEV), cls.to(DEV)
    out = Guarded(B * n * E)
    ok(lib, lib.sg_global_debias(P(td), P(cd), B, n, E, float(factor), P(out.view), stream()))
    return out.finish().view(B, n, E)


def check_debias(got, tok, cls, factor, case):
    ref, bnd = T.debias_reference(tok, cls, factor)
    r = check_within(got, ref, bnd, f"global_debias {case}")
    WORST[("global_debias", case)] = max(WORST[("global_debias", case)], r)
    if factor == 0:
        assert torch.equal(got.view(torch.int32), tok.view(torch.int32)), f"{case}: factor 0 must return the input bit for bit"
    else:
        t = median_tightness(bnd, ref)
        TIGHT["global_debias"] = max(TIGHT["global_debias"], t)
        assert t <= T.TIGHT_LIMIT, f"{case}: median bound / |ref| = {t:.3g}"
    return r


@pytest.mark.parametrize("n", T.DEBIAS_N)
@pytest.mark.parametrize("E", T.DEBIAS_E)
def test_global_debias_vs_f64(lib, E, n):
    worst = 0.0
    for B in T.DEBIAS_B:
        tok, cls = T.make_debias_case(B, n, E, seed=B)
        for factor in T.DEBIAS_FACTORS:
            worst = max(worst, check_debias(run_debias(lib, tok, cls, factor), tok, cls, factor, f"E {E} n {n} B {B} factor {factor}"))
    print(f"global_debias E {E} n {n}: worst err / bound {worst:.3g}")


def test_global_debias_grid_limit(lib):
    """65535 images fill gridDim.y; 65536 are refused, like null pointers and non-positive sizes."""
    tok, cls = T.make_debias_case(65535, 1, 2, seed=1)
    r = check_debias(run_debias(lib, tok, cls, 0.2), tok, cls, 0.2, "B 65535 n 1 E 2")
    print(f"global_debias B 65535: worst err / bound {r:.3g}")
    tok, cls = T.make_debias_case(2, 5, 48, seed=1)
    td, cd = tok.to(DEV), cls.to(DEV)
    out = Guarded(65536 * 2)
    s = stream()
    for args in ((P(td), P(cd), 65536, 1, 2, 0.2, P(out.view)), (None, P(cd), 2, 5, 48, 0.2, P(out.view)), (P(td), None, 2, 5, 48, 0.2, P(out.view)),
                 (P(td), P(cd), 0, 5, 48, 0.2, P(out.view)), (P(td), P(cd), 2, 0, 48, 0.2, P(out.view)), (P(td), P(cd), 2, 5, 0, 0.2, P(out.view)),
                 (P(td), P(cd), -1, 5, 48, 0.2, P(out.view)), (P(td), P(cd), 2, -5, 48, 0.2, P(out.view)), (P(td), P(cd), 2, 5, -48, 0.2, P(out.view))):
        refused(lib, lib.sg_global_debias(*args, s), out, "sg_global_debias")
    rc = lib.sg_global_debias(P(td), P(cd), 2, 5, 48, 0.2, None, s)
    assert rc != 0 and b"sg_global_debias" in lib.sg_last_error()


def test_global_debias_wrapper(lib):
    """ops.global_debias on a non-contiguous tokens view and on f16 inputs: the reference on the values the wrapper converts."""
    from clip_decontamination_amd import ops
    tok, cls = T.make_debias_case(3, 10, 65, seed=2)
    td = tok.to(DEV)[:, ::2, :]
    assert not td.is_contiguous()
    got = ops.global_debias(td, cls.to(DEV), 0.2)
    torch.cuda.synchronize()
    check_debias(got.cpu(), tok[:, ::2, :].contiguous(), cls, 0.2, "wrapper, strided tokens")
    tok, cls = T.make_debias_case(3, 5, 64, seed=2)
    th, ch = tok.half(), cls.half()
    got = ops.global_debias(th.to(DEV), ch.to(DEV), -1.5)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32
    check_debias(got.cpu(), th.float(), ch.float(), -1.5, "wrapper, f16 inputs")


# ---- sg_adaptive_conv --------------------------------------------------------------------------------------------------------------------
def run_conv(lib, inp, filt):
    B, Cc = inp.shape[:2]
    _, h, w, d, _ = filt.shape
    idev, fdev = inp.to(DEV), filt.to(DEV)
    out = Guarded(B * Cc * h * w)
    ok(lib, lib.sg_adaptive_conv(P(idev), P(fdev), B, Cc, h, w, d, P(out.view), stream()))
    return out.finish().view(B, Cc, h, w)


def check_conv(got, inp, filt, case, tight=True):
    d = filt.shape[-1]
    ref = T.adaptive_conv_reference(inp, filt)
    bnd = T.adaptive_conv_bound(ref, d)
    r = check_within(got, ref["out"], bnd, f"adaptive_conv {case}")
    WORST[("adaptive_conv", case)] = max(WORST[("adaptive_conv", case)], r)
    if tight:
        t = median_tightness(bnd, ref["out"])
        TIGHT["adaptive_conv"] = max(TIGHT["adaptive_conv"], t)
        assert t <= T.TIGHT_LIMIT, f"{case}: median bound / |ref| = {t:.3g}"
    return r


@pytest.mark.parametrize("w", T.CONV_W)
@pytest.mark.parametrize("h", T.CONV_H)
def test_adaptive_conv_vs_f64(lib, h, w):
    worst = 0.0
    for d in T.CONV_D:
        for B, Cc in T.CONV_BC:
            inp, filt = T.make_conv_case(B, Cc, h, w, d, seed=B + Cc)
            worst = max(worst, check_conv(run_conv(lib, inp, filt), inp, filt, f"h {h} w {w} d {d} B {B} C {Cc}", tight=h * w >= 9))
    print(f"adaptive_conv h {h} w {w}: worst err / bound {worst:.3g}")


@pytest.mark.parametrize("d,h,w", [(7, 5, 65), (3, 9, 130)])
def test_adaptive_conv_onehot_selects_bit_for_bit(lib, d, h, w):
    inp, filt, t = T.make_conv_case(2, 3, h, w, d, seed=1, onehot=True)
    got = run_conv(lib, inp, filt)
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    sel = torch.stack([inp[b][:, y + t[b] // d, x + t[b] % d] for b in range(2)])
    assert torch.equal(got.view(torch.int32), sel.view(torch.int32))
    EXACT["adaptive_conv one-hot"] += got.numel()


def test_adaptive_conv_grid_limit(lib):
    """B C = 65535 fills gridDim.z (the kernel splits it back into b = z / C, c = z % C); 65536 is refused, like null pointers and
    non-positive sizes."""
    inp, filt = T.make_conv_case(255, 257, 1, 1, 1, seed=3)
    r = check_conv(run_conv(lib, inp, filt), inp, filt, "B 255 C 257 h 1 w 1 d 1")
    print(f"adaptive_conv B C 65535: worst err / bound {r:.3g}")
    inp, filt = T.make_conv_case(2, 3, 4, 5, 3, seed=3)
    idev, fdev = inp.to(DEV), filt.to(DEV)
    out = Guarded(65536)
    s = stream()
    for args in ((P(idev), P(fdev), 256, 256, 1, 1, 1, P(out.view)), (None, P(fdev), 2, 3, 4, 5, 3, P(out.view)), (P(idev), None, 2, 3, 4, 5, 3, P(out.view)),
                 (P(idev), P(fdev), 0, 3, 4, 5, 3, P(out.view)), (P(idev), P(fdev), 2, 0, 4, 5, 3, P(out.view)), (P(idev), P(fdev), 2, 3, 0, 5, 3, P(out.view)),
                 (P(idev), P(fdev), 2, 3, 4, 0, 3, P(out.view)), (P(idev), P(fdev), 2, 3, 4, 5, 0, P(out.view)), (P(idev), P(fdev), -2, 3, 4, 5, 3, P(out.view)),
                 (P(idev), P(fdev), 2, 3, 4, 5, -3, P(out.view))):
        refused(lib, lib.sg_adaptive_conv(*args, s), out, "sg_adaptive_conv")
    rc = lib.sg_adaptive_conv(P(idev), P(fdev), 2, 3, 4, 5, 3, None, s)
    assert rc != 0 and b"sg_adaptive_conv" in lib.sg_last_error()


def test_adaptive_conv_wrapper(lib):
    from clip_decontamination_amd import ops
    inp, filt = T.make_conv_case(2, 3, 5, 65, 7, seed=4)
    got = ops.adaptive_conv(inp.to(DEV), filt.to(DEV))
    torch.cuda.synchronize()
    check_conv(got.cpu(), inp, filt, "wrapper")


def test_zz_worst_ratios():
    """Runs last (module order): the err / bound table of the module."""
    per = defaultdict(lambda: (0.0, ""))
    for (k, case), v in WORST.items():
        if v >= per[k][0]:
            per[k] = (v, case)
    for k in sorted(per):
        print(f"  {k:>16}: largest err / bound {per[k][0]:.3g} at {per[k][1]}; largest median bound / |ref| {TIGHT[k]:.3g}")
    print("  byte-for-byte cells:", dict(EXACT))
    assert WORST and all(v <= 1.0 for v in WORST.values())
