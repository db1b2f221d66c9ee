"""Test-time augmentation at the C boundary and behind SegPipeline, without a GPU: include/segearth_hip.h declares sg_tta_head,
sg_tta_accumulate and sg_tta_finish, the library exports them and the ctypes table carries their signatures; the entries refuse bad
arguments through the error channel before any device work; the options are validated and every refusal names its reason on a stub
pipeline; with the options off ``tail_route`` returns exactly the rows of an instance built without them, and with them on the two
new rows."""
import ctypes
import itertools
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
ENTRIES = ("sg_tta_head", "sg_tta_accumulate", "sg_tta_finish")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.S)
    return None if m is None else [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype(param: str):
    if "*" in param or param.startswith("sg_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[param.split()[0]]


def test_header_library_and_ctypes_table_agree():
    from clip_decontamination_amd import _lib, ops
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        params = _params(name)
        assert params is not None, f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == [_ctype(p) for p in params], name
    assert _params("sg_tta_head")[:6] == ["const float* tile_logits", "int64_t logit_elems", "const int32_t* windows", "int total_tiles",
                                          "const int32_t* views", "int V"]
    assert _params("sg_tta_head")[-5:] == ["int64_t* labels", "float* conf", "float* probs", "int flags", "sg_stream s"]
    assert _params("sg_tta_accumulate") == ["const float* probs_view", "int K", "int out_h", "int out_w", "int flip", "float* acc", "int first",
                                            "sg_stream s"]
    assert _params("sg_tta_finish") == ["const float* acc", "int V", "int K", "int out_h", "int out_w", "float prob_thd", "int bg_idx",
                                        "int64_t* labels", "float* conf", "float* probs", "sg_stream s"]
    for macro, value in (("SG_TTA_MAX_VIEWS", ops.TTA_MAX_VIEWS), ("SG_TTA_VIEW_FIELDS", ops.TTA_VIEW_FIELDS)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)", _header())
        assert m and int(m.group(1)) == value, macro
    assert (ops.TTA_MAX_VIEWS, ops.TTA_VIEW_FIELDS, ops.TTA_MAX_Q) == (8, 11, 64)
    for name in ("tta_views", "tta_head", "tta_accumulate", "tta_finish"):
        assert callable(getattr(ops, name)), name


def test_entries_refuse_bad_arguments_before_any_device_work():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                                        # a non-null pointer that is never followed
    good = [3, 0, 2, 2, 4, 4, 0, 0, 8, 8, 1]                                        # T, first tile, gh, gw, up, pad, h, w, flip

    def head(rows=(good,), V=1, Q=5, K=5, bg=0, oh=8, ow=8, tiles=3, elems=3 * 5 * 4, views=True, flags=0):
        table = (ctypes.c_int32 * (11 * len(rows)))(*[x for r in rows for x in r])
        return lib.sg_tta_head(one, elems, one, tiles, table if views else None, V, Q, oh, ow, one, K, 50.0, 0.0, bg, one, None, None, flags, None)

    second = [2, 3, 2, 2, 4, 4, 0, 0, 8, 8, 0]
    for kw, word in ((dict(views=False), "null pointer"), (dict(V=0), "V=0 views"), (dict(V=9, rows=(good,) * 9), "V=9 views"),
                     (dict(Q=65, K=65), "Q=65 must lie in [1, 64]"), (dict(Q=0), "Q=0 must lie in"), (dict(K=6), "K=6 must lie in [1, Q=5]"),
                     (dict(bg=5), "bg_idx=5 outside [0, K=5)"), (dict(bg=-1), "bg_idx=-1 outside"), (dict(oh=0), "bad output size 0x8"),
                     (dict(flags=3), "flags=3 is no SG_RESIZED_"), (dict(rows=([0] + good[1:],)), "view 0 has a bad shape"),
                     (dict(rows=(good[:8] + [0, 8, 0],)), "view 0 has a bad shape"), (dict(rows=(good[:10] + [2],)), "flip=2"),
                     (dict(rows=(good, [2, 2] + second[2:]), V=2, tiles=5, elems=100), "view 1 starts at tile 2, but the views before it hold 3"),
                     (dict(tiles=4), "the views hold 3 tiles and 60 logits, the buffers 4 and 60"), (dict(elems=61), "the buffers 3 and 61")):
        rc = head(**kw)
        err = lib.sg_last_error().decode()
        assert rc == -1 and "sg_tta_head:" in err and word in err, (kw, rc, err)
    for call, word in ((lambda: lib.sg_tta_accumulate(None, 3, 4, 4, 0, one, 1, None), "null pointer"),
                       (lambda: lib.sg_tta_accumulate(one, 3, 4, 4, 0, one, 1, None), "the view's planes are the accumulator"),
                       (lambda: lib.sg_tta_accumulate(one, 0, 4, 4, 0, ctypes.c_void_p(16), 1, None), "bad shape K=0"),
                       (lambda: lib.sg_tta_accumulate(one, 3, 4, 4, 2, ctypes.c_void_p(16), 1, None), "flip=2"),
                       (lambda: lib.sg_tta_finish(None, 2, 3, 4, 4, 0.0, 0, one, None, None, None), "null pointer"),
                       (lambda: lib.sg_tta_finish(one, 0, 3, 4, 4, 0.0, 0, one, None, None, None), "V=0 views"),
                       (lambda: lib.sg_tta_finish(one, 9, 3, 4, 4, 0.0, 0, one, None, None, None), "V=9 views"),
                       (lambda: lib.sg_tta_finish(one, 2, 3, 0, 4, 0.0, 0, one, None, None, None), "bad shape"),
                       (lambda: lib.sg_tta_finish(one, 2, 3, 4, 4, 0.0, 3, one, None, None, None), "bg_idx=3 outside [0, K=3)")):
        rc = call()
        err = lib.sg_last_error().decode()
        assert rc == -1 and word in err, (word, rc, err)


# ---- options and refusals on a stub pipeline ----------------------------------------------------------------------------------------------
def _net():
    return types.SimpleNamespace(visual=types.SimpleNamespace(device="cpu", cfg=types.SimpleNamespace(patch=16, embed_dim=8)))


def _pipe(Q=8, **kw):
    from clip_decontamination_amd import pipeline
    return pipeline.SegPipeline(_net(), torch.zeros(Q, 8), torch.arange(Q) % 5, **kw)


def test_options_are_validated_and_every_refusal_names_its_reason():
    from clip_decontamination_amd import pipeline as P
    off = P.SegPipeline.__new__(P.SegPipeline)                                      # the class-level defaults: off
    assert (off.tta_scales, off.tta_flip, off.tta_head) == (None, False, "auto") and not off.tta_on()
    assert not _pipe().tta_on() and not _pipe(tta_head="canvas").tta_on()
    on = _pipe(tta_scales=(0.75, 1.0, 1.25), tta_flip=True)
    assert on.tta_on() and on.tta_scales == (0.75, 1.0, 1.25) and on.tta_fused() == P.TTA_AUTO_FUSED
    assert _pipe(tta_flip=True).tta_on() and _pipe(tta_flip=True).tta_scales is None     # the flip alone: scales (1.0,)
    assert _pipe(tta_scales=0.5).tta_scales == (0.5,)
    with pytest.raises(ValueError, match="tta_head must be one of"):
        _pipe(tta_head="lean")
    with pytest.raises(ValueError, match="tta_scales must be"):
        _pipe(tta_scales=(1.0, 0.0))
    with pytest.raises(ValueError, match="at most 8 views, got 10"):
        _pipe(tta_scales=(0.5, 0.75, 1.0, 1.25, 1.5), tta_flip=True)
    for kw, why in ((dict(tile_group="world"), P.TTA_TILE_GROUP), (dict(pamr_steps=2), P.TTA_PAMR), (dict(area_thd=0.1), P.TTA_AREA)):
        with pytest.raises(ValueError, match=re.escape(why)):
            _pipe(tta_flip=True, **kw)
        _pipe(**kw) if "tile_group" not in kw else None                             # without the option the instance is built as before
    with pytest.raises(ValueError, match=re.escape(P.TTA_TOPK)):
        on.topk_k(3)
    with pytest.raises(ValueError, match=re.escape(P.TTA_TOPK)):
        on.segment_scene(torch.zeros(40, 40, 3, dtype=torch.uint8), 16, 32, topk=2)
    with pytest.raises(ValueError, match=re.escape(P.TTA_TOPK)):
        list(on.label_groups([torch.zeros(40, 40, 3, dtype=torch.uint8)], 16, 32, topk=2))
    with pytest.raises(ValueError, match=re.escape(P.TTA_TILE_GROUP)):
        on.segment_scene(torch.zeros(40, 40, 3, dtype=torch.uint8), 16, 32, group="world")
    assert "not built" in P.TTA_TILE_GROUP and "not built" in P.TTA_PAMR and "not built" in P.TTA_AREA and "not built" in P.TTA_TOPK
    # "fused" where the fused head cannot run: refused with the reason; "auto" takes the canvas route there
    for kw, word in ((dict(Q=65), "65 queries exceed the fused head's 64"), (dict(blend="hann"), "blend='hann' needs the weighted stitch"),
                     (dict(upsampler=object()), "JBU upsampler")):
        with pytest.raises(ValueError, match="tta_head='fused' cannot serve this instance: .*" + re.escape(word)):
            _pipe(tta_flip=True, tta_head="fused", **kw)
        auto = _pipe(tta_flip=True, **kw)
        assert not auto.tta_fused() and auto.tail_route("labels").route == P.TTA_CANVAS
        _pipe(tta_head="fused", **kw)                                               # with the views off the option is idle


def test_the_route_rows():
    """Options off: ``tail_route`` returns the rows of an instance built without them, whatever tta_head says.  On: the two new rows."""
    from clip_decontamination_amd import pipeline as P
    combos = list(itertools.product(("labels", "probs", "topk"), (False, True), (False, True)))
    for Q in (8, 65):
        for kw in ({}, dict(label_head="fused", prob_head="fused"), dict(resize_head="fused"), dict(area_thd=0.1), dict(pamr_steps=1),
                   dict(blend="hann")):
            plain, idle = _pipe(Q, **kw), _pipe(Q, tta_head="canvas", tta_scales=None, tta_flip=False, **kw)
            for want, given, differs in combos:
                k = 3 if want == "topk" else 0
                if want == "topk" and "area_thd" in kw:
                    continue
                a, b = plain.tail_route(want, k, given, differs), idle.tail_route(want, k, given, differs)
                assert a == b and a.route in (P.HEAD, P.RESIZED_HEAD, P.CANVAS_MULTI, P.CANVAS_EACH)
    K = 5
    fused = _pipe(8, tta_scales=(0.5, 1.0), tta_head="fused")
    auto = _pipe(8, tta_scales=(0.5, 1.0))                                          # "auto" follows the measurement (TTA_AUTO_FUSED)
    assert auto.tail_route("labels").route == (P.TTA_HEAD if P.TTA_AUTO_FUSED else P.TTA_CANVAS)
    assert fused.tail_route("labels") == P.TailRoute(P.TTA_HEAD, 8) and fused.tail_route("probs") == P.TailRoute(P.TTA_HEAD, 8 + 4 * K)
    assert fused.tail_route("labels", differs=True, given=True).route == P.TTA_HEAD
    canvas = _pipe(8, tta_scales=(0.5, 1.0), tta_head="canvas")
    assert canvas.tail_route("labels") == canvas.tail_route("probs") == P.TailRoute(P.TTA_CANVAS, 8 + 8 * K + 4 * 8)
    assert _pipe(65, tta_flip=True).tail_route("probs").route == P.TTA_CANVAS


def test_the_views_of_a_scene():
    """``tta_view_scene``: the scene object itself at its own size; F.interpolate's bilinear resize otherwise, a u8 scene rounded back to
    u8; the flip mirrors the width of either layout."""
    from clip_decontamination_amd.pipeline import tta_view_scene
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (10, 14, 3), generator=g, dtype=torch.uint8)
    f32 = torch.randn(3, 10, 14, generator=g)
    assert tta_view_scene(u8, (10, 14), False) is u8 and tta_view_scene(f32, (10, 14), False) is f32
    assert torch.equal(tta_view_scene(u8, (10, 14), True), torch.flip(u8, dims=[1]))
    assert torch.equal(tta_view_scene(f32, (10, 14), True), torch.flip(f32, dims=[2]))
    up = torch.nn.functional.interpolate(f32[None], size=(13, 18), mode="bilinear", align_corners=False)[0]
    assert torch.equal(tta_view_scene(f32, (13, 18), False), up) and torch.equal(tta_view_scene(f32, (13, 18), True), torch.flip(up, dims=[2]))
    v = tta_view_scene(u8, (5, 7), True)
    ref = torch.nn.functional.interpolate(u8.permute(2, 0, 1).float()[None], size=(5, 7), mode="bilinear", align_corners=False)[0]
    assert v.dtype == torch.uint8 and v.shape == (5, 7, 3) and v.is_contiguous()
    assert torch.equal(v, torch.flip(ref.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0), dims=[1]))
