"""Weighted window blending at the drop-in boundary, without a GPU: include/segearth_hip.h declares the four entries with their
counterparts' parameters plus (ramp, ramp_len), the library exports them and the ctypes table carries them; each refuses a null ramp
and a ramp_len outside [1, SG_BLEND_MAX_RAMP] through the error channel before any device work; ``ops.blend_args`` refuses what the
constructors refuse; and, with the recorder ops of tools/record_tail_routes.py, ``blend="hann"`` sends plain labels to
label_head_blend[_multi] and everything else to stitch_blend[_multi] while ``blend="uniform"`` makes exactly the calls of an instance
built without the option."""
import ctypes
import importlib.util
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
PAIRS = {"sg_stitch_blend": "sg_stitch", "sg_stitch_blend_multi": "sg_stitch_multi", "sg_label_head_blend": "sg_label_head",
         "sg_label_head_blend_multi": "sg_label_head_multi"}


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
    for new, old in PAIRS.items():
        pn, po = _params(new), _params(old)
        assert pn is not None, f"{new} is not declared in the header"
        assert hasattr(lib, new), f"{new} declared in the header but not exported"
        # the counterpart's parameters, then the ramp in front of the stream
        assert pn == po[:-1] + ["const float* ramp", "int ramp_len", po[-1]], (new, pn)
        res, args = _lib.SIGNATURES[new]
        assert res is ctypes.c_int and args == [_ctype(p) for p in pn]
        assert len(args) == len(_lib.SIGNATURES[old][1]) + 2
        assert _lib.SIGNATURES[old][1] == [_ctype(p) for p in po]                  # the existing entries are what they were
    m = re.search(r"#define\s+SG_BLEND_MAX_RAMP\s+(\d+)", _header())
    assert m and int(m.group(1)) == ops.BLEND_MAX_RAMP == 2048
    for name in ("blend_ramp", "blend_args", "blend_table", "stitch_blend", "stitch_blend_multi", "label_head_blend", "label_head_blend_multi"):
        assert callable(getattr(ops, name)), name


def test_entries_refuse_a_bad_ramp_before_any_device_work():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                                        # a non-null pointer that is never followed
    big = 2049

    def calls(ramp, n):
        return {
            "sg_stitch_blend": lambda: lib.sg_stitch_blend(one, one, 1, 3, 2, 2, 4, 4, 0, 0, 4, 4, one, ramp, n, None),
            "sg_stitch_blend_multi": lambda: lib.sg_stitch_blend_multi(one, one, one, 1, 3, 2, 2, 4, 4, 0, 0, one, one, one, one, 1, 1, 48, one,
                                                                       ramp, n, None),
            "sg_label_head_blend": lambda: lib.sg_label_head_blend(one, one, 1, 3, 2, 2, 4, 4, 0, 0, 4, 4, one, 3, 50.0, 0.0, 0, one, one,
                                                                   ramp, n, None),
            "sg_label_head_blend_multi": lambda: lib.sg_label_head_blend_multi(one, one, one, 1, 3, 2, 2, 4, 4, 0, 0, one, one, one, one, 1, 1, 16,
                                                                               one, 3, 50.0, 0.0, 0, one, one, ramp, n, None),
        }

    for ramp, n, word in ((None, 4, "null ramp"), (one, 0, "ramp_len=0"), (one, -3, "ramp_len=-3"), (one, big, f"ramp_len={big}")):
        for name, fn in calls(ramp, n).items():
            rc = fn()
            err = lib.sg_last_error().decode()
            assert rc == -1 and name + ":" in err and word in err, (name, word, rc, err)
    # the counterpart's own checks still stand
    assert lib.sg_stitch_blend(None, one, 1, 3, 2, 2, 4, 4, 0, 0, 4, 4, one, one, 4, None) == -1
    assert "sg_stitch_blend: null pointer" in lib.sg_last_error().decode()
    assert lib.sg_label_head_blend(one, one, 1, 3, 2, 2, 4, 4, 0, 0, 4, 4, one, 4, 50.0, 0.0, 0, one, one, one, 4, None) == -1
    assert "K=4 must lie in" in lib.sg_last_error().decode()


def test_blend_args():
    from clip_decontamination_amd import ops, pipeline
    assert ops.blend_args("uniform") == ("uniform", None)
    assert ops.blend_args("hann", 16) == ("hann", 16) and ops.blend_args("linear", 2047) == ("linear", 2047)
    for kind in ("cosine", "Hann", None, 1):
        with pytest.raises(ValueError, match="blend must be one of"):
            ops.blend_args(kind)
    for R in (0, -1, 2048, 1.5, "4", True):
        with pytest.raises(ValueError, match="blend_ramp must be"):
            ops.blend_args("hann", R)
    with pytest.raises(ValueError, match="blend_ramp must be"):
        ops.blend_ramp("hann", 0)
    off = pipeline.SegPipeline.__new__(pipeline.SegPipeline)                        # the class-level defaults: off
    assert off.blend == "uniform" and off.blend_ramp is None and off._ramp((32, 32)) is None
    net = types.SimpleNamespace(visual=types.SimpleNamespace(device="cpu", cfg=types.SimpleNamespace(patch=16, embed_dim=8)))
    import torch
    for kw, word in ((dict(blend="box"), "blend must be one of"), (dict(blend="hann", blend_ramp=0), "blend_ramp must be")):
        with pytest.raises(ValueError, match=word):
            pipeline.SegPipeline(net, torch.zeros(8, 8), torch.arange(8) % 5, **kw)
    pipe = pipeline.SegPipeline(net, torch.zeros(8, 8), torch.arange(8) % 5, blend="hann")
    assert pipe._ramp((32, 48)).numel() == 17 and pipe._ramp((1, 9)).numel() == 2    # R = max(1, min(h, w) // 2), L = R + 1
    assert pipe._ramp((32, 48)) is pipe._ramp((40, 32))                              # one table per (kind, R, device)
    with pytest.raises(ValueError, match="window size is not known"):
        pipe._ramp(None)
    assert pipeline.SegPipeline(net, torch.zeros(8, 8), torch.arange(8) % 5, blend="linear", blend_ramp=5)._ramp(None).numel() == 6


# ---- routes, with the recorder ops of tools/record_tail_routes.py ---------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("record_tail_routes", os.path.join(ROOT, "tools", "record_tail_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _routes(entry, wanted, Q, **options):
    """The ops calls of ``entry`` for ``wanted`` on the recorder's three images, as record_tail_routes.record() notes them; the blended
    ops are recorded under their own names and return what their unweighted recorders return."""
    import torch
    from clip_decontamination_amd import ops, pipeline
    tool = _tool()
    log = []
    stand_ins = tool._recorders(torch, log)

    def blended(name, n_lead):
        plain = stand_ins[name.replace("_blend", "")]

        def fn(*args, **kw):
            ramp = args[-1] if name.startswith("stitch") else args[n_lead]
            rest = args[:-1] if name.startswith("stitch") else args[:n_lead] + args[n_lead + 1:]
            out = plain(*rest, **kw)
            log[-1] = log[-1].replace(name.replace("_blend", "") + "(", name + f"(L={ramp.numel()},", 1)
            return out
        return fn

    stand_ins.update(stitch_blend=blended("stitch_blend", 0), stitch_blend_multi=blended("stitch_blend_multi", 0),
                     label_head_blend=blended("label_head_blend", 10), label_head_blend_multi=blended("label_head_blend_multi", 12))
    saved = {name: getattr(ops, name) for name in stand_ins}
    net = types.SimpleNamespace(visual=types.SimpleNamespace(device=torch.device("cpu"), cfg=types.SimpleNamespace(patch=16, embed_dim=8)))
    scenes = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in tool.IMAGES]
    try:
        for name, fn in stand_ins.items():
            setattr(ops, name, fn)
        pipe = pipeline.SegPipeline(net, torch.zeros(Q, 8), torch.arange(Q) % tool.K, prob_thd=tool.PROB_THD, **options)
        pipe._packed_tile_logits = lambda buf, g, f: torch.zeros(f.tile_hi - f.tile_lo, Q, 2, 2)
        pipe.tile_logits = lambda scene, windows, tile_hw, scene_index=None, grid_of_tiles=None: torch.zeros(len(windows), Q, 2, 2)
        kw = {"want_probs": wanted == "probs", "topk": 3 if wanted == "topk3" else 0}
        if entry == "segment_scenes":
            pipe.segment_scenes(scenes, tool.STRIDE, tool.CROP, **kw)
        else:
            for s in scenes:
                pipe.segment_scene(s, tool.STRIDE, tool.CROP, **kw)
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    return log


def _names(log):
    return [c.split("(")[0] for c in log]


GATHERS = {"stitch", "stitch_multi", "label_head", "label_head_multi", "prob_head", "prob_head_multi", "topk_head", "topk_head_multi",
           "label_head_resized", "label_head_resized_multi", "topk_head_resized", "topk_head_resized_multi", "area_relabel", "area_relabel_multi"}


@pytest.mark.parametrize("entry", ["segment_scene", "segment_scenes"])
def test_hann_sends_plain_labels_to_the_blended_label_head(entry):
    multi = "_multi" if entry == "segment_scenes" else ""
    log = _routes(entry, "labels", 65, blend="hann")
    names = _names(log)
    assert set(names) == {"label_head_blend" + multi}, log
    # the recorder's images: two with 32 x 32 windows (R = 16), one of 24 x 24 (R = 12)
    assert sorted({c.split(",")[0] for c in log}) == [f"label_head_blend{multi}(L=13", f"label_head_blend{multi}(L=17"], log
    assert _names(_routes(entry, "labels", 65, blend="hann", blend_ramp=5)) == names
    assert set(_names(_routes(entry, "labels", 8, blend="linear", label_head="fused"))) == {"label_head_blend" + multi}


@pytest.mark.parametrize("entry", ["segment_scene", "segment_scenes"])
@pytest.mark.parametrize("wanted,Q,options", [("probs", 65, {}), ("probs", 8, dict(prob_head="fused")), ("topk3", 65, {}), ("topk3", 8, {}),
                                              ("labels", 8, {}), ("labels", 65, dict(area_thd=0.1)),
                                              ("labels", 8, dict(area_thd=0.1, label_head="fused")), ("labels", 65, dict(pamr_steps=2)),
                                              ("labels", 65, dict(label_head="canvas"))])
def test_hann_sends_everything_else_to_the_blended_stitch(entry, wanted, Q, options):
    multi = "_multi" if entry == "segment_scenes" else ""
    log = _routes(entry, wanted, Q, blend="hann", **options)
    names = _names(log)
    assert "stitch_blend" + multi in names and not GATHERS & set(names), log          # no unweighted gather runs behind a blended one
    if wanted == "topk3":
        assert "topk_from_probs" in names
    # the rest of the canvas route is the unweighted call's: the same calls with stitch[_multi] in place of the blended one
    if wanted != "topk3":                                                           # (unweighted top-k without PAMR is a head, no canvas)
        plain = _routes(entry, wanted, Q, **dict(options, label_head="canvas", prob_head="canvas"))
        assert [re.sub(r"^stitch_blend(_multi)?\(L=\d+,", r"stitch\1(", c) for c in log] == plain


@pytest.mark.parametrize("entry", ["segment_scene", "segment_scenes"])
@pytest.mark.parametrize("wanted", ["labels", "probs", "topk3"])
@pytest.mark.parametrize("Q", [8, 65])
def test_uniform_makes_exactly_the_calls_of_an_instance_without_the_option(entry, wanted, Q):
    for options in ({}, dict(label_head="fused", prob_head="fused"), dict(area_thd=0.1) if wanted != "topk3" else {}):
        off = _routes(entry, wanted, Q, blend="uniform", blend_ramp=9, **options)
        assert off == _routes(entry, wanted, Q, **options)
        assert not any("blend" in c for c in off)
