"""Every refusal of the eighteen head entries of csrc/head.hip (sg_stitch, sg_label_head, sg_prob_head, sg_topk_head, their _blend,
_resized and _multi forms, sg_area_relabel) and of sg_tta_head for the checks it shares with them: the return code is -1 and
``sg_last_error()`` is the expected string, compared whole.  Every check of every entry fires at least once, and for every entry at
least two calls break two checks at once, which pins the order the checks run in.

Every call here is refused before any device work.  The arguments are built from the header's parameter names: without a GPU every
pointer is a never-followed ``c_void_p(8)``; with one, the ``const`` pointers point into a zeroed device buffer and the others into a
second one, each larger than anything the stated shapes address, so that a call let through by mistake launches on valid memory."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")

TALL = 4 * 65536                                                                    # the first height whose rows of 4 leave one launch
BIG = 1 << 31                                                                       # the first block count past INT32_MAX
BASE = dict(T=2, Q=3, gh=4, gw=4, up_h=8, up_w=8, pad_t=0, pad_l=0, H=8, W=8, out_h=8, out_w=8, N=2, total_blocks=2, out_pixels=128,
            canvas_elems=3 * 128, K=3, k=2, bg_idx=0, logit_scale=50.0, prob_thd=0.0, flags=0, ramp_len=4, s=None)
IN_BYTES, OUT_BYTES = 8 << 20, 32 << 20                                            # Q = 5000 below reads 640 KB; H = TALL writes 24 MiB
VIEW = [2, 0, 4, 4, 8, 8, 0, 0, 8, 8, 0]                                            # sg_tta_head's one view: T, first tile, gh, gw, up, pad, h, w, flip
TTA = dict(logit_elems=2 * 3 * 16, total_tiles=2, V=1)

_state = {}


def _params(name):
    if "header" not in _state:
        _state["header"] = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", _state["header"], flags=re.S)
    assert m is not None, f"{name} is not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _pointer(param):
    """A pointer the entry may follow: into the zeroed input buffer for a ``const`` parameter, into the output buffer otherwise."""
    if not torch.cuda.is_available():
        return ctypes.c_void_p(8)
    if "buffers" not in _state:
        _state["buffers"] = (torch.zeros(IN_BYTES, dtype=torch.uint8, device="cuda"), torch.zeros(OUT_BYTES, dtype=torch.uint8, device="cuda"))
    return ctypes.c_void_p(_state["buffers"][0 if param.startswith("const") else 1].data_ptr())


def _call(lib, entry, **kw):
    """``entry`` on BASE with ``kw`` over it; a pointer parameter named in ``kw`` with None is passed as NULL."""
    views = (ctypes.c_int32 * len(VIEW))(*kw.pop("view", VIEW))                    # host memory: the entry reads the table itself
    values = {**BASE, **TTA, **kw}
    args = []
    for p in _params(entry):
        name = p.split()[-1].lstrip("*")
        if name == "s":
            args.append(None)
        elif name == "views":
            args.append(values.get("views", views))
        elif "*" in p:
            args.append(values[name] if name in values else _pointer(p))
        else:
            args.append(values[name])
    rc = getattr(lib, entry)(*args)
    return rc, lib.sg_last_error().decode()


# ---- the rows: (arguments over BASE, the message after "<entry>: ") ------------------------------------------------------------------------
def _nulls(*names):
    return [({n: None}, "null pointer") for n in names]


SHAPE1 = "bad shape T=%d Q=%d gh=%d gw=%d up=%dx%d H=%d W=%d"
SHAPE1_ROWS = [(dict(T=0), SHAPE1 % (0, 3, 4, 4, 8, 8, 8, 8)), (dict(Q=0, K=0), SHAPE1 % (2, 0, 4, 4, 8, 8, 8, 8)),
               (dict(gh=0), SHAPE1 % (2, 3, 0, 4, 8, 8, 8, 8)), (dict(gw=-1), SHAPE1 % (2, 3, 4, -1, 8, 8, 8, 8)),
               (dict(up_h=0), SHAPE1 % (2, 3, 4, 4, 0, 8, 8, 8)), (dict(up_w=0), SHAPE1 % (2, 3, 4, 4, 8, 0, 8, 8)),
               (dict(pad_t=-1), SHAPE1 % (2, 3, 4, 4, 8, 8, 8, 8)), (dict(pad_l=-1), SHAPE1 % (2, 3, 4, 4, 8, 8, 8, 8)),
               (dict(H=0), SHAPE1 % (2, 3, 4, 4, 8, 8, 0, 8)), (dict(W=0), SHAPE1 % (2, 3, 4, 4, 8, 8, 8, 0))]
SHAPE1R = SHAPE1 + " out=%dx%d"
SHAPE1R_ROWS = [(kw, msg + " out=8x8") for kw, msg in SHAPE1_ROWS] + \
               [(dict(out_h=0), SHAPE1R % (2, 3, 4, 4, 8, 8, 8, 8, 0, 8)), (dict(out_w=-2), SHAPE1R % (2, 3, 4, 4, 8, 8, 8, 8, 8, -2))]
SHAPEN = "bad shape T=%d Q=%d gh=%d gw=%d N=%d"
SHAPEN_ROWS = [(dict(T=0), SHAPEN % (0, 3, 4, 4, 2)), (dict(Q=0, K=0), SHAPEN % (2, 0, 4, 4, 2)), (dict(gh=0), SHAPEN % (2, 3, 0, 4, 2)),
               (dict(gw=0), SHAPEN % (2, 3, 4, 0, 2)), (dict(up_h=0), SHAPEN % (2, 3, 4, 4, 2)), (dict(up_w=-1), SHAPEN % (2, 3, 4, 4, 2)),
               (dict(pad_t=-1), SHAPEN % (2, 3, 4, 4, 2)), (dict(pad_l=-3), SHAPEN % (2, 3, 4, 4, 2)), (dict(N=0), SHAPEN % (2, 3, 4, 4, 0)),
               (dict(N=3), SHAPEN % (2, 3, 4, 4, 3))]
STITCH_ROWS = [(dict(T=0), "bad shape"), (dict(Q=0), "bad shape"), (dict(gh=0), "bad shape"), (dict(gw=0), "bad shape"),
               (dict(H=0), "bad shape"), (dict(W=-1), "bad shape")]
CANVAS_TALL, OUTPUT_TALL = "canvas too tall for one launch", "output too tall for one launch"
K_ROWS = [(dict(K=0), "K=0 must lie in [1, Q=3]"), (dict(K=4), "K=4 must lie in [1, Q=3]"), (dict(K=-1), "K=-1 must lie in [1, Q=3]")]
TOPK_ROWS = [(dict(k=0), "k=0 must lie in [1, min(8, K=3)]"), (dict(k=4), "k=4 must lie in [1, min(8, K=3)]"),
             (dict(Q=12, K=12, k=9), "k=9 must lie in [1, min(8, K=12)]"), (dict(K=1, k=2), "k=2 must lie in [1, min(8, K=1)]")]
BG_ROWS = [(dict(bg_idx=-1), "bg_idx=-1 outside [0, K=3)"), (dict(bg_idx=3), "bg_idx=3 outside [0, K=3)")]
BLOCKS = "total_blocks=%d outside (0, 2^31)"
BLOCK_ROWS = [(dict(total_blocks=0), BLOCKS % 0), (dict(total_blocks=-5), BLOCKS % -5), (dict(total_blocks=BIG), BLOCKS % BIG)]
PIXEL_ROWS = [(dict(out_pixels=0), "out_pixels=0 holds no image"), (dict(out_pixels=-7), "out_pixels=-7 holds no image")]
CANVAS_ROWS = [(dict(canvas_elems=2), "canvas_elems=2 holds no canvas"), (dict(canvas_elems=-1), "canvas_elems=-1 holds no canvas")]
NULL_RAMP = "null ramp"
RAMP_ROWS = [(dict(ramp=None), NULL_RAMP), (dict(ramp_len=0), "ramp_len=0 outside [1, 2048]"), (dict(ramp_len=2049), "ramp_len=2049 outside [1, 2048]")]
FLAGS = "flags=%d is no SG_RESIZED_* value"
FLAG_ROWS = [(dict(flags=3), FLAGS % 3), (dict(flags=-1), FLAGS % -1)]
NO_FIT = "the staged form does not fit: a block's footprint of 34 x 514 canvas pixels exceeds the stage of 512"
FIT_ROWS = [(dict(flags=2, out_h=1, out_w=1), NO_FIT)]                              # 4 * 8 / 1 + 2 rows by 64 * 8 / 1 + 2 columns of canvas
AREA_K = "K=5000 exceeds 4096 (SG_AREA_MAX_K, the limit of sg_class_area)"
AREA_K_ROWS = [(dict(Q=5000, K=5000), AREA_K)]
MULTI_IN = ("tile_logits", "windows", "tile_image", "image_hw", "image_tiles", "block_prefix")
PROBS_NULL = "probs is NULL (labels alone: %s)"

TABLE = {
    # ---- the stitch: a bare "bad shape" that leaves up_h, up_w, pad_t and pad_l alone ----
    "sg_stitch": _nulls("tile_logits", "windows", "canvas") + STITCH_ROWS + [
        (dict(H=TALL), CANVAS_TALL),
        (dict(canvas=None, T=0), "null pointer"), (dict(T=0, H=TALL), "bad shape"), (dict(windows=None, H=TALL), "null pointer")],
    "sg_stitch_blend": _nulls("tile_logits", "windows", "canvas") + RAMP_ROWS + STITCH_ROWS + [
        (dict(H=TALL), CANVAS_TALL),
        (dict(canvas=None, ramp=None), "null pointer"), (dict(ramp=None, T=0), NULL_RAMP), (dict(ramp=None, ramp_len=0), NULL_RAMP),
        (dict(ramp_len=0, Q=0), "ramp_len=0 outside [1, 2048]"), (dict(W=0, H=TALL), "bad shape")],
    "sg_stitch_multi": _nulls(*MULTI_IN, "canvas_offset", "canvases") + SHAPEN_ROWS + BLOCK_ROWS + CANVAS_ROWS + [
        (dict(canvases=None, N=0), "null pointer"), (dict(N=0, total_blocks=0), SHAPEN % (2, 3, 4, 4, 0)),
        (dict(total_blocks=0, canvas_elems=0), BLOCKS % 0)],
    "sg_stitch_blend_multi": _nulls(*MULTI_IN, "canvas_offset", "canvases") + RAMP_ROWS + SHAPEN_ROWS + BLOCK_ROWS + CANVAS_ROWS + [
        (dict(tile_image=None, ramp=None), "null pointer"), (dict(ramp=None, T=0), NULL_RAMP),
        (dict(ramp_len=2049, N=3), "ramp_len=2049 outside [1, 2048]"), (dict(up_h=0, total_blocks=BIG), SHAPEN % (2, 3, 4, 4, 2)),
        (dict(total_blocks=BIG, canvas_elems=1), BLOCKS % BIG)],
    # ---- the label head ----
    "sg_label_head": _nulls("tile_logits", "windows", "query_idx", "labels") + SHAPE1_ROWS + K_ROWS + [
        (dict(H=TALL), CANVAS_TALL),
        (dict(labels=None, T=0), "null pointer"), (dict(T=0, K=4), SHAPE1 % (0, 3, 4, 4, 8, 8, 8, 8)),
        (dict(K=4, H=TALL), "K=4 must lie in [1, Q=3]")],
    "sg_label_head_multi": _nulls(*MULTI_IN, "out_offset", "query_idx", "labels") + SHAPEN_ROWS + K_ROWS + BLOCK_ROWS + PIXEL_ROWS + [
        (dict(query_idx=None, N=0), "null pointer"), (dict(N=3, K=0), SHAPEN % (2, 3, 4, 4, 3)),
        (dict(K=4, total_blocks=0), "K=4 must lie in [1, Q=3]"), (dict(total_blocks=0, out_pixels=0), BLOCKS % 0)],
    "sg_label_head_blend": _nulls("tile_logits", "windows", "query_idx", "labels") + RAMP_ROWS + SHAPE1_ROWS + K_ROWS + [
        (dict(H=TALL), CANVAS_TALL),
        (dict(labels=None, ramp=None), "null pointer"), (dict(ramp=None, T=0), NULL_RAMP),
        (dict(ramp_len=0, K=4), "ramp_len=0 outside [1, 2048]"), (dict(up_w=0, K=4), SHAPE1 % (2, 3, 4, 4, 8, 0, 8, 8)),
        (dict(K=0, H=TALL), "K=0 must lie in [1, Q=3]")],
    "sg_label_head_blend_multi": _nulls(*MULTI_IN, "out_offset", "query_idx", "labels") + RAMP_ROWS + SHAPEN_ROWS + K_ROWS + BLOCK_ROWS +
    PIXEL_ROWS + [
        (dict(image_hw=None, ramp_len=0), "null pointer"), (dict(ramp=None, N=0), NULL_RAMP),
        (dict(ramp_len=0, total_blocks=0), "ramp_len=0 outside [1, 2048]"), (dict(T=0, K=4), SHAPEN % (0, 3, 4, 4, 2)),
        (dict(K=4, out_pixels=0), "K=4 must lie in [1, Q=3]"), (dict(total_blocks=-5, out_pixels=0), BLOCKS % -5)],
    # ---- the probability head: probs has a refusal of its own, after the other pointers ----
    "sg_prob_head": _nulls("tile_logits", "windows", "query_idx", "labels") + [(dict(probs=None), PROBS_NULL % "sg_label_head")] +
    SHAPE1_ROWS + K_ROWS + [
        (dict(H=TALL), CANVAS_TALL),
        (dict(labels=None, probs=None), "null pointer"), (dict(probs=None, T=0), PROBS_NULL % "sg_label_head"),
        (dict(H=0, K=4), SHAPE1 % (2, 3, 4, 4, 8, 8, 0, 8)), (dict(K=4, H=TALL), "K=4 must lie in [1, Q=3]")],
    "sg_prob_head_multi": _nulls(*MULTI_IN, "out_offset", "query_idx", "labels") + [(dict(probs=None), PROBS_NULL % "sg_label_head_multi")] +
    SHAPEN_ROWS + K_ROWS + BLOCK_ROWS + PIXEL_ROWS + [
        (dict(windows=None, probs=None), "null pointer"), (dict(probs=None, N=0), PROBS_NULL % "sg_label_head_multi"),
        (dict(N=0, K=0), SHAPEN % (2, 3, 4, 4, 0)), (dict(K=0, total_blocks=0), "K=0 must lie in [1, Q=3]"),
        (dict(total_blocks=BIG, out_pixels=-7), BLOCKS % BIG)],
    # ---- the top-k head ----
    "sg_topk_head": _nulls("tile_logits", "windows", "query_idx", "classes", "probs") + SHAPE1_ROWS + K_ROWS + TOPK_ROWS + [
        (dict(H=TALL), CANVAS_TALL),
        (dict(classes=None, W=0), "null pointer"), (dict(T=0, k=0), SHAPE1 % (0, 3, 4, 4, 8, 8, 8, 8)),
        (dict(K=4, k=0), "K=4 must lie in [1, Q=3]"), (dict(k=0, H=TALL), "k=0 must lie in [1, min(8, K=3)]")],
    "sg_topk_head_multi": _nulls(*MULTI_IN, "out_offset", "query_idx", "classes", "probs") + SHAPEN_ROWS + K_ROWS + TOPK_ROWS + BLOCK_ROWS +
    PIXEL_ROWS + [
        (dict(probs=None, N=0), "null pointer"), (dict(gw=0, K=4), SHAPEN % (2, 3, 4, 0, 2)), (dict(K=4, k=0), "K=4 must lie in [1, Q=3]"),
        (dict(k=4, total_blocks=0), "k=4 must lie in [1, min(8, K=3)]"), (dict(total_blocks=0, out_pixels=0), BLOCKS % 0)],
    # ---- the heads at another output size: "output too tall", then the flags, then the staged fit ----
    "sg_label_head_resized": _nulls("tile_logits", "windows", "query_idx", "labels") + SHAPE1R_ROWS + K_ROWS + FLAG_ROWS + FIT_ROWS + [
        (dict(out_h=TALL), OUTPUT_TALL),
        (dict(tile_logits=None, out_h=0), "null pointer"), (dict(out_w=0, K=4), SHAPE1R % (2, 3, 4, 4, 8, 8, 8, 8, 8, 0)),
        (dict(K=4, out_h=TALL), "K=4 must lie in [1, Q=3]"), (dict(out_h=TALL, flags=3), OUTPUT_TALL),
        (dict(K=0, flags=2, out_h=1, out_w=1), "K=0 must lie in [1, Q=3]")],
    "sg_label_head_resized_multi": _nulls(*MULTI_IN, "out_hw", "out_offset", "query_idx", "labels") + SHAPEN_ROWS + K_ROWS + BLOCK_ROWS +
    PIXEL_ROWS + FLAG_ROWS + [
        (dict(out_hw=None, T=0), "null pointer"), (dict(T=0, K=4), SHAPEN % (0, 3, 4, 4, 2)),
        (dict(K=4, total_blocks=0), "K=4 must lie in [1, Q=3]"), (dict(total_blocks=0, out_pixels=0), BLOCKS % 0),
        (dict(out_pixels=0, flags=3), "out_pixels=0 holds no image")],
    "sg_topk_head_resized": _nulls("tile_logits", "windows", "query_idx", "classes", "probs") + SHAPE1R_ROWS + K_ROWS + TOPK_ROWS + FLAG_ROWS +
    FIT_ROWS + [
        (dict(out_h=TALL), OUTPUT_TALL),
        (dict(probs=None, k=0), "null pointer"), (dict(H=0, K=4), SHAPE1R % (2, 3, 4, 4, 8, 8, 0, 8, 8, 8)),
        (dict(K=4, k=0), "K=4 must lie in [1, Q=3]"), (dict(k=0, out_h=TALL), "k=0 must lie in [1, min(8, K=3)]"),
        (dict(out_h=TALL, flags=-1), OUTPUT_TALL), (dict(k=4, flags=2, out_h=1, out_w=1), "k=4 must lie in [1, min(8, K=3)]")],
    "sg_topk_head_resized_multi": _nulls(*MULTI_IN, "out_hw", "out_offset", "query_idx", "classes", "probs") + SHAPEN_ROWS + K_ROWS + TOPK_ROWS +
    BLOCK_ROWS + PIXEL_ROWS + FLAG_ROWS + [
        (dict(classes=None, N=0), "null pointer"), (dict(N=0, K=4), SHAPEN % (2, 3, 4, 4, 0)), (dict(K=4, k=0), "K=4 must lie in [1, Q=3]"),
        (dict(k=0, total_blocks=0), "k=0 must lie in [1, min(8, K=3)]"), (dict(total_blocks=0, out_pixels=0), BLOCKS % 0),
        (dict(out_pixels=0, flags=3), "out_pixels=0 holds no image")],
    # ---- the second decision of area_thd: K against SG_AREA_MAX_K and the background index between K and the launch limits ----
    "sg_area_relabel": _nulls("tile_logits", "windows", "query_idx", "keep", "conf", "labels") + SHAPE1_ROWS + K_ROWS + AREA_K_ROWS + BG_ROWS + [
        (dict(H=TALL), CANVAS_TALL),
        (dict(keep=None, T=0), "null pointer"), (dict(T=0, K=4), SHAPE1 % (0, 3, 4, 4, 8, 8, 8, 8)),
        (dict(K=4, bg_idx=-1), "K=4 must lie in [1, Q=3]"), (dict(Q=5000, K=5000, bg_idx=-1), AREA_K),
        (dict(bg_idx=3, H=TALL), "bg_idx=3 outside [0, K=3)")],
    "sg_area_relabel_multi": _nulls(*MULTI_IN, "out_offset", "query_idx", "keep", "conf", "labels") + SHAPEN_ROWS + K_ROWS + AREA_K_ROWS + BG_ROWS +
    BLOCK_ROWS + PIXEL_ROWS + [
        (dict(conf=None, N=0), "null pointer"), (dict(N=0, K=4), SHAPEN % (2, 3, 4, 4, 0)),
        (dict(K=0, bg_idx=0), "K=0 must lie in [1, Q=3]"), (dict(Q=5000, K=5000, bg_idx=5000), AREA_K),
        (dict(bg_idx=-1, total_blocks=0), "bg_idx=-1 outside [0, K=3)"), (dict(total_blocks=0, out_pixels=0), BLOCKS % 0)],
    # ---- sg_tta_head: the checks it shares (K, the background index, the flags) among its own ----
    "sg_tta_head": _nulls("tile_logits", "windows", "views", "query_idx", "labels") + K_ROWS + BG_ROWS + FLAG_ROWS + [
        (dict(V=0), "V=0 views, must lie in [1, 8]"), (dict(Q=65, K=65), "Q=65 must lie in [1, 64] (more queries: sg_tta_accumulate / sg_tta_finish)"),
        (dict(out_h=0), "bad output size 0x8"), (dict(out_h=TALL), OUTPUT_TALL),
        (dict(view=[0] + VIEW[1:]), "view 0 has a bad shape T=0 gh=4 gw=4 up=8x8 pad=0,0 H=8 W=8"),
        (dict(V=9, K=4), "V=9 views, must lie in [1, 8]"), (dict(Q=0, K=0), "Q=0 must lie in [1, 64] (more queries: sg_tta_accumulate / sg_tta_finish)"),
        (dict(K=4, bg_idx=-1), "K=4 must lie in [1, Q=3]"), (dict(bg_idx=3, out_w=0), "bg_idx=3 outside [0, K=3)"),
        (dict(bg_idx=3, flags=3), "bg_idx=3 outside [0, K=3)"), (dict(out_h=TALL, flags=3), OUTPUT_TALL),
        (dict(flags=3, view=[0] + VIEW[1:]), FLAGS % 3)],
}


def test_the_table_names_every_head_entry_and_the_tta_head():
    from clip_decontamination_amd import _lib
    family = [n for n in _lib.SIGNATURES if re.match(r"sg_(stitch|label_head|prob_head|topk_head|area_relabel)", n)]
    assert len(family) == 18 and sorted(family + ["sg_tta_head"]) == sorted(TABLE)


@pytest.mark.parametrize("entry", sorted(TABLE))
def test_every_refusal_is_the_expected_one(entry):
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    for kw, msg in TABLE[entry]:
        rc, err = _call(lib, entry, **kw)
        assert rc == -1 and err == f"{entry}: {msg}", (entry, kw, rc, err)
