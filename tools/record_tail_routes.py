#!/usr/bin/env python3
"""Records which ops calls every tail of SegPipeline makes, on the CPU, with no library load (tests/test_tail_routes_cpu.py).

A SegPipeline is built over a stub net; the ``ops`` functions the tails call are replaced by recorders that note their name and the
arguments that decide a route (prob_thd, k, want_probs, want_conf, form, the sizes) and return zero tensors of the right shapes and
dtypes; ``_packed_tile_logits`` and ``tile_logits`` return zero tile logits; ``pipeline.plan_images`` is wrapped to note the
``pixel_bytes`` the planner is given, evaluated per image.  Only names that the pipeline keeps stable are hooked, so the same recorder
runs on any commit:

    python tools/record_tail_routes.py --repo <checkout of the commit to record> --out tests/tail_routes_cpu.json

``record()`` enumerates the cross product of AXES and returns {"axes", "calls", "sequences", "cases"}: ``cases[i]`` is, for the i-th
element of the product in itertools order, an index into ``sequences``, whose entries are lists of indices into ``calls`` (strings).
A case that raises is recorded as the calls up to there plus the exception type and the first words of its message.
"""
import argparse
import itertools
import json
import os
import sys
import types

AXES = (
    ("entry", ("segment_scene", "segment_scenes")),
    ("wanted", ("labels", "probs", "topk3")),
    ("ori_shapes", ("none", "equal", "one_differs")),
    ("label_head", ("auto", "fused", "canvas")),
    ("prob_head", ("auto", "fused", "canvas")),
    ("resize_head", ("canvas", "fused")),
    ("pamr", (0, 2)),
    ("area_thd", (None, 0.1)),
    ("Q", (8, 65)),
    ("flush_bytes", ("default", 1)),
)
IMAGES = ((40, 56), (40, 56), (24, 24))          # two share a window size (32 x 32 at crop 32), the third is smaller than the crop
ORI = {"none": None, "equal": [(40, 56), (40, 56), (24, 24)], "one_differs": [(40, 56), (50, 70), (24, 24)]}
CROP, STRIDE, K, PROB_THD = 32, 16, 5, 0.25


def case_keys():
    return [dict(zip([n for n, _ in AXES], v)) for v in itertools.product(*[vals for _, vals in AXES])]


def _hw(hw):
    return "x".join(str(int(v)) for v in hw)


def _hws(hws):
    return "[" + ",".join(_hw(hw) for hw in hws) + "]"


def _shape(x):
    import torch
    if torch.is_tensor(x):
        return str(x.dtype).replace("torch.", "") + _hw(x.shape).join("[]")
    if isinstance(x, (list, tuple)):
        return "(" + ",".join(_shape(v) for v in x) + ")"
    return repr(x)


def _recorders(torch, log):
    """name -> stand-in for ops.<name>, same signature as the real one."""
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    z = torch.zeros

    def prefix(counts):
        out = [0]
        for c in counts:
            out.append(out[-1] + int(c))
        return out

    def views(flat, planes, hws):
        pix = prefix(h * w for h, w in hws)
        return [flat[planes * pix[n]:planes * pix[n + 1]].view(planes, h, w) for n, (h, w) in enumerate(hws)]

    def stitch(tile_logits, windows, up_hw, pad_tl, canvas_hw):
        log.append(f"stitch(hw={_hw(canvas_hw)},T={tile_logits.shape[0]})")
        return z(tile_logits.shape[1], *canvas_hw)

    def stitch_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles):
        log.append(f"stitch_multi(hw={_hws(image_hw)},T={tile_logits.shape[0]})")
        Q = tile_logits.shape[1]
        flat = z(Q * sum(h * w for h, w in image_hw))
        return flat, views(flat, Q, image_hw)

    def resize_bilinear(src, size):
        log.append(f"resize_bilinear(C={src.shape[0]},from={_hw(src.shape[1:])},to={_hw(size)})")
        return z(src.shape[0], *size)

    def postprocess(logits, query_idx, num_classes, logit_scale, prob_thd, bg_idx, want_probs=True):
        log.append(f"postprocess(Q={logits.shape[0]},hw={_hw(logits.shape[1:])},prob_thd={float(prob_thd)},want_probs={bool(want_probs)})")
        H, W = logits.shape[1:]
        return (z(num_classes, H, W) if want_probs else None), z(1, H, W, dtype=i64)

    def postprocess_multi(canvases, canvas_hw, query_idx, num_classes, logit_scale, prob_thd, bg_idx, out_hw=None, want_probs=True,
                          canvas_offsets=None, flat_labels=False, flat_probs=False):
        out_hw = list(canvas_hw) if out_hw is None else [tuple(s) for s in out_hw]
        log.append(f"postprocess_multi(from={_hws(canvas_hw)},to={_hws(out_hw)},prob_thd={float(prob_thd)},want_probs={bool(want_probs)},"
                   f"flat_labels={bool(flat_labels)},flat_probs={bool(flat_probs)})")
        n = sum(h * w for h, w in out_hw)
        labels, probs = z(n, dtype=i64), (z(num_classes * n) if want_probs else None)
        lab = [v.view(1, *v.shape[1:]) for v in views(labels, 1, out_hw)]
        prb = views(probs, num_classes, out_hw) if want_probs else [None] * len(out_hw)
        if flat_labels and flat_probs:
            return prb, lab, labels, probs
        return (prb, lab, labels) if flat_labels else (prb, lab)

    def label_head(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes, logit_scale, prob_thd, bg_idx, want_conf=False):
        log.append(f"label_head(hw={_hw(canvas_hw)},prob_thd={float(prob_thd)},want_conf={bool(want_conf)})")
        labels = z(1, *canvas_hw, dtype=i64)
        return (labels, z(*canvas_hw)) if want_conf else labels

    def label_head_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes, logit_scale,
                         prob_thd, bg_idx, want_conf=False, flat_conf=False):
        log.append(f"label_head_multi(hw={_hws(image_hw)},prob_thd={float(prob_thd)},want_conf={bool(want_conf)},flat_conf={bool(flat_conf)})")
        n = sum(h * w for h, w in image_hw)
        labels, conf = z(n, dtype=i64), z(n)
        lab = views(labels, 1, image_hw)
        if want_conf:
            return lab, labels, (conf if flat_conf else [v[0] for v in views(conf, 1, image_hw)])
        return lab, labels

    def prob_head(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes, logit_scale, prob_thd, bg_idx):
        log.append(f"prob_head(hw={_hw(canvas_hw)},prob_thd={float(prob_thd)})")
        return z(num_classes, *canvas_hw), z(1, *canvas_hw, dtype=i64)

    def prob_head_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes, logit_scale,
                        prob_thd, bg_idx, flat_probs=False):
        log.append(f"prob_head_multi(hw={_hws(image_hw)},prob_thd={float(prob_thd)},flat_probs={bool(flat_probs)})")
        n = sum(h * w for h, w in image_hw)
        labels, probs = z(n, dtype=i64), z(num_classes * n)
        prb, lab = views(probs, num_classes, image_hw), views(labels, 1, image_hw)
        return (prb, lab, labels, probs) if flat_probs else (prb, lab, labels)

    def topk_head(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes, logit_scale, k):
        log.append(f"topk_head(hw={_hw(canvas_hw)},k={int(k)})")
        return z(k, *canvas_hw, dtype=i32), z(k, *canvas_hw)

    def topk_head_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes, logit_scale, k):
        log.append(f"topk_head_multi(hw={_hws(image_hw)},k={int(k)})")
        n = sum(h * w for h, w in image_hw)
        return views(z(k * n, dtype=i32), k, image_hw), views(z(k * n), k, image_hw)

    def label_head_resized(tile_logits, windows, up_hw, pad_tl, canvas_hw, out_hw, query_idx, num_classes, logit_scale, prob_thd, bg_idx,
                           want_conf=False, form="auto"):
        log.append(f"label_head_resized(from={_hw(canvas_hw)},to={_hw(out_hw)},prob_thd={float(prob_thd)},want_conf={bool(want_conf)},form={form})")
        labels = z(1, *out_hw, dtype=i64)
        return (labels, z(*out_hw)) if want_conf else labels

    def label_head_resized_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, out_hw, query_idx, num_classes,
                                 logit_scale, prob_thd, bg_idx, want_conf=False, form="auto"):
        log.append(f"label_head_resized_multi(from={_hws(image_hw)},to={_hws(out_hw)},prob_thd={float(prob_thd)},want_conf={bool(want_conf)},"
                   f"form={form})")
        n = sum(h * w for h, w in out_hw)
        labels, conf = z(n, dtype=i64), z(n)
        lab = views(labels, 1, out_hw)
        return (lab, labels, [v[0] for v in views(conf, 1, out_hw)]) if want_conf else (lab, labels)

    def topk_head_resized(tile_logits, windows, up_hw, pad_tl, canvas_hw, out_hw, query_idx, num_classes, logit_scale, k, form="auto"):
        log.append(f"topk_head_resized(from={_hw(canvas_hw)},to={_hw(out_hw)},k={int(k)},form={form})")
        return z(k, *out_hw, dtype=i32), z(k, *out_hw)

    def topk_head_resized_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, out_hw, query_idx, num_classes,
                                logit_scale, k, form="auto"):
        log.append(f"topk_head_resized_multi(from={_hws(image_hw)},to={_hws(out_hw)},k={int(k)},form={form})")
        n = sum(h * w for h, w in out_hw)
        return views(z(k * n, dtype=i32), k, out_hw), views(z(k * n), k, out_hw)

    def topk_from_probs(probs, query_idx, k):
        log.append(f"topk_from_probs(hw={_hw(probs.shape[1:])},k={int(k)})")
        return z(k, *probs.shape[1:], dtype=i32), z(k, *probs.shape[1:])

    def scene_planes(scene):
        hw = scene.shape[:2] if scene.dtype == torch.uint8 else scene.shape[-2:]
        return z(3, *hw)

    def pamr(logits, guide, steps, dilations=(8, 16), inplace=False):
        log.append(f"pamr(hw={_hw(logits.shape[1:])},guide={_hw(guide.shape[1:])},steps={int(steps)},inplace={bool(inplace)})")
        return logits

    def class_area(labels, K, counts=None):
        log.append(f"class_area(n={labels.numel()})")
        return z(K, dtype=i64)

    def class_area_multi(labels, image_pixels, K):
        log.append(f"class_area_multi(pixels={[int(p) for p in image_pixels]})")
        return z(len(image_pixels), K, dtype=i64)

    def area_keep(counts, bg_idx, area_thd):
        log.append(f"area_keep(shape={_hw(counts.shape)},area_thd={float(area_thd)})")
        return torch.ones(counts.shape, dtype=i32)

    def area_filter_probs(probs, labels, keep, prob_thd, bg_idx):
        log.append(f"area_filter_probs(hw={_hw(probs.shape[1:])},prob_thd={float(prob_thd)})")
        return labels

    def area_filter_probs_multi(probs, labels, keep, out_hw, prob_thd, bg_idx):
        log.append(f"area_filter_probs_multi(hw={_hws(out_hw)},prob_thd={float(prob_thd)})")
        return labels

    def area_relabel(tile_logits, windows, up_hw, pad_tl, canvas_hw, query_idx, num_classes, logit_scale, prob_thd, bg_idx, keep, conf, labels):
        log.append(f"area_relabel(hw={_hw(canvas_hw)},prob_thd={float(prob_thd)})")
        return labels

    def area_relabel_multi(tile_logits, windows, tile_image, up_hw, pad_tl, image_hw, image_tiles, query_idx, num_classes, logit_scale,
                           prob_thd, bg_idx, keep, conf, labels):
        log.append(f"area_relabel_multi(hw={_hws(image_hw)},prob_thd={float(prob_thd)})")
        return labels

    scope = locals()
    return {k: scope[k] for k in sorted(scope) if callable(scope[k]) and k not in ("z", "prefix", "views")}


def record():
    """The route of every case of AXES on the ``clip_decontamination_amd`` that is importable."""
    import torch
    from clip_decontamination_amd import ops, pipeline

    log = []
    stand_ins = _recorders(torch, log)
    saved = {name: getattr(ops, name) for name in stand_ins}
    real_plan = pipeline.plan_images

    def plan_images(shapes, stride, crop, patch, tiles_per_launch, tile_bytes=0, pixel_bytes=0, flush_bytes=None):
        per_image = [int(pixel_bytes(i)) if callable(pixel_bytes) else int(pixel_bytes) * h * w for i, (h, w) in enumerate(shapes)]
        log.append(f"plan_images(pixel_bytes={per_image})")
        return real_plan(shapes, stride, crop, patch, tiles_per_launch, tile_bytes, pixel_bytes, flush_bytes)

    cpu = torch.device("cpu")
    net = types.SimpleNamespace(visual=types.SimpleNamespace(device=cpu, cfg=types.SimpleNamespace(patch=16, embed_dim=8)))
    scenes = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in IMAGES]
    calls, sequences, cases = {}, {}, []
    try:
        for name, fn in stand_ins.items():
            setattr(ops, name, fn)
        pipeline.plan_images = plan_images
        for c in case_keys():
            del log[:]
            Q = c["Q"]
            try:
                pipe = pipeline.SegPipeline(net, torch.zeros(Q, 8), torch.arange(Q) % K, prob_thd=PROB_THD, label_head=c["label_head"],
                                            prob_head=c["prob_head"], resize_head=c["resize_head"], pamr_steps=c["pamr"],
                                            area_thd=c["area_thd"])
                if c["flush_bytes"] != "default":
                    pipe.flush_bytes = c["flush_bytes"]
                pipe._packed_tile_logits = lambda buf, g, f, Q=Q: (log.append(f"_packed_tile_logits(T={f.tile_hi - f.tile_lo})"),
                                                                   torch.zeros(f.tile_hi - f.tile_lo, Q, 2, 2))[1]
                pipe.tile_logits = lambda scene, windows, tile_hw, scene_index=None, grid_of_tiles=None, Q=Q: (
                    log.append(f"tile_logits(T={len(windows)})"), torch.zeros(len(windows), Q, 2, 2))[1]
                kw = {"want_probs": c["wanted"] == "probs", "topk": 3 if c["wanted"] == "topk3" else 0}
                ori = ORI[c["ori_shapes"]]
                if c["entry"] == "segment_scenes":
                    out = pipe.segment_scenes(scenes, STRIDE, CROP, ori_shapes=ori, **kw)
                    log.append("-> " + _shape(out))
                else:
                    for i, s in enumerate(scenes):
                        out = pipe.segment_scene(s, STRIDE, CROP, ori_shape=None if ori is None else ori[i], **kw)
                        log.append("-> " + _shape(out))
            except Exception as e:                                       # the refusals are part of the table
                log.append(f"{type(e).__name__}: {' '.join(str(e).split()[:8])}")
            seq = tuple(calls.setdefault(s, len(calls)) for s in log)
            cases.append(sequences.setdefault(seq, len(sequences)))
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
        pipeline.plan_images = real_plan
    return {"axes": [[n, list(v)] for n, v in AXES], "calls": list(calls), "sequences": [list(s) for s in sequences], "cases": cases}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo))
    table = record()
    with open(a.out, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(table['cases'])} cases, {len(table['sequences'])} distinct sequences, {len(table['calls'])} distinct calls -> {a.out}")


if __name__ == "__main__":
    main()
