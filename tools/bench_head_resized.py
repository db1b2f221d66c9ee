"""Labels and the k best classes at another ori_shape, measured from resident tile logits.  One JSON line per case.

    python tools/bench_head_resized.py --shape dataset --queries 16,64 [--out profiles/head_resized.jsonl]

Shapes
  dataset    64 images of 448 x 448, 9 tiles of 224 at stride 112 each (grids 14 x 14), every image to 1024 x 1024: the configs that resize
             to fit 448 and are scored at the original size.  Multi-image entries, one launch for the 64 images.
  identity   8 images of 448 x 448 at their own size: what "auto" should do where nothing is resized but the resized entry is called.
  downscale  8 images of 1024 x 1024 (64 tiles each) to 448 x 448.  The staged form does not fit; it is not timed.
  scene      119 tiles of 512 at stride 256 on 2048 x 4608 (grids 37 x 37, tiles padded to 518) to 3072 x 6912.  Single-image entries.
Routes, Q = K, labels (k = None) and k in --ks
  direct  ops.label_head_resized[_multi] / ops.topk_head_resized[_multi] with form="direct"
  staged  the same with form="staged"
  canvas  what SegPipeline does with resize_head="canvas": ops.stitch[_multi], then up to 64 queries ops.postprocess_multi with the resize
          fused (labels) or with probabilities + ops.topk_from_probs per image (top-k); beyond 64 queries ops.resize_bilinear +
          ops.postprocess per image.  This route is not touched by the resized heads, so it stands for the tree before them.
All routes of one (shape, Q, k) are timed in the same process in alternating rounds: `repeats` windows of `steps` calls each, device events
around a window; median and (min, max) over the windows.  `peak_extra_mb`: the peak of device memory allocated during one call beyond what
was resident before it.  `agree`: the share of pixels (labels) or (pixel, slot) pairs (top-k) on which the route names the class the
direct route names.  Tile logits are i.i.d. N(0, 0.3^2)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from clip_decontamination_amd import ops  # noqa: E402
from clip_decontamination_amd.pipeline import tile_windows  # noqa: E402

SCALE, THD, BG = 50.0, 0.0, 0
# name -> (images, (h, w), crop, stride, grid, up, pad, (H, W))
SHAPES = {"dataset": (64, (448, 448), 224, 112, 14, 224, 0, (1024, 1024)),
          "identity": (8, (448, 448), 224, 112, 14, 224, 0, (448, 448)),
          "downscale": (8, (1024, 1024), 224, 112, 14, 224, 0, (448, 448)),
          "scene": (1, (2048, 4608), 512, 256, 37, 518, 3, (3072, 6912))}


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def window_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def peak_extra_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return round((peak - base) / 1e6, 1)


def flat(x):
    """The classes a route returned (one tensor or one per image), as one vector for `agree`."""
    return torch.cat([t.reshape(-1) for t in x]) if isinstance(x, (list, tuple)) else x.reshape(-1)


def alternate(routes, steps, warmup, repeats):
    times = {name: [] for name in routes}
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    for _ in range(repeats):
        for name, fn in routes.items():                                    # alternating within a round
            times[name].append(window_ms(fn, steps))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="dataset", choices=sorted(SHAPES))
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--queries", default="16,64,130,256")
    ap.add_argument("--ks", default="0,1,5,8", help="0 = labels")
    ap.add_argument("--out", default=None, help="appended to, one line per case")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_resized needs a GPU: nothing is measured without one")
    N, (h, w), crop, stride, grid, up, pad, out = SHAPES[a.shape]
    one = tile_windows(h, w, (stride, stride), (crop, crop))
    T = N * len(one)
    win = torch.tensor(one * N, dtype=torch.int32, device="cuda")
    tile_image = [n for n in range(N) for _ in one]
    image_hw, image_tiles, out_hw = [(h, w)] * N, [(n * len(one), len(one)) for n in range(N)], [out] * N
    fits = ops.resized_footprint((h, w), out)
    fits = fits[0] * fits[1] <= ops.RESIZED_STAGE_PIX
    geometry = f"{N} x {len(one)} tiles of {crop} at stride {stride} on {h}x{w}, grids {grid}x{grid}, to {out[0]}x{out[1]}"

    def emit(**kw):
        kw.update(shape=a.shape, geometry=geometry, steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(kw)
        print(line, flush=True)
        if a.out:                                                          # appended line by line: a cut-off run keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for Q in [int(q) for q in a.queries.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(Q)
        tl = 0.3 * torch.randn(T, Q, grid, grid, device="cuda", generator=gen)
        qi = torch.arange(Q, dtype=torch.int32, device="cuda")
        geo = ((up, up), (pad, pad))

        def fused(k, form):
            if N == 1:
                if k:
                    return ops.topk_head_resized(tl, win, *geo, (h, w), out, qi, Q, SCALE, k, form=form)[0]
                return ops.label_head_resized(tl, win, *geo, (h, w), out, qi, Q, SCALE, THD, BG, form=form)
            if k:
                return ops.topk_head_resized_multi(tl, win, tile_image, *geo, image_hw, image_tiles, out_hw, qi, Q, SCALE, k, form=form)[0]
            return ops.label_head_resized_multi(tl, win, tile_image, *geo, image_hw, image_tiles, out_hw, qi, Q, SCALE, THD, BG, form=form)[1]

        def canvas(k):
            if N == 1:
                canvases, views = None, [ops.stitch(tl, win, *geo, (h, w))]
            else:
                canvases, views = ops.stitch_multi(tl, win, tile_image, *geo, image_hw, image_tiles)
            if Q <= ops.POSTPROCESS_MAX_Q and N > 1:
                prb, _, labels = ops.postprocess_multi(canvases, image_hw, qi, Q, SCALE, THD, BG, out_hw, bool(k), flat_labels=True)
                return [ops.topk_from_probs(p, qi, k)[0] for p in prb] if k else labels
            res = []
            for c in views:
                p, l_ = ops.postprocess(ops.resize_bilinear(c, out), qi, Q, SCALE, THD, BG, want_probs=bool(k))
                res.append(ops.topk_from_probs(p, qi, k)[0] if k else l_.reshape(-1))
            return res

        for k in [int(x) for x in a.ks.split(",") if int(x) <= Q]:
            routes = {"direct": lambda: fused(k, "direct"), "canvas": lambda: canvas(k)}
            if fits:
                routes["staged"] = lambda: fused(k, "staged")
            times = alternate(routes, a.steps, a.warmup, a.repeats)
            ref = flat(routes["direct"]())
            pix = N * out[0] * out[1]
            for name, fn in routes.items():
                got = flat(fn())
                emit(case=name, Q=Q, K=Q, k=k or None, ms=spread(times[name]), mpix_per_s=round(pix / 1e3 / statistics.median(times[name]), 1),
                     peak_extra_mb=peak_extra_mb(fn), tile_logits_mb=round(tl.numel() * 4 / 1e6, 1), agree=round(float((got == ref).float().mean()), 6))
                del got
            del ref
        del tl


if __name__ == "__main__":
    main()
